"""The tuning knobs (spmv_hip_set_tuning / spmv_hip_get_tuning / spmv_hip_tuning_key, sp.tuning): no device needed.

KNOBS below is the specification, and the one place in the tests where a default or a refusal text is written down: the
keys in the library's order, each with its default, values it takes (given -> stored: the edges of its range, and what
a normalising knob makes of a value), values just outside that it refuses, and the whole refusal message.  The table
in csrc/hip/spmv_device.hip, the declarations in csrc/hip/tuning.hpp and the comment in include/spmv_hip.h are held to
it; every other test sets knobs with sp.tuning, which puts back what was there."""
import ctypes as C
import json
import os
import re
import subprocess
import sys

import pytest

import sparsematrixvectormultiplication_amd as sp
from conftest import ROOT

INT_MAX, INT_MIN = 2**31 - 1, -2**31
TILE_ROWS_MAX = 32768   # kTileRowsMax of csrc/hip/tile_kernels.hpp (the %d of the tile_rows refusal)


def same(*values):
    return [(v, v) for v in values]


BOOL = [(0, 0), (1, 1), (7, 1), (-1, 1), (INT_MIN, 1)]
TRI = [(-1, -1), (-5, -1), (INT_MIN, -1), (0, 0), (1, 1), (3, 1), (INT_MAX, 1)]
# (key, default, [(given, stored)], [refused], the message of a refusal)
KNOBS = [
    ("stream_cap", 0, same(0, 1024, 2048, 3072, 4096, 8192), [-1, 1, 1023, 1025, 3071, 3073, 8191, 8193, 16384],
     "set_tuning: stream_cap must be 0 (auto), 1024, 2048, 3072, 4096 or 8192"),
    ("stream_block", 256, same(256, 512, 1024), [0, 255, 257, 511, 513, 1023, 1025, 2048],
     "set_tuning: stream_block must be 256, 512 or 1024"),
    ("stream_nt", 1, BOOL, [], None),
    ("stream_xcd", 0, same(-1, 0, 1, 16, INT_MAX), [-2, INT_MIN], "set_tuning: stream_xcd must be -1, 0 or a positive run length"),
    ("stream_kind", -1, same(-1, 0, 5, 6), [-2, 1, 4, 7],
     "set_tuning: stream_kind must be -1 (auto), 0 (csr_stream), 5 (x-window) or 6 (tiles)"),
    ("stream_tile", -1, same(-1, 0, 1), [-2, 2], "set_tuning: stream_tile must be -1 (auto), 0 or 1"),
    ("tile_lmax", 1536, same(1, 1536, 65536), [0, 65537], "set_tuning: tile_lmax must be 1..65536"),
    ("tile_rows", 0, same(0, 256, 512, 768, TILE_ROWS_MAX - 256, TILE_ROWS_MAX), [257, 128, 255, 1, -256, TILE_ROWS_MAX + 1, TILE_ROWS_MAX + 256],
     f"set_tuning: tile_rows must be 0 (auto) or a multiple of 256 in 256..{TILE_ROWS_MAX}"),
    ("halo_split", 1, BOOL, [], None),
    ("halo_overlap", 1, BOOL, [], None),
    ("tile_pack", 1, BOOL, [], None),
    ("tile_long", 1, same(0, 1, 2), [-1, 3], "set_tuning: tile_long must be 0, 1 (rows with >= 2^20 entries together) or 2 (always)"),
    ("tile_balance", 1, BOOL, [], None),
    ("tile_min_pass", 256, same(0, 256, 2048), [-1, 2049], "set_tuning: tile_min_pass must be 0 (no remainder) .. 2048"),
    ("tile_places", 0, same(0, 8, 16, 4096), [4, 4104, 7, 9, -8, 4097],
     "set_tuning: tile_places must be 0 (the chip's) or a multiple of 8 up to 4096"),
    ("tile_items", 1008, same(8, 1008, 65536), [7, 65537], "set_tuning: tile_items must be 8..65536"),
    ("local_patterns", -1, TRI, [], None),
    ("local_share", -1, same(-1, 0, 1, 2), [-2, 3], "set_tuning: local_share must be -1 (auto: on), 0, 1 or 2 (on, hashing the length only)"),
    ("local_segment_cap", 0, same(0, 1, 16, INT_MAX), [-1, INT_MIN], "set_tuning: local_segment_cap must be 0 (the LDS budget's) or a number of bytes"),
    ("tile_mid_items", 0, same(0, 1, 65536), [-1, 65537], "set_tuning: tile_mid_items must be 0 (auto: three rounds of the CUs) .. 65536"),
    ("tile_streams", 1, BOOL, [], None),
    ("tile_fit", 1, BOOL, [], None),
    ("skew_rows", 1, BOOL, [], None),
    ("tile_probe", 0, [(0, 0), (1, 1), (15, 15), (16, 0), (31, 15), (-1, 15), (2001, 1)], [], None),
    ("probe_depth", 4, same(4, 16), [3, 5, 15, 17, 0, 8], "set_tuning: probe_depth must be 4 or 16"),
    ("tile_gather_ahead", 0, BOOL, [], None),
    ("tile_expand", -1, TRI, [], None),
    ("tile_mid_lo", 0, same(0, 8, 1024), [7, 1025, 1, -1], "set_tuning: tile_mid_lo must be 0 (auto) or 8..1024"),
    ("tile_mid", 1, BOOL, [], None),
    ("place_tries", 12, same(0, 12, 16), [-1, 17], "set_tuning: place_tries must be 0..16"),
    ("tile_plan_on_device", 1, BOOL, [], None),
    ("tile_density", 4, same(0, 4, 4096), [-1, 4097], "set_tuning: tile_density must be 0 (never stage) .. 4096"),
    ("gather_mode", 0, same(0, 1), [-1, 2], "set_tuning: gather_mode must be 0 (broadcasts) or 1 (padded all-gather)"),
    ("local_nt", -1, same(-1, 0, 1), [-2, 2], "set_tuning: local_nt must be -1 (auto), 0 or 1"),
    ("local_cap", 0, same(0, 1024, 2048, 3072), [-1, 1, 1023, 1025, 3071, 3073, 4096], "set_tuning: local_cap must be 0, 1024, 2048 or 3072"),
    ("plan_on_device", 1, BOOL, [], None),
    ("stream_local", 1, BOOL, [], None),
]
KEYS = [k[0] for k in KNOBS]
DEFAULTS = {k[0]: k[1] for k in KNOBS}


@pytest.fixture(autouse=True)
def knobs_put_back():
    before = sp.tuning_values()
    yield
    for key, value in before.items():
        sp.set_tuning(key, value)


def last_error():
    return sp.lib().spmv_hip_last_error().decode()


def test_the_keys_and_their_defaults_in_a_fresh_process():
    assert len(KEYS) == len(set(KEYS)) == 37
    env = {k: v for k, v in os.environ.items() if k != "SPMV_TUNING"}
    code = (f"import sys, json; sys.path.insert(0, {ROOT!r}); import sparsematrixvectormultiplication_amd as sp; "
            "print(json.dumps(list(sp.tuning_values().items())))")
    out = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr[-2000:]
    got = [tuple(item) for item in json.loads(out.stdout.strip().splitlines()[-1])]
    assert got == [(k[0], k[1]) for k in KNOBS]


@pytest.mark.parametrize("key,default,taken,refused,message", KNOBS, ids=KEYS)
def test_values_taken_and_refused(key, default, taken, refused, message):
    assert (message is None) == (not refused)
    for given, stored in taken:
        sp.set_tuning(key, given)
        assert sp.get_tuning(key) == stored, (key, given)
        assert sp.tuning_values()[key] == stored
    for held in {taken[0][1], taken[-1][1]}:        # a refusal leaves the knob as it was, whatever it holds
        sp.set_tuning(key, held)
        for value in refused:
            with pytest.raises(sp.SpmvHipError) as err:
                sp.set_tuning(key, value)
            assert str(err.value) == "spmv_hip_set_tuning: " + message, (key, value)
            assert last_error() == message
            assert sp.get_tuning(key) == held, (key, value)


def test_unknown_and_null_keys():
    L = sp.lib()
    before = sp.tuning_values()
    for key in ("pipe_wgs_per_cu", "", "stream_cap ", "STREAM_CAP", "g_stream_cap"):
        with pytest.raises(sp.SpmvHipError) as err:
            sp.set_tuning(key, 1)
        assert str(err.value) == f"spmv_hip_set_tuning: set_tuning: unknown key '{key}'"
        with pytest.raises(sp.SpmvHipError) as err:
            sp.get_tuning(key)
        assert str(err.value) == f"spmv_hip_get_tuning: get_tuning: unknown key '{key}'"
    value = C.c_int(-77)
    assert L.spmv_hip_set_tuning(None, 1) == -1 and last_error() == "set_tuning: NULL key"
    assert L.spmv_hip_get_tuning(None, C.byref(value)) == -1 and last_error() == "get_tuning: NULL argument"
    assert L.spmv_hip_get_tuning(b"stream_cap", None) == -1 and last_error() == "get_tuning: NULL argument"
    assert L.spmv_hip_get_tuning(b"no_such_knob", C.byref(value)) == -1 and value.value == -77
    assert sp.tuning_values() == before
    # the enumeration: every key once, NULL on both sides of it
    assert [L.spmv_hip_tuning_key(i).decode() for i in range(len(KEYS))] == KEYS
    for index in (-1, len(KEYS), len(KEYS) + 1, INT_MAX, INT_MIN):
        assert L.spmv_hip_tuning_key(index) is None


def test_tuning_restores_what_was_there_not_the_default():
    sp.set_tuning("tile_lmax", 777)
    sp.set_tuning("stream_kind", 6)
    with sp.tuning(tile_lmax=2048, stream_kind=0):
        assert (sp.get_tuning("tile_lmax"), sp.get_tuning("stream_kind")) == (2048, 0)
    assert (sp.get_tuning("tile_lmax"), sp.get_tuning("stream_kind")) == (777, 6)
    with sp.tuning():
        pass
    assert sp.get_tuning("tile_lmax") == 777
    # a normalising knob goes back to what it held, whatever was given
    sp.set_tuning("tile_probe", 5)
    with sp.tuning(tile_probe=31, local_patterns=-9):
        assert (sp.get_tuning("tile_probe"), sp.get_tuning("local_patterns")) == (15, -1)
    assert sp.get_tuning("tile_probe") == 5


def test_tuning_nests():
    sp.set_tuning("local_patterns", 1)
    with sp.tuning(local_patterns=0, tile_rows=256):
        with sp.tuning(local_patterns=1, stream_xcd=3):
            assert sp.get_tuning("local_patterns") == 1 and sp.get_tuning("stream_xcd") == 3
            with sp.tuning(tile_rows=512):
                assert sp.get_tuning("tile_rows") == 512
            assert sp.get_tuning("tile_rows") == 256
        assert sp.get_tuning("local_patterns") == 0 and sp.get_tuning("stream_xcd") == DEFAULTS["stream_xcd"]
    assert sp.get_tuning("local_patterns") == 1 and sp.get_tuning("tile_rows") == DEFAULTS["tile_rows"]


def test_tuning_restores_when_the_body_raises():
    sp.set_tuning("place_tries", 3)
    with pytest.raises(ZeroDivisionError):
        with sp.tuning(place_tries=0, tile_items=64):
            assert sp.get_tuning("place_tries") == 0
            1 / 0
    assert sp.get_tuning("place_tries") == 3 and sp.get_tuning("tile_items") == DEFAULTS["tile_items"]


def test_a_refused_knob_restores_those_already_set_and_raises():
    sp.set_tuning("local_cap", 1024)
    before = sp.tuning_values()
    entered = False
    with pytest.raises(sp.SpmvHipError, match="tile_rows must be 0"):
        with sp.tuning(local_cap=3072, tile_rows=257, stream_kind=6):
            entered = True
    assert not entered and sp.tuning_values() == before and before["local_cap"] == 1024
    with pytest.raises(sp.SpmvHipError, match="get_tuning: unknown key 'no_such_knob'"):
        with sp.tuning(local_cap=2048, no_such_knob=1):
            entered = True
    assert not entered and sp.tuning_values() == before


def test_the_header_documents_every_key_with_its_default():
    text = open(os.path.join(ROOT, "include", "spmv_hip.h")).read()
    block = text[text.index("/* Kernel tuning knobs"):text.index("int spmv_hip_set_tuning(")]
    assert sorted(set(re.findall(r'"([a-z_]+)" \(-?\d+\)', block))) == sorted(KEYS)
    for key, default in DEFAULTS.items():
        assert f'"{key}" ({default})' in block, key
    for name in ("spmv_hip_get_tuning", "spmv_hip_tuning_key"):
        assert re.search(rf"\b{name}\(", text), name
