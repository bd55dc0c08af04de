#!/usr/bin/env python3
"""The x-window kernel's three ways to get its slots, side by side on ONE handle (same arrays, same placement):
the slot stream (local_patterns 0), the pattern plan (local_patterns 1) and the measurement-only probe that reads no
slots at all (the STAMP instantiation, y wrong).  Events per launch for the first two; first-start-to-last-end of one
stamped launch for the slot stream and the probe; and, from a launch stamped "records are back" (mode 2000 + warm), the
share of a block's life that is its head -- start to the last of its records.  Run it under `rocprofv3 --kernel-trace --stats` or `--pmc ...` to get
the three instantiations' counters by kernel name.

usage: probe_patterns.py [rounds] [case substring ...]"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import sparsematrixvectormultiplication_amd as sp  # noqa: E402
from sparsematrixvectormultiplication_amd import synth  # noqa: E402
from sparsematrixvectormultiplication_amd.device import set_tuning  # noqa: E402

rounds = int(sys.argv[1]) if len(sys.argv) > 1 else 5
want = sys.argv[2:]
sp.hip_init(0)
set_tuning("place_tries", 0)
set_tuning("local_patterns", 1)
cases = [("nlpkkt120-like 120x120x123", lambda: synth.kkt_like()),
         ("fem-large 40x40x257x3", lambda: synth.fem_like((40, 40, 257), 1))]
if want:
    cases = [c for c in cases if any(w in c[0] for w in want)]
for name, gen in cases:
    M, rp, col, val = gen()
    with sp.CsrDevice(M, M, rp, col, val) as dev:
        dev.set_x(np.ones(M))
        info = dev.info()
        ev = {0: [], 1: []}
        span = {3: [], 1003: []}
        life, head = [], []   # per round: a block's median life, and the median time until its records were back
        for _ in range(rounds):
            for p in (0, 1):
                set_tuning("local_patterns", p)
                ev[p].append(float(dev.time(sp.CSR_STREAM, 3, 40, zero_y=False).mean()) * 1e3)
            set_tuning("local_patterns", 0)
            for mode in (3, 1003):
                start, end, _, _ = dev.stamp_blocks(mode)
                span[mode].append((end.max() - start.min()) * 0.01)
                if mode == 3:
                    life.append(float(np.median(end - start)) * 0.01)
            # the HEAD of a block (stamp word 2 = "records are back", mode 2000 + warm): kernel arguments and the
            # block's records, everything in front of its first vector load
            start, back, _, _ = dev.stamp_blocks(2003)
            head.append(float(np.median(back - start)) * 0.01)
        set_tuning("local_patterns", 1)

        def fmt(v, d=1):
            return f"{' '.join(f'{u:.{d}f}' for u in v)} (median {np.median(v):.{d}f})"
        print(f"{name}: nnz={int(rp[-1])} blocks {info['local_blocks']} pattern slots {info.get('pattern_slots', '?')} | "
              f"events: slot stream {fmt(ev[0])} | pattern plan {fmt(ev[1])} us | stamped span: slot stream "
              f"{fmt(span[3])} | no slots (probe) {fmt(span[1003])} us", flush=True)
        print(f"{name}: a block's life (slot stream, median over blocks) {fmt(life, 2)} us | its head, start to records back "
              f"{fmt(head, 2)} us | head / life {np.median(head) / np.median(life):.3f}", flush=True)
