#!/usr/bin/env python3
"""Median per dispatch of every counter of rocprofv3 --pmc / --kernel-trace output, by kernel instantiation.

usage: pmc_by_kernel.py <dir> [<dir> ...] [--match csr_stream_local]
Each <dir> is searched for *_counter_collection.csv (one line per dispatch and counter) and *_kernel_trace.csv (one
line per dispatch: its duration).  Kernel names are cut to their template arguments."""
import csv
import glob
import os
import re
import sys
from collections import defaultdict
from statistics import median

args = sys.argv[1:]
match = "csr_stream_local"
if "--match" in args:
    i = args.index("--match")
    match = args[i + 1]
    del args[i:i + 2]


def short(name):
    m = re.match(r"(?:void )?(?:spmv::)?([\w:]+<[^()]*>)", name)
    return m.group(1) if m else name[:60]


rows = defaultdict(lambda: defaultdict(list))
meta = {}
for d in args:
    for f in glob.glob(os.path.join(d, "**", "*_counter_collection.csv"), recursive=True):
        for r in csv.DictReader(open(f)):
            if match not in r["Kernel_Name"]:
                continue
            k = short(r["Kernel_Name"])
            rows[k][r["Counter_Name"]].append(float(r["Counter_Value"]))
            meta[k] = (r["VGPR_Count"], r["LDS_Block_Size"], r["Scratch_Size"])
    for f in glob.glob(os.path.join(d, "**", "*_kernel_trace.csv"), recursive=True):
        for r in csv.DictReader(open(f)):
            if match not in r["Kernel_Name"]:
                continue
            k = short(r["Kernel_Name"])
            rows[k]["duration_us"].append((int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) * 1e-3)
            meta.setdefault(k, (r.get("VGPR_Count", "?"), r.get("LDS_Block_Size", "?"), r.get("Scratch_Size", "?")))
for k in sorted(rows):
    v, lds, scr = meta[k]
    print(f"{k}  (VGPRs {v}, LDS {lds} B, scratch {scr})")
    for c in sorted(rows[k]):
        vals = rows[k][c]
        print(f"    {c:24s} median {median(vals):16.6g}   dispatches {len(vals)}")
