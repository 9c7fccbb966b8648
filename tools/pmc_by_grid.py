#!/usr/bin/env python3
"""Mean per-launch counter values per (kernel, grid size) from a directory of rocprofv3 --pmc CSV passes with kernel
traces -- pmc_summary.py for runs that launch one kernel at several shapes.  `us_under_counters_median` is the kernel's
duration in those passes (slower than a plain run)."""
import collections
import csv
import glob
import json
import os
import re
import sys


def name_of(r):
    return re.sub(r"\(anonymous namespace\)::", "", r["Kernel_Name"]).split("(")[0].replace("void ", "")


d = sys.argv[1]
keep = lambda n: "project" in n or "attn" in n or "reduce_slabs" in n
vals = collections.defaultdict(lambda: collections.defaultdict(list))
for f in glob.glob(os.path.join(d, "**", "*counter_collection.csv"), recursive=True):
    for r in csv.DictReader(open(f)):
        if keep(name_of(r)):
            vals[(name_of(r), int(r["Grid_Size"]))][r["Counter_Name"]].append(float(r["Counter_Value"]))
dur = collections.defaultdict(list)
for f in glob.glob(os.path.join(d, "**", "*kernel_trace.csv"), recursive=True):
    for r in csv.DictReader(open(f)):
        if keep(name_of(r)):
            grid = int(r["Grid_Size_X"]) * int(r["Grid_Size_Y"]) * int(r["Grid_Size_Z"])
            dur[(name_of(r), grid)].append((int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3)
out = {}
for k in sorted(vals):
    v = sorted(dur.get(k, [0.0]))
    out[f"{k[0]} grid={k[1]}"] = dict({c: round(sum(x) / len(x)) for c, x in sorted(vals[k].items())},
                                      launches=len(v), us_under_counters_median=round(v[len(v) // 2], 1))
print(json.dumps(out, indent=1))
