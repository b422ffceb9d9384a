#!/usr/bin/env python3
"""Mean per-dispatch value of every counter for kernels whose name contains a substring, from the
counter_collection.csv files under $PROFILE_OUT/pmc_<tag>_*: python tools/pmc_summary.py <tag> [substring]"""
import csv, glob, os, sys
OUT = os.environ.get("PROFILE_OUT") or os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profile_out")
tag = sys.argv[1]
pat = sys.argv[2] if len(sys.argv) > 2 else "fused"
acc = {}
for f in sorted(glob.glob(os.path.join(OUT, f"pmc_{tag}_*/**/*counter_collection.csv"), recursive=True)):
    per = {}
    for r in csv.DictReader(open(f)):
        if pat not in r["Kernel_Name"]:
            continue
        per.setdefault((r["Counter_Name"], r["Dispatch_Id"]), 0.0)
        per[(r["Counter_Name"], r["Dispatch_Id"])] += float(r["Counter_Value"])
    for (name, _), v in per.items():
        acc.setdefault(name, []).append(v)
for name in sorted(acc):
    v = acc[name]
    print(f"{name:32s} n={len(v):4d} mean={sum(v)/len(v):16.1f}")
