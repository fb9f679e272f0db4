#!/usr/bin/env python3
"""Median and minimum duration of the full-size launches of every kernel in a `rocprofv3 --kernel-trace --output-format csv` directory
(full-size: the largest grid that kernel was launched with in the run).   python scripts/kernel_medians.py DIR [NAME_REGEX]"""
import csv
import glob
import os
import re
import statistics
import sys
from collections import defaultdict

per = defaultdict(list)
for f in glob.glob(os.path.join(sys.argv[1], "**", "*kernel_trace.csv"), recursive=True):
    for r in csv.DictReader(open(f)):
        grid = int(r["Grid_Size_X"]) * int(r["Grid_Size_Y"]) * int(r["Grid_Size_Z"])
        name = re.sub(r"\(anonymous namespace\)::|^void |\(.*$", "", r["Kernel_Name"])
        per[name].append((grid, (int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3))
pat = re.compile(sys.argv[2] if len(sys.argv) > 2 else ".")
for name in sorted(per):
    if pat.search(name):
        full = [t for g, t in per[name] if g == max(g for g, _ in per[name])]
        print(f"{name:24s} {len(full):4d} launches  median {statistics.median(full):9.1f} us  min {min(full):9.1f} us")
