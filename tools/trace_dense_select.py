#!/usr/bin/env python3
"""Per-kernel split of bench_dense_select.py's 1024 x 1024 calls from a kernel trace taken in a run of its own:
    rocprofv3 --kernel-trace --output-format csv -d DIR -- python tools/bench_dense_select.py --only-c3 --no-record
    python tools/trace_dense_select.py DIR
Every dispatch is keyed by its kernel and by the kernels enqueued before and after it, which tells the calls apart (the fit of the
variance call stands between a fit and a variance kernel, the fit of the _ev call with v_star between two variance kernels, ...).
Writes the median, minimum and maximum duration of every key seen at least five times to profiles/dense_select_trace.json."""
import collections
import csv
import glob
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KERNELS = ("dense_gauss_evidence", "dense_gauss_keep", "dense_variance_big", "dense_big_kernel", "dense_grid_points")


def short(name):
    for k in KERNELS:
        if k in name:
            return k
    return name[:40]


rows = []
for path in glob.glob(os.path.join(sys.argv[1], "**", "*kernel_trace.csv"), recursive=True):
    with open(path) as fh:
        for r in csv.DictReader(fh):
            rows.append((int(r["Start_Timestamp"]), int(r["End_Timestamp"]), short(r["Kernel_Name"])))
rows.sort()
ms = collections.defaultdict(list)
for i, (s, e, n) in enumerate(rows):
    before = rows[i - 1][2] if i else "-"
    after = rows[i + 1][2] if i + 1 < len(rows) else "-"
    ms["%s | after %s | before %s" % (n, before, after)].append((e - s) / 1e6)
out = {"what": "kernel durations in ms from rocprofv3 --kernel-trace of tools/bench_dense_select.py --only-c3 --no-record "
               "(1024 patches x 1024 pts, m = 400), keyed by kernel and by the kernels enqueued before and after it",
       "kernels": {k: {"count": len(v), "ms_median": float(np.median(v)), "ms_min": float(min(v)), "ms_max": float(max(v))}
                   for k, v in sorted(ms.items()) if len(v) >= 5}}
with open(os.path.join(ROOT, "profiles", "dense_select_trace.json"), "w") as fh:
    json.dump(out, fh, indent=1)
    fh.write("\n")
print(json.dumps(out, indent=1))
