#!/usr/bin/env python3
"""Side measurement (not the headline bench): one map insertion -- gpc_patches_insert_cloud_dev plus gpc_sparse_remap of the depth and
the colour GP -- on a model that is resident on the device, against the composition available without it: gpc_patches_fetch and
gpc_sparse_get_state, the NumPy restatement of the insertion (tests/mapping_ref.py, frames from the oracle's compute_rotation), and
gpc_sparse_set_state into new objects.  The model is the cloud; the scan is the same surface moved by half a patch along x, so kept
leaves (most), fresh leaves (the column of voxels the scan opens, and untrained old leaves it covers) and idle leaves (untrained old
leaves it does not cover) occur where the cloud has them: the record counts each kind.  Sizes as tools/bench_registration.py;
capacity 100, default hyper-parameters, res 0.15, sz 20, min_nbr 100.  Median of --reps timed calls, profiler off; the host
composition is timed once (it takes seconds to minutes).  Prints one JSON line (and writes it to --out).

    python tools/bench_mapping.py --case c1 --out profiles/mapping_bench_c1.json
    python tools/bench_mapping.py --case big --no-host
    rocprofv3 --kernel-trace --stats -d DIR -o map -- python tools/bench_mapping.py --case big --reps 3 --no-host
    python tools/bench_mapping.py --case big --no-host --stats-csv DIR/.../map_kernel_stats.csv   # adds the per-kernel split
"""
import argparse
import csv
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import torch  # noqa: E402
from gp_compressor_amd import capi, synth  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--case", choices=["c1", "big"], default="c1")
ap.add_argument("--reps", type=int, default=20)
ap.add_argument("--warmup", type=int, default=3)
ap.add_argument("--no-host", action="store_true", help="skip the host composition (profiling runs; the big case takes minutes)")
ap.add_argument("--stats-csv", help="kernel_stats.csv of a rocprofv3 --kernel-trace --stats run of this tool")
ap.add_argument("--out")
a = ap.parse_args()

res, sz, cap, min_nbr = 0.15, 20, 100, 100
if a.case == "c1":
    xyz, rgb = synth.plane_cloud(10000, seed=1)
    name = "C1: plane_cloud(10000)"
else:
    xyz, rgb = synth.plane_cloud(2_100_000, seed=11, extent=0.15 * 90)
    name = "plane_cloud(2.1 M), extent 13.5"
assert torch.cuda.is_available(), "needs the GPU: there is no CPU path to time"
ctx = capi.Context(0)
pt = ctx.project_cloud(ctx.make_cloud(xyz, rgb), res, sz)
v = pt.view
gd = capi.Sparse(ctx, capi.default_params_sparse(1, capacity=cap), v.P, 1)
gc = capi.Sparse(ctx, capi.default_params_sparse(3, capacity=cap), v.P, 3)
gd.add_dev(v.off, v.n_max, v.n_total, v.x0, v.x1, v.y)
gc.add_dev(v.off, v.n_max, v.n_total, v.x0, v.x1, v.rgb)
ctx.synchronize()
sizes = gd.sizes()
scan_xyz = (xyz.astype(np.float64) + np.array([res / 2, 0.0, 0.0])).astype(np.float32)
scan = ctx.make_cloud(scan_xyz, rgb)
n = len(scan)
d_scan = torch.from_numpy(scan.view(np.uint8).reshape(-1, 32)).cuda()
torch.cuda.synchronize()

# ---- the insertion and the two remaps on the device
t_ins, t_map = [], []
for k in range(a.warmup + a.reps):
    ctx.synchronize()
    t0 = time.perf_counter()
    new, o2n = pt.insert_cloud(d_scan, min_nbr=min_nbr, depth=gd, n=n)      # (synchronous: sizes depend on the data)
    t1 = time.perf_counter()
    gd2, gc2 = gd.remap(new.view.P, o2n), gc.remap(new.view.P, o2n)         # (synchronous: the table is the caller's again)
    t2 = time.perf_counter()
    t_ins.append(t1 - t0)
    t_map.append(t2 - t1)
    if k < a.warmup + a.reps - 1:
        for o in (gd2, gc2, new):
            o.close()
tot = np.array(t_ins[a.warmup:]) + np.array(t_map[a.warmup:])
P2 = int(new.view.P)
cnt = np.diff(new.fetch()["off"])
old = np.zeros(P2, bool)
old[o2n] = True
kept = old.copy()
kept[o2n] = sizes > 0
rec = {"workload": f"{name}, res {res}, capacity {cap}, min_nbr {min_nbr}, scan = cloud moved by res/2 along x", "n": n, "P": int(v.P),
       "P_new": P2, "points_inserted": int(new.view.n_total), "leaves_kept": int(kept.sum()), "leaves_new": int((~old).sum()),
       "old_untrained_recut": int((old & ~kept & (cnt > 0)).sum()), "old_untrained_without_points": int((old & ~kept & (cnt == 0)).sum()),
       "gpu_insert_ms": 1e3 * float(np.median(t_ins[a.warmup:])), "gpu_remap_both_ms": 1e3 * float(np.median(t_map[a.warmup:])),
       "gpu_total_ms": 1e3 * float(np.median(tot)), "gpu_total_ms_min_max": [1e3 * float(tot.min()), 1e3 * float(tot.max())],
       "gpu_points_per_s": n / float(np.median(tot)), "reps_timed": a.reps}

# ---- the composition available without it
if not a.no_host:
    import mapping_ref as mr
    import oracle_lib as O
    grid = mr.model_grid(xyz, res, sz)
    t0 = time.perf_counter()
    b = pt.fetch()
    st_d, st_c = gd.state(), gc.state()
    t1 = time.perf_counter()
    want = mr.insert(b, grid, sizes > 0, scan_xyz, rgb, min_nbr, compute_rotation=O.compute_rotation)
    t2 = time.perf_counter()
    Pn = len(want["cls"])
    host_objs = []
    for g_old, st, ny in ((gd, st_d, 1), (gc, st_c, 3)):
        g_new = capi.Sparse(ctx, capi.default_params_sparse(ny, capacity=cap), Pn, ny)
        bv = np.zeros(Pn, np.int32)
        bv[want["old_to_new"]] = g_old.sizes()
        full = []
        for arr in st:
            z = np.zeros((Pn,) + arr.shape[1:])
            z[want["old_to_new"]] = arr
            full.append(z)
        g_new.set_state(bv, full[0], full[3], full[1], full[2])
        host_objs.append(g_new)
    t3 = time.perf_counter()
    rec.update({"host_total_ms": 1e3 * (t3 - t0), "host_fetch_ms": 1e3 * (t1 - t0), "host_insert_numpy_ms": 1e3 * (t2 - t1),
                "host_set_state_ms": 1e3 * (t3 - t2), "host_points_per_s": n / (t3 - t0),
                "same_leaf_table": bool(Pn == P2 and np.array_equal(want["old_to_new"], o2n)),
                "same_offsets": bool(Pn == P2 and np.array_equal(want["off"], new.fetch()["off"]))})
    for o in host_objs:
        o.close()

# ---- the per-kernel split of a profiled run
if a.stats_csv:
    rows = list(csv.DictReader(open(a.stats_csv)))
    keep = [r for r in rows if any(k in r["Name"] for k in ("mp_", "pc_", "sp_remap", "rocprim", "radix", "onesweep", "scan"))]
    rec["kernel_split"] = [{"kernel": r["Name"][:160], "calls": int(r["Calls"]), "avg_us": float(r["AverageNs"]) / 1e3,
                            "percent": float(r["Percentage"])} for r in keep]
line = json.dumps(rec)
print(line)
if a.out:
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(line + "\n")
for o in (gd2, gc2, new, gd, gc, pt):
    o.close()
ctx.close()
