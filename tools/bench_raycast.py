#!/usr/bin/env python3
"""Side measurement (not the headline bench): one ray cast (gpc_patches_raycast_dev, gp_mapping::train_classification) of a cloud
against its own map, resident on the device -- rays per second -- and the occupancy batch (gpc_occupancy_batch_dev) on the cells it
labels.  res 0.15, sz 20 as in tools/bench_registration.py; the sensor stands above the cloud's centre.  Every leaf counts as trained
(depth = NULL), so every owned ray walks.  The timed call includes its 32-byte read-back of the counts.  Prints one JSON line (and
writes it to --out).

    python tools/bench_raycast.py --case c1            # BASELINE config 1: plane_cloud(10000)
    python tools/bench_raycast.py --case big           # 2.1 M points, ~8100 leaves
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402
from gp_compressor_amd import capi, synth  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--case", choices=["c1", "big"], default="c1")
ap.add_argument("--steps", type=int, default=20)
ap.add_argument("--warmup", type=int, default=3)
ap.add_argument("--height", type=float, default=2.0, help="the sensor's height above the cloud's centre")
ap.add_argument("--out")
a = ap.parse_args()

res, sz = 0.15, 20
if a.case == "c1":
    xyz, rgb = synth.plane_cloud(10000, seed=1)
    name = "C1: plane_cloud(10000)"
else:
    xyz, rgb = synth.plane_cloud(2_100_000, seed=11, extent=0.15 * 90)
    name = "plane_cloud(2.1 M), extent 13.5"
assert torch.cuda.is_available(), "needs the GPU: there is no CPU path to time"
ctx = capi.Context(0)
cloud = ctx.make_cloud(xyz, rgb)
n = len(cloud)
pt = ctx.project_cloud(cloud, res, sz)
v = pt.view
origin = xyz.astype(np.float64).mean(axis=0) + np.array([0.0, 0.0, a.height])
d_cloud = torch.from_numpy(cloud.view(np.uint8).reshape(-1, 32)).cuda()
d_cells = torch.zeros((v.P, v.m), dtype=torch.uint8, device="cuda")
torch.cuda.synchronize()

times, counts = [], None
for k in range(a.warmup + a.steps):
    d_cells.zero_()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    counts = pt.raycast(d_cloud, origin, d_cells, n=n)          # (synchronous: it ends in the read-back of the counts)
    times.append(time.perf_counter() - t0)
t_cast = float(np.median(times[a.warmup:]))

times_b, sizes = [], None
for k in range(a.warmup + a.steps):
    t0 = time.perf_counter()
    off, x0, x1, y, n_total, n_max = pt.occupancy_batch(d_cells)    # (includes the allocation of its outputs)
    times_b.append(time.perf_counter() - t0)
    sizes = (n_total, n_max)
t_batch = float(np.median(times_b[a.warmup:]))
cells = d_cells.cpu().numpy()

rec = {"workload": f"{name}, res {res}, sz {sz}, sensor {a.height} above the centre, every leaf trained", "n": n, "P": int(v.P),
       "rays": int(counts[0]), "noop_rays": int(counts[1]), "occupied_writes": int(counts[2]), "free_writes": int(counts[3]),
       "cells_occupied": int(np.sum(cells == capi.CELL_OCCUPIED)), "cells_free": int(np.sum(cells == capi.CELL_FREE)),
       "raycast_ms": 1e3 * t_cast, "raycast_ms_min_max": [1e3 * min(times[a.warmup:]), 1e3 * max(times[a.warmup:])],
       "rays_per_s": n / t_cast, "occupancy_batch_ms": 1e3 * t_batch, "batch_points": int(sizes[0]), "batch_n_max": int(sizes[1]),
       "steps_timed": a.steps}
line = json.dumps(rec)
print(line)
if a.out:
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(line + "\n")
pt.close()
ctx.close()
