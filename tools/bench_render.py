#!/usr/bin/env python3
"""Side measurement (not the headline bench): one rendered image (gpc_patches_render_dev) of a map resident on the device -- a
640 x 480 pinhole image, mean only and with colour, at the reference's default hyper-parameters and capacity 100 (res 0.15, sz 20 as in
tools/bench_raycast.py).  The timed call includes its 20-byte read-back of the counts; the rays are made once by gpc_camera_rays_dev.
Walk length is worked out on the host from the ranges: the voxel planes between a ray's entry into the grid box and its hit (or its
exit), plus one.  Prints one JSON line (and writes it to --out).

    python tools/bench_render.py --case c1             # BASELINE config 1: plane_cloud(10000), seen from above
    python tools/bench_render.py --case big            # 2.1 M points, ~8100 leaves, seen from above its centre
    python tools/bench_render.py --case deep           # four stacked sheets seen from the side, between the sheets: long walks
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
ap.add_argument("--case", choices=["c1", "big", "deep"], default="c1")
ap.add_argument("--steps", type=int, default=20)
ap.add_argument("--warmup", type=int, default=3)
ap.add_argument("--width", type=int, default=640)
ap.add_argument("--height", type=int, default=480)
ap.add_argument("--out")
a = ap.parse_args()

res, sz = 0.15, 20
down = np.array([[1.0, 0.0, 0.0], [0.0, -1.0, 0.0], [0.0, 0.0, -1.0]])          # columns: the camera's x, y, z in the world
if a.case == "c1":
    xyz, rgb = synth.plane_cloud(10000, seed=1)
    name, origin, Rc, focal = "C1: plane_cloud(10000) from 1.2 above its centre", np.array([0.6, 0.6, 1.2]), down, 0.55 * a.width
elif a.case == "big":
    xyz, rgb = synth.plane_cloud(2_100_000, seed=11, extent=0.15 * 90)
    name, origin, Rc, focal = "plane_cloud(2.1 M), extent 13.5, from 8 above its centre", np.array([6.75, 6.75, 8.0]), down, 0.6 * a.width
else:
    ext, gap = 0.15 * 60, 0.15 * 6
    parts = [synth.plane_cloud(400_000, seed=20 + k, extent=ext) for k in range(4)]
    xyz = np.concatenate([p[0] + np.array([0.0, 0.0, k * gap], np.float32) for k, p in enumerate(parts)])
    rgb = np.concatenate([p[1] for p in parts])
    # from beside the stack, half way up, looking along +x and a little down: most rays run between two sheets for a long way
    c, s = np.cos(0.12), np.sin(0.12)
    Rc = np.array([[0.0, -s, c], [-1.0, 0.0, 0.0], [0.0, -c, -s]])
    name, origin, focal = "deep: four sheets of plane_cloud(400 k), extent 9, 0.9 apart, seen from the side", np.array([-1.0, 4.5, 1.6]), 0.8 * a.width
assert torch.cuda.is_available(), "needs the GPU: there is no CPU path to time"
ctx = capi.Context(0)
pt = ctx.project_cloud(ctx.make_cloud(xyz, rgb), res, sz)
v = pt.view
gd = capi.Sparse(ctx, capi.default_params_sparse(1), v.P, 1)
gc = capi.Sparse(ctx, capi.default_params_sparse(3), v.P, 3)
gd.add_dev(v.off, v.n_max, v.n_total, v.x0, v.x1, v.y)
gc.add_dev(v.off, v.n_max, v.n_total, v.x0, v.x1, v.rgb)
ctx.synchronize()
dirs = ctx.camera_rays(Rc, focal, focal, (a.width - 1) / 2, (a.height - 1) / 2, a.width, a.height)
n = a.width * a.height


def timed(colour):
    times, out = [], None
    for _ in range(a.warmup + a.steps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = pt.render(origin, dirs, gd, gc if colour else None, want=("range",))   # (synchronous: it ends in the read-back of the counts;
        times.append(time.perf_counter() - t0)                                     #  includes the allocation of its outputs)
    t = times[a.warmup:]
    return float(np.median(t)), [min(t), max(t)], out


t_mean, mm_mean, out = timed(False)
t_col, mm_col, _ = timed(True)
counts = out["counts"]

# walk length from the ranges: voxel planes crossed between the entry into the grid box and the hit (or the exit), plus one
d = dirs.cpu().numpy()
rng = out["range"].cpu().numpy()
mn = xyz.min(axis=0).astype(np.float64)
kmax = np.floor((xyz.max(axis=0).astype(np.float64) - mn) / res)
with np.errstate(divide="ignore", invalid="ignore"):
    t1, t2 = (mn - origin) / d, (mn + (kmax + 1) * res - origin) / d
    tn, tf = np.nanmax(np.minimum(t1, t2), axis=1), np.nanmin(np.maximum(t1, t2), axis=1)
meets = (tn <= tf) & (tf >= 0)
t_in = np.maximum(tn, 0.0)
t_end = np.where(np.isnan(rng), tf, rng)
k_in = np.floor((origin + t_in[:, None] * d - mn) / res)
k_end = np.floor((origin + t_end[:, None] * d - mn) / res)
walk = np.where(meets, np.sum(np.abs(np.clip(k_end, 0, kmax) - np.clip(k_in, 0, kmax)), axis=1) + 1, 0)

rec = {"workload": f"{name}, res {res}, sz {sz}, {a.width} x {a.height}, default hyper-parameters, capacity 100", "n_points": len(xyz),
       "P": int(v.P), "mean_basis": float(np.mean(gd.sizes())), "rays": int(counts[0]), "hits": int(counts[1]), "outside": int(counts[2]),
       "surface_tests": int(counts[3]), "tests_per_ray": counts[3] / n, "residual_rejections": int(counts[4]),
       "walk_mean": float(walk[meets].mean()) if meets.any() else 0.0, "walk_max": int(walk.max()),
       "render_ms": 1e3 * t_mean, "render_ms_min_max": [1e3 * x for x in mm_mean], "rays_per_s": n / t_mean,
       "render_colour_ms": 1e3 * t_col, "render_colour_ms_min_max": [1e3 * x for x in mm_col], "rays_per_s_colour": n / t_col,
       "steps_timed": a.steps}
line = json.dumps(rec)
print(line)
if a.out:
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(line + "\n")
for o in (gd, gc, pt):
    o.close()
ctx.close()
