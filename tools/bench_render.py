#!/usr/bin/env python3
"""Side measurement (not the headline bench): one rendered image (gpc_patches_render_dev) of a map resident on the device -- a
640 x 480 pinhole image, mean only and with colour, at the reference's default hyper-parameters and capacity 100 (res 0.15, sz 20 as in
tools/bench_raycast.py).  The timed call includes its 20-byte read-back of the counts; the rays are made once by gpc_camera_rays_dev.
Walk length is worked out on the host from the ranges: the voxel planes between a ray's entry into the grid box and its hit (or its
exit), plus one.  Prints one JSON line (and writes it to --out).

    python tools/bench_render.py --case c1             # BASELINE config 1: plane_cloud(10000), seen from above
    python tools/bench_render.py --case big            # 2.1 M points, ~8100 leaves, seen from above its centre
    python tools/bench_render.py --case deep           # four stacked sheets seen from the side, between the sheets: long walks
    python tools/bench_render.py --case big --attrs --out-attrs profiles/render_attrs_bench.json
        # ... and a second record: render alone, render + gpc_patches_render_attrs_dev (sigma and normal), and the route a caller had
        # without that entry (D2H of leaf / local, NumPy stable argsort and CSR, H2D, predict_points_dev, host scatter) for the same
        # image.  The three are timed in turn, alternating, each call ending in a synchronise; medians with min and max.
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
ap.add_argument("--attrs", action="store_true", help="also time render + attrs against render alone and the host-bucketed route")
ap.add_argument("--out-attrs")
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
if a.attrs:
    P = int(v.P)

    def render_only():
        return pt.render(origin, dirs, gd, None, want=("leaf", "local"))

    def render_attrs():
        return pt.render(origin, dirs, gd, None, want=("leaf", "local", "sigma", "normal"))

    def render_host_route():
        """what a caller did for sigma before the attrs entry: download, bucket on the host, upload, predict_points_dev, scatter back"""
        o = render_only()
        leaf, local = o["leaf"].cpu().numpy(), o["local"].cpu().numpy()
        valid = leaf >= 0
        key = np.where(valid, leaf, P)
        order = np.argsort(key, kind="stable")
        nv = int(valid.sum())
        off = np.concatenate([[0], np.cumsum(np.bincount(key[valid], minlength=P)[:P])]).astype(np.int32)
        idx = order[:nv]
        d_off = torch.from_numpy(off).cuda()
        d_x0, d_x1 = torch.from_numpy(np.ascontiguousarray(local[idx, 1])).cuda(), torch.from_numpy(np.ascontiguousarray(local[idx, 2])).cuda()
        d_f, d_s = torch.empty(max(nv, 1), dtype=torch.float64, device="cuda"), torch.empty(max(nv, 1), dtype=torch.float64, device="cuda")
        torch.cuda.synchronize()
        gd.predict_points_dev(d_off, nv, d_x0, d_x1, d_f, d_s)
        ctx.synchronize()
        sigma = np.full(n, np.nan)
        sigma[idx] = d_s.cpu().numpy()[:nv]
        return o, sigma

    # ... and the device work of the sigma alone, on one render's outputs: the scattered entry (keys, sort, offsets, gather, predict,
    # scatter) against predict_points_dev on the same entries already bucketed -- the difference is what the bucketing costs
    base = render_only()
    b_leaf, b_local = base["leaf"], base["local"]
    h_leaf, h_local = b_leaf.cpu().numpy(), b_local.cpu().numpy()
    h_key = np.where(h_leaf >= 0, h_leaf, P)
    h_idx = np.argsort(h_key, kind="stable")[:int((h_leaf >= 0).sum())]
    b_off = torch.from_numpy(np.concatenate([[0], np.cumsum(np.bincount(h_key[h_leaf >= 0], minlength=P)[:P])]).astype(np.int32)).cuda()
    b_x0, b_x1 = (torch.from_numpy(np.ascontiguousarray(h_local[h_idx, c])).cuda() for c in (1, 2))
    b_f, b_s, b_sig = (torch.empty(n, dtype=torch.float64, device="cuda") for _ in range(3))
    torch.cuda.synchronize()

    def sigma_scattered():
        gd.predict_scattered_dev(n, b_leaf, b_local.data_ptr() + 8, b_local.data_ptr() + 16, 3, None, b_sig)
        ctx.synchronize()

    def sigma_bucketed():
        gd.predict_points_dev(b_off, len(h_idx), b_x0, b_x1, b_f, b_s)
        ctx.synchronize()

    routes = {"render": render_only, "render_attrs": render_attrs, "render_host_bucketed_sigma": render_host_route,
              "sigma_scattered_dev": sigma_scattered, "sigma_prebucketed_dev": sigma_bucketed}
    times = {k: [] for k in routes}
    last = {}
    for it in range(a.warmup + a.steps):
        for k, fn in routes.items():                                             # alternating: the three see the same machine state
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            last[k] = fn()
            torch.cuda.synchronize()
            if it >= a.warmup:
                times[k].append(time.perf_counter() - t0)
    # the two routes to sigma agree bit for bit
    same = last["render_attrs"]["sigma"].cpu().numpy().tobytes() == last["render_host_bucketed_sigma"][1].tobytes()
    rec2 = {"workload": rec["workload"], "P": P, "rays": n, "hits": int(counts[1]), "steps_timed": a.steps, "warmup": a.warmup,
            "protocol": "host clock around calls that end in a device synchronise; the routes alternate inside one loop; "
                        "profiler off; one run on one MI355X; output allocation of the binding included in every route",
            "sigma_bytes_equal_host_route": bool(same)}
    for k, t in times.items():
        rec2[k + "_ms"] = 1e3 * float(np.median(t))
        rec2[k + "_ms_min_max"] = [1e3 * min(t), 1e3 * max(t)]
    rec2["attrs_over_render"] = rec2["render_attrs_ms"] / rec2["render_ms"]
    rec2["bucketing_ms"] = rec2["sigma_scattered_dev_ms"] - rec2["sigma_prebucketed_dev_ms"]
    line2 = json.dumps(rec2)
    print(line2)
    if a.out_attrs:
        os.makedirs(os.path.dirname(os.path.abspath(a.out_attrs)), exist_ok=True)
        with open(a.out_attrs, "w") as f:
            f.write(line2 + "\n")
for o in (gd, gc, pt):
    o.close()
ctx.close()
