#!/usr/bin/env python3
"""Side measurement (not the headline bench): one gp_registration step (gpc_registration_step) on a model that is resident on the
device, against the composition available without it -- host NumPy assignment (tests/registration_ref.py), two host-pointer
gpc_sparse_likelihood calls and a host reduction -- on the same inputs.  Capacity 100, the reference's default hyper-parameters,
res 0.15, sz 20; the scan is the model cloud under a small rigid motion.  Prints one JSON line (and writes it to --out).

    python tools/bench_registration.py --case c1            # BASELINE config 1: plane_cloud(10000)
    python tools/bench_registration.py --case big           # 2.1 M points, ~8100 leaves
    rocprofv3 --kernel-trace --stats -d DIR -o reg -- python tools/bench_registration.py --case big --steps 3 --no-host
    python tools/bench_registration.py --case big --stats-csv DIR/.../reg_kernel_stats.csv   # adds the per-kernel split
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
import registration_ref as ref  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--case", choices=["c1", "big"], default="c1")
ap.add_argument("--steps", type=int, default=20)
ap.add_argument("--warmup", type=int, default=3)
ap.add_argument("--no-host", action="store_true", help="skip the host composition (profiling runs)")
ap.add_argument("--stats-csv", help="kernel_stats.csv of a rocprofv3 --kernel-trace --stats run of this tool")
ap.add_argument("--out")
a = ap.parse_args()

res, sz, cap = 0.15, 20, 100
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
ang = 0.002
Rz = np.array([[np.cos(ang), -np.sin(ang), 0], [np.sin(ang), np.cos(ang), 0], [0, 0, 1]])
c0 = xyz.astype(np.float64).mean(axis=0)
scan_xyz = ((xyz.astype(np.float64) - c0) @ Rz.T + c0 + np.array([0.003, -0.002, 0.001])).astype(np.float32)
scan = ctx.make_cloud(scan_xyz, rgb)
n = len(scan)
prm = capi.default_params_registration(step=0.0)      # the pose stays put: every timed step does the same work

# ---- the step on the device
reg = capi.Registration(ctx, pt, gd, gc)
d_scan = torch.from_numpy(scan.view(np.uint8).reshape(-1, 32)).cuda()
torch.cuda.synchronize()
times = []
for k in range(a.warmup + a.steps):
    # every timed step starts from the same scan: at these hyper-parameters single points can give a non-finite gradient (sigma <= 0
    # after cancellation, as in the reference), and a cloud moved by it would leave the following steps nothing to do
    reg.set_cloud(d_scan, n=n)
    ctx.synchronize()
    t0 = time.perf_counter()
    out = reg.step(prm)                                # (synchronous: it ends in the 72-byte read-back)
    times.append(time.perf_counter() - t0)
t_gpu = float(np.median(times[a.warmup:]))
rec = {"workload": f"{name}, res {res}, capacity {cap}, default hyper-parameters", "n": n, "P": int(v.P),
       "bv_mean": float(sizes.mean()), "n_used": int(out[8]), "finite": bool(np.all(np.isfinite(out))),
       "gpu_step_ms": 1e3 * t_gpu, "gpu_step_ms_min_max": [1e3 * min(times[a.warmup:]), 1e3 * max(times[a.warmup:])],
       "gpu_points_per_s": n / t_gpu, "steps_timed": a.steps}

# ---- the composition available without it
if not a.no_host:
    b = pt.fetch()
    grid = ref.grid_of(xyz, res)
    trained = sizes > 0
    t0 = time.perf_counter()
    owner, local = ref.assign(scan_xyz, b, grid, trained)
    order, off = ref.bucket(owner, v.P)
    used = order[:off[-1]]
    q = local[used]
    col = np.ascontiguousarray((rgb[used].astype(np.float64) - b["rgb_mean"][owner[used]]).T)
    t1 = time.perf_counter()
    dX, l = gd.likelihood(off, q[:, 1], q[:, 2], q[:, 0][None, :])
    dC, cl = gc.likelihood(off, q[:, 1], q[:, 2], col)
    t2 = time.perf_counter()
    R = b["R"][owner[used]]
    d = l[:, None] * dC + cl[:, None] * dX
    dg = np.einsum("nij,nj->ni", R, d)
    x = np.einsum("nij,nj->ni", R, q) + b["mean"][owner[used]]
    g = np.concatenate([dg, np.cross(x, dg)], axis=1)
    delta = g.sum(axis=0) / max(len(used), 1)
    t3 = time.perf_counter()
    scale = np.abs(g).sum(axis=0) / max(len(used), 1)
    bad = ~(np.isfinite(g).all(axis=1))
    rec.update({"host_nonfinite_points": int(bad.sum()), "host_step_ms": 1e3 * (t3 - t0), "host_assign_ms": 1e3 * (t1 - t0), "host_likelihood_calls_ms": 1e3 * (t2 - t1),
                "host_reduce_ms": 1e3 * (t3 - t2), "host_points_per_s": n / (t3 - t0),
                "same_n_used": bool(len(used) == int(out[8])),
                "ls_rel_diff": float(abs(l.sum() / max(len(used), 1) - out[6]) / max(abs(out[6]), 1e-300)),
                "delta_diff_over_mean_abs_g": float(np.max(np.abs(delta - out[:6]) / np.maximum(scale, 1e-300)))})

# ---- the per-kernel split of a profiled run
if a.stats_csv:
    rows = list(csv.DictReader(open(a.stats_csv)))
    keep = [r for r in rows if any(k in r["Name"] for k in ("rg_", "sparse_likelihood", "rocprim", "radix", "onesweep"))]
    rec["kernel_split"] = [{"kernel": r["Name"][:160], "calls": int(r["Calls"]), "avg_us": float(r["AverageNs"]) / 1e3,
                            "percent": float(r["Percentage"])} for r in keep]
line = json.dumps(rec)
print(line)
if a.out:
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(line + "\n")
for o in (reg, gd, gc, pt):
    o.close()
ctx.close()
