#!/usr/bin/env python3
"""Side measurement: what pruning a trained sparse model costs (gpc_sparse_prune_dev) against the only route to a smaller model that
existed before it -- training new objects at the lower capacity from the points (gpc_sparse_add_dev).  8192 patches x 256 points,
capacity 100, the basis-filling kernel (every patch ends with 100 vectors); prune to 50 and to 25.  Every timed prune works on a fresh
identity-remap copy made outside the events; median of 20 HIP-event times each.  Algorithmic bytes: sum over the removals of 32 b^2
per patch (one read and one write of C and Q at the size before the removal), against the HBM peak bench.py uses.
Writes profiles/prune_bench.json and prints it."""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402
from gp_compressor_amd import capi, synth  # noqa: E402

P, n, res, CAP, REPS = 8192, 256, 0.15, 100, 20
KEEPS = (50, 25)
HBM_PEAK_GBPS = 8000.0     # as bench.py
dev = torch.device("cuda:0")
ctx = capi.Context(0)
ctx.set_stream(torch.cuda.current_stream().cuda_stream)
t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
off, x0, x1, y = synth.make_patches(P, n, res=res, seed=5)
perm = synth.sattolo_perms(off, seed=7)
kw = dict(sigmaf_sq=1.0, l_sq=(res / 8) ** 2, noise=1e-4)
d_off, d_x0, d_x1, d_y, d_perm = t(off), t(x0), t(x1), t(y), t(perm)
ident = np.arange(P, dtype=np.int32)
torch.cuda.synchronize()


def timed(call):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    call()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1)


def train(g):
    g.add_dev(d_off, n, P * n, d_x0, d_x1, d_y, d_perm)


full = capi.Sparse(ctx, capi.default_params_sparse(1, capacity=CAP, **kw), P, 1)
train(full)
ctx.synchronize()
b0 = full.sizes().astype(np.int64)
stat = lambda a: {"ms_median": float(np.median(a)), "ms_min": float(np.min(a)), "ms_max": float(np.max(a))}
rec = {"workload": f"{P} patches x {n} pts, capacity {CAP}, basis-filling kernel (l_sq = (res/8)^2, noise 1e-4), ny = 1",
       "reps": REPS, "basis_before": {"min": int(b0.min()), "mean": float(b0.mean()), "max": int(b0.max())}, "hbm_peak_GBps": HBM_PEAK_GBPS,
       "prune": {}}
for keep in KEEPS:
    small = capi.Sparse(ctx, capi.default_params_sparse(1, capacity=keep, **kw), P, 1)
    ms_p, ms_a = [], []
    for rep in range(REPS + 1):                      # the first round warms up
        copy = full.remap(P, ident)                  # synchronous, outside the events
        tp = timed(lambda: copy.prune_dev(keep=keep))
        if rep == REPS:
            assert np.array_equal(copy.sizes(), np.minimum(b0, keep))
        copy.close()
        small.reset()
        ctx.synchronize()
        ta = timed(lambda: train(small))
        if rep:
            ms_p.append(tp)
            ms_a.append(ta)
    small.close()
    nbytes = float(sum(32.0 * b * b for b0_ in b0 for b in range(keep + 1, int(b0_) + 1)))
    sp, sa = stat(ms_p), stat(ms_a)
    gbps = nbytes / (sp["ms_median"] * 1e-3) / 1e9
    rec["prune"][str(keep)] = {"prune": sp, "patches_per_s": P / (sp["ms_median"] * 1e-3), "removed_per_patch": float(np.mean(b0 - np.minimum(b0, keep))),
                               "algorithmic_bytes": nbytes, "algorithmic_GBps": gbps, "hbm_frac": gbps / HBM_PEAK_GBPS,
                               "retrain_at_lower_capacity": sa, "retrain_over_prune": sa["ms_median"] / sp["ms_median"]}
full.close()
os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
with open(os.path.join(ROOT, "profiles", "prune_bench.json"), "w") as fh:
    json.dump(rec, fh, indent=1)
    fh.write("\n")
print(json.dumps(rec))
ctx.close()
