#!/usr/bin/env python3
"""Side measurement: rate control to a byte budget (gpc_rate_allocate_dev) on the workload of tools/bench_prune_rd.py: 8192 patches x 256
points, capacity 100, the basis-filling kernel (every patch ends with 100 vectors), ny = 1.  The budget is the byte count of a uniform
keep = 50.  Median of 20 HIP-event times each, all in this process:
  (a) the curve pass: prune_rd_dev(keep=1, max_mse=inf) with removed, mse0 and mse, on a fresh identity-remap copy per run;
  (b) the allocation call: rate_allocate_dev over the 8192 rows (its fixed sequence of launches, no read-back);
  (c) the applying prune: prune_dev(target = b - k) on a fresh copy per run.
Quality: sum_p n_p mse_p of the allocation against the uniform prune's own sum at the same byte count (both read by prune_rd_dev with a
target that removes nothing).  Writes profiles/allocate_bench.json and prints it."""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402
from gp_compressor_amd import capi, synth  # noqa: E402

P, n, res, CAP, REPS, KEEP, UNIT = 8192, 256, 0.15, 100, 20, 50, 24
dev = torch.device("cuda:0")
ctx = capi.Context(0)
ctx.set_stream(torch.cuda.current_stream().cuda_stream)
t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
off, x0, x1, y = synth.make_patches(P, n, res=res, seed=5)
perm = synth.sattolo_perms(off, seed=7)
kw = dict(sigmaf_sq=1.0, l_sq=(res / 8) ** 2, noise=1e-4)
d_off, d_x0, d_x1, d_y, d_perm = t(off), t(x0), t(x1), t(y), t(perm)
ident = np.arange(P, dtype=np.int32)
N = P * n
torch.cuda.synchronize()


def timed(call):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    call()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1)


def stats(ms):
    return {"ms_median": float(np.median(ms)), "ms_min": float(np.min(ms)), "ms_max": float(np.max(ms))}


def series(call, fresh=True, keep_last=False):
    """REPS timed calls after one warm-up round, each on a fresh copy made outside the events (fresh) or on nothing; keep_last: the last copy"""
    ms, copy = [], None
    for rep in range(REPS + 1):
        copy = full.remap(P, ident) if fresh else None
        tm = timed(lambda: call(copy))
        if copy is not None and not (keep_last and rep == REPS):
            copy.close()
        if rep:
            ms.append(tm)
    return stats(ms), copy


def errors(g):
    """every patch's error as it stands (a prune_rd call whose target removes nothing)"""
    e = torch.zeros(P, dtype=torch.float64, device=dev)
    tg = t(g.sizes())
    torch.cuda.synchronize()
    g.prune_rd_dev(d_off, N, d_x0, d_x1, d_y, target=tg, mse0=e)
    ctx.synchronize()
    return e.cpu().numpy()


full = capi.Sparse(ctx, capi.default_params_sparse(1, capacity=CAP, **kw), P, 1)
full.add_dev(d_off, n, N, d_x0, d_x1, d_y, d_perm)
ctx.synchronize()
b0 = full.sizes().astype(np.int64)
ld = full.ld()
need = UNIT * int(np.sum(b0 - np.minimum(b0, KEEP)))
n_p = np.diff(off).astype(np.float64)
d_removed = torch.zeros(P, dtype=torch.int32, device=dev)
d_mse0 = torch.zeros(P, dtype=torch.float64, device=dev)
d_mse = torch.full((P, ld), float("nan"), dtype=torch.float64, device=dev)
d_w, d_count = t(n_p), t(b0.astype(np.int32))
d_k = torch.zeros(P, dtype=torch.int32, device=dev)
d_target = torch.zeros(P, dtype=torch.int32, device=dev)
d_res = torch.zeros(32, dtype=torch.uint8, device=dev)
torch.cuda.synchronize()

rec = {"workload": f"{P} patches x {n} pts, capacity {CAP}, basis-filling kernel (l_sq = (res/8)^2, noise 1e-4), ny = 1", "reps": REPS,
       "basis_before": {"min": int(b0.min()), "mean": float(b0.mean()), "max": int(b0.max())}, "need_bytes": need,
       "rows": P, "ld": ld, "sweep_bytes": P * ld * 8, "launches_per_call": 137}
rec["a_curve_pass"], _ = series(lambda g: g.prune_rd_dev(d_off, N, d_x0, d_x1, d_y, keep=1, removed=d_removed, mse=d_mse, mse0=d_mse0))


def allocate(_):
    ctx.rate_allocate_dev(P, ld, d_removed, d_mse0, d_mse, need, w=d_w, unit_all=UNIT, refine=True, count=d_count, k=d_k, target=d_target,
                          result=d_res)


rec["b_allocate"], _ = series(allocate, fresh=False)
result = capi.rate_result(d_res)
k = d_k.cpu().numpy().astype(np.int64)
rec["b_over_a"] = rec["b_allocate"]["ms_median"] / rec["a_curve_pass"]["ms_median"]
rec["result"] = result
rec["k"] = {"min": int(k.min()), "mean": float(k.mean()), "max": int(k.max())}
rec["c_apply_prune"], pruned = series(lambda g: g.prune_dev(target=d_target), keep_last=True)
assert np.array_equal(pruned.sizes(), np.maximum(1, b0 - k)) and result["saved"] >= need and result["feasible"] == 1
e_alloc = errors(pruned)
pruned.close()
uniform = full.remap(P, ident)
uniform.prune_dev(keep=KEEP)
ctx.synchronize()
e_unif = errors(uniform)
uniform.close()
e_full = errors(full)
fin = np.isfinite(e_full) & np.isfinite(e_unif) & np.isfinite(e_alloc)        # (the sums run over the patches finite in all three)
tot = lambda e: float(np.sum((n_p * e)[fin]))
rec["quality"] = {"patches_summed": int(fin.sum()), "sum_n_mse_before": tot(e_full), "sum_n_mse_uniform_keep50": tot(e_unif), "sum_n_mse_allocated": tot(e_alloc),
                  "allocated_over_uniform": tot(e_alloc) / tot(e_unif), "bytes_saved_uniform": need, "bytes_saved_allocated": result["saved"]}
full.close()
os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
with open(os.path.join(ROOT, "profiles", "allocate_bench.json"), "w") as fh:
    json.dump(rec, fh, indent=1)
    fh.write("\n")
print(json.dumps(rec))
ctx.close()
