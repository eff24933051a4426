#!/usr/bin/env python3
"""Side measurement: what the distortion costs in a prune (gpc_sparse_prune_rd_dev against gpc_sparse_prune_dev).  The workload of
tools/bench_prune.py: 8192 patches x 256 points, capacity 100, the basis-filling kernel (every patch ends with 100 vectors).  Every timed
call works on a fresh identity-remap copy made outside the events; median of 20 HIP-event times each, all in this process:
  (a) prune_dev(keep=50): the yardstick;
  (b) prune_rd_dev(keep=50, max_mse=inf): the same removals plus the look-ahead; (b)/(a) is the price of the distortion;
  (c) prune_rd_dev(keep=1, max_mse_p = 2 mse0): the time, and the min, mean and max basis left.
By count the look-ahead adds about n b kernel values per step, the removal itself moves 32 b^2 bytes per step.  The FP64 rate of the
look-ahead is an ESTIMATE: 25 operations per kernel value (distance, exponent, the table-driven exp, sigma_f^2, one FMA) is a count of the
source, not of the ISA, and the look-ahead's time is the difference (b) - (a) of two medians.
Writes profiles/prune_rd_bench.json and prints it."""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402
from gp_compressor_amd import capi, synth  # noqa: E402

P, n, res, CAP, REPS, KEEP = 8192, 256, 0.15, 100, 20, 50
HBM_PEAK_GBPS = 8000.0     # as bench.py
FP64_PEAK_TFLOPS = 78.6    # vector FP64 of the MI355X
OPS_PER_KERNEL_VALUE = 25  # distance, exponent, table exp, sigma_f^2, one FMA into f
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


def series(call, check=None):
    """median / min / max of REPS timed calls, each on a fresh copy (one warm-up round first); check(copy) after the last one"""
    ms = []
    for rep in range(REPS + 1):
        copy = full.remap(P, ident)                  # synchronous, outside the events
        tm = timed(lambda: call(copy))
        if rep == REPS and check:
            check(copy)
        copy.close()
        if rep:
            ms.append(tm)
    return {"ms_median": float(np.median(ms)), "ms_min": float(np.min(ms)), "ms_max": float(np.max(ms))}


full = capi.Sparse(ctx, capi.default_params_sparse(1, capacity=CAP, **kw), P, 1)
full.add_dev(d_off, n, N, d_x0, d_x1, d_y, d_perm)
ctx.synchronize()
b0 = full.sizes().astype(np.int64)
d_mse0 = torch.zeros(P, dtype=torch.float64, device=dev)
d_bound = torch.zeros(P, dtype=torch.float64, device=dev)
d_target = t(b0.astype(np.int32))
torch.cuda.synchronize()
full.prune_rd_dev(d_off, N, d_x0, d_x1, d_y, target=d_target, mse0=d_mse0)      # removes nothing: the error of the trained model
ctx.synchronize()
d_bound.copy_(2.0 * d_mse0)
torch.cuda.synchronize()
mse0 = d_mse0.cpu().numpy()

left = {}


def sizes_to(name):
    def f(copy):
        left[name] = copy.sizes().astype(np.int64)
    return f


rec = {"workload": f"{P} patches x {n} pts, capacity {CAP}, basis-filling kernel (l_sq = (res/8)^2, noise 1e-4), ny = 1",
       "reps": REPS, "basis_before": {"min": int(b0.min()), "mean": float(b0.mean()), "max": int(b0.max())},
       "mse0": {"min": float(mse0.min()), "median": float(np.median(mse0)), "max": float(mse0.max())},
       "hbm_peak_GBps": HBM_PEAK_GBPS, "fp64_peak_TFLOPS": FP64_PEAK_TFLOPS}
a = series(lambda g: g.prune_dev(keep=KEEP), sizes_to("a"))
assert np.array_equal(left["a"], np.minimum(b0, KEEP))
rec["a_prune_keep50"] = a
steps = [(int(b_), KEEP) for b_ in b0]
removal_bytes = float(sum(32.0 * b * b for b_, k in steps for b in range(k + 1, b_ + 1)))
kvalues = float(sum(n * (b - 1) for b_, k in steps for b in range(k + 1, b_ + 1)))
rec["counts_keep50"] = {"removal_bytes": removal_bytes, "lookahead_kernel_values": kvalues,
                        "lookahead_flops_estimate": kvalues * OPS_PER_KERNEL_VALUE, "ops_per_kernel_value_assumed": OPS_PER_KERNEL_VALUE}
b = series(lambda g: g.prune_rd_dev(d_off, N, d_x0, d_x1, d_y, keep=KEEP), sizes_to("b"))
assert np.array_equal(left["b"], left["a"])
c = series(lambda g: g.prune_rd_dev(d_off, N, d_x0, d_x1, d_y, keep=1, max_mse_p=d_bound), sizes_to("c"))
extra_s = (b["ms_median"] - a["ms_median"]) * 1e-3
rec["prune_rd"] = {"b_prune_rd_keep50_inf": b, "b_over_a": b["ms_median"] / a["ms_median"],
             "lookahead_ms": extra_s * 1e3,
             "lookahead_rate_estimate": {"TFLOPS": kvalues * OPS_PER_KERNEL_VALUE / extra_s / 1e12,
                                         "of_fp64_peak": kvalues * OPS_PER_KERNEL_VALUE / extra_s / 1e12 / FP64_PEAK_TFLOPS},
             "c_prune_rd_keep1_2mse0": c,
             "c_basis_left": {"min": int(left["c"].min()), "mean": float(left["c"].mean()), "max": int(left["c"].max())}}
full.close()
os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
with open(os.path.join(ROOT, "profiles", "prune_rd_bench.json"), "w") as fh:
    json.dump(rec, fh, indent=1)
    fh.write("\n")
print(json.dumps(rec))
ctx.close()
