#!/usr/bin/env python3
"""Side measurement: what the width search of gpc_sparse_quantize_rd_dev costs.  The workload of tools/bench_prune_rd.py: 8192 patches x
256 points, capacity 100, the basis-filling kernel (every patch ends with 100 vectors), ny = 1.  The call only reads the object, so every
run works on the same trained object; median of 20 HIP-event times each, all in this process:
  (a) prune_rd_dev(target >= b): removes nothing, ONE error evaluation per patch (mse0) -- the yardstick for an evaluation;
  (b) quantize_rd_dev(max_mse = 0): mse0 plus all 16 widths, 17 evaluations per patch;
  (c) quantize_rd_dev(max_mse_p = 1.1 mse0): mse0 plus the widths up to the accepted one; the width histogram, and the coefficient
      payload of a version-2 model file against version 1 (24 bytes per depth vector).
By count an evaluation is n b kernel values per patch; (b) is 16 of them beyond mse0.  Reported: the time per evaluated width,
((b) - (a)) / 16 and ((c) - (a)) / mean widths evaluated, against (a).  No expectation is stated beyond that count.
Writes profiles/quantize_bench.json and prints it."""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402
from gp_compressor_amd import capi, synth  # noqa: E402

P, n, res, CAP, REPS = 8192, 256, 0.15, 100, 20
dev = torch.device("cuda:0")
ctx = capi.Context(0)
ctx.set_stream(torch.cuda.current_stream().cuda_stream)
t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
off, x0, x1, y = synth.make_patches(P, n, res=res, seed=5)
perm = synth.sattolo_perms(off, seed=7)
kw = dict(sigmaf_sq=1.0, l_sq=(res / 8) ** 2, noise=1e-4)
d_off, d_x0, d_x1, d_y, d_perm = t(off), t(x0), t(x1), t(y), t(perm)
N = P * n
torch.cuda.synchronize()


def timed(call):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    call()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1)


def series(call):
    """median / min / max of REPS timed calls (one warm-up round first)"""
    ms = [timed(call) for _ in range(REPS + 1)][1:]
    return {"ms_median": float(np.median(ms)), "ms_min": float(np.min(ms)), "ms_max": float(np.max(ms))}


g = capi.Sparse(ctx, capi.default_params_sparse(1, capacity=CAP, **kw), P, 1)
g.add_dev(d_off, n, N, d_x0, d_x1, d_y, d_perm)
ctx.synchronize()
b0 = g.sizes().astype(np.int64)
ld = g.ld()
d_target = t(b0.astype(np.int32))
d_mse0 = torch.zeros(P, dtype=torch.float64, device=dev)
d_mseq = torch.zeros(P, dtype=torch.float64, device=dev)
d_bits = torch.zeros(P, dtype=torch.int32, device=dev)
d_qa = torch.zeros((P, 1, ld), dtype=torch.int16, device=dev)
d_qb = torch.zeros((P, ld, 2), dtype=torch.int16, device=dev)
d_rng = torch.zeros((P, 3, 2), dtype=torch.float32, device=dev)
d_curve = torch.full((P, 16), float("nan"), dtype=torch.float64, device=dev)
torch.cuda.synchronize()

a = series(lambda: g.prune_rd_dev(d_off, N, d_x0, d_x1, d_y, target=d_target, mse0=d_mse0))
ctx.synchronize()
mse0 = d_mse0.cpu().numpy()
assert np.array_equal(g.sizes(), b0)
d_bound = (1.1 * d_mse0).contiguous()
torch.cuda.synchronize()
outs = dict(bits=d_bits, q_alpha=d_qa, q_bv=d_qb, range=d_rng, mse0=d_mse0, mse_q=d_mseq, curve=d_curve)
b = series(lambda: g.quantize_rd_dev(d_off, N, d_x0, d_x1, d_y, max_mse=0.0, **outs))
ctx.synchronize()
curve = d_curve.cpu().numpy()
assert np.all(d_bits.cpu().numpy() == 0) and not np.any(np.isnan(curve)) and np.array_equal(d_mse0.cpu().numpy(), mse0)
c = series(lambda: g.quantize_rd_dev(d_off, N, d_x0, d_x1, d_y, max_mse_p=d_bound, **outs))
ctx.synchronize()
bits = d_bits.cpu().numpy().astype(np.int64)
evaluated = np.where(bits > 0, bits, 16)
v1_bytes = float(np.sum(24 * b0))
v2_bytes = float(np.sum(np.where(bits > 0, 8 * 3 + (b0 * 3 * bits + 7) // 8, 24 * b0)))
per_width_b = (b["ms_median"] - a["ms_median"]) / 16.0
per_width_c = (c["ms_median"] - a["ms_median"]) / float(evaluated.mean())
rec = {"workload": f"{P} patches x {n} pts, capacity {CAP}, basis-filling kernel (l_sq = (res/8)^2, noise 1e-4), ny = 1",
       "reps": REPS, "basis": {"min": int(b0.min()), "mean": float(b0.mean()), "max": int(b0.max())},
       "mse0": {"min": float(mse0.min()), "median": float(np.median(mse0)), "max": float(mse0.max())},
       "kernel_values_per_evaluation": float(np.sum(n * b0)),
       "a_prune_rd_one_evaluation": a,
       "b_quantize_rd_all_16_widths": b,
       "b_ms_per_width": per_width_b, "b_width_over_a": per_width_b / a["ms_median"],
       "c_quantize_rd_1p1_mse0": c,
       "c_widths_evaluated_mean": float(evaluated.mean()),
       "c_ms_per_width": per_width_c, "c_width_over_a": per_width_c / a["ms_median"],
       "c_width_histogram": {str(w): int(np.sum(bits == w)) for w in range(0, 17) if np.any(bits == w)},
       "curve_median_over_mse0": [float(np.median(curve[:, w] / mse0)) for w in range(16)],
       "payload_bytes": {"v1": v1_bytes, "v2": v2_bytes, "v2_over_v1": v2_bytes / v1_bytes}}
g.close()
os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
with open(os.path.join(ROOT, "profiles", "quantize_bench.json"), "w") as fh:
    json.dump(rec, fh, indent=1)
    fh.write("\n")
print(json.dumps(rec))
ctx.close()
