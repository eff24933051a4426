#!/usr/bin/env python3
"""Side measurement: what the Laplace evidence read-out and the selection among candidates cost on top of the probit fit with its
variance and probability, at the shape of bench_irls_var.py -- 1024 patches x 1024 labelled points (one 8.8 MB factor slot per patch:
9 GB), the 20 x 20 grid.  gpc_dense_irls_fit_predict_var_dev (the path before the evidence existed) against
gpc_dense_irls_fit_predict_ev_dev, and three _var calls with three sets of hyper-parameters against one gpc_dense_irls_select_dev over
the same three; median of 20 HIP-event times each, alternating.  Writes profiles/irls_select_bench.json and prints it."""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402
from gp_compressor_amd import capi, synth  # noqa: E402

P, n, res, sz, REPS = 1024, 1024, 0.15, 20, 20
m = sz * sz
dev = torch.device("cuda:0")
ctx = capi.Context(0)
ctx.set_stream(torch.cuda.current_stream().cuda_stream)
t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
off, x0, x1, y = synth.make_patches(P, n, res=res, seed=5)
lab = synth.occupancy_labels(off, y[0])
l_sq = (res / 3) ** 2
cands = [(1.0, l_sq / 4, 0.25), (1.0, l_sq, 0.25), (1.0, l_sq * 4, 0.25)]
prms = [capi.default_params_dense(sigmaf_sq=c[0], l_sq=c[1], noise=c[2], noise_model=2) for c in cands]
prm = prms[1]
ir = capi.default_params_irls(max_iter=20, tol=1e-9)
d_off, d_x0, d_x1, d_y = t(off), t(x0), t(x1), t(lab)
f, v, p = (torch.empty((P, m), dtype=torch.float64, device=dev) for _ in range(3))
lq = torch.empty((P,), dtype=torch.float64, device=dev)
it, st, best = (torch.empty((P,), dtype=torch.int32, device=dev) for _ in range(3))
torch.cuda.synchronize()
names = {}


def var(q=prm):
    ctx.dense_irls_fit_predict_var_dev(q, ir, P, d_off, n, P * n, d_x0, d_x1, d_y, m, None, None, res, sz, f, v_star=v, p_star=p,
                                       iters=it, status=st)


def ev():
    ctx.dense_irls_fit_predict_ev_dev(prm, ir, P, d_off, n, P * n, d_x0, d_x1, d_y, m, None, None, res, sz, f, v_star=v, p_star=p,
                                      iters=it, status=st, log_q=lq)


def var3():
    for q in prms:
        var(q)


def select():
    ctx.dense_irls_select_dev(prm, ir, cands, P, d_off, n, P * n, d_x0, d_x1, d_y, m, None, None, res, sz, f_star=f, v_star=v, p_star=p,
                              log_q=lq, best=best, iters=it, status=st)


def timed(call):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    call()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1)


calls = (("var", var), ("ev", ev), ("var3", var3), ("select", select))
for name, call in calls[::-1]:      # warm-up, the largest workspace first: it grows once
    call()
    torch.cuda.synchronize()
    names[name] = ctx.last_dense_kernel()
ms = {name: [] for name, _ in calls}
for _ in range(REPS):
    for name, call in calls:
        ms[name].append(timed(call))
won = np.bincount(best.cpu().numpy() + 1, minlength=len(cands) + 1)
ok = bool(torch.isfinite(lq[best >= 0]).all().item()) and bool((best >= -1).all().item())
med = {k: float(np.median(a)) for k, a in ms.items()}
stat = lambda k: {"ms_median": med[k], "ms_min": float(np.min(ms[k])), "ms_max": float(np.max(ms[k]))}
rec = {"workload": f"{P} patches x {n} labelled pts, probit IRLS (tol {ir.tol:g}, <= {ir.max_iter} steps), {sz}x{sz} grid",
       "reps": REPS, "kernel": names["ev"],
       "var": stat("var"), "ev": stat("ev"),
       "readout_extra_ms": med["ev"] - med["var"], "readout_extra_frac": med["ev"] / med["var"] - 1.0,
       "readout_bytes_per_patch": 8 * 4 * n,
       "candidates": [list(c) for c in cands], "three_var_calls": stat("var3"), "select_3": stat("select"),
       "select_extra_ms": med["select"] - med["var3"], "select_extra_frac": med["select"] / med["var3"] - 1.0,
       "winners_none_then_per_candidate": [int(x) for x in won], "ok": ok}
os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
with open(os.path.join(ROOT, "profiles", "irls_select_bench.json"), "w") as fh:
    json.dump(rec, fh, indent=1)
    fh.write("\n")
print(json.dumps(rec))
ctx.close()
