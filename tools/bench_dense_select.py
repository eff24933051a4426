#!/usr/bin/env python3
"""Side measurement: what the log marginal likelihood and the selection among candidates cost on top of the dense fit, at the two
headline shapes -- 8192 patches x 256 points (C2, the one-wave kernel) and 1024 x 1024 (the tiled kernel) -- with m = 400 point-wise
X* (the 20 x 20 grid as points).  Each figure is set against the existing entry timed in the same process:
  ev_v against var     gpc_dense_fit_predict_ev_dev with v_star against gpc_dense_fit_predict_dev with the variance: the read-out
  ev against mean      ... without v_star against the plain mean-only call: the export plus the read-out
  select_3 against ev3 one gpc_dense_select_dev over three candidates against three such _ev calls: the keep-best steps
  ev_grid against grid_mean   the grid form as gp_compressor::set_dense_candidates calls it (evidence only, the 20 x 20 grid materialised as
                       points) against gpc_dense_fit_predict_grid_dev, whose one-wave kernel predicts the grid with its separable form
median of 20 HIP-event times each, alternating, one process.  Writes profiles/dense_select_bench.json and prints it.
--only-c3: the 1024 x 1024 shape alone; --no-record: print only; --ev-first: ev_v timed ahead of var in every round, recorded to
profiles/dense_select_bench_ev_first.json (a call that follows a variance call runs slower whichever entry it came through)."""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402
from gp_compressor_amd import capi, synth  # noqa: E402

res, sz, REPS = 0.15, 20, 20
m = sz * sz
dev = torch.device("cuda:0")
ctx = capi.Context(0)
ctx.set_stream(torch.cuda.current_stream().cuda_stream)
t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
g0 = res * ((np.arange(sz) + 0.5) / sz - 0.5)
d_xs0, d_xs1 = t(np.tile(g0, sz)), t(np.repeat(g0, sz))


def timed(call):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    call()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1)


def shape(P, n):
    off, x0, x1, y = synth.make_patches(P, n, res=res, seed=5)
    base = capi.default_params_dense()
    cands = [(base.sigmaf_sq, base.l_sq / 16, base.noise), (base.sigmaf_sq, base.l_sq, base.noise), (base.sigmaf_sq, base.l_sq * 16, base.noise)]
    prms = [capi.default_params_dense(sigmaf_sq=c[0], l_sq=c[1], noise=c[2]) for c in cands]
    pv = capi.default_params_dense(want_variance=1)
    d_off, d_x0, d_x1, d_y = t(off), t(x0), t(x1), t(y)
    f = torch.empty((P, 1, m), dtype=torch.float64, device=dev)
    v = torch.empty((P, m), dtype=torch.float64, device=dev)
    ev_ = torch.empty((P, 1), dtype=torch.float64, device=dev)
    st, best = (torch.empty((P,), dtype=torch.int32, device=dev) for _ in range(2))
    torch.cuda.synchronize()
    head = (P, d_off, n, P * n, d_x0, d_x1, d_y, 1, m, d_xs0, d_xs1)

    def mean():
        ctx.dense_fit_predict_dev(base, *head, f, status=st)

    def var():
        ctx.dense_fit_predict_dev(pv, *head, f, v_star=v, status=st)

    def ev_v():
        ctx.dense_fit_predict_ev_dev(base, *head, 0.0, 0, f, v_star=v, status=st, log_ev=ev_)

    def ev(q=base):
        ctx.dense_fit_predict_ev_dev(q, *head, 0.0, 0, f, status=st, log_ev=ev_)

    def grid_mean():
        ctx.dense_fit_predict_grid_dev(base, P, d_off, n, P * n, d_x0, d_x1, d_y, 1, res, sz, f, status=st)

    def ev_grid():
        ctx.dense_fit_predict_ev_dev(base, P, d_off, n, P * n, d_x0, d_x1, d_y, 1, 0, None, None, res, sz, f, status=st, log_ev=ev_)

    def ev3():
        for q in prms:
            ev(q)

    def select():
        ctx.dense_select_dev(base, cands, *head, 0.0, 0, f_star=f, log_ev=ev_, best=best, status=st)

    calls = (("mean", mean), ("var", var), ("ev_v", ev_v), ("ev", ev), ("grid_mean", grid_mean), ("ev_grid", ev_grid), ("ev3", ev3),
             ("select_3", select))
    if "--ev-first" in sys.argv:       # the same calls with ev_v ahead of var: does a difference between the two follow the entry or the order
        calls = (calls[0], calls[2], calls[1]) + calls[3:]
    names = {}
    for name, call in calls[::-1]:      # warm-up, the largest workspace first: it grows once
        call()
        torch.cuda.synchronize()
        names[name] = ctx.last_dense_kernel()
    ms = {name: [] for name, _ in calls}
    for _ in range(REPS):
        for name, call in calls:
            ms[name].append(timed(call))
    med = {k: float(np.median(a)) for k, a in ms.items()}
    rec = {k: {"ms_median": med[k], "ms_min": float(np.min(ms[k])), "ms_max": float(np.max(ms[k])), "kernel": names[k]} for k in ms}
    won = np.bincount(best.cpu().numpy() + 1, minlength=len(cands) + 1)
    rec.update(workload=f"{P} patches x {n} pts, m = {m} point-wise", candidates=[list(c) for c in cands],
               readout_extra_ms=med["ev_v"] - med["var"], readout_extra_frac=med["ev_v"] / med["var"] - 1.0,
               export_and_readout_extra_ms=med["ev"] - med["mean"], export_and_readout_extra_frac=med["ev"] / med["mean"] - 1.0,
               select_extra_ms=med["select_3"] - med["ev3"], select_extra_frac=med["select_3"] / med["ev3"] - 1.0,
               grid_form_extra_ms=med["ev_grid"] - med["grid_mean"], grid_form_extra_frac=med["ev_grid"] / med["grid_mean"] - 1.0,
               readout_bytes_per_patch=8 * 3 * n, winners_none_then_per_candidate=[int(x) for x in won],
               ok=bool(torch.isfinite(ev_[best >= 0]).all().item()))
    return rec


out = {"reps": REPS}
if "--ev-first" in sys.argv:
    out["order"] = "ev_v ahead of var"
if "--only-c3" not in sys.argv:
    out["c2_8192x256"] = shape(8192, 256)
out["c3_1024x1024"] = shape(1024, 1024)
if "--no-record" in sys.argv:
    print(json.dumps(out))
    ctx.close()
    sys.exit(0)
os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
with open(os.path.join(ROOT, "profiles", "dense_select_bench_ev_first.json" if "--ev-first" in sys.argv else "dense_select_bench.json"), "w") as fh:
    json.dump(out, fh, indent=1)
    fh.write("\n")
print(json.dumps(out))
ctx.close()
