#!/usr/bin/env python3
"""Side measurement: what the latent variance and the occupancy probability cost on top of the probit Newton / IRLS fit, at C5's
shape in a quarter of its batch -- 1024 patches x 1024 labelled points (one 8.8 MB factor slot per patch: 9 GB), the 20 x 20 grid.
gpc_dense_irls_fit_predict_dev against gpc_dense_irls_fit_predict_var_dev, median of 20 HIP-event times each, alternating.
Writes profiles/irls_var_bench.json and prints it."""
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
prm = capi.default_params_dense(sigmaf_sq=1.0, l_sq=(res / 3) ** 2, noise=0.25, noise_model=2)
ir = capi.default_params_irls(max_iter=20, tol=1e-9)
d_off, d_x0, d_x1, d_y = t(off), t(x0), t(x1), t(lab)
f, v, p = (torch.empty((P, m), dtype=torch.float64, device=dev) for _ in range(3))
it = torch.empty((P,), dtype=torch.int32, device=dev)
st = torch.empty((P,), dtype=torch.int32, device=dev)
torch.cuda.synchronize()
names = {}


def plain():
    ctx.dense_irls_fit_predict_dev(prm, ir, P, d_off, n, P * n, d_x0, d_x1, d_y, m, None, None, res, sz, f, None, None, it, st)


def var():
    ctx.dense_irls_fit_predict_var_dev(prm, ir, P, d_off, n, P * n, d_x0, d_x1, d_y, m, None, None, res, sz, f, v_star=v, p_star=p,
                                       iters=it, status=st)


def timed(call):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    call()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1)


for name, call in (("plain", plain), ("var", var)):      # warm-up: the workspace grows here
    call()
    torch.cuda.synchronize()
    names[name] = ctx.last_dense_kernel()
ms = {"plain": [], "var": []}
for _ in range(REPS):
    ms["plain"].append(timed(plain))
    ms["var"].append(timed(var))
steps = it.cpu().numpy()
ok = bool((st == 0).all().item()) and all(bool(torch.isfinite(a).all().item()) for a in (f, v, p)) and bool(((p >= 0) & (p <= 1)).all().item())
med = {k: float(np.median(a)) for k, a in ms.items()}
rec = {"workload": f"{P} patches x {n} labelled pts, probit IRLS (tol {ir.tol:g}, <= {ir.max_iter} steps), {sz}x{sz} grid",
       "newton_steps_mean": float(steps.mean()), "reps": REPS,
       "plain": {"kernel": names["plain"], "ms_median": med["plain"], "ms_min": float(np.min(ms["plain"])), "ms_max": float(np.max(ms["plain"]))},
       "with_variance_and_probability": {"kernel": names["var"], "ms_median": med["var"], "ms_min": float(np.min(ms["var"])),
                                         "ms_max": float(np.max(ms["var"]))},
       "extra_ms": med["var"] - med["plain"], "extra_frac": med["var"] / med["plain"] - 1.0,
       "flop_estimate_frac": float(n * n * m / (steps.mean() * n ** 3 / 3.0)), "ok": ok}
os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
with open(os.path.join(ROOT, "profiles", "irls_var_bench.json"), "w") as fh:
    json.dump(rec, fh, indent=1)
    fh.write("\n")
print(json.dumps(rec))
ctx.close()
