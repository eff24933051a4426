"""The probit GP's latent predictive variance and occupancy probability (gpc_dense_irls_fit_predict_var, include/gpc.h) restated in
NumPy, shared by test_irls_var_cpu.py (the restatement on its own, without a GPU) and test_irls_var_gpu.py (the kernels against it).

Batches, regime, models and tolerances are irls_cases.py's; X* is variance_cases.xstar's.  The Newton / IRLS loop is the oracle's
(oracle/gpc_oracle.c, orc_dense_irls_fit) with q and r taken from the oracle's pinned functor, but in the form the kernels factor:
B = I + diag(s) K diag(s), s = W^1/2, and it keeps the L and the s of the LAST SOLVE PERFORMED:
    f* = k*^T a,   v* = sigma_f^2 - |L^-1 (s o k*)|^2,   p* = 0.5 erfc(-z / sqrt 2),  z = f* / sqrt(s20 + max(v*, 0)).
"""
import math

import numpy as np

import irls_cases as IC
import variance_cases as VC

SF, L_SQ, S20 = IC.REGIME
C_EXP = float(np.float32(-0.5)) / L_SQ      # the constant of the exponent as the kernels and the oracle form it

# The v* gate.  The issue's rule: VTOL * sigma_f^2 with test_dense_variance_gpu.py's VTOL = 1e-11, unless the float64 restatement's own
# error against the longdouble one (E64, of sigma_f^2, worst over the w4_batch patches up to 128 points) exceeds a sixteenth of that,
# in which case 16 * E64.  Measured by test_irls_var_cpu.py::test_restatement_variance_against_longdouble: E64 = 7e-16, far below
# 1e-11 / 16 = 6.25e-13, so the gate in force is VTOL * sigma_f^2 = 1e-11; the CPU test asserts that this still holds.
VTOL = 1e-11
E64_MEASURED = 7e-16
V_GATE = VTOL * SF if E64_MEASURED <= VTOL * SF / 16 else 16 * E64_MEASURED
P_SELF_TOL = 1e-14                          # p* against the functor applied in NumPy to the GPU's own f*, v*: erfc to a few ulp on [0, 1]
V_LO, V_HI = -1e-12 * SF, SF * (1 + 1e-12)  # the range of a predictive variance, up to rounding

_erfc = np.vectorize(math.erfc, otypes=[np.float64])
try:
    from scipy.linalg import solve_triangular as _solve_tri
except ImportError:                         # any solver does: the factor is well conditioned (eigenvalues of B >= 1)
    _solve_tri = None


def _lsolve(L, X, trans=False):
    """L^-1 X (or L^-T X) for a lower-triangular L."""
    if _solve_tri is not None:
        return _solve_tri(L, X, lower=True, trans=1 if trans else 0, check_finite=False)
    return np.linalg.solve(L.T if trans else L, X)


_CACHE = {}


def phi(f, v, s20=S20):
    """The functor's ef of model 2 at sigma_x = v, y = +1: P(y = +1 | x*)."""
    z = np.asarray(f, dtype=np.float64) / np.sqrt(s20 + np.maximum(v, 0.0))
    return 0.5 * _erfc(-z * 0.70710678118654752440)


def p_gate(f_scale, f, v, model=2):
    """The derivative bound of Phi for p* against the restatement's: 0.4 (e_f / sigma + |z| e_v / (2 sigma^2)) + 1e-14, with e_f =
    FTOL[model] * f_scale (the patch's max-norm) and e_v = V_GATE."""
    sig2 = S20 + np.maximum(v, 0.0)
    sig = np.sqrt(sig2)
    return 0.4 * (IC.FTOL[model] * f_scale / sig + np.abs(f / sig) * V_GATE / (2.0 * sig2)) + 1e-14


def kernel(x0, x1, q0, q1, dtype=np.float64):
    d0, d1 = x0.astype(dtype)[:, None] - q0.astype(dtype)[None, :], x1.astype(dtype)[:, None] - q1.astype(dtype)[None, :]
    return dtype(SF) * np.exp(dtype(C_EXP) * (d0 * d0 + d1 * d1))


def _functor(oracle, model):
    L = oracle.lib()
    return (L.orc_probit_std_dx_ln, L.orc_probit_std_dx2_ln) if model == 2 else (L.orc_probit_dx_ln, L.orc_probit_dx2_ln)


def fit_patch(oracle, model, x0, x1, y, max_iter, tol, f_init):
    """One patch's Newton / IRLS loop.  Returns status, iters, a, fhat and (L, s) of the last solve (None after a failure)."""
    n = len(x0)
    dx, dx2 = _functor(oracle, model)
    K = kernel(x0, x1, x0, x1)
    f = y * f_init
    a = np.zeros(n)
    last = None
    status, iters = 0, 0
    for it in range(max_iter):
        yf = list(zip(y.tolist(), f.tolist()))
        q = np.array([dx(S20, yi, fi, 0.0) for yi, fi in yf])
        r = np.array([dx2(S20, yi, fi, 0.0) for yi, fi in yf])
        W = -r
        if not (np.all(W > 0.0) and np.all(W < np.inf)) or np.any(q != q):
            status = 2
            break
        s = np.sqrt(W)
        t = f + q / W
        B = np.eye(n) + (s[:, None] * K) * s[None, :]
        try:
            L = np.linalg.cholesky(B)
        except np.linalg.LinAlgError:
            status = 1
            break
        u = _lsolve(L, _lsolve(L, s * t), trans=True)
        a = s * u
        fn = t - u / s
        delta = float(np.max(np.abs(fn - f))) if np.all(np.isfinite(fn)) else float("nan")
        f = fn
        last = (L, s)
        iters = it + 1
        if delta != delta:
            status = 2
            break
        if delta <= tol:
            break
        if it + 1 == max_iter:
            status = 5
    if status in (1, 2):
        return status, iters, np.full(n, np.nan), np.full(n, np.nan), None
    return status, iters, a, f, last


def variance_step(L, s, Ks):
    """v* (m,) in float64 from the last solve's factor."""
    V = _lsolve(L, s[:, None] * Ks)
    return SF - np.sum(V * V, axis=0)


def variance_step_hp(x0, x1, s, xs0, xs1):
    """The variance step in np.longdouble for small patches: B = I + diag(s) K diag(s) from a longdouble K, a right-looking Cholesky that
    carries s o K* along (it leaves as L^-1 (s o K*)), v* = sigma_f^2 - the squared column norms.  s: the float64 s of the last solve."""
    LD = np.longdouble
    n = len(x0)
    sl = s.astype(LD)
    A = (sl[:, None] * kernel(x0, x1, x0, x1, LD)) * sl[None, :]
    A[np.diag_indices(n)] += LD(1)
    Bm = sl[:, None] * kernel(x0, x1, xs0, xs1, LD)
    for j in range(n):
        r = np.sqrt(A[j, j])
        col = A[j + 1:, j] / r
        Bm[j] /= r
        A[j + 1:, j + 1:] -= col[:, None] * col[None, :]
        Bm[j + 1:] -= col[:, None] * Bm[j][None, :]
    return LD(SF) - np.sum(Bm * Bm, axis=0)


def restate(oracle, batch, model, xs, max_iter=IC.MAX_ITER, idx=None, keep_last=False, **kw):
    """The definition on the patches idx (default: all) of a labelled batch: a dict of f, v, p (P, m; p only under model 2), alpha, fhat
    (N,), iters, status (P,) -- rows of patches outside idx are NaN / -1 -- and, with keep_last, last[i] = (L, s) per patch."""
    arg = dict(IC.MODELS[model])
    arg.update(kw)
    off, x0, x1, lab = batch
    P, N, m = len(off) - 1, int(off[-1]), len(xs[0])
    out = dict(f=np.full((P, m), np.nan), v=np.full((P, m), np.nan), p=np.full((P, m), np.nan), alpha=np.full(N, np.nan),
               fhat=np.full(N, np.nan), iters=np.full(P, -1, dtype=np.int32), status=np.full(P, -1, dtype=np.int32), last={})
    for i in (range(P) if idx is None else idx):
        sl = slice(off[i], off[i + 1])
        n = int(off[i + 1] - off[i])
        if n == 0:
            out["f"][i], out["v"][i], out["p"][i], out["iters"][i], out["status"][i] = 0.0, SF, 0.5, 0, 0
            continue
        st, it, a, fh, last = fit_patch(oracle, model, x0[sl], x1[sl], lab[sl], max_iter, arg["tol"], arg["f_init"])
        out["status"][i], out["iters"][i], out["alpha"][sl], out["fhat"][sl] = st, it, a, fh
        if last is None:
            continue
        Ks = kernel(x0[sl], x1[sl], xs[0], xs[1])
        out["f"][i] = Ks.T @ a
        out["v"][i] = variance_step(last[0], last[1], Ks)
        if model == 2:
            out["p"][i] = phi(out["f"][i], out["v"][i])
        if keep_last:
            out["last"][i] = last
    return out


def cached(key, make):
    """A restatement, computed once per process and never written to."""
    if key not in _CACHE:
        out = make()
        for a in out.values():
            if isinstance(a, np.ndarray):
                a.setflags(write=False)
        _CACHE[key] = out
    return _CACHE[key]


XS400 = dict(w4=("xs400", 71), tiles=("xs400", 72))


def xs400(which):
    return VC.xstar(400, seed=XS400[which][1])


def w4_ref(oracle, model=2):
    return cached(("w4", model), lambda: restate(oracle, IC.w4_batch(), model, xs400("w4"), keep_last=True))


def tile_ref(oracle, model=2):
    """The tile-count sweep: model 2 on every patch, model 1 on the patches up to MODEL1_CAP points."""
    idx = None if model == 2 else IC.cap_index(IC.MODEL1_CAP)
    return cached(("tiles", model), lambda: restate(oracle, IC.tile_batch(), model, xs400("tiles"), idx=idx))


def grid_ref(oracle, shape, m):
    return cached(("grid", shape, m), lambda: restate(oracle, IC.grid_batch(shape), 2, VC.xstar(m, seed=73)))


def pinned_batch(shape):
    """The batch of the pinned-step-count test: grid_batch(shape) without its single-point patch.  tol = 0 pins the step count only while
    no iterate repeats exactly; on one point Newton's method is a scalar iteration that reaches its fixed point to the last bit within six
    steps (on the device: in five), meets max|df| <= 0 there and rightly ends with GPC_STATUS_OK."""
    full = IC.grid_batch(shape)
    return IC.take(full, [i for i, n in enumerate(np.diff(full[0])) if n != 1])[0]


def pinned_ref(oracle, shape, max_iter):
    """tol = 0 and a step cap: the restatement run for exactly max_iter steps."""
    return cached(("pinned", shape, max_iter), lambda: restate(oracle, pinned_batch(shape), 2, VC.xstar(37, seed=74), max_iter=max_iter, tol=0.0))


def many_pick(which):
    """The patches of many_batch(which) that are compared: the edges (0, 1, the neighbours of the empty and of the NaN-label patches, those
    patches themselves) and random ones, 64 in all, fixed seed."""
    c = IC.MANY[which]
    P = c["P"]
    pick = {0, 1}
    for i in tuple(c["empty"]) + tuple(c["nan"]):
        pick.update(j for j in (i - 1, i, i + 1) if 0 <= j < P)
    rng = np.random.default_rng(c["seed"] + 7)
    for j in rng.permutation(P):
        if len(pick) >= 64:
            break
        pick.add(int(j))
    return sorted(pick)


def many_ref(oracle, which, every=False):
    """many_batch(which) restated on many_pick (every: on all patches -- the CPU test's convergence check)."""
    idx = None if every else many_pick(which)
    return cached(("many", which, every), lambda: restate(oracle, IC.many_batch(which), 2, VC.xstar(37, seed=90), idx=idx))
