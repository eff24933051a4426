"""The Laplace evidence of the probit occupancy GP (gpc_dense_irls_fit_predict_ev, include/gpc.h) and the selection among candidate
hyper-parameters built on it (gpc_dense_irls_select) restated in NumPy, shared by test_irls_ev_cpu.py (the restatement on its own,
without a GPU) and test_irls_ev_gpu.py (the kernels against it).

The restatement: irls_var_cases.fit_patch gives a, fhat and (L, s) of the last solve performed; per patch of n points
    log q = -0.5 sum_j a_j fhat_j + sum_j log ef(y_j fhat_j / sqrt(s20)) - sum_{j<n} log L_jj,   ef(z) = 0.5 erfc(-z / sqrt 2)
formed with math.erfc and math.log (Rasmussen & Williams 2006, Alg. 3.1 line 10).  Batches, regime and tolerances of the fit are
irls_cases.py's; fit_patch_theta is fit_patch with the hyper-parameters as arguments, for the candidates of the selection batch."""
import math

import numpy as np

import irls_cases as IC
import irls_var_cases as IV

SF, L_SQ, S20 = IC.REGIME

# The log q gate.  The issue's rule: EV_TOL (1 + |log q|) with EV_TOL = 1e-11, the project's VTOL -- the same factor and the same export
# as v* --, unless the float64 restatement's own error against the longdouble one (E64, relative to 1 + |log q|, worst over the w4_batch
# patches up to 128 points) exceeds a sixteenth of that, in which case 16 E64.  Measured by
# test_irls_ev_cpu.py::test_restatement_against_longdouble: E64 = 1.7e-16, far below 1e-11 / 16 = 6.25e-13, so the gate in force is
# 1e-11 (1 + |log q|); the CPU test asserts that this still holds.
EV_TOL = 1e-11
E64_MEASURED = 1.7e-16
EV_RTOL = EV_TOL if E64_MEASURED <= EV_TOL / 16 else 16 * E64_MEASURED


def ev_gate(log_q):
    return EV_RTOL * (1.0 + np.abs(log_q))


def log_q_terms(a, fh, y, L, s20=S20):
    """The three sums of the definition: a^T fhat, sum log ef, sum log L_jj."""
    rs = math.sqrt(s20)
    quad = math.fsum(float(ai) * float(fi) for ai, fi in zip(a, fh))
    lik = math.fsum(_log_ef(float(yi) * float(fi) / rs) for yi, fi in zip(y, fh))
    ldet = math.fsum(math.log(float(d)) for d in np.diag(L))
    return quad, lik, ldet


def _log_ef(z):
    e = 0.5 * math.erfc(-z * 0.70710678118654752440)
    return math.log(e) if e > 0.0 else -math.inf


def log_q_of(a, fh, y, L, s20=S20):
    quad, lik, ldet = log_q_terms(a, fh, y, L, s20)
    return -0.5 * quad + lik - ldet


def log_q_hp(x0, x1, y, a, fh, s, sf=SF, l_sq=L_SQ, s20=S20):
    """The three sums in np.longdouble for small patches, from the float64 a, fhat and s of the last solve: the quadratic form as a
    longdouble dot product; log ef with erfc from mpmath at 30 digits where it is installed (else math.erfc, the logarithm and the sum in
    longdouble); sum log L_jj from a right-looking longdouble Cholesky of B = I + diag(s) K diag(s) with a longdouble K."""
    LD = np.longdouble
    n = len(x0)
    quad = np.sum(a.astype(LD) * fh.astype(LD))
    try:
        import mpmath
        mpmath.mp.dps = 30
        rs = mpmath.sqrt(mpmath.mpf(s20))
        lik = sum(mpmath.log(mpmath.erfc(-mpmath.mpf(float(yi)) * mpmath.mpf(float(fi)) / rs / mpmath.sqrt(2)) / 2) for yi, fi in zip(y, fh))
        lik = LD(str(lik))
    except ImportError:
        rs = math.sqrt(s20)
        lik = np.sum(np.log(np.array([0.5 * math.erfc(-float(yi) * float(fi) / rs * 0.70710678118654752440) for yi, fi in zip(y, fh)], dtype=LD)))
    sl = s.astype(LD)
    d0, d1 = x0.astype(LD)[:, None] - x0.astype(LD)[None, :], x1.astype(LD)[:, None] - x1.astype(LD)[None, :]
    c_exp = LD(float(np.float32(-0.5)) / l_sq)
    A = (sl[:, None] * (LD(sf) * np.exp(c_exp * (d0 * d0 + d1 * d1)))) * sl[None, :]
    A[np.diag_indices(n)] += LD(1)
    ldet = LD(0)
    for j in range(n):
        r = np.sqrt(A[j, j])
        ldet += np.log(r)
        col = A[j + 1:, j] / r
        A[j + 1:, j + 1:] -= col[:, None] * col[None, :]
    return -LD(0.5) * quad + lik - ldet


def restate(oracle, batch, max_iter=IC.MAX_ITER, idx=None, keep=False, **kw):
    """The definition on the patches idx (default: all) of a labelled batch in the regime of irls_cases.py: a dict of log_q (P,), iters,
    status (P,) -- rows of patches outside idx are NaN / -1 -- and, with keep, fit[i] = (a, fhat, L, s) per fitted patch."""
    arg = dict(IC.MODELS[2])
    arg.update(kw)
    off, x0, x1, lab = batch
    P = len(off) - 1
    out = dict(log_q=np.full(P, np.nan), iters=np.full(P, -1, dtype=np.int32), status=np.full(P, -1, dtype=np.int32), fit={})
    for i in (range(P) if idx is None else idx):
        sl = slice(off[i], off[i + 1])
        if off[i + 1] == off[i]:
            out["log_q"][i], out["iters"][i], out["status"][i] = 0.0, 0, 0
            continue
        st, it, a, fh, last = IV.fit_patch(oracle, 2, x0[sl], x1[sl], lab[sl], max_iter, arg["tol"], arg["f_init"])
        out["status"][i], out["iters"][i] = st, it
        if last is None:
            continue
        out["log_q"][i] = log_q_of(a, fh, lab[sl], last[0])
        if keep:
            out["fit"][i] = (a, fh, last[0], last[1])
    return out


def w4_ref(oracle):
    return IV.cached(("ev_w4",), lambda: restate(oracle, IC.w4_batch(), keep=True))


def tile_ref(oracle):
    return IV.cached(("ev_tiles",), lambda: restate(oracle, IC.tile_batch()))


def pinned_ref(oracle, shape, max_iter):
    return IV.cached(("ev_pinned", shape, max_iter), lambda: restate(oracle, IV.pinned_batch(shape), max_iter=max_iter, tol=0.0))


def many_ref(oracle, which):
    return IV.cached(("ev_many", which), lambda: restate(oracle, IC.many_batch(which), idx=IV.many_pick(which)))


# ------------------------------------------------------------------------------------------------------------------ the selection batch
# 16 patches x 256 points, uniform in the +- res / 2 window; labels drawn from Phi(f / sqrt(s20)) with f sampled from a GP of length scale
# l_sq = (res / 3)^2 and amplitude 9, s20 = 0.25; candidates l_sq x {1/16, 1, 16} at sigmaf_sq = 1.  With SELECT_SEED the restatement
# picks candidate 1 on every patch with a gap of at least SELECT_GAP to the runner-up (test_irls_ev_cpu.py asserts it), so the GPU test
# needs no near-tie allowance.
SELECT_P, SELECT_N, SELECT_AMP, SELECT_SEED, SELECT_GAP = 16, 256, 9.0, 23, 1.0
CANDIDATES = tuple((SF, L_SQ * k, S20) for k in (1.0 / 16, 1.0, 16.0))
_phi = np.vectorize(lambda z: 0.5 * math.erfc(-z * 0.70710678118654752440), otypes=[np.float64])


def select_batch(seed=SELECT_SEED, P=SELECT_P, n=SELECT_N):
    rng = np.random.default_rng(seed)
    off = (np.arange(P + 1) * n).astype(np.int32)
    x0, x1 = rng.uniform(-IC.RES / 2, IC.RES / 2, P * n), rng.uniform(-IC.RES / 2, IC.RES / 2, P * n)
    lab = np.zeros(P * n)
    for i in range(P):
        sl = slice(off[i], off[i + 1])
        d0, d1 = x0[sl, None] - x0[None, sl], x1[sl, None] - x1[None, sl]
        K = SELECT_AMP * np.exp(-0.5 * (d0 * d0 + d1 * d1) / L_SQ) + 1e-8 * SELECT_AMP * np.eye(n)
        f = np.linalg.cholesky(K) @ rng.standard_normal(n)
        lab[sl] = np.where(rng.uniform(size=n) < _phi(f / math.sqrt(S20)), 1.0, -1.0)
    return off, x0, x1, lab


def with_empty(batch, at):
    """The batch with an empty patch inserted in front of patch `at`."""
    off, x0, x1, lab = batch
    return np.concatenate([off[:at + 1], off[at:]]).astype(np.int32), x0, x1, lab


def fit_patch_theta(oracle, x0, x1, y, theta, max_iter=IC.MAX_ITER, tol=IC.MODELS[2]["tol"], f_init=IC.MODELS[2]["f_init"]):
    """irls_var_cases.fit_patch (model 2) with theta = (sigmaf_sq, l_sq, s20) as arguments: the same statements in the same order, so that
    at theta = REGIME it gives fit_patch's bits (asserted by test_irls_ev_cpu.py)."""
    sf, l_sq, s20 = theta
    n = len(x0)
    dx, dx2 = oracle.lib().orc_probit_std_dx_ln, oracle.lib().orc_probit_std_dx2_ln
    c_exp = float(np.float32(-0.5)) / l_sq
    d0, d1 = x0[:, None] - x0[None, :], x1[:, None] - x1[None, :]
    K = np.float64(sf) * np.exp(np.float64(c_exp) * (d0 * d0 + d1 * d1))
    f = y * f_init
    a = np.zeros(n)
    last = None
    status, iters = 0, 0
    for it in range(max_iter):
        yf = list(zip(y.tolist(), f.tolist()))
        q = np.array([dx(s20, yi, fi, 0.0) for yi, fi in yf])
        r = np.array([dx2(s20, yi, fi, 0.0) for yi, fi in yf])
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
        u = IV._lsolve(L, IV._lsolve(L, s * t), trans=True)
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


def select_ref(oracle, seed=SELECT_SEED):
    """The restatement on the selection batch: log_q_all (H, P), status (H, P), iters (H, P) and best (P,) by the rule of gpc_dense_irls_select
    (eligible: status 0 and a finite log q; the lowest index that attains the maximum)."""
    def make():
        off, x0, x1, lab = select_batch(seed)
        H, P = len(CANDIDATES), len(off) - 1
        lq, st, it = np.full((H, P), np.nan), np.full((H, P), -1, dtype=np.int32), np.full((H, P), -1, dtype=np.int32)
        for h, theta in enumerate(CANDIDATES):
            for i in range(P):
                sl = slice(off[i], off[i + 1])
                st[h, i], it[h, i], a, fh, last = fit_patch_theta(oracle, x0[sl], x1[sl], lab[sl], theta)
                if last is not None:
                    lq[h, i] = log_q_of(a, fh, lab[sl], last[0], theta[2])
        return dict(log_q_all=lq, status=st, iters=it, best=best_of(lq, st))
    return IV.cached(("ev_select", seed), make)


def best_of(lq, st):
    H, P = lq.shape
    best = np.full(P, -1, dtype=np.int32)
    for i in range(P):
        for h in range(H):
            if st[h, i] == 0 and np.isfinite(lq[h, i]) and (best[i] < 0 or lq[h, i] > lq[best[i], i]):
                best[i] = h
    return best
