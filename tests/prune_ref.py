"""NumPy restatement of the prune rule (include/gpc.h, gpc_sparse_prune) and the cases the prune tests share.

The rule continues the reference's capacity deletion (src/sparse_gp.hpp:206-223, delete_bv :252-295; field variant
src/sparse_gp_field.hpp:219-263):

    loop:
      if b <= 1: stop
      s_i = (sum_c alpha[c][i]^2) / (Q_ii + C_ii),  i ascending
      (minscore, loc) = arg-min as the reference scans: `if (i == 0 || s_i < minscore)`
      if b > max(1, target): remove;  else if minscore < score_tol: remove;  else stop
      order += [loc]; scores += [minscore]; delete_bv(loc); b -= 1

Everything here works in the dtype it is given: float64 to stand beside the oracle, numpy.longdouble (x87 extended, 64-bit mantissa) to
measure how far two correct float64 evaluations of the same chain may drift apart (E64, tests/test_prune_cpu.py).
"""
import numpy as np

RES = 0.15
GAP_MIN = 1e-6      # a patch is compared only while the two smallest scores of every step differ by more than this (relative)

# capacity, l_sq = (res / div)^2, points per patch, keeps, patches.  Together the rows put b on both sides of 16, 64 and 128 and reach the
# three workgroup shapes (64 threads at capacity <= 64, 128 at <= 100, else 256).  The capacity -1 row is the exact GP, nothing is deleted
# while it trains: with eps_tol = 1e-3 and this l_sq the CPU oracle keeps 130 to 132 of a patch's 132 points.
REGIMES = [
    (16, 3.0, 60, (5,), 24),
    (40, 6.0, 120, (12,), 24),
    (64, 8.0, 200, (20,), 12),
    (100, 10.0, 300, (65, 30), 12),
    (-1, 10.0, 132, (60,), 8),
]

# E64 per array: the largest gap, over the regimes above (ny = 1 and ny = 3, oracle-trained states), between the float64 oracle and the
# longdouble restatement started from the same bits, relative to the array's largest magnitude in the patch.  Measured by
# tests/test_prune_cpu.py::test_e64 (which fails if the measurement exceeds these figures); the GPU gate is 64 x E64.  The figures are the
# measured 1.701e-10, 3.418e-11, 1.020e-11, 0, 4.362e-10, 1.970e-09 with the third digit rounded up; every one comes from the capacity -1
# row (130 vectors, noise 1e-2).  BV is only ever copied, so its gate is equality.
E64 = dict(alpha=1.71e-10, C=3.42e-11, Q=1.03e-11, BV=0.0, mean=4.37e-10, sigma=1.98e-9)
GATE_FACTOR = 64.0


def kernel_kw(cap, div, ny):
    return dict(sigmaf_sq=1.0, l_sq=(RES / div) ** 2, noise=1e-2 if ny == 1 else 1.0, eps_tol=1e-3, capacity=cap)


def oracle_params(oracle, cap, div, ny, bug=0):
    kw = kernel_kw(cap, div, ny)
    return oracle.sparse_params(ny, p0=kw["sigmaf_sq"], p1=kw["l_sq"], s20=kw["noise"], eps_tol=kw["eps_tol"], capacity=cap,
                                field_delete_bug=bug)


def batch(cap, n, P, ny):
    """uniform points, a smooth surface plus noise (gp_compressor_amd.synth.make_patches), one insertion order per patch"""
    from gp_compressor_amd import synth
    off, x0, x1, y = synth.make_patches(P, n, res=RES, seed=100 + (cap % 97) + ny, ragged=False, ny=ny)
    return off, x0, x1, y, synth.sattolo_perms(off, seed=11)


# ---- the arg-min ------------------------------------------------------------------------------------------------------------------

def sp_take(ov, oi, val, idx):
    """SP_TAKE of csrc/sparse_device.h: does (ov, oi) come before (val, idx) in the order in which the reference's scan picks its minimum --
    a NaN at index 0 first, then by value with NaN last, then by index"""
    nan0 = lambda v, i: i == 0 and v != v
    return bool(nan0(ov, oi) or (not nan0(val, idx) and (ov < val or (ov == val and oi < idx) or (val != val and ov == ov))))


def argmin_scan(s):
    """the reference's scan, literally (src/sparse_gp.hpp:210-217)"""
    minscore, loc = s[0], 0
    for i in range(1, len(s)):
        if s[i] < minscore:
            minscore, loc = s[i], i
    return loc, minscore


def argmin_take(s, order):
    """the same minimum as a fold of SP_TAKE over the indices in any `order` (what a tree reduction does)"""
    loc = order[0]
    for i in order[1:]:
        if sp_take(s[i], i, s[loc], loc):
            loc = i
    return loc, s[loc]


def scores_of(alpha, C, Q):
    a2 = np.zeros(alpha.shape[1], dtype=alpha.dtype)
    for c in range(alpha.shape[0]):
        a2 = a2 + alpha[c] * alpha[c]
    with np.errstate(all="ignore"):
        return a2 / (np.diagonal(Q) + np.diagonal(C))


def score_gap(s):
    """relative distance of the two smallest scores (inf when fewer than two are finite)"""
    f = np.sort(np.asarray(s, dtype=np.float64)[np.isfinite(np.asarray(s, dtype=np.float64))])
    if len(f) < 2:
        return np.inf
    return float((f[1] - f[0]) / max(abs(f[1]), np.finfo(np.float64).tiny))


# ---- delete_bv and the loop ---------------------------------------------------------------------------------------------------------

def delete_bv(alpha, C, Q, BV, loc, field_bug):
    """delete_bv(loc) on alpha (ny, b), C, Q (b, b), BV (b, 2); returns the (b - 1)-sized state.  Operation order of oracle/gpc_oracle.c."""
    ny, b = alpha.shape
    last, nb = b - 1, b - 1
    alpha, C, Q, BV = alpha.copy(), C.copy(), Q.copy(), BV.copy()
    alphastar = alpha[:, loc].copy()
    alpha[:, loc] = alpha[:, last]
    out = []
    for M in (C, Q):
        star = M[loc, loc]
        col = M[:, loc].copy()
        col[loc] = col[last]
        rep = M[:, last].copy()
        rep[loc] = rep[last]
        M[loc, :] = rep
        M[:, loc] = rep
        out.append((star, col[:nb]))
    (cstar, Cstar), (qstar, Qstar) = out
    qc = Qstar + Cstar
    den = qstar + cstar
    with np.errstate(all="ignore"):
        if ny == 1:
            alpha[0, :nb] -= (alphastar[0] / den) * qc
        else:
            m = den * qc if field_bug else qc / den
            alpha[:, :nb] -= alphastar[:, None] * m[None, :]
        qq = np.outer(Qstar, Qstar) / qstar
        cc = np.outer(qc, qc) / den
        C[:nb, :nb] += qq - cc
        Q[:nb, :nb] -= qq
    BV[loc] = BV[last]
    return alpha[:, :nb], C[:nb, :nb], Q[:nb, :nb], BV[:nb]


def prune(alpha, C, Q, BV, target, score_tol=0.0, field_bug=0, dtype=np.float64):
    """The rule on one patch's state (alpha (ny, b), C and Q (b, b) as M[i, j], BV (b, 2)).  Returns dict(order, scores, gap, alpha, C, Q,
    BV): gap is the smallest score_gap over the steps taken."""
    alpha, C, Q = (np.array(a, dtype=dtype) for a in (alpha, C, Q))
    BV = np.array(BV, dtype=np.float64)
    t = max(1, int(target))
    order, scores, gap = [], [], np.inf
    while alpha.shape[1] > 1:
        s = scores_of(alpha, C, Q)
        loc, m = argmin_scan(s)
        if not (alpha.shape[1] > t or m < score_tol):
            break
        gap = min(gap, score_gap(s))
        order.append(loc)
        scores.append(float(m))
        alpha, C, Q, BV = delete_bv(alpha, C, Q, BV, loc, field_bug)
    return dict(order=np.array(order, dtype=np.int32), scores=np.array(scores), gap=gap, alpha=alpha, C=C, Q=Q, BV=BV)


def oracle_prune(g, target, score_tol=0.0):
    """The same loop with the oracle's own delete_bv (tests/oracle_lib.Sparse `g`, modified in place): the scan reads the oracle's state."""
    t = max(1, int(target))
    order, scores, gap = [], [], np.inf
    while g.size() > 1:
        alpha, C, Q, _ = g.state()
        s = scores_of(alpha, C, Q)
        loc, m = argmin_scan(s)
        if not (g.size() > t or m < score_tol):
            break
        gap = min(gap, score_gap(s))
        order.append(loc)
        scores.append(float(m))
        g.delete_bv(loc)
    alpha, C, Q, BV = g.state()
    return dict(order=np.array(order, dtype=np.int32), scores=np.array(scores), gap=gap, alpha=alpha, C=C, Q=Q, BV=BV)


def predict(alpha, C, BV, xs0, xs1, sigmaf_sq, l_sq, noise):
    """predict_measurements (src/sparse_gp.hpp:299-351) in the dtype of alpha: mean (ny, m), sigma (m)"""
    dt = alpha.dtype
    X = np.stack([xs0, xs1], 1).astype(dt)
    d = X[:, None, :] - BV.astype(dt)[None, :, :]
    k = dt.type(sigmaf_sq) * np.exp(dt.type(np.float32(-0.5)) / dt.type(l_sq) * (d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]))    # (m, b)
    mean = alpha @ k.T
    var = dt.type(noise) + dt.type(sigmaf_sq) + np.einsum("pi,ij,pj->p", k, C, k)
    return mean, np.sqrt(np.maximum(var, 0))


def rel_gap(a, ref):
    """largest |a - ref| relative to the largest magnitude of ref"""
    ref = np.asarray(ref, dtype=np.longdouble)
    scale = np.max(np.abs(ref)) if ref.size else 0
    if not ref.size:
        return 0.0
    return float(np.max(np.abs(np.asarray(a, dtype=np.longdouble) - ref)) / (scale if scale > 0 else 1))


ARRAYS = ("alpha", "C", "Q", "BV", "mean", "sigma")


def gaps(a, ref, kw, xs0, xs1, a_pred=None):
    """rel_gap per array between two results of prune / oracle_prune; the read-outs of `a` are a_pred = (mean, sigma) when given (the GPU's
    or the oracle's own predict), else the restatement's on a's state"""
    out = {k: rel_gap(a[k], ref[k]) for k in ("alpha", "C", "Q", "BV")}
    pr = predict(np.asarray(ref["alpha"]), np.asarray(ref["C"]), ref["BV"], xs0, xs1, kw["sigmaf_sq"], kw["l_sq"], kw["noise"])
    pa = a_pred if a_pred is not None else predict(np.asarray(a["alpha"]), np.asarray(a["C"]), a["BV"], xs0, xs1, kw["sigmaf_sq"], kw["l_sq"],
                                                   kw["noise"])
    out["mean"] = rel_gap(pa[0], pr[0])
    out["sigma"] = rel_gap(pa[1], pr[1])
    return out


# ---- the cases ------------------------------------------------------------------------------------------------------------------------

def case_ids():
    """(capacity, div, n, P, ny, keep) of every numeric case"""
    return [(cap, div, n, P, ny, keep) for cap, div, n, keeps, P in REGIMES for ny in (1, 3) for keep in keeps]


def oracle_states(oracle, cap, div, n, P, ny, bug=0):
    """the regime's batch trained on the CPU oracle: a list of per-patch states (alpha (ny, b), C, Q (b, b), BV (b, 2))"""
    off, x0, x1, y, perm = batch(cap, n, P, ny)
    op = oracle_params(oracle, cap, div, ny, bug)
    out = []
    for i in range(P):
        sl = slice(off[i], off[i + 1])
        g = oracle.Sparse(op, max(cap, n) + 2)
        g.add_measurements(x0[sl], x1[sl], y[:, sl], perm[sl])
        out.append(g.state())
    return out


def run_oracle(oracle, states, cap, div, ny, keep, xs0, xs1, score_tol=0.0, bug=0):
    """oracle_prune of every state (loaded with set_state: the same bits), with the oracle's own read-out on the grid"""
    op = oracle_params(oracle, cap, div, ny, bug)
    out = []
    for alpha, C, Q, BV in states:
        g = oracle.Sparse(op, alpha.shape[1] + 2)
        g.set_state(alpha, C, Q, BV)
        r = oracle_prune(g, keep, score_tol)
        r["pred"] = g.predict(xs0, xs1)
        out.append(r)
    return out


def measure_e64(oracle, states, cap, div, ny, keep, xs0, xs1):
    """One case on the CPU: the oracle, the float64 restatement and the longdouble restatement from the same bits.  Returns (oracle results,
    kept patch indices, gaps of the float64 restatement per kept patch, gaps of the oracle against longdouble per kept patch)."""
    kw = kernel_kw(cap, div, ny)
    orc = run_oracle(oracle, states, cap, div, ny, keep, xs0, xs1)
    kept, g64, gld = [], [], []
    for i, (st, o) in enumerate(zip(states, orc)):
        if not o["gap"] > GAP_MIN:
            continue
        r64 = prune(*st, keep, dtype=np.float64)
        rld = prune(*st, keep, dtype=np.longdouble)
        assert np.array_equal(r64["order"], o["order"]) and np.array_equal(rld["order"], o["order"]), (i, o["order"], r64["order"], rld["order"])
        kept.append(i)
        g64.append(gaps(r64, o, kw, xs0, xs1))
        gld.append(gaps(o, rld, kw, xs0, xs1, a_pred=o["pred"]))
    return orc, kept, g64, gld
