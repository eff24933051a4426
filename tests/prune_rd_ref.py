"""NumPy restatement of the distortion-bounded prune rule (include/gpc.h, gpc_sparse_prune_rd) on top of prune_ref, the cases the
prune_rd tests share and the constants measured for them.

Per patch, with its points (x0, x1, y (ny, n)), floor t = max(1, target) and bound B:

    mse0 = mse(current state)
    loop:
      if b <= 1 or b <= t: stop                                  (mse_next = NaN)
      (minscore, loc) = prune_ref.argmin_scan(prune_ref.scores_of(state))
      state' = prune_ref.delete_bv(state, loc);  e = mse(alpha', BV')      (the look-ahead IS the error of the state delete_bv leaves)
      if !(e <= B): mse_next = e; stop
      order += [loc]; scores += [minscore]; mse += [e]; state = state'

mse of (alpha, BV) on the points, in the summation order the header fixes: k_ij as prune_ref.predict forms it; f_ci over j ascending
(numpy.cumsum is sequential); e_i over c ascending; point i into class i mod 64, each class in ascending i; the 64 class sums by the xor
tree d = 32 .. 1; divided by n * ny.  Everything runs in the dtype it is given (float64, numpy.longdouble).
"""
import numpy as np

import prune_ref as pr

BAND = 1e-6         # a patch is compared only while no error the loop saw lies within this (relative) of its bound

# The look-ahead of the float64 restatement against the oracle: its own delete_bv followed by its own predict at the patch's points, the
# error summed plainly in float64.  Measured by tests/test_prune_rd_cpu.py::test_lookahead_vs_oracle over the first removals of two
# patches per regime (oracle-trained states, ny = 1 and 3): 6.010e-15 relative (capacity -1, ny = 1), third digit rounded up.  The
# two differ by the order of the sums over j and over the points only; the gate is the project's usual factor times the figure, so that
# another libm's exp (a few ulp, entering as ulp * sqrt-ish of the terms) does not trip it while a wrong row, column or swap (1e-2) does.
E_LOOKAHEAD = 6.02e-15

# E64_MSE: the largest relative gap of the `mse` trace between the float64 and the longdouble restatement started from the same bits,
# counted while the two pick the same order, over all regimes of prune_ref.REGIMES (ny = 1 and 3, oracle-trained states) pruned down to
# one vector.  Measured by tests/test_prune_rd_cpu.py::test_e64_mse (which fails if the measurement exceeds the record): 7.839e-11, from
# the capacity -1 row (ny = 3), third digit rounded up.  The GPU gate is prune_ref.GATE_FACTOR (64) times the record, the convention of
# prune_ref.E64.
E64_MSE = 7.84e-11


def kernel_matrix(BV, x0, x1, sigmaf_sq, l_sq, dtype):
    """k (n, b) with the expression of prune_ref.predict"""
    dt = np.dtype(dtype)
    X = np.stack([x0, x1], 1).astype(dt)
    d = X[:, None, :] - np.asarray(BV).astype(dt)[None, :, :]
    return dt.type(sigmaf_sq) * np.exp(dt.type(np.float32(-0.5)) / dt.type(l_sq) * (d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]))


def class_sum(e):
    """the n per-point errors in the fixed order: class i mod 64 in ascending i, then the xor tree d = 32, 16, .. 1"""
    acc = np.zeros(64, dtype=e.dtype)
    for i0 in range(0, len(e), 64):
        c = e[i0:i0 + 64]
        acc[:len(c)] = acc[:len(c)] + c
    lanes = np.arange(64)
    d = 32
    while d >= 1:
        acc = acc + acc[lanes ^ d]
        d >>= 1
    return acc[0]


def mse_of(alpha, BV, x0, x1, y, sigmaf_sq, l_sq, dtype=np.float64):
    dt = np.dtype(dtype)
    ny, b = alpha.shape
    n = len(x0)
    if n == 0:
        return dt.type(np.nan)
    alpha = np.asarray(alpha, dtype=dt)
    yv = np.asarray(y, dtype=dt).reshape(ny, n)
    with np.errstate(all="ignore"):
        k = kernel_matrix(BV, x0, x1, sigmaf_sq, l_sq, dt)
        e = np.zeros(n, dtype=dt)
        for c in range(ny):
            f = np.cumsum(alpha[c][None, :] * k, axis=1)[:, -1] if b else np.zeros(n, dtype=dt)
            r = yv[c] - f
            e = e + r * r
        return class_sum(e) / dt.type(n * ny)


def prune_rd(alpha, C, Q, BV, x0, x1, y, target, bound, kw, field_bug=0, dtype=np.float64):
    """The rule on one patch.  bound: a number, or a callable mse0 -> bound (relative bounds).  Returns dict(order, scores, mse, mse0,
    mse_next, bound, gap, band, alpha, C, Q, BV): gap is the smallest prune_ref.score_gap over the scans made (the stopping one
    included), band the smallest relative distance to the bound of the errors the loop saw (accepted steps and the stopping look-ahead)."""
    dt = np.dtype(dtype)
    alpha, C, Q = (np.array(a, dtype=dt) for a in (alpha, C, Q))
    BV = np.array(BV, dtype=np.float64)
    sf, l_sq = kw["sigmaf_sq"], kw["l_sq"]
    t = max(1, int(target))
    order, scores, mse, gap, band = [], [], [], np.inf, np.inf
    mse0 = mse_of(alpha, BV, x0, x1, y, sf, l_sq, dt)
    B = bound(mse0) if callable(bound) else bound
    nxt = dt.type(np.nan)
    while len(x0) and alpha.shape[1] > 1 and alpha.shape[1] > t:
        s = pr.scores_of(alpha, C, Q)
        loc, m = pr.argmin_scan(s)
        gap = min(gap, pr.score_gap(s))
        new = pr.delete_bv(alpha, C, Q, BV, loc, field_bug)
        e = mse_of(new[0], new[3], x0, x1, y, sf, l_sq, dt)
        if np.isfinite(float(e)) and np.isfinite(float(B)) and float(B) > 0:
            band = min(band, abs(float(e) - float(B)) / float(B))
        if not (e <= B):
            nxt = e
            break
        order.append(loc)
        scores.append(float(m))
        mse.append(e)
        alpha, C, Q, BV = new
    return dict(order=np.array(order, dtype=np.int32), scores=np.array(scores), mse=np.array(mse, dtype=dt), mse0=mse0, mse_next=nxt,
                bound=B, gap=gap, band=band, alpha=alpha, C=C, Q=Q, BV=BV)


def comparable(r):
    """the two exclusions of the GPU comparison, on a restatement run"""
    return r["gap"] > pr.GAP_MIN and r["band"] > BAND


def rel(a, ref):
    """largest elementwise |a - ref| / |ref| (0 for empty input)"""
    a, ref = np.asarray(a, dtype=np.longdouble).ravel(), np.asarray(ref, dtype=np.longdouble).ravel()
    if not ref.size:
        return 0.0
    return float(np.max(np.abs(a - ref) / np.abs(ref)))


def regimes():
    """(capacity, div, n, P, ny) of every regime row: prune_ref.REGIMES with ny = 1 and 3"""
    return [(cap, div, n, P, ny) for cap, div, n, _, P in pr.REGIMES for ny in (1, 3)]


def points(cap, n, P, ny):
    """the regime's batch as per-patch (x0, x1, y (ny, n)) -- the points its states were trained on"""
    off, x0, x1, y, _ = pr.batch(cap, n, P, ny)
    return off, x0, x1, y, [(x0[off[i]:off[i + 1]], x1[off[i]:off[i + 1]], y[:, off[i]:off[i + 1]]) for i in range(P)]
