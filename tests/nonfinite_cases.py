"""Non-finite inputs and loaded states for the sparse add (test infrastructure: tests/test_oracle.py, tests/test_sparse_nonfinite_gpu.py,
tests/sparse_sweep.py).

The hyper-parameters are the well-conditioned ones of test_sparse_batch_vs_oracle (the GPU and the CPU oracle take the same decisions on
finite data).  Every injected value is a NaN or an infinity that no finite intermediate can meet by overflow, so which entries come out NaN
and which +-inf does not depend on the order of a sum."""
import numpy as np

RES = 0.15
KW1 = dict(sigmaf_sq=1.0, l_sq=(RES / 8) ** 2, noise=1e-4)      # add-path regime (ny = 1; ny = 3 takes noise 1.0)
KW_BIG = dict(sigmaf_sq=1.0, l_sq=(RES / 6) ** 2, noise=1e-2, eps_tol=1e-3)   # capacity > 48: smoke()'s well-conditioned regime
KW_LOAD = dict(sigmaf_sq=1.0, l_sq=(RES / 20) ** 2, noise=1e-4)  # loaded states: a lattice basis with a short length scale

# poisons of a patch's points (case B1); each takes (x0, x1, y, o, n, order) -- the patch's points are o .. o + n - 1, `order` the
# patch-local insertion order -- and writes in place
POISONS = ("y_nan", "y_inf", "x0_nan", "x1_inf_first")


def poison(kind, x0, x1, y, o, n, order):
    mid = o + int(order[n // 2])
    if kind == "y_nan":                 # alpha goes NaN; C and Q stay finite
        y[0, mid] = np.nan
    elif kind == "y_inf":               # one channel of three (or the only one)
        y[y.shape[0] - 1, mid] = np.inf
    elif kind == "x0_nan":
        x0[mid] = np.nan
    elif kind == "x1_inf_first":        # k* = NaN on the FIRST point: the reference's C(0, 0), Q(0, 0), alpha_0 are NaN
        x1[o + int(order[0])] = np.inf
    else:
        raise ValueError(kind)


def one_point_nan(off, x0, x1, y, j):
    """the batch with patch j cut down to one point whose coordinates are NaN -> (off, x0, x1, y, keep) with keep the kept point indices"""
    keep = np.concatenate([np.arange(off[i], off[i + 1] if i != j else off[i] + 1) for i in range(len(off) - 1)]).astype(np.int64)
    counts = np.diff(off).copy()
    counts[j] = 1
    off2 = np.zeros_like(off)
    off2[1:] = np.cumsum(counts)
    x0, x1, y = x0[keep].copy(), x1[keep].copy(), np.ascontiguousarray(y[:, keep])
    x0[off2[j]] = np.nan
    x1[off2[j]] = np.nan
    return off2, x0, x1, y, keep


def lattice_state(b, ny, seed, kw=KW_LOAD, res=RES):
    """A finite state of the exact recursion on b basis vectors (jittered lattice over the patch): Q = K^-1, C = -(K + s20 I)^-1,
    alpha = (K + s20 I)^-1 y, both matrices exactly symmetric (include/gpc.h: a loaded state must be) -> alpha (ny, b), C, Q, BV (b, 2)"""
    rng = np.random.default_rng(seed)
    m = int(np.ceil(np.sqrt(b)))
    g = res * ((np.arange(m) + 0.5) / m - 0.5)
    xx, yy = np.meshgrid(g, g)
    BV = np.stack([xx.ravel(), yy.ravel()], axis=1)[:b] + rng.uniform(-0.1, 0.1, size=(b, 2)) * (res / m)
    d2 = ((BV[:, None, :] - BV[None, :, :]) ** 2).sum(-1)
    K = kw["sigmaf_sq"] * np.exp(-0.5 / kw["l_sq"] * d2)
    Q = np.linalg.inv(K)
    Ci = np.linalg.inv(K + kw["noise"] * np.eye(b))
    sym = lambda M: (M + M.T) / 2
    y = rng.normal(0.0, 0.01 if ny == 1 else 50.0, size=(ny, b))
    return np.ascontiguousarray(y @ Ci), sym(-Ci), sym(Q), np.ascontiguousarray(BV)


def loaded_case(case, cap, ny, seed=0):
    """The loaded states of case B2 -> (alpha, C or None, Q or None, BV):
      a  the decompressor's load (C, Q NULL), b == capacity, alpha_0 = 0: the reference deletes vector 0 (0/0 at index 0 sticks)
      b  the same with alpha_3 = 0 (a NaN score elsewhere is skipped: both delete the new vector)
      c  alpha_0 = NaN with finite C and Q, b == capacity: every score is NaN after a full update, vector 0 goes
      d  Q(2, 5) = Q(5, 2) = +inf on a basis of `cap` vectors (loaded into a larger capacity): s_hat is +-inf in two rows"""
    alpha, C, Q, BV = lattice_state(cap, ny, seed)
    if case == "a":
        alpha[:, 0] = 0.0
        return alpha, None, None, BV
    if case == "b":
        alpha[:, 3] = 0.0
        return alpha, None, None, BV
    if case == "c":
        alpha[0, 0] = np.nan
        return alpha, C, Q, BV
    if case == "d":
        Q[2, 5] = Q[5, 2] = np.inf
        return alpha, C, Q, BV
    raise ValueError(case)


def new_points(n, ny, seed, res=RES):
    """n fresh points over the patch (the add call that follows a load): x0, x1 (n,), y (ny, n)"""
    rng = np.random.default_rng(seed + 1000)
    x0 = rng.uniform(-res / 2, res / 2, size=n)
    x1 = rng.uniform(-res / 2, res / 2, size=n)
    y = rng.normal(0.0, 0.01 if ny == 1 else 50.0, size=(ny, n))
    return x0, x1, np.ascontiguousarray(y)


def ref_capacity_argmin(alpha, Qd, Cd):
    """src/sparse_gp.hpp:206-217 transcribed: the vector a capacity deletion removes (alpha (ny, b), the diagonals of Q and C)"""
    minscore, minloc = np.float64(0.0), -1
    with np.errstate(all="ignore"):
        for i in range(alpha.shape[1]):
            a2 = np.float64(0.0)
            for c in range(alpha.shape[0]):
                a2 = a2 + alpha[c, i] * alpha[c, i]
            score = a2 / (np.float64(Qd[i]) + np.float64(Cd[i]))      # IEEE: 0/0 = NaN, a/0 = +-inf
            if i == 0 or score < minscore:
                minscore, minloc = score, i
    return minloc
