"""Handmade states, query sets, an extended-precision reference and forward-error bounds for the kernels that READ a sparse GP state:
sparse_predict_kernel / sparse_predict_small_kernel (mean, sigma, confidence), sparse_likelihood_kernel (l, dX and the raw pass) and
sparse_train_kernel.  Test infrastructure (tests/test_readout_cpu.py, tests/test_sparse_readout_gpu.py); importable without a GPU.

Nothing is trained: a state of exactly b basis vectors is written down and loaded with Sparse.set_state, so the basis sizes at which
the kernels change path -- the 16-row tiles of sp_ck_chunk, its four waves, SP_RT = 4 row tiles per wave, the four-deep prefetch, the 16-
and 32-vector kernels, the 240-row limit of the MFMA branch of the likelihood kernel -- are hit exactly, and a case costs milliseconds.

The reference is the closed form of registration_ref.closed_form_likelihood and np_restatement.train_sigmaf_np evaluated in
np.longdouble (the x87 80-bit type: eps = 2^-63, 2048 times finer than the float64 the kernels compute in).

Bounds (EPS = 2^-52; all derived from the operations the kernels perform, none from what a kernel returned)
---------------------------------------------------------------------------------------------------------
Every rounding is counted as one EPS, twice its worst case u = EPS / 2: a sum of n products in any order carries gamma_n = n u / (1 - n u)
on the sum of the magnitudes of its terms and is given n EPS; the device's table-driven exp is held to 2 ulp (as
test_sparse_small_basis_predict_kernel assumes) and is given 4 EPS.

k_j = sf exp(a_j), a_j = c |x - BV_j|^2.  The argument is rounded before the exponential sees it, and exp has condition number |a_j|.
gpc_rbf_neg rounds SIX times on the way: the two differences x - BV_j, the product d1 d1, the fused d0 d0 + (d1 d1), the quotient c = -0.5 / l^2
on the host and the product c sq -- a relative error of the argument of at most 6 u, 6 EPS as counted here.  So k_j carries a relative error of
(6 |a_j| + 4) EPS.  [The plan for this module counted ONE rounding of the argument, (|a_j| + 4) EPS; a correct float64 evaluation of a
one-vector mean uses 0.63 of a bound made from that.  The term was re-derived from the operations above, not fitted to a result.]

  mean     |f_c - ref|   <= EPS sum_j (b + 8 + 6 |a_j|) |alpha_cj| |k_j|
               per term: the factor k_j (6 |a_j| + 4), the b-term sum (b), four EPS spare.  b = 0: f = 0 exactly, bound 0.
  sigma^2  |s2 - ref|    <= (2 b + 16 + 2 amax) EPS (mag + sf + s20),   mag = sum_ij |k_i| |C_ij| |k_j|,  amax = max_j |a_j| of the query
               as planned: the b-term sum of V = C k and the b-term sum k^T V (2 b), two factors k, the two additions of
               s20 + k* + k^T C k.  It is not widened for the six roundings of the argument: a term with a large |a| has a small k, and
               the worst case of the operations with every rounding at its full u,
                   EPS [ (b + 8) mag + 6 sum_ij |a_i| |k_i| |C_ij| |k_j| + 2 (sf + s20) ]        (`s2_worst` of evaluate()),
               stays below it at every query of every case (asserted in tests/test_readout_cpu.py; 0.53 of it at most).  The kernels return
               sigma = sqrt(s2); squared back that adds <= 4 EPS s2 (a square root within 1 ulp, one product), which sigma2_tolerance() adds.
  conf     |conf - ref|  <= 100 / (sf + s20) * (sigma^2 bound) + 400 EPS
               100 (1 - s2 / (k* + s20)): the quotient is <= 1 for a state with negative definite C; a division, a subtraction from
               1 and a product, each within u of a value <= 1, times 100, rounded up to 4 EPS 100.
  l, dX    the project's statement in test_sparse_likelihood_and_derivatives: 1e-8 of the largest reference value of the patch's queries
               (sigma enters dX as sigma^-3 and l through exp(-|off|^2 / (2 sigma)); with sigma >= s20 / 2 and |off| = O(0.1) the derived
               sigma^2 error of <= 1e-12 is amplified by <= 1e4).
  training the statement in test_sparse_train_sigmaf: 1e-9 on the parameter, 1e-8 (+ 1e-12) on the last gradient relative to its
               largest component, 1e-7 (+ 1e-9) on the likelihood trace relative to its largest entry.
"""
import functools

import numpy as np

from np_restatement import train_sigmaf_np
from registration_ref import closed_form_likelihood, likelihood_tail

LD = np.longdouble
EPS = float(np.finfo(np.float64).eps)
RES = 0.15
SF, S20 = 1.0, 1e-2
L5, L8 = (RES / 5) ** 2, (RES / 8) ** 2
N_EXTRA = 37                      # uniform queries per patch on top of its own basis vectors: m = b + 37
NOISE_Y = 0.05
TRAIN_STEP, TRAIN_MAXC = float(np.float32(1e-4)), 3

# capacity -> the basis sizes of its patches (include/gpc.h: ld = round_up(capacity + 1, 16), 256 for capacity -1).  Patch 0 is the empty
# one and HAS points; one more empty patch WITHOUT points is put in the middle of every batch (patches()).
BASES = {
    15: (0, 1, 15, 16),
    100: (0, 1, 3, 4, 5, 16, 17, 31, 32, 33, 47, 48, 49, 63, 64, 65, 100, 101),
    239: (0, 33, 64, 65, 127, 128, 129, 191, 192, 193, 200, 239, 240),
    -1: (0, 1, 20, 33, 65, 129, 255, 256),
}
# (capacity, ny, l^2): both length scales on small and on large objects
CASES = [(15, 1, L5), (100, 1, L8), (100, 3, L5), (239, 1, L5), (-1, 1, L8), (-1, 3, L5)]
CASE_IDS = [f"cap{c}-ny{ny}" for c, ny, _ in CASES]


def ld_of(capacity):
    return 256 if capacity == -1 else (capacity + 1 + 15) & ~15


def patches(capacity):
    """[(b, has_points)] of the object's batch: BASES[capacity] with an empty, point-less patch in the middle"""
    bs = [(b, True) for b in BASES[capacity]]
    bs.insert(len(bs) // 2, (0, False))
    return bs


def smooth_y(ny, x0, x1):
    """(ny, n): a smooth surface per channel, amplitude ~0.5, a few periods over the patch"""
    u, v = np.asarray(x0) / RES, np.asarray(x1) / RES
    return np.stack([0.5 * np.sin(2 * np.pi * ((1.0 + 0.5 * c) * u + 0.17 * c)) + 0.3 * np.cos(2 * np.pi * (0.8 - 0.2 * c) * v) for c in range(ny)])


def state(b, ny, l_sq, seed):
    """A genuine GP state of exactly b vectors: BV (b, 2) uniform in the +-RES/2 window, C = -(K_BV + s20 I)^-1 symmetrised,
    alpha (ny, b) = ((K_BV + s20 I)^-1 y_BV)^T for smooth_y.  sigma_f^2 = 1, s20 = 1e-2: |C| <= 1 / s20 and sigma^2 >= s20 - O(1e-13)
    at every query.  Returns alpha, C, BV (Q is not read by the read-out kernels: loaded as zeros)."""
    rng = np.random.default_rng(seed)
    BV = rng.uniform(-RES / 2, RES / 2, size=(b, 2))
    if b == 0:
        return np.zeros((ny, 0)), np.zeros((0, 0)), BV
    d2 = ((BV[:, None, :] - BV[None, :, :]) ** 2).sum(-1)
    Ci = np.linalg.inv(SF * np.exp(-0.5 / l_sq * d2) + S20 * np.eye(b))
    Ci = 0.5 * (Ci + Ci.T)
    alpha = smooth_y(ny, BV[:, 0], BV[:, 1]) @ Ci
    return np.ascontiguousarray(alpha), -Ci, BV


def _freeze(d):
    for v in d.values():
        if isinstance(v, np.ndarray):
            v.flags.writeable = False
    return d


@functools.lru_cache(maxsize=None)
def batch(capacity, ny, l_sq):
    """The object's loaded state and its ragged query set (read-only arrays, built once):
    P, ld, b (P,), alpha (P, ny, ld), C (P, ld, ld), BV (P, ld, 2) as Sparse.set_state takes them; off (P + 1,), q0, q1 (N,), yq (ny, N)
    -- every patch with points gets its own basis vectors followed by N_EXTRA uniform points; yq = smooth_y + N(0, NOISE_Y)."""
    pl = patches(capacity)
    P, ld = len(pl), ld_of(capacity)
    bs = np.array([b for b, _ in pl], dtype=np.int32)
    alpha, C, BV = np.zeros((P, ny, ld)), np.zeros((P, ld, ld)), np.zeros((P, ld, 2))
    rng = np.random.default_rng(7000 + 10 * (capacity % 1000) + ny)
    q0, q1, cnt = [], [], []
    for i, (b, pts) in enumerate(pl):
        a, c, v = state(b, ny, l_sq, seed=1000 * (capacity % 1000) + 10 * i + ny)
        alpha[i, :, :b], C[i, :b, :b], BV[i, :b] = a, c, v
        n = b + N_EXTRA if pts else 0
        cnt.append(n)
        if pts:
            q0.append(np.concatenate([v[:, 0], rng.uniform(-RES / 2, RES / 2, N_EXTRA)]))
            q1.append(np.concatenate([v[:, 1], rng.uniform(-RES / 2, RES / 2, N_EXTRA)]))
    off = np.concatenate([[0], np.cumsum(cnt)]).astype(np.int32)
    q0, q1 = np.concatenate(q0), np.concatenate(q1)
    yq = smooth_y(ny, q0, q1) + rng.normal(0.0, NOISE_Y, (ny, len(q0)))
    return _freeze(dict(capacity=capacity, ny=ny, l_sq=l_sq, P=P, ld=ld, b=bs, alpha=alpha, C=C, BV=BV, off=off, q0=q0, q1=q1,
                        yq=np.ascontiguousarray(yq)))


CLAMP_B = 65


@functools.lru_cache(maxsize=None)
def clamp_batch():
    """One clamp decision far from its boundary: a capacity-100 object of three patches (65, 65 and 20 vectors, l^2 = L8), the middle
    one with C replaced by -(2 / sf) I.  At a query that IS basis vector j, k_j = sf exactly and k^T C k = -(2 / sf) |k|^2 <= -2 sf, so
    s20 + sf + k^T C k <= s20 - sf < 0: sigma is clamped to 0 and the confidence form is 100 (1 - 0) = 100.  Same layout as batch()."""
    ny, ld, l_sq = 1, ld_of(100), L8
    bs = np.array([CLAMP_B, CLAMP_B, 20], dtype=np.int32)
    P = len(bs)
    alpha, C, BV = np.zeros((P, ny, ld)), np.zeros((P, ld, ld)), np.zeros((P, ld, 2))
    rng = np.random.default_rng(4242)
    q0, q1 = [], []
    for i, b in enumerate(bs):
        a, c, v = state(int(b), ny, l_sq, seed=4300 + i)
        if i == 1:
            c = -(2.0 / SF) * np.eye(b)
        alpha[i, :, :b], C[i, :b, :b], BV[i, :b] = a, c, v
        q0.append(np.concatenate([v[:, 0], rng.uniform(-RES / 2, RES / 2, N_EXTRA)]))
        q1.append(np.concatenate([v[:, 1], rng.uniform(-RES / 2, RES / 2, N_EXTRA)]))
    off = np.concatenate([[0], np.cumsum(bs + N_EXTRA)]).astype(np.int32)
    return _freeze(dict(capacity=100, ny=ny, l_sq=l_sq, P=P, ld=ld, b=bs, alpha=alpha, C=C, BV=BV, off=off, q0=np.concatenate(q0),
                        q1=np.concatenate(q1)))


def patch_state(B, i):
    """alpha (ny, b), C (b, b), BV (b, 2) of patch i of a batch"""
    b = int(B["b"][i])
    return B["alpha"][i][:, :b], B["C"][i][:b, :b], B["BV"][i][:b]


def evaluate(B, i, q0, q1, yq=None, dtype=LD, C=None):
    """The closed form for patch i of batch B at the queries q0, q1 (yq: zeros when only the prediction is wanted), in `dtype`
    (None: float64 NumPy).  C: another matrix in the place of the patch's.  Returns closed_form_likelihood's parts plus
      f (ny, m), s2 (m,) not clamped, conf (m,) the confidence form of the clamped s2,
      fb (ny, m), s2b (m,), confb (m,): the bounds of the module docstring (float64)."""
    alpha, Cm, BV = patch_state(B, i)
    if C is not None:
        Cm = C
    b, ny = len(BV), alpha.shape[0]
    with np.errstate(invalid="ignore" if yq is None else "warn"):     # (prediction only: l and dX of a sigma^2 < 0 are nobody's business)
        r = closed_form_likelihood(SF, B["l_sq"], S20, alpha, Cm, BV, q0, q1, np.zeros((ny, len(q0))) if yq is None else yq, dtype=dtype,
                                   parts=True)
    one = (dtype or np.float64)(1)
    kk = one * SF + one * S20
    r["f"], r["s2"] = r["mu"], r["sigma"]
    r["conf"] = 100 * (one - np.maximum(r["sigma"], 0) / kk)
    absK, absA = np.abs(np.asarray(r["K"], dtype=np.float64)), np.abs(np.asarray(r["A"], dtype=np.float64))
    amax = np.max(absA, axis=0) if b else np.zeros(len(q0))
    CabsK = np.abs(Cm) @ absK
    mag = np.sum(absK * CabsK, axis=0)
    r["amax"], r["mag"] = amax, mag
    r["fb"] = EPS * (np.abs(alpha) @ ((b + 8 + 6 * absA) * absK))
    r["s2b"] = (2 * b + 16 + 2 * amax) * EPS * (mag + SF + S20)
    r["s2_worst"] = EPS * ((b + 8) * mag + 6 * np.sum(absA * absK * CabsK, axis=0) + 2 * (SF + S20))
    r["confb"] = 100.0 / (SF + S20) * r["s2b"] + 400 * EPS
    return r


def sigma2_tolerance(r):
    """the sigma^2 bound for a kernel that returns sigma = sqrt(s2) and is compared as sigma^2 (module docstring)"""
    return r["s2b"] + 4 * EPS * np.maximum(np.asarray(r["s2"], dtype=np.float64), 0.0)


@functools.lru_cache(maxsize=None)
def ragged_reference(capacity, ny, l_sq, dtype=LD):
    """evaluate() for every patch of the batch on its own queries ([None] for a patch without points); built once per dtype"""
    B = batch(capacity, ny, l_sq)
    out = []
    for i in range(B["P"]):
        sl = slice(B["off"][i], B["off"][i + 1])
        out.append(evaluate(B, i, B["q0"][sl], B["q1"][sl], B["yq"][:, sl], dtype=dtype) if sl.stop > sl.start else None)
    return out


@functools.lru_cache(maxsize=None)
def train_reference(capacity, l_sq, dtype=LD):
    """train_sigmaf_np (step = float32(1e-4), max_counter = 3) for every patch of the ny = 1 batch on its own queries:
    [(p0, iters, ls, delta)]"""
    B = batch(capacity, 1, l_sq)
    out = []
    for i in range(B["P"]):
        sl = slice(B["off"][i], B["off"][i + 1])
        alpha, Cm, BV = patch_state(B, i)
        out.append(train_sigmaf_np(SF, l_sq, S20, alpha[0], Cm, BV, B["q0"][sl], B["q1"][sl], B["yq"][0, sl], TRAIN_STEP, TRAIN_MAXC,
                                   dtype=dtype))
    return out


def train_errors(got, ref):
    """error / bound of (p0, ls, delta) against a train_sigmaf_np result, at the bounds of test_sparse_train_sigmaf"""
    p0, ls, delta = got
    pr, ir, lr, dr = ref
    f = lambda a: np.asarray(a, dtype=LD)
    e = [float(abs(f(p0) - pr) / (1e-9 * abs(pr)))]
    if ir:
        e.append(float(np.max(np.abs(f(ls) - lr)) / (1e-7 * np.max(np.abs(lr)) + 1e-9)))
        e.append(float(np.max(np.abs(f(delta) - dr)) / (1e-8 * np.max(np.abs(dr)) + 1e-12)))
    return max(e)


def drop_row_of_C(r, ny):
    """l and dX of the patch with row j of C zeroed, for every j at once: (b, m, 3), (b, m).  Zeroing the row takes v_j = (C k)_j out of
    k^T C k and out of sigma_dx = 2 k_dx^T v; everything else in the closed form is unchanged."""
    K, CK, Kdx = (np.asarray(r[k], dtype=np.float64) for k in ("K", "CK", "Kdx"))
    sigma = np.asarray(r["sigma"], dtype=np.float64)[None, :] - K * CK
    sdx = np.asarray(r["sdx"], dtype=np.float64)[None, :, :] - 2.0 * Kdx * CK[:, :, None]
    return likelihood_tail(ny, sigma, sdx, np.asarray(r["second"], dtype=np.float64), np.asarray(r["offs"], dtype=np.float64),
                           np.asarray(r["sq"], dtype=np.float64))
