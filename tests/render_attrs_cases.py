"""Case builders, restatements and bounds of the scattered sparse read-out (gpc_sparse_predict_scattered) and of the render attributes
(gpc_patches_render_attrs).  Test infrastructure (tests/test_render_attrs_cpu.py, tests/test_sparse_scatter_gpu.py,
tests/test_render_attrs_gpu.py); importable without a GPU.

Scattered read-out
------------------
bucket() is the host statement of what the device does: key = patch id, or P for a skipped entry; a STABLE argsort; off from the counts.
scatter_pattern() draws the patch-id patterns of the GPU test, scattered_reference() evaluates every entry under its own patch with
readout_cases.evaluate (np.longdouble) through that bucketing.

Normal at a hit
---------------
With L = leaf, q = (local[1], local[2]), k_j = sf exp(a_j), a_j = c |q - BV_j|^2:
    g_d = sum_j alpha_j k_j (BV_jd - q_d) / l^2  (d = 0, 1: the kernel's fx, fy),  v = (1, -g_0, -g_1),  w = R v,  normal = w / |w|,
negated when it faces away from the origin.  normal_ref() evaluates this in np.longdouble, or in float64 in the kernel's association
(sequential sums, w_a = (R[a, 0] + R[a, 1] v1) + R[a, 2] v2, len = sqrt((w0 w0 + w1 w1) + w2 w2)).

Bounds (EPS = 2^-52, every rounding counted as one EPS as in readout_cases; derived from the operations, none from a result)
    gradient  |g_d - ref| <= gb_d = EPS sum_j (b + 10 + 6 |a_j|) |alpha_j| |k_j| |BV_jd - q_d| / l^2
                  per term: the factor k_j (6 |a_j| + 4, readout_cases), the b-term sum (b), the difference BV_jd - q_d, its product
                  with alpha_j k_j, the division by l^2 (3), three EPS spare.
    normal    per world component <= nb = 2 (gb_0 + gb_1) + 16 EPS
                  R is orthonormal, so |delta w| <= |delta v| <= gb_0 + gb_1 plus the five roundings of the three-term sum on
                  components <= |w|; |w| >= 1 (v_0 = 1), and normalising a vector of length >= 1 does not expand an error: the
                  projection orthogonal to w / |w| divided by |w|.  The factor 2 and the 16 EPS cover the sum's roundings, the square
                  root, the quotient and the second-order term.
The orientation is the one decision: where |n_ref . e| <= 1e-6 |e| (e = origin - x) the sign is not compared, and at most 1 % of a
pose's hits may be excused so (tests/test_render_attrs_cpu.py shows the poses meet that for the restatement alone).
"""
import numpy as np

import raycast_cases as rcs
import readout_cases as RC
import render_cases as rc
import render_ref as rn

LD = np.longdouble
EPS = RC.EPS
PATTERNS = ("uniform", "one_patch", "descending", "gaps", "chunks", "sprinkled", "all_skipped")
COUNTS = (0, 1, 63, 64, 65, 255, 256, 257)
BIG_COUNT = 100_003                       # the sort's multi-workgroup path; odd, no multiple of a tile
OBJECTS = [(100, 1, RC.L8), (100, 3, RC.L5), (-1, 1, RC.L8)]
OBJECT_IDS = ["cap100-ny1", "cap100-ny3", "cap-1-ny1"]


# ---- scattered read-out ----------------------------------------------------------------------------------------------------------
def bucket(patch, P):
    """order (n,): entry indices in bucket order, the skipped ones last; off (P + 1,) int32; the number of valid entries"""
    patch = np.asarray(patch, dtype=np.int64)
    valid = (patch >= 0) & (patch < P)
    key = np.where(valid, patch, P)
    order = np.argsort(key, kind="stable")
    off = np.concatenate([[0], np.cumsum(np.bincount(key[valid], minlength=P)[:P])]).astype(np.int32)
    return order, off, int(valid.sum())


def scatter_pattern(name, B, n, seed):
    """patch (n,) int32, q0, q1 (n,) in the +-RES/2 window for pattern `name` on batch B.  "chunks" fixes its own n: per-patch counts of
    exactly 31, 32 and 33 on patches of the regular kernel (its sigma path works in chunks of SP_PC = 32) and 32, 33 on a 16- and a
    32-vector patch, in shuffled order."""
    rng = np.random.default_rng(seed)
    P, b = B["P"], B["b"]
    skipped = np.array([-1, P, 2 ** 31 - 1])
    if name == "uniform":
        patch = rng.integers(0, P, n)
    elif name == "one_patch":
        patch = np.full(n, int(np.argmax(b)))
    elif name == "descending":
        patch = np.sort(rng.integers(0, P, n))[::-1]
    elif name == "gaps":
        patch = rng.choice(np.arange(0, P, 2), n)
    elif name == "chunks":
        big = [int(i) for i in np.flatnonzero(b > 32)]
        pick = [big[0], big[len(big) // 2], big[-1], int(np.flatnonzero((b > 0) & (b <= 16))[-1]), int(np.flatnonzero((b > 16) & (b <= 32))[-1])]
        patch = rng.permutation(np.repeat(pick, [31, 32, 33, 32, 33]))
    elif name == "sprinkled":
        patch = np.where(rng.random(n) < 0.25, rng.choice(skipped, n), rng.integers(0, P, n))
    elif name == "all_skipped":
        patch = rng.choice(skipped, n)
    else:
        raise KeyError(name)
    n = len(patch)
    return patch.astype(np.int32), rng.uniform(-RC.RES / 2, RC.RES / 2, n), rng.uniform(-RC.RES / 2, RC.RES / 2, n)


def scattered_reference(B, patch, q0, q1, dtype=LD):
    """bucket() followed by readout_cases.evaluate per patch, scattered back: f (ny, n), s2 (n,) in `dtype` and the bounds fb (ny, n),
    s2tol (n,) = sigma2_tolerance; NaN at the skipped entries"""
    n, ny = len(patch), B["ny"]
    order, off, _ = bucket(patch, B["P"])
    dt = dtype or np.float64
    f, s2 = np.full((ny, n), np.nan, dtype=dt), np.full(n, np.nan, dtype=dt)
    fb, tol = np.full((ny, n), np.nan), np.full(n, np.nan)
    for p in range(B["P"]):
        idx = order[off[p]:off[p + 1]]
        if len(idx):
            r = RC.evaluate(B, p, q0[idx], q1[idx], dtype=dtype)
            f[:, idx], s2[idx], fb[:, idx], tol[idx] = r["f"], r["s2"], r["fb"], RC.sigma2_tolerance(r)
    return dict(f=f, s2=s2, fb=fb, s2tol=tol)


def entrywise_reference(B, patch, q0, q1, dtype=LD):
    """the same, every entry evaluated on its own"""
    n, ny = len(patch), B["ny"]
    dt = dtype or np.float64
    f, s2 = np.full((ny, n), np.nan, dtype=dt), np.full(n, np.nan, dtype=dt)
    for i in range(n):
        if 0 <= patch[i] < B["P"]:
            r = RC.evaluate(B, int(patch[i]), q0[i:i + 1], q1[i:i + 1], dtype=dtype)
            f[:, i], s2[i] = r["f"][:, 0], r["s2"][0]
    return dict(f=f, s2=s2)


# ---- the render scene: the two-sheet model with handmade depth states of every basis size -------------------------------------------
RES, SZ = rcs.RES, rcs.SZ
L_SQ = (RES / 5) ** 2
KW_DEPTH = dict(sigmaf_sq=RC.SF, l_sq=L_SQ, noise=RC.S20, capacity=100)       # (sf, s20 as readout_cases.evaluate assumes them)
SIZES = (1, 16, 17, 32, 33, 64, 65, 100)
AMP = 0.01                                # the surfaces stay a centimetre from their planes: inside their voxels
PRM = dict(eps_rel=rn.EPS_REL_SCENES)
ORIENT_REL, ORIENT_CAP = 1e-6, 0.01


def depth_batch(P, sizes=None, seed=77):
    """handmade depth states in the style of readout_cases.state for P leaves of res 0.25: leaf L has sizes[L] basis vectors uniform in
    the window, C = -(K_BV + s20 I)^-1 symmetrised, alpha = AMP smooth_y(BV) (K_BV + s20 I)^-1.  A dict as readout_cases.batch returns
    (capacity 100, ld 112, ny 1; read-only)."""
    ld = RC.ld_of(100)
    b = np.array([SIZES[L % len(SIZES)] for L in range(P)] if sizes is None else sizes, dtype=np.int32)
    alpha, C, BV = np.zeros((P, 1, ld)), np.zeros((P, ld, ld)), np.zeros((P, ld, 2))
    for L in range(P):
        n = int(b[L])
        if n == 0:
            continue
        rng = np.random.default_rng(seed * 1000 + L)
        v = rng.uniform(-RES / 2, RES / 2, size=(n, 2))
        d2 = ((v[:, None, :] - v[None, :, :]) ** 2).sum(-1)
        Ci = np.linalg.inv(RC.SF * np.exp(-0.5 / L_SQ * d2) + RC.S20 * np.eye(n))
        Ci = 0.5 * (Ci + Ci.T)
        y = AMP * RC.smooth_y(1, v[:, 0] * (RC.RES / RES), v[:, 1] * (RC.RES / RES))
        alpha[L, :, :n], C[L, :n, :n], BV[L, :n] = y @ Ci, -Ci, v
    return RC._freeze(dict(capacity=100, ny=1, l_sq=L_SQ, P=P, ld=ld, b=b, alpha=alpha, C=C, BV=BV))


def gp_of_batch(B):
    """the batch as tests/render_ref.py reads a GP"""
    return dict(sf=RC.SF, l_sq=B["l_sq"], b=B["b"], alpha=B["alpha"], BV=B["BV"])


def pose_rays(pose, frames):
    """(origin, dirs) of a pose of render_cases.POSES: its 23 x 17 image, the 1 x 1 image and the hand-made rays"""
    return rc.scene_rays(pose, frames["R"][4][:, 1])


def gradient(B, L, q1, q2, dtype=LD):
    """(g_0, g_1) of leaf L at q and the bounds (gb_0, gb_1).  dtype None: float64, sequential sums in the kernel's order"""
    b = int(min(B["b"][L], B["ld"]))
    dt = dtype or np.float64
    al, bv = np.asarray(B["alpha"][L][0, :b], dtype=dt), np.asarray(B["BV"][L][:b], dtype=dt)
    q1, q2, lsq = dt(q1), dt(q2), dt(B["l_sq"])
    d0, d1 = q1 - bv[:, 0], q2 - bv[:, 1]
    if dtype is None:
        a = (rn.C_HALF / lsq) * (d0 * d0 + d1 * d1)
    else:
        a = dt(-0.5) / lsq * (d0 * d0 + d1 * d1)
    k = dt(RC.SF) * np.exp(a)
    w = al * k
    e0, e1 = bv[:, 0] - q1, bv[:, 1] - q2
    seq = (lambda t: np.cumsum(t)[-1] if b else dt(0)) if dtype is None else (lambda t: np.sum(t) if b else dt(0))
    g = (seq(w * e0) / lsq, seq(w * e1) / lsq)
    mag = (b + 10 + 6 * np.abs(np.asarray(a, dtype=np.float64))) * np.abs(np.asarray(w, dtype=np.float64))
    gb = tuple(float(EPS * np.sum(mag * np.abs(np.asarray(e, dtype=np.float64))) / B["l_sq"]) for e in (e0, e1))
    return g, gb


def normal_ref(B, frames, L, local, origin=None, dtype=LD):
    """dict(n (3,) the unit normal of leaf L at local = (f, q1, q2) in the world -- facing `origin` when one is given, else with the
    sign of the frame's first column --, fx, fy, nb the bound per component, ne = n_unoriented . e and e_len (None without an origin))"""
    dt = dtype or np.float64
    (fx, fy), (gb0, gb1) = gradient(B, L, local[1], local[2], dtype)
    R, mu = np.asarray(frames["R"][L], dtype=dt), np.asarray(frames["mean"][L], dtype=dt)
    v1, v2 = -fx, -fy
    w = np.array([(R[a, 0] + R[a, 1] * v1) + R[a, 2] * v2 for a in range(3)], dtype=dt)
    n = w / np.sqrt((w[0] * w[0] + w[1] * w[1]) + w[2] * w[2])
    out = dict(fx=fx, fy=fy, nb=2.0 * (gb0 + gb1) + 16 * EPS, ne=None, e_len=None)
    if origin is not None:
        f, q1, q2 = (dt(v) for v in local)
        x = np.array([((R[a, 0] * f + R[a, 1] * q1) + R[a, 2] * q2) + mu[a] for a in range(3)], dtype=dt)
        e = np.asarray(origin, dtype=dt) - x
        ne = (n[0] * e[0] + n[1] * e[1]) + n[2] * e[2]
        out.update(ne=ne, e_len=np.sqrt(np.sum(e * e)))
        if ne < 0:
            n = -n
    out["n"] = n
    return out


def excused(r):
    """the orientation of this hit is not compared: the reference's own n . e is within ORIENT_REL |e| of zero"""
    return bool(abs(r["ne"]) <= ORIENT_REL * r["e_len"])


def restate(frames, grid, B, pose):
    """render_ref.render of a pose on (frames, grid, B): origin, dirs, rays"""
    o, dirs = pose_rays(pose, frames)
    return o, dirs, rn.render(frames, grid, gp_of_batch(B), o, dirs, PRM)
