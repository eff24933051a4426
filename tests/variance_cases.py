"""Inputs of the dense predictive-variance tests (test_dense_variance_gpu.py) and an extended-precision restatement of what they
compute, shared with test_variance_cases_cpu.py so that the batches and the oracle they are compared with can be checked without a GPU.

Every batch is drawn as _mixed_batch draws it (points uniform in the patch window, a smooth surface plus noise, zero mean per patch);
X* is a set of points, not the patch grid: uniform in a window slightly larger than the patch, so some lie outside the data."""
import numpy as np

# hyper-parameter regimes: (sigma_f^2, l^2, sigma_n^2); DEFAULT is gaussian_process.h's (0.05, 3, 0.04, each squared)
DEFAULT = (0.05 * 0.05, 3.0 * 3.0, 0.04 * 0.04)
SHORT = (0.5, 0.05 ** 2, 1e-3)              # table-driven exponential everywhere
MEDIUM = (0.5, 0.5 ** 2, 1e-3)              # polynomial Gram tiles, table-driven K*
ZERO_NOISE = (1.0, 0.003 ** 2, 0.0)         # l = 3 mm against a ~ 8 mm point spacing: SPD without a noise term unless a point repeats

# test 1: every tile count at which the super-row solve of dense_variance_big_kernel changes its shape (nt = 1, 2, 16 | 17: rI = 1 | 18,
# 32 | 33, 34, 48 | 49, 63, 64), patches of <= 16 tiles inside a slot of 64 tile columns, empty patches
TILE_SIZES = [1024, 0, 1, 16, 17, 255, 256, 257, 272, 273, 400, 511, 512, 513, 528, 529, 767, 768, 769, 784, 1008, 1009, 1023, 1024, 0, 300]

# test 3: more patches than any CDNA part has compute units
MANY_P = 600
MANY_EMPTY = (7, 263, 519, 599)
MANY_DUP = (5, 300, 590)                    # 300 points each, point 280 repeats point 11: the failing pivot is in the second super-row
MANY_DUP_AT = (280, 11)


def _mixed_batch(sizes, seed, res=0.15):
    """A batch with exactly the given point counts (zeros allowed), surfaces as synth.make_patches draws them."""
    rng = np.random.default_rng(seed)
    off = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int32)
    N = int(off[-1])
    x0, x1 = rng.uniform(-res / 2, res / 2, N), rng.uniform(-res / 2, res / 2, N)
    y = np.zeros((1, N))
    for i, n in enumerate(sizes):
        sl = slice(off[i], off[i + 1])
        d = 0.01 * np.sin(rng.uniform(5, 30) * x0[sl] + rng.uniform(0, 6)) * np.cos(rng.uniform(5, 30) * x1[sl]) + rng.normal(0, 0.003, n)
        y[0, sl] = d - (d.mean() if n else 0.0)
    return off, x0, x1, y


def with_planes(off, x0, x1, y, ny, seed):
    """The batch with ny target planes: further surfaces over the same points, drawn as _mixed_batch draws the first."""
    rng = np.random.default_rng(seed)
    planes = [y[0]]
    for _ in range(1, ny):
        p = np.zeros_like(y[0])
        for i in range(len(off) - 1):
            sl = slice(off[i], off[i + 1])
            n = int(off[i + 1] - off[i])
            d = 0.01 * np.sin(rng.uniform(5, 30) * x0[sl] + rng.uniform(0, 6)) * np.cos(rng.uniform(5, 30) * x1[sl]) + rng.normal(0, 0.003, n)
            p[sl] = d - (d.mean() if n else 0.0)
        planes.append(p)
    return off, x0, x1, np.stack(planes, 0)


def xstar(m, seed):
    """m prediction points, uniform in [-0.09, 0.09]^2: not a grid, and a fifth of them outside the 0.15 patch window."""
    rng = np.random.default_rng(seed)
    return rng.uniform(-0.09, 0.09, m), rng.uniform(-0.09, 0.09, m)


def take_patches(off, x0, x1, y, idx):
    """The sub-batch of patches idx (in that order) and the indices of its points in the full batch."""
    cnt = np.diff(off)[idx]
    sub = np.concatenate([[0], np.cumsum(cnt)]).astype(np.int32)
    pts = np.concatenate([np.arange(off[i], off[i + 1]) for i in idx] + [np.zeros(0, dtype=np.int64)]).astype(np.int64)
    return (sub, np.ascontiguousarray(x0[pts]), np.ascontiguousarray(x1[pts]), np.ascontiguousarray(y[:, pts])), pts


def tile_batch(ny):
    off, x0, x1, y = _mixed_batch(TILE_SIZES, seed=41)
    return with_planes(off, x0, x1, y, ny, seed=42)


def many_sizes():
    rng = np.random.default_rng(23)
    sizes = rng.integers(1, 337, MANY_P)
    sizes[0] = 336
    sizes[list(MANY_EMPTY)] = 0
    sizes[list(MANY_DUP)] = 300
    return [int(s) for s in sizes]


def many_batch():
    """Test 3's batch: 600 patches of 1 .. 336 points; under ZERO_NOISE the patches MANY_DUP are singular, under DEFAULT they are not."""
    off, x0, x1, y = _mixed_batch(many_sizes(), seed=24)
    a, b = MANY_DUP_AT
    for i in MANY_DUP:
        x0[off[i] + a], x1[off[i] + a] = x0[off[i] + b], x1[off[i] + b]
    return off, x0, x1, y


def edge_sizes(n_max):
    """Sizes on and next to every tile edge up to n_max, with an empty and a single-point patch: 0, 1, 15, 16, 17, ..., n_max - 1, n_max."""
    s = {0, 1}
    for k in range(16, n_max + 1, 16):
        s.update((k - 1, k, k + 1))
    return sorted(v for v in s if v <= n_max)


def edge_batch(n_max, dup=False):
    """Test 4's batch for the register kernel's template of n_max points; dup: in the middle patch the third point from the end repeats
    point 2 (the failing pivot is in the patch's last tile column).  Returns the batch and the index of that patch."""
    sizes = edge_sizes(n_max)
    off, x0, x1, y = _mixed_batch(sizes, seed=50 + n_max)
    mid = len(sizes) // 2
    if dup:
        n = sizes[mid]
        x0[off[mid] + n - 3], x1[off[mid] + n - 3] = x0[off[mid] + 2], x1[off[mid] + 2]
    return (off, x0, x1, y), mid


def chunk_sizes(P):
    """Test 6: four groups of P / 4 patches, one per export layout of the variance path: 40 .. 190 points (register kernel), 200 .. 256
    (one-wave kernel's slots), 257 .. 300 (tiled slots), and 100 .. 330 mixed."""
    rng = np.random.default_rng(61)
    q = P // 4
    return [int(s) for s in np.concatenate([rng.integers(40, 191, q), rng.integers(200, 257, q), rng.integers(257, 301, q),
                                            rng.integers(100, 331, P - 3 * q)])]


def chunk_batch(P):
    return _mixed_batch(chunk_sizes(P), seed=62)


def hp_fit_predict(regime, x0, x1, y, xs0, xs1, double_noise=1):
    """Fit, predictive mean and variance of one patch in np.longdouble (80-bit on x86): a right-looking Cholesky of K + (1 + double_noise)
    sn^2 I that carries K* and y along (so that they leave as L^-1 K* and L^-1 y), v = sf^2 - |L^-1 k*|^2 per column, the back-substitution
    alpha = L^-T (L^-1 y), and f* = K*^T alpha.  The constant of the exponent is float32(-0.5) / l^2 evaluated in double, as in the kernels
    and the oracle.  y: (ny, n).  Returns status (0 | 1: a pivot is not positive), f* (ny, m), v (m,), alpha (ny, n), all longdouble."""
    LD = np.longdouble
    sf, l_sq, sn = regime
    n, m, ny = len(x0), len(xs0), y.shape[0]
    c = LD(float(np.float32(-0.5)) / l_sq)
    p0, p1, q0, q1 = x0.astype(LD), x1.astype(LD), xs0.astype(LD), xs1.astype(LD)
    d0, d1 = p0[:, None] - p0[None, :], p1[:, None] - p1[None, :]
    A = LD(sf) * np.exp(c * (d0 * d0 + d1 * d1))
    A[np.diag_indices(n)] += LD(sn) * (1 + int(bool(double_noise)))
    e0, e1 = p0[:, None] - q0[None, :], p1[:, None] - q1[None, :]
    Ks = LD(sf) * np.exp(c * (e0 * e0 + e1 * e1))               # (n, m)
    B = np.concatenate([Ks, y.astype(LD).T], axis=1)            # (n, m + ny)
    for j in range(n):
        d = A[j, j]
        if not d > 0:
            nan = np.full((ny, m), np.nan, dtype=LD)
            return 1, nan, np.full(m, np.nan, dtype=LD), np.full((ny, n), np.nan, dtype=LD)
        r = np.sqrt(d)
        A[j, j] = r
        col = A[j + 1:, j] / r
        A[j + 1:, j] = col
        B[j] /= r
        A[j + 1:, j + 1:] -= col[:, None] * col[None, :]
        B[j + 1:] -= col[:, None] * B[j][None, :]
    v = LD(sf) - np.sum(B[:, :m] * B[:, :m], axis=0)
    al = B[:, m:].copy()                                        # z = L^-1 y, (n, ny)
    for i in range(n - 1, -1, -1):
        al[i] = (al[i] - A[i + 1:, i] @ al[i + 1:]) / A[i, i]
    return 0, (Ks.T @ al).T, v, al.T
