"""Inputs of the reprojection tests at the batch sizes where the loops of reproject.hip wrap (test_reproject_gpu.py, the tail of the sharded
flow in test_collective_gpu.py) and the oracle's cloud for them, shared with test_reproject_cases_cpu.py so that the cases can be checked
for what they claim without a GPU.

The reference of every comparison is the CPU oracle called per point (orc_reproject, orc_flatten_colors); all comparisons are exact."""
import ctypes as C

import numpy as np

from gp_compressor_amd.capi import Context

POINT_DTYPE = Context.POINT_DTYPE
RES = 0.15
SCAN_THREADS = 1024             # RP_SCAN_THREADS of reproject.hip: thread t of the scan holds patches [t * per, (t + 1) * per)

# batch sizes of the compaction tests: the last size with one patch per scan thread, the first with two, and either side of three
COMPACTION_P = (1023, 1024, 1025, 2047, 2049)
COMPACTION_M = 4
PATTERNS = ("all", "random", "first_only", "last_only", "head_empty", "tail_empty", "period2", "period3", "none")
ROW_M = (255, 256, 257, 513)    # either side of one pass of the emit kernel's 256-thread loop over q, and past two passes
ROW_P = 3

# the clamp's corner cases of test_reproject_bit_exact: NaN / inf -> 255, negative -> 0, > 255 -> 255, > 32767 wraps as short, out of int
# range -> 0 ...
SPECIALS_BASE = [np.nan, np.inf, -np.inf, -1e-9, -0.9999, 255.0, 255.9999, 256.0, 32767.9, 32768.0, 40000.0, 65535.5, 65536.0, 65791.0,
                 1e9, 3e9, -3e9, 1e300, -1e300, 0.0, 127.5]
# ... and the edges of the int and short conversions that rp_flatten spells out: the last double that truncates into int and the first that
# does not, on both sides (INT_MIN's low 16 bits are 0); -32768.5 truncates to the most negative short (-> 0), -32769 wraps to +32767
# (-> 255), -65536 wraps to 0
SPECIALS_EDGES = [2147483647.5, 2147483648.0, -2147483648.0, -2147483649.0, -32768.5, -32769.0, -65536.0]
SPECIALS = SPECIALS_BASE + SPECIALS_EDGES
# the byte each special flattens to, by the arithmetic above (checked against the oracle in test_reproject_cases_cpu.py)
SPECIAL_BYTES = [255, 255, 255, 0, 0, 255, 255, 255, 255, 0, 0, 0, 0, 255,
                 0, 0, 0, 0, 0, 0, 127,
                 0, 0, 0, 0, 0, 255, 0]
# specials whose outcome is a wrapped short: the int fits, its low 16 bits read as a short are another number
WRAPPED_SHORT = (32768.0, 40000.0, 65535.5, 65536.0, 65791.0, 1e9, -32769.0, -65536.0)
# specials outside int: the conversion yields INT_MIN, whose low 16 bits are zero
INT_OVERFLOW = (3e9, -3e9, 1e300, -1e300, 2147483648.0, -2147483649.0)


def per_of(P):
    """patches per thread of reproject_scan_kernel"""
    return (P + SCAN_THREADS - 1) // SCAN_THREADS


def rotate_of(P):
    """Where the compaction test of P patches starts in the list of specials: a pattern with one trained patch holds twelve of them at
    m = 4, and the five sizes between them run the whole list."""
    return 12 * COMPACTION_P.index(P) if P in COMPACTION_P else 0


def compaction_case(P, name, seed=7):
    """bv and the inputs of the compaction test of P patches under the pattern `name`"""
    bv = bv_pattern(name, P, seed)
    return bv, inputs(P, COMPACTION_M, seed, True, bv, rotate_of(P))


def bv_pattern(name, P, seed):
    """bv_count (P,) int32 of a trained / untrained pattern, or None for `all` (the entry then takes every patch as trained).  Trained entries
    are 1, 5 or 200: the kernel counts the non-zero entries, it does not add them.  No definition refers to how the scan splits P."""
    if name == "all":
        return None
    rng = np.random.default_rng([seed, P])
    on = np.zeros(P, dtype=bool)
    if name == "random":
        on = rng.integers(0, 3, P) != 0
    elif name == "first_only":
        on[0] = True
    elif name == "last_only":
        on[P - 1] = True
    elif name == "head_empty":
        on[int(np.ceil(0.6 * P)):] = True
    elif name == "tail_empty":
        on[:P - int(np.ceil(0.6 * P))] = True
    elif name == "period2":
        on[0::2] = True
    elif name == "period3":
        on[0::3] = True
    elif name != "none":
        raise ValueError(name)
    return np.where(on, rng.choice(np.array([1, 5, 200]), P), 0).astype(np.int32)


def trained(P, bv):
    return np.arange(P) if bv is None else np.flatnonzero(bv)


def special_patches(P, bv):
    """The patches that take the clamp specials: a trained one among the first ten (the first trained one if there is none), the trained
    one nearest P / 2 and the last trained one -- so the clamp is exercised wherever the compaction puts a patch.  Where two of them
    coincide the trained patches next nearest P / 2 step in; fewer than three only when fewer are trained."""
    t = trained(P, bv)
    if len(t) == 0:
        return []
    head = t[t < 10]
    mid = t[np.argsort(np.abs(t - P // 2), kind="stable")]
    picks = {int(head[-1]) if len(head) else int(t[0]), int(mid[0]), int(t[-1])}
    for p in mid:
        if len(picks) == 3:
            break
        picks.add(int(p))
    return sorted(picks)


def special_sites(P, m, bv, rotate=0):
    """(patch, channel, q, value) of every special that is planted: the list, started at `rotate`, dealt round-robin over special_patches,
    each patch filling its 3 m colour slots from the front.  Three patches of m = 4 hold all 28; a single trained patch of m = 4 holds the
    twelve from `rotate` on (the compaction tests rotate with the batch size, so every special is run under those patterns too)."""
    pts = special_patches(P, bv)
    sites, used = [], {p: 0 for p in pts}
    for k in range(len(SPECIALS)):
        if not pts:
            break
        p = pts[k % len(pts)]
        if used[p] >= 3 * m:
            continue
        c, q = divmod(used[p], m)
        used[p] += 1
        sites.append((p, c, q, SPECIALS[(k + rotate) % len(SPECIALS)]))
    return sites


def inputs(P, m, seed, colours=True, bv=None, rotate=0):
    """xs0, xs1 (m,): arbitrary points in +-RES / 2, not a grid; f (P, m); R (P, 9): a random orthonormal frame per patch, column-major;
    mu (P, 3) in +-50, so that the float cast rounds; cs (P, 3, m) and cm (P, 3), or None, None.  The clamp specials are written into
    cs + cm at special_sites(P, m, bv, rotate); the colour means of those patches are multiples of 0.5, so that (special - cm) + cm is the
    special itself at every edge of a conversion."""
    rng = np.random.default_rng([seed, P, m])
    xs0, xs1 = rng.uniform(-RES / 2, RES / 2, m), rng.uniform(-RES / 2, RES / 2, m)
    f = rng.normal(0, 0.01, (P, m))
    Q, _ = np.linalg.qr(rng.normal(size=(P, 3, 3)))
    R = np.ascontiguousarray(np.swapaxes(Q, 1, 2).reshape(P, 9))      # column-major storage of Q: columns = normal, u, v
    mu = rng.uniform(-50, 50, (P, 3))
    if not colours:
        return xs0, xs1, f, R, mu, None, None
    cs = rng.normal(0, 90, (P, 3, m))
    cm = rng.uniform(0, 255, (P, 3))
    for p in special_patches(P, bv):
        cm[p] = rng.integers(0, 511, 3) * 0.5
    for p, c, q, v in special_sites(P, m, bv, rotate):
        cs[p, c, q] = v - cm[p, c] if np.isfinite(v) else v
    return xs0, xs1, f, R, mu, cs, cm


NON_FINITE = (np.nan, np.inf, -np.inf, 1e300)       # 1e300 times a frame entry is a finite double that overflows the float cast


def non_finite_rows(f, rows):
    """A copy of f with two of NaN, +inf, -inf, 1e300 in each of the given rows (four rows or more use all four): what a patch with status
    GPC_STATUS_NOT_SPD hands the kernel in the dense flow, which has no bv_count."""
    g = f.copy()
    m = f.shape[1]
    assert m >= 3
    for k, r in enumerate(rows):
        g[r, k % m] = NON_FINITE[k % 4]
        g[r, (k + 2) % m] = NON_FINITE[(k + 1) % 4]
    return g


def expected(oracle, xs0, xs1, f, R, mu, cs, cm, bv):
    """The cloud the reference's patch loop gives: orc_reproject and orc_flatten_colors per point, untrained patches skipped, as full
    32-byte records (w = 1, a = 255, pad = 0, rgb = 0 without colours)."""
    L = oracle.lib()
    P, m = f.shape
    xyz_all, rgb_all = [], []
    xyz = (C.c_float * 3)()
    rgb = (C.c_uint8 * 3)()
    for i in trained(P, bv):
        Ri, mi = oracle._dp(np.ascontiguousarray(R[i])), oracle._dp(np.ascontiguousarray(mu[i]))
        for q in range(m):
            L.orc_reproject(Ri, mi, float(f[i, q]), float(xs0[q]), float(xs1[q]), xyz)
            xyz_all.append((xyz[0], xyz[1], xyz[2]))
            if cs is not None:
                c3 = np.ascontiguousarray(cs[i, :, q] + cm[i])
                L.orc_flatten_colors(oracle._dp(c3), rgb)
                rgb_all.append((rgb[0], rgb[1], rgb[2]))
    out = np.zeros(len(xyz_all), dtype=POINT_DTYPE)
    assert len(out) == m * len(trained(P, bv))
    if len(out):
        xyz_a = np.array(xyz_all, dtype=np.float32)         # (the c_float values come back as Python floats: exact in float32)
        out["x"], out["y"], out["z"] = xyz_a[:, 0], xyz_a[:, 1], xyz_a[:, 2]
        if cs is not None:
            rgb_a = np.array(rgb_all, dtype=np.uint8)
            out["r"], out["g"], out["b"] = rgb_a[:, 0], rgb_a[:, 1], rgb_a[:, 2]
    out["w"], out["a"] = 1.0, 255
    return out


def f_of_records(f, bv):
    """f of every record of the cloud, in record order"""
    return f[trained(f.shape[0], bv)].reshape(-1)


def assert_same_cloud(got, want, f_rec=None):
    """got == want, by bits -- except xyz of the records whose f was NaN (f_rec: f per record), which are NaN in both: the payload of a
    propagated NaN is not something x86 and the GPU owe each other."""
    assert got.dtype == want.dtype == POINT_DTYPE and got.shape == want.shape, (got.shape, want.shape)
    if f_rec is None or not np.any(np.isnan(f_rec)):
        assert got.tobytes() == want.tobytes(), _first_difference(got, want)
        return
    nan = np.isnan(f_rec)
    assert got[~nan].tobytes() == want[~nan].tobytes(), _first_difference(got[~nan], want[~nan])
    g, w = got[nan].copy(), want[nan].copy()
    for k in ("x", "y", "z"):
        assert np.all(np.isnan(g[k])) and np.all(np.isnan(w[k])), k
        g[k] = w[k] = 0.0
    assert g.tobytes() == w.tobytes(), _first_difference(g, w)


def _first_difference(got, want):
    a, b = got.view(np.uint8).reshape(-1, 32), want.view(np.uint8).reshape(-1, 32)
    bad = np.flatnonzero(np.any(a != b, axis=1))
    if len(bad) == 0:
        return "no difference"
    return "%d of %d records differ, first at %d: got %s, want %s" % (len(bad), len(a), bad[0], got[bad[0]], want[bad[0]])
