"""Inputs, extended-precision reference and gate of the dense mean's accuracy tests (test_dense_accuracy_gpu.py), shared with
test_dense_accuracy_cases_cpu.py so that everything the GPU test relies on can be checked without a GPU.

What test_dense_gpu.py's FTOL = 1e-9 and ATOL = 1e-8 mean, and what they do not: they bound the gap between a kernel and the float64
oracle relative to the BATCH's largest value, 300 to 10 000 times above what two honest float64 evaluations of these systems differ
by.  Here every route's f* and alpha are held, patch by patch, against the 80-bit restatement variance_cases.hp_fit_predict at

    gate = 8 * E64 + 32 * 2^-53

where E64 is the float64 oracle's own error against the same restatement on the same batch, measured on the CPU and recorded below
(E64; test_dense_accuracy_cases_cpu.py fails when a fresh measurement exceeds a record).  Factor 8: two float64 evaluations that differ
in summation order, FMA contraction and a <= 2 ulp exponential are equally far from the exact solve, and per-patch luck spreads E64 by
up to about 10 at one size (variance_cases' own measurements: 6.6e-14 .. 6.0e-13 at 17 .. 529 points), most of which the worst over a
batch removes.  The floor covers one- and two-point patches, where E64 can be 0.  Nothing in the gate comes from a GPU run.

Error measure, per patch: max|f - f_hp| / max|f_hp| over the patch (all planes), likewise alpha; an empty patch must be exactly 0, a
patch whose max|f_hp| is 0 is compared absolutely; a batch's error is the worst over its patches.

Two kinds of batches, all drawn by variance_cases._mixed_batch / with_planes:
  edge       one batch per route family (<= 256 points, <= 512, the tiled kernel) with the smallest sizes at which that family changes
             shape; the families are prefixes of one batch, so a patch's extended-precision solve is shared.  ny = 1 and 3, both noise
             conventions, the regimes DEFAULT, SHORT, MEDIUM.
  threshold  patches that put each exponential selector's bound just under and just over each of its thresholds, with the bound
             attained (see threshold_batch)."""
import fractions

import numpy as np

import variance_cases as VC

RES, SZ = 0.15, 12              # the grid entry's X*: oracle.grid(RES, SZ), 144 cells (nine MFMA output tiles' worth, none full)
M_PTS = 37                      # the point-wise entry's X*: variance_cases.xstar(M_PTS, XSTAR_SEED)
XSTAR_SEED = 307
GATE_FACTOR = 8.0
GATE_FLOOR = 32.0 * 2.0 ** -53
GATE_CAP = 1e-10                # a case whose gate would exceed this is too ill-conditioned to tell anything: replace the case

REGIMES = {"default": VC.DEFAULT, "short": VC.SHORT, "medium": VC.MEDIUM}

# ---------------------------------------------------------------------------------------------------------------------------
# edge batches
# ---------------------------------------------------------------------------------------------------------------------------
# <= 256: empty, one point, every side of the first tile edge, the 64 | 65 edge of the one-wave kernel's lane loop, 191 | 192 | 193 (the
# register-tile kernel's NT = 12 | 16 templates and the two-wave shape's lower end), 255 | 256, a few in between; the largest first
SIZES_256 = [256, 0, 1, 15, 16, 17, 40, 64, 65, 100, 128, 129, 191, 192, 193, 224, 255, 256, 0, 7]
# <= 512: the NT = 17 class (257 .. 272), the first size past it, the 512 instance's last tile
SIZES_512 = SIZES_256 + [257, 272, 273, 400, 511, 512]
# tiled kernel: one patch just past 512 and the one 1024-point patch (its 80-bit solve takes seconds: there is exactly one)
SIZES_TILED = SIZES_512 + [513, 1024]
FAMILIES = {"n256": len(SIZES_256), "n512": len(SIZES_512), "tiled": len(SIZES_TILED)}      # family -> number of leading patches
EDGE_SEED, EDGE_PLANE_SEED = 301, 302

# ---------------------------------------------------------------------------------------------------------------------------
# threshold batches
# ---------------------------------------------------------------------------------------------------------------------------
EXP_SMALL_MAX, EXP_TINY_MAX = 2.0 ** -5, 2.0 ** -8      # gpc_device.h GPC_EXP_SMALL_MAX (degree 7 below), GPC_EXP_TINY_MAX (degree 5 below)
SIDE = {"under": 1.0 - 2.0 ** -20, "over": 1.0 + 2.0 ** -20}
THR_SIZES = {"t256": [200, 256, 223, 241], "t512": [231, 300, 256]}     # the <= 256 kernels | one patch above 256 for the others
# (seed 312 drew a 300-point patch whose mean all but cancels over the grid: the oracle's own f* error there, 1.2e-11, put the gate at
# GATE_CAP.  Such a case tells nothing, so it was replaced; seeds 313 .. 315 all give 1e-12 .. 2e-12.)
THR_SEED = {"t256": 311, "t512": 313}
GRID_SHIFT = 0.4                # test_dense_mfma_exp_regimes' shift of the patch off the origin of its frame
# (selector, threshold, side).  2^-3 "under" is not a threshold of any kernel: it is where the degree-7 polynomial would be 1.5e-12 off
# if a selector let it through, as 2^-5 "under" is for degree 5 -- the table-driven exponential must be what runs there.
THR_SETTINGS = [(sel, thr, side) for sel in ("gram", "grid") for thr in (EXP_SMALL_MAX, EXP_TINY_MAX) for side in ("under", "over")] + \
               [("gram", 2.0 ** -3, "under"), ("grid", 2.0 ** -3, "under")]
# sigma_f^2 and sigma_n^2 of the threshold regimes (l^2 follows from the threshold).  A signal-to-noise ratio of 50, between DEFAULT's 1.6 and
# MEDIUM's 500: at these length scales (l = 0.4 .. 2.4 against a 0.15 window) MEDIUM's ratio makes f* = K*^T alpha cancel so far that the
# oracle's own f* error puts the gate above GATE_CAP, and under DEFAULT's a wrong polynomial moves f* by barely more than the gate.  With
# this one the CPU-only check of what the gate catches (degree 5 evaluated up to 2^-5, degree 7 up to 2^-3, in a float64 NumPy solve of
# these batches: test_dense_accuracy_cases_cpu.py) gives 3 .. 8 times the f* gate and 180 .. 220 times the alpha gate for a wrong Gram
# polynomial, 85 .. 165 times the f* gate for a wrong grid-factor polynomial, and every gate of these batches stays below 1.2e-11.
THR_SF, THR_SN = 0.05, 1e-3


def _fma(a, b, c):
    """round(a * b + c) with one rounding, as the kernels' __builtin_fma"""
    F = fractions.Fraction
    return float(F(a) * F(b) + F(c))


def selector_bounds_tile(x0, x1, res=RES):
    """The squared-distance bounds of dense_mfma.hip (small_gram / small_grid) and dense_mfma_big.hip for one patch, in their association:
    r = max-norm extent around the first point; Gram 8 r r, grid (res / 2 + max(|x_first|) + r)^2.  The selectors compare -c times these
    with 2^-5."""
    r = max(float(np.max(np.abs(x0 - x0[0]))), float(np.max(np.abs(x1 - x1[0]))))
    b = 0.5 * res + max(abs(float(x0[0])), abs(float(x1[0]))) + r
    return 8.0 * r * r, b * b


def selector_bounds_w1(x0, x1, res=RES):
    """The same for dense_mfma_w1.hip (mode_g / mode_p): the bounding box's squared diagonal fma(rx, rx, ry ry), and the square of
    res / 2 + the box's largest |coordinate|.  Compared with 2^-8 and 2^-5; mode_p is 0 whenever mode_g is."""
    mn0, mx0, mn1, mx1 = float(np.min(x0)), float(np.max(x0)), float(np.min(x1)), float(np.max(x1))
    rx, ry = mx0 - mn0, mx1 - mn1
    hb = 0.5 * res
    bq = max(hb + max(abs(mn0), abs(mx0)), hb + max(abs(mn1), abs(mx1)))
    return _fma(rx, rx, ry * ry), bq * bq


def c_exp(l_sq):
    """The constant of the exponent as host and oracle form it: (double)(-0.5f) / l_sq"""
    return float(np.float32(-0.5)) / l_sq


def modes_tile(x0, x1, l_sq):
    """(small_gram, small_grid) of the register-tile and the tiled kernel for one patch"""
    g, p = selector_bounds_tile(x0, x1)
    c = c_exp(l_sq)
    return -c * g <= EXP_SMALL_MAX, -c * p <= EXP_SMALL_MAX


def modes_w1(x0, x1, l_sq):
    """(mode_g, mode_p) of the one-wave kernel for one patch: 2 degree 5, 1 degree 7, 0 table-driven"""
    g, p = selector_bounds_w1(x0, x1)
    c = c_exp(l_sq)
    mode = lambda t: 2 if t <= EXP_TINY_MAX else 1 if t <= EXP_SMALL_MAX else 0
    mg = mode(-c * g)
    return mg, (mode(-c * p) if mg else 0)


def threshold_batch(sizeset, selector):
    """A batch whose patches all have the same bounding box: the first point at the centre of the window, the next two pinned at
    opposite corners.  Then the max-norm extent around the first point is half the window, and the register-tile kernel's 8 r^2 and the
    one-wave kernel's box diagonal are both the largest squared distance of the patch: the Gram bound is attained.  selector "grid": the
    patch is shifted off the origin of its frame, so that the grid factors' bound (the largest |coordinate| plus res / 2) is what crosses
    the threshold while the Gram bound stays below it.  ny = 1: the one-wave kernel takes the depth plane alone."""
    off, x0, x1, y = VC._mixed_batch(THR_SIZES[sizeset], seed=THR_SEED[sizeset])
    h = RES / 2
    for i in range(len(off) - 1):
        o = off[i]
        x0[o], x1[o] = 0.0, 0.0
        x0[o + 1], x1[o + 1] = -h, -h
        x0[o + 2], x1[o + 2] = h, h
    if selector == "grid":
        x0, x1 = x0 + GRID_SHIFT, x1 - GRID_SHIFT
    return off, x0, x1, y


def threshold_l_sq(sizeset, selector, thr, side):
    """l^2 at which -c * bound = thr * SIDE[side] for the batch's common bound (the first patch's, in the tile kernels' association; the
    other patches and the one-wave kernel's association differ from it by roundings, 2^-30 of the margin)."""
    off, x0, x1, _ = _full_batch((sizeset, selector))
    g, p = selector_bounds_tile(x0[:off[1]], x1[:off[1]])
    return 0.5 * (g if selector == "gram" else p) / (thr * SIDE[side])


def largest_true_argument(x0, x1, selector, sz=SZ):
    """The largest squared distance that really enters an exponential of one patch, in longdouble: over all pairs of points ("gram"), or
    along one axis between a point and a cell centre of the sz x sz grid ("grid")."""
    LD = np.longdouble
    p0, p1 = x0.astype(LD), x1.astype(LD)
    if selector == "gram":
        d0, d1 = p0[:, None] - p0[None, :], p1[:, None] - p1[None, :]
        return np.max(d0 * d0 + d1 * d1)
    g = LD(RES) * ((np.arange(sz).astype(LD) + LD(0.5)) / LD(sz) - LD(0.5))
    return max(np.max((p0[:, None] - g[None, :]) ** 2), np.max((p1[:, None] - g[None, :]) ** 2))


# ---------------------------------------------------------------------------------------------------------------------------
# cases: (kind, ...) tuples that name a batch, a regime and a noise convention
# ---------------------------------------------------------------------------------------------------------------------------
def edge_cases():
    return [("edge", fam, reg, dbl, ny) for fam in FAMILIES for reg in REGIMES for dbl in (1, 0) for ny in (1, 3)]


def threshold_cases():
    return [("thr", ss, sel, thr, side) for ss in THR_SIZES for (sel, thr, side) in THR_SETTINGS]


def case_id(case):
    if case[0] == "edge":
        return "edge-%s-%s-dbl%d-ny%d" % case[1:]
    return "thr-%s-%s-2^%d-%s" % (case[1], case[2], int(round(np.log2(case[3]))), case[4])


_BATCH, _HP, _XS, _ORACLE = {}, {}, {}, {}


def _frozen(*arrays):
    for a in arrays:
        a.setflags(write=False)
    return arrays


def xstars():
    """(grid xs0, xs1), (point-wise xs0, xs1); the grid is synth.grid's formula, equal to oracle.grid(RES, SZ) bit for bit"""
    if not _XS:
        g = RES * ((np.arange(SZ, dtype=np.float64) + 0.5) / SZ - 0.5)
        _XS["grid"] = _frozen(np.ascontiguousarray(np.tile(g, SZ)), np.ascontiguousarray(np.repeat(g, SZ)))
        _XS["pts"] = _frozen(*VC.xstar(M_PTS, seed=XSTAR_SEED))
    return _XS["grid"], _XS["pts"]


def _full_batch(key):
    """"edge": the tiled family's batch with three planes, of which every edge case's batch is a prefix; (sizeset, selector): that
    threshold batch.  Read-only, built once."""
    if key not in _BATCH:
        if key == "edge":
            b = VC.with_planes(*VC._mixed_batch(SIZES_TILED, seed=EDGE_SEED), ny=3, seed=EDGE_PLANE_SEED)
        else:
            b = threshold_batch(*key)
        _BATCH[key] = _frozen(*b)
    return _BATCH[key]


def case_inputs(case):
    """(off, x0, x1, y), regime, double_noise of a case; y has the case's ny planes.  Read-only arrays."""
    if case[0] == "edge":
        _, fam, reg, dbl, ny = case
        off, x0, x1, y = _full_batch("edge")
        P = FAMILIES[fam]
        N = int(off[P])
        return (off[:P + 1], x0[:N], x1[:N], _frozen(np.ascontiguousarray(y[:ny, :N]))[0]), REGIMES[reg], dbl
    _, ss, sel, thr, side = case
    return _full_batch((ss, sel)), (THR_SF, threshold_l_sq(ss, sel, thr, side), THR_SN), 1


def _both_xstars():
    (g0, g1), (q0, q1) = xstars()
    return np.concatenate([g0, q0]), np.concatenate([g1, q1])


def _hp_keys(case):
    """The (batch, patch, regime, noise convention) keys of a case's non-empty patches"""
    (off, _, _, _), regime, dbl = case_inputs(case)
    key = "edge" if case[0] == "edge" else (case[1], case[2])
    return [(key, i, regime, dbl) for i in range(len(off) - 1) if off[i + 1] > off[i]]


def _hp_solve(k):
    key, i, regime, dbl = k
    off, x0, x1, y = _full_batch(key)
    sl = slice(int(off[i]), int(off[i + 1]))
    st, f, _, al = VC.hp_fit_predict(regime, x0[sl], x1[sl], y[:, sl], *_both_xstars(), double_noise=dbl)
    assert st == 0, k
    return _frozen(f, al)


def prefetch(cases, workers=8):
    """Solve what reference() will ask for, the largest patches first, on a few threads (NumPy's longdouble loops release the GIL)"""
    import concurrent.futures
    todo = sorted({k for c in cases for k in _hp_keys(c) if k not in _HP}, key=lambda k: -int(np.diff(_full_batch(k[0])[0])[k[1]]))
    xstars()
    with concurrent.futures.ThreadPoolExecutor(workers) as ex:
        for k, r in zip(todo, ex.map(_hp_solve, todo)):
            _HP[k] = r


def reference(case):
    """The 80-bit fit of every patch of a case: f_grid (P, ny, SZ SZ), f_pts (P, ny, M_PTS), alpha (ny, N), longdouble.  One
    hp_fit_predict per (patch, regime, noise convention) and process: both X* sets go through as one, the planes ride along (the
    columns of a solve do not see each other), and the families share their patches."""
    (off, _, _, y), _, _ = case_inputs(case)
    P, ny, N, mg = len(off) - 1, y.shape[0], int(off[-1]), SZ * SZ
    f = np.zeros((P, ny, mg + M_PTS), dtype=np.longdouble)
    al = np.zeros((ny, N), dtype=np.longdouble)
    for k in _hp_keys(case):
        if k not in _HP:
            _HP[k] = _hp_solve(k)
        i = k[1]
        fi, ai = _HP[k]
        f[i], al[:, int(off[i]):int(off[i + 1])] = fi[:ny], ai[:ny]
    return f[:, :, :mg], f[:, :, mg:], al


def batch_error(got, want, off, per_point):
    """The error measure of this module.  per_point False: got, want (P, ny, m); True: (ny, N), cut by off.  Returns the batch's error
    and the index of the patch that sets it; an empty patch that is not exactly 0 gives inf."""
    worst, at = 0.0, -1
    for i in range(len(off) - 1):
        sl = slice(int(off[i]), int(off[i + 1]))
        g, w = (got[:, sl], want[:, sl]) if per_point else (got[i], want[i])
        if sl.start == sl.stop:
            e = 0.0 if (g.size == 0 or np.all(g == 0)) else np.inf
        else:
            scale = float(np.max(np.abs(w)))
            e = float(np.max(np.abs(g.astype(np.longdouble) - w))) / (scale if scale > 0 else 1.0)
            if not np.all(np.isfinite(g)):
                e = np.inf
        if e > worst:
            worst, at = e, i
    return worst, at


def errors(case, f_grid=None, f_pts=None, alpha=None):
    """Batch errors of whichever outputs are given against reference(case): dict name -> (error, patch)"""
    (off, _, _, _), _, _ = case_inputs(case)
    rg, rp, ra = reference(case)
    out = {}
    if f_grid is not None:
        out["f_grid"] = batch_error(f_grid, rg, off, False)
    if f_pts is not None:
        out["f_pts"] = batch_error(f_pts, rp, off, False)
    if alpha is not None:
        out["alpha"] = batch_error(alpha, ra, off, True)
    return out


def oracle_fit(oracle, case):
    """The float64 oracle on a case: f_grid, f_pts, alpha, status"""
    (off, _, _, y), regime, dbl = case_inputs(case)
    key = ("edge" if case[0] == "edge" else (case[1], case[2]), regime, dbl)
    if key not in _ORACLE:
        # one fit of the largest batch with all its planes and both X* sets: a patch does not see the other patches, a plane's solve
        # not the other planes, a prediction not the other X*
        p = oracle.dense_params(*regime, ref_double_noise=dbl)
        f, _, st, al = oracle.dense_fit_predict_batch(p, *_full_batch(key[0]), *_both_xstars(), want_alpha=True)
        _ORACLE[key] = _frozen(f, st, al)
    f, st, al = _ORACLE[key]
    P, ny, N, mg = len(off) - 1, y.shape[0], int(off[-1]), SZ * SZ
    return np.ascontiguousarray(f[:P, :ny, :mg]), np.ascontiguousarray(f[:P, :ny, mg:]), np.ascontiguousarray(al[:ny, :N]), st[:P]


def measure_e64(oracle, case):
    """(E64 of f* on the grid, of f* on the points, of alpha) for one case"""
    fg, fp, al, st = oracle_fit(oracle, case)
    assert np.all(st == 0), case
    e = errors(case, fg, fp, al)
    return e["f_grid"][0], e["f_pts"][0], e["alpha"][0]


def gate(e64):
    return GATE_FACTOR * e64 + GATE_FLOOR


def gates(case):
    """name -> gate of a case's three outputs, from the record"""
    fg, fp, al = E64[case_id(case)]
    return {"f_grid": gate(fg), "f_pts": gate(fp), "alpha": gate(al)}


# ---------------------------------------------------------------------------------------------------------------------------
# E64: the float64 oracle (oracle/gpc_oracle.c, -O2 -ffp-contract=off) against reference(), per case: (f* grid entry, f* point-wise entry,
# alpha).  Measured on the CPU by test_dense_accuracy_cases_cpu.py::test_recorded_e64_holds, which prints a fresh table and fails when
# a measurement exceeds its record; the figures are the measurements rounded up to three digits.
# ---------------------------------------------------------------------------------------------------------------------------
E64 = {
    "edge-n256-default-dbl1-ny1": (2.96e-12, 2.84e-12, 2.43e-15),
    "edge-n256-default-dbl1-ny3": (5.84e-13, 4.10e-13, 2.32e-15),
    "edge-n256-default-dbl0-ny1": (3.23e-12, 3.05e-12, 3.45e-15),
    "edge-n256-default-dbl0-ny3": (4.64e-13, 4.14e-13, 2.99e-15),
    "edge-n256-short-dbl1-ny1": (8.42e-13, 6.79e-13, 2.19e-13),
    "edge-n256-short-dbl1-ny3": (8.42e-13, 6.88e-13, 2.55e-13),
    "edge-n256-short-dbl0-ny1": (1.65e-12, 1.11e-12, 4.37e-13),
    "edge-n256-short-dbl0-ny3": (1.81e-12, 1.35e-12, 4.04e-13),
    "edge-n256-medium-dbl1-ny1": (4.69e-12, 2.91e-12, 2.19e-13),
    "edge-n256-medium-dbl1-ny3": (2.33e-12, 1.80e-12, 2.10e-13),
    "edge-n256-medium-dbl0-ny1": (4.30e-12, 3.19e-12, 4.29e-13),
    "edge-n256-medium-dbl0-ny3": (5.30e-12, 3.46e-12, 4.12e-13),
    "edge-n512-default-dbl1-ny1": (2.96e-12, 2.84e-12, 3.08e-15),
    "edge-n512-default-dbl1-ny3": (7.06e-13, 4.18e-13, 4.12e-15),
    "edge-n512-default-dbl0-ny1": (3.23e-12, 3.05e-12, 5.74e-15),
    "edge-n512-default-dbl0-ny3": (1.26e-12, 7.75e-13, 5.74e-15),
    "edge-n512-short-dbl1-ny1": (2.04e-12, 1.05e-12, 3.20e-13),
    "edge-n512-short-dbl1-ny3": (2.41e-12, 1.28e-12, 3.29e-13),
    "edge-n512-short-dbl0-ny1": (4.30e-12, 2.80e-12, 5.45e-13),
    "edge-n512-short-dbl0-ny3": (6.31e-12, 2.69e-12, 6.10e-13),
    "edge-n512-medium-dbl1-ny1": (6.20e-12, 4.15e-12, 3.07e-13),
    "edge-n512-medium-dbl1-ny3": (8.41e-12, 4.46e-12, 2.91e-13),
    "edge-n512-medium-dbl0-ny1": (1.08e-11, 4.87e-12, 5.17e-13),
    "edge-n512-medium-dbl0-ny3": (1.04e-11, 6.29e-12, 5.50e-13),
    "edge-tiled-default-dbl1-ny1": (2.96e-12, 2.84e-12, 3.43e-15),
    "edge-tiled-default-dbl1-ny3": (7.06e-13, 4.18e-13, 4.12e-15),
    "edge-tiled-default-dbl0-ny1": (3.23e-12, 3.05e-12, 5.74e-15),
    "edge-tiled-default-dbl0-ny3": (1.26e-12, 7.75e-13, 5.74e-15),
    "edge-tiled-short-dbl1-ny1": (3.24e-12, 1.53e-12, 4.36e-13),
    "edge-tiled-short-dbl1-ny3": (2.87e-12, 1.76e-12, 3.95e-13),
    "edge-tiled-short-dbl0-ny1": (5.45e-12, 4.00e-12, 7.26e-13),
    "edge-tiled-short-dbl0-ny3": (6.31e-12, 4.00e-12, 6.70e-13),
    "edge-tiled-medium-dbl1-ny1": (6.20e-12, 4.15e-12, 3.33e-13),
    "edge-tiled-medium-dbl1-ny3": (8.41e-12, 4.46e-12, 4.14e-13),
    "edge-tiled-medium-dbl0-ny1": (1.08e-11, 6.78e-12, 8.49e-13),
    "edge-tiled-medium-dbl0-ny3": (1.04e-11, 6.43e-12, 7.96e-13),
    "thr-t256-gram-2^-5-under": (7.04e-13, 3.26e-13, 3.92e-14),
    "thr-t256-gram-2^-5-over": (8.02e-13, 5.59e-13, 3.06e-14),
    "thr-t256-gram-2^-8-under": (6.96e-13, 8.31e-13, 2.42e-14),
    "thr-t256-gram-2^-8-over": (8.45e-13, 5.03e-13, 2.53e-14),
    "thr-t256-grid-2^-5-under": (9.28e-14, 9.85e-14, 2.43e-14),
    "thr-t256-grid-2^-5-over": (1.09e-13, 8.69e-14, 2.89e-14),
    "thr-t256-grid-2^-8-under": (3.29e-13, 2.52e-13, 3.46e-14),
    "thr-t256-grid-2^-8-over": (3.63e-13, 2.85e-13, 3.09e-14),
    "thr-t256-gram-2^-3-under": (3.79e-13, 3.43e-13, 2.62e-14),
    "thr-t256-grid-2^-3-under": (9.04e-14, 8.64e-14, 2.68e-14),
    "thr-t512-gram-2^-5-under": (1.04e-12, 7.07e-13, 3.78e-14),
    "thr-t512-gram-2^-5-over": (8.65e-13, 9.30e-13, 3.04e-14),
    "thr-t512-gram-2^-8-under": (1.39e-12, 1.22e-12, 3.16e-14),
    "thr-t512-gram-2^-8-over": (1.02e-12, 6.98e-13, 3.26e-14),
    "thr-t512-grid-2^-5-under": (1.60e-13, 1.32e-13, 4.30e-14),
    "thr-t512-grid-2^-5-over": (1.63e-13, 1.21e-13, 3.73e-14),
    "thr-t512-grid-2^-8-under": (5.42e-13, 4.07e-13, 3.38e-14),
    "thr-t512-grid-2^-8-over": (4.94e-13, 5.02e-13, 4.37e-14),
    "thr-t512-gram-2^-3-under": (4.23e-13, 4.05e-13, 3.11e-14),
    "thr-t512-grid-2^-3-under": (9.64e-14, 9.84e-14, 2.86e-14),
}
