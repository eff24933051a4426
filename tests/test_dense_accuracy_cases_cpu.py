"""What test_dense_accuracy_gpu.py relies on, checked without a GPU (dense_accuracy_cases.py): the recorded E64 still bounds a fresh
measurement of the float64 oracle against the 80-bit restatement, the size lists hold every tile edge, every threshold batch sits on
the intended side of the intended threshold with the bound attained, the oracle and the restatement find every case SPD, no gate exceeds
1e-10 -- and the gate has teeth: a float64 NumPy solve of the threshold batches whose exponential is the degree-5 polynomial at 2^-5 (or
the degree-7 one at 2^-3), in the Gram matrix or in the grid factors, which is what a wrong selector would run, exceeds it.

Measured E64, worst per kind of batch: f* 1.07e-11 (MEDIUM, single noise, <= 512 points), alpha 8.5e-13 (MEDIUM, single noise, 1024
points); under DEFAULT f* 3.2e-12 and alpha 5.7e-15; threshold batches f* 1.4e-12, alpha 4.4e-14.  The largest gate is 8.6e-11."""
import math

import numpy as np
import pytest

import dense_accuracy_cases as DA

ALL_CASES = DA.edge_cases() + DA.threshold_cases()


@pytest.fixture(scope="module")
def measured(oracle):
    """case id -> fresh (E64 f* grid, f* points, alpha); measure_e64 asserts that oracle and restatement report every patch SPD"""
    DA.prefetch(ALL_CASES)
    return {DA.case_id(c): DA.measure_e64(oracle, c) for c in ALL_CASES}


def test_recorded_e64_holds(measured):
    print("E64 = {")
    for cid, e in measured.items():
        print('    "%s": (%.3e, %.3e, %.3e),' % ((cid,) + e))
    print("}")
    assert sorted(DA.E64) == sorted(measured)
    for cid, e in measured.items():
        for fresh, rec, what in zip(e, DA.E64[cid], ("f_grid", "f_pts", "alpha")):
            assert fresh <= rec, (cid, what, fresh, rec)
            assert rec <= 2.0 * fresh, (cid, what, fresh, rec)          # a record far above the measurement would be a loose gate


def test_no_gate_exceeds_the_cap():
    worst = max(max(DA.gates(c).values()) for c in ALL_CASES)
    print("largest gate: %.3e" % worst)
    assert worst <= DA.GATE_CAP
    assert DA.GATE_FACTOR == 8.0 and DA.GATE_FLOOR == 32.0 * 2.0 ** -53 and DA.GATE_CAP == 1e-10
    assert DA.gate(0.0) == DA.GATE_FLOOR and DA.gate(1e-12) == 8e-12 + DA.GATE_FLOOR


def test_size_lists_hold_every_tile_edge():
    assert {0, 1, 15, 16, 17, 64, 65, 191, 192, 193, 255, 256} <= set(DA.SIZES_256) and max(DA.SIZES_256) == 256
    assert DA.SIZES_512[:len(DA.SIZES_256)] == DA.SIZES_256 and {257, 272, 273, 511, 512} <= set(DA.SIZES_512) and max(DA.SIZES_512) == 512
    assert DA.SIZES_TILED[:len(DA.SIZES_512)] == DA.SIZES_512 and DA.SIZES_TILED[len(DA.SIZES_512):] == [513, 1024]
    assert DA.SIZES_TILED.count(1024) == 1                      # the one patch whose 80-bit solve takes seconds
    assert DA.SIZES_256[0] == 256                               # (the largest patch first: the batch's size class is known at patch 0)
    for ss, sizes in DA.THR_SIZES.items():
        assert all(200 <= n <= 256 for n in sizes) if ss == "t256" else sum(n > 256 for n in sizes) == 1
    # the cases are what the issue lists: three families x three regimes x both noise conventions x ny 1 and 3
    assert len(DA.edge_cases()) == 3 * 3 * 2 * 2 and len({DA.case_id(c) for c in ALL_CASES}) == len(ALL_CASES)
    for fam, P in DA.FAMILIES.items():
        for ny in (1, 3):
            (off, x0, x1, y), regime, dbl = DA.case_inputs(("edge", fam, "default", 0, ny))
            want = {"n256": DA.SIZES_256, "n512": DA.SIZES_512, "tiled": DA.SIZES_TILED}[fam]
            assert np.array_equal(np.diff(off), want) and y.shape == (ny, sum(want)) and x0.shape == x1.shape == (sum(want),)
            assert regime == DA.VC.DEFAULT and dbl == 0
    # ny = 1 is plane 0 of ny = 3, and the planes differ
    y1, y3 = DA.case_inputs(("edge", "n512", "short", 1, 1))[0][3], DA.case_inputs(("edge", "n512", "short", 1, 3))[0][3]
    assert np.array_equal(y1[0], y3[0]) and not np.array_equal(y3[0], y3[1]) and not np.array_equal(y3[1], y3[2])


def test_xstars():
    (g0, g1), (q0, q1) = DA.xstars()
    assert g0.shape == (DA.SZ ** 2,) and q0.shape == (DA.M_PTS,)
    assert DA.M_PTS % 16 != 0 and DA.SZ ** 2 % 256 != 0
    assert np.any(np.abs(q0) > DA.RES / 2) and np.max(np.abs(g0)) < DA.RES / 2


def test_grid_is_the_oracles(oracle):
    (g0, g1), _ = DA.xstars()
    o0, o1 = oracle.grid(DA.RES, DA.SZ)
    assert np.array_equal(g0, o0) and np.array_equal(g1, o1)


# what each kernel must choose at a setting: (small_gram, small_grid) of the tile kernels -- None: not what the setting is about, and
# (mode_g, mode_p) of the one-wave kernel
INTENDED = {
    ("gram", 2.0 ** -5, "under"): ((True, None), (1, None)), ("gram", 2.0 ** -5, "over"): ((False, None), (0, 0)),
    ("gram", 2.0 ** -8, "under"): ((True, None), (2, None)), ("gram", 2.0 ** -8, "over"): ((True, None), (1, None)),
    ("gram", 2.0 ** -3, "under"): ((False, None), (0, 0)),
    ("grid", 2.0 ** -5, "under"): ((True, True), (1, 1)), ("grid", 2.0 ** -5, "over"): ((True, False), (1, 0)),
    ("grid", 2.0 ** -8, "under"): ((True, True), (2, 2)), ("grid", 2.0 ** -8, "over"): ((True, True), (2, 1)),
    ("grid", 2.0 ** -3, "under"): ((True, False), (1, 0)),
}


@pytest.mark.parametrize("case", DA.threshold_cases(), ids=DA.case_id)
def test_threshold_batch_is_where_it_should_be(case):
    _, ss, sel, thr, side = case
    (off, x0, x1, y), regime, dbl = DA.case_inputs(case)
    assert y.shape[0] == 1 and dbl == 1 and regime[0] == DA.THR_SF and regime[2] == DA.THR_SN
    c = DA.c_exp(regime[1])
    (want_tg, want_tp), (want_mg, want_mp) = INTENDED[(sel, thr, side)]
    k = 0 if sel == "gram" else 1
    for i in range(len(off) - 1):
        p0, p1 = x0[off[i]:off[i + 1]], x1[off[i]:off[i + 1]]
        bt, bw = DA.selector_bounds_tile(p0, p1), DA.selector_bounds_w1(p0, p1)
        # each kernel's own bound, in its own association, is on the intended side, 2^-20 away to within roundings
        for b in (bt[k], bw[k]):
            assert abs(-c * b / thr - DA.SIDE[side]) <= 2.0 ** -40
            assert (-c * b < thr) if side == "under" else (-c * b > thr)
        tg, tp = DA.modes_tile(p0, p1, regime[1])
        mg, mp = DA.modes_w1(p0, p1, regime[1])
        assert tg == want_tg and (want_tp is None or tp == want_tp), (i, tg, tp)
        assert mg == want_mg and (want_mp is None or mp == want_mp), (i, mg, mp)
        # the bound is attained: the corner points make the largest argument that really occurs equal to it
        true = DA.largest_true_argument(p0, p1, sel)
        if sel == "gram":
            for b in (bt[0], bw[0]):
                assert abs(float(true / np.longdouble(b)) - 1.0) <= 2.0 ** -40
        else:
            # ... up to the grid's half cell: the outermost cell CENTRE is res / (2 sz) inside the window that the selectors bound
            for b in (bt[1], bw[1]):
                want = (np.sqrt(np.longdouble(b)) - np.longdouble(DA.RES) / (2 * DA.SZ)) ** 2
                assert abs(float(true / want) - 1.0) <= 2.0 ** -40 and true < b
            assert -c * bt[0] < thr * 0.5 and -c * bw[0] < thr * 0.5         # the Gram bound is well on the polynomial side of this threshold


def test_threshold_batches_share_one_box():
    for ss in DA.THR_SIZES:
        for sel in ("gram", "grid"):
            off, x0, x1, _ = DA.threshold_batch(ss, sel)
            boxes = {(x0[off[i]:off[i + 1]].min(), x0[off[i]:off[i + 1]].max(), x1[off[i]:off[i + 1]].min(), x1[off[i]:off[i + 1]].max(),
                      x0[off[i]], x1[off[i]]) for i in range(len(off) - 1)}
            assert len(boxes) == 1
            s = DA.GRID_SHIFT if sel == "grid" else 0.0
            assert boxes.pop()[4:] == (s, -s)


def test_error_measure():
    off = np.array([0, 2, 2, 3], dtype=np.int32)
    want = np.array([[1.0, -4.0, 0.0]], dtype=np.longdouble)
    got = np.array([[1.0, -4.0, 0.0]])
    assert DA.batch_error(got, want, off, True) == (0.0, -1)
    got[0, 0] = 1.5
    assert DA.batch_error(got, want, off, True) == (0.125, 0)             # relative to the patch's largest value
    got[0, 2] = 0.25
    assert DA.batch_error(got, want, off, True) == (0.25, 2)              # max|want| = 0: absolute
    got[0, 2] = np.nan
    assert DA.batch_error(got, want, off, True)[0] == np.inf
    f_want = np.zeros((3, 1, 4), dtype=np.longdouble)
    f_want[0], f_want[2] = 2.0, 1.0
    f = f_want.astype(np.float64)
    assert DA.batch_error(f, f_want, off, False)[0] == 0.0
    f[1, 0, 3] = 1e-300                                                    # an empty patch must be exactly 0
    assert DA.batch_error(f, f_want, off, False) == (np.inf, 1)


def _taylor(t, deg):
    """exp(-t) as its Taylor polynomial of degree deg (Horner)"""
    p = np.zeros_like(t)
    for k in range(deg, -1, -1):
        p = p * t + (-1.0) ** k / math.factorial(k)
    return p


@pytest.mark.parametrize("ss", list(DA.THR_SIZES))
@pytest.mark.parametrize("sel", ["gram", "grid"])
@pytest.mark.parametrize("thr,deg", [(2.0 ** -5, 5), (2.0 ** -3, 7)])
def test_gate_catches_a_polynomial_used_past_its_threshold(ss, sel, thr, deg):
    """The batch whose Gram (grid) bound is just under thr, fitted in float64 (NumPy / LAPACK) with exp and with the Taylor polynomial a
    wrong selector would run there -- in the Gram matrix, or in the separable grid factors of K*.  The honest fit is inside the gate;
    the wrong Gram polynomial misses it on f* (3 .. 8 gates) and by two orders of magnitude on alpha, the wrong grid polynomial leaves
    alpha alone and misses the f* gate by two orders of magnitude.  No device code is involved."""
    case = ("thr", ss, sel, thr, "under")
    (off, x0, x1, y), (sf, l_sq, sn), dbl = DA.case_inputs(case)
    (g0, g1), _ = DA.xstars()
    c = DA.c_exp(l_sq)
    gate = DA.gates(case)
    for wrong in (False, True):
        ex = (lambda t: _taylor(t, deg)) if wrong else (lambda t: np.exp(-t))
        ex_gram, ex_grid = (ex, lambda t: np.exp(-t)) if sel == "gram" else (lambda t: np.exp(-t), ex)
        fg, al = np.zeros((len(off) - 1, 1, DA.SZ ** 2)), np.zeros_like(y)
        for i in range(len(off) - 1):
            sl = slice(off[i], off[i + 1])
            d0, d1 = x0[sl, None] - x0[None, sl], x1[sl, None] - x1[None, sl]
            K = sf * ex_gram(-c * (d0 * d0 + d1 * d1))
            K[np.diag_indices(K.shape[0])] += sn * (1 + dbl)
            L = np.linalg.cholesky(K)
            al[:, sl] = np.linalg.solve(L.T, np.linalg.solve(L, y[:, sl].T)).T
            e0, e1 = x0[sl, None] - g0[None, :], x1[sl, None] - g1[None, :]
            fg[i] = al[:, sl] @ (sf * ex_grid(-c * (e0 * e0)) * ex_grid(-c * (e1 * e1)))         # one factor per axis, as the kernels form K*
        e = DA.errors(case, f_grid=fg, alpha=al)
        rf, ra = e["f_grid"][0] / gate["f_grid"], e["alpha"][0] / gate["alpha"]
        print("%s, %s bound 2^%d (1 - 2^-20), %s: f* %.2e = %.2f gates, alpha %.2e = %.2f gates"
              % (ss, sel, round(math.log2(thr)), "degree %d" % deg if wrong else "exp", e["f_grid"][0], rf, e["alpha"][0], ra))
        if not wrong:
            assert rf <= 1.0 and ra <= 2.0      # (LAPACK's blocked solve: measured 0.1 of the f* gate, 0.4 .. 0.8 of the alpha gate)
        elif sel == "gram":
            assert rf > 2.0 and ra > 64.0
        else:
            assert rf > 32.0
