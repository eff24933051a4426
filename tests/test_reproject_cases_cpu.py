"""The inputs of the reprojection tests at the sizes where the kernels' loops wrap (reproject_cases.py), checked without a GPU: stated on
the oracle alone, the cases are what the GPU tests take them for -- a GPU test must not pass because an input was vacuous."""
import ctypes as C

import numpy as np
import pytest

import reproject_cases as RC

# the compaction sizes, and one size above the emit kernel's grid as an MI355X has it (8 x 256 CUs + 1 is 2049 again) and as a part with
# 304 CUs would
SIZES = sorted(set(RC.COMPACTION_P) | {8 * 256 + 1, 8 * 304 + 1})
CHANNEL = ("r", "g", "b")


def _flatten(oracle, x):
    c3 = np.array([x, 0.0, 0.0])
    rgb = (C.c_uint8 * 3)()
    oracle.lib().orc_flatten_colors(oracle._dp(c3), rgb)
    return int(rgb[0])


def test_specials_and_their_outcomes(oracle):
    """the list holds the existing corner values and the conversion edges, the oracle flattens each to the byte the case table states,
    and every outcome of the clamp occurs: 0, 255, a wrapped short (to 0 and to 255) and the zero of an int overflow"""
    assert len(RC.SPECIALS) == len(RC.SPECIAL_BYTES) == 28 and RC.SPECIALS[:21] == RC.SPECIALS_BASE
    for v in (2147483647.5, 2147483648.0, -2147483648.0, -2147483649.0, -32768.5, -32769.0, -65536.0):
        assert v in RC.SPECIALS_EDGES
    got = [_flatten(oracle, v) for v in RC.SPECIALS]
    assert got == RC.SPECIAL_BYTES
    by = dict(zip([repr(v) for v in RC.SPECIALS], got))
    assert {0, 255, 127} == set(got)
    assert {by[repr(v)] for v in RC.WRAPPED_SHORT} == {0, 255} and all(abs(v) < 2147483648.0 for v in RC.WRAPPED_SHORT)
    assert {by[repr(v)] for v in RC.INT_OVERFLOW} == {0} and all(not -2147483649.0 < v < 2147483648.0 for v in RC.INT_OVERFLOW)
    # either side of each edge the outcome is stated by a neighbour in the list: the last double inside int and the first outside
    assert by[repr(32767.9)] == 255 and by[repr(32768.0)] == 0 and by[repr(-32768.5)] == 0 and by[repr(-32769.0)] == 255


def _consecutive_mix_in_each_third(bv):
    P = len(bv)
    on = bv != 0
    for k in range(3):
        seg = on[k * P // 3:(k + 1) * P // 3]
        if not np.any(seg[1:] != seg[:-1]):
            return False
    return True


@pytest.mark.parametrize("P", SIZES)
def test_compaction_cases(oracle, P):
    """every pattern at one batch size: the pattern, where the specials sit, and the oracle's cloud"""
    m = RC.COMPACTION_M
    print("P = %d, per = %d" % (P, RC.per_of(P)))
    for name in RC.PATTERNS:
        bv, (xs0, xs1, f, R, mu, cs, cm) = RC.compaction_case(P, name)
        assert (bv is None) == (name == "all")
        t = RC.trained(P, bv)
        if bv is not None:
            assert bv.dtype == np.int32 and bv.shape == (P,) and set(np.unique(bv)) <= {0, 1, 5, 200}
            assert np.array_equal(bv, RC.bv_pattern(name, P, 7))           # deterministic
            if name != "none" and len(t) > 3:
                assert len(set(bv[t].tolist())) > 1                         # the count is not the sum
        n_on = len(t)
        if name == "none":
            assert n_on == 0
        elif name != "all":
            assert 0 < n_on < P
        if name in ("random", "period2", "period3"):
            assert _consecutive_mix_in_each_third(bv)
        assert {"first_only": [0], "last_only": [P - 1]}.get(name, t.tolist()) == t.tolist()
        if name == "head_empty":
            assert not bv[:int(np.ceil(0.6 * P))].any() and bv[int(np.ceil(0.6 * P)):].all()
        if name == "tail_empty":
            assert not bv[P - int(np.ceil(0.6 * P)):].any() and bv[:P - int(np.ceil(0.6 * P))].all()
        # shapes and ranges of the inputs
        assert xs0.shape == xs1.shape == (m,) and max(np.max(np.abs(xs0)), np.max(np.abs(xs1))) <= RC.RES / 2
        assert f.shape == (P, m) and R.shape == (P, 9) and mu.shape == (P, 3) and cs.shape == (P, 3, m) and cm.shape == (P, 3)
        Q = R.reshape(P, 3, 3)
        assert np.max(np.abs(Q @ np.swapaxes(Q, 1, 2) - np.eye(3))) < 1e-13
        assert np.max(np.abs(mu)) <= 50 and np.any(mu.astype(np.float32).astype(np.float64) != mu)
        # the specials: in trained patches, at the head of the batch, near its middle and at its end
        pts = RC.special_patches(P, bv)
        sites = RC.special_sites(P, m, bv, RC.rotate_of(P))
        assert len(pts) == min(3, n_on) and all(p in t for p in pts)
        if n_on:
            assert pts[-1] == t[-1] and (pts[0] < 10 or t[0] >= 10)
        if n_on >= 3:
            assert sorted(repr(s[3]) for s in sites) == sorted(repr(v) for v in RC.SPECIALS)
            assert abs(pts[1] - P // 2) <= np.min(np.abs(np.setdiff1d(t, [pts[0], pts[2]]) - P // 2))
        elif n_on == 1:
            assert len(sites) == 3 * m
        want = RC.expected(oracle, xs0, xs1, f, R, mu, cs, cm, bv)
        assert want.dtype == RC.POINT_DTYPE and want.itemsize == 32
        assert len(want) == m * (P if bv is None else int(np.count_nonzero(bv)))
        assert np.all(want["w"] == 1.0) and np.all(want["a"] == 255) and not want["pad"].any()
        rank = {int(p): k for k, p in enumerate(t)}
        for p, c, q, v in sites:
            s = cs[p, c, q] + cm[p, c]
            if np.isnan(v):
                assert np.isnan(s)
            elif v in RC.SPECIALS_EDGES or not np.isfinite(v) or v == np.trunc(v) or abs(v) >= 1e9:
                assert s == v, (v, s)
            else:
                assert abs(s - v) <= 1e-12 * max(1.0, abs(v)), (v, s)
            assert want[CHANNEL[c]][rank[p] * m + q] == RC.SPECIAL_BYTES[[repr(x) for x in RC.SPECIALS].index(repr(v))], (p, c, q, v)
        if n_on:
            assert {0, 255} <= set(np.unique(np.stack([want["r"], want["g"], want["b"]])))


def test_single_patch_patterns_run_every_special_between_the_sizes():
    """first_only and last_only hold twelve specials at m = 4: the five compaction sizes between them plant the whole list, each size
    a different dozen (every other pattern with a trained patch plants all 28 at every size: test_compaction_cases)"""
    for name in ("first_only", "last_only"):
        seen = set()
        for P in RC.COMPACTION_P:
            vals = [s[3] for s in RC.special_sites(P, RC.COMPACTION_M, RC.bv_pattern(name, P, 7), RC.rotate_of(P))]
            assert len(vals) == 12
            seen |= {repr(v) for v in vals}
        assert seen == {repr(v) for v in RC.SPECIALS}


def test_row_length_cases(oracle):
    """P = 3 at the row lengths either side of the emit kernel's 256-thread pass: every special in every run that has colours"""
    for m in RC.ROW_M:
        for name in ("all", "period2"):
            bv = RC.bv_pattern(name, RC.ROW_P, 11)
            assert RC.trained(RC.ROW_P, bv).tolist() == ([0, 1, 2] if bv is None else [0, 2])
            sites = RC.special_sites(RC.ROW_P, m, bv)
            assert sorted(repr(s[3]) for s in sites) == sorted(repr(v) for v in RC.SPECIALS)
        xs0, xs1, f, R, mu, cs, cm = RC.inputs(RC.ROW_P, m, 11, colours=False)
        assert cs is None and cm is None and xs0.shape == (m,)
        assert len(np.unique(xs0)) == len(np.unique(xs1)) == m                     # points, not a grid
    want = RC.expected(oracle, xs0, xs1, f, R, mu, None, None, RC.bv_pattern("period2", RC.ROW_P, 11))
    assert len(want) == 2 * RC.ROW_M[-1] and not (want["r"].any() or want["g"].any() or want["b"].any()) and np.all(want["a"] == 255)


def test_non_finite_rows(oracle):
    """the non-finite case: rows among the trained patches of the random pattern, all four values present, the rest of f untouched, and
    the oracle's records NaN where f is NaN and infinite floats where f is infinite or overflows the cast"""
    P, m = 1025, RC.COMPACTION_M
    bv, (xs0, xs1, f, R, mu, cs, cm) = RC.compaction_case(P, "random")
    t = RC.trained(P, bv)
    rows = [int(t[0]), int(t[1]), int(t[len(t) // 2]), int(t[-2]), int(t[-1])]
    g = RC.non_finite_rows(f, rows)
    changed = np.flatnonzero(np.any((g != f) | np.isnan(g), axis=1))
    assert changed.tolist() == sorted(rows) and np.all(bv[rows] != 0)
    vals = g[rows].reshape(-1)
    assert np.isnan(vals).any() and (vals == np.inf).any() and (vals == -np.inf).any() and (vals == 1e300).any()
    assert np.sum(~np.isfinite(g) | (g == 1e300)) == 2 * len(rows)
    want = RC.expected(oracle, xs0, xs1, g, R, mu, cs, cm, bv)
    clean = RC.expected(oracle, xs0, xs1, f, R, mu, cs, cm, bv)
    fr = RC.f_of_records(g, bv)
    Rr = np.repeat(R[t], m, axis=0)
    odd = ~np.isfinite(fr) | (fr == 1e300)
    assert want[~odd].tobytes() == clean[~odd].tobytes()
    for k, key in enumerate(("x", "y", "z")):
        assert np.all(np.isnan(want[key][np.isnan(fr)]))
        big = odd & ~np.isnan(fr)
        assert np.array_equal(want[key][big], (np.sign(fr[big]) * np.sign(Rr[big, k]) * np.inf).astype(np.float32))
    for key in ("r", "g", "b", "a", "w"):
        assert np.array_equal(want[key], clean[key])
