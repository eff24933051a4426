"""The reference and the inputs of test_dense_variance_gpu.py, checked without a GPU.

The GPU tests compare the variance kernels with the CPU oracle at 4e-9 of sigma_f^2 (v) and 1e-9 (f*).  Here the oracle itself is held
against an 80-bit restatement of the same formulas (variance_cases.hp_fit_predict) at 1e-13 sigma_f^2 and 1e-10: 25 times or more above
the gaps measured between the two (worst: 3.9e-15 sigma_f^2 on v at 1024 points, 3.1e-12 on f* at 529 points with l = 0.5), and 100
times below the bounds of the GPU tests that rely on it.  The case builders are checked for what the GPU tests assume of them."""
import numpy as np
import pytest

import variance_cases as VC

V_RTOL, F_RTOL = 1e-13, 1e-10


def _against_hp(oracle, regime, off, x0, x1, y, xs0, xs1, idx):
    (so_, sx0, sx1, sy), _ = VC.take_patches(off, x0, x1, y, idx)
    fo, vo, sto = oracle.dense_fit_predict_batch(oracle.dense_params(*regime), so_, sx0, sx1, sy, xs0, xs1, variance=True)
    for j in range(len(idx)):
        sl = slice(so_[j], so_[j + 1])
        st, f, v, _ = VC.hp_fit_predict(regime, sx0[sl], sx1[sl], sy[:, sl], xs0, xs1)
        assert st == 0 and sto[j] == 0
        ev = float(np.max(np.abs(vo[j] - v))) / regime[0]
        ef = float(np.max(np.abs(fo[j] - f))) / max(float(np.max(np.abs(f))), 1e-300)
        print("n = %d, regime %s: |v - v_hp| / sf^2 = %.2e, f* %.2e" % (so_[j + 1] - so_[j], regime, ev, ef))
        assert ev <= V_RTOL and ef <= F_RTOL, (idx[j], ev, ef)


@pytest.mark.parametrize("regime", [VC.DEFAULT, VC.SHORT, VC.MEDIUM], ids=["default", "short", "medium"])
def test_oracle_variance_against_extended_precision(oracle, regime):
    """One tile row past a super-row (17), 17 tiles (272), 34 tiles (529): oracle against the 80-bit restatement, ny = 3."""
    sizes = [17, 272, 529]
    off, x0, x1, y = VC.with_planes(*VC._mixed_batch(sizes, seed=71), ny=3, seed=72)
    xs0, xs1 = VC.xstar(21, seed=73)
    _against_hp(oracle, regime, off, x0, x1, y, xs0, xs1, [0, 1, 2])


@pytest.mark.parametrize("regime", [VC.DEFAULT, VC.ZERO_NOISE], ids=["default", "zero_noise"])
def test_many_patch_batch_and_its_oracle(oracle, regime):
    """Test 3's batch is what the test says it is, the oracle fits every patch that has no repeated point in both regimes, and on five
    of them it agrees with the 80-bit restatement."""
    sizes = VC.many_sizes()
    off, x0, x1, y = VC.many_batch()
    assert len(sizes) == VC.MANY_P == 600 and np.array_equal(np.diff(off), sizes)
    assert sizes[0] == 336 and max(sizes) == 336
    assert tuple(np.flatnonzero(np.asarray(sizes) == 0)) == VC.MANY_EMPTY
    a, b = VC.MANY_DUP_AT
    for i in VC.MANY_DUP:
        assert sizes[i] == 300
        assert x0[off[i] + a] == x0[off[i] + b] and x1[off[i] + a] == x1[off[i] + b]
    # no other patch repeats a point
    for i in range(VC.MANY_P):
        pts = np.stack([x0[off[i]:off[i + 1]], x1[off[i]:off[i + 1]]], 1)
        assert len(np.unique(pts, axis=0)) == sizes[i] - (1 if i in VC.MANY_DUP else 0)
    xs0, xs1 = VC.xstar(1, seed=74)
    _, _, st = oracle.dense_fit_predict_batch(oracle.dense_params(*regime), off, x0, x1, y, xs0, xs1, variance=True)
    good = np.ones(VC.MANY_P, dtype=bool)
    good[list(VC.MANY_DUP)] = False
    assert np.all(st[good] == 0)
    if regime == VC.DEFAULT:
        assert np.all(st == 0)              # (with a noise term a repeated point is harmless)
    xs0, xs1 = VC.xstar(37, seed=31)
    _against_hp(oracle, regime, off, x0, x1, y, xs0, xs1, [0, 1, 6, 299, 598])


def test_restatement_on_a_repeated_point():
    """The restatement reports what the kernels report for a singular patch -- status 1, NaN everywhere -- on two coincident points
    (the second pivot is exactly zero in any precision: both rows of K are equal)."""
    x0, x1 = np.array([0.01, 0.01, 0.02]), np.array([0.0, 0.0, 0.03])
    st, f, v, al = VC.hp_fit_predict(VC.ZERO_NOISE, x0, x1, np.ones((1, 3)), *VC.xstar(4, seed=1))
    assert st == 1 and np.all(np.isnan(f)) and np.all(np.isnan(v)) and np.all(np.isnan(al))


def test_case_builders():
    assert VC.TILE_SIZES.count(0) == 2 and max(VC.TILE_SIZES) == 1024
    nts = {(n + 15) // 16 for n in VC.TILE_SIZES}
    assert {1, 2, 16, 17, 18, 32, 33, 34, 48, 49, 63, 64} <= nts
    off, x0, x1, y = VC.tile_batch(3)
    assert y.shape == (3, sum(VC.TILE_SIZES)) and np.array_equal(np.diff(off), VC.TILE_SIZES)
    assert not np.array_equal(y[0], y[1]) and not np.array_equal(y[1], y[2])
    assert np.array_equal(VC.tile_batch(1)[3][0], y[0])
    idx = [i for i, n in enumerate(VC.TILE_SIZES) if n <= 528]
    (so_, sx0, _, sy), pts = VC.take_patches(off, x0, x1, y, idx)
    assert int(np.max(np.diff(so_))) == 528 and np.array_equal(sx0, x0[pts]) and sy.shape == (3, so_[-1])
    for n_max, want in ((64, 13), (128, 25), (192, 37)):
        s = VC.edge_sizes(n_max)
        assert len(s) == want and s[:5] == [0, 1, 15, 16, 17] and s[-2:] == [n_max - 1, n_max]
        (o, a0, a1, _), mid = VC.edge_batch(n_max, dup=True)
        n = s[mid]
        assert n >= 32 and a0[o[mid] + n - 3] == a0[o[mid] + 2] and a1[o[mid] + n - 3] == a1[o[mid] + 2]
    for P in (2100, 4200):
        s = np.asarray(VC.chunk_sizes(P))
        q = P // 4
        assert len(s) == P and s[:q].max() <= 190 and 192 < s[q:2 * q].max() <= 256 and s[q:2 * q].min() >= 200
        assert s[2 * q:3 * q].min() >= 257 and s[2 * q:3 * q].max() <= 300 and s[3 * q:].max() <= 330 and 300 < s.max() <= 330
    xs0, xs1 = VC.xstar(129, seed=3)
    assert xs0.shape == (129,) and np.max(np.abs(xs0)) <= 0.09 and np.any(np.abs(xs0) > 0.075) and np.any(np.abs(xs1) > 0.075)
