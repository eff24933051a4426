"""The reference and the inputs of test_irls_gpu.py, checked without a GPU.

The GPU tests compare the Newton / IRLS kernels with the CPU oracle (orc_dense_irls_fit) at 1e-8 (model 2) and 1e-6 (model 1) of the
max-norm.  Here the oracle itself is held against Algorithm 3.1 of Rasmussen & Williams as printed (np_restatement.laplace_mode_rw: the
B = I + W^1/2 K W^1/2 route, LAPACK) up to 1024 points at test_oracle.py's bounds, the case builders are checked for what the GPU tests
assume of them, and so are the conditions on the oracle's results that those tests lean on (which patches converge, after how many steps,
what a NaN label and the singular start give)."""
import numpy as np
import pytest

import irls_cases as IC
import np_restatement as R
import variance_cases as VC

XS1 = (np.zeros(1), np.zeros(1))            # one prediction point: these tests are about the fit


@pytest.mark.parametrize("model", [2, 1])
def test_oracle_irls_against_rw_alg31_up_to_1024(oracle, model):
    """orc_dense_irls_fit against Algorithm 3.1 as printed at 17, 272, 529 and 1024 points: the same iteration count, fhat to 1e-10 and a
    to 1e-9 of their max-norms (test_oracle.py's bounds, there up to 300 points).  Measured on the batch below: worst gaps 9.5e-14 on
    fhat and 1.4e-12 on a (model 1, 1024 points) -- 1e4 times below the 1e-8 of the GPU tests that rely on the oracle."""
    batch = IC.labelled(VC._mixed_batch([17, 272, 529, 1024], seed=83))
    off, x0, x1, lab = batch
    f, al, fh, it, st = IC.oracle_fit(oracle, batch, model, XS1)
    assert np.all(st == 0)
    for i in range(4):
        sl = slice(off[i], off[i + 1])
        X = np.stack([x0[sl], x1[sl]], 1)
        fr, ar, ir = R.laplace_mode_rw(X, lab[sl], *IC.REGIME, std_phi=(model == 2), max_iter=IC.MAX_ITER, **IC.MODELS[model])
        ef = float(np.max(np.abs(fr - fh[sl]))) / float(np.max(np.abs(fr)))
        ea = float(np.max(np.abs(ar - al[sl]))) / float(np.max(np.abs(ar)))
        print("model %d, n = %d: %d steps, |fhat - fhat_rw| = %.2e, |a - a_rw| = %.2e" % (model, off[i + 1] - off[i], it[i], ef, ea))
        assert ir == it[i]
        assert ef <= 1e-10 and ea <= 1e-9, (i, ef, ea)


def test_case_builders():
    assert IC.TILE_SIZES_BIG.count(0) == 2 and IC.TILE_SIZES_BIG[0] == max(IC.TILE_SIZES_BIG) == 1024
    nts = {(n + 15) // 16 for n in IC.TILE_SIZES_BIG if n}
    assert set(range(1, 6)) | set(range(16, 22)) | {32, 33, 48, 49} | set(range(60, 65)) == nts
    for lo, hi in ((1, 5), (60, 64)):       # every nt mod 4 at both ends of the range
        assert {nt % 4 for nt in nts if lo <= nt <= hi} == {0, 1, 2, 3}
    full = IC.tile_batch()
    off, x0, x1, lab = full
    assert np.array_equal(np.diff(off), IC.TILE_SIZES_BIG) and lab.shape == x0.shape and set(np.unique(lab)) == {-1.0, 1.0}
    for cap, ntw in zip(IC.CAPS, (64, 33, 17)):
        idx = IC.cap_index(cap)
        (so, sx0, sx1, sl), pts = IC.take(full, idx)
        n_max = int(np.max(np.diff(so)))
        assert n_max == cap > 256 and (n_max + 15) // 16 == ntw                     # the eight-wave shape, three slot strides
        assert np.array_equal(sx0, x0[pts]) and np.array_equal(sl, lab[pts]) and np.count_nonzero(np.diff(so) == 0) == 2
    assert IC.cap_index(IC.MODEL1_CAP) == IC.cap_index(513)
    w4 = IC.w4_batch()
    s = np.diff(w4[0]).tolist()
    assert s == VC.edge_sizes(256) and s[:5] == [0, 1, 15, 16, 17] and s[-2:] == [255, 256] and len(s) == 49
    for which, P, n_hi in (("big", 600, 336), ("w4", 1100, 96)):
        c = IC.MANY[which]
        sizes = np.asarray(IC.many_sizes(which))
        off, x0, x1, lab = IC.many_batch(which)
        assert len(sizes) == P == c["P"] and np.array_equal(np.diff(off), sizes)
        assert sizes[0] == n_hi == sizes.max() and sizes[sizes > 0].min() == 1
        assert tuple(np.flatnonzero(sizes == 0)) == c["empty"]
        bad = np.flatnonzero(np.isnan(lab))
        assert bad.tolist() == [off[i] + at for i, at in zip(c["nan"], c["nan_at"])]
        n0, at0 = sizes[c["nan"][0]], c["nan_at"][0]
        assert at0 == n0 - 1 and n0 % 16 != 0                                      # the last point, with padding rows behind it
        for i, at in list(zip(c["nan"], c["nan_at"]))[1:]:
            assert 0 < at // 16 < (sizes[i] - 1) // 16                              # a middle tile
        for i in c["nan"]:                                                         # healthy neighbours in index and a stride later
            for j in (i - 1, i + 1, (i + 256) % P, (i + 512) % P):
                assert sizes[j] > 0 and np.all(np.isfinite(lab[off[j]:off[j + 1]]))
        assert set(np.unique(lab[np.isfinite(lab)])) == {-1.0, 1.0}
    assert IC.MANY["big"]["P"] > 2 * 256 and IC.MANY["w4"]["P"] > 4 * 256           # more patches than either shape is given workgroups
    for shape, n_max in (("big", 420), ("w4", 256)):
        o = IC.grid_batch(shape)[0]
        assert len(o) == 6 and int(np.max(np.diff(o))) == n_max and np.count_nonzero(np.diff(o) == 0) == 1


def _finite_patches(off, lab):
    return np.array([bool(np.all(np.isfinite(lab[off[i]:off[i + 1]]))) for i in range(len(off) - 1)])


@pytest.mark.parametrize("which", ["big", "w4"])
def test_many_patch_batches_on_the_oracle(oracle, which):
    """What the GPU tests of the two 600- and 1100-patch batches lean on, model 2: every patch with finite labels ends with status 0
    under max_iter = 30, every non-empty one after at least 4 steps (so a cap of 2 is never a borderline decision: status 5, iters 2);
    a NaN label gives status 2, iters 0 and NaN f*, alpha, fhat for its own patch under both models."""
    c = IC.MANY[which]
    batch = IC.many_batch(which)
    off, _, _, lab = batch
    n = np.diff(off)
    fin = _finite_patches(off, lab)
    assert np.array_equal(np.flatnonzero(~fin), c["nan"])
    f, al, fh, it, st = IC.oracle_fit(oracle, batch, 2, XS1)
    assert np.all(st[fin] == 0) and np.all(it[fin & (n > 0)] >= 4) and it.max() < IC.MAX_ITER and np.all(it[n == 0] == 0)
    print("many_%s, model 2: %d .. %d steps" % (which, it[fin & (n > 0)].min(), it.max()))
    f2, al2, fh2, it2, st2 = IC.oracle_fit(oracle, batch, 2, XS1, max_iter=2)
    assert np.all(st2[fin & (n > 0)] == 5) and np.all(it2[fin & (n > 0)] == 2) and np.all(st2[n == 0] == 0)
    sub, pts = IC.take(batch, c["nan"])
    for model in (2, 1):
        for r in (IC.oracle_fit(oracle, sub, model, XS1), IC.oracle_fit(oracle, sub, model, XS1, max_iter=2)):
            assert np.all(r[4] == 2) and np.all(r[3] == 0) and all(np.all(np.isnan(a)) for a in r[:3])
    for i in c["nan"]:
        assert st[i] == 2 and it[i] == 0 and np.all(np.isnan(f[i])) and np.all(np.isnan(al[off[i]:off[i + 1]])) and np.all(np.isnan(fh[off[i]:off[i + 1]]))
    keep = np.ones(off[-1], dtype=bool)
    keep[pts] = False
    assert np.all(np.isfinite(al[keep])) and np.all(np.isfinite(fh[keep])) and np.all(np.isfinite(f[fin]))


@pytest.mark.parametrize("model", [2, 1])
def test_sweeps_converge_on_the_oracle(oracle, model):
    """Every patch of the tile-count sweeps ends with status 0 under max_iter = 30 and every non-empty one needs at least 4 steps: the
    whole sweep under model 2, the sizes up to 529 under model 1, the four-wave batch under both.  Drawn with other seeds here (the GPU
    test computes its own oracle results and asserts the statuses again)."""
    sizes = IC.TILE_SIZES_BIG if model == 2 else [n for n in IC.TILE_SIZES_BIG if n <= IC.MODEL1_CAP]
    for batch in (IC.labelled(VC._mixed_batch(sizes, seed=87)), IC.labelled(VC._mixed_batch(VC.edge_sizes(256), seed=88))):
        n = np.diff(batch[0])
        _, _, _, it, st = IC.oracle_fit(oracle, batch, model, XS1)
        print("model %d, %d patches up to %d points: %d .. %d steps" % (model, len(n), n.max(), it[n > 0].min(), it.max()))
        assert np.all(st == 0) and np.all(it[n > 0] >= 4) and it.max() < IC.MAX_ITER and np.all(it[n == 0] == 0)


def test_failure_cases_on_the_oracle(oracle):
    """Model 1 from f_init = 0 is singular (erf(0) = 0): status 2 and iters 0 for every non-empty patch, status 0 for the empty ones.
    A zero label: model 1 fails at step 0; model 2 does NOT fail (z = 0 gives a finite positive weight) -- it is no failure case there."""
    for which in ("w4", "big"):
        sub, _ = IC.take(IC.many_batch(which), range(40))
        n = np.diff(sub[0])
        f, al, fh, it, st = IC.oracle_fit(oracle, sub, 1, XS1, f_init=0.0)
        assert np.count_nonzero(n == 0) == 1 and np.all(st[n > 0] == 2) and np.all(st[n == 0] == 0) and np.all(it == 0)
        assert np.all(np.isnan(al)) and np.all(np.isnan(fh)) and np.all(np.isnan(f[n > 0])) and np.all(f[n == 0] == 0)
    off, x0, x1, lab = IC.labelled(VC._mixed_batch([40], seed=89))
    lab[17] = 0.0
    r1 = IC.oracle_fit(oracle, (off, x0, x1, lab), 1, XS1)
    assert r1[4][0] == 2 and r1[3][0] == 0
    r2 = IC.oracle_fit(oracle, (off, x0, x1, lab), 2, XS1, max_iter=200)
    assert r2[4][0] in (0, 5) and r2[3][0] >= 1 and np.all(np.isfinite(r2[2]))
