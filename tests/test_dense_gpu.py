"""GPU parity tests of the dense path (gaussian_process fit + predict) through the C-ABI.

Oracle: oracle/gpc_oracle.c (and the NumPy/LAPACK golden fixtures).  Stated tolerance: the HIP path and the CPU
oracle are two fp64 evaluations of the same well-conditioned system (kappa(K + 2 sn^2 I) <= 1 + n sf^2 / (2 sn^2),
~200 at n = 256, ~800 at n = 1024) that differ in summation order, FMA contraction and exp() (<= 2 ulp):
    |f*_gpu - f*_cpu| <= 1e-9 * max|f*|      |alpha_gpu - alpha_cpu| <= 1e-8 * max|alpha|     |V*_gpu - V*_cpu| <= 1e-11
What these round figures do and do not catch, and the measured gate that f* and alpha of every route are held to, is in test_dense_accuracy_gpu.py.
"""
import os

import numpy as np
import pytest

from gp_compressor_amd import synth
from variance_cases import DEFAULT, SHORT, _mixed_batch, with_planes

pytestmark = pytest.mark.gpu

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
FTOL, ATOL, VTOL = 1e-9, 1e-8, 1e-11


@pytest.fixture(scope="module")
def gp():
    from gp_compressor_amd import capi
    capi.load()          # raises if the HIP library is missing: no fallback
    ctx = capi.Context(0)
    yield capi, ctx
    ctx.close()


def _close(f, want, tol):
    scale = max(float(np.max(np.abs(want))), 1e-300)
    err = float(np.max(np.abs(f - want)))
    assert err <= tol * scale, (err, scale)


def _dense_case(name):
    z = np.load(os.path.join(GOLD, "dense_cases.npz"))
    return {k.split(".", 1)[1]: z[k] for k in z.files if k.startswith(name + ".")}


@pytest.mark.parametrize("name", ["tiny", "c1", "rgb", "n256"])
def test_dense_golden(gp, name, monkeypatch):
    capi, ctx = gp
    d = _dense_case(name)
    p = capi.default_params_dense(want_variance=1)
    f, v, st, al = ctx.dense_fit_predict(p, d["off"], d["x0"], d["x1"], d["y"], d["xs0"], d["xs1"], want_alpha=True)
    assert np.all(st == 0)
    _close(f, d["f_star"], FTOL)
    _close(al, d["alpha"], ATOL)
    assert np.max(np.abs(v - d["v_star"])) <= VTOL
    # the variance kernel picks four or eight waves per workgroup by how the 16-point blocks fill its rounds: both shapes do the
    # same arithmetic per block on the same factor, so forcing either one gives the same variance bit for bit (the mean goes through
    # alpha, whose backward solve adds with LDS atomics in no fixed order: equal to a rounding or two, run to run)
    for w4 in ("0", "1"):
        monkeypatch.setenv("GPC_VAR_W4", w4)
        f2, v2, st2, _ = ctx.dense_fit_predict(p, d["off"], d["x0"], d["x1"], d["y"], d["xs0"], d["xs1"], want_alpha=True)
        assert np.array_equal(v2, v) and np.array_equal(st2, st)
        _close(f2, f, 1e-12)


@pytest.fixture(params=["dispatch", "generic", "big", "reg", "big_w4", "w2"])
def kernel_choice(request, monkeypatch):
    """Run a test with the normal dispatch -- the one-wave-per-patch kernel for the depth plane of n <= 256 (at every batch size here:
    GPC_W1_MIN_P=2; in production from 4 patches per CU up), the register-tile MFMA kernel for colour planes, the tiled left-looking
    MFMA kernel above 256 points --, with the generic global-workspace kernel forced, with the left-looking kernel forced for every n
    (its two-wave / four-workgroups-per-CU shape below 257 points for the depth plane), with the register-tile kernel for every
    n <= 256 ("reg": GPC_NO_W1), with the tiled kernel's four-wave shape ("big_w4"), and with the two-wave shape where round 3's first
    headline ran it ("w2": GPC_W2, depth plane of 193 .. 256 points).  The environment is read at every call."""
    for e in ("GPC_FORCE_GENERIC", "GPC_FORCE_BIG", "GPC_BIG_NO_W2", "GPC_NO_W1", "GPC_W2", "GPC_W1_MIN_P"):
        monkeypatch.delenv(e, raising=False)
    if request.param == "dispatch":
        monkeypatch.setenv("GPC_W1_MIN_P", "2")
    elif request.param == "generic":
        monkeypatch.setenv("GPC_FORCE_GENERIC", "1")
    elif request.param == "big":
        monkeypatch.setenv("GPC_FORCE_BIG", "1")
    elif request.param == "reg":
        monkeypatch.setenv("GPC_NO_W1", "1")
    elif request.param == "big_w4":
        monkeypatch.setenv("GPC_FORCE_BIG", "1")
        monkeypatch.setenv("GPC_BIG_NO_W2", "1")
    elif request.param == "w2":
        monkeypatch.setenv("GPC_NO_W1", "1")
        monkeypatch.setenv("GPC_W2", "1")
    return request.param


@pytest.mark.parametrize("P,n,ny,ragged,seed", [(37, 64, 1, True, 1), (9, 200, 3, True, 2), (5, 256, 1, False, 3),
                                                (3, 300, 1, True, 4), (2, 515, 3, True, 5), (40, 17, 1, True, 6),
                                                (11, 128, 1, True, 7), (6, 192, 1, True, 8), (300, 256, 1, True, 9),
                                                (3, 512, 1, False, 10), (1, 1024, 1, False, 11)])   # C3 / C5 patch sizes
def test_dense_vs_oracle(gp, oracle, kernel_choice, P, n, ny, ragged, seed):
    capi, ctx = gp
    off, x0, x1, y = synth.make_patches(P, n, seed=seed, ragged=ragged, ny=ny)
    xs0, xs1 = synth.grid(0.15, 12)
    for dbl in (1, 0):
        p = capi.default_params_dense(want_variance=1, ref_double_noise=dbl)
        f, v, st, al = ctx.dense_fit_predict(p, off, x0, x1, y, xs0, xs1, want_alpha=True)
        if kernel_choice == "dispatch":      # the variance runs on the MFMA pipe at every size: register-tile or tiled fit + its solve kernel
            nm = int(np.max(np.diff(off)))
            assert ctx.last_dense_kernel().endswith(" + dense_variance" if nm <= 256 else " + dense_variance_big"), ctx.last_dense_kernel()
        fo, vo, so, ao = oracle.dense_fit_predict_batch(oracle.dense_params(ref_double_noise=dbl), off, x0, x1, y, xs0, xs1,
                                                        variance=True, want_alpha=True)
        assert np.array_equal(st, so)
        _close(f, fo, FTOL)
        _close(al, ao, ATOL)
        assert np.max(np.abs(v - vo)) <= VTOL
    # mean-only call: this is what dispatches to the register-tile kernel (n <= 256) or the tiled left-looking MFMA kernel (n <= 1024)
    p = capi.default_params_dense()
    f, _, st, al = ctx.dense_fit_predict(p, off, x0, x1, y, xs0, xs1, want_alpha=True)
    fo, _, so, ao = oracle.dense_fit_predict_batch(oracle.dense_params(), off, x0, x1, y, xs0, xs1, want_alpha=True)
    n_max = int(np.max(np.diff(off)))
    # depth plane, n <= 256, more than one patch: one wave per patch (dense_mfma_w1); "w2": the two-wave shape of the tiled kernel for
    # 193 .. 256 points; otherwise the register-tile kernel
    small1 = n_max <= 256 and y.shape[0] == 1 and P > 1
    want_small = "dense_mfma_w1" if (small1 and kernel_choice == "dispatch") else \
                 "dense_mfma_big_w2" if (small1 and n_max > 192 and kernel_choice == "w2") else "dense_mfma_nt"
    uniform = int(np.min(np.diff(off))) == n_max        # one size class, known on the host (P n_max == n_total): no split launches
    want_kernel = {"generic": "dense_generic", "big": "dense_mfma_big", "big_w4": "dense_mfma_big"}.get(
        kernel_choice, ("dense_mfma_nt16 + " if (P > 1 and not (uniform and n_max > 272)) else "dense_mfma_big") if n_max > 256 else want_small)
    if kernel_choice == "dispatch" and 256 < n_max <= 512 and y.shape[0] == 1 and P > 1:
        want_kernel = "dense_mfma_w1_512"       # round 4: the 512-point instance of the one-wave kernel takes the depth plane up to 512 points
    assert ctx.last_dense_kernel().startswith(want_kernel), ctx.last_dense_kernel()
    assert np.array_equal(st, so)
    _close(f, fo, FTOL)
    _close(al, ao, ATOL)


def test_dense_other_hyperparameters(gp, oracle):
    capi, ctx = gp
    off, x0, x1, y = synth.make_patches(6, 90, seed=12, ragged=True)
    xs0, xs1 = synth.grid(0.15, 9)
    kw = dict(sigmaf_sq=1.0, l_sq=0.05 ** 2, noise=1e-3)
    p = capi.default_params_dense(want_variance=1, **kw)
    f, v, st = ctx.dense_fit_predict(p, off, x0, x1, y, xs0, xs1)
    fo, vo, so = oracle.dense_fit_predict_batch(oracle.dense_params(kw["sigmaf_sq"], kw["l_sq"], kw["noise"]), off, x0, x1, y,
                                                xs0, xs1, variance=True)
    assert np.all(st == 0)
    _close(f, fo, 1e-8)           # kappa ~ 1 + n/(2e-3) ~ 5e4 here
    assert np.max(np.abs(v - vo)) <= 1e-9


@pytest.mark.parametrize("l_sq,shift,tol", [(0.05 ** 2, 0.0, 1e-8), (0.5 ** 2, 0.0, FTOL), (9.0, 0.4, FTOL), (9.0, 30.0, FTOL)])
def test_dense_mfma_exp_regimes(gp, oracle, l_sq, shift, tol):
    """The register-tile kernel picks its exponential per patch: the degree-7 polynomial when the patch extent proves
    |c| d^2 <= 2^-5 for every Gram (resp. grid) argument, the table-driven exp otherwise.  Short length scale -> table
    everywhere; l = 0.5 -> polynomial Gram, table grid (|c| (res/2 + |x| + r)^2 > 2^-5); patches far from the origin
    of their frame -> polynomial Gram, table grid; defaults are polynomial everywhere (other tests)."""
    capi, ctx = gp
    res, sz = 0.15, 20
    off, x0, x1, y = synth.make_patches(5, 200, seed=33, ragged=True)
    x0, x1 = x0 + shift, x1 - shift
    kw = dict(sigmaf_sq=0.5, l_sq=l_sq, noise=1e-3)
    p = capi.default_params_dense(**kw)
    po = oracle.dense_params(kw["sigmaf_sq"], kw["l_sq"], kw["noise"])
    xs0, xs1 = oracle.grid(res, sz)
    f1, st1 = ctx.dense_fit_predict_grid(p, off, x0, x1, y, res, sz)
    assert ctx.last_dense_kernel().startswith("dense_mfma")
    f2, _, st2 = ctx.dense_fit_predict(p, off, x0, x1, y, xs0, xs1)
    fo, _, so = oracle.dense_fit_predict_batch(po, off, x0, x1, y, xs0, xs1)
    assert np.all(st1 == 0) and np.all(st2 == 0) and np.all(so == 0)
    _close(f1, fo, tol)
    _close(f2, fo, tol)


def test_dense_edge_cases(gp, oracle):
    capi, ctx = gp
    xs0, xs1 = synth.grid(0.15, 5)
    p = capi.default_params_dense(want_variance=1)
    # P == 0
    f, v, st = ctx.dense_fit_predict(p, np.zeros(1, np.int32), np.zeros(0), np.zeros(0), np.zeros((1, 0)), xs0, xs1)
    assert f.shape == (0, 1, 25)
    # empty patches (n == 0) between real ones, and a single-point patch
    off = np.array([0, 0, 1, 1, 8, 8], dtype=np.int32)
    rng = np.random.default_rng(0)
    x0, x1 = rng.uniform(-0.07, 0.07, 8), rng.uniform(-0.07, 0.07, 8)
    y = rng.normal(0, 0.01, (1, 8))
    f, v, st = ctx.dense_fit_predict(p, off, x0, x1, y, xs0, xs1)
    fo, vo, so = oracle.dense_fit_predict_batch(oracle.dense_params(), off, x0, x1, y, xs0, xs1, variance=True)
    assert np.array_equal(st, so) and np.all(st == 0)
    assert np.all(f[[0, 2, 4]] == 0) and np.all(v[[0, 2, 4]] == p.sigmaf_sq)   # prior mean / prior variance
    _close(f, fo, FTOL)
    assert np.max(np.abs(v - vo)) <= VTOL
    # not SPD: duplicated point, zero noise -> status 1, NaN outputs (the oracle does the same)
    p0 = capi.default_params_dense(noise=0.0)
    off = np.array([0, 3, 6], dtype=np.int32)
    x0 = np.array([0.01, 0.01, 0.02, 0.0, 0.03, -0.02])
    x1 = np.array([0.0, 0.0, 0.03, 0.01, -0.01, 0.02])
    y = np.array([[1.0, 2.0, 3.0, 0.1, 0.2, 0.3]])
    f, v, st, al = ctx.dense_fit_predict(p0, off, x0, x1, y, xs0, xs1, want_alpha=True)
    fo, vo, so = oracle.dense_fit_predict_batch(oracle.dense_params(sigman_sq=0.0), off, x0, x1, y, xs0, xs1)
    assert st.tolist() == so.tolist() == [1, 0]
    assert np.all(np.isnan(f[0])) and np.all(np.isnan(al[0, :3])) and np.all(np.isfinite(f[1]))


@pytest.mark.parametrize("want_var", [0, 1])
def test_dense_one_wave_kernel_edge_cases(gp, oracle, monkeypatch, want_var):
    """The one-wave-per-patch kernel (dense_mfma_w1.hip: the depth plane of a batch whose largest patch has 193 .. 256 points) on a
    batch that mixes every tile count 1 .. 16 with sizes on and next to tile boundaries, empty patches, a single point, and a patch
    that is not SPD (duplicated point under zero noise: the failing pivot sits in the third tile column, the patches around it must
    not notice); mean-only and with the predictive variance (factor export + dense_variance_kernel)."""
    capi, ctx = gp
    monkeypatch.setenv("GPC_W1_MIN_P", "2")           # (production: batches of at least four patches per CU)
    res, sz = 0.15, 12
    sizes = [256, 0, 1, 15, 16, 17, 31, 33, 48, 64, 65, 80, 100, 112, 128, 129, 150, 176, 192, 193, 200, 208, 224, 239, 240, 241, 255, 256, 0, 7]
    off, x0, x1, y = _mixed_batch(sizes, seed=5)
    xs0, xs1 = oracle.grid(res, sz)
    p = capi.default_params_dense(want_variance=want_var)
    f, v, st, al = ctx.dense_fit_predict(p, off, x0, x1, y, xs0, xs1, want_alpha=True)
    assert ctx.last_dense_kernel() == ("dense_mfma_w1 + dense_variance" if want_var else "dense_mfma_w1")
    fo, vo, so, ao = oracle.dense_fit_predict_batch(oracle.dense_params(), off, x0, x1, y, xs0, xs1, variance=bool(want_var), want_alpha=True)
    assert np.array_equal(st, so) and np.all(st == 0)
    _close(f, fo, FTOL)
    _close(al, ao, ATOL)
    if want_var:
        assert np.max(np.abs(v - vo)) <= VTOL
    # the grid entry (separable predictive mean) on the same batch
    if not want_var:
        fg, stg = ctx.dense_fit_predict_grid(p, off, x0, x1, y, res, sz)
        assert ctx.last_dense_kernel() == "dense_mfma_w1" and np.all(stg == 0)
        _close(fg, fo, FTOL)
    # launches of 7 patches that reuse the factor slots (GPC_W1_SLOTS; production: 16384) give the same bits
    monkeypatch.setenv("GPC_W1_SLOTS", "7")
    f2, v2, st2, al2 = ctx.dense_fit_predict(p, off, x0, x1, y, xs0, xs1, want_alpha=True)
    monkeypatch.delenv("GPC_W1_SLOTS")
    assert np.array_equal(f2, f) and np.array_equal(al2, al) and np.array_equal(st2, st)
    if want_var:
        assert np.array_equal(v2, v)
    # not SPD in the middle of the batch: a duplicated point under zero noise (short length scale, so that the neighbours -- and the
    # rest of this patch's Gram matrix -- stay well conditioned without a noise term); the failing pivot is in the third tile column
    kw0 = dict(sigmaf_sq=1.0, l_sq=0.01 ** 2, noise=0.0)
    p0 = capi.default_params_dense(want_variance=want_var, **kw0)
    off3, x03, x13, y3 = _mixed_batch([200, 250, 256], seed=6)
    x03[off3[1] + 40] = x03[off3[1] + 35]
    x13[off3[1] + 40] = x13[off3[1] + 35]
    f3, v3, st3, al3 = ctx.dense_fit_predict(p0, off3, x03, x13, y3, xs0, xs1, want_alpha=True)
    fo3, vo3, so3 = oracle.dense_fit_predict_batch(oracle.dense_params(kw0["sigmaf_sq"], kw0["l_sq"], 0.0), off3, x03, x13, y3, xs0, xs1,
                                                   variance=bool(want_var))
    assert ctx.last_dense_kernel().startswith("dense_mfma_w1")
    assert st3.tolist() == so3.tolist() == [0, 1, 0]
    assert np.all(np.isnan(f3[1])) and np.all(np.isnan(al3[0, off3[1]:off3[2]])) and np.all(np.isfinite(f3[[0, 2]]))
    if want_var:
        assert np.all(np.isnan(v3[1])) and np.all(np.isfinite(v3[[0, 2]]))
    _close(f3[[0, 2]], fo3[[0, 2]], 1e-7)          # (zero noise: conditioned by the closest pairs of points)


def test_dense_one_wave_kernel_512_instance(gp, oracle, monkeypatch):
    """Round 4: the one-wave kernel's 512-point instance (dense_w1_kernel<512>: the depth plane of batches whose largest patch has
    257 .. 512 points -- BASELINE config 3, and the ragged batches of a cloud cut for 256-point patches, which the size-class split dealt to
    three kernels).  A batch that mixes every tile count 1 .. 32 with sizes on and next to tile boundaries, empty patches, a single point;
    against the oracle (f* and the weights), grid and point-wise entries; against the tiled kernel path it replaces (GPC_NO_W1_512); slot
    reuse gives the same bits; a non-SPD patch in the middle of the batch (failing pivot in tile column 20) leaves its neighbours alone."""
    capi, ctx = gp
    monkeypatch.setenv("GPC_W1_MIN_P", "2")
    res, sz = 0.15, 12
    sizes = [512, 0, 1, 16, 17, 255, 256, 257, 272, 273, 288, 300, 320, 321, 352, 383, 384, 385, 400, 416, 447, 448, 449, 480, 496, 497, 511, 512, 0, 130, 64]
    off, x0, x1, y = _mixed_batch(sizes, seed=15)
    xs0, xs1 = oracle.grid(res, sz)
    p = capi.default_params_dense()
    f, _, st, al = ctx.dense_fit_predict(p, off, x0, x1, y, xs0, xs1, want_alpha=True)
    assert ctx.last_dense_kernel() == "dense_mfma_w1_512"
    fo, _, so, ao = oracle.dense_fit_predict_batch(oracle.dense_params(), off, x0, x1, y, xs0, xs1, want_alpha=True)
    assert np.array_equal(st, so) and np.all(st == 0)
    _close(f, fo, FTOL)
    _close(al, ao, ATOL)
    fg, stg = ctx.dense_fit_predict_grid(p, off, x0, x1, y, res, sz)
    assert ctx.last_dense_kernel() == "dense_mfma_w1_512" and np.all(stg == 0)
    _close(fg, fo, FTOL)
    monkeypatch.setenv("GPC_W1_SLOTS", "5")
    f2, _, st2, al2 = ctx.dense_fit_predict(p, off, x0, x1, y, xs0, xs1, want_alpha=True)
    monkeypatch.delenv("GPC_W1_SLOTS")
    assert np.array_equal(f2, f) and np.array_equal(al2, al) and np.array_equal(st2, st)
    monkeypatch.setenv("GPC_NO_W1_512", "1")
    f3, _, st3, al3 = ctx.dense_fit_predict(p, off, x0, x1, y, xs0, xs1, want_alpha=True)
    monkeypatch.delenv("GPC_NO_W1_512")
    assert "w1_512" not in ctx.last_dense_kernel() and np.array_equal(st3, st)
    _close(f3, f, FTOL)
    # the variance still goes the tiled kernel's way above 256 points
    pv = capi.default_params_dense(want_variance=1)
    fv, vv, stv = ctx.dense_fit_predict(pv, off, x0, x1, y, xs0, xs1)
    assert ctx.last_dense_kernel().endswith("dense_variance_big") and np.all(stv == 0)
    _close(fv, fo, FTOL)
    # not SPD: a duplicated point under zero noise, failing pivot at point 330 (tile column 20)
    kw0 = dict(sigmaf_sq=1.0, l_sq=0.006 ** 2, noise=0.0)
    p0 = capi.default_params_dense(**kw0)
    off4, x04, x14, y4 = _mixed_batch([400, 500, 512], seed=16)
    x04[off4[1] + 330] = x04[off4[1] + 35]
    x14[off4[1] + 330] = x14[off4[1] + 35]
    f4, _, st4, al4 = ctx.dense_fit_predict(p0, off4, x04, x14, y4, xs0, xs1, want_alpha=True)
    fo4, _, so4 = oracle.dense_fit_predict_batch(oracle.dense_params(kw0["sigmaf_sq"], kw0["l_sq"], 0.0), off4, x04, x14, y4, xs0, xs1)
    assert ctx.last_dense_kernel() == "dense_mfma_w1_512"
    # (the oracle tests the pivot against 0: whether the duplicate leaves +1e-17 or -1e-17 there is luck; the kernels' threshold is relative)
    assert st4.tolist() == [0, 1, 0] and so4[0] == 0 and so4[2] == 0
    assert np.all(np.isnan(f4[1])) and np.all(np.isnan(al4[0, off4[1]:off4[2]])) and np.all(np.isfinite(f4[[0, 2]]))
    _close(f4[[0, 2]], fo4[[0, 2]], 1e-7)


@pytest.mark.parametrize("l_sq,shift,tol", [(0.05 ** 2, 0.0, 1e-8), (0.5 ** 2, 0.0, FTOL), (9.0, 0.4, FTOL), (9.0, 30.0, FTOL)])
def test_dense_one_wave_kernel_exp_regimes(gp, oracle, monkeypatch, l_sq, shift, tol):
    """The exponential regimes of test_dense_mfma_exp_regimes on the one-wave kernel (patches of up to 256 points): table-driven
    Gram tiles and grid factors, polynomial Gram with table-driven grid, polynomial everywhere -- and the variance kernel's own
    small-argument test on the same patches."""
    capi, ctx = gp
    monkeypatch.setenv("GPC_W1_MIN_P", "2")
    res, sz = 0.15, 20
    off, x0, x1, y = synth.make_patches(6, 256, seed=34, ragged=True, n_min=150)
    x0, x1 = x0 + shift, x1 - shift
    kw = dict(sigmaf_sq=0.5, l_sq=l_sq, noise=1e-3)
    po = oracle.dense_params(kw["sigmaf_sq"], kw["l_sq"], kw["noise"])
    xs0, xs1 = oracle.grid(res, sz)
    f1, st1 = ctx.dense_fit_predict_grid(capi.default_params_dense(**kw), off, x0, x1, y, res, sz)
    assert ctx.last_dense_kernel() == "dense_mfma_w1"
    f2, v2, st2 = ctx.dense_fit_predict(capi.default_params_dense(want_variance=1, **kw), off, x0, x1, y, xs0, xs1)
    assert ctx.last_dense_kernel() == "dense_mfma_w1 + dense_variance"
    fo, vo, so = oracle.dense_fit_predict_batch(po, off, x0, x1, y, xs0, xs1, variance=True)
    assert np.all(st1 == 0) and np.all(st2 == 0) and np.all(so == 0)
    _close(f1, fo, tol)
    _close(f2, fo, tol)
    assert np.max(np.abs(v2 - vo)) <= (1e-9 if tol > FTOL else 1e-10)


def test_dense_batch_size_rule(gp, oracle, monkeypatch):
    """Depth plane, n <= 256: batches of at least four patches per CU go to the one-wave-per-patch kernel, smaller ones to the
    register-tile kernel (eight waves per patch: the better latency when the chip is not full); both agree with the oracle."""
    capi, ctx = gp
    for e in ("GPC_W1_MIN_P", "GPC_NO_W1", "GPC_W2", "GPC_FORCE_BIG", "GPC_FORCE_GENERIC"):
        monkeypatch.delenv(e, raising=False)
    res, sz = 0.15, 8
    xs0, xs1 = oracle.grid(res, sz)
    for P, n, want in ((1100, 96, "dense_mfma_w1"), (40, 96, "dense_mfma_nt8"), (1030, 20, "dense_mfma_w1")):
        off, x0, x1, y = synth.make_patches(P, n, seed=P, ragged=True)
        f, st = ctx.dense_fit_predict_grid(capi.default_params_dense(), off, x0, x1, y, res, sz)
        assert ctx.last_dense_kernel() == want, ctx.last_dense_kernel()
        pick = np.arange(0, P, max(1, P // 24))
        sub = np.concatenate([[0], np.cumsum(np.diff(off)[pick])]).astype(np.int32)
        idx = np.concatenate([np.arange(off[i], off[i + 1]) for i in pick])
        fo, _, so = oracle.dense_fit_predict_batch(oracle.dense_params(), sub, x0[idx], x1[idx], y[:, idx], xs0, xs1)
        assert np.all(st == 0)
        _close(f[pick], fo, FTOL)


ROUTE_SWITCHES = ("GPC_FORCE_GENERIC", "GPC_FORCE_BIG", "GPC_NO_W1", "GPC_NO_W1_512", "GPC_W2", "GPC_W1_MIN_P", "GPC_W1_SLOTS", "GPC_NO_SPLIT",
                  "GPC_NO_NT17", "GPC_NO_HINT", "GPC_BIG_NO_W2", "GPC_BIG_NO_W4")


@pytest.mark.parametrize("switch,P,n,ny,ragged,var", [
    ("", 40, 17, 1, True, False), ("", 9, 64, 3, True, False), ("", 12, 200, 1, True, False), ("", 5, 256, 1, False, False),
    ("", 8, 270, 1, True, False), ("", 6, 300, 1, True, False), ("", 6, 300, 3, True, False), ("", 2, 512, 1, False, False),
    ("", 7, 200, 1, True, True), ("GPC_W1_MIN_P", 7, 256, 1, False, True),
    ("GPC_W1_MIN_P", 2, 256, 1, False, False), ("GPC_W1_MIN_P", 9, 64, 1, True, False), ("GPC_W1_MIN_P", 3, 512, 1, False, False),
    ("GPC_W1_MIN_P", 6, 300, 1, True, False), ("GPC_NO_W1", 5, 256, 1, True, False), ("GPC_NO_SPLIT", 6, 300, 1, True, False),
    ("GPC_NO_SPLIT", 8, 270, 1, True, False), ("GPC_FORCE_BIG", 12, 200, 1, True, False), ("GPC_FORCE_BIG", 4, 300, 3, True, False)])
def test_dense_route_is_what_launches(gp, monkeypatch, switch, P, n, ny, ragged, var):
    """The rule that chooses the kernels of a batch is a pure function (csrc/dense_route.h; its edges: test_dense_route_cpu.py).  This ties
    it to the dispatcher: for a real call, the kernel name the context reports is the name the function gives for the same facts under
    the same environment."""
    import torch
    capi, ctx = gp
    for e in ROUTE_SWITCHES:
        monkeypatch.delenv(e, raising=False)
    if switch:
        monkeypatch.setenv(switch, "2" if switch == "GPC_W1_MIN_P" else "1")
    off, x0, x1, y = synth.make_patches(P, n, seed=100 + P + n, ragged=ragged, ny=ny)
    xs0, xs1 = synth.grid(0.15, 6)
    f, v, st = ctx.dense_fit_predict(capi.default_params_dense(want_variance=int(var)), off, x0, x1, y, xs0, xs1)
    assert np.all(st == 0) and np.all(np.isfinite(f)) and (not var or np.all(np.isfinite(v)))
    kind, name, _ = capi.dense_route(P, int(np.max(np.diff(off))), n_total=int(off[-1]), ny=ny, m=xs0.shape[0], variance=var, pointwise=True,
                                     num_cus=torch.cuda.get_device_properties(0).multi_processor_count)
    assert name and kind not in ("nothing", "no route")
    assert ctx.last_dense_kernel() == name, (ctx.last_dense_kernel(), kind, name)


def test_dense_big_kernel_edge_cases(gp, oracle, monkeypatch):
    """The tiled left-looking kernel (n_max > 256; GPC_NO_SPLIT keeps the whole batch on it) on a batch that mixes an empty patch, a tiny patch, a patch that is not
    SPD (duplicated point, zero noise: the failing pivot sits in a late tile column) and full-size patches; grid and
    point-wise entries, ny = 3."""
    capi, ctx = gp
    monkeypatch.setenv("GPC_NO_SPLIT", "1")
    res, sz = 0.15, 8
    xs0, xs1 = oracle.grid(res, sz)
    rng = np.random.default_rng(5)
    counts = [300, 0, 5, 290, 513, 17]
    off = np.concatenate([[0], np.cumsum(counts)]).astype(np.int32)
    N = int(off[-1])
    x0, x1 = rng.uniform(-res / 2, res / 2, N), rng.uniform(-res / 2, res / 2, N)
    y = rng.normal(0, 0.01, (3, N))
    # patch 3: point 280 duplicates point 11 -> with zero noise the Gram matrix is singular at pivot 280 (tile column 17)
    x0[off[3] + 280], x1[off[3] + 280] = x0[off[3] + 11], x1[off[3] + 11]
    # l = 4 mm against a ~9 mm point spacing: K is far from singular without noise, except for the duplicate
    p0 = capi.default_params_dense(noise=0.0, sigmaf_sq=1.0, l_sq=0.004 ** 2)
    po = oracle.dense_params(1.0, 0.004 ** 2, 0.0)
    f, _, st, al = ctx.dense_fit_predict(p0, off, x0, x1, y, xs0, xs1, want_alpha=True)
    assert ctx.last_dense_kernel() == "dense_mfma_big"
    fo, _, so, ao = oracle.dense_fit_predict_batch(po, off, x0, x1, y, xs0, xs1, want_alpha=True)
    assert st.tolist() == so.tolist() == [0, 0, 0, 1, 0, 0]
    assert np.all(np.isnan(f[3])) and np.all(f[1] == 0)
    good = [0, 2, 4, 5]
    for i in good:
        assert np.max(np.abs(f[i] - fo[i])) <= 1e-8 * max(np.max(np.abs(fo[i])), 1e-12), i
    f2, st2 = ctx.dense_fit_predict_grid(p0, off, x0, x1, y, res, sz)
    assert st2.tolist() == st.tolist()
    for i in good:
        assert np.max(np.abs(f2[i] - f[i])) <= 1e-9 * max(np.max(np.abs(f[i])), 1e-12)


def test_dense_size_class_split(gp, oracle, monkeypatch):
    """A ragged batch whose largest patch exceeds 256 points is sorted into size classes on the device: patches of up to
    256 points run on the register-resident kernel, only the larger ones on the tiled kernel.  Same results as the oracle,
    and per kernel the same as when it runs alone; empty patches, a non-SPD patch in each class, status per patch."""
    capi, ctx = gp
    res, sz = 0.15, 10
    rng = np.random.default_rng(17)
    counts = np.concatenate([rng.integers(1, 257, 40), rng.integers(257, 700, 25), [0, 256, 257, 1, 1024, 0, 260, 265, 272, 273]])
    rng.shuffle(counts)
    off = np.concatenate([[0], np.cumsum(counts)]).astype(np.int32)
    P, N = len(counts), int(off[-1])
    x0, x1 = rng.uniform(-res / 2, res / 2, N), rng.uniform(-res / 2, res / 2, N)
    y = rng.normal(0, 0.01, (1, N))
    small = int(np.flatnonzero((counts > 40) & (counts <= 256))[0])
    mid = int(np.flatnonzero(counts == 265)[0])         # the NT = 17 class (256 < n <= 272)
    big = int(np.flatnonzero(counts > 300)[0])
    for i in (small, mid, big):                 # a duplicated point: singular without noise
        x0[off[i] + 30], x1[off[i] + 30] = x0[off[i] + 3], x1[off[i] + 3]
    p0 = capi.default_params_dense(noise=0.0, sigmaf_sq=1.0, l_sq=0.003 ** 2)
    po = oracle.dense_params(1.0, 0.003 ** 2, 0.0)
    f, st = ctx.dense_fit_predict_grid(p0, off, x0, x1, y, res, sz)
    assert ctx.last_dense_kernel() == "dense_mfma_nt16 + dense_mfma_nt17 + dense_mfma_big"
    xs0, xs1 = oracle.grid(res, sz)
    fo, _, so = oracle.dense_fit_predict_batch(po, off, x0, x1, y, xs0, xs1)
    assert st.tolist() == so.tolist() and st[small] == 1 and st[mid] == 1 and st[big] == 1 and st.sum() == 3
    for i in range(P):
        if st[i] == 0:
            assert np.max(np.abs(f[i] - fo[i])) <= 1e-8 * max(np.max(np.abs(fo[i])), 1e-12), (i, counts[i])
        else:
            assert np.all(np.isnan(f[i]))
    assert np.all(f[counts == 0] == 0)
    # the tiled kernel alone on the same batch: patches of the large class are bit-identical (same kernel, same arithmetic)
    monkeypatch.setenv("GPC_NO_SPLIT", "1")
    f1, st1 = ctx.dense_fit_predict_grid(p0, off, x0, x1, y, res, sz)
    assert ctx.last_dense_kernel() == "dense_mfma_big" and st1.tolist() == st.tolist()
    ok_big = (counts > 256) & (st == 0)
    assert np.max(np.abs(f[ok_big] - f1[ok_big])) <= 1e-10 * np.max(np.abs(f1[ok_big]))


@pytest.mark.parametrize("P,lo,hi", [(1, 384, 384), (1, 273, 273), (12, 273, 384), (9, 300, 512)])
def test_dense_tiled_shapes_agree(gp, oracle, monkeypatch, P, lo, hi):
    """The tiled kernel has two shapes: four waves and two patches per CU for the depth plane up to 384 points (the producer's
    273 .. 324-point class), eight waves and one patch per CU above.  Both against the oracle on the sizes in between, and against
    each other (GPC_BIG_NO_W4 forces the 8-wave shape): same arithmetic in the same order, so they agree far below the tolerance."""
    capi, ctx = gp
    res, sz = 0.15, 12
    rng = np.random.default_rng(7 * P + lo)
    counts = rng.integers(lo, hi + 1, P)
    off = np.concatenate([[0], np.cumsum(counts)]).astype(np.int32)
    N = int(off[-1])
    x0, x1 = rng.uniform(-res / 2, res / 2, N), rng.uniform(-res / 2, res / 2, N)
    y = 0.01 * np.sin(25 * x0) * np.cos(15 * x1) + rng.normal(0, 0.003, N)
    y = (y - np.mean(y))[None, :]
    prm = capi.default_params_dense()
    xs0, xs1 = oracle.grid(res, sz)
    monkeypatch.setenv("GPC_FORCE_BIG", "1")
    f, st, al = ctx.dense_fit_predict_grid(prm, off, x0, x1, y, res, sz, want_alpha=True)
    assert ctx.last_dense_kernel() == "dense_mfma_big"
    monkeypatch.setenv("GPC_BIG_NO_W4", "1")
    f8, st8, al8 = ctx.dense_fit_predict_grid(prm, off, x0, x1, y, res, sz, want_alpha=True)
    fo, _, so, ao = oracle.dense_fit_predict_batch(oracle.dense_params(), off, x0, x1, y, xs0, xs1, want_alpha=True)
    assert np.all(st == 0) and np.all(st8 == 0) and np.all(so == 0)
    for ff, aa in ((f, al), (f8, al8)):
        _close(ff, fo, FTOL)
        _close(aa, ao, ATOL)
    _close(f, f8, 1e-12)


@pytest.mark.parametrize("P,lo,hi", [(1, 272, 272), (1, 257, 257), (24, 257, 272), (40, 200, 272)])
def test_dense_nt17_shape(gp, oracle, monkeypatch, P, lo, hi):
    """Patches of 257 .. 272 points (what the octree leaves of a cloud cut for 256-point patches mostly are) stay on the
    register-resident kernel in its NT = 17 shape (depth plane only).  Oracle parity for grid and point-wise entries and alpha; the
    tiled kernel on the same batch (GPC_NO_NT17) agrees to its own tolerance; three channels still take the tiled kernel."""
    capi, ctx = gp
    res, sz = 0.15, 20
    rng = np.random.default_rng(100 + P + lo)
    counts = rng.integers(lo, hi + 1, P)
    off = np.concatenate([[0], np.cumsum(counts)]).astype(np.int32)
    N = int(off[-1])
    x0, x1 = rng.uniform(-res / 2, res / 2, N), rng.uniform(-res / 2, res / 2, N)
    y = 0.01 * np.sin(30 * x0) * np.cos(20 * x1) + rng.normal(0, 0.003, N)
    y = (y - np.mean(y))[None, :]
    prm = capi.default_params_dense()
    xs0, xs1 = oracle.grid(res, sz)
    f, st, al = ctx.dense_fit_predict_grid(prm, off, x0, x1, y, res, sz, want_alpha=True)
    name = ctx.last_dense_kernel()
    assert name == ("dense_mfma_nt17" if P == 1 else "dense_mfma_nt16 + dense_mfma_nt17"), name
    fo, _, so, ao = oracle.dense_fit_predict_batch(oracle.dense_params(), off, x0, x1, y, xs0, xs1, want_alpha=True)
    assert np.all(st == 0) and np.all(so == 0)
    _close(f, fo, FTOL)
    _close(al, ao, ATOL)
    f2, _, st2 = ctx.dense_fit_predict(prm, off, x0, x1, y, xs0, xs1)
    _close(f2, fo, FTOL)
    monkeypatch.setenv("GPC_NO_NT17", "1")
    f3, st3 = ctx.dense_fit_predict_grid(prm, off, x0, x1, y, res, sz)
    assert "nt17" not in ctx.last_dense_kernel()
    _close(f3, f, 1e-10)
    monkeypatch.delenv("GPC_NO_NT17")
    if P > 1:
        y3 = np.concatenate([y, 2 * y, -y], axis=0)
        f4, st4 = ctx.dense_fit_predict_grid(prm, off, x0, x1, y3, res, sz)
        assert ctx.last_dense_kernel() == "dense_mfma_nt16 + dense_mfma_big"
        _close(f4[:, 0, :], fo[:, 0, :], FTOL)
    # stale-LDS check of the new shape: NaN poison in every CU's LDS before the call
    monkeypatch.setenv("GPC_POISON_LDS", "1")
    f5, st5 = ctx.dense_fit_predict_grid(prm, off, x0, x1, y, res, sz)
    monkeypatch.delenv("GPC_POISON_LDS")
    assert np.all(st5 == 0)
    _close(f5, fo, FTOL)


def test_dense_argument_errors(gp):
    capi, ctx = gp
    xs0, xs1 = synth.grid(0.15, 4)
    off, x0, x1, y = synth.make_patches(2, 8, seed=1)
    p = capi.default_params_dense()
    with pytest.raises(capi.GpcError) as e:
        ctx.dense_fit_predict(p, off, x0, x1, np.concatenate([y, y]), xs0, xs1)      # ny == 2
    assert e.value.code == capi.GPC_EINVAL
    with pytest.raises(capi.GpcError) as e:
        ctx.dense_fit_predict(p, np.array([0, 5, 3], np.int32), x0, x1, y, xs0, xs1)  # decreasing offsets
    assert e.value.code == capi.GPC_EINVAL
    big = synth.make_patches(1, 1100, seed=1)
    with pytest.raises(capi.GpcError) as e:
        ctx.dense_fit_predict(p, big[0], big[1], big[2], big[3], xs0, xs1)
    assert e.value.code == capi.GPC_ERANGE
    with pytest.raises(capi.GpcError) as e:
        ctx.dense_fit_predict(capi.default_params_dense(l_sq=0.0), off, x0, x1, y, xs0, xs1)
    assert e.value.code == capi.GPC_EINVAL


@pytest.mark.parametrize("n,ny", [(100, 1), (256, 1), (256, 3), (300, 1)])
def test_dense_grid_entry_matches_pointwise(gp, oracle, n, ny):
    """gpc_dense_fit_predict_grid builds the grid of gp_compressor.cpp:317-332 itself; results equal the point-wise entry."""
    capi, ctx = gp
    off, x0, x1, y = synth.make_patches(7, n, seed=21, ragged=True, ny=ny)
    res, sz = 0.15, 20
    xs0, xs1 = oracle.grid(res, sz)
    p = capi.default_params_dense()
    f1, _, st1 = ctx.dense_fit_predict(p, off, x0, x1, y, xs0, xs1)
    f2, st2 = ctx.dense_fit_predict_grid(p, off, x0, x1, y, res, sz)
    fo, _, so = oracle.dense_fit_predict_batch(oracle.dense_params(), off, x0, x1, y, xs0, xs1)
    assert np.array_equal(st1, st2) and np.all(st1 == 0)
    _close(f2, f1, 1e-11)
    _close(f2, fo, FTOL)


GRID_BATCHES = (([256, 0, 1, 100, 37], 1), ([512, 17, 300, 0], 1), ([200, 0, 64, 5], 3), ([300, 40, 0], 3))
GRID_REGIMES = ((DEFAULT, FTOL), (SHORT, 1e-8))      # polynomial everywhere | table-driven (test_dense_mfma_exp_regimes' bound)
_GRID_REF = {}


def _grid_case(oracle, b, r, sz):
    """Batch b of GRID_BATCHES and the oracle's fit of it under regime r on oracle.grid(res, sz): computed once, never written to."""
    if (b, r, sz) not in _GRID_REF:
        sizes, ny = GRID_BATCHES[b]
        batch = with_planes(*_mixed_batch(sizes, seed=120 + b), ny=ny, seed=130 + b)
        xs0, xs1 = oracle.grid(0.15, sz)
        fo, _, so = oracle.dense_fit_predict_batch(oracle.dense_params(*GRID_REGIMES[r][0]), *batch, xs0, xs1)
        for a in batch + (xs0, xs1, fo, so):
            a.setflags(write=False)
        _GRID_REF[(b, r, sz)] = (batch, xs0, xs1, fo, so)
    return _GRID_REF[(b, r, sz)]


@pytest.mark.parametrize("sz", [1, 2, 15, 16, 17, 31, 32, 33, 40])
def test_dense_grid_sizes(gp, oracle, kernel_choice, sz):
    """The separable-grid predictive mean of every kernel at the grid sizes where it changes path: a single cell (one stored value out
    of the 32 x 32 the MFMA tiles hold; the one-wave kernel evaluates the other rows far outside the polynomial's range and must not
    store them), one output tile and the 16 | 17 edge, a full second tile (31, 32), and the per-point loop above 32 (33, 40).  Four small
    batches (one-wave kernel and its 512-point instance, register-tile kernel with three planes, the size-class split with three planes;
    empty and tiny patches in each), polynomial and table-driven exponential.  Against the oracle on oracle.grid(res, sz) and against
    the point-wise entry on the same points.
    Measured on MI355X, worst over every kernel choice, size and batch: 4.5e-12 (defaults) and 1.9e-12 (short length scale) against the
    oracle.  Against the point-wise entry the worst of each of four runs was 4.0e-12, 3.1e-12, 3.5e-12, 4.0e-12, every time at sz = 1
    under the defaults on a kernel whose solves are not bit-reproducible (the tiled and the register-tile kernel: 2.9e-12 .. 4.0e-12 on
    the three batches they take): the two calls are two fits, and a single cell leaves no other value to set the scale.  Everything else
    stayed below 1.9e-12 in all four runs: every sz > 1, the short length scale, and the one-wave and generic kernels at sz = 1
    (1.5e-12).  So up to about 4e-12 at sz = 1 on those kernels is noise; a gap of that size anywhere else is not."""
    capi, ctx = gp
    res = 0.15
    # per batch: the exact name under the normal dispatch (the register-tile kernel by prefix: its tile count is in the name), a prefix
    # under every forced choice -- test_dense_vs_oracle's expectations for these shapes
    split = "dense_mfma_nt16 + dense_mfma_big"
    want = {"dispatch": ("dense_mfma_w1", "dense_mfma_w1_512", "dense_mfma_nt", split),
            "reg": ("dense_mfma_nt", "dense_mfma_nt16 + ", "dense_mfma_nt", split),
            "w2": ("dense_mfma_big_w2", "dense_mfma_nt16 + ", "dense_mfma_nt", split),
            "generic": ("dense_generic",) * 4, "big": ("dense_mfma_big",) * 4, "big_w4": ("dense_mfma_big",) * 4}[kernel_choice]
    for r, (regime, tol) in enumerate(GRID_REGIMES):
        p = capi.default_params_dense(sigmaf_sq=regime[0], l_sq=regime[1], noise=regime[2])
        for b in range(len(GRID_BATCHES)):
            batch, xs0, xs1, fo, so = _grid_case(oracle, b, r, sz)
            f, st = ctx.dense_fit_predict_grid(p, *batch, res, sz)
            name = ctx.last_dense_kernel()
            assert name == want[b] if (kernel_choice == "dispatch" and b != 2) else name.startswith(want[b]), (kernel_choice, b, name)
            assert f.shape == (len(GRID_BATCHES[b][0]), GRID_BATCHES[b][1], sz * sz)
            assert np.all(st == 0) and np.all(so == 0)
            f2, _, st2 = ctx.dense_fit_predict(p, *batch, xs0, xs1)
            assert np.all(st2 == 0)
            ef, e2 = float(np.max(np.abs(f - fo))) / float(np.max(np.abs(fo))), float(np.max(np.abs(f - f2))) / float(np.max(np.abs(f2)))
            print("sz=%d %s batch %d regime %d (%s): |f - f_o| = %.2e, |f - f_pointwise| = %.2e" % (sz, kernel_choice, b, r, name, ef, e2))
            _close(f, fo, tol)
            _close(f, f2, 1e-11)


def test_dense_device_pointers_on_torch_stream(gp, oracle):
    import torch
    capi, ctx = gp
    dev = torch.device("cuda:0")
    off, x0, x1, y = synth.make_patches(33, 128, seed=8, ragged=True)
    xs0, xs1 = synth.grid(0.15, 20)
    P, N, m = 33, int(off[-1]), 400
    t = lambda a: torch.from_numpy(a).to(dev)
    d_off, d_x0, d_x1, d_y, d_xs0, d_xs1 = t(off), t(x0), t(x1), t(y), t(xs0), t(xs1)
    f = torch.full((P, 1, m), float("nan"), dtype=torch.float64, device=dev)
    st = torch.full((P,), -1, dtype=torch.int32, device=dev)
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        ctx.set_stream(side.cuda_stream)
        ctx.dense_fit_predict_dev(capi.default_params_dense(), P, d_off, 128, N, d_x0, d_x1, d_y, 1, m, d_xs0, d_xs1, f,
                                  status=st)
    side.synchronize()
    ctx.set_stream(None)
    fo, _, so = oracle.dense_fit_predict_batch(oracle.dense_params(), off, x0, x1, y, xs0, xs1)
    assert np.all(st.cpu().numpy() == 0)
    _close(f.cpu().numpy(), fo, FTOL)


@pytest.mark.parametrize("P,n,label", [(8192, 256, "C2"), (8192, 512, "C3 (one GPU's share of 65536 patches)"), (4096, 1024, "C5")])
def test_dense_full_size_properties(gp, oracle, P, n, label):
    """BASELINE configs 2, 3 and 5 at their full per-GPU size (m = 400): size-independent properties (linearity in y,
    the normal equations through alpha on a sample) plus the oracle on a random sample of patches."""
    capi, ctx = gp
    res, sz = 0.15, 20
    off, x0, x1, y = synth.make_patches(P, n, res=res, seed=2)
    rng = np.random.default_rng(99)
    y2 = rng.normal(0, 0.01, size=y.shape)
    p = capi.default_params_dense()
    fa, sta, ala = ctx.dense_fit_predict_grid(p, off, x0, x1, y, res, sz, want_alpha=True)
    assert ctx.last_dense_kernel() == {256: "dense_mfma_w1", 512: "dense_mfma_w1_512", 1024: "dense_mfma_big"}[n], ctx.last_dense_kernel()
    fb, stb = ctx.dense_fit_predict_grid(p, off, x0, x1, y2, res, sz)
    fc, stc = ctx.dense_fit_predict_grid(p, off, x0, x1, y + 2.0 * y2, res, sz)
    assert np.all(sta == 0) and np.all(stb == 0) and np.all(stc == 0)
    assert np.all(np.isfinite(fa))
    # linearity of the posterior mean in the targets
    _close(fc, fa + 2.0 * fb, 1e-10)
    # (K + 2 sn^2 I) alpha = y, checked per patch with an independent NumPy Gram matrix on a sample
    xs0, xs1 = oracle.grid(res, sz)
    sample = rng.choice(P, size=24 if n <= 256 else 6, replace=False)
    for i in sample:
        sl = slice(off[i], off[i + 1])
        X = np.stack([x0[sl], x1[sl]], 1)
        d = X[:, None, :] - X[None, :, :]
        K = 0.0025 * np.exp(-0.5 / 9.0 * (d[..., 0] ** 2 + d[..., 1] ** 2)) + 2 * 0.0016 * np.eye(n)
        assert np.max(np.abs(K @ ala[0, sl] - y[0, sl])) <= 1e-12 * max(1.0, np.max(np.abs(ala[0, sl])))
    sub_off = np.concatenate([[0], np.cumsum([n] * len(sample))]).astype(np.int32)
    idx = np.concatenate([np.arange(off[i], off[i + 1]) for i in sample])
    fo, _, so = oracle.dense_fit_predict_batch(oracle.dense_params(), sub_off, x0[idx], x1[idx], y[:, idx], xs0, xs1)
    _close(fa[sample], fo, FTOL)


def test_dense_headline_kernel_is_bit_reproducible(gp):
    """The one-wave kernel (dense_mfma_w1, the C2 bench path) gives the same bits run after run: a patch is the business of a single
    wave, there is no LDS atomic and no hand-over whose arrival order could enter a sum.  (The register-resident kernel is reproducible
    to a rounding or two only: seven waves add into w_k in arrival order; VERDICT round 2, "weak".)"""
    capi, ctx = gp
    res, sz = 0.15, 20
    off, x0, x1, y = synth.make_patches(2048, 256, res=res, seed=77, ragged=True, n_min=200)
    p = capi.default_params_dense()
    f0, st0, al0 = ctx.dense_fit_predict_grid(p, off, x0, x1, y, res, sz, want_alpha=True)
    assert ctx.last_dense_kernel() == "dense_mfma_w1" and np.all(st0 == 0)
    for _ in range(3):
        f1, st1, al1 = ctx.dense_fit_predict_grid(p, off, x0, x1, y, res, sz, want_alpha=True)
        assert np.array_equal(f1, f0) and np.array_equal(al1, al0) and np.array_equal(st1, st0)


def test_one_wave_kernel_survives_a_refused_workspace(gp, monkeypatch):
    """The one-wave kernel wants one 304 KB factor slot per patch of a launch.  When the device refuses that (GPC_WS_FAIL_ABOVE makes
    gpc_ws_reserve fail like an exhausted device) the batch goes through in smaller launches that reuse fewer slots,
    and below that on the register-resident kernel, which needs no workspace -- same results, never an error for the caller; the
    context keeps a usable workspace afterwards."""
    from gp_compressor_amd import capi as capi_mod
    capi, _ = gp
    ctx = capi_mod.Context(0)                     # own context: the module's may already hold a large workspace
    res, sz = 0.15, 20
    off, x0, x1, y = synth.make_patches(2048, 256, res=res, seed=78, ragged=True, n_min=200)
    p = capi.default_params_dense()
    f0, st0 = ctx.dense_fit_predict_grid(p, off, x0, x1, y, res, sz)
    assert ctx.last_dense_kernel() == "dense_mfma_w1" and np.all(st0 == 0)
    ctx.close()
    slot = 152 * 2048
    for limit, want in ((slot * 1100, "dense_mfma_w1"), (slot * 100, "dense_mfma_nt16")):
        c2 = capi_mod.Context(0)
        monkeypatch.setenv("GPC_WS_FAIL_ABOVE", str(limit))
        monkeypatch.setenv("GPC_W1_MIN_P", "64")
        f1, st1 = c2.dense_fit_predict_grid(p, off, x0, x1, y, res, sz)
        assert c2.last_dense_kernel() == want, c2.last_dense_kernel()
        monkeypatch.delenv("GPC_WS_FAIL_ABOVE")
        assert np.all(st1 == 0) and np.max(np.abs(f1 - f0)) <= 1e-9 * np.max(np.abs(f0))
        f2, st2 = c2.dense_fit_predict_grid(p, off, x0, x1, y, res, sz)      # and the context is whole afterwards
        assert c2.last_dense_kernel() == "dense_mfma_w1" and np.array_equal(f2, f0)
        c2.close()


def test_dense_does_not_read_stale_lds(gp, oracle, monkeypatch):
    """LDS keeps what the previous kernel on the CU left there.  A sparse exact-GP run on duplicated points fills it with
    NaN / Inf; a dense batch whose sizes are not multiples of 32 must not let those leak into its predictive sums (the rows
    between 16 ceil(n / 16) and the next multiple of 32 are never written by the solve; the sums once multiplied them by a
    zero kernel factor instead of skipping them, and a whole patch came out NaN when the sparse tests had run first)."""
    capi, ctx = gp
    res, sz = 0.15, 20
    # 0. the library's own diagnostic: NaN in every LDS word of every CU before each kernel family (GPC_POISON_LDS)
    monkeypatch.setenv("GPC_POISON_LDS", "1")
    # 1. and the sequence that exposed the bug: every CU runs sparse patches whose state degenerates to NaN / Inf (capacity -1, each point added twice)
    Pp = 1024
    off, x0, x1, y = synth.make_patches(Pp, 24, res=res, seed=5)
    g = capi.Sparse(ctx, capi.default_params_sparse(1, sigmaf_sq=1.0, l_sq=(res / 8) ** 2, noise=1e-4, capacity=-1), Pp, 1)
    g.add(off, x0, x1, y)
    g.add(off, x0, x1, y)
    al, C_, Q, BV = g.state()
    assert not np.all(np.isfinite(C_[:, :4, :4]))                      # the poison is there
    # ... and spread over the whole LDS by the kernels that stage C K products of that state in it
    xs0, xs1 = synth.grid(res, sz)
    g.predict(xs0, xs1)
    g.likelihood(off, x0, x1, y)
    g.close()
    # 2. ragged dense batches on the register-resident and on the tiled kernel
    for n_hi, P in ((200, 2048), (400, 1024)):
        off, x0, x1, y = synth.make_patches(P, n_hi, res=res, seed=6, ragged=True, n_min=n_hi // 3)
        p0 = capi.default_params_dense(sigmaf_sq=1.0, l_sq=(res / 4) ** 2, noise=1e-3)
        f, st = ctx.dense_fit_predict_grid(p0, off, x0, x1, y, res, sz)
        assert np.all(st == 0) and np.all(np.isfinite(f))
        xs0, xs1 = oracle.grid(res, sz)
        sel = np.arange(0, P, P // 16)
        soff = np.concatenate([[0], np.cumsum(np.diff(off)[sel])]).astype(np.int32)
        idx = np.concatenate([np.arange(off[i], off[i + 1]) for i in sel])
        fo, _, so = oracle.dense_fit_predict_batch(oracle.dense_params(1.0, (res / 4) ** 2, 1e-3), soff, x0[idx], x1[idx], y[:, idx], xs0, xs1)
        assert np.max(np.abs(f[sel] - fo)) <= 1e-8 * np.max(np.abs(fo))


def test_host_pointer_entry_pipeline_and_pinned_buffers(gp, oracle, monkeypatch):
    """The host-pointer entries cut a batch of >= 2048 patches into four chunks and overlap upload, kernel and download
    (csrc/dense_host.hip, dense_host): a ragged 3-channel batch through the pipeline, through the single-chunk form
    (GPC_HOST_NO_PIPELINE) and from page-locked caller buffers (gpc_host_alloc) gives the same grids, alpha and status; the
    oracle on a sample.  Point-wise X* with the variance goes through the same chunking."""
    capi, ctx = gp
    P, res, sz = 2100, 0.15, 10
    off, x0, x1, y = synth.make_patches(P, 48, res=res, seed=91, ragged=True, ny=3)
    prm = capi.default_params_dense()
    f, st, al = ctx.dense_fit_predict_grid(prm, off, x0, x1, y, res, sz, want_alpha=True)
    monkeypatch.setenv("GPC_HOST_NO_PIPELINE", "1")
    f1, st1, al1 = ctx.dense_fit_predict_grid(prm, off, x0, x1, y, res, sz, want_alpha=True)
    monkeypatch.delenv("GPC_HOST_NO_PIPELINE")
    tol = 1e-12 * np.max(np.abs(f1))                    # the dense kernel's LDS atomics meet in arrival order: equal to an ulp or two
    assert np.all(st == 0) and np.array_equal(st, st1)
    assert np.max(np.abs(f - f1)) <= tol and np.max(np.abs(al - al1)) <= 1e-12 * np.max(np.abs(al1))
    # page-locked caller buffers: transferred in place
    pin = {k: ctx.host_array(a.shape, a.dtype) for k, a in (("off", off), ("x0", x0), ("x1", x1), ("y", y))}
    for k, a in (("off", off), ("x0", x0), ("x1", x1), ("y", y)):
        pin[k][...] = a
    pf = ctx.host_array((P, 3, sz * sz))
    pst = ctx.host_array((P,), np.int32)
    import ctypes as C
    rc = ctx.lib.gpc_dense_fit_predict_grid(ctx.h, C.byref(prm), P, pin["off"].ctypes.data, pin["x0"].ctypes.data, pin["x1"].ctypes.data,
                                            pin["y"].ctypes.data, 3, res, sz, pf.ctypes.data, None, pst.ctypes.data)
    assert rc == 0 and np.all(pst == 0) and np.max(np.abs(pf - f1)) <= tol
    for a in list(pin.values()) + [pf, pst]:
        ctx.free_host_array(a)
    # oracle on a sample of patches from every chunk
    xs0, xs1 = synth.grid(res, sz)
    for i in (0, 524, 525, 1049, 1575, 2099):
        sl = slice(off[i], off[i + 1])
        fo, _, _ = oracle.dense_fit_predict_batch(oracle.dense_params(), np.array([0, off[i + 1] - off[i]], dtype=np.int32), x0[sl], x1[sl],
                                                  y[:, sl], xs0, xs1)
        _close(f[i], fo[0], FTOL)
    # point-wise X* + variance (the generic kernel) through the chunked entry
    pv = capi.default_params_dense(want_variance=1)
    fv, vv, stv = ctx.dense_fit_predict(pv, off, x0, x1, y[:1], xs0, xs1)
    assert np.all(stv == 0)
    _close(fv[:, 0, :], f1[:, 0, :], 1e-9)
    i = 1600
    sl = slice(off[i], off[i + 1])
    _, vo, _ = oracle.dense_fit_predict_batch(oracle.dense_params(), np.array([0, off[i + 1] - off[i]], dtype=np.int32), x0[sl], x1[sl],
                                              y[:1, sl], xs0, xs1, variance=True)
    assert np.max(np.abs(vv[i] - vo[0])) <= VTOL


@pytest.mark.gpu
def test_host_pointer_two_stream_mode_with_a_chunk_of_small_patches(gp, oracle, monkeypatch):
    """The two-stream form of the host-pointer pipeline (eight chunks, kernels of consecutive chunks on two streams, each in its own half of
    the workspace: csrc/dense_host.hip, dense_host) is for batches whose EVERY chunk goes to the one-wave kernel.  With the variance wanted a
    chunk of patches of <= 192 points goes to the register kernel, whose factor export starts at the base of the workspace -- under the
    other stream's live factor slots if the pipeline forked anyway (round 4 did, up to this test).  Batch: 8192 patches of 250 points with
    patches 1024 .. 2047 (chunk 1) cut to 150; the call must equal the one-stream form and the oracle on patches of both kinds."""
    capi, ctx = gp
    P, res, sz = 8192, 0.15, 8
    off_f, x0_f, x1_f, y_f = synth.make_patches(P, 250, res=res, seed=131)
    counts = np.full(P, 250)
    counts[1024:2048] = 150
    keep = (np.arange(250)[None, :] < counts[:, None]).reshape(-1)
    off = np.zeros(P + 1, dtype=np.int32)
    off[1:] = np.cumsum(counts)
    x0, x1, y = np.ascontiguousarray(x0_f[keep]), np.ascontiguousarray(x1_f[keep]), np.ascontiguousarray(y_f[:, keep])
    xs0, xs1 = synth.grid(res, sz)
    pv = capi.default_params_dense(want_variance=1)
    f, v, st = ctx.dense_fit_predict(pv, off, x0, x1, y, xs0, xs1)
    monkeypatch.setenv("GPC_HOST_ONE_STREAM", "1")
    f1, v1, st1 = ctx.dense_fit_predict(pv, off, x0, x1, y, xs0, xs1)
    monkeypatch.delenv("GPC_HOST_ONE_STREAM")
    assert np.all(st == 0) and np.array_equal(st, st1)
    assert np.max(np.abs(f - f1)) <= 1e-12 * np.max(np.abs(f1)) and np.max(np.abs(v - v1)) <= 1e-12 * np.max(np.abs(v1))
    for i in (0, 1023, 1024, 1500, 2047, 2048, 5000, 8191):
        sl = slice(off[i], off[i + 1])
        fo, vo, _ = oracle.dense_fit_predict_batch(oracle.dense_params(), np.array([0, off[i + 1] - off[i]], dtype=np.int32), x0[sl], x1[sl],
                                                   y[:, sl], xs0, xs1, variance=True)
        _close(f[i], fo[0], FTOL)
        assert np.max(np.abs(v[i] - vo[0])) <= VTOL
    # the same batch without the variance: every chunk is the one-wave kernel's, the pipeline forks, same results as the single stream's
    pm = capi.default_params_dense()
    g2, _, s2 = ctx.dense_fit_predict(pm, off, x0, x1, y, xs0, xs1)
    monkeypatch.setenv("GPC_HOST_ONE_STREAM", "1")
    g1, _, s1 = ctx.dense_fit_predict(pm, off, x0, x1, y, xs0, xs1)
    assert np.all(s2 == 0) and np.array_equal(s1, s2) and np.array_equal(g1, g2)
    _close(g2[:, 0, :], f1[:, 0, :], 1e-9)


@pytest.mark.gpu
def test_two_stream_pipeline_beside_another_threads_call(gp):
    """include/gpc.h: a context is thread-safe.  While a host-pointer call runs its chunks on the context's two compute streams, another
    thread's device-pointer call on the same context uses the SAME workspace from the context's stream: here 2040 patches of 190 points
    with the variance -- the register kernel, whose factor export (2040 x 288 KB from the base of the workspace) reaches across both
    halves the pipeline's chunks keep their factor slots in.  csrc/gpc_internal.h, gpc_ws_reserve, orders the two against each other;
    every result of both threads must equal what the same call gives alone."""
    import threading
    import torch
    capi, ctx = gp
    dev = torch.device("cuda:0")
    P, res, sz = 8192, 0.15, 8
    m = sz * sz
    off, x0, x1, y = synth.make_patches(P, 250, res=res, seed=141)
    xs0, xs1 = synth.grid(res, sz)
    pm = capi.default_params_dense()
    fa_ref, _, sa_ref = ctx.dense_fit_predict(pm, off, x0, x1, y, xs0, xs1)
    assert np.all(sa_ref == 0)
    PB = 2040                       # (its export ends just below the end of the pipeline's two halves: 602 of 637 MB -- no re-growth)
    offb, xb0, xb1, yb = synth.make_patches(PB, 190, res=res, seed=142)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    d = [t(a) for a in (offb, xb0, xb1, yb, xs0, xs1)]
    torch.cuda.synchronize()
    pv = capi.default_params_dense(want_variance=1)

    def run_b():
        f = torch.empty((PB, 1, m), dtype=torch.float64, device=dev)
        v = torch.empty((PB, m), dtype=torch.float64, device=dev)
        st = torch.empty((PB,), dtype=torch.int32, device=dev)
        torch.cuda.synchronize()
        ctx.dense_fit_predict_dev(pv, PB, d[0], 190, int(offb[-1]), d[1], d[2], d[3], 1, m, d[4], d[5], f, v_star=v, status=st)
        ctx.synchronize()
        return f.cpu().numpy(), v.cpu().numpy(), st.cpu().numpy()
    fb_ref, vb_ref, sb_ref = run_b()
    assert np.all(sb_ref == 0)
    bad, done, err = {"a": 0, "b": 0}, {"a": 0, "b": 0}, []
    gate = threading.Barrier(2)

    def check_a(r):
        return np.array_equal(r[2], sa_ref) and np.array_equal(r[0], fa_ref)        # the one-wave kernel is deterministic

    def check_b(r):                                                                 # (the register kernel's LDS atomics meet in arrival order)
        f, v, st = r
        return (np.array_equal(st, sb_ref) and np.max(np.abs(f - fb_ref)) <= 1e-12 * np.max(np.abs(fb_ref))
                and np.max(np.abs(v - vb_ref)) <= 1e-12 * np.max(np.abs(vb_ref)))

    def worker(name, fn, check, reps):
        try:
            gate.wait(timeout=60)
            for _ in range(reps):
                bad[name] += 0 if check(fn()) else 1
                done[name] += 1
        except Exception as e:       # noqa: BLE001 -- reported below
            err.append((name, repr(e)))
    # (a call of A takes ~2 ms, one of B ~5 ms with its allocations: ~0.4 s side by side)
    ths = [threading.Thread(target=worker, args=("a", lambda: ctx.dense_fit_predict(pm, off, x0, x1, y, xs0, xs1), check_a, 120), daemon=True),
           threading.Thread(target=worker, args=("b", run_b, check_b, 60), daemon=True)]
    for th in ths:
        th.start()
    for th in ths:
        th.join(timeout=240)
    assert not err and not any(th.is_alive() for th in ths), err
    assert done == {"a": 120, "b": 60}
    assert bad == {"a": 0, "b": 0}, bad
