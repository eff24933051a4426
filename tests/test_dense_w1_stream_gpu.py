"""The one-wave dense kernel's L_kk^-T stream (csrc/dense_mfma_w1.hip) through the C-ABI, against the CPU oracle.

The 256-point instance writes its triangular L_kk^-T two per image, keeps the last step's in LDS and walks a backward stream aligned at the
even tile count (tests/test_w1_stream_model.py is the lane-by-lane model of it).  These cases put every tile count at which the packing,
the LDS read-out or the stream's alignment changes shape -- nt = 1 (a pair half empty), 2, 3 (odd: the last pair has no partner), 4 (the
last step is the first), 5 (a last step of one column), 6 .. 16, odd and even -- through every way in: the point-wise and the grid entry,
alpha_out, the variance path (whose solve kernel reads the exported slots: their layout must not have moved), a failing pivot behind step 0
and one in the last step, launches that reuse the factor slots, and the 512-point instance, which keeps one image per tile.

Batches of eight patches; tolerances are those of tests/test_dense_gpu.py (two fp64 evaluations of one well-conditioned system).
"""
import numpy as np
import pytest

from variance_cases import _mixed_batch

pytestmark = pytest.mark.gpu

FTOL, ATOL, VTOL = 1e-9, 1e-8, 1e-11          # tests/test_dense_gpu.py
RES, SZ = 0.15, 12
W1, W1_VAR, W1_512 = "dense_mfma_w1", "dense_mfma_w1 + dense_variance", "dense_mfma_w1_512"

# every batch holds a patch of more than 192 points (the variance takes the one-wave kernel from 193 points up) and none of more than 256
BATCHES = {
    "nt1-5": [16, 0, 17, 48, 64, 65, 80, 255],
    "nt6-9": [96, 112, 128, 0, 129, 256, 33, 1],
    "nt10-16": [145, 161, 177, 193, 209, 225, 241, 0],
}
SIZES_512 = [257, 400, 512, 0, 300, 64, 511, 273]
SEEDS = {"nt1-5": 41, "nt6-9": 42, "nt10-16": 43, "512": 44}
_REF = {}


@pytest.fixture(scope="module")
def gp():
    from gp_compressor_amd import capi
    capi.load()          # raises if the HIP library is missing: no fallback
    ctx = capi.Context(0)
    yield capi, ctx
    ctx.close()


@pytest.fixture(autouse=True)
def _small_batches_on_the_one_wave_kernel(monkeypatch):
    for e in ("GPC_FORCE_GENERIC", "GPC_FORCE_BIG", "GPC_NO_W1", "GPC_NO_W1_512", "GPC_W2", "GPC_W1_SLOTS", "GPC_POISON_LDS"):
        monkeypatch.delenv(e, raising=False)
    monkeypatch.setenv("GPC_W1_MIN_P", "2")           # (production: batches of at least four patches per CU)


def _close(f, want, tol):
    scale = max(float(np.max(np.abs(want))), 1e-300)
    err = float(np.max(np.abs(f - want)))
    assert err <= tol * scale, (err, scale)


def _case(oracle, name):
    """The batch, its prediction points (the grid's, so that both entries share one reference) and the oracle's answer: once per module."""
    if name not in _REF:
        sizes = SIZES_512 if name == "512" else BATCHES[name]
        batch = _mixed_batch(sizes, seed=SEEDS[name])
        xs = oracle.grid(RES, SZ)
        ref = oracle.dense_fit_predict_batch(oracle.dense_params(), *batch, *xs, variance=name != "512", want_alpha=True)
        for a in (*batch, *xs, *ref):
            if isinstance(a, np.ndarray):
                a.setflags(write=False)
        _REF[name] = (batch, xs, ref)
    return _REF[name]


@pytest.mark.parametrize("name", list(BATCHES))
def test_pointwise_grid_and_alpha(gp, oracle, name):
    capi, ctx = gp
    batch, xs, (fo, _, so, ao) = _case(oracle, name)
    p = capi.default_params_dense()
    f, _, st, al = ctx.dense_fit_predict(p, *batch, *xs, want_alpha=True)
    assert ctx.last_dense_kernel() == W1
    assert np.array_equal(st, so) and np.all(st == 0)
    _close(f, fo, FTOL)
    _close(al, ao, ATOL)
    empty = np.flatnonzero(np.diff(batch[0]) == 0)
    assert np.all(f[empty] == 0)
    fg, stg, alg = ctx.dense_fit_predict_grid(p, *batch, RES, SZ, want_alpha=True)
    assert ctx.last_dense_kernel() == W1 and np.all(stg == 0)
    _close(fg, fo, FTOL)
    _close(alg, ao, ATOL)
    f1, _, st1 = ctx.dense_fit_predict(p, *batch, *xs)      # without alpha_out
    assert ctx.last_dense_kernel() == W1 and np.array_equal(f1, f) and np.array_equal(st1, st)


@pytest.mark.parametrize("name", list(BATCHES))
def test_variance_reads_the_exported_slots(gp, oracle, name):
    capi, ctx = gp
    batch, xs, (fo, vo, so, ao) = _case(oracle, name)
    p = capi.default_params_dense(want_variance=1)
    f, v, st, al = ctx.dense_fit_predict(p, *batch, *xs, want_alpha=True)
    assert ctx.last_dense_kernel() == W1_VAR
    assert np.array_equal(st, so) and np.all(st == 0)
    _close(f, fo, FTOL)
    _close(al, ao, ATOL)
    assert np.max(np.abs(v - vo)) <= VTOL
    empty = np.flatnonzero(np.diff(batch[0]) == 0)
    assert np.all(v[empty] == p.sigmaf_sq) and np.all(f[empty] == 0)
    # without alpha_out the weights live in the workspace, behind the (now shorter) L_kk^-T area
    f2, v2, st2 = ctx.dense_fit_predict(p, *batch, *xs)
    assert ctx.last_dense_kernel() == W1_VAR
    assert np.array_equal(f2, f) and np.array_equal(v2, v) and np.array_equal(st2, st)


@pytest.mark.parametrize("want_var", [0, 1])
def test_failing_pivot_behind_step_0_and_in_the_last_step(gp, oracle, want_var):
    """A duplicated point under zero noise (short length scale: everything else stays well conditioned).  Patch 1: point 85 repeats point 35,
    the pivot fails in tile column 5, one step behind step 0.  Patch 6: point 230 repeats point 35, tile column 14 of 16: the last step,
    whose inverses the backward solve would have read from LDS."""
    capi, ctx = gp
    kw0 = dict(sigmaf_sq=1.0, l_sq=0.01 ** 2, noise=0.0)
    p0 = capi.default_params_dense(want_variance=want_var, **kw0)
    off, x0, x1, y = _mixed_batch([200, 250, 256, 64, 0, 130, 250, 17], seed=46)
    for patch, at in ((1, 85), (6, 230)):
        x0[off[patch] + at] = x0[off[patch] + 35]
        x1[off[patch] + at] = x1[off[patch] + 35]
    xs = oracle.grid(RES, SZ)
    f, v, st, al = ctx.dense_fit_predict(p0, off, x0, x1, y, *xs, want_alpha=True)
    assert ctx.last_dense_kernel() == (W1_VAR if want_var else W1)
    fo, vo, so = oracle.dense_fit_predict_batch(oracle.dense_params(kw0["sigmaf_sq"], kw0["l_sq"], 0.0), off, x0, x1, y, *xs, variance=bool(want_var))
    good = [0, 2, 3, 4, 5, 7]
    # (the oracle tests the pivot against 0: whether a duplicate leaves +1e-17 or -1e-17 there is luck; the kernel's threshold is relative)
    want_st = np.zeros(8, dtype=st.dtype)
    want_st[[1, 6]] = capi.STATUS_NOT_SPD
    assert np.array_equal(st, want_st) and np.all(so[good] == 0)
    for patch in (1, 6):
        assert np.all(np.isnan(f[patch])) and np.all(np.isnan(al[0, off[patch]:off[patch + 1]]))
        if want_var:
            assert np.all(np.isnan(v[patch]))
    assert np.all(np.isfinite(f[good]))
    _close(f[good], fo[good], 1e-7)          # (zero noise: conditioned by the closest pairs of points; tests/test_dense_gpu.py)
    if want_var:
        assert np.all(np.isfinite(v[good]))
    for patch in good:
        assert np.all(np.isfinite(al[0, off[patch]:off[patch + 1]]))


@pytest.mark.parametrize("want_var", [0, 1])
def test_slot_reuse_gives_the_same_bits(gp, oracle, monkeypatch, want_var):
    """Launches of three patches that reuse three factor slots: the L_kk^-T area is indexed by slot.  Then other work on the same context
    and the first batch again."""
    capi, ctx = gp
    p = capi.default_params_dense(want_variance=want_var)
    kernel = W1_VAR if want_var else W1
    runs = {}
    for name in ("nt1-5", "nt10-16"):
        batch, xs, _ = _case(oracle, name)
        runs[name] = ctx.dense_fit_predict(p, *batch, *xs, want_alpha=True)
        assert ctx.last_dense_kernel() == kernel
    monkeypatch.setenv("GPC_W1_SLOTS", "3")
    for name in ("nt1-5", "nt10-16", "nt1-5"):
        batch, xs, _ = _case(oracle, name)
        got = ctx.dense_fit_predict(p, *batch, *xs, want_alpha=True)
        assert ctx.last_dense_kernel() == kernel
        for a, b in zip(got, runs[name]):
            assert (a is None and b is None) or np.array_equal(a, b)
    monkeypatch.delenv("GPC_W1_SLOTS")
    for name in ("nt10-16", "nt1-5"):                  # two calls in a row, whole slots again
        batch, xs, _ = _case(oracle, name)
        got = ctx.dense_fit_predict(p, *batch, *xs, want_alpha=True)
        for a, b in zip(got, runs[name]):
            assert (a is None and b is None) or np.array_equal(a, b)


def test_512_point_instance(gp, oracle, monkeypatch):
    """n = 257, 400, 512 and their neighbours on dense_w1_kernel<512>: against the oracle and against the tiled path."""
    capi, ctx = gp
    batch, xs, (fo, _, so, ao) = _case(oracle, "512")
    p = capi.default_params_dense()
    f, _, st, al = ctx.dense_fit_predict(p, *batch, *xs, want_alpha=True)
    assert ctx.last_dense_kernel() == W1_512
    assert np.array_equal(st, so) and np.all(st == 0)
    _close(f, fo, FTOL)
    _close(al, ao, ATOL)
    fg, stg = ctx.dense_fit_predict_grid(p, *batch, RES, SZ)
    assert ctx.last_dense_kernel() == W1_512 and np.all(stg == 0)
    _close(fg, fo, FTOL)
    monkeypatch.setenv("GPC_W1_SLOTS", "3")
    f2, _, st2, al2 = ctx.dense_fit_predict(p, *batch, *xs, want_alpha=True)
    monkeypatch.delenv("GPC_W1_SLOTS")
    assert ctx.last_dense_kernel() == W1_512
    assert np.array_equal(f2, f) and np.array_equal(al2, al) and np.array_equal(st2, st)
    monkeypatch.setenv("GPC_NO_W1_512", "1")
    f3, _, st3, al3 = ctx.dense_fit_predict(p, *batch, *xs, want_alpha=True)
    monkeypatch.delenv("GPC_NO_W1_512")
    assert "w1_512" not in ctx.last_dense_kernel() and np.array_equal(st3, st)
    _close(f3, f, FTOL)
    _close(al3, al, ATOL)
