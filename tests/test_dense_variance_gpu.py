"""GPU parity tests of the dense predictive variance (csrc/dense_variance.hip) against the CPU oracle, through the C-ABI.

Whenever the variance is requested the mean comes out of the variance kernel too (the fit kernel skips its prediction phase), so
every case checks f*, the weights, the status and v.  What the cases pin: every tile count at which the super-row solve of
dense_variance_big_kernel changes shape, X* counts that are no multiple of 16 (the lane guard, the partial round, the rounds of
four), more patches than workgroups (the grid-stride loop and what it re-uses from one patch to the next), failed and empty patches
on every export, the exponential regimes above 256 points, and the chunked host-pointer entry across the factor-export layouts.

Tolerances are test_dense_gpu.py's (two fp64 evaluations of the same well-conditioned system): 1e-9 max|f*|, 1e-8 max|alpha|, 1e-11 on
v at sigma_f^2 = 0.0025.  The oracle's own error against an 80-bit restatement is 4e-15 sigma_f^2 and 3e-12 (test_variance_cases_cpu.py);
one dropped or mis-addressed 16 x 16 tile of the factor moves v by about 1e-4 sigma_f^2.  X* is point-wise and not a grid
(variance_cases.xstar)."""
import numpy as np
import pytest

import variance_cases as VC

pytestmark = pytest.mark.gpu

FTOL, ATOL, VTOL = 1e-9, 1e-8, 1e-11
BIG = "dense_mfma_big + dense_variance_big"
_REF = {}


@pytest.fixture(scope="module")
def gp():
    from gp_compressor_amd import capi
    capi.load()          # raises if the HIP library is missing: no fallback
    ctx = capi.Context(0)
    yield capi, ctx
    ctx.close()


@pytest.fixture(autouse=True)
def _plain_dispatch(monkeypatch):
    for e in ("GPC_FORCE_GENERIC", "GPC_FORCE_BIG", "GPC_BIG_NO_W2", "GPC_BIG_NO_W4", "GPC_NO_W1", "GPC_NO_W1_512", "GPC_W2",
              "GPC_W1_MIN_P", "GPC_W1_SLOTS", "GPC_VAR_W4", "GPC_NO_SPLIT", "GPC_HOST_NO_PIPELINE", "GPC_HOST_ONE_STREAM"):
        monkeypatch.delenv(e, raising=False)


def _close(f, want, tol):
    scale = max(float(np.max(np.abs(want))), 1e-300)
    err = float(np.max(np.abs(f - want)))
    assert err <= tol * scale, (err, scale)


def _ref(key, make):
    """An oracle result, computed once per module and never written to."""
    if key not in _REF:
        out = make()
        for a in out:
            if isinstance(a, np.ndarray):
                a.setflags(write=False)
        _REF[key] = out
    return _REF[key]


def _params(capi, regime, **kw):
    return capi.default_params_dense(want_variance=1, sigmaf_sq=regime[0], l_sq=regime[1], noise=regime[2], **kw)


def _run(ctx, capi, regime, batch, xs):
    f, v, st, al = ctx.dense_fit_predict(_params(capi, regime), *batch, *xs, want_alpha=True)
    return f, v, st, al


def _oracle(oracle, regime, batch, xs):
    return oracle.dense_fit_predict_batch(oracle.dense_params(*regime), *batch, *xs, variance=True, want_alpha=True)


def _check_range(v, sf):
    """Every finite variance lies between 0 and the prior's, to rounding."""
    fin = v[np.isfinite(v)]
    assert fin.size == 0 or (fin.min() >= -1e-12 * sf and fin.max() <= sf * (1 + 1e-12)), (fin.min(), fin.max())


def _check(got, ref, off, sf, ftol=FTOL, atol=ATOL, vtol=VTOL, label=""):
    """GPU against oracle on a batch whose every patch is SPD: equal status, f*, alpha, v; empty patches give the prior exactly."""
    f, v, st, al = got
    fo, vo, so, ao = ref
    assert np.array_equal(st, so) and np.all(st == 0)
    ev = float(np.max(np.abs(v - vo))) if v.size else 0.0
    print("%s: max|v - v_o| = %.3e (%.2e sf^2), max|f - f_o| / max|f_o| = %.3e" % (
        label, ev, ev / sf, float(np.max(np.abs(f - fo))) / max(float(np.max(np.abs(fo))), 1e-300) if f.size else 0.0))
    _close(f, fo, ftol)
    _close(al, ao, atol)
    assert ev <= vtol, ev
    empty = np.flatnonzero(np.diff(off) == 0)
    assert np.all(v[empty] == sf) and np.all(f[empty] == 0)
    _check_range(v, sf)


# ---------------------------------------------------------------------------------------------------------------- 1. tile counts

@pytest.mark.parametrize("cap", [1024, 528, 512])
@pytest.mark.parametrize("ny", [1, 3])
def test_variance_big_tile_counts(gp, oracle, ny, cap):
    """dense_variance_big_kernel at every tile count where its walk changes: nt = 1, 2, 16 (one super-row, no scratch), 17 (a last
    super-row of ONE tile row), 18, 32, 33, 34, 48, 49, 63, 64, small patches inside slots of 64 tile columns, two empty patches; depth
    plane and three planes.  cap = 528: the same patches up to 528 points alone, slots of 33 tile columns (the eight-wave fit's export:
    the four-wave fit shape takes the depth plane up to 512 points only); cap = 512: slots of 32 columns, which is that four-wave
    shape's export for ny = 1."""
    capi, ctx = gp
    full = VC.tile_batch(ny)
    xs = VC.xstar(131, seed=43)
    ref = _ref(("tiles", ny), lambda: _oracle(oracle, VC.DEFAULT, full, xs))
    idx = [i for i, n in enumerate(VC.TILE_SIZES) if n <= cap]
    batch, pts = VC.take_patches(*full, idx)
    assert int(np.max(np.diff(batch[0]))) == cap
    got = _run(ctx, capi, VC.DEFAULT, batch, xs)
    assert ctx.last_dense_kernel() == BIG, ctx.last_dense_kernel()
    _check(got, (ref[0][idx], ref[1][idx], ref[2][idx], ref[3][:, pts]), batch[0], VC.DEFAULT[0], label="tiles ny=%d cap=%d" % (ny, cap))


# ---------------------------------------------------------------------------------------------------------------- 2. X* counts

M_LIST = (1, 15, 16, 17, 63, 64, 65, 127, 128, 129)


@pytest.mark.parametrize("m", M_LIST)
def test_variance_big_xstar_counts(gp, oracle, m):
    """X* counts around the 16-point block and the eight-wave round on the big kernel: a partial block (q < m), a single point, and
    m = 129 -- nine blocks on eight waves, the second round has one active wave with one valid column while seven serve the stream."""
    capi, ctx = gp
    batch = VC._mixed_batch([300, 520, 0, 270], seed=44)
    xs = VC.xstar(m, seed=100 + m)
    got = _run(ctx, capi, VC.DEFAULT, batch, xs)
    assert ctx.last_dense_kernel() == BIG, ctx.last_dense_kernel()
    _check(got, _oracle(oracle, VC.DEFAULT, batch, xs), batch[0], VC.DEFAULT[0], label="big m=%d" % m)


@pytest.mark.parametrize("m", M_LIST)
def test_variance_small_xstar_counts(gp, oracle, monkeypatch, m):
    """The same X* counts on dense_variance_kernel<16> behind the one-wave fit, in rounds of eight (GPC_VAR_W4=0) and of four (=1)
    blocks: each against the oracle, and the two bit-identical in v (same arithmetic per block on the same factor)."""
    capi, ctx = gp
    monkeypatch.setenv("GPC_W1_MIN_P", "2")
    batch = VC._mixed_batch([40, 100, 180, 0, 250, 7], seed=45)
    xs = VC.xstar(m, seed=200 + m)
    ref = _oracle(oracle, VC.DEFAULT, batch, xs)
    vs = []
    for w4 in ("0", "1"):
        monkeypatch.setenv("GPC_VAR_W4", w4)
        got = _run(ctx, capi, VC.DEFAULT, batch, xs)
        assert ctx.last_dense_kernel() == "dense_mfma_w1 + dense_variance", ctx.last_dense_kernel()
        _check(got, ref, batch[0], VC.DEFAULT[0], label="small m=%d w4=%s" % (m, w4))
        vs.append(got[1])
    assert np.array_equal(vs[0], vs[1])


# ---------------------------------------------------------------------------------------------------------------- 3. more patches than workgroups

def _thirds(ctx, capi, regime, batch, xs):
    """The batch in three calls of 200 patches: no workgroup of the variance kernel meets a second patch."""
    fs, vs, sts = [], [], []
    for k in range(3):
        sub, _ = VC.take_patches(*batch, list(range(200 * k, 200 * k + 200)))
        f, v, st, _ = _run(ctx, capi, regime, sub, xs)
        assert ctx.last_dense_kernel() == BIG
        fs.append(f), vs.append(v), sts.append(st)
    return np.concatenate(fs), np.concatenate(vs), np.concatenate(sts)


def test_variance_big_grid_stride_loop(gp, oracle):
    """600 patches of 1 .. 336 points on at most 256 workgroups: every workgroup of dense_variance_big_kernel runs two or three patches,
    re-using its LDS vectors and its scratch (patch 0 is the largest; patches 5, 300, 590 have two super-rows), and passes four empty
    patches.  Default hyper-parameters, every patch against the oracle; and against the same batch in three calls of 200 patches.
    Measured on MI355X: max|v - v_o| = 7.8e-18 (3.1e-15 sigma_f^2), max|f - f_o| = 3.2e-13 max|f_o|."""
    capi, ctx = gp
    batch = VC.many_batch()
    xs = VC.xstar(37, seed=31)
    got = _run(ctx, capi, VC.DEFAULT, batch, xs)
    assert ctx.last_dense_kernel() == BIG, ctx.last_dense_kernel()
    ref = _ref(("many", "default"), lambda: _oracle(oracle, VC.DEFAULT, batch, xs))
    assert np.array_equal(np.flatnonzero(np.diff(batch[0]) == 0), VC.MANY_EMPTY)
    _check(got, ref, batch[0], VC.DEFAULT[0], label="600 patches, defaults")
    f3, v3, st3 = _thirds(ctx, capi, VC.DEFAULT, batch, xs)
    assert np.array_equal(st3, got[2])
    _close(f3, got[0], 1e-12)
    _close(v3, got[1], 1e-12)


def test_variance_big_grid_stride_loop_failed_patches(gp, oracle):
    """The same batch without a noise term (sigma_f^2 = 1, l = 3 mm): in patches 5, 300 and 590 point 280 repeats point 11, the fit
    fails at a pivot of the second super-row, and the variance kernel must write NaN for them and `continue` as one workgroup -- their
    neighbours in index and the patches one workgroup stride later are compared like every other patch.  (The oracle's status of the
    three is not compared: it tests the pivot against 0, and whether the repeat leaves +1e-17 or -1e-17 there is luck.)
    Measured on MI355X over the 597 other patches: worst |v - v_o| = 1.8e-13 sigma_f^2, worst |f - f_o| = 1.8e-12 max|f_o|."""
    capi, ctx = gp
    regime = VC.ZERO_NOISE
    batch = VC.many_batch()
    off = batch[0]
    xs = VC.xstar(37, seed=31)
    f, v, st, al = _run(ctx, capi, regime, batch, xs)
    assert ctx.last_dense_kernel() == BIG, ctx.last_dense_kernel()
    fo, vo, so, ao = _ref(("many", "zero_noise"), lambda: _oracle(oracle, regime, batch, xs))
    bad = list(VC.MANY_DUP)
    good = np.setdiff1d(np.arange(VC.MANY_P), bad)
    assert st[bad].tolist() == [1, 1, 1] and np.all(st[good] == 0) and np.all(so[good] == 0)
    for i in bad:
        assert np.all(np.isnan(f[i])) and np.all(np.isnan(v[i])) and np.all(np.isnan(al[0, off[i]:off[i + 1]]))
    worst_v = worst_f = 0.0
    for i in good:
        scale = max(float(np.max(np.abs(fo[i]))), 1e-300)
        ef, ev = float(np.max(np.abs(f[i] - fo[i]))) / scale, float(np.max(np.abs(v[i] - vo[i]))) / regime[0]
        worst_f, worst_v = max(worst_f, ef), max(worst_v, ev)
        assert np.all(np.isfinite(al[0, off[i]:off[i + 1]]))
        assert ef <= 1e-7 and ev <= 1e-7, (i, int(off[i + 1] - off[i]), ef, ev)
    print("600 patches, zero noise: worst |v - v_o| / sf^2 = %.3e, worst |f - f_o| / max|f_o| = %.3e" % (worst_v, worst_f))
    empty = list(VC.MANY_EMPTY)
    assert np.all(v[empty] == regime[0]) and np.all(f[empty] == 0)
    _check_range(v, regime[0])
    f3, v3, st3 = _thirds(ctx, capi, regime, batch, xs)
    assert np.array_equal(st3, st) and np.array_equal(np.isnan(f3), np.isnan(f)) and np.array_equal(np.isnan(v3), np.isnan(v))
    _close(f3[good], f[good], 1e-12)
    _close(v3[good], v[good], 1e-12)


# ---------------------------------------------------------------------------------------------------------------- 4. register-kernel export

@pytest.mark.parametrize("n_max,nt", [(64, 4), (128, 8), (192, 12)])
def test_variance_register_export_with_failures(gp, oracle, n_max, nt):
    """dense_variance_kernel<4 | 8 | 12> behind the register-tile fit's export: sizes on and next to every tile edge, an empty and a
    single-point patch, against the oracle; then without a noise term and with a repeated point in the middle patch -- status 1 and
    NaN there, every other patch finite and within 1e-7 (the project's bound for this conditioning)."""
    capi, ctx = gp
    name = "dense_mfma_nt%d + dense_variance" % nt
    xs = VC.xstar(53, seed=46)
    batch, _ = VC.edge_batch(n_max)
    got = _run(ctx, capi, VC.DEFAULT, batch, xs)
    assert ctx.last_dense_kernel() == name, ctx.last_dense_kernel()
    _check(got, _oracle(oracle, VC.DEFAULT, batch, xs), batch[0], VC.DEFAULT[0], label="register n_max=%d" % n_max)
    regime = VC.ZERO_NOISE
    batch, mid = VC.edge_batch(n_max, dup=True)
    off = batch[0]
    P = len(off) - 1
    f, v, st, al = _run(ctx, capi, regime, batch, xs)
    assert ctx.last_dense_kernel() == name, ctx.last_dense_kernel()
    fo, vo, so, _ = _oracle(oracle, regime, batch, xs)
    good = np.setdiff1d(np.arange(P), [mid])
    assert st[mid] == 1 and np.all(st[good] == 0) and np.all(so[good] == 0)
    assert np.all(np.isnan(f[mid])) and np.all(np.isnan(v[mid])) and np.all(np.isnan(al[0, off[mid]:off[mid + 1]]))
    assert np.all(np.isfinite(f[good])) and np.all(np.isfinite(v[good])) and np.all(np.isfinite(np.delete(al[0], np.arange(off[mid], off[mid + 1]))))
    for i in good:
        assert np.max(np.abs(f[i] - fo[i])) <= 1e-7 * max(float(np.max(np.abs(fo[i]))), 1e-300), i
        assert np.max(np.abs(v[i] - vo[i])) <= 1e-7 * regime[0], i
    assert np.all(v[0] == regime[0]) and np.all(f[0] == 0)         # the empty patch
    _check_range(v, regime[0])


# ---------------------------------------------------------------------------------------------------------------- 5. exponential regimes

@pytest.mark.parametrize("l_sq,shift,tol", [(0.05 ** 2, 0.0, 1e-8), (0.5 ** 2, 0.0, FTOL), (9.0, 0.4, FTOL), (9.0, 30.0, FTOL)])
def test_variance_big_exp_regimes(gp, oracle, l_sq, shift, tol):
    """The regimes of test_dense_one_wave_kernel_exp_regimes (sigma_f^2 = 0.5, noise 1e-3) above 256 points, where the variance kernel
    evaluates K* with the table-driven exponential only.  Bounds: that test's, times 520 / 256 -- the condition-number bound
    1 + n sf^2 / (2 sn^2) of test_dense_gpu.py's docstring is linear in n."""
    capi, ctx = gp
    grow = 520.0 / 256.0
    off, x0, x1, y = VC._mixed_batch([300, 520, 377, 451], seed=47)
    batch = (off, x0 + shift, x1 - shift, y)
    xs = VC.xstar(64, seed=48)
    regime = (0.5, l_sq, 1e-3)
    f, v, st, _ = _run(ctx, capi, regime, batch, xs)
    assert ctx.last_dense_kernel() == BIG, ctx.last_dense_kernel()
    fo, vo, so, _ = _oracle(oracle, regime, batch, xs)
    assert np.all(st == 0) and np.all(so == 0)
    ev = float(np.max(np.abs(v - vo)))
    print("exp regime l_sq=%g shift=%g: max|v - v_o| = %.3e, f %.3e" % (l_sq, shift, ev, float(np.max(np.abs(f - fo))) / max(float(np.max(np.abs(fo))), 1e-300)))
    _close(f, fo, tol * grow)
    assert ev <= (1e-9 if tol > FTOL else 1e-10) * grow
    _check_range(v, regime[0])


# ---------------------------------------------------------------------------------------------------------------- 6. chunked host entry

@pytest.mark.parametrize("P", [2100, 4200])
def test_variance_host_pipeline_across_export_layouts(gp, oracle, monkeypatch, P):
    """The host-pointer entry dispatches each chunk by the chunk's own largest patch, so consecutive chunks lay different factor exports
    into the same workspace.  Four groups of P / 4 patches: 40 .. 190 points, 200 .. 256, 257 .. 300, 100 .. 330 mixed.  P = 2100 goes
    through in two chunks (one-wave slots with the small patches inside them, then tiled slots); P = 4200 in four, one per group:
    register kernel's export, one-wave slots, tiled slots of 19 and of 21 tile columns.  With GPC_HOST_NO_PIPELINE the whole batch has
    n_max = 330 and every patch, the small ones included, goes through the tiled export and dense_variance_big: an independent path
    for the small tile counts.  Both agree to the run-to-run bound; 64 patches, the first and last of every group among them, against
    the oracle."""
    capi, ctx = gp
    monkeypatch.setenv("GPC_W1_MIN_P", "2")
    batch = VC.chunk_batch(P)
    xs = VC.xstar(25, seed=49)
    prm = _params(capi, VC.DEFAULT)
    f, v, st, al = ctx.dense_fit_predict(prm, *batch, *xs, want_alpha=True)
    assert ctx.last_dense_kernel() == BIG, ctx.last_dense_kernel()
    monkeypatch.setenv("GPC_HOST_NO_PIPELINE", "1")
    f1, v1, st1, al1 = ctx.dense_fit_predict(prm, *batch, *xs, want_alpha=True)
    assert ctx.last_dense_kernel() == BIG, ctx.last_dense_kernel()
    assert np.all(st == 0) and np.array_equal(st, st1)
    _close(f, f1, 1e-12)
    _close(v, v1, 1e-12)
    _close(al, al1, 1e-12)
    q = P // 4
    edges = [0, q - 1, q, 2 * q - 1, 2 * q, 3 * q - 1, 3 * q, P - 1]
    rest = np.setdiff1d(np.arange(P), edges)
    pick = sorted(edges + np.random.default_rng(63).choice(rest, 64 - len(edges), replace=False).tolist())
    assert len(pick) == 64
    sub, pts = VC.take_patches(*batch, pick)
    fo, vo, so, ao = _oracle(oracle, VC.DEFAULT, sub, xs)
    assert np.all(so == 0)
    for g_f, g_v, g_a in ((f, v, al), (f1, v1, al1)):
        _close(g_f[pick], fo, FTOL)
        _close(g_a[:, pts], ao, ATOL)
        assert np.max(np.abs(g_v[pick] - vo)) <= VTOL
    _check_range(v, VC.DEFAULT[0])
    _check_range(v1, VC.DEFAULT[0])
