"""GPU parity tests of the Newton / IRLS instances of the tiled kernel (dense_big_kernel<..., IRLS>, csrc/dense_mfma_big.hip) against the
CPU oracle, through the C-ABI.

What the cases pin, beyond test_probit_gpu.py: every tile count at which the four-columns-per-step factorisation changes shape, inside
slots of 64, 33 and 17 tile columns; the four-wave shape at every tile edge up to 256 points; more patches than workgroups (the ticket
deal, a second patch on LDS the first one left); patches that fail in the step prologue (a NaN label, the singular start of model 1)
beside healthy ones; the step cap; a healthy call after a failed one on the same context; NaN in every LDS word before the call; the
optional outputs left NULL; and the grid read-out of both shapes at the sizes where it changes path (one tile, two, the 32 | 33 switch to
the per-point loop).

Tolerances are test_probit_gpu.py's: equal status, |iters - iters_oracle| <= 1, f*, fhat and alpha within 1e-8 (model 2) or 1e-6
(model 1) of the patch's max-norm.  The oracle itself agrees with R&W's Algorithm 3.1 to 1e-13 / 1e-12 at these sizes
(test_irls_cases_cpu.py).  Inputs: irls_cases.py."""
import numpy as np
import pytest

import irls_cases as IC
import variance_cases as VC

pytestmark = pytest.mark.gpu

BIG, W4 = "dense_mfma_big_irls", "dense_mfma_big_w4_irls"
SZ = 20
_REF = {}


@pytest.fixture(scope="module")
def gp():
    from gp_compressor_amd import capi
    capi.load()          # raises if the HIP library is missing: no fallback
    ctx = capi.Context(0)
    yield capi, ctx
    ctx.close()


@pytest.fixture(autouse=True)
def _plain_env(monkeypatch):
    monkeypatch.delenv("GPC_POISON_LDS", raising=False)


def _ref(key, make):
    """An oracle result, computed once per module and never written to."""
    if key not in _REF:
        out = make()
        for a in out:
            if isinstance(a, np.ndarray):
                a.setflags(write=False)
        _REF[key] = out
    return _REF[key]


def _sub(ref, off, idx, pts):
    """The rows of a full-batch oracle result that belong to the sub-batch (idx, pts)."""
    f, al, fh, it, st = ref
    idx = list(idx)
    return f[idx], al[pts], fh[pts], it[idx], st[idx]


def _params(capi, model):
    return capi.default_params_dense(sigmaf_sq=IC.REGIME[0], l_sq=IC.REGIME[1], noise=IC.REGIME[2], noise_model=model)


def _irls(capi, model, max_iter=IC.MAX_ITER, **kw):
    arg = dict(IC.MODELS[model])
    arg.update(kw)
    return capi.default_params_irls(max_iter=max_iter, **arg)


def _run(ctx, capi, model, batch, sz=SZ, xs=None, **kw):
    if xs is not None:
        return ctx.dense_irls_fit_predict(_params(capi, model), _irls(capi, model, **kw), *batch, xs0=xs[0], xs1=xs[1])
    return ctx.dense_irls_fit_predict(_params(capi, model), _irls(capi, model, **kw), *batch, res=IC.RES, sz=sz)


def _gap(a, b):
    return float(np.max(np.abs(a - b))) / max(float(np.max(np.abs(b))), 1e-300) if b.size else 0.0


def _check(got, ref, off, model, label, want_status=0, iters_exact=None):
    """GPU against oracle, patch by patch.  Patches whose oracle status is 2 (NaN) must be NaN in exactly their own rows with the
    oracle's iteration count; every other patch has status want_status (0, or 5 under a step cap: the outputs are the last iterate) and
    f*, fhat, alpha within the model's tolerance of the patch's max-norm; empty patches give f* == 0, iters == 0, status 0."""
    f, al, fh, it, st = got
    fo, alo, fho, ito, sto = ref
    n = np.diff(off)
    assert np.array_equal(st, sto), (label, np.flatnonzero(st != sto)[:8], st[st != sto][:8], sto[st != sto][:8])
    tol = IC.FTOL[model]
    worst = [0.0, 0.0, 0.0]
    for i in range(len(n)):
        sl = slice(off[i], off[i + 1])
        if n[i] == 0:
            assert st[i] == 0 and it[i] == 0 and np.all(f[i] == 0), (label, i)
            continue
        if sto[i] == 2:
            assert it[i] == ito[i] and np.all(np.isnan(f[i])) and np.all(np.isnan(al[sl])) and np.all(np.isnan(fh[sl])), (label, i)
            continue
        assert st[i] == want_status, (label, i, st[i])
        if iters_exact is not None:
            assert it[i] == iters_exact == ito[i], (label, i, it[i], ito[i])
        assert abs(int(it[i]) - int(ito[i])) <= 1, (label, i, it[i], ito[i])
        assert np.all(np.isfinite(f[i])) and np.all(np.isfinite(al[sl])) and np.all(np.isfinite(fh[sl])), (label, i)
        g = (_gap(f[i], fo[i]), _gap(fh[sl], fho[sl]), _gap(al[sl], alo[sl]))
        worst = [max(w, e) for w, e in zip(worst, g)]
        assert max(g) <= tol, (label, i, int(n[i]), g)
    print("%s: worst |f* - f*_o| = %.2e, |fhat - fhat_o| = %.2e, |a - a_o| = %.2e of the patch's max-norm" % ((label,) + tuple(worst)))


def _same(f, g, tol, label):
    """Two GPU runs of the same patches: NaN in the same places, finite values within tol of the max-norm."""
    assert np.array_equal(np.isnan(f), np.isnan(g)), label
    fin = np.isfinite(g)
    assert not fin.any() or float(np.max(np.abs(f[fin] - g[fin]))) <= tol * max(float(np.max(np.abs(g[fin]))), 1e-6), label


def _grid(oracle, sz=SZ):
    return oracle.grid(IC.RES, sz)


def _tile_ref(oracle, model):
    """The oracle on the tile-count sweep (model 1: on the sizes up to 529 only), as rows of the full batch."""
    full = IC.tile_batch()
    if model == 2:
        return _ref(("tiles", 2), lambda: IC.oracle_fit(oracle, full, 2, _grid(oracle)))

    def make():
        idx = IC.cap_index(IC.MODEL1_CAP)
        sub, pts = IC.take(full, idx)
        f, al, fh, it, st = IC.oracle_fit(oracle, sub, 1, _grid(oracle))
        P, N = len(IC.TILE_SIZES_BIG), int(full[0][-1])
        F, A, H = np.full((P, f.shape[1]), np.nan), np.full(N, np.nan), np.full(N, np.nan)
        I, S = np.full(P, -1, dtype=np.int32), np.full(P, -1, dtype=np.int32)
        F[idx], A[pts], H[pts], I[idx], S[idx] = f, al, fh, it, st
        return F, A, H, I, S
    return _ref(("tiles", 1), make)


# ---------------------------------------------------------------------------------------------------------------- 1, 5. tile counts, eight waves

def _tile_counts(gp, oracle, cap, model, label):
    capi, ctx = gp
    full = IC.tile_batch()
    idx = IC.cap_index(cap)
    batch, pts = IC.take(full, idx)
    assert int(np.max(np.diff(batch[0]))) == cap
    ref = _sub(_tile_ref(oracle, model), full[0], idx, pts)
    assert np.all(ref[4] == 0)
    got = _run(ctx, capi, model, batch)
    assert ctx.last_dense_kernel() == BIG, ctx.last_dense_kernel()
    _check(got, ref, batch[0], model, "%s cap=%d model=%d" % (label, cap, model))
    if cap == 513:
        # the point-wise entry on 37 scattered X*: against the oracle, and each entry's f* against its own alpha through a NumPy K*
        xs = VC.xstar(37, seed=84)
        ref37 = _ref(("tiles37", model), lambda: IC.oracle_fit(oracle, batch, model, xs))
        got37 = _run(ctx, capi, model, batch, xs=xs)
        assert ctx.last_dense_kernel() == BIG
        _check(got37, ref37, batch[0], model, "%s cap=513 model=%d, 37 X*" % (label, model))
        worst = 0.0
        for r, q in ((got, _grid(oracle)), (got37, xs)):
            for i in np.flatnonzero(np.diff(batch[0]) > 0):
                sl = slice(batch[0][i], batch[0][i + 1])
                d2 = (batch[1][sl, None] - q[0][None, :]) ** 2 + (batch[2][sl, None] - q[1][None, :]) ** 2
                Ks = IC.REGIME[0] * np.exp(float(np.float32(-0.5)) / IC.REGIME[1] * d2)
                worst = max(worst, _gap(r[0][i], r[1][sl] @ Ks))
        print("%s cap=513 model=%d: worst |f* - K*^T alpha| = %.2e of the patch's max-norm, both entries" % (label, model, worst))
        assert worst <= 1e-11


@pytest.mark.parametrize("cap,model", [(1024, 2), (513, 2), (272, 2), (513, 1), (272, 1)])
def test_irls_big_tile_counts(gp, oracle, cap, model):
    """dense_big_kernel<8, 1024, ..., IRLS> at tile counts 1 .. 5, 16 .. 21, 32, 33, 48, 49, 60 .. 64 (every nt mod 4 of the
    four-columns-per-step walk at both ends), sizes on and next to tile edges, two empty patches; the same patches up to 513 and up to
    272 points alone, in slots of 33 and of 17 tile columns.  Model 2 from f = 0 and model 1 from f = 0.25 y (caps 513 and 272).  At
    cap 513 the point-wise entry too, on 37 scattered X* against the oracle, and the read-out of both entries alone: f* against the
    call's own alpha through a NumPy K*, 1e-11.
    Measured on MI355X, worst over the patches (f*, fhat, alpha; of the patch's max-norm).  Model 2: 7.8e-14, 1.7e-14, 1.3e-14 (cap
    1024), 5.0e-14, 1.4e-14, 6.4e-15 (513), 1.9e-14, 1.2e-14, 6.6e-15 (272), 37 X*: 5.8e-14.  Model 1: 2.7e-11, 2.6e-11, 7.1e-10 (513),
    1.4e-13, 2.5e-13, 6.2e-13 (272).  Read-out alone: 5.1e-14 (model 2), 1.1e-13 (model 1)."""
    _tile_counts(gp, oracle, cap, model, "tiles")


NEWTON_N = 272      # model 1: above this many points two calls are compared by the stopping rule (see test_irls_grid_and_pointwise_entries_agree)


def _entries_agree(gp, oracle, model, label="entries"):
    capi, ctx = gp
    batch, _ = IC.take(IC.tile_batch(), IC.cap_index(513))
    off, x0, x1, _ = batch
    xs = _grid(oracle)
    f, al, fh, it, st = _run(ctx, capi, model, batch)
    f2, al2, fh2, it2, st2 = _run(ctx, capi, model, batch, xs=xs)
    assert ctx.last_dense_kernel() == BIG and np.array_equal(st, st2) and np.all(st == 0) and np.all(np.abs(it - it2) <= 1)
    scale = max(float(np.max(np.abs(f))), 1e-6)
    newton = 2.0 * IC.MODELS[model]["tol"]
    worst = {"raw": 0.0, "newton f*": 0.0, "newton fhat": 0.0, "read-out": 0.0}
    for i in np.flatnonzero(np.diff(off) > 0):
        sl = slice(off[i], off[i + 1])
        n = int(off[i + 1] - off[i])
        d = f2[i] - f[i]
        raw = float(np.max(np.abs(d)))
        if model == 2 or n <= NEWTON_N:
            worst["raw"] = max(worst["raw"], raw / scale)
            assert raw <= 1e-11 * scale, (label, model, i, n, raw / scale)
        else:
            dfh = float(np.max(np.abs(fh2[sl] - fh[sl])))
            worst["newton f*"], worst["newton fhat"] = max(worst["newton f*"], raw), max(worst["newton fhat"], dfh)
            assert raw <= newton and dfh <= newton, (label, model, i, n, raw, dfh)
        d2 = (x0[sl, None] - xs[0][None, :]) ** 2 + (x1[sl, None] - xs[1][None, :]) ** 2
        Ks = IC.REGIME[0] * np.exp(float(np.float32(-0.5)) / IC.REGIME[1] * d2)
        res = float(np.max(np.abs(d - (al2[sl] - al[sl]) @ Ks)))
        worst["read-out"] = max(worst["read-out"], res / scale)
        assert res <= 1e-11 * scale, (label, model, i, n, res / scale)
    print("%s cap=513 model=%d, grid against point-wise entry: |df*| = %.2e of max|f*| (1e-11 patches), |df*| = %.2e, |dfhat| = %.2e "
          "absolute (stopping-rule patches), |df* - K*^T dalpha| = %.2e of max|f*|" % (
              label, model, worst["raw"], worst["newton f*"], worst["newton fhat"], worst["read-out"]))


@pytest.mark.parametrize("model", [2, 1])
def test_irls_grid_and_pointwise_entries_agree(gp, oracle, model):
    """The cap-513 sweep through the grid entry and through the point-wise entry on the grid's own points, patch by patch, of max|f*|:
    (i) the same latent mean to 1e-11, test_irls_vs_oracle's statement -- model 2 on every patch, model 1 on the patches up to 272 points;
    (ii) on every patch and under both models, what the ENTRIES contribute to the difference, to the same 1e-11: the two calls are two
    Newton loops, each reports its alpha, and f*_grid - f*_pointwise must equal K*^T (alpha_grid - alpha_pointwise) through a NumPy K*;
    (iii) model 1 above 272 points: |f*_grid - f*_pointwise| and |fhat_grid - fhat_pointwise| <= 2 tol = 2e-7 absolute.
    Why (iii) is not 1e-11: the loop is not bit-reproducible (its solves add into LDS in arrival order), and under model 1 1 / W reaches
    1e4, so f_new = t - W^-1 a cancels and a rounding difference between two calls reaches f amplified by that much -- the noise floor
    because of which test_probit_gpu.py runs model 1 at tol = 1e-7.  What bounds two calls against each other then is the stopping
    rule, not the arithmetic: each loop ends at the first step with max|f_new - f| <= tol, Newton's last step is at least as long as
    the distance left to the mode, so either fhat lies within tol of the mode and the two within 2 tol of each other; f* = K*^T alpha
    reads the same alpha out as fhat = K alpha does, at points between the training points, and moves with it.  (i) stops at 272 points,
    the smallest cap of the sweep, since the amplification grows with the patch.
    Measured on MI355X: (i) 1.9e-14 .. 2.5e-14 (model 2), 4.6e-14 .. 8.3e-14 (model 1 up to 272 points) on four pairs of calls each;
    (ii) 1.8e-14 .. 2.5e-14 (model 2), 6.1e-14 .. 8.0e-14 (model 1); (iii) |df*| 1.6e-11 .. 7.1e-11, |dfhat| 8.6e-11 .. 1.8e-10 absolute.
    Above 272 points the raw gap of model 1 was 3.4e-12 .. 2.0e-11 of max|f*| = 5.5 on five pairs of calls, and the SAME entry called
    twice differs by as much (1.2e-11, 2.9e-12 grid; 2.6e-11 point-wise; alpha by up to 1.0e-9 of its max-norm; equal iteration
    counts): 1e-11 there would pass or fail by rounding luck, which is why (ii) and (iii) take its place."""
    _entries_agree(gp, oracle, model)


# ---------------------------------------------------------------------------------------------------------------- 2, 5. tile counts, four waves

def _w4_tile_counts(gp, oracle, model, label):
    capi, ctx = gp
    batch = IC.w4_batch()
    ref = _ref(("w4", model), lambda: IC.oracle_fit(oracle, batch, model, _grid(oracle)))
    assert np.all(ref[4] == 0)
    got = _run(ctx, capi, model, batch)
    assert ctx.last_dense_kernel() == W4, ctx.last_dense_kernel()
    _check(got, ref, batch[0], model, "%s model=%d" % (label, model))


@pytest.mark.parametrize("model", [2, 1])
def test_irls_w4_tile_counts(gp, oracle, model):
    """dense_big_kernel<4, 256, ..., IRLS> (two workgroups per CU, the HW_ID role swap) on 0, 1 and every tile edge +- 1 up to 256
    points, both models.
    Measured on MI355X (f*, fhat, alpha): 2.8e-14, 9.6e-15, 6.5e-15 (model 2), 2.4e-11, 7.5e-11, 5.9e-11 (model 1)."""
    _w4_tile_counts(gp, oracle, model, "w4 edges")


@pytest.mark.parametrize("case", ["big513", "w4"])
def test_irls_poisoned_lds(gp, oracle, monkeypatch, case):
    """The cap-513 sweep and the four-wave batch with NaN in every LDS word of every CU before the call (GPC_POISON_LDS): the Newton
    loop's vectors live in planes of the solve vectors that the Gaussian instances write and these must not read before writing.
    The cap-513 sweep with everything test_irls_big_tile_counts and test_irls_grid_and_pointwise_entries_agree check there, both models.
    Measured on MI355X: as without the poison -- 5.8e-14, 1.3e-14, 7.5e-15 (cap 513, model 2), 4.0e-11, 2.2e-11, 5.8e-10 (cap 513,
    model 1), 2.9e-14, 8.7e-15, 9.1e-15 (four waves, model 2), 2.4e-11, 1.7e-11, 5.9e-11 (four waves, model 1)."""
    monkeypatch.setenv("GPC_POISON_LDS", "1")
    if case == "big513":
        for model in (2, 1):
            _tile_counts(gp, oracle, 513, model, "poisoned tiles")
        for model in (2, 1):
            _entries_agree(gp, oracle, model, "poisoned entries")
    else:
        for model in (2, 1):
            _w4_tile_counts(gp, oracle, model, "poisoned w4 edges")


# ---------------------------------------------------------------------------------------------------------------- 3. more patches than workgroups

def _many_ref(oracle, which, max_iter=IC.MAX_ITER):
    return _ref(("many", which, max_iter), lambda: IC.oracle_fit(oracle, IC.many_batch(which), 2, VC.xstar(37, seed=90), max_iter=max_iter))


@pytest.mark.parametrize("which,name", [("big", BIG), ("w4", W4)])
def test_irls_more_patches_than_workgroups(gp, oracle, which, name):
    """600 patches of 1 .. 336 points on the eight-wave shape, 1100 of 1 .. 96 points on the four-wave shape: more patches than the
    launch has workgroups (two per CU for up to 512 points, four per CU for up to 256: 512 and 1024 on an MI355X), so the tail is dealt
    by ticket to workgroups whose LDS holds another patch's vectors and hand-over words.
    Four empty patches; three with one NaN label (at the patch's last point, and inside a middle tile) end in the step prologue with
    GPC_STATUS_NAN, iters 0 and NaN in exactly their own rows, and their neighbours in index and a CU count later are compared like
    every other patch.  The same batch in three calls of a third each (no workgroup meets a second patch): equal status, values within
    the oracle tolerance, iters within 1.  Point-wise X* (37 points).
    Measured on MI355X (f*, fhat, alpha): 1.0e-13, 2.2e-14, 1.1e-14 (600 patches), 9.9e-15, 1.3e-14, 8.6e-15 (1100 patches); the thirds
    against the one call 7.0e-14 and 2.6e-14 at worst."""
    capi, ctx = gp
    c = IC.MANY[which]
    batch = IC.many_batch(which)
    off = batch[0]
    xs = VC.xstar(37, seed=90)
    ref = _many_ref(oracle, which)
    bad = list(c["nan"])
    good = np.setdiff1d(np.arange(c["P"]), bad)
    assert ref[4][bad].tolist() == [2, 2, 2] and np.all(ref[4][good] == 0)
    got = _run(ctx, capi, 2, batch, xs=xs)
    assert ctx.last_dense_kernel() == name, ctx.last_dense_kernel()
    assert got[4][bad].tolist() == [capi.STATUS_NAN] * 3 and np.all(got[3][bad] == 0)
    for i in bad:
        for j in (i - 1, i + 1, (i + 256) % c["P"], (i + 512) % c["P"]):
            assert got[4][j] == 0 and np.all(np.isfinite(got[0][j])), (i, j)
    _check(got, ref, off, 2, "many_%s" % which)
    third = -(-c["P"] // 3)
    parts = []
    for k in range(3):
        idx = list(range(third * k, min(third * (k + 1), c["P"])))
        sub, pts = IC.take(batch, idx)
        r = _run(ctx, capi, 2, sub, xs=xs)
        assert ctx.last_dense_kernel() == name
        _check(r, _sub(ref, off, idx, pts), sub[0], 2, "many_%s, third %d" % (which, k))
        parts.append(r)
    f3, al3, fh3, it3, st3 = (np.concatenate([p[j] for p in parts]) for j in range(5))
    assert np.array_equal(st3, got[4]) and np.all(np.abs(it3[good] - got[3][good]) <= 1) and np.array_equal(it3[bad], got[3][bad])
    _check((f3, al3, fh3, it3, st3), got, off, 2, "many_%s, thirds against the one call" % which)


def test_irls_step_cap_on_every_patch(gp, oracle):
    """The 600-patch batch under max_iter = 2 (every healthy patch needs at least 4 steps, test_irls_cases_cpu.py): the cap's exit
    `continue`s into the ticket loop like the other two.  Every non-empty finite patch is GPC_STATUS_NOT_CONVERGED with iters == 2 and
    the oracle's second iterate as outputs; the NaN-label patches are as without the cap.
    Measured on MI355X (f*, fhat, alpha): 9.6e-14, 3.2e-14, 9.1e-15."""
    capi, ctx = gp
    c = IC.MANY["big"]
    batch = IC.many_batch("big")
    ref = _many_ref(oracle, "big", max_iter=2)
    bad = list(c["nan"])
    live = np.setdiff1d(np.flatnonzero(np.diff(batch[0]) > 0), bad)
    assert np.all(ref[4][live] == 5) and np.all(ref[3][live] == 2) and ref[4][bad].tolist() == [2, 2, 2]
    got = _run(ctx, capi, 2, batch, xs=VC.xstar(37, seed=90), max_iter=2)
    assert ctx.last_dense_kernel() == BIG
    assert np.all(got[4][live] == capi.STATUS_NOT_CONVERGED) and np.all(got[3][live] == 2)
    assert got[4][bad].tolist() == [capi.STATUS_NAN] * 3 and np.all(got[3][bad] == 0)
    _check(got, ref, batch[0], 2, "many_big, max_iter=2", want_status=capi.STATUS_NOT_CONVERGED, iters_exact=2)


# ---------------------------------------------------------------------------------------------------------------- 4. whole-batch failure

@pytest.mark.parametrize("which,name", [("w4", W4), ("big", BIG)])
def test_irls_whole_batch_failure_then_healthy_call(gp, oracle, which, name):
    """Model 1 from f = 0 (erf(0) = 0: no finite weight) on the first 40 patches of the many-patch batches: every non-empty patch leaves
    through the badw exit with GPC_STATUS_NAN and iters == 0, the empty one is OK.  The healthy model-2 call right after it on the same
    context (same workspace, same ticket word) must match the oracle.
    Measured on MI355X, the healthy call: 8.6e-15 (four waves), 2.5e-14 (eight waves) on f*."""
    capi, ctx = gp
    full = IC.many_batch(which)
    idx = list(range(40))
    sub, pts = IC.take(full, idx)
    n = np.diff(sub[0])
    xs = VC.xstar(37, seed=90)
    f, al, fh, it, st = _run(ctx, capi, 1, sub, xs=xs, f_init=0.0)
    assert ctx.last_dense_kernel() == name, ctx.last_dense_kernel()
    assert np.all(st[n > 0] == capi.STATUS_NAN) and np.all(st[n == 0] == capi.STATUS_OK) and np.all(it == 0)
    assert np.all(np.isnan(f[n > 0])) and np.all(f[n == 0] == 0) and np.all(np.isnan(al)) and np.all(np.isnan(fh))
    got = _run(ctx, capi, 2, sub, xs=xs)
    assert ctx.last_dense_kernel() == name
    _check(got, _sub(_many_ref(oracle, which), full[0], idx, pts), sub[0], 2, "healthy call after the failed one, %s" % which)


# ---------------------------------------------------------------------------------------------------------------- 6. optional outputs

@pytest.mark.parametrize("shape,name", [("big", BIG), ("w4", W4)])
def test_irls_optional_outputs_null(gp, oracle, shape, name):
    """gpc_dense_irls_fit_predict_dev with alpha_out, fhat_out, iters and status all NULL, then with all of them on a torch side stream
    (gpc_ctx_set_stream): the same f* to 1e-11, and the second call against the oracle.
    Measured on MI355X against the oracle: 3.1e-14 (eight waves), 1.1e-14 (four waves) on f*."""
    import torch
    capi, ctx = gp
    dev = torch.device("cuda:0")
    batch = IC.grid_batch(shape)
    off, x0, x1, lab = batch
    P, N, m = len(off) - 1, int(off[-1]), SZ * SZ
    n_max = int(np.max(np.diff(off)))
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    d_off, d_x0, d_x1, d_y = t(off), t(x0), t(x1), t(lab)
    f0 = torch.full((P, m), float("nan"), dtype=torch.float64, device=dev)
    torch.cuda.synchronize()
    prm, ir = _params(capi, 2), _irls(capi, 2)
    ctx.dense_irls_fit_predict_dev(prm, ir, P, d_off, n_max, N, d_x0, d_x1, d_y, m, None, None, IC.RES, SZ, f0)
    ctx.synchronize()
    assert ctx.last_dense_kernel() == name, ctx.last_dense_kernel()
    f1 = torch.full((P, m), float("nan"), dtype=torch.float64, device=dev)
    al = torch.full((N,), float("nan"), dtype=torch.float64, device=dev)
    fh = torch.full((N,), float("nan"), dtype=torch.float64, device=dev)
    it = torch.full((P,), -1, dtype=torch.int32, device=dev)
    st = torch.full((P,), -1, dtype=torch.int32, device=dev)
    side = torch.cuda.Stream()
    try:
        with torch.cuda.stream(side):
            ctx.set_stream(side.cuda_stream)
            ctx.dense_irls_fit_predict_dev(prm, ir, P, d_off, n_max, N, d_x0, d_x1, d_y, m, None, None, IC.RES, SZ, f1,
                                           alpha_out=al, fhat_out=fh, iters=it, status=st)
        side.synchronize()
    finally:
        ctx.set_stream(None)
    assert ctx.last_dense_kernel() == name
    f0, f1 = f0.cpu().numpy(), f1.cpu().numpy()
    assert np.all(np.isfinite(f0))
    _same(f0, f1, 1e-11, "optional outputs NULL against present")
    ref = _ref(("grid", shape, SZ), lambda: IC.oracle_fit(oracle, batch, 2, _grid(oracle)))
    _check((f1, al.cpu().numpy(), fh.cpu().numpy(), it.cpu().numpy(), st.cpu().numpy()), ref, off, 2, "device pointers, %s" % shape)


# ---------------------------------------------------------------------------------------------------------------- 7. grid sizes

@pytest.mark.parametrize("sz", [1, 2, 15, 16, 17, 31, 32, 33, 40])
@pytest.mark.parametrize("shape,name", [("big", BIG), ("w4", W4)])
def test_irls_grid_sizes(gp, oracle, shape, name, sz):
    """The grid read-out of both shapes: one MFMA output tile (sz <= 16, with sz = 1 a single stored value out of 1024), the 16 | 17
    edge, a full second tile (31, 32), and the per-point loop above 32 (33, 40) -- against the oracle on oracle.grid(res, sz).
    Measured on MI355X, worst over the sizes: 5.4e-14 (eight waves), 1.6e-14 (four waves) on f*."""
    capi, ctx = gp
    batch = IC.grid_batch(shape)
    ref = _ref(("grid", shape, sz), lambda: IC.oracle_fit(oracle, batch, 2, _grid(oracle, sz)))
    assert np.all(ref[4] == 0)
    got = _run(ctx, capi, 2, batch, sz=sz)
    assert ctx.last_dense_kernel() == name, ctx.last_dense_kernel()
    assert got[0].shape == (5, sz * sz)
    _check(got, ref, batch[0], 2, "grid sz=%d, %s" % (sz, shape))
