"""GPU tests of the probit GP's latent predictive variance and occupancy probability (gpc_dense_irls_fit_predict_var[_dev], include/gpc.h):
the IRLS instances of the tiled kernel with the factor export on (csrc/dense_mfma_big.hip) and the row-scaled variance kernel behind
them (dense_variance_big_kernel<true>, csrc/dense_variance.hip), against the NumPy restatement of the definition (irls_var_cases.py,
checked on its own by test_irls_var_cpu.py), through the C-ABI and capi.Mapping.

Gates (irls_var_cases.py): f*, alpha, fhat within FTOL[model] of the patch's max-norm; iters and status equal to the plain entry's on
the same batch; v* within V_GATE = 1e-11 sigma_f^2 of the restatement (E64 = 7e-16, so the rule's 16 E64 branch is not in force); p*
within 1e-14 of the functor applied in NumPy to the GPU's own f*, v*, and within the derivative bound of Phi of the restatement's p*.
On every compared batch: -1e-12 sf <= v* <= sf (1 + 1e-12), p* > 0.5 exactly where f* > 0, and the variance only pulls p* towards 0.5."""
import ctypes as C

import numpy as np
import pytest

from gp_compressor_amd import synth
import irls_cases as IC
import irls_var_cases as IV
import variance_cases as VC

pytestmark = pytest.mark.gpu

BIG, W4 = "dense_mfma_big_irls", "dense_mfma_big_w4_irls"
VAR = " + dense_variance_big"
KEYS = ("f", "v", "p", "alpha", "fhat", "iters", "status")


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


def _params(capi, model):
    return capi.default_params_dense(sigmaf_sq=IC.REGIME[0], l_sq=IC.REGIME[1], noise=IC.REGIME[2], noise_model=model)


def _irls(capi, model, max_iter=IC.MAX_ITER, **kw):
    arg = dict(IC.MODELS[model])
    arg.update(kw)
    return capi.default_params_irls(max_iter=max_iter, **arg)


def _run(ctx, capi, model, batch, xs=None, sz=0, want_v=True, want_p=True, **kw):
    """The host entry; a dict like irls_var_cases.restate's."""
    arg = dict(xs0=xs[0], xs1=xs[1]) if xs is not None else dict(res=IC.RES, sz=sz)
    out = ctx.dense_irls_fit_predict_var(_params(capi, model), _irls(capi, model, **kw), *batch, want_v=want_v, want_p=want_p, **arg)
    return dict(zip(KEYS, out))


def _plain(ctx, capi, model, batch, xs=None, sz=0, **kw):
    arg = dict(xs0=xs[0], xs1=xs[1]) if xs is not None else dict(res=IC.RES, sz=sz)
    return ctx.dense_irls_fit_predict(_params(capi, model), _irls(capi, model, **kw), *batch, **arg)


def _same_bits(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(a.view(np.uint8), b.view(np.uint8))


def _sub(ref, idx, pts):
    """The rows of a full-batch restatement that belong to the sub-batch (idx, pts)."""
    idx = list(idx)
    return dict(f=ref["f"][idx], v=ref["v"][idx], p=ref["p"][idx], alpha=ref["alpha"][pts], fhat=ref["fhat"][pts],
                iters=ref["iters"][idx], status=ref["status"][idx])


def _gap(a, b):
    return float(np.max(np.abs(a - b))) / max(float(np.max(np.abs(b))), 1e-300) if b.size else 0.0


def _properties(got, off, model, label):
    """Test 7, on every patch of a call: the range of v*, the side of p*, and that the variance only pulls p* towards 0.5."""
    f, v, p = got["f"], got["v"], got["p"]
    live = np.isin(got["status"], (0, 5))
    assert np.all(v[live] >= IV.V_LO) and np.all(v[live] <= IV.V_HI), (label, float(v[live].min()), float(v[live].max()))
    if model == 2 and p is not None:
        assert np.array_equal(p[live] > 0.5, f[live] > 0.0), label
        assert np.all(np.abs(p[live] - 0.5) <= np.abs(IV.phi(f[live], 0.0) - 0.5) + 1e-14), label
        assert np.all(p[live] >= 0.0) and np.all(p[live] <= 1.0), label


def _check(got, ref, plain, off, model, label, pick=None, want_status=0):
    """GPU against the restatement, patch by patch (pick: these patches only); iters and status against the plain entry's."""
    n = np.diff(off)
    assert np.array_equal(got["status"], plain[4]) and np.array_equal(got["iters"], plain[3]), (
        label, np.flatnonzero(got["status"] != plain[4])[:8], np.flatnonzero(got["iters"] != plain[3])[:8])
    _properties(got, off, model, label)
    worst = dict(f=0.0, fhat=0.0, alpha=0.0, v=0.0, p_self=0.0, p=0.0)
    for i in (range(len(n)) if pick is None else pick):
        sl = slice(off[i], off[i + 1])
        assert got["status"][i] == ref["status"][i], (label, i, got["status"][i], ref["status"][i])
        if n[i] == 0:
            assert got["status"][i] == 0 and got["iters"][i] == 0 and np.all(got["f"][i] == 0.0) and np.all(got["v"][i] == IV.SF), (label, i)
            assert got["p"] is None or np.all(got["p"][i] == 0.5), (label, i)
            continue
        if ref["status"][i] == 2:
            assert np.all(np.isnan(got["f"][i])) and np.all(np.isnan(got["v"][i])) and (got["p"] is None or np.all(np.isnan(got["p"][i]))), (label, i)
            assert np.all(np.isnan(got["alpha"][sl])) and np.all(np.isnan(got["fhat"][sl])), (label, i)
            continue
        assert got["status"][i] == want_status, (label, i, got["status"][i])
        assert abs(int(got["iters"][i]) - int(ref["iters"][i])) <= 1, (label, i, got["iters"][i], ref["iters"][i])
        for k in ("f", "v", "alpha", "fhat"):
            a = got[k][i] if k in ("f", "v") else got[k][sl]
            assert np.all(np.isfinite(a)), (label, i, k)
        g = dict(f=_gap(got["f"][i], ref["f"][i]), fhat=_gap(got["fhat"][sl], ref["fhat"][sl]), alpha=_gap(got["alpha"][sl], ref["alpha"][sl]))
        ev = float(np.max(np.abs(got["v"][i] - ref["v"][i])))
        for k, e in g.items():
            worst[k] = max(worst[k], e)
        worst["v"] = max(worst["v"], ev / IV.SF)
        print("%s patch %d n=%d: f* %.2e fhat %.2e alpha %.2e of max-norm, v* %.2e" % (label, i, n[i], g["f"], g["fhat"], g["alpha"], ev))
        assert max(g.values()) <= IC.FTOL[model], (label, i, int(n[i]), g)
        assert ev <= IV.V_GATE, (label, i, int(n[i]), ev)
        if model == 2 and got["p"] is not None:
            assert np.all(np.isfinite(got["p"][i])), (label, i)
            e_self = float(np.max(np.abs(got["p"][i] - IV.phi(got["f"][i], got["v"][i]))))
            d = np.abs(got["p"][i] - ref["p"][i])
            gate = IV.p_gate(float(np.max(np.abs(ref["f"][i]))), ref["f"][i], ref["v"][i], model)
            worst["p_self"], worst["p"] = max(worst["p_self"], e_self), max(worst["p"], float(np.max(d)))
            assert e_self <= IV.P_SELF_TOL, (label, i, e_self)
            assert np.all(d <= gate), (label, i, float(np.max(d)), float(np.min(gate)))
    print("%s: worst f* %.2e, fhat %.2e, alpha %.2e of the patch's max-norm; v* %.2e of sigma_f^2; p* %.2e against the functor on the GPU's "
          "own f*, v*, %.2e against the restatement" % (label, worst["f"], worst["fhat"], worst["alpha"], worst["v"], worst["p_self"], worst["p"]))


# ---------------------------------------------------------------------------------------------------------------- 1. tile edges, both shapes

def test_var_w4_tile_edges(gp, oracle):
    """The four-wave IRLS instance with the export on, and the variance kernel on its 16-column slots: 0, 1 and every tile edge +- 1 up
    to 256 points, 400 scattered X*, model 2.
    Measured on MI355X: f*, fhat, alpha 1.2e-14, 1.7e-14, 1.2e-14 of the max-norm; v* 1.4e-15 of sigma_f^2; p* 2.2e-16 (own f*, v*), 9.6e-15."""
    capi, ctx = gp
    batch, xs = IC.w4_batch(), IV.xs400("w4")
    plain = _plain(ctx, capi, 2, batch, xs=xs)
    got = _run(ctx, capi, 2, batch, xs=xs)
    assert ctx.last_dense_kernel() == W4 + VAR, ctx.last_dense_kernel()
    _check(got, IV.w4_ref(oracle), plain, batch[0], 2, "w4 edges")


@pytest.mark.parametrize("cap", IC.CAPS)
def test_var_big_tile_counts(gp, oracle, cap):
    """The eight-wave IRLS instance with the export on, in slots of 64, 33 and 17 tile columns: tile counts on both sides of the variance
    kernel's super-row edges (16 | 17, 32 | 33, 48 | 49), 400 scattered X*, model 2.
    Measured on MI355X (f*, fhat, alpha; v*; p* on own f*, v*; p*): 5.3e-14, 8.9e-14, 4.6e-14; 1.7e-15; 2.2e-16; 3.9e-14 (cap 1024),
    3.2e-14, 3.8e-14, 2.2e-14; 1.3e-15; 2.2e-16; 2.8e-14 (513), 1.2e-14, 1.8e-14, 9.7e-15; 1.1e-15; 2.2e-16; 9.2e-15 (272)."""
    capi, ctx = gp
    full, xs = IC.tile_batch(), IV.xs400("tiles")
    idx = IC.cap_index(cap)
    batch, pts = IC.take(full, idx)
    assert int(np.max(np.diff(batch[0]))) == cap
    plain = _plain(ctx, capi, 2, batch, xs=xs)
    got = _run(ctx, capi, 2, batch, xs=xs)
    assert ctx.last_dense_kernel() == BIG + VAR, ctx.last_dense_kernel()
    _check(got, _sub(IV.tile_ref(oracle), idx, pts), plain, batch[0], 2, "tiles cap=%d" % cap)


def test_var_model1_variance_only(gp, oracle):
    """Model 1 on the sizes up to MODEL1_CAP: v* (and f*, alpha, fhat) against the restatement; p_star is refused with GPC_EINVAL.
    Measured on MI355X: f*, fhat, alpha 1.4e-11, 2.1e-11, 7.8e-11 of the max-norm (FTOL 1e-6); v* 2.7e-12 of sigma_f^2 (gate 1e-11)."""
    capi, ctx = gp
    full, xs = IC.tile_batch(), IV.xs400("tiles")
    idx = IC.cap_index(IC.MODEL1_CAP)
    batch, pts = IC.take(full, idx)
    plain = _plain(ctx, capi, 1, batch, xs=xs)
    got = _run(ctx, capi, 1, batch, xs=xs, want_p=False)
    assert ctx.last_dense_kernel() == BIG + VAR and got["p"] is None
    _check(got, _sub(IV.tile_ref(oracle, 1), idx, pts), plain, batch[0], 1, "tiles model=1")
    with pytest.raises(capi.GpcError) as e:
        _run(ctx, capi, 1, batch, xs=xs)
    assert e.value.code == capi.GPC_EINVAL


# ---------------------------------------------------------------------------------------------------------------- 2. m sweep

@pytest.mark.parametrize("m", [1, 15, 16, 17, 128, 129, 400])
@pytest.mark.parametrize("shape,name", [("big", BIG), ("w4", W4)])
def test_var_m_sweep(gp, oracle, shape, name, m):
    """X* counts of one block, a block edge, exactly one round of eight waves, the first block of a second round, and 400.
    Measured on MI355X, worst over the counts: f* 3.5e-14, v* 1.3e-15, p* 1.5e-14 (eight waves); 9.7e-15, 1.2e-15, 9.6e-15 (four waves)."""
    capi, ctx = gp
    batch, xs = IC.grid_batch(shape), VC.xstar(m, seed=73)
    plain = _plain(ctx, capi, 2, batch, xs=xs)
    got = _run(ctx, capi, 2, batch, xs=xs)
    assert ctx.last_dense_kernel() == name + VAR, ctx.last_dense_kernel()
    assert got["f"].shape == got["v"].shape == got["p"].shape == (5, m)
    _check(got, IV.grid_ref(oracle, shape, m), plain, batch[0], 2, "m=%d, %s" % (m, shape))


# ---------------------------------------------------------------------------------------------------------------- 3. grid form

@pytest.mark.parametrize("sz", [1, 4, 20, 33])
@pytest.mark.parametrize("shape,name", [("big", BIG), ("w4", W4)])
def test_var_grid_form_is_the_pointwise_call(gp, shape, name, sz):
    """xs0 == NULL: the library materialises the sz x sz grid as points -- the same bits as the point-wise call on synth.grid(res, sz)
    (sz = 33 is above the separable read-out's limit of 32).
    Two calls give the same bits because every sum across waves in the tiled kernel has a fixed order (the backward solve's partial
    sums per wave, the grid read-out wave after wave)."""
    capi, ctx = gp
    batch = IC.grid_batch(shape)
    g = _run(ctx, capi, 2, batch, sz=sz)
    assert ctx.last_dense_kernel() == name + VAR, ctx.last_dense_kernel()
    q = _run(ctx, capi, 2, batch, xs=synth.grid(IC.RES, sz))
    assert g["f"].shape == (5, sz * sz) and np.all(g["status"] == 0) and np.all(np.isfinite(g["p"]))
    for k in KEYS:
        assert _same_bits(g[k], q[k]), (k, float(np.nanmax(np.abs(g[k] - q[k]))))


# ---------------------------------------------------------------------------------------------------------------- 4. both outputs NULL

@pytest.mark.parametrize("shape,name", [("big", BIG), ("w4", W4)])
def test_var_both_outputs_null_is_the_plain_entry(gp, shape, name):
    """v_star == p_star == NULL: the call forwards to gpc_dense_irls_fit_predict -- the same kernel (name without the suffix) and bits.
    The forwarded call is the plain entry (one `return` in dense_api.hip), and the plain entry is reproducible from call to call."""
    capi, ctx = gp
    batch = IC.grid_batch(shape)
    for arg in (dict(sz=20), dict(xs=VC.xstar(37, seed=75))):
        plain = _plain(ctx, capi, 2, batch, **arg)
        got = _run(ctx, capi, 2, batch, want_v=False, want_p=False, **arg)
        assert ctx.last_dense_kernel() == name, ctx.last_dense_kernel()
        assert got["v"] is None and got["p"] is None
        for k, a in zip(("f", "alpha", "fhat", "iters", "status"), plain):
            assert _same_bits(got[k], a), (k, arg.keys())


# ---------------------------------------------------------------------------------------------------------------- 5. pinned step count

@pytest.mark.parametrize("max_iter", [1, 2, 6])
@pytest.mark.parametrize("shape,name", [("big", BIG), ("w4", W4)])
def test_var_pinned_step_count(gp, oracle, shape, name, max_iter):
    """tol = 0 and a step cap: every non-empty patch is GPC_STATUS_NOT_CONVERGED, and f*, v*, p* are those of the last iterate -- finite
    and within the gates of the restatement run for the same count (the variance kernel takes that status as a valid fit).  The batch
    leaves out the single-point patch of the grid batches, whose scalar iteration reaches its fixed point exactly (pinned_batch).
    Measured on MI355X, worst over the counts: f* 2.5e-14, v* 1.2e-15, p* 1.3e-14 (eight waves); 8.5e-15, 8.9e-16, 4.6e-15 (four waves)."""
    capi, ctx = gp
    batch, xs = IV.pinned_batch(shape), VC.xstar(37, seed=74)
    n = np.diff(batch[0])
    plain = _plain(ctx, capi, 2, batch, xs=xs, max_iter=max_iter, tol=0.0)
    got = _run(ctx, capi, 2, batch, xs=xs, max_iter=max_iter, tol=0.0)
    assert ctx.last_dense_kernel() == name + VAR
    assert np.all(got["status"][n > 0] == capi.STATUS_NOT_CONVERGED) and np.all(got["iters"][n > 0] == max_iter)
    assert all(np.all(np.isfinite(got[k])) for k in ("f", "v", "p"))
    _check(got, IV.pinned_ref(oracle, shape, max_iter), plain, batch[0], 2, "max_iter=%d tol=0, %s" % (max_iter, shape),
           want_status=capi.STATUS_NOT_CONVERGED)


# ---------------------------------------------------------------------------------------------------------------- 6. more patches than workgroups

@pytest.mark.parametrize("which,name", [("big", BIG), ("w4", W4)])
def test_var_more_patches_than_workgroups(gp, oracle, which, name):
    """600 patches on the eight-wave shape, 1100 on the four-wave shape: the ticket hands out patches, and the factor slot must be the
    patch's.  Empty patches give exactly (0, sf, 0.5); the three NaN-label patches status 2 and NaN in all three outputs, their
    neighbours finite; 64 patches (the edges and random ones) against the restatement; a second call gives identical bits.
    Measured on MI355X: f*, fhat, alpha 2.0e-14, 3.4e-14, 1.6e-14 of the max-norm, v* 1.0e-15, p* 7.6e-15 (600 patches); 5.4e-15,
    6.8e-15, 4.8e-15, 7.8e-16, 3.0e-15 (1100 patches)."""
    capi, ctx = gp
    c = IC.MANY[which]
    batch, xs = IC.many_batch(which), VC.xstar(37, seed=90)
    plain = _plain(ctx, capi, 2, batch, xs=xs)
    got = _run(ctx, capi, 2, batch, xs=xs)
    assert ctx.last_dense_kernel() == name + VAR, ctx.last_dense_kernel()
    for i in c["empty"]:
        assert np.all(got["f"][i] == 0.0) and np.all(got["v"][i] == IV.SF) and np.all(got["p"][i] == 0.5) and got["status"][i] == 0
    for i in c["nan"]:
        assert got["status"][i] == capi.STATUS_NAN and all(np.all(np.isnan(got[k][i])) for k in ("f", "v", "p")), i
        for j in (i - 1, i + 1):
            assert got["status"][j] == 0 and all(np.all(np.isfinite(got[k][j])) for k in ("f", "v", "p")), (i, j)
    live = np.setdiff1d(np.arange(c["P"]), list(c["nan"]))
    assert np.all(got["status"][live] == 0) and all(np.all(np.isfinite(got[k][live])) for k in ("f", "v", "p"))
    _check(got, IV.many_ref(oracle, which), plain, batch[0], 2, "many_%s" % which, pick=IV.many_pick(which))
    again = _run(ctx, capi, 2, batch, xs=xs)
    for k in KEYS:
        assert _same_bits(got[k], again[k]), k


# ---------------------------------------------------------------------------------------------------------------- 9. the map's occupancy probability

def test_mapping_occupancy_probability(gp):
    """Mapping.occupancy_probability on the plane-cloud model of test_mapping_gpu.py with one scan added: f equals Mapping.occupancy's
    within FTOL; p, v and status equal a direct dense_irls_fit_predict_var_dev call on occupancy_batch(cells) bit for bit; a leaf without
    observed cells gives p == 0.5 and v == sigmaf_sq."""
    import torch
    import mapping_cases as mc
    capi, ctx = gp
    res, sz = mc.RES, mc.SZ
    xyz, rgb = mc.model_cloud()
    pt = ctx.project_cloud(ctx.make_cloud(xyz, rgb), res, sz)
    b = pt.fetch()
    hyp = dict(sigmaf_sq=1.0, l_sq=(res / 5) ** 2)
    gd = capi.Sparse(ctx, capi.default_params_sparse(1, noise=1e-3, capacity=24, **hyp), pt.view.P, 1)
    gc = capi.Sparse(ctx, capi.default_params_sparse(3, noise=1.0, capacity=100, **hyp), pt.view.P, 3)
    perm = synth.sattolo_perms(b["off"], seed=6)
    assert np.all(gd.add(b["off"], b["x0"], b["x1"], b["y"][None, :], perm) == 0)
    assert np.all(gc.add(b["off"], b["x0"], b["x1"], np.ascontiguousarray(b["rgb"]), perm) == 0)
    S, cs = mc.overlapping_scan()
    mp = capi.Mapping(ctx, pt, gd, gc, params=capi.default_params_registration(step=1e-7, tol=1e300, min_steps=2, max_steps=10), min_nbr=20)
    try:
        steps, inserted = mp.add_cloud(ctx.make_cloud(S, cs))
        assert inserted
        prm = capi.default_params_dense(sigmaf_sq=1.0, l_sq=(res / 4) ** 2, noise=0.25, noise_model=2)
        P, m = mp.patches.view.P, mp.patches.view.m
        p, f, v, st = (a.cpu().numpy() for a in mp.occupancy_probability(prm))
        f0, st0 = (a.cpu().numpy() for a in mp.occupancy(prm))
        assert p.shape == f.shape == v.shape == (P, m) and np.array_equal(st, st0) and np.all(st == 0)
        for i in range(P):
            assert _gap(f[i], f0[i]) <= IC.FTOL[2] or np.all(f0[i] == 0.0), (i, _gap(f[i], f0[i]))
        cells = mp.cells.cpu().numpy()
        seen = (cells != 0).any(axis=1)
        assert seen.any() and (~seen).any()
        assert np.all(p[~seen] == 0.5) and np.all(v[~seen] == 1.0) and np.all(f[~seen] == 0.0)
        assert np.all(np.isfinite(p)) and np.all((p[seen] >= 0.0) & (p[seen] <= 1.0)) and np.array_equal(p > 0.5, f > 0.0)
        off, x0, x1, y, n_total, n_max = mp.patches.occupancy_batch(mp.cells)
        dev = mp.cells.device
        p2, f2, v2 = (torch.zeros((P, m), dtype=torch.float64, device=dev) for _ in range(3))
        st2 = torch.full((P,), -1, dtype=torch.int32, device=dev)
        torch.cuda.synchronize()
        ctx.dense_irls_fit_predict_var_dev(prm, capi.default_params_irls(), P, off, n_max, n_total, x0, x1, y, m, None, None, res, sz, f2,
                                           v_star=v2, p_star=p2, status=st2)
        ctx.synchronize()
        p2, v2, st2 = p2.cpu().numpy(), v2.cpu().numpy(), st2.cpu().numpy()
        print("direct call against Mapping.occupancy_probability: max |dp| %.2e, |dv| %.2e" % (np.max(np.abs(p - p2)), np.max(np.abs(v - v2))))
        assert _same_bits(st, st2)
        assert _same_bits(p, p2) and _same_bits(v, v2), (float(np.max(np.abs(p - p2))), float(np.max(np.abs(v - v2))))
    finally:
        mp.close()


# ---------------------------------------------------------------------------------------------------------------- 10. errors

def test_var_errors(gp):
    """NULL irls, a Gaussian noise_model, p_star with model 1: GPC_EINVAL.  P == 0 and m == 0: GPC_OK.  A dead context: GPC_EINVAL."""
    capi, ctx = gp
    lib = ctx.lib
    off, x0, x1, lab = IC.grid_batch("w4")
    P, m = len(off) - 1, 16
    xs = VC.xstar(m, seed=76)
    f, v, p = (np.zeros((P, m)) for _ in range(3))
    ptr = capi._ptr

    def call(h, prm, ir, P_=P, m_=m, v_=v, p_=p):
        return lib.gpc_dense_irls_fit_predict_var(h, C.byref(prm), C.byref(ir) if ir is not None else None, P_, ptr(off), ptr(x0), ptr(x1),
                                                  ptr(lab), m_, ptr(xs[0]), ptr(xs[1]), 0.0, 0, ptr(f), ptr(v_), ptr(p_), None, None, None, None)
    ir = _irls(capi, 2)
    assert call(ctx.h, _params(capi, 2), None) == capi.GPC_EINVAL
    assert call(ctx.h, _params(capi, 0), ir) == capi.GPC_EINVAL
    assert call(ctx.h, _params(capi, 1), _irls(capi, 1)) == capi.GPC_EINVAL
    assert call(ctx.h, _params(capi, 1), _irls(capi, 1), p_=None) == capi.GPC_OK          # v_star alone works with model 1
    assert call(ctx.h, _params(capi, 2), ir, P_=0) == capi.GPC_OK
    assert call(ctx.h, _params(capi, 2), ir, m_=0) == capi.GPC_OK
    assert call(ctx.h, _params(capi, 2), ir) == capi.GPC_OK and np.all(np.isfinite(p)) and np.all(np.isfinite(v))
    # a dead context: destroyed while a child lives (the struct stays until the child goes)
    dead = capi.Context(0)
    child = capi.Sparse(dead, capi.default_params_sparse(1), 1, 1)
    h, dead.h = dead.h, None
    lib.gpc_ctx_destroy(h)
    try:
        assert call(h, _params(capi, 2), ir) == capi.GPC_EINVAL
    finally:
        child.close()
