"""GPU tests of the regression GP's log marginal likelihood (gpc_dense_fit_predict_ev[_dev]) and of the selection among candidate
hyper-parameters by it (gpc_dense_select[_dev]), include/gpc.h: the read-out and keep-best kernels of csrc/dense_evidence.hip behind the
three MFMA fits with the factor export on, and the generic kernel's own read-out, against the NumPy restatement of the definition
(dense_ev_cases.py, checked on its own by test_dense_ev_cpu.py).

Gate (dense_ev_cases.py): log_ev within 1e-11 G of the restatement, G = 1 + 0.5 |y^T alpha| + |sum log L_jj| + 0.5 n log 2 pi
(E64 = 1.5e-15, so the rule's 16 E64 branch is not in force).  Measured on MI355X, worst gap over all tests here: 1.9e-15 G (three
planes on the register route, MEDIUM regime); every tile edge from 0 to 1024 points stays below 1.7e-15 G.  Everything else is compared bit for bit, except f* and alpha of the
evidence-only calls, which are the export-on fit's own and are held to the project's FTOL / ATOL (test_dense_gpu.py) against the
restatement, in both regimes and on every route.

Run to run, the one-wave, the tiled and the generic kernel repeat every output bit for bit.  The register kernel's backward solve adds
with LDS atomics in no fixed order (test_dense_gpu.py::test_dense_golden), so its alpha -- and f* and log_ev, which are formed from it --
repeats to a rounding or two: where a test compares two calls on that route, v* and the status are compared bit for bit and the rest
within RUN_TOL = 1e-12 of the max-norm (of G for log_ev), the bound test_dense_golden holds such pairs to.  Bit contracts that involve
alpha are therefore pinned on the one-wave route (GPC_W1_MIN_P=1, a largest patch of 193 .. 256 points) and on the tiled route."""
import ctypes as C

import numpy as np
import pytest

import dense_ev_cases as DC
import variance_cases as VC

pytestmark = pytest.mark.gpu

FTOL, ATOL = 1e-9, 1e-8          # tests/test_dense_gpu.py
RUN_TOL = 1e-12                  # two calls on the register kernel (tests/test_dense_gpu.py::test_dense_golden)
XS = VC.xstar(5, seed=96)
BIG = "dense_mfma_big + dense_variance_big"
W1 = "dense_mfma_w1 + dense_variance"
# an evidence-only call runs no variance kernel, and says so
BIG_EV = "dense_mfma_big + dense_gauss_evidence"
W1_EV = "dense_mfma_w1 + dense_gauss_evidence"
KEYS = ("f", "v", "alpha", "status", "log_ev")
SWITCHES = ("GPC_FORCE_GENERIC", "GPC_FORCE_BIG", "GPC_BIG_NO_W2", "GPC_BIG_NO_W4", "GPC_NO_W1", "GPC_NO_W1_512", "GPC_W2", "GPC_W1_MIN_P",
            "GPC_W1_SLOTS", "GPC_VAR_W4", "GPC_NO_SPLIT", "GPC_HOST_NO_PIPELINE", "GPC_HOST_ONE_STREAM", "GPC_POISON_LDS")


@pytest.fixture(scope="module")
def gp():
    from gp_compressor_amd import capi
    capi.load()          # raises if the HIP library is missing: no fallback
    ctx = capi.Context(0)
    yield capi, ctx
    ctx.close()


@pytest.fixture(autouse=True)
def _plain_dispatch(monkeypatch):
    for e in SWITCHES:
        monkeypatch.delenv(e, raising=False)


def _params(capi, regime, **kw):
    return capi.default_params_dense(sigmaf_sq=regime[0], l_sq=regime[1], noise=regime[2], **kw)


def _ev(ctx, capi, regime, batch, xs=XS, want_v=True, **kw):
    out = ctx.dense_fit_predict_ev(_params(capi, regime, **kw), *batch, xs0=xs[0], xs1=xs[1], want_v=want_v)
    return dict(zip(KEYS, out))


def _same_bits(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(a.view(np.uint8), b.view(np.uint8))


def _same_run(a, b, exact, key, G=None):
    """Two calls' outputs: bit for bit, or (register route) alpha and what is formed from it within RUN_TOL."""
    if exact or key in ("v", "status", "v_star", "best"):
        assert _same_bits(a, b), key
    elif key in ("log_ev", "log_ev_all"):
        assert np.all(np.abs(a - b) <= RUN_TOL * G), key
    else:
        _close(a, b, RUN_TOL)


def _register_name(n_max):
    return "dense_mfma_nt%d + dense_gauss_evidence" % (4 if n_max <= 64 else 8 if n_max <= 128 else 12 if n_max <= 192 else 16)


def _check_ev(got, ref, off, label, pick=None):
    """log_ev of the GPU against the restatement's, patch by patch and plane by plane; returns the worst gap in units of G."""
    n = np.diff(off)
    worst = 0.0
    for i in (range(len(n)) if pick is None else pick):
        assert got["status"][i] == ref["status"][i], (label, i, got["status"][i], ref["status"][i])
        if n[i] == 0:
            assert np.all(got["log_ev"][i] == 0.0) and got["status"][i] == 0, (label, i, got["log_ev"][i])
            continue
        if ref["status"][i] != 0:
            assert np.all(np.isnan(got["log_ev"][i])), (label, i, got["log_ev"][i])
            continue
        for c in range(got["log_ev"].shape[1]):
            assert np.isfinite(got["log_ev"][i, c]), (label, i, c)
            e = abs(float(got["log_ev"][i, c]) - float(ref["log_ev"][i, c]))
            rel = e / float(ref["G"][i, c])
            worst = max(worst, rel)
            print("%s patch %d plane %d n=%d: log_ev %.6f against %.6f, gap %.2e G" % (label, i, c, n[i], got["log_ev"][i, c],
                                                                                    ref["log_ev"][i, c], rel))
            assert e <= DC.gate(ref["G"][i, c]), (label, i, c, int(n[i]), e, float(ref["log_ev"][i, c]))
    print("%s: worst log_ev gap %.2e G (gate %.0e)" % (label, worst, DC.GATE_RTOL))
    return worst


def _close(f, want, tol):
    scale = max(float(np.max(np.abs(want))), 1e-300) if want.size else 1.0
    err = float(np.max(np.abs(f - want))) if want.size else 0.0
    assert err <= tol * scale, (err, scale)


def _ref(regime_name, key, batch, dn=1):
    return DC.cached((regime_name, key, dn), lambda: DC.restate(DC.REGIMES[regime_name], batch, dn))


# ---------------------------------------------------------------------------------------------------------------- 1. tile and lane edges

@pytest.mark.parametrize("name", sorted(DC.REGIMES))
@pytest.mark.parametrize("n", DC.EDGE_SIZES)
def test_ev_tile_and_lane_edges(gp, n, name):
    """One patch of every size at which a read-out can go wrong: 0, 1, the tile edge (15 .. 17), the wave sum's wrap (63 .. 65), the
    register kernel's largest instances (192 | 193, 256), the change of the export layout (256 | 257), the tiled kernel's slots of 17
    | 18 and 32 | 33 tile columns (272 | 273, 511 .. 513) and its largest (1023, 1024).  An evidence-only call: the fit predicts f*
    itself with the export on."""
    capi, ctx = gp
    batch = DC.edge_patch(n)
    got = _ev(ctx, capi, DC.REGIMES[name], batch, want_v=False)
    assert got["v"] is None
    assert ctx.last_dense_kernel() == (_register_name(max(n, 1)) if n <= 256 else BIG_EV), ctx.last_dense_kernel()
    ref = _ref(name, ("edge", n), batch)
    _check_ev(got, ref, batch[0], "edge n=%d %s" % (n, name))
    _close(got["alpha"], ref["alpha"], ATOL)
    _close(got["f"], DC.predict(DC.REGIMES[name], batch, ref["alpha"], XS), FTOL)


# ---------------------------------------------------------------------------------------------------------------- 2. every route

@pytest.mark.parametrize("name", sorted(DC.REGIMES))
def test_ev_every_route_agrees(gp, monkeypatch, name):
    """One sub-batch of at most 256 points on the generic kernel (its own pivots, no export), the register kernel and the one-wave
    kernel: each within the gate of the restatement, under the name expected.  GPC_FORCE_BIG does not apply to it: the 256-point
    shapes of the tiled kernel export no factor, and the variance route sends such a batch to the generic kernel; where the tiled
    kernel is the route anyway (a batch beyond 256 points) the switch changes no bit."""
    capi, ctx = gp
    batch = DC.route_batch()
    ref = _ref(name, "route", batch)
    runs = {}
    for label, env, kernel in (("generic", {"GPC_FORCE_GENERIC": "1"}, "dense_generic"), ("force_big", {"GPC_FORCE_BIG": "1"}, "dense_generic"),
                               ("register", {}, "dense_mfma_nt16 + dense_gauss_evidence"), ("one-wave", {"GPC_W1_MIN_P": "1"}, W1_EV)):
        for k, v in env.items():
            monkeypatch.setenv(k, v)
        runs[label] = _ev(ctx, capi, DC.REGIMES[name], batch, want_v=False)
        assert ctx.last_dense_kernel() == kernel, (label, ctx.last_dense_kernel())
        for k in env:
            monkeypatch.delenv(k)
        _check_ev(runs[label], ref, batch[0], "%s %s" % (label, name))
        # f* and alpha of the export-on fit that predicts for itself, on every route (the one-wave kernel ran this combination -- export on,
        # the true K factorised, m > 0 -- for no caller before the evidence entry)
        _close(runs[label]["alpha"], ref["alpha"], ATOL)
        _close(runs[label]["f"], DC.predict(DC.REGIMES[name], batch, ref["alpha"], XS), FTOL)
    assert _same_bits(runs["generic"]["log_ev"], runs["force_big"]["log_ev"])
    big = VC._mixed_batch([300, 270], seed=77)
    plain = _ev(ctx, capi, DC.REGIMES[name], big, want_v=False)
    assert ctx.last_dense_kernel() == BIG_EV
    monkeypatch.setenv("GPC_FORCE_BIG", "1")
    forced = _ev(ctx, capi, DC.REGIMES[name], big, want_v=False)
    assert ctx.last_dense_kernel() == BIG_EV and _same_bits(plain["log_ev"], forced["log_ev"])
    monkeypatch.setenv("GPC_FORCE_GENERIC", "1")
    anchor = _ev(ctx, capi, DC.REGIMES[name], big, want_v=False)
    assert ctx.last_dense_kernel() == "dense_generic"
    rb = _ref(name, "route_big", big)
    _check_ev(plain, rb, big[0], "tiled %s" % name)
    _check_ev(anchor, rb, big[0], "generic beyond 256 %s" % name)


# ---------------------------------------------------------------------------------------------------------------- 3. one-wave slot reuse

def test_ev_one_wave_slot_reuse(gp, monkeypatch):
    """20 patches of 193 .. 256 points in launches of 8, 8 and 4 that reuse eight factor slots: the read-out of a launch runs before the
    next launch overwrites its slots.  Every patch is right, and the bits are those of one launch with a slot per patch."""
    capi, ctx = gp
    batch = DC.slot_batch()
    monkeypatch.setenv("GPC_W1_MIN_P", "1")
    whole = _ev(ctx, capi, VC.DEFAULT, batch)
    assert ctx.last_dense_kernel() == W1
    monkeypatch.setenv("GPC_W1_SLOTS", "8")
    parts = _ev(ctx, capi, VC.DEFAULT, batch)
    assert ctx.last_dense_kernel() == W1
    _check_ev(parts, _ref("DEFAULT", "slots", batch), batch[0], "three launches")
    for k in KEYS:
        assert _same_bits(whole[k], parts[k]), k


# ---------------------------------------------------------------------------------------------------------------- 4. grid wrap

def test_ev_readout_grid_wraps_over_identical_copies(gp):
    """The read-out runs at most 8 workgroups of 4 waves per CU and strides over the patches: with more than 32 CUs patches its loop takes
    a second trip.  The batch is copies of one 3-point patch, so every copy carries the first copy's bits, and the first is right."""
    import torch
    capi, ctx = gp
    one = DC.edge_patch(3)
    k = 32 * torch.cuda.get_device_properties(0).multi_processor_count + 37
    off = (3 * np.arange(k + 1)).astype(np.int32)
    batch = (off, np.tile(one[1], k), np.tile(one[2], k), np.tile(one[3], (1, k)))
    got = _ev(ctx, capi, VC.DEFAULT, batch, xs=VC.xstar(1, seed=97), want_v=False)
    assert np.all(got["status"] == 0)
    _check_ev(got, _ref("DEFAULT", ("edge", 3), one), one[0], "first copy", pick=[0])
    assert np.all(got["log_ev"].view(np.uint64) == got["log_ev"].view(np.uint64)[0])


# ---------------------------------------------------------------------------------------------------------------- 5. planes

@pytest.mark.parametrize("big", [False, True])
def test_ev_planes(gp, big):
    """ny = 3 on the register and on the tiled route: a log_ev per plane; a NaN in one plane's y poisons that plane of that patch only; a
    repeated point without a noise term is GPC_STATUS_NOT_SPD with NaN in every plane, and leaves the other patches their bits."""
    capi, ctx = gp
    batch = DC.plane_batch(big)
    off, x0, x1, y = batch
    clean = _ev(ctx, capi, VC.MEDIUM, batch)
    assert ctx.last_dense_kernel() == (BIG if big else "dense_mfma_nt12 + dense_variance"), ctx.last_dense_kernel()
    assert clean["log_ev"].shape == (len(off) - 1, 3)
    _check_ev(clean, _ref("MEDIUM", ("planes", big), batch), off, "planes big=%s" % big)
    yp = y.copy()
    yp[1, off[3] + 5] = np.nan
    pois = _ev(ctx, capi, VC.MEDIUM, (off, x0, x1, yp))
    assert np.all(pois["status"] == 0) and not np.isfinite(pois["log_ev"][3, 1])
    keep = np.ones_like(clean["log_ev"], dtype=bool)
    keep[3, 1] = False
    G = _ref("MEDIUM", ("planes", big), batch)["G"]
    _same_run(pois["log_ev"][keep], clean["log_ev"][keep], big, "log_ev", G[keep])
    zero = _ev(ctx, capi, VC.ZERO_NOISE, batch)
    assert np.all(zero["status"] == 0) and np.all(np.isfinite(zero["log_ev"]))
    xd0, xd1 = x0.copy(), x1.copy()
    xd0[off[0] + 9], xd1[off[0] + 9] = xd0[off[0] + 2], xd1[off[0] + 2]
    dup = _ev(ctx, capi, VC.ZERO_NOISE, (off, xd0, xd1, y))
    assert dup["status"][0] == capi.STATUS_NOT_SPD and np.all(dup["status"][1:] == 0)
    assert np.all(np.isnan(dup["log_ev"][0]))
    _same_run(dup["log_ev"][1:].copy(), zero["log_ev"][1:].copy(), big, "log_ev", 1.0 + np.abs(zero["log_ev"][1:]))


# ---------------------------------------------------------------------------------------------------------------- 6. bit contracts

def _dev_batch(batch, xs):
    import torch
    off, x0, x1, y = batch
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    return dict(off=t(off.astype(np.int32)), x0=t(x0), x1=t(x1), y=t(y), xs0=None if xs is None else t(xs[0]), xs1=None if xs is None else t(xs[1]),
                P=len(off) - 1, n_max=int(np.max(np.diff(off))), n_total=int(off[-1]), ny=y.shape[0])


def _ev_dev(ctx, capi, prm, d, m, res=0.0, sz=0, want=("f", "v", "alpha", "status", "log_ev")):
    """gpc_dense_fit_predict_ev_dev into fresh device buffers (NaN / -7); returns the host copies of the outputs in `want`."""
    import torch
    o = dict(f=torch.full((d["P"], d["ny"], m), np.nan, dtype=torch.float64, device="cuda"),
             v=torch.full((d["P"], m), np.nan, dtype=torch.float64, device="cuda"),
             alpha=torch.full((d["ny"], d["n_total"]), np.nan, dtype=torch.float64, device="cuda"),
             status=torch.full((d["P"],), -7, dtype=torch.int32, device="cuda"),
             log_ev=torch.full((d["P"], d["ny"]), np.nan, dtype=torch.float64, device="cuda"))
    torch.cuda.synchronize()
    ctx.dense_fit_predict_ev_dev(prm, d["P"], d["off"], d["n_max"], d["n_total"], d["x0"], d["x1"], d["y"], d["ny"], m, d["xs0"], d["xs1"], res, sz,
                                 o["f"], *(o[k] if k in want else None for k in ("v", "alpha", "status", "log_ev")))
    ctx.synchronize()
    return {k: o[k].cpu().numpy() for k in want}


@pytest.mark.parametrize("route,sizes", [("one-wave", (200, 0, 230, 64)), ("tiled", (300, 0, 270)), ("register", (100, 0, 180, 64))])
def test_ev_bit_contracts(gp, monkeypatch, route, sizes):
    """log_ev == NULL is gpc_dense_fit_predict[_dev]; with v_star the other outputs are the want_variance call's; two calls give one
    log_ev; host and _dev forms agree -- bit for bit on the one-wave and the tiled route; on the register route v* and the status bit for
    bit and the rest as far as two calls of that kernel agree (module docstring)."""
    import torch
    capi, ctx = gp
    exact = route != "register"
    if route == "one-wave":
        monkeypatch.setenv("GPC_W1_MIN_P", "1")
    batch = VC._mixed_batch(list(sizes), seed=78)
    G = DC.restate(VC.DEFAULT, batch)["G"]
    xs = VC.xstar(19, seed=98)
    d = _dev_batch(batch, xs)
    pv = _params(capi, VC.DEFAULT, want_variance=1)
    f0, v0, st0, al0 = ctx.dense_fit_predict(pv, *batch, *xs, want_alpha=True)
    # host form, log_ev == NULL
    fn, vn, aln, stn, evn = ctx.dense_fit_predict_ev(pv, *batch, xs0=xs[0], xs1=xs[1], want_ev=False)
    assert evn is None
    for k, a, b in (("f", fn, f0), ("v", vn, v0), ("alpha", aln, al0), ("status", stn, st0)):
        _same_run(a, b, exact, k)
    assert ctx.last_dense_kernel() == {"one-wave": W1, "tiled": BIG, "register": "dense_mfma_nt12 + dense_variance"}[route]
    # _dev form, log_ev == NULL, against gpc_dense_fit_predict_dev
    fd = torch.full((d["P"], 1, 19), np.nan, dtype=torch.float64, device="cuda")
    vd = torch.full((d["P"], 19), np.nan, dtype=torch.float64, device="cuda")
    ad = torch.full((1, d["n_total"]), np.nan, dtype=torch.float64, device="cuda")
    sd = torch.full((d["P"],), -7, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    ctx.dense_fit_predict_dev(pv, d["P"], d["off"], d["n_max"], d["n_total"], d["x0"], d["x1"], d["y"], 1, 19, d["xs0"], d["xs1"], fd, vd, ad, sd)
    ctx.synchronize()
    plain = dict(f=fd.cpu().numpy(), v=vd.cpu().numpy(), alpha=ad.cpu().numpy(), status=sd.cpu().numpy())
    nul = _ev_dev(ctx, capi, pv, d, 19, want=("f", "v", "alpha", "status"))
    for k in plain:
        _same_run(nul[k], plain[k], exact, k)
    # with log_ev and v_star (want_variance is ignored: 0 here)
    p0 = _params(capi, VC.DEFAULT, want_variance=0)
    a = _ev_dev(ctx, capi, p0, d, 19)
    b = _ev_dev(ctx, capi, p0, d, 19)
    for k in plain:
        _same_run(a[k], plain[k], exact, k)
    _same_run(a["log_ev"], b["log_ev"], exact, "log_ev", G)
    assert np.all(np.isfinite(a["log_ev"]))
    host = _ev(ctx, capi, VC.DEFAULT, batch, xs=xs)
    for k in KEYS:
        _same_run(host[k], a[k], exact, k, G)
    # evidence only: the same log_ev bits, no variance written
    e = _ev_dev(ctx, capi, p0, d, 19, want=("f", "alpha", "status", "log_ev"))
    _same_run(e["log_ev"], a["log_ev"], exact, "log_ev", G)
    # m == 0: the evidence alone
    z = _ev_dev(ctx, capi, p0, dict(d, xs0=None, xs1=None), 0, want=("status", "log_ev"))
    _same_run(z["log_ev"], a["log_ev"], exact, "log_ev", G)
    assert _same_bits(z["status"], a["status"])


def test_ev_grid_form_is_the_pointwise_form_on_the_grid(gp, monkeypatch):
    """xs0 == NULL: the sz x sz grid, materialised by the library, against the point-wise call on the same points, bit for bit (on the
    one-wave route, whose outputs repeat)."""
    capi, ctx = gp
    monkeypatch.setenv("GPC_W1_MIN_P", "1")
    batch = VC._mixed_batch([200, 0, 230], seed=79)
    res, sz = 0.15, 7
    prm = _params(capi, VC.DEFAULT)
    g = dict(zip(KEYS, ctx.dense_fit_predict_ev(prm, *batch, res=res, sz=sz)))
    xs = DC.grid_points(res, sz)
    p = _ev(ctx, capi, VC.DEFAULT, batch, xs=xs)
    assert g["f"].shape == (3, 1, sz * sz) and ctx.last_dense_kernel() == W1
    for k in KEYS:
        assert _same_bits(g[k], p[k]), k


# ---------------------------------------------------------------------------------------------------------------- 7. select

def _select(ctx, capi, batch, cands, xs=XS, want_v=True, skip=(), **kw):
    return ctx.dense_select(_params(capi, (9.0, 9.0, 9.0), **kw), cands, *batch, xs0=xs[0], xs1=xs[1], want_v=want_v, skip=skip)


SKEYS = ("f_star", "v_star", "alpha", "log_ev", "status")


def _winner_rows_are_the_ev_calls(ctx, capi, batch, cands, sel, want_v=True):
    off = batch[0]
    for h, th in enumerate(cands):
        one = _ev(ctx, capi, th, batch, want_v=want_v)
        pick = np.flatnonzero(sel["best"] == h)
        for i in pick:
            sl = slice(off[i], off[i + 1])
            assert _same_bits(sel["f_star"][i].copy(), one["f"][i].copy()) and _same_bits(sel["log_ev"][i].copy(), one["log_ev"][i].copy()), (h, i)
            assert _same_bits(sel["alpha"][:, sl].copy(), one["alpha"][:, sl].copy()) and sel["status"][i] == one["status"][i], (h, i)
            if want_v:
                assert _same_bits(sel["v_star"][i].copy(), one["v"][i].copy()), (h, i)
        assert _same_bits(sel["log_ev_all"][h], one["log_ev"]), h


def test_select_picks_the_generating_scale(gp, monkeypatch):
    """On the batch test_dense_ev_cpu.py decides on the CPU: best is the restatement's on every patch, the duplicate candidate never wins
    over the lower index, every candidate's log_ev is within the gate, and every winner's rows are a separate _ev call's bits (one-wave
    route: the batch's largest patch has 200 points)."""
    capi, ctx = gp
    monkeypatch.setenv("GPC_W1_MIN_P", "1")
    batch = DC.select_batch()
    ref = DC.select_ref()
    sel = _select(ctx, capi, batch, DC.CANDIDATES, want_v=False)
    assert sel["v_star"] is None and ctx.last_dense_kernel() == W1_EV
    assert np.array_equal(sel["best"], ref["best"]) and not np.any(sel["best"] == 3)
    assert np.all(np.abs(sel["log_ev_all"] - ref["log_ev_all"]) <= DC.gate(ref["G"]))
    assert _same_bits(sel["log_ev_all"][3], sel["log_ev_all"][1])
    _winner_rows_are_the_ev_calls(ctx, capi, batch, DC.CANDIDATES, sel, want_v=False)


def test_select_planes_empty_patch_h1_and_null_outputs(gp):
    """Three planes decide by their sum; an empty patch has best 0 with the prior of candidate 0; H = 1 is the _ev call; and with any one
    output pointer NULL the others keep their bits (tiled route: its outputs repeat)."""
    capi, ctx = gp
    batch = DC.plane_batch(True)
    off = batch[0]
    cands = [(0.4, 0.3 ** 2, 2e-3), VC.MEDIUM, (0.6, 0.8 ** 2, 1e-3)]
    sel = _select(ctx, capi, batch, cands)
    s = sel["log_ev_all"][:, :, 0] + sel["log_ev_all"][:, :, 1] + sel["log_ev_all"][:, :, 2]
    want, _ = DC.best_of(sel["log_ev_all"], np.zeros(s.shape, dtype=np.int32))
    assert np.array_equal(sel["best"], want) and np.all(sel["status"] == 0)
    empty = int(np.flatnonzero(np.diff(off) == 0)[0])
    assert sel["best"][empty] == 0 and np.all(sel["f_star"][empty] == 0.0) and np.all(sel["v_star"][empty] == cands[0][0])
    assert np.all(sel["log_ev"][empty] == 0.0)
    _winner_rows_are_the_ev_calls(ctx, capi, batch, cands, sel)
    one = _select(ctx, capi, batch, cands[1:2])
    ev = _ev(ctx, capi, cands[1], batch)
    assert np.all(one["best"] == 0) and _same_bits(one["log_ev_all"][0], ev["log_ev"])
    for a, b in (("f_star", "f"), ("v_star", "v"), ("alpha", "alpha"), ("log_ev", "log_ev"), ("status", "status")):
        assert _same_bits(one[a], ev[b]), a
    # (without v_star no variance kernel runs and f* is the fit's own prediction: that call's bits are the select's without v_star)
    nov = _select(ctx, capi, batch, cands, want_v=False)
    assert np.array_equal(nov["best"], sel["best"]) and _same_bits(nov["log_ev_all"], sel["log_ev_all"])
    for name in ("f_star", "v_star", "alpha", "log_ev", "best", "log_ev_all", "status"):
        part = _select(ctx, capi, batch, cands, skip=(name,))
        assert part[name] is None
        base = nov if name == "v_star" else sel
        for k in sel:
            if k != name and base[k] is not None:
                assert _same_bits(part[k], base[k]), (name, k)


def test_select_without_an_eligible_candidate(gp):
    """A repeated point under candidates without a noise term: no candidate is eligible on that patch -- best = -1, NaN rows, candidate
    0's status -- and a candidate that is eligible elsewhere still wins there."""
    capi, ctx = gp
    off, x0, x1, y = VC._mixed_batch([100, 64], seed=80)
    x0[9], x1[9] = x0[2], x1[2]
    cands = [VC.ZERO_NOISE, (0.5, 0.004 ** 2, 0.0)]
    sel = _select(ctx, capi, (off, x0, x1, y), cands)
    assert sel["best"][0] == -1 and sel["status"][0] == capi.STATUS_NOT_SPD and sel["best"][1] in (0, 1) and sel["status"][1] == 0
    assert np.all(np.isnan(sel["f_star"][0])) and np.all(np.isnan(sel["v_star"][0])) and np.all(np.isnan(sel["log_ev"][0]))
    assert np.all(np.isnan(sel["alpha"][:, :100])) and np.all(np.isnan(sel["log_ev_all"][:, 0]))
    assert np.all(np.isfinite(sel["f_star"][1])) and np.all(np.isfinite(sel["log_ev"][1]))


def test_select_dev_is_the_host_form(gp, monkeypatch):
    """gpc_dense_select_dev on device buffers against the host form, bit for bit, in the grid form (one-wave route)."""
    import torch
    capi, ctx = gp
    monkeypatch.setenv("GPC_W1_MIN_P", "1")
    batch = VC._mixed_batch([200, 0, 230, 64], seed=81)
    res, sz = 0.15, 5
    cands = [VC.MEDIUM, VC.DEFAULT]
    prm = _params(capi, VC.MEDIUM)
    host = ctx.dense_select(prm, cands, *batch, res=res, sz=sz)
    d = _dev_batch(batch, None)
    P, m, H = d["P"], sz * sz, len(cands)
    nan = lambda *s: torch.full(s, np.nan, dtype=torch.float64, device="cuda")
    o = dict(f_star=nan(P, 1, m), v_star=nan(P, m), alpha=nan(1, d["n_total"]), log_ev=nan(P, 1),
             best=torch.full((P,), -7, dtype=torch.int32, device="cuda"), log_ev_all=nan(H, P, 1),
             status=torch.full((P,), -7, dtype=torch.int32, device="cuda"))
    torch.cuda.synchronize()
    ctx.dense_select_dev(prm, cands, P, d["off"], d["n_max"], d["n_total"], d["x0"], d["x1"], d["y"], 1, 0, None, None, res, sz,
                         f_star=o["f_star"], v_star=o["v_star"], alpha_out=o["alpha"], log_ev=o["log_ev"], best=o["best"],
                         log_ev_all=o["log_ev_all"], status=o["status"])
    ctx.synchronize()
    for k in o:
        assert _same_bits(o[k].cpu().numpy(), host[k]), k


# ---------------------------------------------------------------------------------------------------------------- 8. entry rules

def _raw_ev(ctx, capi, prm, off, x0, x1, y, ny, m, xs0, xs1, res, sz, outs, ctx_h=True, P=None):
    """gpc_dense_fit_predict_ev on host arrays, every argument as given (None: NULL); returns the code."""
    p = capi._ptr
    return ctx.lib.gpc_dense_fit_predict_ev(ctx.h if ctx_h else None, C.byref(prm) if prm is not None else None,
                                            (len(off) - 1 if off is not None else 0) if P is None else P, p(off), p(x0), p(x1), p(y), ny, m,
                                            p(xs0), p(xs1), float(res), int(sz), *map(p, outs))


def _fresh_outs(P, ny, m, N):
    return [np.full((P, ny, m), 7.5), np.full((P, m), 7.5), np.full((ny, N), 7.5), np.full(P, -7, dtype=np.int32), np.full((P, ny), 7.5)]


def _untouched(outs):
    return all(np.all(o == (7.5 if o.dtype == np.float64 else -7)) for o in outs if o is not None)


def test_entry_rules_in_order(gp):
    """Every argument rule of include/gpc.h returns its code and writes no output, and where two are broken the earlier one decides (seen
    in the error text)."""
    capi, ctx = gp
    off, x0, x1, y = VC._mixed_batch([20, 30], seed=82)
    xs0, xs1 = XS
    prm = _params(capi, VC.DEFAULT)
    E, R = capi.GPC_EINVAL, capi.GPC_ERANGE
    bad_l = _params(capi, (0.5, 0.0, 1e-3))
    dec = np.array([0, 30, 20], dtype=np.int32)
    off1 = np.array([1, 20, 50], dtype=np.int32)
    big_off = np.array([0, 1025], dtype=np.int32)
    z = np.zeros(1025)
    cases = [
        ("ctx NULL", dict(ctx_h=False), E, None),
        ("params NULL", dict(prm=None), E, "params is NULL"),
        ("sz < 0", dict(xs0=None, xs1=None, sz=-1), E, "sz out of range"),
        ("sz > 1024", dict(xs0=None, xs1=None, sz=1025), E, "sz out of range"),
        ("P < 0", dict(P=-1), E, "negative size"),
        ("off NULL", dict(off=None, P=2), E, "off is NULL"),
        ("off[0] != 0", dict(off=off1), E, "off[0] must be 0"),
        ("off decreasing", dict(off=dec), E, "non-decreasing"),
        ("ny = 2", dict(ny=2), E, "ny must be"),
        ("x0 NULL", dict(x0=None), E, "x0/x1/y is NULL"),
        ("f_star NULL", dict(no_f=True), E, "f_star is NULL"),
        ("n_max > 1024", dict(off=big_off, x0=z, x1=z, y=z[None, :].copy()), R, "GPC_MAX_POINTS"),
        ("l_sq = 0", dict(prm=bad_l), E, "out of range"),
        ("xs1 NULL", dict(xs1=None), E, "xs1 is NULL"),
        # two broken: the earlier rule decides
        ("params NULL + sz", dict(prm=None, xs0=None, xs1=None, sz=-1), E, "params is NULL"),
        ("sz + off[0]", dict(xs0=None, xs1=None, sz=2000, off=off1), E, "sz out of range"),
        ("off decreasing + ny", dict(off=dec, ny=2), E, "non-decreasing"),
        ("l_sq + xs1", dict(prm=bad_l, xs1=None), E, "out of range"),
    ]
    for label, ch, code, text in cases:
        a = dict(prm=prm, off=off, x0=x0, x1=x1, y=y, ny=1, m=len(xs0), xs0=xs0, xs1=xs1, res=0.15, sz=0, ctx_h=True, P=None)
        no_f = ch.pop("no_f", False)
        a.update(ch)
        outs = _fresh_outs(2, 1, len(xs0), 50)
        sent = [None if no_f else outs[0]] + outs[1:]
        rc = _raw_ev(ctx, capi, a["prm"], a["off"], a["x0"], a["x1"], a["y"], a["ny"], a["m"], a["xs0"], a["xs1"], a["res"], a["sz"], sent,
                     ctx_h=a["ctx_h"], P=a["P"])
        assert rc == code, (label, rc)
        assert _untouched(outs), label
        if text is not None:
            assert text in ctx.lib.gpc_last_error(ctx.h).decode(), (label, ctx.lib.gpc_last_error(ctx.h).decode())
    # P == 0 after all the checks: GPC_OK and nothing written; with a broken rule still the rule's code
    outs = _fresh_outs(2, 1, len(xs0), 50)
    e0 = np.zeros(1, dtype=np.int32)
    assert _raw_ev(ctx, capi, prm, e0, x0, x1, y, 1, len(xs0), xs0, xs1, 0.15, 0, outs) == capi.GPC_OK and _untouched(outs)
    assert _raw_ev(ctx, capi, bad_l, e0, x0, x1, y, 1, len(xs0), xs0, xs1, 0.15, 0, outs) == E and _untouched(outs)


def test_select_entry_rules(gp):
    """The select's own rule comes third: H < 1, cand NULL, a candidate with a non-finite or non-positive field (noise may be 0) -- ahead
    of sz, and behind params."""
    capi, ctx = gp
    off, x0, x1, y = VC._mixed_batch([20, 30], seed=82)
    prm = _params(capi, VC.DEFAULT)
    p = capi._ptr

    def call(prm_, H, arr, sz=3, outs=None):
        outs = outs if outs is not None else [None] * 7
        return ctx.lib.gpc_dense_select(ctx.h, C.byref(prm_) if prm_ is not None else None, H, C.addressof(arr) if arr is not None else None,
                                        2, p(off), p(x0), p(x1), p(y), 1, 0, None, None, 0.15, sz, *map(p, outs))

    good = ctx.hyper_array([VC.DEFAULT, (0.5, 0.25, 0.0)])
    f = np.full((2, 1, 9), 7.5)
    best = np.full(2, -7, dtype=np.int32)
    E = capi.GPC_EINVAL
    assert call(prm, 0, good) == E and "H >= 1" in ctx.lib.gpc_last_error(ctx.h).decode()
    assert call(prm, 2, None) == E
    for bad in ((np.nan, 1.0, 1e-3), (1.0, np.inf, 1e-3), (0.0, 1.0, 1e-3), (1.0, -1.0, 1e-3), (1.0, 1.0, -1e-3), (1.0, 1.0, np.nan)):
        outs = [f, None, None, None, best, None, None]
        assert call(prm, 2, ctx.hyper_array([VC.DEFAULT, bad]), outs=outs) == E, bad
        assert "candidate 1" in ctx.lib.gpc_last_error(ctx.h).decode() and np.all(f == 7.5) and np.all(best == -7)
    assert call(None, 0, good) == E and "params is NULL" in ctx.lib.gpc_last_error(ctx.h).decode()
    assert call(prm, 0, good, sz=-1) == E and "H >= 1" in ctx.lib.gpc_last_error(ctx.h).decode()
    assert call(prm, 2, good, sz=-1) == E and "sz out of range" in ctx.lib.gpc_last_error(ctx.h).decode()
    # noise = 0 is a valid candidate, and every output may be NULL
    assert call(prm, 2, good) == capi.GPC_OK
    assert call(prm, 2, good, outs=[f, None, None, None, best, None, None]) == capi.GPC_OK
    assert np.all(np.isfinite(f)) and np.all(best >= 0)


# ---------------------------------------------------------------------------------------------------------------- 9. the probit select

def test_probit_select_is_the_unchanged_path(gp):
    """The probit selection keeps its own keep-best kernel (the Gaussian one is a sibling): on a small batch gpc_dense_irls_select still
    gives, per patch, the bits of gpc_dense_irls_fit_predict_ev under the winning candidate, and the winner its own log_q_all decides."""
    import irls_cases as IC
    import irls_ev_cases as EV
    capi, ctx = gp
    off, x0, x1, lab = EV.select_batch(P=3, n=96)
    prm = capi.default_params_dense(sigmaf_sq=IC.REGIME[0], l_sq=IC.REGIME[1], noise=IC.REGIME[2], noise_model=2)
    irls = capi.default_params_irls(max_iter=IC.MAX_ITER, **IC.MODELS[2])
    sel = ctx.dense_irls_select(prm, irls, EV.CANDIDATES, off, x0, x1, lab, xs0=XS[0], xs1=XS[1])
    f, v, p, al, fh, it, st, lq, best, lq_all = sel
    ones = []
    for th in EV.CANDIDATES:
        ph = capi.default_params_dense(sigmaf_sq=th[0], l_sq=th[1], noise=th[2], noise_model=2)
        ones.append(ctx.dense_irls_fit_predict_ev(ph, irls, off, x0, x1, lab, xs0=XS[0], xs1=XS[1]))
    assert np.array_equal(best, EV.best_of(lq_all, np.stack([o[6] for o in ones]))) and np.all(best >= 0)
    for h, one in enumerate(ones):
        assert _same_bits(lq_all[h], one[7])
        for i in np.flatnonzero(best == h):
            sl = slice(off[i], off[i + 1])
            for a, b in ((f, one[0]), (v, one[1]), (p, one[2])):
                assert _same_bits(a[i].copy(), b[i].copy())
            assert _same_bits(al[sl].copy(), one[3][sl].copy()) and _same_bits(fh[sl].copy(), one[4][sl].copy())
            assert it[i] == one[5][i] and lq[i].tobytes() == one[7][i].tobytes()
