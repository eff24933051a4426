"""GPU tests of the probit GP's Laplace evidence (gpc_dense_irls_fit_predict_ev[_dev]) and of the selection among candidate
hyper-parameters (gpc_dense_irls_select[_dev], capi.Mapping.occupancy_select), include/gpc.h: the read-out and keep-best kernels of
csrc/dense_evidence.hip behind the IRLS instances of the tiled kernel with the factor export on, against the NumPy restatement of the
definition (irls_ev_cases.py, checked on its own by test_irls_ev_cpu.py).

Gate (irls_ev_cases.py): log q within EV_GATE = 1e-11 (1 + |log q|) of the restatement (E64 = 1.7e-16, so the rule's 16 E64 branch is not
in force); iters may differ from the restatement's by at most 1, as in test_irls_var_gpu.py.  Everything else is compared bit for bit."""
import ctypes as C

import numpy as np
import pytest

import irls_cases as IC
import irls_ev_cases as EV
import irls_var_cases as IV
import variance_cases as VC

pytestmark = pytest.mark.gpu

KEYS = ("f", "v", "p", "alpha", "fhat", "iters", "status")
EKEYS = KEYS + ("log_q",)
SKEYS = EKEYS + ("best", "log_q_all")
XS = VC.xstar(37, seed=95)


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


def _params(capi, model=2, theta=IC.REGIME):
    return capi.default_params_dense(sigmaf_sq=theta[0], l_sq=theta[1], noise=theta[2], noise_model=model)


def _irls(capi, max_iter=IC.MAX_ITER, **kw):
    arg = dict(IC.MODELS[2])
    arg.update(kw)
    return capi.default_params_irls(max_iter=max_iter, **arg)


def _ev(ctx, capi, batch, xs=XS, theta=IC.REGIME, want_v=True, want_p=True, **kw):
    out = ctx.dense_irls_fit_predict_ev(_params(capi, 2, theta), _irls(capi, **kw), *batch, xs0=xs[0], xs1=xs[1], want_v=want_v, want_p=want_p)
    return dict(zip(EKEYS, out))


def _var(ctx, capi, batch, xs=XS, theta=IC.REGIME, **kw):
    out = ctx.dense_irls_fit_predict_var(_params(capi, 2, theta), _irls(capi, **kw), *batch, xs0=xs[0], xs1=xs[1])
    return dict(zip(KEYS, out))


def _select(ctx, capi, batch, cands, xs=XS, **kw):
    out = ctx.dense_irls_select(_params(capi, 2), _irls(capi, **kw), cands, *batch, xs0=xs[0], xs1=xs[1])
    return dict(zip(SKEYS, out))


def _same_bits(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(a.view(np.uint8), b.view(np.uint8))


def _check_log_q(got, ref, off, label, pick=None, want_status=0):
    """log q of the GPU against the restatement's, patch by patch (pick: these patches only); returns the worst gap of 1 + |log q|."""
    n = np.diff(off)
    worst = 0.0
    for i in (range(len(n)) if pick is None else pick):
        assert got["status"][i] == ref["status"][i], (label, i, got["status"][i], ref["status"][i])
        if n[i] == 0:
            assert got["log_q"][i] == 0.0 and got["status"][i] == 0 and got["iters"][i] == 0, (label, i, got["log_q"][i])
            continue
        if ref["status"][i] == 2:
            assert np.isnan(got["log_q"][i]), (label, i, got["log_q"][i])
            continue
        assert got["status"][i] == want_status, (label, i, got["status"][i])
        assert abs(int(got["iters"][i]) - int(ref["iters"][i])) <= 1, (label, i, got["iters"][i], ref["iters"][i])
        assert np.isfinite(got["log_q"][i]), (label, i)
        e = abs(float(got["log_q"][i]) - float(ref["log_q"][i]))
        rel = e / (1.0 + abs(float(ref["log_q"][i])))
        worst = max(worst, rel)
        print("%s patch %d n=%d: log q %.6f against %.6f, gap %.2e of 1 + |log q|" % (label, i, n[i], got["log_q"][i], ref["log_q"][i], rel))
        assert e <= EV.ev_gate(ref["log_q"][i]), (label, i, int(n[i]), e, float(ref["log_q"][i]))
    print("%s: worst log q gap %.2e of 1 + |log q| (gate %.0e)" % (label, worst, EV.EV_RTOL))
    return worst


# ---------------------------------------------------------------------------------------------------------------- 1. against the restatement

@pytest.mark.parametrize("cap", IC.CAPS)
def test_ev_big_tile_counts(gp, oracle, cap):
    """The eight-wave instance in slots of 64, 33 and 17 tile columns: every tile count of tile_batch (n = 0, 1, 15, 16, 17 ... 1024), and
    patches smaller than the largest (ntw > nt: the L_kk^-1 images sit behind ntw, not nt, tile columns).
    Measured on MI355X, worst log q gap of 1 + |log q|: 2.2e-15 (cap 1024), 6.9e-16 (513), 6.9e-16 (272); gate 1e-11."""
    capi, ctx = gp
    idx = IC.cap_index(cap)
    batch, pts = IC.take(IC.tile_batch(), idx)
    assert int(np.max(np.diff(batch[0]))) == cap
    got = _ev(ctx, capi, batch)
    full = EV.tile_ref(oracle)
    ref = dict(log_q=full["log_q"][idx], iters=full["iters"][idx], status=full["status"][idx])
    _check_log_q(got, ref, batch[0], "tiles cap=%d" % cap)


def test_ev_w4_tile_edges(gp, oracle):
    """The four-wave instance: 0, 1 and every tile edge +- 1 up to 256 points.
    Measured on MI355X: worst log q gap 8.8e-16 of 1 + |log q|."""
    capi, ctx = gp
    batch = IC.w4_batch()
    got = _ev(ctx, capi, batch)
    _check_log_q(got, EV.w4_ref(oracle), batch[0], "w4 edges")


@pytest.mark.parametrize("max_iter", [1, 2, 6])
@pytest.mark.parametrize("shape", ["big", "w4"])
def test_ev_pinned_step_count(gp, oracle, shape, max_iter):
    """tol = 0 and a step cap: every non-empty patch is GPC_STATUS_NOT_CONVERGED and log q is that of the last iterate, with the L of the
    last solve performed.
    Measured on MI355X, worst over the counts: 1.5e-15 of 1 + |log q| (eight waves), 6.0e-16 (four waves)."""
    capi, ctx = gp
    batch = IV.pinned_batch(shape)
    n = np.diff(batch[0])
    got = _ev(ctx, capi, batch, max_iter=max_iter, tol=0.0)
    assert np.all(got["status"][n > 0] == capi.STATUS_NOT_CONVERGED) and np.all(got["iters"][n > 0] == max_iter)
    assert np.all(np.isfinite(got["log_q"]))
    _check_log_q(got, EV.pinned_ref(oracle, shape, max_iter), batch[0], "max_iter=%d tol=0, %s" % (max_iter, shape),
                 want_status=capi.STATUS_NOT_CONVERGED)


# ---------------------------------------------------------------------------------------------------------------- 2. same bits as _var

@pytest.mark.parametrize("shape", ["big", "w4"])
def test_ev_other_outputs_are_the_var_entry(gp, shape):
    """With log_q requested every other output is bit for bit the _var entry's; log_q == NULL is the _var entry; two _ev calls give one
    log_q bit pattern."""
    capi, ctx = gp
    batch = IC.grid_batch(shape)
    var = _var(ctx, capi, batch)
    got = _ev(ctx, capi, batch)
    for k in KEYS:
        assert _same_bits(got[k], var[k]), k
    again = _ev(ctx, capi, batch)
    for k in EKEYS:
        assert _same_bits(got[k], again[k]), k
    # log_q == NULL through the C-ABI
    off, x0, x1, lab = batch
    P, m = len(off) - 1, len(XS[0])
    f, v, p = (np.full((P, m), np.nan) for _ in range(3))
    al, fh = np.full_like(lab, np.nan), np.full_like(lab, np.nan)
    it, st = np.full(P, -1, dtype=np.int32), np.full(P, -1, dtype=np.int32)
    ptr = capi._ptr
    rc = ctx.lib.gpc_dense_irls_fit_predict_ev(ctx.h, C.byref(_params(capi)), C.byref(_irls(capi)), P, ptr(off), ptr(x0), ptr(x1), ptr(lab), m,
                                               ptr(XS[0]), ptr(XS[1]), 0.0, 0, ptr(f), ptr(v), ptr(p), ptr(al), ptr(fh), ptr(it), ptr(st), None)
    assert rc == capi.GPC_OK
    for k, a in zip(KEYS, (f, v, p, al, fh, it, st)):
        assert _same_bits(a, var[k]), k


# ---------------------------------------------------------------------------------------------------------------- 3. more patches than waves

def test_ev_many_patches(gp, oracle, monkeypatch):
    """The 600-patch many_batch: empty patches give exactly 0, the three NaN-label patches NaN, their neighbours (and 64 patches in all,
    many_pick) stay within the gate; every other patch is finite; the run repeated under GPC_POISON_LDS=1 (LDS and workspace filled with
    NaN before the kernels) gives the same bits.
    Measured on MI355X: worst log q gap 9.5e-16 of 1 + |log q| over the 64 picked patches."""
    capi, ctx = gp
    c = IC.MANY["big"]
    batch = IC.many_batch("big")
    got = _ev(ctx, capi, batch)
    for i in c["empty"]:
        assert got["log_q"][i] == 0.0 and got["status"][i] == 0
    for i in c["nan"]:
        assert got["status"][i] == capi.STATUS_NAN and np.isnan(got["log_q"][i])
    live = np.setdiff1d(np.arange(c["P"]), list(c["nan"]))
    assert np.all(got["status"][live] == 0) and np.all(np.isfinite(got["log_q"][live]))
    assert np.all(got["log_q"][np.setdiff1d(live, list(c["empty"]))] < 0.0)
    _check_log_q(got, EV.many_ref(oracle, "big"), batch[0], "many_big", pick=IV.many_pick("big"))
    monkeypatch.setenv("GPC_POISON_LDS", "1")
    poisoned = _ev(ctx, capi, batch)
    monkeypatch.delenv("GPC_POISON_LDS")
    for k in EKEYS:
        assert _same_bits(got[k], poisoned[k]), k


# ---------------------------------------------------------------------------------------------------------------- 4. entry rules

def test_ev_entry_rules(gp, oracle):
    """noise_model 1 with log_q: GPC_EINVAL.  Only log_q requested (m = 0, no v or p): works, and gives the bits of the full call.  log_q
    with f* but neither v* nor p*: f* is the plain entry's.  Host and _dev entries give the same bits."""
    import torch
    capi, ctx = gp
    lib, ptr = ctx.lib, capi._ptr
    batch = IC.grid_batch("big")
    off, x0, x1, lab = batch
    P, N, m = len(off) - 1, len(lab), len(XS[0])
    full = _ev(ctx, capi, batch)
    lq = np.full(P, np.nan)
    f = np.full((P, m), np.nan)

    def call(prm, m_=0, f_=None):
        return lib.gpc_dense_irls_fit_predict_ev(ctx.h, C.byref(prm), C.byref(_irls(capi)), P, ptr(off), ptr(x0), ptr(x1), ptr(lab), m_,
                                                 ptr(XS[0]), ptr(XS[1]), 0.0, 0, ptr(f_), None, None, None, None, None, None, ptr(lq))
    assert call(_params(capi, 1)) == capi.GPC_EINVAL
    assert call(_params(capi, 0)) == capi.GPC_EINVAL
    assert np.all(np.isnan(lq))
    assert call(_params(capi, 2)) == capi.GPC_OK
    assert _same_bits(lq, full["log_q"])
    lq[:] = np.nan
    assert call(_params(capi, 2), m_=m, f_=f) == capi.GPC_OK
    assert _same_bits(lq, full["log_q"])
    plain = ctx.dense_irls_fit_predict(_params(capi), _irls(capi), *batch, xs0=XS[0], xs1=XS[1])
    assert _same_bits(f, plain[0])
    # the _dev entry on device tensors
    dev = torch.device("cuda", 0)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    d_off, d_x0, d_x1, d_y, d_xs0, d_xs1 = (t(a) for a in (off, x0, x1, lab, XS[0], XS[1]))
    d_f, d_v, d_p = (torch.zeros((P, m), dtype=torch.float64, device=dev) for _ in range(3))
    d_al, d_fh = (torch.zeros(N, dtype=torch.float64, device=dev) for _ in range(2))
    d_lq = torch.zeros(P, dtype=torch.float64, device=dev)
    d_it, d_st = (torch.full((P,), -1, dtype=torch.int32, device=dev) for _ in range(2))
    torch.cuda.synchronize()
    ctx.dense_irls_fit_predict_ev_dev(_params(capi), _irls(capi), P, d_off, int(np.max(np.diff(off))), N, d_x0, d_x1, d_y, m, d_xs0, d_xs1,
                                      0.0, 0, d_f, v_star=d_v, p_star=d_p, alpha_out=d_al, fhat_out=d_fh, iters=d_it, status=d_st, log_q=d_lq)
    ctx.synchronize()
    for k, a in zip(EKEYS, (d_f, d_v, d_p, d_al, d_fh, d_it, d_st, d_lq)):
        assert _same_bits(a.cpu().numpy(), full[k]), k
    # fhat from the workspace (fhat_out == NULL) gives the same log q
    d_lq2 = torch.zeros(P, dtype=torch.float64, device=dev)
    ctx.dense_irls_fit_predict_ev_dev(_params(capi), _irls(capi), P, d_off, int(np.max(np.diff(off))), N, d_x0, d_x1, d_y, m, d_xs0, d_xs1,
                                      0.0, 0, d_f, v_star=d_v, p_star=d_p, log_q=d_lq2)
    ctx.synchronize()
    assert _same_bits(d_lq2.cpu().numpy(), full["log_q"])


# ---------------------------------------------------------------------------------------------------------------- 5. select

@pytest.fixture(scope="module")
def sel(gp):
    """The selection batch: select with the three candidates, and the _ev call per candidate."""
    capi, ctx = gp
    batch = EV.select_batch()
    per = [_ev(ctx, capi, batch, theta=th) for th in EV.CANDIDATES]
    got = _select(ctx, capi, batch, EV.CANDIDATES)
    return batch, per, got


def _rows_equal(got, src, off, i, label):
    """Every output row of patch i of a select call equals that of an _ev call."""
    sl = slice(off[i], off[i + 1])
    for k in ("f", "v", "p"):
        assert _same_bits(got[k][i], src[k][i]), (label, i, k)
    for k in ("alpha", "fhat"):
        assert _same_bits(got[k][sl], src[k][sl]), (label, i, k)
    for k in ("iters", "status", "log_q"):
        assert _same_bits(got[k][i:i + 1], src[k][i:i + 1]), (label, i, k)


def test_select_picks_the_true_scale(gp, oracle, sel):
    """best == 1 everywhere (the restatement's choice, with a top-two gap of at least 1); log_q_all[h] is the _ev call with candidate h bit
    for bit and within the gate of the restatement; every output row of a patch is the winner's _ev call, bit for bit.
    Measured on MI355X: worst log q gap 1.4e-15 of 1 + |log q| over the three candidates."""
    capi, ctx = gp
    batch, per, got = sel
    ref = EV.select_ref(oracle)
    P = len(batch[0]) - 1
    assert np.array_equal(ref["best"], np.ones(P, dtype=np.int32))
    assert got["best"].dtype == np.int32 and np.array_equal(got["best"], ref["best"]), got["best"]
    worst = 0.0
    for h in range(len(EV.CANDIDATES)):
        assert _same_bits(got["log_q_all"][h], per[h]["log_q"]), h
        assert np.all(per[h]["status"] == 0)
        e = np.abs(per[h]["log_q"] - ref["log_q_all"][h])
        worst = max(worst, float(np.max(e / (1 + np.abs(ref["log_q_all"][h])))))
        assert np.all(e <= EV.ev_gate(ref["log_q_all"][h])), (h, float(np.max(e)))
    print("select batch: worst log q gap %.2e of 1 + |log q| over the three candidates" % worst)
    for i in range(P):
        _rows_equal(got, per[int(got["best"][i])], batch[0], i, "select")


def test_select_duplicate_goes_to_the_lower_index(gp, sel):
    """Candidates {c0, c0, c1}: candidate 1 ties with candidate 0 and never wins; the winners are those of {c0, c1}."""
    capi, ctx = gp
    batch, per, _ = sel
    c0, c1 = EV.CANDIDATES[0], EV.CANDIDATES[1]
    got = _select(ctx, capi, batch, (c0, c0, c1))
    assert not np.any(got["best"] == 1) and np.all(got["best"] == 2), got["best"]
    assert _same_bits(got["log_q_all"][0], got["log_q_all"][1]) and _same_bits(got["log_q_all"][0], per[0]["log_q"])
    for i in range(len(batch[0]) - 1):
        _rows_equal(got, per[1], batch[0], i, "duplicate")


def test_select_nothing_eligible(gp, sel):
    """max_iter = 1, tol = 0: every fit ends NOT_CONVERGED, so best is -1 everywhere, the outputs are NaN, and status and iters are those of
    candidate 0; log_q_all still holds every candidate's value at its last iterate."""
    capi, ctx = gp
    batch, _, _ = sel
    got = _select(ctx, capi, batch, EV.CANDIDATES, max_iter=1, tol=0.0)
    c0 = _ev(ctx, capi, batch, theta=EV.CANDIDATES[0], max_iter=1, tol=0.0)
    assert np.all(got["best"] == -1)
    for k in ("f", "v", "p", "alpha", "fhat", "log_q"):
        assert np.all(np.isnan(got[k])), k
    assert np.all(got["status"] == capi.STATUS_NOT_CONVERGED) and np.all(got["iters"] == 1)
    assert _same_bits(got["status"], c0["status"]) and _same_bits(got["iters"], c0["iters"])
    assert _same_bits(got["log_q_all"][0], c0["log_q"]) and np.all(np.isfinite(got["log_q_all"]))


def test_select_empty_patch_and_single_candidate(gp, oracle, sel):
    """A batch with an empty patch: best is 0 there with candidate 0's outputs (f* = 0, v* = cand[0].sigmaf_sq, p* = 0.5, log q = 0), and
    the other patches choose as the restatement does.  H = 1: select gives the _ev bits."""
    capi, ctx = gp
    full, per, _ = sel
    batch, pts = IC.take(full, [0, 1, 2])
    off, x0, x1, lab = batch
    c0 = (2.0, EV.L_SQ / 16, EV.S20)                  # candidate 0 with a sigmaf_sq of its own: what an empty patch reports as v*
    ref = EV.select_ref(oracle)
    for i in range(3):                                # the restatement still prefers candidate 1 on these patches, by a gap of at least 1
        sl = slice(off[i], off[i + 1])
        st0, _, a, fh, last = EV.fit_patch_theta(oracle, x0[sl], x1[sl], lab[sl], c0)
        assert st0 == 0 and EV.log_q_of(a, fh, lab[sl], last[0], c0[2]) + EV.SELECT_GAP <= ref["log_q_all"][1, i]
    batch = EV.with_empty(batch, 1)
    cands = (c0,) + EV.CANDIDATES[1:]
    got = _select(ctx, capi, batch, cands)
    assert got["best"].tolist() == [1, 0, 1, 1], got["best"]
    assert np.all(got["f"][1] == 0.0) and np.all(got["v"][1] == 2.0) and np.all(got["p"][1] == 0.5) and got["log_q"][1] == 0.0
    assert got["status"][1] == 0 and got["iters"][1] == 0 and np.all(got["log_q_all"][:, 1] == 0.0)
    win = _ev(ctx, capi, batch, theta=EV.CANDIDATES[1])
    for i in (0, 2, 3):
        _rows_equal(got, win, batch[0], i, "with an empty patch")
    one = _select(ctx, capi, full, EV.CANDIDATES[1:2])
    assert np.all(one["best"] == 0) and one["log_q_all"].shape == (1, len(full[0]) - 1)
    for k in EKEYS:
        assert _same_bits(one[k], per[1][k]), k
    assert _same_bits(one["log_q_all"][0], per[1]["log_q"])


def test_select_errors(gp, sel):
    """H < 1, NULL cand, a candidate with a non-positive or non-finite field, noise_model != 2: GPC_EINVAL."""
    capi, ctx = gp
    batch, _, _ = sel
    off, x0, x1, lab = IC.take(batch, [0])[0]
    ptr = capi._ptr
    lq = np.zeros(1)

    def call(cands, H=None, model=2, null=False):
        arr = ctx.hyper_array(cands)
        return ctx.lib.gpc_dense_irls_select(ctx.h, C.byref(_params(capi, model)), C.byref(_irls(capi)), len(cands) if H is None else H,
                                             None if null else C.addressof(arr), 1, ptr(off), ptr(x0), ptr(x1), ptr(lab), 0, None, None,
                                             0.0, 0, None, None, None, None, None, ptr(lq), None, None, None, None)
    ok = EV.CANDIDATES
    assert call(ok, H=0) == capi.GPC_EINVAL and call(ok, H=-1) == capi.GPC_EINVAL
    assert call(ok, null=True) == capi.GPC_EINVAL
    assert call(ok, model=1) == capi.GPC_EINVAL and call(ok, model=0) == capi.GPC_EINVAL
    for bad in ((0.0, EV.L_SQ, EV.S20), (1.0, -EV.L_SQ, EV.S20), (1.0, EV.L_SQ, np.nan), (np.inf, EV.L_SQ, EV.S20)):
        assert call(ok[:1] + (bad,)) == capi.GPC_EINVAL, bad
    assert call(ok) == capi.GPC_OK and np.isfinite(lq[0])


# ---------------------------------------------------------------------------------------------------------------- 6. the map

def test_mapping_occupancy_select(gp):
    """Mapping.occupancy_select on the plane-cloud model of test_mapping_gpu.py with two scans added: p, f, v, best, log_q and status
    equal a direct dense_irls_select_dev call on occupancy_batch(cells), bit for bit; a leaf without observed cells has best 0."""
    import torch
    from gp_compressor_amd import synth
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
        assert mp.add_cloud(ctx.make_cloud(S, cs))[1]
        assert mp.add_cloud(ctx.make_cloud(S + np.float32(0.002), cs))[1]
        prm = capi.default_params_dense(sigmaf_sq=1.0, l_sq=(res / 4) ** 2, noise=0.25, noise_model=2)
        cands = [(1.0, (res / 8) ** 2, 0.25), (1.0, (res / 4) ** 2, 0.25), (2.0, (res / 2) ** 2, 0.5)]
        P, m = mp.patches.view.P, mp.patches.view.m
        p, f, v, best, lq, st = (a.cpu().numpy() for a in mp.occupancy_select(prm, cands))
        assert p.shape == f.shape == v.shape == (P, m) and best.shape == lq.shape == st.shape == (P,)
        cells = mp.cells.cpu().numpy()
        seen = (cells != 0).any(axis=1)
        assert seen.any() and (~seen).any()
        assert np.all(best[~seen] == 0) and np.all(p[~seen] == 0.5) and np.all(v[~seen] == 1.0) and np.all(lq[~seen] == 0.0)
        won = best >= 0
        assert won.any() and np.all(best >= -1) and np.all(best < 3) and np.all(st[won] == 0)
        assert np.all(np.isfinite(lq[won])) and np.all(lq[won & seen] < 0.0) and np.all(np.isnan(lq[~won]))
        assert np.all(np.isfinite(p[won])) and np.array_equal(p[won] > 0.5, f[won] > 0.0)
        off, x0, x1, y, n_total, n_max = mp.patches.occupancy_batch(mp.cells)
        dev = mp.cells.device
        p2, f2, v2 = (torch.zeros((P, m), dtype=torch.float64, device=dev) for _ in range(3))
        lq2 = torch.zeros((P,), dtype=torch.float64, device=dev)
        best2, st2 = (torch.full((P,), -7, dtype=torch.int32, device=dev) for _ in range(2))
        torch.cuda.synchronize()
        ctx.dense_irls_select_dev(prm, capi.default_params_irls(), cands, P, off, n_max, n_total, x0, x1, y, m, None, None, res, sz, f_star=f2,
                                  v_star=v2, p_star=p2, log_q=lq2, best=best2, status=st2)
        ctx.synchronize()
        for a, b2 in ((p, p2), (f, f2), (v, v2), (lq, lq2), (best, best2), (st, st2)):
            assert _same_bits(a, b2.cpu().numpy())
        print("occupancy_select: %d leaves, %d seen; winners %s" % (P, int(seen.sum()), np.bincount(best[seen], minlength=3).tolist()))
    finally:
        mp.close()
