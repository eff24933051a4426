"""gpc_sparse_decode[_dev] (csrc/decode.hip): the masked decoder against the chain it replaces, by bytes.

The reference of every record is Sparse.predict_dev (depth, colour) -> Context.reproject_dev on the same objects and frames, computed once
per (object pair, sz); which rows of it the decoder must give, in which order, and the counts are the NumPy rule of tests/decode_cases.py
(checked without a GPU in tests/test_decode_cases_cpu.py).  States are readout_cases batches loaded with set_state, one leaf per basis
size; every leaf of a batch carries another mask pattern."""
import numpy as np
import pytest

import decode_cases as DC
import readout_cases as RC
import reproject_cases as RPC

pytestmark = pytest.mark.gpu
SENT_B, SENT_I = 0xA5, -7


@pytest.fixture(scope="module")
def gp():
    from gp_compressor_amd import capi
    capi.load()
    ctx = capi.Context(0)
    yield capi, ctx
    ctx.close()


def _load(capi, ctx, B):
    prm = capi.default_params_sparse(B["ny"], sigmaf_sq=RC.SF, l_sq=B["l_sq"], noise=RC.S20, capacity=B["capacity"])
    g = capi.Sparse(ctx, prm, B["P"], B["ny"])
    assert g.ld() == B["ld"]
    g.set_state(B["b"], B["alpha"], B["BV"], B["C"], None)
    return g


def _chain(ctx, gd, gc, b, sz, R, mu, cm, res=DC.RES):
    """the unmasked flow: (n_trained * m,) records in (leaf, p) order and row_of (P,): the first record of each trained leaf"""
    import torch
    P, m = len(b), sz * sz
    xs0, xs1 = (torch.from_numpy(a).cuda() for a in DC.grid_points(res, sz))
    f = torch.full((P, m), float("nan"), dtype=torch.float64, device="cuda")
    c = torch.full((P, 3, m), float("nan"), dtype=torch.float64, device="cuda") if gc is not None else None
    d_b = _dev(np.asarray(b, dtype=np.int32))
    d_R, d_mu = _dev(R), _dev(mu)
    d_cm = _dev(cm) if gc is not None else None
    cloud = torch.zeros((P * m, 32), dtype=torch.uint8, device="cuda")
    npts = torch.zeros(1, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    gd.predict_dev(m, xs0, xs1, f)
    if gc is not None:
        gc.predict_dev(m, xs0, xs1, c)
    ctx.reproject_dev(P, m, d_b, xs0, xs1, f, c, d_R, d_mu, d_cm, cloud, npts)
    ctx.synchronize()
    n = int(npts.cpu()[0])
    assert n == m * int(np.sum(b > 0))
    row_of = (np.cumsum(b > 0) - (b > 0)) * m
    return cloud.cpu().numpy()[:n].reshape(-1).view(RPC.POINT_DTYPE), row_of


@pytest.fixture(scope="module")
def world(gp):
    """pair name -> (depth Sparse, colour Sparse | None, b, frames); (pair name, sz) -> the chain's cloud.  Built once, only read."""
    capi, ctx = gp
    objs, clouds = {}, {}

    def pair(name):
        if name not in objs:
            Bd, Bc = DC.pair(name)
            objs[name] = (_load(capi, ctx, Bd), None if Bc is None else _load(capi, ctx, Bc), Bd["b"], DC.frames(Bd["P"]))
        return objs[name]

    def chain(name, sz):
        if (name, sz) not in clouds:
            gd, gc, b, (R, mu, cm) = pair(name)
            clouds[name, sz] = _chain(ctx, gd, gc, b, sz, R, mu, cm)
        return clouds[name, sz]

    yield pair, chain
    for gd, gc, _, _ in objs.values():
        gd.close()
        if gc is not None:
            gc.close()


def _expected(ref, row_of, b, sz, W, cells):
    leaf, point, count, n = DC.rule(b, sz, W, cells)
    return ref[row_of[leaf] + point], leaf, point, count, n


def _dev(a):
    import torch
    return None if a is None else torch.from_numpy(np.array(a, order="C")).cuda()      # (a copy: the cases are read-only arrays)


def _decode_dev(ctx, gd, gc, sz, W, cells, R, mu, cm, capacity=None, extra=0):
    """sizing call + decode through the _dev entry.  capacity None: exactly n_points.  The buffers hold capacity + extra entries and are
    sentinel-filled.  Returns cloud bytes (capacity + extra, 32), leaf, point, count, n_points of the sizing call and of the decode."""
    import torch
    P = gd.P
    d_W, d_cells, d_R, d_mu = _dev(W), _dev(cells), _dev(R), _dev(mu)
    d_cm = _dev(cm) if gc is not None else None
    count0 = torch.full((P,), SENT_I, dtype=torch.int32, device="cuda")
    n0 = torch.full((1,), SENT_I, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    gd.decode_dev(gc, DC.RES, sz, d_W, d_cells, d_R, d_mu, d_cm, 0, None, count=count0, n_points=n0)
    ctx.synchronize()
    n_size = int(n0.cpu()[0])
    cap = n_size if capacity is None else capacity
    cloud = torch.full((cap + extra + 1, 32), SENT_B, dtype=torch.uint8, device="cuda")
    leaf = torch.full((cap + extra + 1,), SENT_I, dtype=torch.int32, device="cuda")
    point = torch.full((cap + extra + 1,), SENT_I, dtype=torch.int32, device="cuda")
    count = torch.full((P,), SENT_I, dtype=torch.int32, device="cuda")
    n1 = torch.full((1,), SENT_I, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    gd.decode_dev(gc, DC.RES, sz, d_W, d_cells, d_R, d_mu, d_cm, cap, cloud, leaf=leaf, point=point, count=count, n_points=n1)
    ctx.synchronize()
    assert np.array_equal(count0.cpu().numpy(), count.cpu().numpy())
    return cloud.cpu().numpy(), leaf.cpu().numpy(), point.cpu().numpy(), count.cpu().numpy(), n_size, int(n1.cpu()[0])


def _records(raw, n):
    return raw[:n].reshape(-1).view(RPC.POINT_DTYPE)


# ---- 1. bit identity -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", DC.MASK_KINDS + ("nomask",))
@pytest.mark.parametrize("sz", DC.SIZES)
@pytest.mark.parametrize("name", list(DC.PAIRS))
def test_bit_identity(gp, world, name, sz, kind):
    capi, ctx = gp
    pair, chain = world
    gd, gc, b, (R, mu, cm) = pair(name)
    ref, row_of = chain(name, sz)
    P = len(b)
    W, cells = (None, None) if kind == "nomask" else DC.masks(P, sz, kind, rot=DC.SIZES.index(sz) + 3 * DC.MASK_KINDS.index(kind))
    want, leaf, point, count, n = _expected(ref, row_of, b, sz, W, cells)
    raw, g_leaf, g_point, g_count, n0, n1 = _decode_dev(ctx, gd, gc, sz, W, cells, R, mu, cm)
    assert n0 == n1 == n and np.array_equal(g_count, count)
    assert np.array_equal(g_leaf[:n], leaf) and np.array_equal(g_point[:n], point)
    bad = DC.same_records(_records(raw, n), want)
    assert bad is None, bad
    assert np.all(raw[n:] == SENT_B) and np.all(g_leaf[n:] == SENT_I) and np.all(g_point[n:] == SENT_I)
    if gc is None:
        rec = _records(raw, n)
        assert not rec["r"].any() and not rec["g"].any() and not rec["b"].any()


def test_row_flags_read_from_global_memory(gp, world):
    """sz = 129: m = 16641 is past the LDS row of the emit kernel (DC_ROW_MAX = 16384), which then reads the flags where they are"""
    capi, ctx = gp
    pair, _ = world
    gd, gc, b, (R, mu, cm) = pair("cap15-norgb")
    sz = DC.SZ_GLOBAL_ROW
    ref, row_of = _chain(ctx, gd, gc, b, sz, R, mu, cm)
    W, cells = DC.masks(len(b), sz, "both", rot=4)
    want, leaf, point, count, n = _expected(ref, row_of, b, sz, W, cells)
    raw, g_leaf, g_point, g_count, n0, n1 = _decode_dev(ctx, gd, gc, sz, W, cells, R, mu, cm)
    assert n0 == n1 == n > 0 and np.array_equal(g_count, count)
    assert np.array_equal(g_leaf[:n], leaf) and np.array_equal(g_point[:n], point)
    bad = DC.same_records(_records(raw, n), want)
    assert bad is None, bad


# ---- 2. sizing and truncation --------------------------------------------------------------------------------------------------------------
def test_sizing_and_truncation(gp, world):
    import torch
    capi, ctx = gp
    pair, chain = world
    name, sz = "cap100", 9
    gd, gc, b, (R, mu, cm) = pair(name)
    ref, row_of = chain(name, sz)
    W, cells = DC.masks(len(b), sz, "both", rot=1)
    want, leaf, point, count, n = _expected(ref, row_of, b, sz, W, cells)
    assert n > 64
    # the sizing call writes no record and no leaf / point entry, even when it is handed the buffers of those
    d = [_dev(a) for a in (W, cells, R, mu, cm)]
    lp = torch.full((2, n), SENT_I, dtype=torch.int32, device="cuda")
    cnt = torch.zeros(len(b), dtype=torch.int32, device="cuda")
    npts = torch.zeros(1, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    gd.decode_dev(gc, DC.RES, sz, *d, n, None, leaf=lp[0], point=lp[1], count=cnt, n_points=npts)
    ctx.synchronize()
    assert int(npts.cpu()[0]) == n and np.array_equal(cnt.cpu().numpy(), count) and np.all(lp.cpu().numpy() == SENT_I)
    for cap in (0, n - 1, n, n + 7):
        raw, g_leaf, g_point, g_count, n0, n1 = _decode_dev(ctx, gd, gc, sz, W, cells, R, mu, cm, capacity=cap, extra=9)
        w = min(n, cap)
        assert n0 == n1 == n and np.array_equal(g_count, count), cap
        bad = DC.same_records(_records(raw, w), want[:w])
        assert bad is None, (cap, bad)
        assert np.array_equal(g_leaf[:w], leaf[:w]) and np.array_equal(g_point[:w], point[:w])
        assert np.all(raw[w:] == SENT_B) and np.all(g_leaf[w:] == SENT_I) and np.all(g_point[w:] == SENT_I), cap


# ---- 3. scan edges -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("P", DC.SCAN_P)
def test_scan_edges(gp, P):
    """P = 1, 2, 1023, 1024, 1025, 2047, 2048, 2049.  decode_scan_kernel is one workgroup of 1024 threads; thread t holds the leaves
    [t per, (t + 1) per) with per = ceil(P / 1024), so the segments change shape where per steps: 1024 | 1025 (per 1 -> 2) and
    2048 | 2049 (2 -> 3); at 1023 the last thread and at 2047 the last leaf of the last thread are missing.  sz = 2, a basis of 0 or 1
    per leaf under every pattern of reproject_cases.bv_pattern, and a random W so that the counts 0 .. 4 all occur."""
    capi, ctx = gp
    sz, m = 2, 4
    rng = np.random.default_rng([17, P])
    prm = capi.default_params_sparse(1, sigmaf_sq=RC.SF, l_sq=RC.L5, noise=RC.S20, capacity=15)
    g = capi.Sparse(ctx, prm, P, 1)
    ld = g.ld()
    alpha = rng.normal(0, 0.05, (P, 1, ld))
    BV = rng.uniform(-DC.RES / 2, DC.RES / 2, (P, ld, 2))
    R, mu, _ = DC.frames(P, seed=9)
    W = rng.integers(0, 2, (P, m)).astype(np.uint8)
    try:
        for name in RPC.PATTERNS:
            b = DC.scan_batch(P, name)
            g.set_state(b, alpha, BV, None, None)
            ref, row_of = _chain(ctx, g, None, b, sz, R, mu, None)
            want, leaf, point, count, n = _expected(ref, row_of, b, sz, W, None)
            raw, g_leaf, g_point, g_count, n0, n1 = _decode_dev(ctx, g, None, sz, W, None, R, mu, None)
            assert n0 == n1 == n and np.array_equal(g_count, count), name
            assert np.array_equal(g_leaf[:n], leaf) and np.array_equal(g_point[:n], point), name
            bad = DC.same_records(_records(raw, n), want)
            assert bad is None, (name, bad)
    finally:
        g.close()


# ---- 4. repeatability ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ("both", "nomask"))
def test_repeatable_and_host_form(gp, world, kind):
    capi, ctx = gp
    pair, chain = world
    name, sz = "cap100", 20
    gd, gc, b, (R, mu, cm) = pair(name)
    W, cells = (None, None) if kind == "nomask" else DC.masks(len(b), sz, kind, rot=6)
    first = _decode_dev(ctx, gd, gc, sz, W, cells, R, mu, cm)
    second = _decode_dev(ctx, gd, gc, sz, W, cells, R, mu, cm)
    for a, c in zip(first, second):
        assert np.array_equal(a, c)
    n = first[5]
    cloud, leaf, point, count, n_host = gd.decode(gc, DC.RES, sz, R, mu, cm, W=W, cells=cells)
    assert n_host == n == len(cloud)
    assert cloud.tobytes() == _records(first[0], n).tobytes()
    assert np.array_equal(leaf, first[1][:n]) and np.array_equal(point, first[2][:n]) and np.array_equal(count, first[3])
    # the host form under a capacity below the count: the full count, that many records, nothing beyond them
    short = gd.decode(gc, DC.RES, sz, R, mu, cm, W=W, cells=cells, capacity=n - 5)
    assert short[4] == n and len(short[0]) == n - 5 and short[0].tobytes() == cloud[:n - 5].tobytes()


# ---- 5. error rules ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("form", ("host", "dev"))
def test_error_rules(gp, world, form):
    import torch
    capi, ctx = gp
    L = ctx.lib
    pair, _ = world
    gd, gc, b, (R, mu, cm) = pair("cap100")
    g15 = pair("cap15-norgb")[0]                      # another P
    P, sz, m = len(b), 3, 9
    cap = P * m
    entry = L.gpc_sparse_decode if form == "host" else L.gpc_sparse_decode_dev
    if form == "host":
        mk = lambda a: np.ascontiguousarray(a)
        outs = [np.full((cap, 32), SENT_B, np.uint8), np.full(cap, SENT_I, np.int32), np.full(cap, SENT_I, np.int32),
                np.full(P, SENT_I, np.int32), np.full(1, SENT_I, np.int32)]
        host = lambda a: a
    else:
        mk = _dev
        outs = [torch.full((cap, 32), SENT_B, dtype=torch.uint8, device="cuda")] + \
               [torch.full((k,), SENT_I, dtype=torch.int32, device="cuda") for k in (cap, cap, P, 1)]
        host = lambda a: a.cpu().numpy()
        torch.cuda.synchronize()
    d_R, d_mu, d_cm = mk(R), mk(mu), mk(cm)
    p = capi._ptr

    def call(depth=gd, rgb=gc, res=DC.RES, sz_=sz, rot=d_R, mean=d_mu, cmean=d_cm, capacity=cap, cloud=outs[0], n_points=outs[4]):
        return entry(depth.h if depth is not None else None, rgb.h if rgb is not None else None, float(res), int(sz_), None, None, p(rot),
                     p(mean), p(cmean), int(capacity), p(cloud), p(outs[1]), p(outs[2]), p(outs[3]), p(n_points))

    def untouched():
        ctx.synchronize()
        return all(np.all(host(o) == (SENT_B if i == 0 else SENT_I)) for i, o in enumerate(outs))

    other = capi.Context(0)
    foreign = capi.Sparse(other, capi.default_params_sparse(3, capacity=100), P, 3)
    ny1 = capi.Sparse(ctx, capi.default_params_sparse(1, capacity=100), P, 1)
    try:
        EINVAL = {
            "NULL depth": dict(depth=None),
            "rgb of another context": dict(rgb=foreign),
            "rgb with another P": dict(depth=g15),
            "rgb with ny != 3": dict(rgb=ny1),
            "depth with ny != 1": dict(depth=gc, rgb=None),
            "sz < 1": dict(sz_=0),
            "res not finite (nan)": dict(res=float("nan")),
            "res not finite (inf)": dict(res=float("inf")),
            "capacity < 0": dict(capacity=-1),
            "NULL rotations": dict(rot=None),
            "NULL means": dict(mean=None),
            "rgb without rgb_means": dict(cmean=None),
            "NULL n_points": dict(n_points=None),
        }
        for why, kw in EINVAL.items():
            assert call(**kw) == capi.GPC_EINVAL, why
            assert untouched(), why
        # P m > 2^31 - 1: 19 * 10632^2 = 2147749056
        assert call(sz_=10632) == capi.GPC_ERANGE and untouched()
        # a dead depth: its context destroyed while it lives
        dead = capi.Context(0)
        child = capi.Sparse(dead, capi.default_params_sparse(1), P, 1)
        h, dead.h = dead.h, None
        L.gpc_ctx_destroy(h)
        try:
            assert call(depth=child, rgb=None) == capi.GPC_EINVAL and untouched()
        finally:
            child.close()
        # NULL rotations / means are no error in the sizing call; rgb == NULL needs no rgb_means
        assert call(rot=None, mean=None, cloud=None, capacity=0) == capi.GPC_OK
        ctx.synchronize()
        assert int(host(outs[4])[0]) == m * int(np.sum(b > 0))
        assert call(rgb=None, cmean=None) == capi.GPC_OK
        ctx.synchronize()
        # P == 0: GPC_OK, n_points = 0
        empty = capi.Sparse(ctx, capi.default_params_sparse(1, capacity=15), 0, 1)
        assert call(depth=empty, rgb=None, rot=None, mean=None) == capi.GPC_OK
        ctx.synchronize()
        assert int(host(outs[4])[0]) == 0
        empty.close()
    finally:
        ny1.close()
        foreign.close()
        other.close()


# ---- 6. on a real map ----------------------------------------------------------------------------------------------------------------------
def test_real_map(gp):
    import torch
    from gp_compressor_amd import synth
    capi, ctx = gp
    res, sz = 0.15, 8
    m = sz * sz
    xyz, rgb = synth.plane_cloud(6000, seed=2)
    pt = ctx.project_cloud(ctx.make_cloud(xyz, rgb), res, sz)
    got = pt.fetch()
    P = pt.view.P
    hyp = dict(sigmaf_sq=1.0, l_sq=(res / 5) ** 2)
    gd = capi.Sparse(ctx, capi.default_params_sparse(1, noise=1e-3, capacity=24, **hyp), P, 1)
    gc = capi.Sparse(ctx, capi.default_params_sparse(3, noise=1.0, capacity=100, **hyp), P, 3)
    gd.add(got["off"], got["x0"], got["x1"], got["y"][None, :])
    gc.add(got["off"], got["x0"], got["x1"], got["rgb"])
    b = gd.sizes()
    Rcm = np.ascontiguousarray(got["R"].transpose(0, 2, 1).reshape(P, 9))
    full, row_of = _chain(ctx, gd, gc, b, sz, Rcm, got["mean"], got["rgb_mean"], res=res)
    out = pt.decode(gd, gc, use_w=True, want=("leaf", "point", "count"))
    leaf, point, count, n = DC.rule(b, sz, got["W"])
    assert n == int(got["W"][b > 0].astype(bool).sum()) == len(out["cloud"]) and 0 < n < m * int(np.sum(b > 0))
    assert np.array_equal(out["leaf"], leaf) and np.array_equal(out["point"], point) and np.array_equal(out["count"], count)
    bad = DC.same_records(out["cloud"], full[row_of[leaf] + point])
    assert bad is None, bad
    # unmasked, the decoder is the whole flow
    assert pt.decode(gd, gc, use_w=False, want=())["cloud"].tobytes() == full.tobytes()
    # a scan of the same surface, moved by a patch, goes into the map; the rays label cells, and no decoded point lies in a FREE one
    mp = capi.Mapping(ctx, pt, gd, gc, capi.default_params_registration(step=1e-7, tol=1e300, min_steps=2, max_steps=10), min_nbr=20)
    try:
        moved = xyz + np.array([res, 0.0, 0.0], dtype=np.float32)
        steps, inserted = mp.add_cloud(ctx.make_cloud(moved, rgb))
        assert inserted
        mp.cells[1::2, 5::7] = capi.CELL_FREE        # (whatever the rays labelled: cells that are FREE for certain)
        torch.cuda.synchronize()
        cells = mp.cells.cpu().numpy()
        assert np.any(cells == capi.CELL_FREE) and np.any(cells != capi.CELL_FREE)
        v = mp.patches.view
        W2 = mp.patches.fetch()["W"]
        b2 = mp.depth.sizes()
        for use_w in (True, False):
            o = mp.decode(use_cells=True, use_w=use_w)
            leaf2, point2, _, n2 = DC.rule(b2, sz, W2 if use_w else None, cells)
            assert len(o["cloud"]) == n2 > 0 and np.array_equal(o["leaf"], leaf2) and np.array_equal(o["point"], point2)
            assert not np.any(cells.reshape(v.P, m)[o["leaf"], DC.cell_of(o["point"], sz)] == capi.CELL_FREE)
        assert len(mp.decode(use_cells=False, use_w=False, want=())["cloud"]) == m * int(np.sum(b2 > 0))
    finally:
        mp.close()

