"""gpc_rate_allocate_dev on the GPU against the NumPy restatement of the rule (rate_alloc_ref.py), bit for bit: the row counts around the
workgroup shapes of the sweep (4 rows per workgroup) and of the scan (tiles of 256 rows), the grid-stride wrap and the multi-tile scan
under GPC_ALLOC_BLOCKS, the lane-stride edges of a long curve, repeatability and the host-pointer form."""
import numpy as np
import pytest

import rate_alloc_ref as RA

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def gp():
    from gp_compressor_amd import capi
    capi.load()
    ctx = capi.Context(0)
    yield capi, ctx
    ctx.close()


def _dev(capi, ctx, pb, need, refine, count=None):
    """one call of the _dev form on fresh device buffers: (k, target, result)"""
    import torch
    up = lambda a: None if a is None else torch.from_numpy(np.ascontiguousarray(a)).cuda()
    kmax, d0, d, w, unit, cnt = (up(a) for a in (pb.kmax, pb.d0, pb.d, pb.w, pb.unit, count))
    k = torch.full((pb.R,), -7, dtype=torch.int32, device="cuda")
    tg = torch.full((pb.R,), -7, dtype=torch.int32, device="cuda") if count is not None else None
    res = torch.zeros(32, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    ctx.rate_allocate_dev(pb.R, pb.ld, kmax, d0, d, need, w=w, w_all=pb.w_all, unit=unit, unit_all=pb.unit_all, refine=refine, count=cnt, k=k,
                          target=tg, result=res)
    ctx.synchronize()
    return k.cpu().numpy(), None if tg is None else tg.cpu().numpy(), capi.rate_result(res)


def _equal(got, want, tag):
    k, tg, res = got
    assert np.array_equal(k, want["k"]), tag
    if want["target"] is not None:
        assert np.array_equal(tg, want["target"]), tag
    for f in ("lambda_bits", "saved", "max_saving", "feasible", "switched_rows"):
        assert res[f] == want[f], (tag, f, res[f], want[f])


def _problem(R, ld, seed):
    """rows that tie in groups (every curve appears up to three times), mixed units, weights, NaN holes and fixed rows"""
    base = RA.random_problem(seed=seed, R=R, ld=ld, kind="nan" if seed % 2 else "monotone", units="mixed", weights="rows")
    src = (np.arange(R) // 3) * 3 if R > 2 else np.arange(R)
    return RA.Problem(base.kmax[src], base.d0[src], base.d[src], w=base.w[src], unit=base.unit[src])


def _some_needs(pb):
    ms = RA.saving(pb, RA.choice(pb, float("inf")))
    return [0, ms // 3, ms // 2 + 5, ms, ms + 1]


# R one below, at and one above the rows of a sweep's workgroup (4) and of a scan tile (256); R = 1
@pytest.mark.parametrize("R", [1, 3, 4, 5, 255, 256, 257])
def test_rate_allocate_dev_equals_the_restatement(gp, R):
    capi, ctx = gp
    pb = _problem(R, 9, seed=R)
    count = (pb.kmax + 1 - (np.arange(R) % 2)).astype(np.int32)
    for need in _some_needs(pb):
        for refine in (1, 0):
            _equal(_dev(capi, ctx, pb, need, refine, count), RA.allocate(pb, need, refine, count), (R, need, refine))


def test_grid_stride_wrap_and_multi_tile_scan(gp, monkeypatch):
    """two workgroups per launch: 8 rows per sweep pass and two tiles per scan pass, with 700 rows in three tiles"""
    capi, ctx = gp
    pb = _problem(700, 9, seed=12)
    want = {need: RA.allocate(pb, need, 1) for need in _some_needs(pb)}
    free = {need: _dev(capi, ctx, pb, need, 1) for need in want}
    monkeypatch.setenv("GPC_ALLOC_BLOCKS", "2")
    for need, w in want.items():
        got = _dev(capi, ctx, pb, need, 1)
        _equal(got, w, ("capped", need))
        _equal(free[need], w, ("free", need))
    assert any(w["switched_rows"] > 0 for w in want.values()), "no case reaches the refinement"
    monkeypatch.setenv("GPC_ALLOC_BLOCKS", "1")
    need = _some_needs(pb)[2]
    _equal(_dev(capi, ctx, pb, need, 1), want[need], ("one workgroup", need))


def test_lane_stride_edges_of_a_long_curve(gp):
    """ld = 257: kmax on both sides of one, two and four passes of the 64 lanes; the best option placed at the edges"""
    capi, ctx = gp
    kmax = np.array([0, 1, 63, 64, 65, 128, 256, 256, 128, 65], dtype=np.int32)
    rng = np.random.default_rng(5)
    e = np.cumsum(rng.random((len(kmax), 258)) ** 2, axis=1)
    for r, at in enumerate((0, 1, 63, 64, 64, 127, 255, 192, 128, 65)):     # a dip: the cheapest error sits at option `at`
        e[r, at] = -1.0
    pb = RA.Problem(kmax, e[:, 0].copy(), e[:, 1:].copy(), w_all=1.0, unit_all=40)
    for need in _some_needs(pb) + [40, 40 * 300]:
        for refine in (1, 0):
            _equal(_dev(capi, ctx, pb, need, refine), RA.allocate(pb, need, refine), (need, refine))


def test_repeatable_and_host_pointer_form(gp):
    capi, ctx = gp
    pb = _problem(257, 9, seed=31)
    count = (pb.kmax + 1).astype(np.int32)
    need = _some_needs(pb)[1]
    a, b = _dev(capi, ctx, pb, need, 1, count), _dev(capi, ctx, pb, need, 1, count)
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) and a[2] == b[2]
    k, tg, res = ctx.rate_allocate(pb.kmax, pb.d0, pb.d, need, w=pb.w, unit=pb.unit, count=count)
    assert np.array_equal(k, a[0]) and np.array_equal(tg, a[1]) and res == a[2]
    k2, res2 = ctx.rate_allocate(pb.kmax, pb.d0, pb.d, need, w=pb.w, unit=pb.unit)
    assert np.array_equal(k2, k) and res2 == res
    # all-equal weights through w_all, one unit through unit_all
    pu = RA.Problem(pb.kmax, pb.d0, pb.d, w_all=2.5, unit_all=40)
    _equal(_dev(capi, ctx, pu, need, 1), RA.allocate(pu, need, 1), "w_all")


def test_empty_problem_and_argument_errors(gp):
    capi, ctx = gp
    L = ctx.lib
    for fn in (L.gpc_rate_allocate, L.gpc_rate_allocate_dev):
        assert fn(ctx.h, 0, 1, None, None, None, None, 1.0, None, 24, 10, 1, None, None, None, None) == capi.GPC_OK
        for bad in ((-1, 1, 1.0, 24), (0, 0, 1.0, 24), (0, 1, float("nan"), 24), (0, 1, -1.0, 24), (0, 1, 1.0, 0)):
            R, ld, w_all, unit_all = bad
            assert fn(ctx.h, R, ld, None, None, None, None, w_all, None, unit_all, 10, 1, None, None, None, None) == capi.GPC_EINVAL, bad
        assert fn(ctx.h, 2, 1, None, None, None, None, 1.0, None, 24, 10, 1, None, None, None, None) == capi.GPC_EINVAL     # NULL rows
    with pytest.raises(capi.GpcError):
        ctx.rate_allocate_dev(0, 1, None, None, None, 0, target=1)                                                          # target without count
