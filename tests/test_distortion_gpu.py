"""gpc_cloud_distortion and gpc_patches_normals on the GPU against the NumPy restatement (tests/distortion_ref.py: a brute-force scan),
BY BITS: the neighbour index, d2, e2, the counts, every sum and maximum.  No tolerance anywhere: the nearest neighbour is exact at
every cell, and the sums have one order."""
import ctypes as C

import numpy as np
import pytest

import distortion_cases as DC
import distortion_ref as DR

pytestmark = pytest.mark.gpu

ALL = ("nn", "d2", "e2")


@pytest.fixture(scope="module")
def gp():
    from gp_compressor_amd import capi
    capi.load()
    ctx = capi.Context(0)
    yield capi, ctx
    ctx.close()


def _device(arr):
    import torch
    d = torch.from_numpy(np.ascontiguousarray(arr).view(np.uint8).reshape(-1)).cuda()
    torch.cuda.synchronize()
    return d


def _bytes(r):
    return b"".join(np.ascontiguousarray(np.asarray(r[k])).tobytes() for k in DR.RESULT_KEYS + ALL)


@pytest.fixture(scope="module")
def lattice():
    a, b, ties = DC.lattice()
    return a, b, DR.distortion(a, b)


def test_lattice_ties_go_to_the_lowest_index_at_every_cell(gp, lattice):
    _, ctx = gp
    a, b, ref = lattice
    runs = [ctx.cloud_distortion(a, b, cell=cell, want=ALL) for cell in DC.LATTICE_CELLS]
    for cell, got in zip(DC.LATTICE_CELLS, runs):
        print("cell", cell, "sse_d1", got["sse_d1"], "matched", got["n_matched"])
        DR.assert_same(got, ref)
    assert len({_bytes(r) for r in runs}) == 1                # no output depends on the cell


def test_points_outside_the_box(gp):
    _, ctx = gp
    a, b, cell = DC.outside_box()
    ref = DR.distortion(a, b)
    for c in (cell, 0.0):
        DR.assert_same(ctx.cloud_distortion(a, b, cell=c, want=ALL), ref)


def test_sparse_table(gp):
    _, ctx = gp
    a, b, cell = DC.sparse_table()
    ref = DR.distortion(a, b)
    for c in (cell, 0.0):
        DR.assert_same(ctx.cloud_distortion(a, b, cell=c, want=ALL), ref)


@pytest.mark.parametrize("na,nb", [(1, 40), (40, 1), (0, 40), (40, 0), (0, 0)] + [(n, 300) for n in DC.SUM_SIZES] + [(64 * 4096 + 1, 50)])
def test_sizes(gp, na, nb):
    _, ctx = gp
    a, b = DC.random_pair(na, nb, seed=na + 7 * nb)
    nrm, _, _ = DC.unit_normals(nb, seed=nb, zeros=0) if nb else (None, None, None)
    ref = DR.distortion(a, b, nrm)
    got = ctx.cloud_distortion(a, b, nrm, want=ALL)
    DR.assert_same(got, ref)
    if nb == 0 or na == 0:
        assert got["n_matched"] == 0 and got["sse_d1"] == 0.0 and got["sse_luma"] == 0.0 and np.all(got["nn"] == -1)
    assert got["n_valid"] == na


def test_max_dist(gp, lattice):
    _, ctx = gp
    a, b, _ = lattice
    extra = DR.make_cloud(np.array([[-1.0, 2.0, 3.0], [-1.0, -1.0, 3.0], [2.0, 2.0, 2.0], [2.0, 2.0, 2.25]]), np.full((4, 3), 9))
    a = np.concatenate([a, extra])
    for md in (1.0, 0.0, 0.5, 0.8660254037844386):
        ref = DR.distortion(a, b, max_dist=md)
        for cell in (0.0, 1.0):
            DR.assert_same(ctx.cloud_distortion(a, b, cell=cell, max_dist=md, want=ALL), ref)
    one = ctx.cloud_distortion(a, b, max_dist=1.0)
    assert one["d2"][-4] == 1.0 and one["nn"][-3] == -1       # d2 exactly 1 is matched, d2 = 2 is not
    zero = ctx.cloud_distortion(a, b, max_dist=0.0)
    assert np.array_equal(zero["nn"] >= 0, DR.distortion(a, b)["d2"] == 0.0) and 0 < zero["n_matched"] < zero["n_valid"]


def test_invalid_records(gp):
    _, ctx = gp
    a, b = DC.random_pair(700, 500, seed=11)
    ai, hit_a = DC.with_invalid(a, seed=12)
    bi, hit_b = DC.with_invalid(b, seed=13)
    ref = DR.distortion(ai, bi)
    got = ctx.cloud_distortion(ai, bi, want=ALL)
    DR.assert_same(got, ref)
    assert np.all(got["nn"][hit_a] == -1) and not np.any(hit_b[got["nn"][~hit_a]]) and got["n_valid"] == int((~hit_a).sum())
    org, holes = DC.organised()
    as_b = ctx.cloud_distortion(a, org, want=ALL)             # an organised cloud with NaN misses, as either argument
    DR.assert_same(as_b, DR.distortion(a, org))
    assert not np.any(holes[as_b["nn"]])                      # the indices refer to the original B
    as_a = ctx.cloud_distortion(org, b, want=ALL)
    DR.assert_same(as_a, DR.distortion(org, b))
    assert as_a["n_valid"] == int((~holes).sum()) and np.all(np.isnan(as_a["d2"][holes]))


def test_far_points_and_coincident_clouds(gp):
    _, ctx = gp
    a, b = DC.random_pair(300, 400, seed=14)
    far = DR.make_cloud(np.array([[1e30, 0, 0], [-3e38, 3e38, 1.0], [0.5, 0.5, 1e10], [0.5, 0.5, -7.0]], dtype=np.float32))
    for cell in (0.0, 0.05):
        DR.assert_same(ctx.cloud_distortion(far, b, cell=cell, want=ALL), DR.distortion(far, b))
    same = ctx.cloud_distortion(b, b, want=ALL)
    assert same["sse_d1"] == 0.0 and same["max_d1"] == 0.0 and same["sse_luma"] == 0.0 and same["n_matched"] == len(b)
    single = np.repeat(b[:1], 33)                             # every record of B at one place: one voxel, ties over all of B
    got = ctx.cloud_distortion(a, single, want=ALL)
    DR.assert_same(got, DR.distortion(a, single))
    assert np.all(got["nn"] == 0)


def test_normals_and_colours(gp):
    _, ctx = gp
    a, b = DC.random_pair(900, 600, seed=15)
    nrm, bad, zero = DC.unit_normals(len(b), seed=16)
    near = b[zero].copy()                                     # a millimetre off the records that carry a zero normal: theirs for sure
    near["z"] += np.float32(0.001)
    a = np.concatenate([a, near])
    ref = DR.distortion(a, b, nrm)
    got = ctx.cloud_distortion(a, b, nrm, want=ALL)
    DR.assert_same(got, ref)
    assert np.array_equal(np.isnan(got["e2"]), bad[got["nn"]]) and got["n_plane"] == int((~bad[got["nn"]]).sum()) < got["n_matched"]
    at_zero = np.isin(got["nn"], zero)
    assert at_zero.sum() >= len(zero) and np.all(got["e2"][at_zero] == 0.0) and np.all(got["d2"][at_zero] > 0.0)
    assert got["sse_rgb"].min() > 0 and got["sse_luma"] > 0
    none = ctx.cloud_distortion(a, b, want=ALL)               # without normals: no plane error anywhere
    assert none["n_plane"] == 0 and none["sse_d2"] == 0.0 and np.all(np.isnan(none["e2"]))


def test_repeatable_and_the_device_form_is_the_host_form(gp):
    import torch
    capi, ctx = gp
    a, b = DC.random_pair(5000, 3000, seed=17)
    a, _ = DC.with_invalid(a, seed=18, share=0.05)
    nrm, _, _ = DC.unit_normals(len(b), seed=19)
    first = ctx.cloud_distortion(a, b, nrm, want=ALL)
    again = ctx.cloud_distortion(a, b, nrm, want=ALL)
    assert _bytes(first) == _bytes(again)
    d_a, d_b, d_n = _device(a), _device(b), _device(nrm)
    nn = torch.full((len(a),), 7, dtype=torch.int32, device="cuda")
    d2 = torch.zeros(len(a), dtype=torch.float64, device="cuda")
    e2 = torch.zeros(len(a), dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()
    res = ctx.cloud_distortion_dev(d_a, len(a), d_b, len(b), d_n, nn=nn, d2=d2, e2=e2)
    dev = dict(res, nn=nn.cpu().numpy(), d2=d2.cpu().numpy(), e2=e2.cpu().numpy())
    assert _bytes(dev) == _bytes(first)
    only = ctx.cloud_distortion_dev(d_a, len(a), d_b, len(b), d_n)      # no per-point output: the same result record
    assert all(DR.same_bits(np.asarray(only[k]), np.asarray(first[k])) for k in DR.RESULT_KEYS)
    DR.assert_same(first, DR.distortion(a, b, nrm))


def _raw(capi, ctx, a, na, b, nb, cell=0.0, max_dist=float("inf"), result=True, handle=True):
    """the host entry with sentinel-filled outputs: returns the code and whether every output is untouched"""
    n = max(len(a), 1)
    nn, d2, e2 = np.full(n, 77, np.int32), np.full(n, 7.5), np.full(n, 7.5)
    res = np.full(capi.DISTORTION_RESULT_DTYPE.itemsize, 0x5a, np.uint8)
    prm = capi.DistortionParams(cell, max_dist)
    rc = ctx.lib.gpc_cloud_distortion(ctx.h if handle else None, a.ctypes.data if a is not None and len(a) else None, na,
                                      b.ctypes.data if b is not None and len(b) else None, nb, None, C.byref(prm), nn.ctypes.data,
                                      d2.ctypes.data, e2.ctypes.data, res.ctypes.data if result else None)
    return rc, bool(np.all(nn == 77) and np.all(d2 == 7.5) and np.all(e2 == 7.5) and np.all(res == 0x5a))


def test_errors_write_nothing(gp):
    import torch
    capi, ctx = gp
    a, b = DC.random_pair(50, 60, seed=20)
    none = a[:0]
    E, R = capi.GPC_EINVAL, capi.GPC_ERANGE
    assert _raw(capi, ctx, a, len(a), b, len(b)) == (capi.GPC_OK, False)
    cases = [(dict(handle=False), E), (dict(na=-1), E), (dict(nb=-1), E), (dict(a=none), E), (dict(b=none), E), (dict(result=False), E),
             (dict(cell=-1.0), E), (dict(cell=float("inf")), E), (dict(cell=float("nan")), E), (dict(max_dist=float("nan")), E),
             (dict(max_dist=-0.5), E), (dict(cell=1e-9), R)]
    for kw, code in cases:
        args = dict(a=a, na=len(a), b=b, nb=len(b))
        args.update(kw)
        assert _raw(capi, ctx, **args) == (code, True), kw
    assert "2^21" in ctx.lib.gpc_last_error(ctx.h).decode()
    # a context that was destroyed while one of its objects lives on
    other = capi.Context(0)
    keep = other.project_cloud(a, 0.15, 4)
    dead = other.h
    other._children.discard(keep)
    other.close()
    res = np.full(capi.DISTORTION_RESULT_DTYPE.itemsize, 0x5a, np.uint8)
    assert ctx.lib.gpc_cloud_distortion(dead, a.ctypes.data, len(a), b.ctypes.data, len(b), None, None, None, None, None, res.ctypes.data) == E
    assert np.all(res == 0x5a)
    keep.close()
    # the device form refuses the same things and leaves its buffers alone
    d_a, d_b = _device(a), _device(b)
    out = torch.full((len(a),), 7.5, dtype=torch.float64, device="cuda")
    rec = torch.full((capi.DISTORTION_RESULT_DTYPE.itemsize,), 0x5a, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    for kw, code in ((dict(cell=-1.0), E), (dict(max_dist=float("nan")), E), (dict(cell=1e-9), R)):
        with pytest.raises(capi.GpcError) as err:
            ctx.cloud_distortion_dev(d_a, len(a), d_b, len(b), d2=out, result=rec, **kw)
        assert err.value.code == code
    ctx.synchronize()
    assert bool((out == 7.5).all()) and bool((rec == 0x5a).all())
    # na == 0 is not an error: the result is all zero
    rc, untouched = _raw(capi, ctx, none, 0, b, len(b))
    assert rc == capi.GPC_OK and not untouched
    zero = ctx.cloud_distortion(none, b)
    assert all(np.all(np.asarray(zero[k]) == 0) for k in DR.RESULT_KEYS)


@pytest.mark.parametrize("case", ["plane", "two_planes"])
def test_patches_normals(gp, case):
    import torch
    from gp_compressor_amd import synth
    capi, ctx = gp
    xyz, rgb = synth.plane_cloud(3000, seed=2, extent=0.6) if case == "plane" else DC.two_planes()
    n = len(xyz)
    pt = ctx.project_cloud(ctx.make_cloud(xyz, rgb), 0.15, 10)
    batch = pt.fetch()
    want = DR.patches_normals(batch, n)
    got = pt.normals(n)
    assert DR.same_bits(got, want)
    unowned = np.setdiff1d(np.arange(n), batch["src"])
    assert np.array_equal(np.flatnonzero(np.isnan(got).any(1)), unowned)          # NaN exactly at the unowned points
    if case == "two_planes":
        assert len(unowned) > 0
    dev = torch.zeros((n + 5, 3), dtype=torch.float32, device="cuda")             # a longer cloud: the tail is unowned
    torch.cuda.synchronize()
    pt.normals(n + 5, out=dev)
    ctx.synchronize()
    assert DR.same_bits(dev.cpu().numpy(), np.concatenate([want, np.full((5, 3), np.nan, np.float32)]))
    # a cloud shorter than the batch's is another cloud: EINVAL, nothing written
    sentinel = np.full((n, 3), 3.0, dtype=np.float32)
    short = pt.view.n_total - 1
    assert ctx.lib.gpc_patches_normals(pt.h, short, sentinel.ctypes.data) == capi.GPC_EINVAL and np.all(sentinel == 3.0)
    if int(batch["src"].max()) >= pt.view.n_total:            # ... also where only a src entry gives it away
        assert ctx.lib.gpc_patches_normals(pt.h, int(batch["src"].max()), sentinel.ctypes.data) == capi.GPC_EINVAL and np.all(sentinel == 3.0)
    assert ctx.lib.gpc_patches_normals(pt.h, n, None) == capi.GPC_EINVAL and ctx.lib.gpc_patches_normals(None, n, sentinel.ctypes.data) == capi.GPC_EINVAL
    # and D2 with them: the producer's normals as normals_b, by bits against the restatement
    cloud = ctx.make_cloud(xyz, rgb)
    moved = ctx.make_cloud(xyz + np.float32(0.003), rgb)
    DR.assert_same(ctx.cloud_distortion(moved, cloud, got, want=ALL), DR.distortion(moved, cloud, want))
    pt.close()
