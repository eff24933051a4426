"""GPU parity of the patch producer (gp_compressor::project_cloud + compute_rotation +
project_points, src/gp_compressor.cpp:177-249, 29-64, 66-118) against the CPU oracle (orc_project_cloud).  Index, byte
and floating-point outputs alike are BIT-EXACT: the kernels evaluate the oracle's expressions in its order."""
import numpy as np
import pytest

from gp_compressor_amd import synth

pytestmark = pytest.mark.gpu

KEYS = ("off", "x0", "x1", "y", "rgb", "R", "mean", "rgb_mean", "W", "src")


@pytest.fixture(scope="module")
def gp():
    from gp_compressor_amd import capi
    capi.load()
    ctx = capi.Context(0)
    yield capi, ctx
    ctx.close()


def _same(a, b):
    for k in KEYS:
        assert a[k].shape == b[k].shape, k
        assert np.array_equal(a[k], b[k]), (k, int(np.sum(a[k] != b[k])))


@pytest.mark.parametrize("case", ["c1_plane", "room", "room_fine", "tilted_sheet", "volume", "far_offset", "lattice"])
def test_producer_matches_oracle_bit_for_bit(gp, oracle, case):
    capi, ctx = gp
    if case == "c1_plane":                        # BASELINE config 1: 10 k points, res 0.15, sz 20
        xyz, rgb = synth.plane_cloud(10000, seed=1)
        res, sz = 0.15, 20
    elif case == "room":                          # every branch of the frame construction, shared spheres at the edges
        xyz, rgb = synth.room_cloud(200000, seed=3)
        res, sz = 0.15, 20
    elif case == "room_fine":                     # many small leaves (lots of them below 4 points: identity frames)
        xyz, rgb = synth.room_cloud(60000, seed=5)
        res, sz = 0.04, 6
    elif case == "tilted_sheet":                  # a sheet at 45 degrees: |n_x| == |n_z| up to rounding, negative coordinates
        xyz, rgb = synth.plane_cloud(30000, seed=7)
        c, s = np.cos(np.pi / 4), np.sin(np.pi / 4)
        xyz = (xyz.astype(np.float64) @ np.array([[c, 0, s], [0, 1, 0], [-s, 0, c]]).T - 0.7).astype(np.float32)
        res, sz = 0.1, 10
    elif case == "volume":                        # a filled cube: all 27 neighbours occupied, no plane to fit, every point has
        rng = np.random.default_rng(21)           # many candidate owners -- the ownership rule decides
        xyz = rng.uniform(-0.5, 0.5, (120000, 3)).astype(np.float32)
        rgb = rng.integers(0, 256, (120000, 3)).astype(np.uint8)
        res, sz = 0.1, 8
    elif case == "far_offset":                    # a small scene 2 km from the origin: the float coordinates are quantised to 1.2e-4
        xyz, rgb = synth.room_cloud(40000, seed=8, size=(2.0, 1.5, 1.0))
        xyz = (xyz.astype(np.float64) + np.array([2000.0, -1500.0, 300.0])).astype(np.float32)
        res, sz = 0.07, 10
    else:                                         # points ON the voxel faces and many exact duplicates: ties in every comparison
        g = np.arange(0, 9) * 0.125
        xyz = np.stack(np.meshgrid(g, g, g[:3], indexing="ij"), -1).reshape(-1, 3)
        xyz = np.concatenate([xyz, xyz, xyz + np.array([0.0625, 0.0, 0.0])]).astype(np.float32)
        rgb = (np.arange(3 * len(xyz)).reshape(-1, 3) * 5 % 256).astype(np.uint8)
        res, sz = 0.125, 4
    want = oracle.project_cloud(xyz, rgb, res, sz)
    pt = ctx.project_cloud(ctx.make_cloud(xyz, rgb), res, sz)
    got = pt.fetch()
    v = pt.view
    assert (v.P, v.n_total, v.m) == (len(want["off"]) - 1, int(want["off"][-1]), sz * sz)
    assert v.n_max == int(np.diff(want["off"]).max())
    _same(got, want)
    # the contract the GP kernels rely on
    assert len(np.unique(got["src"])) == v.n_total                       # exclusive ownership
    assert np.all(np.abs(got["x0"]) <= res / 2) and np.all(np.abs(got["x1"]) <= res / 2)
    pt.close()


def _device(cloud):
    import torch
    d = torch.from_numpy(cloud.view(np.uint8).reshape(-1, 32)).cuda()
    torch.cuda.synchronize()
    return d


def test_producer_edge_cases(gp, oracle):
    capi, ctx = gp
    # empty cloud
    pt = ctx.project_cloud(ctx.make_cloud(np.zeros((0, 3)), np.zeros((0, 3))), 0.1, 4)
    assert (pt.view.P, pt.view.n_total) == (0, 0) and np.array_equal(pt.fetch()["off"], [0])
    pt.close()
    # fewer than 4 points in a sphere: identity frame (src/gp_compressor.cpp:31-34); one point; coincident points
    for xyz in (np.array([[0.01, 0.02, 0.03], [0.02, 0.01, 0.03], [0.9, 0.9, 0.9]]), np.array([[1.0, -2.0, 3.0]]),
                np.tile(np.array([[0.5, 0.5, 0.5]]), (70, 1))):
        rgb = (np.arange(3 * len(xyz)).reshape(-1, 3) * 7 % 256).astype(np.uint8)
        want = oracle.project_cloud(xyz, rgb, 0.1, 4)
        cloud = ctx.make_cloud(xyz, rgb)
        pt = ctx.project_cloud(cloud, 0.1, 4)
        _same(pt.fetch(), want)
        # the device-pointer entry on the same cloud: the same batch
        pt_dev = ctx.project_cloud(_device(cloud), 0.1, 4, n=len(cloud))
        _same(pt_dev.fetch(), pt.fetch())
        assert pt_dev.view.n_max == pt.view.n_max
        pt_dev.close()
        pt.close()
    # argument checking: never aborts, reports
    cloud = ctx.make_cloud(np.array([[0, 0, 0], [1, 1, 1]]), np.zeros((2, 3)))
    for bad_res in (0.0, -1.0, float("nan")):
        with pytest.raises(capi.GpcError) as e:
            ctx.project_cloud(cloud, bad_res, 4)
        assert e.value.code == capi.GPC_EINVAL
    with pytest.raises(capi.GpcError) as e:
        ctx.project_cloud(cloud, 0.1, 0)
    assert e.value.code == capi.GPC_EINVAL
    with pytest.raises(capi.GpcError) as e:
        ctx.project_cloud(cloud, 1e-7, 4)                               # 10^7 voxels along an axis
    assert e.value.code == capi.GPC_ERANGE
    for bad in (np.nan, np.inf):
        c2 = cloud.copy()
        c2["y"][1] = bad
        with pytest.raises(capi.GpcError) as e:
            ctx.project_cloud(c2, 0.1, 4)
        assert e.value.code == capi.GPC_EINVAL


def test_producer_feeds_the_gp_kernels_on_device(gp, oracle):
    """cloud -> patches -> dense GP -> cloud without a host pass over the points: the producer's device view goes straight
    into gpc_dense_fit_predict_grid_dev and gpc_reproject_dev; same result as the host-buffer entry points on the fetched
    batch."""
    import torch
    capi, ctx = gp
    res, sz = 0.15, 20
    xyz, rgb = synth.plane_cloud(10000, seed=1)
    cloud = ctx.make_cloud(xyz, rgb)
    d_cloud = torch.from_numpy(cloud.view(np.uint8).reshape(-1, 32)).cuda()
    pt = ctx.project_cloud(d_cloud, res, sz, n=len(cloud))
    v = pt.view
    b = pt.fetch()
    assert np.array_equal(b["off"], oracle.project_cloud(xyz, rgb, res, sz)["off"])
    pt_host = ctx.project_cloud(cloud, res, sz)                       # the host-pointer entry on the same cloud: the same batch
    _same(pt_host.fetch(), b)
    assert (pt_host.view.P, pt_host.view.n_total, pt_host.view.n_max) == (v.P, v.n_total, v.n_max)
    pt_host.close()
    p = capi.default_params_dense(sigmaf_sq=1.0, l_sq=(res / 8) ** 2, noise=1e-4)
    m = sz * sz
    f = torch.zeros(v.P, m, dtype=torch.float64, device="cuda")
    st = torch.zeros(v.P, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    ctx.dense_fit_predict_grid_dev(p, v.P, v.off, v.n_max, v.n_total, v.x0, v.x1, v.y, 1, res, sz, f, status=st)
    out = torch.zeros(v.P * m, 32, dtype=torch.uint8, device="cuda")
    npts = torch.zeros(1, dtype=torch.int32, device="cuda")
    xs0, xs1 = synth.grid(res, sz)
    d_xs0, d_xs1 = torch.from_numpy(xs0).cuda(), torch.from_numpy(xs1).cuda()
    torch.cuda.synchronize()                       # the context enqueues on its own stream
    ctx.reproject_dev(v.P, m, None, d_xs0, d_xs1, f, None, v.rotations, v.means, None, out, npts)
    ctx.synchronize()
    torch.cuda.synchronize()
    assert int(npts.item()) == v.P * m
    f_host, st_host = ctx.dense_fit_predict_grid(p, b["off"], b["x0"], b["x1"], b["y"][None, :], res, sz)
    assert np.array_equal(st.cpu().numpy(), st_host)
    ok = st_host == 0
    assert ok.sum() >= 0.9 * v.P
    # two launches of the dense kernel agree to rounding (its partial sums meet in LDS atomics, in arrival order)
    assert np.max(np.abs(f.cpu().numpy()[ok] - f_host.reshape(v.P, m)[ok])) <= 1e-9 * np.max(np.abs(f_host.reshape(v.P, m)[ok]))
    rec = out.cpu().numpy().view(capi.Context.POINT_DTYPE).reshape(v.P, m)
    # the reconstructed surface lies on the input surface: z = 0.02 sin(3x) cos(2y) within the sensor noise
    r = rec[ok].reshape(-1)
    inside = (r["x"] > 0.05) & (r["x"] < 1.15) & (r["y"] > 0.05) & (r["y"] < 1.15)
    err = r["z"][inside] - 0.02 * np.sin(3 * r["x"][inside]) * np.cos(2 * r["y"][inside])
    assert inside.sum() > 0.5 * len(r) and np.sqrt(np.mean(err ** 2)) < 0.008
    pt.close()


def test_stale_class_size_hint_leaves_no_patch_behind(gp):
    """The size-class dispatch sizes its launches from a host-side hint when the batch is the producer's own (matched by the `off`
    pointer and P).  A caller that rewrites `off` IN PLACE keeps pointer and P but not the class sizes (ADVICE round 2 / VERDICT round 3,
    item 9): every hinted launch is followed by an overflow launch that takes whatever the hint missed, so the result is the one the
    host-buffer entry gives on the rewritten batch -- every row written, every status set."""
    import torch
    capi, ctx = gp
    res, sz = 0.15, 12
    m = sz * sz
    side = 0.15 * 12                                  # 144 leaves of ~260 points: all three size classes occur
    xyz, rgb = synth.plane_cloud(int(260 * 144 * 1.02), seed=21, extent=side)
    pt = ctx.project_cloud(ctx.make_cloud(xyz, rgb), res, sz)
    v = pt.view
    b = pt.fetch()
    cnt = np.diff(b["off"])
    assert v.n_max > 256 and (cnt <= 256).sum() > 10 and ((cnt > 256) & (cnt <= 272)).sum() > 10
    p = capi.default_params_dense()
    f = torch.full((v.P, m), float("nan"), dtype=torch.float64, device="cuda")
    st = torch.full((v.P,), -7, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    ctx.dense_fit_predict_grid_dev(p, v.P, v.off, v.n_max, v.n_total, v.x0, v.x1, v.y, 1, res, sz, f, status=st)
    ctx.synchronize()
    assert "dense_mfma_nt16" in ctx.last_dense_kernel()
    f_ref, st_ref = ctx.dense_fit_predict_grid(p, b["off"], b["x0"], b["x1"], b["y"][None, :], res, sz)
    assert np.array_equal(st.cpu().numpy(), st_ref) and np.all(st_ref == 0)
    assert np.max(np.abs(f.cpu().numpy() - f_ref.reshape(v.P, m))) <= 1e-9 * np.max(np.abs(f_ref))
    # the rewrite: same points, same P, another partition -- the small class shrinks to a handful, most patches move up a class
    new_off = np.round(np.arange(v.P + 1) * (v.n_total / v.P)).astype(np.int32)
    for q in (3, 40, 90):                                           # (keep a few small ones so that every class list is non-empty)
        new_off[q] = new_off[q - 1] + 230                           # patch q - 1: 230 points, patch q: ~298
    new_cnt = np.diff(new_off)
    assert new_cnt.min() > 0 and new_cnt.max() <= v.n_max and (new_cnt <= 256).sum() < (cnt <= 256).sum() - 5
    assert ctx.lib.gpc_dev_memcpy(ctx.h, v.off, new_off.ctypes.data, new_off.nbytes, 1) == 0
    f.fill_(float("nan"))
    st.fill_(-7)
    torch.cuda.synchronize()
    ctx.dense_fit_predict_grid_dev(p, v.P, v.off, v.n_max, v.n_total, v.x0, v.x1, v.y, 1, res, sz, f, status=st)
    ctx.synchronize()
    f2_ref, st2_ref = ctx.dense_fit_predict_grid(p, new_off, b["x0"], b["x1"], b["y"][None, :], res, sz)
    got, got_st = f.cpu().numpy(), st.cpu().numpy()
    assert np.all(got_st != -7), f"{int((got_st == -7).sum())} patches were never touched"
    assert np.array_equal(got_st, st2_ref)
    ok = st2_ref == 0
    assert ok.sum() >= 0.9 * v.P and np.all(np.isfinite(got[ok]))
    assert np.max(np.abs(got[ok] - f2_ref.reshape(v.P, m)[ok])) <= 1e-9 * np.max(np.abs(f2_ref.reshape(v.P, m)[ok]))
    pt.close()


def test_producer_full_size_c2(gp, oracle):
    """The cloud behind BASELINE config 2's per-GPU batch: ~2 M points in ~8 k leaves of ~256 points.  Bit-exact against
    the oracle at full size (it takes the CPU a few seconds), plus the size-independent properties."""
    capi, ctx = gp
    res, sz = 0.15, 20
    side = 0.15 * 90                                # 90 x 90 = 8100 leaves on a gently curved ground
    xyz, rgb = synth.plane_cloud(2_100_000, seed=11, extent=side)
    want = oracle.project_cloud(xyz, rgb, res, sz)
    pt = ctx.project_cloud(ctx.make_cloud(xyz, rgb), res, sz)
    v = pt.view
    got = pt.fetch()
    _same(got, want)
    cnt = np.diff(got["off"])
    assert 8000 <= v.P <= 9000 and 200 <= np.median(cnt) <= 300 and v.n_total >= 0.99 * len(xyz)
    assert len(np.unique(got["src"])) == v.n_total
    pt.close()


def test_producer_feeds_the_sparse_gps_on_device(gp, oracle):
    """The reference's own flow (sparse depth GP + sparse colour field per leaf, src/gp_compressor.cpp:146-163, 298-380) on
    the device from end to end: producer view -> gpc_sparse_add_dev (depth and RGB) -> gpc_sparse_predict_dev ->
    gpc_reproject_dev with the colour planes; same cloud as the host-buffer entry points give on the fetched batch."""
    import torch
    capi, ctx = gp
    res, sz = 0.15, 12
    m = sz * sz
    xyz, rgb = synth.plane_cloud(10000, seed=2)
    pt = ctx.project_cloud(ctx.make_cloud(xyz, rgb), res, sz)
    v = pt.view
    b = pt.fetch()
    pd = capi.default_params_sparse(1, sigmaf_sq=1.0, l_sq=(res / 2) ** 2, noise=1e-2, capacity=40)
    pc = capi.default_params_sparse(3, sigmaf_sq=1.0, l_sq=(res / 2) ** 2, noise=25.0, capacity=40)
    xs0, xs1 = synth.grid(res, sz)
    d_xs0, d_xs1 = torch.from_numpy(xs0).cuda(), torch.from_numpy(xs1).cuda()
    f = torch.zeros(v.P, m, dtype=torch.float64, device="cuda")
    c = torch.zeros(v.P, 3, m, dtype=torch.float64, device="cuda")
    bv = torch.zeros(v.P, dtype=torch.int32, device="cuda")
    out = torch.zeros(v.P * m, 32, dtype=torch.uint8, device="cuda")
    npts = torch.zeros(1, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    gd, gc = capi.Sparse(ctx, pd, v.P, 1), capi.Sparse(ctx, pc, v.P, 3)
    gd.add_dev(v.off, v.n_max, v.n_total, v.x0, v.x1, v.y)
    gc.add_dev(v.off, v.n_max, v.n_total, v.x0, v.x1, v.rgb)
    gd.predict_dev(m, d_xs0, d_xs1, f)
    gc.predict_dev(m, d_xs0, d_xs1, c)
    sizes = gd.sizes()
    bv.copy_(torch.from_numpy(sizes))
    torch.cuda.synchronize()
    ctx.reproject_dev(v.P, m, bv, d_xs0, d_xs1, f, c, v.rotations, v.means, v.rgb_means, out, npts)
    ctx.synchronize()
    n_out = int(npts.item())
    assert n_out == int((sizes > 0).sum()) * m and n_out >= 0.9 * v.P * m
    dev_cloud = out[:n_out].cpu().numpy().view(capi.Context.POINT_DTYPE).reshape(-1)
    # the same through host buffers (identity insertion order in both)
    hd, hc = capi.Sparse(ctx, pd, v.P, 1), capi.Sparse(ctx, pc, v.P, 3)
    hd.add(b["off"], b["x0"], b["x1"], b["y"][None, :])
    hc.add(b["off"], b["x0"], b["x1"], b["rgb"])
    fh, _, _ = hd.predict(xs0, xs1, want_sigma=False)
    ch, _, _ = hc.predict(xs0, xs1, want_sigma=False)
    host_cloud = ctx.reproject(xs0, xs1, fh[:, 0, :], b["R"].transpose(0, 2, 1).reshape(v.P, 9), b["mean"], c_star=ch,
                               rgb_means=b["rgb_mean"], bv_count=hd.sizes())
    assert np.array_equal(hd.sizes(), sizes)
    assert np.array_equal(dev_cloud, host_cloud)          # the sparse kernels are deterministic: same records, bit for bit
    # and the surface is the input's
    inside = (dev_cloud["x"] > 0.05) & (dev_cloud["x"] < 1.15) & (dev_cloud["y"] > 0.05) & (dev_cloud["y"] < 1.15)
    err = dev_cloud["z"][inside] - 0.02 * np.sin(3 * dev_cloud["x"][inside]) * np.cos(2 * dev_cloud["y"][inside])
    assert np.sqrt(np.mean(err ** 2)) < 0.004
    for g in (gd, gc, hd, hc):
        g.close()
    pt.close()


def test_device_buffer_helpers(gp):
    """gpc_dev_malloc / gpc_dev_memcpy / gpc_dev_free: what a host built without the HIP toolchain chains the _dev entries with."""
    import ctypes as C
    capi, ctx = gp
    L, h = ctx.lib, ctx.h
    p = C.c_void_p()
    assert L.gpc_dev_malloc(h, 1 << 20, C.byref(p)) == 0 and p.value
    src = np.arange(1 << 17, dtype=np.float64)
    dst = np.zeros_like(src)
    q = C.c_void_p()
    assert L.gpc_dev_malloc(h, 1 << 20, C.byref(q)) == 0
    assert L.gpc_dev_memcpy(h, p, src.ctypes.data, src.nbytes, 1) == 0          # H2D
    assert L.gpc_dev_memcpy(h, q, p, src.nbytes, 3) == 0                        # D2D
    assert L.gpc_dev_memcpy(h, dst.ctypes.data, q, src.nbytes, 2) == 0          # D2H
    assert np.array_equal(src, dst)
    assert L.gpc_dev_memcpy(h, dst.ctypes.data, q, src.nbytes, 7) == capi.GPC_EINVAL
    assert L.gpc_dev_memcpy(h, None, q, 8, 2) == capi.GPC_EINVAL
    assert L.gpc_dev_memcpy(h, None, None, 0, 2) == 0                            # nothing to copy
    assert L.gpc_dev_free(h, p) == 0 and L.gpc_dev_free(h, q) == 0 and L.gpc_dev_free(h, None) == 0
    z = C.c_void_p()
    assert L.gpc_dev_malloc(h, 0, C.byref(z)) == 0 and z.value and L.gpc_dev_free(h, z) == 0
    # partial fetch of a patch batch: NULL outputs are skipped
    xyz, rgb = synth.plane_cloud(5000, seed=3)
    pt = ctx.project_cloud(ctx.make_cloud(xyz, rgb), 0.15, 8)
    off = np.zeros(pt.view.P + 1, np.int32)
    W = np.zeros((pt.view.P, 64), np.uint8)
    assert L.gpc_patches_fetch(pt.h, off.ctypes.data, None, None, None, None, None, None, None, W.ctypes.data, None) == 0
    full = pt.fetch()
    assert np.array_equal(off, full["off"]) and np.array_equal(W, full["W"])
    pt.close()
