"""Rate control to a byte budget through the host class and the map: gp_compressor::model_bytes / prune_to_bytes on the plane cloud of
tests/test_quantize_host_gpu.py, and capi.Mapping.prune_to_bytes on the smallest two-scan map of tests/mapping_cases.py."""
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def H():
    from gp_compressor_amd import host_api
    host_api.build()
    return host_api


def _make(H, xyz, rgb, res, sz, model="sparse"):
    g = H.GpCompressor(xyz, rgb, res=res, sz=sz, model=model, seed=7)
    if model == "sparse":
        # (capacity 100 and the colour field deleting as its derivation says: tests/test_prune_rd_host_gpu.py)
        g.set_sparse_kernel(1.0, (res / 4) ** 2, 1e-2, 25.0, 100)
        g.set_field_delete_bug(0)
    return g


def test_host_prune_to_bytes(H, tmp_path):
    res, sz = 0.15, 10
    xyz, rgb = H.synthetic_plane_cloud(2500, seed=1, extent=0.45)
    g = _make(H, xyz, rgb, res, sz)
    with pytest.raises(RuntimeError):
        g.model_bytes()                                                # not trained yet
    full, small = str(tmp_path / "full.gpcm"), str(tmp_path / "small.gpcm")
    n_full = g.save_model(full)                                        # trains
    P = g.L.gpc_host_patch_count(g.h)
    assert P > 4 and n_full == os.path.getsize(full) == g.model_bytes()
    import quantize_ref as qr
    v1 = qr.parse_model(open(full, "rb").read())
    sizes = [np.array([p["gps"][k]["b"] for p in v1["patches"]]) for k in range(2)]          # basis counts, depth and colour
    assert qr.file_bytes(v1) == n_full
    # an infeasible budget throws, names the floor, and leaves the object as it was
    with pytest.raises(RuntimeError, match="floor of [0-9]+ bytes"):
        g.prune_to_bytes(100)
    assert g.model_bytes() == n_full
    again = str(tmp_path / "again.gpcm")
    assert g.save_model(again) == n_full and open(again, "rb").read() == open(full, "rb").read()
    # 60 % of the size
    budget = (6 * n_full) // 10
    rm_d, rm_c = g.prune_to_bytes(budget)
    n_small = g.save_model(small)
    print(f"{P} leaves: {n_full} -> {n_small} bytes (budget {budget}); removed depth {rm_d}, colour {rm_c}")
    assert n_small <= budget and n_small == g.model_bytes() == os.path.getsize(small)
    assert n_full - n_small == 24 * rm_d + 40 * rm_c and rm_d + rm_c > 0
    # the file loads
    cap = P * sz * sz
    xyz1, rgb1 = H.decompress_file(small, cap)
    xyz0, rgb0 = g.load_compressed()
    assert len(xyz1) > 0 and np.array_equal(xyz1.view(np.uint32), xyz0.view(np.uint32)) and np.array_equal(rgb1, rgb0)
    # a budget the model already meets: nothing that raises an error is removed, and the size can only fall
    g.prune_to_bytes(n_small + 1000)
    assert g.model_bytes() <= n_small
    # the floor itself is reachable: every GP at one vector
    g.prune(1, 1)
    floor = g.model_bytes()
    assert floor == n_full - 24 * int(np.sum(sizes[0] - 1)) - 40 * int(np.sum(sizes[1] - 1))
    h = _make(H, xyz, rgb, res, sz)
    h.prune_to_bytes(floor)
    assert h.model_bytes() == floor
    with pytest.raises(RuntimeError, match=f"floor of {floor} bytes"):
        _make(H, xyz, rgb, res, sz).prune_to_bytes(floor - 1)
    # the exceptions of prune_to_error: the dense model, the multi-device flow
    with pytest.raises(RuntimeError):
        _make(H, xyz, rgb, res, sz, model="dense").prune_to_bytes(budget)
    m = _make(H, xyz, rgb, res, sz)
    m.set_devices([0])
    with pytest.raises(RuntimeError):
        m.prune_to_bytes(budget)
    with pytest.raises(RuntimeError):
        g.prune_to_bytes(budget, w_depth=-1.0)


def test_mapping_prune_to_bytes():
    """The 3 x 3 model and the disjoint two-voxel scan: the nine old leaves have no points in the last scan and keep every bit; the two new
    leaves give up what the budget asks, over both GPs at once."""
    import mapping_cases as mc
    from gp_compressor_amd import capi
    capi.load()
    ctx = capi.Context(0)
    RES, SZ = mc.RES, mc.SZ
    kw_d = dict(sigmaf_sq=1.0, l_sq=(RES / 5) ** 2, noise=1e-3, capacity=24)
    kw_c = dict(sigmaf_sq=1.0, l_sq=(RES / 5) ** 2, noise=1.0, capacity=100, ref_field_delete_bug=0)
    A, ca = mc.model_cloud()
    B, cb = mc.disjoint_scan("above")
    pt = ctx.project_cloud(ctx.make_cloud(A, ca), RES, SZ)
    a = pt.fetch()
    P0 = pt.view.P
    gd = capi.Sparse(ctx, capi.default_params_sparse(1, **kw_d), P0, 1)
    gc = capi.Sparse(ctx, capi.default_params_sparse(3, **kw_c), P0, 3)
    assert np.all(gd.add(a["off"], a["x0"], a["x1"], a["y"][None, :]) == 0)
    assert np.all(gc.add(a["off"], a["x0"], a["x1"], np.ascontiguousarray(a["rgb"])) == 0)
    pt2, o2n = pt.insert_cloud(ctx.make_cloud(B, cb), min_nbr=1)
    v = pt2.view
    gd2, gc2 = gd.remap(v.P, o2n), gc.remap(v.P, o2n)
    gd2.add_dev(v.off, v.n_max, v.n_total, v.x0, v.x1, v.y)
    gc2.add_dev(v.off, v.n_max, v.n_total, v.x0, v.x1, v.rgb)
    ctx.synchronize()
    for o_ in (gd, gc, pt):
        o_.close()
    new = np.flatnonzero(np.diff(pt2.fetch()["off"]) > 0)
    mp = capi.Mapping(ctx, pt2, gd2, gc2)
    bd, bc = mp.depth.sizes(), mp.rgb.sizes()
    state = lambda g: (g.sizes(),) + tuple(g.state())
    before = (state(mp.depth), state(mp.rgb))
    most = 24 * int(np.sum(bd[new] - 1)) + 40 * int(np.sum(bc[new] - 1))
    need = most // 2
    kd, kc, res = mp.prune_to_bytes(need)
    print(f"map: need {need} of {most}: depth {bd[new]} - {kd[new]}, colour {bc[new]} - {kc[new]}, saved {res['saved']}, lambda {res['lambda']:.3e}")
    assert res["feasible"] == 1 and res["max_saving"] == most and need <= res["saved"] == 24 * int(kd.sum()) + 40 * int(kc.sum())
    assert np.array_equal(mp.depth.sizes(), bd - kd) and np.array_equal(mp.rgb.sizes(), bc - kc)
    assert np.all(kd[o2n] == 0) and np.all(kc[o2n] == 0)
    for b4, af in zip(before, (state(mp.depth), state(mp.rgb))):
        for x, y_ in zip(b4, af):
            assert np.array_equal(x[o2n], y_[o2n], equal_nan=True)
    # what the map cannot give: the allocation goes as far as it can and says so
    kd2, kc2, res2 = mp.prune_to_bytes(most)
    assert res2["feasible"] == 0 and np.all(mp.depth.sizes()[new] == 1) and np.all(mp.rgb.sizes()[new] == 1)
    assert np.array_equal(mp.depth.sizes()[o2n], bd[o2n]) and np.array_equal(mp.rgb.sizes()[o2n], bc[o2n])
    mp.close()
    ctx.close()
