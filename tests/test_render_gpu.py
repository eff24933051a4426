"""GPU tests of the renderer (gpc_patches_render, gpc_camera_rays_dev; include/gpc.h) against the NumPy restatement
(tests/render_ref.py, pinned without a GPU by tests/test_render_cpu.py) evaluated on the GPU's own frames (fetch()) and states
(Sparse.state()).  Scenes: tests/render_cases.py on raycast_cases.model_cloud (res 0.25, sz 8, 21 leaves), 405 rays each.

Bounds.  The walk and the frame arithmetic are the restatement's expression for expression, so the voxels a ray visits are equal;
the GP sums differ in the last bits (the library's exp, a fused multiply-add), so
  * leaf and hit / miss are compared EXACTLY, except for rays whose restatement margin is below 1e-6 res, of which a scene may hold
    at most 2 % (asserted here; tests/test_render_cpu.py shows on a hand-made state that the scenes stay within that);
  * range: |t_gpu - t_ref| |g'_ref| <= 2 eps_rel res + df, both solves end with |g| <= eps_rel res;
  * local[0] against Sparse.predict_points at (local[1], local[2]) within df;  xyz == float(R local + mean) exactly;
  * df = 1e-8 of the leaf's largest |f| (over its decompression grid and its hits): the same-state bound tests/test_sparse_gpu.py holds
    the kernel sums to;
  * colour bytes equal rp_flatten of the colour predict_points value + rgb_mean, exactly where that value is further than 1e-6 from an
    integer, within 1 elsewhere.
eps_rel is render_ref.EPS_REL_SCENES in the compared scenes (see there); the defaults run in the entries test."""
import numpy as np
import pytest

import mapping_cases as mc
import mapping_ref as mr
import raycast_cases as rcs
import render_cases as rc
import render_ref as rn

pytestmark = pytest.mark.gpu

RES, SZ = rcs.RES, rcs.SZ
M = SZ * SZ
KW_D = dict(sigmaf_sq=1.0, l_sq=(RES / 5) ** 2, noise=1e-3, capacity=24)      # (as tests/test_raycast_gpu.py)
KW_C = dict(sigmaf_sq=1.0, l_sq=(RES / 5) ** 2, noise=1.0, capacity=100)
PRM = dict(eps_rel=rn.EPS_REL_SCENES)
MIN_NBR = 20


@pytest.fixture(scope="module")
def gp():
    from gp_compressor_amd import capi
    capi.load()
    ctx = capi.Context(0)
    yield capi, ctx
    ctx.close()


def _trained(capi, ctx, xyz, rgb):
    pt = ctx.project_cloud(ctx.make_cloud(xyz, rgb), RES, SZ)
    v = pt.view
    pd, pc = capi.default_params_sparse(1, **KW_D), capi.default_params_sparse(3, **KW_C)
    gd, gc = capi.Sparse(ctx, pd, v.P, 1), capi.Sparse(ctx, pc, v.P, 3)
    gd.add_dev(v.off, v.n_max, v.n_total, v.x0, v.x1, v.y)
    gc.add_dev(v.off, v.n_max, v.n_total, v.x0, v.x1, v.rgb)
    ctx.synchronize()
    return pt, gd, gc, pd, pc


@pytest.fixture(scope="module")
def model(gp):
    """the model cloud cut by the producer, its depth and colour GPs trained on every leaf -- shared, read-only"""
    capi, ctx = gp
    A, ca = rcs.model_cloud()
    pt, gd, gc, pd, pc = _trained(capi, ctx, A, ca)
    assert np.all(gd.sizes() > 0)
    s = dict(pt=pt, gd=gd, gc=gc, pd=pd, pc=pc, g=pt.fetch(), grid=mr.model_grid(A, RES, SZ), P=pt.view.P)
    yield s
    for o in (gd, gc, pt):
        o.close()


def _fmax(s, depth, hits_leaf, hits_f):
    """per leaf the largest |f|: over the decompression grid and over the hits"""
    from gp_compressor_amd import synth
    xs0, xs1 = synth.grid(RES, SZ)
    f, _, _ = depth.predict(xs0, xs1, want_sigma=False)
    fmax = np.max(np.abs(f[:, 0, :]), axis=1)
    np.maximum.at(fmax, hits_leaf, np.abs(hits_f))
    return fmax


def _compare(capi, s, depth, rgb, o, dirs, prm_kw=None, cells=None, entry="host"):
    """renders on the GPU and with the restatement and holds the one to the other as the module docstring says; returns (out, rays)"""
    import torch
    prm_kw = dict(PRM, **(prm_kw or {}))
    prm = capi.default_params_render(**prm_kw)
    pt, g, grid = s["pt"], s["g"], s["grid"]
    if entry == "host":
        out = pt.render(o, dirs, depth, rgb, cells, prm)
        cloud = out["cloud"]
    else:
        d_cells = None if cells is None else torch.from_numpy(cells).cuda()
        out = pt.render(o, torch.from_numpy(dirs).cuda(), depth, rgb, d_cells, prm)
        cloud = out["cloud"].cpu().numpy().view(capi.Context.POINT_DTYPE).reshape(-1)
        out = {k: (v.cpu().numpy() if hasattr(v, "cpu") else v) for k, v in out.items()}
    dgp = rn.gp_of(s["pd"], depth.sizes(), depth.state())
    cgp = None if rgb is None else rn.gp_of(s["pc"], rgb.sizes(), rgb.state())
    rays = rn.render(g, grid, dgp, o, dirs, prm_kw, cells, cgp)
    n = len(dirs)
    leaf, rng_, loc, counts = out["leaf"], out["range"], out["local"], out["counts"]
    ref_leaf = np.array([r["leaf"] for r in rays])
    low = np.array([r["margin"] < 1e-6 * RES for r in rays])
    print("rays", n, "GPU hits", int(np.sum(leaf >= 0)), "restatement hits", int(np.sum(ref_leaf >= 0)), "margin below 1e-6 res", int(low.sum()),
          "leaves that differ", int(np.sum(leaf != ref_leaf)), "counts", counts.tolist(), "restatement", rn.counts_of(rays).tolist())
    assert low.sum() <= 0.02 * n
    assert np.array_equal(leaf[~low], ref_leaf[~low])
    # misses
    miss = leaf < 0
    for k in "xyz":
        assert np.all(np.isnan(cloud[k][miss]))
    assert np.all(np.isnan(rng_[miss])) and np.all(np.isnan(loc[miss]))
    assert np.all(cloud["w"] == 1.0) and np.all(cloud["a"] == 255) and np.all(cloud["pad"] == 0.0)
    assert not cloud["r"][miss].any() and not cloud["g"][miss].any() and not cloud["b"][miss].any()
    # hits
    hit = np.flatnonzero(~miss)
    L = leaf[hit]
    assert np.all(np.isfinite(rng_[hit])) and np.all(np.isfinite(loc[hit]))
    fmax = _fmax(s, depth, L, loc[hit, 0])
    df = 1e-8 * fmax
    tol = prm_kw["eps_rel"] * RES
    worst_t = worst_f = 0.0
    for i in hit:
        if low[i] or ref_leaf[i] != leaf[i]:
            continue
        r = rays[i]
        err = abs(rng_[i] - r["t"]) * abs(r["gprime"])
        worst_t = max(worst_t, err / (2 * tol + df[leaf[i]]))
        assert err <= 2 * tol + df[leaf[i]], (i, rng_[i], r["t"], r["gprime"])
    # the depth at the hit against the library's own prediction there, bucketed by leaf
    order = hit[np.argsort(L, kind="stable")]
    off = np.concatenate([[0], np.cumsum(np.bincount(L, minlength=s["P"]))]).astype(np.int32)
    q1, q2 = np.ascontiguousarray(loc[order, 1]), np.ascontiguousarray(loc[order, 2])
    fp, _, _ = depth.predict_points(off, q1, q2)
    if len(order):
        worst_f = float(np.max(np.abs(loc[order, 0] - fp[0]) / np.maximum(df[leaf[order]], 1e-300)))
        assert np.all(np.abs(loc[order, 0] - fp[0]) <= df[leaf[order]])
    print("range error / bound", worst_t, "local[0] - predict_points / df", worst_f)
    # xyz = float(R local + mean), in gpc_reproject's association
    R, mu = g["R"][L], g["mean"][L]
    for a, k in enumerate("xyz"):
        want = (((R[:, a, 0] * loc[hit, 0] + R[:, a, 1] * loc[hit, 1]) + R[:, a, 2] * loc[hit, 2]) + mu[:, a]).astype(np.float32)
        assert cloud[k][hit].tobytes() == want.tobytes()
    # colours
    if rgb is None:
        assert not cloud["r"].any() and not cloud["g"].any() and not cloud["b"].any()
    else:
        cpred, _, _ = rgb.predict_points(off, q1, q2)
        exact = 0
        for c, k in enumerate("rgb"):
            val = cpred[c] + g["rgb_mean"][leaf[order], c]
            want = np.array([rn.flatten(v) for v in val])
            got = cloud[k][order].astype(np.int64)
            near = np.abs(val - np.rint(val)) <= 1e-6
            assert np.array_equal(got[~near], want[~near]) and np.all(np.abs(got - want) <= 1)
            exact += int(np.sum(~near))
        assert exact > 0 or len(order) == 0
    # counts
    ref_counts = rn.counts_of(rays)
    assert counts[0] == n == ref_counts[0] and counts[2] == ref_counts[2]
    assert counts[1] == np.sum(leaf >= 0) and np.sum(leaf[~low] >= 0) == np.sum(ref_leaf[~low] >= 0)
    if not low.any():
        assert np.array_equal(counts, ref_counts)
    return out, rays


@pytest.mark.parametrize("pose", list(rc.POSES))
def test_trained_model_small_images(gp, model, pose):
    capi, ctx = gp
    s = model
    o, dirs = rc.scene_rays(pose, s["g"]["R"][4][:, 1])
    # the pinhole rays are the device's: gpc_camera_rays_dev against its restatement, bit for bit
    _, Rc, f = rc.POSES[pose]
    img = ctx.camera_rays(Rc, f, f, (rc.W_IMG - 1) / 2, (rc.H_IMG - 1) / 2, rc.W_IMG, rc.H_IMG).cpu().numpy()
    one = ctx.camera_rays(Rc, f, f, 0.0, 0.0, 1, 1).cpu().numpy()
    n_img = rc.W_IMG * rc.H_IMG
    assert img.tobytes() == dirs[:n_img].tobytes() and one.tobytes() == dirs[n_img:n_img + 1].tobytes()
    assert ctx.camera_rays(Rc, f, f, 0.0, 0.0, 0, 5).shape == (0, 3)
    out, rays = _compare(capi, s, s["gd"], s["gc"], o, dirs)
    t = rc.holds_every_case(rays, s["grid"])
    assert s["P"] == 21 and t["rays"] == 405 and t["misses"] > 50 and t["outside"] >= 3 and t["non_leaf"] > 5 and t["long"] > 5
    assert t["rejected_then_hit"] > 5
    assert (t["upper"] > 100) if pose == "above" else (t["lower"] > 100)
    # the image is organised: the 1 x 1 image's pixel is the optical axis, whose range is the depth along it
    i = n_img
    assert out["leaf"][i] >= 0 and abs(out["range"][i] - np.dot(np.array([out["cloud"][k][i] for k in "xyz"], dtype=np.float64) - o, Rc[:, 2])) < 1e-6


def test_both_layers_are_hit_over_the_two_poses(model):
    """(on the restatement alone, with the GPU's frames and states: the scenes together hold hits on both layers)"""
    s = model
    dgp = rn.gp_of(s["pd"], s["gd"].sizes(), s["gd"].state())
    tallies = [rc.holds_every_case(rn.render(s["g"], s["grid"], dgp, *rc.scene_rays(p, s["g"]["R"][4][:, 1]), PRM), s["grid"]) for p in rc.POSES]
    assert sum(t["upper"] for t in tallies) > 100 and sum(t["lower"] for t in tallies) > 100


def _handmade(capi, ctx, s, rng, b_of_leaf, ny=1, amp=0.01):
    kw = dict(KW_D if ny == 1 else KW_C, capacity=100)
    prm = capi.default_params_sparse(ny, **kw)
    gs = capi.Sparse(ctx, prm, s["P"], ny)
    b, alpha, BV = rc.handmade_state(rng, s["P"], np.minimum(b_of_leaf, gs.ld()), gs.ld(), ny, amp)
    gs.set_state(b, alpha, BV)
    return gs, prm


@pytest.mark.parametrize("pose", list(rc.POSES))
def test_handmade_states_of_every_basis_size(gp, model, pose):
    """one leaf each (and more) with b = 1, 16, 17, 32, 33, 64, 65 and the capacity, random weights, basis vectors inside the window:
    any chunking of the basis loop shows"""
    capi, ctx = gp
    s = model
    sizes = np.array([1, 16, 17, 32, 33, 64, 65, 100])
    gs, prm = _handmade(capi, ctx, s, np.random.default_rng(31), sizes[np.arange(s["P"]) % len(sizes)])
    assert gs.ld() == 112 and set(gs.sizes()) == set(sizes)
    o, dirs = rc.scene_rays(pose, s["g"]["R"][4][:, 1])
    out, rays = _compare(capi, dict(s, pd=prm), gs, None, o, dirs, entry="device")
    hit_sizes = set(gs.sizes()[out["leaf"][out["leaf"] >= 0]])
    assert len(hit_sizes) >= 6 and sum(r["leaf"] >= 0 for r in rays) > 100
    gs.close()


def test_untrained_leaves_are_walked_through(gp, model):
    capi, ctx = gp
    s = model
    z = (s["grid"]["vox"] - s["grid"]["koff"])[:, 2]
    gs, prm = _handmade(capi, ctx, s, np.random.default_rng(32), np.where(z >= 2, 0, 8))
    o, dirs = rc.scene_rays("above", s["g"]["R"][4][:, 1])
    out, rays = _compare(capi, dict(s, pd=prm), gs, None, o, dirs)
    hit = out["leaf"][out["leaf"] >= 0]
    assert len(hit) > 50 and np.all(z[hit] == 0)
    assert all(z[t["leaf"]] == 0 for r in rays for t in r["tests"]) and max(len(r["visited"]) for r in rays) >= 4
    gs.close()


def test_masks_w_and_cells(gp):
    """a map whose upper leaves in the middle column hold points on half their window only: rays into the empty half pass to the lower
    layer with use_w = 1 and stop with 0; FREE cells of a label buffer send rays on, OCCUPIED and UNOBSERVED ones do not"""
    capi, ctx = gp
    A, ca = rcs.model_cloud()
    keep = ~((A[:, 2] > 0.0) & (A[:, 0] > 0.375) & (A[:, 0] < 0.5))
    keep[0] = True
    pt, gd, gc, pd, pc = _trained(capi, ctx, A[keep], ca[keep])
    s = dict(pt=pt, gd=gd, gc=gc, pd=pd, pc=pc, g=pt.fetch(), grid=mr.model_grid(A[keep], RES, SZ), P=pt.view.P)
    z = (s["grid"]["vox"] - s["grid"]["koff"])[:, 2]
    rng = np.random.default_rng(33)
    tgt = np.stack([rng.uniform(0.40, 0.48, 60), rng.uniform(0.05, 0.7, 60), np.full(60, 0.2)], 1)
    dirs = np.concatenate([tgt - rcs.SENSOR, rc.scene_rays("above", s["g"]["R"][4][:, 1])[1]])
    with_w, rays_w = _compare(capi, s, gd, gc, rcs.SENSOR, dirs)
    without, rays_0 = _compare(capi, s, gd, gc, rcs.SENSOR, dirs, dict(use_w=0))
    lw, l0 = with_w["leaf"][:60], without["leaf"][:60]
    assert np.sum((lw >= 0) & (z[np.maximum(lw, 0)] == 0)) > 25 and np.sum((l0 >= 0) & (z[np.maximum(l0, 0)] >= 2)) > 40
    # labels: a third of the upper layer's hits FREE, a third OCCUPIED, the rest UNOBSERVED
    cells = np.zeros((s["P"], M), np.uint8)
    upper = [i for i, r in enumerate(rays_w) if r["leaf"] >= 0 and z[r["leaf"]] >= 2]
    assert len(upper) > 100
    for j, i in enumerate(upper):
        L, cell = rays_w[i]["leaf"], rays_w[i]["tests"][-1]["cell"]
        if j % 3 == 0:
            cells[L, cell] = capi.CELL_FREE
        elif j % 3 == 1 and cells[L, cell] == 0:
            cells[L, cell] = capi.CELL_OCCUPIED
    labelled, rays_c = _compare(capi, s, gd, gc, rcs.SENSOR, dirs, None, cells)
    went_on = 0
    for i in upper:
        L, cell = rays_w[i]["leaf"], rays_w[i]["tests"][-1]["cell"]
        if rays_w[i]["margin"] < 1e-6 * RES or rays_c[i]["margin"] < 1e-6 * RES:
            continue
        if cells[L, cell] == capi.CELL_FREE:
            assert labelled["leaf"][i] != L
            went_on += labelled["leaf"][i] >= 0 and z[labelled["leaf"][i]] == 0
        else:
            assert labelled["leaf"][i] == L
    assert went_on > 10
    for o in (gd, gc, pt):
        o.close()


def test_colour_of_an_empty_basis_is_the_mean_colour(gp, model):
    capi, ctx = gp
    s = model
    odd = np.arange(s["P"]) % 2 == 1
    gs, prm = _handmade(capi, ctx, s, np.random.default_rng(34), np.where(odd, 0, 20), ny=3, amp=30.0)
    o, dirs = rc.scene_rays("above", s["g"]["R"][4][:, 1])
    out, rays = _compare(capi, dict(s, pc=prm), s["gd"], gs, o, dirs)
    leaf, cloud = out["leaf"], out["cloud"]
    sel = (leaf >= 0) & odd[np.maximum(leaf, 0)]
    assert sel.sum() > 30 and np.sum((leaf >= 0) & ~sel) > 30
    for c, k in enumerate("rgb"):
        assert np.array_equal(cloud[k][sel], [rn.flatten(v) for v in s["g"]["rgb_mean"][leaf[sel], c]])
    assert len(np.unique(cloud["r"][(leaf >= 0) & ~sel])) > 10
    gs.close()


def _look_at(o, target):
    zc = (target - o) / np.linalg.norm(target - o)
    xc = np.cross([0.0, 0.0, 1.0], zc)
    xc /= np.linalg.norm(xc)
    return np.stack([xc, np.cross(zc, xc), zc], 1)


def test_grown_map_through_mapping_render(gp, monkeypatch):
    """capi.Mapping.add_cloud with a scan below the model's corner on every axis (koff > 0 on all three), then Mapping.render with and
    without the occupancy labels.  The registered cloud is recorded at the binding, as tests/test_raycast_gpu.py does."""
    capi, ctx = gp
    A, ca = mc.model_cloud()
    pt0, gd0, gc0, pd, pc = _trained(capi, ctx, A, ca)
    rec = {}
    inner = capi.Patches.raycast

    def recording(self, cloud, origin, cells, depth=None, n=None):
        host = np.zeros(n, dtype=capi.Context.POINT_DTYPE)
        ctx._check(ctx.lib.gpc_dev_memcpy(ctx.h, host.ctypes.data, cloud, host.nbytes, 2))
        rec.update(xyz=np.stack([host["x"], host["y"], host["z"]], 1), rgb=np.stack([host["r"], host["g"], host["b"]], 1), g=self.fetch())
        return inner(self, cloud, origin, cells, depth=depth, n=n)
    monkeypatch.setattr(capi.Patches, "raycast", recording)
    model, grid0, trained0 = pt0.fetch(), mr.model_grid(A, RES, SZ), gd0.sizes() > 0
    mp = capi.Mapping(ctx, pt0, gd0, gc0, params=capi.default_params_registration(step=1e-7, tol=1e300, min_steps=2, max_steps=10),
                      min_nbr=MIN_NBR)
    B, cb = mc.disjoint_scan("below")
    steps, inserted = mp.add_cloud(ctx.make_cloud(B, cb))
    assert inserted
    want = mr.insert(model, grid0, trained0, rec["xyz"], rec["rgb"], MIN_NBR, frames=rec["g"]["R"])
    grid = want["grid"]
    assert np.all(grid["koff"] > 0) and mp.patches.view.P == len(want["cls"]) == 11 and np.all(mp.depth.sizes() > 0)
    s = dict(pt=mp.patches, pd=pd, pc=pc, g=mp.patches.fetch(), grid=grid, P=mp.patches.view.P)
    o = np.array([0.4, 0.4, 1.0])
    dirs = np.concatenate([rn.camera_rays(rc.LOOK_DOWN, 14.0, 14.0, 11.0, 8.0, 23, 17),
                           rn.camera_rays(_look_at(o, np.array([-0.75, -0.625, -0.6])), 60.0, 60.0, 11.0, 8.0, 23, 17)])
    # (the scan's own leaves were untrained when its rays were cast, so it labelled nothing; a later scan would.  Labels by hand:)
    mp.cells[:, ::4] = capi.CELL_FREE
    cells = mp.cells.cpu().numpy()
    leaves_seen = []
    for use_cells in (True, False):
        out, rays = _compare(capi, s, mp.depth, mp.rgb, o, dirs, None, cells if use_cells else None)
        via = mp.render(o, __import__("torch").from_numpy(dirs).cuda(), capi.default_params_render(**PRM), use_cells=use_cells)
        assert np.array_equal(via["leaf"].cpu().numpy(), out["leaf"]) and via["cloud"].cpu().numpy().tobytes() == out["cloud"].tobytes()
        new = want["cls"][np.maximum(out["leaf"], 0)] == mr.FRESH
        assert np.sum((out["leaf"] >= 0) & new) > 20 and np.sum((out["leaf"] >= 0) & ~new) > 50
        assert max(len(r["visited"]) for r in rays) >= 8                     # long walks through the deep grid
        leaves_seen.append(out["leaf"])
    assert np.sum(leaves_seen[0] != leaves_seen[1]) > 20                     # the labels are read
    mp.close()


def test_entries_give_the_same_bytes(gp, model):
    """host entry = device entry = device entry again, at the default parameters, all outputs; outputs not asked for are not needed"""
    import torch
    capi, ctx = gp
    s = model
    o, dirs = rc.scene_rays("inside", s["g"]["R"][4][:, 1])
    cells = np.random.default_rng(35).integers(0, 3, (s["P"], M)).astype(np.uint8)
    host = s["pt"].render(o, dirs, s["gd"], s["gc"], cells)
    assert host["counts"][1] > 50 and host["counts"][0] == len(dirs)
    d_dirs, d_cells = torch.from_numpy(dirs).cuda(), torch.from_numpy(cells).cuda()
    for _ in range(2):
        dev = s["pt"].render(o, d_dirs, s["gd"], s["gc"], d_cells)
        assert np.array_equal(dev["counts"], host["counts"])
        assert dev["cloud"].cpu().numpy().tobytes() == host["cloud"].tobytes()
        for k in ("leaf", "range", "local"):
            assert dev[k].cpu().numpy().tobytes() == host[k].tobytes()
    only = s["pt"].render(o, dirs, s["gd"], s["gc"], cells, want=())
    assert set(only) == {"cloud", "counts"} and only["cloud"].tobytes() == host["cloud"].tobytes()
    # without the colour GP: the same geometry, colours 0
    plain = s["pt"].render(o, dirs, s["gd"], None, cells)
    assert np.array_equal(plain["leaf"], host["leaf"]) and not plain["cloud"]["r"].any() and host["cloud"]["r"].any()


def test_render_contract(gp, model):
    import torch
    capi, ctx = gp
    s = model
    L = ctx.lib
    pt, gd, gc = s["pt"], s["gd"], s["gc"]
    o, dirs = rc.scene_rays("above", s["g"]["R"][4][:, 1])
    dirs = np.ascontiguousarray(dirs[:40])
    n = len(dirs)
    cloud = np.zeros(n, dtype=capi.Context.POINT_DTYPE)
    counts = np.full(5, -1, np.int32)
    prm = capi.default_params_render()

    def call(c, m, d, r, p, org, dr, k, cl, entry=L.gpc_patches_render):
        import ctypes as C
        return entry(c, m, d, r, None, C.byref(p) if p is not None else None, org.ctypes.data if org is not None else None,
                     dr.ctypes.data if dr is not None else None, k, cl.ctypes.data if cl is not None else None, None, None, None,
                     counts.ctypes.data)
    assert call(ctx.h, pt.h, gd.h, gc.h, prm, o, dirs, n, cloud) == capi.GPC_OK and counts[0] == n and counts[1] > 0
    assert call(ctx.h, pt.h, gd.h, gc.h, None, o, dirs, n, cloud) == capi.GPC_OK              # params NULL: the defaults
    # n == 0
    assert call(ctx.h, pt.h, gd.h, gc.h, prm, o, None, 0, None) == capi.GPC_OK and counts.tolist() == [0, 0, 0, 0, 0]
    # a non-finite origin, newton_iters < 0
    for bad in (np.nan, np.inf):
        o2 = o.copy()
        o2[2] = bad
        assert call(ctx.h, pt.h, gd.h, gc.h, prm, o2, dirs, n, cloud) == capi.GPC_EINVAL
    assert call(ctx.h, pt.h, gd.h, gc.h, capi.default_params_render(newton_iters=-1), o, dirs, n, cloud) == capi.GPC_EINVAL
    assert call(ctx.h, pt.h, gd.h, gc.h, capi.default_params_render(newton_iters=0), o, dirs, n, cloud) == capi.GPC_OK
    # depth / rgb with another P or ny
    P = s["P"]
    for wrongP, ny in ((P + 1, 1), (P, 3)):
        wrong = capi.Sparse(ctx, capi.default_params_sparse(ny, **KW_D), wrongP, ny)
        assert call(ctx.h, pt.h, wrong.h, gc.h, prm, o, dirs, n, cloud) == capi.GPC_EINVAL
        wrong.close()
    for wrongP, ny in ((P + 1, 3), (P, 1)):
        wrong = capi.Sparse(ctx, capi.default_params_sparse(ny, **KW_D), wrongP, ny)
        assert call(ctx.h, pt.h, gd.h, wrong.h, prm, o, dirs, n, cloud) == capi.GPC_EINVAL
        wrong.close()
    # a destroyed object (its address is no longer in the context's list), objects of another context, missing arguments
    gone = capi.Sparse(ctx, capi.default_params_sparse(1, **KW_D), P, 1)
    h_gone = gone.h
    gone.close()
    assert call(ctx.h, pt.h, h_gone, gc.h, prm, o, dirs, n, cloud) == capi.GPC_EINVAL
    ctx2 = capi.Context(0)
    other = capi.Sparse(ctx2, capi.default_params_sparse(1, **KW_D), P, 1)
    assert call(ctx.h, pt.h, other.h, gc.h, prm, o, dirs, n, cloud) == capi.GPC_EINVAL
    assert call(ctx2.h, pt.h, other.h, None, prm, o, dirs, n, cloud) == capi.GPC_EINVAL
    other.close()
    ctx2.close()
    assert call(ctx.h, None, gd.h, gc.h, prm, o, dirs, n, cloud) == capi.GPC_EINVAL
    assert call(ctx.h, pt.h, None, gc.h, prm, o, dirs, n, cloud) == capi.GPC_EINVAL
    assert call(ctx.h, pt.h, gd.h, gc.h, prm, None, dirs, n, cloud) == capi.GPC_EINVAL
    assert call(ctx.h, pt.h, gd.h, gc.h, prm, o, None, n, cloud) == capi.GPC_EINVAL
    assert call(ctx.h, pt.h, gd.h, gc.h, prm, o, dirs, n, None) == capi.GPC_EINVAL
    assert call(ctx.h, pt.h, gd.h, gc.h, prm, o, dirs, -1, cloud) == capi.GPC_EINVAL
    # the device entry refuses the same; with counts == NULL it is asynchronous and complete after a synchronize
    d_dirs = torch.from_numpy(dirs).cuda()
    d_cloud = torch.zeros((n, 32), dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    bad = o.copy()
    bad[0] = np.nan
    dev = L.gpc_patches_render_dev
    import ctypes as C
    assert dev(ctx.h, pt.h, gd.h, gc.h, None, C.byref(prm), bad.ctypes.data, d_dirs.data_ptr(), n, d_cloud.data_ptr(), None, None, None,
               None) == capi.GPC_EINVAL
    assert dev(ctx.h, pt.h, gd.h, gc.h, None, C.byref(prm), o.ctypes.data, d_dirs.data_ptr(), n, d_cloud.data_ptr(), None, None, None,
               None) == capi.GPC_OK
    ctx.synchronize()
    assert call(ctx.h, pt.h, gd.h, gc.h, prm, o, dirs, n, cloud) == capi.GPC_OK              # (cloud last held the newton_iters = 0 image)
    assert d_cloud.cpu().numpy().tobytes() == cloud.tobytes() and counts[1] > 0
    # the camera: sizes and intrinsics
    Rc = np.ascontiguousarray(np.eye(3))
    cam = L.gpc_camera_rays_dev
    assert cam(ctx.h, Rc.ctypes.data, 1.0, 1.0, 0.0, 0.0, -1, 2, d_dirs.data_ptr()) == capi.GPC_EINVAL
    assert cam(ctx.h, Rc.ctypes.data, 0.0, 1.0, 0.0, 0.0, 2, 2, d_dirs.data_ptr()) == capi.GPC_EINVAL
    assert cam(ctx.h, Rc.ctypes.data, 1.0, np.nan, 0.0, 0.0, 2, 2, d_dirs.data_ptr()) == capi.GPC_EINVAL
    assert cam(ctx.h, Rc.ctypes.data, 1.0, 1.0, 0.0, 0.0, 2, 2, None) == capi.GPC_EINVAL
    assert cam(ctx.h, Rc.ctypes.data, 1.0, 1.0, 0.0, 0.0, 65536, 65536, d_dirs.data_ptr()) == capi.GPC_ERANGE
    assert cam(ctx.h, Rc.ctypes.data, 1.0, 1.0, 0.0, 0.0, 0, 7, None) == capi.GPC_OK
