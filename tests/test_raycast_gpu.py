"""GPU tests of the ray cast (gp_mapping::train_classification, src/gp_mapping.cpp:154-211): gpc_patches_raycast and
gpc_occupancy_batch_dev against the NumPy restatement (tests/raycast_ref.py, pinned without a GPU by tests/test_raycast_cpu.py)
evaluated on the GPU's own frames and owners, the carry of the cells through capi.Mapping, the probit GP on the labelled batch against
the oracle's IRLS fit, and the contract.

Bounds: cells, counts and the occupancy batch are compared exactly -- the kernels evaluate the restatement's expressions in its
association with contraction off, and the writes are integer atomics.  The IRLS fit carries the bound of tests/test_probit_gpu.py
(1e-8 of a patch's max-norm; the patches here have at most 64 points).  Scene: tests/raycast_cases.py (res 0.25, sz 8)."""
import ctypes as C

import numpy as np
import pytest

import mapping_ref as mr
import raycast_cases as rcs
import raycast_ref as rr

pytestmark = pytest.mark.gpu

RES, SZ = rcs.RES, rcs.SZ
M = SZ * SZ
KW_D = dict(sigmaf_sq=1.0, l_sq=(RES / 5) ** 2, noise=1e-3, capacity=24)
KW_C = dict(sigmaf_sq=1.0, l_sq=(RES / 5) ** 2, noise=1.0, capacity=100)       # (as tests/test_mapping_gpu.py: KW_C_REG)
MIN_NBR = 20


@pytest.fixture(scope="module")
def gp():
    from gp_compressor_amd import capi
    capi.load()
    ctx = capi.Context(0)
    yield capi, ctx
    ctx.close()


# a dyadic point near the sensor: moving every cloud by it puts the sensor at the origin (where a scan's own frame has it, and where
# the registration of capi.Mapping starts) and keeps the model's corner dyadic
SENSOR_D = np.array([0.3125, 0.4375, 1.3125])


def _moved(xyz):
    return (xyz.astype(np.float64) - SENSOR_D).astype(np.float32)


def _model(capi, ctx, colour=False, moved=False):
    """the model cloud cut by the producer, its depth (and colour) GPs trained on every leaf"""
    A, ca = rcs.model_cloud()
    if moved:
        A = _moved(A)
        assert np.array_equal(A[0].astype(np.float64), np.asarray(rcs.CORNER) - SENSOR_D) and np.all(A >= A[0])
    pt = ctx.project_cloud(ctx.make_cloud(A, ca), RES, SZ)
    v = pt.view
    gd = capi.Sparse(ctx, capi.default_params_sparse(1, **KW_D), v.P, 1)
    gd.add_dev(v.off, v.n_max, v.n_total, v.x0, v.x1, v.y)
    gc = None
    if colour:
        gc = capi.Sparse(ctx, capi.default_params_sparse(3, **KW_C), v.P, 3)
        gc.add_dev(v.off, v.n_max, v.n_total, v.x0, v.x1, v.rgb)
    ctx.synchronize()
    assert np.all(gd.sizes() > 0)
    return A, pt, gd, gc


@pytest.fixture(scope="module")
def scene(gp):
    """the scan inserted into the model, the depth GP remapped but not yet trained on it (where train_classification runs), and the
    restatement on the GPU's own frames and owners -- shared, read-only"""
    capi, ctx = gp
    A, pt0, gd0, _ = _model(capi, ctx)
    S, cs = rcs.scan_cloud()
    scan = ctx.make_cloud(S, cs)
    new, o2n = pt0.insert_cloud(scan, min_nbr=MIN_NBR, depth=gd0)
    g = new.fetch()
    want = mr.insert(pt0.fetch(), mr.model_grid(A, RES, SZ), gd0.sizes() > 0, S, cs, MIN_NBR, frames=g["R"])
    assert np.array_equal(g["off"], want["off"]) and np.array_equal(g["src"], want["src"]) and np.array_equal(o2n, want["old_to_new"])
    gd = gd0.remap(new.view.P, o2n)
    trained = gd.sizes() > 0
    ref_t = rr.cast(g, want["grid"], trained, S, rcs.SENSOR)
    ref_all = rr.cast(g, want["grid"], None, S, rcs.SENSOR)
    d = dict(S=S, scan=scan, new=new, g=g, want=want, gd=gd, trained=trained, ref_t=ref_t, ref_all=ref_all, P=new.view.P)
    yield d
    for o in (gd, new, gd0, pt0):
        o.close()


def _zero(P):
    return np.zeros((P, M), np.uint8)


def test_scene_holds_every_case(scene):
    """asserted on the restatement's own output, so that a comparison that passes trivially cannot hide a missing case"""
    s = scene
    P, cls = s["P"], s["want"]["cls"]
    assert P == 22 and np.sum(cls == mr.FRESH) == 1 and not s["trained"][cls == mr.FRESH].any() and s["trained"].sum() == 21
    for ref in (s["ref_t"], s["ref_all"]):
        n, noop, occ, free = ref["counts"]
        assert n == len(s["S"]) == 314 and occ > 200 and free > 200 and ref["misses"].sum() >= 3
        assert rr.both_ways(ref["events"], (P, M)).sum() >= 10
        assert np.sum(ref["owner"] < 0) >= 1
        print("rays", n, "no-ops", noop, "miss their owner's voxel", ref["misses"].sum(), "occupied writes", occ, "free writes", free,
              "cells written both ways", rr.both_ways(ref["events"], (P, M)).sum())
    own = s["ref_all"]["owner"]
    fresh_rays = np.flatnonzero((own >= 0) & (cls[np.maximum(own, 0)] == mr.FRESH))
    assert len(fresh_rays) >= 20
    # ... which do nothing while the fresh leaf is untrained, and write once it counts as trained
    assert s["ref_t"]["noop"][fresh_rays].all() and not s["ref_all"]["noop"][fresh_rays].any()
    # axis-aligned rays walk, through more than one voxel
    axis = [i for i in s["ref_t"]["visited"] if np.all(rr.ray_of(s["S"][i], rcs.SENSOR)[1][:2] == 0.0)]
    assert len(axis) == 3 and max(len(s["ref_t"]["visited"][i]) for i in axis) >= 3
    # the walk crosses voxels that are no leaves, and the largest patch of the labelled batch fits the probit kernel's small shapes
    leaves = {tuple(int(x) for x in v) for v in s["want"]["grid"]["vox"] - s["want"]["grid"]["koff"]}
    assert any(c not in leaves for w in s["ref_t"]["visited"].values() for c in w)


@pytest.mark.parametrize("which", ["depth", "every leaf trained"])
def test_cells_and_counts_equal_the_restatement_exactly(gp, scene, which):
    import torch
    capi, ctx = gp
    s = scene
    depth, ref = (s["gd"], s["ref_t"]) if which == "depth" else (None, s["ref_all"])
    want = rr.cells_maxkey(ref["events"], _zero(s["P"]))
    assert np.array_equal(want, rr.cells_sequential(ref["events"], _zero(s["P"])))
    # host entry
    cells = _zero(s["P"])
    counts = s["new"].raycast(s["scan"], rcs.SENSOR, cells, depth=depth)
    print("counts", counts.tolist(), "restatement", ref["counts"].tolist(), "cells that differ", int(np.sum(cells != want)))
    assert np.array_equal(counts, ref["counts"])
    assert np.array_equal(cells, want)
    assert set(np.unique(cells)) == {capi.CELL_UNOBSERVED, capi.CELL_OCCUPIED, capi.CELL_FREE}
    # device entry, twice: the same bytes
    d_scan = torch.from_numpy(s["scan"].view(np.uint8).reshape(-1, 32)).cuda()
    for _ in range(2):
        d_cells = torch.zeros((s["P"], M), dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()
        c2 = s["new"].raycast(d_scan, rcs.SENSOR, d_cells, depth=depth, n=len(s["scan"]))
        assert np.array_equal(c2, counts) and d_cells.cpu().numpy().tobytes() == cells.tobytes()


def test_first_map_with_cells_that_do_not_fill_whole_waves(gp):
    """a map gpc_project_cloud cut (its batch holds the cloud itself; no origin shift) with sz = 10: m = 100 cells per leaf is no
    multiple of the 64 lanes the batch kernels work in, 1350 rays are several workgroups"""
    import torch
    capi, ctx = gp
    sz = 10
    A, ca = rcs.mc.model_cloud()
    cloud = ctx.make_cloud(A, ca)
    pt = ctx.project_cloud(cloud, RES, sz)
    g, P = pt.fetch(), pt.view.P
    sensor = np.array([0.41, 0.33, 0.9])
    ref = rr.cast(g, mr.model_grid(A, RES, sz), None, A, sensor)
    want = rr.cells_maxkey(ref["events"], np.zeros((P, sz * sz), np.uint8))
    assert P == 9 and ref["counts"][2] > 1000 and ref["counts"][3] > 0 and len(np.unique(want)) == 3
    cells = np.zeros((P, sz * sz), np.uint8)
    counts = pt.raycast(cloud, sensor, cells)
    assert np.array_equal(counts, ref["counts"]) and np.array_equal(cells, want)
    off_w, x0_w, x1_w, y_w = rr.occupancy_batch(want, RES, sz)
    off, x0, x1, y, n_total, n_max = pt.occupancy_batch(torch.from_numpy(cells).cuda())
    assert n_total == int(off_w[-1]) and n_max == int(np.diff(off_w).max()) > 64 and np.array_equal(off.cpu().numpy(), off_w)
    for got, exp in ((x0, x0_w), (x1, x1_w), (y, y_w)):
        assert got.cpu().numpy().tobytes() == exp.tobytes()
    pt.close()


def test_prefilled_cells_keep_their_values_where_no_ray_wrote(gp, scene):
    s = scene
    fresh = rr.cells_maxkey(s["ref_t"]["events"], _zero(s["P"]))
    pre = np.random.default_rng(5).integers(0, 3, (s["P"], M)).astype(np.uint8)
    cells = pre.copy()
    s["new"].raycast(s["scan"], rcs.SENSOR, cells, depth=s["gd"])
    assert np.array_equal(cells, rr.cells_maxkey(s["ref_t"]["events"], pre))
    assert np.array_equal(cells[fresh == 0], pre[fresh == 0]) and np.array_equal(cells[fresh != 0], fresh[fresh != 0])
    assert np.any(pre[fresh == 0] != 0) and np.any(cells != pre)


def test_mapping_carries_the_cells_over_two_scans(gp, monkeypatch):
    """capi.Mapping.add_cloud twice (the second scan opens a leaf below the map's corner, so the grid's origin shifts and old_to_new is
    no identity) against the restatement applied twice.  The registered cloud and the sensor of each call are recorded at the binding."""
    capi, ctx = gp
    A, pt0, gd0, gc0 = _model(capi, ctx, colour=True, moved=True)
    calls = []
    inner = capi.Patches.raycast

    def recording(self, cloud, origin, cells, depth=None, n=None):
        host = np.zeros(n, dtype=capi.Context.POINT_DTYPE)
        ctx._check(ctx.lib.gpc_dev_memcpy(ctx.h, host.ctypes.data, cloud, host.nbytes, 2))
        rec = dict(xyz=np.stack([host["x"], host["y"], host["z"]], 1), rgb=np.stack([host["r"], host["g"], host["b"]], 1),
                   origin=np.array(origin, dtype=np.float64), before=cells.cpu().numpy().copy(), trained=depth.sizes() > 0, g=self.fetch())
        rec["counts"] = inner(self, cloud, origin, cells, depth=depth, n=n)
        calls.append(rec)
        return rec["counts"]
    monkeypatch.setattr(capi.Patches, "raycast", recording)
    prm = capi.default_params_registration(step=1e-7, tol=1e300, min_steps=2, max_steps=10)
    mp = capi.Mapping(ctx, pt0, gd0, gc0, params=prm, min_nbr=MIN_NBR)
    assert mp.cells.shape == (21, M) and not mp.cells.any()
    S, cs = rcs.scan_cloud()
    rng = np.random.default_rng(9)
    ex, ec = rcs.mc.sheet(rng, -0.75, 0.25, 1, 1, rcs.Z_LOWER, npv=30)
    S, S2, cs2 = _moved(S), _moved(np.concatenate([S + np.float32(0.002), ex])), np.concatenate([cs, ec])
    model, grid, cells, tr_before = mp.patches.fetch(), mr.model_grid(A, RES, SZ), _zero(21), mp.depth.sizes() > 0
    for k, (xyz, rgb) in enumerate(((S, cs), (S2, cs2))):
        steps, inserted = mp.add_cloud(ctx.make_cloud(xyz, rgb))
        assert inserted and len(calls) == k + 1
        c = calls[k]
        assert np.any(c["origin"] != 0.0) and np.all(np.abs(c["origin"]) < 1e-3)    # the accumulated translation: the sensor
        g = c["g"]
        want = mr.insert(model, grid, tr_before, c["xyz"], c["rgb"], MIN_NBR, frames=g["R"])
        assert np.array_equal(g["off"], want["off"]) and np.array_equal(g["src"], want["src"])
        P = len(want["cls"])
        carried = _zero(P)
        carried[want["old_to_new"]] = cells
        assert np.array_equal(c["before"], carried)
        assert np.array_equal(c["trained"][want["old_to_new"]], tr_before) and c["trained"].sum() == tr_before.sum()
        ref = rr.cast(g, want["grid"], c["trained"], c["xyz"], c["origin"])
        cells = rr.cells_maxkey(ref["events"], carried)
        assert np.array_equal(c["counts"], ref["counts"]) and ref["counts"][2] > 100 and ref["counts"][3] > 100
        assert np.array_equal(mp.cells.cpu().numpy(), cells)
        model, grid, tr_before = mp.patches.fetch(), want["grid"], mp.depth.sizes() > 0
    assert np.all(grid["koff"] == [3, 0, 0]) and mp.patches.view.P == 23 and not np.array_equal(want["old_to_new"], np.arange(22))
    # the second scan saw through cells the first had not met, and the first scan's labels are still there where it did not
    assert np.any((calls[1]["before"] == 0) & (cells != 0)) and np.any((calls[1]["before"] != 0) & (cells == calls[1]["before"]))
    # the occupancy layer from the map's cells
    p = capi.default_params_dense(sigmaf_sq=1.0, l_sq=(RES / 4) ** 2, noise=0.25, noise_model=2)
    f, st = mp.occupancy(p)
    f, st = f.cpu().numpy(), st.cpu().numpy()
    assert f.shape == (23, M) and np.all(st == 0) and np.all(np.isfinite(f))
    seen = cells != 0
    assert np.all(f[~seen.any(axis=1)] == 0.0)
    # the same fit through the host entry on the restated batch; and the mode sides with its labels (the cell centres are the training
    # points; 0.8 as in tests/test_probit_gpu.py)
    off_w, x0_w, x1_w, y_w = rr.occupancy_batch(cells, RES, SZ)
    fh, *_ = ctx.dense_irls_fit_predict(p, capi.default_params_irls(), off_w, x0_w, x1_w, y_w, res=RES, sz=SZ)
    assert np.max(np.abs(f - fh)) <= 1e-8 * np.max(np.abs(fh))
    assert np.mean(np.sign(f[seen]) == np.where(cells[seen] == 1, 1.0, -1.0)) > 0.8
    mp.close()


def test_occupancy_batch_and_the_probit_fit_on_it(gp, scene, oracle):
    import torch
    capi, ctx = gp
    s = scene
    P = s["P"]
    cells = rr.cells_maxkey(s["ref_t"]["events"], _zero(P))
    off_w, x0_w, x1_w, y_w = rr.occupancy_batch(cells, RES, SZ)
    d_cells = torch.from_numpy(cells).cuda()
    off, x0, x1, y, n_total, n_max = s["new"].occupancy_batch(d_cells)
    assert n_total == int(off_w[-1]) == np.count_nonzero(cells) and n_max == int(np.diff(off_w).max()) <= M
    assert np.array_equal(off.cpu().numpy(), off_w)
    for got, want in ((x0, x0_w), (x1, x1_w), (y, y_w)):
        assert got.cpu().numpy().tobytes() == want.tobytes()
    cnt = np.diff(off_w)
    assert np.any(cnt == 0) and np.any(y_w > 0) and np.any(y_w < 0)          # the fresh leaf is an empty patch
    # the probit GP on the batch, from the device buffers, against the oracle's IRLS fit of the same batch
    s20, l_sq = 0.25, (RES / 4) ** 2
    p = capi.default_params_dense(sigmaf_sq=1.0, l_sq=l_sq, noise=s20, noise_model=2)
    ir = capi.default_params_irls()
    f = torch.empty((P, M), dtype=torch.float64, device="cuda")
    st = torch.full((P,), -1, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    ctx.dense_irls_fit_predict_dev(p, ir, P, off, n_max, n_total, x0, x1, y, M, None, None, RES, SZ, f, status=st)
    ctx.synchronize()
    f, st = f.cpu().numpy(), st.cpu().numpy()
    from gp_compressor_amd import synth
    xs0, xs1 = synth.grid(RES, SZ)
    op = oracle.dense_params(sigmaf_sq=1.0, l_sq=l_sq, sigman_sq=s20)
    fo, alo, fho, ito, sto = oracle.dense_irls_fit_predict_batch(op, 2, off_w, x0_w, x1_w, y_w, xs0, xs1, max_iter=ir.max_iter, tol=ir.tol,
                                                                 f_init=ir.f_init)
    assert np.array_equal(st, sto) and np.all(sto == 0)
    worst = 0.0
    for i in range(P):
        scale = max(np.max(np.abs(fo[i])), 1e-6)
        worst = max(worst, float(np.max(np.abs(f[i] - fo[i])) / scale))
    print("IRLS on the labelled batch vs the oracle: worst relative difference", worst)
    assert worst <= 1e-8
    assert np.all(f[cnt == 0] == 0.0)


def test_raycast_contract(gp, scene):
    import torch
    capi, ctx = gp
    s = scene
    L = ctx.lib
    new, gd, scan, P = s["new"], s["gd"], s["scan"], s["P"]
    pre = np.random.default_rng(6).integers(0, 3, (P, M)).astype(np.uint8)
    org = np.ascontiguousarray(rcs.SENSOR, dtype=np.float64)
    counts = np.zeros(4, np.int32)

    def call(c, m, depth, cloud, n, origin, cells, entry=L.gpc_patches_raycast):
        return entry(c, m, depth, cloud, n, origin.ctypes.data if origin is not None else None,
                     cells.ctypes.data if cells is not None else None, counts.ctypes.data)
    # n == 0: nothing happens
    cells = pre.copy()
    assert call(ctx.h, new.h, gd.h, None, 0, org, cells) == capi.GPC_OK and np.array_equal(cells, pre) and counts[0] == 0
    # a non-finite origin
    for bad in (np.nan, np.inf):
        o2 = org.copy()
        o2[1] = bad
        assert call(ctx.h, new.h, gd.h, scan.ctypes.data, len(scan), o2, cells) == capi.GPC_EINVAL
    # a depth object with another P, a colour GP
    for wrongP, ny in ((P + 1, 1), (P, 3)):
        wrong = capi.Sparse(ctx, capi.default_params_sparse(ny, **KW_D), wrongP, ny)
        assert call(ctx.h, new.h, wrong.h, scan.ctypes.data, len(scan), org, cells) == capi.GPC_EINVAL
        wrong.close()
    # a cloud that is not the batch's: fewer points than the batch holds (known on the host) ...
    n_total = new.view.n_total
    assert n_total < len(scan)
    assert call(ctx.h, new.h, gd.h, scan.ctypes.data, n_total - 1, org, cells) == capi.GPC_EINVAL
    # ... or as many, with a batch entry that points beyond them (found on the device)
    assert s["g"]["src"].max() >= n_total
    assert call(ctx.h, new.h, gd.h, scan.ctypes.data, n_total, org, cells) == capi.GPC_EINVAL
    # a non-finite coordinate
    nan = scan.copy()
    nan["z"][int(np.flatnonzero(s["ref_t"]["owner"] < 0)[0])] = np.nan
    assert call(ctx.h, new.h, gd.h, nan.ctypes.data, len(nan), org, cells) == capi.GPC_EINVAL
    assert np.array_equal(cells, pre)                                       # every refusal left the cells alone
    # ... on the device too, where the refusal is found after the rays were cast
    d_cells = torch.from_numpy(pre).cuda()
    d_nan = torch.from_numpy(nan.view(np.uint8).reshape(-1, 32)).cuda()
    torch.cuda.synchronize()
    rc = L.gpc_patches_raycast_dev(ctx.h, new.h, gd.h, d_nan.data_ptr(), len(nan), org.ctypes.data, d_cells.data_ptr(), counts.ctypes.data)
    assert rc == capi.GPC_EINVAL and np.array_equal(d_cells.cpu().numpy(), pre)
    # objects of another context; missing arguments
    ctx2 = capi.Context(0)
    other = capi.Sparse(ctx2, capi.default_params_sparse(1, **KW_D), P, 1)
    assert call(ctx.h, new.h, other.h, scan.ctypes.data, len(scan), org, cells) == capi.GPC_EINVAL
    assert call(ctx2.h, new.h, None, scan.ctypes.data, len(scan), org, cells) == capi.GPC_EINVAL
    other.close()
    ctx2.close()
    assert call(ctx.h, None, gd.h, scan.ctypes.data, len(scan), org, cells) == capi.GPC_EINVAL
    assert call(ctx.h, new.h, gd.h, None, 5, org, cells) == capi.GPC_EINVAL
    assert call(ctx.h, new.h, gd.h, scan.ctypes.data, -1, org, cells) == capi.GPC_EINVAL
    assert call(ctx.h, new.h, gd.h, scan.ctypes.data, len(scan), None, cells) == capi.GPC_EINVAL
    assert call(ctx.h, new.h, gd.h, scan.ctypes.data, len(scan), org, None) == capi.GPC_EINVAL
    # counts may be NULL; the call is then asynchronous on the device entry and complete after a synchronize
    d_scan = torch.from_numpy(scan.view(np.uint8).reshape(-1, 32)).cuda()
    d_cells = torch.zeros((P, M), dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    assert L.gpc_patches_raycast_dev(ctx.h, new.h, gd.h, d_scan.data_ptr(), len(scan), org.ctypes.data, d_cells.data_ptr(), None) == capi.GPC_OK
    ctx.synchronize()
    assert np.array_equal(d_cells.cpu().numpy(), rr.cells_maxkey(s["ref_t"]["events"], _zero(P)))
    # the occupancy batch refuses missing buffers
    nt = C.c_int32(0)
    assert L.gpc_occupancy_batch_dev(ctx.h, new.h, d_cells.data_ptr(), None, None, None, None, C.addressof(nt), C.addressof(nt)) == capi.GPC_EINVAL
