"""GPU tests of the map insertion, gpc_sparse_remap and the registration step on a grown map at the sizes where their leaf kernels span
workgroups (tests/mapping_scale_cases.py; test_mapping_gpu.py holds the same assertions on a 3 x 3-voxel model, where every leaf-indexed
kernel runs inside one block).

  striped      270 old and 270 (273) new leaves alternating in runs of three: the rank merge, the re-keying into wider key fields, two
               blocks of mp_rekey / mp_flag / mp_merge / pc_bucket_offsets, 9 of mp_frame, 135 of mp_moment / mp_means -- bit for bit
               project_cloud of the union, through both entries
  overlap      266 old leaves, 581 merged, idle / kept / fresh leaves on both sides of leaves 256 and 512, a 10-bit owner sort: against the
               NumPy restatement (tests/mapping_ref.py) on the GPU's own frames, exactly; twice, bit for bit; then the GP states through
               gpc_sparse_remap (one workgroup per old leaf) and a registration step on the grown map
  chunk edges  fresh leaves of exactly 1 .. 257 points: the 64-point chunks of mp_means_kernel's serial depth sum

Bounds: everything the insertion computes is compared exactly (test_mapping_gpu.py says why it can be); fresh frames against the oracle's
compute_rotation of the restatement's sums to 1e-12, locals to 1e-12 res, the registration sums to 1e-8, as the tests of the small model
and test_registration_gpu.py do.  One derived bound: a depth mean, summed one term after the other over c terms, lies within
c 2^-53 sum|d| of the exact mean (the forward bound (c - 1) u sum|d| of the sum, divided by c, plus the roundings of the division and
of the row it is read back from -- at most 3 u sum|d| together, and exact for c = 1)."""
import numpy as np
import pytest

from gp_compressor_amd import synth
import mapping_cases as mc
import mapping_ref as mr
import mapping_scale_cases as ms
import registration_ref as ref

pytestmark = pytest.mark.gpu

RES, SZ = ms.RES, ms.SZ
HYP = dict(sigmaf_sq=1.0, l_sq=(RES / 5) ** 2)
KW_D = dict(HYP, noise=1e-3, capacity=24)
KW_C = dict(HYP, noise=1.0, capacity=100)            # (capacity 100 where likelihoods are evaluated: test_mapping_gpu.py, KW_C_REG)
KW_D12 = dict(HYP, noise=1e-3, capacity=12)          # the carry-over compares states bit for bit: small capacity, deletions happen
KW_C12 = dict(HYP, noise=1.0, capacity=12)
BATCH_KEYS = ("off", "src", "x0", "x1", "y", "rgb") + ms.FRAME_KEYS


@pytest.fixture(scope="module")
def gp():
    from gp_compressor_amd import capi
    capi.load()
    ctx = capi.Context(0)
    yield capi, ctx
    ctx.close()


def _device_cloud(scan):
    import torch
    d = torch.from_numpy(scan.view(np.uint8).reshape(-1, 32)).cuda()
    torch.cuda.synchronize()
    return d


def _train(capi, ctx, b, keep_leaf, kw_d, kw_c, seed=6):
    """depth and colour GPs on the batch b, the leaves outside keep_leaf left empty"""
    P = len(b["mean"])
    cnt = np.diff(b["off"])
    cnt[~keep_leaf] = 0
    keep = np.concatenate([np.arange(b["off"][i], b["off"][i] + cnt[i]) for i in range(P)]).astype(np.int64)
    off_t = np.concatenate([[0], np.cumsum(cnt)]).astype(np.int32)
    perm = synth.sattolo_perms(off_t, seed=seed)
    gd = capi.Sparse(ctx, capi.default_params_sparse(1, **kw_d), P, 1)
    gc = capi.Sparse(ctx, capi.default_params_sparse(3, **kw_c), P, 3)
    st_d = gd.add(off_t, b["x0"][keep], b["x1"][keep], b["y"][None, keep], perm)
    st_c = gc.add(off_t, b["x0"][keep], b["x1"][keep], np.ascontiguousarray(b["rgb"][:, keep]), perm)
    assert np.array_equal(gd.sizes() > 0, keep_leaf) and np.array_equal(gc.sizes() > 0, keep_leaf)
    return gd, gc, st_d, st_c


def _callbacks(pairs):
    """the closed-form likelihood on the GPU's own states (as test_registration_gpu.py)"""
    out = []
    for g, kw in pairs:
        alpha, Cm, _, BV = g.state()
        sizes = g.sizes()

        def f(i, x0, x1, y, alpha=alpha, Cm=Cm, BV=BV, sizes=sizes, kw=kw):
            bb = int(sizes[i])
            return ref.closed_form_likelihood(kw["sigmaf_sq"], kw["l_sq"], kw["noise"], alpha[i][:, :bb], Cm[i][:bb, :bb], BV[i][:bb], x0, x1, y)
        out.append(f)
    return out


# ---- 1: striped, both entries ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("below", [False, True], ids=["above", "below"])
def test_striped_scan_is_project_cloud_of_the_union_bit_for_bit(gp, below):
    capi, ctx = gp
    A, ca = ms.striped_model()
    B, cb, _ = ms.striped_scan(below)
    pt_a = ctx.project_cloud(ctx.make_cloud(A, ca), RES, SZ)
    pt_ab = ctx.project_cloud(ctx.make_cloud(np.concatenate([A, B]), np.concatenate([ca, cb])), RES, SZ)
    scan = ctx.make_cloud(B, cb)
    new_h, o2n_h = pt_a.insert_cloud(scan, min_nbr=1)                                  # the host-pointer entry
    new_d, o2n_d = pt_a.insert_cloud(_device_cloud(scan), min_nbr=1, n=len(scan))      # the device-pointer entry
    a, w, g, g_d = pt_a.fetch(), pt_ab.fetch(), new_h.fetch(), new_d.fetch()
    assert np.array_equal(o2n_h, o2n_d)
    for k in BATCH_KEYS:
        assert ms.same_bits(g[k], g_d[k]), k
    P = pt_ab.view.P
    assert pt_a.view.P == 270 and P == 540 + 3 * below
    for new in (new_h, new_d):
        v = new.view
        assert (v.P, v.m, v.n_total, v.n_max) == (P, SZ * SZ, len(g["src"]), np.diff(g["off"]).max())
    ms.check_union(g, o2n_h, a, w, len(A), len(B))
    # old_to_new is the key merge of the restatement; the origin shifts and the key fields widen as the case says
    want = mr.insert(a, mr.model_grid(A, RES, SZ), np.ones(270, bool), B, cb, 1, frames=g["R"])
    assert np.array_equal(want["grid"]["koff"], [12, 3, 2] if below else [0, 0, 0])
    assert np.array_equal(o2n_h, want["old_to_new"])
    ms.check_insertion(g, o2n_h, want, len(B))
    for o in (new_h, new_d, pt_ab, pt_a):
        o.close()


# ---- 2: overlap at scale ----------------------------------------------------------------------------------------------------------------
class Overlap:
    pass


@pytest.fixture(scope="module")
def overlap(gp):
    """the overlapping insertion at scale, shared (read-only) by the tests below"""
    capi, ctx = gp
    o = Overlap()
    o.case = c = ms.overlap_scale()
    (o.A, o.ca), (o.S, o.cs) = c["model"], c["scan"]
    o.pt = ctx.project_cloud(ctx.make_cloud(o.A, o.ca), RES, SZ)
    o.b = o.pt.fetch()
    o.P0 = o.pt.view.P
    assert o.P0 == 266
    o.trained = np.ones(o.P0, bool)
    o.trained[c["untrained"]] = False
    o.gd, o.gc, _, _ = _train(capi, ctx, o.b, o.trained, KW_D, KW_C)
    o.grid = mr.model_grid(o.A, RES, SZ)
    o.scan = ctx.make_cloud(o.S, o.cs)
    o.new, o.o2n = o.pt.insert_cloud(_device_cloud(o.scan), min_nbr=c["min_nbr"], depth=o.gd, n=len(o.scan))
    o.g = o.new.fetch()
    o.want = mr.insert(o.b, o.grid, o.trained, o.S, o.cs, c["min_nbr"], frames=o.g["R"])
    yield o
    for x in (o.new, o.gd, o.gc, o.pt):
        x.close()


def test_overlap_at_scale_matches_the_restatement_exactly(gp, overlap, oracle):
    o = overlap
    g, want, o2n = o.g, o.want, o.o2n
    cls = want["cls"]
    P = len(cls)
    v = o.new.view
    # the case is what the CPU tests found it to be (there on the oracle's model, here on the device's)
    assert P == 581 and len(ms.voxel_set(o.S)) > 256
    for lo, hi in ((0, 256), (256, 512), (512, P)):
        assert min(ms.class_counts(cls, lo, hi)) >= 1
    assert np.array_equal(np.flatnonzero(cls[o2n] == mr.IDLE), ms.OV_HOLES)
    assert np.array_equal(want["grid"]["koff"], [2, 0, 2])
    # leaf table, offsets, owners, rows, means, masks: exactly
    assert v.P == P and v.m == SZ * SZ
    ms.check_insertion(g, o2n, want, len(o.S))
    assert v.n_total == want["off"][-1] == len(g["src"]) and v.n_max == np.diff(want["off"]).max()
    assert np.all(want["owner"][-o.case["n_lonely"]:] == -1)
    # kept and idle leaves: the model's frames bit for bit; W is the OR; colours are minus the stored mean
    for i in range(o.P0):
        L = o2n[i]
        if cls[L] == mr.FRESH:
            continue
        sl = slice(g["off"][L], g["off"][L + 1])
        for k in ("R", "mean", "rgb_mean"):
            assert ms.same_bits(g[k][L], o.b[k][i]), (k, i)
        hit = np.zeros(SZ * SZ, np.uint8)
        gx = np.clip((SZ * (g["x0"][sl] / RES + 0.5)).astype(int), 0, SZ - 1)
        gy = np.clip((SZ * (g["x1"][sl] / RES + 0.5)).astype(int), 0, SZ - 1)
        hit[SZ * gx + gy] = 1
        assert np.array_equal(g["W"][L], o.b["W"][i] | hit)
        assert np.array_equal(g["rgb"][:, sl], (o.cs[g["src"][sl]].astype(np.float64) - o.b["rgb_mean"][i]).T)
    # fresh frames: the oracle's compute_rotation of the restatement's moment sums
    byo = mr.insert(o.b, o.grid, o.trained, o.S, o.cs, o.case["min_nbr"], compute_rotation=oracle.compute_rotation)
    fresh = np.flatnonzero(cls == mr.FRESH)
    assert len(fresh) > 256 and np.array_equal(byo["cls"], cls)
    assert np.max(np.abs(g["R"][fresh] - byo["R"][fresh])) <= 1e-12


def test_insertion_at_scale_is_reproducible_bit_for_bit(gp, overlap):
    capi, ctx = gp
    o = overlap
    for cloud, n in ((_device_cloud(o.scan), len(o.scan)), (o.scan, None)):            # the same entry again, then the host-pointer entry
        again, o2n = o.pt.insert_cloud(cloud, min_nbr=o.case["min_nbr"], depth=o.gd, n=n)
        g2 = again.fetch()
        assert np.array_equal(o2n, o.o2n)
        assert (again.view.P, again.view.n_total, again.view.n_max) == (o.new.view.P, o.new.view.n_total, o.new.view.n_max)
        for k in BATCH_KEYS:
            assert ms.same_bits(o.g[k], g2[k]), k
        again.close()


# ---- 3: chunk edges ---------------------------------------------------------------------------------------------------------------------
def test_depth_mean_chain_at_the_chunk_edges(gp):
    capi, ctx = gp
    A, ca = mc.model_cloud()
    S, cs = ms.chunk_edge_scan()
    counts = np.array(ms.CHUNK_COUNTS)
    pt = ctx.project_cloud(ctx.make_cloud(A, ca), RES, SZ)
    a = pt.fetch()
    new, o2n = pt.insert_cloud(ctx.make_cloud(S, cs), min_nbr=1)
    g = new.fetch()
    want = mr.insert(a, mr.model_grid(A, RES, SZ), np.ones(9, bool), S, cs, 1, frames=g["R"])
    P = new.view.P
    fresh = np.arange(9, P)
    assert P == 9 + len(counts) and np.array_equal(o2n, np.arange(9))
    assert np.array_equal(np.diff(g["off"])[fresh], counts) and np.all(np.diff(g["off"])[:9] == 0)
    assert new.view.n_max == 257 and new.view.n_total == counts.sum()
    # the restatement sums one term after the other: bit for bit
    for k in ("mean", "rgb_mean", "y"):
        assert ms.same_bits(g[k], want[k]), k
    ms.check_insertion(g, o2n, want, len(S))
    # independently of that order: the shift a leaf took off its rows, d - y read back in extended precision, against the exact mean
    u = np.longdouble(2.0) ** -53
    for L, c in zip(fresh, counts):
        sl = slice(g["off"][L], g["off"][L + 1])
        d = want["local"][g["src"][sl], 0].astype(np.longdouble)
        shift = d - g["y"][sl].astype(np.longdouble)
        exact = d.sum() / np.longdouble(c)
        bound = np.longdouble(c) * u * np.abs(d).sum()
        print(f"chunk edge c = {c}: max |shift - mean| = {float(np.max(np.abs(shift - exact))):.3e}, bound {float(bound):.3e}")
        assert np.all(np.abs(shift - exact) <= bound), c
    for x in (new, pt):
        x.close()


# ---- 4: the GP states follow --------------------------------------------------------------------------------------------------------------
def test_states_carry_over_at_scale_and_training_matches_a_control_object(gp, overlap):
    """gpc_sparse_remap with 266 source patches (a workgroup each) into 581.  Sizes and the whole state, padding included, are compared
    bit for bit; the per-patch point count and status have no read-out of their own and show in the add that follows."""
    import torch
    capi, ctx = gp
    o = overlap
    g, o2n = o.g, o.o2n
    P = o.new.view.P
    v = o.new.view
    rest = np.setdiff1d(np.arange(P), o2n)
    gd, gc, _, _ = _train(capi, ctx, o.b, o.trained, KW_D12, KW_C12)
    assert gd.sizes().max() == 12 and gd.sizes().min() == 0
    for old, kw, ny, plane, seed in ((gd, KW_D12, 1, g["y"][None, :], 11), (gc, KW_C12, 3, g["rgb"], 12)):
        moved = old.remap(P, o2n)
        assert moved.P == P and moved.ld() == old.ld()
        assert np.array_equal(moved.sizes()[o2n], old.sizes()) and np.all(moved.sizes()[rest] == 0)
        so, sm = old.state(), moved.state()
        for x, y in zip(so, sm):
            assert ms.same_bits(y[o2n], x)
            assert not y[rest].any() and not np.signbit(y[rest]).any()                   # every other patch: zero state
        for x, y in zip(so, old.state()):                                                # (old is untouched)
            assert ms.same_bits(x, y)
        # control: the new P, filled from the remapped state, trained through the public host entry
        ctl = capi.Sparse(ctx, capi.default_params_sparse(ny, **kw), P, ny)
        al, Cm, Q, BV = sm
        ctl.set_state(moved.sizes(), al, BV, Cm, Q)
        perm = synth.sattolo_perms(g["off"], seed=seed)
        d_perm = torch.from_numpy(perm).cuda()
        st = torch.full((P,), -1, dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()
        moved.add_dev(v.off, v.n_max, v.n_total, v.x0, v.x1, v.y if ny == 1 else v.rgb, d_perm, st)
        ctx.synchronize()
        st_c = ctl.add(g["off"], g["x0"], g["x1"], np.ascontiguousarray(plane), perm)
        assert np.array_equal(st.cpu().numpy(), st_c) and np.all(st_c == 0)
        b_ = moved.sizes()
        assert np.array_equal(b_, ctl.sizes())
        assert b_.max() == kw["capacity"] and np.diff(g["off"]).max() > kw["capacity"]              # deletions happened
        assert np.all(b_[o2n[o.trained]] > 0) and np.all((b_ > 0) == ((np.diff(g["off"]) > 0) | np.isin(np.arange(P), o2n[o.trained])))
        for name, x, y in zip(("alpha", "C", "Q", "BV"), moved.state(), ctl.state()):
            for i in range(P):                                                           # the live part of every patch
                bb = int(b_[i])
                xs = x[i][:, :bb] if name == "alpha" else (x[i][:bb] if name == "BV" else x[i][:bb, :bb])
                ys = y[i][:, :bb] if name == "alpha" else (y[i][:bb] if name == "BV" else y[i][:bb, :bb])
                assert ms.same_bits(xs, ys), (name, i)
        ctl.close()
        moved.close()
    gd.close()
    gc.close()


# ---- 5: registration on the grown map -------------------------------------------------------------------------------------------------------
def test_registration_step_on_the_grown_map_at_scale(gp, overlap):
    capi, ctx = gp
    o = overlap
    g, want, o2n = o.g, o.want, o.o2n
    P = o.new.view.P
    assert P > 512
    gd, gc = o.gd.remap(P, o2n), o.gc.remap(P, o2n)
    v = o.new.view
    gd.add_dev(v.off, v.n_max, v.n_total, v.x0, v.x1, v.y)
    gc.add_dev(v.off, v.n_max, v.n_total, v.x0, v.x1, v.rgb)
    ctx.synchronize()
    trained = gd.sizes() > 0
    idle = o2n[list(ms.OV_HOLES)]
    assert np.array_equal(np.flatnonzero(~trained), idle)
    # the scan: every third point of model and scan, moved a little, and the probes one voxel outside each face of the grown grid
    px, face = ms.face_probes(want["grid"])
    body = (np.concatenate([o.A, o.S])[::3].astype(np.float64) + np.array([0.004, -0.003, 0.002])).astype(np.float32)
    xyz = np.concatenate([px, body])
    rgb = np.concatenate([np.full((len(px), 3), 128, np.uint8), np.concatenate([o.ca, o.cs])[::3]])
    rgrid = mr.registration_grid(want["grid"])
    ow, lw = ref.assign(xyz, g, rgrid, trained)
    owned = ow[:len(px)] >= 0
    assert all(np.sum(owned[face == f]) >= 1 for f in range(6)), [int(np.sum(owned[face == f])) for f in range(6)]
    assert np.any(ow[len(px):] >= 512) and np.any((ow[len(px):] >= 0) & (ow[len(px):] < 256))
    assert not np.any(np.isin(ow, idle))
    lik_d, lik_c = _callbacks(((gd, KW_D), (gc, KW_C)))
    r0 = ref.reduce_step(rgb, ow, lw, g, lik_d, lik_c)
    assert r0["n_used"] > 0.5 * len(xyz) and np.all(np.isfinite(r0["delta"])) and np.max(np.abs(r0["delta"])) > 0
    reg = capi.Registration(ctx, o.new, gd, gc)
    reg.set_cloud(ctx.make_cloud(xyz, rgb))
    out = reg.step(capi.default_params_registration(step=0.002 / float(np.max(np.abs(r0["delta"])))))
    owner, local = reg.assignment()
    assert np.array_equal(owner, ow) and np.max(np.abs(local - lw)) <= 1e-12 * RES
    assert out[8] == r0["n_used"]
    assert np.all(np.abs(out[:6] - r0["delta"]) <= 1e-8 * r0["gabs"])
    assert abs(out[6] - r0["ls"]) <= 1e-8 * abs(r0["ls"]) and abs(out[7] - r0["cls"]) <= 1e-8 * abs(r0["cls"])
    for x in (reg, gd, gc):
        x.close()
