"""GPU tests of the map insertion (gp_mapping::insert_into_map, /root/reference/src/gp_mapping.cpp): gpc_patches_insert_cloud against
the producer (a disjoint scan: bit for bit project_cloud of the union) and against the NumPy restatement (tests/mapping_ref.py)
evaluated on the GPU's own frames (an overlapping scan: owners, coordinates, means and masks exactly); gpc_sparse_remap and the
training that follows against a control object; the registration round trip; the Mapping flow; the contract.

Bounds: everything the insertion computes is compared exactly -- its kernels evaluate the restatement's expressions in its association
with contraction off, sequential sums in the stated order.  The re-cut frame of an old leaf is compared with the oracle's
compute_rotation of the same moment sums to 1e-12 (the device's sqrt and division are correctly rounded, its Jacobi sweep is the
oracle's; the producer tests pin the same code bit for bit).  The registration step carries the bounds of test_registration_gpu.py
(1e-8 on the GPU's own state).  Clouds: tests/mapping_cases.py (res 0.25, sz 8, about 150 points per voxel, dyadic corners)."""
import ctypes as C

import numpy as np
import pytest

from gp_compressor_amd import synth
import mapping_cases as mc
import mapping_ref as mr
import registration_ref as ref

pytestmark = pytest.mark.gpu

RES, SZ = mc.RES, mc.SZ
KW_D = dict(sigmaf_sq=1.0, l_sq=(RES / 5) ** 2, noise=1e-3, capacity=24)
KW_C = dict(sigmaf_sq=1.0, l_sq=(RES / 5) ** 2, noise=1.0, capacity=24)
# Where likelihoods are evaluated (the registration step, the Mapping flow) the colour field keeps the reference's default capacity,
# as in test_registration_gpu.py: at capacity 24 the field recursion of these colours (amplitude ~100 grey levels against sigma_f = 1)
# diverges through its deletions -- |alpha| beyond 1e150 on the CPU oracle as on the device -- and every likelihood is NaN or 0.
# The carry-over test compares states bit for bit and keeps 24: deletions are what it is about.
KW_C_REG = dict(KW_C, capacity=100)
FRAME_KEYS = ("R", "mean", "rgb_mean", "W")


@pytest.fixture(scope="module")
def gp():
    from gp_compressor_amd import capi
    capi.load()
    ctx = capi.Context(0)
    yield capi, ctx
    ctx.close()


class Model:
    """A -> producer -> depth and colour GPs (capacity 24: deletions happen); the leaves in `untrained` get no points"""

    def __init__(self, capi, ctx, untrained=(), kw_c=KW_C):
        self.capi, self.ctx = capi, ctx
        self.xyz, self.rgb = mc.model_cloud()
        self.pt = ctx.project_cloud(ctx.make_cloud(self.xyz, self.rgb), RES, SZ)
        self.b = b = self.pt.fetch()
        self.P = P = self.pt.view.P
        assert P == 9
        cnt = np.diff(b["off"])
        cnt[list(untrained)] = 0
        keep = np.concatenate([np.arange(b["off"][i], b["off"][i] + cnt[i]) for i in range(P)]).astype(np.int64)
        off_t = np.concatenate([[0], np.cumsum(cnt)]).astype(np.int32)
        perm = synth.sattolo_perms(off_t, seed=6)
        self.gd = capi.Sparse(ctx, capi.default_params_sparse(1, **KW_D), P, 1)
        self.gc = capi.Sparse(ctx, capi.default_params_sparse(3, **kw_c), P, 3)
        assert np.all(self.gd.add(off_t, b["x0"][keep], b["x1"][keep], b["y"][None, keep], perm) == 0)
        assert np.all(self.gc.add(off_t, b["x0"][keep], b["x1"][keep], np.ascontiguousarray(b["rgb"][:, keep]), perm) == 0)
        self.trained = self.gd.sizes() > 0
        assert np.array_equal(self.trained, cnt > 0)
        self.grid = mr.model_grid(self.xyz, RES, SZ)

    def close(self):
        for o in (self.gd, self.gc, self.pt):
            o.close()


def _owner_of(batch, n):
    own = np.full(n, -1, dtype=np.int32)
    for L in range(len(batch["off"]) - 1):
        own[batch["src"][batch["off"][L]:batch["off"][L + 1]]] = L
    return own


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


# ---- 1 ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("where", ["above", "below"])
def test_disjoint_scan_is_project_cloud_of_the_union_bit_for_bit(gp, where):
    capi, ctx = gp
    A, ca = mc.model_cloud()
    B, cb = mc.disjoint_scan(where)
    pt_a = ctx.project_cloud(ctx.make_cloud(A, ca), RES, SZ)
    pt_ab = ctx.project_cloud(ctx.make_cloud(np.concatenate([A, B]), np.concatenate([ca, cb])), RES, SZ)
    new, o2n = pt_a.insert_cloud(ctx.make_cloud(B, cb), min_nbr=1)
    a, g, w = pt_a.fetch(), new.fetch(), pt_ab.fetch()
    P = pt_ab.view.P
    assert new.view.P == P == 11 and new.view.m == SZ * SZ
    # old_to_new is the key merge: the restatement's, and where the union's leaves hold A's points
    want = mr.insert(a, mr.model_grid(A, RES, SZ), np.ones(9, bool), B, cb, 1, frames=g["R"])
    assert np.array_equal(want["grid"]["koff"] > 0, [where == "below"] * 3)
    assert np.array_equal(o2n, want["old_to_new"])
    holds_a = np.array([np.all(w["src"][w["off"][L]:w["off"][L + 1]] < len(A)) for L in range(P)])
    assert np.array_equal(np.flatnonzero(holds_a), o2n)
    # all frames, colour means, masks: the union's, in the union's leaf order (= key order)
    for k in FRAME_KEYS:
        assert g[k].tobytes() == w[k].tobytes(), k
        assert g[k][o2n].tobytes() == a[k].tobytes(), k
    # old leaves have empty batches; the new leaves hold the union's scan rows
    cnt = np.diff(g["off"])
    assert np.all(cnt[o2n] == 0)
    new_leaves = np.setdiff1d(np.arange(P), o2n)
    assert np.array_equal(cnt[new_leaves], np.diff(w["off"])[new_leaves]) and new.view.n_total == cnt.sum() > 0.9 * len(B)
    assert new.view.n_max == cnt.max()
    for L in new_leaves:
        s, t = slice(g["off"][L], g["off"][L + 1]), slice(w["off"][L], w["off"][L + 1])
        for k in ("x0", "x1", "y"):
            assert g[k][s].tobytes() == w[k][t].tobytes(), k
        assert np.ascontiguousarray(g["rgb"][:, s]).tobytes() == np.ascontiguousarray(w["rgb"][:, t]).tobytes()
        assert np.array_equal(g["src"][s] + len(A), w["src"][t])
    for o in (new, pt_ab, pt_a):
        o.close()


# ---- 2 ------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def overlap(gp):
    """the overlapping insertion, shared (read-only) by the tests below: model with leaves 0 and 6 untrained, min_nbr 20"""
    capi, ctx = gp
    m = Model(capi, ctx, untrained=(0, 6))
    S, cs = mc.overlapping_scan()
    new, o2n = m.pt.insert_cloud(ctx.make_cloud(S, cs), min_nbr=20, depth=m.gd)
    g = new.fetch()
    want = mr.insert(m.b, m.grid, m.trained, S, cs, 20, frames=g["R"])
    yield m, S, cs, new, o2n, g, want
    new.close()
    m.close()


def test_overlapping_scan_matches_the_restatement_exactly(gp, overlap, oracle):
    m, S, cs, new, o2n, g, want = overlap
    P = new.view.P
    assert P == len(want["cls"]) and P % 4 != 0 and P > m.P
    assert np.array_equal(o2n, want["old_to_new"])
    # the four combinations are in the case
    cls = want["cls"]
    assert cls[o2n[0]] == mr.FRESH and cls[o2n[6]] == mr.IDLE and np.all(cls[o2n[m.trained]] == mr.KEPT)
    assert cls[o2n[0]] == mr.FRESH and o2n[0] < o2n[1] and cls[o2n[1]] == mr.KEPT
    vox = {tuple(v) for v in want["vox"]}
    assert (6, 0, 0) in vox and (0, 6, 0) not in vox
    # owners and coordinates, exactly; every scan point owned at most once
    assert np.array_equal(g["off"], want["off"])
    assert len(np.unique(g["src"])) == len(g["src"]) == new.view.n_total
    assert np.array_equal(_owner_of(g, len(S)), want["owner"])
    assert np.all(want["owner"][-5:] == -1)
    for k in ("src", "x0", "x1", "y", "rgb", "mean", "rgb_mean", "W"):
        assert g[k].tobytes() == want[k].tobytes(), k
    # a point of the fresh leaf 0 that the kept leaf 1 accepts as well went to leaf 0
    L0, L1 = int(o2n[0]), int(o2n[1])
    p = S[g["src"][g["off"][L0]:g["off"][L0 + 1]]].astype(np.float64)
    d = p - (m.grid["mn"] + (np.array([1, 0, 0]) + 0.5) * RES)
    q = ref.local_coords(p, np.repeat(g["R"][L1][None], len(p), 0), np.repeat(g["mean"][L1][None], len(p), 0))
    assert np.any((np.sum(d * d, axis=1) <= m.grid["radius"] ** 2) & np.all(np.abs(q[:, 1:]) <= RES / 2, axis=1))
    # kept and idle leaves: the model's frames bit for bit; W is the OR; colours are minus the stored mean
    for i in range(m.P):
        L = o2n[i]
        sl = slice(g["off"][L], g["off"][L + 1])
        if cls[L] == mr.FRESH:
            continue
        for k in ("R", "mean", "rgb_mean"):
            assert g[k][L].tobytes() == m.b[k][i].tobytes(), (k, i)
        hit = np.zeros(SZ * SZ, np.uint8)
        gx = np.clip((SZ * (g["x0"][sl] / RES + 0.5)).astype(int), 0, SZ - 1)
        gy = np.clip((SZ * (g["x1"][sl] / RES + 0.5)).astype(int), 0, SZ - 1)
        hit[SZ * gx + gy] = 1
        assert np.array_equal(g["W"][L], m.b["W"][i] | hit)
        assert np.array_equal(g["rgb"][:, sl], (cs[g["src"][sl]].astype(np.float64) - m.b["rgb_mean"][i]).T)
    assert np.diff(g["off"])[o2n[6]] == 0
    # fresh frames: the oracle's compute_rotation of the same sums
    byo = mr.insert(m.b, m.grid, m.trained, S, cs, 20, compute_rotation=oracle.compute_rotation)
    fresh = np.flatnonzero(cls == mr.FRESH)
    assert len(fresh) >= 4 and np.max(np.abs(g["R"][fresh] - byo["R"][fresh])) <= 1e-12


# ---- 3 ------------------------------------------------------------------------------------------------------------------------------
def test_states_carry_over_and_training_matches_a_control_object(gp, overlap):
    import torch
    capi, ctx = gp
    m, S, cs, new, o2n, g, want = overlap
    P = new.view.P
    v = new.view
    rest = np.setdiff1d(np.arange(P), o2n)
    for old, kw, ny, plane, seed in ((m.gd, KW_D, 1, g["y"][None, :], 11), (m.gc, KW_C, 3, g["rgb"], 12)):
        moved = old.remap(P, o2n)
        assert moved.P == P and moved.ld() == old.ld()
        assert np.array_equal(moved.sizes()[o2n], old.sizes()) and np.all(moved.sizes()[rest] == 0)
        so, sm = old.state(), moved.state()
        for x, y in zip(so, sm):
            assert y[o2n].tobytes() == x.tobytes()
        for x, y in zip(so, old.state()):                                  # (old is untouched)
            assert x.tobytes() == y.tobytes()
        # control: the new P, filled from the remapped state, trained through the public host entry
        bv = moved.sizes()
        ctl = capi.Sparse(ctx, capi.default_params_sparse(ny, **kw), P, ny)
        al, Cm, Q, BV = sm
        for a in (al, Cm, Q, BV):
            a[rest] = 0.0
        ctl.set_state(bv, al, BV, Cm, Q)
        perm = synth.sattolo_perms(g["off"], seed=seed)
        d_perm = torch.from_numpy(perm).cuda()
        st = torch.full((P,), -1, dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()
        moved.add_dev(v.off, v.n_max, v.n_total, v.x0, v.x1, v.y if ny == 1 else v.rgb, d_perm, st)
        ctx.synchronize()
        st_c = ctl.add(g["off"], g["x0"], g["x1"], np.ascontiguousarray(plane), perm)
        assert np.array_equal(st.cpu().numpy(), st_c) and np.all(st_c == 0)
        assert np.array_equal(moved.sizes(), ctl.sizes())
        assert moved.sizes().max() == kw["capacity"] and np.diff(g["off"]).max() > kw["capacity"]      # deletions happened
        for name, x, y in zip(("alpha", "C", "Q", "BV"), moved.state(), ctl.state()):
            b_ = moved.sizes()
            for i in range(P):                                             # the live part of every patch
                bb = int(b_[i])
                xs = x[i][:, :bb] if name == "alpha" else (x[i][:bb] if name == "BV" else x[i][:bb, :bb])
                ys = y[i][:, :bb] if name == "alpha" else (y[i][:bb] if name == "BV" else y[i][:bb, :bb])
                assert xs.tobytes() == ys.tobytes(), (name, i)
        ctl.close()
        moved.close()
    # bad tables
    L = ctx.lib
    h = C.c_void_p()
    for bad in (o2n[::-1].copy(), np.concatenate([o2n[:-1], [P]]).astype(np.int32), np.concatenate([[0, 0], o2n[2:]]).astype(np.int32)):
        assert L.gpc_sparse_remap(m.gd.h, P, bad.ctypes.data, C.byref(h)) == capi.GPC_EINVAL and h.value is None
    assert L.gpc_sparse_remap(m.gd.h, m.P - 1, o2n.ctypes.data, C.byref(h)) == capi.GPC_EINVAL
    assert L.gpc_sparse_remap(m.gd.h, P, None, C.byref(h)) == capi.GPC_EINVAL


# ---- 4 ------------------------------------------------------------------------------------------------------------------------------
def test_registration_on_the_grown_map(gp):
    capi, ctx = gp
    m = Model(capi, ctx, kw_c=KW_C_REG)
    A, ca = m.xyz, m.rgb
    B, cb = mc.disjoint_scan("below")                                      # the origin shifts on every axis
    new, o2n = m.pt.insert_cloud(ctx.make_cloud(B, cb), min_nbr=1, depth=m.gd)
    g = new.fetch()
    P = new.view.P
    want = mr.insert(m.b, m.grid, m.trained, B, cb, 1, frames=g["R"])
    assert np.all(want["grid"]["koff"] > 0)
    gd, gc = m.gd.remap(P, o2n), m.gc.remap(P, o2n)
    # the model's own points find the frames they found before the insertion
    zero = capi.default_params_registration(step=0.0)
    before, after = m.capi.Registration(ctx, m.pt, m.gd, m.gc), capi.Registration(ctx, new, gd, gc)
    for r in (before, after):
        r.set_cloud(ctx.make_cloud(A, ca))
        r.step(zero)
    (ob, lb), (oa, la) = before.assignment(), after.assignment()
    assert np.array_equal(oa, np.where(ob >= 0, o2n[np.maximum(ob, 0)], -1)) and la.tobytes() == lb.tobytes()
    assert np.sum(ob >= 0) > 0.9 * len(A)
    before.close()
    # train the new leaves, then one step of a moved copy of the whole map against the restatement on the GPU's own state
    v = new.view
    gd.add_dev(v.off, v.n_max, v.n_total, v.x0, v.x1, v.y)
    gc.add_dev(v.off, v.n_max, v.n_total, v.x0, v.x1, v.rgb)
    ctx.synchronize()
    trained = gd.sizes() > 0
    assert trained.all()
    lik_d, lik_c = _callbacks(((gd, KW_D), (gc, KW_C_REG)))
    xyz = (np.concatenate([A, B]).astype(np.float64) + np.array([0.004, -0.003, 0.002])).astype(np.float32)
    rgb = np.concatenate([ca, cb])
    rgrid = mr.registration_grid(want["grid"])
    ow, lw = ref.assign(xyz, g, rgrid, trained)
    r0 = ref.reduce_step(rgb, ow, lw, g, lik_d, lik_c)
    assert r0["n_used"] > 0.5 * len(xyz) and np.all(np.isfinite(r0["delta"])) and np.max(np.abs(r0["delta"])) > 0
    assert np.sum(np.isin(ow, np.setdiff1d(np.arange(P), o2n))) > 0.5 * len(B)          # the new leaves take part
    after.set_cloud(ctx.make_cloud(xyz, rgb))
    out = after.step(capi.default_params_registration(step=0.002 / float(np.max(np.abs(r0["delta"])))))
    owner, local = after.assignment()
    assert np.array_equal(owner, ow) and np.max(np.abs(local - lw)) <= 1e-12 * RES
    assert out[8] == r0["n_used"]
    assert np.all(np.abs(out[:6] - r0["delta"]) <= 1e-8 * r0["gabs"])
    assert abs(out[6] - r0["ls"]) <= 1e-8 * abs(r0["ls"]) and abs(out[7] - r0["cls"]) <= 1e-8 * abs(r0["cls"])
    # the working cloud as a device pointer
    d_cloud, n = after.cloud_dev()
    assert n == len(xyz) and d_cloud != 0
    for o in (after, gd, gc, new):
        o.close()
    m.close()


def test_mapping_add_cloud_inserts_or_drops(gp):
    capi, ctx = gp
    m = Model(capi, ctx, kw_c=KW_C_REG)
    S, cs = mc.overlapping_scan()
    prm = capi.default_params_registration(step=1e-7, tol=1e300, min_steps=2, max_steps=10)
    mp = capi.Mapping(ctx, m.pt, m.gd, m.gc, params=prm, min_nbr=20)
    steps, inserted = mp.add_cloud(ctx.make_cloud(S, cs))
    assert (steps, inserted) == (3, True)
    P1 = mp.patches.view.P
    assert P1 > m.P and mp.depth.P == mp.rgb.P == P1 and m.pt.h is None and m.gd.h is None
    assert np.sum(mp.depth.sizes() > 0) > m.P
    # the loop runs into max_steps: the scan is dropped, the map stays
    mp.params = capi.default_params_registration(step=1e-7, tol=1e300, min_steps=0, max_steps=1)
    pt_before = mp.patches
    steps, inserted = mp.add_cloud(ctx.make_cloud(S + np.float32(0.001), cs))
    assert (steps, inserted) == (1, False) and mp.patches is pt_before and mp.patches.view.P == P1
    # and the grown map takes another scan
    mp.params = prm
    steps, inserted = mp.add_cloud(ctx.make_cloud(S + np.float32(0.002), cs))
    assert inserted and mp.patches.view.P >= P1
    mp.close()


# ---- 5 ------------------------------------------------------------------------------------------------------------------------------
def test_insertion_contract(gp, overlap):
    import torch
    capi, ctx = gp
    L = ctx.lib
    m, S, cs, new, o2n, g, want = overlap
    scan = ctx.make_cloud(S, cs)
    # a repeat call, from a device buffer: identical bits
    d_scan = torch.from_numpy(scan.view(np.uint8).reshape(-1, 32)).cuda()
    torch.cuda.synchronize()
    again, o2n2 = m.pt.insert_cloud(d_scan, min_nbr=20, depth=m.gd, n=len(scan))
    g2 = again.fetch()
    assert np.array_equal(o2n, o2n2)
    for k in g:
        assert g[k].tobytes() == g2[k].tobytes(), k
    # n = 0: a copy of the model, old_to_new the identity
    empty, ident = m.pt.insert_cloud(ctx.make_cloud(np.zeros((0, 3)), np.zeros((0, 3))), min_nbr=20, depth=m.gd)
    e = empty.fetch()
    assert np.array_equal(ident, np.arange(m.P)) and empty.view.P == m.P and empty.view.n_total == 0 and np.all(e["off"] == 0)
    for k in FRAME_KEYS:
        assert e[k].tobytes() == m.b[k].tobytes(), k
    # a scan wholly inside kept leaves: P' = P, every point where the registration assignment puts it
    A, ca = m.xyz, m.rgb
    inside = np.flatnonzero(_owner_of(m.b, len(A)) == 4)[:100]
    same, ident = m.pt.insert_cloud(ctx.make_cloud(A[inside], ca[inside]), min_nbr=1000, depth=m.gd)
    s = same.fetch()
    assert same.view.P == m.P and np.array_equal(ident, np.arange(m.P))
    ow, lw = ref.assign(A[inside], m.b, m.grid, m.trained)
    assert np.array_equal(_owner_of(s, len(inside)), ow) and np.sum(ow >= 0) > 50
    assert np.array_equal(s["y"], lw[s["src"], 0]) and np.array_equal(s["x0"], lw[s["src"], 1])
    # the old objects still answer as before
    b2 = m.pt.fetch()
    for k in m.b:
        assert m.b[k].tobytes() == b2[k].tobytes(), k
    # bad arguments
    h = C.c_void_p()
    tab = np.zeros(m.P, np.int32)

    def call(c, model, depth, cloud, n, min_nbr=20):
        return L.gpc_patches_insert_cloud(c, model, depth, cloud, n, min_nbr, C.byref(h), tab.ctypes.data)
    bad = scan.copy()
    bad["y"][7] = np.nan
    assert call(ctx.h, m.pt.h, m.gd.h, bad.ctypes.data, len(bad)) == capi.GPC_EINVAL
    bad["y"][7] = np.inf
    assert call(ctx.h, m.pt.h, m.gd.h, bad.ctypes.data, len(bad)) == capi.GPC_EINVAL
    far = scan.copy()
    far["x"][3] = 1e9
    assert call(ctx.h, m.pt.h, m.gd.h, far.ctypes.data, len(far)) == capi.GPC_ERANGE
    ctx2 = capi.Context(0)
    other = capi.Sparse(ctx2, capi.default_params_sparse(1, **KW_D), m.P, 1)
    assert call(ctx.h, m.pt.h, other.h, scan.ctypes.data, len(scan)) == capi.GPC_EINVAL          # depth of another context
    assert call(ctx2.h, m.pt.h, other.h, scan.ctypes.data, len(scan)) == capi.GPC_EINVAL         # model of another context
    other.close()
    ctx2.close()
    wrong = capi.Sparse(ctx, capi.default_params_sparse(1, **KW_D), m.P + 1, 1)
    assert call(ctx.h, m.pt.h, wrong.h, scan.ctypes.data, len(scan)) == capi.GPC_EINVAL          # another P
    wrong.close()
    assert call(ctx.h, m.pt.h, m.gc.h, scan.ctypes.data, len(scan)) == capi.GPC_EINVAL           # the colour GP is no depth GP
    assert call(ctx.h, None, m.gd.h, scan.ctypes.data, len(scan)) == capi.GPC_EINVAL
    assert call(ctx.h, m.pt.h, m.gd.h, None, 5) == capi.GPC_EINVAL
    assert call(ctx.h, m.pt.h, m.gd.h, scan.ctypes.data, -1) == capi.GPC_EINVAL
    assert call(ctx.h, m.pt.h, m.gd.h, scan.ctypes.data, len(scan), min_nbr=0) == capi.GPC_EINVAL
    assert L.gpc_patches_insert_cloud(ctx.h, m.pt.h, m.gd.h, scan.ctypes.data, len(scan), 20, None, tab.ctypes.data) == capi.GPC_EINVAL
    assert L.gpc_patches_insert_cloud(ctx.h, m.pt.h, m.gd.h, scan.ctypes.data, len(scan), 20, C.byref(h), None) == capi.GPC_EINVAL
    assert h.value is None
    # destroy orders are free: a new object outlives its model, and the other way round
    for first in ("model", "result"):
        pt = ctx.project_cloud(ctx.make_cloud(A, ca), RES, SZ)
        res, _ = pt.insert_cloud(scan, min_nbr=20)
        (pt if first == "model" else res).close()
        survivor = res if first == "model" else pt
        assert survivor.fetch()["R"].shape[0] == survivor.view.P
        survivor.close()
    for o in (again, empty, same):
        o.close()
