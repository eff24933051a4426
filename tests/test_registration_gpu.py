"""GPU tests of gpc_registration (SURVEY section 8 row f: gp_registration, /root/reference/src/gp_registration.cpp): the step's stages
against the NumPy restatement (tests/registration_ref.py) evaluated on the GPU's own GP state, one step end to end against the CPU
oracle, ownership against the producer, reproducibility, the loop, and the object's contract.

Bounds: owners are exact (the assignment kernel evaluates the restatement's expressions in its association, contraction off);
delta / ls / cls carry the bounds of test_sparse_likelihood_and_derivatives (1e-8 on the GPU's own state, 1e-4 against the oracle's
state), delta measured against the mean absolute per-point contribution sum |g| / n_used, because the sum itself cancels."""
import ctypes as C

import numpy as np
import pytest

from gp_compressor_amd import synth
import registration_ref as ref

pytestmark = pytest.mark.gpu

RES, SZ = 0.15, 20
KW_D = dict(sigmaf_sq=1.0, l_sq=(RES / 5) ** 2, noise=1e-3, capacity=24)
# (colour capacity 100, the reference's default: with a basis of a dozen vectors the colour residuals are tens of grey levels, cl
# underflows to 0 at noise 1.0 and with it the whole gradient l dCX + cl dX -- nothing would be compared)
KW_C = dict(sigmaf_sq=1.0, l_sq=(RES / 5) ** 2, noise=1.0, capacity=100)


@pytest.fixture(scope="module")
def gp():
    from gp_compressor_amd import capi
    capi.load()
    ctx = capi.Context(0)
    yield capi, ctx
    ctx.close()


def _xyz(cloud):
    return np.stack([cloud["x"], cloud["y"], cloud["z"]], 1)


def _rgb(cloud):
    return np.stack([cloud["r"], cloud["g"], cloud["b"]], 1)


class Model:
    """model cloud -> producer -> depth + colour sparse GPs; the patches in `untrained` get no points (b == 0)"""

    def __init__(self, capi, ctx, xyz, rgb, untrained=(), seed=6):
        self.capi, self.ctx, self.xyz, self.rgb = capi, ctx, xyz, rgb
        self.pt = ctx.project_cloud(ctx.make_cloud(xyz, rgb), RES, SZ)
        self.b = b = self.pt.fetch()
        self.P = P = self.pt.view.P
        off = b["off"]
        cnt = np.diff(off)
        cnt[list(untrained)] = 0
        self.keep = keep = np.concatenate([np.arange(off[i], off[i] + cnt[i]) for i in range(P)]).astype(np.int64)
        self.off_t = np.concatenate([[0], np.cumsum(cnt)]).astype(np.int32)
        self.perm = synth.sattolo_perms(self.off_t, seed=seed)
        self.gd = capi.Sparse(ctx, capi.default_params_sparse(1, **KW_D), P, 1)
        self.gc = capi.Sparse(ctx, capi.default_params_sparse(3, **KW_C), P, 3)
        st_d = self.gd.add(self.off_t, b["x0"][keep], b["x1"][keep], b["y"][None, keep], self.perm)
        st_c = self.gc.add(self.off_t, b["x0"][keep], b["x1"][keep], np.ascontiguousarray(b["rgb"][:, keep]), self.perm)
        assert np.all(st_d == 0) and np.all(st_c == 0)
        self.sizes = self.gd.sizes()
        self.trained = self.sizes > 0
        assert np.array_equal(self.trained, cnt > 0)
        self.grid = ref.grid_of(xyz, RES)
        assert len(self.grid["keys"]) == P

    def callbacks(self):
        """the closed-form likelihood on the GPU's own states"""
        out = []
        for g, kw in ((self.gd, KW_D), (self.gc, KW_C)):
            alpha, Cm, _, BV = g.state()
            sizes = g.sizes()

            def f(i, x0, x1, y, alpha=alpha, Cm=Cm, BV=BV, sizes=sizes, kw=kw):
                bb = int(sizes[i])
                return ref.closed_form_likelihood(kw["sigmaf_sq"], kw["l_sq"], kw["noise"], alpha[i][:, :bb], Cm[i][:bb, :bb], BV[i][:bb],
                                                  x0, x1, y)
            out.append(f)
        return out

    def registration(self):
        return self.capi.Registration(self.ctx, self.pt, self.gd, self.gc)

    def close(self):
        for o in (self.gd, self.gc, self.pt):
            o.close()


def _perturbed(xyz):
    a = 0.01
    Rz = np.array([[np.cos(a), -np.sin(a), 0], [np.sin(a), np.cos(a), 0], [0, 0, 1]])
    return ((xyz.astype(np.float64) - 0.6) @ Rz.T + 0.6 + np.array([0.004, -0.003, 0.002])).astype(np.float32)


def _close_rel(got, want, scale, tol):
    assert np.all(np.abs(np.asarray(got) - np.asarray(want)) <= tol * np.asarray(scale)), (got, want, scale)


@pytest.mark.parametrize("kind", ["plane", "room"])
def test_registration_step_matches_the_restatement(gp, kind):
    capi, ctx = gp
    if kind == "plane":
        xyz, rgb = synth.plane_cloud(10000, seed=1)
    else:
        xyz, rgb = synth.room_cloud(40000, seed=3, size=(2.0, 1.5, 1.0))
    m = Model(capi, ctx, xyz, rgb, untrained=(3, 7, 20))
    assert m.trained.sum() >= 0.8 * m.P and not m.trained[3]
    lik_d, lik_c = m.callbacks()
    scan = ctx.make_cloud(_perturbed(xyz), rgb)
    # the step length: about 2 mm of motion per step, from the restatement's own first gradient
    o0, l0 = ref.assign(_xyz(scan), m.b, m.grid, m.trained)
    r0 = ref.reduce_step(rgb, o0, l0, m.b, lik_d, lik_c)
    assert r0["n_used"] > 0.5 * len(xyz) and np.all(np.isfinite(r0["delta"])) and np.max(np.abs(r0["delta"])) > 0
    for ref_sum in (1, 0):
        prm = capi.default_params_registration(step=0.002 / float(np.max(np.abs(r0["delta"]))), ref_translation_sum=ref_sum)
        reg = m.registration()
        reg.set_cloud(scan)
        R0, t0 = reg.transform()
        assert np.array_equal(R0, np.eye(3)) and np.array_equal(t0, np.zeros(3))
        Rc, tc = np.eye(3), np.zeros(3)
        for k in range(5):
            before = reg.cloud()
            assert np.array_equal(_rgb(before), rgb)
            out = reg.step(prm)
            owner, local = reg.assignment()
            ow, lw = ref.assign(_xyz(before), m.b, m.grid, m.trained)
            assert np.array_equal(owner, ow), int(np.sum(owner != ow))                 # exact, no exclusions
            assert np.max(np.abs(local - lw)) <= 1e-12 * RES
            assert not np.any(np.isin(owner, [3, 7, 20]))
            want = ref.reduce_step(rgb, ow, lw, m.b, lik_d, lik_c)
            assert out[8] == want["n_used"] == int(np.sum(owner >= 0))
            _close_rel(out[:6], want["delta"], want["gabs"], 1e-8)
            _close_rel(out[6], want["ls"], abs(want["ls"]), 1e-8)
            _close_rel(out[7], want["cls"], abs(want["cls"]), 1e-8)
            # the update, from the delta the GPU reported
            R, t = ref.gradient_step(out[:6], prm.step)
            Rc, tc = ref.update_pose(Rc, tc, R, t, bool(ref_sum))
            Rg, tg = reg.transform()
            assert np.max(np.abs(Rg - Rc)) <= 1e-12 and np.max(np.abs(tg - tc)) <= 1e-12
            after = _xyz(reg.cloud())
            moved = ref.transform_cloud(_xyz(before), R, t)
            assert np.all(np.abs(after - moved) <= np.spacing(np.maximum(np.abs(after), np.abs(moved))))    # 1 float ulp
            assert np.max(np.abs(after - _xyz(before))) > 0
        reg.close()
    m.close()


def test_reduce_loop_wraps_over_identical_copies(gp):
    """rg_reduce_kernel runs at most 8 workgroups per CU and strides over the used points: with more than 8 * CUs * 256 of them its loop
    takes a second trip.  The scan is k copies of one 10 000-point scan, so the restatement is evaluated on ONE copy: every copy's points
    get the same owners, n_used is k times the copy's, and the means over k identical copies are the copy's means -- a dropped or doubled
    stride moves n_used or a mean by at least 1 / k of itself."""
    import torch
    capi, ctx = gp
    xyz, rgb = synth.plane_cloud(10000, seed=1)
    m = Model(capi, ctx, xyz, rgb, untrained=(3, 7, 20))
    lik_d, lik_c = m.callbacks()
    one = _perturbed(xyz)
    ow, lw = ref.assign(one, m.b, m.grid, m.trained)
    want = ref.reduce_step(rgb, ow, lw, m.b, lik_d, lik_c)
    assert want["n_used"] > 0.5 * len(xyz) and np.max(np.abs(want["delta"])) > 0
    wrap = 8 * torch.cuda.get_device_properties(0).multi_processor_count * 256
    k = wrap // want["n_used"] + 2
    assert (k - 1) * want["n_used"] > wrap                                             # the last copy lies wholly in the second trip
    reg = m.registration()
    reg.set_cloud(ctx.make_cloud(np.tile(one, (k, 1)), np.tile(rgb, (k, 1))))
    out = reg.step(capi.default_params_registration(step=0.0))
    owner, local = reg.assignment()
    owner, local = owner.reshape(k, len(one)), local.reshape(k, len(one), 3)
    assert np.array_equal(owner[0], ow) and np.max(np.abs(local[0] - lw)) <= 1e-12 * RES
    for j in range(1, k):
        assert np.array_equal(owner[j], owner[0]) and local[j].tobytes() == local[0].tobytes(), j
    assert out[8] == k * want["n_used"]
    _close_rel(out[:6], want["delta"], want["gabs"], 1e-8)
    _close_rel(out[6], want["ls"], abs(want["ls"]), 1e-8)
    _close_rel(out[7], want["cls"], abs(want["cls"]), 1e-8)
    reg.close()
    m.close()


def test_registration_step_end_to_end_against_the_oracle(gp, oracle):
    capi, ctx = gp
    xyz, rgb = synth.plane_cloud(10000, seed=1)
    m = Model(capi, ctx, xyz, rgb, untrained=(3, 7))
    ob = oracle.project_cloud(xyz, rgb, RES, SZ)
    gos = []
    for kw, ny, plane in ((KW_D, 1, ob["y"][None, :]), (KW_C, 3, ob["rgb"])):
        op = oracle.sparse_params(ny, p0=kw["sigmaf_sq"], p1=kw["l_sq"], s20=kw["noise"], capacity=kw["capacity"])
        gs = []
        for i in range(m.P):
            go = oracle.Sparse(op, kw["capacity"] + 2)
            a, b_ = m.off_t[i], m.off_t[i + 1]
            if b_ > a:
                sl = slice(ob["off"][i], ob["off"][i] + (b_ - a))
                go.add_measurements(ob["x0"][sl], ob["x1"][sl], np.ascontiguousarray(plane[:, sl]), m.perm[a:b_])
            gs.append(go)
        gos.append(gs)
    trained = np.array([g.size() > 0 for g in gos[0]])
    assert np.array_equal(trained, m.trained)
    scan_xyz = _perturbed(xyz)
    ow, lw = ref.assign(scan_xyz, ob, ref.grid_of(xyz, RES), trained)
    want = ref.reduce_step(rgb, ow, lw, ob, lambda i, x0, x1, y: gos[0][i].likelihood(x0, x1, y),
                           lambda i, x0, x1, y: gos[1][i].likelihood(x0, x1, y))
    reg = m.registration()
    reg.set_cloud(ctx.make_cloud(scan_xyz, rgb))
    out = reg.step(capi.default_params_registration(step=1e-9))
    assert out[8] == want["n_used"] > 0
    _close_rel(out[:6], want["delta"], want["gabs"], 1e-4)
    _close_rel(out[6], want["ls"], abs(want["ls"]), 1e-4)
    _close_rel(out[7], want["cls"], abs(want["cls"]), 1e-4)
    reg.close()
    m.close()


def test_self_registration_reproduces_the_producers_ownership(gp):
    capi, ctx = gp
    xyz, rgb = synth.plane_cloud(10000, seed=1)
    m = Model(capi, ctx, xyz, rgb)
    want = np.full(len(xyz), -1, dtype=np.int32)
    for i in range(m.P):
        want[m.b["src"][m.b["off"][i]:m.b["off"][i + 1]]] = i
    reg = m.registration()
    reg.set_cloud(ctx.make_cloud(xyz, rgb))
    reg.step(capi.default_params_registration(step=0.0))
    owner, _ = reg.assignment()
    differ = np.flatnonzero(owner != want)
    p = xyz.astype(np.float64)
    for i in differ:                                   # the shifted mean rounds differently from the voxel centre on a window's edge
        edge = False
        for L in (owner[i], want[i]):
            if L >= 0:
                q = ref.local_coords(p[i:i + 1], m.b["R"][L:L + 1], m.b["mean"][L:L + 1])[0]
                edge = edge or bool(np.any(np.abs(np.abs(q[1:]) - RES / 2) <= 1e-9 * RES))
        assert edge, (int(i), int(owner[i]), int(want[i]))
    assert len(differ) <= 10, len(differ)
    # a zero step leaves cloud and pose where they were
    assert np.array_equal(_xyz(reg.cloud()), xyz)
    Rg, tg = reg.transform()
    assert np.array_equal(Rg, np.eye(3)) and np.array_equal(tg, np.zeros(3))
    reg.close()
    m.close()


def test_registration_is_reproducible_bit_for_bit(gp):
    import torch
    capi, ctx = gp
    xyz, rgb = synth.room_cloud(40000, seed=3, size=(2.0, 1.5, 1.0))
    m = Model(capi, ctx, xyz, rgb, untrained=(5,))
    scan = ctx.make_cloud(_perturbed(xyz), rgb)
    prm = capi.default_params_registration(step=1e-7)
    res = []
    for dev in (False, True):                          # the second object takes the scan from a device buffer
        reg = m.registration()
        if dev:
            d_scan = torch.from_numpy(scan.view(np.uint8).reshape(-1, 32)).cuda()
            torch.cuda.synchronize()
            reg.set_cloud(d_scan, n=len(scan))
        else:
            reg.set_cloud(scan)
        outs = [reg.step(prm) for _ in range(3)]
        res.append((np.stack(outs), reg.cloud(), *reg.transform()))
        reg.close()
    for a, b in zip(*res):
        assert a.tobytes() == b.tobytes()
    assert np.all(np.isfinite(res[0][0])) and res[0][0][0, 8] > 0.5 * len(xyz)
    m.close()


def test_likelihood_drops_when_the_scan_leaves_the_surface(gp):
    capi, ctx = gp
    xyz, rgb = synth.plane_cloud(10000, seed=1)
    m = Model(capi, ctx, xyz, rgb)
    reg = m.registration()
    prm = capi.default_params_registration(step=0.0)
    reg.set_cloud(ctx.make_cloud(xyz, rgb))
    at_home = reg.step(prm)
    shifted = xyz.copy()
    shifted[:, 2] += np.float32(0.3 * RES)             # along the plane's normal, well beyond sqrt(noise) = 0.03
    reg.set_cloud(ctx.make_cloud(shifted, rgb))
    away = reg.step(prm)
    assert at_home[8] > 0.9 * len(xyz) and away[8] > 0.5 * len(xyz)
    assert at_home[6] > away[6] > 0.0
    reg.close()
    m.close()


def test_registration_run_follows_the_stopping_rule(gp):
    capi, ctx = gp
    xyz, rgb = synth.plane_cloud(10000, seed=1)
    m = Model(capi, ctx, xyz, rgb, untrained=(3,))
    scan = ctx.make_cloud(_perturbed(xyz), rgb)
    # never converged (tol 0): max_steps ends the loop
    prm = capi.default_params_registration(step=1e-7, tol=0.0, min_steps=2, max_steps=5)
    reg, hand = m.registration(), m.registration()
    reg.set_cloud(scan)
    hand.set_cloud(scan)
    trace = reg.run(prm)
    assert trace.shape == (5, 9)
    by_hand = np.stack([hand.step(prm) for _ in range(5)])
    assert trace.tobytes() == by_hand.tobytes()
    assert reg.cloud().tobytes() == hand.cloud().tobytes()
    for s in range(1, 6):
        assert ref.registration_done(s, trace[s - 1, :6], 0.0, 2, 5) == (s == 5)
    # always converged (tol huge): the first step past min_steps ends it; set_cloud restarts the count
    prm2 = capi.default_params_registration(step=1e-7, tol=1e300, min_steps=3, max_steps=50)
    reg.set_cloud(scan)
    assert len(reg.run(prm2)) == 4
    # the count carries over between calls: one more step is past min_steps already
    assert len(reg.run(prm2)) == 1
    # the defaults are the reference's constants
    d = capi.default_params_registration()
    assert (d.step, d.tol, d.min_steps, d.max_steps, d.ref_translation_sum) == (float(np.float32(1e-1)), 0.1, 10, 300, 1)
    reg.close()
    hand.close()
    m.close()


def test_registration_edge_cases(gp):
    capi, ctx = gp
    xyz, rgb = synth.plane_cloud(5000, seed=2)
    m = Model(capi, ctx, xyz, rgb)
    prm = capi.default_params_registration()
    reg = m.registration()
    zeros = np.zeros(9)
    # no scan at all, an empty scan
    assert np.array_equal(reg.step(prm), zeros)
    reg.set_cloud(ctx.make_cloud(np.zeros((0, 3)), np.zeros((0, 3))))
    assert np.array_equal(reg.step(prm), zeros) and len(reg.cloud()) == 0
    # a scan wholly outside the model's grid (and a non-finite coordinate in it)
    far = xyz + np.float32(100.0)
    far[0, 1] = np.nan
    reg.set_cloud(ctx.make_cloud(far, rgb))
    assert np.array_equal(reg.step(prm), zeros)
    owner, local = reg.assignment()
    assert np.all(owner == -1) and np.all(local == 0.0)
    Rg, tg = reg.transform()
    assert np.array_equal(Rg, np.eye(3)) and np.array_equal(tg, np.zeros(3))
    assert np.array_equal(_xyz(reg.cloud())[1:], far[1:])
    reg.close()
    # no trained leaf
    e_d = capi.Sparse(ctx, capi.default_params_sparse(1, **KW_D), m.P, 1)
    e_c = capi.Sparse(ctx, capi.default_params_sparse(3, **KW_C), m.P, 3)
    reg = capi.Registration(ctx, m.pt, e_d, e_c)
    reg.set_cloud(ctx.make_cloud(xyz, rgb))
    assert np.array_equal(reg.step(prm), zeros) and np.all(reg.assignment()[0] == -1)
    reg.close()
    # an empty model
    pt0 = ctx.project_cloud(ctx.make_cloud(np.zeros((0, 3)), np.zeros((0, 3))), RES, SZ)
    z_d = capi.Sparse(ctx, capi.default_params_sparse(1, **KW_D), 0, 1)
    z_c = capi.Sparse(ctx, capi.default_params_sparse(3, **KW_C), 0, 3)
    reg = capi.Registration(ctx, pt0, z_d, z_c)
    reg.set_cloud(ctx.make_cloud(xyz, rgb))
    assert np.array_equal(reg.step(prm), zeros) and np.all(reg.assignment()[0] == -1)
    reg.close()
    for o in (e_d, e_c, z_d, z_c, pt0):
        o.close()
    m.close()


def test_registration_argument_checks_and_ownership(gp):
    capi, ctx = gp
    L = ctx.lib
    xyz, rgb = synth.plane_cloud(5000, seed=2)
    m = Model(capi, ctx, xyz, rgb)
    h = C.c_void_p()

    def create(c, pt, gd, gc):
        return L.gpc_registration_create(c, pt, gd, gc, C.byref(h))
    assert create(ctx.h, m.pt.h, m.gc.h, m.gd.h) == capi.GPC_EINVAL                 # ny the wrong way round
    assert create(ctx.h, m.pt.h, m.gd.h, m.gd.h) == capi.GPC_EINVAL
    other = capi.Sparse(ctx, capi.default_params_sparse(1, **KW_D), m.P + 1, 1)
    assert create(ctx.h, m.pt.h, other.h, m.gc.h) == capi.GPC_EINVAL                # P mismatch
    other.close()
    probit = capi.Sparse(ctx, capi.default_params_sparse(1, noise_model=2, **KW_D), m.P, 1)
    assert create(ctx.h, m.pt.h, probit.h, m.gc.h) == capi.GPC_EINVAL               # the likelihoods are Gaussian
    probit.close()
    for args in ((None, m.gd.h, m.gc.h), (m.pt.h, None, m.gc.h), (m.pt.h, m.gd.h, None)):
        assert create(ctx.h, *args) == capi.GPC_EINVAL
    assert L.gpc_registration_create(ctx.h, m.pt.h, m.gd.h, m.gc.h, None) == capi.GPC_EINVAL
    assert L.gpc_registration_create(None, m.pt.h, m.gd.h, m.gc.h, C.byref(h)) == capi.GPC_EINVAL
    ctx2 = capi.Context(0)
    assert create(ctx2.h, m.pt.h, m.gd.h, m.gc.h) == capi.GPC_EINVAL                # objects of a foreign context
    assert h.value is None
    out = np.zeros(9)
    prm = capi.default_params_registration()
    assert L.gpc_registration_step(None, C.byref(prm), out.ctypes.data) == capi.GPC_EINVAL
    L.gpc_registration_destroy(None)
    reg = m.registration()
    assert L.gpc_registration_step(reg.h, None, out.ctypes.data) == capi.GPC_EINVAL
    assert L.gpc_registration_step(reg.h, C.byref(prm), None) == capi.GPC_EINVAL
    assert L.gpc_registration_set_cloud(reg.h, None, 5) == capi.GPC_EINVAL
    assert L.gpc_registration_set_cloud(reg.h, None, -1) == capi.GPC_EINVAL
    bad = capi.default_params_registration(max_steps=0)
    assert L.gpc_registration_run(reg.h, C.byref(bad), None, None) == capi.GPC_EINVAL
    # create / destroy many times: the context's reference count comes back (the context is freed with its last child)
    for _ in range(50):
        capi.Registration(ctx, m.pt, m.gd, m.gc).close()
    # a parent goes first: every call reports, destroy still works
    reg.set_cloud(ctx.make_cloud(xyz, rgb))
    assert reg.step(prm)[8] > 0
    m.gc.close()
    for call in (lambda: reg.step(prm), lambda: reg.run(prm), reg.transform, reg.cloud, reg.assignment,
                 lambda: reg.set_cloud(ctx.make_cloud(xyz, rgb))):
        with pytest.raises(capi.GpcError) as e:
            call()
        assert e.value.code == capi.GPC_EINVAL
    # an object at the same address is not the one that went
    again = capi.Sparse(ctx, capi.default_params_sparse(3, **KW_C), m.P, 3)
    with pytest.raises(capi.GpcError):
        reg.step(prm)
    again.close()
    reg.close()
    # the context goes first, then the registration object, then its parents -- and the other way round
    for order in ("reg_first", "parents_first"):
        xyz2, rgb2 = synth.plane_cloud(2000, seed=4)
        m2 = Model(capi, ctx2, xyz2, rgb2)
        reg2 = m2.registration()
        reg2.set_cloud(ctx2.make_cloud(xyz2, rgb2))
        assert reg2.step(prm)[8] > 0
        handle = ctx2.h
        ctx2.h = None                                   # (Context.close would close the children first)
        L.gpc_ctx_destroy(handle)
        assert L.gpc_registration_step(reg2.h, C.byref(prm), out.ctypes.data) == capi.GPC_EINVAL
        if order == "reg_first":
            reg2.close()
            m2.close()
        else:
            m2.close()
            reg2.close()
        ctx2 = capi.Context(0)
    ctx2.close()
    m.gd.close()
    m.pt.close()
