"""GPU tests of the render attributes (gpc_patches_render_attrs[_dev]; include/gpc.h): the predictive sigma and the world normal at
the hits of a render.  Scene and model: the two-sheet cloud of tests/raycast_cases.py cut by the producer, the small images of
render_cases.POSES, and handmade depth states of every basis size (render_attrs_cases.depth_batch: C = -(K_BV + s20 I)^-1, surfaces a
centimetre from their planes).  Bounds: tests/render_attrs_cases.py (derived there, shown to hold for the float64 restatement alone by
tests/test_render_attrs_cpu.py); the references are evaluated in np.longdouble on the GPU's own frames (Patches.fetch)."""
import numpy as np
import pytest

import mapping_cases as mc
import raycast_cases as rcs
import readout_cases as RC
import render_attrs_cases as ac
import render_cases as rc
import render_ref as rn

pytestmark = pytest.mark.gpu
LD = ac.LD
RES, SZ = ac.RES, ac.SZ
MIN_NBR = 20
KW_C = dict(sigmaf_sq=1.0, l_sq=(RES / 5) ** 2, noise=1.0, capacity=100)
WANT = ("leaf", "local", "sigma", "normal")


@pytest.fixture(scope="module")
def gp():
    from gp_compressor_amd import capi
    capi.load()
    ctx = capi.Context(0)
    yield capi, ctx
    ctx.close()


def _depth(capi, ctx, B):
    g = capi.Sparse(ctx, capi.default_params_sparse(1, **ac.KW_DEPTH), B["P"], 1)
    assert g.ld() == B["ld"]
    g.set_state(B["b"], B["alpha"], B["BV"], B["C"], None)
    return g


@pytest.fixture(scope="module")
def model(gp):
    """the model cloud cut by the producer, the handmade depth states loaded -- shared, read-only -- and per pose the render with
    every attribute"""
    capi, ctx = gp
    A, ca = rcs.model_cloud()
    pt = ctx.project_cloud(ctx.make_cloud(A, ca), RES, SZ)
    P = pt.view.P
    assert P == 21
    B = ac.depth_batch(P)
    gd = _depth(capi, ctx, B)
    frames = pt.fetch()
    prm = capi.default_params_render(**ac.PRM)
    s = dict(pt=pt, gd=gd, B=B, frames=frames, P=P, prm=prm, out={})
    for pose in rc.POSES:
        o, dirs = ac.pose_rays(pose, frames)
        s["out"][pose] = (o, dirs, pt.render(o, dirs, gd, None, None, prm, want=WANT))
    yield s
    gd.close()
    pt.close()


def _sigma_reference(B, leaf, local):
    """sigma^2 and its tolerance per ray from readout_cases.evaluate (registration_ref.closed_form_likelihood in np.longdouble)"""
    ref = ac.scattered_reference(B, leaf, np.ascontiguousarray(local[:, 1]), np.ascontiguousarray(local[:, 2]))
    return ref["s2"], ref["s2tol"]


@pytest.mark.parametrize("pose", list(rc.POSES))
def test_sigma_and_normal_at_the_hits_of_a_pose(gp, model, pose):
    capi, ctx = gp
    s = model
    B, frames, gd = s["B"], s["frames"], s["gd"]
    o, dirs, out = s["out"][pose]
    assert set(out) == set(WANT) | {"cloud", "counts"}
    leaf, local, sigma, normal = out["leaf"], out["local"], out["sigma"], out["normal"]
    n = len(dirs)
    assert leaf.shape == (n,) and sigma.shape == (n,) and normal.shape == (n, 3)
    hit = leaf >= 0
    hits = np.flatnonzero(hit)
    assert len(hits) > 100 and out["counts"][1] == len(hits)
    # misses
    assert np.all(np.isnan(sigma[~hit])) and np.all(np.isnan(normal[~hit])) and np.sum(~hit) > 50
    assert np.all(np.isfinite(sigma[hit])) and np.all(np.isfinite(normal[hit]))
    # sigma: the bytes of predict_scattered on the render's own outputs, and the closed form
    _, sp, _ = gd.predict_scattered(leaf, np.ascontiguousarray(local[:, 1]), np.ascontiguousarray(local[:, 2]))
    assert sigma.tobytes() == sp.tobytes()
    s2, tol = _sigma_reference(B, leaf, local)
    se = np.asarray(np.abs((sigma[hit] * sigma[hit]).astype(LD) - s2[hit]), dtype=np.float64)
    assert np.all(se <= tol[hit]), float(np.max(se / tol[hit]))
    # the confidence form is the other sigma form of the same call
    conf = s["pt"].render(o, dirs, gd, None, None, s["prm"], want=("conf",))
    assert set(conf) == {"conf", "cloud", "counts"}
    assert conf["conf"].tobytes() == gd.predict_scattered(leaf, np.ascontiguousarray(local[:, 1]), np.ascontiguousarray(local[:, 2]), conf=True)[1].tobytes()
    # normals
    worst = worst_t = 0.0
    n_exc = 0
    for i in hits:
        L = int(leaf[i])
        r = ac.normal_ref(B, frames, L, local[i], o, LD)
        got = normal[i].astype(LD)
        assert abs(np.sqrt(np.sum(got * got)) - 1) <= 4 * ac.EPS, i                                   # unit length
        err = np.max(np.abs(got - r["n"]))
        if ac.excused(r):                                                                             # the orientation: up to sign
            n_exc += 1
            err = min(err, np.max(np.abs(got + r["n"])))
        assert err <= r["nb"], (i, L, float(err), r["nb"])
        worst = max(worst, float(err) / r["nb"])
        R = np.asarray(frames["R"][L], dtype=LD)
        for t in (R @ np.array([r["fx"], 1, 0], dtype=LD), R @ np.array([r["fy"], 0, 1], dtype=LD)):  # the analytic tangents
            dot = abs(np.sum(got * t))
            assert dot <= r["nb"], (i, L, float(dot), r["nb"])
            worst_t = max(worst_t, float(dot) / r["nb"])
    print(f"{pose}: {len(hits)} hits, sigma^2 error / tolerance {float(np.max(se / tol[hit])):.3f}, normal error / bound {worst:.3f}, "
          f"normal . tangent / bound {worst_t:.3f}, orientation excused {n_exc}")
    assert n_exc <= ac.ORIENT_CAP * len(hits)


def test_coverage_of_the_poses(model):
    """each pose has hits, and together they hit several leaves and basis sizes: an all-miss image cannot pass the tests above"""
    s = model
    leaves = set()
    for pose, (o, dirs, out) in s["out"].items():
        hit = out["leaf"][out["leaf"] >= 0]
        assert len(hit) > 100, pose
        leaves |= set(int(L) for L in hit)
    assert len(leaves) >= 2 and len(set(int(s["B"]["b"][L]) for L in leaves)) >= 6


@pytest.mark.parametrize("pose", list(rc.POSES))
def test_without_an_origin_the_normal_keeps_the_frames_sign(gp, model, pose):
    """origin None: the oriented normal up to sign, on the side of the frame's first column; an origin mirrored through the hit
    turns every decided normal round"""
    s = model
    B, frames = s["B"], s["frames"]
    o, dirs, out = s["out"][pose]
    leaf, local, normal = out["leaf"], out["local"], out["normal"]
    _, plain = s["pt"].render_attrs(leaf, local, s["gd"], None, want_sigma=False)
    hit = leaf >= 0
    assert np.all(np.isnan(plain[~hit]))
    same = np.all(plain[hit] == normal[hit], axis=1)
    assert np.all(same | np.all(plain[hit] == -normal[hit], axis=1))
    col = frames["R"][leaf[hit]][:, :, 0]
    assert np.all(np.sum(plain[hit] * col, axis=1) > 0)
    # (a normal (1, -fx, -fy) has a positive first frame component whatever the slope)
    # the far side: origin' = 2 x - origin for ONE hit's x moves the sensor behind that surface
    i = int(np.flatnonzero(hit)[len(np.flatnonzero(hit)) // 2])
    r = ac.normal_ref(B, frames, int(leaf[i]), local[i], o, LD)
    Rm, mu = frames["R"][leaf[i]], frames["mean"][leaf[i]]
    x = np.array([((Rm[a, 0] * local[i, 0] + Rm[a, 1] * local[i, 1]) + Rm[a, 2] * local[i, 2]) + mu[a] for a in range(3)], dtype=LD)
    behind = np.asarray(2 * x - np.asarray(o, dtype=LD), dtype=np.float64)
    _, turned = s["pt"].render_attrs(leaf[i:i + 1], local[i:i + 1], s["gd"], behind, want_sigma=False)
    assert not ac.excused(r) and np.array_equal(turned[0], -normal[i])


def test_entries_give_the_same_bytes(gp, model):
    import torch
    capi, ctx = gp
    s = model
    o, dirs, out = s["out"]["inside"]
    for conf in (False, True):
        sg, nm = s["pt"].render_attrs(out["leaf"], out["local"], s["gd"], o, conf=conf)
        for _ in range(2):
            d_sg, d_nm = s["pt"].render_attrs(torch.from_numpy(out["leaf"]).cuda(), torch.from_numpy(out["local"]).cuda(), s["gd"], o, conf=conf)
            assert d_sg.cpu().numpy().tobytes() == sg.tobytes() and d_nm.cpu().numpy().tobytes() == nm.tobytes()
        if not conf:
            assert sg.tobytes() == out["sigma"].tobytes() and nm.tobytes() == out["normal"].tobytes()
    # the device render with attributes: device tensors, the same bytes
    dev = s["pt"].render(o, torch.from_numpy(dirs).cuda(), s["gd"], None, None, s["prm"], want=WANT)
    for k in WANT:
        assert dev[k].cpu().numpy().tobytes() == out[k].tobytes(), k
    # one output alone
    only_s, none = s["pt"].render_attrs(out["leaf"], out["local"], s["gd"], o, want_normal=False)
    none2, only_n = s["pt"].render_attrs(out["leaf"], out["local"], s["gd"], o, want_sigma=False)
    assert none is None and none2 is None and only_s.tobytes() == out["sigma"].tobytes() and only_n.tobytes() == out["normal"].tobytes()
    # the default `want` is what it was
    assert set(s["pt"].render(o, dirs, s["gd"], None, None, s["prm"])) == {"cloud", "counts", "leaf", "range", "local"}


@pytest.mark.parametrize("n", [0, 1, 255, 256, 257])
def test_hand_filled_arrays(gp, model, n):
    """leaf / local that no render made: leaves outside [0, P), an empty-basis leaf, sizes around the workgroup"""
    capi, ctx = gp
    s = model
    P = s["P"]
    sizes = np.array(s["B"]["b"])
    sizes[3] = 0                                                             # an empty basis
    B = ac.depth_batch(P, sizes=sizes)
    gd = _depth(capi, ctx, B)
    frames = s["frames"]
    rng = np.random.default_rng(90 + n)
    leaf = rng.integers(0, P, n).astype(np.int32)
    leaf[rng.random(n) < 0.2] = 3
    bad = rng.random(n) < 0.2
    leaf[bad] = rng.choice([-1, P, 2 ** 31 - 1, -2 ** 31], int(bad.sum()))
    local = np.ascontiguousarray(np.stack([rng.uniform(-0.01, 0.01, n), rng.uniform(-RES / 2, RES / 2, n), rng.uniform(-RES / 2, RES / 2, n)], 1))
    o = np.array([0.3, 0.4, 3.0])
    sg, nm = s["pt"].render_attrs(leaf, local, gd, o)
    assert sg.shape == (n,) and nm.shape == (n, 3)
    valid = (leaf >= 0) & (leaf < P)
    assert np.all(np.isnan(sg[~valid])) and np.all(np.isnan(nm[~valid]))
    assert sg.tobytes() == gd.predict_scattered(leaf, local[:, 1].copy(), local[:, 2].copy())[1].tobytes()
    s2, tol = _sigma_reference(B, leaf, local)
    for i in np.flatnonzero(valid):
        L = int(leaf[i])
        r = ac.normal_ref(B, frames, L, local[i], o, LD)
        err = np.max(np.abs(nm[i].astype(LD) - r["n"]))
        if ac.excused(r):
            err = min(err, np.max(np.abs(nm[i].astype(LD) + r["n"])))
        assert err <= r["nb"], (i, L, float(err), r["nb"])
        assert abs((sg[i] * sg[i]).astype(LD) - s2[i]) <= tol[i]
        if L == 3:                                                           # the normalised first column of R, towards the sensor
            c = frames["R"][3][:, 0].astype(LD)
            c = c / np.sqrt(np.sum(c * c))
            assert np.max(np.abs(np.abs(nm[i].astype(LD)) - np.abs(c))) <= 16 * ac.EPS and sg[i] == np.sqrt(RC.SF + RC.S20)
    gd.close()


def test_grown_map_through_mapping_render(gp):
    """Mapping.render(..., want=("sigma", "normal")) on a grown map (a scan below the model's corner on every axis): the bytes of the
    render and the attrs call made by hand"""
    import torch
    capi, ctx = gp
    A, ca = mc.model_cloud()
    pt0 = ctx.project_cloud(ctx.make_cloud(A, ca), RES, SZ)
    v = pt0.view
    gd0 = capi.Sparse(ctx, capi.default_params_sparse(1, sigmaf_sq=1.0, l_sq=(RES / 5) ** 2, noise=1e-3, capacity=24), v.P, 1)
    gc0 = capi.Sparse(ctx, capi.default_params_sparse(3, **KW_C), v.P, 3)
    gd0.add_dev(v.off, v.n_max, v.n_total, v.x0, v.x1, v.y)
    gc0.add_dev(v.off, v.n_max, v.n_total, v.x0, v.x1, v.rgb)
    ctx.synchronize()
    mp = capi.Mapping(ctx, pt0, gd0, gc0, params=capi.default_params_registration(step=1e-7, tol=1e300, min_steps=2, max_steps=10),
                      min_nbr=MIN_NBR)
    Bc, cb = mc.disjoint_scan("below")
    steps, inserted = mp.add_cloud(ctx.make_cloud(Bc, cb))
    assert inserted and mp.patches.view.P == 11 and np.all(mp.depth.sizes() > 0)
    o = np.array([0.4, 0.4, 1.0])
    dirs = torch.from_numpy(rn.camera_rays(rc.LOOK_DOWN, 14.0, 14.0, 11.0, 8.0, 23, 17)).cuda()
    prm = capi.default_params_render(**ac.PRM)
    via = mp.render(o, dirs, prm, want=("sigma", "normal"))
    assert set(via) == {"cloud", "counts", "sigma", "normal"}
    hand = mp.patches.render(o, dirs, mp.depth, mp.rgb, mp.cells, prm, want=("leaf", "local"))
    sg, nm = mp.patches.render_attrs(hand["leaf"], hand["local"], mp.depth, o)
    assert via["cloud"].cpu().numpy().tobytes() == hand["cloud"].cpu().numpy().tobytes()
    assert via["sigma"].cpu().numpy().tobytes() == sg.cpu().numpy().tobytes() and via["normal"].cpu().numpy().tobytes() == nm.cpu().numpy().tobytes()
    leaf = hand["leaf"].cpu().numpy()
    hit = leaf >= 0
    assert hit.sum() > 50 and len(set(leaf[hit])) >= 2
    sgh, nmh = sg.cpu().numpy(), nm.cpu().numpy()
    assert np.all(np.isfinite(sgh[hit])) and np.all(sgh[hit] > 0) and np.all(np.isnan(sgh[~hit])) and np.all(np.isnan(nmh[~hit]))
    assert np.all(np.abs(np.sqrt(np.sum(nmh[hit].astype(LD) ** 2, axis=1)) - 1) <= 4 * ac.EPS)
    x = np.stack([via["cloud"].cpu().numpy().view(capi.Context.POINT_DTYPE).reshape(-1)[k] for k in "xyz"], 1).astype(np.float64)
    assert np.all(np.sum(nmh[hit] * (o - x[hit]), axis=1) > 0)                                        # towards the sensor
    mp.close()


def test_render_attrs_contract(gp, model):
    capi, ctx = gp
    s = model
    L = ctx.lib
    pt, gd, P = s["pt"], s["gd"], s["P"]
    o, dirs, out = s["out"]["above"]
    n = 40
    leaf, local = np.ascontiguousarray(out["leaf"][:n]), np.ascontiguousarray(out["local"][:n])
    sg, nm = np.zeros(n), np.zeros((n, 3))
    a = lambda v: v.ctypes.data if v is not None else None
    for entry in (L.gpc_patches_render_attrs, L.gpc_patches_render_attrs_dev):
        dev = entry is L.gpc_patches_render_attrs_dev
        if dev:
            import torch
            keep = [torch.from_numpy(leaf).cuda(), torch.from_numpy(local).cuda(), torch.zeros(n, dtype=torch.float64, device="cuda"),
                    torch.zeros((n, 3), dtype=torch.float64, device="cuda")]
            torch.cuda.synchronize()
            pl, pc, ps, pn = (t.data_ptr() for t in keep)
        else:
            pl, pc, ps, pn = a(leaf), a(local), a(sg), a(nm)
        assert entry(ctx.h, pt.h, gd.h, n, pl, pc, a(o), 0, ps, pn) == capi.GPC_OK
        ctx.synchronize()
        assert entry(ctx.h, pt.h, gd.h, 0, None, None, a(o), 0, None, None) == capi.GPC_OK           # n == 0
        assert entry(ctx.h, pt.h, gd.h, n, pl, pc, None, 0, ps, pn) == capi.GPC_OK                   # no origin
        ctx.synchronize()
        assert entry(None, pt.h, gd.h, n, pl, pc, a(o), 0, ps, pn) == capi.GPC_EINVAL
        assert entry(ctx.h, None, gd.h, n, pl, pc, a(o), 0, ps, pn) == capi.GPC_EINVAL
        assert entry(ctx.h, pt.h, None, n, pl, pc, a(o), 0, ps, pn) == capi.GPC_EINVAL
        assert entry(ctx.h, pt.h, gd.h, -1, pl, pc, a(o), 0, ps, pn) == capi.GPC_EINVAL
        assert entry(ctx.h, pt.h, gd.h, n, None, pc, a(o), 0, ps, pn) == capi.GPC_EINVAL
        assert entry(ctx.h, pt.h, gd.h, n, pl, None, a(o), 0, ps, pn) == capi.GPC_EINVAL
        for bad in (np.nan, np.inf):
            o2 = o.copy()
            o2[1] = bad
            assert entry(ctx.h, pt.h, gd.h, n, pl, pc, a(o2), 0, ps, pn) == capi.GPC_EINVAL
        for wrongP, ny in ((P + 1, 1), (P, 3)):                                                      # depth with another P or ny
            wrong = capi.Sparse(ctx, capi.default_params_sparse(ny, **dict(ac.KW_DEPTH, noise=1.0)), wrongP, ny)
            assert entry(ctx.h, pt.h, wrong.h, n, pl, pc, a(o), 0, ps, pn) == capi.GPC_EINVAL
            wrong.close()
        gone = capi.Sparse(ctx, capi.default_params_sparse(1, **ac.KW_DEPTH), P, 1)                  # a destroyed object
        h_gone = gone.h
        gone.close()
        assert entry(ctx.h, pt.h, h_gone, n, pl, pc, a(o), 0, ps, pn) == capi.GPC_EINVAL
        ctx2 = capi.Context(0)                                                                       # objects of different contexts
        other = capi.Sparse(ctx2, capi.default_params_sparse(1, **ac.KW_DEPTH), P, 1)
        assert entry(ctx.h, pt.h, other.h, n, pl, pc, a(o), 0, ps, pn) == capi.GPC_EINVAL
        assert entry(ctx2.h, pt.h, other.h, n, pl, pc, a(o), 0, ps, pn) == capi.GPC_EINVAL
        other.close()
        ctx2.close()
    assert sg.tobytes() != np.zeros(n).tobytes()
