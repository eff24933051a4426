"""GPU parity of gpc_reproject (reprojection + colour clamp fused, src/gp_compressor.cpp:335-373)
against the CPU oracle (orc_reproject, orc_flatten_colors).  Integer / byte / float-cast work: bit-exact."""
import ctypes as C

import numpy as np
import pytest

import reproject_cases as RC
from gp_compressor_amd import synth

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def gp():
    from gp_compressor_amd import capi
    capi.load()
    ctx = capi.Context(0)
    yield capi, ctx
    ctx.close()


def _oracle_cloud(oracle, xs0, xs1, f, R, mu, cs, cm, bv):
    L = oracle.lib()
    P, m = f.shape
    xyz_all, rgb_all = [], []
    xyz = (C.c_float * 3)()
    rgb = (C.c_uint8 * 3)()
    for i in range(P):
        if bv is not None and bv[i] == 0:
            continue
        Ri, mi = np.ascontiguousarray(R[i]), np.ascontiguousarray(mu[i])
        for q in range(m):
            L.orc_reproject(oracle._dp(Ri), oracle._dp(mi), float(f[i, q]), float(xs0[q]), float(xs1[q]), xyz)
            xyz_all.append((xyz[0], xyz[1], xyz[2]))
            if cs is not None:
                c3 = np.ascontiguousarray(cs[i, :, q] + cm[i])
                L.orc_flatten_colors(oracle._dp(c3), rgb)
                rgb_all.append((rgb[0], rgb[1], rgb[2]))
            else:
                rgb_all.append((0, 0, 0))
    return np.array(xyz_all, dtype=np.float32).reshape(-1, 3), np.array(rgb_all, dtype=np.uint8).reshape(-1, 3)


@pytest.mark.parametrize("P,sz,with_rgb,with_bv", [(7, 6, True, True), (3, 20, True, False), (5, 4, False, True), (1, 1, True, False)])
def test_reproject_bit_exact(gp, oracle, P, sz, with_rgb, with_bv):
    capi, ctx = gp
    rng = np.random.default_rng(100 + P)
    res, m = 0.15, sz * sz
    xs0, xs1 = oracle.grid(res, sz)
    f = rng.normal(0, 0.01, (P, m))
    # random rotations (column-major 9 doubles: columns = normal, u, v) and centres far from the origin (float rounding matters)
    R = np.zeros((P, 9))
    for i in range(P):
        Q, _ = np.linalg.qr(rng.normal(size=(3, 3)))
        R[i] = Q.T.reshape(-1)          # column-major storage of Q
    mu = rng.uniform(-50, 50, (P, 3))
    cs = cm = None
    if with_rgb:
        cs = rng.normal(0, 90, (P, 3, m))
        cm = rng.uniform(0, 255, (P, 3))
        # the clamp's corner cases: NaN / inf -> 255, negative -> 0, > 255 -> 255, > 32767 wraps as short, out of int range -> 0
        specials = [np.nan, np.inf, -np.inf, -1e-9, -0.9999, 255.0, 255.9999, 256.0, 32767.9, 32768.0, 40000.0, 65535.5, 65536.0, 65791.0,
                    1e9, 3e9, -3e9, 1e300, -1e300, 0.0, 127.5]
        flat = cs.reshape(-1)
        idx = rng.choice(flat.size, size=min(len(specials), flat.size), replace=False)
        for k, j in enumerate(idx):
            flat[j] = specials[k] - cm.reshape(-1)[(j // m) % (3 * P)] if np.isfinite(specials[k]) else specials[k]
    bv = None
    if with_bv:
        bv = rng.integers(0, 3, P).astype(np.int32)
        bv[0] = 0
        bv[-1] = 5
    cloud = ctx.reproject(xs0, xs1, f, R, mu, cs, cm, bv)
    xyz_o, rgb_o = _oracle_cloud(oracle, xs0, xs1, f, R, mu, cs, cm, bv)
    assert cloud.shape[0] == xyz_o.shape[0] == m * (P if bv is None else int(np.count_nonzero(bv)))
    got_xyz = np.stack([cloud["x"], cloud["y"], cloud["z"]], 1)
    assert np.array_equal(got_xyz.view(np.uint32), xyz_o.view(np.uint32))          # bit-exact floats
    assert np.array_equal(np.stack([cloud["r"], cloud["g"], cloud["b"]], 1), rgb_o)
    assert np.all(cloud["w"] == 1.0) and np.all(cloud["a"] == 255)
    assert cloud.dtype.itemsize == 32


def test_reproject_empty_and_errors(gp):
    capi, ctx = gp
    xs0, xs1 = synth.grid(0.15, 3)
    out = ctx.reproject(xs0, xs1, np.zeros((2, 9)), np.tile(np.eye(3).reshape(-1), (2, 1)), np.zeros((2, 3)), bv_count=np.zeros(2, np.int32))
    assert out.shape[0] == 0
    with pytest.raises(capi.GpcError) as e:        # colours without their means
        ctx.reproject(xs0, xs1, np.zeros((1, 9)), np.eye(3).reshape(1, 9), np.zeros((1, 3)), c_star=np.zeros((1, 3, 9)))
    assert e.value.code == capi.GPC_EINVAL


# ---- the batch sizes where the loops of reproject.hip wrap (reproject_cases.py; the cases themselves: test_reproject_cases_cpu.py) -----------

def _emit_grid(P):
    """workgroups of reproject_kernel: min(P, 8 x CUs); the kernel strides over the patches beyond them"""
    import torch
    return min(P, 8 * torch.cuda.get_device_properties(0).multi_processor_count)


def _regime(P, bv, what=""):
    n_on = len(RC.trained(P, bv))
    print("%sP = %d, per = %d, emit grid = %d, trained = %d" % (what, P, RC.per_of(P), _emit_grid(P), n_on))
    return n_on


def _check_compaction(ctx, oracle, P, name):
    bv, (xs0, xs1, f, R, mu, cs, cm) = RC.compaction_case(P, name)
    n_on = _regime(P, bv, name + ": ")
    cloud = ctx.reproject(xs0, xs1, f, R, mu, cs, cm, bv)
    assert cloud.shape[0] == RC.COMPACTION_M * n_on
    if name == "none":
        assert cloud.shape[0] == 0
    RC.assert_same_cloud(cloud, RC.expected(oracle, xs0, xs1, f, R, mu, cs, cm, bv))


@pytest.mark.parametrize("name", RC.PATTERNS)
@pytest.mark.parametrize("P", RC.COMPACTION_P)
def test_compaction_where_the_scan_wraps(gp, oracle, P, name):
    """one, two and three patches per scan thread, every trained / untrained pattern: record count and the whole cloud, byte for byte"""
    _check_compaction(gp[1], oracle, P, name)


@pytest.mark.parametrize("name", RC.PATTERNS)
def test_compaction_above_the_emit_grid(gp, oracle, name):
    """more patches than reproject_kernel has workgroups on the card in hand: the grid-stride loop is taken"""
    import torch
    P = 8 * torch.cuda.get_device_properties(0).multi_processor_count + 1
    assert P > _emit_grid(P)
    _check_compaction(gp[1], oracle, P, name)


@pytest.mark.parametrize("with_bv", [False, True])
@pytest.mark.parametrize("with_rgb", [False, True])
@pytest.mark.parametrize("m", RC.ROW_M)
def test_row_lengths_around_the_q_loop(gp, oracle, m, with_rgb, with_bv):
    """the 256-thread loop over a patch's points: one pass short by one, one pass, one pass and one, two passes and one"""
    capi, ctx = gp
    P = RC.ROW_P
    bv = RC.bv_pattern("period2" if with_bv else "all", P, 11)
    xs0, xs1, f, R, mu, cs, cm = RC.inputs(P, m, 11, with_rgb, bv)
    n_on = _regime(P, bv, "m = %d: " % m)
    cloud = ctx.reproject(xs0, xs1, f, R, mu, cs, cm, bv)
    assert cloud.shape[0] == m * n_on
    RC.assert_same_cloud(cloud, RC.expected(oracle, xs0, xs1, f, R, mu, cs, cm, bv))


def test_non_finite_rows_among_the_trained(gp, oracle):
    """NaN, +-inf and 1e300 in f* of trained patches at the head, the middle and the end of a batch of two patches per scan thread:
    NaN records where f* is NaN, infinite floats where it is infinite or overflows the cast, every other record as in the clean run"""
    capi, ctx = gp
    P, m = 1025, RC.COMPACTION_M
    bv, (xs0, xs1, f, R, mu, cs, cm) = RC.compaction_case(P, "random")
    _regime(P, bv)
    t = RC.trained(P, bv)
    g = RC.non_finite_rows(f, [int(t[0]), int(t[1]), int(t[len(t) // 2]), int(t[-2]), int(t[-1])])
    clean = ctx.reproject(xs0, xs1, f, R, mu, cs, cm, bv)
    RC.assert_same_cloud(clean, RC.expected(oracle, xs0, xs1, f, R, mu, cs, cm, bv))
    cloud = ctx.reproject(xs0, xs1, g, R, mu, cs, cm, bv)
    fr = RC.f_of_records(g, bv)
    RC.assert_same_cloud(cloud, RC.expected(oracle, xs0, xs1, g, R, mu, cs, cm, bv), fr)
    odd = ~np.isfinite(fr) | (fr == 1e300)
    assert np.count_nonzero(odd) == 10 and np.count_nonzero(np.isnan(fr)) >= 2
    assert cloud[~odd].tobytes() == clean[~odd].tobytes()
    Rr = np.repeat(R[t], m, axis=0)
    big = odd & ~np.isnan(fr)
    for k, key in enumerate(("x", "y", "z")):
        assert np.all(np.isnan(cloud[key][np.isnan(fr)]))
        assert np.array_equal(cloud[key][big], (np.sign(fr[big]) * np.sign(Rr[big, k]) * np.inf).astype(np.float32))
    for key in ("r", "g", "b", "a", "w", "pad"):
        assert np.array_equal(cloud[key], clean[key])


FILL = 0xA5


def _dev_call(ctx, d, P, m, out, n_pts):
    """gpc_reproject_dev on the device copies d of (bv, xs0, xs1, f, cs, R, mu, cm); returns n_points and the whole buffer's bytes"""
    ctx.reproject_dev(P, m, d[0], d[1], d[2], d[3], d[4], d[5], d[6], d[7], out, n_pts)
    ctx.synchronize()
    return int(n_pts.cpu()[0]), out.cpu().numpy()


def _to_dev(bv, xs0, xs1, f, R, mu, cs, cm):
    import torch
    return [None if a is None else torch.from_numpy(np.ascontiguousarray(a)).cuda() for a in (bv, xs0, xs1, f, cs, R, mu, cm)]


@pytest.mark.parametrize("name", ["random", "none"])
def test_device_entry_writes_its_records_and_nothing_else(gp, oracle, name):
    """gpc_reproject_dev into a buffer of P m records filled with 0xA5: the first n_points records are the host entry's bytes (and the
    oracle's), every byte behind them still holds the fill; with no trained patch n_points is 0 and the whole buffer does"""
    import torch
    capi, ctx = gp
    P, m = 2049, RC.COMPACTION_M
    bv, (xs0, xs1, f, R, mu, cs, cm) = RC.compaction_case(P, name)
    n_on = _regime(P, bv, name + ": ")
    host = ctx.reproject(xs0, xs1, f, R, mu, cs, cm, bv)
    RC.assert_same_cloud(host, RC.expected(oracle, xs0, xs1, f, R, mu, cs, cm, bv))
    ctx.set_stream(torch.cuda.current_stream().cuda_stream)
    try:
        d = _to_dev(bv, xs0, xs1, f, R, mu, cs, cm)
        out = torch.full((P * m, 32), FILL, dtype=torch.uint8, device="cuda")
        n_pts = torch.full((1,), -7, dtype=torch.int32, device="cuda")
        n, raw = _dev_call(ctx, d, P, m, out, n_pts)
    finally:
        ctx.set_stream(None)
    assert n == m * n_on == len(host) and (n == 0) == (name == "none")
    assert raw[:n].tobytes() == host.tobytes()
    assert np.all(raw[n:] == FILL)


def test_back_to_back_calls_on_one_context(gp, oracle):
    """a large batch, a small one into the same buffer, the large one again: the small call's scan fills only its own five entries of
    the workspace's base array, and what the large call left behind them must not be read"""
    import torch
    capi, ctx = gp
    m = RC.COMPACTION_M
    Pl, Ps = 2049, 5
    bvl, big = RC.compaction_case(Pl, "random")
    bvs = RC.bv_pattern("first_only", Ps, 13)
    small = RC.inputs(Ps, m, 13, True, bvs)
    want_l, want_s = RC.expected(oracle, *big, bvl), RC.expected(oracle, *small, bvs)
    nl = _regime(Pl, bvl, "large: ")
    ns = _regime(Ps, bvs, "small: ")
    assert len(want_l) == m * nl and len(want_s) == m * ns == m
    ctx.set_stream(torch.cuda.current_stream().cuda_stream)
    try:
        dl, ds = _to_dev(bvl, *big), _to_dev(bvs, *small)
        out = torch.full((Pl * m, 32), FILL, dtype=torch.uint8, device="cuda")
        n_pts = torch.zeros(1, dtype=torch.int32, device="cuda")
        n1, raw1 = _dev_call(ctx, dl, Pl, m, out, n_pts)
        n2, raw2 = _dev_call(ctx, ds, Ps, m, out, n_pts)
        n3, raw3 = _dev_call(ctx, dl, Pl, m, out, n_pts)
    finally:
        ctx.set_stream(None)
    assert n1 == len(want_l) and raw1[:n1].tobytes() == want_l.tobytes() and np.all(raw1[n1:] == FILL)
    assert n2 == len(want_s) and raw2[:n2].tobytes() == want_s.tobytes()
    assert np.array_equal(raw2[n2:], raw1[n2:])             # behind the small call's records the buffer is as the large call left it
    assert n3 == n1 and np.array_equal(raw3, raw1)
