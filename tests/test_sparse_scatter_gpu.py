"""gpc_sparse_predict_scattered[_dev]: the sparse read-out at (patch, point) pairs in arbitrary order, bucketed on the device
(csrc/sparse_scatter.hip).  States are readout_cases.batch (loaded with set_state, only read); patterns, counts and the references are
tests/render_attrs_cases.py.  Every entry of every case is held to
  (a) the bytes of Sparse.predict_points on the host-bucketed batch (np.argsort(kind="stable")) scattered back: f, sigma, status, in
      both sigma forms;
  (b) independently of the code under test, the np.longdouble closed form of readout_cases.evaluate within its derived bounds fb and
      sigma2_tolerance;
  (c) NaN in every plane at a skipped entry;  (d) the same bytes from a second call;  (e) the same bytes from the host and _dev entries;
with the interleaved layout (stride 3, as a render's `local`) beside the SoA one."""
import numpy as np
import pytest

import readout_cases as RC
import render_attrs_cases as ac

pytestmark = pytest.mark.gpu
LD = RC.LD


@pytest.fixture(scope="module")
def gp():
    from gp_compressor_amd import capi
    capi.load()
    ctx = capi.Context(0)
    yield capi, ctx
    ctx.close()


def _load(capi, ctx, B):
    prm = capi.default_params_sparse(B["ny"], sigmaf_sq=RC.SF, l_sq=B["l_sq"], noise=RC.S20, capacity=B["capacity"])
    g = capi.Sparse(ctx, prm, B["P"], B["ny"])
    assert g.ld() == B["ld"]
    g.set_state(B["b"], B["alpha"], B["BV"], B["C"], None)
    return g


@pytest.fixture(scope="module")
def loaded(gp):
    capi, ctx = gp
    made = {}

    def get(case):
        if case not in made:
            B = RC.batch(*case)
            made[case] = (_load(capi, ctx, B), B)
        return made[case]
    yield get
    for g, _ in made.values():
        g.close()


def _host(capi, g, patch, q0, q1, stride, conf, want_f=True, want_sigma=True):
    """the host entry on SoA arrays (stride 1) or on one interleaved (n, stride) array holding q0, q1 in columns 1 and 2"""
    n = len(patch)
    if stride == 1:
        x0, x1 = np.ascontiguousarray(q0), np.ascontiguousarray(q1)
        p0, p1 = x0.ctypes.data, x1.ctypes.data
    else:
        x = np.full((max(n, 1), stride), 1e300)
        x[:n, 1], x[:n, 2] = q0, q1
        p0, p1 = x.ctypes.data + 8, x.ctypes.data + 16
    f = np.full((g.ny, n), -7.0) if want_f else None
    s = np.full(n, -7.0) if want_sigma else None
    st = np.full(g.P, -1, np.int32)
    ptr = lambda a: a.ctypes.data if (a is not None and n) else None
    rc = g.lib.gpc_sparse_predict_scattered(g.h, n, ptr(patch), p0 if n else None, p1 if n else None, stride, ptr(f), ptr(s), int(conf),
                                            st.ctypes.data)
    assert rc == capi.GPC_OK, g.ctx.lib.gpc_last_error(g.ctx.h)
    return f, s, st


def _dev(capi, ctx, g, patch, q0, q1, stride, conf):
    import torch
    n = len(patch)
    if stride == 1:
        d_x = (torch.from_numpy(np.concatenate([q0, [0.0]])).cuda(), torch.from_numpy(np.concatenate([q1, [0.0]])).cuda())
        p0, p1 = d_x[0].data_ptr(), d_x[1].data_ptr()
    else:
        x = np.full((max(n, 1), stride), 1e300)
        x[:n, 1], x[:n, 2] = q0, q1
        d_x = torch.from_numpy(x).cuda()
        p0, p1 = d_x.data_ptr() + 8, d_x.data_ptr() + 16
    d_patch = torch.from_numpy(np.concatenate([patch, [0]]).astype(np.int32)).cuda()
    d_f = torch.full((g.ny, max(n, 1)), -7.0, dtype=torch.float64, device="cuda")
    d_s = torch.full((max(n, 1),), -7.0, dtype=torch.float64, device="cuda")
    d_st = torch.full((g.P,), -1, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    g.predict_scattered_dev(n, d_patch.data_ptr(), p0, p1, stride, d_f.data_ptr() if n else None, d_s.data_ptr() if n else None, conf,
                            d_st.data_ptr())
    ctx.synchronize()
    f = d_f.cpu().numpy().reshape(-1)[:g.ny * n].reshape(g.ny, n)      # (planes of n)
    return f, d_s.cpu().numpy()[:n], d_st.cpu().numpy()


def _expected(g, B, patch, q0, q1, conf, want_sigma=True):
    """predict_points on the host-bucketed batch, scattered back"""
    n = len(patch)
    order, off, nv = ac.bucket(patch, B["P"])
    fb, sb, st = g.predict_points(off, q0[order[:nv]], q1[order[:nv]], want_sigma=want_sigma, conf=conf)
    f, s = np.full((B["ny"], n), np.nan), np.full(n, np.nan)
    f[:, order[:nv]] = fb
    if want_sigma:
        s[order[:nv]] = sb
    return f, s, st


def _hold(capi, ctx, g, B, patch, q0, q1, strides=(1, 3), ref=None, dev=True):
    """(a) .. (e) for one set of entries; returns the worst error / bound of (b)"""
    n = len(patch)
    valid = (patch >= 0) & (patch < B["P"])
    ref = ac.scattered_reference(B, patch, q0, q1) if ref is None else ref
    worst = dict(f=0.0, s2=0.0)
    for conf in (False, True):
        ef, es, est = _expected(g, B, patch, q0, q1, conf)
        for stride in strides:
            f, s, st = _host(capi, g, patch, q0, q1, stride, conf)
            assert f.tobytes() == ef.tobytes() and s.tobytes() == es.tobytes() and st.tobytes() == est.tobytes(), (n, stride, conf)      # (a)
            assert np.all(np.isnan(f[:, ~valid])) and np.all(np.isnan(s[~valid]))                                                      # (c)
            assert np.all(np.isfinite(f[:, valid])) and np.all(np.isfinite(s[valid]))
            f2, s2, st2 = _host(capi, g, patch, q0, q1, stride, conf)
            assert f2.tobytes() == f.tobytes() and s2.tobytes() == s.tobytes() and st2.tobytes() == st.tobytes()                       # (d)
            if dev:
                fd, sd, std = _dev(capi, ctx, g, patch, q0, q1, stride, conf)
                assert fd.tobytes() == f.tobytes() and sd.tobytes() == s.tobytes() and std.tobytes() == st.tobytes(), (n, stride, conf)   # (e)
        if not conf and valid.any():                                                                                                   # (b)
            fe = np.asarray(np.abs(f[:, valid].astype(LD) - ref["f"][:, valid]), dtype=np.float64)
            fb = ref["fb"][:, valid]
            assert np.all(fe <= fb), (n, float(np.max(fe - fb)))
            se = np.asarray(np.abs((s[valid] * s[valid]).astype(LD) - ref["s2"][valid]), dtype=np.float64)
            assert np.all(se <= ref["s2tol"][valid]), n
            with np.errstate(invalid="ignore", divide="ignore"):
                worst = dict(f=float(np.max(np.where(fb > 0, fe / fb, 0.0))), s2=float(np.max(se / ref["s2tol"][valid])))
    # one output alone: the bytes of the bucketed entry asked for the same (mean without sigma; sigma without a mean plane)
    fm, none, stm = _host(capi, g, patch, q0, q1, 1, False, want_sigma=False)
    em, _, estm = _expected(g, B, patch, q0, q1, False, want_sigma=False)
    assert none is None and fm.tobytes() == em.tobytes() and stm.tobytes() == estm.tobytes()
    none, so, _ = _host(capi, g, patch, q0, q1, 3, False, want_f=False)
    assert none is None and so.tobytes() == _expected(g, B, patch, q0, q1, False)[1].tobytes()
    return worst


@pytest.mark.parametrize("pattern", ac.PATTERNS)
@pytest.mark.parametrize("case", ac.OBJECTS, ids=ac.OBJECT_IDS)
def test_scattered_predict_every_count_and_pattern(gp, loaded, case, pattern):
    capi, ctx = gp
    g, B = loaded(case)
    worst = dict(f=0.0, s2=0.0)
    counts = (0,) if pattern == "chunks" else ac.COUNTS
    for n in counts:
        patch, q0, q1 = ac.scatter_pattern(pattern, B, n, seed=1000 + n)
        w = _hold(capi, ctx, g, B, patch, q0, q1)
        worst = {k: max(worst[k], w[k]) for k in worst}
    print(f"scattered predict {ac.OBJECT_IDS[ac.OBJECTS.index(case)]} [{pattern}]: worst error / bound mean {worst['f']:.3f}, sigma^2 {worst['s2']:.3f}")
    # Sparse.predict_scattered is the host entry
    f, s, st = g.predict_scattered(patch, q0, q1)
    ef, es, est = _expected(g, B, patch, q0, q1, False)
    assert f.tobytes() == ef.tobytes() and s.tobytes() == es.tobytes() and st.tobytes() == est.tobytes()


def test_scattered_predict_hundred_thousand_entries(gp, loaded):
    """about 1e5 entries with skipped ids among them: the sort's multi-workgroup path, many blocks of every stage"""
    capi, ctx = gp
    g, B = loaded(ac.OBJECTS[0])
    patch, q0, q1 = ac.scatter_pattern("sprinkled", B, ac.BIG_COUNT, seed=5)
    w = _hold(capi, ctx, g, B, patch, q0, q1)
    print(f"scattered predict, {ac.BIG_COUNT} entries: worst error / bound mean {w['f']:.3f}, sigma^2 {w['s2']:.3f}")


def test_scattered_predict_sigma_clamp(gp):
    """readout_cases.clamp_batch: the entries that ARE basis vectors of the middle patch give sigma == 0 (confidence form 100), and
    the clamp is reported for that patch only"""
    capi, ctx = gp
    B = RC.clamp_batch()
    g = _load(capi, ctx, B)
    rng = np.random.default_rng(8)
    bv = B["BV"][1][:RC.CLAMP_B]
    other = rng.integers(0, 2, 40) * 2                                       # patches 0 and 2
    patch = np.concatenate([np.full(RC.CLAMP_B, 1), other]).astype(np.int32)
    q0 = np.concatenate([bv[:, 0], rng.uniform(-RC.RES / 2, RC.RES / 2, 40)])
    q1 = np.concatenate([bv[:, 1], rng.uniform(-RC.RES / 2, RC.RES / 2, 40)])
    o = rng.permutation(len(patch))
    patch, q0, q1 = patch[o], q0[o], q1[o]
    f, s, st = g.predict_scattered(patch, q0, q1)
    _, c, stc = g.predict_scattered(patch, q0, q1, conf=True)
    assert st.tolist() == stc.tolist() == [0, capi.STATUS_SIGMA_CLAMPED, 0]
    assert np.all(s[patch == 1] == 0.0) and np.all(c[patch == 1] == 100.0) and np.all(s[patch != 1] > 0.0)
    ef, es, est = _expected(g, B, patch, q0, q1, False)
    assert f.tobytes() == ef.tobytes() and s.tobytes() == es.tobytes() and st.tobytes() == est.tobytes()
    # only the other patches' entries: no clamp is reported
    keep = patch != 1
    assert g.predict_scattered(patch[keep], q0[keep], q1[keep])[2].tolist() == [0, 0, 0]
    g.close()


def test_scattered_predict_contract(gp, loaded):
    capi, ctx = gp
    g, B = loaded(ac.OBJECTS[0])
    L = ctx.lib
    patch, q0, q1 = ac.scatter_pattern("uniform", B, 5, seed=3)
    f, s = np.zeros((1, 5)), np.zeros(5)
    a = lambda v: v.ctypes.data
    for entry in (L.gpc_sparse_predict_scattered, L.gpc_sparse_predict_scattered_dev):
        assert entry(None, 5, a(patch), a(q0), a(q1), 1, a(f), a(s), 0, None) == capi.GPC_EINVAL
        assert entry(g.h, -1, a(patch), a(q0), a(q1), 1, a(f), a(s), 0, None) == capi.GPC_EINVAL
        assert entry(g.h, 5, a(patch), a(q0), a(q1), 0, a(f), a(s), 0, None) == capi.GPC_EINVAL
        assert entry(g.h, 5, None, a(q0), a(q1), 1, a(f), a(s), 0, None) == capi.GPC_EINVAL
        assert entry(g.h, 5, a(patch), None, a(q1), 1, a(f), a(s), 0, None) == capi.GPC_EINVAL
        assert entry(g.h, 5, a(patch), a(q0), None, 1, a(f), a(s), 0, None) == capi.GPC_EINVAL
        assert entry(g.h, 0, None, None, None, 1, None, None, 0, None) == capi.GPC_OK
    # an object without patches: every entry is skipped
    empty = capi.Sparse(ctx, capi.default_params_sparse(1, capacity=15), 0, 1)
    f0, s0, st0 = empty.predict_scattered(np.array([0, -1, 3], np.int32), q0[:3], q1[:3])
    assert np.all(np.isnan(f0)) and np.all(np.isnan(s0)) and st0.shape == (0,)
    empty.close()
