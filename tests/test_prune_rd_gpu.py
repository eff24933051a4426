"""gpc_sparse_prune_rd on the GPU: against the NumPy restatement from the same state bits, against the read-out, bit for bit against
gpc_sparse_prune and against itself, at its edges and through Mapping.prune_to_error.

Set-up of the numeric cases (prune_ref.REGIMES, ny = 1 and ny = 3 with ref_field_delete_bug = 0), as tests/test_prune_gpu.py: the states
are produced by Sparse.add on the GPU and read back with state(); the same bits go into the restatement (tests/prune_rd_ref.py) and into
fresh GPU objects.  The points the error is taken on are the points the states were trained on.  Bounds: B_p = 2 mse0_p with mse0 from a
GPU call that removes nothing (target >= b), keep = 1.  A patch is compared while, in the restatement's run, the two lowest scores of
every scan differ by more than 1e-6 relative and no error the loop saw lies within 1e-6 relative of B_p; at most 5 % of a case's patches
may be left out.  Gates: mse0, mse[:removed] and mse_next within 64 x E64_MSE relative (prune_rd_ref.E64_MSE = 7.84e-11, measured by
tests/test_prune_rd_cpu.py: float64 against longdouble restatement from the same bits), scores rtol 1e-6, the state arrays within
64 x prune_ref.E64; removed, order, the basis count and the stop side equal.

Measured: E64_MSE 7.839e-11 on the CPU (gate 64 x 7.84e-11 = 5.02e-09).  On the MI355X, worst over the cases of this module, relative:
mse0 2.0e-14, mse 3.1e-14, mse_next 2.0e-15 (the order of the sums and the FMAs of the kernel against NumPy's separate products), the
read-out of the pruned object against the last accepted look-ahead 3.8e-16 (0 for ny = 1); C, Q and BV 0 and alpha 0 for ny = 1 (the
restatement's bits), alpha 4.8e-16 for ny = 3.  No patch was left out in any case; with B_p = 2 mse0_p the capacity-100 depth leaves drop
80..99 of 100 vectors, the colour leaves 75..81, and the bound (not the floor) stops every patch for ny = 3 and at capacity -1.
"""
import numpy as np
import pytest

import prune_rd_ref as rd
import prune_ref as pr

pytestmark = pytest.mark.gpu
GATE_MSE = pr.GATE_FACTOR * rd.E64_MSE


@pytest.fixture(scope="module")
def gp():
    from gp_compressor_amd import capi
    capi.load()
    ctx = capi.Context(0)
    yield capi, ctx
    ctx.close()


# ---- the helpers of tests/test_prune_gpu.py (copied: that file stays as it is) ---------------------------------------------------------

def _params(capi, cap, div, ny, bug=0):
    return capi.default_params_sparse(ny, ref_field_delete_bug=bug, **pr.kernel_kw(cap, div, ny))


_trained = {}


def _train(capi, ctx, cap, div, n, P, ny, bug=0):
    """the regime's batch trained by Sparse.add on the GPU: per-patch states as the restatement takes them (computed once per regime)"""
    key = (cap, ny, bug, P)
    if key not in _trained:
        off, x0, x1, y, perm = pr.batch(cap, n, P, ny)
        g = capi.Sparse(ctx, _params(capi, cap, div, ny, bug), P, ny)
        st = g.add(off, x0, x1, y, perm)
        assert np.all(st == 0)
        b = g.sizes()
        alpha, C, Q, BV = g.state()
        g.close()
        _trained[key] = [(alpha[i, :, :b[i]].copy(), C[i, :b[i], :b[i]].copy(), Q[i, :b[i], :b[i]].copy(), BV[i, :b[i]].copy()) for i in range(P)]
    return _trained[key]


def _load(capi, ctx, p, ny, states):
    """a fresh GPU object holding `states` (gpc_sparse_set_state: the same bits); padding zero"""
    P = len(states)
    g = capi.Sparse(ctx, p, P, ny)
    ld = g.ld()
    b = np.array([s[0].shape[1] for s in states], dtype=np.int32)
    alpha, C, Q, BV = np.zeros((P, ny, ld)), np.zeros((P, ld, ld)), np.zeros((P, ld, ld)), np.zeros((P, ld, 2))
    for i, (a, c, q, v) in enumerate(states):
        alpha[i, :, :b[i]], C[i, :b[i], :b[i]], Q[i, :b[i], :b[i]], BV[i, :b[i]] = a, c, q, v
    g.set_state(b, alpha, BV, C, Q)
    return g


def _copy(g):
    return g.remap(g.P, np.arange(g.P, dtype=np.int32))


def _bits(g):
    """everything the object holds, padding included"""
    return (g.sizes(),) + tuple(g.state())


def _same(a, b):
    return all(np.array_equal(x, y, equal_nan=True) for x, y in zip(a, b))


# ---- this module's own ---------------------------------------------------------------------------------------------------------------

def _mse_from_readout(g, off, x0, x1, y):
    """per-patch error of the object as it stands, from Sparse.predict_points, summed in the rule's order"""
    f, _, _ = g.predict_points(off, x0, x1)
    out = np.full(g.P, np.nan)
    for i in range(g.P):
        s = slice(off[i], off[i + 1])
        if off[i + 1] > off[i]:
            r = y[:, s] - f[:, s]
            e = np.zeros(off[i + 1] - off[i])
            for c in range(g.ny):
                e = e + r[c] * r[c]
            out[i] = rd.class_sum(e) / (len(e) * g.ny)
    return out


def _compare(capi, ctx, cap, div, n, P, ny, uniform=False):
    kw = pr.kernel_kw(cap, div, ny)
    states = _train(capi, ctx, cap, div, n, P, ny)
    off, x0, x1, y, _ = pr.batch(cap, n, P, ny)
    g = _load(capi, ctx, _params(capi, cap, div, ny), ny, states)
    b0 = g.sizes()
    start = _bits(g)
    rm, mse0, nxt = g.prune_rd(off, x0, x1, y, target=b0)                     # target >= b: mse0 only, not a byte moves
    assert np.all(rm == 0) and np.all(np.isnan(nxt)) and _same(_bits(g), start)
    assert np.allclose(mse0, _mse_from_readout(g, off, x0, x1, y), rtol=GATE_MSE, atol=0)
    bound = 2.0 * mse0
    if uniform:
        B = float(np.median(bound))
        bound = np.full(P, B)
        rm, m0, nxt, order, scores, mse = g.prune_rd(off, x0, x1, y, keep=1, max_mse=B, want_trace=True)
    else:
        rm, m0, nxt, order, scores, mse = g.prune_rd(off, x0, x1, y, keep=1, max_mse_p=bound, want_trace=True)
    assert np.array_equal(m0, mse0)
    b = g.sizes()
    alpha, C, Q, BV = g.state()
    after = _mse_from_readout(g, off, x0, x1, y)
    g.close()
    worst = dict(mse0=0.0, mse=0.0, mse_next=0.0, readout=0.0, alpha=0.0, C=0.0, Q=0.0, BV=0.0)
    kept = 0
    for i, st in enumerate(states):
        s = slice(off[i], off[i + 1])
        r = rd.prune_rd(*st, x0[s], x1[s], y[:, s], 1, float(bound[i]), kw)
        if not rd.comparable(r):
            continue
        kept += 1
        k = len(r["order"])
        assert rm[i] == k and b[i] == r["alpha"].shape[1] == b0[i] - k, (i, rm[i], k, b[i])
        assert np.array_equal(order[i, :k], r["order"]), (i, order[i, :k], r["order"])
        assert np.all(order[i, k:] == -1) and np.all(np.isnan(scores[i, k:])) and np.all(np.isnan(mse[i, k:]))
        assert bool(nxt[i] > bound[i]) == bool(r["mse_next"] > bound[i]) and np.isnan(nxt[i]) == np.isnan(r["mse_next"]), (i, nxt[i], r["mse_next"])
        assert np.allclose(scores[i, :k], r["scores"], rtol=1e-6, atol=0)
        assert np.all(mse[i, :k] <= bound[i])
        worst["mse0"] = max(worst["mse0"], rd.rel(mse0[i], r["mse0"]))
        worst["mse"] = max(worst["mse"], rd.rel(mse[i, :k], r["mse"]))
        if not np.isnan(nxt[i]):
            worst["mse_next"] = max(worst["mse_next"], rd.rel(nxt[i], r["mse_next"]))
        # consistency with the read-out: the error of the pruned object is the last accepted look-ahead
        worst["readout"] = max(worst["readout"], rd.rel(after[i], mse[i, k - 1] if k else mse0[i]))
        got = dict(alpha=alpha[i, :, :b[i]], C=C[i, :b[i], :b[i]], Q=Q[i, :b[i], :b[i]], BV=BV[i, :b[i]])
        for name in got:
            worst[name] = max(worst[name], pr.rel_gap(got[name], r[name]))
    print(f"cap {cap} ny {ny}{' uniform' if uniform else ''}: kept {kept}/{P}, removed {rm.min()}..{rm.max()}, stopped by the bound "
          f"{int(np.sum(nxt > bound))}/{P}; GPU vs restatement " + " ".join(f"{k} {v:.2e}" for k, v in worst.items()) + f" (mse gate {GATE_MSE:.2e})")
    assert kept >= 0.95 * P, f"{P - kept} of {P} patches left out"
    for name in ("mse0", "mse", "mse_next", "readout"):
        assert worst[name] <= GATE_MSE, (name, worst[name])
    for name in ("alpha", "C", "Q", "BV"):
        assert worst[name] <= pr.GATE_FACTOR * pr.E64[name], (name, worst[name])
    return rm, nxt, bound


@pytest.mark.parametrize("cap,div,n,P,ny", rd.regimes())
def test_prune_rd_vs_restatement(gp, cap, div, n, P, ny):
    capi, ctx = gp
    rm, nxt, bound = _compare(capi, ctx, cap, div, n, P, ny)
    assert np.all(rm >= 9)
    if cap == -1 or ny == 3:                           # (tests/test_prune_rd_cpu.py: the regimes in which the bound stops every patch)
        assert np.all(nxt > bound)


def test_prune_rd_uniform_bound(gp):
    capi, ctx = gp
    cap, div, n, _, P = pr.REGIMES[1]
    _compare(capi, ctx, cap, div, n, P, 1, uniform=True)


BITS = [(40, 6.0, 120, 9, 3), (100, 10.0, 300, 7, 1), (-1, 10.0, 132, 3, 1)]      # test_prune_gpu.py::BITS: 64, 128 and 256 threads


@pytest.mark.parametrize("cap,div,n,P,ny", BITS)
def test_prune_rd_bit_identities(gp, cap, div, n, P, ny, monkeypatch):
    capi, ctx = gp
    states = _train(capi, ctx, cap, div, n, P, ny)
    off, x0, x1, y, _ = pr.batch(cap, n, P, ny)
    g0 = _load(capi, ctx, _params(capi, cap, div, ny), ny, states)
    b0 = g0.sizes()
    k2 = int(b0.min()) // 2
    inf = float("inf")
    # max_mse = inf: the state, removed, order and scores of Sparse.prune(keep), uniform and per patch
    target = np.array([(k2, int(b0.min()) - 7, 0, int(b0.max()) + 3, 1, 3)[i % 6] for i in range(P)], dtype=np.int32)
    for kwargs in (dict(keep=k2), dict(target=target)):
        ga, gb = _copy(g0), _copy(g0)
        rm, order, scores = ga.prune(want_trace=True, **kwargs)
        rmb, m0, nxt, ob, sb, mse = gb.prune_rd(off, x0, x1, y, max_mse=inf, want_trace=True, **kwargs)
        assert _same(_bits(ga), _bits(gb)) and np.array_equal(rm, rmb) and np.array_equal(order, ob)
        assert np.array_equal(scores, sb, equal_nan=True) and np.all(np.isnan(nxt)) and not np.any(np.isnan(m0))
        for i in range(P):
            assert not np.any(np.isnan(mse[i, :rm[i]])) and np.all(np.isnan(mse[i, rm[i]:]))
        ga.close()
        if "keep" in kwargs:
            full = (_bits(gb), rmb, m0, nxt, ob, sb, mse)
        gb.close()
    bits, rm, m0, nxt, order, scores, mse = full
    # two copies, the four-wave shape and every LDS word poisoned: the same bits, mse included
    for env, val in ((None, None), ("GPC_SPARSE_WIDE", "1"), ("GPC_POISON_LDS", "1")):
        if env:
            monkeypatch.setenv(env, val)
        ge = _copy(g0)
        out = ge.prune_rd(off, x0, x1, y, keep=k2, max_mse=inf, want_trace=True)
        if env:
            monkeypatch.delenv(env)
        assert _same(_bits(ge), bits), env
        for a, b_ in zip(out, (rm, m0, nxt, order, scores, mse)):
            assert np.array_equal(a, b_, equal_nan=True), env
        ge.close()
    # a call that stops at step k, then a call with a larger bound == one call with the larger bound, whenever the first bound did not
    # stop a patch earlier than the second would: B2 stops the chain of patch p after s2 steps, B1 = the largest error of its first
    # s1 = s2 // 2 steps (so it is within B2 and the first call stops at or after s1 and at or before s2)
    B1, B2 = np.zeros(P), np.zeros(P)
    for i in range(P):
        tr = mse[i, :rm[i]]
        B2[i] = np.sort(tr)[len(tr) // 2]
        s2 = int(np.argmax(tr > B2[i])) if np.any(tr > B2[i]) else len(tr)
        B1[i] = tr[:max(1, s2 // 2)].max() if s2 > 0 else 0.0
        assert B1[i] <= B2[i] or s2 == 0
        B1[i] = min(B1[i], B2[i])
    g1, g2 = _copy(g0), _copy(g0)
    rm1, _, n1, o1, s1, e1 = g1.prune_rd(off, x0, x1, y, keep=k2, max_mse_p=B1, want_trace=True)
    rm1b, m0b, n1b, o1b, s1b, e1b = g1.prune_rd(off, x0, x1, y, keep=k2, max_mse_p=B2, want_trace=True)
    rm2, m02, n2, o2, s2_, e2 = g2.prune_rd(off, x0, x1, y, keep=k2, max_mse_p=B2, want_trace=True)
    assert _same(_bits(g1), _bits(g2)) and np.array_equal(rm1 + rm1b, rm2) and np.array_equal(n1b, n2, equal_nan=True)
    print(f"cap {cap} ny {ny}: first call removed {rm1}, second {rm1b}, one call with the larger bound {rm2}, without a bound {rm}")
    assert np.any(rm1 > 0) and np.any(rm2 < rm)
    for i in range(P):
        for a, b_, c in ((o1, o1b, o2), (s1, s1b, s2_), (e1, e1b, e2)):
            assert np.array_equal(np.concatenate([a[i, :rm1[i]], b_[i, :rm1b[i]]]), c[i, :rm2[i]])
        # the second call starts from the error the first one left: the look-ahead is the error of the state delete_bv wrote
        assert rd.rel(m0b[i], e1[i, rm1[i] - 1] if rm1[i] else m02[i]) <= GATE_MSE
    for g in (g0, g1, g2):
        g.close()


def test_prune_rd_edges(gp):
    capi, ctx = gp
    cap, div, n, _, _ = pr.REGIMES[0]
    base = _train(capi, ctx, cap, div, n, 6, 1)
    off, x0, x1, y, _ = pr.batch(cap, n, 6, 1)
    kw = pr.kernel_kw(cap, div, 1)
    p = _params(capi, cap, div, 1)
    b = base[0][0].shape[1]
    inf = float("inf")
    # n = 0 patches between trained ones, b = 0 with points, b = 1, b = 2, a patch of 65 points and one of 1 point
    two, one = pr.prune(*base[0], 2), pr.prune(*base[0], 1)
    mk = lambda r: (r["alpha"], r["C"], r["Q"], r["BV"])
    empty = (np.zeros((1, 0)), np.zeros((0, 0)), np.zeros((0, 0)), np.zeros((0, 2)))
    states = [base[0], base[1], empty, mk(one), mk(two), base[2], base[3], base[4]]
    pts = [(x0[off[i]:off[i + 1]], x1[off[i]:off[i + 1]], y[:, off[i]:off[i + 1]]) for i in range(6)]
    cut = lambda t, m: (t[0][:m], t[1][:m], t[2][:, :m])
    # (65 points: the 60 of a patch and 5 of its neighbour's -- one point beyond the first full row of the 64 classes)
    p65 = tuple(np.concatenate([pts[3][k], cut(pts[5], 5)[k]], axis=-1) for k in range(3))
    use = [pts[0], cut(pts[1], 0), pts[2], pts[0], pts[0], cut(pts[2], 0), p65, cut(pts[4], 1)]
    o = np.concatenate([[0], np.cumsum([len(u[0]) for u in use])]).astype(np.int32)
    assert list(np.diff(o)) == [n, 0, n, n, n, 0, 65, 1] and n < 64
    X0, X1, Y = (np.concatenate([u[k] for u in use], axis=-1) for k in range(3))
    Y = np.ascontiguousarray(Y)
    g = _load(capi, ctx, p, 1, states)
    before = _bits(g)
    rm, mse0, nxt, order, scores, mse = g.prune_rd(o, X0, X1, Y, keep=1, max_mse=inf, want_trace=True)
    after = _bits(g)
    assert list(rm) == [b - 1, 0, 0, 0, 1, 0, b - 1, b - 1] and list(after[0]) == [1, b, 0, 1, 1, b, 1, 1]
    assert np.isnan(mse0[1]) and np.isnan(mse0[5]) and np.all(np.isnan(nxt))
    for arr0, arr1 in zip(before[1:], after[1:]):                              # the patches without points: every byte as it was
        assert np.array_equal(arr0[[1, 5]], arr1[[1, 5]]) and np.array_equal(arr0[[2, 3]], arr1[[2, 3]])
    assert np.isclose(mse0[2], np.mean(use[2][2] ** 2), rtol=1e-14, atol=0)
    for i in (0, 3, 4, 6, 7):
        r = rd.prune_rd(*states[i], *use[i], 1, inf, kw)
        assert np.array_equal(order[i, :rm[i]], r["order"]) and rd.rel(mse0[i], r["mse0"]) <= GATE_MSE
        assert rd.rel(mse[i, :rm[i]], r["mse"]) <= GATE_MSE, (i, mse[i, :rm[i]], r["mse"])
    g.close()
    # max_mse = 0 removes nothing on noisy data; a NaN entry of max_mse_p removes nothing; a NaN in y stops its patch at step 0 with NaN
    # errors and its neighbours do what they do without it
    g = _load(capi, ctx, p, 1, base)
    start = _bits(g)
    rm, mse0, nxt = g.prune_rd(off, x0, x1, y, keep=1, max_mse=0.0)
    assert np.all(rm == 0) and np.all(nxt > 0) and np.all(mse0 > 0) and _same(_bits(g), start)
    rm, _, nxt2 = g.prune_rd(off, x0, x1, y, keep=1, max_mse_p=np.full(6, np.nan))
    assert np.all(rm == 0) and np.array_equal(nxt2, nxt) and _same(_bits(g), start)
    yn = y.copy()
    yn[0, off[2] + 5] = np.nan
    bound = np.full(6, 2.0) * mse0
    ga, gb = _copy(g), _copy(g)
    ra = ga.prune_rd(off, x0, x1, y, keep=1, max_mse_p=bound, want_trace=True)
    rb = gb.prune_rd(off, x0, x1, yn, keep=1, max_mse_p=bound, want_trace=True)
    assert rb[0][2] == 0 and np.isnan(rb[1][2]) and np.isnan(rb[2][2]) and ra[0][2] > 0
    others = [0, 1, 3, 4, 5]
    for a, b_ in zip(ra, rb):
        assert np.array_equal(a[others], b_[others], equal_nan=True)
    for x, y_ in zip(_bits(ga), _bits(gb)):
        assert np.array_equal(x[others], y_[others], equal_nan=True)
    assert all(np.array_equal(x[2], y_[2]) for x, y_ in zip(_bits(gb), start))
    for o_ in (g, ga, gb):
        o_.close()
    # loc == last and loc == 0: the vector with a tiny alpha has the lowest score (the construction of test_prune_edges_vs_oracle)
    for where in (b - 1, 0):
        states = []
        for a, c, q, v in base:
            a = a.copy()
            a[0, where] *= 1e-3
            states.append((a, c, q, v))
        g = _load(capi, ctx, p, 1, states)
        rm, mse0, nxt, order, scores, mse = g.prune_rd(off, x0, x1, y, keep=b - 1, max_mse=inf, want_trace=True)
        alpha = g.state()[0]
        assert np.all(rm == 1) and np.all(order[:, 0] == where)
        for i in range(6):
            r = rd.prune_rd(*states[i], *pts[i], b - 1, inf, kw)
            assert rd.rel(mse[i, 0], r["mse"][0]) <= GATE_MSE and pr.rel_gap(alpha[i, :, :b - 1], r["alpha"]) <= pr.GATE_FACTOR * pr.E64["alpha"]
        g.close()


def test_prune_rd_arguments(gp):
    import torch
    capi, ctx = gp
    cap, div, n, _, _ = pr.REGIMES[0]
    states = _train(capi, ctx, cap, div, n, 6, 1)
    off, x0, x1, y, _ = pr.batch(cap, n, 6, 1)
    g = _load(capi, ctx, _params(capi, cap, div, 1), 1, states)
    L = ctx.lib
    N = int(off[-1])
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    d_off, d_x0, d_x1, d_y = t(off), t(x0), t(x1), t(y)
    tg = np.full(6, 4, dtype=np.int32)
    nanb = np.full(6, np.nan)
    before = _bits(g)
    E = capi.GPC_EINVAL
    host = lambda h, o, a, b_, c, keep, tgt, mx, mp: L.gpc_sparse_prune_rd(h, o, a, b_, c, keep, tgt, mx, mp, *[None] * 7)
    dev = lambda h, o, a, b_, c, keep, tgt, mx, mp, nt=N: L.gpc_sparse_prune_rd_dev(h, o, nt, a, b_, c, keep, tgt, mx, mp, *[None] * 7)
    hp = (off.ctypes.data, x0.ctypes.data, x1.ctypes.data, y.ctypes.data)
    dp = (d_off.data_ptr(), d_x0.data_ptr(), d_x1.data_ptr(), d_y.data_ptr())
    for entry, (o, a, b_, c) in ((host, hp), (dev, dp)):
        assert entry(None, o, a, b_, c, 4, None, 1.0, None) == E
        assert entry(g.h, o, a, b_, c, 0, None, 1.0, None) == E                  # keep < 1 with target == NULL
        assert entry(g.h, o, a, b_, c, -3, None, 1.0, None) == E
        assert entry(g.h, o, a, b_, c, 4, None, float("nan"), None) == E
        assert entry(g.h, o, a, b_, c, 4, None, -1e-300, None) == E
        assert entry(g.h, None, a, b_, c, 4, None, 1.0, None) == E               # NULL off with P > 0
        for bad in ((None, b_, c), (a, None, c), (a, b_, None)):
            assert entry(g.h, o, *bad, 4, None, 1.0, None) == E                  # NULL x0 / x1 / y with points
    assert dev(g.h, *dp, 4, None, 1.0, None, nt=-1) == E
    assert _same(_bits(g), before)
    # a NaN max_mse is not looked at when max_mse_p is given; a NaN entry of it removes nothing
    assert host(g.h, *hp, 0, tg.ctypes.data, float("nan"), nanb.ctypes.data) == capi.GPC_OK and _same(_bits(g), before)
    # noise_model 2 refused
    pq = _params(capi, cap, div, 1)
    pq.noise_model = 2
    gq = capi.Sparse(ctx, pq, 6, 1)
    assert host(gq.h, *hp, 4, None, 1.0, None) == E and dev(gq.h, *dp, 4, None, 1.0, None) == E
    gq.close()
    # P == 0
    empty = capi.Sparse(ctx, _params(capi, cap, div, 1), 0, 1)
    assert host(empty.h, None, None, None, None, 4, None, 1.0, None) == capi.GPC_OK
    assert dev(empty.h, None, None, None, None, 4, None, 1.0, None, nt=0) == capi.GPC_OK
    assert empty.prune_rd(np.zeros(1, np.int32), np.zeros(0), np.zeros(0), np.zeros((1, 0)), keep=3)[0].shape == (0,)
    empty.close()
    # the host twin == the _dev form, bit for bit
    gh, gd = _copy(g), _copy(g)
    _, mse0, _ = g.prune_rd(off, x0, x1, y, target=g.sizes())
    bound = 2.0 * mse0
    rm, m0, nxt, order, scores, mse = gh.prune_rd(off, x0, x1, y, target=tg, max_mse_p=bound, want_trace=True)
    ld = g.ld()
    d_t, d_b = t(tg), t(bound)
    d_rm = torch.full((6,), -7, dtype=torch.int32, device="cuda")
    d_o = torch.full((6, ld), -1, dtype=torch.int32, device="cuda")
    d_s, d_e = (torch.full((6, ld), float("nan"), dtype=torch.float64, device="cuda") for _ in range(2))
    d_m0, d_nx = (torch.full((6,), -1.0, dtype=torch.float64, device="cuda") for _ in range(2))
    d_st = torch.full((6,), -1, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    gd.prune_rd_dev(d_off, N, d_x0, d_x1, d_y, keep=0, target=d_t, max_mse=float("nan"), max_mse_p=d_b, removed=d_rm, order=d_o, scores=d_s,
                    mse=d_e, mse0=d_m0, mse_next=d_nx, status=d_st)
    ctx.synchronize()
    for a, b_ in ((d_rm, rm), (d_o, order), (d_s, scores), (d_e, mse), (d_m0, m0), (d_nx, nxt)):
        assert np.array_equal(a.cpu().numpy(), b_, equal_nan=True)
    assert _same(_bits(gh), _bits(gd)) and np.all(d_st.cpu().numpy() == capi.STATUS_OK) and np.any(rm > 0)
    for o_ in (gh, gd, g):
        o_.close()
    # a dead context: destroyed while a child lives (the struct stays until the child goes)
    dead = capi.Context(0)
    child = capi.Sparse(dead, _params(capi, cap, div, 1), 6, 1)
    h, dead.h = dead.h, None
    L.gpc_ctx_destroy(h)
    try:
        assert host(child.h, *hp, 4, None, 1.0, None) == E and dev(child.h, *dp, 4, None, 1.0, None) == E
    finally:
        child.close()


def test_mapping_prune_to_error(gp):
    """The smallest two-scan map of tests/mapping_cases.py: the 3 x 3 model and the disjoint two-voxel scan.  The nine old leaves have no
    points in the last scan and keep every bit; the new leaves shed vectors and satisfy their bound under predict_points."""
    import mapping_cases as mc
    capi, ctx = gp
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
    b = pt2.fetch()
    cnt = np.diff(b["off"])
    new = np.flatnonzero(cnt > 0)
    assert v.P == 11 and np.array_equal(np.flatnonzero(cnt == 0), o2n) and len(new) == 2
    yd, yc = b["y"][None, :], np.ascontiguousarray(b["rgb"])
    mp = capi.Mapping(ctx, pt2, gd2, gc2)
    before = (_bits(mp.depth), _bits(mp.rgb))
    m0d, m0c = _mse_from_readout(mp.depth, b["off"], b["x0"], b["x1"], yd), _mse_from_readout(mp.rgb, b["off"], b["x0"], b["x1"], yc)
    Bd, Bc = 2.0 * float(np.max(m0d[new])), 2.0 * float(np.max(m0c[new]))
    rmd, rmc = mp.prune_to_error(Bd, Bc)
    after = (_bits(mp.depth), _bits(mp.rgb))
    assert np.all(rmd[o2n] == 0) and np.all(rmc[o2n] == 0) and np.all(rmd[new] > 0) and np.all(rmc[new] > 0)
    for b4, af in zip(before, after):
        assert np.array_equal(b4[0] - af[0], rmd if b4 is before[0] else rmc)
        for x, y_ in zip(b4, af):
            assert np.array_equal(x[o2n], y_[o2n], equal_nan=True)
    m1d, m1c = _mse_from_readout(mp.depth, b["off"], b["x0"], b["x1"], yd), _mse_from_readout(mp.rgb, b["off"], b["x0"], b["x1"], yc)
    print(f"map: depth removed {rmd[new]}, error {m0d[new]} -> {m1d[new]} (bound {Bd:.3e}); colour removed {rmc[new]}, {m0c[new]} -> {m1c[new]} "
          f"(bound {Bc:.3e})")
    assert np.all(m1d[new] <= Bd * (1 + GATE_MSE)) and np.all(m1c[new] <= Bc * (1 + GATE_MSE))
    mp.close()
