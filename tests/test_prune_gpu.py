"""gpc_sparse_prune on the GPU: against the CPU oracle driven by delete_bv from the same state bits, at its edges, and bit for bit
against itself.

Set-up of the numeric cases (prune_ref.REGIMES, ny = 1 and ny = 3 with ref_field_delete_bug = 0): the states are produced by Sparse.add on
the GPU and read back with state(); the same bits go into the oracle (set_state) and into fresh GPU objects, so only the prune differs.
A patch is compared while the two lowest scores of every step of the oracle's run differ by more than 1e-6 relative; at most 5 % of a
case's patches may be left out.  Gate: 64 x E64 per array, relative to the array's largest magnitude in the patch (prune_ref.E64,
measured by tests/test_prune_cpu.py: alpha 1.70e-10, C 3.42e-11, Q 1.02e-11, BV 0, mean 4.36e-10, sigma 1.97e-09).  The GPU differs
from the oracle by FMA contraction and by the association of the alpha update, (alphastar / (q* + c*)) * qc against f * qc; a wrong row,
column or swap gives errors of 1e-2 or more, which the factor cannot hide.

Measured on the MI355X (worst over all cases of this module, same relative measure): C, Q and BV 0 in every case and alpha 0 for ny = 1
-- those arrays carry the oracle's bits: sp_delete_bv divides alphastar by (q* + c*) before it multiplies, like the oracle, and its
downdate has no product that feeds a sum, so nothing contracts.  For ny = 3 the alpha update `alpha -= alphastar * m` contracts into one
FMA: alpha 4.8e-16 over the numeric cases, 5.1e-15 in the three-removal case with the reference's multiply (gate 1.1e-08).  mean 3.6e-14
(gate 2.8e-08) and sigma 1.6e-12 (gate 1.3e-07) are the read-out kernel's own summation order.  No patch was left out (smallest
relative distance of the two lowest scores: 4.4e-05).
"""
import numpy as np
import pytest

import prune_ref as pr
from gp_compressor_amd import synth

pytestmark = pytest.mark.gpu
XS0, XS1 = synth.grid(pr.RES, 20)


@pytest.fixture(scope="module")
def gp():
    from gp_compressor_amd import capi
    capi.load()
    ctx = capi.Context(0)
    yield capi, ctx
    ctx.close()


def _params(capi, cap, div, ny, bug=0):
    return capi.default_params_sparse(ny, ref_field_delete_bug=bug, **pr.kernel_kw(cap, div, ny))


_trained = {}


def _train(capi, ctx, cap, div, n, P, ny, bug=0):
    """the regime's batch trained by Sparse.add on the GPU: per-patch states as the oracle takes them (computed once per regime)"""
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


def _unpack(g, i):
    b = int(g.sizes()[i])
    alpha, C, Q, BV = g.state()
    return dict(alpha=alpha[i, :, :b], C=C[i, :b, :b], Q=Q[i, :b, :b], BV=BV[i, :b])


def _against_oracle(capi, ctx, oracle, states, cap, div, ny, keep, bug=0, score_tol=0.0, gate=True):
    """prune `states` on the GPU and on the oracle; asserts order, removed and (gate) the arrays of every kept patch.  Returns the worst
    gap per array, the kept patches, the GPU trace and the oracle's results."""
    kw = pr.kernel_kw(cap, div, ny)
    g = _load(capi, ctx, _params(capi, cap, div, ny, bug), ny, states)
    rm, order, scores = g.prune(keep=keep, score_tol=score_tol, want_trace=True)
    b = g.sizes()
    alpha, C, Q, BV = g.state()
    f, s, _ = g.predict(XS0, XS1)
    g.close()
    orc = pr.run_oracle(oracle, states, cap, div, ny, keep, XS0, XS1, score_tol=score_tol, bug=bug)
    worst, kept = {k: 0.0 for k in pr.ARRAYS}, []
    for i, o in enumerate(orc):
        if not o["gap"] > pr.GAP_MIN:
            continue
        kept.append(i)
        k = len(o["order"])
        assert rm[i] == k and b[i] == o["alpha"].shape[1], (i, rm[i], k, b[i])
        assert np.array_equal(order[i, :k], o["order"]), (i, order[i, :k], o["order"])
        assert np.all(order[i, k:] == -1) and np.all(np.isnan(scores[i, k:]))
        got = dict(alpha=alpha[i, :, :b[i]], C=C[i, :b[i], :b[i]], Q=Q[i, :b[i], :b[i]], BV=BV[i, :b[i]], mean=f[i], sigma=s[i])
        ref = dict(o, mean=o["pred"][0], sigma=o["pred"][1])
        for name in pr.ARRAYS:
            worst[name] = max(worst[name], pr.rel_gap(got[name], ref[name]))
    if gate:
        for name in pr.ARRAYS:
            print(f"cap {cap} ny {ny} keep {keep}: GPU vs oracle, {name}: {worst[name]:.3e} (gate {pr.GATE_FACTOR * pr.E64[name]:.3e})")
        for name in pr.ARRAYS:
            assert worst[name] <= pr.GATE_FACTOR * pr.E64[name], (name, worst[name])
    return worst, kept, (rm, order, scores), orc


@pytest.mark.parametrize("cap,div,n,P,ny,keep", pr.case_ids())
def test_prune_vs_oracle(gp, oracle, cap, div, n, P, ny, keep):
    capi, ctx = gp
    states = _train(capi, ctx, cap, div, n, P, ny)
    if cap == -1:
        assert min(s[0].shape[1] for s in states) > 128         # the regime starts above 128 vectors
    worst, kept, _, orc = _against_oracle(capi, ctx, oracle, states, cap, div, ny, keep)
    print(f"cap {cap} ny {ny} keep {keep}: kept {len(kept)}/{P}, smallest score gap {min(o['gap'] for o in orc):.2e}")
    assert len(kept) >= 0.95 * P, f"{P - len(kept)} of {P} patches have two lowest scores within {pr.GAP_MIN} of each other"


def test_prune_field_bug_short_chain(gp, oracle):
    """ny = 3 with the reference's multiply (ref_field_delete_bug = 1): three removals against the oracle"""
    capi, ctx = gp
    cap, div, n, _, _ = pr.REGIMES[0]
    states = _train(capi, ctx, cap, div, n, 6, 3, bug=1)
    assert len({s[0].shape[1] for s in states}) == 1
    worst, kept, (rm, _, _), _ = _against_oracle(capi, ctx, oracle, states, cap, div, 3, states[0][0].shape[1] - 3, bug=1)
    assert len(kept) == 6 and np.all(rm == 3)


def test_prune_edges_vs_oracle(gp, oracle):
    capi, ctx = gp
    cap, div, n, _, _ = pr.REGIMES[0]
    base = _train(capi, ctx, cap, div, n, 6, 1)
    b = base[0][0].shape[1]
    # loc == last and loc == 0: the vector with a tiny alpha has the lowest score
    for where in (b - 1, 0):
        states = []
        for a, c, q, v in base:
            a = a.copy()
            a[0, where] *= 1e-3
            states.append((a, c, q, v))
        _, kept, (rm, order, _), _ = _against_oracle(capi, ctx, oracle, states, cap, div, 1, b - 1)
        assert len(kept) == 6 and np.all(rm == 1) and np.all(order[:, 0] == where)
    # b = 2 -> 1; b = 1 and b = 0 are left alone
    two = pr.prune(*base[0], 2)
    one = pr.prune(*base[0], 1)
    mk = lambda r: (r["alpha"], r["C"], r["Q"], r["BV"])
    empty = (np.zeros((1, 0)), np.zeros((0, 0)), np.zeros((0, 0)), np.zeros((0, 2)))
    states = [mk(two), mk(one), empty]
    g = _load(capi, ctx, _params(capi, cap, div, 1), 1, states)
    before = _bits(g)
    rm, order, scores = g.prune(keep=1, want_trace=True)
    after = _bits(g)
    assert list(rm) == [1, 0, 0] and list(after[0]) == [1, 1, 0]
    for arr0, arr1 in zip(before[1:], after[1:]):
        assert np.array_equal(arr0[1:], arr1[1:])
    g.close()
    _against_oracle(capi, ctx, oracle, states[:1], cap, div, 1, 1)
    # score mode: a NaN alpha at an index != 0 is never chosen
    states = []
    for a, c, q, v in base:
        a = a.copy()
        a[0, 3] = np.nan
        states.append((a, c, q, v))
    tol = float(np.median(pr.scores_of(*base[0][:3])))
    _, kept, (rm, order, scores), orc = _against_oracle(capi, ctx, oracle, states, cap, div, 1, b, score_tol=tol, gate=False)
    assert len(kept) == 6 and np.all(rm >= 1)
    for i in range(6):
        assert not np.any(np.isnan(scores[i, :rm[i]])) and np.array_equal(scores[i, :rm[i]] < tol, np.ones(rm[i], dtype=bool))
        assert np.allclose(scores[i, :rm[i]], orc[i]["scores"], rtol=1e-6)


def test_prune_nan_status(gp, oracle):
    """a patch whose C(0,0) turns NaN reports GPC_STATUS_NAN (sticky, as after an add); its neighbour stays OK"""
    import torch
    capi, ctx = gp
    cap, div, n, _, _ = pr.REGIMES[0]
    base = _train(capi, ctx, cap, div, n, 6, 1)
    a, c, q, v = base[0]
    c = c.copy()
    c[0, 0] = np.nan
    g = _load(capi, ctx, _params(capi, cap, div, 1), 1, [(a, c, q, v), base[1], (a, c, q, v)])
    keep = a.shape[1] - 2
    status = torch.full((3,), -1, dtype=torch.int32, device="cuda")
    removed = torch.full((3,), -1, dtype=torch.int32, device="cuda")
    target = torch.tensor([keep, keep, a.shape[1]], dtype=torch.int32, device="cuda")
    g.prune_dev(target=target, removed=removed, status=status)
    ctx.synchronize()
    # the oracle on the first state: the NaN score at index 0 sticks, the vector goes, and its NaN c* spreads over C
    op = pr.oracle_params(oracle, cap, div, 1)
    o = oracle.Sparse(op, a.shape[1] + 2)
    o.set_state(a, c, q, v)
    r = pr.oracle_prune(o, keep)
    assert r["order"][0] == 0 and np.isnan(r["C"][0, 0])
    assert removed.cpu().tolist() == [2, 2, 0]
    assert status.cpu().tolist() == [capi.STATUS_NAN, capi.STATUS_OK, capi.STATUS_OK]      # nothing removed: the status is not touched
    assert np.isnan(_unpack(g, 0)["C"][0, 0])
    status.fill_(-1)
    g.prune_dev(keep=a.shape[1], removed=removed, status=status)     # sticky: a call that removes nothing reports it again
    ctx.synchronize()
    assert removed.cpu().tolist() == [0, 0, 0] and status.cpu().tolist() == [capi.STATUS_NAN, capi.STATUS_OK, capi.STATUS_OK]
    g.close()


BITS = [(40, 6.0, 120, 9, 3), (100, 10.0, 300, 7, 1), (-1, 10.0, 132, 3, 1)]


@pytest.mark.parametrize("cap,div,n,P,ny", BITS)
def test_prune_bit_identities(gp, cap, div, n, P, ny, monkeypatch):
    capi, ctx = gp
    states = _train(capi, ctx, cap, div, n, P, ny)
    g0 = _load(capi, ctx, _params(capi, cap, div, ny), ny, states)
    b0 = g0.sizes()
    start = _bits(g0)
    k1, k2 = int(b0.min()) - 7, int(b0.min()) // 2
    # target >= b with score_tol = 0: not a byte moves
    ga = _copy(g0)
    assert np.all(ga.prune(keep=int(b0.max())) == 0) and _same(_bits(ga), start)
    assert np.all(ga.prune(target=b0 + 1) == 0) and _same(_bits(ga), start)
    # k1 then k2 == k2 on a copy; the traces concatenate; entries beyond removed[p] keep their sentinel
    rm1, o1, s1 = ga.prune(keep=k1, want_trace=True)
    rm2, o2, s2 = ga.prune(keep=k2, want_trace=True)
    gb = _copy(g0)
    rm, o, s = gb.prune(keep=k2, want_trace=True)
    assert _same(_bits(ga), _bits(gb)) and np.array_equal(rm, rm1 + rm2) and np.all(gb.sizes() == k2)
    for i in range(P):
        assert np.array_equal(o[i, :rm[i]], np.concatenate([o1[i, :rm1[i]], o2[i, :rm2[i]]]))
        assert np.array_equal(s[i, :rm[i]], np.concatenate([s1[i, :rm1[i]], s2[i, :rm2[i]]]))
        assert np.all(o[i, rm[i]:] == -1) and np.all(np.isnan(s[i, rm[i]:]))
    # two copies: the same bits
    gc = _copy(g0)
    rmc, oc, sc = gc.prune(keep=k2, want_trace=True)
    assert _same(_bits(gc), _bits(gb)) and np.array_equal(oc, o) and np.array_equal(sc, s, equal_nan=True)
    # a per-patch target == the uniform calls, patch by patch (entries below 1 count as 1)
    target = np.array([(k2, k1, 0, int(b0.max()) + 3, 1, 3)[i % 6] for i in range(P)], dtype=np.int32)
    gt = _copy(g0)
    rmt, ot, stt = gt.prune(target=target, want_trace=True)
    bt = _bits(gt)
    for v in sorted(set(target.tolist())):
        gu = _copy(g0)
        rmu, ou, su = gu.prune(keep=max(1, v), want_trace=True)
        bu = _bits(gu)
        for i in np.nonzero(target == v)[0]:
            assert rmt[i] == rmu[i] and np.array_equal(ot[i], ou[i]) and np.array_equal(stt[i], su[i], equal_nan=True)
            assert all(np.array_equal(x[i], y[i], equal_nan=True) for x, y in zip(bt, bu))
        gu.close()
    # the same bits in the four-wave shape and with every LDS word poisoned before the call
    for env in ("GPC_SPARSE_WIDE", "GPC_POISON_LDS"):
        monkeypatch.setenv(env, "1")
        ge = _copy(g0)
        rme, oe, se = ge.prune(keep=k2, want_trace=True)
        monkeypatch.delenv(env)
        assert _same(_bits(ge), _bits(gb)) and np.array_equal(oe, o) and np.array_equal(se, s, equal_nan=True), env
        ge.close()
    # the point counters are not touched, and the pruned object still takes points: the basis grows again, up to its capacity
    if cap > 0:
        off, x0, x1, y, perm = pr.batch(cap, n, P, ny)
        assert np.all(gb.add(off, x0, x1, y, perm) == 0)
        assert np.all(gb.sizes() > k2) and np.all(gb.sizes() <= cap)
    for g in (g0, ga, gb, gc, gt):
        g.close()


def test_prune_arguments(gp):
    import torch
    capi, ctx = gp
    cap, div, n, _, _ = pr.REGIMES[0]
    states = _train(capi, ctx, cap, div, n, 6, 1)
    g = _load(capi, ctx, _params(capi, cap, div, 1), 1, states)
    L = ctx.lib
    tg = np.full(6, 4, dtype=np.int32)
    before = _bits(g)
    for entry in (L.gpc_sparse_prune, L.gpc_sparse_prune_dev):
        assert entry(None, 4, None, 0.0, None, None, None, None) == capi.GPC_EINVAL
        assert entry(g.h, 0, None, 0.0, None, None, None, None) == capi.GPC_EINVAL           # keep < 1 with target == NULL
        assert entry(g.h, -3, None, 0.0, None, None, None, None) == capi.GPC_EINVAL
        assert entry(g.h, 4, None, float("nan"), None, None, None, None) == capi.GPC_EINVAL
        assert entry(g.h, 4, None, -1e-300, None, None, None, None) == capi.GPC_EINVAL
    assert L.gpc_sparse_prune(g.h, 0, tg.ctypes.data, float("nan"), None, None, None, None) == capi.GPC_EINVAL
    assert _same(_bits(g), before)
    # P == 0
    empty = capi.Sparse(ctx, _params(capi, cap, div, 1), 0, 1)
    for entry in (L.gpc_sparse_prune, L.gpc_sparse_prune_dev):
        assert entry(empty.h, 4, None, 0.0, None, None, None, None) == capi.GPC_OK
    assert empty.prune(keep=3).shape == (0,)
    empty.close()
    # the host twin == the _dev form; +inf prunes to one vector; a target with keep unused
    gh, gd = _copy(g), _copy(g)
    rm, order, scores = gh.prune(target=tg, score_tol=0.0, want_trace=True)
    ld = g.ld()
    d_t = torch.from_numpy(tg).cuda()
    d_rm = torch.full((6,), -7, dtype=torch.int32, device="cuda")
    d_o = torch.full((6, ld), -1, dtype=torch.int32, device="cuda")
    d_s = torch.full((6, ld), float("nan"), dtype=torch.float64, device="cuda")
    gd.prune_dev(keep=0, target=d_t, removed=d_rm, order=d_o, scores=d_s)
    ctx.synchronize()
    assert np.array_equal(d_rm.cpu().numpy(), rm) and np.array_equal(d_o.cpu().numpy(), order)
    assert np.array_equal(d_s.cpu().numpy(), scores, equal_nan=True) and _same(_bits(gh), _bits(gd))
    assert np.all(gh.sizes() == 4)
    assert np.all(gh.prune(keep=4, score_tol=float("inf")) == 3) and np.all(gh.sizes() == 1)
    for o in (gh, gd, g):
        o.close()
    # a dead context: destroyed while a child lives (the struct stays until the child goes)
    dead = capi.Context(0)
    child = capi.Sparse(dead, _params(capi, cap, div, 1), 2, 1)
    h, dead.h = dead.h, None
    L.gpc_ctx_destroy(h)
    try:
        for entry in (L.gpc_sparse_prune, L.gpc_sparse_prune_dev):
            assert entry(child.h, 4, None, 0.0, None, None, None, None) == capi.GPC_EINVAL
    finally:
        child.close()
