"""gpc_sparse_quantize_rd and gpc_sparse_dequantize on the GPU: against the NumPy restatement (tests/quantize_ref.py) from the same state
bits, against the read-out, against themselves in every workgroup shape, and at their edges.

Set-up of the numeric cases (prune_ref.REGIMES, ny = 1 and 3), as tests/test_prune_rd_gpu.py: the states are produced by Sparse.add on the
GPU and read back with state(); the same bits go into the restatement and into fresh GPU objects.  The points the error is taken on are the
points the states were trained on.  Bounds: B_p = 1.1 mse0_p with mse0 from a first call.  `bits` is compared for the patches of which, in
the restatement's run, no evaluated error lies within prune_rd_ref.BAND (1e-6 relative) of B_p; at most 5 % of a case's patches may be left
out.  range is compared bit for bit on every patch, the codes bit for bit wherever the widths agree.  Gates: mse0, mse_q and the evaluated
curve entries within prune_ref.GATE_FACTOR (64) x the E64 figure of quantize_ref (prune_rd_ref.E64_MSE = 7.84e-11 unless the CPU
measurement of tests/test_quantize_cpu.py::test_e64_mse_q had to record a larger one).

Measured on the MI355X (gate 64 x 7.84e-11 = 5.02e-09): mse0, mse_q and curve against the restatement at most 2.7e-14 relative over the
regimes (capacity 16, ny = 1; ny = 3 stays below 6e-16) and 1.1e-13 on the synthetic edge states; bits, codes and range equal in every
patch, none left out; widths at 1.1 mse0: depth 9..13, colour 3..6; the read-out of a decoded object against mse_q 0 (ny = 1) and 1.3e-16.
"""
import numpy as np
import pytest

import prune_rd_ref as rd
import prune_ref as pr
import quantize_ref as qr

pytestmark = pytest.mark.gpu
GATE_MSE = pr.GATE_FACTOR * qr.e64()


@pytest.fixture(scope="module")
def gp():
    from gp_compressor_amd import capi
    capi.load()
    ctx = capi.Context(0)
    yield capi, ctx
    ctx.close()


# ---- the helpers of tests/test_prune_rd_gpu.py (copied: that file stays as it is) ------------------------------------------------------

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


def _bits(g):
    """everything the object holds, padding included"""
    return (g.sizes(),) + tuple(g.state())


def _same(a, b):
    return all(np.array_equal(x, y, equal_nan=True) for x, y in zip(a, b))


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


# ---- this module's own -------------------------------------------------------------------------------------------------------------------

def _eq_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


def _check_patch(i, r, out, b, in_band_ok=True):
    """one patch of a quantize_rd result (bits, qa, qb, rng, mse0, mse_q, curve) against the restatement's run r; returns
    (compared: the widths had to agree, worst relative gap of the errors)"""
    bits, qa, qb, rng, mse0, mseq, curve = out
    worst = 0.0
    if np.isnan(float(r["mse0"])):
        assert np.isnan(mse0[i])
    else:
        worst = rd.rel(mse0[i], r["mse0"])
    if r["escaped"]:
        assert bits[i] == 0 and np.isnan(mseq[i]) and np.all(np.isnan(rng[i])) and not qa[i].any() and not qb[i].any()
        assert np.all(np.isnan(curve[i]))
        return True, worst
    assert _eq_bits(rng[i], r["range"]), (i, rng[i], r["range"])
    compared = r["band"] > rd.BAND
    if compared or not in_band_ok:
        assert bits[i] == r["bits"], (i, bits[i], r["bits"], r["band"])
    w = int(bits[i])
    ev = ~np.isnan(r["curve"]) if w == r["bits"] else np.zeros(16, dtype=bool)
    if w == r["bits"]:
        assert np.array_equal(np.isnan(curve[i]), np.isnan(r["curve"])), (i, curve[i], r["curve"])
        worst = max(worst, rd.rel(curve[i][ev], r["curve"][ev]))
        if w > 0:
            assert _eq_bits(qa[i, :, :b], r["q_alpha"]) and _eq_bits(qb[i, :b], r["q_bv"]), i
            assert mseq[i] == curve[i, w - 1] and mseq[i] <= r["bound"]
        else:
            assert np.isnan(mseq[i]) and not qa[i].any() and not qb[i].any()
    assert not qa[i, :, b:].any() and not qb[i, b:].any()                          # entries at and beyond b: as the caller left them
    return compared, worst


def _compare(capi, ctx, cap, div, n, P, ny, factor=1.1):
    kw = pr.kernel_kw(cap, div, ny)
    states = _train(capi, ctx, cap, div, n, P, ny)
    off, x0, x1, y, _ = pr.batch(cap, n, P, ny)
    g = _load(capi, ctx, _params(capi, cap, div, ny), ny, states)
    start = _bits(g)
    first = g.quantize_rd(off, x0, x1, y)                                          # max_mse = inf: bits_min, and mse0
    mse0 = first[4]
    assert np.all(first[0] == 1) and np.allclose(mse0, _mse_from_readout(g, off, x0, x1, y), rtol=GATE_MSE, atol=0)
    bound = factor * mse0
    out = g.quantize_rd(off, x0, x1, y, max_mse_p=bound, want_curve=True)
    again = g.quantize_rd(off, x0, x1, y, max_mse_p=bound, want_curve=True)
    assert _same(_bits(g), start)                                                 # g is only read
    assert all(np.array_equal(a, b_, equal_nan=True) for a, b_ in zip(out, again))
    assert np.array_equal(out[4], mse0)
    g.close()
    kept, worst = 0, 0.0
    for i, st in enumerate(states):
        s = slice(off[i], off[i + 1])
        r = qr.quantize_rd(st[0], st[3], x0[s], x1[s], y[:, s], float(bound[i]), kw)
        c, w = _check_patch(i, r, out, st[0].shape[1])
        kept += c
        worst = max(worst, w)
    bits = out[0]
    print(f"cap {cap} ny {ny} B = {factor} mse0: kept {kept}/{P}, widths {bits.min()}..{bits.max()}, GPU vs restatement (mse0, mse_q, curve) "
          f"{worst:.2e} (gate {GATE_MSE:.2e})")
    assert kept >= 0.95 * P, f"{P - kept} of {P} patches left out"
    assert worst <= GATE_MSE
    assert np.all(bits >= 1)
    return states, (off, x0, x1, y), out


@pytest.mark.parametrize("cap,div,n,P,ny", rd.regimes())
def test_quantize_rd_vs_restatement(gp, cap, div, n, P, ny):
    capi, ctx = gp
    _compare(capi, ctx, cap, div, n, P, ny)


BITS = [(40, 6.0, 120, 9, 3), (100, 10.0, 300, 7, 1), (-1, 10.0, 132, 3, 1)]      # test_prune_gpu.py::BITS: 64, 128 and 256 threads


@pytest.mark.parametrize("cap,div,n,P,ny", BITS)
def test_quantize_rd_curve_and_shapes(gp, cap, div, n, P, ny, monkeypatch):
    """max_mse = 0: the whole curve and bits 0; max_mse = +inf: bits_min; the four-wave shape and poisoned LDS: the same bits"""
    capi, ctx = gp
    kw = pr.kernel_kw(cap, div, ny)
    states = _train(capi, ctx, cap, div, n, P, ny)
    off, x0, x1, y, _ = pr.batch(cap, n, P, ny)
    g = _load(capi, ctx, _params(capi, cap, div, ny), ny, states)
    start = _bits(g)
    out = g.quantize_rd(off, x0, x1, y, max_mse=0.0, want_curve=True)
    bits, qa, qb, rng, mse0, mseq, curve = out
    assert np.all(bits == 0) and np.all(np.isnan(mseq)) and not np.any(np.isnan(curve)) and not qa.any() and not qb.any()
    worst = 0.0
    for i, st in enumerate(states):
        s = slice(off[i], off[i + 1])
        r = qr.quantize_rd(st[0], st[3], x0[s], x1[s], y[:, s], 0.0, kw)
        assert r["bits"] == 0
        worst = max(worst, _check_patch(i, r, out, st[0].shape[1], in_band_ok=False)[1])
    print(f"cap {cap} ny {ny}: 16-entry curve GPU vs restatement {worst:.2e} (gate {GATE_MSE:.2e}); patch 0: {curve[0]}, mse0 {mse0[0]:.4e}")
    assert worst <= GATE_MSE
    for lo in (1, 7, 16):
        o = g.quantize_rd(off, x0, x1, y, bits_min=lo, max_mse=float("inf"), want_curve=True)
        assert np.all(o[0] == lo) and np.array_equal(o[5], curve[:, lo - 1])
        assert np.all(np.isnan(np.delete(o[6], lo - 1, axis=1)))
    bound = 1.1 * mse0
    ref = g.quantize_rd(off, x0, x1, y, max_mse_p=bound, want_curve=True)
    for env in ("GPC_SPARSE_WIDE", "GPC_POISON_LDS"):
        monkeypatch.setenv(env, "1")
        o = g.quantize_rd(off, x0, x1, y, max_mse_p=bound, want_curve=True)
        monkeypatch.delenv(env)
        assert all(np.array_equal(a, b_, equal_nan=True) for a, b_ in zip(o, ref)), env
    assert _same(_bits(g), start)
    g.close()


@pytest.mark.parametrize("cap,div,n,P,ny", BITS)
def test_dequantize(gp, cap, div, n, P, ny):
    capi, ctx = gp
    kw = pr.kernel_kw(cap, div, ny)
    states = _train(capi, ctx, cap, div, n, P, ny)
    off, x0, x1, y, _ = pr.batch(cap, n, P, ny)
    p = _params(capi, cap, div, ny)
    g = _load(capi, ctx, p, ny, states)
    mse0 = g.quantize_rd(off, x0, x1, y)[4]
    bits, qa, qb, rng, _, mseq = g.quantize_rd(off, x0, x1, y, max_mse_p=1.1 * mse0)
    b = g.sizes()
    g.close()
    assert np.all(bits >= 1)
    # the target: an object that holds the raw states (C and Q included); patch 1 is declared raw (bits 0) and must keep every bit
    h = _load(capi, ctx, p, ny, states)
    before = _bits(h)
    w = bits.copy()
    w[1] = 0
    cnt = b.copy()
    cnt[1] = 0                                                                     # (not looked at for a raw patch)
    h.dequantize(cnt, w, qa, qb, rng)
    after = _bits(h)
    for x, y_ in zip(before, after):
        assert np.array_equal(x[1], y_[1])
    sizes, alpha, C, Q, BV = after
    ld = h.ld()
    worst = 0.0
    err = _mse_from_readout(h, off, x0, x1, y)
    for i in range(P):
        if i == 1:
            continue
        a2, v2 = qr.dequantize(qa[i, :, :b[i]], qb[i, :b[i]], rng[i], int(bits[i]))
        assert sizes[i] == b[i] and _eq_bits(alpha[i, :, :b[i]], a2) and _eq_bits(BV[i, :b[i]], v2)
        assert not alpha[i, :, b[i]:].any() and not BV[i, b[i]:].any() and not C[i].any() and not Q[i].any()
        worst = max(worst, rd.rel(err[i], mseq[i]))
    print(f"cap {cap} ny {ny}: widths {bits}, read-out of the dequantised object vs mse_q {worst:.2e} (gate {GATE_MSE:.2e})")
    assert worst <= GATE_MSE
    # arguments: counts and widths out of range, NULL arrays
    L, E = ctx.lib, capi.GPC_EINVAL
    now = _bits(h)
    args = [np.ascontiguousarray(a) for a in (cnt, w, qa, qb, rng)]
    ptr = [a.ctypes.data for a in args]
    for k in range(5):
        assert L.gpc_sparse_dequantize(h.h, *[None if j == k else ptr[j] for j in range(5)]) == E
        assert L.gpc_sparse_dequantize_dev(h.h, *[None if j == k else ptr[j] for j in range(5)]) == E
    assert L.gpc_sparse_dequantize(None, *ptr) == E and L.gpc_sparse_dequantize_dev(None, *ptr) == E
    for arr, bad in ((0, -1), (0, ld + 1), (1, -1), (1, 17)):
        a = args[arr].copy()
        a[0] = bad
        assert L.gpc_sparse_dequantize(h.h, *[a.ctypes.data if j == arr else ptr[j] for j in range(5)]) == E
    assert _same(_bits(h), now)
    h.close()


def _synthetic(rng, ny, b, n, kw, bad=False):
    """a state of b vectors and n points it fits up to noise: (alpha, C, Q, BV), (x0, x1, y)"""
    alpha, BV = rng.normal(size=(ny, b)), rng.uniform(-0.07, 0.07, size=(b, 2))
    x0, x1 = rng.uniform(-0.07, 0.07, n), rng.uniform(-0.07, 0.07, n)
    k = rd.kernel_matrix(BV, x0, x1, kw["sigmaf_sq"], kw["l_sq"], np.float64)
    y = alpha @ k.T + 1e-2 * rng.normal(size=(ny, n))
    if bad:
        alpha[ny - 1, b // 2] = np.nan
    return (alpha, np.zeros((b, b)), np.zeros((b, b)), BV), (x0, x1, np.ascontiguousarray(y))


def _batch_of(pts, ny):
    off = np.concatenate([[0], np.cumsum([len(p[0]) for p in pts])]).astype(np.int32)
    return off, np.concatenate([p[0] for p in pts]), np.concatenate([p[1] for p in pts]), np.ascontiguousarray(np.concatenate([p[2] for p in pts], axis=1))


@pytest.mark.parametrize("cap,div,ny,big", [(16, 3.0, 1, 32), (64, 8.0, 3, 80)])
def test_quantize_rd_edges(gp, cap, div, ny, big):
    """b = 1, b = ld (cap 64: more vectors than the workgroup has threads), n = 1, 64, 65 and 0, an empty basis, a NaN alpha"""
    capi, ctx = gp
    kw = pr.kernel_kw(cap, div, ny)
    rng = np.random.default_rng(cap)
    shape = [(1, 60, False), (big, 64, False), (5, 65, False), (5, 1, False), (5, 0, False), (0, 10, False), (5, 10, True), (big - 15, 130, False)]
    made = [_synthetic(rng, ny, b, n, kw, bad) for b, n, bad in shape]
    states, pts = [m[0] for m in made], [m[1] for m in made]
    off, x0, x1, y = _batch_of(pts, ny)
    g = _load(capi, ctx, _params(capi, cap, div, ny), ny, states)
    assert g.ld() == big
    start = _bits(g)
    mse0 = g.quantize_rd(off, x0, x1, y)[4]
    assert np.isnan(mse0[4]) and np.isnan(mse0[6]) and np.isclose(mse0[5], np.mean(pts[5][2] ** 2), rtol=1e-14, atol=0)
    bound = 1.1 * mse0
    bound[3] = 4.0 * mse0[3]                         # (one point: any error is a large multiple of the state's own)
    out = g.quantize_rd(off, x0, x1, y, max_mse_p=bound, want_curve=True)
    worst = 0.0
    for i, (st, p) in enumerate(zip(states, pts)):
        r = qr.quantize_rd(st[0], st[3], *p, float(bound[i]), kw)
        assert r["escaped"] == (i in (4, 5, 6))
        worst = max(worst, _check_patch(i, r, out, st[0].shape[1])[1])
    print(f"cap {cap} ny {ny}: widths {out[0]}, GPU vs restatement {worst:.2e}")
    assert worst <= GATE_MSE and np.all(out[0][[0, 1, 2, 7]] >= 1)
    # bits_min == bits_max; a NaN entry of max_mse_p
    o = g.quantize_rd(off, x0, x1, y, bits_min=5, bits_max=5, max_mse=float("inf"), want_curve=True)
    assert list(o[0]) == [5, 5, 5, 5, 0, 0, 0, 5] and np.all(np.isnan(np.delete(o[6], 4, axis=1)))
    o0 = g.quantize_rd(off, x0, x1, y, bits_min=5, bits_max=5, max_mse=0.0, want_curve=True)
    assert np.all(o0[0] == 0) and np.array_equal(o0[6], o[6], equal_nan=True) and not o0[1].any() and _eq_bits(o0[3], o[3])
    nb = bound.copy()
    nb[7] = np.nan
    on = g.quantize_rd(off, x0, x1, y, max_mse_p=nb, want_curve=True)
    assert on[0][7] == 0 and np.isnan(on[5][7]) and not np.any(np.isnan(on[6][7])) and not on[1][7].any()
    for a, b_ in zip(on, out):
        assert np.array_equal(a[:7], b_[:7], equal_nan=True)
    assert _same(_bits(g), start)
    g.close()


def test_quantize_rd_arguments_and_dev(gp):
    import torch
    capi, ctx = gp
    cap, div, n, _, _ = pr.REGIMES[0]
    ny, P = 1, 6
    states = _train(capi, ctx, cap, div, n, P, ny)
    off, x0, x1, y, _ = pr.batch(cap, n, P, ny)
    g = _load(capi, ctx, _params(capi, cap, div, ny), ny, states)
    ld, L, E, N = g.ld(), ctx.lib, capi.GPC_EINVAL, int(off[-1])
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    d_off, d_x0, d_x1, d_y = t(off), t(x0), t(x1), t(y)

    def fresh():
        """device outputs holding a sentinel: bits, q_alpha, q_bv (int16 storage), range, mse0, mse_q, curve, status"""
        return [torch.full((P,), -7, dtype=torch.int32, device="cuda"), torch.full((P, ny, ld), -3, dtype=torch.int16, device="cuda"),
                torch.full((P, ld, 2), -3, dtype=torch.int16, device="cuda"), torch.full((P, ny + 2, 2), -1.0, dtype=torch.float32, device="cuda"),
                torch.full((P,), -1.0, dtype=torch.float64, device="cuda"), torch.full((P,), -1.0, dtype=torch.float64, device="cuda"),
                torch.full((P, 16), -1.0, dtype=torch.float64, device="cuda"), torch.full((P,), -9, dtype=torch.int32, device="cuda")]

    def host_outs():
        return [np.full(P, -7, np.int32), np.full((P, ny, ld), 65533, np.uint16), np.full((P, ld, 2), 65533, np.uint16),
                np.full((P, ny + 2, 2), -1.0, np.float32), np.full(P, -1.0), np.full(P, -1.0), np.full((P, 16), -1.0), np.full(P, -9, np.int32)]

    hp = (off.ctypes.data, x0.ctypes.data, x1.ctypes.data, y.ctypes.data)
    dp = (d_off.data_ptr(), d_x0.data_ptr(), d_x1.data_ptr(), d_y.data_ptr())
    ho, do = host_outs(), fresh()
    sentinel_h, sentinel_d = [a.copy() for a in ho], [a.clone() for a in do]
    torch.cuda.synchronize()
    host = lambda h, o, a, b_, c, lo, hi, mx, mp: L.gpc_sparse_quantize_rd(h, o, a, b_, c, lo, hi, mx, mp, *[x.ctypes.data for x in ho])
    dev = lambda h, o, a, b_, c, lo, hi, mx, mp, nt=N: L.gpc_sparse_quantize_rd_dev(h, o, nt, a, b_, c, lo, hi, mx, mp, *[x.data_ptr() for x in do])
    before = _bits(g)
    nanb = np.full(P, np.nan)
    pq = _params(capi, cap, div, ny)
    pq.noise_model = 2
    gq = capi.Sparse(ctx, pq, P, 1)
    for entry, (o, a, b_, c) in ((host, hp), (dev, dp)):
        assert entry(None, o, a, b_, c, 1, 16, 1.0, None) == E
        for lo, hi in ((0, 16), (1, 17), (9, 8), (-1, 4)):
            assert entry(g.h, o, a, b_, c, lo, hi, 1.0, None) == E
        assert entry(g.h, o, a, b_, c, 1, 16, float("nan"), None) == E
        assert entry(g.h, o, a, b_, c, 1, 16, -1e-300, None) == E
        assert entry(g.h, None, a, b_, c, 1, 16, 1.0, None) == E               # NULL off with P > 0
        for bad in ((None, b_, c), (a, None, c), (a, b_, None)):
            assert entry(g.h, o, *bad, 1, 16, 1.0, None) == E                  # NULL x0 / x1 / y with points
        assert entry(gq.h, o, a, b_, c, 1, 16, 1.0, None) == E                 # noise_model 2
    assert dev(g.h, *dp, 1, 16, 1.0, None, nt=-1) == E
    gq.close()
    ctx.synchronize()
    assert all(np.array_equal(a, b_) for a, b_ in zip(ho, sentinel_h)) and all(torch.equal(a, b_) for a, b_ in zip(do, sentinel_d))
    assert _same(_bits(g), before)
    # a NaN max_mse is not looked at when max_mse_p is given; a NaN entry accepts nothing
    assert host(g.h, *hp, 1, 16, float("nan"), nanb.ctypes.data) == capi.GPC_OK
    assert np.all(ho[0] == 0) and np.all(np.isnan(ho[5])) and not np.any(np.isnan(ho[6])) and np.all(ho[1] == 65533) and np.all(ho[7] == 0)
    # P == 0
    empty = capi.Sparse(ctx, _params(capi, cap, div, ny), 0, ny)
    assert L.gpc_sparse_quantize_rd(empty.h, None, None, None, None, 1, 16, 1.0, None, *[None] * 8) == capi.GPC_OK
    assert L.gpc_sparse_quantize_rd_dev(empty.h, None, 0, None, None, None, 1, 16, 1.0, None, *[None] * 8) == capi.GPC_OK
    assert L.gpc_sparse_dequantize(empty.h, None, None, None, None, None) == capi.GPC_OK
    assert empty.quantize_rd(np.zeros(1, np.int32), np.zeros(0), np.zeros(0), np.zeros((ny, 0)))[0].shape == (0,)
    empty.close()
    # the _dev form == the host form bit for bit, with every output and with the outputs NULL one at a time
    mse0 = g.quantize_rd(off, x0, x1, y)[4]
    bound = 1.1 * mse0
    ref = g.quantize_rd(off, x0, x1, y, max_mse_p=bound, want_curve=True)
    d_b = t(bound)
    names = ("bits", "q_alpha", "q_bv", "range", "mse0", "mse_q", "curve", "status")
    for skip in (None,) + names:
        outs = dict(zip(names, fresh()))
        torch.cuda.synchronize()
        kw = {k: (None if k == skip else v) for k, v in outs.items()}
        g.quantize_rd_dev(d_off, N, d_x0, d_x1, d_y, max_mse=float("nan"), max_mse_p=d_b, **kw)
        ctx.synchronize()
        got = {k: v.cpu().numpy() for k, v in outs.items()}
        b = g.sizes()
        for k, want in zip(names[:7], ref):
            if k == skip:
                continue
            have = got[k].view(np.uint16) if k.startswith("q_") else got[k]
            if k == "q_alpha":
                assert all(np.array_equal(have[i, :, :b[i]], want[i, :, :b[i]]) and np.all(have[i, :, b[i]:] == 65533) for i in range(P)), skip
            elif k == "q_bv":
                assert all(np.array_equal(have[i, :b[i]], want[i, :b[i]]) and np.all(have[i, b[i]:] == 65533) for i in range(P)), skip
            elif k == "curve":
                ev = ~np.isnan(want)
                assert np.array_equal(have[ev], want[ev]) and np.all(have[~ev] == -1.0), skip
            else:
                assert np.array_equal(have, want), (skip, k)
        if skip != "status":
            assert np.all(got["status"] == capi.STATUS_OK)
    # decode on device buffers: the state the host form leaves
    outs = dict(zip(names, fresh()))
    g.quantize_rd_dev(d_off, N, d_x0, d_x1, d_y, max_mse_p=d_b, **outs)
    h1, h2 = (capi.Sparse(ctx, _params(capi, cap, div, ny), P, ny) for _ in range(2))
    h1.dequantize_dev(t(g.sizes()), outs["bits"], outs["q_alpha"], outs["q_bv"], outs["range"])
    ctx.synchronize()
    h2.dequantize(g.sizes(), ref[0], ref[1], ref[2], ref[3])
    assert _same(_bits(h1), _bits(h2)) and np.array_equal(h1.sizes(), g.sizes())
    assert _same(_bits(g), before)
    for o_ in (h1, h2, g):
        o_.close()
    # a dead context: destroyed while a child lives
    dead = capi.Context(0)
    child = capi.Sparse(dead, _params(capi, cap, div, ny), P, ny)
    hh, dead.h = dead.h, None
    L.gpc_ctx_destroy(hh)
    try:
        assert host(child.h, *hp, 1, 16, 1.0, None) == E and dev(child.h, *dp, 1, 16, 1.0, None) == E
        zero = np.zeros(P, np.int32)
        assert L.gpc_sparse_dequantize(child.h, *[x.ctypes.data for x in (zero, zero, ho[1], ho[2], ho[3])]) == E
    finally:
        child.close()
