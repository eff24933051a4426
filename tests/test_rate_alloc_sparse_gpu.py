"""Sparse.prune_to_bytes on the GPU: the curves of an identity copy, the allocation, the applying prune.  Small batches of prune_ref.batch
(capacity 20, 64 points, 6 leaves, depth and colour) whose leaves carry different noise levels, so that their rate-distortion slopes
differ and the allocation is not uniform."""
import numpy as np
import pytest

import prune_rd_ref as rd
import prune_ref as pr
import rate_alloc_ref as RA

pytestmark = pytest.mark.gpu
GATE_MSE = pr.GATE_FACTOR * rd.E64_MSE
CAP, DIV, N, P = 20, 3.0, 64, 6


@pytest.fixture(scope="module")
def gp():
    from gp_compressor_amd import capi
    capi.load()
    ctx = capi.Context(0)
    yield capi, ctx
    ctx.close()


_made = {}


def _trained(capi, ctx, ny):
    """the batch with per-leaf noise, and a trained object (made once per ny; callers work on copies)"""
    if ny not in _made:
        off, x0, x1, y, perm = pr.batch(CAP, N, P, ny)
        rng = np.random.default_rng(40 + ny)
        y = np.array(y, dtype=np.float64).reshape(ny, -1).copy()
        for i in range(P):
            s = slice(off[i], off[i + 1])
            y[:, s] += rng.standard_normal((ny, off[i + 1] - off[i])) * (0.002 * 3.0 ** i if ny == 1 else 0.5 * 2.0 ** i)
        # (the colour field deleting as its derivation says, as in tests/test_prune_rd_host_gpu.py)
        g = capi.Sparse(ctx, capi.default_params_sparse(ny, ref_field_delete_bug=0, **pr.kernel_kw(CAP, DIV, ny)), P, ny)
        assert np.all(g.add(off, x0, x1, y, perm) == 0)
        _made[ny] = (off, x0, x1, y, g)
    return _made[ny]


def _copy(g):
    return g.remap(g.P, np.arange(g.P, dtype=np.int32))


def _bits(g):
    return (g.sizes(),) + tuple(g.state())


def _same(a, b):
    return all(np.array_equal(x, y, equal_nan=True) for x, y in zip(a, b))


def _mse_from_readout(g, off, x0, x1, y):
    """per-patch error of the object as it stands, from Sparse.predict_points, summed in the rule's order (tests/test_prune_rd_gpu.py)"""
    f, _, _ = g.predict_points(off, x0, x1)
    out = np.full(g.P, np.nan)
    for i in range(g.P):
        s = slice(off[i], off[i + 1])
        r = y[:, s] - f[:, s]
        e = np.zeros(off[i + 1] - off[i])
        for c in range(g.ny):
            e = e + r[c] * r[c]
        out[i] = rd.class_sum(e) / (len(e) * g.ny)
    return out


@pytest.mark.parametrize("ny", [1, 3])
def test_prune_to_bytes(gp, ny):
    capi, ctx = gp
    off, x0, x1, y, g0 = _trained(capi, ctx, ny)
    unit = 24 if ny == 1 else 40
    b = g0.sizes()
    # the curves, as the call itself takes them
    cv = _copy(g0)
    kmax, mse0, _, _, _, mse = cv.prune_rd(off, x0, x1, y, keep=1, want_trace=True)
    cv.close()
    assert np.array_equal(kmax, b - 1) and np.all(b > 4)
    n_p = np.diff(off).astype(np.float64)
    pb = RA.Problem(kmax, mse0, mse, w=n_p * float(ny), unit_all=unit)
    full = unit * int(kmax.sum())
    for need in (full // 3, full // 2 + 1):
        want = RA.allocate(pb, need, True)
        g = _copy(g0)
        k, res = g.prune_to_bytes(off, x0, x1, y, need)
        print(f"ny {ny}: need {need} of {full}: k {k} of {kmax}, saved {res['saved']}, lambda {res['lambda']:.3e}, switched {res['switched_rows']}")
        assert np.array_equal(k, want["k"]) and all(res[f] == want[f] for f in ("lambda_bits", "saved", "feasible", "switched_rows"))
        assert res["feasible"] == 1 and res["saved"] >= need and res["saved"] == unit * int(k.sum())
        assert len(set(k.tolist())) > 1, "the allocation is uniform: the leaves' slopes do not differ"
        assert np.array_equal(g.sizes(), b - k)
        # bit for bit the state of prune(target = b - k, score_tol = 0) on a second copy
        h = _copy(g0)
        rm = h.prune(target=(b - k).astype(np.int32), score_tol=0.0)
        assert np.array_equal(rm, k) and _same(_bits(g), _bits(h))
        h.close()
        # the read-out error of every leaf is its curve entry e(k)
        e_k = np.array([mse0[i] if k[i] == 0 else mse[i, k[i] - 1] for i in range(P)])
        assert np.allclose(_mse_from_readout(g, off, x0, x1, y), e_k, rtol=GATE_MSE, atol=0)
        g.close()
    # the original was never touched
    assert np.array_equal(g0.sizes(), b)


@pytest.mark.parametrize("ny", [1, 3])
def test_infeasible_need_and_weights(gp, ny):
    capi, ctx = gp
    off, x0, x1, y, g0 = _trained(capi, ctx, ny)
    unit = 24 if ny == 1 else 40
    b = g0.sizes()
    cv = _copy(g0)
    kmax, mse0, _, _, _, mse = cv.prune_rd(off, x0, x1, y, keep=1, want_trace=True)
    cv.close()
    n_p = np.diff(off).astype(np.float64)
    full = unit * int(kmax.sum())
    pb = RA.Problem(kmax, mse0, mse, w=n_p * float(ny), unit_all=unit)
    g = _copy(g0)
    k, res = g.prune_to_bytes(off, x0, x1, y, full + 1)
    want = RA.allocate(pb, full + 1, True)
    assert res["feasible"] == 0 and res["lambda"] == float("inf") and res["max_saving"] == full and res["saved"] == full
    assert np.array_equal(k, want["k"]) and np.array_equal(k, RA.choice(pb, float("inf"))) and np.array_equal(g.sizes(), b - k)
    g.close()
    # a weight per leaf moves the removals away from the heavy leaves; a leaf of weight NaN is fixed
    wt = np.array([100.0, 1.0, 1.0, 1.0, 1.0, float("nan")])
    pw = RA.Problem(kmax, mse0, mse, w=wt * n_p * float(ny), unit_all=unit)
    g = _copy(g0)
    k, res = g.prune_to_bytes(off, x0, x1, y, full // 3, weight=wt, refine=False)
    want = RA.allocate(pw, full // 3, False)
    assert np.array_equal(k, want["k"]) and res["lambda_bits"] == want["lambda_bits"] and k[5] == 0 and res["saved"] >= full // 3
    g.close()
