"""What test_irls_var_gpu.py assumes, checked without a GPU: the NumPy restatement of the probit GP's latent variance and occupancy
probability (irls_var_cases.py) holds on its own -- against a longdouble variance step, against the oracle's Newton loop, in range and
convergent on every batch the GPU tests use --, the route rule sends the IRLS entry with the variance to the exporting instances, and the
two new entries are declared and exported."""
import os
import re

import numpy as np

import irls_cases as IC
import irls_var_cases as IV
import variance_cases as VC


def test_restatement_variance_against_longdouble(oracle):
    """The float64 v* against the longdouble variance step (same s, the float64 loop's) on the w4_batch patches up to 128 points.
    E64 = the worst |v64 - v_ld| of sigma_f^2: measured 7e-16; the v* gate of the GPU tests follows from it by the rule in
    irls_var_cases.py, and the constants there must be what this test finds."""
    batch = IC.w4_batch()
    off, x0, x1, _ = batch
    xs = IV.xs400("w4")
    ref = IV.w4_ref(oracle)
    e64 = 0.0
    for i, (L, s) in ref["last"].items():
        n = int(off[i + 1] - off[i])
        if n > 128:
            continue
        sl = slice(off[i], off[i + 1])
        vld = IV.variance_step_hp(x0[sl], x1[sl], s, xs[0], xs[1])
        e64 = max(e64, float(np.max(np.abs(ref["v"][i].astype(np.longdouble) - vld))) / IV.SF)
    print("E64 = %.2e of sigma_f^2; gate in force %.2e" % (e64, IV.V_GATE))
    assert e64 <= 2.0 * IV.E64_MEASURED, e64
    assert IV.E64_MEASURED <= IV.VTOL * IV.SF / 16 and IV.V_GATE == IV.VTOL * IV.SF


def _in_range(ref, off, model):
    n = np.diff(off)
    for i in np.flatnonzero(ref["status"] >= 0):
        if ref["status"][i] == 2:
            assert np.all(np.isnan(ref["f"][i])) and np.all(np.isnan(ref["v"][i])), i
            continue
        assert ref["status"][i] == 0 and 0 <= ref["iters"][i] <= IC.MAX_ITER, (i, int(n[i]), ref["status"][i])
        assert np.all(ref["v"][i] >= IV.V_LO) and np.all(ref["v"][i] <= IV.V_HI), (i, ref["v"][i].min(), ref["v"][i].max())
        if model == 2:
            assert np.all(ref["p"][i] >= 0.0) and np.all(ref["p"][i] <= 1.0), i


def _against_oracle(oracle, ref, batch, model, xs, idx=None):
    if idx is not None:
        sub, pts = IC.take(batch, idx)
    else:
        sub, pts, idx = batch, slice(None), list(range(len(batch[0]) - 1))
    fo, alo, fho, ito, sto = IC.oracle_fit(oracle, sub, model, xs)
    off = sub[0]
    f, al, fh = ref["f"][idx], ref["alpha"][pts], ref["fhat"][pts]
    assert np.array_equal(ref["status"][idx], sto) and np.all(np.abs(ref["iters"][idx] - ito) <= 1)
    gap = lambda a, b: float(np.max(np.abs(a - b))) / max(float(np.max(np.abs(b))), 1e-300) if b.size else 0.0
    worst = 0.0
    for i in range(len(off) - 1):
        sl = slice(off[i], off[i + 1])
        if sto[i] != 0 or off[i + 1] == off[i]:
            continue
        g = max(gap(f[i], fo[i]), gap(al[sl], alo[sl]), gap(fh[sl], fho[sl]))
        worst = max(worst, g)
        assert g <= IC.FTOL[model], (i, g)
    return worst


def test_restatement_against_oracle_and_in_range(oracle):
    """On the tile-edge batches (both shapes; model 1 on the sizes up to MODEL1_CAP) and the grid batches: every patch converges within
    MAX_ITER, -1e-12 sf <= v* <= sf (1 + 1e-12), 0 <= p* <= 1, and f*, a, fhat agree with the oracle's loop within FTOL[model]."""
    w = []
    b = IC.w4_batch()
    for model in (2, 1):
        ref = IV.w4_ref(oracle, model)
        _in_range(ref, b[0], model)
        w.append(_against_oracle(oracle, ref, b, model, IV.xs400("w4")))
    b = IC.tile_batch()
    _in_range(IV.tile_ref(oracle, 2), b[0], 2)
    w.append(_against_oracle(oracle, IV.tile_ref(oracle, 2), b, 2, IV.xs400("tiles")))
    _in_range(IV.tile_ref(oracle, 1), b[0], 1)
    w.append(_against_oracle(oracle, IV.tile_ref(oracle, 1), b, 1, IV.xs400("tiles"), idx=IC.cap_index(IC.MODEL1_CAP)))
    for shape in ("big", "w4"):
        ref = IV.grid_ref(oracle, shape, 400)
        _in_range(ref, IC.grid_batch(shape)[0], 2)
        w.append(_against_oracle(oracle, ref, IC.grid_batch(shape), 2, VC.xstar(400, seed=73)))
    print("restatement against the oracle, worst of f*, a, fhat per batch: " + ", ".join("%.1e" % x for x in w))


def test_restatement_on_the_many_patch_batches(oracle):
    """many_batch("big") and ("w4"), every patch: the three NaN-label patches end with status 2, every other one converges, in range."""
    for which in ("big", "w4"):
        c = IC.MANY[which]
        ref = IV.many_ref(oracle, which, every=True)
        assert ref["status"][list(c["nan"])].tolist() == [2, 2, 2]
        assert np.all(np.delete(ref["status"], list(c["nan"])) == 0)
        _in_range(ref, IC.many_batch(which)[0], 2)
        assert set(c["empty"]) | set(c["nan"]) <= set(IV.many_pick(which)) and len(IV.many_pick(which)) == 64


def test_pinned_step_counts_do_not_converge(oracle):
    """tol = 0 with max_iter 1, 2, 6 on the pinned batches (the grid batches without their single-point patch, see
    irls_var_cases.pinned_batch): every non-empty patch ends NOT_CONVERGED after exactly that many solves, with finite outputs in range
    (what the GPU test compares with)."""
    for shape in ("big", "w4"):
        n = np.diff(IV.pinned_batch(shape)[0])
        assert np.all(n != 1) and np.sum(n == 0) == 1 and len(n) >= 4
        for k in (1, 2, 6):
            ref = IV.pinned_ref(oracle, shape, k)
            assert np.all(ref["status"][n > 0] == 5) and np.all(ref["iters"][n > 0] == k), (shape, k, ref["status"], ref["iters"])
            assert np.all(np.isfinite(ref["f"])) and np.all(np.isfinite(ref["p"]))
            assert np.all(ref["v"] >= IV.V_LO) and np.all(ref["v"] <= IV.V_HI)


def test_route_of_the_irls_entry_with_the_variance():
    """dense_route with irls and variance: the tiled IRLS instances with the export on, named with the variance kernel behind them, at
    256 and at 257 points; the plain IRLS rows of test_dense_route_cpu.py answer as before."""
    from gp_compressor_amd import capi
    kind, name, shape = capi.dense_route(P=40, n_max=256, irls=True, variance=True, pointwise=True)
    assert (kind, name) == ("tiled", "dense_mfma_big_w4_irls + dense_variance_big"), (kind, name)
    assert shape["waves"] == 4 and shape["npad"] == 256 and shape["export_factor"] == 1
    kind, name, shape = capi.dense_route(P=40, n_max=257, irls=True, variance=True, pointwise=True)
    assert (kind, name) == ("tiled", "dense_mfma_big_irls + dense_variance_big"), (kind, name)
    assert shape["waves"] == 8 and shape["npad"] == 1024 and shape["export_factor"] == 1
    rows = [(dict(P=40, n_max=256, irls=True), "dense_mfma_big_w4_irls", dict(waves=4, npad=256)),
            (dict(P=4096, n_max=17, irls=True, m=0), "dense_mfma_big_w4_irls", dict(waves=4, npad=256)),
            (dict(P=40, n_max=257, irls=True), "dense_mfma_big_irls", dict(waves=8, npad=1024)),
            (dict(P=40, n_max=1024, irls=True), "dense_mfma_big_irls", dict(waves=8, npad=1024, per_cu=1))]
    for facts, want, want_shape in rows:
        kind, name, shape = capi.dense_route(**facts)
        assert (kind, name) == ("tiled", want) and shape["export_factor"] == 0, (facts, kind, name)
        assert all(shape[k] == v for k, v in want_shape.items()), (facts, shape)
    assert capi.dense_route(P=0, n_max=256, irls=True, variance=True, pointwise=True)[:2] == ("nothing", "")


def test_new_symbols_declared_and_exported():
    """gpc_dense_irls_fit_predict_var and _var_dev: declared in include/gpc.h, exported by libgpc_hip.so, bound by capi."""
    import ctypes
    from gp_compressor_amd import capi
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    with open(os.path.join(root, "include", "gpc.h")) as fh:
        hdr = fh.read()
    lib = ctypes.CDLL(capi.LIB_PATH)
    for sym in ("gpc_dense_irls_fit_predict_var", "gpc_dense_irls_fit_predict_var_dev"):
        assert re.search(r"\bint\s+%s\s*\(" % sym, hdr), sym
        assert hasattr(lib, sym), sym
        assert sym in capi.PROTOTYPES
