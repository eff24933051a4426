"""The sparse add's phases on non-finite data, against the CPU oracle and against each other.

Every other sparse test feeds finite data.  Here NaN and infinite inputs (depth returns can be NaN), and loaded states with zero, NaN or
infinite entries (gpc_sparse_set_state loads stored models), go through every kernel shape of the add -- the rows phase, the second rows
phase, the one-wave kernel at SP_BMAX and SP_BMID, the regular kernel in its one-, two- and four-wave and LDS-resident forms -- and through
predict.  Against oracle/gpc_oracle.c (src/sparse_gp.hpp restated line by line), per patch: decision bytes, basis sizes and status words
equal; BV bit for bit; the NaN / +inf / -inf masks of alpha, C, Q, f* and sigma equal; finite entries within 2e-5 of the largest finite
|value| (the tolerance of test_sparse_batch_vs_oracle).  Across shapes (full mode): everything bit for bit, NaN = NaN.
Case data: tests/nonfinite_cases.py."""
import os

import numpy as np
import pytest

import nonfinite_cases as NF
from gp_compressor_amd import synth

pytestmark = pytest.mark.gpu

SHAPES = [None, "GPC_SPARSE_NO_ROWS", "GPC_SPARSE_NO_ROWS2", "GPC_SPARSE_NO_MID", "GPC_SPARSE_NO_SMALL"]
TOL = 2e-5


@pytest.fixture(scope="module")
def gp():
    from gp_compressor_amd import capi
    capi.load()
    ctx = capi.Context(0)
    yield capi, ctx
    ctx.close()


def _kw(ny, kw):
    """three channels: noise 1.0, and the field variant's deletion as derived (F8 fixed; with the reference's multiplication these states
    blow up to |f*| ~ 1e30 and beyond on finite data already)"""
    kw = dict(kw)
    if ny == 3:
        kw["noise"] = 1.0
        kw["ref_field_delete_bug"] = 0
    return kw


def _queries():
    """a grid plus query points with NaN and +-inf coordinates"""
    xs0, xs1 = synth.grid(NF.RES, 6)
    e0 = np.array([np.nan, np.inf, -np.inf, 0.0, 0.01, np.nan, np.inf])
    e1 = np.array([0.0, 0.0, 0.01, np.inf, -np.inf, np.inf, np.nan])
    return np.concatenate([xs0, e0]), np.concatenate([xs1, e1])


def gpu_run(capi, ctx, kw, ny, cap, off, x0, x1, y, perm, env=(), load=None, queries=None):
    """one add call (after an optional gpc_sparse_set_state) under the environment switches `env`"""
    for e in env:
        os.environ[e] = "1"
    try:
        P = len(off) - 1
        g = capi.Sparse(ctx, capi.default_params_sparse(ny, capacity=cap, **kw), P, ny)
        if load is not None:
            ld = g.ld()
            bv = np.array([s[0].shape[1] for s in load], dtype=np.int32)
            al, BV = np.zeros((P, ny, ld)), np.zeros((P, ld, 2))
            hasC = load[0][1] is not None
            Cm, Qm = (np.zeros((P, ld, ld)), np.zeros((P, ld, ld))) if hasC else (None, None)
            for i, (a, C_, Q_, B_) in enumerate(load):
                b = a.shape[1]
                al[i, :, :b], BV[i, :b] = a, B_
                if hasC:
                    Cm[i, :b, :b], Qm[i, :b, :b] = C_, Q_
            g.set_state(bv, al, BV, Cm, Qm)
        st, tr = g.add(off, x0, x1, y, perm, trace=True)
        r = dict(st=st, tr=tr, b=g.sizes(), state=g.state())
        if queries is not None:
            r["f"], r["s"], _ = g.predict(*queries)
            r["c"] = g.predict(*queries, conf=True)[1]
            os.environ["GPC_SPARSE_NO_SMALL_PREDICT"] = "1"
            try:
                r["f_reg"], r["s_reg"], _ = g.predict(*queries)
            finally:
                os.environ.pop("GPC_SPARSE_NO_SMALL_PREDICT", None)
        g.close()
        return r
    finally:
        for e in env:
            os.environ.pop(e, None)


def oracle_run(oracle, kw, ny, cap, off, x0, x1, y, perm, load=None, queries=None):
    P = len(off) - 1
    op = oracle.sparse_params(ny, p0=kw["sigmaf_sq"], p1=kw["l_sq"], s20=kw["noise"], capacity=cap,
                              field_delete_bug=kw.get("ref_field_delete_bug", 1))
    if "eps_tol" in kw:
        op.eps_tol = kw["eps_tol"]
    r = dict(st=np.zeros(P, np.int32), tr=np.zeros(int(off[-1]), np.uint8), b=np.zeros(P, np.int32), state=[], f=[], s=[], c=[])
    for i in range(P):
        sl = slice(off[i], off[i + 1])
        h = oracle.Sparse(op, cap + 2)
        if load is not None:
            h.set_state(*load[i])
        if off[i + 1] > off[i]:
            r["tr"][sl] = h.add_measurements(x0[sl], x1[sl], y[:, sl], None if perm is None else perm[sl], trace=True)
        r["st"][i], r["b"][i] = h.status(), h.size()
        r["state"].append(h.state())
        if queries is not None:
            f, s = h.predict(*queries)
            r["f"].append(f)
            r["s"].append(s)
            r["c"].append(h.predict(*queries, conf=True)[1])
    return r


def close(got, want, what):
    """the NaN / +inf / -inf masks equal, finite entries within TOL of the largest finite |want|"""
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape, what
    for name, m in (("NaN", np.isnan), ("+inf", lambda a: a == np.inf), ("-inf", lambda a: a == -np.inf)):
        assert np.array_equal(m(got), m(want)), f"{what}: {name} masks differ: GPU {np.argwhere(m(got))[:6].tolist()} " \
                                                f"oracle {np.argwhere(m(want))[:6].tolist()}"
    fin = np.isfinite(want)
    if fin.any():
        scale = max(float(np.max(np.abs(want[fin]))), 1e-300)
        err = float(np.max(np.abs(got[fin] - want[fin])))
        assert err <= TOL * scale, f"{what}: max |d| {err:.3e} > {TOL} x {scale:.3e}"


def vs_oracle(g, o, patches, predict=False):
    assert np.array_equal(g["b"], o["b"]), (g["b"], o["b"])
    assert np.array_equal(g["st"], o["st"]), (g["st"], o["st"])
    assert np.array_equal(g["tr"], o["tr"]), np.argwhere(g["tr"] != o["tr"])[:8].ravel().tolist()
    for i in patches:
        b = int(o["b"][i])
        ao, Co, Qo, BVo = o["state"][i]
        ag, Cg, Qg, BVg = (s[i] for s in g["state"])
        assert np.array_equal(BVg[:b], BVo, equal_nan=True), f"patch {i}: BV"
        close(ag[:, :b], ao, f"patch {i}: alpha")
        close(Cg[:b, :b], Co, f"patch {i}: C")
        close(Qg[:b, :b], Qo, f"patch {i}: Q")
        if predict:
            close(g["f"][i], o["f"][i], f"patch {i}: f*")
            close(g["s"][i], o["s"][i], f"patch {i}: sigma")
            close(g["c"][i], o["c"][i], f"patch {i}: confidence")   # (100 x the relative error of sigma^2: within 2e-5 of 100)


def _state(r, i):
    """patch i's state up to its basis size (what lies beyond is whatever the buffers held)"""
    b = int(r["b"][i])
    a, C_, Q_, BV = (s[i] for s in r["state"])
    return a[:, :b], C_[:b, :b], Q_[:b, :b], BV[:b]


def same_bits(a, b, what):
    for k in ("st", "tr", "b"):
        assert np.array_equal(a[k], b[k]), f"{what}: {k}"
    for i in range(len(a["b"])):
        for u, v, n in zip(_state(a, i), _state(b, i), ("alpha", "C", "Q", "BV")):
            assert np.array_equal(u, v, equal_nan=True), f"{what}: patch {i}: {n}"


# ---------------------------------------------------------------------------------------------------------------- B1: non-finite inputs

POISONED = {1: "y_nan", 5: "y_inf", 9: "x0_nan", 13: "x1_inf_first", 17: "one_point_nan", 21: "x1_inf_first", 26: "y_nan"}


def _batch_b1(ny, seed):
    P, n = 40, 150
    off, x0, x1, y = synth.make_patches(P, n, res=NF.RES, seed=seed, ragged=True, ny=ny)
    off, x0, x1, y, _ = NF.one_point_nan(off, x0, x1, y, 17)
    x0[off[17]], x1[off[17]] = 0.01, -0.02                  # the clean twin of the NaN point
    perm = synth.sattolo_perms(off, seed=seed + 1)
    clean = (x0.copy(), x1.copy(), y.copy())
    for j, kind in POISONED.items():
        o, m = int(off[j]), int(off[j + 1] - off[j])
        if kind == "one_point_nan":
            x0[o] = x1[o] = np.nan
        else:
            NF.poison(kind, x0, x1, y, o, m, perm[o:o + m])
    return off, x0, x1, y, perm, clean


@pytest.mark.parametrize("cap", [12, 24, 40, 80, 150])
@pytest.mark.parametrize("ny", [1, 3])
def test_sparse_nonfinite_inputs(gp, oracle, ny, cap, monkeypatch):
    """A ragged batch in which some patches see a NaN or +inf value or coordinate (a middle point, or the first point) or consist of one
    NaN point: the oracle's states, masks and decisions per patch (triangular and LDS-resident modes), every kernel shape bit for bit, and
    the clean patches exactly as in the same batch without the poison (a NaN must not cross a patch boundary of the rows phase's waves)."""
    capi, ctx = gp
    kw = _kw(ny, NF.KW1 if cap <= 48 else NF.KW_BIG)
    off, x0, x1, y, perm, clean = _batch_b1(ny, 70 + cap)
    P = len(off) - 1
    q = _queries()
    o = oracle_run(oracle, kw, ny, cap, off, x0, x1, y, perm, queries=q)
    assert all(o["st"][j] == 2 for j, k in POISONED.items() if k in ("x0_nan", "x1_inf_first", "one_point_nan"))
    for env in ((), ("GPC_SPARSE_RES",)):
        g = gpu_run(capi, ctx, kw, ny, cap, off, x0, x1, y, perm, env=env, queries=q)
        vs_oracle(g, o, range(P), predict=True)
    monkeypatch.setenv("GPC_SPARSE_FULL", "1")
    runs = [gpu_run(capi, ctx, kw, ny, cap, off, x0, x1, y, perm, env=(e,) if e else ()) for e in SHAPES]
    for e, r in zip(SHAPES[1:], runs[1:]):
        same_bits(runs[0], r, e)
    vs_oracle(runs[0], o, range(P))
    ref = gpu_run(capi, ctx, kw, ny, cap, off, *clean, perm)
    for i in set(range(P)) - set(POISONED):
        sl = slice(off[i], off[i + 1])
        assert runs[0]["st"][i] == ref["st"][i] and runs[0]["b"][i] == ref["b"][i] and np.array_equal(runs[0]["tr"][sl], ref["tr"][sl])
        for u, v in zip(_state(runs[0], i), _state(ref, i)):
            assert np.array_equal(u, v), f"clean patch {i} changed by its neighbours' poison"


# ---------------------------------------------------------------------------------------------------------------- B2: loaded states

B2 = [(c, cap, cap) for c in "abc" for cap in (16, 24, 48, 64, 100, 150)] + [("d", 10, 40), ("d", 20, 40)]


@pytest.mark.parametrize("ny", [1, 3])
@pytest.mark.parametrize("case,b,cap", B2)
def test_sparse_nonfinite_loaded_state(gp, oracle, case, b, cap, ny, monkeypatch):
    """gpc_sparse_set_state of states with zero C and Q (the decompressor's load), a zero or NaN alpha, an infinite entry of Q, then one add
    call of 20 points: the capacity deletion follows the reference's scan (a NaN score at index 0 deletes vector 0, elsewhere it is
    skipped), and every shape agrees."""
    capi, ctx = gp
    kw = _kw(ny, NF.KW_LOAD)
    P, n = 4, 20
    load = [NF.loaded_case(case, b, ny, seed=11 * i + b) for i in range(P)]
    pts = [NF.new_points(n, ny, seed=7 * i + b) for i in range(P)]
    off = (np.arange(P + 1) * n).astype(np.int32)
    x0 = np.concatenate([p[0] for p in pts])
    x1 = np.concatenate([p[1] for p in pts])
    y = np.ascontiguousarray(np.concatenate([p[2] for p in pts], axis=1))
    q = _queries()
    o = oracle_run(oracle, kw, ny, cap, off, x0, x1, y, None, load=load, queries=q)
    if case in "abc":
        assert np.all(o["tr"][::n] & 0x0f == 0x03)      # the first point: a full update and one capacity deletion
    for env in ((), ("GPC_SPARSE_RES",)):
        g = gpu_run(capi, ctx, kw, ny, cap, off, x0, x1, y, None, env=env, load=load, queries=q)
        vs_oracle(g, o, range(P), predict=True)
    monkeypatch.setenv("GPC_SPARSE_FULL", "1")
    runs = [gpu_run(capi, ctx, kw, ny, cap, off, x0, x1, y, None, env=(e,) if e else (), load=load) for e in SHAPES]
    for e, r in zip(SHAPES[1:], runs[1:]):
        same_bits(runs[0], r, e)
    vs_oracle(runs[0], o, range(P))


# ---------------------------------------------------------------------------------------------------------------- B3: predict

@pytest.mark.parametrize("cap", [16, 80])
@pytest.mark.parametrize("ny", [1, 3])
def test_sparse_predict_nonfinite_queries(gp, oracle, ny, cap):
    """f* and sigma (plain and as a confidence) at NaN and +-inf query points, for an empty patch and for trained ones: k = 0 at an infinite
    point but k* = NaN, so sigma is NaN (src/sparse_gp.hpp:316-330); the small-basis predict kernels give the regular kernel's mean bit for
    bit and its masks."""
    capi, ctx = gp
    kw = _kw(ny, NF.KW1 if cap <= 48 else NF.KW_BIG)
    off, x0, x1, y = synth.make_patches(6, 100, res=NF.RES, seed=90 + cap, ragged=True, ny=ny)
    counts = np.diff(off)
    counts[2] = 0                                           # an empty patch
    keep = np.concatenate([np.arange(off[i], off[i] + counts[i]) for i in range(6)]).astype(np.int64)
    off = np.concatenate([[0], np.cumsum(counts)]).astype(np.int32)
    x0, x1, y = x0[keep], x1[keep], np.ascontiguousarray(y[:, keep])
    q = _queries()
    o = oracle_run(oracle, kw, ny, cap, off, x0, x1, y, None, queries=q)
    g = gpu_run(capi, ctx, kw, ny, cap, off, x0, x1, y, None, queries=q)
    vs_oracle(g, o, range(6), predict=True)
    assert np.all(np.isnan(np.asarray(o["s"])[:, -7:]))     # every non-finite query: sigma NaN, trained or empty
    assert np.array_equal(g["f"], g["f_reg"], equal_nan=True)
    close(g["s"], g["s_reg"], "sigma: small-basis vs regular predict kernel")
