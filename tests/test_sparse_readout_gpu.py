"""The kernels that read a sparse GP state out again -- sparse_predict_kernel, sparse_predict_small_kernel, sparse_likelihood_kernel (with
its raw pass) and sparse_train_kernel -- per point, at every basis size where they change path, against the extended-precision closed
form of tests/readout_cases.py within the forward-error bounds derived there (tests/test_readout_cpu.py shows, without a GPU, that the
reference is exact to a small fraction of those bounds and that every single term of every sum is worth at least 1000 of them).

Four objects (readout_cases.BASES): capacity 15 (ld 16), 100 (ld 112), 239 (ld 240: the last leading dimension whose likelihood kernel
has the LDS for V = C K on the MFMA pipe, sp_ck_chunk) and -1 (ld 256: the scalar C k loop of the likelihood kernel and of the raw pass),
one patch per basis size, states loaded with set_state.  Patch 0 of every object is EMPTY AND HAS POINTS: an empty basis inside
sp_ck_chunk, which used to send its prefetch in front of the allocation.  Every test prints its worst error / bound.
"""
import numpy as np
import pytest

import readout_cases as RC

pytestmark = pytest.mark.gpu
LD = RC.LD
KK = RC.SF + RC.S20
RES2 = RC.RES / 2


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
    assert np.array_equal(g.sizes(), B["b"])
    return g


@pytest.fixture(scope="module")
def loaded(gp):
    """case -> (Sparse with the case's state, its batch); every object is loaded once and only read afterwards"""
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


def _predict_ratios(r, f, sigma, conf):
    """worst error / bound of one patch: mean (ny, m), sigma (m,) compared as sigma^2, confidence form (m,); an empty basis exactly"""
    out = {}
    fe = np.abs(f.astype(LD) - r["f"])
    if len(r["K"]) == 0:
        assert np.all(f == 0.0) and np.all(sigma == np.sqrt(KK)) and np.all(conf == 0.0)
        return dict(f=0.0, s2=0.0, conf=0.0)
    with np.errstate(invalid="ignore", divide="ignore"):
        out["f"] = float(np.max(np.where(r["fb"] > 0, np.asarray(fe, dtype=np.float64) / r["fb"], np.where(fe == 0, 0.0, np.inf))))
    out["s2"] = float(np.max(np.asarray(np.abs((sigma * sigma).astype(LD) - r["s2"]), dtype=np.float64) / RC.sigma2_tolerance(r)))
    out["conf"] = float(np.max(np.asarray(np.abs(conf.astype(LD) - r["conf"]), dtype=np.float64) / r["confb"]))
    return out


def _worst(acc, new):
    for k, v in new.items():
        acc[k] = max(acc.get(k, 0.0), v)


@pytest.mark.parametrize("case", RC.CASES, ids=RC.CASE_IDS)
def test_readout_predict_points(gp, loaded, case, monkeypatch):
    """predict_points on the ragged queries (every patch: its own basis vectors and 37 more, m = b + 37): mean, sigma^2 and the
    confidence form within the derived bounds, as dispatched (b <= 16 and 17 .. 32 to the one-wave kernels) and with every patch on
    sparse_predict_kernel (GPC_SPARSE_NO_SMALL_PREDICT: b <= 32 is then the partial first tile of sp_ck_chunk, b = 0 its empty case).
    Status words 0, the mean the same bits in both runs and without sigma, empty patches f = 0 and sigma = sqrt(sf + s20)."""
    g, B = loaded(case)
    ref = RC.ragged_reference(*case)
    off, q0, q1 = B["off"], B["q0"], B["q1"]
    means = []
    for mode in ("dispatched", "regular"):
        if mode == "regular":
            monkeypatch.setenv("GPC_SPARSE_NO_SMALL_PREDICT", "1")
        f, s, st = g.predict_points(off, q0, q1, want_sigma=True)
        fc, c, stc = g.predict_points(off, q0, q1, want_sigma=True, conf=True)
        fm, none, stm = g.predict_points(off, q0, q1, want_sigma=False)
        assert none is None and not st.any() and not stc.any() and not stm.any(), (st, stc, stm)
        assert f.tobytes() == fc.tobytes() == fm.tobytes()
        means.append(f)
        worst = {}
        for i in range(B["P"]):
            sl = slice(off[i], off[i + 1])
            if ref[i] is not None:
                _worst(worst, _predict_ratios(ref[i], f[:, sl], s[sl], c[sl]))
        print(f"predict_points {RC.CASE_IDS[RC.CASES.index(case)]} [{mode}]: worst error / bound mean {worst['f']:.3f}, sigma^2 {worst['s2']:.3f}, "
              f"confidence {worst['conf']:.3f}")
        assert max(worst.values()) <= 1.0, worst
    assert means[0].tobytes() == means[1].tobytes()


@pytest.mark.parametrize("m", [1, 31, 32, 33, 65])
def test_readout_predict_grid(gp, loaded, m):
    """predict on a shared grid of m points (one point, one short of a chunk of 32, a chunk, one more, two chunks and one), the
    capacity-100 objects: sigma^2 and the mean of every patch against the reference"""
    rng = np.random.default_rng(500 + m)
    xs0, xs1 = rng.uniform(-RES2, RES2, m), rng.uniform(-RES2, RES2, m)
    for case in [c for c in RC.CASES if c[0] == 100]:
        g, B = loaded(case)
        f, s, st = g.predict(xs0, xs1)
        fcf, c, stc = g.predict(xs0, xs1, conf=True)
        assert f.shape == (B["P"], B["ny"], m) and s.shape == (B["P"], m) and not st.any() and not stc.any()
        assert f.tobytes() == fcf.tobytes()
        worst = {}
        for i in range(B["P"]):
            _worst(worst, _predict_ratios(RC.evaluate(B, i, xs0, xs1), f[i], s[i], c[i]))
        print(f"predict, grid of {m}, capacity 100 ny {B['ny']}: worst error / bound mean {worst['f']:.3f}, sigma^2 {worst['s2']:.3f}, "
              f"confidence {worst['conf']:.3f}")
        assert max(worst.values()) <= 1.0, worst


@pytest.mark.parametrize("case", RC.CASES, ids=RC.CASE_IDS)
def test_readout_likelihood(gp, loaded, case):
    """likelihood on the same ragged queries with yq = smooth y + N(0, 0.05): l and dX of every point within 1e-8 of the patch's
    largest reference value; one output alone gives the same bytes; an empty patch gives dX[:, 1:] = 0 and the prior's likelihood."""
    g, B = loaded(case)
    ny = B["ny"]
    ref = RC.ragged_reference(*case)
    off, q0, q1, yq = B["off"], B["q0"], B["q1"], B["yq"]
    dX, l = g.likelihood(off, q0, q1, yq)
    assert np.all(np.isfinite(dX)) and np.all(np.isfinite(l))
    worst = dict(l=0.0, dX=0.0)
    for i in range(B["P"]):
        sl = slice(off[i], off[i + 1])
        r = ref[i]
        if r is None:
            continue
        el = float(np.max(np.abs(l[sl].astype(LD) - r["l"])) / (1e-8 * np.max(np.abs(r["l"]))))
        top = float(np.max(np.abs(r["dX"])))
        ed = float(np.max(np.abs(dX[sl].astype(LD) - r["dX"]))) / (1e-8 * top) if top > 0 else (0.0 if not dX[sl].any() else np.inf)
        worst = dict(l=max(worst["l"], el), dX=max(worst["dX"], ed))
        if B["b"][i] == 0:
            sq = np.sum(yq[:, sl] * yq[:, sl], axis=0)
            l0 = np.exp(-0.5 * sq / KK) / np.sqrt((2 * np.pi) ** ny * KK)                  # the reference's form at mu = 0, sigma = sf + s20
            assert np.all(dX[sl, 1:] == 0.0) and np.max(np.abs(l[sl] - l0)) <= 1e-8 * np.max(l0), i
    print(f"likelihood {RC.CASE_IDS[RC.CASES.index(case)]}: worst error / (1e-8 of the patch's largest value) l {worst['l']:.2e}, dX {worst['dX']:.2e}")
    assert max(worst.values()) <= 1.0, worst
    d2, none = g.likelihood(off, q0, q1, yq, want_l=False)
    none2, l2 = g.likelihood(off, q0, q1, yq, want_dx=False)
    assert none is None and none2 is None and d2.tobytes() == dX.tobytes() and l2.tobytes() == l.tobytes()


@pytest.mark.parametrize("case", [c for c in RC.CASES if c[1] == 1], ids=[i for c, i in zip(RC.CASES, RC.CASE_IDS) if c[1] == 1])
def test_readout_train_sigmaf(gp, loaded, case):
    """train_sigmaf (step = float32(1e-4), max_counter = 3: five iterations) on the ragged queries of the ny = 1 objects, against
    train_sigmaf_np on the same state: 1e-9 on the parameter, 1e-8 on the last gradient, 1e-7 on the likelihood trace, iteration counts
    equal; fewer than 20 vectors: no iteration, the parameter untouched.  At ld = 256 its raw pass is the scalar C k loop."""
    g, B = loaded(case)
    cap, _, l_sq = case
    ref = RC.train_reference(cap, l_sq)
    p0, iters, ls, delta = g.train_sigmaf(B["off"], B["q0"], B["q1"], B["yq"][0], step=RC.TRAIN_STEP, max_counter=RC.TRAIN_MAXC)
    worst, trained = 0.0, 0
    for i in range(B["P"]):
        assert iters[i] == ref[i][1], (i, iters[i], ref[i][1])
        if B["b"][i] < 20:
            assert iters[i] == 0 and p0[i] == RC.SF and not ls[i].any()
            continue
        trained += 1
        assert iters[i] == RC.TRAIN_MAXC + 2 and np.all(np.isfinite(ls[i])) and np.all(np.isfinite(delta[i]))
        worst = max(worst, RC.train_errors((p0[i], ls[i], delta[i]), ref[i]))
    print(f"train_sigmaf capacity {cap}: {trained} trained patches, worst error / bound {worst:.2e}")
    assert trained == sum(b >= 20 for b in RC.BASES[cap]) and worst <= 1.0, worst


def test_readout_sigma_clamp(gp):
    """One clamp decision far from its boundary: 65 vectors with C = -(2 / sf) I.  At the queries that are basis vectors
    s20 + sf + k^T C k <= s20 - sf < 0: sigma = 0, the confidence form exactly 100, the patch's status GPC_STATUS_SIGMA_CLAMPED; the
    patches beside it keep status 0 and their bounds; so do the patch's other queries, wherever the reference is a bound away from 0."""
    capi, ctx = gp
    B = RC.clamp_batch()
    g = _load(capi, ctx, B)
    off, q0, q1 = B["off"], B["q0"], B["q1"]
    f, s, st = g.predict_points(off, q0, q1, want_sigma=True)
    _, c, stc = g.predict_points(off, q0, q1, want_sigma=True, conf=True)
    g.close()
    assert st.tolist() == stc.tolist() == [0, capi.STATUS_SIGMA_CLAMPED, 0]
    worst = {}
    for i in range(B["P"]):
        sl = slice(off[i], off[i + 1])
        r = RC.evaluate(B, i, q0[sl], q1[sl])
        if i != 1:
            _worst(worst, _predict_ratios(r, f[:, sl], s[sl], c[sl]))
            continue
        s2 = np.asarray(r["s2"], dtype=np.float64)
        tol = RC.sigma2_tolerance(r)
        assert np.all(s2[:RC.CLAMP_B] <= RC.S20 - RC.SF)
        assert np.all(s[sl][:RC.CLAMP_B] == 0.0) and np.all(c[sl][:RC.CLAMP_B] == 100.0)
        neg, pos = s2 < -tol, s2 > tol
        assert np.all(s[sl][neg] == 0.0) and np.all(c[sl][neg] == 100.0)
        _worst(worst, dict(f=float(np.max(np.asarray(np.abs(f[:, sl].astype(LD) - r["f"]), dtype=np.float64) / r["fb"]))))
        if pos.any():
            _worst(worst, dict(s2=float(np.max((np.abs((s[sl] * s[sl]).astype(LD) - r["s2"]).astype(np.float64) / tol)[pos])),
                               conf=float(np.max((np.abs(c[sl].astype(LD) - r["conf"]).astype(np.float64) / r["confb"])[pos]))))
        print(f"clamp patch: {int(neg.sum())} of {len(s2)} queries clamped, {int(pos.sum())} above 0")
    print(f"sigma clamp: worst error / bound mean {worst['f']:.3f}, sigma^2 {worst['s2']:.3f}, confidence {worst['conf']:.3f}")
    assert max(worst.values()) <= 1.0, worst
