"""Conditions on the reference side of tests/test_sparse_readout_gpu.py, checked without a GPU for every case of readout_cases.CASES:
the extended-precision reference is far more exact than the bounds it is held to, the bounds are far smaller than the effect of any
single term a kernel could get wrong, and the handmade states are what they claim to be."""
import numpy as np
import pytest

import readout_cases as RC
from np_restatement import train_sigmaf_np

LD = RC.LD
f64 = lambda a: np.asarray(a, dtype=np.float64)


def _patches(case):
    cap, ny, l_sq = case
    B = RC.batch(cap, ny, l_sq)
    hp, lo = RC.ragged_reference(cap, ny, l_sq), RC.ragged_reference(cap, ny, l_sq, None)
    return B, [(i, int(B["b"][i]), hp[i], lo[i]) for i in range(B["P"]) if hp[i] is not None]


@pytest.mark.parametrize("case", RC.CASES, ids=RC.CASE_IDS)
def test_readout_reference_rounding(case):
    """The float64 NumPy evaluation of the closed form -- a second summation order, in the arithmetic of the kernels -- stays below a
    quarter of every derived bound against the np.longdouble evaluation, and below 1e-10 of the patch's largest value for l and dX: the
    reference's own error (2^-11 of that) is nothing to the bounds."""
    assert np.finfo(LD).eps <= 2.0 ** -63, "np.longdouble is no extended type on this platform"
    B, pp = _patches(case)
    ny = case[1]
    worst = dict(f=0.0, s2=0.0, conf=0.0, l=0.0, dX=0.0)
    for i, b, hp, lo in pp:
        if b:
            with np.errstate(invalid="ignore", divide="ignore"):
                rf = np.where(hp["fb"] > 0, f64(np.abs(lo["f"] - hp["f"])) / hp["fb"], 0.0)
            worst["f"] = max(worst["f"], float(rf.max()))
        else:
            assert np.all(f64(hp["f"]) == 0) and np.all(lo["f"] == 0)
        worst["s2"] = max(worst["s2"], float(np.max(f64(np.abs(lo["s2"] - hp["s2"])) / hp["s2b"])))
        # the sigma^2 bound covers the worst case of the kernels' operations, six roundings of every exponent's argument included
        assert np.all(hp["s2_worst"] <= hp["s2b"]), (i, b, float(np.max(hp["s2_worst"] / hp["s2b"])))
        worst["conf"] = max(worst["conf"], float(np.max(f64(np.abs(lo["conf"] - hp["conf"])) / hp["confb"])))
        for k in ("l", "dX"):
            top = float(np.max(np.abs(hp[k])))
            if top == 0.0:                                           # (an empty field patch: dX = 0)
                assert b == 0 and ny == 3 and k == "dX" and np.all(lo[k] == 0)
                continue
            worst[k] = max(worst[k], float(np.max(np.abs(lo[k] - hp[k]))) / top)
    print(f"float64 against longdouble {case[:2]}: error / bound f {worst['f']:.3f} sigma^2 {worst['s2']:.3f} conf {worst['conf']:.3f}; "
          f"relative l {worst['l']:.1e} dX {worst['dX']:.1e}")
    assert max(worst["f"], worst["s2"], worst["conf"]) < 0.25, worst
    assert max(worst["l"], worst["dX"]) < 1e-10, worst


@pytest.mark.parametrize("case", [c for c in RC.CASES if c[1] == 1], ids=[i for c, i in zip(RC.CASES, RC.CASE_IDS) if c[1] == 1])
def test_readout_reference_rounding_training(case):
    """The same for the training loop and its three per-point sums: float64 against longdouble below a quarter of the 1e-9 / 1e-8 / 1e-7
    bounds, the raw sums below a quarter of the mean and sigma^2 bounds, the iteration counts equal; and the loop's stopping rule is not
    decided by rounding (no gradient norm within 1 % of the 1e-2 threshold)."""
    cap, ny, l_sq = case
    B = RC.batch(cap, 1, l_sq)
    hp, lo = RC.train_reference(cap, l_sq), RC.train_reference(cap, l_sq, None)
    worst, worst_raw, trained = 0.0, 0.0, 0
    for i in range(B["P"]):
        b = int(B["b"][i])
        sl = slice(B["off"][i], B["off"][i + 1])
        assert hp[i][1] == lo[i][1] == ((RC.TRAIN_MAXC + 2) if (b >= 20 and sl.stop > sl.start) else 0), (i, b, hp[i][1], lo[i][1])
        if hp[i][1] == 0:
            assert float(hp[i][0]) == RC.SF
            continue
        trained += 1
        worst = max(worst, RC.train_errors((lo[i][0], lo[i][2], lo[i][3]), hp[i]))
        gn = float(np.sqrt(hp[i][3] @ hp[i][3]))
        assert abs(gn / 1e-2 - 1.0) > 0.01, (i, gn)
        alpha, Cm, BV = RC.patch_state(B, i)
        args = (RC.SF, l_sq, RC.S20, alpha[0], Cm, BV, B["q0"][sl], B["q1"][sl], B["yq"][0, sl], RC.TRAIN_STEP, RC.TRAIN_MAXC)
        qh, ah, hh = train_sigmaf_np(*args, dtype=LD, raw=True)
        ql, al, hl = train_sigmaf_np(*args, raw=True)
        r = RC.ragged_reference(cap, 1, l_sq)[i]
        # h = sum_j |x - BV_j|^2 e_j alpha_j: the mean's bound with the factor d^2 (three more roundings) on every term
        d2 = (B["q0"][sl][:, None] - BV[None, :, 0]) ** 2 + (B["q1"][sl][:, None] - BV[None, :, 1]) ** 2
        hb = RC.EPS * ((d2 * ((b + 12 + 6 * np.abs(f64(r["A"]))) * np.abs(f64(r["K"]))).T) @ np.abs(alpha[0]))
        hb = np.maximum(hb, np.finfo(np.float64).tiny)
        worst_raw = max(worst_raw, float(np.max(f64(np.abs(ql - qh)) / r["s2b"])), float(np.max(f64(np.abs(al - ah)) / r["fb"][0])),
                        float(np.max(f64(np.abs(hl - hh)) / hb)))
    print(f"training, float64 against longdouble (capacity {cap}): {trained} trained patches, error / bound {worst:.1e}, raw sums {worst_raw:.3f}")
    assert trained == sum(b >= 20 for b in RC.BASES[cap]) and worst < 0.25 and worst_raw < 0.25, (trained, worst, worst_raw)


@pytest.mark.parametrize("case", RC.CASES, ids=RC.CASE_IDS)
def test_readout_bounds_are_not_vacuous(case):
    """Sensitivity: for EVERY basis vector j of every patch, leaving the single term v_j k_j out of k^T C k moves sigma^2 at some query of
    the patch by at least 1000 bounds, leaving alpha_cj k_j out of the mean moves f_c by at least 1000 bounds (every channel), and zeroing
    row j of C moves l or dX by at least 1000 of theirs: a kernel that loses, doubles or misplaces one row, one column step or one
    row tile cannot pass."""
    cap, ny, l_sq = case
    B, pp = _patches(case)
    weakest = dict(s2=np.inf, f=np.inf, lik=np.inf)
    for i, b, hp, lo in pp:
        if b == 0:
            continue
        K, CK = f64(hp["K"]), f64(hp["CK"])
        s2 = np.max(np.abs(K * CK) / RC.sigma2_tolerance(hp)[None, :], axis=1)                     # (b,)
        alpha = RC.patch_state(B, i)[0]
        with np.errstate(invalid="ignore", divide="ignore"):
            t = np.abs(alpha[:, :, None] * K[None, :, :]) / hp["fb"][:, None, :]                 # (ny, b, m)
        f = np.max(np.where(np.isfinite(t), t, 0.0), axis=2)
        with np.errstate(invalid="ignore", over="ignore"):            # (without the row sigma falls below 0 at some queries: not counted)
            dXj, lj = RC.drop_row_of_C(lo, ny)
        lb, db = 1e-8 * float(np.max(np.abs(hp["l"]))), 1e-8 * float(np.max(np.abs(hp["dX"])))
        gap = lambda a, ref: np.where(np.isnan(a), 0.0, np.abs(a - ref))
        lik = np.maximum(np.max(gap(lj, lo["l"][None, :]), axis=1) / lb, np.max(gap(dXj, lo["dX"][None, :, :]), axis=(1, 2)) / db)
        assert s2.min() >= 1000 and f.min() >= 1000 and lik.min() >= 1000, (i, b, s2.min(), f.min(), lik.min())
        weakest = dict(s2=min(weakest["s2"], s2.min()), f=min(weakest["f"], f.min()), lik=min(weakest["lik"], lik.min()))
    print(f"weakest single term / bound {case[:2]}: sigma^2 {weakest['s2']:.1e}, mean {weakest['f']:.1e}, l or dX {weakest['lik']:.1e}")


@pytest.mark.parametrize("case", RC.CASES, ids=RC.CASE_IDS)
def test_readout_states_are_well_formed(case):
    """C exactly symmetric and at most 1 / s20 in magnitude, padding zero, the basis sizes the ones of the table (every object with the
    empty patch 0 that has points and an empty one without points in the middle), m = b + 37, sigma^2 >= s20 / 2 at every query."""
    cap, ny, l_sq = case
    B, pp = _patches(case)
    ld = B["ld"]
    assert ld == RC.ld_of(cap) and B["C"].shape == (B["P"], ld, ld) and B["alpha"].shape == (B["P"], ny, ld)
    sizes = B["b"].tolist()
    mid = len(RC.BASES[cap]) // 2
    assert sizes[:mid] + sizes[mid + 1:] == list(RC.BASES[cap]) and sizes[0] == 0 and sizes[mid] == 0 and max(sizes) <= ld
    cnt = np.diff(B["off"])
    assert cnt[mid] == 0 and cnt[0] == RC.N_EXTRA
    assert np.array_equal(np.delete(cnt, mid), np.delete(B["b"], mid) + RC.N_EXTRA)
    for i in range(B["P"]):
        b = sizes[i]
        C, al, BV = B["C"][i], B["alpha"][i], B["BV"][i]
        assert np.array_equal(C, C.T) and np.all(C[b:] == 0) and np.all(C[:, b:] == 0) and np.all(al[:, b:] == 0) and np.all(BV[b:] == 0)
        assert np.all(np.abs(C) <= 1.0 / RC.S20) and np.all(np.abs(BV) <= RC.RES / 2)
        if b:
            assert np.all(np.linalg.eigvalsh(C[:b, :b]) < 0) and len(np.unique(BV[:b], axis=0)) == b
    for i, b, hp, lo in pp:
        assert len(hp["s2"]) == b + RC.N_EXTRA
        assert float(np.min(hp["s2"])) >= RC.S20 / 2 and float(np.max(hp["s2"])) <= RC.SF + RC.S20
        assert np.all(np.isfinite(f64(hp["dX"]))) and np.all(f64(hp["l"]) > 0)


def test_readout_clamp_state_is_far_from_its_boundary():
    """C = -(2 / sf) I on 65 vectors: at the queries that are basis vectors s20 + sf + k^T C k <= s20 - sf, a whole sf below the clamp's
    threshold and ~1e13 bounds away from it; the two patches beside it are ordinary states (sigma^2 >= s20 / 2)."""
    B = RC.clamp_batch()
    assert B["b"].tolist() == [RC.CLAMP_B, RC.CLAMP_B, 20] and np.array_equal(B["C"][1], -(2.0 / RC.SF) * np.diag(np.arange(B["ld"]) < RC.CLAMP_B))
    for i in range(3):
        sl = slice(B["off"][i], B["off"][i + 1])
        r = RC.evaluate(B, i, B["q0"][sl], B["q1"][sl])
        if i == 1:
            at_bv = f64(r["s2"])[:RC.CLAMP_B]
            assert np.all(at_bv <= RC.S20 - RC.SF) and np.all(-at_bv >= 1e12 * RC.sigma2_tolerance(r)[:RC.CLAMP_B])
            assert np.all(f64(r["conf"])[:RC.CLAMP_B] == 100.0)
        else:
            assert float(np.min(r["s2"])) >= RC.S20 / 2
