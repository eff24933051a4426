"""The distortion-bounded prune rule on the CPU (tests/prune_rd_ref.py): the restatement's look-ahead pinned to the oracle's own delete_bv
and predict, the measurement of E64_MSE, and the conditions the GPU cases of tests/test_prune_rd_gpu.py rest on.

Measured here (oracle-trained states of prune_ref.REGIMES, ny = 1 and 3):
  look-ahead against the oracle, first removals of two patches per regime: at most 6.0e-15 relative (capacity -1, ny = 1;
  record E_LOOKAHEAD, gate 64 x);
  E64_MSE (float64 against longdouble restatement from the same bits, `mse` trace down to one vector while the orders agree): 7.84e-11,
  from the capacity -1 row, ny = 3 (ny = 1 there: 5.2e-11; the capped rows stay below 1.9e-11);
  with B_p = 2 mse0_p: no error the loop saw within 1e-6 of its bound, no two lowest scores within prune_ref.GAP_MIN, and per ny at least
  one regime in which every patch removes at least 9 vectors and is stopped by the bound (ny = 1: capacity -1; ny = 3: every regime).
  Smallest distance of a seen error to its bound 1.2e-05, smallest score gap 4.4e-05; capacity 100 removes 80..99 (depth) and 75..81
  (colour) of 100 vectors.
"""
import numpy as np
import pytest

import prune_rd_ref as rd
import prune_ref as pr


@pytest.fixture(scope="module")
def trained(oracle):
    """regime -> (per-patch oracle-trained states, per-patch points)"""
    return {(cap, ny): (pr.oracle_states(oracle, cap, div, n, P, ny), rd.points(cap, n, P, ny)[4]) for cap, div, n, P, ny in rd.regimes()}


def test_class_sum_order():
    """the fixed order, on values whose sum depends on it: classes in ascending i, then the xor tree"""
    rng = np.random.default_rng(3)
    for n in (1, 63, 64, 65, 130, 300):
        e = rng.uniform(0, 1, n) * 10.0 ** rng.integers(-8, 8, n)
        acc = [0.0] * 64
        for i in range(n):
            acc[i % 64] += e[i]
        d = 32
        while d:
            acc = [acc[l] + acc[l ^ d] for l in range(64)]
            d >>= 1
        assert len(set(acc)) == 1 and rd.class_sum(e) == acc[0]
    y = rng.normal(size=(3, 5))
    assert rd.mse_of(np.zeros((3, 0)), np.zeros((0, 2)), np.zeros(5), np.zeros(5), y, 1.0, 1.0) == pytest.approx(np.mean(y * y), rel=1e-15)
    assert np.isnan(rd.mse_of(np.zeros((1, 2)), np.zeros((2, 2)), np.zeros(0), np.zeros(0), np.zeros((1, 0)), 1.0, 1.0))


@pytest.mark.parametrize("cap,div,n,P,ny", rd.regimes())
def test_lookahead_vs_oracle(oracle, trained, cap, div, n, P, ny):
    """first removals of two patches: the restatement's look-ahead error against the oracle's delete_bv followed by its predict"""
    states, pts = trained[(cap, ny)]
    kw = pr.kernel_kw(cap, div, ny)
    op = pr.oracle_params(oracle, cap, div, ny)
    worst = 0.0
    for i in (0, P - 1):
        x0, x1, y = pts[i]
        alpha, C, Q, BV = states[i]
        g = oracle.Sparse(op, alpha.shape[1] + 2)
        g.set_state(alpha, C, Q, BV)
        for _ in range(6):
            loc, _ = pr.argmin_scan(pr.scores_of(alpha, C, Q))
            new = pr.delete_bv(alpha, C, Q, BV, loc, 0)
            e = rd.mse_of(new[0], new[3], x0, x1, y, kw["sigmaf_sq"], kw["l_sq"])
            g.delete_bv(loc)
            f = np.asarray(g.predict(x0, x1)[0]).reshape(ny, -1)
            e_or = float(np.sum((y - f) ** 2) / (len(x0) * ny))
            worst = max(worst, abs(float(e) - e_or) / e_or)
            alpha, C, Q, BV = new
    print(f"cap {cap} ny {ny}: look-ahead vs oracle {worst:.3e} (record {rd.E_LOOKAHEAD:.3e}, gate {pr.GATE_FACTOR * rd.E_LOOKAHEAD:.3e})")
    assert worst <= pr.GATE_FACTOR * rd.E_LOOKAHEAD


def test_e64_mse(trained):
    """E64_MSE over all regimes down to one vector"""
    worst = 0.0
    for cap, div, n, P, ny in rd.regimes():
        states, pts = trained[(cap, ny)]
        kw = pr.kernel_kw(cap, div, ny)
        w, same = 0.0, 0
        for st, (x0, x1, y) in zip(states, pts):
            r64 = rd.prune_rd(*st, x0, x1, y, 1, np.inf, kw, dtype=np.float64)
            rld = rd.prune_rd(*st, x0, x1, y, 1, np.inf, kw, dtype=np.longdouble)
            k = 0
            while k < min(len(r64["order"]), len(rld["order"])) and r64["order"][k] == rld["order"][k]:
                k += 1
            same += k
            w = max(w, rd.rel([r64["mse0"]] + list(r64["mse"][:k]), [rld["mse0"]] + list(rld["mse"][:k])))
        print(f"cap {cap} ny {ny}: float64 vs longdouble mse trace {w:.3e} over {same} common steps")
        worst = max(worst, w)
    print(f"E64_MSE measured: {worst:.3e} (record {rd.E64_MSE:.3e})")
    assert worst <= rd.E64_MSE


def test_gpu_case_conditions(trained):
    """B_p = 2 mse0_p on the oracle-trained states: what the comparison of tests/test_prune_rd_gpu.py assumes"""
    deep = {1: [], 3: []}
    total = 0
    for cap, div, n, P, ny in rd.regimes():
        states, pts = trained[(cap, ny)]
        kw = pr.kernel_kw(cap, div, ny)
        runs = [rd.prune_rd(*st, x0, x1, y, 1, lambda m: 2.0 * m, kw) for st, (x0, x1, y) in zip(states, pts)]
        total += len(runs)
        rm = [len(r["order"]) for r in runs]
        by_bound = [bool(r["mse_next"] > r["bound"]) for r in runs]
        print(f"cap {cap} ny {ny}: removed {min(rm)}..{max(rm)} of {states[0][0].shape[1]}, stopped by the bound {sum(by_bound)}/{P}, "
              f"smallest band {min(r['band'] for r in runs):.2e}, smallest score gap {min(r['gap'] for r in runs):.2e}")
        for r in runs:
            assert r["band"] > rd.BAND and r["gap"] > pr.GAP_MIN
        if min(rm) >= 9 and all(by_bound):
            deep[ny].append(cap)
    print(f"{total} patches; regimes where every patch removes >= 9 vectors and stops by the bound: {deep}")
    assert deep[1] and deep[3]


def test_rule_edges():
    """the stop rule on a toy state: the floor, target >= b, a zero bound, a NaN bound, a NaN in y, a patch without points"""
    rng = np.random.default_rng(1)
    b, n = 6, 40
    A = rng.normal(size=(b, b))
    Q = A @ A.T + b * np.eye(b)
    C = -0.1 * np.linalg.inv(Q + np.eye(b))
    st = (rng.normal(size=(1, b)), C, Q, rng.uniform(-0.07, 0.07, size=(b, 2)))
    x0, x1, y = rng.uniform(-0.07, 0.07, n), rng.uniform(-0.07, 0.07, n), rng.normal(size=(1, n))
    kw = dict(sigmaf_sq=1.0, l_sq=0.02 ** 2)
    full = rd.prune_rd(*st, x0, x1, y, 1, np.inf, kw)
    ref = pr.prune(*st, 1)
    assert np.array_equal(full["order"], ref["order"]) and np.array_equal(full["alpha"], ref["alpha"]) and np.isnan(full["mse_next"])
    assert len(full["mse"]) == b - 1
    r = rd.prune_rd(*st, x0, x1, y, b, np.inf, kw)
    assert len(r["order"]) == 0 and r["mse0"] == full["mse0"] and np.isnan(r["mse_next"])
    r = rd.prune_rd(*st, x0, x1, y, 1, 0.0, kw)
    assert len(r["order"]) == 0 and r["mse_next"] == full["mse"][0]
    r = rd.prune_rd(*st, x0, x1, y, 1, np.nan, kw)
    assert len(r["order"]) == 0 and r["mse_next"] == full["mse"][0]
    k = int(np.argmax(full["mse"] > full["mse"][0])) if np.any(full["mse"] > full["mse"][0]) else 1
    r = rd.prune_rd(*st, x0, x1, y, 1, float(full["mse"][:k].max()), kw)       # stops at the FIRST look-ahead beyond the bound
    assert len(r["order"]) == k and r["mse_next"] == full["mse"][k]
    yn = y.copy()
    yn[0, 7] = np.nan
    r = rd.prune_rd(*st, x0, x1, yn, 1, np.inf, kw)
    assert len(r["order"]) == 0 and np.isnan(r["mse0"]) and np.isnan(r["mse_next"])
    r = rd.prune_rd(*st, x0[:0], x1[:0], y[:, :0], 1, np.inf, kw)
    assert len(r["order"]) == 0 and np.isnan(r["mse0"]) and np.array_equal(r["alpha"], st[0])
