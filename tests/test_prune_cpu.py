"""The prune rule on the CPU: the NumPy restatement (tests/prune_ref.py) pinned to the oracle's delete_bv, its arg-min and stop rule at
their edges, and the measurement of E64 -- how far the float64 oracle is from the same chain in longdouble, started from the same bits,
per array and relative to the array's largest magnitude in the patch.  The GPU gate of tests/test_prune_gpu.py is 64 x E64.

Measured here (oracle-trained states of prune_ref.REGIMES, ny = 1 and 3): E64 = alpha 1.70e-10, C 3.42e-11, Q 1.02e-11, BV 0,
mean 4.36e-10, sigma 1.97e-09, all from the capacity -1 row (130 vectors, noise 1e-2); the ny = 3 rows stay below 1e-13 except C at
capacity -1 (3.4e-11).  No patch was left out: the smallest relative distance of the two lowest scores over every step of every patch is
4.4e-05 (capacity 40, ny = 3); at capacity -1 it is 1.8e-04.  The float64 restatement gives the oracle's bits (gap 0 in every array).
test_e64 prints the figures per case and fails when one exceeds prune_ref.E64.
"""
import numpy as np
import pytest

import prune_ref as pr
from gp_compressor_amd import synth

XS0, XS1 = synth.grid(pr.RES, 20)


@pytest.fixture(scope="module")
def measured(oracle):
    """every numeric case once: case -> (oracle results, kept, gaps64, gapsld, P)"""
    out, trained = {}, {}
    for cap, div, n, P, ny, keep in pr.case_ids():
        if (cap, ny) not in trained:
            trained[(cap, ny)] = pr.oracle_states(oracle, cap, div, n, P, ny)
        out[(cap, ny, keep)] = pr.measure_e64(oracle, trained[(cap, ny)], cap, div, ny, keep, XS0, XS1) + (P,)
    return out


def test_argmin_edges():
    nan = np.nan
    assert pr.argmin_scan(np.array([nan, 1.0, 0.5]))[0] == 0                      # a NaN score at index 0 is chosen
    assert pr.argmin_scan(np.array([2.0, nan, 0.5, nan]))[0] == 2                 # a NaN score at another index never is
    assert pr.argmin_scan(np.array([2.0, nan, nan]))[0] == 0
    assert pr.argmin_scan(np.array([3.0, 1.0, 1.0, 2.0, 1.0]))[0] == 1            # equal scores go to the lower index
    assert pr.argmin_scan(np.array([np.inf, np.inf]))[0] == 0
    # the SP_TAKE order gives the scan's answer whatever the shape of the reduction
    rng = np.random.default_rng(5)
    for trial in range(300):
        b = int(rng.integers(1, 40))
        s = rng.choice([0.25, 0.5, 1.0, 2.0, np.inf, nan], size=b, p=[0.2, 0.2, 0.2, 0.2, 0.05, 0.15])
        want = pr.argmin_scan(s)[0]
        for _ in range(4):
            assert pr.argmin_take(s, list(rng.permutation(b)))[0] == want, (s, want)


def _toy(b=6, ny=1, seed=1):
    rng = np.random.default_rng(seed)
    A = rng.normal(size=(b, b))
    Q = A @ A.T + b * np.eye(b)
    C = -0.1 * np.linalg.inv(Q + np.eye(b))
    return rng.normal(size=(ny, b)), C, Q, rng.uniform(-0.07, 0.07, size=(b, 2))


def test_stop_rule():
    st = _toy()
    r = pr.prune(*st, target=6)                       # target >= b, score_tol = 0: nothing goes
    assert len(r["order"]) == 0 and all(np.array_equal(a, b_) for a, b_ in zip((r["alpha"], r["C"], r["Q"], r["BV"]), st))
    assert len(pr.prune(*st, target=9)["order"]) == 0
    r = pr.prune(*st, target=4)
    assert len(r["order"]) == 2 and r["alpha"].shape == (1, 4)
    r = pr.prune(*st, target=6, score_tol=np.inf)     # +inf ends at b = 1
    assert len(r["order"]) == 5 and r["alpha"].shape == (1, 1)
    r = pr.prune(*st, target=0, score_tol=0.0)        # a target below 1 counts as 1
    assert len(r["order"]) == 5
    al = st[0].copy()
    al[0, 0] = np.nan                                 # a NaN minimum (index 0 sticks) stops the score branch ...
    r = pr.prune(al, *st[1:], target=6, score_tol=np.inf)
    assert len(r["order"]) == 0
    r = pr.prune(al, *st[1:], target=5, score_tol=np.inf)      # ... but not the count branch, which removes it and goes on
    assert r["order"][0] == 0 and np.isnan(r["scores"][0])
    al = st[0].copy()
    al[0, 3] = np.nan                                 # a NaN elsewhere is never the minimum while another score is there
    r = pr.prune(al, *st[1:], target=5, score_tol=0.0)
    assert len(r["order"]) == 1 and r["order"][0] != 3


@pytest.mark.parametrize("cap,ny,keep", [(c[0], c[4], c[5]) for c in pr.case_ids()])
def test_restatement_vs_oracle(measured, cap, ny, keep):
    """From the same state bits the oracle driven by delete_bv and the float64 restatement remove the same vectors in the same order
    (asserted inside measure_e64) and their final states differ by at most E64."""
    orc, kept, g64, gld, P = measured[(cap, ny, keep)]
    assert len(kept) >= 0.95 * P, f"{P - len(kept)} of {P} patches have two lowest scores within {pr.GAP_MIN} of each other"
    for i in kept:
        assert len(orc[i]["order"]) == max(0, orc[i]["alpha"].shape[1] + len(orc[i]["order"]) - keep) and orc[i]["alpha"].shape[1] == keep
    for k in pr.ARRAYS:
        worst = max(g[k] for g in g64)
        print(f"cap {cap} ny {ny} keep {keep}: float64 restatement vs oracle, {k}: {worst:.3e} (E64 {pr.E64[k]:.3e})")
        assert worst <= pr.E64[k]


def test_field_bug_short_chain(oracle):
    """ny = 3 with the reference's multiply (ref_field_delete_bug = 1), three removals: same order, same state to E64"""
    cap, div, n, _, P = pr.REGIMES[0]
    states = pr.oracle_states(oracle, cap, div, n, 4, 3, bug=1)
    keep = states[0][0].shape[1] - 3
    orc = pr.run_oracle(oracle, states, cap, div, 3, keep, XS0, XS1, bug=1)
    for st, o in zip(states, orc):
        r = pr.prune(*st, keep, field_bug=1)
        assert np.array_equal(r["order"], o["order"]) and len(o["order"]) == st[0].shape[1] - keep
        for k in ("alpha", "C", "Q", "BV"):
            assert pr.rel_gap(r[k], o[k]) <= pr.E64[k]


def test_e64(measured):
    """E64 per array over every case; the smallest score gap of the kept patches"""
    worst = {k: 0.0 for k in pr.ARRAYS}
    for (cap, ny, keep), (orc, kept, g64, gld, P) in measured.items():
        gap = min(orc[i]["gap"] for i in kept)
        line = {k: max(g[k] for g in gld) for k in pr.ARRAYS}
        print(f"cap {cap} ny {ny} keep {keep}: kept {len(kept)}/{P}, smallest score gap {gap:.2e}, oracle vs longdouble " +
              " ".join(f"{k} {v:.2e}" for k, v in line.items()))
        for k in pr.ARRAYS:
            worst[k] = max(worst[k], line[k])
    print("E64 measured:", {k: float(f"{v:.3e}") for k, v in worst.items()})
    for k in pr.ARRAYS:
        assert worst[k] <= pr.E64[k], (k, worst[k], pr.E64[k])
