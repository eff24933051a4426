"""The allocation rule of gpc_rate_allocate on the CPU: the host twin (gpc_test_rate_allocate_host, the kernels' own source) against the
NumPy restatement (rate_alloc_ref.py), bit for bit -- the arithmetic is fully specified, so nothing is a tolerance -- and the rule's
invariants: a feasible answer meets the saving, the refinement splits ties down to less than one row's step, and the unrefined choice is
optimal among the allocations that save as much."""
import numpy as np
import pytest

import rate_alloc_ref as RA

CASES = {
    "random": dict(seed=1, R=37, ld=12, kind="random"),
    "monotone": dict(seed=2, R=29, ld=20, kind="monotone", weights="rows"),
    "non_monotone_weighted": dict(seed=3, R=23, ld=9, kind="random", weights="rows"),
    "nan_holes_and_nan_d0": dict(seed=4, R=31, ld=11, kind="nan"),
    "kmax_zero": dict(seed=5, R=16, ld=7, kind="kmax0"),
    "mixed_units": dict(seed=6, R=33, ld=10, kind="random", units="mixed", weights="rows"),
    "identical_rows": dict(seed=7, R=40, ld=8, kind="identical"),
    "one_row": dict(seed=8, R=1, ld=5, kind="random"),
}


@pytest.fixture(scope="module")
def capi():
    from gp_compressor_amd import build, capi as m
    build.build()
    m.load()
    return m


def _check(capi, pb, need, refine, count):
    want = RA.allocate(pb, need, refine, count)
    k, tg, res = capi.test_rate_allocate_host(*pb.args()[:3], need, w=pb.w, w_all=pb.w_all, unit=pb.unit, unit_all=pb.unit_all, refine=refine,
                                              count=count)
    tag = (need, refine)
    assert np.array_equal(k, want["k"]), tag
    assert np.array_equal(tg, want["target"]), tag
    for f in ("lambda_bits", "saved", "max_saving", "feasible", "switched_rows"):
        assert res[f] == want[f], (tag, f, res[f], want[f])
    assert res["saved"] == RA.saving(pb, k)
    if res["feasible"]:
        assert res["saved"] >= need, tag
    else:
        assert res["max_saving"] < need and res["lambda"] == float("inf")
    return k, res


@pytest.mark.parametrize("name", sorted(CASES))
@pytest.mark.parametrize("refine", [0, 1])
def test_host_twin_equals_the_restatement(capi, name, refine):
    pb = RA.random_problem(**CASES[name])
    count = (pb.kmax + np.arange(pb.R) % 3).astype(np.int32)          # basis counts at and above kmax + 1: target reaches its floor of 1
    for need in RA.needs_of(pb):
        _check(capi, pb, need, refine, count)


def test_refinement_splits_identical_rows(capi):
    pb = RA.random_problem(**CASES["identical_rows"])
    ms = RA.saving(pb, RA.choice(pb, float("inf")))
    assert ms == 40 * 8 * 24
    for need in (1, 25, ms // 4, ms // 2 + 7, ms - 24):
        k1, r1 = _check(capi, pb, need, 1, pb.kmax)
        k0, r0 = _check(capi, pb, need, 0, pb.kmax)
        assert 0 <= r1["saved"] - need < 24, (need, r1)                # less than one row's step (a step here is one removal)
        assert r0["saved"] >= r1["saved"] and r0["lambda_bits"] == r1["lambda_bits"]
        assert np.all(np.diff(k1) <= 0), "rows are switched in ascending row order"
        assert len(set(k0.tolist())) == 1, "without the refinement identical rows move together"


def test_unrefined_choice_is_optimal_on_brute_forced_problems(capi):
    """R <= 6, kmax <= 4, small-integer data: no allocation that saves at least what ours saves has a total sum D below ours by more than
    a relative 1e-12 (the rounding of the lambda * rate terms)."""
    for seed in range(12):
        rng = np.random.default_rng(100 + seed)
        pb = RA.random_problem(seed=200 + seed, R=int(rng.integers(2, 7)), ld=4, kind="integer", units="mixed" if seed % 2 else "24")
        every = RA.brute_force(pb)
        for need in RA.needs_of(pb) + [24, 48, 100]:
            k, res = _check(capi, pb, need, 0, pb.kmax)
            ours = RA.total_error(pb, k)
            best = min(e for s, e, _ in every if s >= res["saved"])
            assert best >= ours - 1e-12 * max(abs(ours), 1.0), (seed, need, ours, best)


def test_arguments_are_checked(capi):
    L = capi.load()
    pb = RA.random_problem(seed=9, R=4, ld=3)
    km, d0, d = pb.args()[:3]

    def call(R=4, ld=3, kmax=km, d0_=d0, d_=d, w_all=1.0, unit_all=24, count=None, target=None):
        p = capi._ptr
        return L.gpc_test_rate_allocate_host(R, ld, p(kmax), p(d0_), p(d_), None, w_all, None, unit_all, 10, 1, p(count), None, p(target), None)
    assert call() == capi.GPC_OK
    assert call(R=0, kmax=None, d0_=None, d_=None) == capi.GPC_OK
    tg = np.zeros(4, dtype=np.int32)
    for bad in (dict(R=-1), dict(ld=0), dict(kmax=None), dict(d0_=None), dict(d_=None), dict(w_all=float("nan")), dict(w_all=-1.0),
                dict(unit_all=0), dict(target=tg)):
        assert call(**bad) == capi.GPC_EINVAL, bad
    assert call(target=tg, count=km) == capi.GPC_OK
