"""The dense predictive mean f* and the weights alpha of every route, held patch by patch against the 80-bit restatement
variance_cases.hp_fit_predict at a gate that follows from a measurement, not from a round number (dense_accuracy_cases.py):

    error <= 8 * E64 + 32 * 2^-53      per (batch, regime, noise convention), E64 = the float64 oracle's own error, recorded from the CPU

Batches (dense_accuracy_cases.py): the edge batch of each route family (every size at which a kernel changes shape, ny = 1 and 3, both
noise conventions, three regimes) and the threshold batches, whose patches put the bound of each exponential selector 2^-20 under and
over each threshold with the bound attained.  Routes: those test_dense_gpu.py's kernel_choice reaches, and the nt16 / nt17 size-class
split that GPC_NO_W1_512 leaves a ragged batch above 256 points to.  Every call goes through the grid entry and the point-wise entry;
asserted per call: last_dense_kernel() names the intended route, status equals the oracle's and is 0 everywhere, f* and alpha are
within the gate.  Every figure is printed before anything is asserted.

Measured on MI355X (1568 figures: 7 routes x 56 cases x 2 entries x {f*, alpha}): every route is inside its gate, the worst at 0.73 of it
-- alpha of the 256-point patch under MEDIUM with single noise, 2.39e-12 against E64 = 4.12e-13, the same figure on the register-tile and
the tiled kernel (they share the Gram evaluation, and under MEDIUM the rounding of K is what alpha sees); the one-wave kernel's worst is
0.68 (same regime), the generic kernel's 0.35; f* stays at or below 0.25 of its gate on every route, regime and entry; on the threshold
batches nothing exceeds 0.29.  No route needed a derived bound.  Per route, regime ("threshold": the threshold batches) and entry, the
case with the largest ratio to its gate (error, the E64 of that case, error / gate; alpha does not depend on the entry):

    route     regime     entry   f*: error   E64       / gate    alpha: error  E64       / gate
    dispatch  default    grid    3.71e-12    2.96e-12  0.156     1.11e-14      3.45e-15  0.357
    dispatch  default    pts     5.49e-13    4.18e-13  0.164     1.11e-14      3.45e-15  0.357
    dispatch  short      grid    2.60e-12    2.04e-12  0.159     6.54e-13      2.19e-13  0.372
    dispatch  short      pts     3.72e-12    2.69e-12  0.173     6.54e-13      2.19e-13  0.372
    dispatch  medium     grid    4.34e-12    4.30e-12  0.126     2.39e-12      4.12e-13  0.726
    dispatch  medium     pts     6.54e-12    4.87e-12  0.168     2.39e-12      4.12e-13  0.726
    dispatch  threshold  grid    5.22e-13    3.29e-13  0.198     8.16e-14      3.46e-14  0.291
    dispatch  threshold  pts     5.05e-13    2.52e-13  0.250     8.16e-14      3.46e-14  0.291
    reg       default    grid    5.70e-13    4.64e-13  0.153     2.40e-15      3.08e-15  0.085
    reg       default    pts     5.49e-13    4.18e-13  0.164     2.40e-15      3.08e-15  0.085
    reg       short      grid    2.22e-12    2.04e-12  0.136     1.46e-12      5.45e-13  0.333
    reg       short      pts     3.72e-12    2.69e-12  0.173     1.46e-12      5.45e-13  0.333
    reg       medium     grid    6.73e-12    4.30e-12  0.196     2.39e-12      4.12e-13  0.726
    reg       medium     pts     5.93e-12    4.87e-12  0.152     2.39e-12      4.12e-13  0.726
    reg       threshold  grid    4.66e-13    4.23e-13  0.137     5.86e-14      3.38e-14  0.214
    reg       threshold  pts     5.26e-13    4.05e-13  0.162     5.86e-14      3.38e-14  0.214
    w2        default    grid    3.99e-12    3.23e-12  0.154     3.07e-15      3.45e-15  0.098
    w2        default    pts     5.49e-13    4.18e-13  0.164     3.07e-15      3.45e-15  0.098
    w2        short      grid    9.80e-13    8.42e-13  0.145     1.46e-12      5.45e-13  0.333
    w2        short      pts     3.72e-12    2.69e-12  0.173     1.46e-12      5.45e-13  0.333
    w2        medium     grid    4.96e-12    4.30e-12  0.144     2.39e-12      4.12e-13  0.726
    w2        medium     pts     5.93e-12    4.87e-12  0.152     2.39e-12      4.12e-13  0.726
    w2        threshold  grid    3.86e-13    4.23e-13  0.114     5.86e-14      3.38e-14  0.214
    w2        threshold  pts     3.97e-13    2.85e-13  0.174     5.86e-14      3.38e-14  0.214
    big       default    grid    4.82e-12    3.23e-12  0.187     2.82e-15      2.99e-15  0.103
    big       default    pts     5.60e-13    4.10e-13  0.171     2.82e-15      2.99e-15  0.103
    big       short      grid    9.80e-13    8.42e-13  0.145     1.46e-12      5.45e-13  0.333
    big       short      pts     3.72e-12    2.69e-12  0.173     1.46e-12      5.45e-13  0.333
    big       medium     grid    4.96e-12    4.30e-12  0.144     2.39e-12      4.12e-13  0.726
    big       medium     pts     5.93e-12    4.87e-12  0.152     2.39e-12      4.12e-13  0.726
    big       threshold  grid    5.23e-13    4.23e-13  0.154     5.86e-14      3.38e-14  0.214
    big       threshold  pts     9.81e-13    6.98e-13  0.176     5.86e-14      3.38e-14  0.214
    big_w4    default    grid    4.82e-12    3.23e-12  0.187     2.82e-15      2.99e-15  0.103
    big_w4    default    pts     5.60e-13    4.10e-13  0.171     2.82e-15      2.99e-15  0.103
    big_w4    short      grid    2.22e-12    2.04e-12  0.136     1.46e-12      5.45e-13  0.333
    big_w4    short      pts     3.72e-12    2.69e-12  0.173     1.46e-12      5.45e-13  0.333
    big_w4    medium     grid    4.72e-12    4.30e-12  0.137     2.39e-12      4.12e-13  0.726
    big_w4    medium     pts     5.93e-12    4.87e-12  0.152     2.39e-12      4.12e-13  0.726
    big_w4    threshold  grid    5.23e-13    4.23e-13  0.154     5.86e-14      3.38e-14  0.214
    big_w4    threshold  pts     9.81e-13    6.98e-13  0.176     5.86e-14      3.38e-14  0.214
    generic   default    grid    5.20e-13    4.64e-13  0.140     3.75e-15      3.43e-15  0.121
    generic   default    pts     5.09e-13    4.18e-13  0.152     3.75e-15      3.43e-15  0.121
    generic   short      grid    6.99e-12    5.45e-12  0.160     5.41e-13      4.04e-13  0.167
    generic   short      pts     5.00e-12    4.00e-12  0.156     5.41e-13      4.04e-13  0.167
    generic   medium     grid    1.16e-11    1.04e-11  0.139     1.15e-12      4.14e-13  0.348
    generic   medium     pts     5.63e-12    4.87e-12  0.144     1.15e-12      4.14e-13  0.348
    generic   threshold  grid    5.77e-13    4.23e-13  0.170     4.31e-14      3.11e-14  0.171
    generic   threshold  pts     5.48e-13    3.26e-13  0.210     4.31e-14      3.11e-14  0.171
    split     default    grid    5.70e-13    4.64e-13  0.153     1.11e-14      3.45e-15  0.357
    split     default    pts     5.49e-13    4.18e-13  0.164     1.11e-14      3.45e-15  0.357
    split     short      grid    2.22e-12    2.04e-12  0.136     6.54e-13      2.19e-13  0.372
    split     short      pts     3.72e-12    2.69e-12  0.173     6.54e-13      2.19e-13  0.372
    split     medium     grid    1.12e-11    1.08e-11  0.129     2.39e-12      4.12e-13  0.726
    split     medium     pts     5.93e-12    4.87e-12  0.152     2.39e-12      4.12e-13  0.726
    split     threshold  grid    5.22e-13    3.29e-13  0.198     8.16e-14      3.46e-14  0.291
    split     threshold  pts     5.05e-13    2.52e-13  0.250     8.16e-14      3.46e-14  0.291
"""
import numpy as np
import pytest

import dense_accuracy_cases as DA

pytestmark = pytest.mark.gpu

ROUTES = {
    "dispatch": {"GPC_W1_MIN_P": "2"},                              # one-wave kernel, its 512 instance, register-tile (colour), tiled above 512
    "reg": {"GPC_NO_W1": "1"},
    "w2": {"GPC_NO_W1": "1", "GPC_W2": "1"},
    "big": {"GPC_FORCE_BIG": "1"},
    "big_w4": {"GPC_FORCE_BIG": "1", "GPC_BIG_NO_W2": "1"},
    "generic": {"GPC_FORCE_GENERIC": "1"},
    "split": {"GPC_W1_MIN_P": "2", "GPC_NO_W1_512": "1"},          # the size-class split instead of the one-wave kernel's 512 instance
}
SWITCHES = ("GPC_FORCE_GENERIC", "GPC_FORCE_BIG", "GPC_NO_W1", "GPC_NO_W1_512", "GPC_W2", "GPC_W1_MIN_P", "GPC_W1_SLOTS", "GPC_NO_SPLIT",
            "GPC_NO_NT17", "GPC_NO_HINT", "GPC_BIG_NO_W2", "GPC_BIG_NO_W4")
SPLIT1, SPLIT3 = "dense_mfma_nt16 + dense_mfma_nt17 + dense_mfma_big", "dense_mfma_nt16 + dense_mfma_big"
# the intended kernel per route, size class of the batch (largest patch <= 256, <= 512, 1024) and ny: (ny = 1, ny = 3)
WANT = {
    "dispatch": {"n256": ("dense_mfma_w1", "dense_mfma_nt16"), "n512": ("dense_mfma_w1_512", SPLIT3), "tiled": (SPLIT1, SPLIT3)},
    "reg": {"n256": ("dense_mfma_nt16", "dense_mfma_nt16"), "n512": (SPLIT1, SPLIT3), "tiled": (SPLIT1, SPLIT3)},
    "w2": {"n256": ("dense_mfma_big_w2", "dense_mfma_nt16"), "n512": (SPLIT1, SPLIT3), "tiled": (SPLIT1, SPLIT3)},
    "big": {"n256": ("dense_mfma_big_w2", "dense_mfma_big_w4"), "n512": ("dense_mfma_big",) * 2, "tiled": ("dense_mfma_big",) * 2},
    "big_w4": {"n256": ("dense_mfma_big_w4",) * 2, "n512": ("dense_mfma_big",) * 2, "tiled": ("dense_mfma_big",) * 2},
    "generic": {k: ("dense_generic",) * 2 for k in ("n256", "n512", "tiled")},
    "split": {"n256": ("dense_mfma_w1", "dense_mfma_nt16"), "n512": (SPLIT1, SPLIT3), "tiled": (SPLIT1, SPLIT3)},
}
SIZE_CLASS = {"n256": "n256", "n512": "n512", "tiled": "tiled", "t256": "n256", "t512": "n512"}

_ORACLE = {}


@pytest.fixture(scope="module")
def gp():
    from gp_compressor_amd import capi
    capi.load()          # raises if the HIP library is missing: no fallback
    ctx = capi.Context(0)
    yield capi, ctx
    ctx.close()


@pytest.fixture(scope="module")
def solved():
    """Every 80-bit solve of the module, once"""
    DA.prefetch(DA.edge_cases() + DA.threshold_cases())


@pytest.fixture(params=list(ROUTES))
def route(request, monkeypatch):
    for e in SWITCHES:
        monkeypatch.delenv(e, raising=False)
    for k, v in ROUTES[request.param].items():
        monkeypatch.setenv(k, v)
    return request.param


def _oracle_status(oracle, case):
    """The oracle's status per patch of a case (and, for the printed table, its own errors): computed once"""
    cid = DA.case_id(case)
    if cid not in _ORACLE:
        fg, fp, al, st = DA.oracle_fit(oracle, case)
        st.setflags(write=False)
        _ORACLE[cid] = (st, {k: v[0] for k, v in DA.errors(case, fg, fp, al).items()})
    return _ORACLE[cid]


def _check(capi, ctx, oracle, route, case, failures):
    """One case through both entries of the route in force; prints every figure, appends what misses to failures"""
    batch, regime, dbl = DA.case_inputs(case)
    cid, ny = DA.case_id(case), batch[3].shape[0]
    want = WANT[route][SIZE_CLASS[case[1]]][0 if ny == 1 else 1]
    so, eo = _oracle_status(oracle, case)
    gates, e64 = DA.gates(case), dict(zip(("f_grid", "f_pts", "alpha"), DA.E64[cid]))
    p = capi.default_params_dense(sigmaf_sq=regime[0], l_sq=regime[1], noise=regime[2], ref_double_noise=dbl)
    _, (q0, q1) = DA.xstars()
    for entry in ("grid", "pts"):
        if entry == "grid":
            f, st, al = ctx.dense_fit_predict_grid(p, *batch, DA.RES, DA.SZ, want_alpha=True)
        else:
            f, _, st, al = ctx.dense_fit_predict(p, *batch, q0, q1, want_alpha=True)
        name = ctx.last_dense_kernel()
        e = DA.errors(case, alpha=al, **{"f_" + entry: f})
        for what, (err, at) in e.items():
            print("%-8s %-30s %-4s %-7s err %.2e (patch %2d)  E64 %.2e  oracle now %.2e  err / gate %6.3f   %s"
                  % (route, cid, entry, what, err, at, e64[what], eo[what], err / gates[what], name))
            if not err <= gates[what]:
                failures.append((route, cid, entry, what, name, "err %.3e > gate %.3e, patch %d" % (err, gates[what], at)))
        if name != want:
            failures.append((route, cid, entry, "kernel", name, "wanted " + want))
        if not (np.array_equal(st, so) and np.all(st == 0)):
            failures.append((route, cid, entry, "status", name, st.tolist()))


@pytest.mark.parametrize("family", list(DA.FAMILIES))
def test_edge_batch_within_gate(gp, oracle, solved, route, family):
    """The family's edge batch under every regime, both noise conventions, ny = 1 and 3, both entries"""
    capi, ctx = gp
    failures = []
    for case in DA.edge_cases():
        if case[1] == family:
            _check(capi, ctx, oracle, route, case, failures)
    assert not failures, failures


@pytest.mark.parametrize("sizeset", list(DA.THR_SIZES))
def test_threshold_batches_within_gate(gp, oracle, solved, route, sizeset):
    """The selector bounds 2^-20 under and over 2^-5 and 2^-8 (Gram and grid), and under 2^-3, both entries.  Depth plane: with the routes
    above every kernel takes it -- the one-wave kernel with its two polynomial degrees, the register-tile and the tiled kernel with one."""
    capi, ctx = gp
    failures = []
    for case in DA.threshold_cases():
        if case[1] == sizeset:
            _check(capi, ctx, oracle, route, case, failures)
    assert not failures, failures
