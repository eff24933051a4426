"""Every kernel family under GPC_POISON_LDS=1 ("A latent bug found late in the round"): a kernel that reads an LDS word or a
workspace element its call never wrote must show here, whatever ran before it.

One test per record of poison_cases.CASES (test_poison_cpu.py holds the table complete against include/gpc.h).  Protocol per record:
  1. plain    = run on the module's shared, already-used context -- with the family's exact reference held against it where it has one;
  2. poisoned = run on the same context under the switch: every CU's LDS holds the NaN 0x7ff8dead0000beef and the workspace 0xFF bytes
                before every entry;
     fresh    = run on a context created under the switch: every byte its workspace ever had is gpc_ws_reserve's 0xFF fill;
  3. again    = run on the shared context with the switch deleted.
  4. poisoned, fresh and again equal plain by the record's rule: "bits" -- tobytes() of every output, so a leaked poison NaN differs from
     any NaN of the arithmetic -- or "RUN_TOL", test_dense_ev_gpu.RUN_TOL relative to max|plain| on floating outputs, with the non-finite
     positions and every integer output equal exactly (the register kernel alone: poison_cases.py says why)."""
import time

import numpy as np
import pytest

import poison_cases as PC
from test_dense_ev_gpu import RUN_TOL

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def gp():
    from gp_compressor_amd import capi
    capi.load()          # raises if the HIP library is missing: no fallback
    ctx = capi.Context(0)
    yield capi, ctx
    ctx.close()


def _same(case, label, got, plain):
    assert set(got) == set(plain), (case.id, label, sorted(set(got) ^ set(plain)))
    for k, want in plain.items():
        a, w = np.asarray(got[k]), np.asarray(want)
        assert a.shape == w.shape and a.dtype == w.dtype, (case.id, label, k, a.shape, w.shape, a.dtype, w.dtype)
        if case.rule == "bits" or not np.issubdtype(w.dtype, np.floating):
            if a.tobytes() != w.tobytes():
                neq = np.flatnonzero(np.ascontiguousarray(a).reshape(-1).view(np.uint8) != np.ascontiguousarray(w).reshape(-1).view(np.uint8))
                raise AssertionError("%s [%s] output %s: %d bytes differ, the first at element %d; NaNs %d against %d"
                                     % (case.id, label, k, len(neq), neq[0] // max(a.itemsize, 1),
                                        int(np.sum(a != a)) if a.dtype.kind == "f" else 0, int(np.sum(w != w)) if w.dtype.kind == "f" else 0))
            continue
        fin = np.isfinite(w)
        assert np.array_equal(np.isfinite(a), fin) and np.array_equal(np.isnan(a), np.isnan(w)), (case.id, label, k, "non-finite positions")
        assert np.array_equal(a[~fin & ~np.isnan(w)], w[~fin & ~np.isnan(w)]), (case.id, label, k, "infinities")
        if fin.any():
            scale = float(np.max(np.abs(w[fin])))
            err = float(np.max(np.abs(a[fin] - w[fin])))
            assert err <= RUN_TOL * scale, (case.id, label, k, err, scale)


@pytest.mark.parametrize("case", PC.CASES, ids=[c.id for c in PC.CASES])
def test_poisoned_run_equals_the_plain_run(gp, oracle, monkeypatch, case):
    capi, ctx = gp
    for e in PC.SWITCHES:
        monkeypatch.delenv(e, raising=False)
    for k, v in case.env.items():
        monkeypatch.setenv(k, v)
    t0 = time.time()
    plain = case.run(capi, ctx, check=True, oracle=oracle)
    assert plain and all(isinstance(v, np.ndarray) for v in plain.values()), case.id
    t1 = time.time()
    monkeypatch.setenv(PC.POISON, "1")
    poisoned = case.run(capi, ctx)
    other = capi.Context(0)
    try:
        fresh = case.run(capi, other)
    finally:
        other.close()
    monkeypatch.delenv(PC.POISON)
    again = case.run(capi, ctx)
    print("%s: plain run with its reference %.2f s, three more runs %.2f s; rule %s" % (case.id, t1 - t0, time.time() - t1, case.rule))
    for label, got in (("poisoned", poisoned), ("fresh context", fresh), ("again", again)):
        _same(case, label, got, plain)
