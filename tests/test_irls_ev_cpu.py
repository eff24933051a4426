"""What test_irls_ev_gpu.py assumes, checked without a GPU: the NumPy restatement of the probit GP's Laplace evidence (irls_ev_cases.py)
holds on its own -- against a longdouble restatement of its three sums, against the closed form on one point, K a = fhat, sum log L_jj
against slogdet(B) --, the selection batch has the property the GPU test relies on, and the new entries are declared and exported."""
import ctypes
import math
import os
import re

import numpy as np

import irls_cases as IC
import irls_ev_cases as EV
import irls_var_cases as IV


def test_restatement_against_longdouble(oracle):
    """The float64 log q against the longdouble restatement of the three sums (same a, fhat and s, the float64 loop's; the factor redone
    in longdouble) on the w4_batch patches up to 128 points.  E64 = the worst gap relative to 1 + |log q|: measured 1.7e-16; the log q gate
    of the GPU tests follows from it by the rule in irls_ev_cases.py, and the constants there must be what this test finds."""
    off, x0, x1, lab = IC.w4_batch()
    ref = EV.w4_ref(oracle)
    e64, seen = 0.0, 0
    for i, (a, fh, L, s) in ref["fit"].items():
        n = int(off[i + 1] - off[i])
        if n > 128:
            continue
        sl = slice(off[i], off[i + 1])
        hp = EV.log_q_hp(x0[sl], x1[sl], lab[sl], a, fh, s)
        e64 = max(e64, float(abs(np.longdouble(ref["log_q"][i]) - hp) / (1 + abs(hp))))
        seen += 1
    print("E64 = %.2e of 1 + |log q| over %d patches; gate in force %.2e (1 + |log q|)" % (e64, seen, EV.EV_RTOL))
    assert seen >= 10
    assert e64 <= 2.0 * EV.E64_MEASURED, e64
    # the gate rule: 1e-11 unless E64 exceeds a sixteenth of it, then 16 E64
    assert EV.EV_TOL == 1e-11
    assert EV.EV_RTOL == (EV.EV_TOL if EV.E64_MEASURED <= EV.EV_TOL / 16 else 16 * EV.E64_MEASURED)
    assert EV.E64_MEASURED <= EV.EV_TOL / 16 and EV.EV_RTOL == 1e-11
    assert EV.ev_gate(np.array([-3.0]))[0] == 1e-11 * 4.0


def test_one_point_closed_form(oracle):
    """One point: log q = -a f / 2 + log Phi(y f / sqrt s20) - log(1 + W sigmaf_sq) / 2 with W = -r at the iterate the last step
    started from."""
    off, x0, x1, lab = IC.w4_batch()
    ref = EV.w4_ref(oracle)
    ones = [i for i in ref["fit"] if off[i + 1] - off[i] == 1]
    assert ones
    for i in ones:
        a, fh, L, s = ref["fit"][i]
        y = float(lab[off[i]])
        W = float(s[0]) ** 2
        want = -0.5 * float(a[0]) * float(fh[0]) + math.log(0.5 * math.erfc(-y * float(fh[0]) / math.sqrt(EV.S20) / math.sqrt(2.0))) \
            - 0.5 * math.log(1.0 + W * EV.SF)
        assert abs(ref["log_q"][i] - want) <= 1e-14 * (1 + abs(want)), (i, ref["log_q"][i], want)
        assert ref["log_q"][i] < 0.0


def test_k_alpha_is_fhat_and_logdet(oracle):
    """On the w4_batch patches up to 128 points: K a = fhat (what makes -a^T fhat / 2 the prior term) within the fit's tolerance, and
    sum log L_jj = slogdet(B) / 2."""
    off, x0, x1, lab = IC.w4_batch()
    ref = EV.w4_ref(oracle)
    worst_k = worst_d = 0.0
    for i, (a, fh, L, s) in ref["fit"].items():
        n = int(off[i + 1] - off[i])
        if n > 128:
            continue
        sl = slice(off[i], off[i + 1])
        K = IV.kernel(x0[sl], x1[sl], x0[sl], x1[sl])
        worst_k = max(worst_k, float(np.max(np.abs(K @ a - fh))) / max(float(np.max(np.abs(fh))), 1e-300))
        B = np.eye(n) + (s[:, None] * K) * s[None, :]
        sign, ld = np.linalg.slogdet(B)
        ldet = EV.log_q_terms(a, fh, lab[sl], L)[2]
        assert sign == 1.0
        worst_d = max(worst_d, abs(ldet - 0.5 * ld) / (1 + abs(ldet)))
    print("K a - fhat: %.2e of the max-norm; sum log L_jj against slogdet(B) / 2: %.2e" % (worst_k, worst_d))
    assert worst_k <= 1e-9 and worst_d <= 1e-13


def test_restatement_cases(oracle):
    """The cases of the definition on the batches the GPU tests use: an empty patch gives 0, a NaN label status 2 and NaN, every other
    picked patch of many_batch converges with a finite negative log q; the pinned batches end NOT_CONVERGED with a finite log q."""
    c = IC.MANY["big"]
    ref = EV.many_ref(oracle, "big")
    for i in c["empty"]:
        assert ref["log_q"][i] == 0.0 and ref["status"][i] == 0
    for i in c["nan"]:
        assert ref["status"][i] == 2 and np.isnan(ref["log_q"][i])
    rest = [i for i in IV.many_pick("big") if i not in c["empty"] and i not in c["nan"]]
    assert np.all(ref["status"][rest] == 0) and np.all(np.isfinite(ref["log_q"][rest])) and np.all(ref["log_q"][rest] < 0.0)
    for shape in ("big", "w4"):
        n = np.diff(IV.pinned_batch(shape)[0])
        ref = EV.pinned_ref(oracle, shape, 2)
        assert np.all(ref["status"][n > 0] == 5) and np.all(np.isfinite(ref["log_q"])) and np.all(ref["log_q"][n == 0] == 0.0)


def test_fit_patch_theta_is_fit_patch(oracle):
    """fit_patch_theta at the regime of irls_cases.py gives irls_var_cases.fit_patch's bits."""
    off, x0, x1, lab = IC.grid_batch("w4")
    for i in (0, 3, 4):
        sl = slice(off[i], off[i + 1])
        arg = IC.MODELS[2]
        r0 = IV.fit_patch(oracle, 2, x0[sl], x1[sl], lab[sl], IC.MAX_ITER, arg["tol"], arg["f_init"])
        r1 = EV.fit_patch_theta(oracle, x0[sl], x1[sl], lab[sl], IC.REGIME)
        assert r0[:2] == r1[:2]
        for u, v in zip(r0[2:4] + r0[4], r1[2:4] + r1[4]):
            assert np.array_equal(u, v)


def test_selection_batch_property(oracle):
    """The selection batch: 16 patches x 256 points, three candidates; the restatement converges everywhere and picks candidate 1 on
    every patch with a gap of at least 1 in log q to the runner-up -- the GPU gate (1e-11 (1 + |log q|)) is nowhere near it."""
    off, x0, x1, lab = EV.select_batch()
    assert len(off) - 1 == 16 and np.all(np.diff(off) == 256) and set(np.unique(lab)) == {-1.0, 1.0}
    assert len(EV.CANDIDATES) == 3 and [c[1] / EV.L_SQ for c in EV.CANDIDATES] == [1.0 / 16, 1.0, 16.0]
    ref = EV.select_ref(oracle)
    lq = ref["log_q_all"]
    assert np.all(ref["status"] == 0) and np.all(np.isfinite(lq)) and ref["iters"].max() <= IC.MAX_ITER
    assert np.all(ref["best"] == 1), ref["best"]
    srt = np.sort(lq, axis=0)
    gap = float(np.min(srt[-1] - srt[-2]))
    print("smallest top-two gap %.2f; log q of the winners %.1f .. %.1f" % (gap, lq[1].min(), lq[1].max()))
    assert gap >= EV.SELECT_GAP
    assert gap > 1e6 * float(np.max(EV.ev_gate(lq)))
    # the rule itself: ties to the lower index, NaN and a failed status never win, nothing eligible gives -1
    st = np.zeros((3, 4), dtype=np.int32)
    st[0, 3] = 5
    q = np.array([[1.0, np.nan, -np.inf, 9.0], [1.0, -2.0, -np.inf, np.nan], [0.5, -1.0, np.nan, np.inf]])
    assert EV.best_of(q, st).tolist() == [0, 2, -1, -1]


def test_new_symbols_declared_and_exported():
    """The four new entries: declared in include/gpc.h, exported by libgpc_hip.so, bound by capi; gpc_hyper is three doubles."""
    from gp_compressor_amd import capi
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    with open(os.path.join(root, "include", "gpc.h")) as fh:
        hdr = fh.read()
    lib = ctypes.CDLL(capi.LIB_PATH)
    for sym in ("gpc_dense_irls_fit_predict_ev", "gpc_dense_irls_fit_predict_ev_dev", "gpc_dense_irls_select", "gpc_dense_irls_select_dev"):
        assert re.search(r"\bint\s+%s\s*\(" % sym, hdr), sym
        assert hasattr(lib, sym), sym
        assert sym in capi.PROTOTYPES
    assert re.search(r"typedef struct gpc_hyper\s*\{\s*double sigmaf_sq, l_sq, noise;\s*\}\s*gpc_hyper;", hdr)
    assert ctypes.sizeof(capi.Hyper) == 3 * ctypes.sizeof(ctypes.c_double)
    assert [f[0] for f in capi.Hyper._fields_] == ["sigmaf_sq", "l_sq", "noise"]
    for name in ("dense_irls_fit_predict_ev", "dense_irls_fit_predict_ev_dev", "dense_irls_select", "dense_irls_select_dev"):
        assert hasattr(capi.Context, name), name
    assert hasattr(capi.Mapping, "occupancy_select")
