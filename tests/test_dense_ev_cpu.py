"""CPU tests of the restatement in dense_ev_cases.py that test_dense_ev_gpu.py compares the kernels with: the log marginal likelihood of
the regression GP (gpc_dense_fit_predict_ev, include/gpc.h) and the selection rule of gpc_dense_select.  No GPU, no HIP library."""
import math

import numpy as np
import pytest

import dense_ev_cases as DC
import variance_cases as VC


def _e64(regime, batch, dn=1):
    """Worst |float64 - longdouble| / G over the non-empty patches and planes of a batch."""
    off, x0, x1, y = batch
    worst = 0.0
    for i in range(len(off) - 1):
        sl = slice(off[i], off[i + 1])
        if off[i + 1] == off[i]:
            continue
        st, ev, G, _ = DC.log_ev_f64(regime, x0[sl], x1[sl], y[:, sl], dn)
        assert st == 0
        hp = DC.log_ev_hp(regime, x0[sl], x1[sl], y[:, sl], dn)
        worst = max(worst, float(np.max(np.abs(ev.astype(np.longdouble) - hp) / G)))
    return worst


@pytest.mark.parametrize("name", sorted(DC.REGIMES))
def test_restatement_against_longdouble(name):
    """E64: the float64 restatement against the longdouble one, relative to G, on every patch of the GPU tests' batches up to 256 points
    and on one 1024-point patch.  The figure written into dense_ev_cases.py still holds, and with it the gate in force."""
    regime = DC.REGIMES[name]
    worst = max(_e64(regime, DC.edge_patch(n)) for n in DC.EDGE_SIZES if 0 < n <= 256)
    for b in (DC.route_batch(), DC.slot_batch(), DC.plane_batch(False)):
        worst = max(worst, _e64(regime, b))
    big = _e64(regime, DC.edge_patch(1024))
    print("%s: E64 = %.3e (patches up to 256 points), %.3e (1024 points); recorded %.1e" % (name, worst, big, DC.E64_MEASURED))
    assert max(worst, big) <= DC.E64_MEASURED
    assert DC.GATE_RTOL == (DC.EV_RTOL if 16 * DC.E64_MEASURED <= DC.EV_RTOL else 16 * DC.E64_MEASURED)
    assert DC.GATE_RTOL == 1e-11            # the branch in force, as the GPU tests' docstrings quote it


def test_selection_batch_is_decided_by_the_restatement_alone():
    """On the selection batch the restatement picks the generating scale on every patch, never the duplicate, and its best beats its
    second best among the three distinct candidates by more than twice the gate: the GPU test needs no near-tie allowance."""
    off = DC.select_batch()[0]
    n = np.diff(off)
    assert len(n) == DC.SELECT_P and n.min() >= 64 and n.max() <= 200
    assert all(abs(DC.SELECT_L[k + 1] / DC.SELECT_L[k] - 4.0) < 1e-12 for k in range(2)) and DC.CANDIDATES[3] == DC.CANDIDATES[1]
    r = DC.select_ref()
    assert np.all(r["status"] == 0)
    assert np.array_equal(r["best"], np.arange(DC.SELECT_P) % 3)
    s = np.sort(r["sums"][:3], axis=0)
    margin = s[-1] - s[-2]
    g = 2.0 * DC.gate(np.max(r["G"][:, :, 0], axis=0))
    print("margins %s, twice the gate at most %.2e" % (np.array2string(margin, precision=2), g.max()))
    assert np.all(margin > g)
    assert np.array_equal(r["log_ev_all"][3], r["log_ev_all"][1])


def test_best_of_rule():
    """Strict >, lowest index on a tie, NaN and a bad status never win, -1 without an eligible candidate; the sum runs in plane order."""
    ev = np.array([[[1.0, 2.0]], [[2.0, 1.0]], [[np.nan, 9.0]], [[5.0, 5.0]]])           # (H = 4, P = 1, ny = 2)
    st = np.array([[0], [0], [0], [1]], dtype=np.int32)
    best, s = DC.best_of(ev, st)
    assert best[0] == 0 and s[0, 0] == 3.0 and s[1, 0] == 3.0
    best, _ = DC.best_of(ev[2:], st[2:])
    assert best[0] == -1
    best, _ = DC.best_of(np.array([[[-np.inf]], [[-3.0]]]), np.zeros((2, 1), dtype=np.int32))
    assert best[0] == 1


@pytest.mark.parametrize("dn", [0, 1])
def test_closed_form_single_point(dn):
    """n = 1: log_ev = -0.5 y^2 / a - 0.5 log a - 0.5 log 2 pi with a = sigmaf_sq + c noise, c = 1 + ref_double_noise."""
    sf, l_sq, sn = VC.MEDIUM
    for yv in (0.3, -1.7, 0.0):
        a = sf + (1 + dn) * sn
        want = -0.5 * yv * yv / a - 0.5 * math.log(a) - 0.5 * math.log(2 * math.pi)
        st, ev, G, al = DC.log_ev_f64(VC.MEDIUM, np.array([0.01]), np.array([-0.02]), np.array([[yv]]), dn)
        assert st == 0 and abs(ev[0] - want) <= 4e-16 * G[0] and abs(al[0, 0] - yv / a) <= 1e-15 * abs(yv / a)


def test_double_noise_is_a_shift_of_the_noise():
    """ref_double_noise = 1 at noise s is ref_double_noise = 0 at noise 2 s, bit for bit; and it changes the value."""
    batch = DC.edge_patch(65)
    sf, l_sq, sn = VC.DEFAULT
    one = DC.restate(VC.DEFAULT, batch, 1)
    two = DC.restate((sf, l_sq, 2 * sn), batch, 0)
    zero = DC.restate(VC.DEFAULT, batch, 0)
    assert np.array_equal(one["log_ev"], two["log_ev"]) and not np.array_equal(one["log_ev"], zero["log_ev"])


def test_empty_singular_and_planes():
    """An empty patch gives 0; a repeated point without noise gives status 1 and NaN in every plane; the planes are independent."""
    st, ev, G, al = DC.log_ev_f64(VC.DEFAULT, np.zeros(0), np.zeros(0), np.zeros((3, 0)))
    assert st == 0 and np.array_equal(ev, np.zeros(3))
    off, x0, x1, y = DC.plane_batch(False)
    sl = slice(off[0], off[1])
    full = DC.log_ev_f64(VC.MEDIUM, x0[sl], x1[sl], y[:, sl])
    for c in range(3):
        one = DC.log_ev_f64(VC.MEDIUM, x0[sl], x1[sl], y[c:c + 1, sl])
        assert one[1][0] == full[1][c]
    xd0, xd1 = x0[sl].copy(), x1[sl].copy()
    xd0[5], xd1[5] = xd0[2], xd1[2]
    st, ev, _, _ = DC.log_ev_f64(VC.ZERO_NOISE, xd0, xd1, y[:, sl])
    assert st == 1 and np.all(np.isnan(ev))
