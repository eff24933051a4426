"""The dense kernels on non-finite inputs, on every route (dense_nonfinite_cases.py; the contract is in include/gpc.h, dense section).

Routes, switches and intended kernels are those of test_dense_accuracy_gpu.py (imported); with the variance the names are WANT_VAR below.
Per case the grid entry (training poisons only) and the point-wise entry run -- without the variance, with it, and with it but without
alpha_out.  Asserted per call, after every figure is printed:
    * last_dense_kernel() names the intended route;
    * the status vector is the oracle's (test_dense_nonfinite_cpu.py holds the oracle to the same pattern);
    * x-poisoned patch: status GPC_STATUS_NOT_SPD, every entry of its f*, alpha and v* NaN;
    * y-poisoned patch: status 0, the poisoned channel's alpha and f* non-finite throughout, its other channels clean, its v* the bits of
      the clean call;
    * NaN X*: column j of f* and v* NaN on every non-empty patch; infinite X*: column j of f* is 0 on every patch (exp(-inf) = 0 against
      every training point: that, not NaN, is what the oracle gives) and v* NaN on every non-empty patch (k(x*, x*) = sf exp(c (inf - inf)^2));
      the empty patch under either: f* = 0 and v* = sigma_f^2, as dense_variance.hip and dense_generic.hip write an empty patch without
      evaluating anything -- the oracle's v* there is NaN, and include/gpc.h makes the prior the contract;
    * everything clean -- other patches, channels, columns -- is finite, within 1e-12 max|.| of the same call on the unpoisoned batch
      (the project's run-to-run spread for outputs that pass the LDS atomics of the backward solve), within FTOL / ATOL / VTOL of
      test_dense_gpu.py against the oracle, and v* has the BITS of the unpoisoned call.  One exception by construction: under an X*
      poison the other columns of v* are held to 1e-12 max|v*| instead of to the bits, because dense_variance.hip:96-110 picks the
      exponential (polynomial | table) from the extent of ALL of X*, and an infinite X* moves every column to the table.
The stride batch (4200 patches, a third poisoned) goes through the host-pointer grid entry on every route, in the pipeline's four chunks
and in one (GPC_HOST_NO_PIPELINE: a stride of 1024 has its successor pairs only there), on the one-wave route also with GPC_W1_SLOTS = 5
and 7, once with GPC_POISON_LDS=1 and once through the point-wise entry with the variance; same assertions per patch, and the worst clean
deviation over the successor pairs (i poisoned, i + G clean and smaller) is printed separately.

What the test found: v* in the column of an infinite X* was sigma_f^2 on every route (the kernels took k(x*, x*) = sf as a constant) where
the reference arithmetic gives NaN; gpc_kss (gpc_device.h) now forms it as the sparse path's sp_kstar does.  Nothing else missed.

Measured on MI355X, 5548 calls (5296 of them on a poisoned batch): every assertion holds on all seven routes.  Worst figure over the
poisoned calls of a route -- clean entries against the same call on the unpoisoned batch and against the oracle, relative to the
largest entry (v* against the oracle: absolute) -- and the successor pairs of the stride batch at that route's stride (all with deviation 0 and finite):

    route     calls  f*: clean   oracle    alpha: clean  oracle    v*: clean   oracle     successor pairs (ny = 1 | 3)
    dispatch    760  9.79e-14   5.06e-13  6.33e-16      3.73e-15  1.73e-16    8.67e-18   461 (5 slots), 455 (7 slots) | one workgroup per patch
    reg         756  9.79e-14   5.06e-13  6.33e-16      3.73e-15  1.73e-16    8.67e-18   one workgroup per patch
    w2          756  9.79e-14   5.06e-13  5.85e-16      3.73e-15  1.73e-16    8.67e-18   one workgroup per patch
    big         756  0.00e+00   4.94e-13  0.00e+00      3.73e-15  0.00e+00    8.67e-18   340 at 1024 (5 in four chunks) | 406 at 512 (235)
    big_w4      756  0.00e+00   4.94e-13  0.00e+00      3.73e-15  0.00e+00    8.67e-18   406 at 512 (235) | 406 at 512 (235)
    generic     756  0.00e+00   6.26e-13  0.00e+00      5.08e-15  0.00e+00    1.73e-18   340 at 1024 (5) | 340 at 1024 (5)
    split       756  9.79e-14   5.06e-13  7.48e-16      3.73e-15  1.73e-16    8.67e-18   one workgroup per patch
The non-zero "clean" figures of f* and alpha are the register-tile kernel's own run-to-run spread (its backward solve adds with LDS
atomics; a tenth of the 1e-12 allowed), the same under a training poison as under an X* poison; the one-wave, the tiled and the generic
kernel gave the bits of the unpoisoned call.  v* lost its bits in 12 calls, all of them an infinite X* under dense_variance_kernel.

Every selector and comparison the kernels wrote for this case, the mutation that would undo it and the case that fails then -- argued
from the code, nothing here breaks the library on purpose:
    mfma_tile.h:179, :249    `!(pd > pivot_tol)` as `pd <= pivot_tol`: a NaN pivot passes and the patch keeps status 0.  The status
                             assertion of every x poison: :179 (mf_diag_factor) on reg, w2, big, big_w4 and split, :249 (mf_diag_factor_c)
                             on dispatch and split at ny = 1.  Position (c) is the sharpest: the NaN enters with the last pivot of the
                             last tile, beside the identity padding, and no later pivot is there to flag it instead.
    dense_generic.hip:42     the same comparison in diag_chol_wave: every x poison on generic, and on big / big_w4 at n256 with the variance.
    gpc_device.h:57-73       gpc_exp_neg, "a NaN argument still comes out as NaN": its clamp written `!(x >= -760.0) ? -760.0 : x`, or a
                             NaN select to 0, makes exp(NaN) = 0.  An infinite coordinate is what reaches it in the default regime (an
                             infinite extent fails every small-argument test, so the patch runs table-driven): its diagonal entry is
                             exp(c (inf - inf)^2), the row beside it exp(-inf) = 0, and with exp(NaN) = 0 the patch is SPD again --
                             status 0, finite outputs.  x1_pinf and x0_ninf at every position and x_two_pinf, on every MFMA route.  The
                             `(int)` of a NaN there is harmless only because the table index is masked to 0 .. 63 and the NaN returns
                             through p; no test here may make it otherwise.
    dense_mfma_w1.hip:266    `nan_box` forced false changes no output: fmin / fmax drop a NaN coordinate, so the box of x0_nan is that of
                             its finite points, and the NaN extent of a patch whose points all share an infinite coordinate (the
                             one-point patch, position (d)) still fails `tg <= ...`, which is false for NaN.  It guards the comparisons
                             behind it against being rewritten as `!(tg > ...)`.  With both mutations a one-point patch takes the
                             degree-5 polynomial on coordinates scaled to NaN: the Gram entry is NaN all the same.  Every mode maps a NaN
                             argument to NaN, and a polynomial at an infinite argument gives +-inf beside a NaN diagonal, so the patch
                             ends NaN with status 1 whichever mode runs: the selector decides speed, and what x1_pinf / x0_nan at (a), (b),
                             (d) on dispatch and split pin is that outcome and the untouched neighbours.
    dense_mfma.hip:291,      "false for NaN / inf extents" (small_gram, small_grid): as above for the training points -- an infinite extent
    dense_mfma_big.hip:268   in the polynomial gives +-inf entries beside the NaN diagonal, the patch is NaN either way.
    dense_variance.hip:102   "a NaN extent fails the test below" (small_k) decides VALUES for X*: an infinite X* let into the polynomial
                             (the `<=` rewritten, or the extent clamped) gives k* = +-inf instead of 0 and f* of column j is no longer 0:
                             xs_pinf on every route with the variance.  A NaN X* is dropped by fmax, leaves the extent alone and comes out
                             NaN from either branch (xs_nan keeps the bits of the other columns, as measured).
    gpc_device.h gpc_kss     `sf` in its place (the parent commit): v* of xs_pinf's column is sigma_f^2, not NaN.
    select, not multiply     a 0.0 lane mask in place of a select makes 0 x NaN of a padding lane or a left-over slot: the clean neighbours
                             of every x poison, the clean channels of every y poison at ny = 3 (0 x inf), the stride batch's successor
                             pairs (a smaller clean patch in the workgroup, factor slot or LDS image a larger poisoned one left) and the
                             GPC_POISON_LDS run."""
import numpy as np
import pytest

import dense_nonfinite_cases as NF
from test_dense_accuracy_gpu import ROUTES, SWITCHES, WANT, route  # noqa: F401  (route: the fixture)
from test_dense_gpu import ATOL, FTOL, VTOL

pytestmark = pytest.mark.gpu

RUN_TOL = 1e-12                 # run-to-run spread of f* and alpha (test_dense_golden, test_host_pointer_entry_pipeline_and_pinned_buffers)
NT16V, BIGV = "dense_mfma_nt16 + dense_variance", "dense_mfma_big + dense_variance_big"
# the intended kernels of the point-wise entry WITH the variance, per route, size class and ny: (ny = 1, ny = 3).  The variance has no
# size-class split and no 512 instance; GPC_FORCE_BIG leaves n <= 256 with the variance to the generic kernel (dense_route.h)
WANT_VAR = {
    "dispatch": {"n256": ("dense_mfma_w1 + dense_variance", NT16V), "n512": (BIGV,) * 2, "tiled": (BIGV,) * 2},
    "reg": {"n256": (NT16V,) * 2, "n512": (BIGV,) * 2, "tiled": (BIGV,) * 2},
    "w2": {"n256": (NT16V,) * 2, "n512": (BIGV,) * 2, "tiled": (BIGV,) * 2},
    "big": {"n256": ("dense_generic",) * 2, "n512": (BIGV,) * 2, "tiled": (BIGV,) * 2},
    "big_w4": {"n256": ("dense_generic",) * 2, "n512": (BIGV,) * 2, "tiled": (BIGV,) * 2},
    "generic": {k: ("dense_generic",) * 2 for k in ("n256", "n512", "tiled")},
    "split": {"n256": ("dense_mfma_w1 + dense_variance", NT16V), "n512": (BIGV,) * 2, "tiled": (BIGV,) * 2},
}
# the stride batch (largest patch: 47 points): the grid entry's kernel per route (ny = 1, ny = 3) and the stride G at which that kernel
# hands a workgroup on (None: one workgroup per patch)
WANT_STRIDE = {
    "dispatch": ("dense_mfma_w1", "dense_mfma_nt4"), "reg": ("dense_mfma_nt4",) * 2, "w2": ("dense_mfma_nt4",) * 2,
    "big": ("dense_mfma_big_w2", "dense_mfma_big_w4"), "big_w4": ("dense_mfma_big_w4",) * 2, "generic": ("dense_generic",) * 2,
    "split": ("dense_mfma_w1", "dense_mfma_nt4"),
}
STRIDE_OF = {"dense_mfma_big_w2": 1024, "dense_mfma_big_w4": 512, "dense_generic": 1024}

_STRIDE_ORACLE = {}


@pytest.fixture(scope="module")
def gp():
    from gp_compressor_amd import capi
    capi.load()          # raises if the HIP library is missing: no fallback
    ctx = capi.Context(0)
    yield capi, ctx
    ctx.close()


def _call(capi, ctx, entry, b, q):
    """One call of an entry -- "grid", "pts", "ptsv" (with the variance), each with alpha wanted, or "ptsvn" (the variance, alpha_out
    NULL: the one-wave kernel then keeps the weights in its workspace) -> dict(st, f, al | None, v | None), the kernel's name"""
    p = capi.default_params_dense(want_variance=int(entry.startswith("ptsv")))
    if entry == "grid":
        f, st, al = ctx.dense_fit_predict_grid(p, *b, NF.RES, NF.SZ, want_alpha=True)
        v = None
    elif entry == "ptsvn":
        f, v, st = ctx.dense_fit_predict(p, *b, *q)
        al = None
    else:
        f, v, st, al = ctx.dense_fit_predict(p, *b, *q, want_alpha=True)
    return dict(st=st, f=f, al=al, v=v), ctx.last_dense_kernel()


def _dev(a, b, mask):
    return float(np.max(np.abs(a[mask] - b[mask]))) if np.any(mask) else 0.0


def _amax(a, mask=None):
    a = a if mask is None else a[mask]
    return max(float(np.max(np.abs(a))), 1e-300) if a.size else 1e-300


def _judge(tag, e, out, name, want, ref, orc, v_bits, failures):
    """The assertions of one call, figures first.  ref: the same call on the unpoisoned batch; orc: the oracle on the unpoisoned batch."""
    fig = {}
    for k, mk, tol in (("f", "f_clean", FTOL), ("al", "al_clean", ATOL)):
        if out[k] is None:
            fig[k] = (0.0, 0.0, tol)
            continue
        finite = np.isfinite(out[k]) & e[mk]
        fig[k] = (_dev(out[k], ref[k], finite) / _amax(ref[k]), _dev(out[k], orc[k], finite) / _amax(orc[k]), tol)
    has_v = out["v"] is not None
    if has_v:
        finite = np.isfinite(out["v"]) & e["v_clean"]
        same = bool(np.array_equal(out["v"][e["v_clean"]].view(np.uint64), ref["v"][e["v_clean"]].view(np.uint64)))
        fig["v"] = (_dev(out["v"], ref["v"], finite) / _amax(ref["v"]), _dev(out["v"], orc["v"], finite), VTOL)
        prior = _dev(out["v"], np.full_like(out["v"], NF.REGIME[0]), e["v_prior"])
    print("%-46s %-30s  f* vs clean %.2e oracle %.2e | alpha %.2e %.2e | v* %s" % (
        tag, name, fig["f"][0], fig["f"][1], fig["al"][0], fig["al"][1],
        "vs clean %.2e (bits %s) oracle %.2e prior %.2e" % (fig["v"][0], same, fig["v"][1], prior) if has_v else "-"))
    if name != want:
        failures.append((tag, "kernel", name, "wanted " + want))
    for msg in NF.pattern_failures(e, out, entry_has_v=has_v):
        failures.append((tag, name, msg))
    for k in ("f", "al"):
        if not fig[k][0] <= RUN_TOL:
            failures.append((tag, name, "%s: clean entries %.3e from the clean call (relative to its largest)" % (k, fig[k][0])))
        if not fig[k][1] <= fig[k][2]:
            failures.append((tag, name, "%s: clean entries %.3e from the oracle (relative to its largest)" % (k, fig[k][1])))
    if has_v:
        if v_bits and not same:
            failures.append((tag, name, "v*: clean entries do not have the bits of the clean call (off by %.3e)" % fig["v"][0]))
        if not fig["v"][0] <= RUN_TOL:
            failures.append((tag, name, "v*: clean entries %.3e from the clean call" % fig["v"][0]))
        if not fig["v"][1] <= VTOL:
            failures.append((tag, name, "v*: clean entries %.3e from the oracle" % fig["v"][1]))
        if not prior <= VTOL:
            failures.append((tag, name, "v*: a prior entry is %.3e from sigma_f^2" % prior))


def _want(route, family, ny, entry):
    return (WANT_VAR if entry.startswith("ptsv") else WANT)[route][family][0 if ny == 1 else 1]


def _clean_calls(capi, ctx, oracle, route, family, ny, entries, failures):
    """The entries on the unpoisoned batch: the reference of `within 1e-12 of the clean call`, itself held to the oracle"""
    b, q = NF.batch(family, ny), NF.xstars()
    orc = NF.oracle_clean(oracle, family, ny)
    none = NF.expect_masks(b[0], ny, NF.M_PTS)
    ref = {}
    for entry in entries:
        ref[entry], name = _call(capi, ctx, entry, b, q)
        _judge("%s %s-%d clean %s" % (route, family, ny, entry), none, ref[entry], name, _want(route, family, ny, entry), ref[entry],
               orc["grid" if entry == "grid" else "pts"], True, failures)
    return ref, orc


@pytest.mark.parametrize("ny", [1, 3])
@pytest.mark.parametrize("family", list(NF.FAMILIES))
def test_training_poisons(gp, oracle, route, family, ny):
    """x and y poisons at the positions (a) .. (d): grid entry, point-wise entry without the variance, with it, and with it but without alpha_out"""
    capi, ctx = gp
    failures = []
    entries = ("grid", "pts", "ptsv", "ptsvn")
    ref, orc = _clean_calls(capi, ctx, oracle, route, family, ny, entries, failures)
    for case in NF.train_cases():
        if case[0] != family or case[1] != ny:
            continue
        e = NF.expect(case)
        so = NF.oracle_case(oracle, case)[0]
        b, q = NF.poisoned(case)
        for entry in entries:
            oe = "grid" if entry == "grid" else "pts"
            assert np.array_equal(so[oe]["st"], e["status"])                    # the oracle's status is the pattern's
            out, name = _call(capi, ctx, entry, b, q)
            _judge("%s %s %s" % (route, NF.case_id(case), entry), e, out, name, _want(route, family, ny, entry), ref[entry], orc[oe], True, failures)
    assert not failures, failures


@pytest.mark.parametrize("family", list(NF.FAMILIES))
def test_xstar_poisons(gp, oracle, route, family):
    """One coordinate of one X* NaN or infinite: point-wise entry without and with the variance, ny = 1 and 3"""
    capi, ctx = gp
    failures = []
    for ny in (1, 3):
        ref, orc = _clean_calls(capi, ctx, oracle, route, family, ny, ("pts", "ptsv"), failures)
        for case in NF.xs_cases():
            if case[0] != family or case[1] != ny:
                continue
            e = NF.expect(case)
            b, q = NF.poisoned(case)
            for entry in ("pts", "ptsv"):
                out, name = _call(capi, ctx, entry, b, q)
                # v_bits False: dense_variance.hip:96-110, see the module docstring
                _judge("%s %s %s" % (route, NF.case_id(case), entry), e, out, name, _want(route, family, ny, entry), ref[entry], orc["pts"], False,
                       failures)
    assert not failures, failures


def _stride_oracle(oracle, ny, grid):
    key = (ny, grid)
    if key not in _STRIDE_ORACLE:
        _STRIDE_ORACLE[key] = NF._oracle_run(oracle, NF.stride_batch(ny)[1], NF.xstars(), grid)
    return _STRIDE_ORACLE[key]


def _stride_run(capi, ctx, oracle, tag, ny, entry, want, G, chunks, failures):
    """The stride batch and its unpoisoned twin through one entry; the successor pairs of stride G (in `chunks` kernel batches) apart"""
    bad_b, clean_b, _, _ = NF.stride_batch(ny)
    q = NF.xstars()
    ref, _ = _call(capi, ctx, entry, clean_b, q)
    out, name = _call(capi, ctx, entry, bad_b, q)
    e = NF.stride_expect(ny, NF.M_PTS)
    _judge(tag, e, out, name, want, ref, _stride_oracle(oracle, ny, entry == "grid"), True, failures)
    pairs = NF.successor_pairs(G, chunks, ny) if G else np.zeros((0, 2), dtype=np.int64)
    succ = pairs[:, 1]
    worst = float(np.max(np.abs(out["f"][succ] - ref["f"][succ]))) / _amax(ref["f"]) if len(succ) else 0.0
    print("%-46s successor pairs at stride %s in %d chunk(s): %d, worst clean f* deviation %.2e, all finite %s"
          % (tag, G, chunks, len(succ), worst, bool(np.all(np.isfinite(out["f"][succ])))))
    return len(succ)


@pytest.mark.parametrize("ny", [1, 3])
def test_stride_batch(gp, oracle, route, monkeypatch, ny):
    """4200 patches, a third poisoned, through the host-pointer grid entry: the pipeline's four chunks and one chunk; the one-wave
    route also in launches of 5 and 7 factor slots"""
    capi, ctx = gp
    failures = []
    want = WANT_STRIDE[route][0 if ny == 1 else 1]
    G = STRIDE_OF.get(want)
    n_pairs = 0
    for chunks in (NF.STRIDE_CHUNKS, 1):
        if chunks == 1:
            monkeypatch.setenv("GPC_HOST_NO_PIPELINE", "1")
        tag = "%s stride-%d grid chunks=%d" % (route, ny, chunks)
        n_pairs = max(n_pairs, _stride_run(capi, ctx, oracle, tag, ny, "grid", want, G, chunks, failures))
    monkeypatch.delenv("GPC_HOST_NO_PIPELINE")
    if G:
        assert n_pairs >= NF.MIN_PAIRS
    if route == "dispatch" and ny == 1:
        for slots in NF.W1_SLOTS:                       # (after the route fixture, which clears every switch)
            monkeypatch.setenv("GPC_W1_SLOTS", str(slots))
            k = _stride_run(capi, ctx, oracle, "%s stride-%d grid slots=%d" % (route, ny, slots), ny, "grid", want, slots, NF.STRIDE_CHUNKS, failures)
            assert k >= NF.MIN_PAIRS
        monkeypatch.delenv("GPC_W1_SLOTS")
    assert not failures, failures


def test_stride_batch_with_variance_and_with_poisoned_lds(gp, oracle, monkeypatch):
    """The stride batch once through the point-wise entry with the variance (three channels: the register kernel's factor export and
    dense_variance_kernel), and once with NaN in every LDS word of every CU before the kernels run (GPC_POISON_LDS, one-wave kernel)"""
    capi, ctx = gp
    for e_ in SWITCHES:
        monkeypatch.delenv(e_, raising=False)
    for k, v in ROUTES["dispatch"].items():
        monkeypatch.setenv(k, v)
    failures = []
    _stride_run(capi, ctx, oracle, "dispatch stride-3 ptsv", 3, "ptsv", "dense_mfma_nt4 + dense_variance", None, NF.STRIDE_CHUNKS, failures)
    monkeypatch.setenv("GPC_POISON_LDS", "1")
    _stride_run(capi, ctx, oracle, "dispatch stride-1 grid poisoned LDS", 1, "grid", "dense_mfma_w1", None, NF.STRIDE_CHUNKS, failures)
    monkeypatch.delenv("GPC_POISON_LDS")
    assert not failures, failures
