"""The table of the poison runs (test_poison_gpu.py), shared with test_poison_cpu.py, which holds it complete against include/gpc.h.

A kernel that reads an LDS word or a workspace element the call in hand never wrote gives an answer that depends on what ran before it
on that CU and in that context.  With GPC_POISON_LDS=1 every entry first fills the LDS of every CU with the NaN 0x7ff8dead0000beef and the
context's workspace with 0xFF (gpc_debug_poison_lds), and a workspace that grows comes filled with 0xFF instead of zeros (gpc_ws_reserve):
such a read then shows in the output as a NaN or a -1.  Every record below is one small pinned case of one kernel family; the GPU test
runs it plain, poisoned on the used context, poisoned on a context created under the switch, and plain again, and compares the four.

A record:
    id        the test's parameter id
    entries   the C-ABI entries of include/gpc.h it exercises.  A host-pointer twin of the sparse, cutter, map, ray-cast, render, decode,
              reproject, distortion and rate entries stages its arguments in buffers of its own and calls its _dev form, which makes the
              poison call: such a case names the _dev entry.  The dense host entries have a pipeline of their own and are named as such.
    env       the switches (DESIGN.md, section Switches) that select the kernel shape; everything in SWITCHES that a case does not set is
              unset while it runs
    run       run(capi, ctx, check=False, oracle=None) -> {name: ndarray}.  Builds its inputs from the case modules that pin the family,
              creates every object it needs on ctx and closes it again, and asserts the launched shape where the library reports it
              (Context.last_dense_kernel).  With check=True it also holds its outputs to the family's exact reference, by the family's own
              assertion (`oracle`: tests/oracle_lib.py).
    rule      "bits": tobytes() equality of every output, NaN payloads included -- every family the project asserts repeatable bit for
              bit.  "RUN_TOL": test_dense_ev_gpu.RUN_TOL (1e-12 of max|plain|, the two-call figure of test_dense_golden) on the floating
              outputs, the set of non-finite positions and every integer output exactly.  Only the register kernel (dense_mfma_nt*) has
              it: its backward solve adds into alpha with LDS atomics in arrival order.  The one-wave kernel has no LDS atomics at all;
              the tiled kernel's atomics are patch tickets, a workgroup-scope step counter and atomicMax on bit patterns, none of which
              orders a sum; the generic kernel has none (include/gpc.h states the same contract for the evidence).
    note      which kernel and why this shape

Sparse states are compared as the bit-identity tests of test_sparse_gpu.py compare them: basis counts, status, decision bytes, and alpha,
C, Q, BV within each patch's basis.  The rows beyond it are no output: gpc_sparse_create does not clear the state buffers, so they hold
what the allocation happened to hold and what the deletions left, and every run here trains objects of its own (test_prune_gpu._bits
compares the padding of copies of ONE object; two objects agree within their bases only).  The same holds for the states that the
prune, remap and dequantize cases read back."""
import collections

import numpy as np

Case = collections.namedtuple("Case", "id entries env run rule note")

POISON = "GPC_POISON_LDS"
# every switch that chooses a kernel or a shape of a family below: unset unless the case sets it
SWITCHES = ("GPC_FORCE_GENERIC", "GPC_FORCE_BIG", "GPC_BIG_NO_W2", "GPC_BIG_NO_W4", "GPC_NO_W1", "GPC_NO_W1_512", "GPC_W2", "GPC_W1_MIN_P",
            "GPC_W1_SLOTS", "GPC_VAR_W4", "GPC_NO_SPLIT", "GPC_NO_NT17", "GPC_NO_HINT", "GPC_HOST_NO_PIPELINE", "GPC_HOST_ONE_STREAM",
            "GPC_SPARSE_FULL", "GPC_SPARSE_NO_FUSE", "GPC_SPARSE_NO_LIST", "GPC_SPARSE_NO_MID", "GPC_SPARSE_NO_RES", "GPC_SPARSE_NO_ROWS",
            "GPC_SPARSE_NO_ROWS2", "GPC_SPARSE_NO_SMALL", "GPC_SPARSE_NO_SMALL_PREDICT", "GPC_SPARSE_RES", "GPC_SPARSE_TRI_MIN",
            "GPC_SPARSE_WIDE", "GPC_ALLOC_BLOCKS", POISON)

CASES = []


# ---- helpers ------------------------------------------------------------------------------------------------------------------------------

def _t(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _dev_batch(batch):
    off, x0, x1, y = batch
    y = np.atleast_2d(y)
    return dict(off=_t(np.asarray(off, dtype=np.int32)), x0=_t(x0), x1=_t(x1), y=_t(y), P=len(off) - 1, n_max=int(np.max(np.diff(off))),
                n_total=int(off[-1]), ny=y.shape[0])


def _dense_dev(ctx, prm, d, xs=None, res=0.0, sz=0, want_v=False):
    """gpc_dense_fit_predict_dev (xs given) or gpc_dense_fit_predict_grid_dev into sentinel-filled device buffers: f, [v,] alpha, status"""
    import torch
    m = len(xs[0]) if xs is not None else sz * sz
    nan = lambda *s: torch.full(s, float("nan"), dtype=torch.float64, device="cuda")
    f, al = nan(d["P"], d["ny"], m), nan(d["ny"], d["n_total"])
    v = nan(d["P"], m) if want_v else None
    st = torch.full((d["P"],), -7, dtype=torch.int32, device="cuda")
    head = (prm, d["P"], d["off"], d["n_max"], d["n_total"], d["x0"], d["x1"], d["y"], d["ny"])
    if xs is not None:
        xs0, xs1 = _t(xs[0]), _t(xs[1])
        torch.cuda.synchronize()
        ctx.dense_fit_predict_dev(*head, m, xs0, xs1, f, v, al, st)
    else:
        assert not want_v
        torch.cuda.synchronize()
        ctx.dense_fit_predict_grid_dev(*head, res, sz, f, al, st)
    ctx.synchronize()
    out = dict(f=f.cpu().numpy(), alpha=al.cpu().numpy(), status=st.cpu().numpy())
    if want_v:
        out["v"] = v.cpu().numpy()
    return out


def _name(ctx):
    """last_dense_kernel() as an output: the four runs must have launched the same thing"""
    return np.frombuffer(ctx.last_dense_kernel().encode(), dtype=np.uint8).copy()


def _put(out, prefix, d):
    for k, v in d.items():
        out[prefix + "." + k] = v


def _sparse_within_basis(g):
    """sizes and the state of a Sparse with everything beyond each patch's basis zeroed (module docstring)"""
    b = g.sizes()
    alpha, C_, Q, BV = (a.copy() for a in g.state())
    for i, nb in enumerate(b):
        alpha[i][:, nb:] = 0.0
        C_[i][nb:, :] = 0.0
        C_[i][:, nb:] = 0.0
        Q[i][nb:, :] = 0.0
        Q[i][:, nb:] = 0.0
        BV[i][nb:] = 0.0
    return dict(b=b, alpha=alpha, C=C_, Q=Q, BV=BV)


def _records(cloud):
    return np.ascontiguousarray(cloud).view(np.uint8).copy()


# ---- dense mean: every route of test_dense_accuracy_gpu.ROUTES on the edge batch of every size class ---------------------------------------------

def _dense_mean(route, family, ny):
    import dense_accuracy_cases as DA
    import test_dense_accuracy_gpu as TA
    want = TA.WANT[route][TA.SIZE_CLASS[family]][0 if ny == 1 else 1]
    host = (route, family, ny) == ("dispatch", "n256", 1)          # the host twins once

    def run(capi, ctx, check=False, oracle=None):
        batch, regime, dbl = DA.case_inputs(("edge", family, "default", 1, ny))
        p = capi.default_params_dense(sigmaf_sq=regime[0], l_sq=regime[1], noise=regime[2], ref_double_noise=dbl)
        d = _dev_batch(batch)
        out = {}
        _put(out, "grid", _dense_dev(ctx, p, d, res=DA.RES, sz=DA.SZ))
        assert ctx.last_dense_kernel() == want, (ctx.last_dense_kernel(), want)
        _put(out, "pts", _dense_dev(ctx, p, d, xs=DA.xstars()[1]))
        assert ctx.last_dense_kernel() == want, (ctx.last_dense_kernel(), want)
        assert np.all(out["grid.status"] == 0) and np.all(out["pts.status"] == 0)
        if host:
            f, st, al = ctx.dense_fit_predict_grid(p, *batch, DA.RES, DA.SZ, want_alpha=True)
            _put(out, "host_grid", dict(f=f, status=st, alpha=al))
            f, _, st, al = ctx.dense_fit_predict(p, *batch, *DA.xstars()[1], want_alpha=True)
            _put(out, "host_pts", dict(f=f, status=st, alpha=al))
        return out
    return run, want


def _add_dense_mean():
    import test_dense_accuracy_gpu as TA
    for route, env in TA.ROUTES.items():
        for family in TA.DA.FAMILIES:
            for ny in (1, 3):
                run, want = _dense_mean(route, family, ny)
                entries = ["gpc_dense_fit_predict_dev", "gpc_dense_fit_predict_grid_dev"]
                if (route, family, ny) == ("dispatch", "n256", 1):
                    entries += ["gpc_dense_fit_predict", "gpc_dense_fit_predict_grid"]
                rule = "RUN_TOL" if "_nt" in want else "bits"
                CASES.append(Case("dense-mean-%s-%s-ny%d" % (route, family, ny), tuple(entries), env, run, rule,
                                  want + (": the register kernel's alpha meets in arrival order (LDS atomics)" if rule == "RUN_TOL"
                                          else ": no atomics that order a sum")))


_add_dense_mean()


# ---- dense variance ---------------------------------------------------------------------------------------------------------------------------------

def _dense_variance(sizes, seed, xseed, want, host):
    def run(capi, ctx, check=False, oracle=None):
        import variance_cases as VC
        batch = VC._mixed_batch(list(sizes), seed=seed)
        xs = VC.xstar(17, seed=xseed)
        pv = capi.default_params_dense(sigmaf_sq=VC.DEFAULT[0], l_sq=VC.DEFAULT[1], noise=VC.DEFAULT[2], want_variance=1)
        out = {}
        _put(out, "dev", _dense_dev(ctx, pv, _dev_batch(batch), xs=xs, want_v=True))
        assert ctx.last_dense_kernel() == want, (ctx.last_dense_kernel(), want)
        assert np.all(out["dev.status"] == 0)
        if host:
            f, v, st, al = ctx.dense_fit_predict(pv, *batch, *xs, want_alpha=True)
            _put(out, "host", dict(f=f, v=v, status=st, alpha=al))
        return out
    return run


for _w4 in ("0", "1"):
    # (the batches and X* seeds of test_variance_big_xstar_counts and test_variance_small_xstar_counts at m = 17: a partial block of 16)
    CASES.append(Case("dense-variance-big-w4_%s" % _w4, ("gpc_dense_fit_predict_dev",), {"GPC_VAR_W4": _w4},
                      _dense_variance([300, 520, 0, 270], 44, 117, "dense_mfma_big + dense_variance_big", False), "bits",
                      "tiled fit with the factor export, dense_variance_big; m = 17 is one block and one column"))
    CASES.append(Case("dense-variance-small-w4_%s" % _w4, ("gpc_dense_fit_predict_dev", "gpc_dense_fit_predict"),
                      {"GPC_VAR_W4": _w4, "GPC_W1_MIN_P": "2"},
                      _dense_variance([40, 100, 180, 0, 250, 7], 45, 217, "dense_mfma_w1 + dense_variance", _w4 == "0"), "bits",
                      "one-wave fit with the factor export, dense_variance_kernel<16> on a ragged batch of at most 256 points"))


# ---- dense evidence and selection --------------------------------------------------------------------------------------------------------------------

def _dense_ev(route, sizes):
    want = {"one-wave": "dense_mfma_w1 + dense_variance", "tiled": "dense_mfma_big + dense_variance_big",
            "register": "dense_mfma_nt12 + dense_variance"}[route]

    def run(capi, ctx, check=False, oracle=None):
        import torch
        import dense_ev_cases as DC
        import variance_cases as VC
        batch = VC._mixed_batch(list(sizes), seed=78)                       # test_ev_bit_contracts
        xs = VC.xstar(19, seed=98)
        d = _dev_batch(batch)
        d.update(xs0=_t(xs[0]), xs1=_t(xs[1]))
        p0 = capi.default_params_dense(sigmaf_sq=VC.DEFAULT[0], l_sq=VC.DEFAULT[1], noise=VC.DEFAULT[2], want_variance=0)
        nan = lambda *s: torch.full(s, float("nan"), dtype=torch.float64, device="cuda")
        P, N, m = d["P"], d["n_total"], 19
        o = dict(f=nan(P, 1, m), v=nan(P, m), alpha=nan(1, N), status=torch.full((P,), -7, dtype=torch.int32, device="cuda"), log_ev=nan(P, 1))
        torch.cuda.synchronize()
        ctx.dense_fit_predict_ev_dev(p0, P, d["off"], d["n_max"], N, d["x0"], d["x1"], d["y"], 1, m, d["xs0"], d["xs1"], 0.0, 0, o["f"],
                                     o["v"], o["alpha"], o["status"], o["log_ev"])
        ctx.synchronize()
        assert ctx.last_dense_kernel() == want, (ctx.last_dense_kernel(), want)
        out = {}
        _put(out, "ev", {k: t.cpu().numpy() for k, t in o.items()})
        assert np.all(out["ev.status"] == 0) and np.all(np.isfinite(out["ev.log_ev"]))
        # the selection among dense_ev_cases.CANDIDATES on the same batch, grid form (test_select_dev_is_the_host_form)
        res, sz, H = 0.15, 5, len(DC.CANDIDATES)
        ms = sz * sz
        s = dict(f_star=nan(P, 1, ms), v_star=nan(P, ms), alpha=nan(1, N), log_ev=nan(P, 1),
                 best=torch.full((P,), -7, dtype=torch.int32, device="cuda"), log_ev_all=nan(H, P, 1),
                 status=torch.full((P,), -7, dtype=torch.int32, device="cuda"))
        prm = capi.default_params_dense(sigmaf_sq=9.0, l_sq=9.0, noise=9.0)
        torch.cuda.synchronize()
        ctx.dense_select_dev(prm, list(DC.CANDIDATES), P, d["off"], d["n_max"], N, d["x0"], d["x1"], d["y"], 1, 0, None, None, res, sz,
                             f_star=s["f_star"], v_star=s["v_star"], alpha_out=s["alpha"], log_ev=s["log_ev"], best=s["best"],
                             log_ev_all=s["log_ev_all"], status=s["status"])
        ctx.synchronize()
        out["select.kernel"] = _name(ctx)
        _put(out, "select", {k: t.cpu().numpy() for k, t in s.items()})
        return out
    return run


for _route, _sizes in (("one-wave", (200, 0, 230, 64)), ("tiled", (300, 0, 270)), ("register", (100, 0, 180, 64))):
    CASES.append(Case("dense-evidence-" + _route, ("gpc_dense_fit_predict_ev_dev", "gpc_dense_select_dev"),
                      {"GPC_W1_MIN_P": "1"} if _route == "one-wave" else {}, _dense_ev(_route, _sizes),
                      "RUN_TOL" if _route == "register" else "bits",
                      "fit with the factor export, variance, dense_gauss_evidence and the keep-best kernel of the selection; "
                      + ("register kernel: alpha, f* and log_ev repeat to RUN_TOL (include/gpc.h)" if _route == "register" else "no atomics")))


# ---- host-pointer dense pipeline ---------------------------------------------------------------------------------------------------------------------

def _dense_host(capi, ctx, check=False, oracle=None):
    """2100 patches of at most 32 points through gpc_dense_fit_predict_grid: more than 2048 patches are cut into chunks, and a chunk's
    poison call covers the launch's own region of the workspace only"""
    from gp_compressor_amd import synth
    off, x0, x1, y = synth.make_patches(2100, 32, res=0.15, seed=91, ragged=True)
    f, st, al = ctx.dense_fit_predict_grid(capi.default_params_dense(), off, x0, x1, y, 0.15, 10, want_alpha=True)
    assert np.all(st == 0)
    return dict(f=f, status=st, alpha=al, kernel=_name(ctx))


for _id, _env in (("default", {}), ("one-stream", {"GPC_HOST_ONE_STREAM": "1"})):
    CASES.append(Case("dense-host-pipeline-" + _id, ("gpc_dense_fit_predict_grid",), _env, _dense_host, "RUN_TOL",
                      "the chunked host entry; patches of at most 32 points go to the register kernel (LDS atomics: RUN_TOL)"))


# ---- sparse add: one case per kernel shape ------------------------------------------------------------------------------------------------------------

def _sparse_add(ny, cap, kernel, P, n):
    def run(capi, ctx, check=False, oracle=None):
        from gp_compressor_amd import synth
        res = 0.15
        # the batch of test_sparse_rows_phase_is_bit_identical: ragged, one empty patch, a patch count that is no multiple of 4
        off, x0, x1, y = synth.make_patches(P, n, res=res, seed=23 + cap + P, ragged=True, ny=ny, n_min=1)
        cnt = np.diff(off)
        keep = np.ones(off[-1], bool)
        keep[off[5]:off[6]] = False
        cnt[5] = 0
        off = np.concatenate([[0], np.cumsum(cnt)]).astype(np.int32)
        x0, x1, y = x0[keep], x1[keep], np.ascontiguousarray(y[:, keep])
        perm = synth.sattolo_perms(off, seed=9)
        kw = dict(capacity=cap)
        if kernel == "fill":
            kw.update(sigmaf_sq=1.0, l_sq=(res / 8) ** 2, noise=1e-4 if ny == 1 else 1.0)
        if kernel == "geo":
            kw.update(sigmaf_sq=1.0, l_sq=(res * 2) ** 2, noise=1e-6, eps_tol=1e-14)
        if kernel == "mixed":
            kw.update(sigmaf_sq=1.0, l_sq=(res / 3) ** 2, noise=1e-3 if ny == 1 else 1.0, eps_tol=1e-3)
        g = capi.Sparse(ctx, capi.default_params_sparse(ny, **kw), P, ny)
        try:
            st1, tr1 = g.add(off, x0, x1, y, perm, trace=True)
            st2, tr2 = g.add(off, x0, x1, y, trace=True)          # online growth: the second call starts from trained states
            out = dict(st1=st1, st2=st2, tr1=tr1, tr2=tr2, **_sparse_within_basis(g))
        finally:
            g.close()
        assert out["b"][5] == 0 and st1[5] == 0
        if kernel == "default":
            assert out["b"].max() <= 40                           # the regime the rows phase exists for
        if cap > 0:
            assert out["b"].max() <= cap
        return out
    return run


# shape -> (ny, capacity, regime, P, n): parameter rows of the *_is_bit_identical tests of test_sparse_gpu.py.  What each switch selects:
# csrc/sparse.hip, sp_add_launch and sp_workgroup_threads.
_ADD = [
    ("default-cap12", {}, (1, 12, "default", 37, 150), "rows phase (four patches per wave) and its work list, one wave per patch behind it"),
    ("default-cap100", {}, (1, 100, "fill", 21, 90), "two waves per patch, triangular passes, mid phase"),
    ("default-cap200-mixed", {}, (1, 200, "mixed", 50, 180), "four waves per patch, triangular passes, sparse and full updates alternate"),
    ("default-cap-1", {}, (1, -1, "mixed", 9, 60), "the exact GP: ld = 256"),
    ("no_small-cap50-ny3", {"GPC_SPARSE_NO_SMALL": "1"}, (3, 50, "fill", 33, 120), "the regular kernel alone, one wave per patch, three planes"),
    ("wide-cap33-geo", {"GPC_SPARSE_WIDE": "1"}, (1, 33, "geo", 29, 180), "four waves per patch at a small capacity, geometric deletions"),
    ("res-cap100", {"GPC_SPARSE_RES": "1"}, (1, 100, "fill", 21, 90), "64 < capacity <= 120: C and Q of the patch in flight packed in LDS"),
    ("full-cap100", {"GPC_SPARSE_FULL": "1"}, (1, 100, "fill", 21, 90), "full passes over C and Q instead of triangular ones"),
    ("no_fuse-cap100", {"GPC_SPARSE_NO_FUSE": "1"}, (1, 100, "fill", 21, 90), "the next point's mat-vecs as a pass of their own"),
    ("no_list-cap12", {"GPC_SPARSE_NO_LIST": "1"}, (1, 12, "default", 37, 150), "static shares instead of the work lists"),
    ("no_rows-cap12", {"GPC_SPARSE_NO_ROWS": "1"}, (1, 12, "default", 37, 150), "the one-wave small-basis kernel from the first point"),
    ("no_rows2-cap40-ny3", {"GPC_SPARSE_NO_ROWS2": "1"}, (3, 40, "mixed", 33, 120), "the one-wave kernel instead of the second rows phase"),
    ("no_mid-cap200-mixed", {"GPC_SPARSE_NO_MID": "1"}, (1, 200, "mixed", 50, 180), "bases of 25 .. 48 vectors straight to the regular kernel"),
]
for _id, _env, _args, _note in _ADD:
    CASES.append(Case("sparse-add-" + _id, ("gpc_sparse_add_dev",), _env, _sparse_add(*_args), "bits", _note))


# ---- sparse read-outs ------------------------------------------------------------------------------------------------------------------------------

def _sparse_readout(case):
    def run(capi, ctx, check=False, oracle=None):
        import readout_cases as RC
        import render_attrs_cases as AC
        import test_sparse_readout_gpu as TR
        B = RC.batch(*case)
        ny = B["ny"]
        g = TR._load(capi, ctx, B)
        try:
            off, q0, q1, yq = B["off"], B["q0"], B["q1"], B["yq"]
            out = {}
            f, s, st = g.predict_points(off, q0, q1, want_sigma=True)
            _put(out, "points", dict(f=f, sigma=s, status=st))
            f, c, st = g.predict_points(off, q0, q1, want_sigma=True, conf=True)
            _put(out, "points_conf", dict(f=f, conf=c, status=st))
            rng = np.random.default_rng(500 + 33)                      # test_readout_predict_grid at m = 33: a chunk of 32 and one more
            xs0, xs1 = rng.uniform(-RC.RES / 2, RC.RES / 2, 33), rng.uniform(-RC.RES / 2, RC.RES / 2, 33)
            f, s, st = g.predict(xs0, xs1)
            _put(out, "grid", dict(f=f, sigma=s, status=st))
            dX, l = g.likelihood(off, q0, q1, yq)
            _put(out, "likelihood", dict(dX=dX, l=l))
            patch, p0, p1 = AC.scatter_pattern("sprinkled", B, 257, seed=1257)      # test_scattered_predict_every_count_and_pattern
            f, s, st = g.predict_scattered(patch, p0, p1)
            _put(out, "scattered", dict(f=f, sigma=s, status=st))
            if ny == 1:                                                # (last: it moves the object's sigma_f)
                sf, iters, ls, delta = g.train_sigmaf(off, q0, q1, yq[0], step=RC.TRAIN_STEP, max_counter=RC.TRAIN_MAXC)
                _put(out, "train", dict(p0=sf, iters=iters, ls=ls, delta=delta))
        finally:
            g.close()
        return out
    return run


def _add_readouts():
    import readout_cases as RC
    small, large, field = RC.CASES[0], RC.CASES[4], RC.CASES[5]
    assert small[0] == 15 and large[:2] == (-1, 1) and field[:2] == (-1, 3)
    entries = ("gpc_sparse_predict_dev", "gpc_sparse_predict_points_dev", "gpc_sparse_predict_scattered_dev", "gpc_sparse_likelihood_dev")
    train = ("gpc_sparse_train_sigmaf_dev",)
    for cid, case, env, ent in (("cap15", small, {}, entries + train), ("cap-1", large, {}, entries + train), ("cap-1-ny3", field, {}, entries),
                                ("cap15-regular", small, {"GPC_SPARSE_NO_SMALL_PREDICT": "1"}, entries + train),
                                ("cap-1-regular", large, {"GPC_SPARSE_NO_SMALL_PREDICT": "1"}, entries + train)):
        CASES.append(Case("sparse-readout-" + cid, ent, env, _sparse_readout(case), "bits",
                          "readout_cases: every basis size of the object, an empty patch with and one without points"))


_add_readouts()


# ---- rate control: prune, prune to a bound, dequantize ----------------------------------------------------------------------------------------------------

def _rate_control(ny):
    def run(capi, ctx, check=False, oracle=None):
        import prune_ref as pr
        cap, div, n, P, _, keep = [c for c in pr.case_ids() if c[4] == ny][0]
        assert (cap, keep) == (16, 5)                                 # the smallest regime: 64 threads per patch (256 under GPC_SPARSE_WIDE)
        off, x0, x1, y, perm = pr.batch(cap, n, P, ny)
        prm = capi.default_params_sparse(ny, ref_field_delete_bug=0, **pr.kernel_kw(cap, div, ny))      # (test_prune_gpu._params)
        g = capi.Sparse(ctx, prm, P, ny)
        made = [g]
        try:
            assert np.all(g.add(off, x0, x1, y, perm) == 0)
            ident = np.arange(P, dtype=np.int32)
            out = {}
            a = g.remap(P, ident)
            made.append(a)
            rm, order, scores = a.prune(keep=keep, want_trace=True)
            _put(out, "prune", dict(removed=rm, order=order, scores=scores, **_sparse_within_basis(a)))
            assert np.all(a.sizes() == keep)
            b = g.remap(P, ident)
            made.append(b)
            rm, mse0, nxt, order, scores, mse = b.prune_rd(off, x0, x1, y, keep=2, want_trace=True)
            _put(out, "prune_rd", dict(removed=rm, mse0=mse0, next=nxt, order=order, scores=scores, mse=mse, **_sparse_within_basis(b)))
            bits, qa, qb, rng, _, _ = g.quantize_rd(off, x0, x1, y, bits_min=6)
            assert np.all(bits == 6)                                   # (max_mse = +inf: bits_min, test_quantize_rd_curve_and_shapes)
            c = capi.Sparse(ctx, prm, P, ny)
            made.append(c)
            c.dequantize(g.sizes(), bits, qa, qb, rng)
            _put(out, "dequantize", _sparse_within_basis(c))
        finally:
            for o in made:
                o.close()
        return out
    return run


for _ny in (1, 3):
    for _id, _env in (("default", {}), ("wide", {"GPC_SPARSE_WIDE": "1"})):
        CASES.append(Case("rate-control-ny%d-%s" % (_ny, _id), ("gpc_sparse_prune_dev", "gpc_sparse_prune_rd_dev", "gpc_sparse_dequantize_dev",
                                                              "gpc_sparse_remap"), _env, _rate_control(_ny), "bits",
                          "capacity 16: one wave per patch, four under GPC_SPARSE_WIDE; copies by the identity remap"))


# ---- rate allocation ---------------------------------------------------------------------------------------------------------------------------------

def _rate_allocate(capi, ctx, check=False, oracle=None):
    import rate_alloc_ref as RA
    import test_rate_alloc_gpu as TA
    pb = TA._problem(257, 9, seed=31)                                  # one row past a scan tile of 256, a row past a sweep's group of 4
    count = (pb.kmax + 1).astype(np.int32)
    need = TA._some_needs(pb)[1]
    k, tg, res = TA._dev(capi, ctx, pb, need, 1, count)
    if check:
        TA._equal((k, tg, res), RA.allocate(pb, need, 1, count), "poison case")
    out = dict(k=k, target=tg)
    for f in ("lambda_bits", "saved", "max_saving", "feasible", "switched_rows"):
        out[f] = np.asarray(res[f])
    return out


for _id, _env in (("default", {}), ("two-blocks", {"GPC_ALLOC_BLOCKS": "2"})):
    CASES.append(Case("rate-allocate-" + _id, ("gpc_rate_allocate_dev",), _env, _rate_allocate, "bits",
                      "257 rows: the sweeps' and the scan's partial last group; two workgroups: the grid-stride wrap and a scan over two tiles"))


# ---- the cloud cutter ----------------------------------------------------------------------------------------------------------------------------------

def _cutter(which):
    def run(capi, ctx, check=False, oracle=None):
        from gp_compressor_amd import synth
        import test_producer_gpu as TP
        if which == "lattice":          # test_producer_matches_oracle_bit_for_bit, "lattice": points on the voxel faces, exact duplicates
            g = np.arange(0, 9) * 0.125
            xyz = np.stack(np.meshgrid(g, g, g[:3], indexing="ij"), -1).reshape(-1, 3)
            xyz = np.concatenate([xyz, xyz, xyz + np.array([0.0625, 0.0, 0.0])]).astype(np.float32)
            rgb = (np.arange(3 * len(xyz)).reshape(-1, 3) * 5 % 256).astype(np.uint8)
            res, sz = 0.125, 4
        else:
            xyz, rgb = synth.plane_cloud(3000, seed=2, extent=0.6)
            res, sz = 0.15, 10
        pt = ctx.project_cloud(ctx.make_cloud(xyz, rgb), res, sz)
        try:
            got = pt.fetch()
            v = pt.view
            out = dict(got, view=np.array([v.P, v.n_total, v.n_max, v.m], dtype=np.int64))
        finally:
            pt.close()
        if check:
            TP._same(got, oracle.project_cloud(xyz, rgb, res, sz))
        return out
    return run


for _which in ("lattice", "plane"):
    CASES.append(Case("cutter-" + _which, ("gpc_project_cloud_dev",), {}, _cutter(_which), "bits",
                      "voxel table, leaf walk, moments, frames, ownership, emit: scratch carved from the workspace"))


# ---- map insertion and remap -----------------------------------------------------------------------------------------------------------------------------

def _map_overlap(capi, ctx, check=False, oracle=None):
    import mapping_cases as mc
    import mapping_ref as mr
    import test_mapping_gpu as TM
    m = TM.Model(capi, ctx, untrained=(0, 6))                           # the 3 x 3 model, two leaves without a GP
    made = []
    try:
        S, cs = mc.overlapping_scan()
        new, o2n = m.pt.insert_cloud(ctx.make_cloud(S, cs), min_nbr=20, depth=m.gd)
        made.append(new)
        g = new.fetch()
        gd, gc = m.gd.remap(new.view.P, o2n), m.gc.remap(new.view.P, o2n)
        made += [gd, gc]
        out = dict(g, o2n=o2n)
        _put(out, "depth", _sparse_within_basis(gd))
        _put(out, "colour", _sparse_within_basis(gc))
        if check:
            want = mr.insert(m.b, m.grid, m.trained, S, cs, 20, frames=g["R"])
            assert np.array_equal(g["off"], want["off"]) and np.array_equal(g["src"], want["src"]) and np.array_equal(o2n, want["old_to_new"])
            assert np.array_equal(gd.sizes()[o2n], m.gd.sizes())
    finally:
        for o in made:
            o.close()
        m.close()
    return out


def _map_chunk_edges(capi, ctx, check=False, oracle=None):
    import mapping_cases as mc
    import mapping_scale_cases as ms
    A, ca = mc.model_cloud()
    S, cs = ms.chunk_edge_scan()
    pt = ctx.project_cloud(ctx.make_cloud(A, ca), mc.RES, mc.SZ)
    new = None
    try:
        new, o2n = pt.insert_cloud(ctx.make_cloud(S, cs), min_nbr=1)
        out = dict(new.fetch(), o2n=o2n)
    finally:
        if new is not None:
            new.close()
        pt.close()
    return out


CASES.append(Case("map-overlap", ("gpc_patches_insert_cloud_dev", "gpc_sparse_remap"), {}, _map_overlap, "bits",
                  "old leaves extended, fresh leaves, untrained leaves re-cut; the GP states follow through gpc_sparse_remap"))
CASES.append(Case("map-chunk-edges", ("gpc_patches_insert_cloud_dev",), {}, _map_chunk_edges, "bits",
                  "fresh leaves of 1 .. 257 points: the depth-mean chain at its chunk edges"))


# ---- registration -----------------------------------------------------------------------------------------------------------------------------------------

def _registration(capi, ctx, check=False, oracle=None):
    import torch
    from gp_compressor_amd import synth
    import test_registration_gpu as TG
    xyz, rgb = synth.plane_cloud(5000, seed=2)
    m = TG.Model(capi, ctx, xyz, rgb)
    reg = m.registration()
    try:
        scan = ctx.make_cloud(TG._perturbed(xyz), rgb)
        d_scan = torch.from_numpy(scan.view(np.uint8).reshape(-1, 32)).cuda()
        torch.cuda.synchronize()
        reg.set_cloud(d_scan, n=len(scan))
        step = reg.step(capi.default_params_registration(step=1e-7))
        owner, local = reg.assignment()
        R, t = reg.transform()
        out = dict(step=step, owner=owner, local=local, cloud=_records(reg.cloud()), R=R, t=t)
        assert np.all(np.isfinite(step)) and step[8] > 0.5 * len(xyz)
        # ... and the loop: gpc_registration_run from the same start, three steps
        reg.set_cloud(d_scan, n=len(scan))
        out["trace"] = reg.run(capi.default_params_registration(step=1e-7, tol=0.0, min_steps=2, max_steps=3))
        assert out["trace"].shape == (3, 9) and out["trace"][0].tobytes() == step.tobytes()
        out["run_cloud"] = _records(reg.cloud())
    finally:
        reg.close()
        m.close()
    return out


CASES.append(Case("registration", ("gpc_registration_set_cloud_dev", "gpc_registration_step", "gpc_registration_run"), {}, _registration, "bits",
                  "assign, gather, reduce, update, transform: the 9 doubles of a step, owner, local, the moved cloud and the pose"))


# ---- ray casting --------------------------------------------------------------------------------------------------------------------------------------------

def _raycast(capi, ctx, check=False, oracle=None):
    import torch
    import mapping_ref as mr
    import raycast_cases as rcs
    import raycast_ref as rr
    import test_raycast_gpu as TC
    A, pt0, gd0, _ = TC._model(capi, ctx)                              # the scene fixture of test_raycast_gpu.py
    made = [gd0, pt0]
    try:
        S, cs = rcs.scan_cloud()
        scan = ctx.make_cloud(S, cs)
        new, o2n = pt0.insert_cloud(scan, min_nbr=TC.MIN_NBR, depth=gd0)
        made.insert(0, new)
        gd = gd0.remap(new.view.P, o2n)
        made.insert(0, gd)
        P = new.view.P
        d_scan = torch.from_numpy(scan.view(np.uint8).reshape(-1, 32)).cuda()
        d_cells = torch.zeros((P, TC.M), dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()
        counts = new.raycast(d_scan, rcs.SENSOR, d_cells, depth=gd, n=len(scan))
        ctx.synchronize()
        cells = d_cells.cpu().numpy()
        off, x0, x1, y, n_total, n_max = new.occupancy_batch(d_cells)
        ctx.synchronize()
        out = dict(counts=counts, cells=cells, off=off.cpu().numpy(), x0=x0.cpu().numpy(), x1=x1.cpu().numpy(), y=y.cpu().numpy(),
                   sizes=np.array([n_total, n_max], dtype=np.int64))
        if check:
            g = new.fetch()
            want = mr.insert(pt0.fetch(), mr.model_grid(A, TC.RES, TC.SZ), gd0.sizes() > 0, S, cs, TC.MIN_NBR, frames=g["R"])
            ref = rr.cast(g, want["grid"], gd.sizes() > 0, S, rcs.SENSOR)
            want_cells = rr.cells_maxkey(ref["events"], np.zeros((P, TC.M), np.uint8))
            assert np.array_equal(counts, ref["counts"]) and np.array_equal(cells, want_cells)
            off_w, x0_w, x1_w, y_w = rr.occupancy_batch(want_cells, TC.RES, TC.SZ)
            assert n_total == int(off_w[-1]) and n_max == int(np.diff(off_w).max()) and np.array_equal(out["off"], off_w)
            assert out["x0"].tobytes() == x0_w.tobytes() and out["x1"].tobytes() == x1_w.tobytes() and out["y"].tobytes() == y_w.tobytes()
    finally:
        for o in made:
            o.close()
    return out


CASES.append(Case("raycast", ("gpc_patches_raycast_dev", "gpc_occupancy_batch_dev"), {}, _raycast, "bits",
                  "314 rays into 22 leaves, one of them untrained; the labelled cells as the probit GP's batch"))


# ---- rendering and its attributes ---------------------------------------------------------------------------------------------------------------------------

def _render(pose):
    def run(capi, ctx, check=False, oracle=None):
        import mapping_ref as mr
        import raycast_cases as rcs
        import render_cases as rc
        import test_render_gpu as TN
        A, ca = rcs.model_cloud()
        pt, gd, gc, pd, pc = TN._trained(capi, ctx, A, ca)
        try:
            g = pt.fetch()
            o, dirs = rc.scene_rays(pose, g["R"][4][:, 1])
            _, Rc, f = rc.POSES[pose]
            img = ctx.camera_rays(Rc, f, f, (rc.W_IMG - 1) / 2, (rc.H_IMG - 1) / 2, rc.W_IMG, rc.H_IMG).cpu().numpy()
            prm = capi.default_params_render(**TN.PRM)
            r = pt.render(o, dirs, gd, gc, None, prm, want=("leaf", "range", "local", "sigma", "normal"))
            out = dict(img=img, cloud=_records(r["cloud"]), **{k: r[k] for k in ("leaf", "range", "local", "sigma", "normal", "counts")})
            assert np.sum(r["leaf"] >= 0) > 50 and np.sum(r["leaf"] < 0) > 50
            if check:
                assert img.tobytes() == dirs[:rc.W_IMG * rc.H_IMG].tobytes()
                s = dict(pt=pt, gd=gd, gc=gc, pd=pd, pc=pc, g=g, grid=mr.model_grid(A, TN.RES, TN.SZ), P=pt.view.P)
                again, _ = TN._compare(capi, s, gd, gc, o, dirs)
                for k in ("leaf", "range", "local"):
                    assert again[k].tobytes() == r[k].tobytes(), k
        finally:
            for x in (gd, gc, pt):
                x.close()
        return out
    return run


CASES.append(Case("render-above", ("gpc_camera_rays_dev", "gpc_patches_render_dev", "gpc_patches_render_attrs_dev"), {}, _render("above"), "bits",
                  "the 23 x 17 image, the 1 x 1 image and the hand-made rays of render_cases from above: walk, surface solve, colours, "
                  "sigma and normal at the hits through the scattered sparse predict"))


# ---- masked decode ----------------------------------------------------------------------------------------------------------------------------------------------

def _decode(name, sz, rot):
    def run(capi, ctx, check=False, oracle=None):
        import decode_cases as DC
        import test_decode_gpu as TD
        Bd, Bc = DC.pair(name)
        gd = TD._load(capi, ctx, Bd)
        gc = None if Bc is None else TD._load(capi, ctx, Bc)
        try:
            b = Bd["b"]
            R, mu, cm = DC.frames(Bd["P"])
            W, cells = DC.masks(len(b), sz, "both", rot=rot)
            raw, leaf, point, count, n0, n1 = TD._decode_dev(ctx, gd, gc, sz, W, cells, R, mu, cm)
            assert n0 == n1 > 0
            if check:
                ref, row_of = TD._chain(ctx, gd, gc, b, sz, R, mu, cm)
                want, w_leaf, w_point, w_count, n = TD._expected(ref, row_of, b, sz, W, cells)
                assert n0 == n and np.array_equal(count, w_count) and np.array_equal(leaf[:n], w_leaf) and np.array_equal(point[:n], w_point)
                bad = DC.same_records(TD._records(raw, n), want)
                assert bad is None, bad
        finally:
            gd.close()
            if gc is not None:
                gc.close()
        return dict(cloud=raw, leaf=leaf, point=point, count=count, n=np.array([n0, n1], dtype=np.int64))
    return run


def _add_decode():
    import decode_cases as DC
    for sz in (8, 9):                                                  # m = 64: one block of points; 81: a block and a partial one
        rot = DC.SIZES.index(sz) + 3 * DC.MASK_KINDS.index("both")     # (test_bit_identity's rotation of the mask patterns)
        CASES.append(Case("decode-cap100-sz%d" % sz, ("gpc_sparse_decode_dev",), {}, _decode("cap100", sz, rot), "bits",
                          "count, scan over the leaves in the workspace, emit with the kept flags in LDS; depth and colour"))
    CASES.append(Case("decode-global-row", ("gpc_sparse_decode_dev",), {}, _decode("cap15-norgb", DC.SZ_GLOBAL_ROW, 4), "bits",
                      "sz = 129: m is past the LDS row of the emit kernel, the flags are read from global memory"))


_add_decode()


# ---- reproject -----------------------------------------------------------------------------------------------------------------------------------------------------

def _reproject(capi, ctx, check=False, oracle=None):
    import reproject_cases as RPC
    bv, (xs0, xs1, f, R, mu, cs, cm) = RPC.compaction_case(1025, "random")
    assert cs is not None and bv is not None
    cloud = ctx.reproject(xs0, xs1, f, R, mu, cs, cm, bv)
    assert len(cloud) == RPC.COMPACTION_M * len(RPC.trained(1025, bv)) > 0
    if check:
        RPC.assert_same_cloud(cloud, RPC.expected(oracle, xs0, xs1, f, R, mu, cs, cm, bv))
    return dict(cloud=_records(cloud), n=np.array([len(cloud)], dtype=np.int64))


CASES.append(Case("reproject", ("gpc_reproject_dev",), {}, _reproject, "bits",
                  "1025 patches: two per thread of the scan, whose offsets live in the workspace; colours and a random trained pattern"))


# ---- cloud distortion and the patch normals ---------------------------------------------------------------------------------------------------------------------------

_ALL = ("nn", "d2", "e2")


def _result_arrays(r):
    return {k: np.asarray(v) for k, v in r.items()}


def _distortion_lattice(cell):
    def run(capi, ctx, check=False, oracle=None):
        import distortion_cases as DS
        import distortion_ref as DR
        a, b, _ = DS.lattice()
        got = ctx.cloud_distortion(a, b, cell=cell, want=_ALL)
        if check:
            DR.assert_same(got, DR.distortion(a, b))
        return _result_arrays(got)
    return run


def _distortion_invalid(capi, ctx, check=False, oracle=None):
    import distortion_cases as DS
    import distortion_ref as DR
    a, b = DS.random_pair(700, 500, seed=11)                           # test_invalid_records
    ai, _ = DS.with_invalid(a, seed=12)
    bi, _ = DS.with_invalid(b, seed=13)
    nrm, _, _ = DS.unit_normals(len(bi), seed=16)
    got = ctx.cloud_distortion(ai, bi, nrm, want=_ALL)
    if check:
        DR.assert_same(got, DR.distortion(ai, bi, nrm))
    return _result_arrays(got)


def _patches_normals(capi, ctx, check=False, oracle=None):
    from gp_compressor_amd import synth
    import distortion_ref as DR
    xyz, rgb = synth.plane_cloud(3000, seed=2, extent=0.6)             # test_patches_normals, "plane"
    n = len(xyz)
    pt = ctx.project_cloud(ctx.make_cloud(xyz, rgb), 0.15, 10)
    try:
        got = pt.normals(n)
        longer = pt.normals(n + 5)                                     # a longer cloud: the tail is unowned
        if check:
            want = DR.patches_normals(pt.fetch(), n)
            assert DR.same_bits(got, want) and DR.same_bits(longer, np.concatenate([want, np.full((5, 3), np.nan, np.float32)]))
    finally:
        pt.close()
    return dict(normals=got, longer=longer)


for _cell in (0.0, 1.0):
    CASES.append(Case("distortion-lattice-cell%g" % _cell, ("gpc_cloud_distortion_dev",), {}, _distortion_lattice(_cell), "bits",
                      "ties at every distance; cell 0 is the library's choice of the search table, 1.0 the lattice's own spacing"))
CASES.append(Case("distortion-invalid-normals", ("gpc_cloud_distortion_dev",), {}, _distortion_invalid, "bits",
                  "700 against 500 records with non-finite ones on both sides, D2 along unit normals with NaN and zero rows"))
CASES.append(Case("patches-normals", ("gpc_patches_normals_dev",), {}, _patches_normals, "bits",
                  "the src check's flag is a workspace word; NaN fill, then the owning leaf's normal per point"))


# ---- entries without a case ----------------------------------------------------------------------------------------------------------------------------------------------

# entry -> (test file, test): already run under the poison by a test of their own
# (the eight probit entries share one call record and one launcher, csrc/dense_irls_api.hip, which makes the poison call: the Newton
# loop under test_irls_poisoned_lds, its variance, probability and evidence read-outs under test_ev_many_patches, whose entry is the
# one the selection runs once per candidate)
COVERED_ELSEWHERE = {
    "gpc_dense_irls_fit_predict_dev": ("test_irls_gpu.py", "test_irls_poisoned_lds"),
    "gpc_dense_irls_fit_predict_var_dev": ("test_irls_ev_gpu.py", "test_ev_many_patches"),
    "gpc_dense_irls_fit_predict_ev_dev": ("test_irls_ev_gpu.py", "test_ev_many_patches"),
    "gpc_dense_irls_select_dev": ("test_irls_ev_gpu.py", "test_ev_many_patches"),
    "gpc_sparse_quantize_rd_dev": ("test_quantize_gpu.py", "test_quantize_rd_curve_and_shapes"),
}

# entry -> why no poison run can tell anything about it (true of its code)
EXEMPT = {
    "gpc_patches_view_dev": "launches nothing: copies the view struct of the batch on the host",
    "gpc_registration_cloud_dev": "launches nothing: returns the address and the count of the working cloud",
    "gpc_allgather_fstar_dev": "ncclAllGather, then unpermute_rows_kernel: a gather through the comm's own table, no LDS, no workspace",
    "gpc_unpermute_fstar_dev": "unpermute_rows_kernel alone: a gather through the comm's own table, no LDS, no workspace",
    # (no _dev entry, listed because it launches: every other object call that launches makes the poison call -- gpc_sparse_remap,
    # gpc_registration_set_cloud[_dev], gpc_noise_eval)
    "gpc_registration_create": "rg_reset_kernel alone: writes the identity pose into the object's own state, no LDS, no workspace",
}


def entries_with_a_case():
    return {e for c in CASES for e in c.entries}
