"""The table of the stream-order runs (test_stream_order_gpu.py), shared with test_stream_order_cpu.py, which holds it against include/gpc.h.

include/gpc.h promises of every gpc_*_dev entry that its work is enqueued on the context's stream -- behind what the caller put there
before the call, ahead of what the caller puts there after it -- and that the call does not wait for the device unless its own comment
says so.  A test that hands the library finished buffers and synchronises before it looks holds none of that.  The runs here put the
call between a busy stream and a pair of copies: the inputs arrive on the stream just ahead of the call and are overwritten just behind
it, the outputs are copied away on the stream at once.  The poison records (poison_cases.py) are closed functions that synchronise
before they call, so they cannot be put behind a gate; the records here are open.

A record:
    id        the test's parameter id
    entries   the C-ABI entries of include/gpc.h whose stream contract the case holds
    env       the switches (DESIGN.md, section Switches) that select the kernel shape; everything in poison_cases.SWITCHES that a case
              does not set is unset while it runs
    inputs    inputs() -> (real, decoy): two dicts of the same keys, NumPy arrays, every array the entry reads through a pointer.  Both are
              complete, valid inputs.  Only VALUE arrays differ -- coordinates, targets, labels, records, quantised words.  Every array a
              kernel uses as an offset, an index or a count (INDEX_NAMES, and every int32 / int64 array whatever its name) is THE SAME
              OBJECT in both dicts: a mis-ordered run can change values, never an address.  Built without a GPU.
    setup     setup(capi, ctx, real) -> Made: the trained or loaded objects the entry reads, synchronised, and
                  outs    {name: (shape, dtype)} -- the device arrays the entry writes; the test allocates them and fills them with the
                          sentinel of their type before every run (SENTINEL)
                  states  {name: Sparse} -- objects whose state the entry writes, read back as poison_cases._sparse_within_basis reads
                          them (on the host, after the stream has been synchronised: the state buffers have no exported address)
                  call    call(bufs, outs): the _dev call, nothing else; bufs and outs are dicts of device tensors
                  reset   None, or a function the test runs (and synchronises) before every run: what puts a written state back
                  kernel  substrings of Context.last_dense_kernel() after the call, or ()
                  close   closes what setup made
    outputs   the names in Made.outs and Made.states, for the CPU test
    syncs     False: the header says the entry never synchronises, and the test queries the gate's event right after the call returned;
              (True, line): the entry's own comment, at that line of include/gpc.h, says it synchronises
    rule      "bits" | "RUN_TOL", as in poison_cases.py: RUN_TOL for the register kernel (dense_mfma_nt*) alone
    share     {output: s}: the smallest share of elements by which the real and the decoy result must differ, where it is not "more than
              half"; integer outputs only, each with the reason in `note`
    note      which kernel, why this shape, why a smaller share
    blind     None, or why no decoy can reach the entry: it reads no device VALUE array (nothing, or index arrays and an object's state
              only).  Such a case holds what is left: the sentinel and the snapshots (a wrong stream shows as long as the gate holds
              the caller's, a missing join while the unjoined kernel runs) and the query behind the call.

Each case is the smallest shape at which its kernel shape still launches -- except the three heavy sparse objects and the two split
batches, which are sized so that the kernel on the forked stream is the long one: a join that is missing shows only while the unjoined
kernel is still running when the copy of its output starts."""
import collections
import zlib

import numpy as np

import poison_cases as PC

Case = collections.namedtuple("Case", "id entries env inputs setup outputs syncs rule share note blind", defaults=(None,))
ONE = 1e-9               # a share floor that asks for one differing element at least
Made = collections.namedtuple("Made", "outs states call reset kernel close")

SWITCHES = PC.SWITCHES
# a NaN no arithmetic produces, and -7 in every integer width
SENTINEL = {"float64": 0x7FF8DEAD0000BEEF, "float32": 0x7FC0BEEF, "int32": -7, "uint8": 0xF9, "uint16": 0xFFF9}
# arrays that size a loop or address memory: the same object in both input sets
INDEX_NAMES = ("off", "patch", "kmax", "target", "src", "bv_count", "n_points", "capacity", "perm", "count", "bits", "leaf")

CASES = []


def same_index_arrays(real, decoy, blind=None):
    """the decoy rule, checked without a GPU: None, or what breaks it"""
    if set(real) != set(decoy):
        return "keys differ: %s" % sorted(set(real) ^ set(decoy))
    for k in real:
        a, b = real[k], decoy[k]
        if a.shape != b.shape or a.dtype != b.dtype:
            return "%s: shape or type differs" % k
        if (k in INDEX_NAMES or a.dtype in (np.int32, np.int64)) and a is not b:
            return "%s: an index array must be one object in both sets" % k
    if all(real[k] is decoy[k] for k in real) and not blind:
        return "no value array differs: the case is blind"
    if blind and not all(real[k] is decoy[k] for k in real):
        return "a case that calls itself blind has a decoy"
    return None


def _noop():
    return None


# ---- dense -------------------------------------------------------------------------------------------------------------------------------

def _dense_inputs(sizes, m, seed, ny=1, labels=False, wild=False):
    import variance_cases as VC

    def inputs():
        sets = []
        for s in (seed, seed + 1000):
            off, x0, x1, y = VC._mixed_batch(list(sizes), seed=s)
            if ny > 1:
                off, x0, x1, y = VC.with_planes(off, x0, x1, y, ny, seed=s + 1)
            if labels:                                                   # (synth.occupancy_labels: the sign of the depth plane)
                y = np.where(y[0] >= 0.0, 1.0, -1.0)
            if wild and s != seed:
                # the decoy of a selection, and of a Newton loop: targets without a surface under them -- white noise of unit variance,
                # labels dealt at random -- so that another candidate wins and the loop takes another number of steps
                rng = np.random.default_rng(s + 3)
                y = np.where(rng.random(y.shape) < 0.5, 1.0, -1.0) if labels else rng.standard_normal(y.shape)
            xs0, xs1 = VC.xstar(m, seed=s + 2)
            sets.append(dict(off=off, x0=x0, x1=x1, y=np.ascontiguousarray(y), xs0=xs0, xs1=xs1))
        sets[1]["off"] = sets[0]["off"]
        return sets[0], sets[1]
    return inputs


def _dense_setup(kind, m, ny=1, kernel=()):
    """kind: "var" (gpc_dense_fit_predict_dev with the variance), "mean" (without), "grid", "ev", "select", and the probit entries
    "irls", "irls_var", "irls_ev", "irls_select" """
    def setup(capi, ctx, real):
        import dense_ev_cases as DC
        import variance_cases as VC
        off = real["off"]
        P, N, n_max = len(off) - 1, int(off[-1]), int(np.max(np.diff(off)))
        sf, l_sq, sn = VC.DEFAULT
        prm = capi.default_params_dense(sigmaf_sq=sf, l_sq=l_sq, noise=sn, want_variance=int(kind == "var"))
        res, sz = 0.15, 5
        f8, i4 = "float64", "int32"
        if kind in ("var", "mean"):
            outs = dict(f=((P, ny, m), f8), alpha=((ny, N), f8), status=((P,), i4))
            if kind == "var":
                outs["v"] = ((P, m), f8)

            def call(b, o):
                ctx.dense_fit_predict_dev(prm, P, b["off"], n_max, N, b["x0"], b["x1"], b["y"], ny, m, b["xs0"], b["xs1"], o["f"], o.get("v"),
                                          o["alpha"], o["status"])
        elif kind == "grid":
            outs = dict(f=((P, ny, sz * sz), f8), alpha=((ny, N), f8), status=((P,), i4))

            def call(b, o):
                ctx.dense_fit_predict_grid_dev(prm, P, b["off"], n_max, N, b["x0"], b["x1"], b["y"], ny, res, sz, o["f"], o["alpha"], o["status"])
        elif kind == "ev":
            outs = dict(f=((P, 1, m), f8), v=((P, m), f8), alpha=((1, N), f8), status=((P,), i4), log_ev=((P, 1), f8))

            def call(b, o):
                ctx.dense_fit_predict_ev_dev(prm, P, b["off"], n_max, N, b["x0"], b["x1"], b["y"], 1, m, b["xs0"], b["xs1"], 0.0, 0, o["f"], o["v"],
                                             o["alpha"], o["status"], o["log_ev"])
        elif kind == "select":
            H = len(DC.CANDIDATES)
            outs = dict(f=((P, 1, m), f8), v=((P, m), f8), alpha=((1, N), f8), log_ev=((P, 1), f8), best=((P,), i4), log_ev_all=((H, P, 1), f8),
                        status=((P,), i4))

            def call(b, o):
                ctx.dense_select_dev(prm, list(DC.CANDIDATES), P, b["off"], n_max, N, b["x0"], b["x1"], b["y"], 1, m, b["xs0"], b["xs1"], 0.0, 0,
                                     f_star=o["f"], v_star=o["v"], alpha_out=o["alpha"], log_ev=o["log_ev"], best=o["best"],
                                     log_ev_all=o["log_ev_all"], status=o["status"])
        else:
            import irls_ev_cases as IC
            pq = capi.default_params_dense(sigmaf_sq=1.0, l_sq=(res / 3) ** 2, noise=0.25, noise_model=2)     # (smoke()'s probit regime)
            irls = capi.default_params_irls()
            outs = dict(f=((P, m), f8), alpha=((N,), f8), fhat=((N,), f8), iters=((P,), i4), status=((P,), i4))
            if kind != "irls":
                outs.update(v=((P, m), f8), p=((P, m), f8))
            if kind in ("irls_ev", "irls_select"):
                outs["log_q"] = ((P,), f8)
            head = lambda b: (pq, irls, P, b["off"], n_max, N, b["x0"], b["x1"], b["y"], m, b["xs0"], b["xs1"], 0.0, 0)
            if kind == "irls":
                def call(b, o):
                    ctx.dense_irls_fit_predict_dev(*head(b), o["f"], o["alpha"], o["fhat"], o["iters"], o["status"])
            elif kind == "irls_var":
                def call(b, o):
                    ctx.dense_irls_fit_predict_var_dev(*head(b), o["f"], o["v"], o["p"], o["alpha"], o["fhat"], o["iters"], o["status"])
            elif kind == "irls_ev":
                def call(b, o):
                    ctx.dense_irls_fit_predict_ev_dev(*head(b), o["f"], o["v"], o["p"], o["alpha"], o["fhat"], o["iters"], o["status"], o["log_q"])
            else:
                cand = list(IC.CANDIDATES)
                outs.update(best=((P,), i4), log_q_all=((len(cand), P), f8))

                def call(b, o):
                    h = head(b)
                    ctx.dense_irls_select_dev(h[0], h[1], cand, *h[2:], f_star=o["f"], v_star=o["v"], p_star=o["p"], alpha_out=o["alpha"],
                                              fhat_out=o["fhat"], log_q=o["log_q"], best=o["best"], log_q_all=o["log_q_all"], iters=o["iters"],
                                              status=o["status"])
        return Made(outs, {}, call, None, kernel, _noop)
    return setup


_DENSE_OUT = {"var": ("f", "v", "alpha", "status"), "mean": ("f", "alpha", "status"), "grid": ("f", "alpha", "status"),
              "ev": ("f", "v", "alpha", "status", "log_ev"), "select": ("f", "v", "alpha", "log_ev", "best", "log_ev_all", "status"),
              "irls": ("f", "alpha", "fhat", "iters", "status"), "irls_var": ("f", "v", "p", "alpha", "fhat", "iters", "status"),
              "irls_ev": ("f", "v", "p", "alpha", "fhat", "iters", "status", "log_q"),
              "irls_select": ("f", "v", "p", "alpha", "fhat", "iters", "status", "log_q", "best", "log_q_all")}
_DENSE_ENTRY = {"var": "gpc_dense_fit_predict_dev", "mean": "gpc_dense_fit_predict_dev", "grid": "gpc_dense_fit_predict_grid_dev",
                "ev": "gpc_dense_fit_predict_ev_dev", "select": "gpc_dense_select_dev", "irls": "gpc_dense_irls_fit_predict_dev",
                "irls_var": "gpc_dense_irls_fit_predict_var_dev", "irls_ev": "gpc_dense_irls_fit_predict_ev_dev",
                "irls_select": "gpc_dense_irls_select_dev"}
_STATUS = "status is 0 for every patch that factors, whatever its values"
_BEST = "best is one of a handful of candidate indices and iters a small step count: most patches of both sets agree, one at least must not"


def _dense(cid, kind, sizes, env, kernel, rule, note, m=17, ny=1):
    share = {"status": 0.0}
    if kind in ("select", "irls_select"):
        share["best"] = ONE
    if kind.startswith("irls"):
        share["iters"] = ONE
    seed = zlib.crc32(cid.encode()) % 100000              # (of the id, not of the case's place in the table)
    CASES.append(Case(cid, (_DENSE_ENTRY[kind],), env, _dense_inputs(sizes, m, seed, ny, labels=kind.startswith("irls"), wild=len(share) > 1),
                      _dense_setup(kind, m, ny, kernel), _DENSE_OUT[kind], False, rule, share,
                      note + "; " + _STATUS + ("; " + _BEST if len(share) > 1 else "")))


# (the batches of poison_cases' variance and evidence records: the smallest that reach each route with its factor export)
_REG, _W1, _BIG = (100, 0, 180, 64), (200, 0, 230, 64), (300, 520, 0, 270)
for _kind in ("var", "ev"):
    _dense("dense-register-" + _kind, _kind, _REG, {}, ("dense_mfma_nt",), "RUN_TOL",
           "register kernel (dense_mfma_nt12): alpha meets in arrival order (LDS atomics), factor export, dense_variance")
    _dense("dense-one-wave-" + _kind, _kind, _W1, {"GPC_W1_MIN_P": "1"}, ("dense_mfma_w1",), "bits",
           "one-wave kernel with the factor export in the workspace, dense_variance")
    _dense("dense-tiled-" + _kind, _kind, _BIG, {}, ("dense_mfma_big",), "bits", "tiled kernel with the factor export, dense_variance_big")
for _kind in ("var", "ev"):
    _dense("dense-generic-" + _kind, _kind, (40, 0, 100, 7), {"GPC_FORCE_GENERIC": "1"}, ("dense_generic",), "bits",
           "generic kernel with the factor export and the variance behind it")
for _route, _sz, _envs, _rule in (("register", _REG, {}, "RUN_TOL"), ("tiled", _BIG, {}, "bits")):
    _dense("dense-%s-select" % _route, "select", _sz, _envs, (), _rule,
           "the selection on the %s%s route" % (_route, " kernel's (register: RUN_TOL)" if _rule == "RUN_TOL" else ""))
_dense("dense-register-grid-ny3", "grid", (40, 100, 180, 0, 250, 7), {}, ("dense_mfma_nt",), "RUN_TOL",
       "gpc_dense_fit_predict_grid_dev on the register kernel, three target planes", ny=3)
_dense("dense-one-wave-select", "select", _W1, {"GPC_W1_MIN_P": "1"}, (), "bits",
       "the selection: one fit with evidence per candidate and the keep-best kernel behind each, all on the caller's stream")
# The size-class split (csrc/dense_api.hip, dense_split): n <= 256 on the caller's stream, 257 .. 272 on s_in, the rest on s_out.
# out-heavy: the tiled class is the long one; in-heavy: the NT = 17 class is -- 800 patches, three rounds of one workgroup per CU, beside
# ONE patch of the smallest tiled size and one of 16 points, so that s_in is still busy when the other two have joined.
_OUT_HEAVY = (300, 260, 100, 520) + (400, 330, 512, 290) * 6 + (0, 272, 256)
_IN_HEAVY = (273, 16, 0) + (257, 272, 265, 270) * 200
for _id, _sizes in (("out-heavy", _OUT_HEAVY), ("in-heavy", _IN_HEAVY)):
    _dense("dense-split-" + _id, "mean", _sizes, {"GPC_NO_W1": "1"}, ("dense_mfma_nt16 + dense_mfma_nt17 + dense_mfma_big",), "RUN_TOL",
           "ragged batch with patches in all three size classes, forked over the caller's stream, s_in and s_out; the two register "
           "classes make it RUN_TOL")
for _kind in ("irls", "irls_var", "irls_ev", "irls_select"):
    _dense("dense-" + _kind.replace("_", "-"), _kind, (100, 0, 180, 64), {}, (), "bits",
           "probit Newton loop on the device" + {"irls": "", "irls_var": ", latent variance and probability", "irls_ev": ", Laplace evidence",
                                                 "irls_select": ", selection by Laplace evidence"}[_kind])


# ---- sparse read-outs ------------------------------------------------------------------------------------------------------------------

HEAVY_P, HEAVY_N, HEAVY_CAP = 256, 4096, 47
_HEAVY_B = {"le16": (16, 24, 40), "17to32": (32, 8, 40), "gt32": (47, 8, 24)}      # (the heavy bucket's size, the two single patches')


def heavy_state(which):
    """readout_cases.state for an object of HEAVY_P patches, all but two of them in one bucket of sp_predict_launch (b <= 16, 17 .. 32,
    more): patches 1 and 2 are the other two buckets'.  Eight distinct states of the heavy size, repeated."""
    import readout_cases as RC
    ld = RC.ld_of(HEAVY_CAP)
    heavy, one, two = _HEAVY_B[which]
    b = np.full(HEAVY_P, heavy, dtype=np.int32)
    b[1], b[2] = one, two
    alpha, C, BV = np.zeros((HEAVY_P, 1, ld)), np.zeros((HEAVY_P, ld, ld)), np.zeros((HEAVY_P, ld, 2))
    made = {}
    for i in range(HEAVY_P):
        key = (int(b[i]), i % 8)
        if key not in made:
            made[key] = RC.state(key[0], 1, RC.L5, seed=9000 + 10 * key[0] + key[1])
        a, c, v = made[key]
        alpha[i, :, :b[i]], C[i, :b[i], :b[i]], BV[i, :b[i]] = a, c, v
    return dict(capacity=HEAVY_CAP, ny=1, l_sq=RC.L5, P=HEAVY_P, ld=ld, b=b, alpha=alpha, C=C, BV=BV)


def _grid_inputs(m, seed):
    def inputs():
        import readout_cases as RC
        sets = []
        for s in (seed, seed + 1):
            rng = np.random.default_rng(s)
            sets.append(dict(xs0=rng.uniform(-RC.RES / 2, RC.RES / 2, m), xs1=rng.uniform(-RC.RES / 2, RC.RES / 2, m)))
        return tuple(sets)
    return inputs


def _load(capi, ctx, B):
    import test_sparse_readout_gpu as TR
    return TR._load(capi, ctx, B)


def _predict_setup(batch, m, sigma):
    def setup(capi, ctx, real):
        g = _load(capi, ctx, batch())
        outs = dict(f=((g.P, g.ny, m), "float64"), status=((g.P,), "int32"))
        if sigma:
            outs["sigma"] = ((g.P, m), "float64")

        def call(b, o):
            g.predict_dev(m, b["xs0"], b["xs1"], o["f"], o.get("sigma"), False, o["status"])
        return Made(outs, {}, call, None, (), g.close)
    return setup


def _heavy_off():
    """every patch of a heavy object HEAVY_N points of its own, patches 1 and 2 -- the other two buckets' -- one point each"""
    cnt = np.full(HEAVY_P, HEAVY_N)
    cnt[1] = cnt[2] = 1
    return np.concatenate([[0], np.cumsum(cnt)]).astype(np.int32)


def _heavy_inputs(seed):
    def inputs():
        import readout_cases as RC
        off = _heavy_off()
        sets = []
        for s in (seed, seed + 1):
            rng = np.random.default_rng(s)
            sets.append(dict(off=off, x0=rng.uniform(-RC.RES / 2, RC.RES / 2, int(off[-1])), x1=rng.uniform(-RC.RES / 2, RC.RES / 2, int(off[-1]))))
        return tuple(sets)
    return inputs


def _heavy_setup(which):
    def setup(capi, ctx, real):
        g = _load(capi, ctx, heavy_state(which))
        N = len(real["x0"])

        def call(b, o):
            g.predict_points_dev(b["off"], N, b["x0"], b["x1"], o["f"], o["sigma"], False, o["status"])
        return Made(dict(f=((1, N), "float64"), sigma=((N,), "float64"), status=((g.P,), "int32")), {}, call, None, (), g.close)
    return setup


_PSTATUS = "status is 0 for every patch the kernels reach, whatever the query"
for _which, _what in (("le16", "sparse_predict_small_kernel<16> on the context's own stream"),
                      ("17to32", "sparse_predict_small_kernel<32> on s_in"), ("gt32", "sparse_predict_kernel on s_out")):
    CASES.append(Case("sparse-predict-sigma-heavy-" + _which, ("gpc_sparse_predict_points_dev",), {}, _heavy_inputs(40), _heavy_setup(_which),
                      ("f", "sigma", "status"), False, "bits", {"status": 0.0},
                      "the fork of sp_predict_launch with all patches but two in the bucket of " + _what + ", %d points each, and one patch "
                      "with one point in each of the other two: the heavy bucket's kernel is still running when the other two have joined; "
                      % HEAVY_N + _PSTATUS))


def _cap100():
    import readout_cases as RC
    return RC.batch(*RC.CASES[1])


CASES.append(Case("sparse-predict-mean", ("gpc_sparse_predict_dev",), {}, _grid_inputs(33, 50), _predict_setup(_cap100, 33, False),
                  ("f", "status"), False, "bits", {"status": 0.0},
                  "mean only: the three launches on the caller's stream, no fork; every basis size of readout_cases' capacity-100 object; "
                  + _PSTATUS))
CASES.append(Case("sparse-predict-sigma", ("gpc_sparse_predict_dev",), {}, _grid_inputs(33, 51), _predict_setup(_cap100, 33, True),
                  ("f", "status", "sigma"), False, "bits", {"status": 0.0},
                  "the fork of sp_predict_launch on a shared grid: every basis size of the capacity-100 object, patches in all three buckets; "
                  + _PSTATUS))
CASES.append(Case("sparse-predict-sigma-regular", ("gpc_sparse_predict_dev",), {"GPC_SPARSE_NO_SMALL_PREDICT": "1"}, _grid_inputs(33, 52),
                  _predict_setup(_cap100, 33, True), ("f", "status", "sigma"), False, "bits", {"status": 0.0},
                  "sparse_predict_kernel alone on the caller's stream; " + _PSTATUS))


def _points_inputs(seed, with_y):
    def inputs():
        import readout_cases as RC
        B = _cap100()
        real = dict(off=B["off"], x0=B["q0"], x1=B["q1"])
        rng = np.random.default_rng(seed)
        N = len(B["q0"])
        decoy = dict(off=B["off"], x0=rng.uniform(-RC.RES / 2, RC.RES / 2, N), x1=rng.uniform(-RC.RES / 2, RC.RES / 2, N))
        if with_y:
            real["y"] = B["yq"]
            decoy["y"] = RC.smooth_y(B["ny"], decoy["x0"], decoy["x1"]) + rng.normal(0.0, RC.NOISE_Y, (B["ny"], N))
        return real, decoy
    return inputs


def _points_setup(capi, ctx, real):
    g = _load(capi, ctx, _cap100())
    N = len(real["x0"])

    def call(b, o):
        g.predict_points_dev(b["off"], N, b["x0"], b["x1"], o["f"], o["sigma"], False, o["status"])
    return Made(dict(f=((g.ny, N), "float64"), sigma=((N,), "float64"), status=((g.P,), "int32")), {}, call, None, (), g.close)


def _likelihood_setup(capi, ctx, real):
    g = _load(capi, ctx, _cap100())
    N = len(real["x0"])

    def call(b, o):
        g.likelihood_dev(b["off"], N, b["x0"], b["x1"], b["y"], o["dX"], o["l"])
    return Made(dict(dX=((N, 3), "float64"), l=((N,), "float64")), {}, call, None, (), g.close)


def _scattered_inputs():
    import readout_cases as RC
    import render_attrs_cases as AC
    patch, p0, p1 = AC.scatter_pattern("uniform", _cap100(), 257, seed=1257)
    rng = np.random.default_rng(1258)
    return (dict(patch=patch, x0=p0, x1=p1),
            dict(patch=patch, x0=rng.uniform(-RC.RES / 2, RC.RES / 2, 257), x1=rng.uniform(-RC.RES / 2, RC.RES / 2, 257)))


def _scattered_setup(capi, ctx, real):
    g = _load(capi, ctx, _cap100())
    n = len(real["patch"])

    def call(b, o):
        g.predict_scattered_dev(n, b["patch"], b["x0"], b["x1"], 1, o["f"], o["sigma"], False, o["status"])
    return Made(dict(f=((g.ny, n), "float64"), sigma=((n,), "float64"), status=((g.P,), "int32")), {}, call, None, (), g.close)


CASES.append(Case("sparse-predict-points", ("gpc_sparse_predict_points_dev",), {}, _points_inputs(61, False), _points_setup,
                  ("f", "sigma", "status"), False, "bits", {"status": 0.0},
                  "ragged queries with sigma: the fork of sp_predict_launch at every basis size; " + _PSTATUS))
CASES.append(Case("sparse-predict-scattered", ("gpc_sparse_predict_scattered_dev",), {}, _scattered_inputs, _scattered_setup,
                  ("f", "sigma", "status"), False, "bits", {"status": 0.0},
                  "257 (patch, point) pairs: bucketing in the workspace, the forked predict, the scatter back; " + _PSTATUS))
CASES.append(Case("sparse-likelihood", ("gpc_sparse_likelihood_dev",), {}, _points_inputs(62, True), _likelihood_setup, ("dX", "l"), False,
                  "bits", {}, "sparse_likelihood_kernel on the ragged queries of the capacity-100 object"))


# ---- sparse add ---------------------------------------------------------------------------------------------------------------------------

def _add_inputs():
    from gp_compressor_amd import synth
    res = 0.15
    off, x0, x1, y = synth.make_patches(37, 150, res=res, seed=23 + 12 + 37, ragged=True, ny=1, n_min=1)      # poison_cases: default-cap12
    perm = synth.sattolo_perms(off, seed=9)
    rng = np.random.default_rng(77)
    N = int(off[-1])
    d0, d1 = rng.uniform(-res / 2, res / 2, N), rng.uniform(-res / 2, res / 2, N)
    dy = (0.012 * np.sin(17.0 * d0 + 1.0) * np.cos(11.0 * d1) + rng.normal(0.0, 0.003, N))[None, :]
    return dict(off=off, x0=x0, x1=x1, y=y, perm=perm), dict(off=off, x0=d0, x1=d1, y=np.ascontiguousarray(dy), perm=perm)


def _add_setup(capi, ctx, real):
    off = real["off"]
    P, N, n_max = len(off) - 1, int(off[-1]), int(np.max(np.diff(off)))
    g = capi.Sparse(ctx, capi.default_params_sparse(1, capacity=12), P, 1)

    def call(b, o):
        g.add_dev(b["off"], n_max, N, b["x0"], b["x1"], b["y"], b["perm"], o["status"])
    return Made(dict(status=((P,), "int32")), dict(g=g), call, g.reset, (), g.close)


for _id, _env, _note in (("default", {}, "rows phase, its work list, one wave per patch behind it"),
                         ("no-rows", {"GPC_SPARSE_NO_ROWS": "1"}, "the one-wave small-basis kernel from the first point")):
    CASES.append(Case("sparse-add-" + _id, ("gpc_sparse_add_dev",), _env, _add_inputs, _add_setup, ("status", "g"), False, "bits",
                      {"status": 0.0, "g.b": 0.0},
                      _note + "; the object is emptied before every run; status is 0 and the basis sits at its capacity for both sets"))


# ---- reproject ---------------------------------------------------------------------------------------------------------------------------

_RP, _RM = 1025, 4


def _reproject_inputs():
    import reproject_cases as RPC
    bv = RPC.bv_pattern("random", _RP, 13)
    sets = []
    for seed in (13, 14):
        xs0, xs1, f, R, mu, cs, cm = RPC.inputs(_RP, _RM, seed, True, None)
        sets.append(dict(bv_count=bv, xs0=xs0, xs1=xs1, f=f, R=R, mu=mu, cs=cs, cm=cm))
    return tuple(sets)


def _reproject_setup(capi, ctx, real):
    n = _RM * int(np.count_nonzero(real["bv_count"]))

    def call(b, o):
        ctx.reproject_dev(_RP, _RM, b["bv_count"], b["xs0"], b["xs1"], b["f"], b["cs"], b["R"], b["mu"], b["cm"], o["cloud"], o["n_points"])
    return Made(dict(cloud=((n, 32), "uint8"), n_points=((1,), "int32")), {}, call, None, (), _noop)


CASES.append(Case("reproject", ("gpc_reproject_dev",), {}, _reproject_inputs, _reproject_setup, ("cloud", "n_points"), False, "bits",
                  {"n_points": 0.0},
                  "1025 patches: two per thread of the scan, whose offsets live in the workspace; a cloud buffer of exactly n_points "
                  "32-byte records, compared record by record; n_points depends on bv_count alone"))


# ---- cloud distortion: an entry that synchronises ---------------------------------------------------------------------------------------------

def _distortion_inputs():
    import distortion_cases as DS
    from gp_compressor_amd import capi
    rec = lambda c: np.ascontiguousarray(c).view(np.uint8).reshape(-1, 32).copy()
    sets = []
    for seed in (11, 21):                                       # (seed 11: test_distortion_gpu's pair of 700 against 500 records)
        a, b = DS.random_pair(700, 500, seed=seed)
        assert a.dtype == capi.Context.POINT_DTYPE
        sets.append(dict(a=rec(a), b=rec(b)))
    return tuple(sets)


def _distortion_setup(capi, ctx, real):
    na, nb = len(real["a"]), len(real["b"])

    def call(b, o):
        ctx.cloud_distortion_dev(b["a"], na, b["b"], nb, None, nn=o["nn"], d2=o["d2"], result=o["result"])
    return Made(dict(nn=((na,), "int32"), d2=((na,), "float64"), result=((1, 88), "uint8")), {}, call, None, (), _noop)


CASES.append(Case("cloud-distortion", ("gpc_cloud_distortion_dev",), {}, _distortion_inputs, _distortion_setup, ("nn", "d2", "result"),
                  (True, 939), "bits", {},
                  "synchronises while it builds the search table; the search and the sums are enqueued behind that: the outputs are "
                  "complete once the stream is.  result is compared as one record of 88 bytes"))


# ---- rate control: the object of prune_ref's smallest regime (capacity 16, 24 patches of 60 points, one wave per patch) ---------------------

def _rate_regime():
    import prune_ref as pr
    cap, div, n, P, _, keep = [c for c in pr.case_ids() if c[4] == 1][0]
    assert (cap, keep) == (16, 5)
    return pr, cap, div, n, P


def _rate_object(capi, ctx):
    """trained anew: the entries below change the object, so every run starts from one of these (Made.reset)"""
    pr, cap, div, n, P = _rate_regime()
    off, x0, x1, y, perm = pr.batch(cap, n, P, 1)
    g = capi.Sparse(ctx, capi.default_params_sparse(1, ref_field_delete_bug=0, **pr.kernel_kw(cap, div, 1)), P, 1)
    assert np.all(g.add(off, x0, x1, y, perm) == 0)
    return g


def _rate_inputs():
    """the object's own training points, and the same points dealt to the patches in reverse"""
    pr, cap, div, n, P = _rate_regime()
    off, x0, x1, y, _ = pr.batch(cap, n, P, 1)
    return (dict(off=off, x0=x0, x1=x1, y=np.ascontiguousarray(y)),
            dict(off=off, x0=x0[::-1].copy(), x1=x1[::-1].copy(), y=np.ascontiguousarray(y[:, ::-1])))


def _no_inputs():
    return {}, {}


def _rate_setup(kind):
    def setup(capi, ctx, real):
        box = {"g": _rate_object(capi, ctx)}
        P = box["g"].P
        N = len(real["x0"]) if real else 0
        f8, i4 = "float64", "int32"

        def renew():
            box["g"].close()
            box["g"] = _rate_object(capi, ctx)
        state = lambda: PC._sparse_within_basis(box["g"])
        if kind == "prune":
            outs, states = dict(removed=((P,), i4), status=((P,), i4)), dict(g=state)

            def call(b, o):
                box["g"].prune_dev(keep=5, removed=o["removed"], status=o["status"])
        elif kind == "prune_rd":
            outs, states = dict(removed=((P,), i4), mse0=((P,), f8), status=((P,), i4)), {}

            def call(b, o):
                box["g"].prune_rd_dev(b["off"], N, b["x0"], b["x1"], b["y"], keep=2, removed=o["removed"], mse0=o["mse0"], status=o["status"])
        else:
            outs, states = dict(bits=((P,), i4), mse0=((P,), f8), mse_q=((P,), f8), status=((P,), i4)), {}

            def call(b, o):
                box["g"].quantize_rd_dev(b["off"], N, b["x0"], b["x1"], b["y"], bits_min=6, bits=o["bits"], mse0=o["mse0"], mse_q=o["mse_q"],
                                         status=o["status"])
        return Made(outs, states, call, None if kind == "quantize_rd" else renew, (), lambda: box["g"].close())
    return setup


CASES.append(Case("sparse-prune", ("gpc_sparse_prune_dev",), {}, _no_inputs, _rate_setup("prune"), ("removed", "status", "g"), False, "bits", {},
                  "sparse_prune_kernel to five vectors per patch; a newly trained object before every run",
                  blind="reads no caller array but the optional index array `target`: its input is the object's own state"))
CASES.append(Case("sparse-prune-rd", ("gpc_sparse_prune_rd_dev",), {}, _rate_inputs, _rate_setup("prune_rd"), ("removed", "mse0", "status"), False,
                  "bits", {"removed": 0.0, "status": 0.0},
                  "sparse_prune_rd_kernel to two vectors without a bound: removed and status depend on the state alone, mse0 on the points; a "
                  "newly trained object before every run"))
CASES.append(Case("sparse-quantize-rd", ("gpc_sparse_quantize_rd_dev",), {}, _rate_inputs, _rate_setup("quantize_rd"),
                  ("bits", "mse0", "mse_q", "status"), False, "bits", {"bits": 0.0, "status": 0.0},
                  "sparse_quantize_rd_kernel without a bound: bits is bits_min and status 0 for both sets, the two errors are the points'"))
def _train_setup(capi, ctx, real):
    import readout_cases as RC
    import torch
    box = {"g": _load(capi, ctx, _cap100())}
    P, N = box["g"].P, len(real["x0"])
    ls = torch.zeros((P, RC.TRAIN_MAXC + 2), dtype=torch.float64, device="cuda")      # (rows beyond iters are not written: no output of the case)
    torch.cuda.synchronize()

    def renew():
        box["g"].close()
        box["g"] = _load(capi, ctx, _cap100())

    def call(b, o):
        box["g"].train_sigmaf_dev(b["off"], N, b["x0"], b["x1"], b["y"], RC.TRAIN_STEP, RC.TRAIN_MAXC, o["p0"], o["iters"], ls, o["delta"])
    return Made(dict(p0=((P,), "float64"), iters=((P,), "int32"), delta=((P, 2), "float64")), {}, call, renew, (), lambda: box["g"].close())


CASES.append(Case("sparse-train-sigmaf", ("gpc_sparse_train_sigmaf_dev",), {}, _points_inputs(63, True), _train_setup, ("p0", "iters", "delta"),
                  False, "bits", {"iters": 0.0},
                  "the raw likelihood pass and sparse_train_kernel on readout_cases' capacity-100 object: the twelve patches of its nineteen "
                  "that hold twenty vectors or more train (src/sparse_gp.hpp:609), the others return sigma_f as it is; the object is loaded "
                  "anew before every run; iters is 0 or at its cap for the patches of both sets"))


def _dequantize_inputs():
    _, cap, _, _, P = _rate_regime()
    ld = 32                                                    # (round_up(capacity + 1, 16))
    rng = np.random.default_rng(6)
    bv_count, bits = np.full(P, 10, dtype=np.int32), np.full(P, 6, dtype=np.int32)
    sets = []
    for lo, hi in ((-1.0, 1.0), (-0.7, 1.3)):
        rg = np.empty((P, 3, 2), dtype=np.float32)
        rg[..., 0], rg[..., 1] = lo, hi
        sets.append(dict(bv_count=bv_count, bits=bits, q_alpha=rng.integers(0, 64, (P, 1, ld)).astype(np.uint16),
                         q_bv=rng.integers(0, 64, (P, ld, 2)).astype(np.uint16), range=rg))
    return tuple(sets)


def _dequantize_setup(capi, ctx, real):
    pr, cap, div, n, P = _rate_regime()
    g = capi.Sparse(ctx, capi.default_params_sparse(1, ref_field_delete_bug=0, **pr.kernel_kw(cap, div, 1)), P, 1)
    assert g.ld() == real["q_alpha"].shape[2]

    def call(b, o):
        g.dequantize_dev(b["bv_count"], b["bits"], b["q_alpha"], b["q_bv"], b["range"])

    def state():                                               # (C and Q are zero behind a dequantize: no output of the case)
        s = PC._sparse_within_basis(g)
        return {k: s[k] for k in ("b", "alpha", "BV")}
    return Made({}, dict(g=state), call, g.reset, (), g.close)


CASES.append(Case("sparse-dequantize", ("gpc_sparse_dequantize_dev",), {}, _dequantize_inputs, _dequantize_setup, ("g",), False, "bits", {"g.b": 0.0},
                  "ten 6-bit codes per patch into an emptied object; the decoy has other codes and other ranges, b is bv_count for both"))


# ---- rate allocation, the camera's rays, the collectives ---------------------------------------------------------------------------------

def _allocate_problem():
    import test_rate_alloc_gpu as TA
    pb = TA._problem(257, 9, seed=30)                          # (poison_cases: one row past a scan tile; an even seed: monotone curves)
    return pb, (pb.kmax + 1).astype(np.int32)


def _allocate_inputs():
    pb, count = _allocate_problem()
    kmax, unit = np.ascontiguousarray(pb.kmax), np.ascontiguousarray(pb.unit)
    real = dict(kmax=kmax, unit=unit, count=count, d0=np.ascontiguousarray(pb.d0), d=np.ascontiguousarray(pb.d), w=np.ascontiguousarray(pb.w))
    return real, dict(real, d0=real["d0"] * 0.61, d=real["d"] * 0.61, w=np.ascontiguousarray(real["w"][::-1]))


def _allocate_setup(capi, ctx, real):
    import test_rate_alloc_gpu as TA
    pb, _ = _allocate_problem()
    need = TA._some_needs(pb)[1]

    def call(b, o):
        ctx.rate_allocate_dev(pb.R, pb.ld, b["kmax"], b["d0"], b["d"], need, w=b["w"], w_all=pb.w_all, unit=b["unit"], unit_all=pb.unit_all,
                              refine=1, count=b["count"], k=o["k"], target=o["target"], result=o["result"])
    return Made(dict(k=((pb.R,), "int32"), target=((pb.R,), "int32"), result=((1, 32), "uint8")), {}, call, None, (), _noop)


CASES.append(Case("rate-allocate", ("gpc_rate_allocate_dev",), {}, _allocate_inputs, _allocate_setup, ("k", "target", "result"), False, "bits",
                  {"k": ONE, "target": ONE},
                  "257 rows: 137 launches on the caller's stream, scratch in the workspace; the decoy scales the errors and deals the weights "
                  "in reverse, which moves k and target in some rows and lambda in the 32-byte result, compared as one record"))


def _camera_setup(capi, ctx, real):
    W, H = 23, 17
    Rc = np.ascontiguousarray(np.linalg.qr(np.random.default_rng(3).normal(size=(3, 3)))[0])

    def call(b, o):
        ctx._check(ctx.lib.gpc_camera_rays_dev(ctx.h, capi._ptr(Rc), 20.0, 21.0, (W - 1) / 2, (H - 1) / 2, W, H, capi._ptr(o["dirs"])))
    return Made(dict(dirs=((W * H, 3), "float64")), {}, call, None, (), _noop)


CASES.append(Case("camera-rays", ("gpc_camera_rays_dev",), {}, _no_inputs, _camera_setup, ("dirs",), False, "bits", {},
                  "the 23 x 17 image of render_cases", blind="reads no device array: R is a host pointer read at call time"))


def _gather_inputs():
    rng = np.random.default_rng(8)
    return dict(rows=rng.normal(size=(37, 7))), dict(rows=rng.normal(size=(37, 7)))


def _comm_setup(gather):
    def setup(capi, ctx, real):
        P, row = real["rows"].shape
        comm = capi.Comm(ctx, 1, 0)
        comm.set_partition(P, np.random.default_rng(17).permutation(P).astype(np.int32))
        if gather:
            def call(b, o):
                comm.allgather_fstar_dev(row, b["rows"], o["gathered"], o["f_star"])
            outs = dict(gathered=((P, row), "float64"), f_star=((P, row), "float64"))
        else:
            def call(b, o):
                comm.unpermute_fstar_dev(row, b["rows"], o["f_star"])
            outs = dict(f_star=((P, row), "float64"))
        return Made(outs, {}, call, None, (), comm.close)
    return setup


CASES.append(Case("allgather-one-rank", ("gpc_allgather_fstar_dev",), {}, _gather_inputs, _comm_setup(True), ("gathered", "f_star"), False, "bits", {},
                  "the collective on a one-rank communicator and unpermute_rows_kernel behind it, 37 rows of 7 doubles"))
CASES.append(Case("unpermute-one-rank", ("gpc_unpermute_fstar_dev",), {}, _gather_inputs, _comm_setup(False), ("f_star",), False, "bits", {},
                  "unpermute_rows_kernel alone through the communicator's table"))


# ---- the map: cutter, insertion, ray cast, occupancy batch, normals, registration, remap, render, decode -------------------------------------

_MAP_RES, _MAP_SZ, _MAP_N = 0.15, 10, 3000


def _plane_records(seed, shift=0.0, n=_MAP_N, extent=0.6):
    """(n, 32) uint8: the records of synth.plane_cloud, moved along x"""
    from gp_compressor_amd import capi, synth
    xyz, rgb = synth.plane_cloud(n, seed=seed, extent=extent)
    xyz = xyz + np.array([shift, 0.0, 0.0], dtype=np.float32)
    return np.ascontiguousarray(capi.Context.make_cloud(capi.Context, xyz, rgb)).view(np.uint8).reshape(-1, 32).copy()


def _as_cloud(capi, rec):
    return np.ascontiguousarray(rec).reshape(-1).view(capi.Context.POINT_DTYPE)


def _map(capi, ctx, seed=2):
    """the plane cloud cut by the producer, depth and colour GPs trained on every leaf (smoke()'s model in small)"""
    pt = ctx.project_cloud(_as_cloud(capi, _plane_records(seed)), _MAP_RES, _MAP_SZ)
    v = pt.view
    kw = dict(sigmaf_sq=1.0, l_sq=(_MAP_RES / 5) ** 2)
    gd = capi.Sparse(ctx, capi.default_params_sparse(1, noise=1e-3, capacity=24, **kw), v.P, 1)
    gc = capi.Sparse(ctx, capi.default_params_sparse(3, noise=1.0, capacity=100, **kw), v.P, 3)
    gd.add_dev(v.off, v.n_max, v.n_total, v.x0, v.x1, v.y)
    gc.add_dev(v.off, v.n_max, v.n_total, v.x0, v.x1, v.rgb)
    ctx.synchronize()
    return pt, gd, gc


def _close_all(*objs):
    def close():
        for o in objs:
            if o is not None:
                o.close()
    return close


def _batch_arrays(pt):
    g = pt.fetch()
    return {k: np.ascontiguousarray(g[k]) for k in ("off", "x0", "x1", "y", "R", "mean", "src")}


def _cloud_inputs(name, seeds, shift=0.0):
    def inputs():
        return {name: _plane_records(seeds[0], shift)}, {name: _plane_records(seeds[1], shift)}
    return inputs


def _project_setup(capi, ctx, real):
    box = {}

    def drop():
        if box.get("pt") is not None:
            box.pop("pt").close()

    def call(b, o):
        box["pt"] = ctx.project_cloud(b["cloud"], _MAP_RES, _MAP_SZ, n=_MAP_N)
    return Made({}, dict(batch=lambda: _batch_arrays(box["pt"])), call, drop, (), drop)


CASES.append(Case("project-cloud", ("gpc_project_cloud_dev",), {}, _cloud_inputs("cloud", (2, 3)), _project_setup, ("batch",), (True, 680), "bits", {},
                  "the cutter on 3000 points of a plane; the batch it allocates is fetched on the host; the decoy is another cloud of the "
                  "same length, which moves every array of the batch"))


def _normals_setup(capi, ctx, real):
    pt = ctx.project_cloud(_as_cloud(capi, _plane_records(2)), _MAP_RES, _MAP_SZ)

    def call(b, o):
        pt.normals(_MAP_N, out=o["normals"])
    return Made(dict(normals=((_MAP_N, 3), "float32")), {}, call, None, (), pt.close)


CASES.append(Case("patches-normals", ("gpc_patches_normals_dev",), {}, _no_inputs, _normals_setup, ("normals",), (True, 960), "bits", {},
                  "NaN fill, the src test (one synchronisation), the owning leaf's normal per point",
                  blind="reads no caller array: its input is the batch object"))


def _insert_setup(capi, ctx, real):
    pt, gd, gc = _map(capi, ctx)
    box = {}

    def drop():
        if box.get("new") is not None:
            box.pop("new").close()

    def call(b, o):
        box["new"], box["o2n"] = pt.insert_cloud(b["scan"], min_nbr=20, depth=gd, n=_MAP_N)

    def read():                                                # (a kept leaf keeps its frame and its mean: no output of the case)
        d = _batch_arrays(box["new"])
        return dict({k: d[k] for k in ("off", "x0", "x1", "y", "src")}, o2n=np.ascontiguousarray(box["o2n"]))
    return Made({}, dict(new=read), call, drop, (), lambda: (drop(), _close_all(gd, gc, pt)()))


CASES.append(Case("insert-cloud", ("gpc_patches_insert_cloud_dev",), {}, _cloud_inputs("scan", (2, 3), shift=_MAP_RES), _insert_setup, ("new",),
                  (True, 730), "bits", {"new.o2n": 0.0},
                  "a scan moved by one voxel into the trained map: old leaves extended, fresh leaves cut; o2n places the old leaves, the same "
                  "for both scans where they meet the same voxels"))


def _cells_inputs():
    """labels for up to 64 leaves of 100 cells, four fifths observed: mostly occupied in the real set, mostly free in the decoy"""
    sets = []
    for seed, p in ((31, (0.2, 0.7, 0.1)), (32, (0.2, 0.1, 0.7))):
        rng = np.random.default_rng(seed)
        sets.append(dict(cells=rng.choice(np.arange(3, dtype=np.uint8), size=(64, _MAP_SZ * _MAP_SZ), p=p)))
    return tuple(sets)


def _occupancy_setup(capi, ctx, real):
    import ctypes as C
    pt = ctx.project_cloud(_as_cloud(capi, _plane_records(2)), _MAP_RES, _MAP_SZ)
    P, m = pt.view.P, pt.view.m
    assert P <= 64 and m == _MAP_SZ * _MAP_SZ
    sizes = {}

    def call(b, o):
        nt, nm = C.c_int32(0), C.c_int32(0)
        ctx._check(ctx.lib.gpc_occupancy_batch_dev(ctx.h, pt.h, capi._ptr(b["cells"]), capi._ptr(o["off"]), capi._ptr(o["x0"]), capi._ptr(o["x1"]),
                                                   capi._ptr(o["y"]), C.addressof(nt), C.addressof(nm)))
        sizes["n"] = np.array([nt.value, nm.value], dtype=np.int64)
    outs = dict(off=((P + 1,), "int32"), x0=((P * m,), "float64"), x1=((P * m,), "float64"), y=((P * m,), "float64"))
    return Made(outs, dict(sizes=lambda: dict(n=sizes["n"])), call, None, (), pt.close)


CASES.append(Case("occupancy-batch", ("gpc_occupancy_batch_dev",), {}, _cells_inputs, _occupancy_setup, ("off", "x0", "x1", "y", "sizes"), (True, 778),
                  "bits", {"sizes.n": ONE},
                  "the labelled cells of the first P leaves as the probit GP's ragged batch; x0, x1 and y are compacted, so other labels move "
                  "every entry behind the first gap; n_total moves with them (sizes.n), n_max need not"))


def _raycast_setup(capi, ctx, real):
    import torch
    pt, gd, gc = _map(capi, ctx)
    P, m = pt.view.P, pt.view.m
    cells = torch.zeros((P, m), dtype=torch.uint8, device="cuda")
    origin = np.array([0.3, 0.3, 2.0])
    got = {}

    def call(b, o):
        got["counts"] = pt.raycast(b["cloud"], origin, cells, depth=gd, n=_MAP_N)
    return Made({}, dict(rays=lambda: dict(cells=cells.cpu().numpy(), counts=np.ascontiguousarray(got["counts"]))), call, cells.zero_, (),
                _close_all(gd, gc, pt))


CASES.append(Case("raycast", ("gpc_patches_raycast_dev",), {}, _cloud_inputs("cloud", (2, 3)), _raycast_setup, ("rays",), (True, 766), "bits",
                  {"rays.cells": ONE, "rays.counts": ONE},
                  "3000 rays from above into the map cut from the real cloud; the decoy is another cloud of the same length (src stays in "
                  "range); cells are zeroed before every run; most cells and the ray count agree between the sets, some labels (rays.cells) "
                  "and the write counts (rays.counts) must not"))


def _registration_setup(kind):
    def setup(capi, ctx, real):
        import torch
        pt, gd, gc = _map(capi, ctx)
        reg = capi.Registration(ctx, pt, gd, gc)
        prm = capi.default_params_registration(step=1e-7, tol=0.0, min_steps=2, max_steps=3)
        scan = torch.from_numpy(_plane_records(2, shift=0.004)).cuda()
        torch.cuda.synchronize()
        got = {}
        if kind == "set_cloud":
            def call(b, o):
                reg.set_cloud(b["scan"], n=_MAP_N)
            reset = None
        elif kind == "step":
            def call(b, o):
                got["out"] = reg.step(prm)
            reset = lambda: reg.set_cloud(scan, n=_MAP_N)
        else:
            def call(b, o):
                got["out"] = reg.run(prm)
            reset = lambda: reg.set_cloud(scan, n=_MAP_N)

        def read():
            d = dict(cloud=np.ascontiguousarray(reg.cloud()).view(np.uint8).reshape(-1, 32).copy())
            if "out" in got:
                d["out"] = np.ascontiguousarray(got["out"])
            return d
        return Made({}, dict(reg=read), call, reset, (), _close_all(reg, gd, gc, pt))
    return setup


CASES.append(Case("registration-set-cloud", ("gpc_registration_set_cloud_dev",), {}, _cloud_inputs("scan", (2, 3), shift=0.004),
                  _registration_setup("set_cloud"), ("reg",), False, "bits", {},
                  "rg_reset_kernel and the copy of the scan on the caller's stream; the working cloud is read back on the host"))
CASES.append(Case("registration-step", ("gpc_registration_step",), {}, _no_inputs, _registration_setup("step"), ("reg",), (True, 1003), "bits", {},
                  "assign, gather, reduce, update, transform: the nine doubles and the moved cloud; the scan is set again before every run",
                  blind="reads no caller array: its input is the object's working cloud"))
CASES.append(Case("registration-run", ("gpc_registration_run",), {}, _no_inputs, _registration_setup("run"), ("reg",), (True, 1008), "bits", {},
                  "three steps from the same start: the trace and the moved cloud",
                  blind="reads no caller array: its input is the object's working cloud"))


def _remap_setup(capi, ctx, real):
    g = _rate_object(capi, ctx)
    table = np.arange(g.P, dtype=np.int32) + 3                 # (strictly increasing: the first three patches of the new object are empty)
    box = {}

    def drop():
        if box.get("new") is not None:
            box.pop("new").close()

    def call(b, o):
        box["new"] = g.remap(g.P + 3, table)
    return Made({}, dict(new=lambda: PC._sparse_within_basis(box["new"])), call, drop, (), lambda: (drop(), g.close()))


CASES.append(Case("sparse-remap", ("gpc_sparse_remap",), {}, _no_inputs, _remap_setup, ("new",), (True, 471), "bits", {},
                  "a new object of P + 3 patches with the old ones behind three empty ones: four clears and the gather on the caller's stream, "
                  "then a synchronisation, after which the host table is the caller's again",
                  blind="takes a host table read at call time: its input is the old object's state"))


def _dirs_inputs():
    """rays straight down onto the plane's patch window, and the same rays dealt in reverse"""
    rng = np.random.default_rng(12)
    n = 391
    d = np.stack([rng.uniform(-0.12, 0.12, n), rng.uniform(-0.12, 0.12, n), -np.ones(n)], 1)
    return dict(dirs=np.ascontiguousarray(d)), dict(dirs=np.ascontiguousarray(d[::-1]))


_RENDER_ORIGIN = np.array([0.3, 0.3, 1.0])


def _render_setup(with_counts):
    def setup(capi, ctx, real):
        import ctypes as C
        pt, gd, gc = _map(capi, ctx)
        n = len(real["dirs"])
        prm = capi.default_params_render()
        org = np.ascontiguousarray(_RENDER_ORIGIN)
        counts = np.zeros(5, dtype=np.int32)

        def call(b, o):
            ctx._check(ctx.lib.gpc_patches_render_dev(ctx.h, pt.h, gd.h, gc.h, None, C.byref(prm), capi._ptr(org), capi._ptr(b["dirs"]), n,
                                                      capi._ptr(o["cloud"]), capi._ptr(o["leaf"]), capi._ptr(o["range"]), capi._ptr(o["local"]),
                                                      capi._ptr(counts) if with_counts else None))
        outs = dict(cloud=((n, 32), "uint8"), leaf=((n,), "int32"), range=((n,), "float64"), local=((n, 3), "float64"))
        states = dict(host=lambda: dict(counts=counts.copy())) if with_counts else {}
        return Made(outs, states, call, None, (), _close_all(gd, gc, pt))
    return setup


for _wc in (False, True):
    CASES.append(Case("render-counts" if _wc else "render", ("gpc_patches_render_dev",), {}, _dirs_inputs, _render_setup(_wc),
                      ("cloud", "leaf", "range", "local") + (("host",) if _wc else ()), (True, 825) if _wc else False, "bits",
                      {"leaf": ONE, "host.counts": 0.0} if _wc else {"leaf": ONE},
                      "391 rays from one metre above the plane, all hits: walk, surface solve, colours; "
                      + ("counts != NULL: the call synchronises; counts are the rays' totals, the same for the reversed rays (host.counts)" if _wc
                         else "counts == NULL: never synchronises") + "; leaf is the same leaf for many reversed rays"))


def _attrs_inputs():
    """hits on the map's leaves: leaf (shared), local coordinates in the window (values)"""
    rng = np.random.default_rng(14)
    n = 257
    leaf = rng.integers(0, 9, n).astype(np.int32)              # (the plane of 0.6 x 0.6 is cut into at least nine leaves)
    sets = [dict(leaf=leaf, local=np.ascontiguousarray(np.concatenate([rng.normal(0, 0.005, (n, 1)), rng.uniform(-0.07, 0.07, (n, 2))], 1)))
            for _ in range(2)]
    return tuple(sets)


def _attrs_setup(capi, ctx, real):
    pt, gd, gc = _map(capi, ctx)
    assert pt.view.P >= 9
    n = len(real["leaf"])
    org = np.ascontiguousarray(_RENDER_ORIGIN)

    def call(b, o):
        ctx._check(ctx.lib.gpc_patches_render_attrs_dev(ctx.h, pt.h, gd.h, n, capi._ptr(b["leaf"]), capi._ptr(b["local"]), capi._ptr(org), 0,
                                                        capi._ptr(o["sigma"]), capi._ptr(o["normal"])))
    return Made(dict(sigma=((n,), "float64"), normal=((n, 3), "float64")), {}, call, None, (), _close_all(gd, gc, pt))


CASES.append(Case("render-attrs", ("gpc_patches_render_attrs_dev",), {}, _attrs_inputs, _attrs_setup, ("sigma", "normal"), False, "bits", {},
                  "sigma and normal at 257 hits: the scattered predict and with it the fork of sp_predict_launch, a fourth way in"))


def _decode_inputs():
    """W and cells for up to 64 leaves: the decoy's masks are dealt anew"""
    sets = []
    for seed in (41, 42):
        rng = np.random.default_rng(seed)
        sets.append(dict(W=(rng.random((64, _MAP_SZ * _MAP_SZ)) < 0.9).astype(np.uint8),
                         cells=np.where(rng.random((64, _MAP_SZ * _MAP_SZ)) < 0.1, 2, 1).astype(np.uint8)))
    return tuple(sets)


def _decode_setup(capi, ctx, real):
    pt, gd, gc = _map(capi, ctx)
    v = pt.view
    P, m = v.P, v.m
    assert P <= 64
    cap = P * m

    def call(b, o):
        gd.decode_dev(gc, _MAP_RES, _MAP_SZ, b["W"], b["cells"], v.rotations, v.means, v.rgb_means, cap, o["cloud"], leaf=o["leaf"], point=o["point"],
                      count=o["count"], n_points=o["n_points"])
    outs = dict(cloud=((cap, 32), "uint8"), leaf=((cap,), "int32"), point=((cap,), "int32"), count=((P,), "int32"), n_points=((1,), "int32"))
    return Made(outs, {}, call, None, (), _close_all(gd, gc, pt))


CASES.append(Case("decode", ("gpc_sparse_decode_dev",), {}, _decode_inputs, _decode_setup, ("cloud", "leaf", "point", "count", "n_points"), False, "bits",
                  {"leaf": ONE, "point": ONE, "n_points": 0.0},
                  "count, scan, emit on the map's own frames with a capacity of every cell; four cells of five hold data, so records, "
                  "leaf and point are compacted and other masks move them behind the first gap (leaf less than half: long runs of one "
                  "leaf); n_points is one number, which two masks may share"))


# ---- the hinted split ---------------------------------------------------------------------------------------------------------------------------

_HINT_N = 6600                 # (leaves of 235 .. 290 points: all three size classes)


def _hint_inputs():
    import variance_cases as VC
    sets = []
    for seed in (71, 72):
        rng = np.random.default_rng(seed)
        xs0, xs1 = VC.xstar(17, seed=seed)
        sets.append(dict(y=rng.normal(0.0, 0.01, (1, _HINT_N)), xs0=xs0, xs1=xs1))      # (one target per point of the CLOUD: the batch holds fewer)
    return tuple(sets)


def _hint_setup(capi, ctx, real):
    import variance_cases as VC
    box = {}
    prm = capi.default_params_dense(sigmaf_sq=VC.DEFAULT[0], l_sq=VC.DEFAULT[1], noise=VC.DEFAULT[2])

    import torch
    d_cloud = torch.from_numpy(_plane_records(5, n=_HINT_N, extent=0.75)).cuda()
    torch.cuda.synchronize()

    def cut():                                                  # (gpc_project_cloud_dev anew before every run: the hint is the context's LAST cut)
        if box.get("pt") is not None:
            box.pop("pt").close()
        box["pt"] = ctx.project_cloud(d_cloud, _MAP_RES, _MAP_SZ, n=_HINT_N)
    cut()
    v = box["pt"].view
    P, N = v.P, v.n_total
    cnt = np.diff(box["pt"].fetch()["off"])
    assert N <= _HINT_N and cnt.max() > 272 and cnt.min() <= 256, (cnt.min(), cnt.max())

    def call(b, o):
        w = box["pt"].view
        ctx.dense_fit_predict_dev(prm, w.P, w.off, w.n_max, w.n_total, w.x0, w.x1, b["y"], 1, 17, b["xs0"], b["xs1"], o["f"], None, o["alpha"],
                                  o["status"])
    return Made(dict(f=((P, 1, 17), "float64"), alpha=((1, N), "float64"), status=((P,), "int32")), {}, call, cut, ("dense_mfma_big",),
                lambda: box["pt"].close())


CASES.append(Case("dense-split-hinted", ("gpc_dense_fit_predict_dev",), {"GPC_NO_W1": "1"}, _hint_inputs, _hint_setup, ("f", "alpha", "status"), False,
                  "RUN_TOL", {"status": 0.0},
                  "off, x0 and x1 are the cutter's own arrays on this context, cut anew before every run: the class launches are sized by "
                  "the producer's hint and an overflow launch of the generic kernel follows each; register classes: RUN_TOL; " + _STATUS))


# ---- entries without a stream case ------------------------------------------------------------------------------------------------------------

# entry -> why the gated protocol cannot tell anything about it (true of its code)
EXEMPT = {
    "gpc_patches_view_dev": "launches nothing: copies the view struct of the batch on the host",
    "gpc_registration_cloud_dev": "launches nothing: returns the address and the count of the working cloud",
}


def entries_with_a_case():
    return {e for c in CASES for e in c.entries}
