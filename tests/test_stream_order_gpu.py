"""The stream contract of the _dev entries (include/gpc.h; DESIGN.md, "The stream contract"): one test per record of stream_cases.CASES
and per caller's stream (test_stream_order_cpu.py holds the table against the header).

The caller's stream S is a torch.cuda.Stream() ("side") or HIP's default stream, handle 0, the value Context.set_stream documents
("default").  The context's OWN stream cannot be gated from outside: its handle is not exported, so nothing can be put ahead of a call
on it.  It is the stream of every other GPU test of the suite.

Protocol for one case:
  1. Reference (module fixture, context on its own stream, everything synchronised): `call` on the real inputs, `call` on the decoy
     inputs.  The workspace has grown and the kernels are loaded.  Every output must differ between the two in more than half of its
     elements by bits (an integer output may state a smaller share in the table, with its reason): a decoy that cannot change an output
     would make the case blind.
  2. Gated run.  The input buffers hold the decoy, the outputs the sentinel (a NaN no arithmetic produces, or -7).  On S, in this order:
     the gate and the event g_end behind it; copies of the real inputs into the input buffers; `call`; copies of every output into
     snapshot buffers; copies of the decoy back over the input buffers.  Then S is synchronised.  The snapshots must equal the real
     reference by the case's rule.  A fork that does not wait for S, or a launch on another stream, reads the decoy; a missing join
     leaves the sentinel in the snapshot, or reads the decoy that came back.
  3. Validity.  g_end.query() is False right before `call`; and right after `call` returned, for the entries documented as never
     synchronising.  A run whose gate ended too early FAILS and says so.
  4. The gated run is repeated at once on the same context: events and workspace are reused.

The gate is a chain of fp64 torch.matmul on S.  Its length is measured, not assumed: the fixture times one matmul with stream events,
times -- with time.perf_counter, ungated -- how long the input copies and the warm `call` of every never-synchronising case take to
return, and repeats the matmul until the gate lasts at least GATE_FACTOR times the longest of them."""
import contextlib
import math
import os
import time

import numpy as np
import pytest

import poison_cases as PC
import stream_cases as SC
from test_dense_ev_gpu import RUN_TOL

pytestmark = pytest.mark.gpu

GATE_N = 2048             # the gate's matrices
GATE_FACTOR = 20          # the gate lasts this many times the longest return time: a slow host, a first-use module load
GATE_MIN = 8


@contextlib.contextmanager
def _env(case):
    """the case's switches and no other of SC.SWITCHES, put back afterwards"""
    saved = {k: os.environ.get(k) for k in SC.SWITCHES}
    try:
        for k in SC.SWITCHES:
            os.environ.pop(k, None)
        os.environ.update(case.env)
        yield
    finally:
        for k, v in saved.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def _t(a):
    import torch
    return torch.from_numpy(np.array(a, order="C")).cuda()          # (a copy: the case modules hand out read-only arrays)


def _fill(t):
    """the sentinel of the tensor's type in every element"""
    import torch
    name = str(t.dtype).replace("torch.", "")
    v = SC.SENTINEL[name]
    if name == "float64":
        t.view(torch.int64).fill_(v)
    elif name == "float32":
        t.view(torch.int32).fill_(v)
    elif name == "uint16":
        t.view(torch.int16).fill_(v - 65536)
    else:
        t.fill_(v)


def _sentinel_like(a):
    word = {8: np.uint64, 4: np.uint32, 2: np.uint16, 1: np.uint8}[a.dtype.itemsize]
    return np.full(a.shape, SC.SENTINEL[str(a.dtype)] & (2 ** (8 * a.dtype.itemsize) - 1), dtype=word).view(a.dtype)


def _elements(a):
    """the array as rows of bytes, one per element; a 2-D uint8 array is an array of records"""
    a = np.ascontiguousarray(a)
    if a.dtype == np.uint8 and a.ndim == 2:
        return a
    return a.reshape(-1).view(np.uint8).reshape(a.size, a.itemsize)


def _differ(a, b):
    return np.any(_elements(a) != _elements(b), axis=1)


class Rig:
    pass


class Prepared:
    pass


def _read(p):
    """every output of the case on the host (the caller has synchronised)"""
    out = {k: t.cpu().numpy() for k, t in p.outs.items()}
    for name, g in p.made.states.items():
        for k, v in _state(g).items():
            out[name + "." + k] = np.asarray(v)
    return out


def _state(g):
    """a Sparse as poison_cases reads it, or the case's own reader of an object it makes anew before every run"""
    return g() if callable(g) else PC._sparse_within_basis(g)


def _plain(rig, p, which):
    """`call` on one input set with everything synchronised around it"""
    import torch
    for k, b in p.bufs.items():
        if k in p.varying:
            b.copy_(which[k])
    for t in p.outs.values():
        _fill(t)
    if p.made.reset:
        p.made.reset()
    torch.cuda.synchronize()
    rig.ctx.synchronize()
    p.made.call(p.bufs, p.outs)
    rig.ctx.synchronize()
    torch.cuda.synchronize()
    return _read(p)


def _prepare(rig, case):
    import torch
    p = Prepared()
    real, decoy = case.inputs()
    bad = SC.same_index_arrays(real, decoy, case.blind)
    assert bad is None, (case.id, bad)
    with _env(case):
        p.made = case.setup(rig.capi, rig.ctx, real)
        rig.ctx.synchronize()
        assert set(p.made.outs) | set(p.made.states) == set(case.outputs), case.id
        p.varying = [k for k in real if real[k] is not decoy[k]]
        p.d_real = {k: _t(real[k]) for k in real}
        p.d_decoy = {k: (_t(decoy[k]) if k in p.varying else p.d_real[k]) for k in real}
        p.bufs = {k: (p.d_real[k].clone() if k in p.varying else p.d_real[k]) for k in real}
        p.outs = {k: torch.empty(shape, dtype=getattr(torch, dt), device="cuda") for k, (shape, dt) in p.made.outs.items()}
        p.snaps = {k: torch.empty_like(t) for k, t in p.outs.items()}
        p.ref = _plain(rig, p, p.d_real)
        for sub in p.made.kernel:
            assert sub in rig.ctx.last_dense_kernel(), (case.id, rig.ctx.last_dense_kernel(), sub)
        p.ref_decoy = _plain(rig, p, p.d_decoy)
        # a decoy that cannot change an output would make the case blind; nor may an output keep its sentinel
        for k, a in p.ref.items():
            if a.shape != p.ref_decoy[k].shape:                 # (a batch the library sized from the data: another size altogether)
                continue
            d = _differ(a, p.ref_decoy[k])
            if "." in k and k.split(".")[1] != "b":          # a state array: its elements are those within either basis
                d = d[np.any(_elements(a) != 0, axis=1) | np.any(_elements(p.ref_decoy[k]) != 0, axis=1)]
            share = float(np.mean(d)) if d.size else 0.0
            floor = 0.0 if case.blind else case.share.get(k)          # (a blind case has no decoy: both runs are the same run)
            assert (share > 0.5) if floor is None else (share >= floor), \
                "%s: output %s differs between the real and the decoy inputs in %.3f of its elements" % (case.id, k, share)
            if floor is not None and not case.blind:
                assert np.issubdtype(a.dtype, np.integer), (case.id, k)
            if k in p.outs:
                left = float(np.mean(~_differ(a, _sentinel_like(a))))
                assert left < 0.5, "%s: output %s keeps its sentinel in %.3f of its elements" % (case.id, k, left)
        # how long the copies and the warm call take to return, ungated
        p.t_return = 0.0
        if not case.syncs:
            for _ in range(2):
                if p.made.reset:
                    p.made.reset()
                torch.cuda.synchronize()
                rig.ctx.synchronize()
                t0 = time.perf_counter()
                for k in p.varying:
                    p.bufs[k].copy_(p.d_real[k], non_blocking=True)
                p.made.call(p.bufs, p.outs)
                p.t_return = max(p.t_return, time.perf_counter() - t0)
                rig.ctx.synchronize()
                torch.cuda.synchronize()
    return p


@pytest.fixture(scope="module")
def rig():
    import torch
    from gp_compressor_amd import capi
    capi.load()          # raises if the HIP library is missing: no fallback
    r = Rig()
    r.capi, r.ctx = capi, capi.Context(0)
    g = torch.Generator(device="cuda").manual_seed(5)
    r.A = torch.rand((GATE_N, GATE_N), dtype=torch.float64, device="cuda", generator=g) / GATE_N      # (row sums below 1: stays finite)
    r.B0 = torch.rand_like(r.A)                         # the chain shrinks B: every gate starts from this copy, as the timed one does
    r.B, r.C = r.B0.clone(), torch.empty_like(r.A)
    r.prepared, r.errors = {}, {}
    for case in SC.CASES:
        try:
            r.prepared[case.id] = _prepare(r, case)
        except Exception as e:                            # (reported by the case's own tests)
            r.errors[case.id] = e
    # one matmul of the gate, by stream events
    side = torch.cuda.Stream()
    r.B.copy_(r.B0)
    torch.cuda.synchronize()
    with torch.cuda.stream(side):
        for _ in range(3):
            torch.mm(r.A, r.B, out=r.C)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(side)
        for _ in range(10):
            torch.mm(r.A, r.B, out=r.C)
            torch.mm(r.A, r.C, out=r.B)
        e1.record(side)
    side.synchronize()
    r.t_mm = e0.elapsed_time(e1) * 1e-3 / 20
    r.t_return, r.slowest = max([(p.t_return, cid) for cid, p in r.prepared.items()] + [(0.0, "-")])
    r.count = max(GATE_MIN, int(math.ceil(GATE_FACTOR * r.t_return / r.t_mm)))
    r.count += r.count & 1
    print("\nstream gate: one fp64 matmul of %d^2 takes %.3f ms; the longest return of the copies and a warm call is %.3f ms (%s); "
          "%d matmuls: a gate of %.1f ms" % (GATE_N, r.t_mm * 1e3, r.t_return * 1e3, r.slowest, r.count, r.count * r.t_mm * 1e3))
    yield r
    torch.cuda.synchronize()
    for p in r.prepared.values():
        p.made.close()
    r.ctx.close()


def _compare(case, label, got, want, decoy):
    for k, w in want.items():
        a = got[k]
        assert a.shape == w.shape and a.dtype == w.dtype, (case.id, label, k)
        if case.rule == "bits" or not np.issubdtype(w.dtype, np.floating):
            bad = _differ(a, w)
        else:
            # (as test_poison_gpu._same: RUN_TOL of max|plain| on the finite values, the non-finite ones in the same places -- and no
            # sentinel among them)
            fin = np.isfinite(w)
            scale = float(np.max(np.abs(w[fin]))) if fin.any() else 0.0
            with np.errstate(invalid="ignore"):
                close = fin & np.isfinite(a) & (np.abs(a - w) <= RUN_TOL * scale)
            nans = np.isnan(a) & np.isnan(w) & _differ(a, _sentinel_like(a)).reshape(w.shape)
            bad = ~(close | nans | ~_differ(a, w).reshape(w.shape)).reshape(-1)
        if bad.any():
            sent = ~_differ(a, _sentinel_like(a)) if "." not in k else np.zeros(bad.shape, bool)
            as_decoy = ~_differ(a, decoy[k])
            raise AssertionError("%s [%s] output %s: %d of %d elements are not the plain run's, the first at %d; of those %d hold the "
                                 "sentinel (a join is missing) and %d the decoy run's value (the work ran before its inputs came, or "
                                 "after they went)" % (case.id, label, k, int(bad.sum()), bad.size, int(np.flatnonzero(bad)[0]),
                                                       int((bad & sent.reshape(-1)).sum()), int((bad & as_decoy.reshape(-1)).sum())))


def _gated(rig, case, p, S, label):
    """one gated run on stream S, which the context has been switched to"""
    import torch
    for k in p.varying:
        p.bufs[k].copy_(p.d_decoy[k])
    for t in list(p.outs.values()) + list(p.snaps.values()):
        _fill(t)
    rig.B.copy_(rig.B0)
    torch.cuda.synchronize()
    if p.made.reset:
        p.made.reset()
    rig.ctx.synchronize()
    torch.cuda.synchronize()
    g_end = torch.cuda.Event()
    with torch.cuda.stream(S):
        for _ in range(rig.count // 2):
            torch.mm(rig.A, rig.B, out=rig.C)
            torch.mm(rig.A, rig.C, out=rig.B)
        g_end.record(S)
        for k in p.varying:
            p.bufs[k].copy_(p.d_real[k], non_blocking=True)
        before = g_end.query()
        p.made.call(p.bufs, p.outs)
        after = g_end.query()
        for k, t in p.outs.items():
            p.snaps[k].copy_(t, non_blocking=True)
        for k in p.varying:
            p.bufs[k].copy_(p.d_decoy[k], non_blocking=True)
    S.synchronize()
    got = {k: t.cpu().numpy() for k, t in p.snaps.items()}
    rig.ctx.synchronize()
    torch.cuda.synchronize()
    for name, g in p.made.states.items():
        for k, v in _state(g).items():
            got[name + "." + k] = np.asarray(v)
    ms = rig.count * rig.t_mm * 1e3
    assert not before, "%s [%s]: the gate (%.1f ms) had ended before the call was made: the run shows nothing" % (case.id, label, ms)
    if not case.syncs:
        assert not after, ("%s [%s]: the gate (%.1f ms) had ended when the call returned: the entry waited for the stream, which the "
                           "header says it never does -- or the gate was too short, and the run shows nothing" % (case.id, label, ms))
    _compare(case, label, got, p.ref, p.ref_decoy)
    return got


def _stream(which):
    import torch
    S = torch.cuda.Stream() if which == "side" else torch.cuda.default_stream()
    assert (S.cuda_stream == 0) == (which == "default")
    return S


def _prepared(rig, case):
    if case.id in rig.errors:
        raise rig.errors[case.id]
    return rig.prepared[case.id]


@pytest.mark.parametrize("which", ["side", "default"])
@pytest.mark.parametrize("case", SC.CASES, ids=[c.id for c in SC.CASES])
def test_entry_is_ordered_on_the_callers_stream(rig, case, which):
    import torch
    p = _prepared(rig, case)
    S = _stream(which)
    t0 = time.time()
    with _env(case):
        rig.ctx.synchronize()
        rig.ctx.set_stream(S.cuda_stream)
        try:
            first = _gated(rig, case, p, S, which + ", first run")
            second = _gated(rig, case, p, S, which + ", second run")
        finally:
            torch.cuda.synchronize()
            rig.ctx.synchronize()
            rig.ctx.set_stream(None)
    if case.rule == "bits":
        for k in first:
            assert first[k].tobytes() == second[k].tobytes(), (case.id, k)
    print("%s on the %s stream: gate of %d matmuls (%.1f ms), this case's copies and call return in %.3f ms; two gated runs %.2f s"
          % (case.id, which, rig.count, rig.count * rig.t_mm * 1e3, p.t_return * 1e3, time.time() - t0))


def test_gate_is_long_enough(rig):
    """the figures of DESIGN.md: the gate covers GATE_FACTOR return times of the slowest case"""
    assert not rig.errors, sorted(rig.errors)
    assert rig.t_mm > 0 and rig.count * rig.t_mm >= GATE_FACTOR * rig.t_return
    print("one matmul %.3f ms, longest return %.3f ms (%s), %d matmuls" % (rig.t_mm * 1e3, rig.t_return * 1e3, rig.slowest, rig.count))


@pytest.mark.parametrize("one_stream", [False, True], ids=["two-stream", "GPC_HOST_ONE_STREAM"])
def test_host_entry_behind_a_gated_dev_call(rig, one_stream):
    """mixed entries on one context: a gated gpc_dense_fit_predict_dev on the one-wave route, whose factors live in the workspace, and at
    once the host-pointer gpc_dense_fit_predict of another batch, whose pipeline has streams of its own and the same workspace
    (gpc_ws_reserve, gpc_pipe_chunk_order).  Both results are their plain runs'."""
    import torch
    from gp_compressor_amd import synth
    case = next(c for c in SC.CASES if c.id == "dense-one-wave-var")
    p = _prepared(rig, case)
    # (poison_cases._dense_host: more than 2048 patches are cut into chunks, which is where the pipeline forks; patches of at most 32
    # points go to the register kernel, hence RUN_TOL below)
    batch = synth.make_patches(2100, 32, res=0.15, seed=91, ragged=True)
    prm = rig.capi.default_params_dense()
    run_host = lambda: rig.ctx.dense_fit_predict_grid(prm, *batch, 0.15, 10, want_alpha=True)
    S = torch.cuda.Stream()
    with _env(case):
        if one_stream:
            os.environ["GPC_HOST_ONE_STREAM"] = "1"
        rig.ctx.synchronize()
        plain = run_host()
        assert np.all(plain[1] == 0)
        dev_call = p.made.call
        host = []
        try:
            rig.ctx.set_stream(S.cuda_stream)
            p2 = Prepared()
            p2.__dict__.update(p.__dict__)
            p2.made = p.made._replace(call=lambda b, o: (dev_call(b, o), host.append(run_host())))
            # (the host entry is synchronous: the second query of the event is not made)
            _gated(rig, case._replace(syncs=(True, 0)), p2, S, "dev call, then the host entry")
        finally:
            torch.cuda.synchronize()
            rig.ctx.synchronize()
            rig.ctx.set_stream(None)
    assert len(host) == 1
    for name, a, w in zip(("f", "status", "alpha"), host[0], plain):
        if name == "status":
            assert np.array_equal(a, w)
            continue
        err, scale = float(np.max(np.abs(a - w))), float(np.max(np.abs(w)))
        print("host entry behind a gated _dev call, %s: max difference %.3e of %.3e" % (name, err, scale))
        assert np.all(np.isfinite(a)) and err <= RUN_TOL * scale, "the host entry's %s differs from its plain run behind a gated _dev call" % name


@pytest.mark.parametrize("which", ["side", "default"])
def test_chain_under_one_gate(rig, which):
    """gpc_project_cloud_dev, then -- behind ONE gate, nothing synchronised in between -- gpc_sparse_add_dev for depth and for colour on
    the batch's own arrays, gpc_sparse_predict_dev with sigma and for the colours, gpc_reproject_dev; the outputs are copied off on the
    stream at once.  They must be those of the same chain synchronised after every call.  (The cutter synchronises, so the gate stands
    behind it: the cloud arrives on the stream ahead of the cutter, and is overwritten behind it.)"""
    import torch
    import decode_cases as DC
    capi, ctx = rig.capi, rig.ctx
    d_real, d_decoy = (torch.from_numpy(SC._plane_records(s)).cuda() for s in (2, 3))
    buf = d_decoy.clone()
    xs0, xs1 = (torch.from_numpy(np.ascontiguousarray(a)).cuda() for a in DC.grid_points(SC._MAP_RES, SC._MAP_SZ))
    m = SC._MAP_SZ * SC._MAP_SZ
    kw = dict(sigmaf_sq=1.0, l_sq=(SC._MAP_RES / 5) ** 2)
    pd, pc = capi.default_params_sparse(1, noise=1e-3, capacity=24, **kw), capi.default_params_sparse(3, noise=1.0, capacity=100, **kw)
    S = _stream(which)

    def chain(gated):
        made = []
        sync = (lambda: None) if gated else ctx.synchronize
        try:
            buf.copy_(d_decoy)
            torch.cuda.synchronize()
            with torch.cuda.stream(S):
                buf.copy_(d_real, non_blocking=True)
                pt = ctx.project_cloud(buf, SC._MAP_RES, SC._MAP_SZ, n=SC._MAP_N)          # (synchronises)
                made.append(pt)
                buf.copy_(d_decoy, non_blocking=True)
            v = pt.view
            P = v.P
            gd, gc = capi.Sparse(ctx, pd, P, 1), capi.Sparse(ctx, pc, P, 3)
            made[:0] = [gd, gc]
            o = dict(f=torch.empty((P, 1, m), dtype=torch.float64, device="cuda"), sigma=torch.empty((P, m), dtype=torch.float64, device="cuda"),
                     c=torch.empty((P, 3, m), dtype=torch.float64, device="cuda"), cloud=torch.empty((P * m, 32), dtype=torch.uint8, device="cuda"),
                     n_points=torch.empty((1,), dtype=torch.int32, device="cuda"))
            snaps = {k: torch.empty_like(t) for k, t in o.items()}
            for t in list(o.values()) + list(snaps.values()):
                _fill(t)
            rig.B.copy_(rig.B0)
            torch.cuda.synchronize()
            ctx.synchronize()
            g_end = torch.cuda.Event()
            with torch.cuda.stream(S):
                if gated:
                    for _ in range(rig.count // 2):
                        torch.mm(rig.A, rig.B, out=rig.C)
                        torch.mm(rig.A, rig.C, out=rig.B)
                g_end.record(S)
                before = g_end.query()
                gd.add_dev(v.off, v.n_max, v.n_total, v.x0, v.x1, v.y)
                sync()
                gc.add_dev(v.off, v.n_max, v.n_total, v.x0, v.x1, v.rgb)
                sync()
                gd.predict_dev(m, xs0, xs1, o["f"], o["sigma"])
                sync()
                gc.predict_dev(m, xs0, xs1, o["c"])
                sync()
                ctx.reproject_dev(P, m, None, xs0, xs1, o["f"], o["c"], v.rotations, v.means, v.rgb_means, o["cloud"], o["n_points"])
                after = g_end.query()
                sync()
                for k, t in o.items():
                    snaps[k].copy_(t, non_blocking=True)
            S.synchronize()
            if gated:
                assert not before and not after, "the gate (%d matmuls) had ended before the chain was enqueued: the run shows nothing" % rig.count
            return {k: t.cpu().numpy() for k, t in snaps.items()}
        finally:
            torch.cuda.synchronize()
            ctx.synchronize()
            for x in made:
                x.close()

    ctx.synchronize()
    ctx.set_stream(S.cuda_stream)
    try:
        want = chain(False)
        assert int(want["n_points"][0]) == want["cloud"].shape[0] > 0
        for rep in ("first", "second"):
            got = chain(True)
            for k, w in want.items():
                bad = _differ(got[k], w)
                assert not bad.any(), ("chain under one gate, %s run on the %s stream: %d of %d elements of %s are not the synchronised chain's, "
                                       "%d of them hold the sentinel" % (rep, which, int(bad.sum()), bad.size, k,
                                                                         int((bad & ~_differ(got[k], _sentinel_like(got[k]))).sum())))
    finally:
        torch.cuda.synchronize()
        ctx.synchronize()
        ctx.set_stream(None)


def test_switching_streams_behind_a_synchronise(rig):
    """gpc_ctx_set_stream only swaps the handle (include/gpc.h): the documented sequence is a call on S1, gpc_ctx_synchronize, set_stream(S2),
    a call on S2 -- both gated, both right, on the forked sparse predict that shares events and the two side streams between them"""
    import torch
    case = next(c for c in SC.CASES if c.id == "sparse-predict-points")
    p = _prepared(rig, case)
    S1, S2 = torch.cuda.Stream(), torch.cuda.Stream()
    with _env(case):
        rig.ctx.synchronize()
        try:
            rig.ctx.set_stream(S1.cuda_stream)
            a = _gated(rig, case, p, S1, "S1")
            rig.ctx.synchronize()
            rig.ctx.set_stream(S2.cuda_stream)
            b = _gated(rig, case, p, S2, "S2 after synchronize and set_stream")
            rig.ctx.synchronize()
            rig.ctx.set_stream(0)
            c = _gated(rig, case, p, torch.cuda.default_stream(), "default stream after synchronize and set_stream")
        finally:
            torch.cuda.synchronize()
            rig.ctx.synchronize()
            rig.ctx.set_stream(None)
    for k in a:
        assert a[k].tobytes() == b[k].tobytes() == c[k].tobytes(), k
