"""GPU tests of the argument rules and the staging of the gpc_sparse_* entries (include/gpc.h): what every entry rejects, with which
code, in its host form and in its _dev form, written here as literal tables, and that the host twin of each of the ten staged pairs
leaves the bytes of its _dev twin in every output and in the object.  Everything goes through the C-ABI with explicit NULLs; nothing is
compared against a tolerance.

Objects: P = 4 patches of 0, 1, 5 and 20 points at capacity 8 (gpc_sparse_ld 16) -- an empty patch, a one-point patch, a patch above
the capacity, so that deletions happen -- as a Gaussian object with ny = 1, one with ny = 3 and a probit object (noise_model 2); and
objects of P = 0.  Data: gp_compressor_amd/synth.py."""
import ctypes as C
import types

import numpy as np
import pytest

from gp_compressor_amd import synth

pytestmark = pytest.mark.gpu

E, R, OK = -22, -34, 0      # GPC_EINVAL, GPC_ERANGE, GPC_OK (include/gpc.h)
COUNTS = (0, 1, 5, 20)
RES, CAP, LD = 0.15, 8, 16
M, K, MAXC = 3, 7, 3        # grid points of predict, entries of predict_scattered, max_counter of train_sigmaf
INF, NAN = float("inf"), float("nan")

# entry -> (the arguments of the host form, (the argument the extra ones of the _dev form follow, those), the outputs)
PAIRS = {
    "add": ("g off x0 x1 third perm status", ("off", "n_max n_total"), "status"),
    "predict": ("g m x0 x1 third sigma conf status", None, "third sigma status"),
    "predict_points": ("g off x0 x1 third sigma conf status", ("off", "n_total"), "third sigma status"),
    "predict_scattered": ("g n patch x0 x1 stride f sigma conf status", None, "f sigma status"),
    "likelihood": ("g off x0 x1 third dX l", ("off", "n_total"), "dX l"),
    "train_sigmaf": ("g off x0 x1 third step max_counter p0 iters ls delta", ("off", "n_total"), "p0 iters ls delta"),
    "prune": ("g keep target score_tol removed order scores status", None, "removed order scores status"),
    "prune_rd": ("g off x0 x1 third keep target max_mse max_mse_p removed order scores mse mse0 mse_next status", ("off", "n_total"),
                 "removed order scores mse mse0 mse_next status"),
    "quantize_rd": ("g off x0 x1 third bits_min bits_max max_mse max_mse_p bits q_alpha q_bv range mse0 mse_q curve status",
                    ("off", "n_total"), "bits q_alpha q_bv range mse0 mse_q curve status"),
    "dequantize": ("g bv_count bits q_alpha q_bv range", None, ""),
}
# the entries with one form (host pointers)
SINGLES = {
    "reset": ("g", None, ""),
    "set_trace": ("g trace", None, ""),
    "sizes": ("g bv_count", None, "bv_count"),
    "get_state": ("g alpha C Q BV", None, "alpha C Q BV"),
    "set_state": ("g bv_count alpha C Q BV", None, ""),
}
ENTRIES = dict(PAIRS, **SINGLES)
I32 = ("off", "perm", "patch", "target", "status", "iters", "removed", "order", "bits", "bv_count")
DTYPE = dict({k: np.int32 for k in I32}, q_alpha=np.uint16, q_bv=np.uint16, range=np.float32)
SENTINEL = {np.int32: -7, np.uint16: 0xABCD, np.float32: -12345.5, np.float64: -12345.5}
DUMMY = np.zeros(8, dtype=np.uint8)      # what an array of no elements points at: never NULL


def _sig(entry, dev):
    host, extra, _ = ENTRIES[entry]
    names = host.split()
    if dev and extra:
        at = names.index(extra[0]) + 1
        names[at:at] = extra[1].split()
    return names


def _forms(entry):
    return (False, True) if entry in PAIRS else (False,)


def _outs(entry):
    return ENTRIES[entry][2].split()


def _dtype(name):
    return DTYPE.get(name, np.float64)


def _batch(ny, probit=False, counts=COUNTS, seed=11):
    """the ragged batch: every patch its own make_patches call, so that a patch's data does not depend on the others"""
    parts = [synth.make_patches(1, n, res=RES, seed=seed + i, ny=ny) for i, n in enumerate(counts) if n > 0]
    off = np.zeros(len(counts) + 1, dtype=np.int32)
    off[1:] = np.cumsum(counts)
    cat = lambda k, ax: np.ascontiguousarray(np.concatenate([p[k] for p in parts], axis=ax)) if parts else np.zeros((ny, 0) if k == 3 else 0)
    x0, x1, y = cat(1, 0), cat(2, 0), cat(3, 1)
    if probit:
        y = synth.occupancy_labels(off, y[0])[None, :]
    perm = synth.sattolo_perms(off, seed=5) if parts else np.zeros(0, dtype=np.int32)
    return dict(off=off, x0=x0, x1=x1, y=np.ascontiguousarray(y), perm=perm)


def _values(o, entry):
    """valid arguments of an entry on the object o, by name (arrays as numpy arrays, None: NULL)"""
    b, P, ny, N = o.batch, o.P, o.ny, o.N
    v = dict(g=o.h, off=b["off"], n_max=int(np.max(np.diff(b["off"]))) if P else 0, n_total=N, x0=b["x0"], x1=b["x1"], third=b["y"], perm=b["perm"],
             conf=0, m=M, n=K, stride=1, step=float(np.float32(1e-4)), max_counter=MAXC, keep=2, target=None, score_tol=0.0, max_mse=INF,
             max_mse_p=None, bits_min=5, bits_max=9, trace=None)
    rng = np.random.default_rng(3)
    if entry == "predict":
        v["x0"], v["x1"] = rng.uniform(-RES / 2, RES / 2, size=(2, M))
    if entry == "predict_scattered":
        # patch 3 twice, a miss on either side of the range, every other patch once
        v["patch"] = np.array([3, -1, 2, 3, 4, 1, 0], dtype=np.int32)
        v["x0"], v["x1"] = rng.uniform(-RES / 2, RES / 2, size=(2, K))
    if entry == "dequantize":
        v.update(o.codes)
    if entry == "set_state":
        v.update(o.saved)
    return v


def _shape(o, entry, k, v):
    P, ny, ld, N = o.P, o.ny, LD, o.N
    own = {"predict": dict(third=(P, ny, M), sigma=(P, M)), "predict_points": dict(third=(ny, N), sigma=(N,)),
           "predict_scattered": dict(f=(ny, K), sigma=(K,))}.get(entry, {})
    if k in own:
        return own[k]
    W = max(int(v["max_counter"]), 0) + 2
    return dict(status=(P,), dX=(N, 3), l=(N,), p0=(P,), iters=(P,), ls=(P, W), delta=(P, 2), removed=(P,), order=(P, ld), scores=(P, ld),
                mse=(P, ld), mse0=(P,), mse_next=(P,), bits=(P,), q_alpha=(P, ny, ld), q_bv=(P, ld, 2), range=(P, ny + 2, 2), mse_q=(P,),
                curve=(P, 16), bv_count=(P,), alpha=(P, ny, ld), C=(P, ld, ld), Q=(P, ld, ld), BV=(P, ld, 2))[k]


def _mark(gp, entry):
    """leaves a known text in the context, so that a call's own text can be told from an older one"""
    if entry == "sizes":
        tmp = C.c_void_p()
        assert gp.lib.gpc_sparse_create(gp.ctx.h, None, 1, 1, C.byref(tmp)) == E
    else:
        assert gp.lib.gpc_sparse_sizes(gp.marker, None) == E
    return gp.lib.gpc_last_error(gp.ctx.h).decode()


def _call(gp, o, entry, dev, change=None, null=()):
    """One call of an entry through the C-ABI: host arrays or (dev) device buffers, every output pre-filled with its sentinel; `change`
    replaces arguments by name (None: NULL; ("@", name, bytes): an address inside the array `name`), the outputs in `null` are NULL.
    Returns (rc, the outputs as numpy arrays, the error text, the text that was there before)."""
    torch = gp.torch
    change = dict(change or {})
    v = _values(o, entry)
    v.update(change)
    outs = {}
    for k in _outs(entry):
        if k in null or (k in change and change[k] is None):
            v[k] = None
        else:
            dt = _dtype(k)
            v[k] = outs[k] = np.full(_shape(o, entry, k, v), SENTINEL[dt], dtype=dt)
    on_dev = dev and entry in PAIRS
    tensors, address = {}, {}
    for k, a in v.items():
        if isinstance(a, np.ndarray):
            a = np.ascontiguousarray(a, dtype=_dtype(k))
            if k not in outs:
                v[k] = a
            flat = a.reshape(-1).view(np.uint8) if a.size else DUMMY
            if on_dev:
                tensors[k] = torch.from_numpy(flat.copy()).cuda()
                address[k] = tensors[k].data_ptr()
            else:
                tensors[k] = flat
                address[k] = flat.ctypes.data
    args = []
    for k in _sig(entry, dev):
        a = v[k]
        if isinstance(a, tuple):
            a = address[a[1]] + a[2]
        elif isinstance(a, np.ndarray):
            a = address[k]
        args.append(a)
    if on_dev:
        torch.cuda.synchronize()
    before = _mark(gp, entry)
    rc = getattr(gp.lib, "gpc_sparse_" + entry + ("_dev" if dev else ""))(*args)
    if on_dev:
        gp.ctx.synchronize()
        outs = {k: tensors[k].cpu().numpy().view(a.dtype)[:a.size].reshape(a.shape) for k, a in outs.items()}
    return rc, outs, gp.lib.gpc_last_error(gp.ctx.h).decode(), before


def _written(outs):
    """the names of the outputs that no longer hold their sentinel everywhere"""
    return [k for k, a in outs.items() if not np.all(a == SENTINEL[a.dtype.type])]


def _same_bits(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def _state(gp, o):
    """the object as gpc_sparse_get_state and gpc_sparse_sizes report it"""
    s = dict(bv_count=np.zeros(o.P, dtype=np.int32), alpha=np.zeros((o.P, o.ny, LD)), C=np.zeros((o.P, LD, LD)), Q=np.zeros((o.P, LD, LD)),
             BV=np.zeros((o.P, LD, 2)))
    assert gp.lib.gpc_sparse_sizes(o.h, s["bv_count"].ctypes.data) == OK
    assert gp.lib.gpc_sparse_get_state(o.h, *(s[k].ctypes.data for k in ("alpha", "C", "Q", "BV"))) == OK
    return s


def _restore(gp, o):
    assert gp.lib.gpc_sparse_set_state(o.h, *(o.saved[k].ctypes.data for k in ("bv_count", "alpha", "C", "Q", "BV"))) == OK


def _object(gp, name, P, ny, probit=False, ctx_h=None):
    capi = gp.capi
    kw = dict(sigmaf_sq=1.0, l_sq=(RES / 4) ** 2, capacity=CAP, noise=0.25 if probit else (1e-2 if ny == 1 else 25.0), ref_field_delete_bug=0,
              noise_model=2 if probit else 0)
    h = C.c_void_p()
    assert gp.lib.gpc_sparse_create(gp.ctx.h if ctx_h is None else ctx_h, C.byref(capi.default_params_sparse(ny, **kw)), P, ny, C.byref(h)) == OK
    o = types.SimpleNamespace(name=name, h=h, P=P, ny=ny, batch=_batch(ny, probit, COUNTS if P else ()))
    o.N = int(o.batch["off"][-1])
    assert gp.lib.gpc_sparse_ld(h) == LD
    # codes that pass the rules of gpc_sparse_dequantize: no basis vector, width 5
    o.codes = dict(bv_count=np.zeros(P, dtype=np.int32), bits=np.full(P, 5, dtype=np.int32), q_alpha=np.zeros((P, ny, LD), dtype=np.uint16),
                   q_bv=np.zeros((P, LD, 2), dtype=np.uint16), range=np.zeros((P, ny + 2, 2), dtype=np.float32))
    o.saved = dict(bv_count=np.zeros(P, dtype=np.int32), alpha=np.zeros((P, ny, LD)), C=np.zeros((P, LD, LD)), Q=np.zeros((P, LD, LD)),
                   BV=np.zeros((P, LD, 2)))
    return o


@pytest.fixture(scope="module")
def gp():
    import torch
    from gp_compressor_amd import capi
    capi.load()          # raises if the HIP library is missing: no fallback
    ctx = capi.Context(0)
    gp = types.SimpleNamespace(capi=capi, ctx=ctx, lib=ctx.lib, torch=torch)
    gp.objs = {n: _object(gp, n, P, ny, pb) for n, P, ny, pb in (("g1", 4, 1, False), ("g3", 4, 3, False), ("pb", 4, 1, True),
                                                                  ("z", 0, 1, False), ("z3", 0, 3, False), ("pz", 0, 1, True))}
    gp.marker = gp.objs["g1"].h
    # the trained state every comparison starts from, and (Gaussian objects) its codes at width 5 for gpc_sparse_dequantize
    for n in ("g1", "g3", "pb"):
        o = gp.objs[n]
        rc, _, msg, _ = _call(gp, o, "add", False)
        assert rc == OK, msg
        o.saved = _state(gp, o)
        assert list(o.saved["bv_count"][:2]) == [0, 1] and (n == "pb" or o.saved["bv_count"][3] == CAP), o.saved["bv_count"]
        if n != "pb":
            rc, q, msg, _ = _call(gp, o, "quantize_rd", False)
            assert rc == OK and q["bits"][3] == 5, (msg, q["bits"])
            o.codes = dict(bv_count=o.saved["bv_count"], bits=q["bits"], q_alpha=q["q_alpha"], q_bv=q["q_bv"], range=q["range"])
    yield gp
    for o in gp.objs.values():
        gp.lib.gpc_sparse_destroy(o.h)
    ctx.close()


@pytest.fixture(autouse=True)
def _plain_env(monkeypatch):
    monkeypatch.delenv("GPC_POISON_LDS", raising=False)


# ---------------------------------------------------------------------------------------------------------------- (a) the rule table

def _off(*v):
    return np.array(v, dtype=np.int32)


def _perm_with(k, value):
    p = _batch(1)["perm"].copy()
    p[k] = value
    return p


def _codes_with(name, value):
    a = np.full(4, 5 if name == "bits" else 0, dtype=np.int32)
    a[1] = value
    return a


# fault -> (object, what changes in the call, the entries it is applied to (None: every entry that has the changed arguments), the forms
# (None: both), the code, a piece of the error text (None: the call leaves no text)).  Every other argument of a cell is valid: the fault
# is the only one.  The codes are those include/gpc.h states; where it is silent the row says so.
RULES = {
    "object NULL":             ("g1", dict(g=None), None, None, E, None),
    "off NULL":                ("g1", dict(off=None), None, None, E, "off is NULL"),
    "off[0] = 1":              ("g1", dict(off=_off(1, 1, 1, 6, 26)), None, "host", E, "off[0] must be 0"),            # from the code
    "off decreasing":          ("g1", dict(off=_off(0, 1, 0, 6, 26)), None, "host", E, "non-decreasing"),              # from the code
    "n_total -1":              ("g1", dict(n_total=-1), None, "dev", E, "negative size"),
    "n_max -1":                ("g1", dict(n_max=-1), None, "dev", E, "negative size"),
    "m -1":                    ("g1", dict(m=-1), None, None, E, "negative m"),
    "n -1":                    ("g1", dict(n=-1), None, None, E, "negative size"),
    "x0 NULL":                 ("g1", dict(x0=None), None, None, E, "is NULL"),
    "x1 NULL":                 ("g1", dict(x1=None), None, None, E, "is NULL"),
    "y / f / f_star NULL":     ("g1", dict(third=None), None, None, E, "is NULL"),
    "patch NULL":              ("g1", dict(patch=None), None, None, E, "patch/x0/x1 is NULL"),
    "perm beyond its patch":   ("g1", dict(perm=_perm_with(6, 20)), ("add",), "host", E, "perm[6] = 20 outside patch 3"),      # from the code
    "perm negative":           ("g1", dict(perm=_perm_with(1, -1)), ("add",), "host", E, "perm[1] = -1 outside patch 2"),      # from the code
    "stride 0":                ("g1", dict(stride=0), None, None, E, "stride must be >= 1"),
    "keep 0, target NULL":     ("g1", dict(keep=0), None, None, E, "keep must be >= 1"),
    "score_tol NaN":           ("g1", dict(score_tol=NAN), None, None, E, "score_tol must be >= 0"),
    "score_tol -1":            ("g1", dict(score_tol=-1.0), None, None, E, "score_tol must be >= 0"),
    "max_mse NaN":             ("g1", dict(max_mse=NAN), None, None, E, "max_mse must be >= 0"),
    "max_mse -1":              ("g1", dict(max_mse=-1.0), None, None, E, "max_mse must be >= 0"),
    "bits_min 0":              ("g1", dict(bits_min=0), None, None, E, "widths must satisfy"),
    "bits_max 17":             ("g1", dict(bits_max=17), None, None, E, "widths must satisfy"),
    "bits_min > bits_max":     ("g1", dict(bits_min=9, bits_max=8), None, None, E, "widths must satisfy"),
    "probit object":           ("pb", dict(), ("prune_rd", "quantize_rd", "likelihood", "train_sigmaf"), None, E, "Gaussian"),
    "train_sigmaf with ny 3":  ("g3", dict(), ("train_sigmaf",), None, E, "ny == 1"),                                  # from the code
    "max_counter -1":          ("g1", dict(max_counter=-1), None, None, E, "max_counter must be in [0, 10000]"),       # from the code
    "max_counter 10001":       ("g1", dict(max_counter=10001), None, None, E, "max_counter must be in [0, 10000]"),    # from the code
    "step NaN":                ("g1", dict(step=NAN), None, None, E, "step is NaN"),                                   # from the code
    "p0 NULL":                 ("g1", dict(p0=None), None, None, E, "p0/iters/ls/delta is NULL"),                      # from the code
    "iters NULL":              ("g1", dict(iters=None), None, None, E, "p0/iters/ls/delta is NULL"),                   # from the code
    "ls NULL":                 ("g1", dict(ls=None), None, None, E, "p0/iters/ls/delta is NULL"),                      # from the code
    "delta NULL":              ("g1", dict(delta=None), None, None, E, "p0/iters/ls/delta is NULL"),                   # from the code
    # gpc_sparse_dequantize, gpc_sparse_sizes, gpc_sparse_set_state
    "bv_count NULL":           ("g1", dict(bv_count=None), None, None, E, "bv_count"),
    "bits NULL":               ("g1", dict(bits=None), ("dequantize",), None, E, "bv_count/bits/q_alpha/q_bv/range is NULL"),
    "q_alpha NULL":            ("g1", dict(q_alpha=None), ("dequantize",), None, E, "bv_count/bits/q_alpha/q_bv/range is NULL"),
    "q_bv NULL":               ("g1", dict(q_bv=None), ("dequantize",), None, E, "bv_count/bits/q_alpha/q_bv/range is NULL"),
    "range NULL":              ("g1", dict(range=None), ("dequantize",), None, E, "bv_count/bits/q_alpha/q_bv/range is NULL"),
    "bits[1] 17":              ("g1", dict(bits=_codes_with("bits", 17)), ("dequantize",), "host", E, "bits[1] = 17 outside [0, 16]"),
    "bits[1] -1":              ("g1", dict(bits=_codes_with("bits", -1)), ("dequantize",), "host", E, "bits[1] = -1 outside [0, 16]"),
    "bv_count[1] 17":          ("g1", dict(bv_count=_codes_with("bv_count", 17)), ("dequantize",), "host", E, "bv_count[1] = 17 outside [0, 16]"),
    "bv_count[1] 17, state":   ("g1", dict(bv_count=_codes_with("bv_count", 17)), ("set_state",), None, R, "bv_count[1] = 17 outside [0, 16]"),  # from the code
    "bv_count[1] -1, state":   ("g1", dict(bv_count=_codes_with("bv_count", -1)), ("set_state",), None, R, "bv_count[1] = -1 outside [0, 16]"),  # from the code
    "alpha NULL":              ("g1", dict(alpha=None), ("set_state",), None, E, "bv_count/alpha/BV is NULL"),         # from the code
    "BV NULL":                 ("g1", dict(BV=None), ("set_state",), None, E, "bv_count/alpha/BV is NULL"),            # from the code
}


def _cells(only, forms, change_of):
    """the (entry, dev) pairs a row is applied to: the entries, in the forms, that have every argument the row changes"""
    want = {None: (False, True), "host": (False,), "dev": (True,)}[forms]
    for entry in ENTRIES:
        if only is not None and entry not in only:
            continue
        for dev in _forms(entry):
            if dev in want and all(k in _sig(entry, dev) for k in change_of(dev)):
                yield entry, dev


def _run_row(gp, name, obj, change_of, only, forms, code_of, text):
    """A row on all its cells: the code, the text -- set by this call, or none at all -- and no output written.  change_of, code_of: per form."""
    bad, n = [], 0
    for entry, dev in _cells(only, forms, change_of):
        rc, outs, msg, before = _call(gp, gp.objs[obj], entry, dev, change_of(dev))
        n += 1
        want = code_of(dev)
        print("cell %-24s %-18s %-4s rc %d (%s)" % (name, entry, "dev" if dev else "host", rc, msg if rc else ""))
        if rc != want:
            bad.append((entry, dev, "code", rc, want))
        elif _written(outs):
            bad.append((entry, dev, "written", _written(outs)))
        elif want != OK and (msg != before if text is None else (msg == before or text not in msg)):
            bad.append((entry, dev, "text", msg))
    assert n > 0 and not bad, bad


@pytest.mark.parametrize("fault", list(RULES))
def test_rule_table(gp, fault):
    """Every entry that has the argument, host and _dev, against one fault"""
    obj, change, only, forms, code, text = RULES[fault]
    _run_row(gp, fault, obj, lambda dev: change, only, forms, lambda dev: code, text)
    if fault == "object NULL":
        assert gp.lib.gpc_sparse_ld(None) == E
        gp.lib.gpc_sparse_destroy(None)


# ------------------------------------------------------------------------------------------------------ (b) where the twins differ today

def _nothing():
    return np.zeros(5, dtype=np.int32)


# The host twin and the _dev twin do not apply their rules in one order, and where the nothing-to-do return sits among them differs: these
# cells are what each answers TODAY.  A later change may decide them one way; until then each row is part of the entries' behaviour.
# fault -> (object, entries, what changes in the host call, in the _dev call, the host twin's code, the _dev twin's, a piece of the text)
TWINS = {
    # the noise-model rule of gpc_sparse_likelihood_dev stands before its nothing-to-do return; the host twin returns first
    "likelihood, probit, P = 0":           ("pz", ("likelihood",), dict(), dict(), OK, E, "Gaussian"),
    "likelihood, probit, no points":       ("pb", ("likelihood",), dict(off=_nothing()), dict(off=_nothing(), n_total=0), OK, E, "Gaussian"),
    "likelihood, probit, no output":       ("pb", ("likelihood",), dict(dX=None, l=None), dict(dX=None, l=None), OK, E, "Gaussian"),
    # gpc_sparse_train_sigmaf returns at P == 0 before any other rule; the _dev twin applies all of them first
    "train_sigmaf, P = 0, max_counter -1": ("z", ("train_sigmaf",), dict(max_counter=-1), dict(max_counter=-1), OK, E, "max_counter"),
    "train_sigmaf, P = 0, step NaN":       ("z", ("train_sigmaf",), dict(step=NAN), dict(step=NAN), OK, E, "step is NaN"),
    "train_sigmaf, P = 0, ny 3":           ("z3", ("train_sigmaf",), dict(), dict(), OK, E, "ny == 1"),
    "train_sigmaf, P = 0, probit":         ("pz", ("train_sigmaf",), dict(), dict(), OK, E, "Gaussian"),
    # the size rules of the _dev twins hold at P == 0 as well; the host twins take no sizes and return at P == 0
    "P = 0, n_total -1":                   ("z", None, dict(), dict(n_total=-1), OK, E, "negative size"),
    "P = 0, n_max -1":                     ("z", ("add",), dict(), dict(n_max=-1), OK, E, "negative size"),
    "P = 0, n_total 3, x0 NULL":           ("z", None, dict(), dict(n_total=3, x0=None), OK, E, "is NULL"),
    # gpc_sparse_dequantize checks the counts and widths it can read; the _dev twin cannot, and its kernel clamps them
    "dequantize, bits[1] 17":              ("g1", ("dequantize",), dict(bits=_codes_with("bits", 17)), dict(bits=_codes_with("bits", 17)), E, OK, "bits[1]"),
    "dequantize, bv_count[1] 17":          ("g1", ("dequantize",), dict(bv_count=_codes_with("bv_count", 17)), dict(bv_count=_codes_with("bv_count", 17)),
                                            E, OK, "bv_count[1]"),
}


@pytest.mark.parametrize("fault", list(TWINS))
def test_twin_differences(gp, fault):
    obj, only, host, dev, code_host, code_dev, text = TWINS[fault]
    if only is None:
        only = tuple(e for e in PAIRS if all(k in _sig(e, True) for k in dev))
    _run_row(gp, fault, obj, lambda d: dev if d else host, only, None, lambda d: code_dev if d else code_host, text)
    if obj == "g1":
        _restore(gp, gp.objs[obj])        # (the clamped codes were decoded into the object)


# ---------------------------------------------------------------------------------------------------------------- create and remap

def _params(gp, ny=1, **kw):
    return gp.capi.default_params_sparse(ny, **dict(dict(sigmaf_sq=1.0, l_sq=1e-3, capacity=CAP), **kw))


# fault -> (ny, params fields, P, the code, a piece of the text); every row: *out is NULL afterwards.  All from include/gpc.h's code
# list (GPC_EINVAL: bad argument, GPC_ERANGE: capacity > GPC_MAX_BV) and the order of gpc_sparse_create.
CREATE = {
    "P -1":              (1, dict(), -1, E, "negative P"),
    "ny 2":              (2, dict(), 4, E, "ny must be 1"),
    "ny 0":              (0, dict(), 4, E, "ny must be 1"),
    "capacity 0":        (1, dict(capacity=0), 4, E, "capacity must be > 0 or -1"),
    "capacity -2":       (1, dict(capacity=-2), 4, E, "capacity must be > 0 or -1"),
    "capacity 256":      (1, dict(capacity=256), 4, R, "capacity 256 > 255"),
    "noise_model 3":     (1, dict(noise_model=3), 4, E, "noise_model must be 0, 1 or 2"),
    "noise_model -1":    (1, dict(noise_model=-1), 4, E, "noise_model must be 0, 1 or 2"),
    "probit with ny 3":  (3, dict(noise_model=2), 4, E, "probit noise needs ny == 1"),
    "l_sq 0":            (1, dict(l_sq=0.0), 4, E, "kernel parameters out of range"),
    "sigmaf_sq 0":       (1, dict(sigmaf_sq=0.0), 4, E, "kernel parameters out of range"),
    "l_sq NaN":          (1, dict(l_sq=NAN), 4, E, "kernel parameters out of range"),
}
WILD = 0xDEAD0


def test_create_rules(gp):
    lib, ctx = gp.lib, gp.ctx
    bad = []
    for fault, (ny, kw, P, code, text) in CREATE.items():
        h = C.c_void_p(WILD)
        before = _mark(gp, "create")
        rc = lib.gpc_sparse_create(ctx.h, C.byref(_params(gp, ny if ny in (1, 3) else 1, **kw)), P, ny, C.byref(h))
        msg = lib.gpc_last_error(ctx.h).decode()
        print("create %-18s rc %d (%s)" % (fault, rc, msg))
        if rc != code or h.value is not None or msg == before or text not in msg:
            bad.append((fault, rc, h.value, msg))
    assert not bad, bad
    h = C.c_void_p(WILD)
    before = _mark(gp, "create")
    assert lib.gpc_sparse_create(None, C.byref(_params(gp)), 4, 1, C.byref(h)) == E and h.value == WILD       # no context: no text, nothing written
    assert lib.gpc_last_error(ctx.h).decode() == before
    assert lib.gpc_sparse_create(ctx.h, C.byref(_params(gp)), 4, 1, None) == E and "out is NULL" in lib.gpc_last_error(ctx.h).decode()
    assert lib.gpc_sparse_create(ctx.h, None, 4, 1, C.byref(h)) == E and h.value is None and "params is NULL" in lib.gpc_last_error(ctx.h).decode()
    # the edges that pass: capacity 255 is the largest, -1 asks for it by name; P = 0
    for kw, P, ld in ((dict(capacity=255), 1, 256), (dict(capacity=-1), 1, 256), (dict(), 0, LD)):
        assert lib.gpc_sparse_create(ctx.h, C.byref(_params(gp, **kw)), P, 1, C.byref(h)) == OK and lib.gpc_sparse_ld(h) == ld, kw
        lib.gpc_sparse_destroy(h)


# fault -> (P_new, the table (None: NULL), a piece of the text): GPC_EINVAL (include/gpc.h), *out NULL afterwards
REMAP = {
    "P_new 3 < P":         (3, _off(0, 1, 2, 3), "P_new 3 is smaller than the object's P 4"),
    "table NULL":          (6, None, "old_to_new is NULL"),
    "table not increasing": (6, _off(0, 2, 2, 3), "old_to_new[2] = 2"),
    "table decreasing":    (6, _off(0, 3, 2, 5), "old_to_new[2] = 2"),
    "entry negative":      (6, _off(-1, 1, 2, 3), "old_to_new[0] = -1"),
    "entry 6 = P_new":     (6, _off(0, 1, 2, 6), "old_to_new[3] = 6"),
}


def test_remap_rules(gp):
    lib, ctx, g1 = gp.lib, gp.ctx, gp.objs["g1"]
    bad = []
    for fault, (P_new, table, text) in REMAP.items():
        h = C.c_void_p(WILD)
        before = _mark(gp, "remap")
        rc = lib.gpc_sparse_remap(g1.h, P_new, None if table is None else table.ctypes.data, C.byref(h))
        msg = lib.gpc_last_error(ctx.h).decode()
        print("remap %-22s rc %d (%s)" % (fault, rc, msg))
        if rc != E or h.value is not None or msg == before or text not in msg:
            bad.append((fault, rc, h.value, msg))
    assert not bad, bad
    table = _off(0, 1, 2, 3)
    h = C.c_void_p(WILD)
    before = _mark(gp, "remap")
    assert lib.gpc_sparse_remap(None, 6, table.ctypes.data, C.byref(h)) == E and h.value == WILD and lib.gpc_last_error(ctx.h).decode() == before
    assert lib.gpc_sparse_remap(g1.h, 6, table.ctypes.data, None) == E and "out is NULL" in lib.gpc_last_error(ctx.h).decode()
    # a table that passes: the state moves, bit for bit, and the other patches are empty and zero
    _restore(gp, g1)
    table = _off(1, 2, 4, 5)
    assert lib.gpc_sparse_remap(g1.h, 6, table.ctypes.data, C.byref(h)) == OK
    new = types.SimpleNamespace(h=h, P=6, ny=1)
    s = _state(gp, new)
    lib.gpc_sparse_destroy(h)
    for k, a in s.items():
        assert _same_bits(np.ascontiguousarray(a[table]), g1.saved[k]) and not np.any(a[[0, 3]]), k


# ---------------------------------------------------------------------------------------------------------------- (c) the P = 0 object

@pytest.mark.parametrize("obj", ["z", "z3", "pz"])
def test_empty_object(gp, obj):
    """P = 0 with valid arguments: GPC_OK from every entry the object's kind allows, and nothing written -- but for the scattered read-out,
    where every entry is a miss (f and sigma NaN, include/gpc.h)."""
    lib, o = gp.lib, gp.objs[obj]
    # (what an object of this kind is refused whatever its P: the rows of TWINS and RULES)
    refused_dev = {"z": (), "z3": ("train_sigmaf",), "pz": ("train_sigmaf", "likelihood", "prune_rd", "quantize_rd")}[obj]
    refused_host = {"z": (), "z3": (), "pz": ("prune_rd", "quantize_rd")}[obj]
    for entry in ENTRIES:
        for dev in _forms(entry):
            rc, outs, msg, _ = _call(gp, o, entry, dev)
            want = E if entry in (refused_dev if dev else refused_host) else OK
            assert rc == want, (entry, dev, rc, msg)
            if entry == "predict_scattered":
                assert np.all(np.isnan(outs["f"])) and np.all(np.isnan(outs["sigma"])) and _written(outs) == ["f", "sigma"], (dev, outs)
                rc, outs, msg, _ = _call(gp, o, entry, dev, dict(n=0))
                assert rc == OK, (entry, dev, msg)
            assert not _written(outs), (entry, dev, _written(outs))
    assert lib.gpc_sparse_ld(o.h) == LD
    for P_new in (0, 2):
        h = C.c_void_p()
        assert lib.gpc_sparse_remap(o.h, P_new, None, C.byref(h)) == OK and h.value
        sizes = np.full(max(P_new, 1), -7, dtype=np.int32)
        assert lib.gpc_sparse_sizes(h, sizes.ctypes.data) == OK and np.all(sizes[:P_new] == 0) and np.all(sizes[P_new:] == -7)
        lib.gpc_sparse_destroy(h)


# ---------------------------------------------------------------------------------------------------------------- (d) a dead context

def test_dead_context(gp):
    """An object whose context was destroyed first can only be destroyed: every entry that takes it is GPC_EINVAL before it looks at
    another argument or at the device, and leaves no text.  (gpc_sparse_ld reads the object alone and still answers.)"""
    lib, capi = gp.lib, gp.capi
    dead = capi.Context(0)
    h, dead.h = dead.h, None
    o = _object(gp, "dead", 4, 1, ctx_h=h)
    other = _object(gp, "dead3", 4, 3, ctx_h=h)
    lib.gpc_ctx_destroy(h)
    try:
        for entry in ENTRIES:
            for dev in _forms(entry):
                rc, outs, msg, before = _call(gp, o, entry, dev)
                assert rc == E and not _written(outs) and msg == before, (entry, dev, rc, msg, _written(outs))
        new = C.c_void_p(WILD)
        table = _off(0, 1, 2, 3)
        assert lib.gpc_sparse_remap(o.h, 4, table.ctypes.data, C.byref(new)) == E and new.value == WILD
        assert lib.gpc_sparse_create(h, C.byref(_params(gp)), 4, 1, C.byref(new)) == E and new.value == WILD
        n = np.full(1, -7, dtype=np.int32)
        for fn in (lib.gpc_sparse_decode, lib.gpc_sparse_decode_dev):
            assert fn(o.h, other.h, RES, 2, None, None, None, None, None, 0, None, None, None, None, n.ctypes.data) == E and n[0] == -7, fn
        assert lib.gpc_sparse_ld(o.h) == LD                                                                           # from the code
    finally:
        lib.gpc_sparse_destroy(o.h)
        lib.gpc_sparse_destroy(other.h)       # the last child releases the context


# ---------------------------------------------------------------------------------------------------------------- (e) host equals _dev

def _both(gp, o, entry, change_of=lambda dev: {}, null=()):
    """the entry's host twin and its _dev twin, each on the saved state: (outputs, state afterwards) of either"""
    got = {}
    for dev in (False, True):
        _restore(gp, o)
        rc, outs, msg, _ = _call(gp, o, entry, dev, change_of(dev), null)
        assert rc == OK, (entry, dev, rc, msg)
        got[dev] = (outs, _state(gp, o))
    return got[False], got[True]


def _rows_beyond(a, first):
    """the entries [p][first[p]:] of a [P][ld] or [P][ld][.] array"""
    return np.concatenate([a[p, first[p]:].reshape(-1) for p in range(len(first))])


def _sentinel_regions(o, entry, outs, state):
    """what the call is documented to leave alone (include/gpc.h) still holds the sentinel"""
    held = lambda a: np.all(a == SENTINEL[a.dtype.type])
    if entry in ("prune", "prune_rd"):
        rm = outs["removed"]
        assert rm[3] > 0 and np.all(rm >= 0) and np.all(rm < LD), rm
        for k in ("order", "scores") + (("mse",) if entry == "prune_rd" else ()):
            assert held(_rows_beyond(outs[k], rm)) and not held(outs[k][3, :rm[3]]), k
    if entry == "quantize_rd":
        b = state["bv_count"]
        assert outs["bits"][3] == 5 and outs["bits"][0] == 0, outs["bits"]
        assert held(_rows_beyond(outs["q_bv"], b)) and held(_rows_beyond(np.ascontiguousarray(outs["q_alpha"].transpose(0, 2, 1)), b))
        assert not held(outs["q_bv"][3, :b[3]]) and not held(outs["q_alpha"][3, :, :b[3]])
        # max_mse = +inf accepts bits_min = 5: no other width is evaluated; the empty patch escapes, nothing of it is written
        assert held(outs["curve"][:, :4]) and held(outs["curve"][:, 5:]) and not held(outs["curve"][3, 4])
        assert held(outs["q_bv"][0]) and held(outs["q_alpha"][0]) and held(outs["range"][0]) and held(outs["curve"][0])


PAIR_CELLS = [(obj, entry) for obj in ("g1", "g3") for entry in PAIRS if not (obj == "g3" and entry == "train_sigmaf")]


@pytest.mark.parametrize("obj,entry", PAIR_CELLS)
def test_host_equals_dev(gp, obj, entry):
    """Each staged pair on the saved state, every output pre-filled on both sides: the host twin leaves the bytes of the _dev twin in
    every output and in the object.  A staging size that is wrong on the way up or down shows here."""
    o = gp.objs[obj]
    # the add call brings new points: full updates into a full basis, so that deletions follow
    new = _batch(o.ny, seed=41)
    change = dict(x0=new["x0"], x1=new["x1"], third=new["y"]) if entry == "add" else {}
    (h_out, h_state), (d_out, d_state) = _both(gp, o, entry, lambda dev: change)
    for k in h_state:
        assert _same_bits(h_state[k], d_state[k]), ("state", k)
    changed = any(not _same_bits(h_state[k], o.saved[k]) for k in h_state)
    assert changed == (entry in ("add", "prune", "prune_rd")) or entry == "dequantize", (entry, changed)
    for k in _outs(entry):
        if k == "ls":
            # gpc_sparse_train_sigmaf hands its twin a zeroed ls: behind the iters[p] steps a patch took the host form reads 0, the _dev
            # form leaves the caller's words (from the code)
            it = h_out["iters"]
            assert np.all(it >= 0) and np.all(it <= MAXC + 2) and np.any(it < MAXC + 2), it
            for p in range(o.P):
                assert _same_bits(h_out[k][p, :it[p]], d_out[k][p, :it[p]]), (k, p)
                assert np.all(h_out[k][p, it[p]:] == 0.0) and np.all(d_out[k][p, it[p]:] == SENTINEL[np.float64]), (k, p)
            continue
        assert _same_bits(h_out[k], d_out[k]), (entry, k)
    _sentinel_regions(o, entry, h_out, h_state)
    _sentinel_regions(o, entry, d_out, d_state)
    if entry == "add":
        # (the patch above the capacity took a new vector in and deleted one)
        assert np.all(h_state["bv_count"] <= CAP) and h_state["bv_count"][3] == CAP and not _same_bits(h_state["BV"][3], o.saved["BV"][3])
    if entry == "dequantize":
        assert _same_bits(h_state["bv_count"], o.saved["bv_count"]) and not np.any(h_state["C"][3]) and np.any(h_state["alpha"][3])


@pytest.mark.parametrize("obj", ["g1", "g3"])
def test_scattered_interleaved(gp, obj):
    """gpc_sparse_predict_scattered on interleaved coordinates (x1 = x0 + 1, stride 3: the `local` rows of a render) -- the host twin
    stages them as one array -- against its _dev twin and against the same coordinates as two arrays."""
    o = gp.objs[obj]
    v = _values(o, "predict_scattered")
    local = np.full((K, 3), 9.0)
    local[:, 1], local[:, 2] = v["x0"], v["x1"]
    inter = dict(local=local, x0=("@", "local", 8), x1=("@", "local", 16), stride=3)
    (h_out, _), (d_out, _) = _both(gp, o, "predict_scattered", lambda dev: inter)
    (s_out, _), _ = _both(gp, o, "predict_scattered")
    for k in ("f", "sigma", "status"):
        assert _same_bits(h_out[k], d_out[k]) and _same_bits(h_out[k], s_out[k]), k
    miss = v["patch"] >= o.P
    miss |= v["patch"] < 0
    assert np.all(np.isnan(h_out["f"][:, miss])) and np.all(np.isfinite(h_out["f"][:, v["patch"] == 3]))


# ---------------------------------------------------------------------------------------------------------------- (f) optional outputs

@pytest.mark.parametrize("entry", ["prune", "prune_rd", "quantize_rd"])
@pytest.mark.parametrize("obj", ["g1", "g3"])
def test_optional_outputs(gp, obj, entry):
    """Every output of the three rate-control entries may be NULL: the host twin with all of them NULL, with every second one NULL and
    with the others NULL leaves the object, and the outputs it still has, with the bits of the full call."""
    o = gp.objs[obj]
    names = _outs(entry)
    _restore(gp, o)
    rc, full, msg, _ = _call(gp, o, entry, False)
    assert rc == OK, msg
    state = _state(gp, o)
    for null in (tuple(names), tuple(names[0::2]), tuple(names[1::2])):
        _restore(gp, o)
        rc, got, msg, _ = _call(gp, o, entry, False, null=null)
        assert rc == OK and sorted(got) == sorted(set(names) - set(null)), (null, msg)
        after = _state(gp, o)
        for k in state:
            assert _same_bits(after[k], state[k]), (null, "state", k)
        for k in got:
            assert _same_bits(got[k], full[k]), (null, k)
