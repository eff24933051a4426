"""GPU tests of the argument rules and the levels of the eight probit IRLS entries (gpc_dense_irls_fit_predict, its _var and _ev forms
and gpc_dense_irls_select, each with its _dev twin; include/gpc.h): one rule list for all of them, written here as a literal table, and
three levels -- the plain fit, the fit with the factor export, the selection loop -- that must give one bit pattern whichever entry
reaches them.  Everything goes through the C-ABI with explicit NULLs; nothing is compared against a tolerance.

Inputs: irls_cases.grid_batch("w4") and ("big") -- five patches each, one empty, one of 1 or 17 points, the largest of 256 or 420
points, so both IRLS kernel shapes run -- in irls_cases.REGIME with MODELS[2]'s start and tolerance; X* point-wise
(variance_cases.xstar(4)) or the sz = 2 grid."""
import ctypes as C
import itertools

import numpy as np
import pytest

import irls_cases as IC
import variance_cases as VC

pytestmark = pytest.mark.gpu

ENTRIES = ("plain", "var", "ev", "select")
SYMBOL = {"plain": "gpc_dense_irls_fit_predict", "var": "gpc_dense_irls_fit_predict_var", "ev": "gpc_dense_irls_fit_predict_ev",
          "select": "gpc_dense_irls_select"}
# the outputs of each entry in the order of its prototype
OUT = {"plain": ("f", "alpha", "fhat", "iters", "status"),
       "var": ("f", "v", "p", "alpha", "fhat", "iters", "status"),
       "ev": ("f", "v", "p", "alpha", "fhat", "iters", "status", "log_q"),
       "select": ("f", "v", "p", "alpha", "fhat", "log_q", "best", "log_q_all", "iters", "status")}
FILL = dict(f=np.nan, v=np.nan, p=np.nan, alpha=np.nan, fhat=np.nan, log_q=np.nan, log_q_all=np.nan, iters=-1, status=-1, best=-2)
XS = VC.xstar(4, seed=97)
SZ = 2
FORMS = ("points", "grid")
W4, BIG = "dense_mfma_big_w4_irls", "dense_mfma_big_irls"
VAR = " + dense_variance_big"


@pytest.fixture(scope="module")
def gp():
    from gp_compressor_amd import capi
    capi.load()          # raises if the HIP library is missing: no fallback
    ctx = capi.Context(0)
    yield capi, ctx
    ctx.close()


@pytest.fixture(autouse=True)
def _plain_env(monkeypatch):
    monkeypatch.delenv("GPC_POISON_LDS", raising=False)


@pytest.fixture(scope="module")
def batches():
    return {s: IC.grid_batch(s) for s in ("w4", "big")}


def _same_bits(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(a.view(np.uint8), b.view(np.uint8))


def _untouched(outs):
    """The names of the output arrays that no longer hold their fill."""
    return [k for k, a in outs.items() if a is not None and not (np.all(np.isnan(a)) if np.isnan(FILL[k]) else np.all(a == FILL[k]))]


def _call(gp, entry, dev, batch, form, model=2, noise=IC.REGIME[2], irls_null=False, irls_kw=None, P=None, m=None, sz=SZ, xs1_null=False,
          null=(), H=1, cand_null=False):
    """One call of an entry through the C-ABI: host arrays or (dev) device tensors, outputs pre-filled (FILL), those named in `null`
    passed as NULL.  Returns (rc, outputs as numpy arrays or None, error text, last dense kernel)."""
    import torch
    capi, ctx = gp
    off, x0, x1, lab = batch
    Pn, N = len(off) - 1, len(lab)
    grid = form == "grid"
    m_shape = SZ * SZ if grid else len(XS[0])
    prm = capi.default_params_dense(sigmaf_sq=IC.REGIME[0], l_sq=IC.REGIME[1], noise=noise, noise_model=model)
    arg = dict(IC.MODELS[model] if model in IC.MODELS else IC.MODELS[2])
    arg.update(irls_kw or {})
    arg.setdefault("max_iter", IC.MAX_ITER)
    irls = capi.default_params_irls(**arg)
    shape = dict(f=(Pn, m_shape), v=(Pn, m_shape), p=(Pn, m_shape), alpha=(N,), fhat=(N,), log_q=(Pn,), log_q_all=(max(H, 1), Pn), iters=(Pn,),
                 status=(Pn,), best=(Pn,))
    outs = {k: None if k in null else np.full(shape[k], FILL[k], dtype=np.int32 if k in ("iters", "status", "best") else np.float64)
            for k in OUT[entry]}
    ins = dict(off=np.ascontiguousarray(off, dtype=np.int32), x0=x0, x1=x1, y=lab, xs0=None if grid else XS[0],
               xs1=None if grid or xs1_null else XS[1])
    if dev:
        d = torch.device("cuda", 0)
        up = lambda a: None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(d)
        ins_c, outs_c = {k: up(a) for k, a in ins.items()}, {k: up(a) for k, a in outs.items()}
        torch.cuda.synchronize()
    else:
        ins_c, outs_c = ins, outs
    ptr = capi._ptr
    Pa = Pn if P is None else P
    args = [ctx.h, C.byref(prm), None if irls_null else C.byref(irls)]
    if entry == "select":
        arr = ctx.hyper_array([IC.REGIME] * max(H, 1))
        args += [H, None if cand_null else C.addressof(arr)]
    args += [Pa, ptr(ins_c["off"])]
    if dev:
        args += [int(np.max(np.diff(off))) if Pa > 0 else 0, N if Pa > 0 else 0]
    args += [ptr(ins_c["x0"]), ptr(ins_c["x1"]), ptr(ins_c["y"]), m_shape if m is None else m, ptr(ins_c["xs0"]), ptr(ins_c["xs1"]), IC.RES, sz]
    args += [ptr(outs_c[k]) for k in OUT[entry]]
    rc = getattr(ctx.lib, SYMBOL[entry] + ("_dev" if dev else ""))(*args)
    if dev:
        ctx.synchronize()
        outs = {k: None if a is None else a.cpu().numpy() for k, a in outs_c.items()}
    return rc, outs, ctx.lib.gpc_last_error(ctx.h).decode(), ctx.last_dense_kernel()


# ---------------------------------------------------------------------------------------------------------------- 1. the rule table

E, R, OK = -22, -34, 0      # GPC_EINVAL, GPC_ERANGE, GPC_OK (include/gpc.h)
# fault -> (the X* forms it exists in, what changes in the call, the code of (plain, var, ev, select); None: no such cell).  Read off the
# rule list of include/gpc.h, not off the library.  Every other argument of a cell is valid: the fault is the only one.
RULES = {
    "irls NULL":            (FORMS, dict(irls_null=True), (E, E, E, E)),
    "noise_model 0":        (FORMS, dict(model=0), (E, E, E, E)),
    "p_star with model 1":  (FORMS, dict(model=1), (None, E, E, E)),
    "log_q with model 1":   (FORMS, dict(model=1), (None, None, E, E)),
    "max_iter 0":           (FORMS, dict(irls_kw=dict(max_iter=0)), (E, E, E, E)),
    "tol -1":               (FORMS, dict(irls_kw=dict(tol=-1.0)), (E, E, E, E)),
    "f_init NaN":           (FORMS, dict(irls_kw=dict(f_init=np.nan)), (E, E, E, E)),
    "noise 0":              (FORMS, dict(noise=0.0), (E, E, E, E)),
    "sz -1":                (("grid",), dict(sz=-1), (E, E, E, E)),
    "sz 1025":              (("grid",), dict(sz=1025), (E, E, E, E)),
    "xs1 NULL":             (("points",), dict(xs1_null=True), (E, E, E, E)),
    "f_star NULL":          (FORMS, dict(null=("f",)), (E, E, E, OK)),
    "P -1":                 (FORMS, dict(P=-1), (E, E, E, E)),
    "1025-point patch":     (FORMS, dict(), (R, R, R, R)),
    "H 0":                  (FORMS, dict(H=0), (None, None, None, E)),
    "cand NULL":            (FORMS, dict(cand_null=True), (None, None, None, E)),
}
# which optional outputs a cell leaves NULL so that its fault stays the only one: with model 1 neither the other of p_star / log_q
MODEL1_NULL = {"p_star with model 1": {"var": (), "ev": ("log_q",), "select": ()},
               "log_q with model 1": {"ev": ("p",), "select": ("p",)}}


@pytest.mark.parametrize("fault,form", [(f, form) for f in RULES for form in RULES[f][0]])
def test_rule_table(gp, batches, fault, form):
    """Every entry, host and _dev, against one fault: the code of the table, an error text, and no output written."""
    _, change, codes = RULES[fault]
    batch = IC.labelled(VC._mixed_batch([1025, 3], seed=87)) if fault == "1025-point patch" else batches["w4"]
    bad = []
    for entry, want in zip(ENTRIES, codes):
        if want is None:
            continue
        kw = dict(change)
        if fault in MODEL1_NULL:
            kw["null"] = MODEL1_NULL[fault][entry]
        for dev in (False, True):
            rc, outs, msg, _ = _call(gp, entry, dev, batch, form, **kw)
            print("cell %-20s %-6s %-4s %-6s rc %d (%s)" % (fault, entry, "dev" if dev else "host", form, rc, msg if rc else ""))
            if rc != want:
                bad.append((entry, dev, "code", rc, want))
            elif want != OK and (not msg or _untouched(outs)):
                bad.append((entry, dev, "text or outputs", msg, _untouched(outs)))
    assert not bad, bad


@pytest.mark.parametrize("form", FORMS)
def test_empty_batch_is_ok_and_writes_nothing(gp, batches, form):
    """P = 0 with valid arguments: GPC_OK from every entry, nothing written."""
    for entry in ENTRIES:
        for dev in (False, True):
            rc, outs, _, _ = _call(gp, entry, dev, batches["w4"], form, P=0)
            assert rc == OK and not _untouched(outs), (entry, dev, rc, _untouched(outs))


# ---------------------------------------------------------------------------------------------------------------- 2. the levels

def _ok(res, label):
    assert res[0] == OK, (label, res[0], res[2])
    return res[1]


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("shape", ["w4", "big"])
def test_levels(gp, batches, shape, form):
    """The plain fit, the fit with the export, the selection loop: whichever entry reaches a level gives that level's bits and leaves
    its kernel name (the names are those the library reported before the entries were folded into one record)."""
    batch = batches[shape]
    fit = W4 if shape == "w4" else BIG
    full, name = {}, {}
    for entry in ENTRIES:
        res = _call(gp, entry, True, batch, form)
        full[entry], name[entry] = _ok(res, entry), res[3]
        host = _ok(_call(gp, entry, False, batch, form), entry + " host")
        for k in OUT[entry]:
            assert _same_bits(host[k], full[entry][k]), ("host against _dev", entry, k)
    assert name == dict(plain=fit, var=fit + VAR, ev=fit + VAR, select=fit + VAR), name
    for entry in ENTRIES:
        assert np.all(full[entry]["status"] >= 0) and np.all(full[entry]["iters"] >= 0), entry       # (every patch was written)
    # _ev without log_q is _var
    for dev in (True, False):
        res = _call(gp, "ev", dev, batch, form, null=("log_q",))
        got = _ok(res, "ev without log_q")
        assert res[3] == fit + VAR
        for k in OUT["var"]:
            assert _same_bits(got[k], full["var"][k]), ("ev without log_q", dev, k)
    # _var without v_star and p_star is the plain entry; so is _var with nothing to predict, in what it still writes
    for dev in (True, False):
        res = _call(gp, "var", dev, batch, form, null=("v", "p"))
        got = _ok(res, "var without v, p")
        assert res[3] == fit
        for k in OUT["plain"]:
            assert _same_bits(got[k], full["plain"][k]), ("var without v, p", dev, k)
        res = _call(gp, "var", dev, batch, form, m=0, sz=0)
        got = _ok(res, "var with m = 0")
        assert res[3] == fit and not _untouched({k: got[k] for k in ("f", "v", "p")})
        for k in ("alpha", "fhat", "iters", "status"):
            assert _same_bits(got[k], full["plain"][k]), ("var with m = 0", dev, k)
    # _ev with nothing to predict: the export fit and the evidence alone
    for dev in (True, False):
        res = _call(gp, "ev", dev, batch, form, m=0, sz=0)
        got = _ok(res, "ev with m = 0")
        assert res[3] == fit + VAR and _same_bits(got["log_q"], full["ev"]["log_q"]), dev
    # select with params as its one candidate is _ev
    assert np.all(full["select"]["best"] == 0)
    for k in OUT["ev"]:
        assert _same_bits(full["select"][k], full["ev"][k]), ("select with one candidate", k)
    assert _same_bits(full["select"]["log_q_all"][0], full["ev"]["log_q"])


# ---------------------------------------------------------------------------------------------------------------- 3. optional outputs

@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("entry", ["ev", "select"])
def test_optional_outputs_from_the_workspace(gp, batches, entry, form):
    """alpha_out, fhat_out, iters, status: every subset passed as NULL to the _dev entry -- the workspace then stands in for the missing
    buffer -- leaves the bits of the remaining outputs as they are."""
    batch = batches["w4"]
    full = _ok(_call(gp, entry, True, batch, form), entry)
    opt = ("alpha", "fhat", "iters", "status")
    for r in range(1, len(opt) + 1):
        for null in itertools.combinations(opt, r):
            got = _ok(_call(gp, entry, True, batch, form, null=null), (entry, null))
            for k in OUT[entry]:
                if k not in null:
                    assert _same_bits(got[k], full[k]), (entry, null, k)
