"""Non-finite inputs of the dense path: the batches, the poisons and the pattern each must give, as data (test infrastructure:
test_dense_nonfinite_cpu.py holds the CPU oracle to the pattern, test_dense_nonfinite_gpu.py every route of the kernels).  No GPU import.

Every injected value is a NaN or an infinity that no finite intermediate can meet by overflow (the rule of nonfinite_cases.py), so
whether an entry comes out finite or not does not depend on the order of a sum.  Default regime, ref_double_noise = 1, ny = 1 and 3.

Families (variance_cases._mixed_batch; each ragged, with an empty and a one-point patch; the poisoned patch sits between two clean
patches of other tile counts):
    n256   [33, 1, 17, 200, 16, 0, 255, 256]    the one-wave kernel, the register tile, the two-wave shape
    n512   [512, 257, 1, 300, 17, 0, 511]       the 512 instance, the size-class split (257: NT = 17, 300: tiled)
    tiled  [513, 1, 600, 16, 0, 1024]           the tiled kernel's eight-wave shape; one 1024-point patch (the oracle is O(n^3))
Positions of the poisoned point: (a) the first 16-point tile, (b) the last tile column, (c) the last point n - 1 of a patch whose n is no
multiple of 16 (next to the identity padding; "c17" in n512: the 257-point patch, whose last point is alone in its tile), (d) the only
point of the one-point patch.

The pattern (PATTERN below says it per kind; `expect` turns it into masks):
    x poisons   status GPC_STATUS_NOT_SPD; f*, alpha and v* of the patch all NaN.  The diagonal entry is sf * exp(c (inf - inf)^2) = NaN
                (a NaN coordinate: the whole row), and a pivot that is NaN is not positive.
    y poisons   status 0; alpha and f* of the poisoned channel non-finite in every entry (the oracle: NaN, or +-inf where the poison is
                the last or the only point; where the infinities of a sum cancel depends on its order, so non-finite is what is
                asked); the other channels and v* as in the clean run.
    X* = NaN    (point-wise entry, one coordinate of column j) column j of f* and of v* NaN on every non-empty patch.
    X* = +inf   the kernel value is exp(-inf) = 0 against every training point, so column j of f* is 0 on every patch; v* of column j is
                k(x*, x*) - 0 = sf * exp(c (inf - inf)^2) = NaN on every non-empty patch (gpc_kss, gpc_device.h).
    the empty patch under either: f* = 0 and v* = the prior sf -- the kernels write an empty patch without evaluating anything, where the
                oracle's v* is NaN (it evaluates k(x*, x*) there too).  include/gpc.h makes the prior the contract; it is the one entry
                where the pattern is not the reference's arithmetic (v_prior_oracle_nan).
Everything else -- the other patches, channels and columns -- is clean: the oracle shows the bits of the unpoisoned run."""
import numpy as np

import variance_cases as VC

RES, SZ = 0.15, 5               # the grid entry's X*: 25 cells
M_PTS = 25                      # the point-wise entry's X*: variance_cases.xstar(M_PTS, XSTAR_SEED); blocks of 16: one full, one partial
XSTAR_SEED = 407
REGIME = VC.DEFAULT
STATUS_NOT_SPD = 1              # include/gpc.h GPC_STATUS_NOT_SPD

FAMILIES = {"n256": [33, 1, 17, 200, 16, 0, 255, 256], "n512": [512, 257, 1, 300, 17, 0, 511], "tiled": [513, 1, 600, 16, 0, 1024]}
SEED = {"n256": 401, "n512": 402, "tiled": 403}
# family -> position -> patch
TARGET = {"n256": {"a": 3, "b": 3, "c": 3, "d": 1}, "n512": {"a": 3, "b": 3, "c": 3, "c17": 1, "d": 2}, "tiled": {"a": 2, "b": 2, "c": 2, "d": 1}}

X_KINDS = ("x0_nan", "x1_pinf", "x0_ninf", "x_two_pinf")
Y_KINDS = ("y_nan", "y_pinf", "y_ninf")
XS_KINDS = ("xs_nan", "xs_pinf")
KINDS = X_KINDS + Y_KINDS
PATTERN = {"x0_nan": "patch NaN, status 1", "x1_pinf": "patch NaN, status 1", "x0_ninf": "patch NaN, status 1",
           "x_two_pinf": "patch NaN, status 1", "y_nan": "channel non-finite, status 0", "y_pinf": "channel non-finite, status 0",
           "y_ninf": "channel non-finite, status 0", "xs_nan": "column NaN (empty patch: f* = 0, v* = prior | oracle NaN)",
           "xs_pinf": "column f* = 0, v* NaN (empty patch: v* = prior | oracle NaN)"}
VALUE = {"x0_nan": np.nan, "x1_pinf": np.inf, "x0_ninf": -np.inf, "x_two_pinf": np.inf, "y_nan": np.nan, "y_pinf": np.inf, "y_ninf": -np.inf,
         "xs_nan": np.nan, "xs_pinf": np.inf}
# X* poisons: (kind, axis, column) -- once inside the first 16-point block, once in the partial last block
XS_POISONS = (("xs_nan", 0, 3), ("xs_nan", 1, 21), ("xs_pinf", 1, 3), ("xs_pinf", 0, 21))

_BATCH = {}


def batch(family, ny):
    """The family's clean batch (off, x0, x1, y (ny, N)); read-only"""
    key = (family, ny)
    if key not in _BATCH:
        b = VC.with_planes(*VC._mixed_batch(FAMILIES[family], seed=SEED[family], res=RES), ny, seed=SEED[family] + 50)
        for a in b:
            a.setflags(write=False)
        _BATCH[key] = b
    return _BATCH[key]


def xstars():
    q0, q1 = VC.xstar(M_PTS, XSTAR_SEED)
    return q0, q1


def _points(pos, n, two):
    """Patch-local indices of the poisoned point(s)"""
    last_tile = 16 * ((n - 1) // 16)
    if pos == "a":
        return (3, 9) if two else (5,)
    if pos == "b":
        return (last_tile + 1, min(last_tile + 6, n - 1)) if two else (last_tile + 1,)
    if pos in ("c", "c17"):
        assert n % 16
        return (2, n - 1) if two else (n - 1,)
    assert pos == "d" and n == 1 and not two
    return (0,)


def train_cases():
    """(family, ny, kind, position, patch, points, channel): one poisoned patch per case; for ny = 3 the y poisons go to one channel,
    which varies with the kind and the position"""
    out = []
    for fam, sizes in FAMILIES.items():
        for ny in (1, 3):
            for ki, kind in enumerate(KINDS):
                for pi, (pos, j) in enumerate(TARGET[fam].items()):
                    if kind == "x_two_pinf" and pos == "d":
                        continue
                    ch = (ki + pi) % ny if kind in Y_KINDS else -1
                    out.append((fam, ny, kind, pos, j, _points(pos, sizes[j], kind == "x_two_pinf"), ch))
    return out


def xs_cases():
    """(family, ny, kind, axis, column): one coordinate of one X* of the point-wise entry"""
    return [(fam, ny) + p for fam in FAMILIES for ny in (1, 3) for p in XS_POISONS]


def case_id(case):
    return "-".join(str(c) for c in case if not isinstance(c, tuple))


def poisoned(case):
    """The inputs of a case: (off, x0, x1, y), (xs0, xs1) -- fresh writable copies of what the poison touches"""
    fam, ny, kind = case[:3]
    off, x0, x1, y = batch(fam, ny)
    q0, q1 = xstars()
    if kind in XS_KINDS:
        q = [q0.copy(), q1.copy()]
        q[case[3]][case[4]] = VALUE[kind]
        return (off, x0, x1, y), tuple(q)
    _, _, _, _, j, pts, ch = case
    x0, x1, y = x0.copy(), x1.copy(), y.copy()
    for p in pts:
        i = int(off[j]) + p
        if kind in ("x0_nan", "x0_ninf", "x_two_pinf"):
            x0[i] = VALUE[kind]
        elif kind == "x1_pinf":
            x1[i] = VALUE[kind]
        else:
            y[ch, i] = VALUE[kind]
    return (off, x0, x1, y), (q0, q1)


def expect_masks(off, ny, m, xpatches=(), ypatches=(), nan_col=None, inf_col=None):
    """The pattern as masks over the outputs f* (P, ny, m), alpha (ny, N), v* (P, m):
        status                      per patch
        f_nan, al_nan, v_nan        must be NaN
        f_bad, al_bad               must be non-finite
        f_zero, v_prior             must be 0 (the column of an infinite X*; the empty patch) | sigma_f^2 (the empty patch under a
                                    non-finite X*; v_prior_oracle_nan: the oracle's own v* is NaN there -- all of them today)
       everything outside the masks is clean.  xpatches: x-poisoned patches; ypatches: (patch, channel)."""
    P, N = len(off) - 1, int(off[-1])
    e = {"status": np.zeros(P, dtype=np.int32)}
    for k, shape in (("f_nan", (P, ny, m)), ("f_bad", (P, ny, m)), ("f_zero", (P, ny, m)), ("al_nan", (ny, N)), ("al_bad", (ny, N)),
                     ("v_nan", (P, m)), ("v_prior", (P, m)), ("v_prior_oracle_nan", (P, m))):
        e[k] = np.zeros(shape, dtype=bool)
    for j in xpatches:
        e["status"][j] = STATUS_NOT_SPD
        e["f_nan"][j] = True
        e["v_nan"][j] = True
        e["al_nan"][:, off[j]:off[j + 1]] = True
    for j, ch in ypatches:
        e["f_bad"][j, ch] = True
        e["al_bad"][ch, off[j]:off[j + 1]] = True
    empty = np.diff(off) == 0
    if nan_col is not None:
        e["f_nan"][~empty, :, nan_col] = True
        e["v_nan"][~empty, nan_col] = True
        e["f_zero"][empty, :, nan_col] = True
        e["v_prior"][empty, nan_col] = True
        e["v_prior_oracle_nan"][empty, nan_col] = True
    if inf_col is not None:
        e["f_zero"][:, :, inf_col] = True
        e["v_nan"][~empty, inf_col] = True
        e["v_prior"][empty, inf_col] = True
        e["v_prior_oracle_nan"][empty, inf_col] = True
    e["f_clean"] = ~(e["f_nan"] | e["f_bad"] | e["f_zero"])
    e["al_clean"] = ~(e["al_nan"] | e["al_bad"])
    e["v_clean"] = ~(e["v_nan"] | e["v_prior"])
    return e


def expect(case):
    fam, ny, kind = case[:3]
    off = batch(fam, ny)[0]
    if kind in XS_KINDS:
        return expect_masks(off, ny, M_PTS, nan_col=case[4] if kind == "xs_nan" else None, inf_col=case[4] if kind == "xs_pinf" else None)
    j, ch = case[4], case[6]
    return expect_masks(off, ny, M_PTS, xpatches=(j,)) if kind in X_KINDS else expect_masks(off, ny, M_PTS, ypatches=((j, ch),))


def pattern_failures(e, out, entry_has_v=True):
    """What of the pattern `e` the outputs miss (the part that needs no clean run): out = dict(st, f, al | None, v | None).  -> list of str"""
    bad = []
    if not np.array_equal(out["st"], e["status"]):
        bad.append("status %s, wanted %s" % (np.flatnonzero(out["st"] != e["status"]).tolist(), e["status"][out["st"] != e["status"]].tolist()))
    f, al, v = out["f"], out.get("al"), out.get("v")
    if not np.all(np.isnan(f[e["f_nan"]])):
        bad.append("f*: %d entries that must be NaN are not" % int(np.sum(~np.isnan(f[e["f_nan"]]))))
    if np.any(np.isfinite(f[e["f_bad"]])):
        bad.append("f*: %d finite entries in a poisoned channel" % int(np.sum(np.isfinite(f[e["f_bad"]]))))
    if not np.all(f[e["f_zero"]] == 0.0):
        bad.append("f*: %d entries that must be 0 are not" % int(np.sum(f[e["f_zero"]] != 0.0)))
    if not np.all(np.isfinite(f[e["f_clean"]])):
        bad.append("f*: %d clean entries are not finite" % int(np.sum(~np.isfinite(f[e["f_clean"]]))))
    if al is not None:
        if not np.all(np.isnan(al[e["al_nan"]])):
            bad.append("alpha: %d entries that must be NaN are not" % int(np.sum(~np.isnan(al[e["al_nan"]]))))
        if np.any(np.isfinite(al[e["al_bad"]])):
            bad.append("alpha: %d finite entries in a poisoned channel" % int(np.sum(np.isfinite(al[e["al_bad"]]))))
        if not np.all(np.isfinite(al[e["al_clean"]])):
            bad.append("alpha: %d clean entries are not finite" % int(np.sum(~np.isfinite(al[e["al_clean"]]))))
    if v is not None and entry_has_v:
        if not np.all(np.isnan(v[e["v_nan"]])):
            bad.append("v*: %d entries that must be NaN are not" % int(np.sum(~np.isnan(v[e["v_nan"]]))))
        if not np.all(np.isfinite(v[e["v_clean"]])):
            bad.append("v*: %d clean entries are not finite" % int(np.sum(~np.isfinite(v[e["v_clean"]]))))
    return bad


# ---------------------------------------------------------------------------------------------------------------------------
# the oracle on the cases, once per process
# ---------------------------------------------------------------------------------------------------------------------------
_CLEAN, _CASE = {}, {}


def _freeze(d):
    for a in d.values():
        if a is not None:
            a.setflags(write=False)
    return d


def _oracle_run(oracle, b, q, grid):
    """dict(st, f, al, v) of the oracle on a batch: f on the grid (no variance: the grid entry has none) or on the points q"""
    p = oracle.dense_params(*REGIME)
    if grid:
        f, _, st, al = oracle.dense_fit_predict_batch(p, *b, *oracle.grid(RES, SZ), want_alpha=True)
        return _freeze(dict(st=st, f=f, al=al, v=None))
    f, v, st, al = oracle.dense_fit_predict_batch(p, *b, *q, variance=True, want_alpha=True)
    return _freeze(dict(st=st, f=f, al=al, v=v))


def oracle_clean(oracle, family, ny):
    """{"grid": ..., "pts": ...} of the clean batch"""
    key = (family, ny)
    if key not in _CLEAN:
        b = batch(family, ny)
        _CLEAN[key] = {"grid": _oracle_run(oracle, b, None, True), "pts": _oracle_run(oracle, b, xstars(), False)}
    return _CLEAN[key]


def oracle_case(oracle, case):
    """{"grid": ..., "pts": ...} of the oracle on the poisoned batch of a case ("grid" is None for an X* poison).  The oracle fits patch
    after patch and shares nothing between them (gpc_oracle.c, orc_dense_fit_predict_batch), so a training poison is run on the
    poisoned patch and its two neighbours and the rest is taken from the clean run -- with one 1024-point solve per family instead of
    one per case; that the neighbours keep their bits is what the CPU test then shows on them.  -> (outputs, patches actually run)"""
    cid = case_id(case)
    if cid in _CASE:
        return _CASE[cid]
    fam, ny, kind = case[:3]
    b, q = poisoned(case)
    clean = oracle_clean(oracle, fam, ny)
    if kind in XS_KINDS:
        res = ({"grid": None, "pts": _oracle_run(oracle, b, q, False)}, list(range(len(b[0]) - 1)))
    else:
        j = case[4]
        idx = [j - 1, j, j + 1]
        sub, pts = VC.take_patches(*b, idx)
        out = {}
        for entry in ("grid", "pts"):
            r = _oracle_run(oracle, sub, q, entry == "grid")
            full = {k: (None if v is None else v.copy()) for k, v in clean[entry].items()}
            full["st"][idx], full["f"][idx] = r["st"], r["f"]
            full["al"][:, pts] = r["al"]
            if full["v"] is not None:
                full["v"][idx] = r["v"]
            out[entry] = _freeze(full)
        res = (out, idx)
    _CASE[cid] = res
    return res


# ---------------------------------------------------------------------------------------------------------------------------
# the stride batch
# ---------------------------------------------------------------------------------------------------------------------------
# 4200 patches of 17 .. 47 points, never a multiple of 16; a seeded pseudo-random third of them poisoned, alternating x0_nan, x1_pinf and
# y_nan.  4200 is what test_variance_host_pipeline_across_export_layouts runs: the host-pointer entries cut it into four chunks of 1050
# patches (dense_host.hip: P >= 4096), each a batch of its own for the kernels, and it exceeds every launcher's grid:
#     dense_mfma.hip       launch_nt: grid = P, one workgroup per patch -- nothing is handed on
#     dense_mfma_big.hip   dense_big_ws_bytes: grid = min(P, num_cus * per_cu), per_cu = 4 (two waves) | 2 (four waves) | 1 (eight waves):
#                          1024 | 512 | 256 on the 256 CUs of an MI355X; a workgroup goes on to patch blockIdx.x + k * grid
#     dense_generic.hip    dense_generic_ws_bytes: grid = min(P, num_cus * per_cu), per_cu = 4 at these sizes: 1024, same stride
#     dense_variance.hip   dvb_grid = min(P, num_cus) = 256 (dense_variance_big_kernel, same stride); dense_variance_kernel: one per patch
#     dense_mfma_w1.hip    launches of `slots` patches (DENSE_W1_MAX_SLOTS = 8192, GPC_W1_SLOTS overrides): patch base + s takes factor
#                          slot s after patch base - slots + s: a stride of the slot count (5 and 7 in the test)
STRIDE_P = 4200
STRIDE_SEED = 411
STRIDE_KINDS = ("x0_nan", "x1_pinf", "y_nan")
STRIDE_CHUNKS = 4               # dense_host.hip: P >= 4096 (GPC_HOST_NO_PIPELINE: 1)
GRIDS = {"dense_mfma_big 8 waves / dvb_grid": 256, "dense_mfma_big 4 waves": 512, "dense_mfma_big 2 waves / dense_generic": 1024}
W1_SLOTS = (5, 7)
MIN_PAIRS = 50
_STRIDE = {}


def stride_batch(ny):
    """-> (off, x0, x1, y) poisoned, the same clean, kind per patch (-1: clean, else index into STRIDE_KINDS), channel per patch"""
    if ny not in _STRIDE:
        rng = np.random.default_rng(STRIDE_SEED)
        sizes = rng.integers(17, 48, STRIDE_P)
        sizes[sizes == 32] = 33
        sizes[0], sizes[1] = 47, 17
        off, x0, x1, y = VC.with_planes(*VC._mixed_batch([int(s) for s in sizes], seed=STRIDE_SEED + 1, res=RES), ny, seed=STRIDE_SEED + 2)
        hit = np.flatnonzero(rng.random(STRIDE_P) < 1.0 / 3.0)
        kind = np.full(STRIDE_P, -1)
        kind[hit] = np.arange(len(hit)) % 3
        chan = np.where(kind == 2, np.arange(STRIDE_P) % ny, -1)
        at = rng.integers(0, 1 << 30, STRIDE_P) % sizes           # the poisoned point of each patch
        px0, px1, py = x0.copy(), x1.copy(), y.copy()
        for j in hit:
            i = int(off[j] + at[j])
            if kind[j] == 0:
                px0[i] = np.nan
            elif kind[j] == 1:
                px1[i] = np.inf
            else:
                py[chan[j], i] = np.nan
        for a in (off, x0, x1, y, px0, px1, py, kind, chan):
            a.setflags(write=False)
        _STRIDE[ny] = ((off, px0, px1, py), (off, x0, x1, y), kind, chan)
    return _STRIDE[ny]


def stride_expect(ny, m):
    (off, _, _, _), _, kind, chan = stride_batch(ny)
    return expect_masks(off, ny, m, xpatches=np.flatnonzero((kind == 0) | (kind == 1)).tolist(),
                        ypatches=[(int(j), int(chan[j])) for j in np.flatnonzero(kind == 2)])


def successor_pairs(G, chunks=1, ny=1):
    """The pairs (i, i + G) of one kernel batch -- the call cut into `chunks` as the host pipeline cuts it, indices counted inside a chunk
    -- with i poisoned, i + G clean and n_i > n_(i + G): the clean patches that run in a workgroup, a factor slot or an LDS image that a
    poisoned, larger patch has just left.  -> (i, i + G) as global patch indices, int array (K, 2)"""
    (off, _, _, _), _, kind, _ = stride_batch(ny)
    n = np.diff(off)
    out = []
    for c in range(chunks):
        lo, hi = STRIDE_P * c // chunks, STRIDE_P * (c + 1) // chunks
        i = np.arange(lo, hi - G) if hi - G > lo else np.zeros(0, dtype=np.int64)
        ok = (kind[i] >= 0) & (kind[i + G] < 0) & (n[i] > n[i + G])
        out.append(np.stack([i[ok], i[ok] + G], axis=1))
    return np.concatenate(out, axis=0)
