"""Cases of the masked decoder (gpc_sparse_decode, csrc/decode.hip) and a NumPy statement of its rule -- which points are kept, in which
order, and the counts -- shared by test_decode_cases_cpu.py (the cases are what they claim, no GPU) and test_decode_gpu.py.

The rule (include/gpc.h): m = sz * sz; grid point p has gx = p % sz, gy = p // sz; its cell in the layout of W and of `cells` is
c(p) = sz * gx + gy, the producer's cell function, transposed against p.  Leaf L is decoded iff b[L] > 0; (L, p) is kept iff L is decoded
and W is None or W[L, c(p)] != 0 and cells is None or cells[L, c(p)] != CELL_FREE.  Kept points come in ascending (L, p).

The records themselves are not restated here: the GPU test takes them from the chain the decoder replaces (Sparse.predict_dev on both
objects -> Context.reproject_dev) and selects rows by this rule; every comparison is exact.

States are readout_cases.batch(...) loaded with set_state; frames are reproject_cases.inputs(...)'s random orthonormal frames."""
import functools

import numpy as np

import readout_cases as RC
import reproject_cases as RPC

CELL_UNOBSERVED, CELL_OCCUPIED, CELL_FREE = 0, 1, 2      # include/gpc.h
RES = RC.RES
SIZES = (1, 3, 8, 9, 20)                                  # m = 1, 9, 64, 81, 400: below, at and above one block of 64 points, and many
ROW_LDS_MAX = 16384                                       # DC_ROW_MAX of decode.hip: above it the kept flags are read from global memory
SZ_GLOBAL_ROW = 129                                       # the first sz with m > ROW_LDS_MAX
MASK_KINDS = ("W", "cells", "both")
PATTERNS = ("all", "none", "first", "last", "k63", "k64", "k65", "checker", "half", "last_block", "row_gx0")
# (depth case, colour case or None, colour leaves reversed): readout_cases.CASES entries
PAIRS = {
    "cap100": ((100, 1, RC.L8), (100, 3, RC.L5), False),
    "ld256": ((-1, 1, RC.L8), (-1, 3, RC.L5), False),
    "cap15-norgb": ((15, 1, RC.L5), None, False),
    "cap100-reversed": ((100, 1, RC.L8), (100, 3, RC.L5), True),
}
# the scan of decode.hip: one workgroup of SCAN_THREADS threads, thread t holds the leaves [t * per, (t + 1) * per), per = ceil(P / 1024);
# the segments change shape where per steps: between P = 1024 and 1025 and between 2048 and 2049
SCAN_THREADS = 1024
SCAN_P = (1, 2, 1023, 1024, 1025, 2047, 2048, 2049)


def cell_of(p, sz):
    """c(p): the cell of grid point p in the layout of W and cells"""
    p = np.asarray(p)
    return sz * (p % sz) + p // sz


def kept(b, sz, W=None, cells=None):
    """(P, m) bool in GRID order: point (L, p) is kept"""
    b = np.asarray(b)
    P, m = len(b), sz * sz
    c = cell_of(np.arange(m), sz)
    k = np.repeat((b > 0)[:, None], m, axis=1)
    if W is not None:
        k &= np.asarray(W).reshape(P, m)[:, c] != 0
    if cells is not None:
        k &= np.asarray(cells).reshape(P, m)[:, c] != CELL_FREE
    return k


def rule(b, sz, W=None, cells=None):
    """leaf (n,), point (n,), count (P,), n of the decoder under the given masks"""
    k = kept(b, sz, W, cells)
    leaf, point = np.nonzero(k)                    # row-major: ascending (L, p)
    count = k.sum(axis=1).astype(np.int32)
    return leaf.astype(np.int32), point.astype(np.int32), count, int(count.sum())


def patterns_for(m):
    """the patterns a grid of m points can hold: `exactly k kept` needs m >= k"""
    return [n for n in PATTERNS if not (n[0] == "k" and int(n[1:]) > m)]


def claimed_count(name, m, sz):
    """the number of kept points the pattern's name claims (None: the name makes no claim)"""
    if name[0] == "k" and name[1:].isdigit():
        return int(name[1:])
    return {"all": m, "none": 0, "first": 1, "last": 1, "row_gx0": sz, "last_block": m - 64 * ((m - 1) // 64),
            "checker": (m + 1) // 2 if sz % 2 else m // 2}.get(name)


def pattern(name, sz, seed):
    """(m,) bool in GRID order (index p): the points the pattern keeps"""
    m = sz * sz
    p = np.arange(m)
    rng = np.random.default_rng([seed, sz, PATTERNS.index(name)])
    k = np.zeros(m, dtype=bool)
    if name == "all":
        k[:] = True
    elif name == "first":
        k[0] = True
    elif name == "last":
        k[m - 1] = True
    elif name[0] == "k" and name[1:].isdigit():
        k[rng.choice(m, int(name[1:]), replace=False)] = True
    elif name == "checker":
        k = ((p % sz) + (p // sz)) % 2 == 0
    elif name == "half":
        k = rng.integers(0, 2, m) == 1
    elif name == "last_block":
        k = p >= 64 * ((m - 1) // 64)
    elif name == "row_gx0":
        k = p % sz == 0
    elif name != "none":
        raise ValueError(name)
    return k


def to_cells(k, sz):
    """a kept set in grid order -> (m,) bool in the layout of W / cells"""
    out = np.zeros(sz * sz, dtype=bool)
    out[cell_of(np.arange(sz * sz), sz)] = k
    return out


def leaf_patterns(P, sz, rot):
    """the pattern name of every leaf: all of patterns_for(m) in turn, started at `rot`"""
    names = patterns_for(sz * sz)
    return [names[(i + rot) % len(names)] for i in range(P)]


def masks(P, sz, kind, rot=0, seed=11):
    """W, cells ((P, m) uint8 or None) of a batch in which leaf i carries pattern leaf_patterns(P, sz, rot)[i].
    W: kept cells are 1 or 255, dropped cells 0.  cells: kept cells are OCCUPIED or UNOBSERVED, dropped cells FREE.  both: W carries the
    leaf's pattern and cells the pattern five places on, so that the kept set is an intersection neither mask gives alone."""
    m = sz * sz
    rng = np.random.default_rng([seed, P, sz, rot])

    def grid(shift):
        names = leaf_patterns(P, sz, rot + shift)
        return np.stack([to_cells(pattern(n, sz, seed + i), sz) for i, n in enumerate(names)])

    W = cells = None
    if kind in ("W", "both"):
        W = np.where(grid(0), rng.choice(np.array([1, 255], dtype=np.uint8), (P, m)), 0).astype(np.uint8)
    if kind in ("cells", "both"):
        cells = np.where(grid(5 if kind == "both" else 0), rng.choice(np.array([CELL_OCCUPIED, CELL_UNOBSERVED], dtype=np.uint8), (P, m)),
                         CELL_FREE).astype(np.uint8)
    return W, cells


def reverse_leaves(B):
    """the batch with its leaves in reverse order (same P, ld, parameters)"""
    return dict(B, b=B["b"][::-1].copy(), alpha=B["alpha"][::-1].copy(), C=B["C"][::-1].copy(), BV=B["BV"][::-1].copy())


@functools.lru_cache(maxsize=None)
def pair(name):
    """depth batch, colour batch or None"""
    d, c, rev = PAIRS[name]
    Bd = RC.batch(*d)
    Bc = None if c is None else RC.batch(*c)
    if rev:
        Bc = reverse_leaves(Bc)
    assert Bc is None or Bc["P"] == Bd["P"]
    return Bd, Bc


@functools.lru_cache(maxsize=None)
def frames(P, seed=5):
    """R (P, 9) column-major orthonormal frames, mu (P, 3) in +-50, cm (P, 3) colour means (reproject_cases.inputs); read-only"""
    _, _, _, R, mu, _, cm = RPC.inputs(P, 4, seed, True)
    for a in (R, mu, cm):
        a.flags.writeable = False
    return R, mu, cm


def grid_points(res, sz):
    """xs0, xs1 (m,) of the decoder's grid, by the expression of the header"""
    p = np.arange(sz * sz)
    gx, gy = (p % sz).astype(np.float64), (p // sz).astype(np.float64)
    return res * ((gx + 0.5) / float(sz) - 0.5), res * ((gy + 0.5) / float(sz) - 0.5)


def scan_batch(P, name, seed=3):
    """b (P,) int32 in {0, 1} of the scan tests: reproject_cases.bv_pattern's trained / untrained patterns (`all`: every leaf has one vector)"""
    bv = RPC.bv_pattern(name, P, seed)
    return np.ones(P, dtype=np.int32) if bv is None else (bv != 0).astype(np.int32)


def same_records(got, want):
    """None when the record arrays are equal by bytes, where an x, y or z that is NaN in both counts as equal; else a description"""
    if got.dtype != want.dtype or got.shape != want.shape:
        return "shape / dtype: %s %s against %s %s" % (got.shape, got.dtype, want.shape, want.dtype)
    g, w = got.copy(), want.copy()
    for k in ("x", "y", "z"):
        both = np.isnan(g[k]) & np.isnan(w[k])
        g[k][both] = 0.0
        w[k][both] = 0.0
    if g.tobytes() == w.tobytes():
        return None
    return RPC._first_difference(g, w)
