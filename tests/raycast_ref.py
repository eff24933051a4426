"""NumPy restatement of the ray cast (test infrastructure; the product never imports this module).

gp_mapping::train_classification (src/gp_mapping.cpp:154-211): every scan ray, from the sensor to its point, labels the cell it meets
on the plane of every trained leaf between the sensor and the leaf that owns the point -- occupied on the owner's plane, free on the
others.  Two formulations of the write:
  (a) cells_sequential: the scan in index order, every write as it comes (:167-210: the last scan index wins a cell);
  (b) cells_maxkey: the largest key (i + 1) << 1 | is_free per (leaf, cell), which is what the kernels do with atomicMax.
Both consume the same list of events, which cast() produces ray by ray with the per-ray rule of csrc/raycast.hip: slab test on the
owner's voxel, then a walk from that voxel back towards the sensor across the entry face of the voxel in hand.  occupancy_batch()
restates gpc_occupancy_batch_dev.

Built on registration_ref / mapping_ref: `grid` is mapping_ref.model_grid() or the grid mapping_ref.insert() returns; voxels are
handled in UNSHIFTED integer coordinates c = k - koff.  Every floating-point expression is evaluated in the association the kernels
use, on np.float64 / np.float32 scalars (no contraction), so cells and counts can be compared exactly.
"""
import numpy as np

UNOBSERVED, OCCUPIED, FREE = 0, 1, 2
INF = np.float64(np.inf)


def owner_of(batch, n):
    """gp_indices: the leaf whose bucket holds scan point i, -1 = unowned"""
    own = np.full(n, -1, dtype=np.int64)
    off, src = batch["off"], batch["src"]
    for L in range(len(off) - 1):
        own[src[off[L]:off[L + 1]]] = L
    return own


def ray_of(p32, origin):
    """o (3,) float64 = double(float(origin)); delta (3,) float64 = double(p - float(origin)), the difference taken in float (:169)"""
    o32 = np.asarray(origin, dtype=np.float64).astype(np.float32)
    d32 = np.asarray(p32, dtype=np.float32) - o32
    return o32.astype(np.float64), d32.astype(np.float64)


def faces(grid, c):
    """low and high faces of the voxel with unshifted coordinates c"""
    c = np.asarray(c, dtype=np.int64)
    return grid["mn"] + c.astype(np.float64) * grid["res"], grid["mn"] + (c + 1).astype(np.float64) * grid["res"]


def slab(grid, c, o, delta):
    """(meets, near, far) of the ray o + t delta against voxel c: per axis near / far = min / max of the two face parameters; an axis
    with delta == 0 needs lo <= o < hi and counts as -inf / +inf"""
    lo, hi = faces(grid, c)
    tn, tf, ok = -INF, INF, True
    with np.errstate(divide="ignore", over="ignore"):
        for a in range(3):
            if delta[a] != 0.0:
                t1, t2 = (lo[a] - o[a]) / delta[a], (hi[a] - o[a]) / delta[a]
                tn, tf = max(tn, min(t1, t2)), min(tf, max(t1, t2))
            elif not (lo[a] <= o[a] < hi[a]):
                ok = False
    return bool(ok and tn <= tf and tf >= 0.0), tn, tf


def walk(grid, c_owner, o, delta):
    """the unshifted voxels the walk visits, the owner's first"""
    c = np.asarray(c_owner, dtype=np.int64).copy()
    lo_c, hi_c = -grid["koff"], grid["kmax"] - grid["koff"]
    out = []
    for _ in range(int(np.sum(grid["kmax"])) + 1):
        out.append(tuple(int(v) for v in c))
        best, ax = -INF, -1
        with np.errstate(divide="ignore", over="ignore"):
            for a in range(3):
                if delta[a] == 0.0:
                    continue
                kf = c[a] if delta[a] > 0.0 else c[a] + 1
                na = ((grid["mn"][a] + np.float64(kf) * grid["res"]) - o[a]) / delta[a]
                if na > best:                                             # strict: the first axis that attains the maximum
                    best, ax = na, a
        if ax < 0 or not best > 0.0:                                      # the sensor is in or behind this voxel
            break
        c[ax] += -1 if delta[ax] > 0.0 else 1
        if c[ax] < lo_c[ax] or c[ax] > hi_c[ax]:
            break
    return out


def plane_cell(R, mean, origin, delta, res, sz):
    """:191-202 for one leaf: the cell the ray origin + d delta meets on its plane, or -1 (window missed, or d / loc not finite)"""
    org = np.asarray(origin, dtype=np.float64)
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        num = R[0, 0] * (mean[0] - org[0]) + R[1, 0] * (mean[1] - org[1]) + R[2, 0] * (mean[2] - org[2])
        den = R[0, 0] * delta[0] + R[1, 0] * delta[1] + R[2, 0] * delta[2]
        d = num / den
        e = [(org[a] + d * delta[a]) - mean[a] for a in range(3)]
        t = [R[0, a] * e[0] + R[1, a] * e[1] + R[2, a] * e[2] for a in range(3)]
    if not (np.isfinite(d) and np.all(np.isfinite(t))):
        return -1
    half = res / 2.0
    if t[1] > half or t[1] < -half or t[2] > half or t[2] < -half:
        return -1
    gx = min(max(int(float(sz) * (t[1] / res + 0.5)), 0), sz - 1)
    gy = min(max(int(float(sz) * (t[2] / res + 0.5)), 0), sz - 1)
    return sz * gx + gy


def cast(batch, grid, trained, scan_xyz, origin, owner=None):
    """batch: fetched batch of the map (R (P, 3, 3), mean (P, 3), off, src); trained (P,) bool or None (every leaf); owner: (n,) or None
    (from the batch).  Returns dict(events = [(i, leaf, cell, is_free)] in scan order, far leaf first inside a ray; noop (n,) bool;
    misses (n,) bool: owned by a trained leaf whose voxel the ray does not meet; counts = [rays, no-ops, occupied writes, free writes];
    visited = {i: [unshifted voxels]} of the rays that walk)"""
    p32 = np.asarray(scan_xyz, dtype=np.float32).reshape(-1, 3)
    n = len(p32)
    P = len(batch["mean"])
    res, sz = grid["res"], grid["sz"]
    vox = grid["vox"] - grid["koff"]
    leaf_of = {tuple(int(x) for x in v): L for L, v in enumerate(vox)}
    trained = np.ones(P, bool) if trained is None else np.asarray(trained, dtype=bool)
    own = owner_of(batch, n) if owner is None else np.asarray(owner)
    events, visited = [], {}
    noop, misses = np.ones(n, bool), np.zeros(n, bool)
    for i in range(n):
        m = int(own[i])
        if m < 0 or not trained[m]:
            continue
        o, delta = ray_of(p32[i], origin)
        if not slab(grid, vox[m], o, delta)[0]:
            misses[i] = True
            continue
        noop[i] = False
        visited[i] = walk(grid, vox[m], o, delta)
        for c in visited[i]:
            L = leaf_of.get(c, -1)
            if L < 0 or not trained[L]:
                continue
            cell = plane_cell(batch["R"][L], batch["mean"][L], origin, delta, res, sz)
            if cell >= 0:
                events.append((i, L, cell, int(L != m)))
    nfree = sum(e[3] for e in events)
    counts = np.array([n, int(noop.sum()), len(events) - nfree, nfree], dtype=np.int32)
    return dict(events=events, noop=noop, misses=misses, counts=counts, visited=visited, owner=own)


def cells_sequential(events, cells0):
    """(a): the writes in the order the sequential loop makes them"""
    cells = np.array(cells0, dtype=np.uint8, copy=True)
    for i, L, cell, is_free in events:
        cells[L, cell] = FREE if is_free else OCCUPIED
    return cells


def cells_maxkey(events, cells0):
    """(b): the largest key per (leaf, cell), then the resolve"""
    cells = np.array(cells0, dtype=np.uint8, copy=True)
    key = np.zeros(cells.shape, dtype=np.uint32)
    for i, L, cell, is_free in events:
        key[L, cell] = max(int(key[L, cell]), ((i + 1) << 1) | is_free)
    cells[(key != 0) & (key & 1 == 1)] = FREE
    cells[(key != 0) & (key & 1 == 0)] = OCCUPIED
    return cells


def both_ways(events, shape):
    """(P, m) bool: cells that an occupied write and a free write both reach"""
    occ, fre = np.zeros(shape, bool), np.zeros(shape, bool)
    for i, L, cell, is_free in events:
        (fre if is_free else occ)[L, cell] = True
    return occ & fre


def occupancy_batch(cells, res, sz):
    """gpc_occupancy_batch_dev: per leaf the observed cells in ascending cell index at their centres (src/gp_compressor.cpp:326-327),
    y = +1 occupied / -1 free: off (P + 1,), x0, x1, y"""
    cells = np.asarray(cells)
    P = cells.shape[0]
    L, c = np.nonzero(cells != UNOBSERVED)                                # row-major: ascending leaf, ascending cell inside
    off = np.concatenate([[0], np.cumsum(np.bincount(L, minlength=P))]).astype(np.int32)
    gx, gy = c // sz, c % sz
    x0 = res * ((gx.astype(np.float64) + 0.5) / float(sz) - 0.5)
    x1 = res * ((gy.astype(np.float64) + 0.5) / float(sz) - 0.5)
    y = np.where(cells[L, c] == OCCUPIED, 1.0, -1.0)
    return off, x0, x1, y
