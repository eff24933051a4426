"""NumPy restatement of the map insertion (test infrastructure; the product never imports this module).

gp_mapping::insert_into_map (src/gp_mapping.cpp:37-152) with transform_to_old (:213-243) and transform_to_new (:245-291), stated as
the project states the producer and the registration assignment: a scan point belongs to the first leaf, in merged leaf order, that
accepts it.  Built on registration_ref (key packing, local_coords).  Voxels are handled in UNSHIFTED integer coordinates
c = floor((x - mn) / res), which may be negative; the device's shifted coordinate is c + koff.

Every floating-point expression is evaluated in the association the GPU kernels use (NumPy's element-wise operations do not
contract; sequential sums are cumsum), so owners, local coordinates and fresh-leaf means can be compared exactly.
"""
import numpy as np

import registration_ref as ref

IDLE, KEPT, FRESH = 0, 1, 2


def model_grid(model_xyz, res, sz):
    """grid of a first model (registration_ref.grid_of) plus what the insertion needs: sz, koff = 0, the leaves' voxel coordinates"""
    g = ref.grid_of(model_xyz, res)
    k = g["keys"]
    m = (1 << ref.B) - 1
    g.update(sz=int(sz), koff=np.zeros(3, np.int64), vox=np.stack([k & m, (k >> ref.B) & m, k >> (2 * ref.B)], 1).astype(np.int64))
    return g


def _order(vox):
    """row order of ascending (z, y, x)"""
    return np.lexsort((vox[:, 0], vox[:, 1], vox[:, 2]))


def _seq_sum(a):
    """sum of the rows of a, one after the other"""
    return np.cumsum(a, axis=0)[-1] if len(a) else np.zeros(a.shape[1:])


def insert(model, grid, trained, scan_xyz, scan_rgb, min_nbr, frames=None, compute_rotation=None):
    """model: fetched batch of the map (R (P, 3, 3), mean, rgb_mean, W); grid: model_grid() or the grid a previous insert returned;
    trained (P,) bool.  Fresh-leaf frames come from frames[(leaf id)] (array (P', 3, 3), e.g. the GPU's own) if given, else from
    compute_rotation(M, k) (oracle_lib.compute_rotation).  Returns a dict: the new batch (off, x0, x1, y, rgb, src, R, mean, rgb_mean,
    W), vox (P', 3), cls (P',), old_to_new (P,), grid."""
    p32 = np.asarray(scan_xyz, dtype=np.float32).reshape(-1, 3)
    p = p32.astype(np.float64)
    col = np.asarray(scan_rgb, dtype=np.uint8).reshape(-1, 3).astype(np.float64)
    n = len(p)
    mn, res, sz = grid["mn"], grid["res"], grid["sz"]
    r2, half = grid["radius"] * grid["radius"], grid["half"]
    P0 = len(grid["vox"])
    vox0 = grid["vox"] - grid["koff"]                                     # unshifted
    old_of = {tuple(v): i for i, v in enumerate(vox0)}
    c = np.floor((p - mn) / res).astype(np.int64) if n else np.zeros((0, 3), np.int64)
    # the scan's voxels, each with its points in ascending scan index
    pts_of = {}
    for i in range(n):
        pts_of.setdefault(tuple(c[i]), []).append(i)

    def centre(v):
        return mn + (np.asarray(v, dtype=np.float64) + 0.5) * res

    def sphere(v):
        """scan points in the search sphere of voxel v, in hit order: neighbour voxels in (dz, dy, dx) order, ascending index inside"""
        cen = centre(v)
        hits = []
        for dz in (-1, 0, 1):
            for dy in (-1, 0, 1):
                for dx in (-1, 0, 1):
                    idx = pts_of.get((v[0] + dx, v[1] + dy, v[2] + dz))
                    if idx is None:
                        continue
                    idx = np.asarray(idx)
                    d = p[idx] - cen
                    hits.extend(idx[d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1] + d[:, 2] * d[:, 2] <= r2].tolist())
        return np.asarray(hits, dtype=np.int64)

    # leaves of the result: every old leaf, every new voxel with >= min_nbr scan points in its sphere (:126)
    spheres = {}
    new_vox = []
    for v in pts_of:
        if v not in old_of:
            spheres[v] = sphere(v)
            if len(spheres[v]) >= min_nbr:
                new_vox.append(v)
    vox = np.concatenate([vox0, np.asarray(new_vox, dtype=np.int64).reshape(-1, 3)])
    order = _order(vox)
    vox = vox[order]
    P = len(vox)
    pos = np.empty(P, np.int64)
    pos[order] = np.arange(P)
    o2n = pos[:P0].astype(np.int32)
    leaf_of = {tuple(v): L for L, v in enumerate(vox)}
    # classes and frames
    cls = np.zeros(P, np.int32)
    R = np.zeros((P, 3, 3))
    org = np.zeros((P, 3))
    for L in range(P):
        v = tuple(vox[L])
        i = old_of.get(v)
        if i is not None and trained[i]:
            cls[L] = KEPT
        else:
            if v not in spheres:
                spheres[v] = sphere(v)
            cls[L] = FRESH if (i is None or len(spheres[v]) >= min_nbr) else IDLE
        if cls[L] == FRESH:
            if frames is not None:
                R[L] = frames[L]
            else:
                h = spheres[v]
                p4 = np.concatenate([p[h], np.ones((len(h), 1))], axis=1)
                M = _seq_sum(p4[:, :, None] * p4[:, None, :]) if len(h) else np.zeros((4, 4))
                R[L] = compute_rotation(M, len(h))
            org[L] = centre(v)
        else:
            R[L] = model["R"][i]
            org[L] = model["mean"][i]
    # ownership: candidates in ascending leaf order = ascending (dz, dy, dx)
    owner = np.full(n, -1, dtype=np.int32)
    local = np.zeros((n, 3))
    for dz in (-1, 0, 1):
        for dy in (-1, 0, 1):
            for dx in (-1, 0, 1):
                idx = np.flatnonzero(owner < 0)
                if len(idx) == 0:
                    continue
                nb = c[idx] + np.array([dx, dy, dz])
                L = np.array([leaf_of.get(tuple(v), -1) for v in nb], dtype=np.int64)
                ok = L >= 0
                ok[ok] = cls[L[ok]] != IDLE
                idx, L, nb = idx[ok], L[ok], nb[ok]
                if len(idx) == 0:
                    continue
                cen = mn + (nb.astype(np.float64) + 0.5) * res
                d = p[idx] - cen
                ok = d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1] + d[:, 2] * d[:, 2] <= r2            # radiusSearch (:96)
                idx, L = idx[ok], L[ok]
                q = ref.local_coords(p[idx], R[L], org[L])
                ok = ~((q[:, 1] > half) | (q[:, 1] < -half) | (q[:, 2] > half) | (q[:, 2] < -half))
                owner[idx[ok]] = L[ok]
                local[idx[ok]] = q[ok]
    # the batch: patch order, ascending scan index inside a patch
    src, off = ref.bucket(owner, P)
    total = int(off[P])
    src = src[:total].astype(np.int32)
    x0, x1, y = local[src, 1].copy(), local[src, 2].copy(), local[src, 0].copy()
    rgb = np.zeros((3, total))
    mean, rgb_mean = np.zeros((P, 3)), np.zeros((P, 3))
    W = np.zeros((P, sz * sz), np.uint8)
    for L in range(P):
        sl = slice(off[L], off[L + 1])
        cnt = off[L + 1] - off[L]
        i = old_of.get(tuple(vox[L]))
        if cls[L] == FRESH:
            mean[L] = org[L]
            if cnt > 0:
                mnd = _seq_sum(y[sl, None])[0] / float(cnt)
                rgb_mean[L] = col[src[sl]].sum(axis=0) / float(cnt)                                # integers: exact in any order
                y[sl] = y[sl] - mnd
                mean[L] = org[L] + mnd * R[L][:, 0]
        else:
            mean[L], rgb_mean[L] = model["mean"][i], model["rgb_mean"][i]
            W[L] = model["W"][i]                                                                     # :242 | untouched
        rgb[:, sl] = (col[src[sl]] - rgb_mean[L]).T
        if cnt > 0:
            gx = np.clip((float(sz) * (x0[sl] / res + 0.5)).astype(np.int64), 0, sz - 1)
            gy = np.clip((float(sz) * (x1[sl] / res + 0.5)).astype(np.int64), 0, sz - 1)
            W[L, sz * gx + gy] = 1
    # the grown grid
    koff = grid["koff"].copy()
    kmax = grid["kmax"].copy()
    if n:
        koff = np.maximum(grid["koff"], -c.min(axis=0))
        kmax = np.maximum(grid["kmax"] - grid["koff"], c.max(axis=0)) + koff
    sh = vox + koff
    g = dict(grid, koff=koff, kmax=kmax, vox=sh, keys=ref._key(sh[:, 0], sh[:, 1], sh[:, 2]))
    return dict(off=off, x0=x0, x1=x1, y=y, rgb=rgb, src=src, R=R, mean=mean, rgb_mean=rgb_mean, W=W, vox=vox, cls=cls,
                old_to_new=o2n, owner=owner, local=local, grid=g)


def registration_grid(grid):
    """the grid as registration_ref.assign reads it: unshifted coordinates from an anchor moved down by koff whole voxels (exact when
    mn and res are dyadic, as in the tests)"""
    return dict(grid, mn=grid["mn"] - grid["koff"].astype(np.float64) * grid["res"])
