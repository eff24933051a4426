"""Clouds of the mapping tests at the sizes where the insertion's leaf kernels span workgroups (test infrastructure).

The conventions of mapping_cases.py hold: res 0.25, sz 8, dyadic anchors with one point exactly on the minimum corner, sheet() -- here
at 40 points per voxel, which keeps the NumPy restatement (mapping_ref.insert) within seconds.  sheet()'s surface leaves its voxel layer
once x or y runs over more than a few voxels (0.05 sin 3x turns negative, 0.03 y climbs), so a large area is laid in tiles of the absolute
3 x 3-voxel lattice, each tile sheet() in its own local coordinates [0, 0.75): the whole surface stays inside one voxel layer, and every
function below asserts the voxel set it promises.

  striped_model / striped_scan   old and new leaves alternate in runs of three along x, 30 rows: 270 + 270 leaves, a rank merge that
                                 interleaves in every row, several blocks of every leaf-indexed kernel
  overlap_scale                  266 old leaves, all three classes on both sides of leaf 256 and leaf 512 of the merged table
  chunk_edge_scan                fresh leaves that own exactly c points, c around the 64-point chunks of the depth-mean chain
  face_probes                    points one voxel outside a grid, next to its boundary leaves (the registration walk's clamped rows)
"""
import numpy as np

import mapping_cases as mc

RES, SZ, MODEL_Z = mc.RES, mc.SZ, mc.MODEL_Z
NPV = 40
TILE = 3


def voxels(xyz, anchor=(0.0, 0.0, 0.0)):
    """floor((x - anchor) / res) per point, in binary64 as every cutter computes it"""
    return np.floor((np.asarray(xyz, dtype=np.float32).astype(np.float64) - np.asarray(anchor, dtype=np.float64)) / RES).astype(np.int64)


def voxel_set(xyz, anchor=(0.0, 0.0, 0.0)):
    return {tuple(v) for v in np.unique(voxels(xyz, anchor), axis=0)}


def tiled_sheet(rng, col0, row0, ncols, nrows, z=MODEL_Z, npv=NPV, layer=0):
    """voxel columns col0 .. col0 + ncols - 1, rows row0 .. row0 + nrows - 1 of voxel layer `layer`, covered by sheet() tile by tile"""
    xs, cs = [], []
    for ty in range(row0 // TILE, (row0 + nrows - 1) // TILE + 1):
        for tx in range(col0 // TILE, (col0 + ncols - 1) // TILE + 1):
            a, b = max(col0, TILE * tx), min(col0 + ncols, TILE * (tx + 1))
            c, d = max(row0, TILE * ty), min(row0 + nrows, TILE * (ty + 1))
            xyz, rgb = mc.sheet(rng, (a - TILE * tx) * RES, (c - TILE * ty) * RES, b - a, d - c, z, npv=npv)
            shift = np.array([TILE * tx * RES, TILE * ty * RES, layer * RES])
            xs.append((xyz.astype(np.float64) + shift).astype(np.float32))
            cs.append(rgb)
    return np.concatenate(xs), np.concatenate(cs)


def _block(col0, row0, ncols, nrows, layer=0):
    return {(x, y, layer) for x in range(col0, col0 + ncols) for y in range(row0, row0 + nrows)}


# ---- striped: old and new keys alternate in runs of three ---------------------------------------------------------------------------
STRIPE_ROWS = 30
A_COLS, B_COLS = (0, 8, 16), (4, 12, 20)
BELOW_CORNER = (-12, -3, -2)                 # voxel coordinates of the second variant's extra block of B (3 x 1 voxels)


def _stripes(rng, cols):
    parts = [tiled_sheet(rng, c, 0, 3, STRIPE_ROWS) for c in cols]
    return np.concatenate([p[0] for p in parts]), np.concatenate([p[1] for p in parts])


def striped_model(seed=21):
    """A: x-columns {0,1,2, 8,9,10, 16,17,18} x 30 y-rows of layer 0 from the corner (0, 0, 0): 270 leaves"""
    xyz, rgb = _stripes(np.random.default_rng(seed), A_COLS)
    xyz[0] = (0.0, 0.0, 0.0)
    want = set().union(*[_block(c, 0, 3, STRIPE_ROWS) for c in A_COLS])
    assert voxel_set(xyz) == want and len(want) == 270
    return xyz, rgb


def striped_scan(below=False, seed=22):
    """B: x-columns {4,5,6, 12,13,14, 20,21,22} x the same 30 rows; columns 3, 7, 11, 15, 19 stay empty, so every B voxel is an empty voxel
    layer away from every A voxel.  below=True: B holds 3 more voxels from BELOW_CORNER on, below A's corner on all three axes: the grid's
    origin shifts on each (koff = 12, 3, 2) and every key field gets one more bit (kmax 34, 32, 2 against 18, 29, 0).
    Returns xyz, rgb (ordered by_voxel), the anchor of the union (its minimum corner)."""
    rng = np.random.default_rng(seed)
    xyz, rgb = _stripes(rng, B_COLS)
    want = set().union(*[_block(c, 0, 3, STRIPE_ROWS) for c in B_COLS])
    corner = (B_COLS[0] * RES, 0.0, 0.0)
    anchor = (0.0, 0.0, 0.0)
    if below:
        bx, by, bz = BELOW_CORNER
        ex, ec = tiled_sheet(rng, bx, by, 3, 1, layer=bz)
        xyz, rgb = np.concatenate([ex, xyz]), np.concatenate([ec, rgb])
        want |= _block(bx, by, 3, 1, bz)
        corner = anchor = (bx * RES, by * RES, bz * RES)
    xyz[0] = corner
    assert voxel_set(xyz) == want and len(want) == 270 + 3 * bool(below)
    assert np.all(xyz.astype(np.float64) >= np.asarray(corner))
    xyz, rgb = mc.by_voxel(xyz, rgb, anchor)
    return xyz, rgb, anchor


# ---- overlap at scale ---------------------------------------------------------------------------------------------------------------
OV_COLS, OV_ROWS = 19, 14
OV_MIN_NBR = 20
OV_BELOW_ROWS = 12                           # the scan's second sheet, two layers below the model: 19 x 12 fresh leaves AHEAD of every old one
OV_HOLES = (7, 14, 126, 133, 252)            # untrained old leaves the scan leaves (all but) empty: idle
OV_LONELY = ((0, 14, -2), (2, 14, -2), (4, 14, -2), (6, 14, -2), (8, 14, -2), (10, 14, -2))    # 5 points each: no leaf, unowned points
OV_SMALL = ((14, 14, -2),)                   # 30 points each: fresh leaves of fewer than 64 sphere points


def overlap_scale(seed=23):
    """dict(model=(xyz, rgb), untrained, scan=(xyz, rgb), min_nbr, n_lonely).

    model: 19 x 14 voxels of layer 0 (P0 = 266 = 256 + 10 = 4 * 66 + 2), leaf i = 19 row + col; every 7th leaf (i % 7 == 0) stays untrained.
    scan:  the model's surface cut afresh, moved by 0.4 res along x and 3 mm in depth, over columns -2 .. 18 and rows 0 .. 15 (two columns
           beyond the model on the low-x side, two rows on the high-y side; the shift carries it into column 19), with holes of radius res
           (three points kept) around the untrained leaves OV_HOLES;
           a second sheet two layers below the model (19 x 12 voxels): with the low-x columns it puts more than 246 new leaves ahead of
           the model's last rows, so that old leaves stand on both sides of merged leaf 512 as well as of leaf 256;
           OV_SMALL: isolated voxels of 30 points; OV_LONELY, last in the scan: isolated voxels of 5 points (< min_nbr)."""
    rng = np.random.default_rng(seed)
    xyz, rgb = tiled_sheet(rng, 0, 0, OV_COLS, OV_ROWS)
    xyz[0] = (0.0, 0.0, 0.0)
    assert voxel_set(xyz) == _block(0, 0, OV_COLS, OV_ROWS)
    untrained = np.arange(0, OV_COLS * OV_ROWS, 7)
    s, c = tiled_sheet(rng, -2, 0, OV_COLS + 2, OV_ROWS + 2)
    s = (s.astype(np.float64) + np.array([0.4 * RES, 0.0, 0.003])).astype(np.float32)
    keep = np.ones(len(s), bool)
    for i in OV_HOLES:
        assert i in untrained
        cen = (np.array([i % OV_COLS, i // OV_COLS, 0]) + 0.5) * RES
        near = np.flatnonzero(np.linalg.norm(s.astype(np.float64) - cen, axis=1) < RES)
        keep[near[3:]] = False
    s, c = s[keep], c[keep]
    parts = [(s, c), tiled_sheet(rng, 0, 0, OV_COLS, OV_BELOW_ROWS, layer=-2)]
    for v, npv in [(v, 30) for v in OV_SMALL] + [(v, 5) for v in OV_LONELY]:
        parts.append(tiled_sheet(rng, v[0], v[1], 1, 1, npv=npv, layer=v[2]))
    sx, sc = np.concatenate([p[0] for p in parts]), np.concatenate([p[1] for p in parts])
    vs = voxel_set(sx)
    assert {v[2] for v in vs} == {-2, 0} and min(v[0] for v in vs) == -2 and min(v[1] for v in vs) == 0
    assert max(v[0] for v in vs) == OV_COLS and max(v[1] for v in vs) == OV_ROWS + 1
    return dict(model=(xyz, rgb), untrained=untrained, scan=(sx, sc), min_nbr=OV_MIN_NBR, n_lonely=5 * len(OV_LONELY))


# ---- chunk edges of the depth-mean chain --------------------------------------------------------------------------------------------
CHUNK_COUNTS = (1, 3, 4, 63, 64, 65, 127, 128, 129, 191, 192, 193, 256, 257)


def chunk_edge_voxels():
    """voxel j (unshifted, in the grid of mapping_cases.model_cloud): every other column of row 5, layer 2 -- an empty layer around each,
    well away from the 3 x 3 model in layer 0"""
    return np.array([(5 + 2 * j, 5, 2) for j in range(len(CHUNK_COUNTS))], dtype=np.int64)


def chunk_edge_scan(seed=24):
    """Voxel j holds exactly CHUNK_COUNTS[j] points, all inside the centred box of half-side res / 4: such a point passes the +-res / 2
    window of ANY frame (|R^T e| <= |e| <= sqrt(3) res / 4 < res / 2) and lies in the search sphere, so with min_nbr = 1 the voxel becomes
    a fresh leaf that owns exactly its own points.  Along z (the normal of the flat box, so the depth) the offsets have random signs and
    magnitudes log-uniform over three decades, which makes the order of a serial sum visible in its last bits.  Points of one voxel are
    consecutive (ascending scan index = patch order).  Returns xyz, rgb."""
    rng = np.random.default_rng(seed)
    xs, cs = [], []
    q = 0.9 * RES / 4
    for v, cnt in zip(chunk_edge_voxels(), CHUNK_COUNTS):
        cen = (v.astype(np.float64) + 0.5) * RES
        e = np.stack([rng.uniform(-q, q, cnt), rng.uniform(-q, q, cnt),
                      rng.choice([-1.0, 1.0], cnt) * q * 10.0 ** rng.uniform(-3.0, 0.0, cnt)], 1)
        p = (cen + e).astype(np.float32)
        assert np.all(np.abs(p.astype(np.float64) - cen) <= RES / 4)
        xs.append(p)
        cs.append(rng.integers(0, 256, (cnt, 3)).astype(np.uint8))
    return np.concatenate(xs), np.concatenate(cs)


# ---- points one voxel outside a grid ------------------------------------------------------------------------------------------------
def face_probes(grid, per_face=12, seed=25):
    """grid: the grid a mapping_ref.insert returned (mn, koff, kmax, vox in shifted coordinates).  For each of the six faces of the grid,
    next to up to per_face boundary leaves: points 1e-4, 2e-3 and 2e-2 res outside the face, jittered by +-0.15 res across it -- inside the
    leaf's search sphere (|e| < 0.57 res), one voxel outside the grid.  Returns xyz (m, 3) float32, face (m,) = 2 axis + (0 low | 1 high)."""
    rng = np.random.default_rng(seed)
    mn, koff, kmax, vox = grid["mn"], grid["koff"], grid["kmax"], grid["vox"]
    out, face = [], []
    for axis in range(3):
        for high in (0, 1):
            edge = kmax[axis] if high else 0
            leaves = vox[vox[:, axis] == edge]
            assert len(leaves) > 0
            for v in leaves[np.linspace(0, len(leaves) - 1, min(per_face, len(leaves))).astype(int)]:
                cen = mn + ((v - koff).astype(np.float64) + 0.5) * RES
                for t in (1e-4, 2e-3, 2e-2):
                    e = rng.uniform(-0.15, 0.15, 3) * RES
                    e[axis] = (0.5 + t) * RES * (1 if high else -1)
                    out.append(cen + e)
                    face.append(2 * axis + high)
    xyz = np.asarray(out).astype(np.float32)
    face = np.asarray(face)
    k = np.floor((xyz.astype(np.float64) - mn) / RES).astype(np.int64) + koff
    for f in range(6):
        ka = k[face == f, f // 2]
        assert np.all(ka == (kmax[f // 2] + 1 if f % 2 else -1)), (f, ka)
    return xyz, face


# ---- comparison helpers (shared by the CPU tests, which also show that each of them can fail, and the GPU tests) ----------------------
FRAME_KEYS = ("R", "mean", "rgb_mean", "W")
ROW_KEYS = ("x0", "x1", "y")


def same_bits(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and np.ascontiguousarray(a).tobytes() == np.ascontiguousarray(b).tobytes()


def owner_of(batch, n):
    """owner of each of the n scan points in a batch (-1: none); every point at most once"""
    own = np.full(n, -1, dtype=np.int32)
    src = batch["src"]
    assert len(np.unique(src)) == len(src) == batch["off"][-1]
    for L in range(len(batch["off"]) - 1):
        own[src[batch["off"][L]:batch["off"][L + 1]]] = L
    return own


def check_union(got, o2n, a, w, n_a, n_b):
    """the insertion `got` (a fetched batch or the restatement's dict) of a disjoint scan of n_b points into the batch `a` of a model of n_a
    points is the batch `w` of the union: the assertions of test_disjoint_scan_is_project_cloud_of_the_union_bit_for_bit"""
    P0, P = len(a["mean"]), len(w["mean"])
    assert len(got["mean"]) == P and len(got["off"]) == P + 1 and len(o2n) == P0 and P > P0 > 0
    # old_to_new: where the union's leaves hold A's points
    holds_a = np.array([np.all(w["src"][w["off"][L]:w["off"][L + 1]] < n_a) for L in range(P)])
    assert np.array_equal(np.flatnonzero(holds_a), o2n), "old_to_new"
    for k in FRAME_KEYS:
        assert same_bits(got[k], w[k]), k
        assert same_bits(got[k][o2n], a[k]), k
    cnt = np.diff(got["off"])
    assert got["off"][0] == 0 and np.all(cnt[o2n] == 0)
    new_leaves = np.setdiff1d(np.arange(P), o2n)
    assert len(new_leaves) == P - P0
    assert np.array_equal(cnt[new_leaves], np.diff(w["off"])[new_leaves]), "off"
    assert len(got["src"]) == cnt.sum() > 0.9 * n_b
    for L in new_leaves:
        s, t = slice(got["off"][L], got["off"][L + 1]), slice(w["off"][L], w["off"][L + 1])
        for k in ROW_KEYS:
            assert same_bits(got[k][s], w[k][t]), (k, L)
        assert same_bits(got["rgb"][:, s], w["rgb"][:, t]), ("rgb", L)
        assert np.array_equal(got["src"][s] + n_a, w["src"][t]), ("src", L)
    return new_leaves


def check_insertion(got, o2n, want, n):
    """the fetched insertion `got` of n scan points against the restatement `want` (evaluated on got's frames): leaf table, offsets, owners,
    rows, means and masks, exactly"""
    P = len(want["cls"])
    assert P > 0 and len(got["off"]) == P + 1 == len(want["off"])
    assert np.array_equal(o2n, want["old_to_new"]), "old_to_new"
    assert np.array_equal(got["off"], want["off"]), "off"
    assert np.array_equal(owner_of(got, n), want["owner"]), "owner"
    assert got["off"][-1] > 0
    for k in ("off", "src") + ROW_KEYS + ("rgb",) + FRAME_KEYS:
        assert same_bits(got[k], want[k]), k


def class_counts(cls, lo, hi):
    """(idle, kept, fresh) among the merged leaves lo .. hi - 1"""
    return tuple(int(np.sum(cls[lo:hi] == k)) for k in (0, 1, 2))
