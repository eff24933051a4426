"""Synthetic clouds of the mapping tests (test infrastructure): gently curved sheets of about 150 points per voxel at res = 0.25.

Every cloud has one point exactly on a dyadic minimum corner, and all coordinates are small dyadic-anchored floats, so (x - mn) / res,
the voxel centres and p - centre are exact in binary64 and a whole-voxel shift of the anchor is invisible: project_cloud(A + B)
then cuts A's leaves exactly as project_cloud(A) does.
"""
import numpy as np

RES, SZ = 0.25, 8
# height of the model sheet: well below the voxel centres (0.125), so that a fresh leaf's window (around the centre, in a tilted frame)
# and a kept neighbour's (around its mean on the surface) overlap in a sliver that holds scan points
MODEL_Z = 0.04


def sheet(rng, x0, y0, nx, ny, z, npv=150):
    """nx x ny voxels of a curved sheet at height z, npv points per voxel on average: xyz (n, 3) float32, rgb (n, 3) uint8"""
    n = nx * ny * npv
    x = x0 + rng.random(n) * nx * RES
    y = y0 + rng.random(n) * ny * RES
    zz = z + 0.05 * np.sin(3 * x) + 0.03 * y + 0.002 * rng.standard_normal(n)
    xyz = np.stack([x, y, zz], 1).astype(np.float32)
    rgb = np.clip(np.stack([120 + 80 * np.sin(9 * x), 100 + 300 * (y - y0), 90 + 60 * np.cos(7 * (x + y))], 1)
                  + rng.integers(-8, 9, (n, 3)), 0, 255).astype(np.uint8)
    return xyz, rgb


def by_voxel(xyz, rgb, anchor):
    """the cloud re-ordered by voxel in ascending (z, y, x), scan order kept inside a voxel: a leaf's search-sphere hit order (the
    producer's patch order) and ascending scan index (the insertion's patch order) then coincide"""
    k = np.floor((xyz.astype(np.float64) - np.asarray(anchor, dtype=np.float64)) / RES).astype(np.int64)
    o = np.lexsort((np.arange(len(k)), k[:, 0], k[:, 1], k[:, 2]))
    return xyz[o], rgb[o]


def model_cloud(seed=1):
    """A: 3 x 3 voxels from the corner (0, 0, 0)"""
    rng = np.random.default_rng(seed)
    xyz, rgb = sheet(rng, 0.0, 0.0, 3, 3, MODEL_Z)
    xyz[0] = (0.0, 0.0, 0.0)
    return xyz, rgb


def disjoint_scan(where, seed=2):
    """B: 2 voxels, an empty voxel layer (at least) away from A on every axis it differs in.  'above': beyond A's maximum corner
    (the grid grows upwards only); 'below': below A's minimum corner on all three axes (the origin shifts on each)."""
    rng = np.random.default_rng(seed)
    if where == "above":
        corner = (1.25, 1.0, 0.75)
        xyz, rgb = sheet(rng, corner[0], corner[1], 2, 1, 0.84)
    else:
        corner = (-1.0, -0.75, -0.75)
        xyz, rgb = sheet(rng, corner[0], corner[1], 2, 1, -0.6)
    xyz[0] = corner
    assert np.all(xyz >= np.asarray(corner, dtype=np.float32))
    return by_voxel(xyz, rgb, corner)


def overlapping_scan(seed=3):
    """A's surface moved by 0.4 res along x and 3 mm in depth, with
      * the points around voxel (0, 2, 0) removed but for three (an untrained old leaf there is not re-cut),
      * 30 points in an isolated voxel (a fresh leaf with fewer than 64 sphere points),
      * 5 points in another isolated voxel (below min_nbr = 20: no leaf, the points stay unowned)."""
    rng = np.random.default_rng(seed)
    xyz, rgb = sheet(rng, 0.0, 0.0, 3, 3, MODEL_Z)
    xyz = (xyz.astype(np.float64) + np.array([0.4 * RES, 0.0, 0.003])).astype(np.float32)
    cen = np.array([0.125, 0.625, 0.125])
    near = np.linalg.norm(xyz.astype(np.float64) - cen, axis=1) < 0.25
    keep = ~near
    keep[np.flatnonzero(near)[:3]] = True
    xyz, rgb = xyz[keep], rgb[keep]
    ix, ic = sheet(rng, 1.5, 0.0, 1, 1, MODEL_Z, npv=30)
    jx, jc = sheet(rng, 0.0, 1.5, 1, 1, MODEL_Z, npv=5)
    return np.concatenate([xyz, ix, jx]), np.concatenate([rgb, ic, jc])
