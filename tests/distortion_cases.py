"""The clouds of the gpc_cloud_distortion tests (tests/test_distortion_gpu.py), and what each claims to hold: exact ties, points on voxel
faces, points outside B's box, an almost empty table, invalid records.  tests/test_distortion_cpu.py checks the claims without a GPU."""
import numpy as np

import distortion_ref as DR

LATTICE_CELLS = (0.0, 0.5, 1.0, 1.5, 100.0)      # 0: the library's choice
SUM_SIZES = (63, 64, 65, 4095, 4096, 4097)


def _colours(rng, n):
    return rng.integers(0, 256, (n, 3)).astype(np.uint8)


def lattice(seed=5, side=6):
    """B: the integer points of a side^3 cube, each at two indices, shuffled.  A: those points (2 candidates each), the edge midpoints
    (4), the face midpoints (8), the cell centres (16): every coordinate is a multiple of 1/2, so every d2 is exact and the ties are
    ties by bits; at cell 0.5, 1 and 1.5 the points lie ON voxel faces.  Returns a, b, and the number of candidates per point of A."""
    rng = np.random.default_rng(seed)
    g = np.arange(side)
    pts = np.stack(np.meshgrid(g, g, g, indexing="ij"), -1).reshape(-1, 3).astype(np.float64)
    b_xyz = np.concatenate([pts, pts])[rng.permutation(2 * len(pts))]
    h = np.arange(side - 1) + 0.5
    groups = [(pts, 2)]
    for axes, ties in (((0,), 4), ((1,), 4), ((2,), 4), ((0, 1), 8), ((0, 2), 8), ((1, 2), 8), ((0, 1, 2), 16)):
        ax = [h if k in axes else g for k in range(3)]
        groups.append((np.stack(np.meshgrid(*ax, indexing="ij"), -1).reshape(-1, 3), ties))
    a_xyz = np.concatenate([p for p, _ in groups])
    ties = np.concatenate([np.full(len(p), t) for p, t in groups])
    order = rng.permutation(len(a_xyz))
    a_xyz, ties = a_xyz[order], ties[order]
    return DR.make_cloud(a_xyz, _colours(rng, len(a_xyz))), DR.make_cloud(b_xyz, _colours(rng, len(b_xyz))), ties


def outside_box(cell=0.1, seed=6):
    """B: 300 points in the unit cube.  A: at 0.1, 3 and 40 cell sides outside B's box, beyond each of its six faces and beyond a corner"""
    rng = np.random.default_rng(seed)
    b_xyz = rng.uniform(0, 1, (300, 3)).astype(np.float32)
    lo, hi = b_xyz.min(0).astype(np.float64), b_xyz.max(0).astype(np.float64)
    rows = []
    for k in (0.1, 3.0, 40.0):
        for ax in range(3):
            for side in (0, 1):
                p = rng.uniform(lo, hi)
                p[ax] = lo[ax] - k * cell if side == 0 else hi[ax] + k * cell
                rows.append(p)
        rows.append(hi + k * cell)
    a_xyz = np.array(rows, dtype=np.float32)
    return DR.make_cloud(a_xyz, _colours(rng, len(a_xyz))), DR.make_cloud(b_xyz, _colours(rng, len(b_xyz))), cell


def sparse_table(cell=0.01, seed=7):
    """B: 500 points in one voxel and one point 200 voxels away along x: a table of two occupied voxels in a row of 201.  A: points near
    both, and points half-way between, 100 empty voxels from either."""
    rng = np.random.default_rng(seed)
    far = np.array([200.5 * cell, 0.4 * cell, 0.6 * cell])
    b_xyz = np.concatenate([rng.uniform(0, cell, (500, 3)), far[None]]).astype(np.float32)
    near = rng.uniform(-cell, 2 * cell, (40, 3))
    at_far = far + rng.uniform(-cell, cell, (20, 3))
    mid = np.stack([rng.uniform(99 * cell, 102 * cell, 30), rng.uniform(-2 * cell, 3 * cell, 30), rng.uniform(-2 * cell, 3 * cell, 30)], 1)
    a_xyz = np.concatenate([near, at_far, mid]).astype(np.float32)
    return DR.make_cloud(a_xyz, _colours(rng, len(a_xyz))), DR.make_cloud(b_xyz, _colours(rng, len(b_xyz))), cell


def random_pair(na, nb, seed, spread=1.0):
    """two noisy samples of one wavy sheet, random colours"""
    rng = np.random.default_rng(seed)

    def sheet(n):
        u, v = rng.uniform(0, spread, n), rng.uniform(0, spread, n)
        return np.stack([u, v, 0.05 * np.sin(5 * u) * np.cos(4 * v) + rng.normal(0, 0.004, n)], 1).astype(np.float32)
    return DR.make_cloud(sheet(na), _colours(rng, na)), DR.make_cloud(sheet(nb), _colours(rng, nb))


def with_invalid(cloud, seed, share=0.15):
    """some records with a NaN, +inf or -inf coordinate: returns the cloud and the mask of the records hit"""
    rng = np.random.default_rng(seed)
    c = cloud.copy()
    hit = rng.random(len(c)) < share
    for i in np.flatnonzero(hit):
        c[("x", "y", "z")[rng.integers(3)]][i] = (np.nan, np.inf, -np.inf)[rng.integers(3)]
    return c, hit


def organised(width=40, height=30, seed=8, miss=0.3):
    """a render-style organised cloud: record v * width + u is pixel (u, v) of a depth image of a wavy wall; misses are x = y = z = NaN"""
    rng = np.random.default_rng(seed)
    u, v = np.meshgrid(np.arange(width), np.arange(height))
    x, y = (u.ravel() - width / 2) * 0.01, (v.ravel() - height / 2) * 0.01
    z = 1.0 + 0.03 * np.sin(9 * x) * np.cos(7 * y)
    xyz = np.stack([x * z, y * z, z], 1).astype(np.float32)
    holes = rng.random(len(xyz)) < miss
    xyz[holes] = np.nan
    rgb = _colours(rng, len(xyz))
    rgb[holes] = 0
    return DR.make_cloud(xyz, rgb), holes


def unit_normals(n, seed, nan_share=0.2, zeros=3):
    """random unit normals (float32); some rows NaN in one component, a few all zero.  Returns normals, the NaN rows, the zero rows"""
    rng = np.random.default_rng(seed)
    v = rng.normal(size=(n, 3))
    v = (v / np.linalg.norm(v, axis=1, keepdims=True)).astype(np.float32)
    bad = rng.random(n) < nan_share
    v[bad, rng.integers(0, 3, int(bad.sum()))] = np.nan
    zero = rng.choice(np.flatnonzero(~bad), zeros, replace=False)
    v[zero] = 0.0
    return v, bad, zero


def two_planes(n=6000, seed=9):
    """a floor and a wall meeting at a right angle: near the edge the fitted frames are tilted, and some points fall in no leaf's window"""
    rng = np.random.default_rng(seed)
    h = n // 2
    floor = np.stack([rng.uniform(0, 0.6, h), rng.uniform(0, 0.6, h), rng.normal(0, 0.002, h)], 1)
    wall = np.stack([rng.normal(0, 0.002, n - h), rng.uniform(0, 0.6, n - h), rng.uniform(0, 0.6, n - h)], 1)
    return np.concatenate([floor, wall]).astype(np.float32), _colours(rng, n)
