"""CPU tests (-m "not gpu") of the NumPy restatement of the ray cast (tests/raycast_ref.py): what the GPU tests compare the kernels
with is pinned here without a GPU -- the two formulations of the write against each other, closed-form scenes, and the voxel walk
against a brute-force slab test over every voxel of the grid.  Scenes: tests/raycast_cases.layered_map (res 0.25, sz 8)."""
import numpy as np

import raycast_cases as rcs
import raycast_ref as rr

RES, SZ = rcs.RES, rcs.SZ


def _scene(order="shuffled", seed=4):
    """two tilted layers of 3 x 3 leaves two voxel layers apart, a sensor above; about 40 points per leaf on the lower layer, on the upper
    one only on the leaves of its first column.  order: "shuffled", or "upper first" (every point of the upper layer before every
    point of the lower one)"""
    batch, grid = rcs.layered_map([(0, 0.02), (2, -0.03)], kz_max=4, tilt=0.08, seed=seed)
    rng = np.random.default_rng(seed)
    lower, upper = [], []
    for L in range(18):
        if L >= 9 and grid["vox"][L][0] != 0:
            continue
        u, v = rng.uniform(-0.12, 0.12, 40), rng.uniform(-0.12, 0.12, 40)
        (upper if L >= 9 else lower).append(rcs.points_on(batch, grid, L, u, v))
    lower, upper = np.concatenate(lower), np.concatenate(upper)
    xyz = np.concatenate([upper, lower])
    if order == "shuffled":
        xyz = xyz[rng.permutation(len(xyz))]
    batch, owner = rcs.own(batch, grid, xyz)
    return batch, grid, xyz, owner, np.array([0.31, 0.44, 1.3])


def test_sequential_and_max_key_formulations_agree():
    batch, grid, xyz, owner, sensor = _scene()
    out = rr.cast(batch, grid, None, xyz, sensor)
    ev = out["events"]
    zero = np.zeros((18, SZ * SZ), np.uint8)
    a, b = rr.cells_sequential(ev, zero), rr.cells_maxkey(ev, zero)
    assert np.array_equal(a, b)
    # the scene holds what the comparison is about
    assert out["counts"][2] > 100 and out["counts"][3] > 100 and rr.both_ways(ev, zero.shape).sum() >= 5
    assert np.sum(owner >= 0) > 0.9 * len(xyz) and out["counts"][0] == len(xyz)
    assert out["counts"][1] == out["noop"].sum() == np.sum(owner < 0) + out["misses"].sum()
    assert np.all(a[:9][a[:9] != 0] == rr.OCCUPIED) and np.any(a[9:] == rr.FREE) and np.any(a[9:] == rr.OCCUPIED)
    # a pre-filled buffer keeps its values where nothing is written, in both formulations
    pre = np.random.default_rng(0).integers(0, 3, zero.shape).astype(np.uint8)
    a2, b2 = rr.cells_sequential(ev, pre), rr.cells_maxkey(ev, pre)
    assert np.array_equal(a2, b2) and np.array_equal(a2[a == 0], pre[a == 0]) and np.array_equal(a2[a != 0], a[a != 0])


def test_reversed_scan_flips_exactly_the_cells_written_both_ways():
    """With every point of the upper layer before every point of the lower one, each cell that both kinds of ray write is written
    occupied first and free last, so the reversed scan flips exactly those cells.  (In an arbitrary order a cell written
    occupied - free - occupied would not flip: the general statement, asserted on the shuffled scene, is that the cells that change are
    those whose first and last write differ in kind.)"""
    zero = np.zeros((18, SZ * SZ), np.uint8)
    for order in ("upper first", "shuffled"):
        batch, grid, xyz, owner, sensor = _scene(order)
        n = len(xyz)
        ev = rr.cast(batch, grid, None, xyz, sensor)["events"]
        rev_batch, _ = rcs.own(dict(R=batch["R"], mean=batch["mean"]), grid, xyz[::-1])
        ev_rev = rr.cast(rev_batch, grid, None, xyz[::-1], sensor)["events"]
        assert sorted((n - 1 - i, L, c, f) for i, L, c, f in ev_rev) == sorted(ev)      # the same writes, renumbered
        fwd, rev = rr.cells_maxkey(ev, zero), rr.cells_maxkey(ev_rev, zero)
        both = rr.both_ways(ev, zero.shape)
        first, last = {}, {}
        for i, L, c, f in ev:
            first.setdefault((L, c), f)
            last[(L, c)] = f
        differ = np.zeros(zero.shape, bool)
        for k in first:
            differ[k] = first[k] != last[k]
        assert np.array_equal(fwd != rev, differ) and np.all(both[differ]) and differ.sum() >= 5
        if order == "upper first":
            assert np.array_equal(fwd != rev, both)
            assert np.all(fwd[both] == rr.FREE) and np.all(rev[both] == rr.OCCUPIED)


def test_one_flat_leaf_under_the_sensor_gives_its_mask():
    """dyadic points on a flat leaf, a dyadic sensor: p - o is exact in float, d is exactly 1, the intersection is the point itself --
    every ray marks the cell its point lies in, which is the leaf's W"""
    batch, grid = rcs.layered_map([(0, 0.0)], kz_max=6, nx=1, ny=1)
    rng = np.random.default_rng(1)
    u, v = rng.integers(-127, 128, 200) / 1024.0, rng.integers(-127, 128, 200) / 1024.0
    xyz = rcs.points_on(batch, grid, 0, u, v)
    assert np.array_equal(xyz.astype(np.float64), batch["mean"][0] + np.stack([u, v, 0 * u], 1))
    batch, owner = rcs.own(batch, grid, xyz)
    assert np.all(owner == 0)
    out = rr.cast(batch, grid, None, xyz, np.array([0.375, 0.25, 1.5]))
    cells = rr.cells_maxkey(out["events"], np.zeros((1, SZ * SZ), np.uint8))
    W = np.zeros((1, SZ * SZ), np.uint8)
    gx = np.clip((float(SZ) * (u / RES + 0.5)).astype(np.int64), 0, SZ - 1)
    gy = np.clip((float(SZ) * (v / RES + 0.5)).astype(np.int64), 0, SZ - 1)
    W[0, SZ * gx + gy] = 1
    assert np.array_equal(cells, W) and W.sum() > 40
    assert [(i, L, f) for i, L, c, f in out["events"]] == [(i, 0, 0) for i in range(200)]
    assert np.array_equal(out["counts"], [200, 0, 200, 0])


def test_two_parallel_layers_free_cell_by_similar_triangles():
    batch, grid = rcs.layered_map([(0, 0.0), (2, 0.0)], kz_max=3)
    sensor = np.array([0.375, 0.375, 2.125])                               # above the centre of the middle column; dyadic
    z_lo, z_up = batch["mean"][0][2], batch["mean"][9][2]
    # a point of the lower layer's leaf (0, 0); the ray climbs towards the sensor's column and crosses the upper plane at
    # s + (z_up - s_z) / (p_z - s_z) (p - s)
    p = np.array([[0.0625 + 1 / 64, 0.1875 + 1 / 64, z_lo]], dtype=np.float32)
    batch, owner = rcs.own(batch, grid, p)
    assert owner[0] == 0
    out = rr.cast(batch, grid, None, p, sensor)
    q = sensor + (z_up - sensor[2]) / (float(p[0, 2]) - sensor[2]) * (p[0].astype(np.float64) - sensor)
    k = np.floor(q / RES).astype(int)
    L_up = 9 + 3 * k[1] + k[0]
    assert k[2] == 2 and tuple(grid["vox"][L_up]) == tuple(k)
    loc = q - batch["mean"][L_up]                                           # FLAT frame: u = x, v = y
    frac = SZ * (loc[:2] / RES + 0.5)
    assert np.all(np.abs(frac - np.round(frac)) > 1e-3)                    # well inside a cell: rounding cannot move it
    cell_up = SZ * int(frac[0]) + int(frac[1])
    own_loc = p[0].astype(np.float64) - batch["mean"][0]
    cell_own = SZ * int(SZ * (own_loc[0] / RES + 0.5)) + int(SZ * (own_loc[1] / RES + 0.5))
    # far leaf first: the owner's occupied cell, then the free cell on the upper layer; the planes of the other leaves the ray passes
    # are met outside their windows
    assert out["events"] == [(0, 0, cell_own, 0), (0, L_up, cell_up, 1)]
    cells = rr.cells_sequential(out["events"], np.zeros((18, SZ * SZ), np.uint8))
    assert cells[0, cell_own] == rr.OCCUPIED and cells[L_up, cell_up] == rr.FREE and np.count_nonzero(cells) == 2


def test_walk_visits_the_voxels_of_a_brute_force_slab_test():
    """rays from non-dyadic sensors (no face is met at the same parameter as another) to random points: the walk from the point's voxel
    visits exactly the grid's voxels that the ray meets at or before that voxel, nearest to the point first"""
    _, grid = rcs.layered_map([(0, 0.0)], kz_max=5, nx=5, ny=4)
    kmax = grid["kmax"]
    rng = np.random.default_rng(7)
    every = [(x, y, z) for z in range(kmax[2] + 1) for y in range(kmax[1] + 1) for x in range(kmax[0] + 1)]
    lengths = []
    for t in range(200):
        hi = (kmax + 1) * RES
        p = (rng.uniform(0.01, 0.99, 3) * hi).astype(np.float32)
        # inside the grid, beside it, above it
        sensor = rng.uniform(-0.3, 1.3, 3) * hi + np.array([0.0137, 0.0071, 0.0113]) if t % 2 else rng.uniform(0.01, 0.99, 3) * hi
        o, delta = rr.ray_of(p, sensor)
        c0 = np.floor((p.astype(np.float64) - grid["mn"]) / RES).astype(np.int64)
        ok, near0, far0 = rr.slab(grid, c0, o, delta)
        assert ok and near0 <= 1.0 <= far0
        got = rr.walk(grid, c0, o, delta)
        want = {}
        for c in every:
            ok, near, far = rr.slab(grid, c, o, delta)
            if ok and near < far and near <= near0:
                want[c] = near
        assert set(got) == set(want) and len(got) == len(set(got))
        assert got == sorted(want, key=lambda c: -want[c])                 # from the point back towards the sensor
        lengths.append(len(got))
    assert max(lengths) >= 8 and min(lengths) == 1


def test_closed_forms_axis_aligned_ray_and_sensor_inside_the_owner():
    batch, grid = rcs.layered_map([(0, 0.0), (2, 0.0)], kz_max=4)
    z_lo = batch["mean"][0][2]
    # straight down the column of voxel (1, 2): delta_x = delta_y = 0 -- the owner's voxel, then one voxel per layer up to the grid's top
    p = np.array([[0.3, 0.6, z_lo]], dtype=np.float32)
    sensor = np.array([float(p[0, 0]), float(p[0, 1]), 1.3])
    b1, owner = rcs.own(batch, grid, p)
    L = int(owner[0])
    assert tuple(grid["vox"][L]) == (1, 2, 0)
    out = rr.cast(b1, grid, None, p, sensor)
    o, delta = rr.ray_of(p[0], sensor)
    assert delta[0] == 0.0 and delta[1] == 0.0 and delta[2] < 0.0
    assert out["visited"][0] == [(1, 2, z) for z in range(5)]
    up = 9 + 3 * 2 + 1
    loc = p[0, :2].astype(np.float64) - batch["mean"][L][:2]
    cell = SZ * int(SZ * (loc[0] / RES + 0.5)) + int(SZ * (loc[1] / RES + 0.5))
    assert out["events"] == [(0, L, cell, 0), (0, up, cell, 1)]           # the same (x, y) on both planes
    # an axis-aligned ray beside the owner's column does not meet its voxel: nothing happens
    assert not rr.slab(grid, (0, 2, 0), o, delta)[0] and rr.slab(grid, (1, 2, 0), o, delta)[0]
    # the sensor inside the owner's voxel: that voxel alone, one occupied write
    inside = batch["mean"][L] + np.array([0.05, -0.03, 0.06])
    out = rr.cast(b1, grid, None, p, inside)
    assert out["visited"][0] == [(1, 2, 0)] and [e[1:] for e in out["events"]] == [(L, cell, 0)]
    assert np.array_equal(out["counts"], [1, 0, 1, 0])
    # an untrained owner, an unowned point: no-ops
    tr = np.ones(18, bool)
    tr[L] = False
    assert np.array_equal(rr.cast(b1, grid, tr, p, sensor)["counts"], [1, 1, 0, 0])
    assert np.array_equal(rr.cast(b1, grid, None, p, sensor, owner=np.array([-1]))["counts"], [1, 1, 0, 0])
    # an untrained leaf on the way is passed through without a write
    tr = np.ones(18, bool)
    tr[up] = False
    assert rr.cast(b1, grid, tr, p, sensor)["events"] == [(0, L, cell, 0)]


def test_occupancy_batch_restatement():
    cells = np.zeros((4, SZ * SZ), np.uint8)
    cells[0, [5, 17, 63]] = [rr.FREE, rr.OCCUPIED, rr.FREE]
    cells[2, 0] = rr.OCCUPIED
    off, x0, x1, y = rr.occupancy_batch(cells, RES, SZ)
    assert np.array_equal(off, [0, 3, 3, 4, 4]) and np.array_equal(y, [-1, 1, -1, 1])
    c = np.array([5, 17, 63, 0])
    assert np.allclose(x0, RES * ((c // SZ + 0.5) / SZ - 0.5), rtol=0, atol=1e-15)
    assert np.allclose(x1, RES * ((c % SZ + 0.5) / SZ - 0.5), rtol=0, atol=1e-15)
    assert np.all(np.abs(x0) < RES / 2) and x0[3] == -RES / 2 + RES / (2 * SZ)
