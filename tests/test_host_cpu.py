"""CPU tests (-m "not gpu") of the host-side mirror of gp_compressor::project_cloud / compute_rotation / project_points
(src/gp_compressor.cpp:29-118, 177-249): the producer of the patch buffers the GPU path consumes."""
import numpy as np
import pytest


@pytest.fixture(scope="module")
def H():
    from gp_compressor_amd import host_api
    host_api.build()
    return host_api


def test_project_cloud_c1_contract(H):
    res, sz = 0.15, 20
    xyz, rgb = H.synthetic_plane_cloud(10000, seed=1)
    g = H.GpCompressor(xyz, rgb, res=res, sz=sz)
    b = g.project_cloud()
    P = len(b["off"]) - 1
    counts = np.diff(b["off"])
    # 8 x 8 occupied voxels; ownership is exclusive, and like in the reference a point that falls outside +-res/2 in the
    # tilted frame of every leaf whose search sphere reaches it is claimed by nobody (src/gp_compressor.cpp:85-87)
    assert 60 <= P <= 90 and 9900 <= counts.sum() <= 10000
    assert counts.max() <= 400 and np.median(counts[counts > 0]) > 100
    # value ranges the kernels are told to expect: X in [-res/2, res/2]^2, depth and colours mean-removed
    assert np.all(np.abs(b["x0"]) <= res / 2 + 1e-9) and np.all(np.abs(b["x1"]) <= res / 2 + 1e-9)
    for i in range(P):
        sl = slice(b["off"][i], b["off"][i + 1])
        if counts[i] == 0:
            continue
        assert abs(b["y"][sl].mean()) < 1e-9 and np.all(np.abs(b["rgb"][:, sl].mean(axis=1)) < 1e-9)
        assert np.abs(b["y"][sl]).max() < np.sqrt(3) / 2 * res
        R = b["R"][i]
        assert np.allclose(R.T @ R, np.eye(3), atol=1e-9) and np.linalg.det(R) > 0.999      # a rotation
        assert abs(R[2, 0]) > 0.9                                                         # normal ~ +z for this cloud
    # re-projecting the patch-frame points gives back exactly the input points (each once)
    rec = []
    for i in range(P):
        sl = slice(b["off"][i], b["off"][i + 1])
        pts = np.stack([b["y"][sl], b["x0"][sl], b["x1"][sl]], 0)
        rec.append((b["R"][i] @ pts).T + b["mean"][i])
    rec = np.concatenate(rec)
    from scipy.spatial import cKDTree
    dist, idx = cKDTree(xyz.astype(np.float64)).query(rec)
    assert dist.max() < 1e-6                      # every patch-frame point is an input point ...
    assert len(np.unique(idx)) == len(idx)        # ... and no input point is used twice


def test_project_cloud_edge_cases(H):
    # empty cloud, fewer than 4 points in a leaf (identity rotation, src/gp_compressor.cpp:31-34)
    g = H.GpCompressor(np.zeros((0, 3), np.float32), np.zeros((0, 3), np.uint8), res=0.1, sz=4)
    assert len(g.project_cloud()["off"]) == 1
    xyz = np.array([[0.01, 0.02, 0.03], [0.02, 0.01, 0.03], [0.9, 0.9, 0.9]], np.float32)
    rgb = np.array([[10, 20, 30], [30, 20, 10], [255, 0, 0]], np.uint8)
    b = H.GpCompressor(xyz, rgb, res=0.1, sz=4).project_cloud()
    assert np.diff(b["off"]).sum() == 3
    assert np.allclose(b["R"][0], np.eye(3))


def test_host_producer_equals_oracle_bit_for_bit(H, oracle):
    """The C++ host producer, the oracle (oracle/gpc_oracle_producer.c) and the GPU producer (tests/test_producer_gpu.py)
    evaluate the same expressions in the same order: identical batches, down to the last bit."""
    from gp_compressor_amd import synth
    for (xyz, rgb), res, sz in ((synth.plane_cloud(10000, seed=1), 0.15, 20), (synth.room_cloud(50000, seed=3), 0.15, 20),
                                (synth.room_cloud(20000, seed=5), 0.04, 6)):
        b = H.GpCompressor(xyz, rgb, res=res, sz=sz).project_cloud()
        o = oracle.project_cloud(xyz, rgb, res, sz)
        for k in b:
            assert np.array_equal(b[k], o[k]), k


def test_oracle_plane_fit_is_the_smallest_singular_vector(oracle):
    """compute_rotation (src/gp_compressor.cpp:35-36) takes JacobiSVD(points^T).matrixV().col(3); the oracle solves the 4x4
    moment matrix with cyclic Jacobi.  Pinned against LAPACK's SVD of the same k x 4 matrix, and the frame rules of
    :40-63 (dominant axis positive, right-handed, orthonormal)."""
    rng = np.random.default_rng(0)
    for trial in range(40):
        n = rng.normal(size=3)
        n /= np.linalg.norm(n)
        k = int(rng.integers(4, 400))
        basis = np.linalg.svd(n[None, :])[2][1:]                        # two in-plane directions
        pts = rng.uniform(-0.1, 0.1, (k, 2)) @ basis + rng.normal(0, 0.002, (k, 1)) * n + rng.uniform(-3, 3, 3)
        pts = pts.astype(np.float32).astype(np.float64)
        p4 = np.concatenate([pts, np.ones((k, 1))], 1)
        R = oracle.compute_rotation(p4.T @ p4, k)
        v = np.linalg.svd(p4, full_matrices=False)[2][3, :3]
        v /= np.linalg.norm(v)
        assert min(np.abs(R[:, 0] - v).max(), np.abs(R[:, 0] + v).max()) < 1e-7
        a = int(np.argmax(np.abs(R[:, 0])))
        assert R[a, 0] > 0
        assert np.allclose(R.T @ R, np.eye(3), atol=1e-12) and abs(np.linalg.det(R) - 1) < 1e-12
        e = np.eye(3)[(a + 2) % 3]                                        # x dir: z cross n, y dir: x cross n, z dir: y cross n
        c1 = np.cross(e, R[:, 0])
        assert np.allclose(R[:, 1], c1 / np.linalg.norm(c1), atol=1e-12)
    assert np.array_equal(oracle.compute_rotation(np.eye(4), 3), np.eye(3))   # fewer than 4 points (:31-34)


# ---- the shard layout of the multi-GPU flows (cut_shard / scatter_slots of host/gp_compressor.cpp) ---------------------------------
# No test machine has two GPUs, so padding slots, an all-padding device and the plane-strided colour copy run nowhere on the GPU: they are
# checked here, through gpc_host_shard / gpc_host_shard_scatter, against "slot q of device r holds patch slots[r, q]'s rows" restated in
# numpy from project_cloud()'s batch and capi.partition_patches.
CAPACITY = 40


def _projected(H, xyz, rgb, res, sz, capacity=CAPACITY):
    g = H.GpCompressor(xyz, rgb, res=res, sz=sz)
    g.set_sparse_kernel(1.0, (res / 2) ** 2, 1e-2, 25.0, capacity)
    g.capacity = capacity                                   # what the sparse flow hands gpc_partition_patches as the cost model
    return g, g.project_cloud()


@pytest.fixture(scope="module")
def c1(H):
    g, b = _projected(H, *H.synthetic_plane_cloud(10000, seed=1), res=0.15, sz=20)
    assert len(b["off"]) - 1 == 64
    return g, b


def _table(g, b, world, sparse):
    from gp_compressor_amd import capi
    return capi.partition_patches(b["off"], world, g.capacity if sparse else 0)


def _check_layout(g, b, world, sparse):
    off, slots = b["off"], _table(g, b, world, sparse)
    P, N = len(off) - 1, int(b["off"][-1])
    rng = np.random.default_rng(world)
    perm_d, perm_c = (rng.integers(0, 1 << 30, N).astype(np.int32) for _ in range(2))     # any values: they must only travel
    seen = []
    for r in range(world):
        s = g.shard(world, r, sparse=sparse, perm_d=perm_d, perm_c=perm_c)
        assert np.array_equal(s["slots"], slots[r])
        real = [int(p) for p in slots[r] if p >= 0]
        n = np.array([off[p + 1] - off[p] if p >= 0 else 0 for p in slots[r]], dtype=np.int64)
        assert np.array_equal(s["off"], np.concatenate([[0], np.cumsum(n)]))              # a padding slot is an empty local patch ...
        assert s["n_max"] == max([off[p + 1] - off[p] for p in real], default=0)          # ... and adds nothing to n_max
        rows = np.concatenate([np.arange(off[p], off[p + 1]) for p in real] + [np.zeros(0, np.int64)]).astype(np.int64)
        assert len(rows) == s["off"][-1]
        for k in ("x0", "x1", "y"):
            assert s[k].shape == (len(rows),) and np.array_equal(s[k], b[k][rows]), k
        assert s["rgb"].shape == (3, len(rows)) and np.array_equal(s["rgb"], b["rgb"][:, rows])   # three planes at the local stride
        assert np.array_equal(s["pd"], perm_d[rows]) and np.array_equal(s["pc"], perm_c[rows])
        bare = g.shard(world, r, sparse=sparse)                                           # the dense flow: no insertion orders
        assert len(bare["pd"]) == len(bare["pc"]) == 0
        for k in ("slots", "off", "x0", "x1", "y", "rgb"):
            assert np.array_equal(bare[k], s[k]), k
        seen += real
    assert sorted(seen) == list(range(P))                                                 # every patch in exactly one slot
    return slots


def _check_scatter(g, b, world, sparse):
    slots = _table(g, b, world, sparse)
    P, S = len(b["off"]) - 1, slots.shape[1]
    guarded = np.full(P + 2, -7, dtype=np.int32)            # one sentinel on either side: a write at index -1 or P lands there
    out = guarded[1:-1]
    for r in range(world):
        g.shard_scatter(world, r, 1000 * r + np.arange(S, dtype=np.int32), out, sparse=sparse)
    want = np.full(P, -7, dtype=np.int32)
    for r in range(world):
        for q in range(S):
            if slots[r, q] >= 0:
                want[slots[r, q]] = 1000 * r + q
    assert np.array_equal(out, want) and not np.any(out == -7)
    assert guarded[0] == -7 and guarded[-1] == -7


@pytest.mark.parametrize("world", [3, 5])
def test_shard_layout_padding_at_the_end_of_the_table(c1, world):
    g, b = c1
    for sparse in (False, True):
        slots = _check_layout(g, b, world, sparse)
        assert np.any(slots == -1)                          # 64 patches over 3 or 5 devices: the table does hold padding


def test_shard_layout_device_with_nothing_but_padding(c1):
    g, b = c1
    P = len(b["off"]) - 1
    world = P + 6
    slots = _check_layout(g, b, world, False)
    assert slots.shape == (world, 1)
    padded = [r for r in range(world) if slots[r, 0] < 0]
    assert len(padded) == 6
    for r in padded:
        s = g.shard(world, r)
        assert s["off"].tolist() == [0, 0] and s["n_max"] == 0
        assert all(s[k].size == 0 for k in ("x0", "x1", "y", "rgb"))
    for r in set(range(world)) - set(padded):
        p = slots[r, 0]
        assert g.shard(world, r)["off"].tolist() == [0, b["off"][p + 1] - b["off"][p]]


def test_shard_layout_under_both_cost_models(H, c1):
    """the dense (n^3) and the sparse (n min(n, capacity)^2) table differ, and each is laid out as dealt: on C1 (132 ... 191 points a
    patch, capacity 40) and on a ragged room cloud (15665 patches of 0 ... 6 points, empty ones included; at capacity 40 the two costs
    would coincide there, min(n, capacity) = n, so its sparse GPs get capacity 2)"""
    from gp_compressor_amd import synth
    room = _projected(H, *synth.room_cloud(20000, seed=5), res=0.04, sz=6, capacity=2)
    assert np.any(np.diff(room[1]["off"]) == 0) and np.diff(room[1]["off"]).max() > 2
    for g, b in (c1, room):
        dense, sparse = _check_layout(g, b, 3, False), _check_layout(g, b, 3, True)
        assert not np.array_equal(dense, sparse)
        for sp in (False, True):
            _check_scatter(g, b, 3, sp)


def test_shard_scatter_skips_padding(c1):
    g, b = c1
    for world in (3, 5, len(b["off"]) - 1 + 6):
        for sparse in (False, True):
            _check_scatter(g, b, world, sparse)


def test_shard_layout_of_a_tiny_cloud(H):
    xyz = np.array([[0.01, 0.02, 0.03], [0.02, 0.01, 0.03], [0.9, 0.9, 0.9]], np.float32)
    rgb = np.array([[10, 20, 30], [30, 20, 10], [255, 0, 0]], np.uint8)
    g, b = _projected(H, xyz, rgb, res=0.1, sz=4)
    assert 1 <= len(b["off"]) - 1 < 4                       # fewer patches than devices
    for sparse in (False, True):
        _check_layout(g, b, 4, sparse)
        _check_scatter(g, b, 4, sparse)
    g, b = _projected(H, np.zeros((0, 3), np.float32), np.zeros((0, 3), np.uint8), res=0.1, sz=4)
    s = g.shard(2, 1)                                       # no patch at all: no slot either
    assert s["off"].tolist() == [0] and s["slots"].size == 0 and s["n_max"] == 0
