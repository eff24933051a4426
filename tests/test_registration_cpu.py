"""The NumPy restatement of the registration step (tests/registration_ref.py), checked without a GPU: its assignment against the
CPU oracle's patch producer, and the algebra of its gradient step and stopping rule against /root/reference/src/gp_registration.cpp
(:51-58, :67-70, :83-85).  The GPU tests (test_registration_gpu.py) compare the kernels with this restatement."""
import numpy as np

from gp_compressor_amd import synth
import registration_ref as ref


def test_restated_assignment_matches_the_oracle_producer(oracle):
    """Registering the model cloud on itself at the identity pose with every leaf trained is the producer's own ownership pass
    (src/gp_compressor.cpp:81-89 against src/gp_registration.cpp:101-108), except that the window is taken around the patch's
    stored (shifted) mean instead of the voxel centre: the two differ by a multiple of the normal, so q[1], q[2] agree up to
    rounding and only a point within rounding of the window's edge can change hands."""
    res, sz = 0.15, 20
    xyz, rgb = synth.plane_cloud(10000, seed=1)
    b = oracle.project_cloud(xyz, rgb, res, sz)
    P = len(b["off"]) - 1
    want = np.full(len(xyz), -1, dtype=np.int32)
    for i in range(P):
        want[b["src"][b["off"][i]:b["off"][i + 1]]] = i
    grid = ref.grid_of(xyz, res)
    assert len(grid["keys"]) == P
    owner, local = ref.assign(xyz, b, grid, np.ones(P, dtype=bool))
    # the patch-frame coordinates of the points both agree on are the producer's, before its mean removal
    same = np.flatnonzero((owner == want) & (want >= 0))
    pos = np.zeros(len(xyz), dtype=np.int64)
    pos[b["src"]] = np.arange(len(b["src"]))
    assert np.max(np.abs(local[same, 1] - b["x0"][pos[same]])) <= 1e-12 * res
    assert np.max(np.abs(local[same, 2] - b["x1"][pos[same]])) <= 1e-12 * res
    differ = np.flatnonzero(owner != want)
    p = xyz.astype(np.float64)
    for i in differ:                                   # only points on a window's edge may differ
        edge = False
        for L in (owner[i], want[i]):
            if L >= 0:
                q = ref.local_coords(p[i:i + 1], b["R"][L:L + 1], b["mean"][L:L + 1])[0]
                edge = edge or bool(np.any(np.abs(np.abs(q[1:]) - res / 2) <= 1e-9 * res))
        assert edge, (int(i), int(owner[i]), int(want[i]))
    assert len(differ) <= 10, len(differ)


def test_restated_bucket_is_patch_order_then_scan_order():
    owner = np.array([2, -1, 0, 2, 0, -1, 1, 2], dtype=np.int32)
    order, off = ref.bucket(owner, 4)
    assert order.tolist() == [2, 4, 6, 0, 3, 7, 1, 5] and off.tolist() == [0, 2, 3, 6, 6]


def test_restated_gradient_step_algebra():
    rng = np.random.default_rng(4)
    delta = rng.normal(0, 1.0, 6)
    step = float(np.float32(1e-1))
    R, t = ref.gradient_step(delta, step)
    assert np.max(np.abs(R @ R.T - np.eye(3))) <= 1e-15 and abs(np.linalg.det(R) - 1.0) <= 1e-15
    assert np.array_equal(t, step * delta[:3])
    # a pure rotation about one axis is that axis' AngleAxis matrix (:53-55)
    Rz, _ = ref.gradient_step(np.array([0, 0, 0, 0, 0, 2.0]), 0.25)
    assert np.allclose(Rz, [[np.cos(0.5), -np.sin(0.5), 0], [np.sin(0.5), np.cos(0.5), 0], [0, 0, 1]], atol=1e-16)
    Rx, _ = ref.gradient_step(np.array([0, 0, 0, 2.0, 0, 0]), 0.25)
    assert np.allclose(Rx @ np.array([0, 1.0, 0]), [0, np.cos(0.5), np.sin(0.5)], atol=1e-16)
    # two steps: the composition form tracks the motion the cloud actually made, the reference's sum (:84) does not
    d2 = rng.normal(0, 1.0, 6)
    R2, t2 = ref.gradient_step(d2, step)
    pts = rng.normal(0, 1.0, (5, 3))
    moved = (pts @ R.T + t) @ R2.T + t2
    Rc, tc = ref.update_pose(*ref.update_pose(np.eye(3), np.zeros(3), R, t, False), R2, t2, False)
    assert np.max(np.abs(pts @ Rc.T + tc - moved)) <= 1e-14
    Rs, ts = ref.update_pose(*ref.update_pose(np.eye(3), np.zeros(3), R, t, True), R2, t2, True)
    assert np.array_equal(Rs, Rc) and np.array_equal(ts, t + t2)
    assert np.max(np.abs(ts - tc)) > 1e-3                                  # (R2 t + t2 != t + t2 for a real rotation)
    # float round trip of transform_pointcloud (:36)
    xyz = rng.normal(0, 1.0, (7, 3)).astype(np.float32)
    out = ref.transform_cloud(xyz, R, t)
    assert out.dtype == np.float32 and np.max(np.abs(out - (xyz.astype(np.float64) @ R.T + t))) <= 2.0 ** -23 * 4


def test_restated_stopping_rule():
    """step_nbr > 10 && (step_nbr >= max_steps || (|delta.head<3>()| < 0.1 && |delta.tail<3>()| < 0.1))  (:69)"""
    small, big = np.full(6, 0.01), np.array([0.2, 0, 0, 0, 0, 0.0])
    rot_big = np.array([0, 0, 0, 0, 0.2, 0.0])
    assert not ref.registration_done(10, small)            # never before the 11th step
    assert ref.registration_done(11, small)
    assert not ref.registration_done(11, big) and not ref.registration_done(11, rot_big)       # BOTH norms
    assert not ref.registration_done(299, big) and ref.registration_done(300, big)
    assert ref.registration_done(5, big, min_steps=2, max_steps=5) and not ref.registration_done(4, big, min_steps=2, max_steps=5)
    assert not ref.registration_done(11, np.full(6, np.nan)) and ref.registration_done(300, np.full(6, np.nan))
