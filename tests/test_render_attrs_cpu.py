"""CPU tests (-m "not gpu") of the scattered sparse read-out and of the render attributes: the four new entries of the C-ABI and
their binding, and the restatements and bounds of tests/render_attrs_cases.py that the GPU tests hold the kernels to, pinned here
without a GPU -- the float64 statement of the normal (the kernel's association) against np.longdouble inside the derived bound on every
hit of the GPU test's poses, the share of hits whose orientation is excused, and the host bucketing against entry-by-entry evaluation.
The scene is the GPU tests' (raycast_cases.model_cloud, render_cases.POSES) with the frames the CPU oracle's project_cloud cuts."""
import ctypes as C

import numpy as np
import pytest

import mapping_ref as mr
import raycast_cases as rcs
import readout_cases as RC
import render_attrs_cases as ac

LD = ac.LD
NEW = ("gpc_sparse_predict_scattered", "gpc_sparse_predict_scattered_dev", "gpc_patches_render_attrs", "gpc_patches_render_attrs_dev")


def test_library_exports_the_new_entries_and_they_refuse_null_handles():
    from gp_compressor_amd import build, capi
    build.build()
    lib = capi.load()
    raw = C.CDLL(capi.LIB_PATH)
    for name in NEW:
        assert hasattr(raw, name) and name in capi.PROTOTYPES, name
    buf = np.zeros(8)
    idx = np.zeros(2, np.int32)
    for name in NEW[:2]:
        assert getattr(lib, name)(None, 2, idx.ctypes.data, buf.ctypes.data, buf.ctypes.data, 1, None, buf.ctypes.data, 0, None) == capi.GPC_EINVAL
    for name in NEW[2:]:
        assert getattr(lib, name)(None, None, None, 2, idx.ctypes.data, buf.ctypes.data, None, 0, buf.ctypes.data, None) == capi.GPC_EINVAL
    for cls, names in ((capi.Sparse, ("predict_scattered", "predict_scattered_dev")), (capi.Patches, ("render_attrs",))):
        for n in names:
            assert callable(getattr(cls, n)), n


@pytest.fixture(scope="module")
def scene(oracle):
    """frames and grid of the model cloud as the oracle cuts it, the handmade depth states, and per pose the restatement's render"""
    A, ca = rcs.model_cloud()
    frames = oracle.project_cloud(A, ca, ac.RES, ac.SZ)
    grid = mr.model_grid(A, ac.RES, ac.SZ)
    P = len(frames["mean"])
    assert P == len(grid["vox"]) == 21
    B = ac.depth_batch(P)
    return dict(frames=frames, grid=grid, B=B, poses={p: ac.restate(frames, grid, B, p) for p in ac.rc.POSES})


def test_float64_normal_stays_inside_the_derived_bound_on_every_hit(scene):
    """the bound holds for the reference alone: the float64 restatement in the kernel's association against np.longdouble, the gradient
    per component inside gb_d and the world normal per component inside nb = 2 (gb_0 + gb_1) + 16 EPS, unit length within 4 EPS"""
    B, frames = scene["B"], scene["frames"]
    worst_g = worst_n = 0.0
    leaves = set()
    for pose, (o, dirs, rays) in scene["poses"].items():
        hits = [r for r in rays if r["leaf"] >= 0]
        assert len(hits) > 100, pose
        for r in hits:
            L = r["leaf"]
            leaves.add(L)
            (g_hi, gb), (g_64, _) = ac.gradient(B, L, r["local"][1], r["local"][2], LD), ac.gradient(B, L, r["local"][1], r["local"][2], None)
            for d in range(2):
                err = float(abs(LD(g_64[d]) - g_hi[d]))
                assert err <= gb[d], (pose, L, d, err, gb[d])
                worst_g = max(worst_g, err / gb[d])
            hi, lo = ac.normal_ref(B, frames, L, r["local"], o, LD), ac.normal_ref(B, frames, L, r["local"], o, None)
            if ac.excused(hi):
                continue
            err = np.max(np.abs(np.asarray(lo["n"], dtype=LD) - hi["n"]))
            assert err <= hi["nb"], (pose, L, float(err), hi["nb"])
            worst_n = max(worst_n, float(err) / hi["nb"])
            n64 = np.asarray(lo["n"], dtype=LD)
            assert abs(np.sqrt(np.sum(n64 * n64)) - 1) <= 4 * ac.EPS
            # ... and it is a normal: orthogonal to the analytic tangents R (fx, 1, 0) and R (fy, 0, 1) of the surface f(q)
            R = np.asarray(frames["R"][L], dtype=LD)
            for t in (R @ np.array([hi["fx"], 1, 0], dtype=LD), R @ np.array([hi["fy"], 0, 1], dtype=LD)):
                assert abs(np.sum(n64 * t)) <= hi["nb"]
    print(f"float64 restatement: worst error / bound gradient {worst_g:.3f}, normal {worst_n:.3f}; {len(leaves)} leaves hit, basis sizes",
          sorted(set(int(B['b'][L]) for L in leaves)))
    assert len(leaves) >= 2 and len(set(int(B["b"][L]) for L in leaves)) >= 6


def test_poses_meet_the_orientation_cap_for_the_reference_alone(scene):
    """at most 1 % of a pose's hits have |n_ref . e| <= 1e-6 |e|; everywhere else the normal of the reference faces the sensor"""
    B, frames = scene["B"], scene["frames"]
    for pose, (o, dirs, rays) in scene["poses"].items():
        hits = [r for r in rays if r["leaf"] >= 0]
        refs = [ac.normal_ref(B, frames, r["leaf"], r["local"], o, LD) for r in hits]
        n_exc = sum(ac.excused(r) for r in refs)
        flipped = sum(r["ne"] < 0 for r in refs)
        print(pose, "hits", len(hits), "excused", n_exc, "normals turned round to face the sensor", flipped)
        assert len(hits) > 100 and n_exc <= ac.ORIENT_CAP * len(hits)
        for r, h in zip(refs, hits):
            x = np.asarray(h["x"], dtype=LD)
            assert ac.excused(r) or np.sum(r["n"] * (np.asarray(o, dtype=LD) - x)) > 0


def test_empty_basis_gives_the_frames_first_column():
    B = ac.depth_batch(3, sizes=[0, 5, 0])
    Rm = rcs._rot(0.3, -0.2) @ rcs.FLAT
    frames = dict(R=np.stack([Rm] * 3), mean=np.zeros((3, 3)))
    for dtype in (LD, None):
        r = ac.normal_ref(B, frames, 0, np.array([0.0, 0.01, -0.02]), None, dtype)
        assert np.max(np.abs(np.asarray(r["n"], dtype=np.float64) - Rm[:, 0])) <= 4 * ac.EPS and r["nb"] == 16 * ac.EPS
    up = ac.normal_ref(B, frames, 1, np.array([0.0, 0.01, -0.02]), np.array([0.0, 0.0, 5.0]), LD)
    down = ac.normal_ref(B, frames, 1, np.array([0.0, 0.01, -0.02]), np.array([0.0, 0.0, -5.0]), LD)
    assert np.array_equal(up["n"], -down["n"]) and up["n"][2] > 0


@pytest.mark.parametrize("pattern", ac.PATTERNS)
def test_bucketing_then_evaluate_is_entry_by_entry_evaluation(pattern):
    """the host statement of the device's bucketing: stable argsort by patch id, skipped entries last, off from the counts; evaluating
    the buckets and scattering back is evaluating every entry on its own, to the rounding of the longdouble sums (any order of a b-term
    sum is within b eps_ld of the sum of its terms' magnitudes, which fb / EPS and s2tol / EPS exceed: twice that between two orders)"""
    B = RC.batch(100, 1, RC.L8)
    patch, q0, q1 = ac.scatter_pattern(pattern, B, 65, seed=11)
    order, off, nv = ac.bucket(patch, B["P"])
    valid = (patch >= 0) & (patch < B["P"])
    assert nv == valid.sum() == off[-1] and sorted(order) == list(range(len(patch)))
    assert np.array_equal(np.flatnonzero(~valid), np.sort(order[nv:]))
    for p in range(B["P"]):
        idx = order[off[p]:off[p + 1]]
        assert np.all(patch[idx] == p) and np.all(np.diff(idx) > 0)               # its entries, in ascending i
    if pattern == "chunks":
        assert sorted(np.bincount(patch)[np.bincount(patch) > 0]) == [31, 32, 32, 33, 33]
    if pattern in ("sprinkled", "all_skipped"):
        assert set(patch[~valid]) == {-1, B["P"], 2 ** 31 - 1}
    a, e = ac.scattered_reference(B, patch, q0, q1), ac.entrywise_reference(B, patch, q0, q1)
    assert np.array_equal(np.isnan(a["f"][0]), ~valid) and np.array_equal(np.isnan(a["s2"]), ~valid)
    eps_ld = float(np.finfo(LD).eps)
    ok = valid
    assert np.all(np.abs(a["f"][:, ok] - e["f"][:, ok]) <= 2 * eps_ld * a["fb"][:, ok] / ac.EPS)
    assert np.all(np.abs(a["s2"][ok] - e["s2"][ok]) <= 2 * eps_ld * a["s2tol"][ok] / ac.EPS)
