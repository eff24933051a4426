"""CPU tests of the map insertion's NumPy restatement (tests/mapping_ref.py) against the CPU oracle, and of the library's exports.

The restatement is what the GPU tests (test_mapping_gpu.py) compare gpc_patches_insert_cloud with; here it is pinned itself: inserting
a scan B that touches no voxel around the model A into the oracle's project_cloud(A) must give project_cloud(A + B).  The clouds
(mapping_cases.py) are anchored on dyadic corners, so the anchor's whole-voxel shift is invisible and A's leaves come out of
project_cloud(A + B) exactly as out of project_cloud(A)."""
import ctypes as C

import numpy as np
import pytest

import mapping_cases as mc
import mapping_ref as mr
import registration_ref as ref

RES, SZ = mc.RES, mc.SZ


def _leaf_voxels(xyz, anchor):
    """voxel coordinates (relative to `anchor`) of the leaves project_cloud cuts, in leaf order"""
    g = mr.model_grid(xyz, RES, SZ)
    shift = np.round((g["mn"] - np.asarray(anchor, dtype=np.float64)) / RES).astype(np.int64)
    return g["vox"] + shift


@pytest.mark.parametrize("where", ["above", "below"])
def test_inserting_a_disjoint_scan_is_project_cloud_of_the_union(oracle, where):
    A, ca = mc.model_cloud()
    B, cb = mc.disjoint_scan(where)
    pa = oracle.project_cloud(A, ca, RES, SZ)
    pab = oracle.project_cloud(np.concatenate([A, B]), np.concatenate([ca, cb]), RES, SZ)
    Pa, Pab = len(pa["mean"]), len(pab["mean"])
    assert Pa == 9 and Pab == 11
    grid = mr.model_grid(A, RES, SZ)
    got = mr.insert(pa, grid, np.ones(Pa, bool), B, cb, 1, compute_rotation=oracle.compute_rotation)
    # leaf keys: the merge, in the union's leaf order
    want_vox = _leaf_voxels(np.concatenate([A, B]), grid["mn"])
    assert np.array_equal(got["vox"], want_vox)
    assert np.array_equal(got["grid"]["koff"] > 0, np.array([where == "below"] * 3))
    o2n = got["old_to_new"]
    new = np.setdiff1d(np.arange(Pab), o2n)
    assert len(new) == 2 and np.array_equal(got["cls"][new], [mr.FRESH] * 2) and np.all(got["cls"][o2n] == mr.KEPT)
    # the premise: A's leaves are cut from the union as from A alone
    for k in ("R", "mean", "rgb_mean", "W"):
        assert np.array_equal(pab[k][o2n], pa[k]), k
    # old leaves: nothing of the scan, frames kept; new leaves: the union's rows, bit for bit
    for k in ("R", "mean", "rgb_mean", "W"):
        assert np.array_equal(got[k], pab[k]), k
    assert np.all(np.diff(got["off"])[o2n] == 0)
    assert got["off"][-1] == int(np.diff(pab["off"])[new].sum()) > 0.9 * len(B)
    for L in new:
        a, b = got["off"][L], got["off"][L + 1]
        a2, b2 = pab["off"][L], pab["off"][L + 1]
        assert b - a == b2 - a2 > 0
        for k in ("x0", "x1", "y"):
            assert np.array_equal(got[k][a:b], pab[k][a2:b2]), k
        assert np.array_equal(got["rgb"][:, a:b], pab["rgb"][:, a2:b2])
        assert np.array_equal(got["src"][a:b] + len(A), pab["src"][a2:b2])


def test_inserting_nothing_copies_the_model(oracle):
    A, ca = mc.model_cloud()
    pa = oracle.project_cloud(A, ca, RES, SZ)
    P = len(pa["mean"])
    trained = np.ones(P, bool)
    trained[4] = False                                   # an untrained leaf with nothing around it stays idle
    got = mr.insert(pa, mr.model_grid(A, RES, SZ), trained, np.zeros((0, 3)), np.zeros((0, 3)), 1, compute_rotation=oracle.compute_rotation)
    assert np.array_equal(got["old_to_new"], np.arange(P)) and np.all(got["off"] == 0)
    assert got["cls"][4] == mr.IDLE and np.all(np.delete(got["cls"], 4) == mr.KEPT)
    for k in ("R", "mean", "rgb_mean", "W"):
        assert np.array_equal(got[k], pa[k]), k
    assert np.array_equal(got["grid"]["keys"], ref.grid_of(A, RES)["keys"])


def test_overlapping_scan_holds_every_kind_of_leaf(oracle):
    """the scenario of the GPU test, on the oracle's model: kept, fresh (old and new) and idle leaves, a new voxel below min_nbr, a
    fresh leaf ahead of a kept neighbour that would have taken one of its points, every scan point owned at most once"""
    A, ca = mc.model_cloud()
    S, cs = mc.overlapping_scan()
    pa = oracle.project_cloud(A, ca, RES, SZ)
    trained = np.ones(9, bool)
    trained[[0, 6]] = False                              # voxel (0, 0, 0): re-cut; voxel (0, 2, 0): three scan points around it
    got = mr.insert(pa, mr.model_grid(A, RES, SZ), trained, S, cs, 20, compute_rotation=oracle.compute_rotation)
    P = len(got["cls"])
    o2n = got["old_to_new"]
    assert P % 4 != 0 and P > 9
    assert got["cls"][o2n[0]] == mr.FRESH and got["cls"][o2n[6]] == mr.IDLE
    assert np.all(got["cls"][o2n[trained]] == mr.KEPT)
    new = np.setdiff1d(np.arange(P), o2n)
    assert np.all(got["cls"][new] == mr.FRESH)
    vox = {tuple(v) for v in got["vox"]}
    assert (6, 0, 0) in vox and (0, 6, 0) not in vox     # 30 points: a leaf; 5 points: none
    src = got["src"]
    assert len(np.unique(src)) == len(src) == got["off"][-1] < len(S)
    assert np.all(got["owner"][-5:] == -1)               # the five stay unowned
    # a point of the fresh leaf 0 that its kept neighbour (voxel (1, 0, 0)) would accept as well
    L0, L1 = int(o2n[0]), int(o2n[1])
    mine = src[got["off"][L0]:got["off"][L0 + 1]]
    p = S[mine].astype(np.float64)
    cen1 = got["grid"]["mn"] + (np.array([1, 0, 0]) + 0.5) * RES
    d = p - cen1
    q = ref.local_coords(p, np.repeat(got["R"][L1][None], len(p), 0), np.repeat(pa["mean"][1][None], len(p), 0))
    both = (np.sum(d * d, axis=1) <= got["grid"]["radius"] ** 2) & np.all(np.abs(q[:, 1:]) <= RES / 2, axis=1)
    assert both.any()
    # kept leaves: frames and means are the model's; W is the OR; colours are minus the stored mean
    for i in np.flatnonzero(trained):
        L = o2n[i]
        assert np.array_equal(got["R"][L], pa["R"][i]) and np.array_equal(got["mean"][L], pa["mean"][i])
        assert np.all(got["W"][L] >= pa["W"][i])
        sl = slice(got["off"][L], got["off"][L + 1])
        assert np.array_equal(got["rgb"][:, sl], (cs[src[sl]].astype(np.float64) - pa["rgb_mean"][i]).T)
    sphere_counts = [int(np.sum(np.sum((S.astype(np.float64) - (got["grid"]["mn"] + (v + 0.5) * RES)) ** 2, axis=1)
                                <= got["grid"]["radius"] ** 2)) for v in got["vox"][new]]
    assert min(sphere_counts) < 64 < max(sphere_counts)


def test_library_exports_the_mapping_entry_points():
    from gp_compressor_amd import build, capi
    build.build()
    lib = C.CDLL(capi.LIB_PATH)
    for name in ("gpc_patches_insert_cloud", "gpc_patches_insert_cloud_dev", "gpc_sparse_remap", "gpc_registration_cloud_dev"):
        assert hasattr(lib, name), name
        assert name in capi.PROTOTYPES, name
