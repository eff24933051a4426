"""CPU tests of the mapping cases at scale (tests/mapping_scale_cases.py): the NumPy restatement (tests/mapping_ref.py) is pinned against the
CPU oracle at these sizes before the GPU is compared with it (test_mapping_scale_gpu.py), the cases are shown to hold what they promise,
and every comparison helper the GPU tests rely on is shown to fail on a single wrong slot."""
import math

import numpy as np
import pytest

import mapping_cases as mc
import mapping_ref as mr
import mapping_scale_cases as ms
import registration_ref as ref

RES, SZ = ms.RES, ms.SZ


def _fails(check, *args):
    try:
        check(*args)
    except AssertionError:
        return True
    return False


def _with(d, key, value):
    out = dict(d)
    out[key] = value
    return out


# ---- striped ------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module", params=[False, True], ids=["above", "below"])
def striped(oracle, request):
    A, ca = ms.striped_model()
    B, cb, anchor = ms.striped_scan(request.param)
    pa = oracle.project_cloud(A, ca, RES, SZ)
    pab = oracle.project_cloud(np.concatenate([A, B]), np.concatenate([ca, cb]), RES, SZ)
    got = mr.insert(pa, mr.model_grid(A, RES, SZ), np.ones(len(pa["mean"]), bool), B, cb, 1, compute_rotation=oracle.compute_rotation)
    return request.param, A, B, pa, pab, got


def test_striped_insertion_is_project_cloud_of_the_union(striped):
    below, A, B, pa, pab, got = striped
    P0, P = len(pa["mean"]), len(pab["mean"])
    assert P0 == 270 and P == 540 + 3 * below
    o2n = got["old_to_new"]
    new = ms.check_union(got, o2n, pa, pab, len(A), len(B))
    assert np.all(got["cls"][new] == mr.FRESH) and np.all(got["cls"][o2n] == mr.KEPT)
    # the grid: origin shifts and key widths
    g0, g = mr.model_grid(A, RES, SZ), got["grid"]
    assert np.array_equal(g["koff"], [12, 3, 2] if below else [0, 0, 0])
    assert np.array_equal(g["kmax"], [34, 32, 2] if below else [22, 29, 0])
    bits = lambda kmax: [max(int(k).bit_length(), 1) for k in kmax]
    assert bits(g0["kmax"]) == [5, 5, 1] and bits(g["kmax"]) == ([6, 6, 2] if below else [5, 5, 1])
    # old and new keys alternate in runs of three inside every row of the merged table
    rows = o2n.reshape(ms.STRIPE_ROWS, 3, 3) - (3 if below else 0)
    for r in range(ms.STRIPE_ROWS):
        assert np.array_equal(rows[r].ravel(), 18 * r + np.array([0, 1, 2, 6, 7, 8, 12, 13, 14]))
    # both lists pass 256, and the merged table 512
    assert P0 > 256 and len(new) > 256 and P > 512


def test_striped_helper_fails_on_a_single_wrong_slot(striped):
    below, A, B, pa, pab, got = striped
    o2n = got["old_to_new"]
    args = (pa, pab, len(A), len(B))
    ms.check_union(got, o2n, *args)
    bad = o2n.copy()
    bad[257] += 1                                        # one slot of old_to_new, beyond the first block
    assert _fails(ms.check_union, got, bad, *args)
    off = got["off"].copy()
    L = np.flatnonzero(np.diff(off) > 1)[-1]
    off[L + 1] -= 1                                      # one leaf's segment, one row short (its neighbour's, one long)
    assert _fails(ms.check_union, _with(got, "off", off), o2n, *args)
    y = got["y"].copy()
    y[-1] = np.nextafter(y[-1], np.inf)                  # one ulp in one row
    assert _fails(ms.check_union, _with(got, "y", y), o2n, *args)
    mean = got["mean"].copy()
    mean[300, 1] = -mean[300, 1]
    assert _fails(ms.check_union, _with(got, "mean", mean), o2n, *args)


# ---- overlap at scale ---------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def overlap(oracle):
    c = ms.overlap_scale()
    A, ca = c["model"]
    S, cs = c["scan"]
    pa = oracle.project_cloud(A, ca, RES, SZ)
    trained = np.ones(len(pa["mean"]), bool)
    trained[c["untrained"]] = False
    got = mr.insert(pa, mr.model_grid(A, RES, SZ), trained, S, cs, c["min_nbr"], compute_rotation=oracle.compute_rotation)
    return c, pa, trained, got


def test_overlap_scale_holds_what_it_promises(overlap):
    c, pa, trained, got = overlap
    S = c["scan"][0]
    P0, P = len(pa["mean"]), len(got["cls"])
    assert P0 == 266 and P0 % 4 == 2 and P0 % 64 == 10
    U = len(ms.voxel_set(S))
    assert U > 256 and P > 512 and P % 4 != 0
    cls, o2n = got["cls"], got["old_to_new"]
    # idle, kept and fresh leaves on both sides of leaf 256 and of leaf 512
    for lo, hi in ((0, 256), (256, 512), (512, P)):
        assert min(ms.class_counts(cls, lo, hi)) >= 1, (lo, hi)
    assert o2n[0] < 256 and o2n[-1] >= 512
    assert np.all(cls[o2n[trained]] == mr.KEPT)
    idle = np.flatnonzero(cls[o2n] == mr.IDLE)
    assert np.array_equal(idle, ms.OV_HOLES) and np.all(np.diff(got["off"])[o2n[idle]] == 0)
    rest = np.setdiff1d(c["untrained"], ms.OV_HOLES)
    assert np.all(cls[o2n[rest]] == mr.FRESH)                                 # untrained, enough scan points: cut afresh
    new = np.setdiff1d(np.arange(P), o2n)
    assert np.all(cls[new] == mr.FRESH) and len(new) > 256
    # voxels below min_nbr give no leaf and leave their points unowned; the 30-point voxels are leaves
    vox = {tuple(v) for v in got["vox"]}
    assert len(ms.OV_LONELY) >= 5 and not any(v in vox for v in ms.OV_LONELY) and all(v in vox for v in ms.OV_SMALL)
    assert np.all(got["owner"][-c["n_lonely"]:] == -1) and got["off"][-1] < len(S)
    assert len(np.unique(got["src"])) == len(got["src"]) == got["off"][-1] > 0.9 * len(S)
    # the grid grew downwards along x (two columns) and z (two layers), not along y
    g = got["grid"]
    assert np.array_equal(g["koff"], [2, 0, 2]) and np.array_equal(g["kmax"], [21, 15, 2])
    # every patch spans less than two 64-point chunks (chunk_edge_scan has the long ones)
    assert 64 > np.diff(got["off"]).max() > 32


def test_overlap_helper_fails_on_a_single_wrong_slot(overlap):
    c, pa, trained, got = overlap
    n = len(c["scan"][0])
    batch = {k: got[k] for k in ("off", "src", "x0", "x1", "y", "rgb") + ms.FRAME_KEYS}
    o2n = got["old_to_new"]
    ms.check_insertion(batch, o2n, got, n)
    bad = o2n.copy()
    bad[265] -= 1
    assert _fails(ms.check_insertion, batch, bad, got, n)
    off = got["off"].copy()
    off[513] += 1
    assert _fails(ms.check_insertion, _with(batch, "off", off), o2n, got, n)
    src = got["src"].copy()
    a, b = got["off"][300], got["off"][301]
    assert b - a >= 2
    src[a], src[a + 1] = src[a + 1], src[a]              # two rows of one patch the wrong way round: owners agree, order does not
    assert _fails(ms.check_insertion, _with(batch, "src", src), o2n, got, n)
    W = got["W"].copy()
    W[520, 5] ^= 1
    assert _fails(ms.check_insertion, _with(batch, "W", W), o2n, got, n)


def test_face_probes_are_owned_on_every_face(overlap):
    """what the registration test at scale relies on: next to each face of the grown grid, points one voxel outside it that a boundary
    leaf owns"""
    c, pa, trained, got = overlap
    P, o2n = len(got["cls"]), got["old_to_new"]
    px, face = ms.face_probes(got["grid"])
    tr = np.diff(got["off"]) > 0
    tr[o2n[trained]] = True
    ow, _ = ref.assign(px, got, mr.registration_grid(got["grid"]), tr)
    assert all(np.sum(ow[face == f] >= 0) >= 1 for f in range(6))


# ---- chunk edges --------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def chunks(oracle):
    A, ca = mc.model_cloud()
    S, cs = ms.chunk_edge_scan()
    pa = oracle.project_cloud(A, ca, RES, SZ)
    got = mr.insert(pa, mr.model_grid(A, RES, SZ), np.ones(len(pa["mean"]), bool), S, cs, 1, compute_rotation=oracle.compute_rotation)
    return S, pa, got


def test_chunk_edge_leaves_own_exactly_their_points(chunks):
    S, pa, got = chunks
    o2n = got["old_to_new"]
    P = len(got["cls"])
    assert np.array_equal(o2n, np.arange(9)) and P == 9 + len(ms.CHUNK_COUNTS)          # layer 2: behind the model in leaf order
    fresh = np.arange(9, P)
    assert np.array_equal(got["vox"][fresh], ms.chunk_edge_voxels())
    assert np.array_equal(np.diff(got["off"])[fresh], ms.CHUNK_COUNTS) and np.all(np.diff(got["off"])[:9] == 0)
    assert np.array_equal(got["src"], np.arange(len(S)))
    # the order of the depth sum shows: the sequential mean is not the correctly rounded one on every leaf, and the depths have both
    # signs and three decades of magnitude
    differs = 0
    for L in fresh:
        d = got["local"][got["src"][got["off"][L]:got["off"][L + 1]], 0]
        differs += (np.cumsum(d)[-1] / len(d)) != (math.fsum(d) / len(d))
        if len(d) >= 63:
            assert d.min() < 0 < d.max() and np.abs(d).max() > 30 * np.abs(d).min()
    assert differs >= 3
    d = np.abs(got["local"][:, 0])
    assert d.max() > 1000 * d.min()


def test_chunk_helper_fails_on_a_single_wrong_slot(chunks):
    S, pa, got = chunks
    batch = {k: got[k] for k in ("off", "src", "x0", "x1", "y", "rgb") + ms.FRAME_KEYS}
    o2n = got["old_to_new"]
    ms.check_insertion(batch, o2n, got, len(S))
    off = got["off"].copy()
    off[9 + ms.CHUNK_COUNTS.index(64) + 1] += 1          # the 64-point leaf takes the first point of the 65-point one
    assert _fails(ms.check_insertion, _with(batch, "off", off), o2n, got, len(S))
    bad = o2n.copy()
    bad[8] = 9
    assert _fails(ms.check_insertion, batch, bad, got, len(S))
    mean = got["mean"].copy()
    L = 9 + ms.CHUNK_COUNTS.index(129)
    mean[L] = np.nextafter(mean[L], np.inf)              # a depth mean summed in another order moves the leaf's mean by ulps
    assert _fails(ms.check_insertion, _with(batch, "mean", mean), o2n, got, len(S))
