"""Rays and hand-made GP states of the render tests (test infrastructure).  The map is raycast_cases.model_cloud(): two curved sheets of
3 x 3 voxels, the upper one straddling a voxel boundary (about 27 leaves at res 0.25, sz 8), cut by the producer."""
import numpy as np

import raycast_cases as rcs
import render_ref as rn

RES, SZ = rcs.RES, rcs.SZ
LOOK_DOWN = np.array([[1.0, 0.0, 0.0], [0.0, -1.0, 0.0], [0.0, 0.0, -1.0]])      # columns: the camera's x, y, z in the world
INSIDE = np.array([0.3, 0.4, -0.1])                                              # between the sheets, in the empty voxel layer 1


def _tilted(angle):
    """LOOK_DOWN turned by `angle` about the world's y axis: the optical axis leans towards +x"""
    c, s = np.cos(angle), np.sin(angle)
    return np.array([[c, 0.0, s], [0.0, 1.0, 0.0], [-s, 0.0, c]]) @ LOOK_DOWN


# name -> (origin, camera matrix, focal length in pixels); every image is 23 x 17 (391 rays: six waves and a part) plus a 1 x 1 image
POSES = {"above": (rcs.SENSOR, LOOK_DOWN, 26.0), "inside": (INSIDE, _tilted(0.55), 9.0)}
W_IMG, H_IMG = 23, 17


def handmade_rays(origin, u_axis):
    """axis-aligned rays, a ray along a leaf's in-plane axis (parallel to its plane), one that misses the box, NaN / inf / zero ones"""
    far = np.array([5.0, 5.0, 5.0]) - origin                                     # away from the box
    return np.array([[0.0, 0.0, -1.0], [0.0, 0.0, 3.0], [1.0, 0.0, 0.0], [-2.0, 0.0, 0.0], [0.0, 0.5, 0.0], [0.0, -1.0, 0.0],
                     u_axis, -u_axis, far, [0.0, 0.0, 1e-300], [np.nan, 0.0, -1.0], [0.0, np.inf, -1.0], [0.0, 0.0, 0.0]])


def scene_rays(name, u_axis):
    """(origin, dirs (n, 3)) of a scene: the image, the 1 x 1 image, the hand-made rays; n = 391 + 1 + 13"""
    o, R, f = POSES[name]
    img = rn.camera_rays(R, f, f, (W_IMG - 1) / 2, (H_IMG - 1) / 2, W_IMG, H_IMG)
    one = rn.camera_rays(R, f, f, 0.0, 0.0, 1, 1)
    return np.asarray(o, dtype=np.float64), np.concatenate([img, one, handmade_rays(o, np.asarray(u_axis, dtype=np.float64))])


def handmade_state(rng, P, b, ld, ny=1, amp=0.01):
    """bv_count (P,), alpha (P, ny, ld), BV (P, ld, 2): b basis vectors per leaf inside the window, random weights of `amp`"""
    b = np.broadcast_to(np.asarray(b, dtype=np.int32), (P,)).copy()
    alpha, BV = np.zeros((P, ny, ld)), np.zeros((P, ld, 2))
    for L in range(P):
        alpha[L, :, :b[L]] = amp * rng.standard_normal((ny, b[L]))
        BV[L, :b[L]] = rng.uniform(-RES / 2, RES / 2, (b[L], 2))
    return b, alpha, BV


def holds_every_case(rays, grid):
    """what a scene of the GPU tests must contain, asserted on the restatement's own output; returns the tally it printed"""
    leaves = {tuple(int(x) for x in v): L for L, v in enumerate(grid["vox"] - grid["koff"])}
    z_of = {L: c[2] for c, L in leaves.items()}
    hit = [r for r in rays if r["leaf"] >= 0]
    tally = dict(rays=len(rays), hits=len(hit), lower=sum(z_of[r["leaf"]] == 0 for r in hit), upper=sum(z_of[r["leaf"]] >= 2 for r in hit),
                 misses=len(rays) - len(hit), outside=sum(r["outside"] for r in rays),
                 non_leaf=sum(any(c not in leaves for c in r["visited"]) for r in rays), long=sum(len(r["visited"]) >= 3 for r in rays),
                 rejected_then_hit=sum(len(r["tests"]) >= 2 for r in hit), low_margin=sum(r["margin"] < 1e-6 * RES for r in rays))
    print(tally)
    return tally
