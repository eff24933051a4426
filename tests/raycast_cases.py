"""Scenes of the ray-cast tests (test infrastructure).

  * layered_map(): a hand-made map for the tests that run without a GPU -- layers of 3 x 3 leaves with (optionally tilted) plane
    frames, the grid anchored at the dyadic corner (0, 0, 0), and scan points ON those planes, owned through
    registration_ref.assign / bucket exactly as the device would own them;
  * model_cloud() / scan_cloud(): the clouds of the GPU tests, cut by the device itself -- two mapping_cases.sheet layers of 3 x 3
    voxels two voxels apart, the upper one straddling a voxel boundary; a scan of about 20 points per voxel on the lower layer
    everywhere and on the upper one only where x < 0.4, shuffled, with points exactly under the sensor (axis-aligned rays) and an
    isolated voxel that becomes a fresh leaf.
"""
import numpy as np

import mapping_cases as mc
import registration_ref as ref

RES, SZ = mc.RES, mc.SZ
SENSOR = np.array([0.3, 0.45, 1.3])
# the model's dyadic minimum corner: voxel boundaries at z = -0.3125, -0.0625, 0.1875 -- the lower layer (z in -0.45 .. -0.37) lies in
# voxel layer 0, the upper one (z in 0.17 .. 0.25) in layers 2 and 3
CORNER = (0.0, 0.0, -0.5625)
Z_UPPER, Z_LOWER = 0.17, -0.45


def model_cloud(seed=21):
    rng = np.random.default_rng(seed)
    lo, cl = mc.sheet(rng, 0.0, 0.0, 3, 3, Z_LOWER)
    up, cu = mc.sheet(rng, 0.0, 0.0, 3, 3, Z_UPPER)
    xyz, rgb = np.concatenate([lo, up]), np.concatenate([cl, cu])
    xyz[0] = CORNER
    assert np.all(xyz >= np.asarray(CORNER, dtype=np.float32))
    return xyz, rgb


def _on_sheet(x, y, z):
    return z + 0.05 * np.sin(3 * x) + 0.03 * y


def scan_cloud(seed=22):
    rng = np.random.default_rng(seed)
    lo, cl = mc.sheet(rng, 0.0, 0.0, 3, 3, Z_LOWER, npv=20)
    up, cu = mc.sheet(rng, 0.0, 0.0, 3, 3, Z_UPPER, npv=20)
    keep = up[:, 0] < 0.4
    fr, cf = mc.sheet(rng, 1.5, 0.0, 1, 1, Z_LOWER, npv=30)                 # an isolated voxel: a fresh leaf (min_nbr 20)
    xyz, rgb = np.concatenate([lo, up[keep], fr]), np.concatenate([cl, cu[keep], cf])
    o = rng.permutation(len(xyz))
    xyz, rgb = xyz[o], rgb[o]
    # exactly under the sensor (x, y equal to the sensor's as floats): delta_x = delta_y = 0
    sx, sy = np.float32(SENSOR[0]), np.float32(SENSOR[1])
    under = np.array([[sx, sy, _on_sheet(float(sx), float(sy), Z_LOWER)], [sx, sy, _on_sheet(float(sx), float(sy), Z_LOWER) + 0.001],
                      [sx, sy, _on_sheet(float(sx), float(sy), Z_UPPER)]], dtype=np.float32)
    at = [5, len(xyz) // 2, len(xyz) - 3]                                    # early, in the middle, late in the scan
    for j, q in zip(at, under):
        xyz = np.insert(xyz, j, q, axis=0)
        rgb = np.insert(rgb, j, (128, 128, 128), axis=0)
    return xyz.astype(np.float32), rgb.astype(np.uint8)


# ---- the hand-made map ------------------------------------------------------------------------------------------------------------
def _rot(ax, ay):
    cx, sx, cy, sy = np.cos(ax), np.sin(ax), np.cos(ay), np.sin(ay)
    Rx = np.array([[1, 0, 0], [0, cx, -sx], [0, sx, cx]])
    Ry = np.array([[cy, 0, sy], [0, 1, 0], [-sy, 0, cy]])
    return Rx @ Ry


FLAT = np.array([[0.0, 1.0, 0.0], [0.0, 0.0, 1.0], [1.0, 0.0, 0.0]])          # columns: normal = z, u = x, v = y


def layered_map(layers, kz_max, tilt=0.0, nx=3, ny=3, seed=0):
    """layers: [(kz, dz)]: a layer of nx x ny leaves in voxel layer kz whose plane passes dz above the voxel centres; tilt: the largest
    rotation angle of a leaf's frame about x and y (0: every frame is FLAT).  Returns batch (R, mean; off / src are added by own())
    and grid (as mapping_ref.model_grid gives it)."""
    rng = np.random.default_rng(seed)
    vox = np.array([(kx, ky, kz) for kz, _ in sorted(layers) for ky in range(ny) for kx in range(nx)], dtype=np.int64)
    dz = np.array([d for _, d in sorted(layers) for _ in range(nx * ny)])
    P = len(vox)
    mn = np.zeros(3)
    mean = mn + (vox.astype(np.float64) + 0.5) * RES
    mean[:, 2] += dz
    R = np.stack([(_rot(*(tilt * rng.uniform(-1, 1, 2))) if tilt else np.eye(3)) @ FLAT for _ in range(P)])
    radius = float(np.float32(np.sqrt(np.float32(3.0))) / np.float32(2.0)) * RES
    grid = dict(mn=mn, res=RES, radius=radius, half=RES / 2.0, kmax=np.array([nx - 1, ny - 1, kz_max], dtype=np.int64),
                keys=ref._key(vox[:, 0], vox[:, 1], vox[:, 2]), sz=SZ, koff=np.zeros(3, np.int64), vox=vox)
    assert np.all(np.diff(grid["keys"]) > 0)
    return dict(R=R, mean=mean), grid


def points_on(batch, grid, leaf, u, v):
    """the points mean + u U + v V of a leaf's plane, as float32"""
    R, mean = batch["R"][leaf], batch["mean"][leaf]
    return (mean + np.outer(u, R[:, 1]) + np.outer(v, R[:, 2])).astype(np.float32)


def own(batch, grid, xyz, trained=None):
    """adds off / src to the batch: the scan's points bucketed by their owners (registration_ref.assign: first accepting leaf)"""
    P = len(batch["mean"])
    owner, _ = ref.assign(xyz, batch, grid, np.ones(P, bool) if trained is None else trained)
    order, off = ref.bucket(owner, P)
    return dict(batch, off=off, src=order[:off[P]].astype(np.int32)), owner
