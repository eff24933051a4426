"""CPU tests (-m "not gpu") of the renderer: the C-ABI's new symbols, and the NumPy restatement (tests/render_ref.py) that the GPU
tests compare the kernel with, pinned here without a GPU -- flat leaves against the analytic ray-plane intersections found by brute
force over every leaf (no walk), one curved leaf against a bracketing root finder, the forward walk against the ray cast's backward
one, and the share of rays whose outcome the restatement itself calls undecided.  Scenes: tests/raycast_cases.layered_map (res 0.25,
sz 8)."""
import ctypes as C
import math

import numpy as np
import pytest

import raycast_cases as rcs
import raycast_ref as rr
import render_ref as rn

RES, SZ = rcs.RES, rcs.SZ
M = SZ * SZ
SENSOR = np.array([0.31, 0.44, 1.6])                                        # above the grid box of the scenes below (z < 1.25)


def test_library_exports_the_render_entries():
    from gp_compressor_amd import capi
    lib = C.CDLL(capi.LIB_PATH)
    for name in ("gpc_patches_render", "gpc_patches_render_dev", "gpc_camera_rays_dev", "gpc_default_params_render"):
        assert hasattr(lib, name), name
        assert name in capi.PROTOTYPES, name
    assert C.sizeof(capi.RenderParams) == 24
    p = capi.default_params_render()
    assert (p.newton_iters, p.use_w, p.eps_rel) == (4, 1, 1e-6) and p.t_max == math.inf
    assert capi.default_params_render(newton_iters=7, t_max=2.5).t_max == 2.5
    assert rn.DEFAULTS == dict(newton_iters=p.newton_iters, use_w=p.use_w, eps_rel=p.eps_rel, t_max=p.t_max)


def _flat_gp(P, ld=16):
    """b = 1, alpha = 0: f == 0, the surface is the leaf's plane"""
    return dict(sf=1.0, l_sq=1.0, b=np.ones(P, np.int32), alpha=np.zeros((P, 1, ld)), BV=np.zeros((P, ld, 2)))


def _layers(tilt=0.0, seed=3):
    """an upper layer of 3 x 3 leaves in voxel layer 3 and a lower one in layer 1, every cell of W set"""
    batch, grid = rcs.layered_map([(1, -0.02), (3, 0.03)], kz_max=4, tilt=tilt, seed=seed)
    batch["W"] = np.ones((18, M), np.uint8)
    return batch, grid


def _fan(rng, origin, n, z=0.3):
    """rays from origin towards points spread over (and beyond) the footprint of the layers, at height z"""
    tgt = np.stack([rng.uniform(-0.45, 1.2, n), rng.uniform(-0.45, 1.2, n), np.full(n, z)], 1)
    return tgt - origin


def _brute(batch, grid, o, d, prm, cells=None):
    """the outcome of a ray over flat leaves without a walk: every leaf whose voxel the ray meets (slab test) is a candidate in the order
    the ray enters the voxels; the first whose plane intersection passes the acceptance rule wins.  Returns (leaf, t, x)."""
    prm = dict(rn.DEFAULTS, **prm)
    vox = grid["vox"] - grid["koff"]
    cand = []
    for L in range(len(vox)):
        meets, tn, tf = rr.slab(grid, vox[L], o, d)
        if meets:
            cand.append((max(tn, 0.0), L))
    for _, L in sorted(cand):
        R, mu = batch["R"][L], batch["mean"][L]
        den = R[:, 0] @ d
        if den == 0.0:
            continue
        t = (R[:, 0] @ (mu - o)) / den
        x = o + t * d
        q = R.T @ (x - mu)
        cen = grid["mn"] + (vox[L] + 0.5) * grid["res"]
        if not (0.0 < t <= prm["t_max"]) or np.any(np.abs(q[1:]) > grid["half"]) or np.linalg.norm(x - cen) > grid["radius"]:
            continue
        g = np.clip((SZ * (q[1:] / RES + 0.5)).astype(int), 0, SZ - 1)
        cell = SZ * g[0] + g[1]
        if prm["use_w"] and batch["W"][L, cell] == 0:
            continue
        if cells is not None and cells[L, cell] == rn.FREE:
            continue
        return L, t, x
    return -1, np.nan, None


def _check_against_brute(batch, grid, o, dirs, prm=None, cells=None):
    rays = rn.render(batch, grid, _flat_gp(18), o, dirs, prm, cells)
    used = 0
    for r, d in zip(rays, dirs):
        if r["tie"] or r["margin"] < 1e-9:
            continue
        used += 1
        L, t, x = _brute(batch, grid, o, d, prm or {}, cells)
        assert r["leaf"] == L, (d, r["leaf"], L, r["visited"])
        if L >= 0:
            assert abs(r["t"] - t) <= 1e-12 * max(1.0, abs(t)) and np.max(np.abs(r["x"] - x)) <= 1e-12
            assert r["local"][0] == 0.0 and np.array_equal(r["x"], r["x"])
        else:
            assert np.isnan(r["t"]) and np.all(np.isnan(r["local"])) and np.all(np.isnan(r["x"]))
    assert used >= 0.95 * len(dirs)
    return rays


def test_flat_layers_first_layer_occludes_the_second():
    batch, grid = _layers()
    rng = np.random.default_rng(0)
    dirs = _fan(rng, SENSOR, 300)
    rays = _check_against_brute(batch, grid, SENSOR, dirs)
    leaf = np.array([r["leaf"] for r in rays])
    # every ray that passes the upper layer's footprint stops there: the lower layer is reached only from the side, under the rim
    assert np.sum(leaf >= 9) > 100 and np.sum(leaf < 0) > 20
    for r in rays:
        if r["leaf"] >= 0:
            x = r["x"]
            if 0.0 < x[0] < 0.75 and 0.0 < x[1] < 0.75 and r["leaf"] < 9:
                up = SENSOR + (0.905 - SENSOR[2]) / (x[2] - SENSOR[2]) * (x - SENSOR)     # where it crossed the upper plane z = 0.905
                assert not (0.0 <= up[0] <= 0.75 and 0.0 <= up[1] <= 0.75)
    cnt = rn.counts_of(rays)
    assert cnt[0] == 300 and cnt[1] == np.sum(leaf >= 0) and cnt[2] == sum(r["outside"] for r in rays) and cnt[4] == 0
    assert cnt[3] >= cnt[1]


def test_holes_in_w_and_free_cells_let_the_ray_through():
    batch, grid = _layers()
    rng = np.random.default_rng(1)
    dirs = _fan(rng, SENSOR, 200)
    base = rn.render(batch, grid, _flat_gp(18), SENSOR, dirs)
    through = [i for i, r in enumerate(base) if r["leaf"] >= 9 and r["margin"] > 1e-9]
    assert len(through) > 60
    # a W hole on the upper layer: the ray goes on (to the lower layer, or out), unless use_w is off
    holes = batch["W"].copy()
    cells = np.zeros((18, M), np.uint8)
    for i in through[::2]:
        holes[base[i]["leaf"], base[i]["tests"][-1]["cell"]] = 0
        cells[base[i]["leaf"], base[i]["tests"][-1]["cell"]] = rn.FREE
    for i in through[1::2]:                                                  # occupied and unobserved cells stop a ray as before
        if cells[base[i]["leaf"], base[i]["tests"][-1]["cell"]] == 0:
            cells[base[i]["leaf"], base[i]["tests"][-1]["cell"]] = rr.OCCUPIED
    holed = dict(batch, W=holes)
    a = _check_against_brute(holed, grid, SENSOR, dirs)
    b = _check_against_brute(holed, grid, SENSOR, dirs, dict(use_w=0))
    c = _check_against_brute(batch, grid, SENSOR, dirs, None, cells)
    went_on = 0
    for i in through:
        L, cell = base[i]["leaf"], base[i]["tests"][-1]["cell"]
        assert b[i]["leaf"] == L
        for out, masked in ((a[i], holes[L, cell] == 0), (c[i], cells[L, cell] == rn.FREE)):
            if masked:
                assert out["leaf"] < 9 and len(out["tests"]) >= len(base[i]["tests"])
                went_on += out["leaf"] >= 0
            else:
                assert out["leaf"] == L
    assert went_on > 20                                                      # ... and reach the lower layer


def test_tilted_frames_axis_aligned_rays_inside_start_and_t_max():
    batch, grid = _layers(tilt=0.08)
    rng = np.random.default_rng(2)
    dirs = _fan(rng, SENSOR, 250)
    rays = _check_against_brute(batch, grid, SENSOR, dirs)
    leaf = np.array([r["leaf"] for r in rays])
    assert np.sum(leaf >= 9) > 80 and np.sum((leaf >= 0) & (leaf < 9)) >= 1 and np.sum(leaf < 0) > 10
    assert max(len(r["visited"]) for r in rays) >= 5 and any(len(r["tests"]) >= 2 for r in rays)
    # straight down (d_x = d_y = 0), from above and from between the layers; straight up from there meets the upper layer from below
    above, inside = np.array([0.3, 0.45, 1.6]), np.array([0.3, 0.45, 0.6])
    down, up = np.array([[0.0, 0.0, -1.0]]), np.array([[0.0, 0.0, 2.0]])
    r = _check_against_brute(batch, grid, above, down)[0]
    assert r["leaf"] >= 9 and [c[:2] for c in r["visited"]] == [(1, 1)] * len(r["visited"]) and r["visited"][0][2] == 4
    r = _check_against_brute(batch, grid, inside, down)[0]
    assert 0 <= r["leaf"] < 9 and r["visited"][0] == (1, 1, 2) and not r["outside"]
    r = _check_against_brute(batch, grid, inside, up)[0]
    assert r["leaf"] >= 9 and r["visited"][0] == (1, 1, 2)
    # beside the box, and pointing away from it: never meets the grid
    for o, d in ((np.array([2.0, 0.4, 1.6]), [0.0, 0.0, -1.0]), (above, [0.0, 0.0, 1.0]), (above, [np.nan, 0.0, -1.0]), (above, [0.0, 0.0, 0.0])):
        r = rn.render(batch, grid, _flat_gp(18), o, np.array([d]))[0]
        assert r["outside"] and r["leaf"] == -1 and not r["visited"]
    # t_max cuts a hit: every later surface is further still
    hit = next(r for r, d in zip(rays, dirs) if r["leaf"] >= 9 and r["margin"] > 1e-9)
    d = dirs[[i for i, r in enumerate(rays) if r is hit][0]][None, :]
    assert _check_against_brute(batch, grid, SENSOR, d, dict(t_max=hit["t"] * 1.01))[0]["leaf"] == hit["leaf"]
    assert _check_against_brute(batch, grid, SENSOR, d, dict(t_max=hit["t"] * 0.99))[0]["leaf"] == -1


def test_one_curved_leaf_against_a_bracketing_root_finder():
    from scipy.optimize import brentq
    batch, grid = rcs.layered_map([(0, 0.0)], kz_max=0, nx=1, ny=1)
    batch["W"] = np.ones((1, M), np.uint8)
    gp = dict(sf=1.0, l_sq=(RES / 2) ** 2, b=np.ones(1, np.int32), alpha=np.zeros((1, 1, 16)), BV=np.zeros((1, 16, 2)))
    gp["alpha"][0, 0, 0], gp["BV"][0, 0] = 0.03, (0.02, -0.03)             # a 3 cm bump
    o = np.array([0.3, -0.1, 0.9])
    rng = np.random.default_rng(5)
    tgt = np.stack([rng.uniform(0.01, 0.24, 60), rng.uniform(0.01, 0.24, 60), np.full(60, 0.125)], 1)
    dirs = tgt - o
    rays = rn.render(batch, grid, gp, o, dirs)
    R, mu = batch["R"][0], batch["mean"][0]
    tol = rn.DEFAULTS["eps_rel"] * RES
    hits = 0
    for r, d in zip(rays, dirs):
        a, c = R.T @ (o - mu), R.T @ d

        def g(t):
            return (a[0] + t * c[0]) - rn.gp_mean(gp, 0, a[1] + t * c[1], a[2] + t * c[2], grad=False)[0]
        t0 = -a[0] / c[0]
        root = brentq(g, t0 - 0.1, t0 + 0.1, xtol=1e-15, rtol=8.9e-16)
        s = r["tests"][0]
        assert s["finite"] and not s["resid"]                                # four Newton iterations from the plane converge
        assert abs(s["t"] - root) <= tol / abs(s["gprime"])
        if r["leaf"] == 0:
            hits += 1
            assert abs(r["local"][0]) > 1e-4 or np.hypot(*(r["local"][1:] - gp["BV"][0, 0])) > 0.3
    assert hits > 40 and max(r["local"][0] for r in rays if r["leaf"] == 0) > 0.02


def test_forward_walk_reversed_is_the_ray_casts_walk():
    """rays from a sensor (above the box, and inside it) through points on leaf planes: the forward walk's voxel list up to the owner's
    voxel, reversed, is raycast_ref.walk from that voxel"""
    batch, grid = rcs.layered_map([(0, 0.02), (2, -0.03)], kz_max=4, tilt=0.08, seed=4)
    rng = np.random.default_rng(4)
    xyz = np.concatenate([rcs.points_on(batch, grid, L, rng.uniform(-0.12, 0.12, 12), rng.uniform(-0.12, 0.12, 12)) for L in range(18)])
    owned, owner = rcs.own(batch, grid, xyz)
    empty = dict(_flat_gp(18), b=np.zeros(18, np.int32))                     # no leaf is trained: the walk crosses the whole box
    vox = grid["vox"] - grid["koff"]
    compared = longest = 0
    for sensor in (np.array([0.31, 0.44, 1.3]), np.array([0.6, 0.2, 0.6])):
        for i in np.flatnonzero(owner >= 0):
            o, delta = rr.ray_of(xyz[i], sensor)
            c_own = tuple(int(v) for v in vox[owner[i]])
            if not rr.slab(grid, vox[owner[i]], o, delta)[0]:
                continue
            r = rn.render(batch, grid, empty, o, delta[None, :])[0]
            if r["tie"]:
                continue
            assert not r["tests"] and c_own in r["visited"]
            fwd = r["visited"][:r["visited"].index(c_own) + 1]
            assert fwd[::-1] == rr.walk(grid, vox[owner[i]], o, delta)
            compared += 1
            longest = max(longest, len(fwd))
    assert compared > 300 and longest >= 4


def _random_gp(rng, P, b, ld=32, amp=0.01):
    gp = dict(sf=1.0, l_sq=(RES / 5) ** 2, b=np.full(P, b, np.int32), alpha=np.zeros((P, 1, ld)), BV=np.zeros((P, ld, 2)))
    gp["alpha"][:, 0, :b] = amp * rng.standard_normal((P, b))
    gp["BV"][:, :b] = rng.uniform(-RES / 2, RES / 2, (P, b, 2))
    return gp


def test_undecided_rays_stay_below_the_cap():
    """The GPU tests compare hit / miss and the leaf exactly, except for rays whose margin is below 1e-6 res, and allow at most 2 % of
    a scene's rays to be excluded.  On a hand-made curved state of the same geometry (two tilted layers, res 0.25, the images of the
    GPU tests) the share is far below that: a margin is a length, the boundaries are lines in a 3 cm-scale window.  (With eps_rel =
    1e-6 instead of render_ref.EPS_REL_SCENES every converged test would count as undecided: see there.)"""
    batch, grid = _layers(tilt=0.08)
    rng = np.random.default_rng(7)
    gp = _random_gp(rng, 18, 12)
    look_down = np.array([[1.0, 0.0, 0.0], [0.0, -1.0, 0.0], [0.0, 0.0, -1.0]])
    for o, (w, h, f) in ((SENSOR, (23, 17, 18.0)), (np.array([0.3, 0.45, 0.6]), (23, 17, 9.0))):
        dirs = rn.camera_rays(look_down, f, f, (w - 1) / 2, (h - 1) / 2, w, h)
        rays = rn.render(batch, grid, gp, o, dirs, dict(eps_rel=rn.EPS_REL_SCENES))
        low = sum(r["margin"] < 1e-6 * RES for r in rays)
        hits = sum(r["leaf"] >= 0 for r in rays)
        print("rays", len(rays), "hits", hits, "margin below 1e-6 res", low)
        assert low <= 0.02 * len(rays) and hits > 0.3 * len(rays)
    assert np.array_equal(rn.camera_rays(np.eye(3), 2.0, 4.0, 1.0, 0.5, 3, 2)[4], [0.0, 0.125, 1.0])
    assert [rn.flatten(v) for v in (-3.2, 0.9, 254.99, 255.0, 300.0, 32768.0, 65536.0 + 7.5, np.nan, np.inf)] == \
        [0, 0, 254, 255, 255, 0, 7, 255, 255]
