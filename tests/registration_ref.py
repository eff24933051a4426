"""NumPy restatement of one gp_registration step (test infrastructure; the product never imports this module).

Written from /root/reference/src/gp_registration.cpp: the leaf walk of compute_transformation (:146-174) with get_local_points
(:94-113) as a per-point "first leaf that accepts" rule, the combination and the Jacobian (:196, :202-216, :40-49, :245),
gradient_step (:51-58), the pose update (:83-85), transform_pointcloud (:32-38) and registration_done (:67-70).  The model's
octree is replaced by the voxel table gp_compressor::project_cloud cut the model with (src/gp_compressor.cpp:177-249: leaves of
side res anchored at the cloud's minimum corner, visited in ascending (z, y, x) order), rebuilt here from the model cloud.

The assignment evaluates every expression in the association the GPU kernel uses (NumPy's element-wise operations do not
contract), so owners can be compared exactly.
"""
import numpy as np

B = 21                      # bits per voxel coordinate (the producer refuses more than 2^21 voxels along an axis)


def grid_of(model_xyz, res):
    """The voxel grid and leaf table of a model cloud: dict(mn, res, radius, half, kmax, keys); leaf id = index into keys."""
    xyz = np.asarray(model_xyz, dtype=np.float32)
    mn = xyz.min(axis=0).astype(np.float64)
    mx = xyz.max(axis=0).astype(np.float64)
    kmax = np.floor((mx - mn) / res).astype(np.int64)
    k = np.floor((xyz.astype(np.float64) - mn) / res).astype(np.int64)
    keys = np.unique(_key(k[:, 0], k[:, 1], k[:, 2]))
    radius = float(np.float32(np.sqrt(np.float32(3.0))) / np.float32(2.0)) * res       # sqrt(3.0f)/2.0f*res (:123)
    return dict(mn=mn, res=float(res), radius=radius, half=res / 2.0, kmax=kmax, keys=keys)


def _key(kx, ky, kz):
    return (kz.astype(np.int64) << (2 * B)) | (ky.astype(np.int64) << B) | kx.astype(np.int64)


def local_coords(p, R, mean):
    """R^T (p - mean) per point (:104); p (n, 3) float64, R (n, 3, 3) with columns normal, u, v, mean (n, 3)"""
    e = p - mean
    return np.stack([R[:, 0, a] * e[:, 0] + R[:, 1, a] * e[:, 1] + R[:, 2, a] * e[:, 2] for a in range(3)], axis=1)


def assign(scan_xyz, batch, grid, trained):
    """owner (n,) int32 (-1: unused) and local (n, 3) = (depth, x0, x1) in the owner's frame.  batch: the fetched patch batch
    (R (P, 3, 3), mean (P, 3)); trained (P,) bool: leaves whose depth GP is not empty (:158)."""
    p = np.asarray(scan_xyz, dtype=np.float32).astype(np.float64)
    n = len(p)
    mn, res, keys, kmax = grid["mn"], grid["res"], grid["keys"], grid["kmax"]
    P = len(keys)
    owner = np.full(n, -1, dtype=np.int32)
    local = np.zeros((n, 3))
    if n == 0 or P == 0:
        return owner, local
    with np.errstate(invalid="ignore", over="ignore"):
        kd = np.floor((p - mn) / res)
        near = np.all((kd >= -1.0) & (kd <= kmax + 1.0), axis=1)       # further out no leaf's sphere reaches (radius < 1.5 res)
    k = np.where(near[:, None], kd, 0.0).astype(np.int64)
    r2 = grid["radius"] * grid["radius"]
    half = grid["half"]
    for dz in (-1, 0, 1):                                               # ascending key order = leaf order
        for dy in (-1, 0, 1):
            for dx in (-1, 0, 1):
                nb = k + np.array([dx, dy, dz])
                cand = near & (owner < 0) & np.all((nb >= 0) & (nb <= kmax), axis=1)
                idx = np.flatnonzero(cand)
                if len(idx) == 0:
                    continue
                key = _key(nb[idx, 0], nb[idx, 1], nb[idx, 2])
                L = np.searchsorted(keys, key)
                ok = (L < P) & (keys[np.minimum(L, P - 1)] == key)
                idx, L, c = idx[ok], L[ok], nb[idx][ok]
                ok = trained[L]
                idx, L, c = idx[ok], L[ok], c[ok]
                cen = mn + (c.astype(np.float64) + 0.5) * res
                d = p[idx] - cen
                ok = d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1] + d[:, 2] * d[:, 2] <= r2       # radiusSearch (:161)
                idx, L = idx[ok], L[ok]
                q = local_coords(p[idx], batch["R"][L], batch["mean"][L])
                ok = ~((q[:, 1] > half) | (q[:, 1] < -half) | (q[:, 2] > half) | (q[:, 2] < -half))   # :105
                owner[idx[ok]] = L[ok]
                local[idx[ok]] = q[ok]
    return owner, local


def bucket(owner, P):
    """patch order, ascending scan index within a patch, unused points last: order (n,), off (P + 1,)"""
    key = np.where(owner < 0, P, owner)
    order = np.argsort(key, kind="stable")
    off = np.concatenate([[0], np.cumsum(np.bincount(key, minlength=P + 1)[:P])]).astype(np.int32)
    return order, off


def likelihood_tail(ny, sigma, sdx, second, offs, sq, pi=np.pi):
    """The per-point end of closed_form_likelihood, after the sums over the basis: sigma (..., m), sdx and second (..., m, 2),
    offs (ny, m), sq (m,) -> dX (..., m, 3), l (..., m).  Leading axes broadcast (a stack of variants of the sums at once)."""
    lik = 1.0 / np.sqrt((2 * pi) ** ny * sigma) * np.exp(-0.5 / sigma * sq)
    exppart = 0.5 / sigma ** 1.5 * np.exp(-0.5 / sigma * sq)
    d12 = exppart[..., None] * (-sdx + second + sdx / sigma[..., None] * sq[..., None])
    d0 = -1.0 / sigma ** 1.5 * offs[0] * exppart if ny == 1 else np.zeros_like(sigma)
    return np.concatenate([d0[..., None], d12], axis=-1), lik


def closed_form_likelihood(p0, p1, s20, alpha, Cm, BV, q0, q1, yq, dtype=None, parts=False):
    """likelihood and likelihood_dx (src/sparse_gp.hpp:387-427, 463-508; field src/sparse_gp_field.hpp:322-392) on a given state:
    alpha (ny, b), Cm (b, b), BV (b, 2), query q0, q1 (m,), yq (ny, m).  Returns dX (m, 3), l (m,).
    dtype: evaluate in that type (np.longdouble for an extended-precision reference) instead of the arguments' own.
    parts=True: a dict of the intermediate quantities as well -- A (b, m) the exponent's argument, K (b, m), mu (ny, m) the
    predictive mean, CK (b, m), sigma (m,) = s20 + k* + k^T C k (not clamped), Kdx, sdx, second, offs, sq, dX, l."""
    pi = np.pi
    if dtype is not None:
        p0, p1, s20 = dtype(p0), dtype(p1), dtype(s20)
        alpha, Cm, BV, q0, q1, yq = (np.asarray(a, dtype=dtype) for a in (alpha, Cm, BV, q0, q1, yq))
        pi = 4 * np.arctan(dtype(1))
    ny = alpha.shape[0]
    Xq = np.stack([q0, q1], 1)
    D = Xq[None, :, :] - BV[:, None, :]
    A = -0.5 / p1 * np.sum(D * D, axis=2)
    K = p0 * np.exp(A)
    mu = alpha @ K
    CK = Cm @ K
    sigma = s20 + p0 + np.sum(K * CK, axis=0)
    offs = yq - mu
    sq = np.sum(offs * offs, axis=0)
    Kdx = -(1.0 / p1) * D * K[:, :, None]
    sdx = 2.0 * np.einsum("imd,im->md", Kdx, CK)
    second = 2.0 * np.einsum("imd,ci,cm->md", Kdx, alpha, offs)
    dX, lik = likelihood_tail(ny, sigma, sdx, second, offs, sq, pi)
    if parts:
        return dict(A=A, K=K, mu=mu, CK=CK, sigma=sigma, Kdx=Kdx, sdx=sdx, second=second, offs=offs, sq=sq, dX=dX, l=lik)
    return dX, lik


def reduce_step(scan_rgb, owner, local, batch, lik_depth, lik_rgb):
    """Stages 2 and 4.  lik_depth(i, x0, x1, y (1, m)) and lik_rgb(i, x0, x1, c (3, m)) return (dX (m, 3), l (m,)) of patch i.
    Returns dict(delta (6,), ls, cls, n_used, gabs (6,) = sum |g| / n_used, the scale a difference of delta is measured in)."""
    P = len(batch["mean"])
    order, off = bucket(owner, P)
    rgb = np.asarray(scan_rgb, dtype=np.float64)
    G = np.zeros((0, 6))
    ls, cls = np.zeros(0), np.zeros(0)
    for i in range(P):
        idx = order[off[i]:off[i + 1]]
        if len(idx) == 0:
            continue
        q = local[idx]
        col = (rgb[idx] - batch["rgb_mean"][i]).T                                  # :169-171
        dX, l = lik_depth(i, q[:, 1], q[:, 2], q[:, 0][None, :])
        dC, cl = lik_rgb(i, q[:, 1], q[:, 2], np.ascontiguousarray(col))
        d = l[:, None] * dC + cl[:, None] * dX                                     # :196
        R = batch["R"][i]
        dg = d @ R.T                                                               # :204
        x = q @ R.T + batch["mean"][i]                                             # :206
        g = np.concatenate([dg, np.cross(x, dg)], axis=1)                          # d_glob^T J(x), J = [I | -[x]_x] (:40-49)
        G = np.concatenate([G, g])
        ls, cls = np.concatenate([ls, l]), np.concatenate([cls, cl])
    n_used = len(G)
    if n_used == 0:
        return dict(delta=np.zeros(6), ls=0.0, cls=0.0, n_used=0, gabs=np.zeros(6))
    return dict(delta=G.sum(axis=0) / n_used, ls=ls.sum() / n_used, cls=cls.sum() / n_used, n_used=n_used,
                gabs=np.abs(G).sum(axis=0) / n_used)


def gradient_step(delta, step):
    """R = Rx Ry Rz, t = step delta[0:3]  (:51-58)"""
    a, b, c = step * delta[3], step * delta[4], step * delta[5]
    Rx = np.array([[1, 0, 0], [0, np.cos(a), -np.sin(a)], [0, np.sin(a), np.cos(a)]])
    Ry = np.array([[np.cos(b), 0, np.sin(b)], [0, 1, 0], [-np.sin(b), 0, np.cos(b)]])
    Rz = np.array([[np.cos(c), -np.sin(c), 0], [np.sin(c), np.cos(c), 0], [0, 0, 1]])
    return Rx @ Ry @ Rz, step * np.asarray(delta[:3], dtype=np.float64)


def update_pose(R_cloud, t_cloud, R, t, ref_translation_sum=True):
    """:83-84 as written (t_cloud += t) or the composition of the rigid motions (t_cloud = R t_cloud + t)"""
    return R @ R_cloud, (t_cloud + t) if ref_translation_sum else (R @ t_cloud + t)


def transform_cloud(xyz, R, t):
    """(R p.cast<double>() + t).cast<float>()  (:36)"""
    return (np.asarray(xyz, dtype=np.float32).astype(np.float64) @ R.T + t).astype(np.float32)


def registration_done(step_nbr, delta, tol=0.1, min_steps=10, max_steps=300):
    """:69, with its constants as parameters"""
    return bool(step_nbr > min_steps and (step_nbr >= max_steps or
                                          (np.linalg.norm(delta[:3]) < tol and np.linalg.norm(delta[3:]) < tol)))
