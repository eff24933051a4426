#!/usr/bin/env python3
"""Side measurement (not the headline bench): the masked decoder gpc_sparse_decode_dev against the flow it replaces, on the C4-defaults
batch of bench.py -- 32768 leaves x 256 points streamed in 4 add calls at the reference's default hyper-parameters (basis ~13), the colour
GP trained alike, sz = 20 -- in one process, every leg the median of --steps HIP-event times after --warmup calls:

    A   Sparse.predict_dev (depth) + Sparse.predict_dev (colour) + Context.reproject_dev: the yardstick
    B   the decoder with no mask
    C   the decoder under W of fill 0.25, 0.5, 0.75 (every leaf: a random contiguous run of cells)
    D   the sizing call alone (count + scan) under the fill-0.5 mask

Per leg: the time, points per second, and the bytes written and read by the arithmetic of the rule (not counters).  Also, on the plane
cloud of tests/test_decode_host_gpu.py through the host class: the mean nearest-neighbour distance from the decoded points to the
original cloud, masked and unmasked.  Prints one JSON line (and writes it to --out).

    python tools/bench_decode.py --out profiles/decode_bench.json
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402
from gp_compressor_amd import capi, host_api, synth  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--leaves", type=int, default=32768)
ap.add_argument("--steps", type=int, default=20)
ap.add_argument("--warmup", type=int, default=5)
ap.add_argument("--out")
a = ap.parse_args()

RES, SZ, N, CHUNKS, CAP = 0.15, 20, 256, 4, 200
M = SZ * SZ
P = a.leaves
assert torch.cuda.is_available(), "needs the GPU: there is no CPU path to time"
ctx = capi.Context(0)
torch.cuda.set_stream(torch.cuda.Stream())
ctx.set_stream(torch.cuda.current_stream().cuda_stream)      # kernels and events share torch's current stream
t = lambda x: torch.from_numpy(np.ascontiguousarray(x)).cuda()


def trained(ny):
    off, x0, x1, y = synth.make_patches(P, N, res=RES, seed=4, ny=ny)
    g = capi.Sparse(ctx, capi.default_params_sparse(ny, capacity=CAP), P, ny)
    cn = N // CHUNKS
    coff = t((np.arange(P + 1) * cn).astype(np.int32))
    for c in range(CHUNKS):
        idx = (off[:-1, None].astype(np.int64) + np.arange(c * cn, (c + 1) * cn)[None, :]).reshape(-1)
        g.add_dev(coff, cn, P * cn, t(x0[idx]), t(x1[idx]), t(y[:, idx]))
        torch.cuda.synchronize()
    return g


gd, gc = trained(1), trained(3)
bd, bc = gd.sizes().astype(np.int64), gc.sizes().astype(np.int64)
rng = np.random.default_rng(5)
Q, _ = np.linalg.qr(rng.normal(size=(P, 3, 3)))
d_R = t(np.swapaxes(Q, 1, 2).reshape(P, 9))
d_mu, d_cm = t(rng.uniform(-50, 50, (P, 3))), t(rng.uniform(0, 255, (P, 3)))
xs0, xs1 = synth.grid(RES, SZ)
d_xs0, d_xs1, d_bv = t(xs0), t(xs1), t(bd.astype(np.int32))
f = torch.empty((P, M), dtype=torch.float64, device="cuda")
c = torch.empty((P, 3, M), dtype=torch.float64, device="cuda")
cloud = torch.empty((P * M, 32), dtype=torch.uint8, device="cuda")
npts = torch.zeros(1, dtype=torch.int32, device="cuda")
count = torch.zeros(P, dtype=torch.int32, device="cuda")


def window_mask(fill):
    """W (P, m) uint8: per leaf a contiguous run of round(fill m) cells from a random start"""
    k = int(round(fill * M))
    start = rng.integers(0, M - k + 1, P)
    cell = np.arange(M)[None, :]
    return ((cell >= start[:, None]) & (cell < start[:, None] + k)).astype(np.uint8)


def leg_a():
    gd.predict_dev(M, d_xs0, d_xs1, f)
    gc.predict_dev(M, d_xs0, d_xs1, c)
    ctx.reproject_dev(P, M, d_bv, d_xs0, d_xs1, f, c, d_R, d_mu, d_cm, cloud, npts)


def decode(W, sizing=False):
    gd.decode_dev(gc, RES, SZ, W, None, d_R, d_mu, d_cm, 0 if sizing else P * M, None if sizing else cloud, count=count, n_points=npts)


def timed(fn):
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(a.steps)]
    for _ in range(a.warmup):
        fn()
    torch.cuda.synchronize()
    for s, e in ev:
        s.record()
        fn()
        e.record()
    torch.cuda.synchronize()
    ms = [s.elapsed_time(e) for s, e in ev]
    return float(np.median(ms)), [min(ms), max(ms)], int(npts.cpu()[0])


trained_leaves = bd > 0
state_bytes = int(8 * (3 * bd[trained_leaves].sum() + 5 * bc[trained_leaves].sum()) + 15 * 8 * trained_leaves.sum())
legs = {}


def record(name, ms, mm, n, written, read, **kw):
    legs[name] = dict(ms=ms, ms_min_max=mm, points=n, points_per_s=(n / (1e-3 * ms) if n else 0.0), bytes_written=int(written), bytes_read=int(read),
                      **kw)


ms, mm, n_full = timed(leg_a)
ref_bytes = cloud[:n_full].cpu().numpy().tobytes()
# A: f* and C* go out (8 + 24 bytes per point) and come back, the records go out; states, grid and frames are read
record("A_predict_predict_reproject", ms, mm, n_full, 64 * n_full, 32 * n_full + state_bytes + 16 * M)
ms, mm, n = timed(lambda: decode(None))
same = cloud[:n].cpu().numpy().tobytes() == ref_bytes and n == n_full
record("B_decode_no_mask", ms, mm, n, 32 * n + 8 * P + 4, state_bytes + 8 * P, same_bytes_as_A=bool(same))
masks = {}
for fill in (0.25, 0.5, 0.75):
    masks[fill] = t(window_mask(fill))
    ms, mm, n = timed(lambda: decode(masks[fill]))
    # W is read twice: by the count and by the emit
    record(f"C_decode_fill_{fill}", ms, mm, n, 32 * n + 8 * P + 4, state_bytes + 8 * P + 2 * P * M, fill=n / n_full)
ms, mm, n = timed(lambda: decode(masks[0.5], sizing=True))
record("D_sizing_fill_0.5", ms, mm, n, 8 * P + 4, 4 * P + P * M + 4 * P)

# what the mask is for: distance of the decoded points to the cloud they came from (the plane cloud of tests/test_decode_host_gpu.py)
xyz, rgb = host_api.synthetic_plane_cloud(2500, seed=1, extent=0.45)
g = host_api.GpCompressor(xyz, rgb, res=0.15, sz=10, model="sparse", seed=7)
g.set_sparse_kernel(1.0, (0.15 / 2) ** 2, 1e-2, 25.0, 40)
full_xyz = g.roundtrip()[0]
masked_xyz = g.load_compressed(masked=True)[0]


def mean_nn(pts):
    d = torch.cdist(torch.from_numpy(pts.astype(np.float64)), torch.from_numpy(xyz.astype(np.float64)))
    return float(d.min(dim=1).values.mean())


rec = {"workload": f"C4 defaults: {P} leaves x {N} points in {CHUNKS} add calls, capacity {CAP}, depth + colour GP at the reference's default "
                   f"hyper-parameters, sz {SZ}; decode of the whole batch to 32-byte records",
       "P": P, "m": M, "mean_basis_depth": float(bd.mean()), "mean_basis_rgb": float(bc.mean()), "steps_timed": a.steps, "warmup": a.warmup,
       "protocol": "median of HIP-event times around the enqueued calls, one process, profiler off, one run on one MI355X; bytes by the "
                   "arithmetic of the rule, not counters",
       "legs": legs, "B_over_A": legs["B_decode_no_mask"]["ms"] / legs["A_predict_predict_reproject"]["ms"],
       "plane_cloud_nn": {"cloud": "plane_cloud(2500, extent 0.45), res 0.15, sz 10, host class", "points_unmasked": int(len(full_xyz)),
                          "points_masked": int(len(masked_xyz)), "mean_nn_unmasked_m": mean_nn(full_xyz), "mean_nn_masked_m": mean_nn(masked_xyz)}}
line = json.dumps(rec)
print(line)
if a.out:
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        fh.write(line + "\n")
for o in (gd, gc):
    o.close()
ctx.close()
