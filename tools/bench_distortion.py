#!/usr/bin/env python3
"""Side measurement (not the headline bench): gpc_cloud_distortion_dev on the decode of tools/bench_decode.py -- the C4-defaults batch, 32768
leaves x 256 points at the reference's default hyper-parameters, decoded at sz = 20 to 13 M records -- against a synthetic original of the
same surface: per leaf 256 of its 400 decoded grid points, moved by N(0, 2 mm) per axis, colours by N(0, 6) per channel.  One process,
every leg the median of --steps HIP-event times after --warmup calls:

    decoded -> original and original -> decoded, each at the library's cell (cell = 0), at half and at twice that cell
    the yardstick: a chunked brute force on the same GPU (torch.cdist over blocks of B, running minimum), timed on --brute points of A
    against the whole of B and scaled to the whole of A

Per leg: the time, A points per second, and the bytes one point's search reads by the arithmetic of the rule when it ends after rings 0
and 1 (the usual case here: the neighbour is closer than one cell): 9 row searches of ceil(log2 voxels) 8-byte keys and two 4-byte
segment ends each, and 20 bytes (the 16-byte sorted record and its 4-byte index) per candidate in the 27 voxels, counted on a sample.
Prints one JSON line (and writes it to --out).

    python tools/bench_distortion.py --out profiles/distortion_bench.json
"""
import argparse
import json
import math
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
ap.add_argument("--warmup", type=int, default=3)
ap.add_argument("--brute", type=int, default=8192, help="points of A the brute-force yardstick is timed on")
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


# the decode of tools/bench_decode.py: random frames, leaf centres in a 100 m cube
gd, gc = trained(1), trained(3)
rng = np.random.default_rng(5)
Q, _ = np.linalg.qr(rng.normal(size=(P, 3, 3)))
d_R = t(np.swapaxes(Q, 1, 2).reshape(P, 9))
d_mu, d_cm = t(rng.uniform(-50, 50, (P, 3))), t(rng.uniform(0, 255, (P, 3)))
dec = torch.zeros((P * M, 32), dtype=torch.uint8, device="cuda")
npts = torch.zeros(1, dtype=torch.int32, device="cuda")
gd.decode_dev(gc, RES, SZ, None, None, d_R, d_mu, d_cm, P * M, dec, n_points=npts)
torch.cuda.synchronize()
n_dec = int(npts.cpu()[0])
dec = dec[:n_dec].contiguous()

# the synthetic original: per leaf 256 of its decoded points, with sensor noise
gen = torch.Generator(device="cuda").manual_seed(6)
leaves = n_dec // M
pick = torch.rand((leaves, M), device="cuda", generator=gen).argsort(dim=1)[:, :N] + (torch.arange(leaves, device="cuda") * M)[:, None]
org = dec[pick.reshape(-1)].clone()
xyz = org[:, :12].view(torch.float32)
xyz += 0.002 * torch.randn(xyz.shape, device="cuda", generator=gen)
col = org[:, 16:19]
col.copy_((col.to(torch.float32) + 6.0 * torch.randn(col.shape, device="cuda", generator=gen)).round().clamp(0, 255).to(torch.uint8))
n_org = len(org)
torch.cuda.synchronize()


def xyz64(c):
    return c[:, :12].view(torch.float32).to(torch.float64)


def library_cell(b):
    """the rule of include/gpc.h for cell = 0, restated: (cell, occupied voxels at it)"""
    p = xyz64(b)
    mn = p.min(0).values
    e = torch.sort(p.max(0).values - mn, descending=True).values.cpu().numpy()
    n = len(b)
    floor = e[0] / 2 ** 20

    def occupied(c):
        k = torch.floor((p - mn) / c).to(torch.int64)
        return int(torch.unique((k[:, 2] << 42) | (k[:, 1] << 21) | k[:, 0]).numel())
    c0 = max(math.sqrt(4.0 * e[0] * e[1] / n), floor)
    crowd = n / occupied(c0)
    c = max(c0 * math.sqrt(4.0 / crowd), floor) if crowd > 8.0 else c0
    return c, occupied(c)


def candidates(aq, b, cell, sample=4096):
    """mean number of B's points in the 27 voxels around the voxel of a point of A (a sample of A), and the occupied voxels"""
    pb = xyz64(b)
    mn = pb.min(0).values
    kmax = torch.floor((pb.max(0).values - mn) / cell).to(torch.int64)
    pack = lambda k: (k[:, 2] << 42) | (k[:, 1] << 21) | k[:, 0]
    keys, counts = torch.unique(pack(torch.floor((pb - mn) / cell).to(torch.int64)), return_counts=True)
    sel = torch.randperm(len(aq), device="cuda", generator=gen)[:sample]
    ka = torch.minimum(torch.maximum(torch.floor((xyz64(aq[sel]) - mn) / cell).to(torch.int64), torch.zeros_like(kmax)), kmax)
    total = torch.zeros(len(sel), dtype=torch.int64, device="cuda")
    for dz in (-1, 0, 1):
        for dy in (-1, 0, 1):
            for dx in (-1, 0, 1):
                k = ka + torch.tensor([dx, dy, dz], device="cuda")
                ok = ((k >= 0) & (k <= kmax)).all(1)
                want = pack(k.clamp(min=0))
                j = torch.searchsorted(keys, want).clamp(max=len(keys) - 1)
                total += torch.where(ok & (keys[j] == want), counts[j], torch.zeros_like(counts[j]))
    return float(total.to(torch.float64).mean()), int(len(keys))


res_dev = torch.zeros(capi.DISTORTION_RESULT_DTYPE.itemsize, dtype=torch.uint8, device="cuda")


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
    return float(np.median(ms)), [min(ms), max(ms)]


legs = {}
first = {}
for name, (qa, na, qb, nb) in {"decoded_to_original": (dec, n_dec, org, n_org), "original_to_decoded": (org, n_org, dec, n_dec)}.items():
    lib_cell, _ = library_cell(qb)
    for label, cell_arg, cell in (("library", 0.0, lib_cell), ("half", 0.5 * lib_cell, 0.5 * lib_cell), ("twice", 2.0 * lib_cell, 2.0 * lib_cell)):
        fn = lambda: ctx.cloud_distortion_dev(qa, na, qb, nb, cell=cell_arg, result=res_dev)
        ms, mm = timed(fn)
        r = res_dev.cpu().numpy().view(capi.DISTORTION_RESULT_DTYPE)[0]
        raw = res_dev.cpu().numpy().tobytes()
        first.setdefault(name, raw)
        cand, vox = candidates(qa, qb, cell)
        legs[f"{name}_cell_{label}"] = dict(
            ms=ms, ms_min_max=mm, cell=cell, points=na, points_per_s=na / (1e-3 * ms), occupied_voxels=vox, candidates_two_rings=cand,
            search_bytes_per_point_two_rings=9 * (math.ceil(math.log2(max(vox, 2))) * 8 + 8) + 20.0 * cand,
            same_result_as_library_cell=bool(raw == first[name]), n_matched=int(r["n_matched"]),
            mse_d1=float(r["sse_d1"] / max(int(r["n_matched"]), 1)))


def brute(qa, qb, block=1 << 15):
    pa, pb = xyz64(qa), xyz64(qb)
    best = torch.full((len(pa),), float("inf"), dtype=torch.float64, device="cuda")
    for lo in range(0, len(pb), block):
        best = torch.minimum(best, torch.cdist(pa, pb[lo:lo + block]).min(dim=1).values)
    return best


sub = dec[torch.randperm(n_dec, device="cuda", generator=gen)[:a.brute]].contiguous()
ms_b, mm_b = timed(lambda: brute(sub, org))
d_b = brute(sub, org)
d2 = torch.zeros(len(sub), dtype=torch.float64, device="cuda")
ctx.cloud_distortion_dev(sub, len(sub), org, n_org, d2=d2, result=res_dev)
ctx.synchronize()
lib_ms = legs["decoded_to_original_cell_library"]["ms"]
yard = dict(subsample_points=len(sub), ms=ms_b, ms_min_max=mm_b, points_per_s=len(sub) / (1e-3 * ms_b), ms_scaled_to_all_of_A=ms_b * n_dec / len(sub),
            exact_search_speedup_over_scaled_brute_force=ms_b * n_dec / len(sub) / lib_ms,
            max_abs_difference_of_distances_m=float((d2.sqrt() - d_b).abs().max()))

# the figures DESIGN.md quotes, on the plane cloud of tests/test_decode_host_gpu.py through the host class: what the mask buys, and one
# rate-distortion step (the model file as trained against the same model pruned to 60 % of its bytes)
xyz_p, rgb_p = host_api.synthetic_plane_cloud(2500, seed=1, extent=0.45)
PEAK = 0.45
g = host_api.GpCompressor(xyz_p, rgb_p, res=0.15, sz=10, model="sparse", seed=7)
g.set_sparse_kernel(1.0, (0.15 / 2) ** 2, 1e-2, 25.0, 40)
g.set_field_delete_bug(0)
orig_p = ctx.make_cloud(xyz_p, rgb_p)


def plane_row(dxyz, drgb):
    rep = g.distortion(dxyz, drgb, PEAK)
    one = ctx.cloud_distortion(ctx.make_cloud(dxyz, drgb), orig_p, want=("d2",))
    return dict(points=int(len(dxyz)), mean_nn_m=float(np.sqrt(one["d2"]).mean()), mse_d1=[float(v) for v in rep["d1"]["mse"]],
                psnr_d1=float(rep["d1"]["psnr"]), psnr_d2=float(rep["d2"]["psnr"]), psnr_luma=float(rep["luma"]["psnr"]))


full = g.roundtrip()
plane = {"cloud": "plane_cloud(2500, extent 0.45), res 0.15, sz 10, host class; peak 0.45 m (the cloud's extent)",
         "unmasked": plane_row(full[0], full[1]), "masked": plane_row(*g.load_compressed(masked=True))}
bytes_full = g.model_bytes()
budget = int(0.6 * bytes_full)
removed = g.prune_to_bytes(budget)
plane["rate_distortion"] = {"save_model": dict(model_bytes=bytes_full, psnr_d1=plane["unmasked"]["psnr_d1"]),
                            "prune_to_bytes": dict(budget=budget, model_bytes=g.model_bytes(), removed=list(removed), **plane_row(*g.load_compressed()))}

rec = {"workload": f"C4 defaults: {P} leaves x {N} points in {CHUNKS} add calls, capacity {CAP}, decoded at sz {SZ} to {n_dec} records; synthetic original: "
                   f"{N} of each leaf's {M} decoded points + N(0, 2 mm), {n_org} records",
       "steps_timed": a.steps, "warmup": a.warmup,
       "protocol": "median of HIP-event times around the whole call (compaction, table, sort of A, search, sums; it synchronises inside), one process, "
                   "profiler off, one run on one MI355X; bytes by the arithmetic of the rule, not counters",
       "legs": legs, "brute_force_yardstick": yard, "plane_cloud": plane}
line = json.dumps(rec)
print(line)
if a.out:
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        fh.write(line + "\n")
for o in (gd, gc):
    o.close()
ctx.close()
