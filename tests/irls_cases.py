"""Inputs of the probit Newton / IRLS tests (test_irls_gpu.py), shared with test_irls_cases_cpu.py so that the batches and what the GPU
tests assume of the oracle on them can be checked without a GPU.

Every batch is drawn by variance_cases._mixed_batch and labelled by synth.occupancy_labels (+1 at or above the patch's mean depth, -1
below).  Regime: test_irls_vs_oracle's -- sigma_f^2 = 1, l = res / 3, s20 = 0.25.  Two likelihoods: model 2 (a proper CDF) from the
textbook start f = 0 with tol 1e-10, model 1 (the reference's "Phi") from f = 0.25 y with tol 1e-7 (test_probit_gpu.py says why no lower)."""
import numpy as np

from gp_compressor_amd import synth
import variance_cases as VC

RES = 0.15
REGIME = (1.0, (RES / 3) ** 2, 0.25)        # (sigma_f^2, l^2, s20)
MAX_ITER = 30
MODELS = {2: dict(f_init=0.0, tol=1e-10), 1: dict(f_init=0.25, tol=1e-7)}
FTOL = {2: 1e-8, 1: 1e-6}                   # f*, fhat, alpha against the oracle, of the patch's max-norm (test_probit_gpu.py)

# tile counts 1 .. 5, 16 .. 21, 32, 33, 48, 49 and 60 .. 64: every nt mod 4 (the kernel takes four tile columns per step) at both ends of
# the range, sizes on and next to tile edges, two empty patches
TILE_SIZES_BIG = [1024, 0, 1, 15, 16, 17, 47, 48, 49, 63, 64, 65, 80, 255, 256, 257, 272, 273, 304, 320, 321, 511, 512, 513, 767, 768, 769,
                  960, 961, 976, 977, 992, 993, 1008, 1009, 1023, 0, 300]
# sub-batches by largest patch: slots of 64, 33 and 17 tile columns, all on the eight-wave shape (n_max > 256)
CAPS = (1024, 513, 272)
MODEL1_CAP = 529                            # the model-1 sweep runs on the sizes up to here (caps 513 and 272)

# more patches than workgroups: (P, largest patch, empty patches, patches with one NaN label, their size, where the NaN sits)
MANY = {
    "big": dict(P=600, n_hi=336, empty=(7, 263, 519, 599), nan=(5, 300, 590), nan_n=300, nan_at=(299, 150, 37), seed=91),
    "w4": dict(P=1100, n_hi=96, empty=(7, 263, 519, 1099), nan=(5, 300, 1090), nan_n=90, nan_at=(89, 40, 20), seed=93),
}


def labelled(batch):
    """(off, x0, x1, labels (N,)) of a _mixed_batch."""
    off, x0, x1, y = batch
    return off, x0, x1, synth.occupancy_labels(off, y[0])


def take(batch, idx):
    """take_patches for a labelled batch: the sub-batch of patches idx and the indices of its points in the full batch."""
    off, x0, x1, lab = batch
    (so, sx0, sx1, sy), pts = VC.take_patches(off, x0, x1, lab[None, :], list(idx))
    return (so, sx0, sx1, np.ascontiguousarray(sy[0])), pts


def tile_batch():
    return labelled(VC._mixed_batch(TILE_SIZES_BIG, seed=81))


def cap_index(cap):
    return [i for i, n in enumerate(TILE_SIZES_BIG) if n <= cap]


def w4_batch():
    """The four-wave shape's batch: 0, 1, then every tile edge +- 1 up to 256 points."""
    return labelled(VC._mixed_batch(VC.edge_sizes(256), seed=82))


def many_sizes(which):
    c = MANY[which]
    rng = np.random.default_rng(c["seed"])
    sizes = rng.integers(1, c["n_hi"] + 1, c["P"])
    sizes[0], sizes[1] = c["n_hi"], 1
    sizes[list(c["empty"])] = 0
    sizes[list(c["nan"])] = c["nan_n"]
    return [int(s) for s in sizes]


def many_batch(which):
    """P patches of 1 .. n_hi points, patch 0 the largest, four empty, three with one NaN label: at the patch's last point in the
    first of them (only the i < n guard stands between it and the padding), inside a middle tile in the other two."""
    c = MANY[which]
    off, x0, x1, lab = labelled(VC._mixed_batch(many_sizes(which), seed=c["seed"] + 1))
    for i, at in zip(c["nan"], c["nan_at"]):
        lab[off[i] + at] = np.nan
    return off, x0, x1, lab


def grid_batch(shape):
    """Five patches for the grid-size sweep on the eight-wave ("big") or the four-wave ("w4") shape."""
    sizes = [300, 0, 17, 420, 129] if shape == "big" else [256, 0, 1, 100, 37]
    return labelled(VC._mixed_batch(sizes, seed=85 if shape == "big" else 86))


def oracle_fit(oracle, batch, model, xs, max_iter=MAX_ITER, **kw):
    """orc_dense_irls_fit_predict_batch in the regime above: f* (P, m), alpha (N,), fhat (N,), iters (P,), status (P,)."""
    arg = dict(MODELS[model])
    arg.update(kw)
    return oracle.dense_irls_fit_predict_batch(oracle.dense_params(sigmaf_sq=REGIME[0], l_sq=REGIME[1], sigman_sq=REGIME[2]), model,
                                               *batch, *xs, max_iter=max_iter, **arg)
