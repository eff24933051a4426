"""GPU test of the C-ABI's multi-GPU entry points (include/gpc.h "multi-GPU"): a 1-rank RCCL communicator
on the one GPU of the box -- the all-gather degenerates to a copy, but the partition table, its inverse on the device, the
un-permutation kernel, the run-time binding of RCCL and both creation paths (gpc_comm_create with a unique id, the
single-process gpc_comm_create_all with a gpc_group bracket) are the code the N-rank run executes.  The N > 1 exchange
itself is rehearsed on CPU ranks with gloo (tests/test_dist_cpu.py) and runs in bench.py at N > 1."""
import ctypes as C

import numpy as np
import pytest

from gp_compressor_amd import synth

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def gp():
    from gp_compressor_amd import capi
    capi.load()
    ctx = capi.Context(0)
    yield capi, ctx
    ctx.close()


def _partition(capi, P, seed):
    off, _, _, _ = synth.make_patches(P, 64, seed=seed, ragged=True)
    slots = capi.partition_patches(off, 1)          # world 1: LPT order = patches sorted by cost, a non-trivial permutation
    assert sorted(slots.reshape(-1).tolist()) == list(range(P))
    return slots


def test_allgather_unpermute_one_rank(gp):
    import torch
    capi, ctx = gp
    ctx.set_stream(torch.cuda.current_stream().cuda_stream)
    P, row = 37, 3 * 25
    slots = _partition(capi, P, 5)
    comm = capi.Comm(ctx, 1, 0)
    assert "rccl" in capi.load().gpc_comm_library().decode().lower()
    comm.set_partition(P, slots)
    dev = torch.device("cuda:0")
    local = torch.randn((P, row), dtype=torch.float64, device=dev)          # row s = the grid of the patch in slot s
    gathered = torch.empty_like(local)
    f_star = torch.empty_like(local)
    comm.allgather_fstar_dev(row, local, gathered, f_star)
    ctx.synchronize()
    assert torch.equal(gathered, local)
    want = np.empty((P, row))
    want[slots.reshape(-1)] = local.cpu().numpy()
    assert np.array_equal(f_star.cpu().numpy(), want)
    # odd row length (the 8-byte path of the un-permutation kernel)
    row2 = 7
    loc2 = torch.randn((P, row2), dtype=torch.float64, device=dev)
    g2, f2 = torch.empty_like(loc2), torch.empty_like(loc2)
    comm.allgather_fstar_dev(row2, loc2, g2, f2)
    ctx.synchronize()
    w2 = np.empty((P, row2))
    w2[slots.reshape(-1)] = loc2.cpu().numpy()
    assert np.array_equal(f2.cpu().numpy(), w2)
    # a table that is not a partition is refused
    bad = slots.copy().reshape(-1)
    bad[1] = bad[0]
    with pytest.raises(capi.GpcError):
        comm.set_partition(P, bad)
    comm.close()
    ctx.set_stream(None)


def test_single_process_group_form(gp):
    """gpc_comm_create_all + gpc_group_start / gpc_group_end: how one host process drives the GPUs of a node (here: one)."""
    import torch
    capi, ctx = gp
    lib = capi.load()
    ctx.set_stream(torch.cuda.current_stream().cuda_stream)
    P, row = 19, 400
    slots = _partition(capi, P, 9)
    (comm,) = capi.Comm.all([ctx])
    assert lib.gpc_comm_world(comm.h) == 1 and lib.gpc_comm_rank(comm.h) == 0
    comm.set_partition(P, slots)
    dev = torch.device("cuda:0")
    local = torch.randn((P, row), dtype=torch.float64, device=dev)
    gathered, f_star = torch.empty_like(local), torch.empty_like(local)
    assert lib.gpc_group_start() == 0
    comm.allgather_fstar_dev(row, local, gathered, None)        # inside the bracket the collective is only recorded
    assert lib.gpc_group_end() == 0
    comm.unpermute_fstar_dev(row, gathered, f_star)
    ctx.synchronize()
    want = np.empty((P, row))
    want[slots.reshape(-1)] = local.cpu().numpy()
    assert np.array_equal(f_star.cpu().numpy(), want)
    comm.close()
    ctx.set_stream(None)


def test_sharded_dense_flow_through_the_c_abi(gp, oracle):
    """the whole N-rank recipe with world = 1, C-ABI calls only: partition -> this rank's slot batch -> fit + predict ->
    all-gather + un-permute -> the grids of the unsharded call, bit for bit (same kernel, same inputs per patch)"""
    import torch
    from gp_compressor_amd import dist as gdist
    capi, ctx = gp
    ctx.set_stream(torch.cuda.current_stream().cuda_stream)
    P, res, sz = 48, 0.15, 20
    off, x0, x1, y = synth.make_patches(P, 200, res=res, seed=21, ragged=True)
    slots, loff, lx0, lx1, ly = gdist.shard_batch(off, x0, x1, y, 1, 0)
    dev = torch.device("cuda:0")
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    prm = capi.default_params_dense()
    S, m = slots.shape[1], sz * sz
    d = [t(a) for a in (loff, lx0, lx1, ly)]
    local = torch.empty((S, m), dtype=torch.float64, device=dev)
    ctx.dense_fit_predict_grid_dev(prm, S, d[0], int(np.max(np.diff(loff))), int(loff[-1]), d[1], d[2], d[3], 1, res, sz, local)
    comm = capi.Comm(ctx, 1, 0)
    comm.set_partition(P, slots)
    gathered, f_star = torch.empty_like(local), torch.empty((P, m), dtype=torch.float64, device=dev)
    comm.allgather_fstar_dev(m, local, gathered, f_star)
    ctx.synchronize()
    f_ref, st = ctx.dense_fit_predict_grid(prm, off, x0, x1, y, res, sz)
    got = f_star.cpu().numpy()
    assert np.all(st == 0) and np.max(np.abs(got - f_ref[:, 0, :])) <= 1e-12 * np.max(np.abs(f_ref))
    xs0, xs1 = oracle.grid(res, sz)
    fo, _, _ = oracle.dense_fit_predict_batch(oracle.dense_params(), off, x0, x1, y, xs0, xs1)
    assert np.max(np.abs(got - fo[:, 0, :])) <= 1e-9 * np.max(np.abs(fo))
    comm.close()
    ctx.set_stream(None)


# ---- the un-permutation kernel on its own, and chained into the reprojection it feeds -------------------------------------------------------
UNPERMUTE_ROWS = (1, 2, 3, 256, 257, 258)      # even: 16-byte accesses, odd: 8-byte; below, at and above two passes of the 128 threads


@pytest.mark.parametrize("P", [1, 1025, 3000])
def test_unpermute_alone_under_a_random_permutation(gp, P):
    """gpc_unpermute_fstar_dev without a collective: every row of f* is its source row bit for bit, none stays as it was (NaN)"""
    import torch
    capi, ctx = gp
    ctx.set_stream(torch.cuda.current_stream().cuda_stream)
    rng = np.random.default_rng(300 + P)
    slots = rng.permutation(P).astype(np.int32)                 # slot s holds patch slots[s]: not the LPT order of a cost
    comm = capi.Comm(ctx, 1, 0)
    try:
        comm.set_partition(P, slots)
        for row in UNPERMUTE_ROWS:
            elems = row // 2 if row % 2 == 0 else row
            print("P = %d workgroups, rows of %d doubles: %d accesses of %d bytes, %d passes of the 128 threads" % (P, row, elems, 8 * row // elems, -(-elems // 128)))
            gathered = torch.randn((P, row), dtype=torch.float64, device="cuda")
            f_star = torch.full((P, row), float("nan"), dtype=torch.float64, device="cuda")
            comm.unpermute_fstar_dev(row, gathered, f_star)
            ctx.synchronize()
            want = np.empty((P, row))
            want[slots] = gathered.cpu().numpy()
            got = f_star.cpu().numpy()
            assert not np.isnan(got).any()
            assert np.array_equal(got.view(np.uint64), want.view(np.uint64))
    finally:
        comm.close()
        ctx.set_stream(None)


def test_sharded_tail_gather_unpermute_reproject(gp, oracle):
    """the tail of the sharded flow in one piece: f* (P, m) and C* (P, 3 m) in slot order -> all-gather + un-permutation of each (rows of
    m and of 3 m doubles) -> gpc_reproject_dev with a bv_count in patch order; the cloud is the oracle's on the patch-order inputs"""
    import torch
    import reproject_cases as RC
    capi, ctx = gp
    P, m = 1025, RC.COMPACTION_M
    bv, (xs0, xs1, f, R, mu, cs, cm) = RC.compaction_case(P, "random")
    n_on = len(RC.trained(P, bv))
    grid = min(P, 8 * torch.cuda.get_device_properties(0).multi_processor_count)
    print("P = %d, per = %d, emit grid = %d, trained = %d; un-permuted rows of %d and %d doubles" % (P, RC.per_of(P), grid, n_on, m, 3 * m))
    want = RC.expected(oracle, xs0, xs1, f, R, mu, cs, cm, bv)
    slots = np.random.default_rng(41).permutation(P).astype(np.int32)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    ctx.set_stream(torch.cuda.current_stream().cuda_stream)
    comm = capi.Comm(ctx, 1, 0)
    try:
        comm.set_partition(P, slots)
        local_f, local_c = t(f[slots]), t(cs.reshape(P, 3 * m)[slots])      # row s = the grids of the patch in slot s
        gath_f, gath_c = torch.empty_like(local_f), torch.empty_like(local_c)
        f_star = torch.full((P, m), float("nan"), dtype=torch.float64, device="cuda")
        c_star = torch.full((P, 3 * m), float("nan"), dtype=torch.float64, device="cuda")
        comm.allgather_fstar_dev(m, local_f, gath_f, f_star)
        comm.allgather_fstar_dev(3 * m, local_c, gath_c, c_star)
        out = torch.full((P * m, 32), 0xA5, dtype=torch.uint8, device="cuda")
        n_pts = torch.full((1,), -7, dtype=torch.int32, device="cuda")
        d_bv, d_xs0, d_xs1, d_R, d_mu, d_cm = (t(a) for a in (bv, xs0, xs1, R, mu, cm))
        ctx.reproject_dev(P, m, d_bv, d_xs0, d_xs1, f_star, c_star, d_R, d_mu, d_cm, out, n_pts)
        ctx.synchronize()
        n, raw = int(n_pts.cpu()[0]), out.cpu().numpy()
        assert np.array_equal(f_star.cpu().numpy(), f)
    finally:
        comm.close()
        ctx.set_stream(None)
    assert n == m * n_on == len(want)
    assert raw[:n].tobytes() == want.tobytes()
    assert np.all(raw[n:] == 0xA5)


def test_set_partition_refusals_keep_the_table(gp):
    """a slot that names no patch of the batch, a slot below -1 and an empty slot at world 1 (a patch is left without one): GPC_EINVAL
    each, and the un-permutation after each still goes by the table set before"""
    import torch
    capi, ctx = gp
    ctx.set_stream(torch.cuda.current_stream().cuda_stream)
    P, row = 37, 6
    slots = np.random.default_rng(17).permutation(P).astype(np.int32)
    comm = capi.Comm(ctx, 1, 0)
    try:
        comm.set_partition(P, slots)
        gathered = torch.randn((P, row), dtype=torch.float64, device="cuda")
        want = np.empty((P, row))
        want[slots] = gathered.cpu().numpy()
        for at, bad in ((3, P), (P - 1, P + 5), (0, -2), (20, -1)):
            table = slots.copy()
            table[at] = bad
            with pytest.raises(capi.GpcError) as e:
                comm.set_partition(P, table)
            assert e.value.code == capi.GPC_EINVAL
            f_star = torch.full((P, row), float("nan"), dtype=torch.float64, device="cuda")
            comm.unpermute_fstar_dev(row, gathered, f_star)
            ctx.synchronize()
            assert np.array_equal(f_star.cpu().numpy(), want)
    finally:
        comm.close()
        ctx.set_stream(None)
