"""CPU tests (-m "not gpu") of the rule that chooses the kernels of a dense batch (csrc/dense_route.h: dense_route), through the
diagnostic entry gpc_test_dense_route: every edge of the rule at num_cus = 256, no GPU.  The expected names restate the rule as
dense_dispatch, dense_w1_takes, big_shape, the nt_max ladder and w1_npad held it before they became one function; the GPU suite
(test_dense_gpu.py: test_dense_route_is_what_launches) ties the function to what actually launches."""
import pytest

SWITCHES = ("GPC_FORCE_GENERIC", "GPC_FORCE_BIG", "GPC_NO_W1", "GPC_NO_W1_512", "GPC_W2", "GPC_W1_MIN_P", "GPC_W1_SLOTS", "GPC_NO_SPLIT",
            "GPC_NO_NT17", "GPC_NO_HINT", "GPC_BIG_NO_W2", "GPC_BIG_NO_W4", "GPC_VAR_W4", "GPC_HOST_NO_PIPELINE", "GPC_HOST_ONE_STREAM")


@pytest.fixture(scope="module")
def capi():
    from gp_compressor_amd import build, capi as m
    build.build()
    m.load()
    return m


@pytest.fixture
def route(capi, monkeypatch):
    """route(switches, **facts) -> (kind, name, shape) with exactly `switches` set in the environment"""
    def ask(switches=(), **facts):
        for e in SWITCHES:
            monkeypatch.delenv(e, raising=False)
        for e in switches:
            k, _, v = e.partition("=")
            monkeypatch.setenv(k, v or "1")
        return capi.dense_route(**facts)
    return ask


RAGGED = dict(P=40, n_total=40 * 200)       # (any total below P * n_max: more than one size class)
VAR = dict(variance=True, pointwise=True)

# (switches, facts, kind, name, shape entries); depth plane, grid form, mean only unless the facts say otherwise
TABLE = [
    # the batch-size rule of the one-wave kernel: four patches per CU
    ((), dict(P=1024, n_max=256), "one-wave", "dense_mfma_w1", dict(w1_npad=256, w1_slots=8192)),
    ((), dict(P=1023, n_max=256), "register", "dense_mfma_nt16", dict(nt=16, export_factor=0)),
    (("GPC_W1_MIN_P=2",), dict(P=2, n_max=256), "one-wave", "dense_mfma_w1", {}),
    (("GPC_W1_MIN_P=0",), dict(P=1, n_max=256), "register", "dense_mfma_nt16", {}),
    (("GPC_W1_SLOTS=1000",), dict(P=4096, n_max=64), "one-wave", "dense_mfma_w1", dict(w1_slots=1000)),
    ((), dict(P=1024, n_max=256, ny=3), "register", "dense_mfma_nt16", {}),
    # the register kernel's tile counts
    ((), dict(P=40, n_max=64), "register", "dense_mfma_nt4", dict(nt=4)),
    ((), dict(P=40, n_max=65), "register", "dense_mfma_nt8", dict(nt=8)),
    ((), dict(P=40, n_max=128), "register", "dense_mfma_nt8", dict(nt=8)),
    ((), dict(P=40, n_max=129), "register", "dense_mfma_nt12", dict(nt=12)),
    ((), dict(P=40, n_max=192), "register", "dense_mfma_nt12", dict(nt=12)),
    ((), dict(P=40, n_max=193), "register", "dense_mfma_nt16", dict(nt=16)),
    ((), dict(P=40, n_max=256), "register", "dense_mfma_nt16", dict(nt=16)),
    ((), dict(P=40, n_max=0), "register", "dense_mfma_nt4", dict(nt=4)),
    # the variance: the register kernel's export up to 192 points, the one-wave kernel's slots for 193 .. 256 (point-wise X* only)
    ((), dict(P=1024, n_max=192, **VAR), "register", "dense_mfma_nt12 + dense_variance", dict(nt=12, export_factor=1)),
    ((), dict(P=1024, n_max=193, **VAR), "one-wave", "dense_mfma_w1 + dense_variance", dict(w1_npad=256)),
    ((), dict(P=1024, n_max=256, **VAR), "one-wave", "dense_mfma_w1 + dense_variance", {}),
    ((), dict(P=1024, n_max=257, **VAR), "tiled", "dense_mfma_big + dense_variance_big", dict(waves=4, npad=512)),
    ((), dict(P=1024, n_max=256, variance=True, pointwise=False), "register", "dense_mfma_nt16 + dense_variance", {}),
    ((), dict(P=40, n_max=600, n_total=40 * 500, **VAR), "tiled", "dense_mfma_big + dense_variance_big", dict(waves=8, npad=1024, per_cu=1)),
    ((), dict(P=40, n_max=600, n_total=40 * 500, variance=True, pointwise=False), "generic", "dense_generic", {}),
    # 257 .. 512 points: the one-wave kernel's 512-point instance, the tiled kernel's shapes behind it
    ((), dict(P=2000, n_max=512), "one-wave", "dense_mfma_w1_512", dict(w1_npad=512)),
    ((), dict(P=2000, n_max=513), "tiled", "dense_mfma_big", dict(waves=8, npad=1024, per_cu=1)),
    (("GPC_NO_W1_512",), dict(P=2000, n_max=512), "tiled", "dense_mfma_big", dict(waves=4, npad=512, per_cu=2)),
    (("GPC_NO_W1_512",), dict(P=2000, n_max=256), "one-wave", "dense_mfma_w1", {}),
    (("GPC_NO_W1_512", "GPC_BIG_NO_W4"), dict(P=2000, n_max=512), "tiled", "dense_mfma_big", dict(waves=8, npad=1024, per_cu=1)),
    ((), dict(P=2000, n_max=512, ny=3), "tiled", "dense_mfma_big", dict(waves=8, npad=1024, per_cu=1)),
    # ragged batches beyond 256 points: the size classes
    ((), dict(n_max=270, **RAGGED), "split", "dense_mfma_nt16 + dense_mfma_nt17", dict(nt17=1, need_big=0)),
    ((), dict(n_max=272, **RAGGED), "split", "dense_mfma_nt16 + dense_mfma_nt17", dict(nt17=1, need_big=0)),
    ((), dict(n_max=273, **RAGGED), "split", "dense_mfma_nt16 + dense_mfma_nt17 + dense_mfma_big", dict(nt17=1, need_big=1)),
    ((), dict(n_max=300, **RAGGED), "split", "dense_mfma_nt16 + dense_mfma_nt17 + dense_mfma_big",
     dict(nt17=1, need_big=1, waves=4, npad=512, per_cu=2)),
    (("GPC_NO_NT17",), dict(n_max=300, **RAGGED), "split", "dense_mfma_nt16 + dense_mfma_big", dict(nt17=0, need_big=1)),
    (("GPC_NO_NT17",), dict(n_max=270, **RAGGED), "split", "dense_mfma_nt16 + dense_mfma_big", dict(nt17=0, need_big=1)),
    ((), dict(n_max=300, ny=3, **RAGGED), "split", "dense_mfma_nt16 + dense_mfma_big", dict(nt17=0, need_big=1, waves=8, npad=1024)),
    ((), dict(n_max=1024, **RAGGED), "split", "dense_mfma_nt16 + dense_mfma_nt17 + dense_mfma_big", dict(waves=8, npad=1024)),
    ((), dict(P=40, n_max=270), "split", "dense_mfma_nt16 + dense_mfma_nt17", {}),      # uniform, but within the register classes
    ((), dict(P=40, n_max=300), "tiled", "dense_mfma_big", dict(waves=4, npad=512)),    # uniform: one class, known on the host
    ((), dict(P=1, n_max=270), "register", "dense_mfma_nt17", dict(nt=17)),
    ((), dict(P=1, n_max=270, ny=3), "tiled", "dense_mfma_big", dict(waves=8)),
    ((), dict(P=1, n_max=273), "tiled", "dense_mfma_big", dict(waves=4, npad=512)),
    (("GPC_NO_SPLIT",), dict(n_max=300, **RAGGED), "tiled", "dense_mfma_big", dict(waves=4, npad=512)),
    (("GPC_NO_SPLIT",), dict(n_max=270, **RAGGED), "register", "dense_mfma_nt17", dict(nt=17)),
    (("GPC_NO_SPLIT", "GPC_NO_NT17"), dict(n_max=270, **RAGGED), "tiled", "dense_mfma_big", {}),
    ((), dict(n_max=300, **RAGGED, **VAR), "tiled", "dense_mfma_big + dense_variance_big", {}),
    # the diagnostic switches
    (("GPC_FORCE_GENERIC",), dict(P=1024, n_max=256), "generic", "dense_generic", {}),
    (("GPC_FORCE_GENERIC", "GPC_FORCE_BIG"), dict(P=40, n_max=300), "generic", "dense_generic", {}),
    (("GPC_FORCE_BIG",), dict(P=1024, n_max=200), "tiled", "dense_mfma_big_w2", dict(waves=2, npad=256, per_cu=4)),
    (("GPC_FORCE_BIG", "GPC_BIG_NO_W2"), dict(P=1024, n_max=200), "tiled", "dense_mfma_big_w4", dict(waves=4, npad=256, per_cu=2)),
    (("GPC_FORCE_BIG",), dict(P=40, n_max=200, ny=3), "tiled", "dense_mfma_big_w4", dict(waves=4, npad=256, per_cu=2)),
    (("GPC_FORCE_BIG",), dict(P=40, n_max=200, **VAR), "generic", "dense_generic", {}),
    (("GPC_FORCE_BIG",), dict(n_max=300, **RAGGED), "tiled", "dense_mfma_big", {}),
    (("GPC_NO_W1",), dict(P=1024, n_max=256), "register", "dense_mfma_nt16", {}),
    (("GPC_NO_W1", "GPC_W2"), dict(P=1024, n_max=192), "register", "dense_mfma_nt12", {}),
    (("GPC_NO_W1", "GPC_W2"), dict(P=1024, n_max=193), "tiled", "dense_mfma_big_w2", dict(waves=2, npad=256, per_cu=4)),
    (("GPC_NO_W1", "GPC_W2"), dict(P=1024, n_max=257, n_total=1024 * 200), "split", "dense_mfma_nt16 + dense_mfma_nt17", {}),
    (("GPC_NO_W1", "GPC_W2"), dict(P=1, n_max=200), "register", "dense_mfma_nt16", {}),
    (("GPC_W2",), dict(P=1024, n_max=200), "one-wave", "dense_mfma_w1", {}),
    # the IRLS entry: always the tiled kernel
    ((), dict(P=40, n_max=256, irls=True), "tiled", "dense_mfma_big_w4_irls", dict(waves=4, npad=256)),
    ((), dict(P=4096, n_max=17, irls=True, m=0), "tiled", "dense_mfma_big_w4_irls", dict(waves=4, npad=256)),
    ((), dict(P=40, n_max=257, irls=True), "tiled", "dense_mfma_big_irls", dict(waves=8, npad=1024)),
    ((), dict(P=40, n_max=1024, irls=True), "tiled", "dense_mfma_big_irls", dict(waves=8, npad=1024, per_cu=1)),
    (("GPC_FORCE_GENERIC",), dict(P=40, n_max=1024, irls=True), "tiled", "dense_mfma_big_irls", {}),
    # the one-wave kernel's workspace refused: the route the batch would have had without that kernel -- none with the variance
    ((), dict(P=1024, n_max=256, w1_refused=True), "register", "dense_mfma_nt16", dict(nt=16)),
    ((), dict(P=1024, n_max=100, w1_refused=True), "register", "dense_mfma_nt8", dict(nt=8)),
    ((), dict(P=2000, n_max=512, w1_refused=True), "tiled", "dense_mfma_big", dict(waves=4, npad=512)),
    ((), dict(P=2000, n_max=400, n_total=2000 * 300, w1_refused=True), "split", "dense_mfma_nt16 + dense_mfma_nt17 + dense_mfma_big", {}),
    ((), dict(P=1024, n_max=256, w1_refused=True, **VAR), "no route", "", {}),
    ((), dict(P=1023, n_max=256, w1_refused=True, **VAR), "register", "dense_mfma_nt16 + dense_variance", {}),   # (never asked there)
    # nothing to do
    ((), dict(P=0, n_max=256), "nothing", "", {}),
    ((), dict(P=0, n_max=256, irls=True), "nothing", "", {}),
    ((), dict(P=1024, n_max=256, m=0), "nothing", "", {}),
    ((), dict(P=1024, n_max=256, m=0, alpha_out=True), "one-wave", "dense_mfma_w1", {}),
]


@pytest.mark.parametrize("switches,facts,kind,name,shape", TABLE,
                         ids=[" ".join(s) + (" " if s else "") + ",".join(f"{k}={int(v)}" for k, v in f.items()) for s, f, _, _, _ in TABLE])
def test_dense_route_table(route, switches, facts, kind, name, shape):
    got_kind, got_name, got_shape = route(switches, **facts)
    assert (got_kind, got_name) == (kind, name)
    assert {k: got_shape[k] for k in shape} == shape


def test_one_wave_kernel_never_takes_a_single_patch(route):
    for n in (1, 64, 200, 256, 300, 512):
        for sw in ((), ("GPC_W1_MIN_P=0",), ("GPC_W1_MIN_P=1",)):
            assert route(sw, P=1, n_max=n)[0] != "one-wave", (n, sw)


def test_batch_size_rule_follows_the_cu_count(route):
    for cus in (64, 104, 256, 304):
        assert route((), P=4 * cus, n_max=256, num_cus=cus)[1] == "dense_mfma_w1"
        assert route((), P=4 * cus - 1, n_max=256, num_cus=cus)[1] == "dense_mfma_nt16"


def test_irls_grid_keeps_the_plain_shapes_workgroups_per_cu(route):
    """The IRLS instances' grid is sized with what the plain tiled shape of the same batch holds per CU (the patches are handed out by
    ticket: it only decides how many workgroups queue) -- as the IRLS entry always reserved and launched."""
    for sw, n, per_cu in (((), 256, 4), (("GPC_BIG_NO_W2",), 256, 2), ((), 512, 2), (("GPC_BIG_NO_W4",), 512, 1), ((), 1024, 1)):
        assert route(sw, P=40, n_max=n, irls=True)[2]["per_cu"] == per_cu, (sw, n)


def test_switches_are_read_per_call(route):
    assert route(("GPC_FORCE_GENERIC",), P=1024, n_max=256)[1] == "dense_generic"
    assert route((), P=1024, n_max=256)[1] == "dense_mfma_w1"
