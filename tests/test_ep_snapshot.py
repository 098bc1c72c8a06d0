"""smr_ep_save_state / smr_ep_load_state and their cluster forms on the emulator build of the engine (tests/hostsim): the shipped
kernels and C-ABI, every lane a fiber, against the CPU oracle.  The bodies are tests/ep_snapshot_cases.py; the device runs the
same ones in tests/test_zzzz_ep_snapshot_gpu.py."""
import pytest

NAMES = ("smr_ep_snapshot_create", "smr_ep_snapshot_destroy", "smr_ep_save_state", "smr_ep_load_state", "smr_ep_snapshot_info_get",
         "smr_ep_snapshot_export", "smr_ep_snapshot_import", "smr_ep_cluster_save_state", "smr_ep_cluster_load_state",
         "smr_ep_debug_arena_view")
# groups, population, keys, save / load as one launch, seated in an smr_ep_cluster and ticked by it, recovery
SHAPES = [(520, 3, 2, True, False, False), (130, 5, 3, False, True, False), (65, 8, 4, True, False, False), (65, 4, 3, False, False, True)]


@pytest.fixture(scope="module")
def sim():
    import hostsim
    hostsim.build()
    return hostsim


def test_symbols_are_exported_and_bound(sim):
    import summerset_amd
    from summerset_amd import _lib, epaxos
    names = {n for n, _, _ in _lib.SYMBOLS}
    lib = sim.load()
    for n in NAMES:
        assert n in names and getattr(lib, n)
    assert hasattr(summerset_amd, "EPaxosSnapshot")
    for n in ("EPaxosSnapshot", "save_cluster_state", "load_cluster_state"):
        assert hasattr(epaxos, n)
    for n in ("create_like", "save", "load", "info", "export", "import_"):
        assert hasattr(epaxos.EPaxosSnapshot, n)
    for n in ("save_state", "load_state"):
        assert hasattr(epaxos.EPaxosReplicaGroup, n)


@pytest.mark.parametrize("G,R,K,cluster_form,seated,recovery", SHAPES)
def test_shadow_at_every_boundary(sim, oracle, G, R, K, cluster_form, seated, recovery):
    """520 groups are nine tiles, three blocks of the snapshot kernels (the last one mostly idle); 130 groups three tiles of one
    block; 65 the 64 / 65 wavefront edge.  Window 8 and 20 ticks: every row wraps"""
    import ep_snapshot_cases as c
    with sim.patched():
        cov = c.shadow("cpu", oracle, G=G, R=R, K=K, cluster_form=cluster_form, seated=seated, recovery=recovery)
    assert cov["ticks"] == 20


def test_stored_replies_survive(sim, oracle):
    import ep_snapshot_cases as c
    with sim.patched():
        assert c.stored_replies_survive("cpu", oracle) > 0


def test_canonical_bytes(sim, oracle):
    import ep_snapshot_cases as c
    with sim.patched():
        c.canonical_bytes("cpu", oracle)


def test_hand_built_image(sim):
    import ep_snapshot_cases as c
    with sim.patched():
        c.hand_built_image("cpu")


def test_restart_of_one_replica(sim, oracle):
    import ep_snapshot_cases as c
    with sim.patched():
        c.restart_of_one_replica("cpu", oracle)


def test_save_is_stream_ordered(sim, oracle):
    import ep_snapshot_cases as c
    with sim.patched():
        c.stream_order("cpu", oracle)


def test_refusals(sim, oracle):
    import ep_snapshot_cases as c
    with sim.patched():
        c.refusals("cpu", oracle)


def test_snapshot_grows_for_a_larger_window(sim, oracle):
    import ep_snapshot_cases as c
    with sim.patched():
        c.grows_for_a_larger_window("cpu", oracle)


def test_abort_and_restore_in_l2(sim, oracle):
    """(two ranks in one process)"""
    import ep_snapshot_cases as c
    with sim.patched():
        c.abort_and_restore_l2("cpu", oracle, 2)
