"""smr_rsp_*_groups, smr_rsp_cluster_*_groups and smr_rsp_pstore_*_groups on the emulator build of the engine (tests/hostsim): the
shipped kernels and C-ABI, every lane a fiber, against the CPU oracle.  The bodies are tests/rsp_move_groups_cases.py; the device
runs the same ones, at the full shapes, in tests/test_zzzz_rsp_move_groups_gpu.py.  (The emulator runs every lane of the byte
kernels as a fiber, so the clusters here are the smaller ones tests/test_rsp_snapshot.py uses for the stores.)"""
import pytest


@pytest.fixture(scope="module")
def sim():
    import hostsim
    hostsim.build()
    return hostsim


SMALL = dict(G=40, R=3, ft=1, L=61)


def test_symbols_are_exported_and_bound(sim):
    import rsp_move_groups_cases as c
    c.symbols(sim.load())


@pytest.mark.parametrize("cluster", [False, True])
def test_identity_at_every_boundary(sim, oracle, cluster):
    import rsp_move_groups_cases as c
    with sim.patched():
        c.identity_at_every_boundary("cpu", oracle, cluster, sizes=(1, 33, 40, 7, 39), **SMALL)


@pytest.mark.parametrize("cluster", [False, True])
def test_a_move_changes_object_and_position(sim, oracle, cluster):
    import rsp_move_groups_cases as c
    with sim.patched():
        c.move_between_shards("cpu", oracle, cluster)


def test_interchange_replica(sim, oracle):
    import rsp_move_groups_cases as c
    with sim.patched():
        c.interchange_replica("cpu", oracle, n=33, **SMALL)


def test_interchange_store_canonical_bytes(sim, oracle):
    import rsp_move_groups_cases as c
    with sim.patched():
        c.interchange_store("cpu", oracle, G=70, k=37)


def test_interchange_store_voted_plane(sim, oracle):
    import rsp_move_groups_cases as c
    with sim.patched():
        c.interchange_voted_plane("cpu", oracle, n=33, **SMALL)


def test_interchange_craft_store(sim, oracle):
    """the one-plane image: no alias section, craft = 1"""
    import rsp_move_groups_cases as c
    with sim.patched():
        c.interchange_craft_store("cpu", oracle, R=3)


def test_ring_cells_outside_the_live_span(sim, oracle):
    """what the dump cannot show: the replica's raw bytes around a load and a reset through a list"""
    import rsp_move_groups_cases as c
    with sim.patched():
        c.ring_cells_outside_the_live_span("cpu", oracle, k=17, **SMALL)


def test_neighbours_untouched_store(sim, oracle):
    import rsp_move_groups_cases as c
    with sim.patched():
        c.neighbours_untouched_store("cpu", oracle)


def test_neighbours_untouched_replica(sim, oracle):
    import rsp_move_groups_cases as c
    with sim.patched():
        c.neighbours_untouched_replica("cpu", oracle, k=17, **SMALL)


def test_reset_is_create_and_runs_from_scratch(sim, oracle):
    import rsp_move_groups_cases as c
    with sim.patched():
        c.reset_then_run_from_scratch("cpu", oracle)


def test_list_shapes(sim, oracle):
    """330 list entries: six tiles, two blocks of the group kernels"""
    import rsp_move_groups_cases as c
    with sim.patched():
        c.list_shapes("cpu", oracle)


def test_craft_store_moves_with_its_groups(sim, oracle):
    import rsp_move_groups_cases as c
    with sim.patched():
        c.craft_move("cpu", oracle, R=3)


def test_cluster_form_is_the_single_calls(sim, oracle):
    import rsp_move_groups_cases as c
    with sim.patched():
        c.cluster_form("cpu", oracle, n=33, **SMALL)


def test_refusals(sim, oracle):
    import rsp_move_groups_cases as c
    with sim.patched():
        c.refusals("cpu", oracle, **SMALL)


def test_stream_order(sim, oracle):
    import rsp_move_groups_cases as c
    with sim.patched():
        c.stream_order("cpu", oracle, L=61)
