"""smr_raft_save_groups / smr_raft_load_groups / smr_raft_reset_groups and their cluster forms on the emulator build of the engine
(tests/hostsim): the shipped kernels and C-ABI, every lane a fiber, against the CPU oracle.  The bodies are
tests/raft_move_groups_cases.py; the device runs the same ones in tests/test_zzzz_raft_move_groups_gpu.py."""
import pytest


@pytest.fixture(scope="module")
def sim():
    import hostsim
    hostsim.build()
    return hostsim


def test_symbols_are_exported_and_bound(sim):
    import raft_move_groups_cases as c
    c.symbols(sim.load())


@pytest.mark.parametrize("R,order,cluster", [(5, "calls", False), (5, "tick", True), (3, "tick", False), (3, "calls", True)])
def test_move_at_every_boundary(sim, oracle, R, order, cluster):
    """through the single calls and through the cluster forms, in both tick orders"""
    import raft_move_groups_cases as c
    with sim.patched():
        c.move_at_every_boundary("cpu", oracle, R, order, cluster)


def test_list_shapes(sim, oracle):
    """330 list entries: six tiles, two blocks of the group kernels"""
    import raft_move_groups_cases as c
    with sim.patched():
        c.list_shapes("cpu", oracle)


def test_interchange_with_whole_replica_images(sim, oracle):
    import raft_move_groups_cases as c
    with sim.patched():
        c.interchange("cpu", oracle)


def test_other_window_wrapped_rings(sim, oracle):
    import raft_move_groups_cases as c
    with sim.patched():
        c.other_window("cpu", oracle)


def test_craft_queue_counters_masks_and_reset(sim, oracle):
    import raft_move_groups_cases as c
    with sim.patched():
        c.craft_moves("cpu", oracle)


def test_neighbours_untouched_and_reset(sim, oracle):
    import raft_move_groups_cases as c
    with sim.patched():
        c.neighbours_and_reset("cpu", oracle)


def test_cluster_form_is_the_single_calls(sim, oracle):
    import raft_move_groups_cases as c
    with sim.patched():
        c.cluster_form("cpu", oracle)


def test_refusals(sim, oracle):
    import raft_move_groups_cases as c
    with sim.patched():
        c.refusals("cpu", oracle)
