"""smr_raft_save_groups / smr_raft_load_groups / smr_raft_reset_groups and their cluster forms on the device: the bodies of
tests/raft_move_groups_cases.py (which the emulator runs in tests/test_raft_move_groups.py), against the CPU oracle."""
import pytest

pytestmark = pytest.mark.gpu


def test_symbols_are_exported_and_bound(cuda):
    import raft_move_groups_cases as c
    from summerset_amd import _lib
    c.symbols(_lib.load())


@pytest.mark.parametrize("R,order,cluster", [(5, "calls", False), (5, "tick", True), (3, "tick", False), (3, "calls", True)])
def test_move_at_every_boundary(cuda, oracle, R, order, cluster):
    import raft_move_groups_cases as c
    c.move_at_every_boundary(cuda, oracle, R, order, cluster)


def test_list_shapes(cuda, oracle):
    import raft_move_groups_cases as c
    c.list_shapes(cuda, oracle)


def test_list_shapes_permutation_of_66000_groups(cuda):
    """1 032 tiles for the launch's 1 024 wavefronts, every row of the replica side a gather"""
    import raft_move_groups_cases as c
    c.permutation_of_a_large_replica(cuda)


def test_interchange_with_whole_replica_images(cuda, oracle):
    import raft_move_groups_cases as c
    c.interchange(cuda, oracle)


def test_other_window_wrapped_rings(cuda, oracle):
    import raft_move_groups_cases as c
    c.other_window(cuda, oracle)


def test_craft_queue_counters_masks_and_reset(cuda, oracle):
    import raft_move_groups_cases as c
    c.craft_moves(cuda, oracle)


def test_neighbours_untouched_and_reset(cuda, oracle):
    import raft_move_groups_cases as c
    c.neighbours_and_reset(cuda, oracle)


def test_cluster_form_is_the_single_calls(cuda, oracle):
    import raft_move_groups_cases as c
    c.cluster_form(cuda, oracle)


def test_refusals(cuda, oracle):
    import raft_move_groups_cases as c
    c.refusals(cuda, oracle)
