"""smr_ep_*_groups and smr_ep_cluster_*_groups on the device: the bodies of tests/ep_move_groups_cases.py (which the emulator runs
in tests/test_ep_move_groups.py), against the CPU oracle."""
import pytest

pytestmark = pytest.mark.gpu


def test_symbols_are_exported_and_bound(cuda):
    import ep_move_groups_cases as c
    from summerset_amd import _lib
    c.symbols(_lib.load())


@pytest.mark.parametrize("cluster", [False, True])
def test_a_group_image_is_a_selection_of_the_whole_image(cuda, oracle, cluster):
    """G = 130, R = 5, W = 8, K = 3, loss 0.2; lists of 1, 63, 64, 65 and 130 at two boundaries and at the end"""
    import ep_move_groups_cases as c
    c.selection_of_the_whole_image(cuda, oracle, cluster)


@pytest.mark.parametrize("R,K,seated,recovery,cluster", [(3, 3, False, False, False), (5, 3, True, False, True), (8, 4, False, False, True),
                                                         (4, 3, False, True, True)])
def test_a_move_changes_object_and_position(cuda, oracle, R, K, seated, recovery, cluster):
    import ep_move_groups_cases as c
    c.move_between_shards(cuda, oracle, R=R, K=K, seated=seated, recovery=recovery, cluster=cluster)


def test_interchange(cuda, oracle):
    import ep_move_groups_cases as c
    c.interchange(cuda, oracle)


def test_stored_replies_survive_a_move(cuda, oracle):
    import ep_move_groups_cases as c
    assert c.stored_replies_survive(cuda, oracle) > 0


def test_neighbours_untouched_reset_is_create(cuda, oracle):
    """what the dumps cannot show: the replica's raw bytes around a load and a reset through a list"""
    import ep_move_groups_cases as c
    c.neighbours_untouched(cuda, oracle)


def test_a_reset_slot_runs_from_scratch(cuda, oracle):
    import ep_move_groups_cases as c
    c.reset_then_run_from_scratch(cuda, oracle)


def test_list_shapes(cuda, oracle):
    import ep_move_groups_cases as c
    c.list_shapes(cuda, oracle)


def test_list_shapes_permutation_of_a_66000_group_replica(cuda):
    """1 032 tiles for the launch's 1 024 wavefronts, every access of the replica side a gather"""
    import ep_move_groups_cases as c
    c.permutation_of_a_large_replica(cuda)


def test_cluster_form_is_the_single_calls(cuda, oracle):
    import ep_move_groups_cases as c
    c.cluster_form(cuda, oracle)


def test_refusals(cuda, oracle):
    import ep_move_groups_cases as c
    c.refusals(cuda, oracle)


def test_stream_order(cuda, oracle):
    import ep_move_groups_cases as c
    c.stream_order(cuda, oracle)
