"""smr_rsp_*_groups, smr_rsp_cluster_*_groups and smr_rsp_pstore_*_groups on the device: the bodies of
tests/rsp_move_groups_cases.py (which the emulator runs in tests/test_rsp_move_groups.py), against the CPU oracle."""
import pytest

pytestmark = pytest.mark.gpu


def test_symbols_are_exported_and_bound(cuda):
    import rsp_move_groups_cases as c
    from summerset_amd import _lib
    c.symbols(_lib.load())


@pytest.mark.parametrize("cluster", [False, True])
def test_identity_at_every_boundary(cuda, oracle, cluster):
    """shadow_stores' cluster and schedule: R = 5, G = 130, W = 8, L = 61, loss 0.1; lists of 1, 63, 64, 65 and 130"""
    import rsp_move_groups_cases as c
    c.identity_at_every_boundary(cuda, oracle, cluster)


@pytest.mark.parametrize("cluster", [False, True])
def test_a_move_changes_object_and_position(cuda, oracle, cluster):
    import rsp_move_groups_cases as c
    c.move_between_shards(cuda, oracle, cluster)


def test_interchange_replica(cuda, oracle):
    import rsp_move_groups_cases as c
    c.interchange_replica(cuda, oracle)


def test_interchange_store_canonical_bytes(cuda, oracle):
    import rsp_move_groups_cases as c
    c.interchange_store(cuda, oracle)


def test_interchange_store_voted_plane(cuda, oracle):
    import rsp_move_groups_cases as c
    c.interchange_voted_plane(cuda, oracle)


def test_interchange_craft_store(cuda, oracle):
    """the one-plane image: no alias section, craft = 1"""
    import rsp_move_groups_cases as c
    c.interchange_craft_store(cuda, oracle)


def test_ring_cells_outside_the_live_span(cuda, oracle):
    """what the dump cannot show: the replica's raw bytes around a load and a reset through a list"""
    import rsp_move_groups_cases as c
    c.ring_cells_outside_the_live_span(cuda, oracle)


def test_neighbours_untouched_store(cuda, oracle):
    import rsp_move_groups_cases as c
    c.neighbours_untouched_store(cuda, oracle)


def test_neighbours_untouched_replica(cuda, oracle):
    import rsp_move_groups_cases as c
    c.neighbours_untouched_replica(cuda, oracle)


def test_reset_is_create_and_runs_from_scratch(cuda, oracle):
    import rsp_move_groups_cases as c
    c.reset_then_run_from_scratch(cuda, oracle)


def test_list_shapes(cuda, oracle):
    import rsp_move_groups_cases as c
    c.list_shapes(cuda, oracle)


def test_list_shapes_permutation_of_a_66000_group_replica(cuda):
    """1 032 tiles for the launch's 1 024 wavefronts, every row of the replica side a gather"""
    import rsp_move_groups_cases as c
    c.permutation_of_a_large_replica(cuda)


def test_list_shapes_permutation_of_a_66000_group_store(cuda, oracle):
    import rsp_move_groups_cases as c
    c.permutation_of_a_large_store(cuda, oracle)


def test_store_groups_past_4gib(cuda, oracle):
    import rsp_move_groups_cases as c
    c.store_groups_past_4gib(cuda, oracle)


def test_craft_store_moves_with_its_groups(cuda, oracle):
    import rsp_move_groups_cases as c
    c.craft_move(cuda, oracle, R=5)


def test_cluster_form_is_the_single_calls(cuda, oracle):
    import rsp_move_groups_cases as c
    c.cluster_form(cuda, oracle)


def test_refusals(cuda, oracle):
    import rsp_move_groups_cases as c
    c.refusals(cuda, oracle)


def test_stream_order(cuda, oracle):
    import rsp_move_groups_cases as c
    c.stream_order(cuda, oracle)
