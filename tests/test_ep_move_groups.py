"""smr_ep_*_groups and smr_ep_cluster_*_groups on the emulator build of the engine (tests/hostsim): the shipped kernels and C-ABI,
every lane a fiber, against the CPU oracle.  The bodies are tests/ep_move_groups_cases.py; the device runs the same ones, at the
full shapes, in tests/test_zzzz_ep_move_groups_gpu.py.  (Here a case that does not need five replicas runs three, and the finished
clusters have 65 or 130 groups, as in tests/test_ep_snapshot.py.)"""
import pytest


@pytest.fixture(scope="module")
def sim():
    import hostsim
    hostsim.build()
    return hostsim


def test_symbols_are_exported_and_bound(sim):
    import ep_move_groups_cases as c
    c.symbols(sim.load())


@pytest.mark.parametrize("cluster", [False, True])
def test_a_group_image_is_a_selection_of_the_whole_image(sim, oracle, cluster):
    """65 groups: the 64 / 65 wavefront edge; lists of 1, 63, 64 and 65"""
    import ep_move_groups_cases as c
    with sim.patched():
        c.selection_of_the_whole_image("cpu", oracle, cluster, G=65, R=5, sizes=(1, 63, 64, 65))


@pytest.mark.parametrize("R,K,seated,recovery,cluster", [(3, 3, False, False, False), (5, 3, True, False, True), (8, 4, False, False, True),
                                                         (4, 3, False, True, True)])
def test_a_move_changes_object_and_position(sim, oracle, R, K, seated, recovery, cluster):
    import ep_move_groups_cases as c
    with sim.patched():
        c.move_between_shards("cpu", oracle, R=R, K=K, seated=seated, recovery=recovery, cluster=cluster)


def test_interchange(sim, oracle):
    import ep_move_groups_cases as c
    with sim.patched():
        c.interchange("cpu", oracle, G=130, R=3, n=65)


def test_stored_replies_survive_a_move(sim, oracle):
    import ep_move_groups_cases as c
    with sim.patched():
        assert c.stored_replies_survive("cpu", oracle) > 0


def test_neighbours_untouched_reset_is_create(sim, oracle):
    """what the dumps cannot show: the replica's raw bytes around a load and a reset through a list"""
    import ep_move_groups_cases as c
    with sim.patched():
        c.neighbours_untouched("cpu", oracle, G=130, R=3, k=37)


def test_a_reset_slot_runs_from_scratch(sim, oracle):
    import ep_move_groups_cases as c
    with sim.patched():
        c.reset_then_run_from_scratch("cpu", oracle)


def test_list_shapes(sim, oracle):
    """330 list entries: six tiles, two blocks of the group kernels"""
    import ep_move_groups_cases as c
    with sim.patched():
        c.list_shapes("cpu", oracle)


def test_cluster_form_is_the_single_calls(sim, oracle):
    import ep_move_groups_cases as c
    with sim.patched():
        c.cluster_form("cpu", oracle, G=130, R=3)


def test_refusals(sim, oracle):
    import ep_move_groups_cases as c
    with sim.patched():
        c.refusals("cpu", oracle)


def test_stream_order(sim, oracle):
    import ep_move_groups_cases as c
    with sim.patched():
        c.stream_order("cpu", oracle)
