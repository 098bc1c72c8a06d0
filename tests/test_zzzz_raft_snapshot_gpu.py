"""smr_raft_save_state / smr_raft_load_state and their cluster forms on the device: the bodies of tests/raft_snapshot_cases.py
(which the emulator runs in tests/test_raft_snapshot.py) at the shapes the Raft device tests use, against the CPU oracle."""
import pytest

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("arm", ["calls", "tick", "many"])
def test_shadow_at_every_boundary(cuda, oracle, arm):
    import raft_snapshot_cases as c
    cov = c.shadow_cluster(cuda, oracle, G=600, R=5, W=16, K=8, T=44, make_schedule=c.ring_schedule(5, 600, 16, 43, loss=0.05 if arm == "calls" else 0.0),
                           arm=arm, need=c.FULL_COVERAGE)
    assert cov["max_len"] > 2 * 16


@pytest.mark.parametrize("arm,R,G", [("calls", 3, 65), ("tick", 3, 65), ("calls", 7, 63), ("tick", 8, 64), ("tick", 5, 1)])
def test_shadow_other_shapes(cuda, oracle, arm, R, G):
    """(the parameters of the emulator file's test of this name, see there)"""
    import raft_snapshot_cases as c
    need = [n for n in c.FULL_COVERAGE if G > 1 or n not in ("candidate_with_votes", "one_entry", "conflicts")]
    c.shadow_cluster(cuda, oracle, G=G, R=R, W=8, K=8, T=36, make_schedule=c.ring_schedule(R, G, 8, 43), arm=arm, need=need)


def test_shadow_window_8_and_commit_extra(cuda, oracle):
    import raft_snapshot_cases as c
    c.shadow_cluster(cuda, oracle, G=130, R=5, W=8, K=8, T=36, make_schedule=c.ring_schedule(5, 130, 8, 43), arm="tick", need=c.FULL_COVERAGE)
    c.shadow_cluster(cuda, oracle, G=70, R=5, W=64, K=4, T=14, make_schedule=c.ring_schedule(5, 70, 64, 47, n_new_max=3), arm="calls",
                     need=("elected", "one_entry", "voted_for"), commit_extra=1, cluster_form=True)


def test_shadow_more_tiles_than_a_block(cuda, oracle):
    """4 100 groups: 65 tiles, 17 blocks of the snapshot kernels per replica, the last one partly idle -- the offsets across blocks"""
    import raft_snapshot_cases as c
    c.shadow_cluster(cuda, oracle, G=4100, R=5, W=16, K=8, T=30, make_schedule=c.ring_schedule(5, 4100, 16, 43), arm="tick",
                     need=("past_ring", "n_trunc", "elected", "conflicts", "one_entry"))


def test_shadow_more_tiles_than_wavefronts(cuda, oracle):
    """66 000 groups: 1 032 tiles for the launch's 1 024 wavefronts a replica, two tiles each -- a wavefront's own prefix inside its block"""
    import raft_snapshot_cases as c
    c.shadow_cluster(cuda, oracle, G=66000, R=3, W=8, K=4, T=8, make_schedule=c.ring_schedule(3, 66000, 8, 43), arm="tick",
                     need=("past_ring", "elected", "one_entry", "voted_for"))


def test_restart_of_one_replica(cuda, oracle):
    import raft_snapshot_cases as c
    st = c.restart_one_replica(cuda, oracle, G=300)
    assert st["stepped"] > 0 and st["caught_up_at"] is not None


def test_canonical_bytes(cuda, oracle):
    import raft_snapshot_cases as c
    assert c.canonical_bytes(cuda, oracle, G=300) == 15
    c.canonical_bytes_run_ticks(cuda, oracle, G=700)


def test_resize(cuda, oracle):
    import raft_snapshot_cases as c
    c.resize(cuda, oracle, G=256)


def test_craft_shadow_at_every_step(cuda, oracle):
    import raft_snapshot_cases as c
    c.craft_shadow(cuda, oracle, G=777)
    c.craft_shadow(cuda, oracle, G=65, W=64, me=4, ft=2, thr=3, seed=85)


def test_save_is_stream_ordered(cuda, oracle):
    import raft_snapshot_cases as c
    c.stream_order(cuda, oracle, G=4100)


def test_cluster_form(cuda, oracle):
    import raft_snapshot_cases as c
    c.cluster_form(cuda, oracle, G=300)
    c.cluster_form(cuda, oracle, G=64, R=8, seed=99)


def test_cluster_form_craft(cuda, oracle):
    import raft_snapshot_cases as c
    c.craft_cluster_form(cuda, oracle, G=777)


def test_refusals(cuda, oracle):
    import raft_snapshot_cases as c
    c.refusals(cuda, oracle)


def test_snapshot_grows_for_a_larger_window(cuda, oracle):
    import raft_snapshot_cases as c
    c.grows_for_a_larger_window(cuda, oracle)


def test_hand_built_image_into_a_smaller_window(cuda):
    import raft_snapshot_cases as c
    c.hand_built_image(cuda)
