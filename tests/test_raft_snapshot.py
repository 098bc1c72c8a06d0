"""smr_raft_save_state / smr_raft_load_state and their cluster forms on the emulator build of the engine (tests/hostsim): the
shipped kernels and C-ABI, every lane a fiber, against the CPU oracle.  The bodies are tests/raft_snapshot_cases.py; the device
runs the same ones in tests/test_zzzz_raft_snapshot_gpu.py."""
import pytest


@pytest.fixture(scope="module")
def sim():
    import hostsim
    hostsim.build()
    return hostsim


def test_symbols_are_exported_and_bound(sim):
    import summerset_amd
    from summerset_amd import _lib
    names = {n for n, _, _ in _lib.SYMBOLS}
    lib = sim.load()
    for n in ("smr_raft_snapshot_create", "smr_raft_snapshot_destroy", "smr_raft_save_state", "smr_raft_load_state", "smr_raft_snapshot_info_get",
              "smr_raft_snapshot_export", "smr_raft_snapshot_import", "smr_raft_cluster_save_state", "smr_raft_cluster_load_state"):
        assert n in names and getattr(lib, n)
    for n in ("RaftSnapshot", "save_cluster_state", "load_cluster_state"):
        assert hasattr(summerset_amd, n)


@pytest.mark.parametrize("arm,G,W,T", [("tick", 520, 8, 36), ("calls", 130, 16, 44), ("many", 130, 8, 36)])
def test_shadow_at_every_boundary(sim, oracle, arm, G, W, T):
    """520 groups are nine tiles, three blocks of the snapshot kernels (the last one mostly idle): the record offsets across tiles
    and across blocks; 130 groups three tiles of one block.  Windows 8 and 16 and logs past 80: the rings wrap several times."""
    import raft_snapshot_cases as c
    with sim.patched():
        cov = c.shadow_cluster("cpu", oracle, G=G, R=5, W=W, K=8, T=T, make_schedule=c.ring_schedule(5, G, W, 43, loss=0.05 if arm == "calls" else 0.0),
                               arm=arm, need=c.FULL_COVERAGE)
    assert cov["max_len"] > 2 * W


@pytest.mark.parametrize("arm,R,G", [("calls", 3, 65), ("tick", 3, 65), ("calls", 7, 63), ("tick", 8, 64), ("tick", 5, 1)])
def test_shadow_other_shapes(sim, oracle, arm, R, G):
    """(the device file runs the same parameters; one group meets no losing candidate, no log of one entry at a boundary and no
    conflict reply in this schedule, so those three are not asked of it)"""
    import raft_snapshot_cases as c
    need = [n for n in c.FULL_COVERAGE if G > 1 or n not in ("candidate_with_votes", "one_entry", "conflicts")]
    with sim.patched():
        c.shadow_cluster("cpu", oracle, G=G, R=R, W=8, K=8, T=36, make_schedule=c.ring_schedule(R, G, 8, 43), arm=arm, need=need)


def test_shadow_commit_extra_cluster_form_by_calls(sim, oracle):
    import raft_snapshot_cases as c
    with sim.patched():
        c.shadow_cluster("cpu", oracle, G=70, R=5, W=64, K=4, T=14, make_schedule=c.ring_schedule(5, 70, 64, 47, n_new_max=3), arm="calls",
                         need=("elected", "one_entry", "voted_for"), commit_extra=1, cluster_form=True)


def test_restart_of_one_replica(sim, oracle):
    import raft_snapshot_cases as c
    with sim.patched():
        st = c.restart_one_replica("cpu", oracle)
    assert st["stepped"] > 0 and st["caught_up_at"] is not None


def test_canonical_bytes(sim, oracle):
    import raft_snapshot_cases as c
    with sim.patched():
        assert c.canonical_bytes("cpu", oracle) == 15
        c.canonical_bytes_run_ticks("cpu", oracle)


def test_resize(sim, oracle):
    import raft_snapshot_cases as c
    with sim.patched():
        c.resize("cpu", oracle)


def test_craft_shadow_at_every_step(sim, oracle):
    """330 groups: six tiles, two blocks of the snapshot kernels -- the Reconstruct queue's offsets across blocks"""
    import raft_snapshot_cases as c
    with sim.patched():
        c.craft_shadow("cpu", oracle, G=330)
        c.craft_shadow("cpu", oracle, G=65, W=64, me=4, ft=2, thr=3, seed=85)


def test_save_is_stream_ordered(sim, oracle):
    import raft_snapshot_cases as c
    with sim.patched():
        c.stream_order("cpu", oracle)


def test_cluster_form(sim, oracle):
    import raft_snapshot_cases as c
    with sim.patched():
        c.cluster_form("cpu", oracle)
        c.cluster_form("cpu", oracle, G=64, R=8, seed=99)


def test_cluster_form_craft(sim, oracle):
    """330 groups: two blocks per replica"""
    import raft_snapshot_cases as c
    with sim.patched():
        c.craft_cluster_form("cpu", oracle, G=330)


def test_refusals(sim, oracle):
    import raft_snapshot_cases as c
    with sim.patched():
        c.refusals("cpu", oracle)


def test_snapshot_grows_for_a_larger_window(sim, oracle):
    import raft_snapshot_cases as c
    with sim.patched():
        c.grows_for_a_larger_window("cpu", oracle)


def test_hand_built_image_into_a_smaller_window(sim):
    import raft_snapshot_cases as c
    with sim.patched():
        c.hand_built_image("cpu")
