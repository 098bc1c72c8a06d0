"""smr_rsp_save_state / smr_rsp_load_state and their cluster forms on the device: the bodies of tests/rsp_snapshot_cases.py
(which the emulator runs in tests/test_rsp_snapshot.py), against the CPU oracle."""
import pytest

pytestmark = pytest.mark.gpu


def test_symbols_are_exported_and_bound(cuda):
    """(the `cuda` fixture first: torch brings its own HIP runtime, and the engine library must find that one already loaded, as
    in every other device test, also when this file runs alone)"""
    import test_rsp_snapshot as t
    from summerset_amd import _lib
    lib = _lib.load()
    for n in t.NAMES + t.PS_NAMES:
        assert getattr(lib, n)


@pytest.mark.parametrize("G,R,ft,cluster_form", [(520, 3, 1, True), (130, 5, 1, False), (65, 8, 2, True), (65, 3, 0, False)])
def test_shadow_at_every_boundary(cuda, oracle, G, R, ft, cluster_form):
    """(the parameters of the emulator file's test of this name, see there)"""
    import rsp_snapshot_cases as c
    c.shadow_replicas(cuda, oracle, G=G, R=R, ft=ft, cluster_form=cluster_form)


def test_shadow_one_group(cuda, oracle):
    import rsp_snapshot_cases as c
    c.shadow_replicas(cuda, oracle, G=1, R=3, ft=0, loss=0.0, rare=False)


def test_shadow_from_wide_ballots(cuda, oracle):
    import rsp_snapshot_cases as c
    c.shadow_replicas(cuda, oracle, G=130, R=3, ft=0, T=18, round0=2**24 - 2, cluster_form=True)


def test_shadow_more_tiles_than_a_block(cuda, oracle):
    """4 100 groups: 65 tiles, 17 blocks of the snapshot kernels per replica, the last one partly idle -- the offsets across blocks"""
    import rsp_snapshot_cases as c
    c.shadow_replicas(cuda, oracle, G=4100, R=3, ft=1, cluster_form=True)


def test_shadow_more_tiles_than_wavefronts(cuda, oracle):
    """66 000 groups: 1 032 tiles for the launch's 1 024 wavefronts a replica, two tiles each -- a wavefront's own prefix inside
    its block.  Eight ticks: the ring of 8 fills but does not wrap five times, so the schedule's own conditions are not asked"""
    import rsp_snapshot_cases as c
    c.shadow_replicas(cuda, oracle, G=66000, R=3, ft=0, T=8, rare=False, wrapped=False)


def test_canonical_bytes(cuda, oracle):
    import rsp_snapshot_cases as c
    c.canonical_bytes(cuda, oracle, G=300)


def test_restart_of_one_replica(cuda, oracle):
    import rsp_snapshot_cases as c
    st = c.restart_one_replica(cuda, oracle, G=300)
    assert st["stepped"] > 0 and st["caught_up_at"] is not None


def test_hand_built_image(cuda):
    import rsp_snapshot_cases as c
    c.hand_built_image(cuda)


def test_save_is_stream_ordered(cuda, oracle):
    import rsp_snapshot_cases as c
    c.stream_order(cuda, oracle, G=4100)


def test_refusals(cuda, oracle):
    import rsp_snapshot_cases as c
    c.refusals(cuda, oracle)


def test_snapshot_grows_for_a_larger_window(cuda, oracle):
    import rsp_snapshot_cases as c
    c.grows_for_a_larger_window(cuda, oracle)


# ---- the payload stores ----
@pytest.mark.parametrize("G,R,ft,L,staging", [(40, 3, 1, 61, False), (96, 5, 1, 333, False), (40, 8, 2, 61, True), (40, 5, 1, 4113, False), (40, 3, 0, 333, False)])
def test_store_shadow_at_every_boundary(cuda, oracle, G, R, ft, L, staging):
    """(every case's schedule must leave some vote stored on its own, which the body asserts from the stores: with five replicas
    and fault_tolerance 0 this schedule leaves none -- every vote stays an alias -- so the L = 4113 case runs at fault_tolerance 1)"""
    import rsp_snapshot_cases as c
    c.shadow_stores(cuda, oracle, G=G, R=R, ft=ft, L=L, staging=staging)


def test_store_canonical_bytes(cuda, oracle):
    import rsp_snapshot_cases as c
    c.store_canonical_bytes(cuda, oracle)


def test_hand_built_store_image(cuda):
    import rsp_snapshot_cases as c
    c.hand_built_store_image(cuda)


def test_store_save_is_stream_ordered(cuda, oracle):
    import rsp_snapshot_cases as c
    c.store_stream_order(cuda, oracle)


def test_store_refusals(cuda, oracle):
    import rsp_snapshot_cases as c
    c.store_refusals(cuda, oracle)


def test_store_snapshot_grows_for_longer_payloads(cuda, oracle):
    import rsp_snapshot_cases as c
    c.store_grows(cuda, oracle)


@pytest.mark.parametrize("R", [3, 5])
def test_craft_store_shadow_at_every_tick(cuda, oracle, R):
    import rsp_snapshot_cases as c
    c.craft_shadow_stores(cuda, oracle, R)


def test_store_offsets_past_4_gib(cuda, oracle):
    import rsp_snapshot_cases as c
    c.store_past_4gib(cuda, oracle)


def test_store_more_tiles_than_wavefronts(cuda, oracle):
    import rsp_snapshot_cases as c
    c.store_more_tiles_than_wavefronts(cuda, oracle)
