"""smr_ep_save_state / smr_ep_load_state and their cluster forms on the device: the bodies of tests/ep_snapshot_cases.py (which
the emulator runs in tests/test_ep_snapshot.py), against the CPU oracle."""
import pytest

pytestmark = pytest.mark.gpu


def test_symbols_are_exported_and_bound(cuda):
    """(the `cuda` fixture first: torch brings its own HIP runtime, and the engine library must find that one already loaded, as
    in every other device test, also when this file runs alone)"""
    import test_ep_snapshot as t
    from summerset_amd import _lib
    lib = _lib.load()
    for n in t.NAMES:
        assert getattr(lib, n)


def _shapes():
    import test_ep_snapshot as t
    return t.SHAPES


@pytest.mark.parametrize("G,R,K,cluster_form,seated,recovery", _shapes())
def test_shadow_at_every_boundary(cuda, oracle, G, R, K, cluster_form, seated, recovery):
    """(the parameters of the emulator file's test of this name, see there)"""
    import ep_snapshot_cases as c
    c.shadow(cuda, oracle, G=G, R=R, K=K, cluster_form=cluster_form, seated=seated, recovery=recovery)


def test_shadow_more_tiles_than_a_block(cuda, oracle):
    """4 100 groups: 65 tiles, 17 blocks of the snapshot kernels per replica -- the offsets across blocks.  Six ticks: the rings do
    not wrap, so the schedule's own conditions are not asked"""
    import ep_snapshot_cases as c
    c.shadow(cuda, oracle, G=4100, R=3, K=2, T=6, cluster_form=True, want=False)


def test_more_tiles_than_wavefronts(cuda):
    """66 000 groups: 1 032 tiles for the launch's 1 024 wavefronts a replica, two tiles each.  Save, load into a second set: the
    existing dumps of the two sets are equal and the image read in numpy equals them.  (Window 8: the engine takes none smaller)"""
    import ep_snapshot_cases as c
    c.two_sets_large(cuda)


def test_stored_replies_survive(cuda, oracle):
    import ep_snapshot_cases as c
    assert c.stored_replies_survive(cuda, oracle) > 0


def test_canonical_bytes(cuda, oracle):
    import ep_snapshot_cases as c
    c.canonical_bytes(cuda, oracle)


def test_hand_built_image(cuda):
    import ep_snapshot_cases as c
    c.hand_built_image(cuda)


def test_restart_of_one_replica(cuda, oracle):
    import ep_snapshot_cases as c
    c.restart_of_one_replica(cuda, oracle)


def test_save_is_stream_ordered(cuda, oracle):
    import ep_snapshot_cases as c
    c.stream_order(cuda, oracle, G=4100)


def test_refusals(cuda, oracle):
    import ep_snapshot_cases as c
    c.refusals(cuda, oracle)


def test_snapshot_grows_for_a_larger_window(cuda, oracle):
    import ep_snapshot_cases as c
    c.grows_for_a_larger_window(cuda, oracle)


def test_abort_and_restore_in_l2(cuda, oracle):
    """(one rank on the device)"""
    import ep_snapshot_cases as c
    c.abort_and_restore_l2(cuda, oracle, 1)
