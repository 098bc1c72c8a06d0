"""smr_mp_save_state / smr_mp_load_state on the device: the bodies of tests/mp_snapshot_cases.py (which the emulator runs in
tests/test_mp_snapshot.py) at the shapes the MultiPaxos device tests use, against the CPU oracle."""
import pytest

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("straggler_ticks", [0, 1])
def test_shadow_at_every_boundary_leader_changes(cuda, oracle, straggler_ticks):
    import mp_snapshot_cases as c
    c.shadow_at_every_boundary(cuda, oracle, G=200, R=5, S=2, W=64, n_ticks=40, drop_p=0.1, timeout_frac=1.0, hb_every=4,
                               straggler_ticks=straggler_ticks)


def test_shadow_at_every_boundary_other_shapes(cuda, oracle):
    import mp_snapshot_cases as c
    c.shadow_at_every_boundary(cuda, oracle, G=65, R=3, S=2, W=32, n_ticks=30, drop_p=0.2, timeout_frac=0.5, hb_every=2)
    c.shadow_at_every_boundary(cuda, oracle, G=100, R=7, S=2, W=64, n_ticks=30, drop_p=0.15, timeout_frac=0.0, hb_every=4, commit_extra=2)
    A, _ = c.shadow_at_every_boundary(cuda, oracle, G=64, R=5, S=3, W=16, n_ticks=40, drop_p=0.0, timeout_frac=0.0, hb_every=8,
                                      expect_wrapped=True)
    assert A.counters(0)["rejects"] > 0
    c.shadow_at_every_boundary(cuda, oracle, G=64, R=5, S=1, W=64, n_ticks=24, drop_p=0.05, timeout_frac=0.3, hb_every=4, preset=False)


def test_shadow_more_tiles_than_a_block(cuda, oracle):
    """4 100 groups: 65 tiles, 17 blocks of the snapshot kernels, the last one partly idle -- the offsets across blocks"""
    import mp_snapshot_cases as c
    c.shadow_at_every_boundary(cuda, oracle, G=4100, R=5, S=2, W=64, n_ticks=12, drop_p=0.1, timeout_frac=1.0, hb_every=4)


def test_shadow_more_tiles_than_wavefronts(cuda, oracle):
    """66 000 groups: 1 032 tiles for the launch's 1 024 wavefronts, two tiles each -- a wavefront's own prefix inside its block"""
    import mp_snapshot_cases as c
    c.shadow_at_every_boundary(cuda, oracle, G=66000, R=3, S=1, W=8, n_ticks=4, drop_p=0.2, timeout_frac=1.0, hb_every=2)


@pytest.mark.parametrize("a,b", [
    (dict(W=64), dict(W=256)),
    (dict(straggler_ticks=0), dict(straggler_ticks=4)),
    (dict(straggler_ticks=2, rotate=True), dict(straggler_ticks=2)),
    (dict(how=8, straggler_ticks=3), dict(how="tick", straggler_ticks=3)),
    (dict(how=8), dict(how="tick")),
    (dict(how="rounds"), dict(how="tick")),
], ids=["window", "straggler_ticks", "role_rotation", "batches_with_the_list", "fused_batches", "split_rounds"])
def test_canonical_bytes(cuda, oracle, a, b):
    import mp_snapshot_cases as c
    assert c.canonical_bytes(cuda, oracle, a, b, G=300, resume=a.get("W") == 64)


def test_resize_to_a_larger_ring(cuda, oracle):
    import mp_snapshot_cases as c
    c.resize(cuda, oracle, G=256)


def test_save_and_load_under_the_fused_path(cuda, oracle):
    import mp_snapshot_cases as c
    c.under_the_fused_path(cuda, oracle, G=600)


@pytest.mark.parametrize("world", [2, 4])
def test_abort_and_restore_in_l2(cuda, oracle, world):
    import mp_snapshot_cases as c
    c.abort_and_restore_l2(cuda, oracle, world)


def test_refusals(cuda, oracle):
    import mp_snapshot_cases as c
    c.refusals(cuda, oracle)


def test_snapshot_made_small_is_reused_by_a_larger_cluster(cuda, oracle):
    import mp_snapshot_cases as c
    c.reuse_into_a_larger_cluster(cuda, oracle, G=300)
