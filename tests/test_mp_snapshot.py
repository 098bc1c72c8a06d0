"""smr_mp_save_state / smr_mp_load_state on the emulator build of the engine (tests/hostsim): the shipped kernels and
C-ABI, every lane a fiber, against the CPU oracle.  The bodies are tests/mp_snapshot_cases.py; the device runs the same ones
in tests/test_zzzz_mp_snapshot_gpu.py."""
import pytest


@pytest.fixture(scope="module")
def sim():
    import hostsim
    hostsim.build()
    return hostsim


def test_symbols_are_exported_and_bound(sim):
    from summerset_amd import _lib
    names = {n for n, _, _ in _lib.SYMBOLS}
    lib = sim.load()
    for n in ("smr_mp_snapshot_create", "smr_mp_snapshot_destroy", "smr_mp_save_state", "smr_mp_load_state", "smr_mp_snapshot_info_get",
              "smr_mp_snapshot_export", "smr_mp_snapshot_import"):
        assert n in names and getattr(lib, n)


@pytest.mark.parametrize("straggler_ticks", [0, 1])
def test_shadow_at_every_boundary_leader_changes(sim, oracle, straggler_ticks):
    import mp_snapshot_cases as c
    with sim.patched():
        c.shadow_at_every_boundary("cpu", oracle, G=200, R=5, S=2, W=64, n_ticks=40, drop_p=0.1, timeout_frac=1.0, hb_every=4,
                                   straggler_ticks=straggler_ticks)


def test_shadow_at_every_boundary_three_replicas(sim, oracle):
    import mp_snapshot_cases as c
    with sim.patched():
        c.shadow_at_every_boundary("cpu", oracle, G=65, R=3, S=2, W=32, n_ticks=30, drop_p=0.2, timeout_frac=0.5, hb_every=2)


def test_shadow_at_every_boundary_seven_replicas_commit_extra(sim, oracle):
    import mp_snapshot_cases as c
    with sim.patched():
        c.shadow_at_every_boundary("cpu", oracle, G=100, R=7, S=2, W=64, n_ticks=30, drop_p=0.15, timeout_frac=0.0, hb_every=4, commit_extra=2)


def test_shadow_at_every_boundary_wrapped_ring(sim, oracle):
    import mp_snapshot_cases as c
    with sim.patched():
        A, _ = c.shadow_at_every_boundary("cpu", oracle, G=64, R=5, S=3, W=16, n_ticks=40, drop_p=0.0, timeout_frac=0.0, hb_every=8,
                                          expect_wrapped=True)
        assert A.counters(0)["rejects"] > 0


def test_shadow_with_two_blocks_of_the_snapshot_kernels(sim, oracle):
    """330 groups: six tiles, six wavefronts, two blocks (the second half idle) -- the record offsets across blocks"""
    import mp_snapshot_cases as c
    with sim.patched():
        c.shadow_at_every_boundary("cpu", oracle, G=330, R=3, S=1, W=32, n_ticks=8, drop_p=0.2, timeout_frac=1.0, hb_every=3)


def test_shadow_at_every_boundary_natural_bootstrap(sim, oracle):
    import mp_snapshot_cases as c
    with sim.patched():
        c.shadow_at_every_boundary("cpu", oracle, G=64, R=5, S=1, W=64, n_ticks=24, drop_p=0.05, timeout_frac=0.3, hb_every=4, preset=False)


@pytest.mark.parametrize("a,b", [
    (dict(W=64), dict(W=256)),
    (dict(straggler_ticks=0), dict(straggler_ticks=4)),
    (dict(straggler_ticks=2, rotate=True), dict(straggler_ticks=2)),
    (dict(how=8, straggler_ticks=3), dict(how="tick", straggler_ticks=3)),
    (dict(how=8), dict(how="tick")),
    (dict(how="rounds"), dict(how="tick")),
], ids=["window", "straggler_ticks", "role_rotation", "batches_with_the_list", "fused_batches", "split_rounds"])
def test_canonical_bytes(sim, oracle, a, b):
    import mp_snapshot_cases as c
    with sim.patched():
        assert c.canonical_bytes("cpu", oracle, a, b, resume=a.get("W") == 64)


def test_resize_to_a_larger_ring(sim, oracle):
    import mp_snapshot_cases as c
    with sim.patched():
        c.resize("cpu", oracle)


def test_save_and_load_under_the_fused_path(sim, oracle):
    import mp_snapshot_cases as c
    with sim.patched():
        c.under_the_fused_path("cpu", oracle)


@pytest.mark.parametrize("world", [2, 4])
def test_abort_and_restore_in_l2(sim, oracle, world):
    import mp_snapshot_cases as c
    with sim.patched():
        c.abort_and_restore_l2("cpu", oracle, world)


def test_refusals(sim, oracle):
    import mp_snapshot_cases as c
    with sim.patched():
        c.refusals("cpu", oracle)


def test_snapshot_made_small_is_reused_by_a_larger_cluster(sim, oracle):
    import mp_snapshot_cases as c
    with sim.patched():
        c.reuse_into_a_larger_cluster("cpu", oracle)
