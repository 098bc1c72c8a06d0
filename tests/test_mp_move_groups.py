"""smr_mp_save_groups / smr_mp_load_groups / smr_mp_reset_groups on the emulator build of the engine (tests/hostsim): the
shipped kernels and C-ABI, every lane a fiber, against the CPU oracle.  The bodies are tests/mp_move_groups_cases.py; the device
runs the same ones in tests/test_zzzz_mp_move_groups_gpu.py."""
import numpy as np
import pytest


@pytest.fixture(scope="module")
def sim():
    import hostsim
    hostsim.build()
    return hostsim


def test_symbols_are_exported_and_bound(sim):
    import mp_move_groups_cases as c
    c.symbols(sim.load())


@pytest.mark.parametrize("straggler_ticks", [0, 1])
def test_move_at_every_boundary(sim, oracle, straggler_ticks):
    import mp_move_groups_cases as c
    with sim.patched():
        c.move_at_every_boundary("cpu", oracle, straggler_ticks)


@pytest.mark.parametrize("lists", [("reversed", "1", "63", "last"), ("330",)], ids=["1_63_64_65", "330"])
def test_list_shapes(sim, oracle, lists):
    """330 list entries: six tiles, two blocks of the group kernels"""
    import mp_move_groups_cases as c
    with sim.patched():
        c.list_shapes("cpu", oracle, lists)


def test_interchange_with_whole_cluster_images(sim, oracle):
    import mp_move_groups_cases as c
    with sim.patched():
        c.interchange("cpu", oracle)


def test_other_window_wrapped_ring_frozen_group(sim, oracle):
    import mp_move_groups_cases as c
    with sim.patched():
        c.other_window("cpu", oracle)


def test_into_a_long_quiet_cluster_under_batches(sim, oracle):
    import mp_move_groups_cases as c
    with sim.patched():
        on = c.into_a_long_quiet_cluster("cpu", oracle, True)
        off = c.into_a_long_quiet_cluster("cpu", oracle, False)
    for a, b in zip(on, off):
        assert all(np.array_equal(a[k], b[k]) for k in a)


def test_neighbours_untouched_and_reset(sim, oracle):
    import mp_move_groups_cases as c
    with sim.patched():
        c.neighbours_and_reset("cpu", oracle)


def test_partial_live_mask(sim, oracle):
    import mp_move_groups_cases as c
    with sim.patched():
        c.partial_live_mask("cpu", oracle)


def test_refusals(sim, oracle):
    import mp_move_groups_cases as c
    with sim.patched():
        c.refusals("cpu", oracle)
