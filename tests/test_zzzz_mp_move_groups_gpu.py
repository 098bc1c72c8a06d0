"""smr_mp_save_groups / smr_mp_load_groups / smr_mp_reset_groups on the device: the bodies of tests/mp_move_groups_cases.py
(which the emulator runs in tests/test_mp_move_groups.py), against the CPU oracle."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu


def test_symbols_are_exported_and_bound(cuda):
    import mp_move_groups_cases as c
    from summerset_amd import _lib
    c.symbols(_lib.load())


@pytest.mark.parametrize("straggler_ticks", [0, 1])
def test_move_at_every_boundary(cuda, oracle, straggler_ticks):
    import mp_move_groups_cases as c
    c.move_at_every_boundary(cuda, oracle, straggler_ticks)


@pytest.mark.parametrize("lists", [("reversed", "1", "63", "last"), ("330",)], ids=["1_63_64_65", "330"])
def test_list_shapes(cuda, oracle, lists):
    import mp_move_groups_cases as c
    c.list_shapes(cuda, oracle, lists)


def test_list_shapes_permutation_of_66000_groups(cuda, oracle):
    """1 032 tiles for the launch's 1 024 wavefronts, every row of the cluster side a gather"""
    import mp_move_groups_cases as c
    c.permutation_of_a_large_cluster(cuda, oracle)


def test_interchange_with_whole_cluster_images(cuda, oracle):
    import mp_move_groups_cases as c
    c.interchange(cuda, oracle)


def test_other_window_wrapped_ring_frozen_group(cuda, oracle):
    import mp_move_groups_cases as c
    c.other_window(cuda, oracle)


def test_into_a_long_quiet_cluster_under_batches(cuda, oracle):
    import mp_move_groups_cases as c
    on = c.into_a_long_quiet_cluster(cuda, oracle, True)
    off = c.into_a_long_quiet_cluster(cuda, oracle, False)
    for a, b in zip(on, off):
        assert all(np.array_equal(a[k], b[k]) for k in a)


def test_neighbours_untouched_and_reset(cuda, oracle):
    import mp_move_groups_cases as c
    c.neighbours_and_reset(cuda, oracle)


def test_partial_live_mask(cuda, oracle):
    import mp_move_groups_cases as c
    c.partial_live_mask(cuda, oracle)


def test_refusals(cuda, oracle):
    import mp_move_groups_cases as c
    c.refusals(cuda, oracle)
