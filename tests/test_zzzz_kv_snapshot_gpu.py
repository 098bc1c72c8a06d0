"""smr_skv_* and smr_kv_* save / load / chosen groups / compaction on the device: the bodies of tests/kv_snapshot_cases.py (which
the emulator runs in tests/test_kv_snapshot.py), against Python dicts and a model of the documented image, plus the two cases
only the device can hold: a 66 000-group permutation and an image past 4 GiB."""
import pytest

pytestmark = pytest.mark.gpu


def test_symbols_are_exported_and_bound(cuda):
    import kv_snapshot_cases as c
    from summerset_amd import _lib
    c.symbols(_lib.load())


def test_identity_at_every_boundary(cuda):
    """G = 130, the device's slots of 64 and 256 and 32 KiB heaps; lists of 1, 63, 64, 65 and 130"""
    import kv_snapshot_cases as c
    c.identity_at_every_boundary(cuda, slots=(64, 256), heap=(1 << 15, 1 << 14))


def test_canonical_bytes(cuda):
    import kv_snapshot_cases as c
    c.canonical_bytes(cuda)


def test_record_sizes_around_the_pad(cuda):
    import kv_snapshot_cases as c
    c.record_sizes_around_the_pad(cuda)


def test_a_full_table(cuda):
    import kv_snapshot_cases as c
    c.full_table(cuda)


def test_compaction(cuda):
    import kv_snapshot_cases as c
    c.compaction(cuda)


def test_a_move_changes_object_and_position(cuda):
    import kv_snapshot_cases as c
    c.move_between_stores(cuda)


def test_neighbours_untouched(cuda):
    import kv_snapshot_cases as c
    c.neighbours_untouched(cuda)


def test_list_shapes(cuda):
    """330 list entries: six tiles, two blocks of the head launch"""
    import kv_snapshot_cases as c
    c.list_shapes(cuda)


def test_permutation_of_66000_groups_onto_itself(cuda):
    """device only: 1 032 tiles for 1 024 wavefronts, slots = 8, heap_bytes = 256, moved onto itself in reversed order"""
    import kv_snapshot_cases as c
    c.permutation_onto_itself(cuda)


def test_past_4gib(cuda):
    """device only: 70 000 groups x 66 000 bytes of heap, an image larger than 2^32 bytes"""
    import kv_snapshot_cases as c
    c.past_4gib(cuda)


def test_refusals(cuda):
    import kv_snapshot_cases as c
    c.refusals(cuda)


def test_stream_order(cuda):
    import kv_snapshot_cases as c
    c.stream_order(cuda)


def test_token_table(cuda):
    import kv_snapshot_cases as c
    c.token_table(cuda)
