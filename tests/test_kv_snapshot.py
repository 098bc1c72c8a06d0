"""smr_skv_* and smr_kv_* save / load / chosen groups / compaction on the emulator build of the library (tests/hostsim): the shipped
kernels and C-ABI, every lane a fiber, against Python dicts and a model of the documented image.  The bodies are
tests/kv_snapshot_cases.py; the device runs the same ones, and the two cases only it can hold, in
tests/test_zzzz_kv_snapshot_gpu.py.  Shapes are small here: G <= 130, slots 8 .. 64, heap_bytes <= 4 KiB -- with two exceptions that
their cases force: the list of 330 entries needs a store of more groups (G = 400, at slots 8 and heap_bytes 256), and the store
whose every key is overwritten 20 times needs the room for its dead bytes (heap_bytes 8 KiB at G = 70)."""
import pytest


@pytest.fixture(scope="module")
def sim():
    import hostsim
    hostsim.build()
    return hostsim


def test_symbols_are_exported_and_bound(sim):
    import kv_snapshot_cases as c
    c.symbols(sim.load())


def test_identity_at_every_boundary(sim):
    import kv_snapshot_cases as c
    with sim.patched():
        c.identity_at_every_boundary("cpu")


def test_canonical_bytes(sim):
    import kv_snapshot_cases as c
    with sim.patched():
        c.canonical_bytes("cpu")


def test_record_sizes_around_the_pad(sim):
    import kv_snapshot_cases as c
    with sim.patched():
        c.record_sizes_around_the_pad("cpu")


def test_a_full_table(sim):
    import kv_snapshot_cases as c
    with sim.patched():
        c.full_table("cpu")


def test_compaction(sim):
    import kv_snapshot_cases as c
    with sim.patched():
        c.compaction("cpu")


def test_a_move_changes_object_and_position(sim):
    import kv_snapshot_cases as c
    with sim.patched():
        c.move_between_stores("cpu")


def test_neighbours_untouched(sim):
    """... and a save and a load inside red zones around the image and the listed groups' heap strips: zero hits"""
    import kv_snapshot_cases as c
    with sim.patched():
        c.neighbours_untouched("cpu", zones=sim.red_zones)


def test_list_shapes(sim):
    """330 list entries: six tiles, two blocks of the head launch"""
    import kv_snapshot_cases as c
    with sim.patched():
        c.list_shapes("cpu")


def test_refusals(sim):
    import kv_snapshot_cases as c
    with sim.patched():
        c.refusals("cpu")


def test_stream_order(sim):
    import kv_snapshot_cases as c
    with sim.patched():
        c.stream_order("cpu")


def test_token_table(sim):
    import kv_snapshot_cases as c
    with sim.patched():
        c.token_table("cpu")
