"""smr_rsp_save_state / smr_rsp_load_state and their cluster forms on the emulator build of the engine (tests/hostsim): the
shipped kernels and C-ABI, every lane a fiber, against the CPU oracle.  The bodies are tests/rsp_snapshot_cases.py; the device
runs the same ones in tests/test_zzzz_rsp_snapshot_gpu.py."""
import pytest

NAMES = ("smr_rsp_snapshot_create", "smr_rsp_snapshot_destroy", "smr_rsp_save_state", "smr_rsp_load_state", "smr_rsp_snapshot_info_get",
         "smr_rsp_snapshot_export", "smr_rsp_snapshot_import", "smr_rsp_cluster_save_state", "smr_rsp_cluster_load_state")


@pytest.fixture(scope="module")
def sim():
    import hostsim
    hostsim.build()
    return hostsim


def test_symbols_are_exported_and_bound(sim):
    import summerset_amd
    from summerset_amd import _lib, rspaxos
    names = {n for n, _, _ in _lib.SYMBOLS}
    lib = sim.load()
    for n in NAMES:
        assert n in names and getattr(lib, n)
    assert hasattr(summerset_amd, "RSPaxosSnapshot")
    for n in ("RSPaxosSnapshot", "save_cluster_state", "load_cluster_state"):
        assert hasattr(rspaxos, n)
    for n in ("create_like", "save", "load", "info", "export", "import_"):
        assert hasattr(rspaxos.RSPaxosSnapshot, n)


@pytest.mark.parametrize("G,R,ft,cluster_form", [(520, 3, 1, True), (130, 5, 1, False), (65, 8, 2, True), (65, 3, 0, False)])
def test_shadow_at_every_boundary(sim, oracle, G, R, ft, cluster_form):
    """520 groups are nine tiles, three blocks of the snapshot kernels (the last one mostly idle): the record offsets across tiles
    and across blocks; 130 groups three tiles of one block; 65 the 64 / 65 wavefront edge.  Window 8 and logs past 40: the rings
    wrap several times, both leader changes fall on wrapped rings"""
    import rsp_snapshot_cases as c
    with sim.patched():
        cov = c.shadow_replicas("cpu", oracle, G=G, R=R, ft=ft, cluster_form=cluster_form)
    assert cov["ticks"] == 44


def test_shadow_one_group(sim, oracle):
    """(one group cannot reach every rare path of the schedule; the ring still wraps five times)"""
    import rsp_snapshot_cases as c
    with sim.patched():
        c.shadow_replicas("cpu", oracle, G=1, R=3, ft=0, loss=0.0, rare=False)


def test_shadow_from_wide_ballots(sim, oracle):
    """rsp_edges.run_wide_ballots' start: ballots on both sides of 2^32 in the images"""
    import rsp_snapshot_cases as c
    with sim.patched():
        c.shadow_replicas("cpu", oracle, G=130, R=3, ft=0, T=18, round0=2**24 - 2, cluster_form=True)


def test_canonical_bytes(sim, oracle):
    import rsp_snapshot_cases as c
    with sim.patched():
        c.canonical_bytes("cpu", oracle)


def test_restart_of_one_replica(sim, oracle):
    import rsp_snapshot_cases as c
    with sim.patched():
        st = c.restart_one_replica("cpu", oracle)
    assert st["stepped"] > 0 and st["caught_up_at"] is not None


def test_hand_built_image(sim):
    import rsp_snapshot_cases as c
    with sim.patched():
        c.hand_built_image("cpu")


def test_save_is_stream_ordered(sim, oracle):
    import rsp_snapshot_cases as c
    with sim.patched():
        c.stream_order("cpu", oracle, G=130)


def test_refusals(sim, oracle):
    import rsp_snapshot_cases as c
    with sim.patched():
        c.refusals("cpu", oracle)


def test_snapshot_grows_for_a_larger_window(sim, oracle):
    import rsp_snapshot_cases as c
    with sim.patched():
        c.grows_for_a_larger_window("cpu", oracle)


# ---- the payload stores ----
PS_NAMES = ("smr_rsp_pstore_snapshot_create", "smr_rsp_pstore_snapshot_destroy", "smr_rsp_pstore_save", "smr_rsp_pstore_load",
            "smr_rsp_pstore_snapshot_info_get", "smr_rsp_pstore_snapshot_export", "smr_rsp_pstore_snapshot_import")


def test_store_symbols_are_exported_and_bound(sim):
    import summerset_amd
    from summerset_amd import _lib
    names = {n for n, _, _ in _lib.SYMBOLS}
    lib = sim.load()
    for n in PS_NAMES:
        assert n in names and getattr(lib, n)
    assert hasattr(summerset_amd, "PayloadStoreSnapshot")
    assert hasattr(summerset_amd.RSPaxosReplicaWithPayload, "save_state") and hasattr(summerset_amd.RSPaxosReplicaWithPayload, "load_state")


@pytest.mark.parametrize("G,R,ft,L,staging", [(40, 3, 1, 61, False), (40, 3, 0, 61, True)])
def test_store_shadow_at_every_boundary(sim, oracle, G, R, ft, L, staging):
    """(the emulator runs every lane of the byte kernels as a fiber: G = 96 with L = 333 takes six minutes here and L = 4113 longer,
    and eight replicas with staging stores ten, so those shapes run on the device only, tests/test_zzzz_rsp_snapshot_gpu.py)"""
    import rsp_snapshot_cases as c
    with sim.patched():
        c.shadow_stores("cpu", oracle, G=G, R=R, ft=ft, L=L, staging=staging)


def test_store_canonical_bytes(sim, oracle):
    import rsp_snapshot_cases as c
    with sim.patched():
        c.store_canonical_bytes("cpu", oracle)


def test_hand_built_store_image(sim):
    import rsp_snapshot_cases as c
    with sim.patched():
        c.hand_built_store_image("cpu")


def test_store_save_is_stream_ordered(sim, oracle):
    import rsp_snapshot_cases as c
    with sim.patched():
        c.store_stream_order("cpu", oracle, G=40, L=61)


def test_store_refusals(sim, oracle):
    import rsp_snapshot_cases as c
    with sim.patched():
        c.store_refusals("cpu", oracle)


def test_store_snapshot_grows_for_longer_payloads(sim, oracle):
    import rsp_snapshot_cases as c
    with sim.patched():
        c.store_grows("cpu", oracle)


@pytest.mark.parametrize("R", [3, 5])
def test_craft_store_shadow_at_every_tick(sim, oracle, R):
    import rsp_snapshot_cases as c
    with sim.patched():
        c.craft_shadow_stores("cpu", oracle, R)
