"""The EPaxos image's bytes against tests/golden/ep_snapshot_image_digests.json, on the emulator (tests/ep_snapshot_digest_cases.py)."""
import pytest


@pytest.fixture(scope="module")
def sim():
    import hostsim
    hostsim.build()
    return hostsim


def test_ep_replica_image_digest(sim, oracle):
    import ep_snapshot_digest_cases as c
    with sim.patched():
        c.check("cpu", oracle)
