"""The exported snapshot images do not move: one image per kind from a fixed-seed schedule on the emulator build of the engine
(tests/hostsim), against the SHA-256 recorded in tests/golden/snapshot_image_digests.json.  The bodies are
tests/snapshot_digest_cases.py; the device runs the same ones in tests/test_zzzz_snapshot_digests_gpu.py."""
import pytest

import snapshot_digest_cases as c


@pytest.fixture(scope="module")
def sim():
    import hostsim
    hostsim.build()
    return hostsim


@pytest.mark.parametrize("kind", sorted(c.KINDS))
def test_image_is_the_recorded_one(sim, oracle, kind):
    with sim.patched():
        c.same_as_recorded(kind, "cpu", oracle)
