"""The EPaxos image's bytes against tests/golden/ep_snapshot_image_digests.json, on the device: the digest was recorded from the
emulator, the device must produce the same bytes (tests/ep_snapshot_digest_cases.py)."""
import pytest

pytestmark = pytest.mark.gpu


def test_ep_replica_image_digest(cuda, oracle):
    import ep_snapshot_digest_cases as c
    c.check(cuda, oracle)
