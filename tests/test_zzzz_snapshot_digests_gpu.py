"""The exported snapshot images do not move, on the device: the schedules of tests/test_snapshot_digests.py (bodies:
tests/snapshot_digest_cases.py) against the same recorded SHA-256 -- the device's image of a state is the emulator's."""
import pytest

import snapshot_digest_cases as c

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("kind", sorted(c.KINDS))
def test_image_is_the_recorded_one(cuda, oracle, kind):
    c.same_as_recorded(kind, cuda, oracle)
