"""smr_mp_snapshot_from_wal on the device: the bodies of tests/mp_wal_replay_cases.py (which the emulator runs in
tests/test_mp_wal_replay.py), against a literal restatement of recovery.rs:10-116."""
import pytest

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("W", [16, 64])
def test_random_valid_logs(cuda, W):
    import mp_wal_replay_cases as c
    c.random_logs(cuda, W)


def test_canonical_bytes(cuda):
    import mp_wal_replay_cases as c
    c.canonical_bytes(cuda)


def test_order_dependent_bars(cuda):
    import mp_wal_replay_cases as c
    c.order_dependent_bars(cuda)


def test_framing(cuda):
    import mp_wal_replay_cases as c
    c.framing(cuda)


def test_statuses(cuda):
    import mp_wal_replay_cases as c
    c.statuses(cuda)


def test_refusals(cuda):
    import mp_wal_replay_cases as c
    c.refusals(cuda)


def test_listed_groups(cuda):
    import mp_wal_replay_cases as c
    c.listed_groups(cuda)


def test_the_recovered_cluster_goes_on(cuda):
    import mp_wal_replay_cases as c
    c.goes_on(cuda)


def test_offsets_past_4_gib(cuda):
    import mp_wal_replay_cases as c
    c.past_4gib(cuda)


def test_live_mask_below_the_population(cuda):
    import mp_wal_replay_cases as c
    c.live_subset(cuda)
