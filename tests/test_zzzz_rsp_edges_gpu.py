"""The RSPaxos engine and the payload stores on the device away from five replicas, leader 0 and small ballots: the bodies of
tests/rsp_edges.py (which tests/test_hostsim.py runs smaller on the kernel-source emulator) -- populations 3..8 through the
handler calls and through the one-launch steady tick (blocks of 192 .. 512 threads, leaders that are not wavefront 0), ballots
across 2^32 and 2^63, leader changes on wrapped rings, the payload stores at every (n, d) scheme -- bit-exact against
`oracle.RspOracle` after every tick and against `oracle.rs_encode` byte for byte.  G = 130 / 65 / 40: a partial last block, the
64 / 65 wavefront edge.  Stage 10: behind the rest of the suite under `pytest -x`."""
import pytest

import rsp_edges as e

pytestmark = [pytest.mark.gpu, pytest.mark.timeout(600), pytest.mark.stage(10)]


# ---- A. populations through the handler calls ----
@pytest.mark.parametrize("R,ft", [(3, 0), (3, 1), (4, 1), (6, 2), (7, 3), (8, 0), (8, 3)])
def test_closed_loop_at_other_populations(cuda, oracle, R, ft):
    e.run_populations(cuda, oracle, R, ft, G=130)


@pytest.mark.parametrize("R,me,ft", [(3, 0, 0), (3, 2, 1), (7, 3, 2), (8, 0, 0), (8, 7, 3)])
def test_random_handler_calls_at_other_populations(cuda, oracle, R, me, ft):
    e.run_random_calls(cuda, oracle, R, me, ft)


# ---- B. wide ballots ----
@pytest.mark.parametrize("R,ft,W", [(5, 1, 16), (3, 0, 8)])
@pytest.mark.parametrize("round0", [2**24 - 2, 2**55 - 2], ids=["across_2_32", "across_2_63"])
def test_closed_loop_at_wide_ballots(cuda, oracle, round0, R, ft, W):
    e.run_wide_ballots(cuda, oracle, round0, R, ft, W)


@pytest.mark.parametrize("W,me,ft", [(8, 2, 1), (16, 0, 0)])
@pytest.mark.parametrize("round0", [2**24 - 1, 2**55 - 1], ids=["from_2_32", "from_2_63"])
def test_random_handler_calls_from_wide_ballots(cuda, oracle, round0, W, me, ft):
    e.run_random_calls(cuda, oracle, 5, me, ft, W=W, round0=round0)


# ---- C. past the ring ----
@pytest.mark.parametrize("R,seed", [(5, 2), (8, 8)])
def test_leader_changes_past_the_ring(cuda, oracle, R, seed):
    e.run_past_the_ring(cuda, oracle, R, 1, G=130, seed=seed)


# ---- D. the steady tick, call by call and as one launch ----
STEADY = [(5, 3, 1), (5, 4, 0), (3, 0, 0), (3, 2, 1), (4, 1, 1), (7, 6, 2), (8, 0, 3), (8, 7, 1), (8, 5, 0)]


@pytest.mark.parametrize("one_launch", [True, False], ids=["one_launch", "calls"])
@pytest.mark.parametrize("R,leader,ft", STEADY)
def test_steady_tick_at_other_populations_and_leaders(cuda, oracle, R, leader, ft, one_launch):
    e.run_steady_case(cuda, oracle, R, leader, ft, 65, one_launch)


@pytest.mark.parametrize("one_launch", [True, False], ids=["one_launch", "calls"])
@pytest.mark.parametrize("G", [1, 63, 64, 130])
@pytest.mark.parametrize("R,leader,ft", [(8, 7, 1), (3, 2, 1)])
def test_steady_tick_group_counts(cuda, oracle, R, leader, ft, G, one_launch):
    e.run_steady_case(cuda, oracle, R, leader, ft, G, one_launch)


@pytest.mark.parametrize("one_launch", [True, False], ids=["one_launch", "calls"])
@pytest.mark.parametrize("R,leader,ft", [(5, 3, 1), (8, 7, 1), (3, 2, 1)])
@pytest.mark.parametrize("round0", [2**24 - 1, 2**55 - 1], ids=["above_2_32", "above_2_63"])
def test_steady_tick_at_wide_ballots(cuda, oracle, round0, R, leader, ft, one_launch):
    """the leader got there through a Prepare phase behind a first Heartbeat at round0: every ballot of the run is >= 2^32 / 2^63"""
    e.run_steady_case(cuda, oracle, R, leader, ft, 65, one_launch, round0=round0)


# ---- E. the payload stores over the schemes ----
@pytest.mark.parametrize("R,ft,L", [(3, 0, 133), (3, 1, 31), (4, 1, 97), (6, 2, 133), (7, 3, 200), (7, 0, 15), (8, 1, 333), (8, 3, 1), (8, 0, 81)])
def test_bytes_follow_the_engine_at_other_populations(cuda, oracle, R, ft, L):
    e.run_payload_closed_loop(cuda, oracle, R, ft, L)


@pytest.mark.parametrize("R,ft,L,loss", [(3, 1, 50, 0.1), (8, 2, 133, 0.1), (7, 1, 64, 0.05)])
def test_bytes_travel_as_messages_at_other_populations(cuda, oracle, R, ft, L, loss):
    e.run_payload_closed_loop(cuda, oracle, R, ft, L, loss=loss, staging=True)


@pytest.mark.parametrize("scheme", e.MAJORITY_SCHEMES + e.OTHER_SCHEMES, ids=lambda s: "%d_%d" % s)
def test_store_scheme_sweep(cuda, oracle, scheme):
    for L in e.SWEEP_LENGTHS:
        e.run_scheme_sweep(cuda, oracle, scheme[0], scheme[1], L)


def test_one_call_byte_path_with_seven_followers(cuda, oracle, monkeypatch):
    """`put_follow_all` against the separate calls at R = 8: seven followers in the put launch, RS(5, 3); L = 333 is five 16-byte
    columns per group"""
    e.run_one_call(cuda, oracle, monkeypatch, 8, G=12, L=333, T=27, seed=1)


@pytest.mark.parametrize("many", [False, "one_call"], ids=["calls", "put_follow_all"])
@pytest.mark.parametrize("R", [3, 7])
def test_craft_stores_at_other_populations(cuda, oracle, R, many):
    e.run_craft_stores(cuda, oracle, R, many)


# ---- F. creation errors ----
def test_creation_errors_allocate_nothing(cuda):
    e.creation_errors(cuda)
