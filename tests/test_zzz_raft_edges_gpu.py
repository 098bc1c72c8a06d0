"""The Raft engine (csrc/raft_engine.hip) where the schedules of test_raft_gpu.py do not reach -- always against oracle.RaftOracle,
bit for bit, every tick (every message, every reply, every replica's dump(), dump_votes(), total_commits(), ring_guard_hits()),
and with the engine's paths side by side where there are several (the handler calls, `smr_raft_cluster_tick`,
`smr_raft_cluster_replicate`, `smr_raft_leader_run_ticks`, `smr_raft_leader_handle_wire_replies`):

* A  terms across 2^31, 2^32 and 2^63 (the sign of the binding's int64 tensors, the 9-byte varint on the wire);
* B  logs several times the W-entry ring, with the leader's back-pressure and the followers' ring_lo, through elections and outages;
* C  rolling outages of one, two and three replicas of five (the one launch with fewer than R - 1 followers), per-group loss,
     replicas that come back behind, as stale leaders and as candidates of a later term;
* D  conflict replies that send the leader's back-off through its second and third round of eight candidates, below ring_lo,
     at next_slot == 1;
* E  messages of one and two entries against six appends a tick, a replica that comes back more than a message behind;
* F  the one launch with 3, 4, 6 and 8 replicas, 1 / 63 / 64 / 65 groups, every length of follower list, its argument errors;
* G  config 2's 65 536 groups x 5 replicas through the one launch against oracle slices.

Every body is a helper taking its sizes and asserting, on the ORACLE cluster alone, that its schedule reached what it is for;
tests/test_hostsim.py runs them small on the emulator build."""
import numpy as np
import pytest

import raft_cluster as rc

pytestmark = [pytest.mark.gpu, pytest.mark.timeout(1500)]

# start term -> the boundary the run's elections cross (term0 + 1 lies below it, term0 + 2 on it)
WIDE = {2**31 - 2: 2**31, 2**32 - 2: 2**32, 2**63 - 2: 2**63}


def _committed_terms(dumps, W):
    """entry_term of every slot 1 .. last_commit that is still in the ring, all replicas"""
    out = []
    for d in dumps:
        sl = np.arange(W)[:, None]
        ln, lc = d["log_len"].astype(np.int64)[None, :], d["last_commit"].astype(np.int64)[None, :]
        slot = ln - 1 - ((ln - 1 - sl) % W)                              # the newest slot that lives in ring row sl
        out.append(d["entry_term"][(slot >= 1) & (slot <= lc)])
    return np.concatenate(out)


def run_wide_terms(dev, oracle, term0, G, arms=("calls", "tick"), W=64, K=8, T=14, seed=41, order="ticks"):
    """the closed loop from `preset(FOLLOWER, none, term0)`: a first election everywhere, then three outages that chase the
    leader of a fifth of the groups (four elections there, two in two other fifths, one in the rest)"""
    sch = rc.Outages(5, G, seed, windows=[(3, 5, (0,)), (6, 8, (3,)), (9, 11, (1,))])
    st = rc.run_closed_loop(dev, oracle, G, 5, W, K, T, sch, term0=term0, arms=arms, order=order)
    b = np.uint64(WIDE[term0])
    ct = np.stack([d["curr_term"] for d in st["dumps"]])
    et = _committed_terms(st["dumps"], W)
    assert ct.max() >= np.uint64(term0 + 3) or G < 5, (term0, int(ct.max()) - term0)      # at least three elections somewhere
    assert (ct < b).any() and (ct >= b).any() and (et < b).any() and (et >= b).any(), (term0, len(et))
    assert (et[et > 0] > np.uint64(term0)).all() and st["stepdown_by_reply"] + st["stepdown_by_append_entries"] > 0
    return st


def run_past_the_ring(dev, oracle, G, W, arms=("calls", "tick"), K=8, T=44, n_new_max=5, seed=43, outages=True, term0=0, order="ticks"):
    """up to `n_new_max` appends a tick at every replica for T ticks, one replica after the other (then two at once) away for
    longer than the ring takes to fill: the leader's back-pressure (len - last_snap >= W), leaders and followers whose ring_lo
    moves, replicas that come back W entries behind, elections on wrapped logs.  Returns (stats, ring_guard_hits per replica)."""
    win = [(3, 3 + W // 2 + 2, (1,)), (W // 2 + 8, W + 10, (3,)), (W + 13, W + 18, (0, 2)), (W + 21, W + 24, (4,))] if outages else []
    sch = rc.Outages(5, G, seed, windows=win, n_new_max=n_new_max)
    st = rc.run_closed_loop(dev, oracle, G, 5, W, K, T, sch, term0=term0, arms=arms, order=order)
    ln = np.stack([d["log_len"] for d in st["dumps"]]).max(axis=0)
    rejects = [int(c[2]) for c in st["counters"]]
    if outages:
        assert (ln > 2 * W).mean() >= 0.25, (W, float((ln > 2 * W).mean()))
        assert max(rejects) > 0, rejects
        assert st["elected"] > G and len(st["conflicts"]) >= 2
    else:
        assert ln.max() < W and st["ring_guard_hits"] == [0] * 5, (int(ln.max()), st["ring_guard_hits"])
    print("raft ring W=%d: ring_guard_hits %s, back-pressure rejects %s, longest log %d" % (W, st["ring_guard_hits"], rejects, int(ln.max())))
    return st, st["ring_guard_hits"]


# C: one away, another, two away, three away (no quorum: nothing may commit), one more; replica 0 and replica 3 come back standing
C_WINDOWS = [(3, 6, (0,)), (8, 11, (2,)), (13, 16, (1, 3)), (18, 20, (0, 2, 4)), (22, 25, (4,))]
C_LONELY = {6: 0, 16: 3}


def run_outages(dev, oracle, G, arms=("calls", "tick"), loss=0.0, W=64, K=8, T=34, seed=47, order="ticks"):
    sch = rc.Outages(5, G, seed, windows=C_WINDOWS, lonely=C_LONELY, loss=loss)
    st = rc.run_closed_loop(dev, oracle, G, 5, W, K, T, sch, arms=arms, order=order)
    cm = st["commit"]
    assert len(st["conflicts"]) >= 3 and min(st["conflicts"].values()) > 0, st["conflicts"]
    assert sum(int(v["n_trunc"].sum()) for v in st["votes"]) > 0
    # (a stale leader that comes back meets a reply of the later term first only where its own step comes before its successor's:
    #  in the other two orders every AppendEntries of a tick -- the successor's re-send among them -- is handled before any reply)
    assert st["next_slot_back"] > 0 and st["stepdown_by_append_entries"] > 0 and (st["stepdown_by_reply"] > 0 or order != "ticks"), \
        (st["next_slot_back"], st["stepdown_by_reply"], st["stepdown_by_append_entries"])
    assert (cm[15] > cm[12]).any(), "two of five away: the other three still commit"
    # three of five away in ticks 18 and 19: what is appended then is held by two replicas at most, so the two that are there
    # must not commit it.  (Not "nothing commits": an entry from before may get its third acknowledgement from a re-send.  And
    # only the two that are there: the reference grants a vote to a candidate whose last entry is of the same term however short
    # its log is, messages.rs:428-430, so a replica that is away may hold a commit index its successor's log never reaches.)
    there = [r for r in range(5) if r not in sch.down_at(18)]
    assert sch.down_at(18) == sch.down_at(19) and len(there) == 2
    c17, c19 = st["commits"][17][there], st["commits"][19][there]
    assert (st["len"][19] > st["len"][17]).any()
    if not loss:                                                      # (with loss the run is only compared, not held to this)
        assert ((c19 == c17) | (c19 < st["len"][17][None, :])).all(), "three of five away: nothing new commits"
    assert (cm[-1] > cm[sch.last_outage_end - 1]).all(), ("progress", int((cm[-1] > cm[sch.last_outage_end - 1]).sum()), G)
    assert st["ring_guard_hits"] == [0] * 5, st["ring_guard_hits"]
    return st


def run_small_messages(dev, oracle, G, K, arms=("calls", "tick"), W=64, T=22, seed=53, order="ticks"):
    """messages of at most K entries against up to six appends a tick: the gather's cap, followers that take a log in partial
    batches, a leader that walks a conflict back slot by slot; K = 8: a replica away long enough to come back more than K behind"""
    win = [(4, 9, (1,)), (11, 14, (0,))] if K < 8 else [(3, 10, (2,)), (12, 15, (0,))]
    sch = rc.Outages(5, G, seed, windows=win, n_new_max=6 if K < 8 else 4)
    st = rc.run_closed_loop(dev, oracle, G, 5, W, K, T, sch, arms=arms, order=order)
    assert st["n_entries_max"] == K, (st["n_entries_max"], K)
    assert st["behind_max"] > 8 and sum(st["conflicts"].values()) > 0, (st["behind_max"], st["conflicts"])
    assert (st["commit"][-1] > st["commit"][sch.last_outage_end - 1]).any()
    return st


def run_populations(dev, oracle, R, G, arms=("calls", "tick"), W=64, K=8, seed=59, order="ticks"):
    """R replicas; every other tick some are away -- 1, 2 .. R - 2 of them, rotating -- so that the one launch runs with every
    length of follower list from R - 1 down to 1"""
    win = [(2 + 2 * j, 3 + 2 * j, tuple((3 * j + i) % R for i in range(j + 1))) for j in range(R - 2)]
    sch = rc.Outages(R, G, seed, windows=win)
    st = rc.run_closed_loop(dev, oracle, G, R, W, K, 2 * R + 4, sch, arms=arms, order=order)
    assert st["followers"] >= set(range(1, R)), st["followers"]
    assert (st["commit"][-1] > 0).all() and st["n_msg"] > 0
    return st


def run_empty_messages(dev, oracle, G, arms=("calls", "tick"), T=8, seed=61, order="ticks"):
    """max_entries = 0, which the ABI allows (`smr_raft_leader_gather_entries`) and the oracle defines alike: every AppendEntries
    is sent without entries (a plain Raft follower answers those without the consistency check, messages.rs:46)"""
    st = rc.run_closed_loop(dev, oracle, G, 5, 64, 0, T, rc.Outages(5, G, seed, windows=[(3, 5, (1,))]), arms=arms, order=order)
    assert st["n_msg"] > 0 and st["n_entries_max"] == 0
    # an empty message is answered as a success and moves the leader's match index and last_snap past what the follower holds
    # (what a heartbeat's reply would do if it were fed to the reply handler): a replica elected later leads with
    # last_snap >= log_len, where the append's ring back-pressure (len - last_snap >= W, unsigned) rejects everything
    assert any((d["last_snap"] >= d["log_len"]).any() for d in st["dumps"]) and max(int(c[2]) for c in st["counters"]) > 0
    return st


def run_wide_terms_leader(dev, oracle, term0, G, T=24):
    """the leader alone on synthetic replies from term `term0`: call by call and in batches of ticks (stale replies carry
    term0 - 1, a few a later term: step-downs in the middle of a batch)"""
    import test_raft_gpu as t
    _, orc = t._run(dev, oracle, G=G, R=5, W=64, T=T, higher_p=0.002, term=term0, wide=True)
    _, orb = t._run_batched(dev, oracle, G=G, R=5, W=64, T=T, batches=(1, 16, T - 17), higher_p=0.002, term=term0, wide=True)
    for o in (orc, orb):
        d = o.dump()
        assert (d["curr_term"] == np.uint64(term0)).any() and (d["curr_term"] == np.uint64(term0 + 1)).any() and (d["role"] == 0).any()
        e1 = d["entry_term"][1]                                           # (a leader that stepped down before its first append holds none)
        assert (e1 == np.uint64(term0)).mean() > 0.9 and (e1[e1 > 0] == np.uint64(term0)).all() and d["last_commit"].max() > 0


def run_wide_terms_follower(dev, oracle, term0, G, W=64):
    """test_raft_gpu's follower / election scenario (crafted AppendEntries, timers, RequestVotes, vote replies) from a wide term"""
    import test_raft_gpu as t
    orc = t.test_follower_and_elections_match_oracle(dev, oracle, G, W, term=term0)
    ct = orc.dump()["curr_term"]
    b = np.uint64(WIDE[term0])
    assert (ct > np.uint64(term0)).all() and ct.max() > b + np.uint64(3), (term0, int(ct.min()), int(ct.max()))
    return orc


def run_wide_terms_wire(dev, oracle, term0, G, T=5):
    """the leader's replies as frames whose terms and conflict terms take the long varint forms: the fused entry against the two
    calls against the oracle"""
    import test_zz_reply_ingest_gpu as t
    return t.run_fused_raft_wire_replies(dev, oracle, G=G, T=T, term0=term0)


def run_deep_conflicts(dev, oracle, G, T=34):
    """D: through `handle_msg_append_entries_reply`, through `run_ticks` (batches of 16: a conflict in every tick of a batch, the
    first and the last among them) and through the fused wire entry; W = 64 for the long walks, W = 16 for conflict slots below
    ring_lo on a wrapped log"""
    import test_raft_gpu as t
    import test_zz_reply_ingest_gpu as tw
    out = {}
    for name, W in (("calls", 64), ("calls_ring", 16)):
        out[name] = {}
        t._run(dev, oracle, G=G, R=5, W=W, T=T, deep=True, conflict_p=0.1, info=out[name])
    for name, W in (("batched", 64), ("batched_ring", 16)):
        out[name] = {}
        t._run_batched(dev, oracle, G=G, R=5, W=W, T=T, batches=(16, 16, T - 32), deep=True, conflict_p=0.1, info=out[name])
    out["wire"] = {}
    tw.run_fused_raft_wire_replies(dev, oracle, G=G, T=26, me=0, seed=23, deep=True, info=out["wire"])
    for name in ("calls", "batched"):
        assert out[name]["fall_max"] > 16 and out[name]["at_one"] > 0, (name, out[name])
    for name in ("calls_ring", "batched_ring"):
        assert out[name]["fall_max"] > 8 and out[name]["below_ring"] > 0, (name, out[name])
    assert out["batched"]["conflict_ticks"] >= set(range(T)), "a conflict in every tick of every batch"
    assert out["wire"]["fall_max"] > 16, out["wire"]
    return out


def run_one_launch_shapes(dev, oracle, G, R=5, T=16):
    """test_raft_gpu.run_one_launch_tick with 1 .. R - 2 replicas away in its last ticks (one to R - 1 followers in the launch)"""
    import test_raft_gpu as t
    down = {T - 2 * (R - 2) + 2 * j: tuple((j + i) % R for i in range(j + 1)) for j in range(R - 2)}
    return t.run_one_launch_tick(dev, oracle, G=G, T=T, R=R, down=down)


def run_cluster_tick_argument_errors(dev):
    """what `smr_raft_cluster_tick` refuses, through the binding: no follower, one listed twice, the leader among its followers,
    followers of another window / population / group count, two followers sharing message or reply buffers"""
    import torch
    from summerset_amd import RaftLeaderGroup, SummersetError
    G, R, W, K = 70, 5, 16, 4
    reps = [RaftLeaderGroup(G, R, leader_id=r, window=W, term=1) for r in range(R)]
    z = lambda shape, dt: torch.zeros(shape, dtype=dt, device=dev)

    def call(ld, fs, msgs=None, share_reply=False, rows=R):
        arr = dict(flags=z((rows, G), torch.uint8), term=z((rows, G), torch.int64), end_slot=z((rows, G), torch.int32),
                   conflict_term=z((rows, G), torch.int64), conflict_slot=z((rows, G), torch.int32))
        msgs = msgs or [ld.new_message(K, dev) for _ in fs]
        rp = [{k: v[0 if share_reply else min(f.me, rows - 1)] for k, v in arr.items()} for f in fs]
        first = z((max(rows, 8), G), torch.int32)
        ld.cluster_tick(z(G, torch.int32), first, fs, msgs, rp, arr["term"], arr["end_slot"], arr["flags"], arr["conflict_term"], arr["conflict_slot"])
    call(reps[0], reps[1:])                                                       # (the good call)
    call(reps[0], [reps[3]])
    bad = [lambda: call(reps[0], []),
           lambda: call(reps[0], [reps[1], reps[2], reps[1]]),
           lambda: call(reps[0], [reps[1], reps[0]]),
           lambda: call(reps[0], [reps[1], RaftLeaderGroup(G, R, leader_id=2, window=2 * W, term=1)]),
           lambda: call(reps[0], [reps[1], RaftLeaderGroup(G, 7, leader_id=2, window=W, term=1)]),
           lambda: call(reps[0], [reps[1], RaftLeaderGroup(G + 1, R, leader_id=2, window=W, term=1)]),
           lambda: call(reps[0], [reps[1], reps[2]], msgs=[reps[0].new_message(K, dev)] * 2),
           lambda: call(reps[0], [reps[1], reps[2]], msgs=[reps[0].new_message(K, dev), reps[0].new_message(K + 1, dev)]),
           lambda: call(reps[0], [reps[1], reps[2]], share_reply=True)]
    for i, f in enumerate(bad):
        with pytest.raises(SummersetError):
            f()
            pytest.fail("refusal %d did not happen" % i)
    d = [r.dump() for r in reps]
    call(reps[0], reps[1:])                                                       # the refused calls launched nothing: still usable
    return len(bad), d


def run_config2_cluster(dev, oracle, G=65536, W=64, K=8, T=None, width=256, n_slices=3, seed=67):
    """G: config 2's shape through `smr_raft_cluster_tick` (one launch per sender and tick, 1024 blocks of 64 groups x 5 wavefronts)
    against five oracles per 64-aligned slice of groups, every replica's state every tick: an election in a third of the groups
    in the middle of the run, one replica away for three ticks"""
    import test_baseline_configs_gpu as tb
    from summerset_amd import RaftLeaderGroup
    R = 5
    T = T or 2 * W + 4
    sl = tb._slices(G, width, n_slices, seed)
    engs = [rc.NumpyRaft(RaftLeaderGroup(G, R, leader_id=r, window=W, term=1), dev) for r in range(R)]
    orcs = [[oracle.RaftOracle(n, R, W, leader_id=r, term=1) for r in range(R)] for _, n in sl]
    for x in engs + [o for oc in orcs for o in oc]:
        x.preset(rc.FOLLOWER, rc.NO, 0)
    rng = np.random.default_rng(seed)
    g = np.arange(G)
    for t in range(T + 1):
        to = np.full((R, G), rc.NO, np.uint8)
        n_new = rng.integers(0, 3, (R, G)).astype(np.uint32)
        down = (3,) if T // 2 + 4 <= t < T // 2 + 7 else ()
        if t == 0:
            to[g % R, g] = 0xFE
        elif t == T // 2:
            gs = np.arange(0, G, 3)
            to[(gs + 2) % R, gs] = (gs % R).astype(np.uint8)
        rc.tick(engs, to, n_new, K, sender_ticks=True, one_launch="tick", down=down, resend=True)
        dumps = [(e.dump(), e.dump_votes()) for e in engs]
        for (g0, n), oc in zip(sl, orcs):
            rc.tick(oc, np.ascontiguousarray(to[:, g0:g0 + n]), np.ascontiguousarray(n_new[:, g0:g0 + n]), K, sender_ticks=True, down=down, resend=True)
            for r in range(R):
                for part, want in zip(dumps[r], (oc[r].dump(), oc[r].dump_votes())):
                    got = tb._cut(part, G, g0, n)
                    for k, v in want.items():
                        assert np.array_equal(got[k].astype(np.uint64), v.astype(np.uint64)), (t, g0, r, k)
    ln = np.concatenate([np.stack([o.dump()["log_len"] for o in oc]).max(axis=0) for oc in orcs])
    ct = np.concatenate([np.stack([o.dump()["curr_term"] for o in oc]).max(axis=0) for oc in orcs])
    assert ln.min() > W and (ct == 2).any() and (ct == 1).any(), (int(ln.min()), W)
    return int(ln.max())


# ---- on the device ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("term0", sorted(WIDE))
def test_wide_terms_closed_loop(cuda, oracle, term0):
    run_wide_terms(cuda, oracle, term0, G=1000)
    run_wide_terms(cuda, oracle, term0, G=600, arms=("calls", "many"), order="senders")


@pytest.mark.parametrize("term0", sorted(WIDE))
def test_wide_terms_leader_follower_and_wire(cuda, oracle, term0):
    run_wide_terms_leader(cuda, oracle, term0, G=1000)
    run_wide_terms_follower(cuda, oracle, term0, G=777)
    assert run_wide_terms_wire(cuda, oracle, term0, G=300) > 0


@pytest.mark.parametrize("W", [16, 8])
def test_closed_loop_past_the_ring(cuda, oracle, W):
    run_past_the_ring(cuda, oracle, G=1000, W=W)
    run_past_the_ring(cuda, oracle, G=600, W=W, arms=("calls", "many"), order="senders")


def test_closed_loop_short_logs_never_reach_the_ring_guard(cuda, oracle):
    run_past_the_ring(cuda, oracle, G=600, W=64, T=10, n_new_max=3, outages=False)


def test_closed_loop_outages(cuda, oracle):
    run_outages(cuda, oracle, G=1000)
    run_outages(cuda, oracle, G=600, arms=("calls", "many"), order="senders")


def test_closed_loop_outages_and_loss(cuda, oracle):
    run_outages(cuda, oracle, G=1000, arms=("calls",), loss=0.1)
    run_outages(cuda, oracle, G=1000, arms=("calls",), loss=0.1, order="receivers")


def test_leader_deep_conflicts(cuda, oracle):
    run_deep_conflicts(cuda, oracle, G=1000)


@pytest.mark.parametrize("K", [1, 2, 8])
def test_closed_loop_message_capacity(cuda, oracle, K):
    run_small_messages(cuda, oracle, G=1000, K=K)


def test_closed_loop_empty_messages(cuda, oracle):
    run_empty_messages(cuda, oracle, G=600)
    run_empty_messages(cuda, oracle, G=600, arms=("calls", "many"), order="senders")


@pytest.mark.parametrize("R", [3, 4, 6, 8])
def test_one_launch_populations_and_follower_lists(cuda, oracle, R):
    run_populations(cuda, oracle, R, G=600)
    run_one_launch_shapes(cuda, oracle, G=200, R=R, T=18)


@pytest.mark.parametrize("G", [1, 63, 64, 65, 600])
def test_one_launch_group_counts(cuda, oracle, G):
    run_one_launch_shapes(cuda, oracle, G=G, T=48 if G == 1 else 16)
    run_populations(cuda, oracle, 5, G=G)
    run_populations(cuda, oracle, 8, G=G)


def test_cluster_tick_argument_errors(cuda):
    run_cluster_tick_argument_errors(cuda)


def test_config2_cluster_tick_at_size(cuda, oracle):
    run_config2_cluster(cuda, oracle)
