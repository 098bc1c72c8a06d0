"""A lock-step RSPaxos tick with the client batches' Accept phase LAST, for the payload stores' one-call byte path
(`put_follow_all`, csrc/rsp_payload.hip) through leader changes.  summerset_amd/rsp_cluster.py's `tick` sends the client
batches' Accepts before the Prepare phase; here every other phase runs first, so that per sender the followers' handlers of
its ONE Accept broadcast are followed by a single byte-path hook `(s, acc, followers)` before anything reads the leader's row:
  1. HearTimeouts -> become_a_leader
  2. step-up Heartbeats and the replies to them
  3. Prepares -> PrepareReply batches (the quorum's re-Accept lists are kept)
  4. Reconstruct reads and their replies, then the Heartbeat the new leader injects behind them
  5. the re-Accept lists, per handler (a payload replica follows after each, `sel` = the sender)
  6. per sender s: its client batches' `req_batch` on the bare engine, each follower's `accept` on the bare engine, the hook,
     then the leader's `accept_replies` (a payload replica's store follows it)
  7. every `hb_every` ticks: the leaders' periodic Heartbeats and the replies
The hook may take at most one sender per call and a follower's store must not follow while its engine holds an unput batch, so
`tick` asserts on every call that at most one replica returns a non-empty client Accept list and that no list is longer than one
entry; `inputs` moves leadership in ALL groups at once (replica 1 times out on 0 at T/3, replica 2 on 1 at 2T/3)."""
import numpy as np

import rsp_cluster as rc
from summerset_amd.rsp_cluster import _deliver_accepts, _deliver_heartbeat, _lost

NULL, NO_REP = rc.NULL, rc.NO_REP
KINDS = ("accept", "accept_reply", "prepare", "prepare_reply", "recon", "recon_reply", "hb")


class PayloadEngine(rc.NumpyEngine):
    """NumpyEngine around an RSPaxosReplicaWithPayload; `bare(name)` is the same handler on the bare engine: no store follows"""

    def bare(self, name):
        fn = getattr(self.e.replica, name)

        def call(*a, **kw):
            out = fn(*[self._t(x) for x in a], **{k: self._t(v) for k, v in kw.items()})
            self._polls.append(self.e.replica.exec_poll())
            return None if out is None else self._n(out)
        return call


def _bare(rep, name):
    return rep.bare(name) if hasattr(rep, "bare") else getattr(rep, name)


def inputs(G, ticks, seed, loss, R=5):
    """per tick: (t, val [G], target [G], timeouts or None, drop or None, heartbeat) -- every message kind lost at `loss`"""
    rng = np.random.default_rng(seed)
    target = np.zeros(G, np.uint8)
    g = np.arange(G)
    for t in range(ticks):
        val = (1 + t * G + g).astype(np.uint32)
        val[rng.random(G) < 0.1] = NULL                          # no batch in this group this tick
        to = None
        if t == ticks // 3 or t == 2 * ticks // 3:               # replica 1 suspects 0, later replica 2 suspects 1: in every group
            r = 1 if t == ticks // 3 else 2
            to = [np.full(G, NO_REP, np.uint8) for _ in range(R)]
            to[r][:] = r - 1
        if t == ticks // 3 + 1:
            target = np.full(G, 1, np.uint8)
        if t == 2 * ticks // 3 + 1:
            target = np.full(G, 2, np.uint8)
        drop = None
        if loss:
            drop = {(k, s, q): rng.random(G) < loss for k in KINDS for s in range(R) for q in range(R) if s != q}
        yield t, val, target, to, drop, t % 3 == 2


def tick(reps, val, target, timeouts=None, drop=None, heartbeat=False, hook=None, stats=None):
    """one tick (see the module's docstring).  hook(s, acc, followers): the byte path behind sender s's client Accepts (acc: its
    req_batch output, numpy); stats (dict, optional): what the tick covered, counted from the engines' dumps around the Accepts.
    Returns the tick's log, as rsp_cluster.tick's."""
    R, G = len(reps), len(val)
    W = reps[0].W
    log = []
    u8 = lambda v: np.full(G, v, np.uint8)
    # 1. HearTimeouts
    bl = [reps[r].become_leader(timeouts[r] if timeouts is not None else u8(NO_REP)) for r in range(R)]
    # 2. step-up heartbeats
    for s in range(R):
        if bl[s]["hb_flags"].any():
            _deliver_heartbeat(reps, s, bl[s]["hb_flags"], bl[s]["hb_ballot"], bl[s]["hb_commit"], bl[s]["hb_exec"], bl[s]["hb_snap"], drop)
    # 3. Prepare phase
    late = []
    for s in range(R):
        if not bl[s]["p_flags"].any():
            continue
        for q in range(R):
            if q == s:
                continue
            fl = (bl[s]["p_flags"] & ~_lost(drop, "prepare", s, q, G)).astype(np.uint8)
            pr = reps[q].prepare(flags=fl, peer=u8(s), trig=bl[s]["p_trig"], ballot=bl[s]["p_ballot"])
            n = np.where(_lost(drop, "prepare_reply", q, s, G), 0, pr["pr_n"]).astype(np.uint32)
            if n.any():
                log.append(dict(kind="prepare_reply", s=s, q=q, rows=int(n.sum()), voted=int((pr["pr_vbal"] > 0).sum())))
                late.append((s, reps[s].prepare_replies(peer=u8(q), pr_n=n, pr_trig=pr["pr_trig"], pr_endp=pr["pr_endp"],
                                                        pr_ballot=pr["pr_ballot"], pr_vbal=pr["pr_vbal"], pr_vval=pr["pr_vval"],
                                                        pr_vmask=pr["pr_vmask"])))
    # 4. reconstruction reads, then the heartbeat the new leader injects behind them (leadership.rs:173-183)
    for s in range(R):
        if not bl[s]["rc_n"].any():
            continue
        for q in range(R):
            if q == s:
                continue
            fl = ((bl[s]["rc_n"] > 0) & ~_lost(drop, "recon", s, q, G)).astype(np.uint8)
            rr = reps[q].reconstruct(flags=fl, rc_n=bl[s]["rc_n"], rc_slot=bl[s]["rc_slot"])
            fl2 = ((rr["rr_n"] > 0) & ~_lost(drop, "recon_reply", q, s, G)).astype(np.uint8)
            if fl2.any():
                log.append(dict(kind="recon_reply", s=s, q=q, rows=int(rr["rr_n"][fl2.astype(bool)].sum())))
                reps[s].reconstruct_reply(flags=fl2, **rr)
        _deliver_heartbeat(reps, s, (bl[s]["rc_n"] > 0).astype(np.uint8), bl[s]["p_ballot"], bl[s]["hb_commit"], bl[s]["hb_exec"],
                           bl[s]["hb_snap"], drop)
    # 5. the Prepare quorum's re-Accepts, per handler
    for s, a in late:
        if a["a_n"].any():
            log.append(dict(kind="re_accept", s=s, n=int(a["a_n"].sum()),
                            empty=int(((a["a_val"] == 0) & (np.arange(len(a["a_val"]))[:, None] < a["a_n"][None, :])).sum())))
        _deliver_accepts(reps, s, a, drop, log)
    # 6. the client batches: per sender req_batch, the followers' Accepts, the byte path, the leader's tally
    senders = 0
    for s in range(R):
        acc = _bare(reps[s], "req_batch")(np.where(target == s, val, NULL).astype(np.uint32))
        if not acc["a_n"].any():
            continue
        senders += 1
        assert senders == 1, "two replicas sent client Accepts in one tick"
        assert int(acc["a_n"].max()) == 1, ("a client Accept list longer than one entry", int(acc["a_n"].max()))
        live = acc["a_n"] > 0
        slot, tok = np.ascontiguousarray(acc["a_slot"][0]), np.ascontiguousarray(acc["a_val"][0])
        row, gi = (slot & (W - 1)).astype(np.int64), np.arange(G)
        ballot, flags = np.zeros((R, G), np.uint64), np.zeros((R, G), np.uint8)
        followers = [q for q in range(R) if q != s]
        for q in followers:
            lost = _lost(drop, "accept", s, q, G)
            if stats is not None:                                # the follower's row before: another live token's shards?
                d = reps[q].dump()
                other = (d["s_val"][row, gi] != NULL) & (d["s_val"][row, gi] != tok) & (d["s_mask"][row, gi] != 0)
                stats["lost_onto_other"] = stats.get("lost_onto_other", 0) + int((live & lost & other).sum())
            fl = (live & ~lost).astype(np.uint8)
            ar = _bare(reps[q], "accept")(flags=fl, peer=u8(s), slot=slot, ballot=acc["a_ballot"], val=tok, mask=u8(1 << q))
            if stats is not None:                                # reached the follower, and its engine did not take shard q of tok
                d = reps[q].dump()
                took = (d["s_val"][row, gi] == tok) & (((d["s_mask"][row, gi] >> q) & 1) != 0)
                stats["not_taken"] = stats.get("not_taken", 0) + int((live & ~lost & ~took).sum())
            got = (ar["r_ballot"] != 0) & ~_lost(drop, "accept_reply", q, s, G)
            flags[q] = got.astype(np.uint8); ballot[q] = ar["r_ballot"]
        if hook is not None:
            hook(s, acc, followers)
        res = reps[s].accept_replies(slot=slot, ballot=ballot, flags=flags)
        log.append(dict(kind="commit", s=s, slot=slot, val=tok, committed=res["committed"] & live.astype(np.uint8)))
    # 7. periodic heartbeats of the replicas that lead
    if heartbeat:
        leaders = [reps[r].is_leader() for r in range(R)]
        for s in range(R):
            if not leaders[s].any():
                continue
            hb = reps[s].bcast_heartbeat(leaders[s])
            _deliver_heartbeat(reps, s, leaders[s], hb["ballot"], hb["commit_bar"], hb["exec_bar"], hb["snap_bar"], drop)
    return log
