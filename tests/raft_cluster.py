"""Closed-loop Raft cluster out of R per-replica handler objects (backend-agnostic: RaftOracle or the
HIP RaftLeaderGroup behind a numpy adapter).  One tick: HearTimeouts -> RequestVote round -> vote
replies; client batches at whoever leads; the AppendEntries those appends produce (one combined
message per leader and follower) -> replies -> the leader's match-index quorum.  `tick` loses nothing unless told to: `down`
(replicas nobody reaches this tick) and `drop` (single groups' messages); `run_closed_loop` drives engine clusters and an oracle
cluster side by side through a schedule and compares everything every tick; `Outages` is such a schedule."""
import numpy as np

NO, NONE32 = 0xFF, 0xFFFFFFFF
FOLLOWER, CANDIDATE, LEADER = 0, 1, 2


class NumpyRaft:
    """RaftLeaderGroup (device tensors) behind the RaftOracle-style numpy interface"""

    def __init__(self, eng, cuda):
        import torch
        self.e, self.cuda, self.torch = eng, cuda, torch
        self.G, self.R = eng.G, eng.R

    def _t(self, a):
        if a is None:
            return None
        v = a.view(np.int64) if a.dtype == np.uint64 else (a.view(np.int32) if a.dtype == np.uint32 else a)
        return self.torch.from_numpy(np.ascontiguousarray(v)).to(self.cuda)

    @staticmethod
    def _n(d, like):
        return {k: d[k].cpu().numpy().view(v) for k, v in like.items()}

    def preset(self, *a):
        self.e.preset(*a)

    def become_candidate(self, src):
        return self._n(self.e.become_a_candidate(self._t(src)), dict(flags=np.uint8, term=np.uint64, last_slot=np.uint32,
                                                                  last_term=np.uint64))

    def handle_request_vote(self, flags, candidate, term, last_slot, last_term):
        o = self.e.handle_msg_request_vote(self._t(flags), self._t(candidate), self._t(term), self._t(last_slot),
                                           self._t(last_term))
        return self._n(o, dict(flags=np.uint8, term=np.uint64))

    def handle_vote_replies(self, term, flags, order=None):
        o = self.e.handle_msg_request_vote_reply(self._t(term), self._t(flags), self._t(order))
        return self._n(o, dict(hb_prev_slot=np.uint32, elected=np.uint8))

    def append_emit(self, n_new):
        return self.e.handle_req_batch_emit(self._t(n_new)).cpu().numpy().view(np.uint32)

    def gather_entries(self, first, K):
        o = self.e.gather_entries(self._t(np.ascontiguousarray(first)), K)
        return self._n(o, dict(flags=np.uint8, leader=np.uint8, term=np.uint64, prev_slot=np.uint32, prev_term=np.uint64,
                               n_entries=np.uint32, entry_term=np.uint64, leader_commit=np.uint32, last_snap=np.uint32))

    def handle_append_entries(self, **m):
        o = self.e.handle_msg_append_entries(**{k: self._t(v) for k, v in m.items()})
        return self._n(o, dict(flags=np.uint8, term=np.uint64, end_slot=np.uint32, conflict_term=np.uint64,
                               conflict_slot=np.uint32))

    def replicate_many(self, followers, firsts, K):
        """my AppendEntries for `followers` (NumpyRaft objects) and their handlers in one launch; returns [(message, reply)] as numpy"""
        torch, dev, G = self.torch, self.cuda, self.G
        msgs = [self.e.new_message(K, dev) for _ in followers]
        z = lambda dt: torch.zeros(G, dtype=dt, device=dev)
        reps = [dict(flags=z(torch.uint8), term=z(torch.int64), end_slot=z(torch.int32), conflict_term=z(torch.int64), conflict_slot=z(torch.int32))
                for _ in followers]
        self.e.replicate_many([f.e for f in followers], [self._t(np.ascontiguousarray(f)) for f in firsts], msgs, reps)
        ml = dict(flags=np.uint8, leader=np.uint8, term=np.uint64, prev_slot=np.uint32, prev_term=np.uint64, n_entries=np.uint32,
                  entry_term=np.uint64, leader_commit=np.uint32, last_snap=np.uint32)
        rl = dict(flags=np.uint8, term=np.uint64, end_slot=np.uint32, conflict_term=np.uint64, conflict_slot=np.uint32)
        return [(self._n(m, ml), self._n(r, rl)) for m, r in zip(msgs, reps)]

    def cluster_tick(self, n_new, followers, K):
        """my append + my AppendEntries for `followers` + their handlers + my reply handler in ONE launch (`smr_raft_cluster_tick`);
        returns (first [R][G], [(message, reply)]) as numpy"""
        torch, dev, G, R = self.torch, self.cuda, self.G, self.R
        msgs = [self.e.new_message(K, dev) for _ in followers]
        z = lambda dt: torch.zeros((R, G), dtype=dt, device=dev)
        arr = dict(flags=z(torch.uint8), term=z(torch.int64), end_slot=z(torch.int32), conflict_term=z(torch.int64), conflict_slot=z(torch.int32))
        first = torch.zeros((R, G), dtype=torch.int32, device=dev)
        reps = [{k: v[f.e.me] for k, v in arr.items()} for f in followers]
        self.e.cluster_tick(self._t(np.ascontiguousarray(n_new)), first, [f.e for f in followers], msgs, reps, arr["term"], arr["end_slot"], arr["flags"],
                            arr["conflict_term"], arr["conflict_slot"])
        ml = dict(flags=np.uint8, leader=np.uint8, term=np.uint64, prev_slot=np.uint32, prev_term=np.uint64, n_entries=np.uint32,
                  entry_term=np.uint64, leader_commit=np.uint32, last_snap=np.uint32)
        rl = dict(flags=np.uint8, term=np.uint64, end_slot=np.uint32, conflict_term=np.uint64, conflict_slot=np.uint32)
        return first.cpu().numpy().view(np.uint32), [(self._n(m, ml), self._n(r, rl)) for m, r in zip(msgs, reps)]

    def handle_replies(self, reply_term, end_slot, flags, conflict_term=None, conflict_slot=None, order=None):
        self.e.handle_msg_append_entries_reply(self._t(reply_term), self._t(end_slot), self._t(flags), self._t(conflict_term),
                                               self._t(conflict_slot), self._t(order))

    def dump(self):
        return self.e.dump()

    def total_commits(self):
        return self.e.total_commits()

    def ring_guard_hits(self):
        return self.e.ring_guard_hits()

    def dump_votes(self):
        return self.e.dump_votes()


def _lose(x, mask):
    """the message / reply `x` without the groups of `mask` (flag 0: nothing arrives)"""
    if mask is None:
        return x
    y = dict(x)
    y["flags"] = np.where(mask, 0, x["flags"]).astype(np.uint8)
    return y


def tick(reps, timeouts, n_new, K, via=None, sender_major=False, one_launch=False, seen=None, sender_ticks=False, down=(), drop=None, resend=False):
    """timeouts[r][G]: HearTimeout source at replica r (0xFF none); n_new[r][G]: client batches handed to
    replica r (those that do not lead redirect them).  Returns nothing; state lives in the replicas.
    sender_major: the replication step goes sender by sender (every follower handles sender 0's message, then sender 1's ..)
    instead of receiver by receiver -- the order in which `one_launch` (NumpyRaft.replicate_many: a sender's messages and their
    handlers in one launch) can stand for the calls; seen (a list): the (sender, receiver, message, reply) tuples of the step.
    sender_ticks: a sender's append, replication and replies before the next sender's append -- the order in which `one_launch="tick"`
    (NumpyRaft.cluster_tick: all three in one launch) can stand for the calls.
    via (optional): via(s, rt, es, fl, ct, cs) -> the same five [R][G] arrays -- the AppendEntriesReplies on their way to
    leader s (tests/test_zz_reply_ingest_gpu.py sends them as frames through the device parser).
    down: replicas nobody reaches this tick -- they take no step (no timer, no vote, no append) and are left out of every sender's
    follower list (the one launch then runs with fewer than R - 1 followers; a sender with none left only appends); their reply
    rows at the senders stay zero (flag 0: no reply).
    drop (call-by-call arms only): drop[(a, b)] = bool [G], the groups whose traffic from a to b is lost this tick -- an
    AppendEntries of a for b (its flag cleared before b's handler sees it) or a's reply to an AppendEntries of b.
    resend: before a sender's own step it sends again to every reachable follower whose match index is behind its log (a reply was
    a conflict, a message or its reply was lost, the follower was away, or the sender has just been elected): one more
    AppendEntries from that follower's next_slot (at most the last entry: a duplicate is legal), and the replies handled.  What the
    reference's leader does on a conflict reply (messages.rs:335-384) and on its heartbeat timer; without it a follower that has
    missed an entry never catches up in this loop, the leader's last_snap stops and its ring fills for good.  Goes through
    `replicate_many` with `one_launch`, through the calls without."""
    R = len(reps)
    G = timeouts.shape[1]
    up = [r for r in range(R) if r not in down]
    assert drop is None or not one_launch, "the one launch gathers and handles in one lane: it cannot lose one group's message"
    lost = lambda a, b: None if drop is None else drop.get((a, b))
    u8 = lambda v: np.full(G, v, np.uint8)
    # elections
    rv = {r: reps[r].become_candidate(np.ascontiguousarray(timeouts[r])) for r in up}
    vote = {}
    for q in up:
        for c in up:
            if c == q:
                continue
            vote[(q, c)] = reps[q].handle_request_vote(rv[c]["flags"], u8(c), rv[c]["term"], rv[c]["last_slot"],
                                                       rv[c]["last_term"])
    for c in up:
        term = np.zeros((R, G), np.uint64); flags = np.zeros((R, G), np.uint8)
        for q in up:
            if q != c:
                term[q] = vote[(q, c)]["term"]; flags[q] = vote[(q, c)]["flags"] & 1
        reps[c].handle_vote_replies(term, flags)

    def exchange(s, q, first):                                  # s's AppendEntries for q and q's reply, call by call
        m = _lose(reps[s].gather_entries(first, K), lost(s, q))
        return m, _lose(reps[q].handle_append_entries(**m), lost(q, s))

    def deliver(s, got, via=None):                              # got[q] = q's reply to s
        rt = np.zeros((R, G), np.uint64); es = np.zeros((R, G), np.uint32); fl = np.zeros((R, G), np.uint8)
        ct = np.zeros((R, G), np.uint64); cs = np.zeros((R, G), np.uint32)
        for q, r_ in got.items():
            rt[q] = r_["term"]; es[q] = r_["end_slot"]; fl[q] = r_["flags"]; ct[q] = r_["conflict_term"]; cs[q] = r_["conflict_slot"]
        if via is not None:
            rt, es, fl, ct, cs = via(s, rt, es, fl, ct, cs)
        reps[s].handle_replies(rt, es, fl, ct, cs)

    def catch_up(s):
        qs = [q for q in up if q != s]
        if not resend or not qs:
            return
        d = reps[s].dump()
        ln = d["log_len"].astype(np.int64)
        firsts = []
        for q in qs:
            behind = (d["role"] == LEADER) & (ln >= 2) & (d["match_slot"][q] + 1 < ln)
            firsts.append(np.where(behind, np.clip(d["next_slot"][q], 1, np.maximum(ln - 1, 1)), NONE32).astype(np.uint32))
        if not any((f != NONE32).any() for f in firsts):
            return
        if one_launch:
            out = reps[s].replicate_many([reps[q] for q in qs], firsts, K)
        else:
            out = [exchange(s, q, f) for q, f in zip(qs, firsts)]
        deliver(s, {q: r_ for q, (m, r_) in zip(qs, out)})
        if seen is not None:
            for q, (m, r_) in zip(qs, out):
                seen.append((s, q, m, r_))
    # replication
    if sender_ticks:                    # sender by sender, each its WHOLE tick: append, AppendEntries + handlers, replies
        for s in up:
            catch_up(s)
            qs = [q for q in up if q != s]
            if not qs:
                reps[s].append_emit(np.ascontiguousarray(n_new[s]))
                continue
            if one_launch == "tick":
                _, out = reps[s].cluster_tick(n_new[s], [reps[q] for q in qs], K)
            else:
                f = reps[s].append_emit(np.ascontiguousarray(n_new[s]))
                out = [exchange(s, q, f[q]) for q in qs]
                deliver(s, {q: r_ for q, (m, r_) in zip(qs, out)})
            if seen is not None:
                for q, (m, r_) in zip(qs, out):
                    seen.append((s, q, m, r_))
        return
    for s in up:
        catch_up(s)
    first = {r: reps[r].append_emit(np.ascontiguousarray(n_new[r])) for r in up}
    rep = {}
    if sender_major:
        for s in up:
            qs = [q for q in up if q != s]
            if not qs:
                continue
            if one_launch:
                out = reps[s].replicate_many([reps[q] for q in qs], [first[s][q] for q in qs], K)
            else:
                out = [exchange(s, q, first[s][q]) for q in qs]
            for q, (m, r) in zip(qs, out):
                rep[(q, s)] = r
                if seen is not None:
                    seen.append((s, q, m, r))
    for q in up if not sender_major else ():
        for s in up:
            if s == q:
                continue
            m, rep[(q, s)] = exchange(s, q, first[s][q])
            if seen is not None:
                seen.append((s, q, m, rep[(q, s)]))
    for s in up:
        deliver(s, {q: rep[(q, s)] for q in up if q != s}, via)


class Outages:
    """A schedule for `run_closed_loop`, computed tick by tick from the ORACLE cluster's state (the engine clusters are held
    equal to it): whole replicas down for windows of ticks, per-group loss, appends at every replica, and timers that fire
    where they would: in a group without an effective leader (no reachable replica that leads in the highest reachable term)
    one reachable follower times out on whoever it believes leads -- the first in a rotation that moves with the group and the
    tick, so that a candidate that loses (shorter log, no quorum) is followed by another.  `lonely[t] = r`: replica r's timers
    fire at tick t in every group it follows, whether its leader lives or not (a replica that comes back and stands with a
    term above the leader's)."""

    def __init__(self, R, G, seed, windows=(), lonely=None, loss=0.0, n_new_max=3):
        self.R, self.G, self.windows, self.lonely, self.loss, self.n_new_max = R, G, tuple(windows), dict(lonely or {}), loss, n_new_max
        self.rng = np.random.default_rng(seed)

    def down_at(self, t):
        return tuple(sorted({r for t0, t1, rs in self.windows if t0 <= t < t1 for r in rs}))

    @property
    def last_outage_end(self):
        return max([t1 for _, t1, _ in self.windows] + [0])

    def __call__(self, t, dumps):
        R, G, rng = self.R, self.G, self.rng
        down = self.down_at(t)
        upm = np.array([r not in down for r in range(R)])
        role = np.stack([d["role"] for d in dumps]); term = np.stack([d["curr_term"] for d in dumps]); lead = np.stack([d["leader"] for d in dumps])
        src = np.where(lead == NO, 0xFE, lead).astype(np.uint8)
        tmax = np.where(upm[:, None], term, 0).max(axis=0)
        led = ((role == LEADER) & (term == tmax[None, :]) & upm[:, None]).any(axis=0)
        to = np.full((R, G), NO, np.uint8)
        g = np.arange(G)
        open_ = ~led
        for k in range(R):
            c = (g + t + k) % R
            ok = open_ & upm[c] & (role[c, g] == FOLLOWER)
            to[c[ok], g[ok]] = src[c[ok], g[ok]]
            open_ &= ~ok
        r = self.lonely.get(t)
        if r is not None and upm[r]:
            ok = role[r] == FOLLOWER
            to[r, ok] = src[r, ok]
        n_new = rng.integers(0, self.n_new_max + 1, (R, G)).astype(np.uint32)
        drop = {(a, b): rng.random(G) < self.loss for a in range(R) for b in range(R) if a != b} if self.loss else None
        return to, n_new, down, drop


def _cover(st, t, before, after, seen, to, down):
    """what the ORACLE cluster's tick t reached (its dumps around the tick, the messages it exchanged)"""
    R = len(before)
    quiet = (to == NO).all(axis=0)                                  # groups where nobody's timer fired: roles as `before` until a message
    stepped = [np.zeros(len(quiet), bool) for _ in range(R)]
    for s, q, m, r in seen:                                         # (in the order they were exchanged)
        on = m["flags"] != 0
        st["n_msg"] += int(on.sum())
        st["n_entries_max"] = max(st["n_entries_max"], int(m["n_entries"][on].max()) if on.any() else 0)
        conf = (r["flags"] & 2) != 0
        if conf.any():
            st["conflicts"][q] = st["conflicts"].get(q, 0) + int(conf.sum())
        # a replica that still leads handles an AppendEntries of a later term (messages.rs:32)
        by_ae = on & quiet & (before[q]["role"] == LEADER) & ~stepped[q] & (m["term"] > before[q]["curr_term"])
        st["stepdown_by_append_entries"] += int(by_ae.sum())
        stepped[q] |= by_ae
        # the sender leads in m.term; a reply of a later term makes it a follower (leadership.rs:16-72, messages.rs:231)
        by_reply = on & ~stepped[s] & ((r["flags"] & 1) != 0) & (r["term"] > m["term"])
        st["stepdown_by_reply"] += int(by_reply.sum())
        stepped[s] |= by_reply
    for r in range(R):
        b, a = before[r], after[r]
        same = (b["role"] == LEADER) & (a["role"] == LEADER) & (b["curr_term"] == a["curr_term"])
        st["next_slot_back"] += int((same[None, :] & (a["next_slot"] < b["next_slot"])).sum())
        if same.any():
            st["next_slot_back_max"] = max(st["next_slot_back_max"], int(np.where(same[None, :], b["next_slot"].astype(np.int64) - a["next_slot"], 0).max()))
        st["elected"] += int(((b["role"] != LEADER) & (a["role"] == LEADER)).sum())
    for r in st["was_down"]:                                        # how far behind the longest log a replica comes back
        if r not in down:
            st["behind_max"] = max(st["behind_max"], int((np.stack([d["log_len"] for d in before]).max(axis=0) - before[r]["log_len"]).max()))
    st["was_down"] = tuple(down)
    st["followers"].add(R - 1 - len(down) if len(down) < R else 0)
    st["commits"].append(np.stack([d["last_commit"] for d in after]))
    st["commit"].append(st["commits"][-1].max(axis=0))
    st["len"].append(np.stack([d["log_len"] for d in after]).max(axis=0))


ARMS = {"calls": False, "tick": "tick", "many": True}


def run_closed_loop(dev, oracle, G, R, W, K, T, schedule, term0=0, arms=("calls", "tick"), info=None, resend=True, order=None):
    """engine clusters (`arms`: "calls" = handler by handler, "tick" = `smr_raft_cluster_tick`, "many" =
    `smr_raft_cluster_replicate`; none: the oracles alone, to tune a schedule) and an oracle cluster from
    `preset(FOLLOWER, none, term0)` through T ticks of `schedule(t, oracle dumps) -> (timeouts, n_new, down, drop)`, in the order
    the arms can share (`order`: "ticks" = a sender's whole tick at a time, what "tick" needs; "senders" = sender by sender, what
    "many" needs; else "receivers").
    Every tick: every message and reply of every arm against the oracle's, every replica's dump(), dump_votes(),
    total_commits() and ring_guard_hits().  Returns what the oracle cluster covered (`_cover`, the final dumps, counters)."""
    order = order or ("ticks" if "tick" in arms else "senders" if "many" in arms else "receivers")
    assert order == "ticks" or "tick" not in arms
    mode = dict(sender_ticks=order == "ticks", sender_major=order == "senders", resend=resend)
    sets = []
    if arms:
        from summerset_amd import RaftLeaderGroup
        sets = [(a, [NumpyRaft(RaftLeaderGroup(G, R, leader_id=r, window=W, term=1), dev) for r in range(R)]) for a in arms]
    orcs = [oracle.RaftOracle(G, R, W, leader_id=r, term=1) for r in range(R)]
    for x in [x for _, s in sets for x in s] + orcs:
        x.preset(FOLLOWER, NO, term0)
    st = dict(n_msg=0, n_entries_max=0, conflicts={}, stepdown_by_reply=0, stepdown_by_append_entries=0, next_slot_back=0,
              next_slot_back_max=0, elected=0, followers=set(), commit=[], commits=[], len=[], behind_max=0, was_down=())
    dumps = [o.dump() for o in orcs]
    for t in range(T):
        to, n_new, down, drop = schedule(t, dumps)
        seen = []
        tick(orcs, to, n_new, K, seen=seen, down=down, drop=drop, **mode)
        after = [o.dump() for o in orcs]
        _cover(st, t, dumps, after, seen, to, down)
        votes = [o.dump_votes() for o in orcs]
        for name, reps in sets:
            sn = []
            tick(reps, to, n_new, K, one_launch=ARMS[name], seen=sn, down=down, drop=drop, **mode)
            assert len(sn) == len(seen), (t, name)
            for (s, q, m1, r1), (s2, q2, m2, r2) in zip(sn, seen):
                assert (s, q) == (s2, q2)
                on = m2["flags"] != 0                                         # (a message's other fields mean something where one is sent)
                for k in m2:
                    sel = (slice(None), on) if k == "entry_term" else slice(None) if k == "flags" else on
                    assert np.array_equal(np.asarray(m1[k])[sel].astype(np.uint64), np.asarray(m2[k])[sel].astype(np.uint64)), (t, name, "message", s, q, k)
                for k in r2:
                    assert np.array_equal(r1[k].astype(np.uint64), r2[k].astype(np.uint64)), (t, name, "reply", s, q, k)
            for r in range(R):
                a = reps[r].dump()
                for n, v in after[r].items():
                    assert np.array_equal(a[n], v), (t, name, r, n, np.nonzero(a[n] != v))
                va = reps[r].dump_votes()
                for n, v in votes[r].items():
                    assert np.array_equal(va[n].astype(np.uint64), v.astype(np.uint64)), (t, name, r, n)
                assert reps[r].total_commits() == orcs[r].total_commits(), (t, name, r, "total_commits")
                assert reps[r].ring_guard_hits() == orcs[r].ring_guard_hits(), (t, name, r, "ring_guard_hits")
        dumps = after
    st.update(dumps=dumps, votes=[o.dump_votes() for o in orcs], counters=[o.counters() for o in orcs],
              ring_guard_hits=[o.ring_guard_hits() for o in orcs], total_commits=[o.total_commits() for o in orcs])
    if info is not None:
        info.update(st)
    return st
