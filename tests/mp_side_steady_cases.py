"""The side launch's block-cooperative steady step (mp_engine.hip: side_steady_tick, `SMR_MP_SIDE_STEADY`): the cases.

Run on the kernel-source emulator by tests/test_mp_side_steady.py and on the device by tests/test_zzzz_mp_side_steady_gpu.py.
Every case drives the engine through `run_ticks` with the straggler list on and compares the full canonical state of every
replica with the CPU oracle after every `run_ticks` call (tests/test_mp_gpu.py's `_compare`: bit-exact, no tolerance), the
commit lists and the counters with it.  The tick inputs are written here, not by `stream.MultiPaxosStream`, because the cases
need what that stream does not do: a timeout in a chosen tick, requests that follow the leader the ORACLE reports, requests to
a follower, ticks without requests, empty batches.

`straggler_ticks` (ttl): 0xFF is the C-ABI's "list off" (SMR_STRAGGLER_OFF) -- `run_ticks` then has no side launch at all; the
longest listing is 0xFE.  The cases that count steps list with 0xFE; 0xFF is run as the list-off arm of the shape sweep."""
import contextlib
import os

import numpy as np

ENV = "SMR_MP_SIDE_STEADY"
NO_REP = 0xFF
LIST_FOREVER = 0xFE


@contextlib.contextmanager
def switch(on):
    """the environment as smr_mp_cluster_create reads it: the step on (the default: variable unset) or off ("0")"""
    old = os.environ.get(ENV)
    if on:
        os.environ.pop(ENV, None)
    else:
        os.environ[ENV] = "0"
    try:
        yield
    finally:
        if old is None:
            os.environ.pop(ENV, None)
        else:
            os.environ[ENV] = old


def _tokens(seed, t, S, G):
    from summerset_amd import stream
    k = np.arange(S, dtype=np.uint64)[:, None]
    g = np.arange(G, dtype=np.uint64)[None, :]
    return ((stream._key(seed, 0x70CE, t, k, g) & np.uint64(0x7FFFFFFF)) | np.uint64(1)).astype(np.uint32)


class Run:
    """one oracle, one or two engines (the step on / off) on the same inputs"""

    def __init__(self, cuda, oracle, G, R, S, W, ttl, hb_every, win_reserve=None, drop_p=0.0, max_drop=None, seed=0x51DE,
                 arms=(True,), cap=None):
        from summerset_amd import MultiPaxosCluster
        self.cuda, self.G, self.R, self.S, self.W, self.hb_every = cuda, G, R, S, W, hb_every
        self.drop_p, self.max_drop, self.seed = drop_p, max_drop, seed
        self.cap = W + 4 if cap is None else cap
        self.clist_cap = G * (S * 4 * 16 + W) + 64
        self.engs = {}
        for on in arms:
            with switch(on):
                self.engs[on] = MultiPaxosCluster(G, R, W, win_reserve=win_reserve, outbox_cap=self.cap, commit_list_cap=self.clist_cap,
                                                  straggler_ticks=ttl)
        self.orc = oracle.MpOracle(G, R, W, win_reserve=win_reserve, cap=self.cap)
        for e in self.engs.values():
            e.preset_leader(0)
        self.orc.preset_leader(0)
        self.t = 0
        self.pending = []
        self.og = [[np.zeros(0, np.uint32)] * 2 for _ in range(R)]
        self.total = 0

    def leaders(self):
        """each group's current leader as the oracle reports it (replica 0's view; every replica's once a change is through)"""
        return self.orc.dump(0)["leader"].astype(np.int64)

    def settled(self, groups):
        """the oracle shows every change of `groups` complete: one leader l named by all replicas, every replica's bal_max_seen at
        l's bal_prepared, every log accepted up to l's log end"""
        d = [self.orc.dump(r) for r in range(self.R)]
        ok = np.ones(len(groups), bool)
        l = d[0]["leader"][groups].astype(np.int64)
        ok &= l < self.R
        l = np.minimum(l, self.R - 1)
        bpd = np.stack([x["bal_prepared"][groups] for x in d])[l, np.arange(len(groups))]
        ln = np.stack([x["log_len"][groups] for x in d])[l, np.arange(len(groups))]
        ok &= bpd != 0
        for x in d:
            ok &= (x["leader"][groups] == l) & (x["bal_max_seen"][groups] == bpd) & (x["log_len"][groups] == ln) & (x["accept_bar"][groups] == ln)
        return bool(ok.all())

    def tick(self, timeout_groups=(), target=None, req_cnt=None, req_val=None, no_requests=False):
        """one tick's inputs -> the oracle now, the engines at the next flush().  timeout_groups: a HearTimeout at the replica behind
        the current leader, about that leader.  target / req_cnt / req_val: [G] / [G] / [S][G] overrides"""
        from summerset_amd import stream
        G, R, S, t = self.G, self.R, self.S, self.t
        lead = self.leaders()
        lead = np.where(lead < R, lead, 0)
        inp = dict(ackctl=stream.random_ackctl(self.seed, t, min(self.cap, S + 4), G, R, self.drop_p, cap=self.cap, max_drop=self.max_drop),
                   heartbeat=(t % self.hb_every) == self.hb_every - 1)
        tg = np.asarray(list(timeout_groups), np.int64)
        if len(tg):
            rep = np.full(G, NO_REP, np.uint8)
            src = np.full(G, NO_REP, np.uint8)
            rep[tg] = (lead[tg] + 1) % R
            src[tg] = lead[tg]
            inp.update(timeout_rep=rep, timeout_src=src)
        if not no_requests:
            inp.update(req_target=(lead if target is None else target).astype(np.uint8),
                       req_cnt=np.full(G, S, np.uint32) if req_cnt is None else req_cnt.astype(np.uint32),
                       req_val=np.ascontiguousarray(_tokens(self.seed, t, S, G) if req_val is None else req_val.astype(np.uint32)))
        self.orc.tick(**inp)
        for r in range(R):
            g_, s_ = self.orc.take_commits(r)
            self.og[r] = [np.concatenate([self.og[r][0], g_]), np.concatenate([self.og[r][1], s_])]
        self.pending.append(inp)
        self.t += 1

    def flush(self, compare=True):
        """the pending ticks as ONE run_ticks call on every engine; then every engine against the oracle, and against each other"""
        import test_mp_gpu as T
        if not self.pending:
            return
        for e in self.engs.values():
            e.run_ticks([T._to_dev(p, self.cuda) for p in self.pending])
        self.pending = []
        polled = {}
        for on, e in self.engs.items():
            if compare:
                T._compare(e, self.orc, self.R, self.t - 1)
            polled[on] = [e.poll_commits(r) for r in range(self.R)]
            for r in range(self.R):
                og, os_ = self.og[r]
                eg, es = polled[on][r]
                assert len(og) == len(eg), "tick %d rep %d commit count %d vs %d (step %s)" % (self.t - 1, r, len(eg), len(og), on)
                ko, ke = np.lexsort((np.arange(len(og)), og)), np.argsort(eg, kind="stable")
                assert np.array_equal(og[ko], eg[ke]) and np.array_equal(os_[ko], es[ke]), (self.t - 1, r, on)
                assert e.counters(r)["commits"] == self.orc.total_commits(r), (self.t - 1, r, on)
        self.total += sum(len(self.og[r][0]) for r in range(self.R))
        self.og = [[np.zeros(0, np.uint32)] * 2 for _ in range(self.R)]
        if len(self.engs) == 2:                                    # the engine against itself
            a, b = self.engs[True], self.engs[False]
            for r in range(self.R):
                da, db = a.dump(r), b.dump(r)
                for k in da:
                    assert np.array_equal(da[k], db[k]), "tick %d rep %d %s: step on and off differ" % (self.t - 1, r, k)
                assert a.counters(r) == b.counters(r), (self.t - 1, r)
                assert a.debug_generic_units(r) == b.debug_generic_units(r), (self.t - 1, r)
                for x, y in zip(polled[True][r], polled[False][r]):
                    assert np.array_equal(np.sort(x), np.sort(y)), (self.t - 1, r)

    def run(self, n_ticks, batches, events=None, **kw):
        """n_ticks ticks, flushed in batches of the sizes `batches` gives in turn; events: tick -> kwargs of tick()"""
        events = events or {}
        bi, left = 0, batches[0]
        for _ in range(n_ticks):
            self.tick(**dict(kw, **events.get(self.t, {})))
            left -= 1
            if left == 0:
                self.flush()
                bi += 1
                left = batches[bi % len(batches)]
        self.flush()

    def steps(self, on=True):
        return self.engs[on].debug_side_steps()


def third(G):
    return np.arange(0, G, 3)


# 1 ---- steady and listed: the step takes every group-tick once the changes are through ---------------------------------------
def steady_and_listed(cuda, oracle, G, R, S, W, hb_every, batch):
    run = Run(cuda, oracle, G, R, S, W, LIST_FOREVER, hb_every, win_reserve=2)
    listed = third(G)
    run.run(8, (1, 3, 4), events={2: dict(timeout_groups=listed)})
    assert run.t == 8 and run.settled(listed), "the oracle does not show the changes of tick 2 complete by tick 7"
    s0 = run.steps()
    for _ in range(16):                                            # (bars move, logs grow: the oracle must show the state settled in every tick)
        run.tick()
        assert run.settled(listed), run.t
        if len(run.pending) == batch or run.t == 24:
            run.flush()
    s1 = run.steps()
    assert s1[0] - s0[0] == len(listed) * 16, (s0, s1, len(listed))
    assert s1[1] - s0[1] == 0, (s0, s1)
    assert run.total > 0
    return run


# 2 ---- reply loss: rows below quorum pin commit_bar, the tally's closed form does not apply -----------------------------------
def reply_loss(cuda, oracle, G, R, S, W, ttl, hb_every, batches):
    run = Run(cuda, oracle, G, R, S, W, ttl, hb_every, win_reserve=2, drop_p=0.2, max_drop=None)
    run.run(28, batches, events={1: dict(timeout_groups=third(G)), 13: dict(timeout_groups=np.arange(1, G, 5))})
    d = run.orc.dump(0)
    assert (d["commit_bar"] < d["log_len"]).any() or run.R == 3
    return run


# 3 ---- a timeout in every position of a batch of 8, in different groups ---------------------------------------------------------
def timeout_in_every_position(cuda, oracle, G, R, S, W, ttl, hb_every):
    run = Run(cuda, oracle, G, R, S, W, ttl, hb_every, win_reserve=2, drop_p=0.1, max_drop=(R - 1) // 2)
    ev = {8 + p: dict(timeout_groups=np.arange(p, G, 8)) for p in range(8)}
    ev.update({24 + p: dict(timeout_groups=np.arange(7 - p, G, 16)) for p in range(8)})     # ... and a second change of some of them
    run.run(40, (8,), events=ev)
    if ttl != NO_REP:
        assert run.steps()[0] > 0, run.steps()
    return run


# 4 ---- requests to a follower (redirects), a tick without requests, an empty batch (token 0) ------------------------------------
def redirects_and_empty_batches(cuda, oracle, G, R, S, W, ttl, hb_every, batches):
    run = Run(cuda, oracle, G, R, S, W, ttl, hb_every, win_reserve=2)
    ev = {1: dict(timeout_groups=third(G))}

    def follower(t):
        tgt = run.leaders()
        tgt = np.where(tgt < R, tgt, 0)
        hit = np.arange(G) % 4 == t % 4
        return np.where(hit, (tgt + 1 + t % (R - 1)) % R, tgt)

    for _ in range(30):
        t = run.t
        kw = dict(ev.get(t, {}))
        if t in (6, 7, 14, 21):
            kw["target"] = follower(t)                              # a quarter of the groups send to a follower: redirects
        if t in (9, 17):
            kw["no_requests"] = True                                # no request arrays at all
        if t in (10, 18):
            kw["req_cnt"] = np.where(np.arange(G) % 2 == 0, 0, S)   # ... and arrays that bring nothing for half the groups
        if t in (11, 12, 19):
            tok = _tokens(run.seed, t, S, G)
            tok[0, np.arange(G) % 3 == t % 3] = 0                   # the empty batch that pins exec_bar
            if S > 1:
                tok[S - 1, np.arange(G) % 5 == 0] = 0
            kw["req_val"] = tok
        if t == 13:
            kw["target"] = np.full(G, NO_REP)                       # addressed to nobody
        run.tick(**kw)
        if len(run.pending) == batches[(t // 3) % len(batches)]:
            run.flush()
    run.flush()
    assert sum(run.engs[True].counters(r)["redirects"] for r in range(R)) > 0
    assert run.steps()[0] > 0
    return run


# 5 ---- the window: one slot short of back-pressure, at it, and a group that overflows and freezes while listed --------------------
def window(cuda, oracle, G, R, S, W, ttl, hb_every, batches, arms=(True, False), win_reserve=None, expect_frozen=False):
    # win_reserve None: as tests/test_mp_gpu.py::test_window_backpressure_and_overflow_flags leaves it (the cluster's default, W / 4);
    # heartbeats far apart: the leader runs to one slot short of back-pressure, then refuses batches.  win_reserve 0: nothing is held
    # back for a leader change, and a change in a group whose window is full freezes it (the overflow flag) while it is listed
    run = Run(cuda, oracle, G, R, S, W, ttl, hb_every, win_reserve=win_reserve, arms=arms)
    ev = {1: dict(timeout_groups=third(G)), 2 * hb_every + 1: dict(timeout_groups=np.arange(1, G, 4)),
          4 * hb_every + 2: dict(timeout_groups=np.arange(2, G, 4))}
    run.run(6 * hb_every + 5, batches, events=ev)
    assert sum(run.engs[True].counters(r)["rejects"] for r in range(R)) > 0
    if expect_frozen:
        frozen = run.orc.dump(0)["overflow"] != 0
        listed = np.zeros(G, bool)
        for e in ev.values():
            listed[e["timeout_groups"]] = True
        assert (frozen & listed).any(), "no listed group froze"
    return run


# 6 ---- the follower's run representation: back to the bulk after ttl runs out ------------------------------------------------------
def hand_back(cuda, oracle, G, R, S, W, ttl, hb_every, batches):
    run = Run(cuda, oracle, G, R, S, W, ttl, hb_every, win_reserve=2, drop_p=0.1, max_drop=(R - 1) // 2)
    run.run(8, (8,), events={1: dict(timeout_groups=third(G))})
    # listed through tick ttl (the mark pass of a batch lists a group for the whole batch): by the batch that starts at or behind
    # tick 1 + ttl the groups are the bulk's again -- the R2 / tally fast paths and the heartbeat's commit learning go on from
    # the state the step left
    back = 8 * ((1 + ttl + 7) // 8)
    s_listed = None
    while run.t < back + 14:
        if run.t == back:
            run.flush()
            s_listed = run.steps()
        run.tick()
        if run.t > back or len(run.pending) == 8:
            run.flush()                                             # every tick for itself past the hand-back
    assert s_listed is not None and s_listed[0] > 0, s_listed
    assert run.steps() == s_listed, "a group-tick on the side launch after every ttl ran out"
    return run


# 7 ---- save and load in the middle of such a run ----------------------------------------------------------------------------------
def save_and_load(cuda, oracle, G, R, S, W, ttl, hb_every):
    from summerset_amd import MultiPaxosCluster
    run = Run(cuda, oracle, G, R, S, W, ttl, hb_every, win_reserve=2, drop_p=0.1, max_drop=(R - 1) // 2, arms=(True, False))
    run.run(13, (8, 5), events={1: dict(timeout_groups=third(G)), 9: dict(timeout_groups=np.arange(1, G, 7))})
    assert run.steps(True)[0] > 0 and run.steps(False)[0] == 0
    a, b = run.engs[True].save_state(), run.engs[False].save_state()
    img = a.export()
    assert img == b.export(), "a cluster that took the step saves another image than one that never did"
    with switch(True):
        fresh = MultiPaxosCluster(G, R, W, win_reserve=2, outbox_cap=run.cap, commit_list_cap=run.clist_cap, straggler_ticks=ttl)
    fresh.load_state(a)
    for r in range(R):
        da, db = fresh.dump(r), run.engs[False].dump(r)
        for k in da:
            assert np.array_equal(da[k], db[k]), (r, k)
    run.engs[True] = fresh                                          # ... and goes on from the loaded state, listed groups and all
    run.run(11, (3, 8))
    return run


# 8 ---- both switch settings through the same stream --------------------------------------------------------------------------------
def both_settings(cuda, oracle, G, R, S, W, ttl, hb_every, batches):
    run = Run(cuda, oracle, G, R, S, W, ttl, hb_every, win_reserve=2, drop_p=0.15, max_drop=None, arms=(True, False))
    ev = {2: dict(timeout_groups=third(G)), 11: dict(timeout_groups=np.arange(2, G, 5)), 12: dict(timeout_groups=np.arange(0, G, 9))}
    run.run(30, batches, events=ev)
    on, off = run.steps(True), run.steps(False)
    assert off[0] == 0 and off[1] == sum(on), (on, off)             # the same list, tick for tick
    assert on[0] > 0
    return run
