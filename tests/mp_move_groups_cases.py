"""Chosen groups between clusters (smr_mp_save_groups / smr_mp_load_groups / smr_mp_reset_groups): the bodies of
tests/test_mp_move_groups.py (emulator, dev = "cpu") and tests/test_zzzz_mp_move_groups_gpu.py (device).

Every comparison is bit-exact against `oracle.MpOracle`.  The oracle cannot move anything: it simply keeps running ALL groups of
the job.  A cluster (`Shard`) holds a table slot -> job group; its inputs are the job stream's arrays gathered by that table
(an empty slot is fed nothing), and its dump is compared column by column with the oracle's (`MP_SCALARS`, `peer_exec_bar`,
`MP_SLOTS`, `overflow`), an empty slot's columns with those of the cluster as it was created."""
import numpy as np

from mp_snapshot_cases import _rows
from test_mp_gpu import _to_dev

NO_REP = 0xFF


def _fields():
    from oracle.oracle import MP_SCALARS, MP_SLOTS
    return list(MP_SCALARS) + ["peer_exec_bar"] + [n for n, _ in MP_SLOTS]


def _job_dumps(orcs, R):
    """the oracles of a job side by side (job group ids run through them), per replica"""
    if len(orcs) == 1:
        return [orcs[0].dump(r) for r in range(R)]
    ds = [[o.dump(r) for o in orcs] for r in range(R)]
    return [{k: np.concatenate([d[k] for d in dr], axis=-1) for k in dr[0]} for dr in ds]


def _cat(inps):
    """the tick inputs of several streams side by side"""
    out = {k: np.ascontiguousarray(np.concatenate([i[k] for i in inps], axis=-1)) for k in inps[0] if k != "heartbeat"}
    out["heartbeat"] = inps[0]["heartbeat"]
    return out


class Shard:
    """a cluster and the host's table of which job group sits in which slot (-1: none)"""

    def __init__(self, n_slots, R, W, dev, **kw):
        from summerset_amd import MultiPaxosCluster
        self.R, self.W, self.dev = R, W, dev
        kw.setdefault("outbox_cap", W + 4)
        self.eng = MultiPaxosCluster(n_slots, R, W, **kw)
        self.fresh = [self.eng.dump(r) for r in range(R)]        # a newly created cluster's columns
        self.tab = np.full(n_slots, -1, np.int64)
        self.polled = 0

    def occupy(self, slots, job_groups):
        self.tab[np.asarray(slots)] = np.asarray(job_groups)

    def occupied(self):
        return np.nonzero(self.tab >= 0)[0]

    def free(self):
        return np.nonzero(self.tab < 0)[0]

    def inputs(self, inp, timeouts=True):
        occ = self.tab >= 0
        j = np.where(occ, self.tab, 0)
        out = dict(req_target=np.where(occ, inp["req_target"][j], 0).astype(np.uint8),
                   req_cnt=np.where(occ, inp["req_cnt"][j], 0).astype(np.uint32),
                   req_val=np.ascontiguousarray(inp["req_val"][:, j]), ackctl=np.ascontiguousarray(inp["ackctl"][:, j]),
                   heartbeat=inp["heartbeat"])
        if timeouts:
            out.update(timeout_rep=np.where(occ, inp["timeout_rep"][j], NO_REP).astype(np.uint8),
                       timeout_src=np.where(occ, inp["timeout_src"][j], NO_REP).astype(np.uint8))
        else:
            assert not (occ & (inp["timeout_rep"][j] != NO_REP)).any()
            out.update(timeout_rep=None, timeout_src=None)
        return out

    def tick(self, inp):
        self.eng.tick(**_to_dev(self.inputs(inp), self.dev))

    def poll(self):
        if not self.eng.commit_list_cap:                          # (created without a commit list: nothing to leave behind)
            return
        for r in range(self.R):
            self.polled += len(self.eng.poll_commits(r)[0])

    def commits(self, r):
        return self.eng.counters(r)["commits"]

    def compare(self, dumps, what, reps=None, slots=True, empty=True):
        occ, emp = self.occupied(), self.free()
        j = self.tab[occ]
        names = _fields() if slots else [n for n in _fields() if not n.startswith("s_")]
        for r in (range(self.R) if reps is None else reps):
            a, x = self.eng.dump(r), dumps[r]
            assert np.array_equal(a["overflow"][occ], x["overflow"][j]), "%s rep %d: overflow flags differ" % (what, r)
            ok = x["overflow"][j] == 0                           # (a frozen group's flag is its state: test_mp_gpu._compare)
            for n in names:
                if not np.array_equal(a[n][..., occ][..., ok], x[n][..., j][..., ok]):
                    bad = np.nonzero((a[n][..., occ] != x[n][..., j]).reshape(-1, len(occ)).any(axis=0) & ok)[0][:5]
                    raise AssertionError("%s rep %d: %s differs at slots %s (job groups %s)" % (what, r, n, occ[bad], j[bad]))
            if empty and len(emp):
                for n in names + ["overflow"]:
                    assert np.array_equal(a[n][..., emp], self.fresh[r][n][..., emp]), "%s rep %d: empty slots, %s" % (what, r, n)


def _move(src, src_slots, dst, dst_slots, reset=True):
    from summerset_amd import move_groups
    src.poll()                                                    # the moved groups' entries stay on the source's list
    snap = move_groups(src.eng, src_slots, dst.eng, dst_slots, reset=reset)
    dst.tab[np.asarray(dst_slots)] = src.tab[np.asarray(src_slots)]
    if reset:
        src.tab[np.asarray(src_slots)] = -1
    return snap


def symbols(lib):
    from summerset_amd import _lib
    names = {n for n, _, _ in _lib.SYMBOLS}
    for n in ("smr_mp_snapshot_create_groups", "smr_mp_save_groups", "smr_mp_load_groups", "smr_mp_reset_groups"):
        assert n in names and getattr(lib, n)


def move_at_every_boundary(dev, oracle, straggler_ticks, G=200, NB=96, R=5, S=2, W=64, n_ticks=24, seed=7):
    """A starts with all job groups, B empty; after every tick a seeded list of 3..40 groups moves A -> B or B -> A into free
    slots (list order and target slots random, slots get reused), then both run the next tick: every occupied slot equals its
    oracle column after every tick, every empty one a new cluster's, and the commits of A and B add up to the oracle's"""
    from summerset_amd import stream
    cap = W + 4
    kw = dict(outbox_cap=cap, commit_list_cap=G * (S * 8 + 2 * W) + 64, straggler_ticks=straggler_ticks)
    A, B = Shard(G, R, W, dev, **kw), Shard(NB, R, W, dev, **kw)
    orc = oracle.MpOracle(G, R, W, cap=cap, record_commits=False)
    A.eng.preset_leader(0); orc.preset_leader(0)
    A.occupy(np.arange(G), np.arange(G))
    st = stream.MultiPaxosStream(G, R, S, cap=cap, n_ticks=n_ticks, drop_p=0.1, timeout_frac=1.0, timeout_span=8, hb_every=4)
    rng = np.random.default_rng(seed)
    saw_outbox = saw_untimed = False
    reused, left = 0, {id(A): set(), id(B): set()}
    for t in range(n_ticks):
        inp = st.tick(t)
        orc.tick(**inp)
        A.tick(inp); B.tick(inp)
        d = _job_dumps([orc], R)
        A.compare(d, "tick %d A" % t); B.compare(d, "tick %d B" % t)
        A.poll(); B.poll()
        for r in range(R):
            assert A.commits(r) + B.commits(r) == orc.total_commits(r), (t, r)
        a_to_b = len(B.occupied()) < 3 or (len(B.free()) >= 3 and rng.random() < 0.55)
        src, dst = (A, B) if a_to_b else (B, A)
        k = int(min(rng.integers(3, 41), len(src.occupied()), len(dst.free())))
        ss = rng.permutation(src.occupied())[:k]
        ds = rng.permutation(dst.free())[:k]
        jg = src.tab[ss]
        saw_untimed = saw_untimed or bool((st.timeout_tick[jg] > t).any())
        reused += len(left[id(dst)] & set(ds.tolist()))
        left[id(src)] |= set(ss.tolist())
        snap = _move(src, ss, dst, ds)
        info = snap.info()
        assert info["n_groups"] == k and info["population"] == R
        saw_outbox = saw_outbox or info["n_outbox"] > 0
        snap.close()
        A.compare(d, "after the move of tick %d, A" % t); B.compare(d, "after the move of tick %d, B" % t)
    assert saw_outbox, "no moved image carried a pending outbox (a group between its prepare quorum and the re-Accepts)"
    assert saw_untimed, "no moved group had its HearTimeout still in front of it"
    assert reused > 0, "no slot was used a second time"
    assert sum(orc.total_commits(r) for r in range(R)) > 0 and A.polled + B.polled > 0


def list_shapes(dev, oracle, lists, GA=333, GB=400, R=3, W=32, S=1, before=6, after=6, seed=3):
    """`lists`: names of the lists moved A -> B at the boundary, each by one call, out of a source whose G is no multiple of 64
    into a target of another G; then both run on"""
    from summerset_amd import stream
    cap = W + 4
    A, B = Shard(GA, R, W, dev, outbox_cap=cap), Shard(GB, R, W, dev, outbox_cap=cap)
    orc = oracle.MpOracle(GA, R, W, cap=cap, record_commits=False)
    A.eng.preset_leader(0); orc.preset_leader(0)
    A.occupy(np.arange(GA), np.arange(GA))
    st = stream.MultiPaxosStream(GA, R, S, cap=cap, n_ticks=before + after, drop_p=0.2, timeout_frac=1.0, timeout_span=before + 2, hb_every=3)
    rng = np.random.default_rng(seed)
    for t in range(before + after):
        if t == before:
            for name in lists:
                occ = A.occupied()
                if name == "reversed":                            # lane i holds a group with (g & 63) != (i & 63)
                    src = np.arange(64, 128)[::-1]
                    assert set(src.tolist()) <= set(occ.tolist()) and ((src & 63) != (np.arange(64) & 63)).all()
                elif name == "last":                              # n = 65 with group G - 1 of a G that is no multiple of 64
                    src = np.concatenate([rng.permutation(occ[occ != GA - 1])[:64], [GA - 1]])
                    assert GA % 64 and GA - 1 in occ
                elif int(name) == 330:                            # six tiles; the last group among them
                    src = rng.permutation(np.concatenate([rng.permutation(occ[occ != GA - 1])[:329], [GA - 1]]))
                else:
                    src = rng.permutation(occ[occ != GA - 1])[:int(name)]
                dstf = B.free()
                dst = rng.permutation(dstf)[:len(src)] if name != "reversed" else dstf[:64]
                _move(A, src, B, dst).close()
            d = _job_dumps([orc], R)
            A.compare(d, "after the moves, A"); B.compare(d, "after the moves, B")
        inp = st.tick(t)
        orc.tick(**inp)
        A.tick(inp); B.tick(inp)
        d = _job_dumps([orc], R)
        A.compare(d, "tick %d A" % t); B.compare(d, "tick %d B" % t)
    for r in range(R):
        assert A.commits(r) + B.commits(r) == orc.total_commits(r)


def permutation_of_a_large_cluster(dev, oracle, G=66000, R=3, W=8, S=1, n_ticks=4, seed=5):
    """more tiles than wavefronts: every group of one cluster, permuted, into a second one in ONE call"""
    from summerset_amd import stream
    cap = W + 4
    A, B = Shard(G, R, W, dev, outbox_cap=cap), Shard(G, R, W, dev, outbox_cap=cap)
    orc = oracle.MpOracle(G, R, W, cap=cap, record_commits=False)
    A.eng.preset_leader(0); orc.preset_leader(0)
    A.occupy(np.arange(G), np.arange(G))
    st = stream.MultiPaxosStream(G, R, S, cap=cap, n_ticks=n_ticks + 2, drop_p=0.2, timeout_frac=1.0, hb_every=2)
    for t in range(n_ticks):
        inp = st.tick(t)
        orc.tick(**inp)
        A.tick(inp)
    rng = np.random.default_rng(seed)
    _move(A, rng.permutation(G), B, rng.permutation(G)).close()
    d = _job_dumps([orc], R)
    A.compare(d, "after the move, A"); B.compare(d, "after the move, B")
    for t in range(n_ticks, n_ticks + 2):
        inp = st.tick(t)
        orc.tick(**inp)
        B.tick(inp)
        B.compare(_job_dumps([orc], R), "tick %d B" % t)


def interchange(dev, oracle, G=130, NB=100, R=5, S=2, W=32, n=70, seed=11):
    """a group image IS an ordinary image: save_groups -> smr_mp_load_state of a fresh n-group cluster, that cluster's
    smr_mp_save_state -> load_groups into other slots of a third, and the bytes agree"""
    from summerset_amd import MpSnapshot, stream
    cap = W + 4
    kw = dict(outbox_cap=cap, commit_list_cap=G * S * 40 + 64)
    A, B, C_ = Shard(G, R, W, dev, **kw), Shard(NB, R, W, dev, **kw), Shard(n, R, W, dev, **kw)
    orc = oracle.MpOracle(G, R, W, cap=cap, record_commits=False)
    A.eng.preset_leader(0); orc.preset_leader(0)
    A.occupy(np.arange(G), np.arange(G))
    st = stream.MultiPaxosStream(G, R, S, cap=cap, n_ticks=24, drop_p=0.1, timeout_frac=1.0, timeout_span=10, hb_every=4)
    rng = np.random.default_rng(seed)
    for t in range(8):
        inp = st.tick(t)
        orc.tick(**inp)
        A.tick(inp)
    A.poll()
    lst = rng.permutation(G)[:n]
    snap = A.eng.save_groups(lst)
    img = snap.export()
    assert snap.info()["n_groups"] == n and len(img) == snap.info()["bytes"]
    C_.eng.load_state(snap)                                       # the existing whole-cluster load
    C_.occupy(np.arange(n), lst)
    d = _job_dumps([orc], R)
    C_.compare(d, "C after load_state of a group image")
    assert C_.eng.save_state().export() == img                    # no tick since the load: the same bytes
    assert MpSnapshot.from_bytes(img, A.eng, n_groups=n).export() == img
    assert MpSnapshot.from_bytes(img, C_.eng).export() == img
    for t in range(8, 16):
        inp = st.tick(t)
        orc.tick(**inp)
        A.tick(inp); C_.tick(inp)
        d = _job_dumps([orc], R)
        A.compare(d, "tick %d A" % t); C_.compare(d, "tick %d C" % t)
    C_.poll()
    whole = C_.eng.save_state()                                   # an ordinary image of an n-group cluster (its counters are ignored)
    dst = rng.permutation(NB)[:n]
    B.eng.load_groups(whole, dst)
    B.occupy(dst, lst)
    B.compare(d, "B after load_groups of a whole-cluster image")
    assert all(B.commits(r) == 0 for r in range(R))               # the counters did not travel
    for t in range(16, 24):
        inp = st.tick(t)
        orc.tick(**inp)
        B.tick(inp)
        B.compare(_job_dumps([orc], R), "tick %d B" % t)


def other_window(dev, oracle, G=64, R=5, S=3, W0=16, W1=64, max_ticks=40, after=10):
    """out of a W0 ring that has wrapped, with a frozen group among the moved ones, into a W1 cluster: scalars and flags are the
    W0 oracle's at the move; groups with a clean history (the W0 and the W1 oracle agree on them, mp_snapshot_cases.resize)
    then follow the W1 oracle, and the frozen group stays frozen"""
    from summerset_amd import stream
    cap0, cap1 = W0 + 4, W1 + 4
    A = Shard(G, R, W0, dev, win_reserve=0, outbox_cap=cap0)
    B = Shard(G + 6, R, W1, dev, win_reserve=0, outbox_cap=cap1)
    o_small = oracle.MpOracle(G, R, W0, win_reserve=0, cap=cap0, record_commits=False)
    o_big = oracle.MpOracle(G, R, W1, win_reserve=0, cap=cap1, record_commits=False)
    for x in (A.eng, o_small, o_big):
        x.preset_leader(0)
    A.occupy(np.arange(G), np.arange(G))
    st = stream.MultiPaxosStream(G, R, S, cap=cap1, n_ticks=max_ticks + after, drop_p=0.1, timeout_frac=1.0, timeout_span=12, hb_every=8)
    # every fourth group is hot (S batches a tick: the small ring fills between two heartbeats, batches are refused, and a
    # leader change on the full ring freezes the group); the others get one batch a tick and wrap the ring with a clean history
    cnt = np.where(np.arange(G) % 4 == 0, S, 1).astype(np.uint32)
    scal = ["leader", "bal_prep_sent", "bal_prepared", "bal_max_seen", "start_slot", "log_len", "accept_bar", "commit_bar", "exec_bar", "snap_bar"]

    def clean():                                                  # groups on which the two oracles agree in every scalar of every replica
        ok = np.ones(G, bool)
        for r in range(R):
            a, b = o_small.dump(r), o_big.dump(r)
            for n_ in scal + ["overflow"]:
                ok &= a[n_] == b[n_]
            ok &= (a["peer_exec_bar"] == b["peer_exec_bar"]).all(axis=0)
        return ok
    t_move = None
    for t in range(max_ticks):
        inp = dict(st.tick(t), req_cnt=cnt)
        o_small.tick(**_rows(inp, cap0)); o_big.tick(**inp)
        A.tick(inp)
        d0 = o_small.dump(0)
        good = clean() & (d0["overflow"] == 0) & (d0["start_slot"] > W0)
        if d0["overflow"].any() and good.sum() >= 3:
            t_move = t
            break
    assert t_move is not None, "no tick with a frozen group beside clean groups whose ring has wrapped"
    ds = _job_dumps([o_small], R)
    A.compare(ds, "the source at the move")
    frozen, follow = np.nonzero(d0["overflow"] != 0)[0], np.nonzero(good)[0]
    lst = np.concatenate([frozen[:2], follow])[::-1].copy()
    dst = np.arange(len(lst)) * 1 + 3
    _move(A, lst, B, dst).close()
    B.compare(ds, "the target at the move", slots=False)          # (another ring: the slot columns lie elsewhere)
    for r in range(R):                                            # ... slot by slot: row slot & (W - 1) of either ring
        a, x = B.eng.dump(r), ds[r]
        for i, g in zip(dst, lst):
            if x["overflow"][g]:
                continue
            for s_ in range(int(x["start_slot"][g]), int(x["log_len"][g])):
                for n_ in [k for k in _fields() if k.startswith("s_")]:
                    assert a[n_][s_ & (W1 - 1), i] == x[n_][s_ & (W0 - 1), g], (r, g, s_, n_)
    nf = len(frozen[:2])
    for t in range(t_move + 1, t_move + 1 + after):
        inp = dict(st.tick(t), req_cnt=cnt)
        o_big.tick(**inp)
        B.tick(inp)
        db = _job_dumps([o_big], R)
        keep = B.tab.copy()
        for r in range(R):
            assert (B.eng.dump(r)["overflow"][dst[-nf:]] != 0).all(), "a frozen group thawed"
        B.tab[dst[-nf:]] = -1                                     # the frozen ones have no W1 history to follow
        B.compare(db, "tick %d in the larger ring" % t, empty=False)
        B.tab = keep
    assert not o_big.dump(0)["overflow"][follow].any()


def into_a_long_quiet_cluster(dev, oracle, side_steady, G=130, NB=128, R=5, S=2, W=64, quiet=48, after=24, batch=8):
    """B (straggler list on, run in batches) has had no HearTimeout for quiet >= 2 * 16 + 4 + 8 ticks: the rest of R3 rides in
    the next R1.  Groups whose HearTimeout was the tick before are then loaded into it, and the batches go on"""
    import mp_side_steady_cases as ss
    from summerset_amd import stream
    assert quiet >= 2 * 16 + 4 + 8 and quiet % batch == 0 and after % batch == 0
    cap = W + 4
    kw = dict(win_reserve=W // 8, outbox_cap=cap)
    with ss.switch(side_steady):
        B = Shard(NB, R, W, dev, straggler_ticks=4, **kw)
    A = Shard(G - 100, R, W, dev, **kw)
    orc = oracle.MpOracle(G, R, W, win_reserve=W // 8, cap=cap, record_commits=False)
    for x in (A.eng, B.eng, orc):
        x.preset_leader(0)
    B.occupy(np.arange(100), np.arange(100)); A.occupy(np.arange(G - 100), np.arange(100, G))
    B.eng.reset_groups(B.free())                                  # (the preset reached the empty slots too)
    st = stream.MultiPaxosStream(G, R, S, cap=cap, n_ticks=quiet + after, drop_p=0.1, timeout_frac=0.0, hb_every=4)
    st.timeout_tick[:] = -1
    late = np.array([103, 107, 108, 121, 129])
    st.timeout_tick[late] = quiet - 1                             # their HearTimeout is the last tick before the move
    moved = np.concatenate([late, [101, 115]])
    pend = []
    for t in range(quiet + after):
        if t == quiet:
            _move(A, moved - 100, B, np.array([127, 100, 111, 105, 126, 102, 119])).close()
            d = _job_dumps([orc], R)
            A.compare(d, "after the move, A"); B.compare(d, "after the move, B")
        inp = st.tick(t)
        orc.tick(**inp)
        A.tick(inp)
        pend.append(_to_dev(B.inputs(inp, timeouts=False), dev))
        if len(pend) == batch:
            B.eng.run_ticks(pend)
            pend = []
            d = _job_dumps([orc], R)
            A.compare(d, "tick %d A" % t); B.compare(d, "tick %d B" % t)
    for r in range(R):
        assert A.commits(r) + B.commits(r) == orc.total_commits(r)
    return [B.eng.dump(r) for r in range(R)]


def neighbours_and_reset(dev, oracle, GA=130, NB=100, R=5, S=2, W=32, seed=13):
    """load_groups and reset_groups change the listed groups and nothing else; a reset slot is a new cluster's and takes a new
    group, which bootstraps by a HearTimeout on replica 0 and follows its own oracle"""
    from summerset_amd import stream
    cap = W + 4
    G = GA + 60
    A, B = Shard(GA, R, W, dev, outbox_cap=cap), Shard(NB, R, W, dev, outbox_cap=cap)
    orc = oracle.MpOracle(G, R, W, cap=cap, record_commits=False)
    for x in (A.eng, B.eng, orc):
        x.preset_leader(0)
    rng = np.random.default_rng(seed)
    A.occupy(np.arange(GA), np.arange(GA))
    B.occupy(rng.permutation(NB)[:60], np.arange(GA, G))
    B.eng.reset_groups(B.free())                                  # (the preset reached the empty slots too)
    kw = dict(cap=cap, n_ticks=20, drop_p=0.1, hb_every=4)
    st = stream.MultiPaxosStream(G, R, S, timeout_frac=1.0, timeout_span=8, **kw)
    for t in range(6):
        inp = st.tick(t)
        orc.tick(**inp)
        A.tick(inp); B.tick(inp)
    d = _job_dumps([orc], R)
    A.compare(d, "tick 5 A"); B.compare(d, "tick 5 B")
    lst = rng.permutation(GA)[:33]
    dst = rng.permutation(B.free())[:33]

    def untouched(sh, before, listed, what):
        rest = np.setdiff1d(np.arange(len(sh.tab)), listed)
        for r in range(R):
            now = sh.eng.dump(r)
            for k in now:
                assert np.array_equal(now[k][..., rest], before[r][k][..., rest]), "%s: rep %d %s of a group not listed changed" % (what, r, k)
    bB = [B.eng.dump(r) for r in range(R)]
    snap = A.eng.save_groups(lst)
    B.eng.load_groups(snap, dst)
    untouched(B, bB, dst, "load_groups")
    B.occupy(dst, A.tab[lst])
    B.compare(d, "B after the load")
    bA = [A.eng.dump(r) for r in range(R)]
    A.eng.reset_groups(lst)
    untouched(A, bA, lst, "reset_groups")
    A.tab[lst] = -1
    A.compare(d, "A after the reset")                             # the reset columns are a new cluster's
    # new groups in the reset slots: job ids G .., their own oracle and a stream keyed by their global ids
    k = len(lst)
    orc2 = oracle.MpOracle(k, R, W, cap=cap, record_commits=False)
    st2 = stream.MultiPaxosStream(k, R, S, timeout_frac=0.0, group_base=G, **kw)
    A.occupy(lst, np.arange(G, G + k))
    for t in range(6, 16):
        i1, i2 = st.tick(t), st2.tick(t)
        if t == 6:                                                # the bootstrap tick: replica 0 times out, no client batch yet
            i2.update(timeout_rep=np.zeros(k, np.uint8), timeout_src=np.full(k, NO_REP, np.uint8), req_cnt=np.zeros(k, np.uint32))
        orc.tick(**i1); orc2.tick(**i2)
        inp = _cat([i1, i2])
        A.tick(inp); B.tick(inp)
        d = _job_dumps([orc, orc2], R)
        A.compare(d, "tick %d A" % t); B.compare(d, "tick %d B" % t)
    assert sum(orc2.total_commits(r) for r in range(R)) > 0
    for r in range(R):
        assert A.commits(r) + B.commits(r) == orc.total_commits(r) + orc2.total_commits(r)


def partial_live_mask(dev, oracle, G=100, R=5, S=2, W=32, live=0b00101, seed=17):
    """two blocks of a spread job that hold replicas 0 and 2: a move carries those two and leaves the others' rows alone"""
    from summerset_amd import MpSnapshot, _lib, stream
    L = _lib.load()
    cap = W + 4
    A, B = Shard(G, R, W, dev, outbox_cap=cap), Shard(G, R, W, dev, outbox_cap=cap)
    orc = oracle.MpOracle(G, R, W, cap=cap, record_commits=False)
    A.eng.preset_leader(0); orc.preset_leader(0); B.eng.preset_leader(1)
    A.occupy(np.arange(G), np.arange(G))
    st = stream.MultiPaxosStream(G, R, S, cap=cap, n_ticks=8, drop_p=0.1, timeout_frac=1.0, timeout_span=6, hb_every=4)
    for t in range(8):
        inp = st.tick(t)
        orc.tick(**inp)
        A.tick(inp)
    for sh in (A, B):
        _lib.check(L.smr_mp_set_live(sh.eng._h, live))
    rng = np.random.default_rng(seed)
    lst, dst = rng.permutation(G)[:40], rng.permutation(G)[:40]
    before = [B.eng.dump(r) for r in range(R)]
    snap = MpSnapshot(A.eng, 40)
    A.eng.save_groups(lst, snap)
    assert snap.info()["live_mask"] == live
    B.eng.load_groups(snap, dst)
    B.occupy(dst, lst)
    lv = [r for r in range(R) if (live >> r) & 1]
    B.compare(_job_dumps([orc], R), "the live replicas", reps=lv, empty=False)
    rest = np.setdiff1d(np.arange(G), dst)
    for r in range(R):
        now = B.eng.dump(r)
        for k in now:
            if k == "overflow":                                   # (one flag per group, shared by the replicas: it travels)
                assert np.array_equal(now[k][rest], before[r][k][rest])
            elif r in lv:
                assert np.array_equal(now[k][..., rest], before[r][k][..., rest]), (r, k)
            else:
                assert np.array_equal(now[k], before[r][k]), "replica %d is not live here: %s changed" % (r, k)


def refusals(dev, oracle):
    """every call that must be refused is, with its code and a message, and a refused load leaves every dump as it was"""
    import ctypes as C

    import pytest
    from summerset_amd import MpSnapshot, MultiPaxosCluster, SummersetError, _lib, stream
    L = _lib.load()
    G, R, S, W, n = 70, 5, 4, 32, 20
    cap = W + 4
    kw = dict(outbox_cap=cap, commit_list_cap=G * S * 16)

    def refused(code, fn, *a):
        with pytest.raises(SummersetError) as e:
            fn(*a)
        assert e.value.code == code and len(e.value.msg) > 8, e.value
        assert L.smr_last_error().decode() == e.value.msg

    def dumps(eng):
        return [eng.dump(r) for r in range(eng.R)]

    def unchanged(eng, before):
        for r in range(eng.R):
            now = eng.dump(r)
            assert all(np.array_equal(now[k], before[r][k]) for k in now)

    src = MultiPaxosCluster(G, R, W, **kw)
    src.preset_leader(0)
    st = stream.MultiPaxosStream(G, R, S, cap=cap, n_ticks=8, drop_p=0.1, timeout_frac=1.0, hb_every=4, timeout_span=4)
    lst = np.arange(n, dtype=np.uint32) + 7
    good = None
    for t in range(8):                                            # an image with a pending outbox and a log longer than 8 slots
        src.tick(**_to_dev(st.tick(t), dev))
        if good is None:
            s = src.save_groups(lst)
            i = s.info()
            if i["n_outbox"] > 0 and i["max_live"] > 8 and i["max_outbox"] > 4:
                good = s
    assert good is not None
    info = good.info()
    unpolled = src.save_state()                                   # the source's commits are still on its list
    for r in range(R):
        src.poll_commits(r)
    tgt = MultiPaxosCluster(G, R, W, **kw)
    tgt.preset_leader(1)
    before = dumps(tgt)
    gp = lst.ctypes.data_as(C.c_void_p)

    # null arguments
    h = C.c_void_p()
    for rc in (L.smr_mp_snapshot_create_groups(None, n, C.byref(h)), L.smr_mp_snapshot_create_groups(src._h, n, None),
               L.smr_mp_save_groups(None, gp, n, good._h, None), L.smr_mp_save_groups(src._h, None, n, good._h, None),
               L.smr_mp_save_groups(src._h, gp, n, None, None), L.smr_mp_load_groups(None, good._h, gp, n, None),
               L.smr_mp_load_groups(tgt._h, None, gp, n, None), L.smr_mp_load_groups(tgt._h, good._h, None, n, None),
               L.smr_mp_reset_groups(None, gp, n, None), L.smr_mp_reset_groups(tgt._h, None, n, None)):
        assert rc == _lib.SMR_ERR_ARG and len(L.smr_last_error()) > 8
    # lists: a duplicate, an id = G, n = 0, n beyond G; an n that differs from the snapshot's
    dup, big = lst.copy(), lst.copy()
    dup[5] = dup[11]; big[3] = G
    for bad in (dup, big, []):
        refused(_lib.SMR_ERR_ARG, tgt.load_groups, good, bad)
        refused(_lib.SMR_ERR_ARG, tgt.reset_groups, bad)
        refused(_lib.SMR_ERR_ARG, src.save_groups, bad, good)
    refused(_lib.SMR_ERR_ARG, MpSnapshot, src, 0)
    refused(_lib.SMR_ERR_ARG, MpSnapshot, src, G + 1)
    refused(_lib.SMR_ERR_ARG, tgt.reset_groups, np.arange(G + 1))
    refused(_lib.SMR_ERR_ARG, tgt.load_groups, good, lst[:-1])
    refused(_lib.SMR_ERR_ARG, src.save_groups, lst[:-1], good)
    assert good.info() == info                                    # the refused saves left the snapshot alone
    # an empty snapshot holds nothing to load
    refused(_lib.SMR_ERR_STATE, tgt.load_groups, MpSnapshot(src, n), lst)
    # an ordinary image whose commits were not polled
    whole_n = MultiPaxosCluster(n, R, W, **kw)
    whole_n.preset_leader(0)
    whole_n.tick(**_to_dev(stream.MultiPaxosStream(n, R, S, cap=cap, n_ticks=2, drop_p=0.0, timeout_frac=0.0, hb_every=4).tick(0), dev))
    assert sum(whole_n.counters(r)["commits"] for r in range(R)) > 0
    refused(_lib.SMR_ERR_ARG, tgt.load_groups, whole_n.save_state(), lst)
    refused(_lib.SMR_ERR_ARG, tgt.load_groups, unpolled, np.arange(G))
    unchanged(tgt, before)

    # another population, commit_extra or live mask; a window or an outbox that is too small
    others = [MultiPaxosCluster(G, 3, W, **kw), MultiPaxosCluster(G, R, W, commit_extra=1, **kw), MultiPaxosCluster(G, R, W, **kw),
              MultiPaxosCluster(G, R, 8, **kw), MultiPaxosCluster(G, R, W, outbox_cap=4, commit_list_cap=G * S * 16)]
    _lib.check(L.smr_mp_set_live(others[2]._h, 0b00101))
    assert info["max_live"] > 8 and info["max_outbox"] > 4
    for o in others:
        o.preset_leader(1)
        b = dumps(o)
        refused(_lib.SMR_ERR_ARG, o.load_groups, good, lst)
        if o in others[:3]:
            refused(_lib.SMR_ERR_ARG, o.save_groups, lst, good)
        unchanged(o, b)
    assert good.info() == info

    # a tick opened round by round with the straggler list on and not yet closed
    op = MultiPaxosCluster(G, R, W, straggler_ticks=2, **kw)
    op.preset_leader(0)
    b = dumps(op)
    d = _to_dev(st.tick(0), dev)
    op.round_local(d["timeout_rep"], d["timeout_src"], d["req_target"], d["req_cnt"], d["req_val"])
    refused(_lib.SMR_ERR_STATE, op.save_groups, lst, MpSnapshot(op, n))
    refused(_lib.SMR_ERR_STATE, op.load_groups, good, lst)
    refused(_lib.SMR_ERR_STATE, op.reset_groups, lst)
    op.round_deliver()
    op.round_replies(d["ackctl"], publish_heartbeat=False)
    op.end_tick()
    op.load_groups(good, lst)                                     # closed: it goes through

    # the good image still loads, and its groups are the source's as they were saved
    unchanged(tgt, before)
    tgt.load_groups(good, lst)
    chk = MultiPaxosCluster(n, R, W, **kw)
    chk.load_state(good)
    for r in range(R):
        a, x = tgt.dump(r), chk.dump(r)
        for k in a:
            assert np.array_equal(a[k][..., lst], x[k]), (r, k)
