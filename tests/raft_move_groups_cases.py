"""Chosen groups between Raft / CRaft replica objects (smr_raft_save_groups / smr_raft_load_groups / smr_raft_reset_groups and
their cluster forms): the bodies of tests/test_raft_move_groups.py (emulator, dev = "cpu") and
tests/test_zzzz_raft_move_groups_gpu.py (device).

Every comparison is bit-exact against `oracle.RaftOracle` / `oracle.CRaftOracle`.  The oracle cannot move anything: it simply
keeps running ALL groups of the job.  A `Shard` is R engine replica objects and the host's table slot -> job group; its inputs are
the job's per-group arrays gathered by that table (an empty slot is fed nothing: no timeout, n_new 0, its messages lost), and its
dumps are compared column by column with the oracles' (`dump`, `dump_votes`; CRaft: `dump_craft`, `dump_masks`), an empty slot's
columns with those of a newly created object.  Every scenario first runs its schedule on the oracles ALONE and asserts what that
run covers; only then are engines made."""
import numpy as np

import raft_cluster as rc
import raft_snapshot_cases as sc
from raft_cluster import CANDIDATE, FOLLOWER, LEADER, NO, NumpyRaft

GROUP_SYMBOLS = ("smr_raft_snapshot_create_groups", "smr_raft_save_groups", "smr_raft_load_groups", "smr_raft_reset_groups",
                 "smr_raft_cluster_save_groups", "smr_raft_cluster_load_groups", "smr_raft_cluster_reset_groups")


def _dumps(x, craft=False):
    """everything a replica (engine adapter or oracle) can be asked per group, as one dict of arrays with the group axis last"""
    d = dict(x.dump())
    d.update(x.dump_votes())
    if craft:
        d.update(x.dump_craft())
        d["mask"] = x.dump_masks()["mask"]
    return d


def _equal_columns(a, ia, b, ib, what):
    for n, v in b.items():
        x, y = np.asarray(a[n])[..., ia].astype(np.uint64), np.asarray(v)[..., ib].astype(np.uint64)
        if not np.array_equal(x, y):
            bad = np.nonzero((x != y).reshape(-1, x.shape[-1]).any(axis=0))[0][:5]
            raise AssertionError("%s: %s differs at positions %s" % (what, n, bad))


def _all_equal(a, b, what):
    for n in b:
        assert np.array_equal(a[n], b[n]), (what, n)


def symbols(lib):
    import summerset_amd
    from summerset_amd import _lib
    names = {n for n, _, _ in _lib.SYMBOLS}
    for n in GROUP_SYMBOLS:
        assert n in names and getattr(lib, n)
    for n in ("move_raft_groups", "save_cluster_groups", "load_cluster_groups", "reset_cluster_groups", "move_groups"):
        assert hasattr(summerset_amd, n)
    assert summerset_amd.move_groups is not summerset_amd.move_raft_groups   # the MultiPaxos one keeps its name


class Shard:
    """R replica objects of n_slots groups and the host's table of which job group sits in which slot (-1: none)"""

    def __init__(self, dev, n_slots, R, W, term0=None, commit_extra=0):
        from summerset_amd import RaftLeaderGroup
        self.R, self.W, self.n, self.dev = R, W, n_slots, dev
        self.reps = [NumpyRaft(RaftLeaderGroup(n_slots, R, leader_id=r, window=W, term=1, commit_extra=commit_extra), dev) for r in range(R)]
        self.fresh = [_dumps(x) for x in self.reps]              # a newly created object's columns
        self.tab = np.full(n_slots, -1, np.int64)
        if term0 is not None:
            for x in self.reps:
                x.preset(FOLLOWER, NO, term0)

    @property
    def engines(self):
        return [x.e for x in self.reps]

    def occupy(self, slots, jobs):
        self.tab[np.asarray(slots)] = np.asarray(jobs)

    def occupied(self):
        return np.nonzero(self.tab >= 0)[0]

    def free(self):
        return np.nonzero(self.tab < 0)[0]

    def reset_free(self):
        """(a preset reaches the empty slots too)"""
        from summerset_amd import reset_cluster_groups
        if len(self.free()):
            reset_cluster_groups(self.engines, self.free())

    def tick(self, to, n_new, K, down, drop, order):
        occ = self.tab >= 0
        j = np.where(occ, self.tab, 0)
        lost = {(a, b): ((drop[(a, b)][j] if drop else np.zeros(self.n, bool)) | ~occ) for a in range(self.R) for b in range(self.R) if a != b}
        rc.tick(self.reps, np.where(occ, to[:, j], NO).astype(np.uint8), np.where(occ, n_new[:, j], 0).astype(np.uint32), K, down=down, drop=lost,
                resend=True, **sc.ORDER[order])

    def compare(self, job, what, empty=True):
        """job[r]: `_dumps` of the job's oracle r"""
        occ, emp = self.occupied(), self.free()
        for r in range(self.R):
            a = _dumps(self.reps[r])
            _equal_columns(a, occ, job[r], self.tab[occ], "%s rep %d" % (what, r))
            if empty and len(emp):
                _equal_columns(a, emp, self.fresh[r], emp, "%s rep %d, empty slots" % (what, r))

    def commits(self, r):
        return self.reps[r].total_commits()

    def close(self):
        sc._close(self.reps)


def _move(src, ss, dst, ds, cluster, reset=True):
    """groups ss of src become groups ds of dst, through the cluster forms or replica by replica through the single calls"""
    from summerset_amd import move_raft_groups
    if cluster:
        snaps = move_raft_groups(src.engines, ss, dst.engines, ds, reset=reset)
    else:
        snaps = []
        for a, b in zip(src.engines, dst.engines):
            snaps.append(a.save_groups(ss))
            b.load_groups(snaps[-1], ds)
            if reset:
                a.reset_groups(ss)
    dst.tab[np.asarray(ds)] = src.tab[np.asarray(ss)]
    if reset:
        src.tab[np.asarray(ss)] = -1
    return snaps


def _job(orcs, craft=False):
    return [_dumps(o, craft) for o in orcs]


def boundary_schedule(R, G, W, seed):
    """outages shorter than the ring takes to fill (so that logs grow past two rings in 24 ticks), one replica that comes back
    standing, loss, up to 5 appends a tick at every replica"""
    win = [(2, 6, (1,)), (8, 11, (2 % R,)), (13, 16, (0,)), (18, 21, (R - 1,))]
    return lambda: rc.Outages(R, G, seed, windows=win, lonely={7: 1, 17: 0}, n_new_max=5, loss=0.05)


MOVE_COVERAGE = ("candidate_with_votes", "next_behind", "past_ring", "past_two_rings", "n_trunc", "one_entry")


def move_at_every_boundary(dev, oracle, R, order, cluster, G=200, NB=96, W=16, K=8, T=24, seed=7):
    """A starts with all job groups, B empty; after every tick a seeded list of 3..40 groups moves A -> B or B -> A into free
    slots (list order and target slots random, slots get reused), then both run the next tick: every occupied slot equals its
    oracle column after every tick, every empty one a new object's, and the commits of A and B add up to the oracle's"""
    mk = boundary_schedule(R, G, W, 41)

    def run(engines):
        sch = mk()
        orcs = sc._oracles(oracle, G, R, W, 0)
        rng = np.random.default_rng(seed)
        A = B = None
        tabs = [np.arange(G), np.full(NB, -1, np.int64)]          # (kept here too: the oracles' own pass has no shards)
        if engines:
            A, B = Shard(dev, G, R, W, 0), Shard(dev, NB, R, W, 0)
            A.occupy(np.arange(G), np.arange(G))
            B.reset_free()
        cov = dict.fromkeys(MOVE_COVERAGE + ("reused", "moves"), 0)
        left = [set(), set()]
        dumps = [o.dump() for o in orcs]
        for t in range(T):
            to, n_new, down, drop = sch(t, dumps)
            rc.tick(orcs, to, n_new, K, down=down, drop=drop, resend=True, **sc.ORDER[order])
            dumps = [o.dump() for o in orcs]
            job = _job(orcs)
            if engines:
                A.tick(to, n_new, K, down, drop, order); B.tick(to, n_new, K, down, drop, order)
                A.compare(job, "tick %d A" % t); B.compare(job, "tick %d B" % t)
                for r in range(R):
                    assert A.commits(r) + B.commits(r) == orcs[r].total_commits(), (t, r)
            nocc = [int((x >= 0).sum()) for x in tabs]
            a_to_b = nocc[1] < 3 or (NB - nocc[1] >= 3 and rng.random() < 0.55)
            s, d = (0, 1) if a_to_b else (1, 0)
            k = int(min(rng.integers(3, 41), nocc[s], len(tabs[d]) - nocc[d]))
            ss = rng.permutation(np.nonzero(tabs[s] >= 0)[0])[:k]
            ds = rng.permutation(np.nonzero(tabs[d] < 0)[0])[:k]
            jg = tabs[s][ss]
            for r in range(R):                                    # what the moved groups carry, on the oracles
                x = job[r]
                ln = x["log_len"][jg]
                peers = np.arange(R)[:, None] != r
                cov["candidate_with_votes"] += int(((x["role"][jg] == CANDIDATE) & (x["votes"][jg] != 0)).sum())
                cov["next_behind"] += int(((x["role"][jg] == LEADER)[None, :] & peers & (x["next_slot"][:, jg] < ln[None, :])).sum())
                cov["past_ring"] += int((ln > W).sum()); cov["past_two_rings"] += int((ln > 2 * W).sum())
                cov["n_trunc"] += int((x["n_trunc"][jg] > 0).sum()); cov["one_entry"] += int((ln == 1).sum())
            cov["reused"] += len(left[d] & set(ds.tolist())); cov["moves"] += 1
            left[s] |= set(ss.tolist())
            tabs[d][ds] = jg; tabs[s][ss] = -1
            if engines:
                src, dst = (A, B) if a_to_b else (B, A)
                snaps = _move(src, ss, dst, ds, cluster)
                for r, sn in enumerate(snaps):
                    info = sn.info()
                    assert info["n_groups"] == k and info["population"] == R and info["replica_id"] == r, info
                    assert not sc.image_counters(sn.export()).any(), "a group image holds zero counters"
                    sn.close()
                assert np.array_equal(A.tab, tabs[0]) and np.array_equal(B.tab, tabs[1])
                A.compare(job, "after the move of tick %d, A" % t); B.compare(job, "after the move of tick %d, B" % t)
        if engines:
            A.close(); B.close()
        cov["commits"] = sum(o.total_commits() for o in orcs)
        return cov
    cov = run(False)
    for n in MOVE_COVERAGE + ("reused", "commits"):
        assert cov[n] > 0, ("the oracle run's moved groups do not cover", n, cov)
    assert run(True) == cov
    return cov


def _run_cluster(dev, oracle, G, R, W, K, T, mk, order="calls", shard=None):
    """a job of G groups on oracles and on one shard that holds them all, T ticks; returns (orcs, shard, schedule, dumps)"""
    sch = mk()
    orcs = sc._oracles(oracle, G, R, W, 0)
    A = shard or Shard(dev, G, R, W, 0)
    A.occupy(np.arange(G), np.arange(G))
    dumps = [o.dump() for o in orcs]
    for t in range(T):
        to, n_new, down, drop = sch(t, dumps)
        rc.tick(orcs, to, n_new, K, down=down, drop=drop, resend=True, **sc.ORDER[order])
        A.tick(to, n_new, K, down, drop, order)
        dumps = [o.dump() for o in orcs]
    A.compare(_job(orcs), "after %d ticks" % T)
    return orcs, A, sch, dumps


def _go_on(orcs, shards, sch, dumps, K, t0, t1, order="calls", what=""):
    for t in range(t0, t1):
        to, n_new, down, drop = sch(t, dumps)
        rc.tick(orcs, to, n_new, K, down=down, drop=drop, resend=True, **sc.ORDER[order])
        dumps = [o.dump() for o in orcs]
        job = _job(orcs)
        for i, s in enumerate(shards):
            s.tick(to, n_new, K, down, drop, order)
            s.compare(job, "%s tick %d shard %d" % (what, t, i))
    return dumps


def list_shapes(dev, oracle, sizes=(1, 63, 64, 65, 330), G=333, R=3, W=8, K=8, T=14, seed=3):
    """lists of every size around a tile and of six tiles (two blocks), ascending, reversed and random, out of a replica whose G
    is no multiple of 64 and whose rings have wrapped: the image's bytes are the canonical bytes of an n-group replica object
    -- one that was load_state'd from the image and saved again -- and that object holds the oracle's columns"""
    from summerset_amd import RaftLeaderGroup
    orcs, A, _, _ = _run_cluster(dev, oracle, G, R, W, K, T, sc.ring_schedule(R, G, W, 43))
    job = _job(orcs)
    roles = np.stack([x["role"] for x in job])
    assert max(int(x["log_len"].max()) for x in job) > 2 * W and (roles == LEADER).any() and (roles == FOLLOWER).any(), "logs past two rings, both roles"
    rng = np.random.default_rng(seed)
    i = 0
    for n in sizes:
        pick = np.sort(np.concatenate([rng.permutation(G - 1)[:n - 1], [G - 1]]).astype(np.int64))   # the last group among them
        for name, lst in (("ascending", pick), ("reversed", pick[::-1].copy()), ("random", rng.permutation(pick))):
            r = i % R
            i += 1
            snap = A.engines[r].save_groups(lst)
            img = snap.export()
            info = snap.info()
            assert info["n_groups"] == n and info["bytes"] == len(img) and not sc.image_counters(img).any(), (n, name, info)
            small = RaftLeaderGroup(n, R, leader_id=r, window=W, term=1)
            small.load_state(snap)
            again = small.save_state()
            assert again.export() == img, (n, name, r, "not the canonical bytes of the n-group replica")
            _equal_columns(_dumps(NumpyRaft(small, dev)), np.arange(n), job[r], lst, "%d %s rep %d" % (n, name, r))
            for x in (snap, again, small):
                x.close()
    A.close()


def permutation_of_a_large_replica(dev, G=66000, R=5, W=8, T=4, seed=5):
    """more tiles than wavefronts (1 032 tiles, 1 024 wavefronts, two tiles each): every group of one replica object through a
    random permutation list in ONE save, and through the same list into a second object, which then equals the first in every
    dump; through the inverse permutation into a third, which is the first permuted twice"""
    import torch
    from summerset_amd import RaftLeaderGroup, stream
    from test_raft_gpu import _replies
    t_ = lambda x: torch.from_numpy(np.ascontiguousarray(x.view(np.int64) if x.dtype == np.uint64 else x.view(np.int32) if x.dtype == np.uint32 else x)).to(dev)
    a, b, c = (RaftLeaderGroup(G, R, 0, W, term=1) for _ in range(3))
    for t in range(T):
        n_new = (stream._key(seed, 9, t, np.arange(G, dtype=np.uint64)) % np.uint64(4)).astype(np.uint32)
        a.handle_req_batch(t_(n_new))
        d = a.dump()
        term, es, fl, ct, cs, order = _replies(seed, t, G, R, d["log_len"], d["curr_term"])
        a.handle_msg_append_entries_reply(t_(term), t_(es), t_(fl), t_(ct), t_(cs), t_(order))
    da = _dumps(NumpyRaft(a, dev))
    assert a.total_commits() > 0 and int(da["log_len"].max()) > W and len(np.unique(da["log_len"])) > 4
    rng = np.random.default_rng(seed)
    p = rng.permutation(G)
    inv = np.argsort(p)
    snap = a.save_groups(p)
    info = snap.info()
    assert info["n_groups"] == G and info["n_entries"] == int(np.count_nonzero(da["entry_term"])) + int((da["log_len"] <= W).sum())
    b.load_groups(snap, p)
    _all_equal(_dumps(NumpyRaft(b, dev)), da, "through the same permutation")
    c.load_groups(snap, inv)                                     # c[inv[i]] = a[p[i]]: c[j] = a[p[p[j]]]
    _equal_columns(_dumps(NumpyRaft(c, dev)), np.arange(G), da, p[p], "through the inverse permutation")
    assert b.total_commits() == 0 and c.total_commits() == 0     # the counters did not travel
    _all_equal(_dumps(NumpyRaft(a, dev)), da, "the source")
    for x in (snap, a, b, c):
        x.close()


def interchange(dev, oracle, G=130, R=5, W=32, K=8, n=70, seed=11):
    """a group image IS an ordinary image: save_groups -> smr_raft_load_state of fresh n-group objects (and the bytes agree),
    those objects run on as a cluster, their smr_raft_save_state images -> load_groups into other slots of the larger objects,
    whose own counters stay as they are while the images' are ignored"""
    from summerset_amd import RaftSnapshot, save_cluster_state
    mk = lambda: rc.Outages(R, G, seed, windows=[(3, 5, (0,)), (11, 13, (2,))], n_new_max=3, loss=0.03)
    orcs, A, sch, dumps = _run_cluster(dev, oracle, G, R, W, K, 8, mk)
    assert sum(o.total_commits() for o in orcs) > 0
    rng = np.random.default_rng(seed)
    lst = rng.permutation(G)[:n]
    C_ = Shard(dev, n, R, W)
    job = _job(orcs)
    for r in range(R):
        snap = A.engines[r].save_groups(lst)
        img = snap.export()
        assert snap.info()["n_groups"] == n and len(img) == snap.info()["bytes"]
        C_.engines[r].load_state(snap)                           # the existing whole-replica load
        again = C_.engines[r].save_state()
        assert again.export() == img                             # a new object's counters are zero: the same bytes
        assert RaftSnapshot(A.engines[r], n).import_(img).export() == img and RaftSnapshot(C_.engines[r]).import_(img).export() == img
        A.engines[r].reset_groups(lst)
        snap.close(); again.close()
    C_.occupy(np.arange(n), lst); A.tab[lst] = -1
    A.compare(job, "A after the groups left"); C_.compare(job, "C after load_state of group images")
    dumps = _go_on(orcs, [A, C_], sch, dumps, K, 8, 16, what="apart")
    for r in range(R):
        assert A.commits(r) + C_.commits(r) == orcs[r].total_commits()
    whole = save_cluster_state(C_.engines)                       # ordinary images of n-group objects, with their counters
    assert sum(int(sc.image_counters(s.export())[0]) for s in whole) > 0
    before = [A.commits(r) for r in range(R)]
    assert sum(before) > 0
    dst = rng.permutation(lst)                                   # the slots the groups left, in another order
    for r in range(R):
        A.engines[r].load_groups(whole[r], dst)
        whole[r].close()
    A.occupy(dst, C_.tab)
    assert [A.commits(r) for r in range(R)] == before            # the target's counters are its own
    A.compare(_job(orcs), "A after load_groups of whole-replica images")
    _go_on(orcs, [A], sch, dumps, K, 16, 22, what="together again")
    for r in range(R):
        assert A.commits(r) + C_.commits(r) == orcs[r].total_commits()
    A.close(); C_.close()


def other_window(dev, oracle, G=64, NB=70, R=5, K=8, W0=16, W1=64, T0=14, T1=30, seed=19):
    """out of W0 rings that have wrapped into W1 replicas: ring_lo travels as what it stands for, so the moved groups go on in the
    larger ring.  The oracle cluster of window W1 ran the same schedule from the start; the groups moved are those on which it
    and the W0 oracle cluster agree in every scalar at the move (no W0 ring has refused them anything), and the comparison
    after the move is with the W1 oracles: every scalar, and the entry terms from the slot the W0 ring still held at the move.
    Moving back into W0 is refused once a moved log's live span is past W0."""
    from summerset_amd import SummersetError, _lib, load_cluster_groups, save_cluster_groups
    mk = lambda: rc.Outages(R, G, seed, windows=[(2, 4, (1,))], n_new_max=2, loss=0.03)
    sch = {W: mk() for W in (W0, W1)}
    orcs = {W: sc._oracles(oracle, G, R, W, 0) for W in (W0, W1)}
    A = Shard(dev, G, R, W0, 0)
    A.occupy(np.arange(G), np.arange(G))
    dumps = {W: [o.dump() for o in orcs[W]] for W in orcs}
    for t in range(T0):
        for W in orcs:
            to, n_new, down, drop = sch[W](t, dumps[W])
            rc.tick(orcs[W], to, n_new, K, down=down, drop=drop, resend=True)
            if W == W0:
                A.tick(to, n_new, K, down, drop, "calls")
            dumps[W] = [o.dump() for o in orcs[W]]
    j0, j1 = _job(orcs[W0]), _job(orcs[W1])
    A.compare(j0, "the source at the move")
    clean = np.ones(G, bool)
    for r in range(R):
        for n_ in j0[r]:
            if n_ != "entry_term":
                clean &= (np.asarray(j0[r][n_]) == np.asarray(j1[r][n_])).reshape(-1, G).all(axis=0)
    wrapped = np.stack([x["log_len"] for x in j0]).max(axis=0) > W0 + 2
    lst = np.nonzero(clean & wrapped)[0][::-1].copy()
    assert len(lst) >= 8, ("too few groups with a wrapped ring and a history no ring has shaped", int(clean.sum()), int(wrapped.sum()))
    lo = np.stack([np.maximum(x["log_len"].astype(np.int64) - W0, 0) for x in j0])[:, lst]   # the first slot a W0 ring still holds
    B = Shard(dev, NB, R, W1)
    dst = np.arange(len(lst)) * 2 + 1
    for s in _move(A, lst, B, dst, True):
        assert s.info()["max_live"] <= W0
        s.close()
    A.compare(j0, "the source after the move")

    def compare_b(job, what):
        for r in range(R):
            a = _dumps(B.reps[r])
            _equal_columns(a, dst, {k: v for k, v in job[r].items() if k != "entry_term"}, lst, "%s rep %d" % (what, r))
            for i, g in enumerate(lst):
                for s_ in range(int(lo[r, i]), int(job[r]["log_len"][g])):
                    if s_ + W1 >= int(job[r]["log_len"][g]):
                        assert a["entry_term"][s_ & (W1 - 1), dst[i]] == job[r]["entry_term"][s_ & (W1 - 1), g], (what, r, g, s_)
            emp = B.free()
            _equal_columns(a, emp, B.fresh[r], emp, "%s rep %d, empty slots" % (what, r))
    compare_b(j1, "the target at the move")
    keep = A.tab.copy()
    for t in range(T0, T1):
        to, n_new, down, drop = sch[W1](t, dumps[W1])
        rc.tick(orcs[W1], to, n_new, K, down=down, drop=drop, resend=True)
        dumps[W1] = [o.dump() for o in orcs[W1]]
        B.tick(to, n_new, K, down, drop, "calls")
        compare_b(_job(orcs[W1]), "tick %d in the larger ring" % t)
    assert np.array_equal(A.tab, keep)
    # back into W0: the live spans have grown past it
    snaps = save_cluster_groups(B.engines, dst)
    assert max(s.info()["max_live"] for s in snaps) > W0
    before = [_dumps(x) for x in A.reps]
    try:
        load_cluster_groups(A.engines, snaps, lst)
        raise AssertionError("a live span above the window was accepted")
    except SummersetError as e:
        assert e.code == _lib.SMR_ERR_ARG and "window" in str(e), e
    k = int(np.argmax([s.info()["max_live"] for s in snaps]))
    try:
        A.engines[k].load_groups(snaps[k], lst)
        raise AssertionError("a live span above the window was accepted")
    except SummersetError as e:
        assert e.code == _lib.SMR_ERR_ARG and "window" in str(e), e
    for r in range(R):
        _all_equal(_dumps(A.reps[r]), before[r], "the refused target")
    for s in snaps:
        s.close()
    A.close(); B.close()


# ---- CRaft ------------------------------------------------------------------------------------------------------------------------
class _Slots:
    """a `_Craft` replica of a shard behind the job's interface: every per-group input gathered by the table, an empty slot fed
    nothing (no entries, no message, no timeout, no reply, no mode call)"""

    def __init__(self, x, tab):
        self.x, self.tab = x, tab

    def _g(self, a, fill=None):
        occ = self.tab >= 0
        v = np.asarray(a)[..., np.where(occ, self.tab, 0)]
        return np.ascontiguousarray(v if fill is None else np.where(occ, v, fill).astype(v.dtype))

    def preset(self, *a):
        assert (self.tab >= 0).all(), "a preset reaches every slot: only before the first move"
        self.x.preset(*a)

    def append(self, n_new): self.x.append(self._g(n_new, 0))
    def become_candidate(self, src): return self.x.become_candidate(self._g(src, NO))
    def handle_vote_replies(self, term, flags, order=None): return self.x.handle_vote_replies(self._g(term), self._g(flags, 0), order)
    def handle_replies(self, rt, es, fl, ct=None, cs=None, order=None): self.x.handle_replies(self._g(rt), self._g(es), self._g(fl, 0), ct, cs, order)
    def bcast_heartbeats(self): return self.x.bcast_heartbeats()
    def switch_assignment_mode(self, to): self.x.switch_assignment_mode(self._g(to, 0xFF))
    def take_reconstructs(self, K=16): return self.x.take_reconstructs(K)
    def handle_reconstruct_reply(self, peer, n, slot, mask): self.x.handle_reconstruct_reply(self._g(peer, NO), self._g(n, 0), self._g(slot), self._g(mask))

    def handle_append_entries(self, **m):
        return self.x.handle_append_entries(**{k: self._g(v, 0 if k == "flags" else None) for k, v in m.items()})


def craft_moves(dev, oracle, G=130, NB=96, R=5, W=32, K=6, ft=1, thr=2, seed=101, t_move=40, t_back=50, n=50):
    """R CRaft replica objects, each walked its own way through a follower's life, an election and a term as the leader of a log
    it did not create (raft_snapshot_cases.craft_steps), with the Reconstruct queues left unpolled.  After step t_move a list of
    groups moves, in one launch for all R objects, into new objects B: the queues, the heartbeat counters, full_copy, the partial
    shard bitmaps travel -- B's poll hands over the moved queues -- and both sides go on, step by step against the oracles.
    After step t_back half of them move back by the single calls into the slots they left (reset then), in another order.
    Every load and reset leaves the groups not listed bit-equal.  A leader's heartbeat timer ticks in an empty slot as in any new
    object, so an empty slot is compared with an object created when the slot was emptied and fed the same calls with nothing
    in them (`twins`)."""
    from summerset_amd import load_cluster_groups, reset_cluster_groups, save_cluster_groups
    full = (1 << R) - 1

    def run(engines):
        gens, orcs, rngs = [], [], []
        for r in range(R):
            steps, rng = sc.craft_steps(G, R, W, r, K, seed + r)
            o = oracle.CRaftOracle(G, R, W, leader_id=r, term=1, fault_tolerance=ft, repeat_threshold=thr)
            gens.append(steps(o)); orcs.append(o); rngs.append(rng)
        new = lambda slots: [sc._Craft(dev, slots, R, W, r, ft, thr) for r in range(R)]
        A, B, twins = (new(G) if engines else None), None, []
        tabA, tabB = np.arange(G), np.full(NB, -1, np.int64)
        bornA, bornB = np.zeros(G, np.int64), np.zeros(NB, np.int64)   # which twin an empty slot is as old as
        nothing = np.full(NB, -1, np.int64)
        mrng = np.random.default_rng(seed)
        cov = dict(queued=0, polled_moved=0, full_copy=0, hb_replied=0, hb_seen=0, hb_repeat=0, partial_masks=0, moved_back=0, steps=0)
        moved = None

        def sides():
            return [(A, tabA, bornA)] + ([(B, tabB, bornB)] if B else [])

        def compare(what):
            if not engines:
                return
            job = _job(orcs, True)
            tw = [[_dumps(x, True) for x in t] for t in twins]
            for X, tab, born in sides():
                occ, emp = np.nonzero(tab >= 0)[0], np.nonzero(tab < 0)[0]
                for r in range(R):
                    a = _dumps(X[r], True)
                    _equal_columns(a, occ, job[r], tab[occ], "%s rep %d" % (what, r))
                    for k in range(len(twins)):
                        e = emp[born[emp] == k]
                        _equal_columns(a, e, tw[k][r], np.zeros(len(e), np.int64), "%s rep %d, empty slots of age %d" % (what, r, k))
            for r in range(R):
                xs = [X[r] for X, _, _ in sides()]
                assert sum(x.total_commits() for x in xs) == orcs[r].total_commits(), (what, r, "commits")
                assert list(sum(x.dump_masks()["counters"] for x in xs)) == list(orcs[r].dump_masks()["counters"]), (what, r, "counters 4, 5")

        def untouched(X, before, listed, what):
            rest = np.setdiff1d(np.arange(len(before[0]["role"])), listed)
            for r in range(R):
                _equal_columns(_dumps(X[r], True), rest, before[r], rest, "%s rep %d: a group not listed" % (what, r))

        def everywhere(r, f):                                     # one step of replica r's life, on whatever holds its groups
            ro = f(orcs[r])
            if engines:
                for X, tab, _ in sides():
                    re_ = f(_Slots(X[r], tab))
                    if isinstance(ro, dict):
                        occ = np.nonzero(tab >= 0)[0]
                        _equal_columns(re_, occ, ro, tab[occ], "rep %d result" % r)
                for t in twins:
                    f(_Slots(t[r], nothing))
            return ro
        i = 0
        while True:
            nxt = [next(g, None) for g in gens]
            if nxt[0] is None:
                break
            for r in range(R):
                name, f, after = nxt[r]
                everywhere(r, f)
                if after == "queue" and i >= t_move:             # (before the move the queues are left to grow: they travel)
                    qo = orcs[r].take_reconstructs(16)
                    if moved is not None:
                        cov["polled_moved"] += int(qo["n"][moved].sum())
                    if engines:
                        for X, tab, _ in sides():
                            occ = np.nonzero(tab >= 0)[0]
                            _equal_columns(X[r].take_reconstructs(16), occ, qo, tab[occ], "step %d rep %d: the polled queue" % (i, r))
                        for t in twins:
                            assert not t[r].take_reconstructs(16)["n"].any()
                    for p in [q for q in range(R) if q != r][:2]:
                        n_ = np.where(rngs[r].random(G) < 0.7, qo["n"], 0).astype(np.uint32)
                        mask = rngs[r].integers(0, 1 << R, qo["slot"].shape).astype(np.uint8)
                        peer = np.full(G, p, np.uint8)
                        peer[rngs[r].random(G) < 0.1] = NO
                        everywhere(r, lambda x: x.handle_reconstruct_reply(peer, n_, qo["slot"], mask))
            if moved is not None and i >= t_move:
                moved = None if any(a == "queue" for _, _, a in nxt) else moved   # (the first poll after the move has been counted)
            cov["steps"] += 1
            compare("step %d (%s)" % (i, nxt[0][0]))
            if i == t_move - 1:
                lst, dst = mrng.permutation(G)[:n], mrng.permutation(NB)[:n]
                moved = lst
                for r in range(R):
                    c, m = orcs[r].dump_craft(), orcs[r].dump_masks()["mask"]
                    cov["full_copy"] += int(c["full_copy_mode"][lst].sum())
                    cov["hb_replied"] += int((c["hb_replied"][:, lst] > 1).sum()); cov["hb_seen"] += int((c["hb_seen"][:, lst] > 0).sum())
                    cov["hb_repeat"] += int((c["hb_repeat"][:, lst] > 0).sum())
                    cov["partial_masks"] += int(((m[:, lst] != 0) & (m[:, lst] != full)).sum())
                if engines:
                    B = new(NB)
                    twins.append(new(NB))
                    bB, bA = [_dumps(x, True) for x in B], [_dumps(x, True) for x in A]
                    snaps = save_cluster_groups([x.e for x in A], lst)
                    cov["queued"] += sum(s.info()["n_reconstructs"] for s in snaps)
                    assert all(s.info()["craft"] == 1 and s.info()["fault_tolerance"] == ft and s.info()["repeat_threshold"] == thr for s in snaps)
                    untouched(A, bA, np.zeros(0, np.int64), "save_groups")
                    load_cluster_groups([x.e for x in B], snaps, dst)
                    untouched(B, bB, dst, "load_groups")
                    reset_cluster_groups([x.e for x in A], lst)
                    untouched(A, bA, lst, "reset_groups")
                    for s in snaps:
                        s.close()
                tabB[dst] = tabA[lst]; tabA[lst] = -1
                compare("after the move")
            if i == t_back - 1:
                back = mrng.permutation(np.nonzero(tabB >= 0)[0])[:n // 2]
                into = mrng.permutation(np.nonzero(tabA < 0)[0])[:n // 2]
                cov["moved_back"] += len(back)
                if engines:
                    twins.append(new(NB))
                    bA, bB = [_dumps(x, True) for x in A], [_dumps(x, True) for x in B]
                    for r in range(R):                            # the single calls
                        s = B[r].e.save_groups(back)
                        A[r].e.load_groups(s, into)
                        B[r].e.reset_groups(back)
                        s.close()
                    untouched(A, bA, into, "load_groups into reset slots"); untouched(B, bB, back, "reset_groups")
                tabA[into] = tabB[back]; tabB[back] = -1
                bornB[back] = 1
                compare("after the move back")
            i += 1
        if engines:
            for x in A + B + [y for t in twins for y in t]:
                x.e.close()
        return cov
    cov = run(False)
    for n_ in ("polled_moved", "full_copy", "hb_replied", "hb_seen", "hb_repeat", "partial_masks", "moved_back"):
        assert cov[n_] > 0, ("the oracle run's moved groups do not cover", n_, cov)
    assert cov["steps"] > t_back + 4, cov
    got = run(True)
    assert got.pop("queued") > 0, "no moved image carried a Reconstruct queue"
    cov.pop("queued")
    assert got == cov
    return got


def neighbours_and_reset(dev, oracle, G=130, NB=100, R=5, W=16, K=8, seed=13):
    """load_groups and reset_groups change the listed groups and nothing else; a reset slot is a new object's, is reused by a
    later load and then runs against the oracle"""
    mk = boundary_schedule(R, G, W, 53)
    orcs, A, sch, dumps = _run_cluster(dev, oracle, G, R, W, K, 8, mk)
    B = Shard(dev, NB, R, W, 0)
    B.reset_free()
    rng = np.random.default_rng(seed)

    def untouched(sh, before, listed, what):
        rest = np.setdiff1d(np.arange(sh.n), listed)
        for r in range(R):
            _equal_columns(_dumps(sh.reps[r]), rest, before[r], rest, "%s rep %d: a group not listed" % (what, r))

    def there(src, ss, dst, ds, cluster, what):
        bs, bd = [_dumps(x) for x in src.reps], [_dumps(x) for x in dst.reps]
        for s in _move(src, ss, dst, ds, cluster, reset=False):
            s.close()
        untouched(dst, bd, ds, what + ": load_groups"); untouched(src, bs, np.zeros(0, np.int64), what + ": save_groups")
        if cluster:
            from summerset_amd import reset_cluster_groups
            reset_cluster_groups(src.engines, ss)
        else:
            for e in src.engines:
                e.reset_groups(ss)
        untouched(src, bs, ss, what + ": reset_groups")
        src.tab[np.asarray(ss)] = -1
        job = _job(orcs)
        src.compare(job, what + ", source"); dst.compare(job, what + ", target")   # (the reset slots: a new object's)
    l1 = rng.permutation(G)[:33]
    there(A, l1, B, rng.permutation(NB)[:33], True, "first move")
    dumps = _go_on(orcs, [A, B], sch, dumps, K, 8, 14, what="apart")
    # the slots A's groups left are used again, by other groups and in another order
    back = rng.permutation(B.occupied())[:20]
    into = rng.permutation(A.free())[:20]
    assert set(into.tolist()) <= set(l1.tolist())
    there(B, back, A, into, False, "into reset slots")
    _go_on(orcs, [A, B], sch, dumps, K, 14, 22, what="reused")
    for r in range(R):
        assert A.commits(r) + B.commits(r) == orcs[r].total_commits()
    A.close(); B.close()


def cluster_form(dev, oracle, G=130, NB=100, R=5, W=16, K=8, T=10, n=70, seed=17):
    """the cluster forms over n_reps = 1, 3, 5 replicas and over four of the five: the single calls' images byte for byte, the
    single calls' states dump for dump, and a replica that is not in the list keeps what it held"""
    from summerset_amd import RaftLeaderGroup, load_cluster_groups, reset_cluster_groups, save_cluster_groups
    orcs, A, _, _ = _run_cluster(dev, oracle, G, R, W, K, T, boundary_schedule(R, G, W, 59))
    rng = np.random.default_rng(seed)
    lst, dst = rng.permutation(G)[:n], rng.permutation(NB)[:n]
    single = []
    for r in range(R):
        s = A.engines[r].save_groups(lst)
        single.append(s.export())
        s.close()
    assert len(set(single)) == R                                  # (the replicas' states differ: a mix-up would show)
    new = lambda: [NumpyRaft(RaftLeaderGroup(NB, R, leader_id=r, window=W, term=1), dev) for r in range(R)]
    for pick in ([3], [2, 0, 4], [0, 1, 2, 3, 4], [4, 1, 0, 3]):
        snaps = save_cluster_groups([A.engines[r] for r in pick], lst)
        for r, s in zip(pick, snaps):
            assert s.export() == single[r], (pick, r)
        one, many = new(), new()
        fresh = [_dumps(x) for x in one]
        for r, s in zip(pick, snaps):
            one[r].e.load_groups(s, dst)
        load_cluster_groups([many[r].e for r in pick], snaps, dst)
        for r in range(R):
            a = _dumps(many[r])
            _all_equal(a, _dumps(one[r]), (pick, r, "loaded"))
            if r in pick:
                _equal_columns(a, dst, _dumps(orcs[r]), lst, "%s rep %d" % (pick, r))
            else:
                _all_equal(a, fresh[r], (pick, r, "not in the list of replicas"))
        half = dst[::2].copy()
        for r in pick:
            one[r].e.reset_groups(half)
        reset_cluster_groups([many[r].e for r in pick], half)
        for r in range(R):
            a = _dumps(many[r])
            _all_equal(a, _dumps(one[r]), (pick, r, "reset"))
            _equal_columns(a, half, fresh[r], half, "%s rep %d reset" % (pick, r))
        for x in snaps:
            x.close()
        sc._close(one); sc._close(many)
    A.close()


def refusals(dev, oracle, G=70, NB=90, R=5, W=16, K=8, n=20):
    """every call that must be refused is, with its code and a message; after each the replicas' dumps and the snapshot's
    exported bytes are what they were"""
    import ctypes as C

    from summerset_amd import (CRaftLeaderGroup, RaftLeaderGroup, RaftSnapshot, SummersetError, _lib, load_cluster_groups, reset_cluster_groups,
                               save_cluster_groups)
    L = _lib.load()
    orcs, A, _, _ = _run_cluster(dev, oracle, G, R, W, K, 8, boundary_schedule(R, G, W, 61))
    src = A.engines
    lst = (np.arange(n) * 3 + 2).astype(np.uint32)
    good = save_cluster_groups(src, lst)
    images = [s.export() for s in good]
    assert max(s.info()["max_live"] for s in good) > 8
    tgt = [RaftLeaderGroup(NB, R, leader_id=r, window=W, term=1) for r in range(R)]
    everything = src + tgt
    before = [_dumps(NumpyRaft(e, dev)) for e in everything]

    def refused(code, fn, *a):
        try:
            rc_ = fn(*a)
        except SummersetError as e:
            assert e.code == code and len(e.msg) > 8, e
            assert L.smr_last_error().decode() == e.msg
        else:
            assert isinstance(rc_, int) and rc_ == code and len(L.smr_last_error()) > 8, rc_
        for e, b in zip(everything, before):
            _all_equal(_dumps(NumpyRaft(e, dev)), b, "a refused call changed a replica")
        assert [s.export() for s in good] == images, "a refused call changed a snapshot"
    ARG, STATE = _lib.SMR_ERR_ARG, _lib.SMR_ERR_STATE
    gp = lst.ctypes.data_as(C.c_void_p)
    arr = lambda xs: (C.c_void_p * len(xs))(*[x._h for x in xs])
    h = C.c_void_p()
    # null arguments
    for f in (lambda: L.smr_raft_snapshot_create_groups(None, n, C.byref(h)), lambda: L.smr_raft_snapshot_create_groups(src[0]._h, n, None),
              lambda: L.smr_raft_save_groups(None, gp, n, good[0]._h, None), lambda: L.smr_raft_save_groups(src[0]._h, None, n, good[0]._h, None),
              lambda: L.smr_raft_save_groups(src[0]._h, gp, n, None, None), lambda: L.smr_raft_load_groups(None, good[0]._h, gp, n, None),
              lambda: L.smr_raft_load_groups(tgt[0]._h, None, gp, n, None), lambda: L.smr_raft_load_groups(tgt[0]._h, good[0]._h, None, n, None),
              lambda: L.smr_raft_reset_groups(None, gp, n, None), lambda: L.smr_raft_reset_groups(tgt[0]._h, None, n, None),
              lambda: L.smr_raft_cluster_save_groups(2, None, gp, n, arr(good[:2]), None), lambda: L.smr_raft_cluster_save_groups(2, arr(src[:2]), gp, n, None, None),
              lambda: L.smr_raft_cluster_save_groups(2, arr(src[:2]), None, n, arr(good[:2]), None),
              lambda: L.smr_raft_cluster_save_groups(2, (C.c_void_p * 2)(src[0]._h, None), gp, n, arr(good[:2]), None),
              lambda: L.smr_raft_cluster_load_groups(2, None, arr(good[:2]), gp, n, None), lambda: L.smr_raft_cluster_load_groups(2, arr(tgt[:2]), None, gp, n, None),
              lambda: L.smr_raft_cluster_load_groups(2, arr(tgt[:2]), arr(good[:2]), None, n, None),
              lambda: L.smr_raft_cluster_reset_groups(2, None, gp, n, None), lambda: L.smr_raft_cluster_reset_groups(2, arr(tgt[:2]), None, n, None)):
        refused(ARG, f)
    # lists: a duplicate, an id = n_groups, n = 0, n beyond n_groups; an n that differs from the snapshot's
    dup, big = lst.copy(), lst.copy()
    dup[5] = dup[11]; big[3] = NB
    for bad in (dup, big, []):
        refused(ARG, tgt[0].load_groups, good[0], bad)
        refused(ARG, tgt[0].reset_groups, bad)
        refused(ARG, load_cluster_groups, tgt, good, bad)
        refused(ARG, reset_cluster_groups, tgt, bad)
    big[3] = G
    for bad in (dup, big, []):
        refused(ARG, src[0].save_groups, bad, good[0])
        refused(ARG, save_cluster_groups, src, bad, good)
    refused(ARG, RaftSnapshot, src[0], 0)
    refused(ARG, RaftSnapshot, src[0], G + 1)
    refused(ARG, tgt[0].reset_groups, np.arange(NB + 1))
    refused(ARG, tgt[0].load_groups, good[0], lst[:-1])
    refused(ARG, src[0].save_groups, lst[:-1], good[0])
    refused(ARG, save_cluster_groups, src, lst[:-1], good)
    # an empty snapshot holds nothing to load
    empty = RaftSnapshot(src[0], n)
    refused(STATE, tgt[0].load_groups, empty, lst)
    refused(STATE, load_cluster_groups, tgt, [empty] + good[1:], lst)
    # another population, replica id, commit_extra, variant, fault_tolerance, repeat_threshold -- into the replica and out of it
    others = [RaftLeaderGroup(NB, 7, leader_id=0, window=W, term=1), RaftLeaderGroup(NB, R, leader_id=1, window=W, term=1),
              RaftLeaderGroup(NB, R, leader_id=0, window=W, term=1, commit_extra=1), CRaftLeaderGroup(NB, R, leader_id=0, window=W, term=1)]
    for o in others:
        everything.append(o); before.append(_dumps(NumpyRaft(o, dev)))
        refused(ARG, o.load_groups, good[0], lst)
        refused(ARG, o.save_groups, lst, good[0])
    c1 = CRaftLeaderGroup(NB, R, leader_id=0, window=W, term=1, fault_tolerance=1, repeat_threshold=3)
    cs = c1.save_groups(lst)
    for kw in (dict(fault_tolerance=0), dict(repeat_threshold=2)):
        c2 = CRaftLeaderGroup(NB, R, leader_id=0, window=W, term=1, **kw)
        everything.append(c2); before.append(_dumps(NumpyRaft(c2, dev)))
        refused(ARG, c2.load_groups, cs, lst)
        refused(ARG, c2.save_groups, lst, cs)
    # a window below max_live
    small = RaftLeaderGroup(NB, R, leader_id=0, window=8, term=1)
    everything.append(small); before.append(_dumps(NumpyRaft(small, dev)))
    refused(ARG, small.load_groups, good[0], lst)
    # the cluster forms: a replica or a snapshot twice, too many, replicas that differ, a snapshot of another replica
    refused(ARG, save_cluster_groups, [src[0], src[1], src[0]], lst, good[:3])
    refused(ARG, save_cluster_groups, src[:2], lst, [good[0], good[0]])
    refused(ARG, load_cluster_groups, [tgt[0], tgt[0]], good[:2], lst)
    refused(ARG, load_cluster_groups, tgt[:2], [good[1], good[1]], lst)
    refused(ARG, reset_cluster_groups, [tgt[0], tgt[1], tgt[0]], lst)
    refused(ARG, reset_cluster_groups, tgt + tgt[:4], lst)
    refused(ARG, save_cluster_groups, src + src[:4], lst, good + good[:4])
    refused(ARG, reset_cluster_groups, [], lst)
    refused(ARG, load_cluster_groups, tgt[:2], [good[1], good[0]], lst)          # made for the other replica id
    refused(ARG, reset_cluster_groups, [tgt[0], others[0]], lst)                 # another population
    refused(ARG, reset_cluster_groups, [tgt[0], others[3]], lst)                 # another variant
    refused(ARG, reset_cluster_groups, [tgt[0], src[1]], lst)                    # another n_groups
    # the good images still load, and their groups are the source's as they were saved
    load_cluster_groups(tgt, good, lst)
    for r in range(R):
        _equal_columns(_dumps(NumpyRaft(tgt[r], dev)), lst, _dumps(orcs[r]), lst, "rep %d" % r)
    for x in good + [empty, cs, c1, small] + others + tgt:
        x.close()
    A.close()
