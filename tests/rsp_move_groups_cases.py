"""Chosen groups between RSPaxos replica objects and between payload stores of both kinds, shard bytes included
(smr_rsp_*_groups, smr_rsp_cluster_*_groups, smr_rsp_pstore_*_groups): the bodies of tests/test_rsp_move_groups.py (emulator,
dev = "cpu") and tests/test_zzzz_rsp_move_groups_gpu.py (device), every size an argument.

Every comparison is bit-exact.  The oracle cannot move anything: `oracle.RspOracle` simply keeps running ALL groups of the job, and
the shard bytes are held against the oracle's encoder (`test_zz_rsp_payload_gpu.Expect` / `check_stores`, `craft_payload_loop`).
A `Shard` is R replicas-with-payload of n_slots groups and the host's table slot -> job group; a `JobRep` is replica r of the whole
job for `rsp_cluster.tick`: every handler call is gathered by the tables, run on every shard and scattered back, so that the
job's message log, executed lists and dumps are compared with the oracles' as those of one cluster, and a move can happen behind
ANY handler call.  Images are parsed with rsp_snapshot_cases.Layout / StoreLayout (DESIGN.md 2's tables alone), which check every
pad region."""
import numpy as np

import rsp_cluster as rc
import rsp_edges as e
import rsp_scenarios as sc
import rsp_snapshot_cases as c
from rsp_snapshot_cases import Layout, StoreLayout, dumps_equal, polls_equal

NULL, NO_REP = rc.NULL, rc.NO_REP
REP_SYMBOLS = ("smr_rsp_snapshot_create_groups", "smr_rsp_save_groups", "smr_rsp_load_groups", "smr_rsp_reset_groups",
               "smr_rsp_cluster_save_groups", "smr_rsp_cluster_load_groups", "smr_rsp_cluster_reset_groups")
STORE_SYMBOLS = ("smr_rsp_pstore_snapshot_create_groups", "smr_rsp_pstore_save_groups", "smr_rsp_pstore_load_groups", "smr_rsp_pstore_reset_groups")


def _tp():
    import test_zz_rsp_payload_gpu as tp
    return tp


def _close(xs):
    for x in xs:
        x.close()


def _refused(f, word=None, code=-1):
    from summerset_amd import SummersetError
    try:
        f()
    except SummersetError as err:
        assert err.code == code and (word is None or word in str(err)), (word, err)
        return
    raise AssertionError("not refused: %s" % word)


# ---- 1. symbols ------------------------------------------------------------------------------------------------------------------
def symbols(lib):
    import summerset_amd
    from summerset_amd import _lib, rspaxos
    names = {n for n, _, _ in _lib.SYMBOLS}
    for n in REP_SYMBOLS + STORE_SYMBOLS:
        assert n in names and getattr(lib, n), n
    for n in ("move_rsp_groups", "move_store_groups", "move_craft_groups", "move_groups", "move_raft_groups"):
        assert hasattr(summerset_amd, n), n
    assert len({summerset_amd.move_groups, summerset_amd.move_raft_groups, summerset_amd.move_rsp_groups}) == 3   # the earlier two keep their names
    for n in ("save_cluster_groups", "load_cluster_groups", "reset_cluster_groups"):
        assert hasattr(rspaxos, n), n
    for cls in (summerset_amd.RSPaxosReplicaGroup, summerset_amd.RSPaxosPayloadStore, summerset_amd.CRaftPayloadStore, summerset_amd.RSPaxosReplicaWithPayload):
        for n in ("save_groups", "load_groups", "reset_groups"):
            assert hasattr(cls, n), (cls, n)


# ---- columns of replicas and stores ----------------------------------------------------------------------------------------------
def rep_columns_equal(a, ia, b, ib, what):
    """dump a's groups ia == dump b's groups ib, every per-group field (the counters are the object's, not a group's)"""
    for n, v in b.items():
        if n == "counters":
            continue
        x, y = np.asarray(a[n])[..., ia], np.asarray(v)[..., ib]
        if not np.array_equal(x, y):
            bad = np.nonzero((x != y).reshape(-1, x.shape[-1]).any(axis=0))[0][:5]
            raise AssertionError("%s: %s differs at list positions %s" % (what, n, bad))


def polls_of(poll, groups):
    """exec_poll's (group, slot, token) restricted to `groups`, as {list position: [(slot, token), ...]}"""
    pos = {int(g): i for i, g in enumerate(np.asarray(groups).tolist())}
    out = {}
    for g, s, v in zip(*[x.tolist() for x in poll]):
        if g in pos:
            out.setdefault(pos[g], []).append((s, v))
    return out


def _planes(st):
    return 2 if type(st)._CREATE == "smr_rsp_pstore_create" else 1


class StoreDump:
    """everything a store can be asked: the headers of every plane, the alias bytes, whole rows (bytes behind the shards' lengths
    included), the counters"""

    def __init__(self, st, rows=True):
        self.planes, self.W, self.R, self.d = _planes(st), st.W, st.R, st.d
        self.hdr = [st.dump(p) for p in range(self.planes)]
        self.alias = st.voted_alias() if self.planes == 2 else None
        self.rows = [[st.read_row(w, p) for w in range(st.W)] for p in range(self.planes)] if rows else None   # [plane][w] -> [R, G, stride]
        self.counters, self.delivered = st.counters(), st.delivered()


def store_columns_equal(a, ia, b, ib, what, tail_of=None):
    """StoreDump a's groups ia == b's groups ib: token, and under a token length, shards, alias and every stored shard's bytes up
    to its length -- whatever the two stores' strides.  tail_of: a StoreDump of a's store from BEFORE a load: the bytes of a's rows
    behind each stored shard's length must be what they were"""
    ia, ib = np.asarray(ia), np.asarray(ib)
    n_cmp = 0
    for p in range(a.planes):
        x, y = a.hdr[p], b.hdr[p]
        assert np.array_equal(x["tok"][:, ia], y["tok"][:, ib]), (what, p, "tok")
        some = y["tok"][:, ib] != NULL
        for k in ("avail", "dlen"):
            assert np.array_equal(np.where(some, x[k][:, ia], 0), np.where(some, y[k][:, ib], 0)), (what, p, k)
        if p == 1:
            assert np.array_equal(np.where(some, a.alias[:, ia], 0), np.where(some, b.alias[:, ib], 0)), (what, "alias")
        if a.rows is None or b.rows is None:
            continue
        for w in range(a.W):
            for i in np.nonzero(some[w])[0]:
                ga, gb = int(ia[i]), int(ib[i])
                sl = (int(y["dlen"][w, gb]) + a.d - 1) // a.d
                st = int(y["avail"][w, gb]) & ~(int(b.alias[w, gb]) if p == 1 else 0)
                for k in range(a.R):
                    if (st >> k) & 1:
                        assert np.array_equal(a.rows[p][w][k, ga, :sl], b.rows[p][w][k, gb, :sl]), (what, p, w, ga, gb, k)
                        n_cmp += 1
                        if tail_of is not None:
                            assert np.array_equal(a.rows[p][w][k, ga, sl:], tail_of.rows[p][w][k, ga, sl:]), (what, "bytes behind the length", p, w, ga, k)
    return n_cmp


def store_groups_unchanged(a, b, groups, what):
    """StoreDumps a and b of ONE store: the given groups' headers, alias bytes and whole row bytes are the same"""
    g = np.asarray(groups)
    for p in range(a.planes):
        for k in ("tok", "avail", "dlen"):
            assert np.array_equal(a.hdr[p][k][:, g], b.hdr[p][k][:, g]), (what, p, k)
        for w in range(a.W):
            assert np.array_equal(a.rows[p][w][:, g], b.rows[p][w][:, g]), (what, p, w, "row bytes")
    if a.planes == 2:
        assert np.array_equal(a.alias[:, g], b.alias[:, g]), (what, "alias")


def store_groups_null(d, groups, what):
    g = np.asarray(groups)
    for p in range(d.planes):
        assert (d.hdr[p]["tok"][:, g] == NULL).all() and not d.hdr[p]["avail"][:, g].any() and not d.hdr[p]["dlen"][:, g].any(), (what, p)
    if d.planes == 2:
        assert not d.alias[:, g].any(), (what, "alias")


# ---- a finished cluster, made once and only read -----------------------------------------------------------------------------------
_CLUSTERS = {}


def finished_cluster(dev, oracle, G, R, ft, L, W=8, T=24, loss=0.1):
    """tests/test_zz_rsp_payload_gpu.make_cluster's cluster after rsp_scenarios.run (both leader changes, wrapped rings), every
    tick against the oracle cluster's dumps; shared by the bodies that only read it.  -> (reps, oracle dumps, Expect)"""
    key = (str(dev), G, R, ft, L, W, T, loss)
    if key not in _CLUSTERS:
        tp = _tp()
        run = lambda reps, on_tick: sc.run(reps, G, T, seed=G + ft, loss=loss, on_tick=on_tick)
        orcs, lo, snaps, execd = e.oracle_run(oracle, run, G, R, W, ft)
        assert max(int(d["len"].max()) for d in snaps[-1]) > W, "wrapped rings"
        reps, engs = tp.make_cluster(dev, G, R, W, ft, L)
        exp = tp.Expect(oracle, R, R // 2 + 1, L)
        sc.run(engs, G, T, seed=G + ft, loss=loss)
        for r in range(R):
            dumps_equal(reps[r].replica.dump(), snaps[-1][r], ("finished cluster", r))
        assert tp.check_stores(reps, exp, "finished cluster") > 0
        _CLUSTERS[key] = (reps, snaps[-1], exp)
    return _CLUSTERS[key]


# ---- 2. identity at every boundary, bytes included ---------------------------------------------------------------------------------
_BASELINES = {}


def identity_at_every_boundary(dev, oracle, cluster, G=130, R=5, ft=1, L=61, W=8, T=44, loss=0.1, sizes=(1, 63, 64, 65, 130)):
    """shadow_stores' cluster and schedule; after EVERY tick a seeded, shuffled list is saved from every replica-with-payload, those
    slots are reset (and equal a new object's columns), and the image is loaded back; the dumps against the oracle's and
    check_stores (engine masks, the oracle's codewords byte for byte) after each, and the schedule goes on with the reloaded objects"""
    from summerset_amd import RSPaxosPayloadStore, RSPaxosReplicaGroup
    from summerset_amd.rspaxos import load_cluster_groups, reset_cluster_groups, save_cluster_groups
    tp = _tp()
    key = (str(dev), G, R, ft, L, W, T, loss)
    if key not in _BASELINES:                                    # the whole-state path alone reaches these counts (run once, shared)
        _BASELINES[key] = c.shadow_stores(dev, oracle, G=G, R=R, ft=ft, L=L, W=W, T=T, loss=loss)
    base = _BASELINES[key]
    assert base["alias"] > 0 and base["lone_vote"] > 0 and base["copied"] > 0 and base["rebuilt"] > 0 and base["unsatisfied"] == 0, base
    run = lambda reps, on_tick: sc.run(reps, G, T, seed=G + ft, loss=loss, on_tick=on_tick)
    orcs, lo, snaps, execd = e.oracle_run(oracle, run, G, R, W, ft)
    reps, engs = tp.make_cluster(dev, G, R, W, ft, L)
    exp = tp.Expect(oracle, R, R // 2 + 1, L)
    fresh_rep = [RSPaxosReplicaGroup(G, R, me=r, window=W, fault_tolerance=ft) for r in range(R)]
    fresh = [x.dump() for x in fresh_rep]
    _close(fresh_rep)
    rng = np.random.default_rng(17)
    seen = dict(alias=0, lone_vote=0, cmp=0, bytes=0, ticks=0, n_exec=0)

    def boundary(t):
        n = min(sizes[t % len(sizes)], G)
        lst = rng.permutation(G)[:n]
        rest = np.setdiff1d(np.arange(G), lst)
        for r in range(R):
            for x, y in zip(engs[r].take_executed(), execd[t][r]):
                assert np.array_equal(x, y), (t, r, "executed")
        polls = [x.replica.exec_poll() for x in reps]
        sd0 = [StoreDump(x.store, rows=False) for x in reps]
        if cluster:
            rs = save_cluster_groups([x.replica for x in reps], lst)
            ps = [x.store.save_groups(lst) for x in reps]
            reset_cluster_groups([x.replica for x in reps], lst)
            for x in reps:
                x.store.reset_groups(lst)
            held = list(zip(rs, ps))
        else:
            held = [x.save_groups(lst) for x in reps]
            for x in reps:
                x.reset_groups(lst)
        for r, x in enumerate(reps):
            d = x.replica.dump()
            rep_columns_equal(d, lst, fresh[r], lst, "tick %d rep %d, reset slots" % (t, r))
            rep_columns_equal(d, rest, snaps[t][r], rest, "tick %d rep %d, beside the reset slots" % (t, r))
            store_groups_null(StoreDump(x.store, rows=False), lst, (t, r, "reset"))
        if cluster:
            load_cluster_groups([x.replica for x in reps], [h[0] for h in held], lst)
            for x, h in zip(reps, held):
                x.store.load_groups(h[1], lst)
        else:
            for x, h in zip(reps, held):
                x.load_groups(h, lst)
        for r, x in enumerate(reps):
            dumps_equal(x.replica.dump(), snaps[t][r], (t, r, "reloaded"))          # (counters included: they never left)
            polls_equal(x.replica.exec_poll(), polls[r], (t, r))
            assert x.store.counters() == sd0[r].counters and x.store.delivered() == sd0[r].delivered, (t, r)
            al, av = sd0[r].alias[:, lst], sd0[r].hdr[1]
            seen["alias"] += int((al != 0).sum())
            seen["lone_vote"] += int(((av["avail"][:, lst] & ~al)[av["tok"][:, lst] != NULL] != 0).sum())
            info = held[r][1].info()
            assert info["n_groups"] == n and info["planes"] == 2 and info["craft"] == 0 and info["max_dlen"] <= L, info
            seen["bytes"] += info["shard_bytes"]
            ri = held[r][0].info()
            assert ri["n_groups"] == n and ri["replica_id"] == r and ri["window"] == W, ri
            seen["n_exec"] += ri["n_exec"]
            _close(held[r])
        seen["cmp"] += tp.check_stores(reps, exp, t)
        seen["ticks"] += 1
    le = run(engs, boundary)
    assert seen["ticks"] == len(snaps) and len(le) == len(lo)
    for (t, a), (_, b) in zip(le, lo):
        assert len(a) == len(b), t
        for x, y in zip(a, b):
            for k in y:
                assert np.array_equal(x[k], y[k]) if isinstance(y[k], np.ndarray) else x[k] == y[k], (t, y["kind"], k)
    assert max(int(r.replica.dump()["len"].max()) for r in reps) >= 5 * W
    tot = {k: sum(r.store.counters()[k] for r in reps) for k in ("copied", "rebuilt", "unsatisfied", "rekeyed")}
    assert tot["copied"] > 0 and tot["rebuilt"] > 0 and tot["unsatisfied"] == 0 and seen["cmp"] > 0, (tot, seen)
    assert seen["alias"] > 0 and seen["lone_vote"] > 0 and seen["bytes"] > 0 and seen["n_exec"] > 0, seen   # ... went through group images
    _close([x.replica for x in reps] + [x.store for x in reps])
    return dict(tot, **seen)


# ---- 3. a move changes object and position -------------------------------------------------------------------------------------------
class Shard:
    """R replicas-with-payload of n_slots groups and the host's table of which job group sits in which slot (-1: none)"""

    def __init__(self, dev, n_slots, R, W, ft, L):
        from summerset_amd import RSPaxosReplicaGroup
        tp = _tp()
        self.n, self.R, self.W = n_slots, R, W
        self.reps, self.engs = tp.make_cluster(dev, n_slots, R, W, ft, L)
        probe = [RSPaxosReplicaGroup(n_slots, R, me=r, window=W, fault_tolerance=ft) for r in range(R)]
        self.fresh = [x.dump() for x in probe]                   # a newly created object's columns
        _close(probe)
        self.tab = np.full(n_slots, -1, np.int64)

    def occupied(self):
        return np.nonzero(self.tab >= 0)[0]

    def free(self):
        return np.nonzero(self.tab < 0)[0]

    def close(self):
        _close([x.replica for x in self.reps] + [x.store for x in self.reps])


# what an empty slot is fed: no timeout, no batch, no message
_QUIET = dict(become_leader=dict(src=NO_REP), req_batch=dict(val=NULL), accept=dict(flags=0), accept_replies=dict(flags=0), prepare=dict(flags=0),
              prepare_replies=dict(pr_n=0), reconstruct=dict(flags=0, rc_n=0), reconstruct_reply=dict(flags=0, rr_n=0), heartbeat=dict(flags=0),
              bcast_heartbeat=dict(flags=0))
_POSITIONAL = dict(become_leader=("src",), req_batch=("val",), bcast_heartbeat=("flags",))


class JobRep:
    """replica r of the whole job for rsp_cluster.tick: every handler call gathered by the shards' tables, run on replica r of
    every shard, scattered back into the job's arrays"""

    def __init__(self, job, r):
        self.job, self.r, self.me, self._polls = job, r, r, []

    def preset_leader(self, leader):
        for sh in self.job.shards:
            sh.engs[self.r].preset_leader(leader)
            if len(sh.free()):
                sh.reps[self.r].reset_groups(sh.free())          # (a preset reaches the empty slots too)

    def __getattr__(self, name):
        if name not in _QUIET:
            raise AttributeError(name)

        def call(*a, **kw):
            kw.update(zip(_POSITIONAL.get(name, ()), a))
            J, out = self.job.J, None
            for sh in self.job.shards:
                occ = sh.tab >= 0
                j = np.where(occ, sh.tab, 0)
                args = {}
                for k, v in kw.items():
                    x = np.asarray(v)[..., j]
                    if k in _QUIET[name]:
                        x = np.where(occ, x, np.asarray(_QUIET[name][k]).astype(x.dtype))
                    args[k] = np.ascontiguousarray(x.astype(np.asarray(v).dtype))
                eng = sh.engs[self.r]
                o = eng(name)(**args)
                g, s, v = eng._polls.pop()
                self._polls.append((sh.tab[g].astype(np.uint32), s, v))
                if o is not None:
                    out = out if out is not None else {k: np.zeros(x.shape[:-1] + (J,), x.dtype) for k, x in o.items()}
                    for k, x in o.items():
                        out[k][..., sh.tab[occ]] = x[..., occ]
            self.job.after_call(name, self.r)
            return out
        return call

    def dump(self):
        out = None
        for sh in self.job.shards:
            d = sh.reps[self.r].replica.dump()
            occ = sh.occupied()
            out = out if out is not None else {k: (np.zeros_like(x) if k == "counters" else np.zeros(x.shape[:-1] + (self.job.J,), x.dtype)) for k, x in d.items()}
            for k, x in d.items():
                if k == "counters":
                    out[k] += x                                  # events stay counted where they happened: the sum is the job's
                else:
                    out[k][..., sh.tab[occ]] = x[..., occ]
        return out

    def is_leader(self):
        return (self.dump()["leader"] == self.me).astype(np.uint8)

    def take_executed(self):
        cols = [np.concatenate([p[i] for p in self._polls]) if self._polls else np.zeros(0, np.uint32) for i in range(3)]
        self._polls = []
        k = np.argsort(cols[0], kind="stable")
        return tuple(x[k] for x in cols)


class _Eng:
    """rc.NumpyEngine with its handlers reachable by name"""

    def __init__(self, eng):
        self.x = eng

    def __call__(self, name):
        return getattr(self.x, name)

    def __getattr__(self, name):
        return getattr(self.x, name)


class Job:
    def __init__(self, dev, oracle, J, sizes, R, W, ft, L, seed, every, cluster):
        self.J, self.R, self.cluster = J, R, cluster
        self.shards = [Shard(dev, n, R, W, ft, L) for n in sizes]
        for sh in self.shards:
            sh.engs = [_Eng(x) for x in sh.engs]
        self.rng = np.random.default_rng(seed)
        perm = self.rng.permutation(J)
        n0 = J * sizes[0] // sum(sizes)
        for sh, jobs in zip(self.shards, (perm[:n0], perm[n0:])):
            sh.tab[self.rng.permutation(sh.n)[:len(jobs)]] = jobs
        self.reps = [JobRep(self, r) for r in range(R)]
        self.calls, self.every, self.running = 0, every, False
        self.cov = dict(moves=0, inside_tick=0, crosses_tile=0, moved=0, exec_moved=0, alias_moved=0, votes_moved=0, reused=0, bytes=0)
        self.left = [set() for _ in self.shards]

    def after_call(self, name, r):
        self.calls += 1
        if self.running and self.calls % self.every == 0:
            self.move(inside=True)

    def move(self, inside=False, k=None, s=None):
        """k seeded groups from shard s into free slots of the other, at other indices"""
        from summerset_amd import move_rsp_groups
        rng = self.rng
        s = int(rng.integers(0, 2)) if s is None else s
        src, dst = self.shards[s], self.shards[1 - s]
        if len(src.occupied()) < 2 or len(dst.free()) < 1:
            src, dst, s = dst, src, 1 - s
        k = int(min(rng.integers(1, 24) if k is None else k, len(src.occupied()) - 1, len(dst.free())))
        ss, ds = rng.permutation(src.occupied())[:k], rng.permutation(dst.free())[:k]
        before = [x.replica.dump() for x in src.reps]
        polls = [(a.replica.exec_poll(), b.replica.exec_poll()) for a, b in zip(src.reps, dst.reps)]
        sd = [StoreDump(x.store) for x in src.reps]
        dd = [StoreDump(x.store) for x in dst.reps]
        stay_s, stay_d = np.setdiff1d(np.arange(src.n), ss), np.setdiff1d(np.arange(dst.n), ds)
        if self.cluster:
            snaps = move_rsp_groups(src.reps, ss, dst.reps, ds)
            held = list(snaps[0]) + list(snaps[1])
        else:
            held = []
            for a, b in zip(src.reps, dst.reps):
                h = a.save_groups(ss)
                b.load_groups(h, ds)
                a.reset_groups(ss)
                held += list(h)
        for r in range(self.R):
            da, db = src.reps[r].replica.dump(), dst.reps[r].replica.dump()
            rep_columns_equal(db, ds, before[r], ss, "moved groups, rep %d" % r)
            rep_columns_equal(da, ss, src.fresh[r], ss, "vacated slots, rep %d" % r)
            rep_columns_equal(da, stay_s, before[r], stay_s, "beside the vacated slots, rep %d" % r)
            assert np.array_equal(da["counters"], before[r]["counters"]), (r, "the source's counters stay")
            want = polls_of(polls[r][0], ss)                     # the unpolled executions travel with their group
            got_s, got_d = src.reps[r].replica.exec_poll(), dst.reps[r].replica.exec_poll()
            assert polls_of(got_d, ds) == want and not polls_of(got_s, ss), (r, "exec list")
            assert polls_of(got_d, stay_d) == polls_of(polls[r][1], stay_d) and polls_of(got_s, stay_s) == polls_of(polls[r][0], stay_s), (r, "exec list")
            self.cov["exec_moved"] += sum(len(v) for v in want.values())
            na, nb = StoreDump(src.reps[r].store), StoreDump(dst.reps[r].store)
            self.cov["bytes"] += store_columns_equal(nb, ds, sd[r], ss, "moved rows, rep %d" % r, tail_of=dd[r])
            store_groups_null(na, ss, ("vacated rows", r))
            store_groups_unchanged(na, sd[r], stay_s, ("beside the vacated rows", r))
            store_groups_unchanged(nb, dd[r], stay_d, ("beside the moved rows", r))
            for p in range(2):                                   # a vacated slot's row bytes are not touched (read_row follows an
                for w in range(src.W):                           # alias into the REQS row: those shards read differently once it is gone)
                    own = ((sd[r].alias[w][None, :] >> np.arange(self.R)[:, None]) & 1) == 0 if p == 1 else np.ones((self.R, src.n), bool)
                    assert np.array_equal(na.rows[p][w][own], sd[r].rows[p][w][own]), (r, p, w, "reset touched row bytes")
            assert na.counters == sd[r].counters and nb.counters == dd[r].counters, (r, "store counters stay")
            self.cov["alias_moved"] += int((sd[r].alias[:, ss] != 0).sum())
            self.cov["votes_moved"] += int((sd[r].hdr[1]["tok"][:, ss] != NULL).sum())
        _close(held)
        self.cov["moves"] += 1; self.cov["moved"] += k; self.cov["inside_tick"] += int(inside)
        self.cov["crosses_tile"] += int(src.n > 64 and (ss < 64).any() and (ss >= 64).any())
        self.cov["reused"] += len(self.left[1 - s] & set(ds.tolist()))
        self.left[s] |= set(ss.tolist())
        dst.tab[ds] = src.tab[ss]
        src.tab[ss] = -1


def move_between_shards(dev, oracle, cluster, J=80, sizes=(70, 40), R=3, ft=1, W=8, L=61, T=21, loss=0.1, every=23):
    """Shards A and B under rsp_scenarios.run as ONE job (leader 0, then replica 1 in the even groups, then replica 2 in half of
    them: moves happen under leaders other than replica 0 and in front of a leader change, whose PrepareReplies then come out of
    moved VOTED cells); behind every `every`-th handler call and after every tick groups move A -> B or B -> A into free slots at
    other indices.  The job's message log, executed lists and dumps are the oracle cluster's, tick by tick"""
    tp = _tp()
    run = lambda reps, on_tick: sc.run(reps, J, T, seed=J + ft, loss=loss, on_tick=on_tick)
    orcs, lo, snaps, execd = e.oracle_run(oracle, run, J, R, W, ft)
    cov = e.reach(orcs, lo)
    assert cov["longest"] > 2 * W, cov
    assert sum(1 for _, out in lo for m in out if m["kind"] == "prepare_reply" and m["voted"] > 0) > 0, "PrepareReplies that carry votes"
    job = Job(dev, oracle, J, sizes, R, W, ft, L, seed=29, every=every, cluster=cluster)
    exp = tp.Expect(oracle, R, R // 2 + 1, L)
    n_cmp = [0]

    def boundary(t):
        for r in range(R):
            for x, y in zip(job.reps[r].take_executed(), execd[t][r]):
                assert np.array_equal(x, y), (t, r, "executed", len(x), len(y))
            dumps_equal(job.reps[r].dump(), snaps[t][r], (t, r))
        for sh in job.shards:
            n_cmp[0] += tp.check_stores(sh.reps, exp, t)
        job.move(k=12 if t % 4 == 1 else None, s=0 if t % 4 == 1 else None)
        for r in range(R):
            dumps_equal(job.reps[r].dump(), snaps[t][r], (t, r, "after the move"))
        for sh in job.shards:
            n_cmp[0] += tp.check_stores(sh.reps, exp, (t, "after the move"))
    job.running = True
    le = run(job.reps, boundary)
    job.running = False
    assert len(le) == len(lo)
    for (t, a), (_, b) in zip(le, lo):
        assert len(a) == len(b), t
        for x, y in zip(a, b):
            for k in y:
                assert np.array_equal(x[k], y[k]) if isinstance(y[k], np.ndarray) else x[k] == y[k], (t, y["kind"], k)
    cv = job.cov
    assert cv["inside_tick"] > 0 and cv["moves"] > cv["inside_tick"] and cv["crosses_tile"] > 0 and cv["reused"] > 0, cv
    assert cv["exec_moved"] > 0 and cv["alias_moved"] > 0 and cv["votes_moved"] > 0 and cv["bytes"] > 0 and n_cmp[0] > 0, cv
    for sh in job.shards:
        sh.close()
    return cv


# ---- 4. interchange and canonical bytes ----------------------------------------------------------------------------------------------
def interchange_replica(dev, oracle, G=130, R=5, ft=1, L=61, n=65):
    """save_groups(list) of a replica == save_state of an n-group replica that holds those groups in list order (made by
    load_state of the group image), byte for byte; the image parses as DESIGN.md 2's image of n groups with the oracle's columns;
    and that object's whole-state image loads back through another list"""
    from summerset_amd import RSPaxosReplicaGroup
    reps, want, _ = finished_cluster(dev, oracle, G, R, ft, L)
    W = reps[0].W
    rng = np.random.default_rng(31)
    n = min(n, G)
    for r, name in ((1, "random"), (R - 1, "descending")):
        lst = rng.permutation(G)[:n] if name == "random" else np.sort(rng.permutation(G)[:n])[::-1].copy()
        a = reps[r].replica
        snap = a.save_groups(lst)
        img = snap.export()
        h, ctr, s, slots, held, execs = Layout(n, R).parse(img, W)
        assert not ctr.any(), "a group image holds zero counters"
        d = want[r]
        for nm in ("leader", "bal_prep_sent", "bal_prepared", "bal_max_seen", "len", "commit_bar", "exec_bar", "snap_bar", "peer_exec_bar", "digest"):
            assert np.array_equal(s[nm], d[nm][..., lst]), (name, nm)
        for nm, dn in c.DUMP_OF.items():
            assert np.array_equal(slots[nm], np.where(held, d[dn][:, lst], 0)), (name, nm)
        poll = a.exec_poll()
        got = {}
        for x, _, slot in sorted(execs):
            got.setdefault(x, []).append(slot)
        assert got == {i: [sl for sl, _ in v] for i, v in polls_of(poll, lst).items()}, (name, "exec list")
        small = RSPaxosReplicaGroup(n, R, me=r, window=W, fault_tolerance=ft)
        small.load_state(snap)                                   # a group image IS an n-group replica's image
        rep_columns_equal(small.dump(), np.arange(n), d, lst, name)
        again = small.save_state()
        assert again.export() == img, (name, "the two kinds of image differ")
        other = RSPaxosReplicaGroup(G, R, me=r, window=W, fault_tolerance=ft)
        lst2 = rng.permutation(G)[:n]
        other.load_groups(again, lst2)                           # ... and an n-group replica's image loads through a list
        rep_columns_equal(other.dump(), lst2, d, lst, name + ", back through a list")
        assert polls_of(other.exec_poll(), lst2) == polls_of(poll, lst), (name, "exec list")
        assert not other.dump()["counters"].any()
        _close([snap, small, again, other])


def _fill_store(dev, oracle, st, G, n, d, W, L, seed=5, rounds=2, first=0):
    """store_canonical_bytes' content: every row holds a payload of L bytes, then -- the ring wrapped -- one of 1 .. 16 bytes (never a
    zero byte, so what a longer payload left behind a short shard shows).  -> {(row, group): the oracle's codeword of what it holds}"""
    import torch
    rng = np.random.default_rng(seed)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    want = {}
    for slot in range(first * W, rounds * W):
        lens = np.full(G, L, np.uint32) if slot < W else rng.integers(1, 17, G).astype(np.uint32)
        data = rng.integers(1, 256, (G, L), dtype=np.uint8)
        tok = (1 + slot * G + np.arange(G)).astype(np.uint32)
        a_slot, a_val = np.zeros((W, G), np.uint32), np.zeros((W, G), np.uint32)
        a_slot[0], a_val[0] = slot, tok
        st.put(dict(a_n=t(np.ones(G, np.int32)), a_slot=t(a_slot.view(np.int32)), a_val=t(a_val.view(np.int32))), t(data), t(lens.view(np.int32)))
        for g in range(G):
            bts = data[g, :lens[g]]
            sl = oracle.rs_shard_len(bts.size, d)
            cw = np.zeros((n, sl), np.uint8)
            cw[:d].reshape(-1)[:bts.size] = bts
            cw[d:] = oracle.rs_encode(d, n - d, bts)
            want[(slot & (W - 1), g)] = cw
    return want


def interchange_store(dev, oracle, n=5, d=3, G=70, W=8, L=333, k=37):
    """the RSPaxos store with store_canonical_bytes' content (L = 333 with d = 3, then 1 .. 16 bytes after the ring wrapped: shard
    lengths that are no multiple of 16, cells with dlen < d): save_groups(list) == save of a k-group store holding those groups in
    list order, byte for byte; every pad region zero (StoreLayout.parse), every shard the oracle's; back through a list into a store
    of another max_data_len"""
    from summerset_amd import RSPaxosPayloadStore
    a = RSPaxosPayloadStore(G, n, W, L, num_data_shards=d)
    want = _fill_store(dev, oracle, a, G, n, d, W, L)
    assert a.read_row(W, 0)[0, 0, 16:a.group_stride].any()       # the rows do hold bytes of the longer payloads behind the short shards
    rng = np.random.default_rng(37)
    k = min(k, G)
    lst = rng.permutation(G)[:k]
    snap = a.save_groups(lst)
    img = snap.export()
    h, ctr, arr, shards = StoreLayout(k, W, 2).parse(img, d)
    assert not ctr.any() and h[8] <= 16 and h[11] == n * k * W == len(shards), h
    for (p, r, x, s), bts in shards.items():
        assert p == 0 and bytes(want[(r, int(lst[x]))][s]) == bts, (p, r, x, s)
    small = RSPaxosPayloadStore(k, n, W, 64, num_data_shards=d)
    small.load(snap)                                             # a group image IS a k-group store's image
    again = small.save()
    assert again.export() == img
    da = StoreDump(a)
    store_columns_equal(StoreDump(small), np.arange(k), da, lst, "k-group store")
    other = RSPaxosPayloadStore(G, n, W, L + 100, num_data_shards=d)     # other strides
    lst2 = rng.permutation(G)[:k]
    other.load_groups(again, lst2)
    assert store_columns_equal(StoreDump(other), lst2, da, lst, "back through a list") == n * k * W
    store_groups_null(StoreDump(other, rows=False), np.setdiff1d(np.arange(G), lst2), "unlisted")
    assert other.counters() == dict(copied=0, rebuilt=0, unsatisfied=0, rekeyed=0)
    assert other.save_groups(lst2).export() == img               # canonical: whatever the strides and the positions
    _close([a, snap, small, again, other])


def interchange_voted_plane(dev, oracle, G=130, R=5, ft=1, L=61, n=65):
    """the same for stores with VOTED cells, aliases among them (the finished cluster's)"""
    from summerset_amd import RSPaxosPayloadStore
    reps, _, exp = finished_cluster(dev, oracle, G, R, ft, L)
    W = reps[0].W
    rng = np.random.default_rng(41)
    n = min(n, G)
    seen = dict(alias=0, lone=0)
    for r in range(R):
        a = reps[r].store
        lst = rng.permutation(G)[:n]
        snap = a.save_groups(lst)
        img = snap.export()
        h, ctr, arr, shards = StoreLayout(n, W, 2).parse(img, a.d)
        da = StoreDump(a)
        assert not ctr.any() and np.array_equal(arr[("alias", 1)], np.where(da.hdr[1]["tok"][:, lst] != NULL, da.alias[:, lst] & da.hdr[1]["avail"][:, lst], 0))
        for (p, w, x, s), bts in shards.items():
            assert bytes(exp.shards(arr[("tok", p)][w, x])[0][s]) == bts, (r, p, w, x, s)
        seen["alias"] += int((arr[("alias", 1)] != 0).sum()); seen["lone"] += sum(1 for key in shards if key[0] == 1)
        small = RSPaxosPayloadStore(n, R, W, max_data_len=L + 100)
        small.load(snap)
        again = small.save()
        assert again.export() == img, (r, "the two kinds of image differ")
        store_columns_equal(StoreDump(small), np.arange(n), da, lst, "n-group store %d" % r)
        _close([snap, small, again])
    assert seen["alias"] > 0 and seen["lone"] > 0, seen


def interchange_craft_store(dev, oracle, R=5, G=40, W=8, L=200, T=12, k=23):
    """the one-plane CRaft store (craft_payload_loop.Loop's, ragged payloads of 1 .. L bytes, the ring wrapped, the last follower cut
    off for three ticks): of the leader's store and of two followers', save_groups(list) == save of a k-group CRaft store holding
    those groups in list order (made by `load` of the group image), byte for byte; the image parses as a one-plane image (no alias
    section, craft = 1), every pad region zero, every shard the oracle's codeword of the batch appended at that (slot, term); back
    through a list into a CRaft store of another max_data_len; and an n-group RSPaxos store refuses it"""
    import craft_payload_loop as cl
    from summerset_amd import CRaftPayloadStore, RSPaxosPayloadStore
    lp = cl.Loop(dev, oracle, G=G, R=R, W=W, L=L, seed=5, many=False)
    for t in range(T):
        lp.tick(p_new=1.0, skip=(R - 1,) if 3 <= t <= 5 else ())
    assert int(lp.reps[0].dump()["log_len"].max()) > W
    by_tok = {(g, cl.craft_token(s_, term)): v for (g, s_, term), v in lp.book.items()}
    rng = np.random.default_rng(97)
    k, d, n_sh, odd = min(k, G), lp.d, 0, 0
    for r in (0, 1, R - 1):
        a = lp.stores[r]
        lst = rng.permutation(G)[:k]
        snap = a.save_groups(lst)
        img = snap.export()
        lay = StoreLayout(k, W, 1)
        assert ("alias", 1) not in lay.at
        h, ctr, arr, shards = lay.parse(img, d)
        assert h[6] == 1 and h[7] == 1 and h[4] == R and h[5] == d and not ctr.any(), h
        da = StoreDump(a)
        for key in ("tok", "dlen", "avail"):
            some = da.hdr[0]["tok"][:, lst] != NULL
            assert np.array_equal(arr[(key, 0)], np.where(some, da.hdr[0][key][:, lst], NULL if key == "tok" else 0)), (r, key)
        assert len(shards) > 0
        for (p, w, x, s_), bts in shards.items():
            data, cw = by_tok[(int(lst[x]), int(arr[("tok", 0)][w, x]))]
            assert p == 0 and int(arr[("dlen", 0)][w, x]) == len(data) and bytes(cw[s_]) == bts, (r, w, x, s_)
            odd += int(cw.shape[1] % 16 != 0)
        n_sh += len(shards)
        small = CRaftPayloadStore(k, R, W, max_data_len=L + 37)
        small.load(snap)                                         # a group image IS a k-group CRaft store's image
        again = small.save()
        assert again.export() == img, (r, "the two kinds of image differ")
        store_columns_equal(StoreDump(small), np.arange(k), da, lst, "k-group CRaft store %d" % r)
        other = CRaftPayloadStore(G, R, W, max_data_len=L + 100)   # other strides
        lst2 = rng.permutation(G)[:k]
        other.load_groups(again, lst2)
        assert store_columns_equal(StoreDump(other), lst2, da, lst, "back through a list") == len(shards)
        store_groups_null(StoreDump(other, rows=False), np.setdiff1d(np.arange(G), lst2), "unlisted")
        back = other.save_groups(lst2)
        assert back.export() == img                              # canonical: whatever the strides and the positions
        rsp = RSPaxosPayloadStore(k, R, W, max_data_len=L)
        _refused(lambda: rsp.load(snap), "made for")
        _close([snap, small, again, other, back, rsp])
    assert n_sh > k * W and odd > 0, (n_sh, odd)                 # full rings; shard lengths that are no multiple of 16
    _close(lp.reps + lp.stores)


# ---- 5. neighbours untouched ---------------------------------------------------------------------------------------------------------
def neighbours_untouched_store(dev, oracle, n=5, d=3, G=70, W=8, L=100, k=23):
    """every row byte of a store written (the region behind the shards' lengths included), a full dump noted; after a load_groups
    and a reset_groups every unlisted group's headers, alias bytes and WHOLE row bytes and the counters are what they were; of the
    listed groups the bytes behind each shard's length are what they were"""
    import torch
    from summerset_amd import RSPaxosPayloadStore
    from summerset_amd.rsp_payload import REQS, VOTED
    t = lambda x: torch.from_numpy(np.ascontiguousarray(x)).to(dev)
    a, b = RSPaxosPayloadStore(G, n, W, L, num_data_shards=d), RSPaxosPayloadStore(G, n, W, L + 50, num_data_shards=d)
    wb = _fill_store(dev, oracle, b, G, n, d, W, L, seed=8, rounds=1)
    full = t(np.full(G, (1 << n) - 1, np.uint8))
    for rnd in range(2):                                         # long payloads, then short ones over them, in both planes: the VOTED
        _fill_store(dev, oracle, a, G, n, d, W, L, seed=7 + rnd, rounds=rnd + 1, first=rnd)   # rows take the REQS rows' shards as votes
        for w in range(W):                                       # stored on their own
            slot = t(np.full(G, rnd * W + w, np.int32))
            a.ingest(a.extract(slot, full, REQS), slot, VOTED)
    d0 = StoreDump(a)
    assert d0.rows[0][0][0, 0, 16:].any() and (d0.hdr[1]["tok"] != NULL).all() and d0.rows[1][0][0, 0, 16:].any()
    rng = np.random.default_rng(43)
    la, lb = rng.permutation(G)[:k], rng.permutation(G)[:k]
    snap = b.save_groups(lb)
    a.load_groups(snap, la)
    d1 = StoreDump(a)
    rest = np.setdiff1d(np.arange(G), la)
    store_groups_unchanged(d1, d0, rest, "beside a load")
    assert d1.counters == d0.counters and d1.delivered == d0.delivered
    assert store_columns_equal(d1, la, StoreDump(b), lb, "loaded", tail_of=d0) == n * k * W
    for w in range(W):                                           # b has no VOTED cells: a's become null, their row bytes stay
        assert (d1.hdr[1]["tok"][:, la] == NULL).all() and np.array_equal(d1.rows[1][w], d0.rows[1][w])
        cw = wb[(w, int(lb[0]))]
        assert np.array_equal(d1.rows[0][w][:, la[0], :cw.shape[1]], cw)
    lc = rng.permutation(G)[:k]
    a.reset_groups(lc)
    d2 = StoreDump(a)
    store_groups_unchanged(d2, d1, np.setdiff1d(np.arange(G), lc), "beside a reset")
    store_groups_null(d2, lc, "reset")
    for p in range(2):
        for w in range(W):
            assert np.array_equal(d2.rows[p][w], d1.rows[p][w]), (p, w, "a reset touched row bytes")
    assert d2.counters == d0.counters
    fresh = RSPaxosPayloadStore(G, n, W, L, num_data_shards=d)   # reset is create
    store_columns_equal(StoreDump(a, rows=False), lc, StoreDump(fresh, rows=False), lc, "reset is create")
    _close([a, b, snap, fresh])


def neighbours_untouched_replica(dev, oracle, G=130, R=5, ft=1, L=61, k=37):
    """a copy of the finished cluster's replica: after a load_groups (other groups' state) and a reset_groups every unlisted
    group's dump columns, the exec list and the counters are what they were; reset slots equal a new object's.  (What the dump
    cannot show -- ring cells outside the live span -- is ring_cells_outside_the_live_span's, below)"""
    from summerset_amd import RSPaxosReplicaGroup
    reps, want, _ = finished_cluster(dev, oracle, G, R, ft, L)
    W, r = reps[0].W, 2 % R
    a = RSPaxosReplicaGroup(G, R, me=r, window=W, fault_tolerance=ft)
    whole = reps[r].replica.save_state()
    a.load_state(whole)
    d0, p0 = a.dump(), a.exec_poll()
    dumps_equal(d0, want[r], "copy")
    rng = np.random.default_rng(47)
    la, lb = rng.permutation(G)[:k], rng.permutation(G)[:k]
    snap = reps[r].replica.save_groups(lb)
    a.load_groups(snap, la)
    d1 = a.dump()
    rest = np.setdiff1d(np.arange(G), la)
    rep_columns_equal(d1, rest, d0, rest, "beside a load")
    rep_columns_equal(d1, la, d0, lb, "loaded")
    assert np.array_equal(d1["counters"], d0["counters"])
    assert polls_of(a.exec_poll(), rest) == polls_of(p0, rest) and polls_of(a.exec_poll(), la) == polls_of(p0, lb)
    lc = rng.permutation(G)[:k]
    a.reset_groups(lc)
    d2 = a.dump()
    rest = np.setdiff1d(np.arange(G), lc)
    rep_columns_equal(d2, rest, d1, rest, "beside a reset")
    fresh = RSPaxosReplicaGroup(G, R, me=r, window=W, fault_tolerance=ft)
    rep_columns_equal(d2, lc, fresh.dump(), lc, "reset is create")
    assert np.array_equal(d2["counters"], d0["counters"]) and not polls_of(a.exec_poll(), lc)
    _close([a, whole, snap, fresh])


class RawArena:
    """the bytes of a replica object's device allocation (`smr_rsp_debug_arena_view`), read and painted as bytes.  Nothing here
    knows the layout inside: which bytes belong to which group is LEARNED, by painting a new object and resetting those groups"""

    def __init__(self, rep, dev):
        import ctypes as C
        from summerset_amd import _lib
        base, n = C.c_void_p(), C.c_uint64()
        _lib.check(_lib.load().smr_rsp_debug_arena_view(rep._h, C.byref(base), C.byref(n)))
        self.base, self.n, self.C, self.dev = base.value, int(n.value), C, dev
        self.hip = None
        if str(dev) != "cpu":
            self.hip = C.CDLL("libamdhip64.so")
            self.hip.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
            self.hip.hipMemset.argtypes = [C.c_void_p, C.c_int, C.c_size_t]

    def _sync(self):
        if self.hip is not None:
            import torch
            torch.cuda.synchronize()

    def read(self):
        self._sync()
        out = np.zeros(self.n, np.uint8)
        if self.hip is None:
            self.C.memmove(out.ctypes.data, self.base, self.n)
        else:
            assert self.hip.hipMemcpy(out.ctypes.data, self.base, self.n, 2) == 0     # hipMemcpyDeviceToHost
        return out

    def paint(self, byte):
        self._sync()
        if self.hip is None:
            self.C.memset(self.base, byte, self.n)
        else:
            assert self.hip.hipMemset(self.base, byte, self.n) == 0
        self._sync()


def ring_cells_outside_the_live_span(dev, oracle, G=130, R=5, ft=1, L=61, k=37, young=3):
    """smr_rsp_dump gives null instances outside a group's live span, so what a load or reset does THERE is looked at in the
    object's raw bytes.  PAINT = 0xA5 is no initial value.  (1) A new object painted all over and reset through a list: the bytes
    that changed are the footprint of those groups -- for all G groups exactly every per-group word, all W ring rows and the
    execution list's rows included (53 + 4 R bytes of scalars, 59 per ring row).  (2) A painted object takes the finished
    replica by load_state (dead cells stay painted); then a load_groups writes inside its list's footprint only, and of groups
    `young` instances long only their scalars, `young` ring rows and the list's rows at most; a reset_groups writes inside
    its list's footprint only and leaves there, byte for byte, what a newly created object holds"""
    import torch
    from summerset_amd import RSPaxosReplicaGroup
    PAINT = 0xA5
    reps, want, _ = finished_cluster(dev, oracle, G, R, ft, L)
    W, r = reps[0].W, 1
    mk = lambda: RSPaxosReplicaGroup(G, R, me=r, window=W, fault_tolerance=ft)   # noqa: E731

    def footprint(lst):
        p = mk()
        raw = RawArena(p, dev)
        raw.paint(PAINT)
        p.reset_groups(lst)
        f = raw.read() != PAINT
        p.close()
        return f
    per_group = 53 + 4 * R + 59 * W
    f_all = footprint(np.arange(G))
    assert int(f_all.sum()) == G * per_group, (int(f_all.sum()), G * per_group)
    rng = np.random.default_rng(89)
    la, lb, lc, ly = (rng.permutation(G)[:k] for _ in range(4))
    fa, fc, fy = footprint(la), footprint(lc), footprint(ly)
    for f in (fa, fc, fy):
        assert int(f.sum()) == k * per_group and not (f & ~f_all).any()
    x = mk()
    raw = RawArena(x, dev)
    raw.paint(PAINT)
    whole = reps[r].replica.save_state()
    x.load_state(whole)
    dumps_equal(x.dump(), want[r], "painted, loaded")
    r0 = raw.read()
    assert ((r0 == PAINT) & f_all).any(), "no dead cell is left painted"
    snap = reps[r].replica.save_groups(lb)
    x.load_groups(snap, la)
    r1 = raw.read()
    ch = r1 != r0
    assert ch.any() and not (ch & ~fa).any(), "a load through a list wrote outside its groups"
    src = mk()                                                   # groups `young` instances long: W - young dead ring rows each
    src.preset_leader(r)
    for t in range(young):
        src.req_batch(torch.from_numpy((1 + t * G + np.arange(G)).astype(np.int32)).to(dev))
    assert (src.dump()["len"] == young).all() and young < W
    ys = src.save_groups(ly)
    x.load_groups(ys, ly)
    r2 = raw.read()
    ch = r2 != r1
    assert ch.any() and not (ch & ~fy).any(), "a load through a list wrote outside its groups"
    assert int(ch.sum()) <= k * (53 + 4 * R + young * 55 + 4 * W), "a load wrote ring rows outside the live span"
    assert int(((r2 == PAINT) & fy).sum()) > 0
    d = x.dump()
    rep_columns_equal(d, ly, src.dump(), ly, "young groups")
    x.reset_groups(lc)
    r3 = raw.read()
    ch = r3 != r2
    assert ch.any() and not (ch & ~fc).any(), "a reset wrote outside its groups"
    z = mk()
    assert np.array_equal(r3[fc], RawArena(z, dev).read()[fc]), "a reset slot is not a new object's, over all W ring rows"
    assert not ((r3 != r0) & ~f_all).any()                       # (the counters and every gap: never touched)
    keep = np.setdiff1d(np.arange(G), np.concatenate([la, ly, lc]))
    rep_columns_equal(x.dump(), keep, want[r], keep, "every group no list named")
    _close([x, whole, snap, src, ys, z])


# ---- 6. reset is create, and a reset slot runs from scratch ------------------------------------------------------------------------
def reset_then_run_from_scratch(dev, oracle, G=40, R=3, ft=1, L=61, W=8, T1=12, T2=14, loss=0.05, k=17):
    """a cluster runs T1 ticks under leader 0 (rings wrapped); then k seeded groups are reset in all replicas and stores and the run
    goes on: replica 1 times out in the reset groups (they know no leader) and leads them from slot 0, while the neighbours go on
    under leader 0.  Tick by tick the reset groups' columns are those of a FRESH oracle cluster fed the same ticks, the
    neighbours' those of the oracle cluster that ran from the start; the executed lists are the two oracles' by group; the stores
    hold the engine's masks and the oracle's codewords, rows of the slots' earlier life under the new ones"""
    tp = _tp()
    rng = np.random.default_rng(53)
    lst = np.sort(rng.permutation(G)[:k])
    in_lst = np.zeros(G, bool); in_lst[lst] = True
    rest = np.nonzero(~in_lst)[0]
    g = np.arange(G)
    kinds = ("accept", "accept_reply", "prepare", "prepare_reply", "recon", "recon_reply", "hb")
    ticks = []
    for t in range(T2):                                          # the second phase's inputs, made once and fed to all three clusters
        val = (1 + (T1 + t) * G + g).astype(np.uint32)
        val[rng.random(G) < 0.1] = NULL
        to = None
        if t == 0:
            to = [np.full(G, NO_REP, np.uint8) for _ in range(R)]
            to[1] = np.where(in_lst, 0, NO_REP).astype(np.uint8)
        target = np.where(in_lst & (t > 0), 1, 0).astype(np.uint8)
        drop = {(kd, a, b): rng.random(G) < loss for kd in kinds for a in range(R) for b in range(R) if a != b}
        ticks.append((val, target, to, drop, t % 3 == 2))

    def phase2(reps, on_tick):
        for t, (val, target, to, drop, hb) in enumerate(ticks):
            rc.tick(reps, val, target, timeouts=to, drop=drop, heartbeat=hb)
            on_tick(t)
    first = lambda reps: sc.run(reps, G, T1, seed=3, loss=loss, changes=False)   # noqa: E731
    old = [oracle.RspOracle(G, R, me=r, W=W, fault_tolerance=ft) for r in range(R)]
    new = [oracle.RspOracle(G, R, me=r, W=W, fault_tolerance=ft) for r in range(R)]
    first(old)
    assert max(int(o.dump()["len"].max()) for o in old) > W
    for o in old:
        o.take_executed()
    want_old, want_new, ex_old, ex_new = [], [], [], []
    phase2(old, lambda t: (want_old.append([o.dump() for o in old]), ex_old.append([o.take_executed() for o in old])))
    phase2(new, lambda t: (want_new.append([o.dump() for o in new]), ex_new.append([o.take_executed() for o in new])))
    assert int(want_new[-1][1]["len"][lst].max()) > W and (want_new[-1][1]["leader"][lst] == 1).all(), "the reset groups elect replica 1 and wrap their rings"
    assert sum(len(x[0]) for t in range(T2) for x in ex_new[t]) > 0
    reps, engs = tp.make_cluster(dev, G, R, W, ft, L)
    exp = tp.Expect(oracle, R, R // 2 + 1, L)
    first(engs)
    fresh = tp.make_cluster(dev, G, R, W, ft, L)[0]
    for x, f in zip(reps, fresh):
        x.reset_groups(lst)
        rep_columns_equal(x.replica.dump(), lst, f.replica.dump(), lst, "reset is create")
        store_columns_equal(StoreDump(x.store, rows=False), lst, StoreDump(f.store, rows=False), lst, "reset is create")
    _close([f.replica for f in fresh] + [f.store for f in fresh])
    for x in engs:
        x.take_executed()
    n_cmp = [0]

    def pick(ex, keep):
        m = keep[ex[0]]
        return tuple(c_[m] for c_ in ex)

    def boundary(t):
        for r in range(R):
            d = reps[r].replica.dump()
            rep_columns_equal(d, lst, want_new[t][r], lst, "tick %d rep %d, the reset groups" % (t, r))
            rep_columns_equal(d, rest, want_old[t][r], rest, "tick %d rep %d, their neighbours" % (t, r))
            got = engs[r].take_executed()
            polls_equal(pick(got, in_lst), pick(ex_new[t][r], in_lst), (t, r, "reset groups"))
            polls_equal(pick(got, ~in_lst), pick(ex_old[t][r], ~in_lst), (t, r, "neighbours"))
        n_cmp[0] += tp.check_stores(reps, exp, t)
    phase2(engs, boundary)
    assert n_cmp[0] > 0
    _close([x.replica for x in reps] + [x.store for x in reps])


# ---- 7. list shapes ------------------------------------------------------------------------------------------------------------------
def list_shapes(dev, oracle, G=333, R=3, ft=1, L=61, sizes=(330, None)):
    """330 entries (six tiles, two blocks) and n = G, ascending, descending and random: the group image of replica and store is the
    image of the n-group object loaded from it, and loads back through the list into new objects with the same columns"""
    from summerset_amd import RSPaxosPayloadStore, RSPaxosReplicaGroup
    reps, want, exp = finished_cluster(dev, oracle, G, R, ft, L, T=12)
    W = reps[0].W
    rng = np.random.default_rng(59)
    i = 0
    for n in sizes:
        n = G if n is None else min(n, G)
        pick = np.sort(np.concatenate([rng.permutation(G - 1)[:n - 1], [G - 1]]).astype(np.int64))
        for name, lst in (("ascending", pick), ("descending", pick[::-1].copy()), ("random", rng.permutation(pick))):
            r = i % R
            i += 1
            rs, ps = reps[r].save_groups(lst)
            ir, ip = rs.export(), ps.export()
            Layout(n, R).parse(ir, W); StoreLayout(n, W, 2).parse(ip, reps[r].store.d)
            small_r, small_s = RSPaxosReplicaGroup(n, R, me=r, window=W, fault_tolerance=ft), RSPaxosPayloadStore(n, R, W, max_data_len=L)
            small_r.load_state(rs); small_s.load(ps)
            ar, as_ = small_r.save_state(), small_s.save()
            assert ar.export() == ir and as_.export() == ip, (n, name)
            rep_columns_equal(small_r.dump(), np.arange(n), want[r], lst, (n, name))
            big_r, big_s = RSPaxosReplicaGroup(G, R, me=r, window=W, fault_tolerance=ft), RSPaxosPayloadStore(G, R, W, max_data_len=L + 100)
            back = rng.permutation(G)[:n]
            big_r.load_groups(ar, back); big_s.load_groups(as_, back)
            rep_columns_equal(big_r.dump(), back, want[r], lst, (n, name, "back"))
            assert store_columns_equal(StoreDump(big_s), back, StoreDump(reps[r].store), lst, (n, name, "back")) > 0
            if n == G and name == "ascending":                   # the full ascending list: the whole-state image but for the counters
                whole = reps[r].replica.save_state()
                wi = whole.export()
                assert wi[:64] == ir[:64] and wi[96:] == ir[96:] and any(wi[64:96])
                ws = reps[r].store.save()
                wsi = ws.export()
                assert wsi[:64] == ip[:64] and wsi[104:] == ip[104:] and any(wsi[64:104])
                _close([whole, ws])
            _close([rs, ps, small_r, small_s, ar, as_, big_r, big_s])


def permutation_of_a_large_replica(dev, G=66000, R=3, W=8):
    """device only: 1 032 tiles for the launch's 1 024 wavefronts; a replica whose groups all differ (one request each, lengths
    0 .. 2 by group) saved through a permutation, loaded through its inverse into a new object: the same dump; through the
    permutation itself into an n-group object: the permuted columns"""
    import torch
    from summerset_amd import RSPaxosReplicaGroup
    assert (G + 63) // 64 > 1024
    a, b, cc = (RSPaxosReplicaGroup(G, R, me=0, window=W) for _ in range(3))
    a.preset_leader(0)
    g = np.arange(G)
    for k in range(2):
        val = np.where(g % 3 > k, 1 + k * G + g, NULL).astype(np.uint32)
        a.req_batch(torch.from_numpy(val.view(np.int32)).to(dev))
    d = a.dump()
    assert set(np.unique(d["len"]).tolist()) == {0, 1, 2}
    perm = np.random.default_rng(61).permutation(G)
    snap = a.save_groups(perm)
    b.load_state(snap)
    rep_columns_equal(b.dump(), g, d, perm, "permuted")
    cc.load_groups(snap, perm)
    rep_columns_equal(cc.dump(), g, d, g, "and back")
    info = snap.info()
    assert info["n_groups"] == G and info["n_slots"] == int(d["len"].sum()), info
    _close([a, b, cc, snap])


def permutation_of_a_large_store(dev, oracle, n=3, d=2, G=66000, W=8, L=16):
    """device only: store_more_tiles_than_wavefronts' store saved through a permutation and loaded through it into a store of other
    strides: equal stores; sampled shards on both sides of tile, wavefront and block edges of the LIST are the oracle's"""
    import torch
    from summerset_amd import RSPaxosPayloadStore
    sl = (L + d - 1) // d
    a, b = RSPaxosPayloadStore(G, n, W, L, num_data_shards=d), RSPaxosPayloadStore(G, n, W, L + 100, num_data_shards=d)
    gen = torch.Generator(device=dev); gen.manual_seed(13)
    data = torch.randint(0, 256, (G, L), dtype=torch.uint8, device=dev, generator=gen)
    ones = torch.ones(G, dtype=torch.int32, device=dev)
    for slot in range(W):
        a_slot = torch.zeros((W, G), dtype=torch.int32, device=dev); a_slot[0] = slot
        a_val = torch.zeros((W, G), dtype=torch.int32, device=dev); a_val[0] = torch.arange(G, dtype=torch.int32, device=dev) + 1 + slot * G
        a.put(dict(a_n=ones, a_slot=a_slot, a_val=a_val), data.roll(slot, 1))
    perm = np.random.default_rng(67).permutation(G)
    snap = a.save_groups(perm)
    info = snap.info()
    assert info["shard_bytes"] == G * W * n * c.a16(sl) and info["n_shards_stored"] == G * W * n and info["n_groups"] == G, info
    b.load_groups(snap, perm)
    c.stores_equal(b, a, "a permutation of 66 000 groups")
    small = RSPaxosPayloadStore(G, n, W, L, num_data_shards=d)
    small.load(snap)                                             # position x holds group perm[x]
    host = data.cpu().numpy()
    for w in (0, W - 1):
        row = small.read_row(w, 0)
        for x in (0, 63, 64, 127, 128, 511, 512, G // 2, 65535, 65536, G - 17, G - 16, G - 1):
            bts = np.roll(host[perm[x]], w)
            cw = np.zeros((n, sl), np.uint8)
            cw[:d].reshape(-1)[:L] = bts
            cw[d:] = oracle.rs_encode(d, n - d, bts)
            assert np.array_equal(row[:, x, :sl], cw), (w, x)
    _close([a, b, small, snap])


# ---- 8. offsets past 4 GiB (device only) -----------------------------------------------------------------------------------------------
def store_groups_past_4gib(dev, oracle, n=3, d=2, G=4096, W=8, L=88000, k=64):
    """store_past_4gib's store (4.3 GB of rows); the k listed groups come from the top of the group range, where ps_off of the
    last rows lies above 2^32: the image is small, its bytes the oracle's codewords, and it loads into the top of a second store"""
    import torch
    from summerset_amd import RSPaxosPayloadStore
    sl = (L + d - 1) // d
    a = RSPaxosPayloadStore(G, n, W, L, num_data_shards=d)
    assert ((W * n - 1) * G + G - k) * a.group_stride > 2**32     # the listed groups' last shards of the last row
    gen = torch.Generator(device=dev); gen.manual_seed(11)
    data = torch.randint(0, 256, (G, L), dtype=torch.uint8, device=dev, generator=gen)
    ones = torch.ones(G, dtype=torch.int32, device=dev)
    for slot in range(W):
        a_slot = torch.zeros((W, G), dtype=torch.int32, device=dev); a_slot[0] = slot
        a_val = torch.zeros((W, G), dtype=torch.int32, device=dev); a_val[0] = torch.arange(G, dtype=torch.int32, device=dev) + 1 + slot * G
        a.put(dict(a_n=ones, a_slot=a_slot, a_val=a_val), data.roll(slot, 1))
    del a_slot, a_val
    lst = (G - 1 - np.random.default_rng(71).permutation(k)).astype(np.int64)       # the top k groups, shuffled
    snap = a.save_groups(lst)
    info = snap.info()
    assert info["shard_bytes"] == k * W * n * c.a16(sl) and info["n_shards_stored"] == k * W * n and info["bytes"] == StoreLayout(k, W, 2).fixed + info["shard_bytes"], info
    h, ctr, arr, shards = StoreLayout(k, W, 2).parse(snap.export(), d)
    host = data[G - k:].cpu().numpy()
    memo = {}
    for (p, w, x, s), bts in shards.items():
        if x % 9 and w not in (0, W - 1):
            continue
        if (w, x) not in memo:
            b = np.roll(host[int(lst[x]) - (G - k)], w)
            cw = np.zeros((n, sl), np.uint8)
            cw[:d].reshape(-1)[:L] = b
            cw[d:] = oracle.rs_encode(d, n - d, b)
            memo[(w, x)] = cw
        assert p == 0 and bytes(memo[(w, x)][s]) == bts, (w, x, s)
    a_rows = a.read_row(W - 1, 0)[:, G - k:, :sl].copy()
    a.close()                                                    # (two such stores do not fit beside each other comfortably)
    b = RSPaxosPayloadStore(G, n, W, L, num_data_shards=d)
    b.load_groups(snap, lst[::-1].copy())                        # position x -> group G - k + (what lst[k - 1 - x] was above G - k)
    hd = b.dump(0)
    assert (hd["avail"][:, G - k:] == (1 << n) - 1).all() and (hd["dlen"][:, G - k:] == L).all() and (hd["tok"][:, :G - k] == NULL).all()
    row = b.read_row(W - 1, 0)
    for x in range(k):
        assert np.array_equal(row[:, int(lst[k - 1 - x]), :sl], a_rows[:, int(lst[x]) - (G - k)]), x
    _close([b, snap])


# ---- 9. the CRaft store --------------------------------------------------------------------------------------------------------------
def craft_move(dev, oracle, R=3, G=40, W=8, L=200, T=12):
    """craft_shadow_stores' loop; every third tick ALL groups move (two lists, shuffled targets) from the live replica objects and
    stores into spares of another max_data_len, at other indices, with move_craft_groups; the loop's book is re-keyed by the same
    permutation and goes on with the spares.  The moved rows are present at once (`lp.check`), a quiet tick behind the move copies
    and rebuilds nothing, later commits still read back the oracle's bytes.  A CRaft group image into an RSPaxos store, and the
    reverse, are refused"""
    import craft_payload_loop as cl
    from summerset_amd import CRaftLeaderGroup, CRaftPayloadStore, RSPaxosPayloadStore, move_craft_groups
    lp = cl.Loop(dev, oracle, G=G, R=R, W=W, L=L, seed=3, many=False)
    rng = np.random.default_rng(73)
    moved = 0
    for t in range(T):
        lp.tick(p_new=1.0, skip=(R - 1,) if 3 <= t <= 5 else ())
        if t % 3 != 2 or 3 <= t <= 5:
            continue
        lp.tick(p_new=0.0); lp.tick(p_new=0.0)                    # (everybody has caught up and learned the commit index)
        sp_rep = [CRaftLeaderGroup(G, R, leader_id=r, window=W, term=1, fault_tolerance=1) for r in range(R)]
        sp_st = [CRaftPayloadStore(G, R, W, max_data_len=L + 100 * (1 + t % 2)) for _ in range(R)]
        perm = rng.permutation(G)
        cut = int(rng.integers(1, G))
        before = [StoreDump(s) for s in lp.stores]
        for lst in (np.arange(cut), np.arange(cut, G)):
            lst = rng.permutation(lst)
            rs, ps = move_craft_groups(lp.reps, lp.stores, lst, sp_rep, sp_st, perm[lst])
            for s in ps:
                info = s.info()
                assert info["planes"] == 1 and info["craft"] == 1 and info["n_groups"] == len(lst), info
                moved += info["shard_bytes"]
            _close(list(rs) + list(ps))
        for r in range(R):
            store_groups_null(StoreDump(lp.stores[r], rows=False), np.arange(G), ("vacated", r))
            assert store_columns_equal(StoreDump(sp_st[r]), perm, before[r], np.arange(G), ("moved rows", r)) > 0
            assert sp_st[r].counters() == dict(copied=0, rebuilt=0, unsatisfied=0, rekeyed=0)
        old = lp.reps + lp.stores
        lp.reps, lp.stores = sp_rep, sp_st
        lp.book = {(int(perm[g]), s, term): v for (g, s, term), v in lp.book.items()}
        for r in range(R):
            lp.check(r, (t, r, "moved"))                         # the rows are present at once
        c0 = [s.counters() for s in lp.stores]
        lp.tick(p_new=0.0)
        for r in range(R):                                       # ... so nothing is refilled by follow / Reconstruct
            c1 = lp.stores[r].counters()
            assert c1["copied"] == c0[r]["copied"] and c1["rebuilt"] == c0[r]["rebuilt"] and c1["unsatisfied"] == 0, (t, r, c0[r], c1)
        _close(old)
    assert int(lp.reps[0].dump()["log_len"].max()) > W and moved > 0
    ex = np.arange(G) % 4 == 1                                   # reconstruct_data commits out of moved rows
    for t in range(3):                                           # (shards {0, 3, 4}: five replicas)
        lp.tick(p_new=1.0 if t < 2 else 0.0, exotic=ex if R == 5 else None)
    assert lp.read_back(lp.leader, lp.reps[lp.leader].dump()["log_len"]) > 0
    for q in range(R):
        lp.read_back(q, lp.reps[q].dump()["log_len"])
    assert lp.checked_cells > 500 and lp.checked_shards > lp.checked_cells
    rsp = RSPaxosPayloadStore(G, R, W, max_data_len=L)
    lst = np.arange(5)
    cs, ps = lp.stores[0].save_groups(lst), rsp.save_groups(lst)
    b0, b1 = StoreDump(rsp), StoreDump(lp.stores[0])
    _refused(lambda: rsp.load_groups(cs, lst), "kind")
    _refused(lambda: lp.stores[0].load_groups(ps, lst), "kind")
    _refused(lambda: rsp.save_groups(lst, cs), "kind")
    store_groups_unchanged(StoreDump(rsp), b0, np.arange(G), "refused"); store_groups_unchanged(StoreDump(lp.stores[0]), b1, np.arange(G), "refused")
    _close([rsp, cs, ps] + lp.reps + lp.stores)


# ---- 10. the cluster form is the single calls ----------------------------------------------------------------------------------------
def cluster_form(dev, oracle, G=130, R=5, ft=1, L=61, n=70):
    """one launch over the R replicas == the R single calls: the same images byte for byte, the same dumps after load and reset"""
    from summerset_amd import RSPaxosReplicaGroup
    from summerset_amd.rspaxos import load_cluster_groups, reset_cluster_groups, save_cluster_groups
    reps, want, _ = finished_cluster(dev, oracle, G, R, ft, L)
    W = reps[0].W
    rng = np.random.default_rng(79)
    n = min(n, G)
    lst, dst = rng.permutation(G)[:n], rng.permutation(G)[:n]
    one = [x.replica.save_groups(lst) for x in reps]
    many = save_cluster_groups([x.replica for x in reps], lst)
    for r in range(R):
        assert one[r].export() == many[r].export(), r
    ta, tb = ([RSPaxosReplicaGroup(G, R, me=r, window=W, fault_tolerance=ft) for r in range(R)] for _ in range(2))
    whole = [x.replica.save_state() for x in reps]
    for r in range(R):
        ta[r].load_state(whole[r]); tb[r].load_state(whole[r])
        ta[r].load_groups(one[r], dst)
    load_cluster_groups(tb, many, dst)
    for r in range(R):
        dumps_equal(ta[r].dump(), tb[r].dump(), ("load", r))
        rep_columns_equal(tb[r].dump(), dst, want[r], lst, ("load", r))
        polls_equal(ta[r].exec_poll(), tb[r].exec_poll(), ("load", r))
        ta[r].reset_groups(lst)
    reset_cluster_groups(tb, lst)
    for r in range(R):
        dumps_equal(ta[r].dump(), tb[r].dump(), ("reset", r))
        polls_equal(ta[r].exec_poll(), tb[r].exec_poll(), ("reset", r))
    _close(one + many + ta + tb + whole)


# ---- 11. refusals --------------------------------------------------------------------------------------------------------------------
def refusals(dev, oracle, G=40, R=3, ft=1, L=61, n=7):
    """every refusal of the header's list: SMR_ERR_ARG / SMR_ERR_STATE with a message, nothing launched, the target unchanged"""
    from summerset_amd import CRaftPayloadStore, PayloadStoreSnapshot, RSPaxosPayloadStore, RSPaxosReplicaGroup, RSPaxosSnapshot
    from summerset_amd.rspaxos import load_cluster_groups, reset_cluster_groups, save_cluster_groups
    reps, want, _ = finished_cluster(dev, oracle, G, R, ft, L)
    W = reps[0].W
    a, st = reps[1].replica, reps[1].store
    lst = np.arange(3, 3 + n)
    good, sgood = a.save_groups(lst), st.save_groups(lst)
    tgt = RSPaxosReplicaGroup(G, R, me=1, window=W, fault_tolerance=ft)
    tgt.load_state(a.save_state())
    tst = RSPaxosPayloadStore(G, R, W, max_data_len=L)
    tst.load(st.save())
    d0, p0, s0 = tgt.dump(), tgt.exec_poll(), StoreDump(tst)

    def unchanged(what):
        dumps_equal(tgt.dump(), d0, what); polls_equal(tgt.exec_poll(), p0, what)
        s1 = StoreDump(tst)
        store_groups_unchanged(s1, s0, np.arange(G), what)
        assert s1.counters == s0.counters, what
    bad_lists = (([], "a list of 0"), (list(range(G + 1)), "a list of"), ([0, G], "is group"), ([0, 2**32 - 1], "is group"), ([4, 5, 4], "listed twice"))
    for bad, word in bad_lists:
        k = len(bad)
        if 0 < k <= G:
            rs, ps = RSPaxosSnapshot(tgt, k), PayloadStoreSnapshot(tst, k)
            rs.import_(a.save_groups(np.arange(k)).export()); ps.import_(st.save_groups(np.arange(k)).export())
        else:
            rs, ps = good, sgood                                 # (no snapshot of 0 or G + 1 groups can be made: below)
        _refused(lambda: tgt.save_groups(bad, rs), word if 0 < k <= G else None); _refused(lambda: tgt.load_groups(rs, bad), word if 0 < k <= G else None)
        _refused(lambda: tgt.reset_groups(bad), word)
        _refused(lambda: tst.save_groups(bad, ps), word if 0 < k <= G else None); _refused(lambda: tst.load_groups(ps, bad), word if 0 < k <= G else None)
        _refused(lambda: tst.reset_groups(bad), word)
        _refused(lambda: reset_cluster_groups([tgt], bad), word)
        unchanged(("list", word))
    for k in (0, G + 1):
        _refused(lambda: RSPaxosSnapshot(tgt, k), "a snapshot of"); _refused(lambda: PayloadStoreSnapshot(tst, k), "a snapshot of")
    other = np.arange(n + 1)                                     # a snapshot made for another n
    _refused(lambda: tgt.save_groups(other, good), "made for"); _refused(lambda: tgt.load_groups(good, other), "made for")
    _refused(lambda: tst.save_groups(other, sgood), "made for"); _refused(lambda: tst.load_groups(sgood, other), "made for")
    whole, swhole = a.save_state(), st.save()                    # ... an image of G groups among them
    _refused(lambda: tgt.load_groups(whole, lst), "made for"); _refused(lambda: tst.load_groups(swhole, lst), "made for")
    unchanged("another n")
    # an image whose n_groups differs from n cannot get into a snapshot of n groups
    _refused(lambda: RSPaxosSnapshot(tgt, n).import_(whole.export()), "the image is of")
    _refused(lambda: PayloadStoreSnapshot(tst, n).import_(swhole.export()), "the image is of")
    # the replica: another population, me, fault_tolerance, window
    for what, kw in (("population", dict(population=R + 2, me=1, window=W, fault_tolerance=ft)), ("me", dict(population=R, me=0, window=W, fault_tolerance=ft)),
                     ("fault_tolerance", dict(population=R, me=1, window=W, fault_tolerance=ft - 1)), ("window", dict(population=R, me=1, window=2 * W, fault_tolerance=ft))):
        o = RSPaxosReplicaGroup(G, **kw)
        o.preset_leader(0)
        b = o.dump()
        word = "window" if what == "window" else "made for another"
        _refused(lambda: o.load_groups(good, lst), word)
        if what != "window":
            _refused(lambda: o.save_groups(lst, good), word)
        _refused(lambda: load_cluster_groups([tgt, o], [good, a.save_groups(lst)], lst))
        dumps_equal(o.dump(), b, what)
        unchanged(what)
        o.close()
    assert good.export() == a.save_groups(lst).export()           # a refused save left the snapshot alone
    # the store: another window, n_shards, n_data_shards, kind; a max_dlen above the target's max_data_len
    others = dict(W=RSPaxosPayloadStore(G, R, 2 * W, L), n=RSPaxosPayloadStore(G, R + 2, W, L, num_data_shards=st.d), d=RSPaxosPayloadStore(G, R, W, L, num_data_shards=st.d - 1),
                  kind=CRaftPayloadStore(G, R, W, L))
    for what, o in others.items():
        b = StoreDump(o)
        _refused(lambda: o.load_groups(sgood, lst), "made for another")
        _refused(lambda: o.save_groups(lst, sgood), "made for another")
        store_groups_unchanged(StoreDump(o), b, np.arange(G), what)
    md = sgood.info()["max_dlen"]
    assert md > 1
    small = RSPaxosPayloadStore(G, R, W, md - 1)
    b = StoreDump(small)
    _refused(lambda: small.load_groups(sgood, lst), "max_data_len")
    store_groups_unchanged(StoreDump(small), b, np.arange(G), "max_dlen")
    assert sgood.export() == st.save_groups(lst).export()
    # nothing saved or imported
    _refused(lambda: tgt.load_groups(RSPaxosSnapshot(tgt, n), lst), "nothing saved", code=-3)
    _refused(lambda: tst.load_groups(PayloadStoreSnapshot(tst, n), lst), "nothing saved", code=-3)
    # the cluster forms: a replica listed twice, replicas that differ
    _refused(lambda: save_cluster_groups([tgt, tgt], lst, [good, RSPaxosSnapshot(tgt, n)]), "listed twice")
    _refused(lambda: reset_cluster_groups([tgt, tgt], lst), "listed twice")
    unchanged("end")
    tgt.load_groups(good, lst); tst.load_groups(sgood, lst)       # ... and the good ones do load
    unchanged("the same groups again")
    _close([good, sgood, tgt, tst, whole, swhole, small] + list(others.values()))


# ---- 12. stream order ----------------------------------------------------------------------------------------------------------------
def stream_order(dev, oracle, G=70, n=5, W=8, L=333, k=40):
    """save, reset and load of listed groups enqueued between puts on one stream, no host synchronisation: the image is the
    state at the save point, the reset slots take the next put as a new store's would, and the load lands behind it"""
    import torch
    from summerset_amd import PayloadStoreSnapshot, RSPaxosPayloadStore, RSPaxosReplicaGroup, RSPaxosSnapshot
    rng = np.random.default_rng(83)
    d = n // 2 + 1
    st, rep = RSPaxosPayloadStore(G, n, W, L), RSPaxosReplicaGroup(G, n, me=0, window=W)
    rep.preset_leader(0)
    datas = [rng.integers(1, 256, (G, L), dtype=np.uint8) for _ in range(5)]
    dv = [torch.from_numpy(x).to(dev) for x in datas]
    vals = [torch.from_numpy((1 + t * G + np.arange(G)).astype(np.int32)).to(dev) for t in range(5)]
    lst, dst = rng.permutation(G)[:k], rng.permutation(G)[:k]
    rs, ps = RSPaxosSnapshot(rep, k), PayloadStoreSnapshot(st, k)
    import contextlib
    side = None if str(dev) == "cpu" else torch.cuda.Stream()    # one non-default stream (the emulator has the null stream alone)
    stream = None if side is None else side.cuda_stream
    if side is not None:
        torch.cuda.synchronize()                                 # everything above is on the device before the first call
    with (torch.cuda.stream(side) if side is not None else contextlib.nullcontext()):   # (the handlers' output tensors are made on it too)
        for t in range(5):
            acc = rep.req_batch(vals[t], stream=stream)
            st.put(acc, dv[t], stream=stream)
            if t == 2:                                           # nothing in front, nothing behind
                rep.save_groups(lst, rs, stream=stream); st.save_groups(lst, ps, stream=stream)
                rep.reset_groups(lst, stream=stream); st.reset_groups(lst, stream=stream)
            if t == 3:
                rep.load_groups(rs, dst, stream=stream); st.load_groups(ps, dst, stream=stream)
    if side is not None:
        side.synchronize()
    h, ctr, arr, shards = StoreLayout(k, W, 2).parse(ps.export(), d)
    want_tok = np.stack([1 + t * G + lst for t in range(3)]).astype(np.uint32)
    assert np.array_equal(arr[("tok", 0)][:3], want_tok) and (arr[("tok", 0)][3:] == NULL).all() and h[11] == 3 * k * n
    for (p, w, x, s), bts in shards.items():
        if x % 5 == 0:
            cw = np.zeros((n, (L + d - 1) // d), np.uint8)
            cw[:d].reshape(-1)[:L] = datas[w][lst[x]]
            cw[d:] = oracle.rs_encode(d, n - d, datas[w][lst[x]])
            assert p == 0 and bytes(cw[s]) == bts, (w, x, s)
    hr, _, sca, _, _, _ = Layout(k, n).parse(rs.export(), W)
    assert (sca["len"] == 3).all()
    # the final state: a group that was reset at t = 2 and not loaded over is a new object's; a group loaded over at t = 3 holds
    # the saved three instances and then tick 4's
    dd, sd = rep.dump(), st.dump(0)
    in_dst = np.zeros(G, bool); in_dst[dst] = True
    in_lst = np.zeros(G, bool); in_lst[lst] = True
    want_len = np.where(in_dst, 4, np.where(in_lst, 0, 5))       # (a reset slot knows no leader: it takes no batch until it is loaded over)
    assert np.array_equal(dd["len"], want_len), "lens"
    src_of = np.arange(G); src_of[dst] = lst
    for g in range(G):
        if in_dst[g]:
            toks = [1 + t * G + src_of[g] for t in range(3)] + [1 + 4 * G + g]
        elif in_lst[g]:
            toks = []
        else:
            toks = [1 + t * G + g for t in range(5)]
        assert sd["tok"][:len(toks), g].tolist() == toks and dd["s_val"][:len(toks), g].tolist() == toks, (g, sd["tok"][:, g], toks)
        assert (sd["tok"][len(toks):, g] == NULL).all()
    _close([st, rep, rs, ps])
