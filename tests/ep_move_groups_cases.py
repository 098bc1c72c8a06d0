"""Chosen groups between EPaxos replica objects (smr_ep_*_groups, smr_ep_cluster_*_groups): the bodies of
tests/test_ep_move_groups.py (emulator, dev = "cpu") and tests/test_zzzz_ep_move_groups_gpu.py (device), every size an argument.

Every comparison is bit-exact, against the CPU oracle or against images computed in numpy from a whole-object image
(`select_image`: ep_snapshot_cases.read_image of the whole image, restricted and reordered to the list, written again by
ep_snapshot_cases.write_image -- both written from DESIGN.md 2's table alone).  The oracle cannot move anything: it keeps running
ALL groups of the job.  A `Shard` is R replica objects of n slots and the host's table slot -> job group; a `JobRep` is replica r
of the whole job behind ep_cluster's numpy interface: every handler call is gathered by the tables, run on replica r of every
shard and scattered back, so the job's outputs, dumps and submissions are compared with the oracle's as those of one cluster."""
import ctypes as C
import inspect

import numpy as np

import ep_cluster as ec
import ep_snapshot_cases as c
from ep_snapshot_cases import LazyEngine, coverage, image_vs_dumps, mk_oracle, mk_reps, read_image, same, schedule, write_image

N, NO_KEY = c.N, c.NO_KEY
SYMBOLS = ("smr_ep_snapshot_create_groups", "smr_ep_save_groups", "smr_ep_load_groups", "smr_ep_reset_groups",
           "smr_ep_cluster_save_groups", "smr_ep_cluster_load_groups", "smr_ep_cluster_reset_groups")
CELL_FIELDS = ("bal", "seq", "status", "key", "bk", "pa_acks", "acc_acks", "avoid", "xp_acks", "xp_has", "xp_max")


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
    from summerset_amd import _lib, epaxos
    names = {n for n, _, _ in _lib.SYMBOLS}
    for n in SYMBOLS:
        assert n in names and getattr(lib, n), n
    assert hasattr(summerset_amd, "move_ep_groups") and summerset_amd.move_ep_groups is epaxos.move_groups
    assert len({summerset_amd.move_groups, summerset_amd.move_raft_groups, summerset_amd.move_rsp_groups, summerset_amd.move_ep_groups}) == 4
    for n in ("save_cluster_groups", "load_cluster_groups", "reset_cluster_groups", "move_groups"):
        assert hasattr(epaxos, n), n
    for n in ("save_groups", "load_groups", "reset_groups"):
        assert hasattr(epaxos.EPaxosReplicaGroup, n), n


# ---- columns and images ----------------------------------------------------------------------------------------------------------
def take(name, x, idx):
    """the groups idx of a dump array (the group is the last axis of every array but `deps`)"""
    x = np.asarray(x)
    return x[:, :, idx] if name == "deps" and x.ndim == 4 else x[..., idx]


def cols_equal(a, ia, b, ib, what):
    """dump a's groups ia == dump b's groups ib, every per-group field (the counters are the object's, not a group's)"""
    if b is None:
        return
    ia, ib = np.asarray(ia), np.asarray(ib)
    for n, v in b.items():
        if n == "counters":
            continue
        x, y = take(n, a[n], ia), take(n, v, ib)
        assert np.array_equal(x, y), "%s: %s differs" % (what, n)


def all_cols_equal(e, ia, dumps, ib, what, recovery=False):
    """replica object e's dump / exec_dump / xp_dump columns ia against a (dump, exec_dump, xp_dump) triple's columns ib"""
    cols_equal(e.dump(), ia, dumps[0], ib, what)
    cols_equal(e.exec_dump(), ia, dumps[1], ib, what + " (exec)")
    if recovery:
        cols_equal(e.xp_dump(), ia, dumps[2], ib, what + " (xp)")


def dumps_of(e, recovery=False):
    return e.dump(), e.exec_dump(), (e.xp_dump() if recovery else None)


def subs_of(poll, groups):
    """(group, row, col) submissions restricted to `groups`, as {list position: [(row, col), ...]}"""
    pos = {int(g): i for i, g in enumerate(np.asarray(groups).tolist())}
    out = {}
    for g, r, col in zip(*[x.tolist() for x in poll]):
        if g in pos:
            out.setdefault(pos[g], []).append((r, col))
    return out


def select_image(whole, lst):
    """the image of the groups `lst` (in that order) computed in numpy from the bytes of a whole-object image: the same header
    fields but n_groups, max_live, max_exec and the totals; zero counters"""
    im = read_image(whole)
    h = im["hdr"]
    lst = np.asarray(lst, np.int64)
    n, R, K, W = len(lst), int(h["population"]), int(h["n_keys"]), int(h["window"])
    ex, rec = int(h["execute"]), int(h["recovery"])
    cfg = dict(G=n, R=R, me=int(h["me"]), oq=int(h["optimized_quorum"]), execute=ex, recovery=rec, W=W, K=K)
    st = {}
    for name, dt, shape in c._scalars(int(h["n_groups"]), R, K, ex):
        if "counters" not in name:
            st[name] = im[name][..., lst]
    for f in CELL_FIELDS:
        st[f] = im[f][..., lst]
    st["deps"] = im["deps"][:, :, lst]
    pos = {int(g): i for i, g in enumerate(lst.tolist())}
    gi, ri, ci = im["reply_at"]
    st["replies"] = {}
    for i, (g, r, col) in enumerate(zip(gi.tolist(), ri.tolist(), ci.tolist())):
        if g in pos:
            st["replies"][(r, col, pos[g])] = {f: im["replies"][f][i] for f in im["replies"].dtype.names if f != "pad"}
    if ex:
        st["exec"] = [(pos[g], r, col) for g, r, col in zip(*[x.tolist() for x in im["exec"]]) if g in pos]
    return write_image(cfg, st)


def save_lists(reps, lst, cluster, snaps=None):
    from summerset_amd import epaxos
    if cluster:
        return epaxos.save_cluster_groups(reps, lst, snaps)
    return [e.save_groups(lst, None if snaps is None else snaps[r]) for r, e in enumerate(reps)]


def load_lists(reps, snaps, lst, cluster):
    from summerset_amd import epaxos
    if cluster:
        epaxos.load_cluster_groups(reps, snaps, lst)
    else:
        for e, s in zip(reps, snaps):
            e.load_groups(s, lst)


def reset_lists(reps, lst, cluster):
    from summerset_amd import epaxos
    if cluster:
        epaxos.reset_cluster_groups(reps, lst)
    else:
        for e in reps:
            e.reset_groups(lst)


# ---- a finished cluster, made once and only read ---------------------------------------------------------------------------------
_FINISHED = {}


def finished_cluster(dev, oracle, G, R, W=8, K=3, T=None, seed=11):
    """ep_snapshot_cases' schedule (loss 0.2, one tick cut short for the last replica) handler by handler, every tick's
    outputs against the oracle cluster's; the unpolled submissions of the last call stay in place (only the first ticks end on
    a handler that executes: T = 1 leaves some, the full run none).  Shared by the bodies that only read it.  -> (replica objects, the oracles' (dump, exec_dump, None) per replica)"""
    key = (str(dev), G, R, W, K, T, seed)
    if key not in _FINISHED:
        T_ = 2 * W + 4 if T is None else T
        orc = mk_oracle(oracle, G, R, W, K)
        reps = mk_reps(G, R, W, K)
        eng = [LazyEngine(e, dev, []) for e in reps]
        rng = np.random.default_rng(seed)
        for t in range(T_):
            keys, drop = schedule(rng, t, R, G, K)
            if t == W + 3:
                k1 = np.ascontiguousarray(keys[R - 1])
                assert np.array_equal(ec.crash_tick(eng, R - 1, k1, np.random.default_rng(seed + t), G),
                                      ec.crash_tick(orc, R - 1, k1, np.random.default_rng(seed + t), G))
                continue
            oe, oo = ec.tick(eng, keys, drop), ec.tick(orc, keys, drop)
            for s in range(R):
                same(oo[s], oe[s], "tick %d, leader %d" % (t, s))
        want = [(o.dump(), o.exec_dump(), None) for o in orc]
        for r in range(R):
            same(want[r][0], reps[r].dump(), "finished cluster, replica %d" % r)
            same(want[r][1], reps[r].exec_dump(), "finished cluster, replica %d" % r)
        _FINISHED[key] = (reps, want)
    return _FINISHED[key]


# ---- 2. a group image is a selection of the whole image, byte for byte -----------------------------------------------------------
def selection_of_the_whole_image(dev, oracle, cluster, G=130, R=5, W=8, K=3, sizes=(1, 63, 64, 65, 130), seed=11):
    """a cluster runs T = 2 W + 4 ticks against the oracle (one tick cut short for the last replica: Accepting cells); at two
    boundaries in between (behind ticks 1 and W + 3) and at the end the whole image of every replica is the oracle's dumps, and for seeded unsorted lists of
    every size export(save_groups(list)) is the numpy selection of that whole image.  What the compared group images held is
    asserted"""
    T = 2 * W + 4
    orc = mk_oracle(oracle, G, R, W, K)
    reps = mk_reps(G, R, W, K)
    eng = [LazyEngine(e, dev, []) for e in reps]
    rng, lrng = np.random.default_rng(seed), np.random.default_rng(seed + 1)
    cov = dict(preaccepting_short=False, accepting=False, committed=False, executed=False, wrapped=False, pending=False, has_entry=False, images=0)
    for t in range(T):
        keys, drop = schedule(rng, t, R, G, K)
        if t == W + 3:
            k1 = np.ascontiguousarray(keys[R - 1])
            assert np.array_equal(ec.crash_tick(eng, R - 1, k1, np.random.default_rng(seed + t), G),
                                  ec.crash_tick(orc, R - 1, k1, np.random.default_rng(seed + t), G))
        else:
            oe, oo = ec.tick(eng, keys, drop), ec.tick(orc, keys, drop)
            for s in range(R):
                same(oo[s], oe[s], "tick %d, leader %d" % (t, s))
        if t not in (1, W + 3, T - 1):                           # (only the first ticks end on a handler that executes: a non-empty exec
            continue                                             #  section; W + 3: Accepting cells; the end: every row wrapped)
        whole = [e.save_state().export() for e in reps]
        for r in range(R):
            image_vs_dumps(read_image(whole[r]), orc[r].dump(), orc[r].exec_dump(), None, "tick %d, replica %d" % (t, r))
        for n in sizes:
            n = min(n, G)
            lst = lrng.permutation(G)[:n]
            snaps = save_lists(reps, lst, cluster)
            for r in range(R):
                img = snaps[r].export()
                assert img == select_image(whole[r], lst), "tick %d, replica %d, a list of %d" % (t, r, n)
                info = snaps[r].info()
                assert info["n_groups"] == n and info["me"] == r and info["window"] == W and info["bytes"] == len(img), info
                coverage(cov, read_image(img), R)
                cov["images"] += 1
            _close(snaps)
    for k in ("wrapped", "preaccepting_short", "accepting", "committed", "executed", "pending"):
        assert cov[k], "no compared group image held: %s" % k
    _close(reps)
    return cov


# ---- 3. a move changes object and position, and the run goes on ------------------------------------------------------------------
class _MapPolls(list):
    """the polls of replica r of one shard, appended under the job's group ids of that moment"""

    def __init__(self, shard, sink):
        super().__init__()
        self.shard, self.sink = shard, sink

    def append(self, poll):
        g, r, col = poll
        assert (self.shard.tab[g] >= 0).all(), "a submission out of an empty slot"
        mapped = (self.shard.tab[g].astype(np.uint32), r, col)
        super().append(mapped)
        self.sink.append(mapped)


class Shard:
    """R replica objects of n slots and the host's table of which job group sits in which slot"""

    def __init__(self, dev, n, R, W, K, recovery, sinks, seated=None):
        from summerset_amd.ep_cluster import EPaxosCluster
        self.n, self.R = n, R
        self.reps = mk_reps(n, R, W, K, True, recovery)
        self.tab = np.full(n, -1, np.int64)
        self.eng = [LazyEngine(e, dev, _MapPolls(self, sinks[r])) for r, e in enumerate(self.reps)]
        probe = mk_reps(n, R, W, K, True, recovery)
        self.fresh = [dumps_of(e, recovery) for e in probe]      # a newly created object's columns
        _close(probe)
        self.cluster = None if seated is None else EPaxosCluster(self.reps, phase_major=seated)

    def close(self):
        if self.cluster is not None:
            self.cluster.close()                                 # (before its replicas)
        _close(self.reps)


_QUIET = dict(flags=0, key=NO_KEY, src=NO_KEY)                   # what an empty slot is fed: no message, no proposal, no timeout


class JobRep:
    """replica r of the whole job behind ep_cluster.NumpyEngine's interface"""

    def __init__(self, job, r):
        self.job, self.r, self.W, self.n_keys = job, r, job.W, job.K

    def __getattr__(self, name):
        fn = getattr(ec.NumpyEngine, name, None)
        if fn is None or name.startswith("_"):
            raise AttributeError(name)
        sig = inspect.signature(fn)

        def call(*a, **kw):
            args = dict(sig.bind(None, *a, **kw).arguments)
            args.pop("self")
            out = None
            for sh in self.job.shards:
                occ = sh.tab >= 0
                j = np.where(occ, sh.tab, 0)
                sub = {}
                for k, v in args.items():
                    if v is None:
                        continue
                    x = np.asarray(v)[..., j]
                    if k in _QUIET:
                        x = np.where(occ, x, np.asarray(_QUIET[k]).astype(x.dtype))
                    sub[k] = np.ascontiguousarray(x.astype(np.asarray(v).dtype))
                o = getattr(sh.eng[self.r], name)(**sub)
                if o is not None:
                    out = out if out is not None else {k: np.zeros(x.shape[:-1] + (self.job.J,), x.dtype) for k, x in o.items()}
                    for k, x in o.items():
                        out[k][..., sh.tab[occ]] = x[..., occ]
            return out
        return call

    def _merged(self, which):
        out = None
        for sh in self.job.shards:
            d = getattr(sh.reps[self.r], which)()
            occ = sh.tab >= 0
            out = out if out is not None else {k: (np.zeros_like(x) if k == "counters" else np.zeros(x.shape[:2] + (self.job.J, x.shape[3]) if k == "deps" else x.shape[:-1] + (self.job.J,), x.dtype))
                                               for k, x in d.items()}
            for k, x in d.items():
                if k == "counters":
                    out[k] += x                                  # events stay counted where they happened: the sum is the job's
                elif k == "deps":
                    out[k][:, :, sh.tab[occ]] = x[:, :, occ]
                else:
                    out[k][..., sh.tab[occ]] = x[..., occ]
        return out

    def dump(self):
        return self._merged("dump")

    def exec_dump(self):
        return self._merged("exec_dump")

    def xp_dump(self):
        return self._merged("xp_dump")

    def take_submissions(self):
        for sh in self.job.shards:
            sh.eng[self.r].flush()
        got = c._sorted_subs(self.job.sinks[self.r])
        del self.job.sinks[self.r][:]
        return got


class Job:
    def __init__(self, dev, J, sizes, R, W, K, recovery, seed, seated, cluster):
        assert sum(sizes) == J
        self.dev, self.J, self.R, self.W, self.K, self.recovery, self.cluster, self.seated = dev, J, R, W, K, recovery, cluster, seated
        self.sinks = [[] for _ in range(R)]
        self.shards = [Shard(dev, n, R, W, K, recovery, self.sinks, seated=(None if not seated else bool(i))) for i, n in enumerate(sizes)]
        self.rng = np.random.default_rng(seed)
        perm = self.rng.permutation(J)
        self.shards[0].tab[:] = perm[:sizes[0]]
        self.shards[1].tab[:] = perm[sizes[0]:]
        self.reps = [JobRep(self, r) for r in range(R)]
        self.cov = dict(moves=0, moved=0, exec_moved=0, crosses_tile=0, not_reset=0, live_moved=0)

    def tick_seated(self, keys, drop):
        """one smr_ep_cluster_tick per shard; -> per shard the leaders' outputs and the slots' job groups"""
        import torch
        t_ = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(self.dev)
        outs = []
        for sh in self.shards:
            for e in sh.eng:
                e.flush()
            out = sh.cluster.tick([t_(keys[r][sh.tab]) for r in range(self.R)], {k: t_(v[sh.tab]) for k, v in drop.items()} if drop else None)
            for e in sh.eng:
                e.e.pending = True
            outs.append([{k: v.cpu().numpy().view(np.uint32 if v.dtype == torch.int32 else np.uint64 if v.dtype == torch.int64 else np.uint8)
                          for k, v in o.items()} for o in out])
        return outs

    def exchange(self, k, reset_b=True, live=None):
        """k seeded groups of shard A and k of shard B change places: saved, the vacated slots reset (B's only with reset_b: a
        load also takes a slot as the last tenant left it), each image loaded into the other shard's vacated slots in another
        order.  The moved columns are the source's, the vacated slots a new object's, the neighbours and the counters untouched,
        and the destination hands over the unpolled submissions the source held, under its own group ids"""
        A, B = self.shards
        rng, R, rec = self.rng, self.R, self.recovery
        live = list(range(R)) if live is None else live
        sa, sb = rng.permutation(A.n)[:k], rng.permutation(B.n)[:k]
        da, db = rng.permutation(sa), rng.permutation(sb)        # where B's groups land in A, A's in B
        ra, rb = [A.reps[r] for r in live], [B.reps[r] for r in live]
        before = {id(sh): [dumps_of(e, rec) for e in sh.reps] for sh in (A, B)}
        pend = {id(sh): [read_image(e.save_state().export())["exec"] for e in sh.reps] for sh in (A, B)}
        snaps_a, snaps_b = save_lists(ra, sa, self.cluster), save_lists(rb, sb, self.cluster)
        reset_lists(ra, sa, self.cluster)
        if reset_b:
            reset_lists(rb, sb, self.cluster)
        for i, r in enumerate(live):
            all_cols_equal(A.reps[r], sa, A.fresh[r], sa, "vacated slots of A, replica %d" % r, rec)
            if reset_b:
                all_cols_equal(B.reps[r], sb, B.fresh[r], sb, "vacated slots of B, replica %d" % r, rec)
        load_lists(rb, snaps_a, db, self.cluster)
        load_lists(ra, snaps_b, da, self.cluster)
        stay_a, stay_b = np.setdiff1d(np.arange(A.n), sa), np.setdiff1d(np.arange(B.n), sb)
        tab_a, tab_b = A.tab.copy(), B.tab.copy()
        A.tab[da], B.tab[db] = tab_b[sb], tab_a[sa]
        for i, r in enumerate(live):
            ba, bb = before[id(A)][r], before[id(B)][r]
            all_cols_equal(B.reps[r], db, ba, sa, "A's groups in B, replica %d" % r, rec)
            all_cols_equal(A.reps[r], da, bb, sb, "B's groups in A, replica %d" % r, rec)
            all_cols_equal(A.reps[r], stay_a, ba, stay_a, "beside the move in A, replica %d" % r, rec)
            all_cols_equal(B.reps[r], stay_b, bb, stay_b, "beside the move in B, replica %d" % r, rec)
            for sh, b in ((A, ba), (B, bb)):
                now = dumps_of(sh.reps[r], rec)
                for x, y in zip(now, b):
                    assert x is None or np.array_equal(x["counters"], y["counters"]), (r, "the counters stay where the events happened")
            # the unpolled submissions travel with their group: what the two objects hand over now, under the job's ids, is what
            # the two whole images held before the move
            want = c._sorted_subs([(tab_a[pend[id(A)][r][0]].astype(np.uint32),) + tuple(pend[id(A)][r][1:]),
                                   (tab_b[pend[id(B)][r][0]].astype(np.uint32),) + tuple(pend[id(B)][r][1:])])
            n0 = len(self.sinks[r])
            for sh in (A, B):
                assert sh.eng[r].e.pending, "a tick left its list in place"
                sh.eng[r].flush()
            got = c._sorted_subs(self.sinks[r][n0:])
            moved_ids = set(tab_a[sa].tolist()) | set(tab_b[sb].tolist())
            if self.seated:                                      # (the image names row 0 where a list entry of the phase-major tick names a
                keep = np.zeros(self.J, bool)                    #  row >= R: there only the moved groups' entries are the image's)
                keep[list(moved_ids)] = True
                got, want = tuple(x[keep[got[0]]] for x in got), tuple(x[keep[want[0]]] for x in want)
            assert len(got[0]) == len(want[0]), (r, "the unpolled submissions after a move")
            for x, y in zip(got, want):
                assert np.array_equal(x, y), (r, "the unpolled submissions after a move")
            self.cov["exec_moved"] += sum(1 for g in want[0].tolist() if g in moved_ids)
            self.cov["live_moved"] += int((ba[0]["status"][..., sa] != 0).sum())
        _close(list(snaps_a) + list(snaps_b))
        self.cov["moves"] += 1; self.cov["moved"] += 2 * k; self.cov["not_reset"] += int(not reset_b)
        self.cov["crosses_tile"] += int((sa < 64).any() and (sa >= 64).any())

    def close(self):
        for sh in self.shards:
            sh.close()


def move_between_shards(dev, oracle, R=3, K=3, W=8, sizes=(70, 40), seated=False, recovery=False, cluster=True, every=3, seed=19):
    """Shards A (70 slots) and B (40) as ONE job of 110 groups beside one oracle cluster of 110 groups; every `every` ticks a
    seeded list of A's groups and one of B's change places (other indices; the vacated slots reset, or -- every other move,
    in B -- left as the last tenant left them), ticks continue.  After every tick and every move the job's dump / exec_dump /
    xp_dump are the oracle's for the group that now sits in each slot, and without the seated clusters the submissions of the
    whole run are the oracle's.  seated: each shard sits in an smr_ep_cluster (its shared per-key table) and is ticked by
    smr_ep_cluster_tick, A in mode 0 and B phase-major; the oracle takes A's groups leader by leader and B's phase by phase.
    recovery: the last tick is cut short for the last replica and, after one more move, replica 0 recovers its row"""
    J, T = sum(sizes), 2 * W + 4
    orc = mk_oracle(oracle, J, R, W, K)
    job = Job(dev, J, sizes, R, W, K, recovery, seed=seed + 1, seated=seated, cluster=cluster)
    rng = np.random.default_rng(seed)
    orc_subs = [[] for _ in range(R)]
    live = list(range(R))

    def compare(what, members):
        for r in members:
            same(orc[r].dump(), job.reps[r].dump(), "%s: dump of replica %d" % (what, r))
            same(orc[r].exec_dump(), job.reps[r].exec_dump(), "%s: exec_dump of replica %d" % (what, r))
            if recovery:
                same(orc[r].xp_dump(), job.reps[r].xp_dump(), "%s: xp_dump of replica %d" % (what, r))
    try:
        for t in range(T):
            keys, drop = schedule(rng, t, R, J, K)
            if recovery and t == T - 1:                          # the last replica's tick is cut short
                k1 = np.ascontiguousarray(keys[R - 1])
                assert np.array_equal(ec.crash_tick(job.reps, R - 1, k1, np.random.default_rng(seed + t), J),
                                      ec.crash_tick(orc, R - 1, k1, np.random.default_rng(seed + t), J))
            elif seated:
                outs = job.tick_seated(keys, drop)
                for i, sh in enumerate(job.shards):
                    mine = np.zeros(J, bool); mine[sh.tab] = True
                    oo = ec.tick(orc, np.where(mine[None, :], keys, NO_KEY).astype(np.uint8), drop, phase_major=bool(i))
                    for s in range(R):
                        same({k: v[..., sh.tab] for k, v in oo[s].items()}, outs[i][s], "tick %d, shard %d, leader %d" % (t, i, s))
            else:
                oe, oo = ec.tick(job.reps, keys, drop), ec.tick(orc, keys, drop)
                for s in range(R):
                    same(oo[s], oe[s], "tick %d, leader %d" % (t, s))
            for r in range(R):
                orc_subs[r].append(orc[r].take_submissions())
            compare("tick %d" % t, live)
            if t == 0 or t % every == every - 1 or t == T - 1:   # (tick 0 ends on a handler that executes: submissions move)
                job.exchange(k=30 if t == 0 else int(job.rng.integers(5, 24)) if t % 2 else 17, reset_b=(job.cov["moves"] % 2 == 0))
                compare("after the move behind tick %d" % t, live)
        if recovery:
            dead, live = R - 1, list(range(R - 1))
            te, to = [], []
            ec.recover_row(job.reps, 0, dead, live, J, rng=np.random.default_rng(seed + 7), loss=0.2, trace=te)
            ec.recover_row(orc, 0, dead, live, J, rng=np.random.default_rng(seed + 7), loss=0.2, trace=to)
            assert len(te) == len(to) and len(te) > 0
            for a, b in zip(te, to):
                assert a[0] == b[0]
                for x, y in zip(a[1:], b[1:]):
                    assert np.array_equal(x, y), "the recovery's trace differs at %s" % (a[0],)
            for r in live:
                orc_subs[r].append(orc[r].take_submissions())
            compare("after the recovery", live)
        if not seated:                                           # (smr_ep_cluster_tick leaves the list of the tick's LAST handler: there
            for r in live:                                       #  the digest of exec_dump stands for the whole order)
                c._subs_equal(c._sorted_subs(orc_subs[r]), job.reps[r].take_submissions(), "the submissions of replica %d" % r)
        cv = job.cov
        assert cv["moves"] >= 5 and cv["crosses_tile"] > 0 and cv["not_reset"] > 0 and cv["exec_moved"] > 0 and cv["live_moved"] > 0, cv
        assert max(int(o.dump()["len"].max()) for o in orc) > W, "wrapped rows"
    finally:
        job.close()
    return job.cov


# ---- 4. interchange ----------------------------------------------------------------------------------------------------------------
def interchange(dev, oracle, G=130, R=5, W=8, K=3, n=65):
    """a save_groups image of n groups, imported into a whole-object snapshot of an n-group replica and loaded with load_state,
    gives the listed groups' columns, and that replica's save_state is the same bytes; its whole image loads through a list into
    n positions of a G-group replica, submissions included"""
    from summerset_amd import EPaxosSnapshot
    rng = np.random.default_rng(31)
    n = min(n, G)
    for r, name, T in ((1, "random", None), (0, "descending", None), (1, "random, after one tick", 1)):
        reps, want = finished_cluster(dev, oracle, G, R, W, K, T=T)
        lst = rng.permutation(G)[:n] if name == "random" else np.sort(rng.permutation(G)[:n])[::-1].copy()
        snap = reps[r].save_groups(lst)
        img = snap.export()
        assert img == select_image(reps[r].save_state().export(), lst), name
        im = read_image(img)
        assert not im["counters"].any() and not im["exec_counters"].any(), "a group image holds zero counters"
        small = mk_reps(n, R, W, K, only=[r])[0]
        ws = EPaxosSnapshot(small).import_(img)                  # a group image IS an n-group replica's image
        small.load_state(ws)
        all_cols_equal(small, np.arange(n), want[r], lst, name)
        again = small.save_state()
        assert again.export() == img, (name, "the two kinds of image differ")
        other = mk_reps(G, R, W, K, only=[r])[0]
        lst2 = rng.permutation(G)[:n]
        other.load_groups(again, lst2)                           # ... and an n-group replica's whole image loads through a list
        all_cols_equal(other, lst2, want[r], lst, name + ", back through a list")
        rest = np.setdiff1d(np.arange(G), lst2)
        fresh = mk_reps(G, R, W, K, only=[r])[0]
        all_cols_equal(other, rest, dumps_of(fresh), rest, name + ", beside the list")
        assert not other.dump()["counters"].any() and not other.exec_dump()["counters"].any()
        assert subs_of(other.exec_poll(), lst2) == subs_of(im["exec"], np.arange(n)), (name, "submissions")
        assert T is None or len(im["exec"][0]) > 0, "unpolled submissions in the image"
        _close([snap, small, ws, again, other, fresh])


# ---- 5. stored replies survive a move ------------------------------------------------------------------------------------------------
def stored_replies_survive(dev, oracle, G=65, R=5, W=8, K=3, seed=5):
    """ep_snapshot_cases.stored_replies_survive's scenario; all groups then move into other positions of new replica objects
    through save_groups / load_groups, and the ballot-0 re-evaluation of smr_ep_heartbeat_timeout reads pa_seq / pa_deps of
    moved groups: its outputs and the dumps are the oracle's under the position map"""
    orc = mk_oracle(oracle, G, R, W, K, execute=False)
    a = mk_reps(G, R, W, K, execute=False, recovery=True)
    ea = [ec.NumpyEngine(e, dev) for e in a]
    rng = np.random.default_rng(seed)
    lostq = [R - 1, R - 2]
    mask = lambda s: np.array([[q in lostq and q != s] * G for q in range(R)])   # noqa: E731
    for t in range(3):
        keys = ec.same_key(rng, R, G, K) if t else ec.zipf_keys(rng, R, G, K)
        oe, oo = ec.tick(ea, keys, via=ec.lost_replies(mask)), ec.tick(orc, keys, via=ec.lost_replies(mask))
        for s in range(R):
            same(oo[s], oe[s], "tick %d, leader %d" % (t, s))
    b = mk_reps(G, R, W, K, execute=False, recovery=True)
    eb = [ec.NumpyEngine(e, dev) for e in b]
    src, dst = rng.permutation(G), rng.permutation(G)            # group src[i] of a becomes group dst[i] of b
    stored = 0
    for r in range(R):
        snap = a[r].save_groups(src)
        stored += int((read_image(snap.export())["replies"]["pa_seq"] != 0).sum())
        b[r].load_groups(snap, dst)
        snap.close()
    assert stored > 0
    u = np.full(G, lostq[0], np.uint8)
    ex = np.full(G, (1 << lostq[0]) | (1 << lostq[1]), np.uint8)
    moved = 0
    for r in range(R - 2):
        he, ho = eb[r].heartbeat_timeout(u, ex), orc[r].heartbeat_timeout(u, ex)
        cols_equal(he, dst, ho, src, "heartbeat_timeout at replica %d" % r)
        cols_equal(eb[r].dump(), dst, orc[r].dump(), src, "dump of replica %d" % r)
        cols_equal(eb[r].xp_dump(), dst, orc[r].xp_dump(), src, "xp_dump of replica %d" % r)
        moved += int(eb[r].dump()["counters"][1])
    assert moved > 0                                             # the re-evaluation took the slow path on the stored replies
    _close(a + b)
    return moved


# ---- 6. neighbours untouched, reset is create ----------------------------------------------------------------------------------------
class RawArena:
    """the bytes of a replica object's device allocation (`smr_ep_debug_arena_view`), read and painted as bytes.  Nothing here
    knows the layout inside: which bytes belong to which group is LEARNED, by painting a new object and resetting or loading
    those groups"""

    def __init__(self, rep, dev):
        from summerset_amd import _lib
        base, n = C.c_void_p(), C.c_uint64()
        _lib.check(_lib.load().smr_ep_debug_arena_view(rep._h, C.byref(base), C.byref(n)))
        self.base, self.n, self.dev = base.value, int(n.value), dev
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
            C.memmove(out.ctypes.data, self.base, self.n)
        else:
            assert self.hip.hipMemcpy(out.ctypes.data, self.base, self.n, 2) == 0     # hipMemcpyDeviceToHost
        return out

    def paint(self, byte):
        self._sync()
        if self.hip is None:
            C.memset(self.base, byte, self.n)
        else:
            assert self.hip.hipMemset(self.base, byte, self.n) == 0
        self._sync()


def reset_bytes_per_group(R, W, K, execute, recovery):
    """what smr_ep_reset_groups writes for one group.  Every ring cell: p0, p1, p2 (16 bytes each; p3 too at
    populations 7 and 8), sq32 (4) and with recovery exp_prepare_max_bal (8); len and commit_bars (4 R each), my_nulls (4),
    rewritten (1); of every key's entry the R highest columns and the KV word (4 each); with execution exec_bars and the
    commit-bar copies (4 R each), digest (8) and n_sub (4)"""
    cell = 48 + (16 if R > 6 else 0) + 4 + (8 if recovery else 0)
    return R * W * cell + 8 * R + 4 + 1 + K * (R + 1) * 4 + ((8 * R + 8 + 4) if execute else 0)


def full_image(n, R, me, W, K):
    """an image of n groups in which everything a load can write is there: every ring cell live (rows of W + 1 instances), my
    row's cells PreAccepting with every reply stored, full submission lists"""
    cfg = dict(G=n, R=R, me=me, oq=1, execute=1, recovery=0, W=W, K=K)
    length = np.full((R, n), W + 1, np.uint32)
    st = dict(len=length, commit_bars=np.ones((R, n), np.uint32), rewritten=np.ones(n, np.uint8), exec_bars=np.ones((R, n), np.uint32),
              prev_cb=np.ones((R, n), np.uint32), digest=np.full(n, 3, np.uint64), highest_cols=np.full((K, R, n), 2, np.uint32),
              kv=np.full((K, n), (1 << 32) | 5, np.uint64))
    st["status"] = np.full((R, W, n), 3, np.uint8); st["status"][me] = 1
    st["bk"] = np.zeros((R, W, n), np.uint8); st["bk"][me] = 1
    st["pa_acks"] = np.zeros((R, W, n), np.uint8); st["pa_acks"][me] = (1 << R) - 1
    st["acc_acks"] = np.zeros((R, W, n), np.uint8)
    st["key"] = np.ones((R, W, n), np.uint8)
    st["bal"] = np.full((R, W, n), 2, np.uint64); st["seq"] = np.full((R, W, n), 7, np.uint64)
    st["deps"] = np.ones((R, W, n, R), np.uint32)
    st["replies"] = {(me, col, g): dict(pa_seq=(4,) * R, pa_deps=((1,) * R,) * R) for g in range(n) for col in range(1, W + 2)}
    st["n_sub"] = np.full(n, 2 * R * W, np.uint32)
    st["exec"] = [(g, j % R, 1 + (j // R) % W) for g in range(n) for j in range(2 * R * W)]
    return write_image(cfg, st)


def neighbours_untouched(dev, oracle, G=130, R=5, W=8, K=3, k=37, young=3):
    """What a load or reset does to the bytes no dump shows is looked at in the object's raw bytes.  PAINT = 0xA5 is no value
    the calls write.  (1) A new object painted all over and reset through a list: the bytes that changed are the RESET
    footprint of those groups -- for all G groups exactly G x reset_bytes_per_group, for k groups k x that, inside the full
    one.  A load also writes the reply tables and the submission list's rows, which a reset need not: the LOAD footprint of a
    list is learned the same way, by loading `full_image` into a painted object, and contains the reset footprint.  (2) Groups
    `young` < W instances long loaded into a painted object: inside the load footprint, and at least W - young cells of every row
    stay painted; scalars and rows are the source's.  (3) A painted object takes the finished replica whole; a load_groups then
    writes inside its list's load footprint only; a reset_groups inside its reset footprint only and leaves there, byte for
    byte, what a newly created object holds; bytes outside every footprint (the counter shards among them) never change; the
    unlisted groups' columns and submissions and the counters are what they were"""
    from summerset_amd import EPaxosSnapshot
    PAINT = 0xA5
    reps, want = finished_cluster(dev, oracle, G, R, W, K)
    r = 1
    mk = lambda: mk_reps(G, R, W, K, only=[r])[0]               # noqa: E731

    def reset_footprint(lst):
        p = mk()
        raw = RawArena(p, dev)
        raw.paint(PAINT)
        p.reset_groups(lst)
        f = raw.read() != PAINT
        p.close()
        return f

    def load_footprint(lst):
        p = mk()
        s = EPaxosSnapshot(p, len(lst)).import_(full_image(len(lst), R, r, W, K))
        raw = RawArena(p, dev)
        raw.paint(PAINT)
        p.load_groups(s, lst)
        f = raw.read() != PAINT
        _close([p, s])
        return f
    per_group = reset_bytes_per_group(R, W, K, True, False)
    f_all = reset_footprint(np.arange(G))
    assert int(f_all.sum()) == G * per_group, (int(f_all.sum()), G * per_group)
    rng = np.random.default_rng(89)
    la, lb, lc, ly = (rng.permutation(G)[:k] for _ in range(4))
    fc, fy = reset_footprint(lc), reset_footprint(ly)
    for f in (fc, fy):
        assert int(f.sum()) == k * per_group and not (f & ~f_all).any()
    l_all, fa_load, fy_load = load_footprint(np.arange(G)), load_footprint(la), load_footprint(ly)
    assert not (f_all & ~l_all).any() and not (fy & ~fy_load).any() and not (fa_load & ~l_all).any()
    assert int(fa_load.sum()) * G == int(l_all.sum()) * k
    # (2) young groups
    src = mk_reps(G, R, W, K)
    es = [ec.NumpyEngine(e, dev) for e in src]
    srng = np.random.default_rng(5)
    for t in range(young):
        ec.tick(es, *schedule(srng, t, R, G, K))
    sd = dumps_of(src[r])
    assert 0 < int(sd[0]["len"].max()) <= young < W
    ys = src[r].save_groups(ly)
    y = mk()
    rawy = RawArena(y, dev)
    rawy.paint(PAINT)
    y.load_groups(ys, ly)
    r1 = rawy.read()
    ch = r1 != PAINT
    assert ch.any() and not (ch & ~fy_load).any(), "a load through a list wrote outside its groups"
    cell = 48 + 4
    assert int(((r1 == PAINT) & fy).sum()) >= k * R * (W - young) * cell, "a load wrote ring cells outside the live span"
    cols_equal(y.dump(), ly, sd[0], ly, "young groups")          # (the other groups of y are paint: only smr_ep_dump is asked)
    _close(src + [ys, y])
    # (3) a loaded object
    x = mk()
    raw = RawArena(x, dev)
    raw.paint(PAINT)
    whole = reps[r].save_state()
    x.load_state(whole)
    all_cols_equal(x, np.arange(G), want[r], np.arange(G), "painted, loaded")
    d0 = dumps_of(x)
    pend = read_image(whole.export())["exec"]
    r0 = raw.read()
    snap = reps[r].save_groups(lb)
    x.load_groups(snap, la)
    r1 = raw.read()
    ch = r1 != r0
    assert ch.any() and not (ch & ~fa_load).any(), "a load through a list wrote outside its groups"
    rest = np.setdiff1d(np.arange(G), la)
    all_cols_equal(x, rest, d0, rest, "beside a load")
    all_cols_equal(x, la, d0, lb, "loaded")
    x.reset_groups(lc)
    r2 = raw.read()
    ch = r2 != r1
    assert ch.any() and not (ch & ~fc).any(), "a reset wrote outside its groups"
    z = mk()
    assert np.array_equal(r2[fc], RawArena(z, dev).read()[fc]), "a reset slot is not a new object's, over all ring cells"
    assert not ((r2 != r0) & ~l_all).any()                       # (the counters and every gap: never touched)
    d2 = dumps_of(x)
    keep = np.setdiff1d(np.arange(G), np.concatenate([la, lc]))
    all_cols_equal(x, keep, want[r], keep, "every group no list named")
    all_cols_equal(x, lc, dumps_of(z), lc, "reset is create")
    for a_, b_ in zip(d2[:2], d0[:2]):
        assert np.array_equal(a_["counters"], b_["counters"]), "the counters are unchanged by load and reset through a list"
    poll = x.exec_poll()
    assert subs_of(poll, keep) == subs_of(pend, keep) and not subs_of(poll, lc), "submissions of the unlisted groups"
    in_c = np.zeros(G, bool); in_c[lc] = True
    la_kept, lb_kept = la[~in_c[la]], lb[~in_c[la]]
    assert subs_of(poll, la_kept) == subs_of(pend, lb_kept)
    _close([x, whole, snap, z])


# ---- 7. a reset slot runs from scratch -----------------------------------------------------------------------------------------------
def reset_then_run_from_scratch(dev, oracle, G=40, R=3, W=8, K=3, T1=12, T2=14, k=17, seed=53):
    """a cluster runs T1 ticks (rows wrapped); then k seeded groups are reset in all replicas and the run goes on for T2 ticks:
    tick by tick the reset groups' outputs, columns and submissions are those of a FRESH oracle cluster fed the same ticks, the
    neighbours' those of the oracle cluster that ran from the start"""
    from summerset_amd import epaxos
    rng = np.random.default_rng(seed)
    lst = np.sort(rng.permutation(G)[:k])
    in_lst = np.zeros(G, bool); in_lst[lst] = True
    rest = np.nonzero(~in_lst)[0]
    old, new = mk_oracle(oracle, G, R, W, K), mk_oracle(oracle, G, R, W, K)
    reps = mk_reps(G, R, W, K)
    eng = [LazyEngine(e, dev, []) for e in reps]

    def subs(e):                                                 # everything since the last call, group-major
        e.flush()
        got = c._sorted_subs(e.e.polls)
        del e.e.polls[:]
        return got
    for t in range(T1):
        keys, drop = schedule(rng, t, R, G, K)
        oe, oo = ec.tick(eng, keys, drop), ec.tick(old, keys, drop)
        for s in range(R):
            same(oo[s], oe[s], "tick %d, leader %d" % (t, s))
    assert max(int(o.dump()["len"].max()) for o in old) > W
    for r in range(R):
        c._subs_equal(old[r].take_submissions(), subs(eng[r]), "the first phase's submissions")
    epaxos.reset_cluster_groups(reps, lst)
    fresh = mk_reps(G, R, W, K)
    for r in range(R):
        all_cols_equal(reps[r], lst, dumps_of(fresh[r]), lst, "reset is create, replica %d" % r)
        all_cols_equal(reps[r], rest, (old[r].dump(), old[r].exec_dump(), None), rest, "beside the reset, replica %d" % r)
    _close(fresh)
    pick = lambda sub, keep: tuple(x[keep[sub[0]]] for x in sub)   # noqa: E731
    n_new = 0
    for t in range(T2):
        keys, drop = schedule(rng, T1 + t, R, G, K)
        oe, oo, on = ec.tick(eng, keys, drop), ec.tick(old, keys, drop), ec.tick(new, keys, drop)
        for s in range(R):
            cols_equal(oe[s], lst, on[s], lst, "tick %d, leader %d, the reset groups" % (t, s))
            cols_equal(oe[s], rest, oo[s], rest, "tick %d, leader %d, their neighbours" % (t, s))
        for r in range(R):
            all_cols_equal(reps[r], lst, (new[r].dump(), new[r].exec_dump(), None), lst, "tick %d rep %d, the reset groups" % (t, r))
            all_cols_equal(reps[r], rest, (old[r].dump(), old[r].exec_dump(), None), rest, "tick %d rep %d, their neighbours" % (t, r))
            got, so, sn = subs(eng[r]), old[r].take_submissions(), new[r].take_submissions()
            n_new += len(pick(sn, in_lst)[0])
            c._subs_equal(pick(got, in_lst), pick(sn, in_lst), (t, r, "reset groups"))
            c._subs_equal(pick(got, ~in_lst), pick(so, ~in_lst), (t, r, "neighbours"))
    assert max(int(o.dump()["len"][:, lst].max()) for o in new) > W and n_new > 0, "the reset groups wrap their rows again, and execute"
    _close(reps)


# ---- 8. list shapes ------------------------------------------------------------------------------------------------------------------
def list_shapes(dev, oracle, G=333, R=3, W=8, K=3, sizes=(330, None)):
    """330 entries (six tiles, two blocks) and n = G, ascending, descending and random: the group image is the numpy selection
    of the whole image and loads back through the list into new objects with the same columns"""
    reps, want = finished_cluster(dev, oracle, G, R, W, K, T=12)
    rng = np.random.default_rng(59)
    i = 0
    for n in sizes:
        n = G if n is None else min(n, G)
        pick = np.sort(np.concatenate([rng.permutation(G - 1)[:n - 1], [G - 1]]).astype(np.int64))
        for name, lst in (("ascending", pick), ("descending", pick[::-1].copy()), ("random", rng.permutation(pick))):
            r = i % R
            i += 1
            whole = reps[r].save_state().export()
            snap = reps[r].save_groups(lst)
            img = snap.export()
            assert img == select_image(whole, lst), (n, name)
            big = mk_reps(G, R, W, K, only=[r])[0]
            back = rng.permutation(G)[:n]
            big.load_groups(snap, back)
            all_cols_equal(big, back, want[r], lst, "%d %s, back" % (n, name))
            assert subs_of(big.exec_poll(), back) == subs_of(read_image(whole)["exec"], lst), (n, name, "submissions")
            if n == G and name == "ascending":                   # the full ascending list: the whole-state image but for the counters
                o = 64 + 8 * 15
                assert whole[:64] == img[:64] and whole[o:] == img[o:] and any(whole[64:o]) and not any(img[64:o])
            _close([snap, big])


def permutation_of_a_large_replica(dev, G=66000, R=3, W=8, K=2, T=4, seed=6):
    """device only: ep_snapshot_cases.two_sets_large's shape (1 032 tiles for the launch's 1 024 wavefronts, two tiles per
    wavefront).  A replica set after T ticks is saved through a permutation and loaded through the same permutation into new
    replicas: the export of save_state is the same bytes before and after (but for the counters, which stay)"""
    import torch
    from summerset_amd import epaxos
    from summerset_amd.ep_cluster import EPaxosCluster
    assert (G + 63) // 64 > 1024
    a, b = mk_reps(G, R, W, K), mk_reps(G, R, W, K)
    cl = EPaxosCluster(a)
    rng = np.random.default_rng(seed)
    for t in range(T):
        keys, drop = schedule(rng, t, R, G, K)
        cl.tick([torch.from_numpy(np.ascontiguousarray(keys[r])).to(dev) for r in range(R)], {k: torch.from_numpy(v).to(dev) for k, v in drop.items()})
    cl.close()
    perm = np.random.default_rng(61).permutation(G)
    before = [e.save_state().export() for e in a]
    snaps = epaxos.save_cluster_groups(a, perm)
    epaxos.load_cluster_groups(b, snaps, perm)
    o = 64 + 8 * 15
    for r in range(R):
        info = snaps[r].info()
        assert info["n_groups"] == G and info["n_cells"] == read_image(before[r])["hdr"]["n_cells"], info
        after = b[r].save_state().export()
        assert after[:64] == before[r][:64] and after[o:] == before[r][o:] and not any(after[64:o]), "replica %d" % r
    _close(snaps + a + b)


# ---- 9. the cluster form is the single calls -----------------------------------------------------------------------------------------
def cluster_form(dev, oracle, G=130, R=5, W=8, K=3, n=70):
    """one launch over the R replicas == the R single calls: the same images byte for byte, the same arenas after load and reset"""
    from summerset_amd import epaxos
    reps, want = finished_cluster(dev, oracle, G, R, W, K)
    rng = np.random.default_rng(79)
    n = min(n, G)
    lst, dst = rng.permutation(G)[:n], rng.permutation(G)[:n]
    one = [e.save_groups(lst) for e in reps]
    many = epaxos.save_cluster_groups(reps, lst)
    for r in range(R):
        assert one[r].export() == many[r].export(), r
    ta, tb = mk_reps(G, R, W, K), mk_reps(G, R, W, K)
    whole = [e.save_state() for e in reps]
    for r in range(R):
        ta[r].load_state(whole[r]); tb[r].load_state(whole[r])
        ta[r].load_groups(one[r], dst)
    epaxos.load_cluster_groups(tb, many, dst)
    for r in range(R):
        assert np.array_equal(RawArena(ta[r], dev).read(), RawArena(tb[r], dev).read()), ("load", r)
        all_cols_equal(tb[r], dst, want[r], lst, "load, replica %d" % r)
        ta[r].reset_groups(lst)
    epaxos.reset_cluster_groups(tb, lst)
    for r in range(R):
        assert np.array_equal(RawArena(ta[r], dev).read(), RawArena(tb[r], dev).read()), ("reset", r)
    # move_ep_groups is save, load and the reset of the source in one call; it returns the snapshots
    from summerset_amd import move_ep_groups
    tc = mk_reps(G, R, W, K)
    m = np.setdiff1d(dst, lst)
    assert len(m) > 0
    before, fresh = [dumps_of(e) for e in tb], [dumps_of(e) for e in tc]
    held = move_ep_groups(tb, m, tc, m[::-1].copy())
    for r in range(R):
        all_cols_equal(tc[r], m[::-1], before[r], m, "moved, replica %d" % r)
        all_cols_equal(tb[r], m, fresh[r], m, "vacated, replica %d" % r)
        assert held[r].info()["n_groups"] == len(m)
    again = move_ep_groups(tc, m[::-1].copy(), tb, m, snaps=held, reset=False)
    assert [id(x) for x in again] == [id(x) for x in held]
    for r in range(R):
        all_cols_equal(tb[r], m, before[r], m, "moved back, replica %d" % r)
        all_cols_equal(tc[r], m[::-1], before[r], m, "the source without a reset, replica %d" % r)
    _close(one + many + ta + tb + tc + whole + held)


# ---- 10. refusals --------------------------------------------------------------------------------------------------------------------
def refusals(dev, oracle, G=65, R=3, W=8, K=3, n=7):
    """every refusal of the header's list: SMR_ERR_ARG (SMR_ERR_STATE for an empty snapshot) with the message's noun, and
    dumps, images and info() as they were"""
    from summerset_amd import EPaxosReplicaGroup, EPaxosSnapshot, _lib, epaxos
    L = _lib.load()
    reps, want = finished_cluster(dev, oracle, G, R, W, K)
    a = reps[1]
    lst = np.arange(3, 3 + n)
    good = a.save_groups(lst)
    img, info = good.export(), good.info()
    base = dict(n_groups=G, population=R, me=1, window=W, n_keys=K, optimized_quorum=True, execute=True, recovery=False)
    mk = lambda **kw: EPaxosReplicaGroup(**dict(base, **kw))    # noqa: E731
    tgt = mk()
    whole = a.save_state()
    tgt.load_state(whole)
    d0 = dumps_of(tgt)

    def unchanged(what):
        for x, y in zip(dumps_of(tgt)[:2], d0[:2]):
            same(y, x, "%s: the replica changed" % (what,))
        assert good.export() == img and good.info() == info, (what, "the snapshot changed")
    # null arguments
    arr = (C.c_uint32 * n)(*lst.tolist())
    one = lambda x: (C.c_void_p * 1)(x._h)                       # noqa: E731
    for call in (lambda: L.smr_ep_save_groups(None, arr, n, good._h, None), lambda: L.smr_ep_save_groups(tgt._h, None, n, good._h, None),
                 lambda: L.smr_ep_save_groups(tgt._h, arr, n, None, None), lambda: L.smr_ep_load_groups(None, good._h, arr, n, None),
                 lambda: L.smr_ep_load_groups(tgt._h, None, arr, n, None), lambda: L.smr_ep_load_groups(tgt._h, good._h, None, n, None),
                 lambda: L.smr_ep_reset_groups(None, arr, n, None), lambda: L.smr_ep_reset_groups(tgt._h, None, n, None),
                 lambda: L.smr_ep_snapshot_create_groups(None, n, C.byref(C.c_void_p())), lambda: L.smr_ep_snapshot_create_groups(tgt._h, n, None),
                 lambda: L.smr_ep_cluster_save_groups(1, None, arr, n, one(good), None), lambda: L.smr_ep_cluster_save_groups(1, one(tgt), arr, n, None, None),
                 lambda: L.smr_ep_cluster_load_groups(1, one(tgt), None, arr, n, None), lambda: L.smr_ep_cluster_reset_groups(1, None, arr, n, None),
                 lambda: L.smr_ep_cluster_reset_groups(1, one(tgt), None, n, None)):
        assert call() == -1 and b"null argument" in L.smr_last_error(), L.smr_last_error()
    unchanged("null arguments")
    # the list
    for bad, word in (([], "a list of 0"), (list(range(G + 1)), "a list of"), ([0, G], "is group"), ([0, 2**32 - 1], "is group"), ([4, 5, 4], "listed twice")):
        k = len(bad)
        rs = EPaxosSnapshot(tgt, k).import_(a.save_groups(np.arange(k)).export()) if 0 < k <= G else good
        _refused(lambda: tgt.save_groups(bad, rs), word if 0 < k <= G else None)
        _refused(lambda: tgt.load_groups(rs, bad), word if 0 < k <= G else None)
        _refused(lambda: tgt.reset_groups(bad), word)
        _refused(lambda: epaxos.reset_cluster_groups([tgt], bad), word)
        unchanged(("list", word))
    for k in (0, G + 1):
        _refused(lambda: EPaxosSnapshot(tgt, k), "a snapshot of")
    other = np.arange(n + 1)                                     # a list length different from the snapshot's
    _refused(lambda: tgt.save_groups(other, good), "made for")
    _refused(lambda: tgt.load_groups(good, other), "made for")
    _refused(lambda: tgt.load_groups(whole, lst), "made for")     # ... a whole-object snapshot of another n_groups among them
    _refused(lambda: EPaxosSnapshot(tgt, n).import_(whole.export()), "the image is of")
    unchanged("another n")
    # another replica id / population / n_keys / execute / recovery / optimized_quorum; another window
    for what, kw in (("me", dict(me=0)), ("population", dict(population=R + 2)), ("n_keys", dict(n_keys=K + 1)), ("execute", dict(execute=False)),
                     ("recovery", dict(recovery=True)), ("optimized_quorum", dict(optimized_quorum=False)), ("window", dict(window=2 * W))):
        o = mk(**kw)
        b = o.dump()
        word = "window" if what == "window" else "made for another"
        _refused(lambda: o.load_groups(good, lst), word)
        if what != "window":                                     # (a larger window only makes the snapshot grow)
            _refused(lambda: o.save_groups(lst, good), word)
        mine = a.save_groups(lst)
        _refused(lambda: epaxos.load_cluster_groups([tgt, o], [good, mine], lst))
        if what in ("population", "n_keys", "execute", "recovery"):
            _refused(lambda: epaxos.reset_cluster_groups([tgt, o], lst), "the replicas differ")
        same(b, o.dump(), what)
        unchanged(what)
        _close([o, mine])
    # nothing saved or imported yet
    empty = EPaxosSnapshot(tgt, n)
    _refused(lambda: tgt.load_groups(empty, lst), "nothing saved", code=-3)
    # the cluster forms: a replica or a snapshot listed twice, replicas that differ
    spare = EPaxosSnapshot(tgt, n)
    t2 = mk(me=2)
    _refused(lambda: epaxos.save_cluster_groups([tgt, tgt], lst, [good, spare]), "listed twice")
    _refused(lambda: epaxos.save_cluster_groups([tgt, t2], lst, [good, good]), "listed twice")
    _refused(lambda: epaxos.reset_cluster_groups([tgt, tgt], lst), "listed twice")
    small = mk(n_groups=G - 1)
    _refused(lambda: epaxos.reset_cluster_groups([tgt, small], lst), "the replicas differ")
    unchanged("end")
    tgt.load_groups(good, lst)                                   # ... and the good one does load
    unchanged("the same groups again")
    _close([good, tgt, whole, empty, spare, t2, small])


# ---- 11. stream order ----------------------------------------------------------------------------------------------------------------
def stream_order(dev, oracle, G=130, R=3, W=8, K=3, k=40, seed=4):
    """save on a stream behind a proposal, reset and load on the same stream in front of the next one, no host synchronisation
    in between, the caller's list array overwritten right after each call returns: the image is the state at the save point, a
    reset slot takes the next proposal as a new object's would, and the load lands behind it"""
    import contextlib

    import torch
    from summerset_amd import EPaxosSnapshot, _lib
    from summerset_amd._lib import check
    L = _lib.load()
    orc = mk_oracle(oracle, G, R, W, K)
    reps = mk_reps(G, R, W, K)
    eng = [ec.NumpyEngine(e, dev) for e in reps]
    rng = np.random.default_rng(seed)
    for t in range(W + 2):
        keys, drop = schedule(rng, t, R, G, K, loss=0.1)
        ec.tick(eng, keys, drop); ec.tick(orc, keys, drop)
    e0, o0 = reps[0], orc[0]
    lst, dst = rng.permutation(G)[:k], rng.permutation(G)[:k]
    ks = [ec.same_key(rng, 1, G, K)[0] for _ in range(3)]
    tk = [torch.from_numpy(x).to(dev) for x in ks]
    snap = EPaxosSnapshot(e0, k)
    side = None if str(dev) == "cpu" else torch.cuda.Stream()    # one non-default stream (the emulator has the null stream alone)
    stream = None if side is None else side.cuda_stream
    sp = _lib.stream_ptr(stream)
    buf = np.zeros(k, np.uint32)

    def with_list(values, call):
        buf[:] = values
        check(call(buf.ctypes.data_as(C.c_void_p)))
        buf[:] = 0xFFFFFFFF                                      # the caller's array is its own again as soon as the call returns
    if side is not None:
        torch.cuda.synchronize()
    with (torch.cuda.stream(side) if side is not None else contextlib.nullcontext()):
        e0.handle_req_batch(tk[0], stream=stream)
        with_list(lst, lambda p: L.smr_ep_save_groups(e0._h, p, k, snap._h, sp))
        with_list(lst, lambda p: L.smr_ep_reset_groups(e0._h, p, k, sp))
        e0.handle_req_batch(tk[1], stream=stream)
        with_list(dst, lambda p: L.smr_ep_load_groups(e0._h, snap._h, p, k, sp))
        e0.handle_req_batch(tk[2], stream=stream)
    if side is not None:
        side.synchronize()
    o0.propose(ks[0])
    saved = (o0.dump(), o0.exec_dump(), None)
    im = read_image(snap.export())
    for f in ("len", "commit_bars", "bal", "seq", "status", "key", "deps", "pa_acks", "acc_acks", "bk", "highest_cols"):
        assert np.array_equal(im[f], take(f, saved[0][f], lst)), "the image between two proposals: %s" % f
    for f in ("exec_bars", "kv", "digest"):
        assert np.array_equal(im[f], take(f, saved[1][f], lst)), "the image between two proposals: %s" % f
    # the final state, per group.  Loaded over (dst[i]): the saved state of lst[i], then the third proposal -- an oracle cannot
    # load, so the oracle's group lst[i] sits the second proposal out and takes dst[i]'s key of the third.  Reset and not loaded
    # over: a new object's, then the second and third proposals.  Named by no list: all three proposals
    in_lst = np.zeros(G, bool); in_lst[lst] = True
    in_dst = np.zeros(G, bool); in_dst[dst] = True
    k1, k2 = np.where(in_lst, NO_KEY, ks[1]).astype(np.uint8), ks[2].copy()
    k2[lst] = ks[2][dst]
    o0.propose(k1); o0.propose(k2)
    fresh = mk_oracle(oracle, G, R, W, K)[0]
    fresh.propose(ks[1]); fresh.propose(ks[2])
    got = dumps_of(e0)
    plain, only_reset = np.nonzero(~in_lst & ~in_dst)[0], np.nonzero(in_lst & ~in_dst)[0]
    assert len(plain) and len(only_reset)
    for i_, (gd, od, fd) in enumerate(zip(got[:2], (o0.dump(), o0.exec_dump()), (fresh.dump(), fresh.exec_dump()))):
        cols_equal(gd, plain, od, plain, "groups no list named (%d)" % i_)
        cols_equal(gd, dst, od, lst, "the load landed behind the second proposal and in front of the third (%d)" % i_)
        cols_equal(gd, only_reset, fd, only_reset, "reset slots take the next proposals as a new object's (%d)" % i_)
    _close(reps + [snap])
