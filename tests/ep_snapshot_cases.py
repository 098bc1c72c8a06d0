"""Bodies of the EPaxos save / load tests (smr_ep_save_state / smr_ep_load_state and their cluster forms), taking the device:
tests/test_ep_snapshot.py runs them on the emulator, tests/test_zzzz_ep_snapshot_gpu.py on the GPU.  The engines and the CPU
oracle are driven by tests/ep_cluster.py.  `read_image` / `write_image` are written from DESIGN.md 2's table alone."""
import ctypes as C

import numpy as np

import ep_cluster as ec

N, NO_KEY = 0xFFFFFFFF, 0xFF
MAGIC, VERSION = 0x53504553, 1
HDR = np.dtype([("magic", "<u4"), ("version", "<u4"), ("bytes", "<u8"), ("n_groups", "<u4"), ("population", "u1"), ("me", "u1"),
                ("optimized_quorum", "u1"), ("execute", "u1"), ("recovery", "u1"), ("reserved0", "u1", 3), ("window", "<u4"),
                ("n_keys", "<u4"), ("max_live", "<u4"), ("n_cells", "<u8"), ("n_exec", "<u8"), ("max_exec", "<u4"), ("n_replies", "<u4")])
CELL = np.dtype([("bal", "<u8"), ("seq", "<u8"), ("deps", "<u4", 8), ("xp_max", "<u8"), ("status", "u1"), ("key", "u1"), ("bk", "u1"),
                 ("pa_acks", "u1"), ("acc_acks", "u1"), ("avoid", "u1"), ("xp_acks", "u1"), ("xp_has", "u1")])
assert HDR.itemsize == 64 and CELL.itemsize == 64


def a8(x):
    return (int(x) + 7) & ~7


# ---- the image ---------------------------------------------------------------------------------------------------
def reply_dtype(R, recovery):
    f = [("pa_seq", "<u8", R)] + ([("xv_seq", "<u8", R)] if recovery else []) + [("pa_deps", "<u4", (R, R))]
    if recovery:
        f += [("xv_deps", "<u4", (R, R)), ("xv_status", "u1", R), ("xv_key", "u1", R)]
    n = np.dtype(f).itemsize
    if a8(n) > n:
        f.append(("pad", "u1", a8(n) - n))
    return np.dtype(f)


def _scalars(G, R, K, execute):
    """(name, dtype, shape) of the fixed part behind the header, in order; every array padded to 8"""
    s = [("counters", "<u8", (7,))] + ([("exec_counters", "<u8", (8,))] if execute else [])
    s += [("len", "<u4", (R, G)), ("commit_bars", "<u4", (R, G)), ("rewritten", "u1", (G,))]
    if execute:
        s += [("exec_bars", "<u4", (R, G)), ("prev_cb", "<u4", (R, G)), ("digest", "<u8", (G,)), ("n_sub", "<u4", (G,))]
    s += [("highest_cols", "<u4", (K, R, G))]
    if execute:
        s += [("kv", "<u8", (K, G))]
    return s


def _cell_order(length, W, G, R):
    """(group, row, column) of every live cell in the image's order: tile-major (64 groups), then row, then k, then group"""
    lo = np.where(length > W, length - W, 0).astype(np.int64)
    n = length.astype(np.int64) - lo
    gi, ri, ci = [], [], []
    for t0 in range(0, G, 64):
        gs = np.arange(t0, min(t0 + 64, G))
        for r in range(R):
            nr = n[r, gs]
            for k in range(int(nr.max()) if len(gs) else 0):
                sel = gs[nr > k]
                gi.append(sel); ri.append(np.full(len(sel), r)); ci.append(lo[r, sel] + k)
    cat = lambda x: np.concatenate(x) if x else np.zeros(0, np.int64)
    return cat(gi), cat(ri), cat(ci)


def _exec_order(n_sub, G):
    """(group, list position) of every exec entry in the image's order: tile-major, then list position, then group"""
    gi, ji = [], []
    for t0 in range(0, G, 64):
        gs = np.arange(t0, min(t0 + 64, G))
        ns = n_sub[gs].astype(np.int64)
        for j in range(int(ns.max()) if len(gs) else 0):
            sel = gs[ns > j]
            gi.append(sel); ji.append(np.full(len(sel), j))
    cat = lambda x: np.concatenate(x) if x else np.zeros(0, np.int64)
    return cat(gi), cat(ji)


def read_image(buf):
    """the image as dump-shaped arrays (cells outside the live spans as the dumps give them), every padding byte checked"""
    b = np.frombuffer(bytes(buf), np.uint8)
    h = b[:64].view(HDR)[0]
    assert h["magic"] == MAGIC and h["version"] == VERSION and int(h["bytes"]) == len(b) and not h["reserved0"].any()
    G, R, K, W = int(h["n_groups"]), int(h["population"]), int(h["n_keys"]), int(h["window"])
    ex, rec, me = int(h["execute"]), int(h["recovery"]), int(h["me"])
    im, off = dict(hdr=h), 64
    for name, dt, shape in _scalars(G, R, K, ex):
        nb = int(np.prod(shape)) * np.dtype(dt).itemsize
        assert off % 8 == 0
        im[name] = b[off:off + nb].view(dt).reshape(shape).copy()
        assert not b[off + nb:off + a8(nb)].any(), "padding of %s" % name
        off += a8(nb)
    assert not b[off:(off + 15) & ~15].any(), "padding in front of the cell records"
    off = (off + 15) & ~15                                       # the cell records start on a multiple of 16
    gi, ri, ci = _cell_order(im["len"], W, G, R)
    assert len(gi) == int(h["n_cells"])
    cells = b[off:off + 64 * len(gi)].view(CELL)
    off += 64 * len(gi)
    assert int(h["max_live"]) == int((im["len"] - np.where(im["len"] > W, im["len"] - W, 0)).max())
    w = ci & (W - 1)
    for f, fill, dt in (("bal", 0, np.uint64), ("seq", 0, np.uint64), ("status", 0, np.uint8), ("key", NO_KEY, np.uint8), ("bk", 0, np.uint8),
                        ("pa_acks", 0, np.uint8), ("acc_acks", 0, np.uint8), ("avoid", 0, np.uint8), ("xp_acks", 0, np.uint8),
                        ("xp_has", 0, np.uint8), ("xp_max", 0, np.uint64)):
        im[f] = np.full((R, W, G), fill, dt)
        im[f][ri, w, gi] = cells[f]
    im["deps"] = np.full((R, W, G, R), N, np.uint32)
    im["deps"][ri, w, gi] = cells["deps"][:, :R]
    assert (cells["deps"][:, R:] == N).all()
    im["cells"] = cells
    tab = (ri == me) | bool(rec)
    assert int(tab.sum()) == int(h["n_replies"])
    rdt = reply_dtype(R, rec)
    reps = b[off:off + rdt.itemsize * int(tab.sum())].view(rdt)
    off += rdt.itemsize * int(tab.sum())
    if "pad" in rdt.names:
        assert not reps["pad"].any()
    im["replies"], im["reply_at"] = reps, (gi[tab], ri[tab], ci[tab])
    # the canonical rule: an entry is carried only where a reader can reach it
    cm = cells[tab]
    lbk = (cm["bk"] & 1) == 1
    for p in range(R):
        on = lbk & (cm["status"] == 1) & (((cm["pa_acks"] >> p) & 1) == 1)
        assert (reps["pa_seq"][~on, p] == 0).all() and (reps["pa_deps"][~on, p] == N).all()
        if rec:
            on = lbk & (((cm["xp_has"] >> p) & 1) == 1)
            assert (reps["xv_seq"][~on, p] == 0).all() and (reps["xv_deps"][~on, p] == N).all()
            assert (reps["xv_status"][~on, p] == 0).all() and (reps["xv_key"][~on, p] == NO_KEY).all()
    if rec:
        tg, tr, tc = im["reply_at"]
        for f, fld, fill, dt, tail in (("vstatus", "xv_status", 0, np.uint8, ()), ("vseq", "xv_seq", 0, np.uint64, ()), ("vkey", "xv_key", NO_KEY, np.uint8, ()),
                                       ("vdeps", "xv_deps", N, np.uint32, (R,))):
            im[f] = np.full((R, W, R) + tail + (G,), fill, dt)
            im[f][tr, tc & (W - 1), ..., tg] = reps[fld]
    ne = int(h["n_exec"])
    xe = b[off:off + 8 * ne].view("<u4").reshape(ne, 2)
    off += 8 * ne
    assert off == len(b)
    if ex:
        xg, xj = _exec_order(im["n_sub"], G)
        assert len(xg) == ne and int(h["max_exec"]) == int(im["n_sub"].max())
        k = np.lexsort((xj, xg))                                 # group-major, list position within a group: smr_ep_exec_poll's order
        im["exec"] = (xg[k].astype(np.uint32), xe[k, 1].astype(np.uint8), xe[k, 0].astype(np.uint32))
    else:
        assert ne == 0
    return im


def write_image(cfg, st):
    """an image from dump-shaped arrays: cfg = dict(G, R, me, oq, execute, recovery, W, K); st: the arrays of `_scalars` by name,
    the cell fields as [R][W][G] (deps [R][W][G][R]), replies as a dict by (row, col, g) -> dict of reply fields, exec as a list
    of (g, row, col) in submission order per group"""
    G, R, K, W, ex, rec, me = cfg["G"], cfg["R"], cfg["K"], cfg["W"], cfg["execute"], cfg["recovery"], cfg["me"]
    parts = []
    for name, dt, shape in _scalars(G, R, K, ex):
        a = np.ascontiguousarray(st.get(name, np.zeros(shape, dt)), dtype=dt).reshape(shape).tobytes()
        parts.append(a + bytes(a8(len(a)) - len(a)))
    n = 64 + sum(len(x) for x in parts)
    parts.append(bytes(((n + 15) & ~15) - n))
    length = np.asarray(st["len"], np.uint32).reshape(R, G)
    gi, ri, ci = _cell_order(length, W, G, R)
    cells = np.zeros(len(gi), CELL)
    w = ci & (W - 1)
    for f in ("bal", "seq", "status", "key", "bk", "pa_acks", "acc_acks", "avoid", "xp_acks", "xp_has", "xp_max"):
        if f in st:
            cells[f] = st[f][ri, w, gi]
        elif f == "key":
            cells[f] = NO_KEY
    cells["deps"] = N
    if "deps" in st:
        cells["deps"][:, :R] = st["deps"][ri, w, gi]
    tab = (ri == me) | bool(rec)
    reps = np.zeros(int(tab.sum()), reply_dtype(R, rec))
    reps["pa_deps"] = N
    if rec:
        reps["xv_deps"] = N; reps["xv_key"] = NO_KEY
    for i, key in enumerate(zip(ri[tab], ci[tab], gi[tab])):
        for f, v in st.get("replies", {}).get(tuple(int(x) for x in key), {}).items():
            reps[f][i] = v
    n_sub = np.asarray(st.get("n_sub", np.zeros(G)), np.int64)
    xg, xj = _exec_order(n_sub, G)
    per = {}
    for g, row, col in st.get("exec", []):
        per.setdefault(g, []).append((col, row))
    xe = np.array([per[int(g)][int(j)] for g, j in zip(xg, xj)], "<u4").reshape(len(xg), 2)
    body = b"".join(parts) + cells.tobytes() + reps.tobytes() + xe.tobytes()
    h = np.zeros(1, HDR)
    live = length.astype(np.int64) - np.where(length > W, length - W, 0)
    for f, v in (("magic", MAGIC), ("version", VERSION), ("bytes", 64 + len(body)), ("n_groups", G), ("population", R), ("me", me),
                 ("optimized_quorum", cfg["oq"]), ("execute", ex), ("recovery", rec), ("window", W), ("n_keys", K), ("max_live", int(live.max())),
                 ("n_cells", len(gi)), ("n_exec", len(xg)), ("max_exec", int(n_sub.max()) if G else 0), ("n_replies", len(reps))):
        h[f] = v
    return h.tobytes() + body


# ---- engines ------------------------------------------------------------------------------------------------------------------
class _Lazy:
    """an EPaxosReplicaGroup whose unpolled submissions are taken right before its next handler call, not right after the last
    one: a save at a tick's end then finds the list in place"""

    def __init__(self, e, polls):
        self.e, self.polls, self.pending = e, polls, False

    def flush(self):
        if self.pending and self.e.execute:
            self.polls.append(self.e.exec_poll())
        self.pending = False

    def __getattr__(self, n):
        a = getattr(self.e, n)
        if n.startswith("handle_") or n == "heartbeat_timeout":
            def call(*x, **k):
                self.flush()
                return a(*x, **k)
            return call
        return a


class LazyEngine(ec.NumpyEngine):
    def __init__(self, eng, dev, polls):
        super().__init__(_Lazy(eng, polls), dev)
        self._polls, self.raw = polls, eng

    def _after_call(self):
        self.e.pending = True

    def flush(self):
        self.e.flush()

    def take_submissions(self):
        self.flush()
        return super().take_submissions()


def mk_reps(G, R, W, K, execute=True, recovery=False, oq=True, only=None):
    from summerset_amd import EPaxosReplicaGroup
    return [EPaxosReplicaGroup(G, R, me=r, window=W, n_keys=K, optimized_quorum=oq, execute=execute, recovery=recovery)
            for r in (range(R) if only is None else only)]


def mk_oracle(oracle, G, R, W, K, execute=True, oq=True):
    return [oracle.EpOracle(G, R, me=r, W=W, n_keys=K, optimized_quorum=oq, execute=execute) for r in range(R)]


def schedule(rng, t, R, G, K, loss=0.2):
    """keys and PreAccept drops of tick t: Zipf and same-key ticks alternate, every (sender, receiver) pair loses PreAccepts at
    `loss`, and every third tick one leader hears nothing in half of its groups (its instance stays PreAccepting)"""
    keys = ec.same_key(rng, R, G, K) if t % 2 else ec.zipf_keys(rng, R, G, K)
    drop = {(s, q): rng.random(G) < loss for s in range(R) for q in range(R) if s != q} if loss > 0 else {}
    if t % 3 == 1:
        for k, m in ec.isolated_leader(R, G, t % R, rng.random(G) < 0.5).items():
            drop[k] = drop.get(k, np.zeros(G, bool)) | m
    return keys, (drop or None)


def same(a, b, what, skip=()):
    for k in a:
        if k not in skip:
            assert np.array_equal(np.asarray(a[k]), np.asarray(b[k])), "%s: %s differs" % (what, k)


def image_vs_dumps(im, d, xd, xp, what):
    """the image, field by field, against the dumps of the replica (or of the oracle's) at the same point"""
    for f in ("len", "commit_bars", "bal", "seq", "status", "key", "deps", "pa_acks", "acc_acks", "bk", "highest_cols"):
        assert np.array_equal(im[f], d[f]), "%s: %s" % (what, f)
    assert np.array_equal(im["counters"][:3], d["counters"]), what
    if xd is not None:
        for f in ("exec_bars", "kv", "digest"):
            assert np.array_equal(im[f], xd[f]), "%s: %s" % (what, f)
        c = im["exec_counters"][:6].copy()
        assert c[3] == 0
        assert np.array_equal(c, xd["counters"]), what
        assert np.array_equal(im["prev_cb"], im["commit_bars"]), "%s: the executor's commit-bar copies at a call boundary" % what
    if xp is not None:
        for f, g in (("xp_acks", "acks"), ("xp_max", "max_bal"), ("avoid", "avoid"), ("xp_has", "has"), ("vstatus", "vstatus"), ("vseq", "vseq"),
                     ("vkey", "vkey"), ("vdeps", "vdeps")):
            assert np.array_equal(im[f], xp[g]), "%s: %s" % (what, g)
        assert np.array_equal(im["counters"][3:7], xp["counters"]), what


def coverage(cov, im, R):
    c = im["cells"]
    q = R // 2 + 1
    pop = np.array([bin(x).count("1") for x in range(256)])
    cov["preaccepting_short"] |= bool(((c["status"] == 1) & ((c["bk"] & 1) == 1) & (pop[c["pa_acks"]] < q)).any())
    cov["accepting"] |= bool((c["status"] == 2).any())
    cov["committed"] |= bool((c["status"] == 3).any())
    cov["executed"] |= bool((c["status"] == 5).any())
    cov["wrapped"] |= bool((im["len"] > int(im["hdr"]["window"])).any())
    cov["pending"] |= int(im["hdr"]["n_exec"]) > 0
    cov["has_entry"] |= bool((c["xp_has"] != 0).any())


def save_set(reps, snaps, cluster_form):
    from summerset_amd import epaxos
    if cluster_form:
        epaxos.save_cluster_state(reps, snaps)
    else:
        for r, s in zip(reps, snaps):
            r.save_state(s)


def load_set(reps, snaps, cluster_form):
    from summerset_amd import epaxos
    if cluster_form:
        epaxos.load_cluster_state(reps, snaps)
    else:
        for r, s in zip(reps, snaps):
            r.load_state(s)


def all_dumps(e, execute=True, recovery=False):
    return e.dump(), (e.exec_dump() if execute else None), (e.xp_dump() if recovery else None)


def _subs_equal(a, b, what):
    for x, y in zip(a, b):
        assert np.array_equal(x, y), what


def _sorted_subs(parts):
    g = np.concatenate([p[0] for p in parts]) if parts else np.zeros(0, np.uint32)
    r = np.concatenate([p[1] for p in parts]) if parts else np.zeros(0, np.uint8)
    c = np.concatenate([p[2] for p in parts]) if parts else np.zeros(0, np.uint32)
    k = np.argsort(g, kind="stable")
    return g[k], r[k], c[k]


# ---- 2. shadow ----------------------------------------------------------------------------------------------------------------
def shadow(dev, oracle, G, R, **kw):
    """`_shadow` with its smr_ep_cluster objects closed whatever happens (they must go before their replicas do)"""
    clusters = []
    try:
        return _shadow(dev, oracle, G, R, clusters=clusters, **kw)
    finally:
        for c in clusters:
            c.close()


def _shadow(dev, oracle, G, R, W=8, K=3, T=None, cluster_form=False, seated=False, recovery=False, seed=11, use_oracle=True,
            want=True, image_out=None, clusters=None):
    """Two engine sets A and B beside the oracle cluster: after every tick the running set is saved, every image read and compared
    with the oracle's dumps, then loaded into the other set -- dirty from three ticks of another seed, later stale -- which runs
    the next tick; the loaded replica hands over the submissions the saved one had not (equal to the image's list).  seated: the sets sit in an smr_ep_cluster each and are ticked by smr_ep_cluster_tick, mode 0 on even ticks'
    set and mode 2 on the other's.  One tick in the middle is cut short for the last replica (ec.crash_tick) so that Accepting
    cells stand at a boundary; with recovery that tick is the last, and the survivors then recover the row through a save / load."""
    import torch
    from summerset_amd import EPaxosSnapshot
    from summerset_amd.ep_cluster import EPaxosCluster
    T = 2 * W + 4 if T is None else T
    orc = mk_oracle(oracle, G, R, W, K) if use_oracle else None
    sets = [mk_reps(G, R, W, K, True, recovery) for _ in range(2)]
    polls = [[] for _ in range(R)]
    eng = [[LazyEngine(e, dev, polls[r]) for r, e in enumerate(s)] for s in sets]
    if seated:
        clusters += [EPaxosCluster(sets[0]), EPaxosCluster(sets[1], phase_major=True)]
    snaps = [EPaxosSnapshot(e) for e in sets[0]]
    rng0 = np.random.default_rng(seed + 1000)
    for t in range(3):                                           # B is dirty
        keys, drop = schedule(rng0, t, R, G, K)
        ec.tick(eng[1], keys, drop)
    for e in eng[1]:
        e.e.pending = False
    for p in polls:
        del p[:]
    rng = np.random.default_rng(seed)
    cov = dict(preaccepting_short=False, accepting=False, committed=False, executed=False, wrapped=False, pending=False, has_entry=False, ticks=0)
    orc_subs = [[] for _ in range(R)]
    run = 0
    t_cut = T - 1 if recovery else W + 3
    live = list(range(R))

    def boundary(members, what):
        """save the running set's members, check the images, load them into the other set, go on with that one"""
        nonlocal run
        ms, mp = [sets[run][r] for r in members], [snaps[r] for r in members]
        save_set(ms, mp, cluster_form)
        for r in members:
            im = read_image(snaps[r].export())
            if image_out is not None:
                image_out.append(snaps[r].export())
            if orc is not None:
                image_vs_dumps(im, orc[r].dump(), orc[r].exec_dump(), orc[r].xp_dump() if recovery else None, "%s, replica %d" % (what, r))
            else:
                image_vs_dumps(im, *all_dumps(sets[run][r], True, recovery), "%s, replica %d" % (what, r))
            coverage(cov, im, R)
            eng[run][r].e.pending = False                        # (its list goes over with the image)
        other = run ^ 1
        load_set([sets[other][r] for r in members], mp, cluster_form)
        for r in members:
            im = read_image(snaps[r].export())
            eng[other][r].e.pending = True
            eng[other][r].flush()                                # the loaded replica hands over what the saved one had not
            _subs_equal(polls[r][-1], im["exec"], "%s, replica %d: the unpolled submissions" % (what, r))
        run = other

    for t in range(T):
        keys, drop = schedule(rng, t, R, G, K)
        if t == t_cut:                                           # the last replica's tick is cut short
            k1 = np.ascontiguousarray(keys[R - 1])
            cut_e = ec.crash_tick(eng[run], R - 1, k1, np.random.default_rng(seed + t), G)
            if orc is not None:
                cut_o = ec.crash_tick(orc, R - 1, k1, np.random.default_rng(seed + t), G)
                assert np.array_equal(cut_e, cut_o)
        elif seated:
            tk = [torch.from_numpy(np.ascontiguousarray(keys[r])).to(dev) for r in range(R)]
            td = {k: torch.from_numpy(v).to(dev) for k, v in drop.items()} if drop else None
            for e in eng[run]:
                e.flush()
            out = clusters[run].tick(tk, td)
            for e in eng[run]:
                e.e.pending = True
            out_e = [{k: v.cpu().numpy().view(np.uint32 if v.dtype == torch.int32 else np.uint64 if v.dtype == torch.int64 else np.uint8)
                      for k, v in o.items()} for o in out]
            if orc is not None:
                out_o = ec.tick(orc, keys, drop, phase_major=bool(run))
                for s in range(R):
                    same(out_o[s], out_e[s], "tick %d, leader %d" % (t, s))
        else:
            out_e = ec.tick(eng[run], keys, drop)
            if orc is not None:
                out_o = ec.tick(orc, keys, drop)
                for s in range(R):
                    same(out_o[s], out_e[s], "tick %d, leader %d" % (t, s))
        if orc is not None:
            for r in range(R):
                orc_subs[r].append(orc[r].take_submissions())
        boundary(live, "tick %d" % t)
        cov["ticks"] += 1
    if recovery:                                                 # the survivors recover the dead replica's row on state that was loaded
        dead, live = R - 1, list(range(R - 1))
        te, to = [], []
        ec.recover_row(eng[run], 0, dead, live, G, rng=np.random.default_rng(seed + 7), loss=0.2, trace=te)
        ec.recover_row(orc, 0, dead, live, G, rng=np.random.default_rng(seed + 7), loss=0.2, trace=to)
        assert len(te) == len(to) and len(te) > 0
        for a, b in zip(te, to):
            assert a[0] == b[0]
            for x, y in zip(a[1:], b[1:]):
                assert np.array_equal(x, y), "the recovery's trace differs at %s" % (a[0],)
        for r in live:
            orc_subs[r].append(orc[r].take_submissions())
        boundary(live, "after the recovery")
    for r in live:
        e = eng[run][r]
        if orc is not None:
            d, xd, xp = all_dumps(e, True, recovery)
            same(orc[r].dump(), d, "final dump of replica %d" % r)
            same(orc[r].exec_dump(), xd, "final exec_dump of replica %d" % r)
            if recovery:
                same(orc[r].xp_dump(), xp, "final xp_dump of replica %d" % r)
            if not seated:                                       # (smr_ep_cluster_tick leaves the list of the tick's LAST handler, as the handler-by-handler
                #  loop does, and nothing polls inside its one call: there the digest of exec_dump stands for the whole order)
                _subs_equal(_sorted_subs(orc_subs[r]), e.take_submissions(), "the submissions of replica %d" % r)
    if want:
        for k in ("preaccepting_short", "accepting", "committed", "executed", "wrapped", "pending"):
            assert cov[k], "no saved image held: %s" % k
        assert cov["has_entry"] or not recovery, "no saved image held a has-entry bit"
    return cov


# ---- 3. stored replies --------------------------------------------------------------------------------------------------------
def stored_replies_survive(dev, oracle, G=65, R=5, W=8, K=3, seed=5):
    """Instances stay PreAccepting with some replies stored (the others lost on their way back); save, load into fresh replicas;
    then the ballot-0 re-evaluation of smr_ep_heartbeat_timeout for a peer whose replies were lost reads pa_seq / pa_deps"""
    orc = mk_oracle(oracle, G, R, W, K, execute=False)
    a = mk_reps(G, R, W, K, execute=False, recovery=True)
    ea = [ec.NumpyEngine(e, dev) for e in a]
    rng = np.random.default_rng(seed)
    lostq = [R - 1, R - 2]                                        # three acks of five stay: a quorum, no fast quorum while two may still answer
    mask = lambda s: np.array([[q in lostq and q != s] * G for q in range(R)])
    for t in range(3):
        keys = ec.same_key(rng, R, G, K) if t else ec.zipf_keys(rng, R, G, K)
        oe, oo = ec.tick(ea, keys, via=ec.lost_replies(mask)), ec.tick(orc, keys, via=ec.lost_replies(mask))
        for s in range(R):
            same(oo[s], oe[s], "tick %d, leader %d" % (t, s))
    b = mk_reps(G, R, W, K, execute=False, recovery=True)
    eb = [ec.NumpyEngine(e, dev) for e in b]
    stored = 0
    for r in range(R):
        snap = a[r].save_state()
        im = read_image(snap.export())
        stored += int((im["replies"]["pa_seq"] != 0).sum())
        b[r].load_state(snap)
    assert stored > 0
    src = np.full(G, lostq[0], np.uint8)
    ex = np.full(G, (1 << lostq[0]) | (1 << lostq[1]), np.uint8)
    moved = 0
    for r in range(R - 2):
        he, ho = eb[r].heartbeat_timeout(src, ex), orc[r].heartbeat_timeout(src, ex)
        same(ho, he, "heartbeat_timeout at replica %d" % r)
        same(orc[r].dump(), eb[r].dump(), "dump of replica %d" % r)
        same(orc[r].xp_dump(), eb[r].xp_dump(), "xp_dump of replica %d" % r)
        moved += int(eb[r].dump()["counters"][1])
    assert moved > 0                                             # the re-evaluation took the slow path on the stored replies
    return moved


# ---- 4. canonical bytes -------------------------------------------------------------------------------------------------------
def canonical_bytes(dev, oracle, G=130, R=5, W=8, K=3, T=12, seed=3):
    """the same schedule handler by handler, by smr_ep_cluster_tick mode 0 (seated in the cluster's shared table) and mode 1,
    and -- without execution -- phase by phase: wherever the four dumps agree the exports are the same bytes"""
    import torch
    from summerset_amd.ep_cluster import EPaxosCluster

    def run(how, execute):
        reps = mk_reps(G, R, W, K, execute=execute)
        cl = None if how in ("handlers", "phase") else EPaxosCluster(reps, per_handler_launches=(how == "mode1"), phase_major=(how == "mode2"))
        eng = [LazyEngine(e, dev, []) for e in reps]
        rng = np.random.default_rng(seed)
        for t in range(T):
            keys, drop = schedule(rng, t, R, G, K)
            if cl is None:
                ec.tick(eng, keys, drop, phase_major=(how == "phase"))
            else:
                cl.tick([torch.from_numpy(np.ascontiguousarray(keys[r])).to(dev) for r in range(R)],
                        {k: torch.from_numpy(v).to(dev) for k, v in drop.items()} if drop else None)
        for e in eng:
            e.e.pending = False
        if execute:                                              # the pending list is the last CALL's: take it on every path
            for e in reps:
                e.exec_poll()
        out = [(e.save_state().export(), all_dumps(e, execute)) for e in reps]
        if how == "mode0":                                       # ... and unseated: the cluster hands the entries back to the private tables
            cl.close()
            again = [e.save_state().export() for e in reps]
            assert [o[0] for o in out] == again, "seated and unseated exports differ"
        return out

    for execute, hows in ((True, ("handlers", "mode0", "mode1")), (False, ("phase", "mode2"))):
        res = [run(h, execute) for h in hows]
        for other, h in zip(res[1:], hows[1:]):
            for r in range(R):
                for da, db in zip(res[0][r][1], other[r][1]):
                    if da is not None:
                        same(da, db, "%s against %s, replica %d" % (hows[0], h, r))
                assert res[0][r][0] == other[r][0], "%s and %s: equal dumps, different bytes (replica %d)" % (hows[0], h, r)
    # export(load(import(export))) is the identity
    from summerset_amd import EPaxosSnapshot
    img = res[0][0][0]
    fresh = mk_reps(G, R, W, K, execute=False, only=[0])[0]
    s = EPaxosSnapshot(fresh).import_(img)
    assert s.export() == img
    fresh.load_state(s)
    assert fresh.save_state().export() == img


# ---- 5. a hand-built image ----------------------------------------------------------------------------------------------------
def hand_built_image(dev, G=70, R=3, W=8, K=2):
    """written from DESIGN.md 2's table: a wrapped row, a short row, an empty row, a Null cell inside a span, a pending
    submission, a stored reply; imported and loaded, the dumps give back what was written"""
    from summerset_amd import EPaxosSnapshot
    me = 1
    cfg = dict(G=G, R=R, me=me, oq=1, execute=1, recovery=0, W=W, K=K)
    rng = np.random.default_rng(2)
    length = np.zeros((R, G), np.uint32)
    length[0] = W + 3 + (np.arange(G) % 5)                       # wrapped
    length[1] = 1 + (np.arange(G) % 3)                           # short
    length[2, 69] = 2                                            # empty but for one group
    st = dict(len=length, commit_bars=np.minimum(length, 1).astype(np.uint32), rewritten=(np.arange(G) % 7 == 0).astype(np.uint8))
    st["exec_bars"] = np.zeros((R, G), np.uint32); st["prev_cb"] = st["commit_bars"].copy()
    st["digest"] = rng.integers(0, 2**63, G, dtype=np.uint64)
    st["highest_cols"] = np.full((K, R, G), N, np.uint32); st["highest_cols"][1, 0] = length[0] - 1
    st["kv"] = np.zeros((K, G), np.uint64); st["kv"][1] = (np.uint64(1) << np.uint64(32)) | np.uint64(5)
    st["counters"] = np.arange(1, 8, dtype=np.uint64); st["exec_counters"] = np.array([9, 8, 7, 0, 5, 4, 0, 0], np.uint64)
    lo = np.where(length > W, length - W, 0)
    live = np.zeros((R, W, G), bool)
    for r in range(R):
        for g in range(G):
            for c in range(int(lo[r, g]), int(length[r, g])):
                live[r, c & (W - 1), g] = True
    st["status"] = np.where(live, 3, 0).astype(np.uint8)
    st["status"][0, int(lo[0, 4] + 2) & (W - 1), 4] = 0           # a Null cell inside a span
    st["status"][me, 0, :] = 1                                   # my row's first cell: PreAccepting, leader bookkeeping, two acks
    st["bk"] = np.zeros((R, W, G), np.uint8); st["bk"][me, 0, :] = 1
    st["pa_acks"] = np.zeros((R, W, G), np.uint8); st["pa_acks"][me, 0, :] = 0b011
    st["acc_acks"] = np.zeros((R, W, G), np.uint8)
    st["key"] = np.where(live & (st["status"] != 0), 1, NO_KEY).astype(np.uint8)
    st["bal"] = np.where(live, 2, 0).astype(np.uint64); st["bal"][0, 1, 3] = (1 << 40) + 2
    st["seq"] = np.where(live, 7, 0).astype(np.uint64); st["seq"][0, 2, 5] = (1 << 33) + 1   # past sq32's 32 bits
    st["deps"] = np.full((R, W, G, R), N, np.uint32); st["deps"][0][live[0]] = (1, N, 0)
    st["replies"] = {(me, 0, g): dict(pa_seq=(4, 9, 0), pa_deps=((1, N, N), (2, 0, N), (N, N, N))) for g in range(G)}
    st["n_sub"] = np.zeros(G, np.uint32); st["n_sub"][[0, 65]] = (2, 1)
    st["exec"] = [(0, 0, int(length[0, 0]) - 1), (0, 1, 0), (65, 0, int(length[0, 65]) - 2)]
    img = write_image(cfg, st)
    rep = mk_reps(G, R, W, K, only=[me])[0]
    snap = EPaxosSnapshot(rep).import_(img)
    assert snap.export() == img
    info = snap.info()
    assert info["n_exec"] == 3 and info["n_cells"] == int(live.sum()) and info["window"] == W and info["me"] == me
    rep.load_state(snap)
    d, xd = rep.dump(), rep.exec_dump()
    for f in ("len", "commit_bars", "bal", "seq", "status", "key", "deps", "pa_acks", "acc_acks", "bk", "highest_cols"):
        assert np.array_equal(d[f], st[f]), f
    assert np.array_equal(d["counters"], st["counters"][:3])
    for f in ("exec_bars", "kv", "digest"):
        assert np.array_equal(xd[f], st[f]), f
    g, r, c = rep.exec_poll()
    assert list(zip(g.tolist(), r.tolist(), c.tolist())) == st["exec"]
    assert rep.save_state().export() == write_image(cfg, dict(st, n_sub=np.zeros(G, np.uint32), exec=[]))   # the poll consumed the list, nothing else moved
    return img, cfg, st


# ---- 6. restart of one replica ------------------------------------------------------------------------------------------------
class Mute:
    """the seat of a replica that is down: proposes nothing, takes no message, answers nothing"""

    def __init__(self, G, R, W, K):
        self.G, self.R, self.W, self.n_keys = G, R, W, K

    def _z(self, **kw):
        G, R = self.G, self.R
        mk = dict(u8=lambda: np.zeros(G, np.uint8), u32=lambda: np.zeros(G, np.uint32), u64=lambda: np.zeros(G, np.uint64),
                  deps=lambda: np.full((R, G), N, np.uint32))
        return {k: mk[v]() for k, v in kw.items()}

    def propose(self, key, exploded=None):
        assert (key == NO_KEY).all()
        return self._z(flags="u8", col="u32", seq="u64", deps="deps")

    def handle_pre_accept(self, *a, **k):
        return self._z(flags="u8", ballot="u64", seq="u64", deps="deps")

    def handle_accept(self, *a, **k):
        return self._z(flags="u8", ballot="u64")

    def handle_commit_notice(self, *a, **k):
        return None

    def handle_pre_accept_replies(self, *a, **k):
        return self._z(decision="u8", seq="u64", deps="deps")

    def handle_accept_replies(self, *a, **k):
        return self._z(committed="u8")


def restart_of_one_replica(dev, oracle, G=65, R=5, W=8, K=3, seed=9):
    """one replica of five is saved and destroyed; the others take two ticks without it (in the oracle cluster its seat is as
    mute for those ticks); a new replica object is created, loaded, and joins"""
    orc = mk_oracle(oracle, G, R, W, K)
    reps = mk_reps(G, R, W, K)
    polls = [[] for _ in range(R)]
    eng = [LazyEngine(e, dev, polls[r]) for r, e in enumerate(reps)]
    rng = np.random.default_rng(seed)
    who, t0, snap = 2, 6, None
    for t in range(t0 + 2 + W + 2):
        keys, drop = schedule(rng, t, R, G, K, loss=0.1)
        keys = ec.silent_rows(keys, t, who, t0, 2)
        if t == t0:
            eng[who].flush()
            snap = reps[who].save_state()
            reps[who].close()
            reps[who] = None
            eng[who] = Mute(G, R, W, K)
        if t == t0 + 2:
            reps[who] = mk_reps(G, R, W, K, only=[who])[0]
            reps[who].load_state(snap)
            eng[who] = LazyEngine(reps[who], dev, polls[who])
        down = t0 <= t < t0 + 2
        oo = ec.tick([Mute(G, R, W, K) if (down and r == who) else orc[r] for r in range(R)], keys, drop)
        oe = ec.tick(eng, keys, drop)
        for s in range(R):
            same(oo[s], oe[s], "tick %d, leader %d" % (t, s))
    for r in range(R):
        same(orc[r].dump(), eng[r].dump(), "final dump of replica %d" % r)
        same(orc[r].exec_dump(), eng[r].exec_dump(), "final exec_dump of replica %d" % r)
        _subs_equal(orc[r].take_submissions(), eng[r].take_submissions(), "the submissions of replica %d" % r)


# ---- 7. stream order ----------------------------------------------------------------------------------------------------------
def stream_order(dev, oracle, G=130, R=3, W=8, K=3, seed=4):
    """a save enqueued right behind a handler launch, no synchronisation, more calls behind it: the image is the state between"""
    import torch
    orc = mk_oracle(oracle, G, R, W, K)
    reps = mk_reps(G, R, W, K)
    eng = [ec.NumpyEngine(e, dev) for e in reps]
    rng = np.random.default_rng(seed)
    for t in range(W + 2):
        keys, drop = schedule(rng, t, R, G, K, loss=0.1)
        ec.tick(eng, keys, drop); ec.tick(orc, keys, drop)
    from summerset_amd import EPaxosSnapshot
    snap = EPaxosSnapshot(reps[0])
    k1 = torch.from_numpy(ec.same_key(rng, 1, G, K)[0]).to(dev)
    k2 = torch.from_numpy(ec.same_key(rng, 1, G, K)[0]).to(dev)
    reps[0].handle_req_batch(k1)                                 # enqueued ...
    reps[0].save_state(snap)                                     # ... the save behind it ...
    reps[0].handle_req_batch(k2)                                 # ... and more behind the save
    orc[0].propose(k1.cpu().numpy())
    im = read_image(snap.export())
    image_vs_dumps(im, orc[0].dump(), orc[0].exec_dump(), None, "the image between two proposals")
    orc[0].propose(k2.cpu().numpy())
    same(orc[0].dump(), reps[0].dump(), "after the second proposal")


# ---- 8. refusals --------------------------------------------------------------------------------------------------------------
def refusals(dev, oracle, G=65, R=3, W=8, K=3):
    from summerset_amd import EPaxosReplicaGroup, EPaxosSnapshot, _lib
    L = _lib.load()
    base = dict(n_groups=G, population=R, me=0, window=W, n_keys=K, optimized_quorum=True, execute=True, recovery=False)
    mk = lambda **kw: EPaxosReplicaGroup(**dict(base, **kw))
    rep = mk()
    eng = ec.NumpyEngine(rep, dev)
    rng = np.random.default_rng(1)
    for t in range(3):
        eng.propose(ec.same_key(rng, 1, G, K)[0])
    good = rep.save_state()
    img = good.export()
    before = (rep.dump(), rep.exec_dump())

    def refused(call, code=None):
        rc = call()
        assert rc < 0 and (code is None or rc == code), rc
        assert L.smr_last_error(), "smr_last_error() is empty"
        same(before[0], rep.dump(), "a refused call changed the replica")
        same(before[1], rep.exec_dump(), "a refused call changed the replica")
        assert good.export() == img, "a refused call changed the snapshot"
        return rc

    one = lambda x: (C.c_void_p * 1)(x._h)
    code = refused(lambda: L.smr_ep_save_state(None, good._h, None))
    refused(lambda: L.smr_ep_save_state(rep._h, None, None), code)
    refused(lambda: L.smr_ep_load_state(None, good._h, None), code)
    refused(lambda: L.smr_ep_load_state(rep._h, None, None), code)
    refused(lambda: L.smr_ep_snapshot_create(None, C.byref(C.c_void_p())), code)
    refused(lambda: L.smr_ep_snapshot_info_get(good._h, None), code)
    refused(lambda: L.smr_ep_snapshot_import(good._h, None, 10), code)
    refused(lambda: int(L.smr_ep_snapshot_export(good._h, None, 10)), code)
    refused(lambda: L.smr_ep_cluster_save_state(1, None, one(good), None), code)
    # a replica that differs in one configuration field, both ways
    for kw in (dict(n_groups=G + 1), dict(population=R + 1), dict(me=1), dict(optimized_quorum=False), dict(execute=False),
               dict(recovery=True), dict(n_keys=K + 1), dict(window=2 * W)):
        other = mk(**kw)
        if "window" not in kw:                                   # (a larger window only makes the snapshot grow: case 9)
            refused(lambda: L.smr_ep_save_state(other._h, good._h, None), code)
        refused(lambda: L.smr_ep_load_state(other._h, good._h, None), code)
        theirs = other.save_state()
        refused(lambda: L.smr_ep_load_state(rep._h, theirs._h, None), code)
        if "window" not in kw:
            refused(lambda: L.smr_ep_snapshot_import(theirs._h, img, len(img)), code)
    # listed twice, n = 0, n = 9
    rep1 = mk(me=1)
    s1 = EPaxosSnapshot(rep1)
    two = lambda a, b: (C.c_void_p * 2)(a._h, b._h)
    refused(lambda: L.smr_ep_cluster_save_state(2, two(rep, rep), two(good, s1), None), code)
    refused(lambda: L.smr_ep_cluster_save_state(2, two(rep, rep1), two(good, good), None), code)
    refused(lambda: L.smr_ep_cluster_save_state(0, one(rep), one(good), None), code)
    nine = (C.c_void_p * 9)(*[rep._h] * 9)
    refused(lambda: L.smr_ep_cluster_save_state(9, nine, (C.c_void_p * 9)(*[good._h] * 9), None), code)
    # malformed images
    h = np.frombuffer(img, np.uint8)[:64].view(HDR)[0]
    im = read_image(img)

    def patched(off, val, dt="<u4"):
        b = bytearray(img)
        b[off:off + np.dtype(dt).itemsize] = np.array([val], dt).tobytes()
        return bytes(b)
    o_len = 64 + 8 * 15
    o_rew = o_len + 2 * a8(4 * R * G)
    fixed = len(img) - 64 * int(h["n_cells"]) - reply_dtype(R, 0).itemsize * int(h["n_replies"]) - 8 * int(h["n_exec"])
    target = EPaxosSnapshot(rep)
    bad = [("truncated", img[:-8]), ("shorter than its header", img[:40]), ("magic", patched(0, MAGIC + 1)), ("version", patched(4, 2)),
           ("reserved", patched(25, 1, "u1")), ("padding", patched(o_rew + G, 1, "u1")), ("count past capacity", patched(40, 1 << 40, "<u8")),
           ("live spans", patched(o_len, int(im["len"][0, 0]) + 1)), ("status = 6", patched(fixed + 56, 6, "u1")),
           ("key = n_keys", patched(fixed + 57, K, "u1")), ("n_replies", patched(60, int(h["n_replies"]) + 1)),
           ("window", patched(28, 12)), ("bytes", patched(8, len(img) + 8, "<u8"))]
    for what, b in bad:
        rc = L.smr_ep_snapshot_import(target._h, b, len(b))
        assert rc == code and L.smr_last_error(), what
        assert L.smr_ep_load_state(rep._h, target._h, None) < 0, what      # nothing was taken: the snapshot is still empty
    empty = EPaxosSnapshot(rep)
    rc = refused(lambda: L.smr_ep_load_state(rep._h, empty._h, None))
    assert rc != code                                            # SMR_ERR_STATE
    assert L.smr_ep_snapshot_info_get(empty._h, C.byref(_lib.EpSnapshotInfo())) == rc
    buf = (C.c_uint8 * len(img))()
    refused(lambda: int(L.smr_ep_snapshot_export(good._h, buf, len(img) - 1)), code)
    assert target.import_(img).export() == img                   # and the good image still goes in


# ---- 9. growth ----------------------------------------------------------------------------------------------------------------
def grows_for_a_larger_window(dev, oracle, G=65, R=3, K=3):
    """a snapshot made for window 8 takes a window-64 replica with full rows"""
    from summerset_amd import EPaxosSnapshot
    small = mk_reps(G, R, 8, K, only=[0])[0]
    snap = EPaxosSnapshot(small)
    W = 64
    orc = mk_oracle(oracle, G, R, W, K)
    reps = mk_reps(G, R, W, K)
    eng = [ec.NumpyEngine(e, dev) for e in reps]
    rng = np.random.default_rng(8)
    for t in range(W + 3):
        keys = ec.same_key(rng, R, G, K)
        ec.tick(eng, keys); ec.tick(orc, keys)
    reps[0].save_state(snap)
    im = read_image(snap.export())
    assert int(im["hdr"]["max_live"]) == W and int(im["hdr"]["window"]) == W
    image_vs_dumps(im, orc[0].dump(), orc[0].exec_dump(), None, "window 64")
    fresh = mk_reps(G, R, W, K, only=[0])[0]
    fresh.load_state(snap)
    same(orc[0].dump(), fresh.dump(), "loaded")
    same(orc[0].exec_dump(), fresh.exec_dump(), "loaded")


# ---- 11. device only ----------------------------------------------------------------------------------------------------------
def two_sets_large(dev, G=66000, R=3, W=8, K=2, T=4, seed=6):
    """more tiles than wavefronts: save, load into a second set; the existing dumps are the yardstick"""
    import torch
    from summerset_amd import epaxos
    from summerset_amd.ep_cluster import EPaxosCluster
    a, b = mk_reps(G, R, W, K), mk_reps(G, R, W, K)
    cl = EPaxosCluster(a)
    rng = np.random.default_rng(seed)
    for t in range(T):
        keys, drop = schedule(rng, t, R, G, K)
        cl.tick([torch.from_numpy(np.ascontiguousarray(keys[r])).to(dev) for r in range(R)], {k: torch.from_numpy(v).to(dev) for k, v in drop.items()})
    snaps = epaxos.save_cluster_state(a)
    epaxos.load_cluster_state(b, snaps)
    for r in range(R):
        da, db = all_dumps(a[r]), all_dumps(b[r])
        same(da[0], db[0], "dump of replica %d" % r)
        same(da[1], db[1], "exec_dump of replica %d" % r)
        image_vs_dumps(read_image(snaps[r].export()), da[0], da[1], None, "replica %d" % r)
        pa, pb = a[r].exec_poll(), b[r].exec_poll()
        _subs_equal(pa, pb, "the unpolled submissions of replica %d" % r)
    cl.close()


# ---- 10. the way back from an aborted L2 tick ---------------------------------------------------------------------------------
def abort_and_restore_l2(dev, oracle, world, R=5, W=8, K=3, T=10, abort_at=(3, 6), seed=13):
    """the in-process spread job (summerset_amd/spread_ep.py, the library's segments): at the ticks of `abort_at` every replica
    is saved, the first three segments of the tick run (with their exchanges), the tick is aborted -- the replicas are half
    updated -- the replicas are loaded back and the whole tick runs; outputs and dumps are the oracle cluster's"""
    import torch
    from summerset_amd import _lib, spread_ep
    G = 65 * world
    job = spread_ep.in_process(G, R, world, dev, window=W, n_keys=K, execute=True)
    for rk in job.ranks:
        rk.use_library_tick()
    orc = mk_oracle(oracle, G, R, W, K)
    L = _lib.load()
    rng = np.random.default_rng(seed)
    t_ = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    where = {(b, r): rk for rk in job.ranks for (b, r) in rk.reps}
    try:
        for t in range(T):
            keys, drop = schedule(rng, t, R, G, K)
            jk = {(b, r): t_(keys[r, rk.range[b][0]:rk.range[b][1]]) for (b, r), rk in where.items()}
            jd = {(b, s, q): t_(m[rk.range[b][0]:rk.range[b][1]]) for (s, q), m in (drop or {}).items() for (b, r), rk in where.items() if r == s}
            if t in abort_at:
                snaps = {k: rk.reps[k].save_state() for k, rk in where.items()}
                before = {k: rk.reps[k].dump() for k, rk in where.items()}
                gens = [rk._lib_steps(jk, jd) for rk in job.ranks]
                for seg in range(3):
                    plans = [next(g) for g in gens]
                    for s_, p in enumerate(plans):               # (the exchange, as in_process.tick moves it)
                        so = 0
                        for d, n in enumerate(p["in_split"]):
                            q = plans[d]
                            ro = sum(q["out_split"][:s_])
                            if n:
                                q["rbuf"][ro:ro + n].copy_(p["sbuf"][so:so + n])
                            so += n
                for g in gens:
                    g.close()
                moved = any(not np.array_equal(before[k]["len"], rk.reps[k].dump()["len"]) for k, rk in where.items())
                assert moved, "three segments left every replica as it was"
                for rk in job.ranks:
                    _lib.check(L.smr_ep_spread_abort_tick(rk._lib_h))
                for k, rk in where.items():
                    rk.reps[k].load_state(snaps[k])
                    same(before[k], rk.reps[k].dump(), "replica %s after abort and load" % (k,))
            out = job.tick(jk, jd)
            oo = ec.tick(orc, keys, drop)
            for (b, s), rk in where.items():
                lo, hi = rk.range[b]
                for f, v in out[(b, s)].items():
                    got = v.cpu().numpy()
                    got = got.view({"int32": np.uint32, "int64": np.uint64}.get(str(got.dtype), got.dtype))
                    assert np.array_equal(got, oo[s][f][..., lo:hi]), "tick %d, block %d, leader %d: %s" % (t, b, s, f)
        for (b, r), rk in where.items():
            lo, hi = rk.range[b]
            d, x = rk.reps[(b, r)].dump(), orc[r].dump()
            for f in d:
                if f == "counters":
                    continue
                want = x[f][:, :, lo:hi] if f == "deps" else x[f][..., lo:hi]
                assert np.array_equal(d[f], want), "block %d replica %d: %s" % (b, r, f)
            xd, xx = rk.reps[(b, r)].exec_dump(), orc[r].exec_dump()
            for f in ("exec_bars", "kv", "digest"):
                assert np.array_equal(xd[f], xx[f][..., lo:hi]), "block %d replica %d: %s" % (b, r, f)
    finally:
        for rk in job.ranks:
            rk.close_library_tick()
