"""Save / load of a MultiPaxos cluster's state (smr_mp_save_state / smr_mp_load_state): the bodies of
tests/test_mp_snapshot.py (emulator, dev = "cpu") and tests/test_zzzz_mp_snapshot_gpu.py (device).  Every comparison is
against the CPU oracle, which cannot load a state but keeps running: a cluster loaded from a snapshot taken after tick t
must agree with it after tick t + 1, t + 2, ...  The one exception is the canonical-bytes test, which compares two engines'
images with each other (and one of them with the oracle)."""
import numpy as np

from test_mp_gpu import _compare, _to_dev


def _same_commits(og, os_, eg, es, what):
    """ordered committed-slot lists: a group's entries in commit order, the order across groups unspecified"""
    assert len(og) == len(eg), "%s: commit count %d vs oracle %d" % (what, len(eg), len(og))
    ko = np.lexsort((np.arange(len(og)), og))
    ke = np.argsort(eg, kind="stable")
    assert np.array_equal(og[ko], eg[ke]) and np.array_equal(os_[ko], es[ke]), what


def _rows(inp, cap):
    """a tick's inputs for an oracle whose outbox holds `cap` entries: the first `cap` rows of a longer reply-order array (an
    engine reads ackctl[j][g] for its own entries j only; the oracle checks the shape)"""
    return dict(inp, ackctl=np.ascontiguousarray(inp["ackctl"][:cap]))


def _bootstrap(eng_list, orc, G, cap, dev):
    """natural bootstrap (no preset leader): replica 0 times out first and commits the no-op slot"""
    from summerset_amd import stream
    t0 = dict(timeout_rep=np.zeros(G, np.uint8), timeout_src=np.full(G, 0xFF, np.uint8),
              ackctl=np.full((cap, G), stream.CTL_IDENTITY, np.uint32), heartbeat=False)
    orc.tick(**t0)
    for e in eng_list:
        e.tick(**_to_dev(t0, dev))


def shadow_at_every_boundary(dev, oracle, G, R, S, W, n_ticks, drop_p, timeout_frac, hb_every, preset=True, commit_extra=0,
                             straggler_ticks=0, seed=None, expect_outbox=None, expect_wrapped=False):
    """A runs the stream against the oracle; after EVERY tick t it is saved (with that tick's commits still unpolled) and a
    FRESH cluster B is loaded from the snapshot: B's dump is the oracle's.  Tick t + 1 then runs on both, both equal the
    oracle in state and in the ordered commit lists (B's: the carried entries of tick t, then tick t + 1's), and in counters."""
    from summerset_amd import MultiPaxosCluster, stream
    cap = W + 4
    kw = dict(outbox_cap=cap, commit_extra=commit_extra, commit_list_cap=G * (S * 8 + 2 * W) + 64)
    A = MultiPaxosCluster(G, R, W, straggler_ticks=straggler_ticks, **kw)
    orc = oracle.MpOracle(G, R, W, cap=cap, commit_extra=commit_extra)
    if preset:
        A.preset_leader(0)
        orc.preset_leader(0)
    else:
        _bootstrap([A], orc, G, cap, dev)
        _compare(A, orc, R, -1)
        for r in range(R):
            _same_commits(*orc.take_commits(r), *A.poll_commits(r), "bootstrap rep %d" % r)
    st = stream.MultiPaxosStream(G, R, S, cap=cap, n_ticks=n_ticks, drop_p=drop_p, timeout_frac=timeout_frac, hb_every=hb_every,
                                 seed=seed or stream.DEFAULT_SEED)
    B, snap, prev = None, None, None
    saw_outbox = saw_wrapped = False
    total = 0
    for t in range(n_ticks):
        inp = st.tick(t)
        d = _to_dev(inp, dev)
        orc.tick(**inp)
        A.tick(**d)
        _compare(A, orc, R, t)
        now = [orc.take_commits(r) for r in range(R)]
        if B is not None:                                         # the cluster loaded after tick t - 1 has run tick t
            B.tick(**d)
            _compare(B, orc, R, t)
            for r in range(R):
                og, os_ = np.concatenate([prev[r][0], now[r][0]]), np.concatenate([prev[r][1], now[r][1]])
                _same_commits(og, os_, *B.poll_commits(r), "loaded at %d, tick %d rep %d" % (t - 1, t, r))
                assert B.counters(r) == A.counters(r) and B.counters(r)["commits"] == orc.total_commits(r), (t, r)
            B.close()
        snap = A.save_state(snap)                                 # tick t's commits are still on A's list: they travel
        info = snap.info()
        assert info["n_groups"] == G and info["population"] == R and info["commit_extra"] == commit_extra and info["live_mask"] == (1 << R) - 1
        d0 = orc.dump(0)
        spans = np.stack([orc.dump(r)["log_len"] - orc.dump(r)["start_slot"] for r in range(R)])
        assert info["n_slots"] == int(spans.sum()) and info["max_live"] == int(spans.max()), (t, info)
        saw_outbox = saw_outbox or info["n_outbox"] > 0
        saw_wrapped = saw_wrapped or bool(d0["overflow"].any()) or bool((d0["start_slot"] > W).any())
        for r in range(R):
            _same_commits(*now[r], *A.poll_commits(r), "tick %d rep %d" % (t, r))
            total += len(now[r][0])
        B = MultiPaxosCluster(G, R, W, straggler_ticks=straggler_ticks, **kw)
        B.load_state(snap)
        _compare(B, orc, R, t)
        prev = now
    for r in range(R):
        assert A.counters(r)["commits"] == orc.total_commits(r)
    assert total > 0
    if expect_outbox if expect_outbox is not None else timeout_frac > 0:
        assert saw_outbox, "no snapshot carried a pending outbox (the Accepts a prepare quorum leaves for the next tick)"
    if expect_wrapped:
        assert saw_wrapped, "no snapshot of a wrapped ring / frozen group"
    return A, orc


def _drive(eng, inputs, how, dev):
    """a list of consecutive ticks' inputs through `eng`: "tick" one call each, "rounds" the four rounds as separate calls,
    an int n: smr_mp_run_ticks in batches of n"""
    if isinstance(how, int):
        for i in range(0, len(inputs), how):
            eng.run_ticks([_to_dev(x, dev) for x in inputs[i:i + how]])
        return
    for inp in inputs:
        d = _to_dev(inp, dev)
        if how == "rounds":
            eng.round_local(d["timeout_rep"], d["timeout_src"], d["req_target"], d["req_cnt"], d["req_val"])
            eng.round_deliver()
            eng.round_replies(d["ackctl"], publish_heartbeat=inp["heartbeat"])
            if inp["heartbeat"]:
                eng.round_heartbeat()
            eng.end_tick()
        else:
            eng.tick(**d)


def canonical_bytes(dev, oracle, a, b, G=130, R=5, S=2, n_ticks=24, every=8, resume=False):
    """two clusters that differ in `a` / `b` (dicts: W, straggler_ticks, rotate, how) run the same stream; after every
    `every` ticks their exported images are equal as bytes (commit lists unpolled: they are part of the image), and the
    first one's state is the oracle's.  resume: the last image, through from_bytes into a fresh cluster, goes on in step
    with the oracle"""
    from summerset_amd import MpSnapshot, MultiPaxosCluster, stream
    Wmax = max(a.get("W", 64), b.get("W", 64))
    Wmin = min(a.get("W", 64), b.get("W", 64))
    cap = Wmax + 4                                                # one ackctl array for both: [cap][G], a smaller outbox reads its first rows
    clist = G * S * (n_ticks + 8) + G * Wmax + 64

    def make(o):
        W = o.get("W", 64)
        e = MultiPaxosCluster(G, R, W, outbox_cap=W + 4, commit_list_cap=clist, straggler_ticks=o.get("straggler_ticks", 0))
        if o.get("rotate"):
            e.set_role_rotation(True)
        e.preset_leader(0)
        return e
    A, B = make(a), make(b)
    orc = oracle.MpOracle(G, R, Wmin, cap=Wmin + 4)
    orc.preset_leader(0)
    st = stream.MultiPaxosStream(G, R, S, cap=cap, n_ticks=n_ticks + 8, drop_p=0.1, timeout_frac=1.0, hb_every=4)
    sa = sb = None
    img = None
    saw_outbox = False
    for t0 in range(0, n_ticks, every):
        ins = [st.tick(t) for t in range(t0, t0 + every)]
        for x in ins:
            orc.tick(**_rows(x, Wmin + 4))
        _drive(A, ins, a.get("how", "tick"), dev)
        _drive(B, ins, b.get("how", "tick"), dev)
        for e, w in ((A, a), (B, b)):
            # (the oracle has the smaller window: compare where the rings have the same shape, scalars otherwise)
            if w.get("W", 64) == Wmin:
                _compare(e, orc, R, t0 + every - 1)
            assert not any(e.counters(r)["rejects"] for r in range(R)) and not e.dump(0)["overflow"].any()
        sa, sb = A.save_state(sa), B.save_state(sb)
        img, imb = sa.export(), sb.export()
        assert len(img) == sa.info()["bytes"] == sb.info()["bytes"]
        if img != imb:
            x, y = np.frombuffer(img, np.uint8), np.frombuffer(imb, np.uint8)
            raise AssertionError("after tick %d the images differ, first at byte %d of %d" % (t0 + every - 1, int(np.nonzero(x != y)[0][0]), len(img)))
        saw_outbox = saw_outbox or sa.info()["n_outbox"] > 0
        assert MpSnapshot.from_bytes(img, A).export() == img      # import, export: the same bytes
    assert sum(orc.total_commits(r) for r in range(R)) > 0
    if resume:
        Wc = a.get("W", 64)
        assert Wc == Wmin
        C_ = MultiPaxosCluster(G, R, Wc, outbox_cap=Wc + 4, commit_list_cap=clist)
        C_.load_state(MpSnapshot.from_bytes(img, C_))
        _compare(C_, orc, R, n_ticks - 1)
        for t in range(n_ticks, n_ticks + 8):
            x = st.tick(t)
            orc.tick(**_rows(x, Wmin + 4))
            C_.tick(**_to_dev(x, dev))
            _compare(C_, orc, R, t)
        for r in range(R):
            assert C_.counters(r)["commits"] == orc.total_commits(r)
    return saw_outbox


def resize(dev, oracle, G=96, R=5, S=2, W0=16, W1=64, n_before=7, n_after=24):
    """a W0 cluster runs to live spans near its ring with nothing refused or frozen; its snapshot goes into a W1 cluster with a
    larger outbox, which continues.  From such a clean history an oracle that had the larger window and capacity all along is
    in the same state: the loaded cluster equals it from the load on, while the small oracle starts refusing batches"""
    from summerset_amd import MultiPaxosCluster, stream
    cap0, cap1 = W0 + 4, W1 + 4
    # win_reserve = 0 on the small ring: its back-pressure starts at a full ring, not a quarter short of it
    small = MultiPaxosCluster(G, R, W0, win_reserve=0, outbox_cap=cap0)
    o_small = oracle.MpOracle(G, R, W0, win_reserve=0, cap=cap0)
    o_big = oracle.MpOracle(G, R, W1, win_reserve=0, cap=cap1)
    for x in (small, o_small, o_big):
        x.preset_leader(0)
    st = stream.MultiPaxosStream(G, R, S, cap=cap1, n_ticks=n_before + n_after, drop_p=0.1, timeout_frac=0.0, hb_every=12)
    for t in range(n_before):
        inp = st.tick(t)
        o_small.tick(**_rows(inp, cap0)); o_big.tick(**inp)
        small.tick(**_to_dev(inp, dev))
        _compare(small, o_small, R, t)
    d = o_small.dump(0)
    span = int((d["log_len"] - d["start_slot"]).max())
    assert span >= W0 - 2 * S, "the stream leaves the small ring far from full (%d of %d)" % (span, W0)
    assert not any(small.counters(r)["rejects"] for r in range(R)) and not d["overflow"].any(), "the history is not clean"
    for n in ("leader", "bal_max_seen", "start_slot", "log_len", "accept_bar", "commit_bar", "exec_bar", "snap_bar"):
        for r in range(R):
            assert np.array_equal(o_small.dump(r)[n], o_big.dump(r)[n]), n   # the two oracles agree up to here
    snap = small.save_state()
    assert snap.info()["max_live"] == span
    big = MultiPaxosCluster(G, R, W1, win_reserve=0, outbox_cap=cap1)
    big.load_state(snap)
    _compare(big, o_big, R, n_before - 1)
    for t in range(n_before, n_before + n_after):
        inp = st.tick(t)
        o_small.tick(**_rows(inp, cap0)); o_big.tick(**inp)
        big.tick(**_to_dev(inp, dev))
        _compare(big, o_big, R, t)
    assert o_small.dump(0)["overflow"].any() or o_small.dump(0)["log_len"].sum() < o_big.dump(0)["log_len"].sum(), \
        "the small ring never got in the way: the resize showed nothing"
    for r in range(R):
        assert big.counters(r)["commits"] == o_big.total_commits(r)   # the counters travelled with the state
    assert not o_big.dump(0)["overflow"].any() and not any(big.counters(r)["rejects"] for r in range(R))


def under_the_fused_path(dev, oracle, G=130, S=3, W=64, n_ticks=72, drop_p=0.3):
    """the shape of test_mp_gpu.run_rest_rides_in_next_r1 (straggler list on, a long quiet stretch: the rest of a tick's R3
    rides in the next tick's R1 launch INSIDE a batch): a save after every batch, the loaded cluster and the original both run
    the next batch and match the oracle.  What this does NOT reach: save's "complete a deferred rest first" branch --
    smr_mp_run_ticks never defers the rest of a batch's last tick, so no batch end has one pending (`deferred` counts the
    batches in which a deferral inside the batch was possible, i.e. that ran mp_rest_then_local)"""
    from summerset_amd import MultiPaxosCluster, stream
    R, H, cap = 5, 4, W + 4
    kw = dict(win_reserve=W // 8, outbox_cap=cap, straggler_ticks=4)
    A = MultiPaxosCluster(G, R, W, **kw)
    orc = oracle.MpOracle(G, R, W, win_reserve=W // 8, cap=cap, record_commits=False)
    A.preset_leader(0); orc.preset_leader(0)
    st = stream.MultiPaxosStream(G, R, S, cap=cap, n_ticks=n_ticks, drop_p=drop_p, timeout_frac=0.3, hb_every=H, timeout_span=5)
    B, snap, batch, deferred = None, None, [], 0
    for t in range(n_ticks):
        inp = st.tick(t)
        orc.tick(**inp)
        if not (inp["timeout_rep"] != 0xFF).any():
            inp["timeout_rep"] = inp["timeout_src"] = None
        batch.append(_to_dev(inp, dev))
        if len(batch) == 8 or t == n_ticks - 1:
            A.run_ticks(batch)
            _compare(A, orc, R, t)
            if B is not None:
                B.run_ticks(batch)
                _compare(B, orc, R, t)
                for r in range(R):
                    assert B.counters(r) == A.counters(r)
                B.close()
            batch = []
            deferred += t >= 5 + 2 * 16 + 4
            snap = A.save_state(snap)
            B = MultiPaxosCluster(G, R, W, **kw)
            B.load_state(snap)
            _compare(B, orc, R, t)
    assert deferred >= 3
    for r in range(R):
        assert A.counters(r)["commits"] == orc.total_commits(r)


def abort_and_restore_l2(dev, oracle, world, G=None, R=5, S=2, W=64, n_ticks=16, abort_at=(3, 6)):
    """the in-process spread job of tests/test_spread_mp.py: at the ticks of `abort_at` every rank's blocks are saved, segments
    0 and 1 of the tick run (with their collectives), the tick is aborted, the blocks are loaded back and the whole tick runs;
    the live replicas' state is the co-located oracle's after that tick and for the >= 8 ticks that follow"""
    from oracle.oracle import MP_SCALARS, MP_SLOTS
    from summerset_amd import SummersetError, _lib, shard, spread_mp, stream
    G = 64 * world * 2 if G is None else G
    cap = W + 4
    job = spread_mp.in_process(G, R, W, world, dev, S, outbox_cap=cap)
    job.preset_leader(0)
    orc = oracle.MpOracle(G, R, W, cap=cap)
    orc.preset_leader(0)
    kw = dict(cap=cap, n_ticks=n_ticks, drop_p=0.1, timeout_frac=1.0, hb_every=3)
    st = stream.MultiPaxosStream(G, R, S, **kw)
    bst = {b: stream.MultiPaxosStream(hi - lo, R, S, group_base=lo, **kw) for b, (lo, hi) in
           ((b, shard.group_range(G, world, b)) for b in range(world)) if hi > lo}
    snaps = None
    assert n_ticks - max(abort_at) - 1 >= 8
    for t in range(n_ticks):
        inp = st.tick(t)
        orc.tick(**inp)
        ins = {b: _to_dev({k: v for k, v in s_.tick(t).items() if k != "heartbeat"}, dev) for b, s_ in bst.items()}
        if t in abort_at:
            snaps = job.save_state(snaps)
            arrs = [r._inputs(ins) for r in job.ranks]
            for k, phase in ((0, "outbox"), (1, "replies")):
                for r, a in zip(job.ranks, arrs):
                    r.segment(k, a, inp["heartbeat"])
                for r in job.ranks:                               # every rank ARRIVES at the collective (the call counts them); the
                    spread_mp._copy_between(job.ranks, phase)     # copy itself runs once, when the last one has -- as in_process.tick
            try:                                                  # the tick is open: neither call is defined here
                job.save_state()
                raise AssertionError("save inside an open spread tick went through")
            except SummersetError as e:
                assert e.code == _lib.SMR_ERR_STATE, e
            try:
                job.load_state(snaps)
                raise AssertionError("load inside an open spread tick went through")
            except SummersetError as e:
                assert e.code == _lib.SMR_ERR_STATE, e
            job.abort_tick()
            job.load_state(snaps)
        job.tick(ins, heartbeat=inp["heartbeat"])
        for rk in job.ranks:
            for b, (cl, live, lo, hi) in rk.blocks.items():
                for r in live:
                    a, x = cl.dump(r), orc.dump(r)
                    assert not a["overflow"].any() and not x["overflow"][lo:hi].any()
                    for name in list(MP_SCALARS) + ["peer_exec_bar"] + [n for n, _ in MP_SLOTS]:
                        assert np.array_equal(a[name], x[name][..., lo:hi]), "tick %d rank %d block %d replica %d: %s differs" % (t, rk.rank, b, r, name)
    total = sum(rk.commits() for rk in job.ranks)
    assert total == sum(orc.total_commits(r) for r in range(R)) and total > 0


def refusals(dev, oracle):
    """every call that must be refused is, with SMR_ERR_ARG / SMR_ERR_STATE and a message, and a refused load leaves the
    cluster's dump as it was"""
    import ctypes as C
    import struct

    import pytest
    from summerset_amd import MpSnapshot, MultiPaxosCluster, SummersetError, _lib, stream
    L = _lib.load()
    G, R, S, W = 70, 5, 4, 32
    cap = W + 4

    def refused(code, fn, *a):
        with pytest.raises(SummersetError) as e:
            fn(*a)
        assert e.value.code == code and len(e.value.msg) > 8, e.value
        assert L.smr_last_error().decode() == e.value.msg

    def unchanged(eng, before):
        for r in range(eng.R):
            now = eng.dump(r)
            assert all(np.array_equal(now[k], before[r][k]) for k in now)

    src = MultiPaxosCluster(G, R, W, outbox_cap=cap, commit_list_cap=G * S * 16)
    orc = oracle.MpOracle(G, R, W, cap=cap)
    src.preset_leader(0); orc.preset_leader(0)
    st = stream.MultiPaxosStream(G, R, S, cap=cap, n_ticks=8, drop_p=0.1, timeout_frac=1.0, hb_every=4, timeout_span=4)
    snap, t_snap = None, None
    for t in range(8):                                            # a snapshot with a pending outbox and a log longer than 8 slots
        inp = st.tick(t)
        orc.tick(**inp)
        src.tick(**_to_dev(inp, dev))
        if t_snap is None:
            snap = src.save_state(snap)
            i = snap.info()
            if i["n_outbox"] > 0 and i["max_live"] > 8 and i["max_outbox"] > 4:
                t_snap = t
    assert t_snap is not None
    _compare(src, orc, R, 7)
    info = snap.info()
    assert info["n_outbox"] > 0 and info["max_live"] > 8 and info["max_outbox"] > 4, info
    img = snap.export()
    assert len(img) == info["bytes"]

    # null arguments
    h = C.c_void_p()
    for rc in (L.smr_mp_snapshot_create(None, C.byref(h)), L.smr_mp_snapshot_create(src._h, None), L.smr_mp_save_state(None, snap._h, None),
               L.smr_mp_save_state(src._h, None, None), L.smr_mp_load_state(None, snap._h, None), L.smr_mp_load_state(src._h, None, None),
               L.smr_mp_snapshot_info_get(None, C.byref(_lib.MpSnapshotInfo())), L.smr_mp_snapshot_info_get(snap._h, None),
               L.smr_mp_snapshot_export(None, (C.c_uint8 * 8)(), 8), L.smr_mp_snapshot_export(snap._h, None, 1 << 30),
               L.smr_mp_snapshot_import(None, img, len(img)), L.smr_mp_snapshot_import(snap._h, None, len(img))):
        assert rc == _lib.SMR_ERR_ARG and len(L.smr_last_error()) > 8
    assert L.smr_mp_snapshot_export(snap._h, (C.c_uint8 * 64)(), 64) == _lib.SMR_ERR_ARG       # too small
    L.smr_mp_snapshot_destroy(None)
    # an empty snapshot holds nothing to load
    refused(_lib.SMR_ERR_STATE, src.load_state, MpSnapshot(src))

    # a snapshot of another G, R, commit_extra or live mask
    others = [MultiPaxosCluster(G + 1, R, W, outbox_cap=cap, commit_list_cap=G * S * 16), MultiPaxosCluster(G, 3, W, outbox_cap=cap, commit_list_cap=G * S * 16),
              MultiPaxosCluster(G, R, W, outbox_cap=cap, commit_extra=1, commit_list_cap=G * S * 16), MultiPaxosCluster(G, R, W, outbox_cap=cap, commit_list_cap=G * S * 16)]
    _lib.check(L.smr_mp_set_live(others[3]._h, 0b00101))
    # a target whose window, outbox_cap or commit_list_cap is too small
    others += [MultiPaxosCluster(G, R, 8, outbox_cap=cap, commit_list_cap=G * S * 16),
               MultiPaxosCluster(G, R, W, outbox_cap=4, commit_list_cap=G * S * 16), MultiPaxosCluster(G, R, W, outbox_cap=cap, commit_list_cap=1)]
    assert info["max_live"] > 8
    for o in others:
        o.preset_leader(1)
        before = [o.dump(r) for r in range(o.R)]
        refused(_lib.SMR_ERR_ARG, o.load_state, snap)
        refused(_lib.SMR_ERR_ARG, o.save_state, snap) if o in others[:4] else None
        unchanged(o, before)
        if o in others[:4]:
            refused(_lib.SMR_ERR_ARG, MpSnapshot.from_bytes, img, o)

    # a tick opened round by round with the straggler list on (the library marks it) and not yet closed
    lst = MultiPaxosCluster(G, R, W, outbox_cap=cap, commit_list_cap=G * S * 16, straggler_ticks=2)
    lst.preset_leader(0)
    lsnap = lst.save_state()
    d = _to_dev(st.tick(0), dev)
    lst.round_local(d["timeout_rep"], d["timeout_src"], d["req_target"], d["req_cnt"], d["req_val"])
    refused(_lib.SMR_ERR_STATE, lst.save_state, lsnap)
    refused(_lib.SMR_ERR_STATE, lst.load_state, lsnap)
    lst.round_deliver()
    lst.round_replies(d["ackctl"], publish_heartbeat=False)
    lst.end_tick()
    lst.save_state(lsnap)
    orc1 = oracle.MpOracle(G, R, W, cap=cap)
    orc1.preset_leader(0)
    orc1.tick(**st.tick(0))
    lst.load_state(lsnap)
    _compare(lst, orc1, R, 0)

    # images: truncated, wrong magic or version, header maxima / counts that contradict the body, bad padding and records
    tgt = MultiPaxosCluster(G, R, W, outbox_cap=cap, commit_list_cap=G * S * 16)
    before = [tgt.dump(r) for r in range(R)]
    hdr = list(struct.unpack_from("<IIIBBBBQQQQIIII", img, 0))

    def with_hdr(i, v):
        x = list(hdr)
        x[i] = v
        return struct.pack("<IIIBBBBQQQQIIII", *x) + img[64:]
    bad = [img[:40], img[:64], img[:len(img) // 2], img[:-1], with_hdr(0, hdr[0] ^ 1), with_hdr(1, 2), with_hdr(1, 0),
           with_hdr(11, hdr[11] + 1), with_hdr(11, hdr[11] - 1), with_hdr(12, hdr[12] + 1), with_hdr(13, hdr[13] + 1),
           with_hdr(8, hdr[8] + 1), with_hdr(9, hdr[9] - 1), with_hdr(10, hdr[10] + 1), with_hdr(7, hdr[7] + 8), with_hdr(6, 1), with_hdr(14, 1)]
    body = bytearray(img)
    body[64 + G] = 1                                              # a padding byte of the overflow section (G = 70: padded to 72)
    bad.append(bytes(body))
    body = bytearray(img)
    body[len(img) - hdr[10] * 8 - hdr[9] * 24 - 56 + 48] = 9      # the status byte of the last slot record
    bad.append(bytes(body))
    body = bytearray(img)
    body[len(img) - hdr[10] * 8 - hdr[9] * 24 - 56 + 52] = R      # ... its source replica: ids stop at R - 1
    bad.append(bytes(body))
    L5 = 64 + 72 + 40 * R                                         # replica 0's scalars: commit_bar of group 0 beyond its log_len
    body = bytearray(img)
    body[L5 + 36 * G:L5 + 36 * G + 4] = struct.pack("<I", struct.unpack_from("<I", img, L5 + 28 * G)[0] + 1)
    bad.append(bytes(body))
    for k, x in enumerate(bad):
        refused(_lib.SMR_ERR_ARG, MpSnapshot.from_bytes, x, tgt)
    # ... and never past len: the image at the very end of a buffer whose next page is not there is the emulator's and the
    # sanitizers' business; here: a length that stops inside a section is refused whatever lies behind it
    for n in (63, 64 + G, len(img) - 56 * 3):
        assert L.smr_mp_snapshot_import(MpSnapshot(tgt)._h, img, n) == _lib.SMR_ERR_ARG
    unchanged(tgt, before)
    # the good image still loads, and runs on with the oracle from the tick it was taken at
    tgt.load_state(MpSnapshot.from_bytes(img, tgt))
    orc2 = oracle.MpOracle(G, R, W, cap=cap)
    orc2.preset_leader(0)
    for t in range(8):
        inp = st.tick(t)
        orc2.tick(**inp)
        if t > t_snap:
            tgt.tick(**_to_dev(inp, dev))
        if t >= t_snap:
            _compare(tgt, orc2, R, t)


def reuse_into_a_larger_cluster(dev, oracle, G=70, R=5, S=2, W0=16, W1=64, n_ticks=14):
    """a snapshot made on an EMPTY cluster with a small ring, then filled from a cluster with a larger ring and outbox whose
    logs have outgrown the first one's whole room: the save call itself makes the room (from the sizes the host knows), reports
    nothing to repeat, and what it kept is right -- checked only AFTER the source has moved on, as the abort-restore path
    does.  Room is always the worst case, so a snapshot made on a young cluster and reused by every save never runs out"""
    from summerset_amd import MpSnapshot, MultiPaxosCluster, stream
    cap = W1 + 4
    young = MultiPaxosCluster(G, R, W0, outbox_cap=W0 + 4)
    snap = MpSnapshot(young)                                      # room: G x R x W0 slots
    src = MultiPaxosCluster(G, R, W1, outbox_cap=cap)
    orc, at_save = oracle.MpOracle(G, R, W1, cap=cap), oracle.MpOracle(G, R, W1, cap=cap)
    for x in (src, orc, at_save):
        x.preset_leader(0)
    st = stream.MultiPaxosStream(G, R, S, cap=cap, n_ticks=n_ticks + 6, drop_p=0.1, timeout_frac=1.0, hb_every=16)
    for t in range(n_ticks):
        inp = st.tick(t)
        orc.tick(**inp); at_save.tick(**inp)
        src.tick(**_to_dev(inp, dev))
    need = sum(int((orc.dump(r)["log_len"] - orc.dump(r)["start_slot"]).sum()) for r in range(R))
    assert need > G * R * W0, "the logs never outgrew the first cluster's room (%d of %d)" % (need, G * R * W0)
    src.save_state(snap)                                          # no confirmation asked for: the source goes on at once
    for t in range(n_ticks, n_ticks + 3):
        inp = st.tick(t)
        orc.tick(**inp)
        src.tick(**_to_dev(inp, dev))
    _compare(src, orc, R, n_ticks + 2)
    assert snap.info()["n_slots"] == need
    src.load_state(snap)                                          # back to the boundary the save was taken at
    _compare(src, at_save, R, n_ticks - 1)
    for t in range(n_ticks, n_ticks + 6):
        inp = st.tick(t)
        at_save.tick(**inp)
        src.tick(**_to_dev(inp, dev))
        _compare(src, at_save, R, t)
