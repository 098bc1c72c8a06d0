"""smr_rsp_save_state / smr_rsp_load_state and their cluster forms: the bodies of tests/test_rsp_snapshot.py (the kernel-source
emulator) and tests/test_zzzz_rsp_snapshot_gpu.py (the device), every size an argument.

Everything is bit-exact and nothing is engine against engine alone: the engines run tests/rsp_edges.py's schedules against
`oracle.RspOracle` -- every message dict, `take_executed()` and the full `dump()` of every replica after every tick -- and what
a snapshot gave back is held against the same oracle dumps.  Every body first asserts ON THE ORACLE CLUSTER ALONE that its
schedule reached what it is for (`rsp_edges.reach` / `assert_reached_every_rare_path`, a wrapped ring).  The image is parsed and
built here from DESIGN.md 2's table alone (`Layout`)."""
import struct

import numpy as np

import rsp_cluster as rc
import rsp_edges as e
import rsp_scenarios as sc

NULL, NO_REP = rc.NULL, rc.NO_REP
MAGIC = 0x53505253                                                           # "SRPS"
SLOT = np.dtype([("bal", "<u8"), ("vbal", "<u8"), ("pmax", "<u8"), ("val", "<u4"), ("vval", "<u4"), ("ltrig", "<u4"), ("lendp", "<u4"),
                 ("rtrig", "<u4"), ("rendp", "<u4"), ("status", "u1"), ("mask", "u1"), ("vmask", "u1"), ("flags", "u1"), ("packs", "u1"),
                 ("aacks", "u1"), ("rsrc", "u1"), ("zero", "u1")])
HDR = "<IIIBBBBIIQQQIIQ"      # magic, version, n_groups, population, me, fault_tolerance, 0, window, max_live, bytes, n_slots, n_exec, max_exec, 0, 0
assert SLOT.itemsize == 56 and struct.calcsize(HDR) == 64


def a8(x):
    return (x + 7) & ~7


class Layout:
    """DESIGN.md 2, "RSPaxos replica image": where the sections of an image of G groups and R replicas are"""
    SCALARS = (("leader", "u1", 1), ("bal_prep_sent", "<u8", 1), ("bal_prepared", "<u8", 1), ("bal_max_seen", "<u8", 1), ("len", "<u4", 1),
               ("commit_bar", "<u4", 1), ("exec_bar", "<u4", 1), ("snap_bar", "<u4", 1), ("peer_exec_bar", "<u4", None), ("digest", "<u8", 1),
               ("xn", "<u4", 1))

    def __init__(self, G, R):
        self.G, self.R = G, R
        off, self.at = 64 + 32, {}
        for name, dt, rows in self.SCALARS:
            n = G * (R if rows is None else rows) * np.dtype(dt).itemsize
            self.at[name] = (off, n, dt)
            off += a8(n)
        self.fixed = off

    def boundaries(self, n_slots, n_exec):
        """the offset of every section's (and every scalar array's) end"""
        return [64, 96] + [o + a8(n) for o, n, _ in self.at.values()] + [self.fixed + 56 * n_slots, self.fixed + 56 * n_slots + a8(4 * n_exec)]

    def parse(self, img, W):
        """-> (header tuple, counters, scalars dict, slots as a dump-shaped dict [W][G], exec list [(group, slot)]); asserts
        every padding byte zero and the counts against the scalars"""
        img = bytes(img)
        h = struct.unpack_from(HDR, img)
        G, R = self.G, self.R
        assert h[0] == MAGIC and h[1] == 1 and h[2] == G and h[3] == R and h[6] == 0 and h[7] == W and h[13] == 0 and h[14] == 0, h
        ctr = np.frombuffer(img, "<u8", 4, 64)
        s = {}
        for name, (off, n, dt) in self.at.items():
            a = np.frombuffer(img, dt, n // np.dtype(dt).itemsize, off)
            s[name] = a.reshape(R, G) if name == "peer_exec_bar" else a
            assert not any(img[off + n:off + a8(n)]), (name, "padding")
        live = np.minimum(s["len"], W)
        lo = s["len"] - live
        assert h[9] == self.fixed + 56 * h[10] + a8(4 * h[11]) == len(img), (h, len(img))
        assert h[10] == int(live.sum()) and h[11] == int(s["xn"].sum()) and h[8] == int(live.max()) and h[12] == int(s["xn"].max()), h
        recs = np.frombuffer(img, SLOT, h[10], self.fixed)
        assert not recs["zero"].any()
        slots = {n: np.zeros((W, G), SLOT.fields[n][0]) for n in SLOT.names if n != "zero"}
        held = np.zeros((W, G), bool)
        k = 0
        for t0 in range(0, G, 64):                                           # tile, row, the groups of the tile that have a row-th live slot
            gs = np.arange(t0, min(t0 + 64, G))
            for row in range(int(live[gs].max()) if len(gs) else 0):
                sel = gs[live[gs] > row]
                w = (lo[sel] + row) & (W - 1)
                for n in slots:
                    slots[n][w, sel] = recs[n][k:k + len(sel)]
                held[w, sel] = True
                k += len(sel)
        assert k == h[10]
        ex_off = self.fixed + 56 * h[10]
        ex = np.frombuffer(img, "<u4", h[11], ex_off)
        assert not any(img[ex_off + 4 * h[11]:])
        execs, k = [], 0
        for t0 in range(0, G, 64):
            gs = np.arange(t0, min(t0 + 64, G))
            for row in range(int(s["xn"][gs].max()) if len(gs) else 0):
                sel = gs[s["xn"][gs] > row]
                execs += zip(sel.tolist(), [row] * len(sel), ex[k:k + len(sel)].tolist())
                k += len(sel)
        return h, ctr, s, slots, held, execs


DUMP_OF = dict(bal="s_bal", vbal="s_vbal", pmax="s_pmax", val="s_val", vval="s_vval", ltrig="s_ltrig", lendp="s_lendp", rtrig="s_rtrig", rendp="s_rendp",
               status="s_status", mask="s_mask", vmask="s_vmask", flags="s_flags", packs="s_packs", aacks="s_aacks", rsrc="s_rsrc")
NULL_CELL = dict(s_bal=0, s_status=0, s_val=NULL, s_mask=0, s_vbal=0, s_vval=NULL, s_vmask=0, s_flags=0, s_ltrig=0, s_lendp=0, s_packs=0, s_aacks=0,
                 s_pmax=0, s_rsrc=0xFF, s_rtrig=0, s_rendp=0)


def same_image(img, d, W, where, polled=None):
    """the exported image against a dump `d` (the oracle's): header, counters, every scalar, every live instance; cells outside
    the live spans are not in the image and null in the dump.  polled: the (group, slot) arrays `exec_poll` gave"""
    G, R = d["len"].shape[0], d["peer_exec_bar"].shape[0]
    h, ctr, s, slots, held, execs = Layout(G, R).parse(img, W)
    assert np.array_equal(ctr, d["counters"]), (where, "counters")
    for n in ("leader", "bal_prep_sent", "bal_prepared", "bal_max_seen", "len", "commit_bar", "exec_bar", "snap_bar", "peer_exec_bar", "digest"):
        assert np.array_equal(s[n], d[n]), (where, n)
    for n, dn in DUMP_OF.items():
        want = np.where(held, d[dn], 0)
        assert np.array_equal(slots[n], want), (where, n)
        assert (d[dn][~held] == NULL_CELL[dn]).all(), (where, dn, "dump outside the span")
    if polled is not None:
        order = sorted(execs)                                                # group-major, list position
        assert [x[0] for x in order] == list(polled[0]) and [x[2] for x in order] == list(polled[1]), (where, "exec list")
    return h


def dumps_equal(a, b, where):
    for n in b:
        assert np.array_equal(a[n], b[n]), (where, n, [x[:4] for x in np.nonzero(a[n] != b[n])])


def polls_equal(a, b, where):
    for x, y in zip(a, b):
        assert np.array_equal(x, y), (where, "exec_poll", len(x), len(y))


def _reps(dev, G, R, W, ft):
    from summerset_amd import RSPaxosReplicaGroup
    return [RSPaxosReplicaGroup(G, R, me=r, window=W, fault_tolerance=ft) for r in range(R)]


def _close(xs):
    for x in xs:
        x.close()


# ---- 2. shadow at every boundary -------------------------------------------------------------------------------------------------
def shadow_replicas(dev, oracle, G, R, ft, W=8, T=44, loss=0.1, seed=None, cluster_form=False, round0=None, rare=True, wrapped=True):
    """rsp_scenarios.run (loss on all seven kinds, two leader changes, the rings wrapping: longest >= 5 W) -- or, with round0,
    rsp_edges.wide_schedule -- and after EVERY tick every replica is saved and loaded into a spare object, whose dump and
    exec_poll must be the original's and the oracle's; the exported image is parsed against the oracle's dump; then the spare is
    swapped in, so every later tick runs on loaded state, and the per-tick oracle parity (messages, executed lists, dumps) goes on
    to the end.  cluster_form: the n replicas in one launch each way.  rare: G = 1 cannot reach every rare path; wrapped: False for
    a run of T = W ticks (the device's widest shape), whose rings fill but do not wrap"""
    from summerset_amd import RSPaxosSnapshot
    from summerset_amd.rspaxos import load_cluster_state, save_cluster_state
    seed = G + ft if seed is None else seed
    if round0 is None:
        schedule = lambda reps, on_tick: sc.run(reps, G, T, seed=seed, loss=loss, on_tick=on_tick)
    else:
        schedule = lambda reps, on_tick: e.wide_schedule(reps, G, T, seed, loss, round0, on_tick)
    orcs, lo, snaps, execd = e.oracle_run(oracle, schedule, G, R, W, ft)
    cov = e.reach(orcs, lo)
    if rare:
        e.assert_reached_every_rare_path(cov, redirects=round0 is None)
    if not wrapped:
        assert cov["longest"] >= W, cov
    elif round0 is None:
        assert cov["longest"] >= 5 * W, cov
    else:
        assert int(max(o.dump()["bal_max_seen"].max() for o in orcs)) >= 2**32 and cov["longest"] > W, cov
    live = [rc.NumpyEngine(x, dev) for x in _reps(dev, G, R, W, ft)]
    spare = _reps(dev, G, R, W, ft)
    held = [RSPaxosSnapshot.create_like(x) for x in spare]
    probe = [RSPaxosSnapshot.create_like(x) for x in spare]                  # import's checks against every state the run passes through
    seen = dict(ticks=0, n_exec=0, max_live=0, max_exec=0)

    def boundary(t):
        for r in range(R):
            for x, y in zip(live[r].take_executed(), execd[t][r]):
                assert np.array_equal(x, y), (t, r, "executed", len(x), len(y))
            dumps_equal(live[r].dump(), snaps[t][r], (t, r))
        if cluster_form:
            save_cluster_state([x.e for x in live], held)
            load_cluster_state(spare, held)
        else:
            for r in range(R):
                live[r].e.save_state(held[r])
                spare[r].load_state(held[r])
        for r in range(R):
            dumps_equal(spare[r].dump(), snaps[t][r], (t, r, "loaded"))
            polled = live[r].e.exec_poll()
            polls_equal(spare[r].exec_poll(), polled, (t, r))
            img = held[r].export()
            h = same_image(img, snaps[t][r], W, (t, r, "image"), polled=(polled[0], polled[1]))
            assert probe[r].import_(img).export() == img, (t, r, "import")
            info = held[r].info()
            assert (info["n_slots"], info["n_exec"], info["max_live"], info["max_exec"], info["window"], info["replica_id"], info["fault_tolerance"]) == \
                (h[10], h[11], h[8], h[12], W, r, ft), info
            seen["n_exec"] += info["n_exec"]; seen["max_live"] = max(seen["max_live"], info["max_live"]); seen["max_exec"] = max(seen["max_exec"], info["max_exec"])
            old = live[r].e
            live[r] = rc.NumpyEngine(spare[r], dev)                          # every later tick runs on loaded state
            spare[r] = old
        seen["ticks"] += 1
    le = schedule(live, boundary)
    assert seen["ticks"] == len(snaps) and len(le) == len(lo)
    for (t, a), (_, b) in zip(le, lo):
        assert len(a) == len(b), t
        for x, y in zip(a, b):
            for k in y:
                assert np.array_equal(x[k], y[k]) if isinstance(y[k], np.ndarray) else x[k] == y[k], (t, y["kind"], k)
    assert seen["n_exec"] > 0 and seen["max_live"] == W, seen                # pending exec lists and full rings went through images
    _close([x.e for x in live] + spare + held + probe)
    return dict(cov, **seen)


# ---- 4. canonical bytes ----------------------------------------------------------------------------------------------------------
def canonical_bytes(dev, oracle, G=130, R=5, leader=3, ft=1, W=8, loss=0.2, T=14, hb_every=3):
    """(a) one logical state reached handler by handler (`rsp_cluster.tick` on the engines), by `SteadyLoop` call by call and by
    `smr_rsp_cluster_steady_tick` in one launch -- tests/test_zz_rsp_steady_gpu.run_steady's tokens and losses, T > W ticks -- gives
    the same bytes for every replica, and they parse to the oracle cluster's dumps; (b) export(load(import(export))) is the
    identity"""
    import torch
    from summerset_amd import RSPaxosSnapshot
    s = leader
    dv = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)

    def ticks():
        rng = np.random.default_rng(G * 7 + ft)
        for t in range(T):
            val = (1 + t * G + np.arange(G)).astype(np.uint32)
            val[rng.random(G) < 0.1] = NULL
            drop = {}
            for q in (q for q in range(R) if q != s):
                drop[("accept", s, q)] = rng.random(G) < loss
                drop[("accept_reply", q, s)] = rng.random(G) < loss
                drop[("hb", s, q)] = rng.random(G) < loss
                drop[("hb", q, s)] = rng.random(G) < loss
            yield val, drop, (t % hb_every) == hb_every - 1
    orcs = [oracle.RspOracle(G, R, me=r, W=W, fault_tolerance=ft) for r in range(R)]
    for o in orcs:
        o.preset_leader(s)
    for val, drop, hb in ticks():
        rc.tick(orcs, val, np.full(G, s, np.uint8), drop=drop, heartbeat=hb)
    want = [o.dump() for o in orcs]
    assert int(want[s]["len"].max()) > W and int(want[s]["counters"][0]) > 0          # the rings wrapped, the leader committed
    assert any((d["commit_bar"] < want[s]["commit_bar"]).any() for d in want)         # ... and the losses left followers behind
    images = []
    for arm in ("handlers", "calls", "one_launch"):
        reps = _reps(dev, G, R, W, ft)
        for x in reps:
            x.preset_leader(s)
        if arm == "handlers":
            engs = [rc.NumpyEngine(x, dev) for x in reps]
            for val, drop, hb in ticks():
                rc.tick(engs, val, np.full(G, s, np.uint8), drop=drop, heartbeat=hb)
        else:
            loop = rc.SteadyLoop(reps, leader=s, one_launch=arm == "one_launch")
            for val, drop, hb in ticks():
                loop.tick(dv(val.view(np.int32)), lost={k: dv(v) for k, v in drop.items()}, heartbeat=hb)
            loop.close()
        out = []
        for r in range(R):
            dumps_equal(reps[r].dump(), want[r], (arm, r))
            snap = reps[r].save_state()
            img = snap.export()
            same_image(img, want[r], W, (arm, r))
            # (b) through bytes into another snapshot, into a fresh replica, out again
            fresh = _reps(dev, G, R, W, ft)[r]
            fresh.load_state(RSPaxosSnapshot(fresh).import_(img))
            dumps_equal(fresh.dump(), want[r], (arm, r, "fresh"))
            polls_equal(fresh.exec_poll(), reps[r].exec_poll(), (arm, r))
            assert fresh.save_state().export() == img, (arm, r, "round trip")
            out.append(img)
            fresh.close(); snap.close()
        images.append(out)
        _close(reps)
    for r in range(R):
        assert images[0][r] == images[1][r] == images[2][r], r
    return images[0]


# ---- 5. restart of one replica -----------------------------------------------------------------------------------------------------
class _Down:
    """what stands at a destroyed replica's place in the engine list while it is away: the closed loop still makes the three calls
    that every replica gets every tick (no HearTimeout, no batch, an Accept that was lost) -- answered with nothing -- and no other"""

    def __init__(self, G, R, W, me):
        self.G, self.R, self.W, self.me = G, R, W, me

    def preset_leader(self, leader):
        raise AssertionError("a call reached a replica that is down")

    def become_leader(self, src):
        assert (src == NO_REP).all()
        z32, z64, z8 = np.zeros(self.G, np.uint32), np.zeros(self.G, np.uint64), np.zeros(self.G, np.uint8)
        return dict(hb_flags=z8, hb_ballot=z64, hb_commit=z32, hb_exec=z32, hb_snap=z32, p_flags=z8, p_trig=z32, p_ballot=z64, rc_n=z32,
                    rc_slot=np.zeros((self.W, self.G), np.uint32))

    def req_batch(self, val):
        assert (val == NULL).all()
        return dict(a_n=np.zeros(self.G, np.uint32), a_slot=np.zeros((self.W, self.G), np.uint32), a_val=np.zeros((self.W, self.G), np.uint32),
                    a_ballot=np.zeros(self.G, np.uint64))

    def accept(self, flags, **kw):
        assert not flags.any()
        return dict(r_ballot=np.zeros(self.G, np.uint64), r_slot=np.zeros(self.G, np.uint32))

    def is_leader(self):
        return np.zeros(self.G, np.uint8)

    def take_executed(self):
        return tuple(np.zeros(0, np.uint32) for _ in range(3))


def restart_one_replica(dev, oracle, G=130, R=5, ft=1, W=8, q=2, t_save=16, k=4, T=34, loss=0.05, seed=71, L=61):
    """tests/test_zz_rsp_payload_gpu.make_cluster's cluster (every replica an engine and its payload store).  Replica q (a
    follower) AND ITS STORE are saved at the end of tick t_save - 1 (`RSPaxosReplicaWithPayload.save_state`, both halves on one
    stream), exported, and both objects DESTROYED; the others run k ticks with every message to and from q lost (on the oracle side q
    is simply cut off by the same drop map: its state stays the saved one); fresh objects are made, the two images imported and
    loaded (`load_state`), and q rejoins.  Parity against the oracle cluster holds after every tick, and `check_stores` (engine
    masks, the oracle's codewords byte for byte) runs on every replica that is up after every tick, on all of them to the end.
    "Caught up": an RSPaxos follower's commit_bar does not move in the steady state at all (it holds one shard of a
    codeword, and the commit-bar run waits for `majority`; the oracle's stays 0, asserted below), so `commit_bar` equal to the
    leader's cannot be reached by any follower, restarted or not; what is asked is what a follower does learn:
    every live instance below the leader's commit bar is Committed at q.  During the outage only the odd groups get batches:
    there q has lost Accepts for good, like any follower that lost one, while in the even groups it missed only Heartbeats and
    catches up at the first one it hears -- both asserted on the oracle cluster alone."""
    import test_zz_rsp_payload_gpu as tp
    from summerset_amd import PayloadStoreSnapshot, RSPaxosPayloadStore, RSPaxosReplicaGroup, RSPaxosReplicaWithPayload, RSPaxosSnapshot
    assert q != 0 and t_save > W and t_save % 3 != 0                         # (tick t_save - 1 carried no Heartbeat: q is behind at the save)
    g = np.arange(G)

    def schedule(reps, on_tick):
        for r in reps:
            r.preset_leader(0)
        rng = np.random.default_rng(seed)
        log = []
        for t in range(T):
            away = t_save <= t < t_save + k
            val = (1 + t * G + g).astype(np.uint32)
            val[rng.random(G) < 0.1] = NULL
            if away:
                val[g % 2 == 0] = NULL
            drop = {(kd, a, b): rng.random(G) < loss for kd in e.KINDS for a in range(R) for b in range(R) if a != b}
            for key in [x for x in drop if q in x[1:]]:                      # q itself loses nothing while it is up: no gaps of its own
                del drop[key]
            if away:
                for kd in e.KINDS:
                    for p in range(R):
                        if p != q:
                            drop[(kd, p, q)] = np.ones(G, bool); drop[(kd, q, p)] = np.ones(G, bool)
            on_tick(t, "before")
            log.append((t, rc.tick(reps, val, np.zeros(G, np.uint8), drop=drop, heartbeat=(t % 3 == 2))))
            on_tick(t, "after")
        return log
    orcs = [oracle.RspOracle(G, R, me=r, W=W, fault_tolerance=ft) for r in range(R)]
    rec = dict(dumps=[], execd=[])

    def o_tick(t, when):
        if when == "after":
            rec["dumps"].append([o.dump() for o in orcs]); rec["execd"].append([o.take_executed() for o in orcs])
    lo = schedule(orcs, o_tick)
    D = rec["dumps"]
    even = g % 2 == 0
    assert (D[t_save - 1][q]["len"] > W).all()                               # saved on a wrapped ring
    dumps_equal(D[t_save + k - 1][q], D[t_save - 1][q], "the oracle's q did not move while it was cut off")
    assert (D[t_save + k - 1][0]["commit_bar"][~even] > D[t_save - 1][0]["commit_bar"][~even]).any()   # the others went on
    # the issue's criterion, commit_bar equal to the leader's, is out of reach of EVERY follower of this schedule, q or not:
    assert all((D[T - 1][r]["commit_bar"] == 0).all() for r in range(1, R)) and (D[T - 1][0]["commit_bar"] > W).mean() > 0.5
    def learned(dq, d0):
        """bool [G]: every live instance of q below the leader's commit bar is Committed or Executed at q"""
        ok = np.ones(G, bool)
        lo = dq["len"] - np.minimum(dq["len"], W)
        for w in range(W):
            s_ = (lo & ~np.uint32(W - 1)) | np.uint32(w)
            s_ = np.where(s_ < lo, s_ + W, s_)
            ok &= ~((s_ < dq["len"]) & (s_ < d0["commit_bar"]) & (dq["s_status"][w] < 3))
        return ok
    assert not learned(D[t_save + k - 1][q], D[t_save + k - 1][0])[even].all()                # behind when it comes back
    caught = [t for t in range(t_save + k, T) if learned(D[t][q], D[t][0])[even].all()]
    assert caught and not learned(D[T - 1][q], D[T - 1][0])[~even].all()
    assert (D[T - 1][q]["len"] > D[t_save - 1][q]["len"]).all()              # q took new Accepts after it came back

    reps, live = tp.make_cluster(dev, G, R, W, ft, L)
    exp = tp.Expect(oracle, R, R // 2 + 1, L)
    st = dict(images=None, stepped=0, cmp=0, copied=None)

    def e_tick(t, when):
        if when == "before" and t == t_save:
            st["copied"] = reps[q].store.counters()["copied"]
            rs, ps = reps[q].save_state()
            info = ps.info()
            assert info["n_cells"] > 0 and info["shard_bytes"] > 0 and reps[q].store.voted_alias().any(), info
            st["images"] = (rs.export(), ps.export())
            _close([rs, ps, reps[q].replica, reps[q].store])                 # (a closed store is an empty seat among the peers' sources)
            live[q] = _Down(G, R, W, q)
        if when == "before" and t == t_save + k:
            fresh = RSPaxosReplicaWithPayload(RSPaxosReplicaGroup(G, R, me=q, window=W, fault_tolerance=ft), RSPaxosPayloadStore(G, R, W, max_data_len=L),
                                              reps[q].payload)
            snaps = (RSPaxosSnapshot(fresh.replica).import_(st["images"][0]), PayloadStoreSnapshot(fresh.store).import_(st["images"][1]))
            fresh.load_state(snaps)
            _close(snaps)
            reps[q] = fresh
            for r in reps:
                r.set_peers(reps)
            live[q] = rc.NumpyEngine(fresh, dev)
            dumps_equal(fresh.replica.dump(), D[t_save - 1][q], "reloaded")
            again = fresh.save_state()
            assert (again[0].export(), again[1].export()) == st["images"], "the fresh objects' own images are not the saved ones"
            _close(again)
        if when == "after":
            up = [r for r in range(R) if not isinstance(live[r], _Down)]
            for r in range(R):
                for x, y in zip(live[r].take_executed(), rec["execd"][t][r]):
                    assert np.array_equal(x, y) or r not in up, (t, r, "executed")
            for r in up:
                dumps_equal(live[r].dump(), D[t][r], (t, r))
                st["stepped"] += 1
            st["cmp"] += tp.check_stores([reps[r] for r in up], exp, (t, up))
    le = schedule(live, e_tick)
    for (t, a), (_, b) in zip(le, lo):
        assert len(a) == len(b), t
        for x, y in zip(a, b):
            for kk in y:
                assert np.array_equal(x[kk], y[kk]) if isinstance(y[kk], np.ndarray) else x[kk] == y[kk], (t, y["kind"], kk)
    assert tp.check_stores(reps, exp, "end") > 0 and st["cmp"] > 0
    assert reps[q].store.counters()["copied"] > st["copied"]                 # q's store took shards after it came back
    assert sum(r.store.counters()["unsatisfied"] for r in reps) == 0
    _close([r.replica for r in reps] + [r.store for r in reps])
    return dict(stepped=st["stepped"], caught_up_at=caught[0], image_bytes=[len(x) for x in st["images"]], shards_compared=st["cmp"])


# ---- 6. hand-built image -----------------------------------------------------------------------------------------------------------
def hand_built_image(dev):
    """an image written in numpy from DESIGN.md 2's table alone -- a wrapped span, a short one and an empty one, an instance of
    every status, one with leader bookkeeping and one with replica bookkeeping, a pending exec list -- is imported and loaded into a
    fresh replica: dump / exec_poll give what was written, and the replica's own next image is these bytes"""
    from summerset_amd import RSPaxosReplicaGroup, RSPaxosSnapshot
    G, R, W, me, ft = 3, 3, 8, 1, 1
    lay = Layout(G, R)
    ln = np.array([11, 2, 0], np.uint32)                                     # live spans [3, 11), [0, 2), none
    xn = np.array([2, 1, 0], np.uint32)
    sc_ = dict(leader=np.array([1, 0, NO_REP], np.uint8), bal_prep_sent=np.array([0x102, 0, 0], np.uint64), bal_prepared=np.array([0x102, 0, 0], np.uint64),
               bal_max_seen=np.array([0x102, 0x101, 0], np.uint64), len=ln, commit_bar=np.array([9, 1, 0], np.uint32), exec_bar=np.array([8, 1, 0], np.uint32),
               snap_bar=np.array([2, 0, 0], np.uint32), peer_exec_bar=np.array([[7, 0, 0], [0, 0, 0], [6, 0, 0]], np.uint32),
               digest=np.array([0xDEADBEEF12345678, 5, 0], np.uint64), xn=xn)
    want = {dn: np.full((W, G), v, np.dtype(SLOT.fields[n][0])) for n, dn in DUMP_OF.items() for v in [NULL_CELL[dn]]}
    cells = {}
    for k, slot in enumerate(range(3, 11)):                                  # group 0: every status; slot 9 leads, slot 10 follows
        c = dict(bal=0x102, vbal=0x101 + k, pmax=0, val=100 + slot, vval=200 + slot, ltrig=0, lendp=0, rtrig=0, rendp=0, status=k % 5, mask=0x7, vmask=0x2,
                 flags=0, packs=0, aacks=0, rsrc=0xFF)
        if slot == 9:
            c.update(flags=1 | 4, ltrig=8, lendp=10, packs=0x3, aacks=0x6, pmax=0x101, status=1)
        if slot == 10:
            c.update(flags=2, rsrc=2, rtrig=9, rendp=10, status=2)
        cells[(0, slot)] = c
    cells[(1, 0)] = dict(bal=0x101, vbal=0x101, pmax=0, val=7, vval=7, ltrig=0, lendp=0, rtrig=0, rendp=0, status=4, mask=0x2, vmask=0x2, flags=2, packs=0,
                         aacks=0, rsrc=0)
    cells[(1, 1)] = dict(bal=0, vbal=0, pmax=0, val=NULL, vval=NULL, ltrig=0, lendp=0, rtrig=0, rendp=0, status=0, mask=0, vmask=0, flags=0, packs=0,
                         aacks=0, rsrc=0xFF)
    assert {c["status"] for c in cells.values()} == {0, 1, 2, 3, 4}
    order = [(g, row) for row in range(W) for g in range(G) if row < min(ln[g], W)]          # one tile: row, then group
    recs = np.zeros(len(order), SLOT)
    for i, (g, row) in enumerate(order):
        slot = int(ln[g]) - min(int(ln[g]), W) + row
        for n, v in cells[(g, slot)].items():
            recs[n][i] = v
            want[DUMP_OF[n]][slot & (W - 1), g] = v
    ex = [(g, row) for row in range(W) for g in range(G) if row < xn[g]]
    ex_slot = {(0, 0): 5, (0, 1): 7, (1, 0): 0}
    execs = np.array([ex_slot[x] for x in ex], "<u4")
    img = bytearray(lay.fixed)
    struct.pack_into("<4Q", img, 64, 11, 3, 0, 2)
    for n, (off, nb, dt) in lay.at.items():
        img[off:off + nb] = np.ascontiguousarray(sc_[n]).astype(dt).tobytes()
    img += recs.tobytes() + execs.tobytes() + bytes(a8(4 * len(execs)) - 4 * len(execs))
    struct.pack_into(HDR, img, 0, MAGIC, 1, G, R, me, ft, 0, W, 8, len(img), len(recs), len(execs), 2, 0, 0)
    img = bytes(img)
    rep = RSPaxosReplicaGroup(G, R, me=me, window=W, fault_tolerance=ft)
    snap = RSPaxosSnapshot(rep).import_(img)
    assert snap.info() == dict(bytes=len(img), n_slots=10, n_exec=3, n_groups=G, window=W, max_live=8, max_exec=2, population=R, replica_id=me, fault_tolerance=ft)
    rep.load_state(snap)
    d = rep.dump()
    for n, v in sc_.items():
        if n != "xn":
            assert np.array_equal(d[n], v), n
    assert list(d["counters"]) == [11, 3, 0, 2]
    for dn in want:
        assert np.array_equal(d[dn], want[dn]), (dn, d[dn], want[dn])
    pg, ps, pv = rep.exec_poll()
    assert list(pg) == [0, 0, 1] and list(ps) == [5, 7, 0] and list(pv) == [105, 107, 7], (pg, ps, pv)
    assert rep.save_state().export() == img
    rep.close(); snap.close()


# ---- 7. stream order ---------------------------------------------------------------------------------------------------------------
def stream_order(dev, oracle, G=300, R=5, ft=1, W=8, T=12, t_save=10):
    """a save enqueued directly behind a steady tick's launch on the same stream, no synchronisation in front or behind, more ticks
    behind it: the image is the state at the save point (the oracle's dumps recorded there)"""
    import torch
    from summerset_amd.rspaxos import load_cluster_state, save_cluster_state
    rng = np.random.default_rng(89)
    vals = [(1 + t * G + np.arange(G)).astype(np.uint32) for t in range(T)]
    for v in vals:
        v[rng.random(G) < 0.1] = NULL
    orcs = [oracle.RspOracle(G, R, me=r, W=W, fault_tolerance=ft) for r in range(R)]
    for o in orcs:
        o.preset_leader(0)
    at_save = None
    for t in range(T):
        rc.tick(orcs, vals[t], np.zeros(G, np.uint8), heartbeat=(t % 3 == 2))
        if t + 1 == t_save:
            at_save = [o.dump() for o in orcs]
    assert int(at_save[0]["len"].max()) > W and int(orcs[0].dump()["counters"][0]) > int(at_save[0]["counters"][0]) > 0
    reps = _reps(dev, G, R, W, ft)
    for x in reps:
        x.preset_leader(0)
    loop = rc.SteadyLoop(reps, leader=0, one_launch=True)
    held, snaps = [], None
    for t in range(T):
        v = torch.from_numpy(vals[t].view(np.int32)).to(dev)
        held.append(v)
        loop.tick(v, heartbeat=(t % 3 == 2))
        if t + 1 == t_save:
            snaps = save_cluster_state(reps)                                 # no synchronisation in front, none behind
    for r in range(R):
        dumps_equal(reps[r].dump(), orcs[r].dump(), ("end", r))
    B = _reps(dev, G, R, W, ft)
    load_cluster_state(B, snaps)
    for r in range(R):
        dumps_equal(B[r].dump(), at_save[r], ("at the save point", r))
        same_image(snaps[r].export(), at_save[r], W, ("at the save point", r))
    loop.close()
    _close(reps + B + snaps)


# ---- 8. refusals -------------------------------------------------------------------------------------------------------------------
def refusals(dev, oracle, G=70, R=5, W=16):
    """SMR_ERR_ARG with smr_last_error() set, and the target's dump the same before and after: null arguments; a replica of another
    G, R, id, fault_tolerance or window; an export buffer too small; imports truncated at every length (every section boundary
    and one byte short among them), with each header field corrupted, with counts that contradict the scalars, with a non-zero
    padding byte, with bookkeeping fields where the flag is absent"""
    import ctypes as C
    import torch
    from summerset_amd import RSPaxosReplicaGroup, RSPaxosSnapshot, SummersetError, _lib
    L = _lib.load()

    def refused(f, word=None, code=-1):
        try:
            rc_ = f()
        except SummersetError as err:
            assert err.code == code and (word is None or word in str(err)), (word, err)
            return
        assert isinstance(rc_, int) and rc_ == code, rc_
        msg = L.smr_last_error().decode()
        assert msg and (word is None or word in msg), (word, msg)
    a = RSPaxosReplicaGroup(G, R, me=1, window=W, fault_tolerance=1)
    a.preset_leader(1)
    a.req_batch(torch.from_numpy((1 + np.arange(G)).astype(np.int32)).to(dev))
    snap = a.save_state()
    h = C.c_void_p()
    refused(lambda: L.smr_rsp_snapshot_create(None, C.byref(h)), "null")
    refused(lambda: L.smr_rsp_snapshot_create(a._h, None), "null")
    refused(lambda: L.smr_rsp_save_state(None, snap._h, None), "null")
    refused(lambda: L.smr_rsp_save_state(a._h, None, None), "null")
    refused(lambda: L.smr_rsp_load_state(None, snap._h, None), "null")
    refused(lambda: L.smr_rsp_load_state(a._h, None, None), "null")
    refused(lambda: L.smr_rsp_snapshot_info_get(None, None), "null")
    refused(lambda: L.smr_rsp_snapshot_info_get(snap._h, None), "null")
    refused(lambda: int(L.smr_rsp_snapshot_export(None, None, 0)), "null")
    refused(lambda: L.smr_rsp_snapshot_import(snap._h, None, 0), "null")
    refused(lambda: L.smr_rsp_snapshot_import(None, None, 0), "null")
    refused(lambda: L.smr_rsp_cluster_save_state(1, None, None, None), "null")
    refused(lambda: L.smr_rsp_cluster_load_state(1, None, None, None), "null")
    refused(lambda: L.smr_rsp_cluster_save_state(9, (C.c_void_p * 9)(), (C.c_void_p * 9)(), None), "1 .. 8")
    refused(lambda: L.smr_rsp_cluster_save_state(2, (C.c_void_p * 2)(a._h, a._h), (C.c_void_p * 2)(snap._h, snap._h), None), "twice")
    L.smr_rsp_snapshot_destroy(None)
    empty = RSPaxosSnapshot(a)
    refused(lambda: a.load_state(empty), "nothing saved", code=-3)
    refused(lambda: empty.info(), "nothing saved", code=-3)
    empty.close()
    da = a.dump()
    image = snap.export()
    others = dict(n_groups=RSPaxosReplicaGroup(G + 1, R, me=1, window=W, fault_tolerance=1), population=RSPaxosReplicaGroup(G, 7, me=1, window=W, fault_tolerance=1),
                  replica_id=RSPaxosReplicaGroup(G, R, me=2, window=W, fault_tolerance=1), fault_tolerance=RSPaxosReplicaGroup(G, R, me=1, window=W, fault_tolerance=0))
    for what, b in others.items():
        b.preset_leader(0)
        before = b.dump()
        refused(lambda: b.load_state(snap), "made for")
        refused(lambda: b.save_state(snap), "made for")
        refused(lambda: RSPaxosSnapshot(b).import_(image), "the image is of" if what != "n_groups" else None)
        dumps_equal(b.dump(), before, what)
    for w2 in (W // 2, 2 * W):                                               # another window: through the snapshot and through its bytes
        b = RSPaxosReplicaGroup(G, R, me=1, window=w2, fault_tolerance=1)
        b.preset_leader(0)
        before = b.dump()
        refused(lambda: b.load_state(snap), "window")
        refused(lambda: b.load_state(RSPaxosSnapshot(b).import_(image)), "window")
        dumps_equal(b.dump(), before, ("window", w2))
        b.close()
    assert snap.export() == image                                            # (a refused save left the snapshot's image alone)
    n = snap.info()["bytes"]
    buf = (C.c_uint8 * n)()
    refused(lambda: int(L.smr_rsp_snapshot_export(snap._h, buf, n - 1)), "takes")
    refused(lambda: int(L.smr_rsp_snapshot_export(snap._h, buf, 0)), "takes")
    assert L.smr_rsp_snapshot_export(snap._h, buf, n) == n and bytes(buf) == image
    # a small image: three groups, a pending execution, bookkeeping of both kinds
    g, r_ = 3, 3
    tiny_rep = RSPaxosReplicaGroup(g, r_, me=0, window=8, fault_tolerance=0)
    orc = oracle.RspOracle(g, r_, me=0, W=8, fault_tolerance=0)
    t32 = lambda x: torch.from_numpy(np.asarray(x, np.uint32).view(np.int32)).to(dev)
    for x in (tiny_rep, orc):
        x.preset_leader(0)
    tiny_rep.req_batch(t32([5, NULL, 6])); orc.req_batch(np.array([5, NULL, 6], np.uint32))
    kw = dict(slot=np.zeros(g, np.uint32), ballot=np.full((r_, g), 0x101, np.uint64), flags=np.array([[0, 0, 0], [1, 0, 0], [0, 0, 0]], np.uint8))
    tiny_rep.accept_replies(t32(kw["slot"]), torch.from_numpy(kw["ballot"].view(np.int64)).to(dev), torch.from_numpy(kw["flags"]).to(dev))
    orc.accept_replies(**kw)
    ts = tiny_rep.save_state()
    tiny = ts.export()
    lay = Layout(g, r_)
    hd = same_image(tiny, orc.dump(), 8, "tiny")
    assert hd[10] == 2 and hd[11] == 1 and len(tiny) == lay.fixed + 2 * 56 + 8 and len(tiny) < 600, hd
    target = RSPaxosSnapshot(tiny_rep)
    cuts = set(lay.boundaries(2, 1))
    assert max(cuts) == len(tiny) and len(tiny) - 1 not in cuts
    for cut in range(len(tiny)):                                             # (a copy of exactly that length: a read past it is a read past the buffer)
        refused(lambda: target.import_(tiny[:cut]))
    target.import_(tiny)
    assert target.export() == tiny
    # each header field corrupted: magic, version, n_groups, population, me, fault_tolerance, reserved0, window, max_live, bytes,
    # n_slots, n_exec, max_exec, reserved1, reserved2
    for off, size in [(0, 4), (4, 4), (8, 4), (12, 1), (13, 1), (14, 1), (15, 1), (16, 4), (20, 4), (24, 8), (32, 8), (40, 8), (48, 4), (52, 4), (56, 8)]:
        for delta in (1, 0x80):
            bad = bytearray(tiny)
            bad[off] = (bad[off] + delta) & 0xFF
            refused(lambda: target.import_(bytes(bad)))
            if size == 8:
                bad = bytearray(tiny)
                bad[off + 7] ^= 0x80                                         # counts near 2^63: bounded before they are multiplied
                refused(lambda: target.import_(bytes(bad)))
    bad = bytearray(tiny); bad[13] = 3
    refused(lambda: target.import_(bytes(bad)), "below its population")
    bad = bytearray(tiny); struct.pack_into("<I", bad, 0, MAGIC ^ 1)
    refused(lambda: target.import_(bytes(bad)), "magic")
    bad = bytearray(tiny); struct.pack_into("<I", bad, 4, 2)
    refused(lambda: target.import_(bytes(bad)), "version")
    # counts against the scalars: a group's len raised, xn raised, the maxima lowered
    bad = bytearray(tiny); struct.pack_into("<I", bad, lay.at["len"][0], 2)
    refused(lambda: target.import_(bytes(bad)), "malformed")
    bad = bytearray(tiny); struct.pack_into("<I", bad, lay.at["xn"][0] + 4, 1)
    refused(lambda: target.import_(bytes(bad)), "malformed")
    bad = bytearray(tiny); struct.pack_into("<I", bad, lay.at["xn"][0], 9)
    refused(lambda: target.import_(bytes(bad)), "malformed")
    bad = bytearray(tiny); struct.pack_into("<I", bad, 20, 0)
    refused(lambda: target.import_(bytes(bad)), "max_live")
    bad = bytearray(tiny); struct.pack_into("<I", bad, 48, 0)
    refused(lambda: target.import_(bytes(bad)), "max_exec")
    # every padding byte; ids and fields of the body
    pads = [p for off, nb, _ in lay.at.values() for p in range(off + nb, off + a8(nb))] + list(range(len(tiny) - 4, len(tiny)))
    assert len(pads) >= 4 * 5 + 5 + 4
    for p in pads:
        bad = bytearray(tiny); bad[p] = 1
        refused(lambda: target.import_(bytes(bad)), "padding")
    rec0 = lay.fixed
    for off, val in ((lay.at["leader"][0], 3), (rec0 + 48, 5), (rec0 + 49, 0x8), (rec0 + 50, 0x10), (rec0 + 51, 0x8), (rec0 + 55, 1), (rec0 + 52, 0x8)):
        bad = bytearray(tiny); bad[off] = val
        refused(lambda: target.import_(bytes(bad)), "malformed")
    r0 = np.frombuffer(tiny, SLOT, 2, rec0)
    assert r0["flags"][0] == 5 and r0["rsrc"][0] == 0xFF and r0["rtrig"][0] == 0          # leader bookkeeping, no replica bookkeeping:
    for off in (rec0 + 40, rec0 + 44, rec0 + 54):                            # rtrig, rendp, rsrc must read as the dump gives them
        bad = bytearray(tiny); bad[off] = 1
        refused(lambda: target.import_(bytes(bad)), "bookkeeping")
    assert r0["flags"][1] == 5
    bad = bytearray(tiny); bad[rec0 + 56 + 51] = 4; bad[rec0 + 56 + 32] = 1  # flags without leader bookkeeping, ltrig left behind
    refused(lambda: target.import_(bytes(bad)), "bookkeeping")
    assert target.export() == tiny                                           # the refused imports left the target's image alone
    fresh = RSPaxosReplicaGroup(g, r_, me=0, window=8, fault_tolerance=0)
    fresh.load_state(target)
    dumps_equal(fresh.dump(), orc.dump(), "tiny")
    polls_equal(fresh.exec_poll(), tiny_rep.exec_poll(), "tiny")
    assert len(fresh.exec_poll()[0]) == 1
    dumps_equal(a.dump(), da, "a")
    _close(list(others.values()) + [a, snap, tiny_rep, ts, target, fresh])


# ---- 9. growth ---------------------------------------------------------------------------------------------------------------------
def grows_for_a_larger_window(dev, oracle, G=70, R=5):
    """a snapshot made for a window-8 replica takes a window-64 replica with full rings: it grows inside that save call"""
    import torch
    from summerset_amd import RSPaxosReplicaGroup, RSPaxosSnapshot
    small, big = RSPaxosReplicaGroup(G, R, me=0, window=8), RSPaxosReplicaGroup(G, R, me=0, window=64)
    o = oracle.RspOracle(G, R, me=0, W=64)
    big.preset_leader(0); o.preset_leader(0)
    snap = RSPaxosSnapshot(small)
    small.save_state(snap)
    assert snap.info()["n_slots"] == 0
    for t in range(70):
        val = (1 + t * G + np.arange(G)).astype(np.uint32)
        val[t % 3::3] = NULL
        big.req_batch(torch.from_numpy(val.view(np.int32)).to(dev)); o.req_batch(val)
    d = o.dump()
    assert int(d["len"].max()) > 40 and int(np.minimum(d["len"], 64).sum()) > 8 * G
    big.save_state(snap)
    same_image(snap.export(), d, 64, "grown")
    assert snap.info()["n_slots"] == int(np.minimum(d["len"], 64).sum())
    fresh = RSPaxosReplicaGroup(G, R, me=0, window=64)
    fresh.load_state(snap)
    dumps_equal(fresh.dump(), d, "grown")
    _close([small, big, snap, fresh])


# ==== the payload stores ==============================================================================================================
PS_MAGIC = 0x42505253                                                        # "SRPB"
PS_HDR = "<IIIIBBBBIQQQQQ"    # magic, version, n_groups, window, n_shards, n_data_shards, planes, craft, max_dlen, bytes, n_cells, n_shards_stored, shard_bytes, 0
assert struct.calcsize(PS_HDR) == 64


def a16(x):
    return (x + 15) & ~15


class StoreLayout:
    """DESIGN.md 2, "payload store image": header, counters u64[5], per plane tok u32 / dlen u32 / avail u8 [W][G] (each padded to
    8), the VOTED plane's alias u8 [W][G], zero bytes to a multiple of 16, then the shard bytes"""

    def __init__(self, G, W, planes):
        self.G, self.W, self.planes, cells = G, W, planes, G * W
        off, self.at = 64 + 40, {}
        for p in range(planes):
            for name, dt in (("tok", "<u4"), ("dlen", "<u4"), ("avail", "u1")):
                n = cells * np.dtype(dt).itemsize
                self.at[(name, p)] = (off, n, dt)
                off += a8(n)
        if planes == 2:
            self.at[("alias", 1)] = (off, cells, "u1")
            off += a8(cells)
        self.hdr_end, self.fixed = off, a16(off)

    def parse(self, img, d):
        """-> (header, counters, {(name, plane): [W][G]}, {(plane, row, group, shard): bytes}); asserts every padding byte zero"""
        img = bytes(img)
        h = struct.unpack_from(PS_HDR, img)
        assert h[0] == PS_MAGIC and h[1] == 1 and h[2] == self.G and h[3] == self.W and h[6] == self.planes and h[13] == 0, h
        assert h[9] == len(img) == self.fixed + h[12], (h, len(img), self.fixed)
        a = {}
        for key, (off, n, dt) in self.at.items():
            a[key] = np.frombuffer(img, dt, self.G * self.W, off).reshape(self.W, self.G)
            assert not any(img[off + n:off + a8(n)]), (key, "padding")
        assert not any(img[self.hdr_end:self.fixed])
        shards, off, n_cells = {}, self.fixed, 0
        for t0 in range(0, self.G, 64):
            for p in range(self.planes):
                for r in range(self.W):
                    for g in range(t0, min(t0 + 64, self.G)):
                        tok, dlen, av = int(a[("tok", p)][r, g]), int(a[("dlen", p)][r, g]), int(a[("avail", p)][r, g])
                        al = int(a[("alias", 1)][r, g]) if p == 1 else 0
                        if tok == NULL:
                            assert dlen == 0 and av == 0 and al == 0, (p, r, g)
                            continue
                        n_cells += 1
                        sl = (dlen + d - 1) // d
                        for k in range(8):
                            if ((av & ~al) >> k) & 1:
                                shards[(p, r, g, k)] = img[off:off + sl]
                                assert not any(img[off + sl:off + a16(sl)]), ("shard padding", p, r, g, k)
                                off += a16(sl)
        assert off == len(img) and n_cells == h[10] and len(shards) == h[11], (off, len(img), n_cells, len(shards), h)
        return h, np.frombuffer(img, "<u8", 5, 64), a, shards


def stores_equal(a, b, where):
    """two stores hold the same state, whatever their strides: headers, alias bytes, counters, every present shard's bytes"""
    assert a.counters() == b.counters() and a.delivered() == b.delivered(), (where, a.counters(), b.counters())
    planes = 2 if type(a)._CREATE == "smr_rsp_pstore_create" else 1
    if planes == 2:
        assert np.array_equal(a.voted_alias(), b.voted_alias()), (where, "alias")
    for p in range(planes):
        x, y = a.dump(p), b.dump(p)
        some = x["tok"] != NULL
        assert np.array_equal(x["tok"], y["tok"]) and np.array_equal(x["avail"][some], y["avail"][some]) and np.array_equal(x["dlen"][some], y["dlen"][some]), (where, p)
        for w in np.nonzero(some.any(axis=1))[0]:
            ra, rb = a.read_row(int(w), p), b.read_row(int(w), p)
            for g in np.nonzero(some[w])[0]:
                sl = (int(x["dlen"][w, g]) + a.d - 1) // a.d
                for k in range(a.R):
                    if (x["avail"][w, g] >> k) & 1:
                        assert np.array_equal(ra[k, g, :sl], rb[k, g, :sl]), (where, p, w, g, k)


def shadow_stores(dev, oracle, G, R, ft, L, W=8, T=44, loss=0.1, staging=False):
    """tests/test_zz_rsp_payload_gpu.make_cluster's cluster under rsp_scenarios.run; after EVERY tick every store is saved and loaded
    into a spare of ANOTHER max_data_len (L and L + 100 take turns: another cap_sl, other strides), counters and alias bytes are
    compared, the spare is swapped in and check_stores (engine masks, the oracle's codewords byte for byte) runs on it"""
    import test_zz_rsp_payload_gpu as tp
    from summerset_amd import PayloadStoreSnapshot, RSPaxosPayloadStore
    reps, engs = tp.make_cluster(dev, G, R, W, ft, L, staging)
    exp = tp.Expect(oracle, R, R // 2 + 1, L)
    spare = [RSPaxosPayloadStore(G, R, W, max_data_len=L + 100) for _ in range(R)]
    assert spare[0].group_stride != reps[0].store.group_stride
    # (a staging store holds a message in flight inside one handler call, no state; `follow` wants its sources in the store's own
    # geometry, so it changes geometry with the store it stages for)
    sp_stage = [RSPaxosPayloadStore(G, R, W, max_data_len=L + 100) for _ in range(R)] if staging else None
    held = [PayloadStoreSnapshot.create_like(r.store) for r in reps]
    probe = PayloadStoreSnapshot.create_like(reps[0].store)                  # import's checks against every state the run passes through
    seen = dict(alias=0, lone_vote=0, cmp=0, bytes=0)

    def boundary(t):
        for r, rep in enumerate(reps):
            rep.store.save(held[r])
            spare[r].load(held[r])
            old = rep.store
            assert old.counters() == spare[r].counters() and np.array_equal(old.voted_alias(), spare[r].voted_alias()), (t, r)
            al, av = old.voted_alias(), old.dump(1)
            seen["alias"] += int((al != 0).sum()); seen["lone_vote"] += int(((av["avail"] & ~al)[av["tok"] != NULL] != 0).sum())
            info = held[r].info()
            img = held[r].export()
            assert len(img) == info["bytes"] and probe.import_(img).export() == img, (t, r, "import")
            seen["bytes"] += info["shard_bytes"]
            assert info["max_dlen"] <= L and info["planes"] == 2 and info["craft"] == 0
            rep.store, spare[r] = spare[r], old                              # every later tick runs on the loaded store
            if staging:
                rep.staging, sp_stage[r] = sp_stage[r], rep.staging
                rep._msg = None                                              # (the message buffer it reuses is sized by the stores' stride)
        seen["cmp"] += tp.check_stores(reps, exp, t)
    sc.run(engs, G, T, seed=G + ft, loss=loss, on_tick=boundary)
    assert max(int(r.replica.dump()["len"].max()) for r in reps) >= 5 * W
    tot = {k: sum(r.store.counters()[k] for r in reps) for k in ("copied", "rebuilt", "unsatisfied", "rekeyed")}
    assert tot["copied"] > 0 and tot["rebuilt"] > 0 and tot["unsatisfied"] == 0 and seen["cmp"] > 0, (tot, seen)
    assert seen["alias"] > 0 and seen["lone_vote"] > 0 and seen["bytes"] > 0, seen   # aliased votes and votes stored on their own went through images
    return dict(tot, **seen)


def store_canonical_bytes(dev, oracle, n=5, d=3, G=70, W=8, L=333):
    """(b) export(load(import(export))) is the identity; (c) two stores of the same content and different max_data_len export the
    same bytes; (d) rows that held payloads of length L and, after the ring wrapped, payloads of 1 .. 16 bytes: every pad region
    of the image is zero (StoreLayout.parse checks each) and every shard is the oracle's"""
    import torch
    from summerset_amd import PayloadStoreSnapshot, RSPaxosPayloadStore
    rng = np.random.default_rng(5)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    a, b = RSPaxosPayloadStore(G, n, W, L, num_data_shards=d), RSPaxosPayloadStore(G, n, W, L + 100, num_data_shards=d)
    want = {}
    for slot in range(2 * W):
        lens = np.full(G, L, np.uint32) if slot < W else rng.integers(1, 17, G).astype(np.uint32)
        data = rng.integers(1, 256, (G, L), dtype=np.uint8)                  # never zero: a byte left over from a longer payload shows
        tok = (1 + slot * G + np.arange(G)).astype(np.uint32)
        a_slot, a_val = np.zeros((W, G), np.uint32), np.zeros((W, G), np.uint32)
        a_slot[0], a_val[0] = slot, tok
        acc = dict(a_n=t(np.ones(G, np.int32)), a_slot=t(a_slot.view(np.int32)), a_val=t(a_val.view(np.int32)))
        for st in (a, b):
            st.put(acc, t(data), t(lens.view(np.int32)))
        if slot >= W:
            for g in range(G):
                bts = data[g, :lens[g]]
                sl = oracle.rs_shard_len(bts.size, d)
                cw = np.zeros((n, sl), np.uint8)
                cw[:d].reshape(-1)[:bts.size] = bts
                cw[d:] = oracle.rs_encode(d, n - d, bts)
                want[(slot & (W - 1), g)] = cw
    row = a.read_row(W, 0)
    assert row[0, 0, 16:a.group_stride].any()                                # the rows do hold bytes of the longer payloads behind the short shards
    sa, sb = a.save(), b.save()
    ia, ib = sa.export(), sb.export()
    assert ia == ib                                                          # (c)
    h, ctr, arr, shards = StoreLayout(G, W, 2).parse(ia, d)                  # (d)
    assert h[8] <= 16 and h[11] == n * G * W and len(shards) == h[11]
    for (p, r, g, k), bts in shards.items():
        assert p == 0 and bytes(want[(r, g)][k]) == bts, (p, r, g, k)
    c = RSPaxosPayloadStore(G, n, W, 64, num_data_shards=d)                  # (b), into a third geometry
    c.load(PayloadStoreSnapshot(c).import_(ia))
    stores_equal(c, a, "round trip")
    assert c.save().export() == ia
    _close([a, b, c, sa, sb])


def hand_built_store_image(dev, G=66, W=8, n=3, d=2):
    """a store image written in numpy from DESIGN.md 2's table alone (no kernel wrote any of it) -- two tiles, so that a VOTED cell
    of tile 0 stands in front of a REQS cell of tile 1; a full codeword; a vote that is wholly an alias of the REQS row; a vote
    with one shard aliased and one stored; a LONE vote, whose REQS cell is empty; the empty batch (token 0, one byte); shard
    lengths of 1, 3, 10, 19 and 32 bytes (padding of 15 .. 0) -- is imported and loaded into fresh stores of two geometries:
    dump / read_row / voted_alias / counters give what was written, and the store's own next image is these bytes"""
    from summerset_amd import PayloadStoreSnapshot, RSPaxosPayloadStore
    lay = StoreLayout(G, W, 2)
    rng = np.random.default_rng(17)
    # (plane, row, group) -> (token, dlen, avail, alias)
    cells = {(0, 1, 0): (77, 37, 0b111, 0), (1, 1, 0): (77, 37, 0b010, 0b010),          # a steady tick's vote: an alias
             (0, 3, 0): (99, 64, 0b101, 0), (1, 3, 0): (99, 64, 0b011, 0b001),          # one shard aliased, one stored
             (1, 2, 1): (88, 5, 0b100, 0),                                              # a lone vote: the REQS cell is empty
             (0, 7, 2): (0, 1, 0b001, 0),                                               # ReqBatch::new(): one byte
             (0, 0, 65): (5, 20, 0b110, 0), (1, 5, 64): (6, 20, 0b001, 0)}              # the second tile
    arr = {key: np.zeros((W, G), dt) for key, (_, _, dt) in lay.at.items()}
    for p in range(2):
        arr[("tok", p)][:] = NULL
    body, shards = bytearray(), {}
    for p, r, g in sorted(cells, key=lambda c: (c[2] // 64, c[0], c[1], c[2])):          # tile, plane, ring row, group
        tok, dlen, av, al = cells[(p, r, g)]
        arr[("tok", p)][r, g], arr[("dlen", p)][r, g], arr[("avail", p)][r, g] = tok, dlen, av
        if p == 1:
            arr[("alias", 1)][r, g] = al
        sl = (dlen + d - 1) // d
        for k in range(n):                                                   # every shard present and no alias, ascending
            if ((av & ~al) >> k) & 1:
                shards[(p, r, g, k)] = rng.integers(1, 256, sl, dtype=np.uint8).tobytes()
                body += shards[(p, r, g, k)] + bytes(a16(sl) - sl)
    assert len(shards) == 11 and len(body) == 3 * 32 + 2 * 32 + 32 + 16 + 16 + 2 * 16 + 16
    img = bytearray(lay.fixed)
    ctr = [1000, 20, 0, 3, 400]                                              # copied, rebuilt, unsatisfied, rekeyed, delivered
    struct.pack_into("<5Q", img, 64, *ctr)
    for key, (off, nb, dt) in lay.at.items():
        img[off:off + nb] = arr[key].astype(dt).tobytes()
    img += body
    struct.pack_into(PS_HDR, img, 0, PS_MAGIC, 1, G, W, n, d, 2, 0, 64, len(img), len(cells), len(shards), len(body), 0)
    img = bytes(img)
    for L in (64, 200):                                                      # max_data_len == max_dlen, and another cap_sl
        st = RSPaxosPayloadStore(G, n, W, L, num_data_shards=d)
        snap = PayloadStoreSnapshot(st).import_(img)
        assert snap.info() == dict(bytes=len(img), n_cells=8, n_shards_stored=11, shard_bytes=len(body), n_groups=G, window=W, max_dlen=64, n_shards=n,
                                   n_data_shards=d, planes=2, craft=0)
        st.load(snap)
        assert st.counters() == dict(copied=1000, rebuilt=20, unsatisfied=0, rekeyed=3) and st.delivered() == 400
        assert np.array_equal(st.voted_alias(), arr[("alias", 1)])
        for p in range(2):
            dmp = st.dump(p)
            for name in ("tok", "dlen", "avail"):
                assert np.array_equal(dmp[name], arr[(name, p)]), (L, p, name)
        rows = {(p, r): st.read_row(r, p) for p, r, _ in cells}
        for (p, r, g, k), bts in shards.items():
            assert rows[(p, r)][k, g, :len(bts)].tobytes() == bts, (L, p, r, g, k)
        for (p, r, g), (tok, dlen, av, al) in cells.items():                 # an aliased vote reads as the REQS cell's shard
            for k in range(n):
                if (al >> k) & 1:
                    bts = shards[(0, r, g, k)]
                    assert rows[(1, r)][k, g, :len(bts)].tobytes() == bts, (L, "alias", r, g, k)
        assert st.save().export() == img, L
        _close([st, snap])


def store_stream_order(dev, oracle, G=70, n=5, W=8, L=333):
    """the store's two launches enqueued directly behind a `put` on the same stream and in front of the next one, no
    host synchronisation in between (the header launch writes the offsets the byte launch reads: they rely on stream order too).
    The image is the state at the save point: every shard the oracle's encoder's, of the tokens put BEFORE the save"""
    import torch
    from summerset_amd import RSPaxosPayloadStore
    rng = np.random.default_rng(23)
    d = n // 2 + 1
    st = RSPaxosPayloadStore(G, n, W, L)
    datas = [rng.integers(1, 256, (G, L), dtype=np.uint8) for _ in range(W + 3)]
    dv = [torch.from_numpy(x).to(dev) for x in datas]
    accs = []
    for t in range(len(datas)):                                              # everything is on the device before the first call
        a_slot, a_val = np.zeros((W, G), np.int32), np.zeros((W, G), np.int32)
        a_slot[0], a_val[0] = t, 1 + t * G + np.arange(G)
        accs.append(dict(a_n=torch.ones(G, dtype=torch.int32, device=dev), a_slot=torch.from_numpy(a_slot).to(dev), a_val=torch.from_numpy(a_val).to(dev)))
    t_save, snap = W + 2, None                                               # rows 0 and 1 hold their second payload at the save
    for t in range(len(datas)):
        st.put(accs[t], dv[t])
        if t + 1 == t_save:
            snap = st.save()                                                 # no synchronisation in front, none behind
    h, ctr, arr, shards = StoreLayout(G, W, 2).parse(snap.export(), d)
    want_tok = np.full((W, G), NULL, np.uint32)
    for t in range(t_save):
        want_tok[t & (W - 1)] = 1 + t * G + np.arange(G)
    assert np.array_equal(arr[("tok", 0)], want_tok) and (arr[("dlen", 0)] == L).all() and (arr[("avail", 0)] == (1 << n) - 1).all()
    assert h[11] == len(shards) == n * G * W
    for (p, r, g, k), bts in shards.items():
        if g % 7 == 0:
            t = r if r + W >= t_save else r + W
            cw = np.zeros((n, (L + d - 1) // d), np.uint8)
            cw[:d].reshape(-1)[:L] = datas[t][g]
            cw[d:] = oracle.rs_encode(d, n - d, datas[t][g])
            assert p == 0 and bytes(cw[k]) == bts, (r, g, k)
    assert (st.dump(0)["tok"][2] == 1 + (W + 2) * G + np.arange(G)).all()    # ... and the store itself went on
    _close([st, snap])


def store_refusals(dev, oracle, G=40, W=8, L=61):
    """SMR_ERR_ARG and the target's state unchanged: a store of another n, d, W, G or kind (both ways); a store whose max_data_len
    is below the image's max_dlen; an export buffer too small; imports truncated at every section boundary and one byte short,
    with a wrong magic or version, with counts that contradict the cell headers, with a non-zero pad byte"""
    import ctypes as C
    import torch
    from summerset_amd import CRaftPayloadStore, PayloadStoreSnapshot, RSPaxosPayloadStore, SummersetError, _lib
    Lb = _lib.load()

    def refused(f, word=None, code=-1):
        try:
            f()
        except SummersetError as err:
            assert err.code == code and (word is None or word in str(err)), (word, err)
            return
        raise AssertionError("not refused: %s" % word)
    t = lambda x: torch.from_numpy(np.ascontiguousarray(x)).to(dev)
    a = RSPaxosPayloadStore(G, 5, W, L)
    rng = np.random.default_rng(9)
    for slot in range(3):
        a_slot, a_val = np.zeros((W, G), np.uint32), np.zeros((W, G), np.uint32)
        a_slot[0], a_val[0] = slot, 1 + slot * G + np.arange(G)
        a.put(dict(a_n=t(np.ones(G, np.int32)), a_slot=t(a_slot.view(np.int32)), a_val=t(a_val.view(np.int32))), t(rng.integers(0, 256, (G, L), dtype=np.uint8)),
              t(rng.integers(1, L + 1, G).astype(np.int32)))
    snap = a.save()
    image = snap.export()
    info = snap.info()
    assert info["n_cells"] == 3 * G and info["n_shards_stored"] == 15 * G and info["max_dlen"] > 16
    others = dict(n=RSPaxosPayloadStore(G, 7, W, L, num_data_shards=3), d=RSPaxosPayloadStore(G, 5, W, L, num_data_shards=2), W=RSPaxosPayloadStore(G, 5, 2 * W, L),
                  G=RSPaxosPayloadStore(G + 1, 5, W, L), kind=CRaftPayloadStore(G, 5, W, L))
    planes = lambda s: 1 if isinstance(s, CRaftPayloadStore) else 2
    state = lambda s: ([s.dump(p) for p in range(planes(s))], s.counters())

    def same_state(x, y):
        return x[1] == y[1] and all(np.array_equal(p[k], q[k]) for p, q in zip(x[0], y[0]) for k in p)
    for what, b in others.items():
        before = state(b)
        refused(lambda: b.load(snap), "made for")
        refused(lambda: b.save(snap), "made for")
        refused(lambda: PayloadStoreSnapshot(b).import_(image), "the image is of")
        assert same_state(state(b), before), what
    cs = others["kind"].save()
    before = state(a)
    refused(lambda: a.load(cs), "made for")                                  # ... and a CRaft image into the RSPaxos store
    refused(lambda: PayloadStoreSnapshot(a).import_(cs.export()), "the image is of")
    small = RSPaxosPayloadStore(G, 5, W, info["max_dlen"] - 1)
    sb = state(small)
    refused(lambda: small.load(snap), "max_data_len")
    refused(lambda: small.load(PayloadStoreSnapshot(small).import_(image)), "max_data_len")
    assert same_state(state(small), sb) and same_state(state(a), before)
    assert snap.export() == image
    n = info["bytes"]
    buf = (C.c_uint8 * n)()
    assert int(Lb.smr_rsp_pstore_snapshot_export(snap._h, buf, n - 1)) == -1 and b"takes" in Lb.smr_last_error()
    assert int(Lb.smr_rsp_pstore_snapshot_export(snap._h, buf, n)) == n and bytes(buf) == image
    empty = PayloadStoreSnapshot(a)
    refused(lambda: a.load(empty), "nothing saved", code=-3)
    lay = StoreLayout(G, W, 2)
    target = PayloadStoreSnapshot(a)
    cuts = sorted({64, 104, lay.hdr_end, lay.fixed, len(image)} | {o + a8(nb) for o, nb, _ in lay.at.values()})
    for cut in cuts:
        for ln in (cut - 1, cut) if cut == len(image) else (cut, cut - 1):
            if ln < len(image):
                refused(lambda: target.import_(image[:ln]))
    for off, val in ((0, 0x54), (4, 2), (8, 1), (12, 1), (16, 1), (17, 1), (18, 1), (19, 1), (20, 0xFF), (24, 1), (32, 1), (40, 1), (48, 16), (56, 1)):
        bad = bytearray(image); bad[off] = (bad[off] + val) & 0xFF           # magic, version, G, W, n, d, planes, craft, max_dlen, bytes, n_cells,
        refused(lambda: target.import_(bytes(bad)))                           # n_shards_stored, shard_bytes, reserved
    bad = bytearray(image); struct.pack_into("<I", bad, 0, PS_MAGIC ^ 1)
    refused(lambda: target.import_(bytes(bad)), "magic")
    bad = bytearray(image); struct.pack_into("<I", bad, 4, 2)
    refused(lambda: target.import_(bytes(bad)), "version")
    o_dlen, o_av, o_tok = lay.at[("dlen", 0)][0], lay.at[("avail", 0)][0], lay.at[("tok", 0)][0]
    bad = bytearray(image); struct.pack_into("<I", bad, o_dlen, struct.unpack_from("<I", image, o_dlen)[0] + 48)      # a longer shard: more bytes than held
    refused(lambda: target.import_(bytes(bad)), "malformed")
    bad = bytearray(image); bad[o_av] = 0x0F                                 # one shard fewer than the counts say
    refused(lambda: target.import_(bytes(bad)), "malformed")
    bad = bytearray(image); bad[o_av] = 0x3F                                 # a sixth shard of five
    refused(lambda: target.import_(bytes(bad)), "malformed")
    bad = bytearray(image); bad[o_av + 3 * G] = 1                            # a cell without a token that holds something
    refused(lambda: target.import_(bytes(bad)), "malformed")
    pads = [p for off, nb, _ in lay.at.values() for p in range(off + nb, off + a8(nb))] + list(range(lay.hdr_end, lay.fixed))
    sl0 = (struct.unpack_from("<I", image, o_dlen)[0] + 2) // 3
    if sl0 % 16:
        pads.append(lay.fixed + sl0)                                         # the first shard's own padding
    for p in pads:
        bad = bytearray(image); bad[p] = 1
        refused(lambda: target.import_(bytes(bad)), "padding")
    target.import_(image)
    assert target.export() == image
    fresh = RSPaxosPayloadStore(G, 5, W, L + 7)
    fresh.load(target)
    stores_equal(fresh, a, "fresh")
    _close(list(others.values()) + [a, snap, cs, small, empty, target, fresh])


def store_grows(dev, oracle, G=40, W=8):
    """a snapshot made from a store of max_data_len 32 takes a store of max_data_len 1000 full of long payloads: it grows in the save"""
    import torch
    from summerset_amd import PayloadStoreSnapshot, RSPaxosPayloadStore
    t = lambda x: torch.from_numpy(np.ascontiguousarray(x)).to(dev)
    small, big = RSPaxosPayloadStore(G, 5, W, 32), RSPaxosPayloadStore(G, 5, W, 1000)
    snap = PayloadStoreSnapshot(small)
    small.save(snap)
    assert snap.info()["shard_bytes"] == 0
    rng = np.random.default_rng(3)
    for slot in range(W):
        a_slot, a_val = np.zeros((W, G), np.uint32), np.zeros((W, G), np.uint32)
        a_slot[0], a_val[0] = slot, 1 + slot * G + np.arange(G)
        big.put(dict(a_n=t(np.ones(G, np.int32)), a_slot=t(a_slot.view(np.int32)), a_val=t(a_val.view(np.int32))), t(rng.integers(0, 256, (G, 1000), dtype=np.uint8)))
    big.save(snap)
    assert snap.info()["shard_bytes"] == G * W * 5 * a16((1000 + 2) // 3) > 2 * G * W * 5 * 16
    fresh = RSPaxosPayloadStore(G, 5, W, 1000)
    fresh.load(snap)
    stores_equal(fresh, big, "grown")
    _close([small, big, snap, fresh])


def craft_shadow_stores(dev, oracle, R, G=40, W=8, L=200, T=14):
    """tests/craft_payload_loop.Loop (the last follower cut off for three ticks and catching up, the ring wrapping); after EVERY
    tick each replica goes through a RaftSnapshot and its one-plane store through the store snapshot into spares (stores of
    max_data_len L and L + 100 take turns), which are swapped in; `lp.check` (engine, store, the oracle's codewords) on every replica"""
    import craft_payload_loop as cl
    from summerset_amd import CRaftLeaderGroup, CRaftPayloadStore, PayloadStoreSnapshot, RaftSnapshot
    lp = cl.Loop(dev, oracle, G=G, R=R, W=W, L=L, seed=3, many=False)
    sp_rep = [CRaftLeaderGroup(G, R, leader_id=r, window=W, term=1, fault_tolerance=1) for r in range(R)]
    sp_st = [CRaftPayloadStore(G, R, W, max_data_len=L + 100) for _ in range(R)]
    rs, ps = [RaftSnapshot(x) for x in lp.reps], [PayloadStoreSnapshot(x) for x in lp.stores]
    moved = 0
    for t in range(T):
        lp.tick(p_new=1.0, skip=(R - 1,) if 3 <= t <= 5 else ())
        for r in range(R):
            lp.reps[r].save_state(rs[r]); sp_rep[r].load_state(rs[r])
            lp.stores[r].save(ps[r]); sp_st[r].load(ps[r])
            info = ps[r].info()
            assert info["planes"] == 1 and info["craft"] == 1
            moved += info["shard_bytes"]
            assert lp.stores[r].counters() == sp_st[r].counters()
            lp.reps[r], sp_rep[r] = sp_rep[r], lp.reps[r]
            lp.stores[r], sp_st[r] = sp_st[r], lp.stores[r]
            lp.check(r, (t, r))
    assert int(lp.reps[0].dump()["log_len"].max()) > W and moved > 0
    assert sum(int(s.counters()["rekeyed"]) for s in lp.stores) > 0 and sum(s.counters()["unsatisfied"] for s in lp.stores) == 0
    assert lp.checked_cells > 1000 and lp.checked_shards > lp.checked_cells
    return lp


def store_past_4gib(dev, oracle, n=3, d=2, G=4096, W=8, L=88000):
    """device only: eight puts fill every row with every shard of 88 000-byte payloads -- 4096 x 8 x 3 shards of 44 000 bytes are
    4.3 GB, so the image's last shards lie past 2^32.  The store is saved, loaded into a second one, and sampled cells on both sides
    of 4 GiB are held against the oracle's encoder; the image's size is arithmetic"""
    import torch
    from summerset_amd import PayloadStoreSnapshot, RSPaxosPayloadStore
    sl = (L + d - 1) // d
    total = G * W * n * a16(sl)
    assert total > 2**32
    a = RSPaxosPayloadStore(G, n, W, L, num_data_shards=d)
    gen = torch.Generator(device=dev); gen.manual_seed(11)
    data = torch.randint(0, 256, (G, L), dtype=torch.uint8, device=dev, generator=gen)
    ones = torch.ones(G, dtype=torch.int32, device=dev)
    for slot in range(W):
        a_slot = torch.zeros((W, G), dtype=torch.int32, device=dev); a_slot[0] = slot
        a_val = torch.zeros((W, G), dtype=torch.int32, device=dev); a_val[0] = torch.arange(G, dtype=torch.int32, device=dev) + 1 + slot * G
        a.put(dict(a_n=ones, a_slot=a_slot, a_val=a_val), data.roll(slot, 1))
    snap = a.save()
    info = snap.info()
    assert info["shard_bytes"] == total and info["n_shards_stored"] == G * W * n and info["bytes"] == StoreLayout(G, W, 2).fixed + total
    del a_slot, a_val
    a_rows = {w: a.read_row(w, 0) for w in (0, W - 1)}
    a.close()                                                                # (two stores and the image do not fit beside each other comfortably)
    b = RSPaxosPayloadStore(G, n, W, L, num_data_shards=d)
    b.load(snap)
    hd = b.dump(0)
    assert (hd["avail"] == (1 << n) - 1).all() and (hd["dlen"] == L).all()
    host = data.cpu().numpy()
    for w in (0, W - 1):                                                     # tile-major: the last tiles' shards are the ones past 4 GiB
        row = b.read_row(w, 0)
        assert np.array_equal(row[:, :, :sl], a_rows[w][:, :, :sl])
        for g in (0, 1, G // 2, G - 65, G - 1):
            bts = np.roll(host[g], w)
            cw = np.zeros((n, sl), np.uint8)
            cw[:d].reshape(-1)[:L] = bts
            cw[d:] = oracle.rs_encode(d, n - d, bts)
            assert np.array_equal(row[:, g, :sl], cw), (w, g)
    _close([b, snap])


def store_more_tiles_than_wavefronts(dev, oracle, n=3, d=2, G=66000, W=8, L=16):
    """device only: 66 000 groups are 1 032 tiles for the header kernel's 1 024 wavefronts, so every wavefront takes two tiles
    (the last ones one or none) and a cell's offset is a sum over tiles of its own wavefront, of its block and of the blocks in
    front.  One put per ring row of 16-byte payloads (66 000 x 8 x 3 shards of 8 bytes, 16 in the image: 25 MB); the store is
    saved, loaded into a second one, the two are equal, and sampled shards on both sides of tile, wavefront and block edges are the
    oracle's encoder's; the image's size is arithmetic"""
    import torch
    from summerset_amd import RSPaxosPayloadStore
    assert (G + 63) // 64 > 1024
    sl = (L + d - 1) // d
    a, b = RSPaxosPayloadStore(G, n, W, L, num_data_shards=d), RSPaxosPayloadStore(G, n, W, L + 100, num_data_shards=d)
    gen = torch.Generator(device=dev); gen.manual_seed(13)
    data = torch.randint(0, 256, (G, L), dtype=torch.uint8, device=dev, generator=gen)
    ones = torch.ones(G, dtype=torch.int32, device=dev)
    for slot in range(W):
        a_slot = torch.zeros((W, G), dtype=torch.int32, device=dev); a_slot[0] = slot
        a_val = torch.zeros((W, G), dtype=torch.int32, device=dev); a_val[0] = torch.arange(G, dtype=torch.int32, device=dev) + 1 + slot * G
        a.put(dict(a_n=ones, a_slot=a_slot, a_val=a_val), data.roll(slot, 1))
    snap = a.save()
    info = snap.info()
    total = G * W * n * a16(sl)
    assert info["shard_bytes"] == total and info["n_shards_stored"] == G * W * n and info["n_cells"] == G * W and info["max_dlen"] == L, info
    assert info["bytes"] == StoreLayout(G, W, 2).fixed + total
    b.load(snap)
    stores_equal(b, a, "more tiles than wavefronts")
    host = data.cpu().numpy()
    for w in (0, W - 1):
        row = b.read_row(w, 0)
        for g in (0, 63, 64, 127, 128, 511, 512, G // 2, 65535, 65536, G - 17, G - 16, G - 1):   # tiles, wavefronts (128 groups), blocks (512)
            bts = np.roll(host[g], w)
            cw = np.zeros((n, sl), np.uint8)
            cw[:d].reshape(-1)[:L] = bts
            cw[d:] = oracle.rs_encode(d, n - d, bts)
            assert np.array_equal(row[:, g, :sl], cw), (w, g)
    _close([a, b, snap])
