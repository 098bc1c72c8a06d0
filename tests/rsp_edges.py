"""The RSPaxos engine (csrc/rsp_engine.hip) and the payload stores (csrc/rsp_payload.hip) away from five replicas, leader 0 and
ballots below 2^12: the bodies of tests/test_zzzz_rsp_edges_gpu.py (the device) and of tests/test_hostsim.py's
`test_rspaxos_edges_*` (the kernel-source emulator, smaller), every size an argument.

Everything is bit-exact: engines against `oracle.RspOracle` after every tick -- every message dict, `take_executed()`, the full
`dump()` of every replica -- and shard bytes against `oracle.rs_encode` / `rs_shard_len`.  Every body first asserts ON THE ORACLE
CLUSTER ALONE that its schedule reached what it is for (voted PrepareReply rows, re-Accepts, empty re-Accepts, reconstruction
rows, commits at the three replicas that lead, redirects, no absorb of a different token, ballots on both sides of a power of
two, a wrapped ring): conditions of the schedule, not measurements of the engine.

  populations   the closed loop of tests/rsp_scenarios.py with R in 3..8: quorum = majority + ft, uint8 masks with every bit in use
  wide ballots  no preset: a first Heartbeat at round0 << 8, then step-ups whose ballots cross 2^32 / 2^63 (uint64 in the engine,
                int64 tensors at the binding, LDS in the one-launch tick)
  past the ring leader changes on logs that have wrapped several times
  steady tick   `SteadyLoop`, call by call and as ONE launch (`rsp_cluster_tick_kernel`: a block of R * 64 threads, wavefront q =
                replica q), with leaders that are not wavefront 0
  schemes       the payload stores at every (n, d) the put kernels are instantiated for"""
import numpy as np

import rsp_cluster as rc
import rsp_scenarios as sc

NULL, NO_REP = rc.NULL, rc.NO_REP
KINDS = ("accept", "accept_reply", "prepare", "prepare_reply", "recon", "recon_reply", "hb")


# ---- closed loops: R oracles first (what the schedule reaches), then R engines against their per-tick record ---------------------
def first_heartbeat(reps, peer, round0):
    """every replica but `peer` hears a Heartbeat from it with ballot (round0 << 8) | (peer + 1) and zero bars: the only way to a
    wide ballot is through the handlers (there is no preset for it)"""
    G = reps[0].G
    out = []
    for r in range(len(reps)):
        if r == peer:
            continue
        rp = reps[r].heartbeat(flags=np.ones(G, np.uint8), peer=np.full(G, peer, np.uint8), ballot=np.full(G, (round0 << 8) | (peer + 1), np.uint64),
                               commit_bar=np.zeros(G, np.uint32), exec_bar=np.zeros(G, np.uint32), snap_bar=np.zeros(G, np.uint32))
        out.append(dict(kind="first_heartbeat", q=r, **rp))
    return out


def wide_schedule(reps, G, T, seed, loss, round0, on_tick=None):
    """nobody is preset.  Before tick 0 the first Heartbeat (peer 1, round0); tick 0: replica 0 times out on 1 in every group (a
    full Prepare phase at round0 + 1); tick 6: replica 1 times out on 0 in the even groups (round0 + 2), the batches follow at tick
    7; tick 12: replica 2 times out as in rsp_scenarios.run (round0 + 3 / round0 + 2), the batches follow at tick 13.  Heartbeats
    every third tick, every message kind lost at `loss`."""
    R = len(reps)
    log = [(-1, first_heartbeat(reps, 1, round0))]
    rng = np.random.default_rng(seed)
    target = np.zeros(G, np.uint8)
    g = np.arange(G)
    none = lambda: [np.full(G, NO_REP, np.uint8) for _ in range(R)]
    for t in range(T):
        val = (1 + t * G + g).astype(np.uint32)
        val[rng.random(G) < 0.1] = NULL
        to = None
        if t == 0:
            to = none(); to[0][:] = 1
        if t == 6:
            to = none(); to[1] = np.where(g % 2 == 0, 0, NO_REP).astype(np.uint8)
        if t == 7:
            target = np.where(g % 2 == 0, 1, target).astype(np.uint8)
        if t == 12:
            to = none(); to[2] = np.where(g % 4 == 0, 1, np.where(g % 4 == 1, 0, NO_REP)).astype(np.uint8)
        if t == 13:
            target = np.where(g % 4 <= 1, 2, target).astype(np.uint8)
        drop = {(k, s, q): rng.random(G) < loss for k in KINDS for s in range(R) for q in range(R) if s != q} if loss else None
        log.append((t, rc.tick(reps, val, target, timeouts=to, drop=drop, heartbeat=(t % 3 == 2))))
        if on_tick:
            on_tick(t)
    return log


def oracle_run(oracle, schedule, G, R, W, ft):
    """schedule(reps, on_tick) -> log on R oracles: (oracles, log, per-tick dumps, per-tick executed lists)"""
    orcs = [oracle.RspOracle(G, R, me=r, W=W, fault_tolerance=ft) for r in range(R)]
    snaps, execd = [], []
    lo = schedule(orcs, lambda t: (snaps.append([o.dump() for o in orcs]), execd.append([o.take_executed() for o in orcs])))
    return orcs, lo, snaps, execd


def engine_run(dev, schedule, G, R, W, ft, lo, snaps, execd):
    """the same schedule on R engines: after every tick every replica's executed list and full state, then every message"""
    from summerset_amd import RSPaxosReplicaGroup
    engs = [rc.NumpyEngine(RSPaxosReplicaGroup(G, R, me=r, window=W, fault_tolerance=ft), dev) for r in range(R)]
    step = [0]

    def check(t):
        for r in range(R):
            got, want = engs[r].take_executed(), execd[t][r]
            for x, y in zip(got, want):
                assert np.array_equal(x, y), (t, r, "executed", len(x), len(y))
            a, b = engs[r].dump(), snaps[t][r]
            for n in b:
                assert np.array_equal(a[n], b[n]), (t, r, n, [x[:4] for x in np.nonzero(a[n] != b[n])])
        step[0] += 1
    le = schedule(engs, check)
    assert step[0] == len(snaps) and len(le) == len(lo)
    for (t, a), (_, b) in zip(le, lo):
        assert len(a) == len(b), t
        for x, y in zip(a, b):
            for k in y:
                assert np.array_equal(x[k], y[k]) if isinstance(y[k], np.ndarray) else x[k] == y[k], (t, y["kind"], k)


def reach(orcs, lo):
    ev = [e for _, out in lo for e in out]
    c = [o.dump()["counters"] for o in orcs]
    return dict(voted=sum(e["voted"] for e in ev if e["kind"] == "prepare_reply"), re_accept=sum(e["n"] for e in ev if e["kind"] == "re_accept"),
                empty=sum(e["empty"] for e in ev if e["kind"] == "re_accept"), recon=sum(e["rows"] for e in ev if e["kind"] == "recon_reply"),
                committed=sum(int(e["committed"].sum()) for e in ev if e["kind"] == "commit"),
                commits=[int(x[0]) for x in c], mixed=[int(x[2]) for x in c], redirects=[int(x[3]) for x in c],
                longest=max(int(o.dump()["len"].max()) for o in orcs))


def assert_reached_every_rare_path(cov, redirects=True):
    assert cov["voted"] > 0 and cov["re_accept"] > 0 and cov["empty"] > 0 and cov["recon"] > 0, cov
    assert min(cov["commits"][:3]) > 0 and cov["committed"] > 0 and not any(cov["mixed"]), cov
    if redirects:
        assert cov["redirects"][1] > 0 or cov["redirects"][2] > 0, cov


def run_populations(dev, oracle, R, ft, G, W=8, loss=0.1, T=21, seed=None):
    """A: rsp_scenarios.run (steady appends, loss on all seven kinds, two leader changes) on R engines"""
    schedule = lambda reps, on_tick: sc.run(reps, G, T, seed=G + ft if seed is None else seed, loss=loss, on_tick=on_tick)
    orcs, lo, snaps, execd = oracle_run(oracle, schedule, G, R, W, ft)
    cov = reach(orcs, lo)
    assert_reached_every_rare_path(cov)
    engine_run(dev, schedule, G, R, W, ft, lo, snaps, execd)
    return cov


def run_past_the_ring(dev, oracle, R, ft, G, W=8, loss=0.1, T=44, seed=None):
    """C: the same loop long enough that both leader changes fall on logs that have wrapped"""
    schedule = lambda reps, on_tick: sc.run(reps, G, T, seed=G + ft if seed is None else seed, loss=loss, on_tick=on_tick)
    orcs, lo, snaps, execd = oracle_run(oracle, schedule, G, R, W, ft)
    cov = reach(orcs, lo)
    assert_reached_every_rare_path(cov)
    assert cov["longest"] >= 5 * W, cov
    g = np.arange(G)
    # the log of the replica that steps up, in the groups where it does, at the end of the tick before: past the ring in all of them
    assert (snaps[T // 3 - 1][1]["len"][g % 2 == 0] > W).all() and (snaps[2 * T // 3 - 1][2]["len"][g % 4 <= 1] > W).all()
    ev = {t: out for t, out in lo}
    for t in (T // 3, 2 * T // 3):                                           # ... and the step-ups happened there: Prepare replies came back
        assert sum(e["rows"] for e in ev[t] if e["kind"] == "prepare_reply") > 0, t
    engine_run(dev, schedule, G, R, W, ft, lo, snaps, execd)
    return cov


def run_wide_ballots(dev, oracle, round0, R, ft, W, G=130, T=18, loss=0.1, seed=None):
    """B: `wide_schedule`; the step-ups run from round0 + 1 to round0 + 3, so round0 = 2^24 - 2 / 2^55 - 2 puts ballots on both sides
    of 2^32 / 2^63 (a ballot is round << 8 | id + 1)"""
    schedule = lambda reps, on_tick: wide_schedule(reps, G, T, G + ft if seed is None else seed, loss, round0, on_tick)
    orcs, lo, snaps, execd = oracle_run(oracle, schedule, G, R, W, ft)
    cov = reach(orcs, lo)
    assert_reached_every_rare_path(cov, redirects=False)
    edge = np.uint64(((round0 + 2) << 8) & ~0xFF)                            # the first power of two above round0 << 8: 2^32 or 2^63
    assert int(edge) in (2**32, 2**63), hex(int(edge))
    bms = np.concatenate([o.dump()["bal_max_seen"] for o in orcs])
    assert bms.min() == np.uint64(((round0 + 1) << 8) | 1) and bms.max() == np.uint64(((round0 + 3) << 8) | 3), (hex(int(bms.min())), hex(int(bms.max())))
    assert (bms < edge).any() and (bms >= edge).any()
    vb = np.concatenate([o.dump()["s_vbal"].reshape(-1) for o in orcs])
    vb = vb[vb != 0]
    if int(edge) == 2**32:
        assert (vb < edge).any() and (vb >= edge).any()
    engine_run(dev, schedule, G, R, W, ft, lo, snaps, execd)
    return cov


def run_random_calls(dev, oracle, R, me, ft, G=150, W=8, steps=120, round0=None):
    """tests/test_zz_rsp_gpu.py's differential body (tests/rsp_random.py: seeded random, not protocol-legal calls) at population R;
    round0: from a wide start -- engine and oracle first hear one Heartbeat of peer (me + 1) % R at round0"""
    import rsp_random as rr
    from summerset_amd import RSPaxosReplicaGroup
    eng = rc.NumpyEngine(RSPaxosReplicaGroup(G, R, me=me, window=W, fault_tolerance=ft), dev)
    orc = oracle.RspOracle(G, R, me=me, W=W, fault_tolerance=ft)
    eng.preset_leader(0); orc.preset_leader(0)

    def same(where):
        for x, y in zip(eng.take_executed(), orc.take_executed()):
            assert np.array_equal(x, y), (where, "executed", len(x), len(y))
        a, b = eng.dump(), orc.dump()
        for n in b:
            assert np.array_equal(a[n], b[n]), (where, n, [x[:4] for x in np.nonzero(a[n] != b[n])])
    if round0 is not None:
        p = (me + 1) % R
        hb = dict(flags=np.ones(G, np.uint8), peer=np.full(G, p, np.uint8), ballot=np.full(G, (round0 << 8) | (p + 1), np.uint64),
                  commit_bar=np.zeros(G, np.uint32), exec_bar=np.zeros(G, np.uint32), snap_bar=np.zeros(G, np.uint32))
        a, b = eng.heartbeat(**hb), orc.heartbeat(**hb)
        for k in b:
            assert np.array_equal(a[k], b[k]), ("first heartbeat", k)
        same("first heartbeat")
        assert (orc.dump()["bal_max_seen"] == np.uint64((round0 << 8) | (p + 1))).all()
    rng = np.random.default_rng(G + W + me)
    seen = set()
    for step in range(steps):
        for name, kw in rr.calls(rng, orc.dump(), G, R, me, W):
            seen.add(name)
            a, b = getattr(eng, name)(**kw), getattr(orc, name)(**kw)
            if b is not None:
                for k in b:
                    assert np.array_equal(a[k], b[k]), (step, name, k, [x[:4] for x in np.nonzero(a[k] != b[k])])
            same((step, name))
    assert len(seen) == 10, seen
    d = orc.dump()                                                           # (with a quorum of all eight, random replies commit nothing)
    if round0 is not None:                                                   # the step-ups went on from the wide start: across 2^32 / 2^63
        assert d["bal_max_seen"].max() > np.uint64(((round0 + 1) << 8)), hex(int(d["bal_max_seen"].max()))
    return d


# ---- the steady tick ---------------------------------------------------------------------------------------------------------
def wide_start(dev, leader, round0):
    """`run_steady`'s start: the first Heartbeat of peer (leader + 1) % R at round0, then one tick of the closed loop in which
    `leader` times out on that peer in every group -- Prepare phase at round0 + 1, no loss -- instead of `preset_leader`"""
    def start(engs, orcs):
        for reps in ([rc.NumpyEngine(e, dev) for e in engs], orcs):
            R, G = len(reps), reps[0].G
            p = (leader + 1) % R
            first_heartbeat(reps, p, round0)
            to = [np.full(G, NO_REP, np.uint8) for _ in range(R)]
            to[leader][:] = p
            rc.tick(reps, np.full(G, NULL, np.uint32), np.full(G, leader, np.uint8), timeouts=to)
        want = np.uint64(((round0 + 1) << 8) | (leader + 1))
        for o in orcs:
            d = o.dump()
            assert (d["leader"] == leader).all() and (d["bal_max_seen"] == want).all(), (o.me, hex(int(want)))
        d = orcs[leader].dump()
        assert (d["bal_prepared"] == want).all() and (d["bal_prep_sent"] == want).all()
        for e, o in zip(engs, orcs):
            a, b = e.dump(), o.dump()
            for n in b:
                assert np.array_equal(a[n], b[n]), ("start", o.me, n)
    return start


def run_steady_case(dev, oracle, R, leader, ft, G, one_launch, round0=None, W=8, loss=0.2, T=14):
    """D: tests/test_zz_rsp_steady_gpu.run_steady (the leader's commits of every tick and every replica's state at the end against
    R oracles in the numpy-staged loop) at population R under leader `leader`, T > W ticks"""
    import test_zz_rsp_steady_gpu as ts
    start = None if round0 is None else wide_start(dev, leader, round0)
    total = ts.run_steady(dev, oracle, G, W, ft, loss, T=T, hb_every=3, one_launch=one_launch, R=R, leader=leader, start=start)
    assert total > 0
    return total


# ---- the payload stores ------------------------------------------------------------------------------------------------------
def run_payload_closed_loop(dev, oracle, R, ft, L, G=40, W=8, loss=0.1, staging=False):
    """E.1: tests/test_zz_rsp_payload_gpu.run_closed_loop with R replicas: RS(majority, R - majority) stores behind every engine"""
    import test_zz_rsp_payload_gpu as tp
    tot, n_exec, n_cmp = tp.run_closed_loop(dev, oracle, G, W, ft, loss, L, staging=staging, R=R)
    assert tot["copied"] > 0 and tot["rebuilt"] > 0 and tot["unsatisfied"] == 0 and n_exec > 0 and n_cmp > 0, (tot, n_exec, n_cmp)
    return tot, n_exec, n_cmp


MAJORITY_SCHEMES = [(3, 2), (4, 3), (5, 3), (6, 4), (7, 4), (8, 5)]
OTHER_SCHEMES = [(2, 1), (3, 1), (8, 1), (8, 2), (6, 5), (7, 6), (8, 6), (8, 7)]     # with the above: every D in 1..7
SWEEP_LENGTHS = (1, 17, 133, 512)


def run_scheme_sweep(dev, oracle, n, d, L, G=40, W=8):
    """E.2: one store of scheme (n, d) without an engine: put -> every header and shard; extract with a mask per group; ingest into
    a second store; get_data.  Lengths around d and around the 16-byte columns of d shards, junk behind every batch's length"""
    import torch
    from summerset_amd import RSPaxosPayloadStore
    from summerset_amd.rsp_payload import REQS
    assert G >= 10
    rng = np.random.default_rng(1000 * n + 10 * d + L)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    full, dm = (1 << n) - 1, (1 << d) - 1
    slot, row, none = W + 3, (W + 3) & (W - 1), 8                           # group `none`: no Accept (a_n = 0)
    lens = rng.integers(1, L + 1, G).astype(np.uint32)
    lens[:6] = [1, L, min(L, d), min(L, 16 * d), min(L, 16 * d + 1), max(1, min(L, 16 * d - 1))]
    data = rng.integers(0, 256, (G, L), dtype=np.uint8)
    data[np.arange(L)[None, :] >= lens[:, None]] = 0x5A                      # bytes past a batch's length: must not reach a shard
    tok = (1000 + np.arange(G)).astype(np.uint32)
    a_n = np.ones(G, np.uint32); a_n[none] = 0
    a_slot, a_val = np.zeros((W, G), np.uint32), np.zeros((W, G), np.uint32)
    a_slot[0], a_val[0] = slot, tok
    on = a_n > 0
    cws = []
    for g in range(G):
        b = data[g, :lens[g]]
        sl = oracle.rs_shard_len(b.size, d)
        cw = np.zeros((n, sl), np.uint8)
        cw[:d].reshape(-1)[:b.size] = b
        cw[d:] = oracle.rs_encode(d, n - d, b)
        cws.append(cw)
    st, other = RSPaxosPayloadStore(G, n, W, L, num_data_shards=d), RSPaxosPayloadStore(G, n, W, L, num_data_shards=d)
    st.put(dict(a_n=t(a_n.view(np.int32)), a_slot=t(a_slot.view(np.int32)), a_val=t(a_val.view(np.int32))), t(data), t(lens.view(np.int32)))

    def check(store, mask, where):
        """row `row` of the REQS plane holds exactly `mask[g]` of token g's codeword; every other row nothing"""
        h = store.dump(REQS)
        want = np.zeros((W, G), np.uint8); want[row] = mask
        assert np.array_equal(h["avail"], want), (where, np.nonzero(h["avail"] != want))
        assert np.array_equal(h["tok"][row], np.where(mask != 0, tok, NULL)) and np.array_equal(h["dlen"][row], np.where(mask != 0, lens, 0)), where
        assert (np.delete(h["tok"], row, 0) == NULL).all(), where
        r = store.read_row(slot, REQS)
        for g in range(G):
            for k in range(n):
                if (mask[g] >> k) & 1:
                    assert np.array_equal(r[k, g, :cws[g].shape[1]], cws[g][k]), (where, g, k, int(lens[g]))
    check(st, np.where(on, full, 0).astype(np.uint8), "put")
    mask = rng.integers(0, full + 1, G).astype(np.uint8)
    mask[:8] = [full, dm, dm << (n - d), 1, full & ~(1 << (n - 1)), full & ~1, 0, full]
    slots = t(np.full(G, slot, np.int32))
    msg = st.extract(slots, t(mask), REQS)
    m = np.where(on, mask, 0).astype(np.uint8)
    got = {k: msg[k].cpu().numpy() for k in ("mask", "tok", "dlen", "buf")}
    assert np.array_equal(got["mask"], m)
    assert np.array_equal(got["tok"].view(np.uint32), np.where(m != 0, tok, NULL)) and np.array_equal(got["dlen"].view(np.uint32), np.where(m != 0, lens, 0))
    for g in range(G):
        for k in range(n):
            if (m[g] >> k) & 1:
                assert np.array_equal(got["buf"][k, g, :cws[g].shape[1]], cws[g][k]), ("extract", g, k)
    other.ingest(msg, slots, REQS)
    check(other, m, "ingest")
    for store, have in ((st, np.where(on, full, 0)), (other, m)):           # RSCodeword::get_data: all the data shards, or an error
        out, ln, ok = (x.cpu().numpy() for x in store.get_data(slots, expect=t(tok.view(np.int32))))
        assert np.array_equal(ok, (have & dm) == dm), (np.nonzero(ok != ((have & dm) == dm)))
        for g in np.nonzero(ok)[0]:
            assert ln[g] == lens[g] and np.array_equal(out[g, :lens[g]], data[g, :lens[g]]), ("get_data", g)
        assert not ln[~ok].any()
    assert st.counters()["unsatisfied"] == 0 and other.counters()["unsatisfied"] == 0


def run_one_call(dev, oracle, monkeypatch, R, G, L, T, seed, W=8, ft=1, loss=0.1):
    """E.3: tests/test_zzz_rsp_payload_one_call_gpu.run_three_arms (`put_follow_all`, deliver on and off, against the separate calls,
    the engines against R oracles, through leader changes) with R replicas: R - 1 followers in the put launch's `PsDeliver` -- seven
    at R = 8, its capacity.  The seed is one under which every coverage condition of that body holds (they are asserted there)."""
    import test_zzz_rsp_payload_one_call_gpu as t
    return t.run_three_arms(dev, oracle, monkeypatch, G, W, ft, loss, L, T, seed=seed, R=R)


def run_craft_stores(dev, oracle, R, many, G=40, W=8, L=200, T=14):
    """E.4: the CRaft stores (`ps_put_kernel<D, true>` / `ps_put_deliver_kernel<D, true>`, one plane) behind R replicas: the loop of
    tests/craft_payload_loop.py -- every tick an append in every group, the last follower cut off for three ticks and catching up,
    the ring wrapping -- every store against its engine and the oracle's codewords after every handler call.  many: False (put,
    follow per follower) or "one_call" (`put_follow_all`)"""
    import craft_payload_loop as cl
    lp = cl.Loop(dev, oracle, G=G, R=R, W=W, L=L, seed=3, many=many)
    for t in range(T):
        lp.tick(p_new=1.0, skip=(R - 1,) if 3 <= t <= 5 else ())
    ln = lp.reps[0].dump()["log_len"]
    assert int(ln.max()) > W and sum(int(s.counters()["rekeyed"]) for s in lp.stores) > 0
    for r in range(R):
        lp.check(r, ("end", r))
    assert lp.checked_cells > 1000 and lp.checked_shards > lp.checked_cells and lp.read_back(0, ln) > 0
    assert sum(s.counters()["unsatisfied"] for s in lp.stores) == 0
    if many == "one_call":
        assert all(s.delivered() > 0 for s in lp.stores[1:]) and lp.stores[0].delivered() == 0
    return lp


# ---- creation errors ---------------------------------------------------------------------------------------------------------
def creation_errors(dev):
    """F: refused before anything is allocated -- on a device the free memory is read around the refused calls, which ask for
    arenas of hundreds of megabytes"""
    import pytest
    import torch
    from summerset_amd import RSPaxosPayloadStore, RSPaxosReplicaGroup, SummersetError
    G, W, L = 1 << 16, 32, 4096
    on_device = getattr(dev, "type", dev) == "cuda"
    if on_device:
        torch.cuda.synchronize()
        free0 = torch.cuda.mem_get_info()[0]
    refused = [lambda: RSPaxosReplicaGroup(G, 2, me=0, window=W),
               lambda: RSPaxosReplicaGroup(G, 9, me=0, window=W),
               lambda: RSPaxosReplicaGroup(G, 5, me=5, window=W),
               lambda: RSPaxosReplicaGroup(G, 8, me=8, window=W)]
    for R in range(3, 9):                                                    # ft = population - majority + 1
        refused.append(lambda R=R: RSPaxosReplicaGroup(G, R, me=0, window=W, fault_tolerance=R - (R // 2 + 1) + 1))
    refused += [lambda: RSPaxosPayloadStore(G, 9, W, L),
                lambda: RSPaxosPayloadStore(G, 9, W, L, num_data_shards=5),
                lambda: RSPaxosPayloadStore(G, 5, W, L, num_data_shards=0),
                lambda: RSPaxosPayloadStore(G, 5, W, L, num_data_shards=5),
                lambda: RSPaxosPayloadStore(G, 8, W, L, num_data_shards=8)]
    for make in refused:
        with pytest.raises(SummersetError):
            make()
    if on_device:                                                            # the smallest of these arenas is 150 MB
        assert torch.cuda.mem_get_info()[0] > free0 - (64 << 20), (free0, torch.cuda.mem_get_info()[0])
    # a store whose d is not the replica's majority cannot follow it; nothing is written
    rep = RSPaxosReplicaGroup(16, 5, me=0, window=8)
    rep.preset_leader(0)
    acc = rep.req_batch(torch.ones(16, dtype=torch.int32, device=dev))
    for n, d in ((5, 2), (5, 4), (6, 4)):
        st = RSPaxosPayloadStore(16, n, 8, 64, num_data_shards=d)
        with pytest.raises(SummersetError):
            st.follow(rep)
        with pytest.raises(SummersetError):
            RSPaxosPayloadStore.follow_many([st], [rep])
        assert not st.dump(0)["avail"].any() and not st.dump(1)["avail"].any() and st.counters() == dict(copied=0, rebuilt=0, unsatisfied=0, rekeyed=0)
        st.close()
    ok = RSPaxosPayloadStore(16, 5, 8, 64)
    ok.put(acc, torch.zeros((16, 64), dtype=torch.uint8, device=dev))
    ok.follow(rep)                                                           # (the same replica, a store of its own scheme)
    assert (ok.dump(0)["avail"][0] == 0x1F).all()
