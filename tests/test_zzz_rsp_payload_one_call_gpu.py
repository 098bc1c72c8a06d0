"""The RSPaxos payload stores' one-call byte path (`smr_rsp_pstore_put_follow_all`, csrc/rsp_payload.hip) through leader
changes, lost and rejected Accepts, Prepare phases and re-Accepts: tests/rsp_one_call.py's tick, whose client Accept phase runs
last, drives three co-located clusters of five `RSPaxosReplicaWithPayload` on the same inputs.  They differ only in the byte
path behind a sender's client Accepts:
  A: put + follow(leader) + follow_many(followers, source=(leader, REQS))
  B: put_follow_all (the put launch writes the followers' shards: ps_deliver_mask / `dlv`)
  C: put_follow_all with SMR_PS_DELIVER=0 (the followers' shards through the byte kernel)
After every tick: the engines against five oracles run on the same schedule (full dump, executed lists), the stores identical
across the arms (headers, every named shard byte, aliases, counters), B's stores against the engine's masks and the oracle's
codewords (check_stores), every executed command read back as its batch.  The shapes cross the put launch's block mapping:
one 16-byte column per group over several blocks, groups that straddle blocks, groups wider than a block."""
import contextlib
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(__file__))

pytestmark = [pytest.mark.gpu, pytest.mark.timeout(900)]


def run_schedule_matches_oracle(dev, oracle, G, W, ft, loss, T, seed):
    """the reordered schedule on five bare engines and on five oracles: full dump and executed lists, tick by tick"""
    import rsp_cluster as rc
    import rsp_one_call as oc
    from summerset_amd import RSPaxosReplicaGroup
    R = 5
    engs = [rc.NumpyEngine(RSPaxosReplicaGroup(G, R, me=r, window=W, fault_tolerance=ft), dev) for r in range(R)]
    orcs = [oracle.RspOracle(G, R, me=r, W=W, fault_tolerance=ft) for r in range(R)]
    for x in engs + orcs:
        x.preset_leader(0)
    stats, ev = {}, []
    for t, val, target, to, drop, hb in oc.inputs(G, T, seed, loss, R):
        lo = oc.tick(orcs, val, target, to, drop, hb, stats=stats)
        le = oc.tick(engs, val, target, to, drop, hb, hook=lambda s, acc, fol: None)
        assert len(le) == len(lo), t
        for x, y in zip(le, lo):
            for k in y:
                assert np.array_equal(x[k], y[k]) if isinstance(y[k], np.ndarray) else x[k] == y[k], (t, y["kind"], k)
        for r in range(R):
            for x, y in zip(engs[r].take_executed(), orcs[r].take_executed()):
                assert np.array_equal(x, y), (t, r, "executed", len(x), len(y))
            a, b = engs[r].dump(), orcs[r].dump()
            for n in b:
                assert np.array_equal(a[n], b[n]), (t, r, n, [x[:4] for x in np.nonzero(a[n] != b[n])])
        ev += lo
    return stats, ev


def run_three_arms(dev, oracle, monkeypatch, G, W, ft, loss, L, T, seed, arms=("A", "B", "C"), R=5):
    """see the module's docstring; `arms`: which of A, B, C run (B always); R: the population.  Returns what the run covered."""
    import rsp_one_call as oc
    import test_zz_rsp_payload_gpu as tp
    from test_craft_payload import _stores_equal
    from summerset_amd.rsp_payload import REQS, VOTED, RSPaxosPayloadStore
    assert "B" in arms
    monkeypatch.delenv("SMR_PS_DELIVER", raising=False)
    exp = tp.Expect(oracle, R, R // 2 + 1, L)
    orcs = [oracle.RspOracle(G, R, me=r, W=W, fault_tolerance=ft) for r in range(R)]
    cl = {}
    for a in arms:
        reps, _ = tp.make_cluster(dev, G, R, W, ft, L)
        cl[a] = (reps, [oc.PayloadEngine(r, dev) for r in reps])
    for x in orcs + [e for a in arms for e in cl[a][1]]:
        x.preset_leader(0)
    n_exec = [0]
    for a in arms:                                               # executions read back right after the handler that ran them
        for rep in cl[a][0]:
            for name in ("accept", "accept_replies", "prepare", "prepare_replies", "reconstruct", "reconstruct_reply", "heartbeat",
                         "bcast_heartbeat", "become_leader"):
                def hooked(*x, _fn=getattr(rep, name), _rep=rep, _name=name, **kw):
                    out = _fn(*x, **kw)
                    n_exec[0] += tp.check_executed(_rep, dev, exp, (_name, _rep.me))
                    return out
                setattr(rep, name, hooked)

    @contextlib.contextmanager
    def deliver_off(on):
        if on:
            monkeypatch.setenv("SMR_PS_DELIVER", "0")
        try:
            yield
        finally:
            if on:
                monkeypatch.delenv("SMR_PS_DELIVER")

    def hook_for(a):
        reps, engs = cl[a]

        def hook(s, acc, followers):
            w, ne = reps[s], engs[s]
            accd = {k: ne._t(acc[k]) for k in ("a_n", "a_slot", "a_val")}
            data, lens = w.payload(accd["a_val"][0].contiguous())        # (a_val row 0 = the tokens req_batch was given, where a_n > 0)
            fs, fr = [reps[q].store for q in followers], [reps[q].replica for q in followers]
            if a == "B":                                          # (before the call) see `foreign` below
                live, tok, gi = acc["a_n"] > 0, acc["a_val"][0], np.arange(G)
                row = (acc["a_slot"][0] & (W - 1)).astype(np.int64)
                for q in followers:
                    e, h, al = reps[q].replica.dump(), reps[q].store.dump(REQS), reps[q].store.voted_alias()
                    ev = e["s_val"][row, gi]
                    foreign[0] += int((live & (ev != tok) & (ev != tp.NULL) & (e["s_mask"][row, gi] != 0) & (h["tok"][row, gi] == ev)
                                       & (h["avail"][row, gi] != 0) & (al[row, gi] == 0)).sum())
            if a == "A":
                w.store.put(accd, data, lens)
                w.store.follow(w.replica)
                RSPaxosPayloadStore.follow_many(fs, fr, (w.store, REQS))
            else:
                with deliver_off(a == "C"):
                    w.store.put_follow_all(w.replica, accd, data, fs, fr, lens=lens)
            for r in [s] + followers:                             # what the bare handlers executed, now that the bytes are there
                n_exec[0] += tp.check_executed(reps[r], dev, exp, ("bare", a, r))
        return hook

    # foreign: a follower whose engine did not take the sender's Accept (lost, or not taken) and whose REQS row holds another live
    # token with no vote aliased into it -- the put launch must write nothing there (ps_deliver_mask's check of the follower's engine)
    foreign = [0]
    stats, ev, n_cmp, moved = {}, [], 0, 0
    bst = [r.store for r in cl["B"][0]]
    al0, v0 = [s.voted_alias() for s in bst], [s.dump(VOTED) for s in bst]
    for t, val, target, to, drop, hb in oc.inputs(G, T, seed, loss, R):
        lo = oc.tick(orcs, val, target, to, drop, hb, stats=stats)
        ev += lo
        ex = [o.take_executed() for o in orcs]
        snap = [o.dump() for o in orcs]
        for a in arms:
            le = oc.tick(cl[a][1], val, target, to, drop, hb, hook=hook_for(a))
            assert len(le) == len(lo), (t, a)
            for r in range(R):
                for x, y in zip(cl[a][1][r].take_executed(), ex[r]):
                    assert np.array_equal(x, y), (t, a, r, "executed", len(x), len(y))
                d = cl[a][0][r].replica.dump()
                for n in snap[r]:
                    assert np.array_equal(d[n], snap[r][n]), (t, a, r, n, [x[:4] for x in np.nonzero(d[n] != snap[r][n])])
        for a in arms[1:]:                                       # every store of every arm identical to the first arm's
            for r in range(R):
                _stores_equal(cl[arms[0]][0][r].store, cl[a][0][r].store, 2, W, (t, arms[0], a, r))
        n_cmp += tp.check_stores(cl["B"][0], exp, (t, "B"))
        for r, s in enumerate(bst):                              # votes that left the REQS row: an alias before, the row's own bytes now
            al1, v1 = s.voted_alias(), s.dump(VOTED)
            moved += int(np.unpackbits(al0[r] & ~al1 & v1["avail"] & np.where(v1["tok"] == v0[r]["tok"], 0xFF, 0).astype(np.uint8)).sum())
            al0[r], v0[r] = al1, v1
    for a in arms:
        for st in (r.store for r in cl[a][0]):
            c = st.counters()
            if a == "B":
                assert 0 < st.delivered() <= c["copied"], (a, st.delivered(), c)
            else:
                assert st.delivered() == 0, (a, st.delivered())
    tot = {k: sum(s.counters()[k] for s in bst) for k in ("copied", "rebuilt", "unsatisfied", "rekeyed")}
    cov = dict(tot, n_exec=n_exec[0], n_cmp=n_cmp, moved=moved, lost_onto_other=stats.get("lost_onto_other", 0),
               not_taken=stats.get("not_taken", 0), re_accept=sum(e["n"] for e in ev if e["kind"] == "re_accept"),
               empty=sum(e["empty"] for e in ev if e["kind"] == "re_accept"),
               longest=max(int(o.dump()["len"].max()) for o in orcs), delivered=sum(s.delivered() for s in bst), foreign=foreign[0])
    print("coverage", dict(G=G, W=W, L=L, T=T, seed=seed, arms=arms), cov)
    # what the run must have covered: conditions, not measurements
    assert cov["lost_onto_other"] > 0 and cov["not_taken"] > 0 and cov["moved"] > 0 and cov["foreign"] > 0, cov
    assert cov["rekeyed"] > 0 and cov["rebuilt"] > 0 and cov["re_accept"] > 0 and cov["empty"] > 0, cov
    assert cov["longest"] > 2 * W and cov["unsatisfied"] == 0 and cov["n_exec"] > 0 and cov["n_cmp"] > 0, cov
    return cov


@pytest.mark.parametrize("G,W,ft,loss,L,T", [(70, 8, 1, 0.1, 67, 27), (96, 16, 1, 0.1, 333, 51)])
def test_reordered_schedule_matches_oracle(cuda, oracle, G, W, ft, loss, L, T):
    stats, ev = run_schedule_matches_oracle(cuda, oracle, G, W, ft, loss, T, seed=G + ft)
    assert stats["lost_onto_other"] > 0 and sum(e["n"] for e in ev if e["kind"] == "re_accept") > 0, stats


# G, W, ft, loss, L (nblk = ceil(ceil(L / 3) / 16) columns per group), T
SHAPES = [(300, 8, 1, 0.1, 40, 27),        # nblk 1: two blocks of 256 whole groups, a partial last block
          (130, 8, 1, 0.1, 4113, 27),      # nblk 86: groups straddle blocks (config 4's L)
          (96, 16, 1, 0.1, 333, 51),       # nblk 7
          (20, 8, 1, 0.1, 12300, 27)]      # nblk 257: every group spans two blocks


SEEDS = {(300, 40): 1, (130, 4113): 2, (96, 333): 1, (20, 12300): 6}     # seeds under which every coverage condition holds


@pytest.mark.parametrize("G,W,ft,loss,L,T", SHAPES)
def test_one_call_byte_path_through_leader_changes(cuda, oracle, monkeypatch, G, W, ft, loss, L, T):
    run_three_arms(cuda, oracle, monkeypatch, G, W, ft, loss, L, T, seed=SEEDS[(G, L)])
