"""The EPaxos command leader's receive side of a tick as ONE launch (`smr_ep_leader_handle_wire_pre_accept_replies`,
csrc/ep_engine.hip: ep_wire_pre_accept_replies_kernel): the acceptors' `[u64 BE length][bincode(PeerMessage)]` frames
(safetcp.rs:46,127-132; PreAcceptReply = epaxos/mod.rs:306-377 variant 1) parsed in the prologue of the reply handler
(messages.rs:96-270), against the two calls it stands for -- `smr_wire_ingest_ep_pre_accept_replies` +
`smr_ep_handle_pre_accept_replies` -- on a second replica in the same state, and against the oracle fed the decoded replies.

The frames are laid out HERE from the type definitions (`PeerMessage::Msg { msg }` = enum tag 0, PeerMsg variant index,
`SlotIdx(u8, usize)`, bincode-standard varints, `Option` = a tag byte): no product encoder for the replies.  Every comparison
is bit-exact.  The runner functions take the device as an argument: tests/test_ep_wire_replies_hostsim.py calls them with "cpu"
under the kernel-source emulation."""
import struct

import ep_cluster as ec
import numpy as np
import pytest

pytestmark = pytest.mark.gpu
NONE32 = 0xFFFFFFFF
STRIDE = 96                                                      # SMR_WIRE_EMIT_EP_STRIDE


def _varint(v):
    if v < 251:
        return bytes([v])
    if v < 1 << 16:
        return b"\xfb" + struct.pack("<H", v)
    if v < 1 << 32:
        return b"\xfc" + struct.pack("<I", v)
    return b"\xfd" + struct.pack("<Q", v)


def _frame(payload):
    return struct.pack(">Q", len(payload)) + payload


def _ep_reply(row, col, ballot, seq, deps, tag=1, extra=b""):
    """deps: None / int per row; `tag`: the Option tag written for a Some (2: no such tag); `extra`: bytes behind the reply
    inside its frame (a reply that does not end where its length says)"""
    body = _varint(0) + _varint(1) + bytes([row]) + _varint(col) + _varint(ballot) + _varint(seq) + _varint(len(deps))
    return _frame(body + b"".join(b"\x00" if d is None else bytes([tag]) + _varint(d) for d in deps) + extra)


def _t(torch, a, device):
    if a is None:
        return None
    v = a.view(np.int64) if a.dtype == np.uint64 else (a.view(np.int32) if a.dtype == np.uint32 else a)
    return torch.from_numpy(np.ascontiguousarray(v)).to(device)


def _layout(torch, device, streams, stride=False):
    """back to back: (buf, conn_off [n + 1], None); emit-stride: slot c at c * 96, (buf, conn_off [n], conn_len uint8 [n])"""
    n = len(streams)
    if stride:
        assert all(len(s) <= STRIDE for s in streams)
        blob = np.zeros(n * STRIDE + 16, np.uint8)
        for c, s in enumerate(streams):
            blob[c * STRIDE:c * STRIDE + len(s)] = np.frombuffer(s, np.uint8)
        off = np.arange(n, dtype=np.int64) * STRIDE
        ln = np.array([len(s) for s in streams], np.uint8)
        return torch.from_numpy(blob).to(device), torch.from_numpy(off).to(device), torch.from_numpy(ln).to(device)
    off = np.zeros(n + 1, np.int64)
    off[1:] = np.cumsum([len(s) for s in streams])
    blob = b"".join(streams)
    buf = torch.from_numpy(np.frombuffer(blob + b"\x00" * 16, np.uint8)[:max(len(blob), 1)].copy()).to(device)
    return buf, torch.from_numpy(off).to(device), None


def _dense(torch, device, G, R, me):
    peers_of = [p for p in range(R) if p != me]
    grp = torch.from_numpy(np.repeat(np.arange(G), R - 1).astype(np.int32)).to(device)
    peer = torch.from_numpy(np.tile(np.array(peers_of, np.uint8), G)).to(device)
    return peers_of, grp, peer


def _same_results(ra, rb, t):
    for k in ("n_replies", "n_others", "n_malformed", "n_deferred"):
        assert ra[k] == rb[k], (t, k, ra[k], rb[k])
    assert np.array_equal(ra["consumed"], rb["consumed"]), t
    assert np.array_equal(ra["status"], rb["status"]), t


def _same_decisions(da, db, t):
    for k in ("decision", "seq", "deps"):
        assert np.array_equal(da[k].cpu().numpy(), db[k].cpu().numpy()), (t, k)


def run_fused_ep_wire_replies(device, oracle, G=300, R=5, W=32, K=6, T=6, seed=31, me=2, execute=False, stride=False):
    """Two replicas `a` (the two calls) and `b` (the fused call) in the same state and an oracle fed the decoded replies: T ticks
    of proposals and synthesised PreAcceptReplies -- equal ones (fast path), differing seq / deps (slow path), ballot 0
    re-evaluations with `exploded`, missing ones, seq above 2^32 and with bit 63 set, None dependencies -- with junk frames
    (Leave, an AcceptReply, a non-Msg outer tag), replies for another column / row, with R + 1 dependencies or a dependency of
    2^32 - 1 or more (all located), second replies (deferred), incomplete tails and malformed frames around them.  Counts, located
    frames, `consumed`, `status`, decisions and the replicas' whole state every tick.  Returns fast + slow decisions."""
    import torch
    from summerset_amd import EPaxosReplicaGroup, stream, wire
    rng = np.random.default_rng(seed)
    F = R - 1
    a = EPaxosReplicaGroup(G, R, me=me, window=W, n_keys=K, execute=execute)
    b = EPaxosReplicaGroup(G, R, me=me, window=W, n_keys=K, execute=execute)
    orc = oracle.EpOracle(G, R, me=me, W=W, n_keys=K, execute=execute) if oracle is not None else None
    ing_a, ing_b = wire.ReplyIngest(G * F, G, R, 6 * G * F, device), wire.ReplyIngest(G * F, G, R, 6 * G * F, device)
    peers_of, grp, peer = _dense(torch, device, G, R, me)
    junk = [_frame(_varint(2)),                                                           # PeerMessage::Leave
            _frame(_varint(0) + _varint(3) + bytes([me]) + _varint(7) + _varint(me + 1)),   # PeerMsg::AcceptReply { slot, ballot }
            _frame(_varint(1) + bytes(range(20)))]                                          # not PeerMessage::Msg: lease traffic
    z = 1.0 / np.arange(1, K + 1) ** 0.99
    z /= z.sum()
    n_fast = n_slow = n_wide = n_reval = 0
    for t in range(T):
        key = rng.choice(K, G, p=z).astype(np.uint8)
        key[rng.random(G) >= 0.9] = 0xFF
        pa = None
        for x in (a, b):
            pa = x.handle_req_batch(_t(torch, key, device))
        col = pa["col"].cpu().numpy().view(np.uint32).copy()
        base_seq = pa["seq"].cpu().numpy().view(np.uint64).copy()
        base_deps = pa["deps"].cpu().numpy().view(np.uint32).copy()
        if orc is not None:
            po = orc.propose(key)
            assert np.array_equal(po["col"], col) and np.array_equal(po["seq"], base_seq) and np.array_equal(po["deps"], base_deps), t
        # the acceptors' replies, as arrays first (what the oracle is fed)
        fl = (rng.random((R, G)) < 0.8).astype(np.uint8)
        fl[me] = 0
        ballot = np.full((R, G), me + 1, np.uint64)
        reval = rng.random((R, G)) < 0.05
        ballot[reval] = 0                                                                  # "failure suspected" re-evaluation
        ballot[rng.random((R, G)) < 0.03] = 77                                             # not my ballot
        seq = np.broadcast_to(base_seq, (R, G)).copy()
        deps = np.broadcast_to(base_deps, (R, R, G)).copy()
        extra = rng.random((R, G)) < 0.1                                                   # a larger seq and one more dependency: slow path
        seq[extra] += np.uint64(1)
        for p in range(R):
            r_ = rng.integers(0, R, G)
            c_ = rng.integers(0, 4, G).astype(np.uint32)
            cur = deps[p, r_, np.arange(G)]
            deps[p, r_, np.arange(G)] = np.where(extra[p], np.where(cur == NONE32, c_, cur + 1), cur)
        wide = rng.random(G) < 0.06                                                        # every acceptor's seq wide: committed wide, the key climbs from there
        big = np.where(np.arange(G) % 2 == 0, np.uint64(1 << 32), np.uint64(1 << 63)) + np.arange(G, dtype=np.uint64) % np.uint64(97) + np.uint64(3)
        assert int(base_seq.max()) < (1 << 64) - 4096                                      # (max_seq + 1 of the next proposal stays far from wrapping)
        seq = np.where(wide[None, :], np.maximum(seq, big[None, :]), seq).astype(np.uint64)
        n_wide += int((wide[None, :] & (fl == 1)).sum()); n_reval += int((reval & (fl == 1)).sum())
        exploded = np.where(rng.random(G) < 0.2, rng.integers(0, 1 << R, G), 0).astype(np.uint8)
        order = np.ascontiguousarray(stream.random_ackctl(13, t, 1, G, R, 0.0)[0]) if t % 2 else None
        # ... then as frames, per connection (group-major, peers ascending, mine left out)
        streams = []
        for g in range(G):
            cg = int(col[g])
            for p in peers_of:
                front, tail = bytearray(), bytearray()
                if rng.random() < 0.15:
                    front += junk[int(rng.integers(0, len(junk)))]
                zz = rng.random()
                some = [int(rng.integers(0, 9)) for _ in range(R)]
                if zz < 0.03:
                    front += _ep_reply(me, cg + 1, me + 1, 4, some)                        # another column: located
                elif zz < 0.06:
                    front += _ep_reply((me + 1) % R, cg, me + 1, 4, some)                  # another row: located
                elif zz < 0.09:
                    front += _ep_reply(me, cg, me + 1, 4, some + [None])                   # R + 1 dependencies: located
                elif zz < 0.12:
                    front += _ep_reply(me, cg, me + 1, 4, some[:-1] + [(1 << 32) - 1 + int(rng.integers(0, 3))])   # a dependency >= 2^32 - 1: located
                main = b""
                if fl[p, g]:
                    main = _ep_reply(me, cg, int(ballot[p, g]), int(seq[p, g]), [None if int(d) == NONE32 else int(d) for d in deps[p, :, g]])
                y = rng.random()
                if fl[p, g]:
                    if y < 0.05:
                        tail += _ep_reply(me, cg, me + 1, 1, [None] * R)                   # a second reply: the next call's
                    elif y < 0.10:
                        tail += _ep_reply(me, cg, 1 << 40, 7, some)[:int(rng.integers(1, 14))]   # an incomplete tail
                    elif y < 0.12:
                        tail += _ep_reply(me, cg, me + 1, 1, some, tag=2)                  # malformed (Option tag 2) behind a delivered reply
                    elif y < 0.14:
                        tail += _ep_reply(me, cg, me + 1, 1, some, extra=b"\x00")          # ... a reply that ends before its frame does
                else:
                    if y < 0.04:
                        tail += _ep_reply(me, cg, me + 1, 1, some, tag=2)                  # malformed, nothing delivered
                    elif y < 0.06:
                        tail += _frame(_varint(0) + _varint(1) + bytes([me]) + _varint(cg) + _varint(1) + _varint(1) + _varint(65))   # n > 64
                    elif y < 0.08:
                        tail += _frame(b"\xff")                                            # a tag that does not parse
                    elif y < 0.10:
                        tail += struct.pack(">Q", 10 ** 12 + 1)                            # a length above 10^12
                s = bytes(front) + main + bytes(tail)
                if stride and len(s) > STRIDE:
                    s = main                                                               # (a slot of the emit layout holds one reply)
                streams.append(s)
        buf, off, ln = _layout(torch, device, streams, stride)
        col_t, ord_t, ex_t = _t(torch, col, device), _t(torch, order, device), _t(torch, exploded, device)
        o = ing_a.ep_pre_accept(buf, off, grp, peer, me, col_t, conn_len=ln)
        da = a.handle_msg_pre_accept_reply(col_t, o["ballot"], o["seq"], o["deps"], o["flags"], ord_t, ex_t)
        poll_a = a.exec_poll() if execute else None
        db = ing_b.ep_pre_accept_into(b, buf, off, col_t, ord_t, ex_t, conn_len=ln)
        poll_b = b.exec_poll() if execute else None
        ra, rb = ing_a.results(), ing_b.results()
        print("tick %d: replies %d others %d malformed %d deferred %d | fused %d %d %d %d" % (
            t, ra["n_replies"], ra["n_others"], ra["n_malformed"], ra["n_deferred"], rb["n_replies"], rb["n_others"], rb["n_malformed"], rb["n_deferred"]))
        _same_results(ra, rb, t)
        srt = lambda q: np.sort(q, order=["conn", "off"])   # noqa: E731
        assert len(ra["others"]) == ra["n_others"] and np.array_equal(srt(ra["others"]), srt(rb["others"])), t
        _same_decisions(da, db, t)
        sa, sb = a.dump(), b.dump()
        for n in sa:
            assert np.array_equal(sa[n], sb[n]), (t, n)
        if execute:
            xa, xb = a.exec_dump(), b.exec_dump()
            for n in xa:
                assert np.array_equal(xa[n], xb[n]), (t, n, "exec")
            for u, v in zip(poll_a, poll_b):
                assert np.array_equal(u, v), (t, "submissions")
        # the replies taken: the flags the test intended (a reply in front of a malformed frame stays delivered, uncounted)
        taken = o["flags"].cpu().numpy()
        assert np.array_equal(taken != 0, fl != 0), t
        ok = (ra["status"] == 0).reshape(G, F)
        assert ra["n_replies"] == int((fl[peers_of, :].T != 0)[ok].sum()), t
        if orc is not None:
            do = orc.handle_pre_accept_replies(col, ballot, seq, np.ascontiguousarray(deps), np.ascontiguousarray(fl), order, exploded)
            for k, dt in (("decision", np.uint8), ("seq", np.uint64), ("deps", np.uint32)):
                assert np.array_equal(db[k].cpu().numpy().view(dt), do[k]), (t, k, "oracle")
            so = orc.dump()
            for n in so:
                assert np.array_equal(sb[n], so[n]), (t, n, "oracle")
            if execute:
                xo = orc.exec_dump()
                for n in ("exec_bars", "kv", "digest"):
                    assert np.array_equal(xb[n], xo[n]), (t, n, "oracle exec")
        dec = db["decision"].cpu().numpy()
        n_fast += int((dec == 3).sum()); n_slow += int((dec == 2).sum())
        assert ra["n_malformed"] > 0 and ra["n_others"] > 0
        assert stride or ra["n_deferred"] > 0
    assert n_fast > 0 and n_slow > 0 and n_wide > 0 and n_reval > 0, (n_fast, n_slow, n_wide, n_reval)
    wide_kept = b.dump()["seq"][me]
    assert (wide_kept > np.uint64(1 << 32)).any() and (wide_kept > np.uint64(1 << 63)).any()
    a.close(); b.close()
    return n_fast + n_slow


def test_fused_ep_wire_replies_equal_the_two_calls(cuda, oracle):
    run_fused_ep_wire_replies(cuda, oracle, G=300, R=5, me=2)
    run_fused_ep_wire_replies(cuda, oracle, G=1100, R=3, me=0, seed=5, T=4)              # 256 groups per block, my id in front
    run_fused_ep_wire_replies(cuda, oracle, G=700, R=7, me=6, W=16, seed=6, T=4)         # the 8-wide instance, 85 groups = 510 of a block's 512 lanes
    run_fused_ep_wire_replies(cuda, oracle, G=300, R=5, me=1, seed=7, T=5, execute=True)   # the execution pass behind the fused call
    run_fused_ep_wire_replies(cuda, oracle, G=300, R=5, me=3, seed=8, T=4, stride=True)  # the emit calls' layout: starts + conn_len


class WireBackend(ec.NumpyEngine):
    """tests/ep_cluster.py's NumpyEngine with the command leader's receive side over the wire: `via` keeps the PreAcceptReplies as
    frames, `handle_pre_accept_replies` hands those frames to the fused entry instead of taking arrays"""

    def __init__(self, eng, device):
        from summerset_amd import wire
        super().__init__(eng, device)
        G, R = eng.G, eng.R
        self.ing = wire.ReplyIngest(G * (R - 1), G, R, G * (R - 1), device)
        self.frames, self.sent = None, 0
        self.n_junk = sum(1 for g in range(G) for q in range(R) if q != eng.me and (g + q) % 9 == 0)

    def via(self, col, ballot, seq, deps, flags):
        me, G, R = self.e.me, self.e.G, self.e.R
        streams = []
        for g in range(G):
            for q in range(R):
                if q == me:
                    continue
                f = bytearray()
                if (g + q) % 9 == 0:
                    f += _frame(_varint(0) + _varint(3) + bytes([me]) + _varint(1) + _varint(7))   # an AcceptReply: located only
                if flags[q, g] & 1:
                    f += _ep_reply(me, int(col[g]), int(ballot[q, g]), int(seq[q, g]), [None if int(d) == NONE32 else int(d) for d in deps[q, :, g]])
                streams.append(bytes(f))
        self.frames = _layout(self.torch, self.cuda, streams)
        self.sent = int((flags & 1).sum())
        return ballot, seq, deps, flags

    def handle_pre_accept_replies(self, col, ballot, seq, deps, flags, order=None, exploded=None, row=None):
        assert row is None                                                                 # (own row only: the fused entry's contract)
        buf, off, _ = self.frames
        self.frames = None
        o = self.ing.ep_pre_accept_into(self.e, buf, off, self._t(col), self._t(order), self._t(exploded))
        self._after_call()
        res = self.ing.results()
        assert res["n_malformed"] == 0 and res["n_deferred"] == 0 and res["n_replies"] == self.sent and res["n_others"] == self.n_junk
        return self._n(o, dict(decision=np.uint8, seq=np.uint64, deps=np.uint32))


def run_fused_ep_cluster_over_the_wire(device, oracle, G=260, R=5, W=32, K=6, T=8):
    from summerset_amd import EPaxosReplicaGroup
    engs = [WireBackend(EPaxosReplicaGroup(G, R, me=r, window=W, n_keys=K), device) for r in range(R)]
    orcs = [oracle.EpOracle(G, R, me=r, W=W, n_keys=K) for r in range(R)]
    rng = np.random.default_rng(5)
    fast = slow = 0
    for t in range(T):
        keys = ec.zipf_keys(rng, R, G, K)
        drop = {(s, q): rng.random(G) < 0.15 for s in range(R) for q in range(R) if s != q}
        oe = ec.tick(engs, keys, drop, via=lambda s, *m: engs[s].via(*m))
        oo = ec.tick(orcs, keys, drop)
        for s in range(R):
            for k in oo[s]:
                assert np.array_equal(oe[s][k], oo[s][k]), (t, s, k)
            fast += int((oo[s]["decision"] == 3).sum()); slow += int((oo[s]["decision"] == 2).sum())
    for r in range(R):
        x, y = engs[r].dump(), orcs[r].dump()
        for n in y:
            assert np.array_equal(x[n], y[n]), (r, n)
    assert fast > 0 and slow > 0
    return fast, slow


def test_fused_ep_cluster_over_the_wire(cuda, oracle):
    """tests/ep_cluster.py's closed loop (PreAccept fan-out with loss, fast and slow path) with every command leader taking its
    PreAcceptReplies as frames through the fused entry; the oracle cluster is wired directly"""
    run_fused_ep_cluster_over_the_wire(cuda, oracle)


def run_fused_ep_wire_block_edges(device):
    """one block's streams longer than its LDS stage (a long filler frame in front of every reply: the lanes behind read the
    buffer), more located frames in a block than its LDS list keeps, `other_cap` below the number of located frames (counted, not
    stored), a last block with a partial count of connections -- and a second call on the same replica with nothing cleared in
    between, whose counts are exact"""
    import torch
    from summerset_amd import EPaxosReplicaGroup, wire
    G, R, me, W, K = 150, 5, 1, 8, 4                                                       # 600 connections: a block of 512 and one of 88
    F, cap = R - 1, 250
    a, b = EPaxosReplicaGroup(G, R, me=me, window=W, n_keys=K), EPaxosReplicaGroup(G, R, me=me, window=W, n_keys=K)
    ing_a, ing_b = wire.ReplyIngest(G * F, G, R, cap, device), wire.ReplyIngest(G * F, G, R, cap, device)
    peers_of, grp, peer = _dense(torch, device, G, R, me)
    fill = _frame(_varint(1) + bytes(51))                                                  # 60 bytes, located
    rng = np.random.default_rng(9)
    for rnd in range(2):
        key = rng.integers(0, K, G).astype(np.uint8)
        pa = None
        for x in (a, b):
            pa = x.handle_req_batch(_t(torch, key, device))
        col = pa["col"].cpu().numpy().view(np.uint32)
        seq = pa["seq"].cpu().numpy().view(np.uint64)
        deps = pa["deps"].cpu().numpy().view(np.uint32)
        streams, n_fill, n_rep = [], 0, 0
        for g in range(G):
            for i, p in enumerate(peers_of):
                c = g * F + i
                s = bytearray()
                if rnd == 0 or c % 2 == 0:
                    s += fill; n_fill += 1
                if rnd == 0 or c % 3:                                                      # (every fourth group: no two replies agree -- slow path)
                    s += _ep_reply(me, int(col[g]), me + 1, int(seq[g]) + (i + 1 if g % 4 == 0 else 0), [None if int(d) == NONE32 else int(d) for d in deps[:, g]])
                    n_rep += 1
                streams.append(bytes(s))
        if rnd == 0:
            assert sum(len(s) for s in streams[:512]) > 512 * 40 + 16 and n_fill > 2 * 256
        buf, off, _ = _layout(torch, device, streams)
        col_t = _t(torch, col, device)
        o = ing_a.ep_pre_accept(buf, off, grp, peer, me, col_t)
        da = a.handle_msg_pre_accept_reply(col_t, o["ballot"], o["seq"], o["deps"], o["flags"])
        db = ing_b.ep_pre_accept_into(b, buf, off, col_t)
        ra, rb = ing_a.results(), ing_b.results()
        print("round %d: fused replies %d others %d malformed %d deferred %d" % (rnd, rb["n_replies"], rb["n_others"], rb["n_malformed"], rb["n_deferred"]))
        _same_results(ra, rb, rnd)
        assert rb["n_replies"] == n_rep and rb["n_others"] == n_fill and rb["n_malformed"] == 0 and rb["n_deferred"] == 0
        assert list(rb["consumed"]) == [len(s) for s in streams]
        # beyond other_cap: counted, not stored; what is stored are whole located frames, each once
        kept = rb["others"]
        assert len(kept) == min(n_fill, cap) and n_fill > cap
        starts = off.cpu().numpy()
        seen = set()
        for r_ in kept:
            c = int(r_["conn"])
            assert (rnd == 0 or c % 2 == 0) and int(r_["off"]) == int(starts[c]) and int(r_["len"]) == len(fill) and int(r_["kind"]) == 0xFF and c not in seen
            seen.add(c)
        _same_decisions(da, db, rnd)
        sa, sb = a.dump(), b.dump()
        for n in sa:
            assert np.array_equal(sa[n], sb[n]), (rnd, n)
        dec = db["decision"].cpu().numpy()
        assert (dec == 3).any() and (dec == 2).any()
    a.close(); b.close()


def test_fused_ep_wire_replies_block_edges(cuda):
    run_fused_ep_wire_block_edges(cuda)


def run_fused_ep_wire_bad_arguments(device):
    """sparse connections, a byte buffer that is not 16-byte aligned, null outputs: refused, nothing launched"""
    import torch
    from summerset_amd import EPaxosReplicaGroup, SummersetError, _lib, wire
    G, R = 64, 5
    rep = EPaxosReplicaGroup(G, R, me=0, window=8, n_keys=4)
    n = G * (R - 1)
    ing = wire.ReplyIngest(n, G, R, 16, device)
    buf = torch.zeros(64, dtype=torch.uint8, device=device)
    off = torch.zeros(n + 1, dtype=torch.int64, device=device)
    col = torch.zeros(G, dtype=torch.int32, device=device)
    ing.ep_pre_accept_into(rep, buf, off, col)                                             # (the arguments below are fine but for the one named)
    assert ing.results()["n_replies"] == 0
    ing.n_conn = 100                                                                       # not n_groups * (population - 1)
    with pytest.raises((SummersetError, AssertionError)):
        ing.ep_pre_accept_into(rep, buf, off, col)
    ing.n_conn = n
    L, p = _lib.load(), lambda x: x.data_ptr()   # noqa: E731
    dec, dseq = torch.zeros(G, dtype=torch.uint8, device=device), torch.zeros(G, dtype=torch.int64, device=device)
    ddeps = torch.zeros((R, G), dtype=torch.int32, device=device)
    st = _lib.stream_ptr(None)
    good = [rep._h, p(buf), buf.numel(), p(off), None, n, p(col), None, None, p(dec), p(dseq), p(ddeps), p(ing.others), ing.other_cap,
            p(ing.counts), p(ing.consumed), p(ing.status), st]
    assert L.smr_ep_leader_handle_wire_pre_accept_replies(*good) == 0
    for i, frag in ((5, "dense"), (1, "16-byte aligned"), (9, "null"), (10, "null"), (11, "null"), (14, "null"), (15, "null"), (16, "null"), (12, "null"),
                    (3, "null"), (6, "null")):
        bad = list(good)
        bad[i] = 100 if i == 5 else p(buf) + 1 if i == 1 else None
        assert L.smr_ep_leader_handle_wire_pre_accept_replies(*bad) == _lib.SMR_ERR_ARG, i
        assert frag in L.smr_last_error().decode(), (i, L.smr_last_error())
    rep.close()


def test_fused_ep_wire_replies_refuse_bad_arguments(cuda):
    run_fused_ep_wire_bad_arguments(cuda)
