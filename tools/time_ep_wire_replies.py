#!/usr/bin/env python3
"""The EPaxos command leader's receive side of a tick, frames -> decisions: ONE launch
(`smr_ep_leader_handle_wire_pre_accept_replies`) beside the two calls it stands for
(`smr_wire_ingest_ep_pre_accept_replies` + `smr_ep_handle_pre_accept_replies`), timed with device events in one process.

    python tools/time_ep_wire_replies.py > profiles/ep_wire_pre_accept_replies_fused_vs_two_calls.log

Shape: R = 5, G = 65 536 -> 262 144 dense connections (the `reply_ingest` leg's size), from a seed.  Every repetition both
replicas (`a`: the two calls, `b`: the fused call; same state throughout) propose one instance per group, every connection gets
one PreAcceptReply to it (80 % equal to the proposal, the rest with a larger seq: ~2 % of the groups take the slow path) and ~15 % of the connections
carry a located frame (Leave / an AcceptReply) in front.  Both byte layouts: back to back (conn_off [n + 1]) and the emit calls'
(slot c at c * SMR_WIRE_EMIT_EP_STRIDE, conn_len).  The frames are written on the device (`smr_wire_emit_ep_pre_accept_replies`
+ a gather), so a repetition costs no host loop.

Steps, each a process of its own under `timeout -k 10`, the second only if the first succeeded, nothing retried:
  parity   a few ticks in both layouts: outputs, counters, consumed / status, located frames and the replicas' whole state equal
  time     warm-up, then >= 30 repetitions per layout; within a repetition the two variants run one after the other, the order
           alternating; outputs compared after every repetition.  One JSON line: medians, quartiles, the spread (the larger
           inter-quartile range of the two) and the verdict per layout.
No device visible: an error (exit status 2), never a fallback."""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

G, R, ME, K, SEED = 65536, 5, 0, 64, 20
STRIDE = 96


def need_gpu():
    import torch
    if not torch.cuda.is_available():
        sys.stderr.write("time_ep_wire_replies: no GPU is visible; this tool measures device calls and has no fallback\n")
        sys.exit(2)
    return torch.device("cuda:0")


class Rig:
    """two replicas in the same state, the frames of a tick on the device, preallocated outputs for both variants"""

    def __init__(self, dev, W):
        import torch
        from summerset_amd import EPaxosReplicaGroup, _lib, wire
        self.torch, self.dev, self.wire, self.L = torch, dev, wire, _lib.load()
        self.F, self.n = R - 1, G * (R - 1)
        self.a = EPaxosReplicaGroup(G, R, me=ME, window=W, n_keys=K)
        self.b = EPaxosReplicaGroup(G, R, me=ME, window=W, n_keys=K)
        self.ing_a, self.ing_b = wire.ReplyIngest(self.n, G, R, self.n, dev), wire.ReplyIngest(self.n, G, R, self.n, dev)
        self.gen = torch.Generator(device=dev)
        self.gen.manual_seed(SEED)
        peers = [p for p in range(R) if p != ME]
        self.peers = peers
        self.grp = torch.arange(G, device=dev, dtype=torch.int32).repeat_interleave(self.F)
        self.peer = torch.tensor(peers, device=dev, dtype=torch.uint8).repeat(G)
        z = lambda shape, dt: torch.zeros(shape, dtype=dt, device=dev)   # noqa: E731
        self.out = {v: dict(decision=z(G, torch.uint8), seq=z(G, torch.int64), deps=z((R, G), torch.int32)) for v in "ab"}
        # the located frames put in front: PeerMessage::Leave (9 bytes), PeerMsg::AcceptReply { slot: (ME, 7), ballot: 1 } (13 bytes)
        leave = [0, 0, 0, 0, 0, 0, 0, 1, 2]
        acc = [0, 0, 0, 0, 0, 0, 0, 5, 0, 3, ME, 7, 1]
        pool = torch.zeros((3, 16), dtype=torch.uint8)
        pool[1, :len(leave)] = torch.tensor(leave, dtype=torch.uint8)
        pool[2, :len(acc)] = torch.tensor(acc, dtype=torch.uint8)
        self.junk, self.junk_len = pool.to(dev), torch.tensor([0, len(leave), len(acc)], device=dev)
        self.stream = _lib.stream_ptr(None)

    def rand(self, *shape):
        return self.torch.rand(shape, device=self.dev, generator=self.gen)

    def tick_frames(self):
        """both replicas propose; -> col, and the acceptors' replies as frames in both layouts"""
        torch, dev = self.torch, self.dev
        key = (self.rand(G) * K).to(torch.uint8)
        pa = None
        for x in (self.a, self.b):
            pa = x.handle_req_batch(key)
        flags = torch.ones(G, dtype=torch.uint8, device=dev)
        ballot = torch.full((G,), ME + 1, dtype=torch.int64, device=dev)
        slots, lens = [], []
        for _ in self.peers:
            u = self.rand(G)
            seq = pa["seq"] + (u < 0.2).to(torch.int64) + (u < 0.1).to(torch.int64)   # no class of three equal replies: slow path, ~2 % of the groups
            fr, ln = self.wire.emit_ep_pre_accept_replies(flags, ME, pa["col"], ballot, seq, pa["deps"])
            slots.append(fr); lens.append(ln)
        fr = torch.stack(slots, dim=1).reshape(self.n, STRIDE)                # connection g * F + k = group g's k-th peer
        ln = torch.stack(lens, dim=1).reshape(self.n).to(torch.int64)
        # ~15 % of the connections: a located frame in front of the reply (the slot's bytes shifted behind it)
        u = self.rand(self.n)
        which = (u < 0.075).to(torch.int64) + 2 * ((u >= 0.075) & (u < 0.15)).to(torch.int64)
        shift = self.junk_len[which]
        j = torch.arange(STRIDE, device=dev)[None, :]
        body = torch.gather(fr, 1, (j - shift[:, None]).clamp(min=0))
        head = self.junk[which][:, :16]
        head = torch.cat([head, torch.zeros((self.n, STRIDE - 16), dtype=torch.uint8, device=dev)], dim=1)
        slot = torch.where(j < shift[:, None], head, body)
        ln2 = ln + shift
        assert int(ln2.max()) <= STRIDE
        slot = torch.where(j < ln2[:, None], slot, torch.zeros_like(slot))
        stride_buf = torch.cat([slot.reshape(-1), torch.zeros(16, dtype=torch.uint8, device=dev)])
        stride_off = torch.arange(self.n, device=dev, dtype=torch.int64) * STRIDE
        stride_len = ln2.to(torch.uint8)
        # back to back: the same bytes compacted
        off = torch.zeros(self.n + 1, dtype=torch.int64, device=dev)
        off[1:] = torch.cumsum(ln2, 0)
        conn = torch.arange(self.n, device=dev).repeat_interleave(ln2)
        src = conn * STRIDE + (torch.arange(int(off[-1]), device=dev) - off[conn])
        dense_buf = torch.cat([slot.reshape(-1)[src], torch.zeros(16, dtype=torch.uint8, device=dev)])
        n_junk = int((which != 0).sum())
        return pa["col"], {"back_to_back": (dense_buf[:int(off[-1])], off, None), "emit_stride": (stride_buf[:self.n * STRIDE], stride_off, stride_len)}, n_junk

    def two_calls(self, col, lay):
        buf, off, ln = lay
        i, o, p = self.ing_a, self.out["a"], lambda t: None if t is None else t.data_ptr()   # noqa: E731
        rc = self.L.smr_wire_ingest_ep_pre_accept_replies(p(buf), buf.numel(), p(off), p(self.grp), p(self.peer), p(ln), self.n, G, R, ME, p(col),
                                                          p(i.u64a), p(i.u64b), p(i.deps), p(i.flags), p(i.others), i.other_cap, p(i.counts),
                                                          p(i.consumed), p(i.status), self.stream)
        rc = rc or self.L.smr_ep_handle_pre_accept_replies(self.a._h, p(col), p(i.u64a), p(i.u64b), p(i.deps), p(i.flags), None, None, p(o["decision"]),
                                                           p(o["seq"]), p(o["deps"]), self.stream)
        assert rc == 0, self.L.smr_last_error()

    def fused(self, col, lay):
        buf, off, ln = lay
        i, o, p = self.ing_b, self.out["b"], lambda t: None if t is None else t.data_ptr()   # noqa: E731
        rc = self.L.smr_ep_leader_handle_wire_pre_accept_replies(self.b._h, p(buf), buf.numel(), p(off), p(ln), self.n, p(col), None, None, p(o["decision"]),
                                                                 p(o["seq"]), p(o["deps"]), p(i.others), i.other_cap, p(i.counts), p(i.consumed),
                                                                 p(i.status), self.stream)
        assert rc == 0, self.L.smr_last_error()

    def same_outputs(self, what, n_junk):
        torch = self.torch
        for k in ("decision", "seq", "deps"):
            assert torch.equal(self.out["a"][k], self.out["b"][k]), (what, k)
        ca, cb = self.ing_a.counts.tolist(), self.ing_b.counts.tolist()
        assert ca == cb == [self.n, n_junk, 0, 0], (what, ca, cb)
        assert torch.equal(self.ing_a.consumed, self.ing_b.consumed) and torch.equal(self.ing_a.status, self.ing_b.status), what
        d = self.out["b"]["decision"]
        return int((d == 3).sum()), int((d == 2).sum())


def step_parity(dev):
    import numpy as np
    rig = Rig(dev, 16)
    fast = slow = 0
    for t in range(4):
        col, lays, n_junk = rig.tick_frames()
        name = ("back_to_back", "emit_stride")[t % 2]
        rig.two_calls(col, lays[name]); rig.fused(col, lays[name])
        f, s = rig.same_outputs((t, name), n_junk)
        fast += f; slow += s
        ra, rb = rig.ing_a.results(), rig.ing_b.results()
        srt = lambda q: np.sort(q, order=["conn", "off"])   # noqa: E731
        assert len(ra["others"]) == n_junk and np.array_equal(srt(ra["others"]), srt(rb["others"])), (t, "others")
    da, db = rig.a.dump(), rig.b.dump()
    for k in da:
        assert np.array_equal(da[k], db[k]), ("state", k)
    assert fast > 0 and slow > 0
    print(json.dumps({"step": "parity", "ok": True, "ticks": 4, "fast": fast, "slow": slow, "connections": rig.n}), flush=True)


def step_time(dev, reps, warmup):
    import numpy as np
    import torch
    W = 8
    while W < 2 * (warmup + reps) + 8:                                        # every repetition proposes one instance per group: the ring never wraps
        W *= 2
    rig = Rig(dev, W)
    ev = lambda: torch.cuda.Event(enable_timing=True)   # noqa: E731
    us = {lay: {"fused": [], "two_calls": []} for lay in ("back_to_back", "emit_stride")}
    fast = slow = 0
    for r in range(2 * (warmup + reps)):
        name = ("back_to_back", "emit_stride")[r % 2]
        col, lays, n_junk = rig.tick_frames()
        lay = lays[name]
        order = (("two_calls", rig.two_calls), ("fused", rig.fused))
        if (r // 2) % 2:
            order = order[::-1]
        torch.cuda.synchronize()
        marks = []
        for what, fn in order:
            e0, e1 = ev(), ev()
            e0.record(); fn(col, lay); e1.record()
            marks.append((what, e0, e1))
        torch.cuda.synchronize()
        if r >= 2 * warmup:
            for what, e0, e1 in marks:
                us[name][what].append(e0.elapsed_time(e1) * 1e3)
        f, s = rig.same_outputs((r, name), n_junk)
        fast += f; slow += s

    def stats(x):
        q1, med, q3 = (float(v) for v in np.percentile(x, [25, 50, 75]))
        return {"median_us": round(med, 2), "q1_us": round(q1, 2), "q3_us": round(q3, 2), "iqr_us": round(q3 - q1, 2), "min_us": round(float(min(x)), 2), "n": len(x)}

    out = {"step": "time", "workload": "EPaxos PreAcceptReply frames -> decisions: %d connections (%d groups x %d peers), one reply each, ~15 %% with a located "
                                       "frame in front" % (rig.n, G, R - 1), "device": torch.cuda.get_device_name(0), "warmup": warmup,
           "fast_decisions": fast, "slow_decisions": slow, "same_outputs_every_repetition": True, "layouts": {}}
    for lay, d in us.items():
        sf, st = stats(d["fused"]), stats(d["two_calls"])
        spread = max(sf["iqr_us"], st["iqr_us"])
        delta = round(sf["median_us"] - st["median_us"], 2)
        out["layouts"][lay] = {"fused": sf, "two_calls": st, "fused_minus_two_calls_us": delta, "spread_us": spread,
                               "verdict": "faster" if -delta > spread else "slower" if delta > spread else "a wash"}
    print(json.dumps(out), flush=True)


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--step", choices=("parity", "time"), help="run one step in this process (default: both, each a child under `timeout -k 10`)")
    ap.add_argument("--reps", type=int, default=40)
    ap.add_argument("--warmup", type=int, default=4)
    args = ap.parse_args()
    assert args.reps >= 30, "at least 30 repetitions per layout"
    if args.step:
        dev = need_gpu()
        return step_parity(dev) if args.step == "parity" else step_time(dev, args.reps, args.warmup)
    need_gpu()
    for step, limit in (("parity", 240), ("time", 300)):                     # the second only if the first succeeded
        rc = subprocess.run(["timeout", "-k", "10", str(limit), sys.executable, os.path.abspath(__file__), "--step", step, "--reps", str(args.reps),
                             "--warmup", str(args.warmup)]).returncode
        if rc != 0:
            sys.stderr.write("time_ep_wire_replies: step %s ended with status %d; stopping\n" % (step, rc))
            sys.exit(rc)


if __name__ == "__main__":
    main()
