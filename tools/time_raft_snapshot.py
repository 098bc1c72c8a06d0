#!/usr/bin/env python3
"""Save and load of one Raft / CRaft replica's state (`smr_raft_save_state` / `smr_raft_load_state`) beside the trivial
alternative, device-to-device `hipMemcpyAsync` of the replica's whole arena (plus the CRaft block), timed with device events in
one process.

    python tools/time_raft_snapshot.py > profiles/raft_snapshot_vs_arena_copy.log

Shapes: the Raft leg's (`bench.py::raft_leg`: G = 65 536, R = 5, W = 512, S = 32 appends and four replies per group and tick;
the leader's object, its ring full after the warm-up) and the CRaft payload leg's engine shape
(`workloads.craft_payload_cluster`: G = 16 384, R = 5, W = 32, fault_tolerance 1; the leader's object, the engines' tick
without the payload bytes).

Steps, each a process of its own under `timeout -k 10`, the second only if the first succeeded, nothing retried:
  parity   a fresh replica loaded from the source's snapshot gives the source's dumps, and again after 8 more ticks on both
  time     24 ticks timed, a save; then >= 30 repetitions of save / load / arena copy, the order alternating within a
           repetition; then 24 ticks on the loaded replica, tick by tick beside a twin that ran the same ticks and was never
           saved or loaded (the control: same state at the end).  One JSON line per shape: medians, quartiles and the spread of
           the three, the image's bytes beside the arena's, the bytes each kernel moves (from the shapes) over its time, and us
           per tick before the save, after the load, and of the twin on the same ticks.
No device visible: an error (exit status 2), never a fallback."""
import argparse
import ctypes as C
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

STEADY, MORE = 24, 8


def need_gpu():
    import torch
    if not torch.cuda.is_available():
        sys.stderr.write("time_raft_snapshot: no GPU is visible; this tool measures device calls and has no fallback\n")
        sys.exit(2)
    return torch.device("cuda:0")


class RaftRig:
    """the Raft leg: leader objects fed S appends and one seeded reply per follower, group and tick"""
    name, G, R, W, S = "raft", 65536, 5, 512, 32

    def __init__(self, dev, n_ticks):
        import numpy as np
        import torch
        self.torch, self.dev = torch, dev
        G, R, S = self.G, self.R, self.S
        rng = np.random.default_rng(0x5EED5EED)
        self.n_new = torch.full((G,), S, dtype=torch.int32, device=dev)
        self.pool = []
        for t in range(n_ticks):
            last = S * (t + 1)
            u = rng.random((R, G))
            flags = (u >= 0.05).astype(np.uint8)
            term = np.full((R, G), 2, np.uint64)
            term[(u >= 0.05) & (u < 0.055)] = 1
            flags[(u >= 0.055) & (u < 0.06)] |= 2
            end_slot = np.maximum(last - rng.integers(0, 4, (R, G)), 0).astype(np.uint32)
            arrs = (term, end_slot, flags, np.full((R, G), 2, np.uint64), np.maximum(end_slot.astype(np.int64) - 1, 1).astype(np.uint32))
            self.pool.append(tuple(torch.from_numpy(x.view(np.int64) if x.dtype == np.uint64 else (x.view(np.int32) if x.dtype == np.uint32 else x)).to(dev)
                                   for x in arrs))

    def make(self):
        from summerset_amd import RaftLeaderGroup
        return RaftLeaderGroup(self.G, self.R, leader_id=0, window=self.W, term=2)

    def subject(self, x):
        return x

    def tick(self, x, t):
        rt, es, fl, ct, cs = self.pool[t]
        x.handle_req_batch(self.n_new)
        x.handle_msg_append_entries_reply(rt, es, fl, ct, cs)

    def dumps(self, x):
        return [x.dump(), x.dump_votes(), {"total_commits": x.total_commits(), "ring_guard_hits": x.ring_guard_hits()}]

    def close(self, x):
        x.close()


class CraftRig:
    """the CRaft payload leg's engines: a co-located cluster's one-launch tick, one batch per group, without the payload bytes"""
    name = "craft"

    def __init__(self, dev, n_ticks):
        import torch
        from summerset_amd import workloads
        self.torch, self.dev, self.wl = torch, dev, workloads
        self.G, self.R, self.W = (workloads.CRAFT_PAYLOAD[k] for k in ("G", "R", "W"))

    def make(self):
        # workloads.craft_payload_cluster without its payload stores (gigabytes of shard bytes this tool never touches)
        from summerset_amd import CRaftLeaderGroup
        torch, G, R, dev = self.torch, self.G, self.R, self.dev
        reps = [CRaftLeaderGroup(G, R, leader_id=r, window=self.W, term=1, fault_tolerance=self.wl.CRAFT_PAYLOAD["ft"]) for r in range(R)]
        for r in range(1, R):
            reps[r].preset(0, 0, 1)
        _, send = reps[0].assignment(dev)
        z = lambda shape, dt: torch.zeros(shape, dtype=dt, device=dev)   # noqa: E731
        bufs = dict(ones=torch.ones(G, dtype=torch.int32, device=dev), em=[send[q].to(torch.uint8).reshape(1, G).contiguous() for q in range(R)],
                    rt=z((R, G), torch.int64), es=z((R, G), torch.int32), fl=z((R, G), torch.uint8), ct=z((R, G), torch.int64), cs=z((R, G), torch.int32),
                    first=z((R, G), torch.int32), msg=[None] * R)
        return (reps, bufs)

    def subject(self, x):
        return x[0][0]                                               # the leader's object

    def tick(self, x, t):
        self.wl.craft_payload_tick(x[0], None, x[1], None, None, bytes_=False)

    def dumps(self, x):
        e = self.subject(x)
        return [e.dump(), e.dump_votes(), e.dump_craft(), e.dump_masks(), {"total_commits": e.total_commits()}]

    def close(self, x):
        for e in x[0]:
            e.close()


RIGS = {"raft": RaftRig, "craft": CraftRig}


def same(rig, a, b, what):
    import numpy as np
    for x, y in zip(rig.dumps(a), rig.dumps(b)):
        for k in x:
            assert np.array_equal(np.asarray(x[k]), np.asarray(y[k])), (rig.name, what, k)


def step_parity(dev, warm):
    for cls in RIGS.values():
        rig = cls(dev, warm + MORE)
        a, b = rig.make(), rig.make()
        for t in range(warm):
            rig.tick(a, t)
        snap = rig.subject(a).save_state()
        info = snap.info()
        if rig.name == "craft":                                      # the followers of b must hold what a's do: the whole cluster travels
            from summerset_amd import load_cluster_state, save_cluster_state
            load_cluster_state(b[0], save_cluster_state(a[0]))
        else:
            rig.subject(b).load_state(snap)
        same(rig, a, b, "loaded")
        for t in range(warm, warm + MORE):
            rig.tick(a, t); rig.tick(b, t)
        same(rig, a, b, "%d ticks on" % MORE)
        assert rig.subject(a).total_commits() > 0 and info["n_entries"] > 0
        print(json.dumps({"step": "parity", "shape": rig.name, "ok": True, "groups": rig.G, "window": rig.W, "warmup_ticks": warm, "snapshot": info}), flush=True)
        rig.close(a); rig.close(b)


def step_time(dev, warm, reps):
    import numpy as np
    import torch
    from summerset_amd import _lib
    note = lambda what: (sys.stderr.write("time_raft_snapshot: %s\n" % what), sys.stderr.flush())   # noqa: E731
    hip = C.CDLL("libamdhip64.so")
    hip.hipMemcpyAsync.restype = C.c_int
    hip.hipMemcpyAsync.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int, C.c_void_p]
    st = _lib.stream_ptr(None)

    def timed_ticks(rig, engines, t0, t1):
        """ticks [t0, t1) on every engine, each engine's tick between its own events, the order alternating: us per tick, per engine"""
        out = [[] for _ in engines]
        for t in range(t0, t1):
            torch.cuda.synchronize()
            marks = []
            for i in (range(len(engines)) if t % 2 == 0 else reversed(range(len(engines)))):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record(); rig.tick(engines[i], t); e1.record()
                marks.append((i, e0, e1))
            torch.cuda.synchronize()
            for i, e0, e1 in marks:
                out[i].append(e0.elapsed_time(e1) * 1e3)
        return out

    def stats(x, nd=2):
        q1, med, q3 = (float(v) for v in np.percentile(x, [25, 50, 75]))
        return {"median_us": round(med, nd), "q1_us": round(q1, nd), "q3_us": round(q3, nd), "iqr_us": round(q3 - q1, nd), "min_us": round(float(min(x)), nd), "n": len(x)}
    for cls in RIGS.values():
        rig = cls(dev, warm + 2 * STEADY)
        a, twin = rig.make(), rig.make()                            # the twin runs the same ticks and is never saved or loaded: the control
        for t in range(warm):
            rig.tick(a, t); rig.tick(twin, t)
        before, _ = timed_ticks(rig, [a, twin], warm, warm + STEADY)
        note("%s: %d ticks before the save done" % (rig.name, STEADY))
        e = rig.subject(a)
        keep = e.save_state()                                         # what the loads take
        info = keep.info()
        scratch = e.save_state()                                      # what the timed saves fill
        scratch.info()
        pieces = e.debug_arena_view()
        arena_bytes = sum(n for _, n in pieces)
        copies = [torch.empty(n, dtype=torch.uint8, device=dev) for _, n in pieces]

        def save():
            e.save_state(scratch)

        def load():
            e.load_state(keep)

        def copy():
            for (p, n), dst in zip(pieces, copies):
                rc = hip.hipMemcpyAsync(dst.data_ptr(), p, n, 3, st)   # hipMemcpyDeviceToDevice
                assert rc == 0, rc
        calls = [("save", save), ("load", load), ("arena_copy", copy)]
        us = {k: [] for k, _ in calls}
        for r in range(4 + reps):
            order = calls[r % 3:] + calls[:r % 3]
            if (r // 3) % 2:
                order = order[::-1]
            torch.cuda.synchronize()
            marks = []
            for what, fn in order:
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record(); fn(); e1.record()
                marks.append((what, e0, e1))
            torch.cuda.synchronize()
            assert scratch.info() == info                             # the state did not move: every save sees the one the loads restore
            if r >= 4:
                for what, e0, e1 in marks:
                    us[what].append(e0.elapsed_time(e1) * 1e3)
        note("%s: %d repetitions done" % (rig.name, reps))
        after, control = timed_ticks(rig, [a, twin], warm + STEADY, warm + 2 * STEADY)
        same(rig, a, twin, "%d ticks after the loads" % STEADY)
        G, R, craft = rig.G, rig.R, info["craft"]
        scal = G * (8 + 7 * 4 + 4 + 3 * 4 * R) + 256 * 64 + (G * (17 * R + 8 + 3) if craft else 0)   # the arena's side of the scalars and peer rows, the counter shards
        ring = info["n_entries"] * (9 if craft else 8) + info["n_reconstructs"] * 12
        nblock = (((G + 63) // 64 + 3) // 4)
        prefix = nblock * G * (16 if craft else 12) // 2              # every block sums the counts in front of it, half of the groups on average
        moved = {"save": {"reads": scal + ring, "writes": info["bytes"], "prefix_reads_l2": prefix},
                 "load": {"reads": info["bytes"], "writes": scal + ring, "prefix_reads_l2": prefix},
                 "arena_copy": {"reads": arena_bytes, "writes": arena_bytes}}
        out = {"step": "time", "shape": rig.name, "workload": "%s: %d groups x %d replicas, W = %d, the leader's object; %d warm-up + %d ticks, then save / load / arena copy"
                                                              % (rig.name, G, R, rig.W, warm, STEADY),
               "device": torch.cuda.get_device_name(0), "reps": reps, "snapshot": info, "image_bytes": info["bytes"], "arena_bytes": arena_bytes,
               "arena_pieces": [n for _, n in pieces], "calls": {}}
        for k, _ in calls:
            s = stats(us[k])
            s["bytes"] = moved[k]
            s["tb_per_s"] = round((moved[k]["reads"] + moved[k]["writes"]) / (s["median_us"] * 1e-6) / 1e12, 3)
            out["calls"][k] = s
        spread = max(out["calls"][k]["iqr_us"] for k in out["calls"])
        for k in ("save", "load"):
            d = out["calls"]["arena_copy"]["median_us"] - out["calls"][k]["median_us"]
            out["calls"][k]["arena_copy_over_this"] = round(out["calls"]["arena_copy"]["median_us"] / out["calls"][k]["median_us"], 2)
            out["calls"][k]["verdict"] = "faster than the arena copy" if d > spread else "slower" if -d > spread else "a wash"
        sb, sa, sc = stats(before), stats(after), stats(control)
        out["ticks_before_save"], out["ticks_after_load"], out["same_ticks_never_loaded"] = sb, sa, sc
        out["after_load_within_spread_of_never_loaded"] = abs(sa["median_us"] - sc["median_us"]) <= max(sa["iqr_us"], sc["iqr_us"])
        out["same_state_as_never_loaded"] = True
        print(json.dumps(out), flush=True)
        for x in (keep, scratch):
            x.close()
        rig.close(a); rig.close(twin)
        del copies


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--step", choices=("parity", "time"), help="run one step in this process (default: both, each a child under `timeout -k 10`)")
    ap.add_argument("--reps", type=int, default=33)
    ap.add_argument("--warmup", type=int, default=24)
    args = ap.parse_args()
    assert args.reps >= 30, "at least 30 repetitions"
    if args.step:
        dev = need_gpu()
        return step_parity(dev, args.warmup) if args.step == "parity" else step_time(dev, args.warmup, args.reps)
    need_gpu()
    for step, limit in (("parity", 300), ("time", 300)):                     # the second only if the first succeeded
        rc = subprocess.run(["timeout", "-k", "10", str(limit), sys.executable, os.path.abspath(__file__), "--step", step, "--reps", str(args.reps),
                             "--warmup", str(args.warmup)]).returncode
        if rc != 0:
            sys.stderr.write("time_raft_snapshot: step %s ended with status %d; stopping\n" % (step, rc))
            sys.exit(rc)


if __name__ == "__main__":
    main()
