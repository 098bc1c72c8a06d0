#!/usr/bin/env python3
"""Save and load of a MultiPaxos cluster's state (`smr_mp_save_state` / `smr_mp_load_state`) beside the trivial alternative, one
device-to-device `hipMemcpyAsync` of the cluster's whole arena, timed with device events in one process.

    python tools/time_mp_snapshot.py > profiles/mp_snapshot_vs_arena_copy.log

Shape: the headline line's (`workloads.headline_cluster` / `headline_stream`: G = 65 536, R = 5, S = 32, W = 512, the bench's
timeout rate), after warm-up ticks.

Steps, each a process of its own under `timeout -k 10`, the second only if the first succeeded, nothing retried:
  parity   a fresh cluster loaded from the source's snapshot gives the source's `dump_range` slices, and again after 8 more
           ticks on both
  time     60 ticks timed, a save; then >= 30 repetitions of save / load / arena copy, the order alternating within a
           repetition; then 60 ticks on the loaded cluster, batch by batch beside a twin that ran the same ticks and was never
           saved or loaded (the control: same state at the end).  One JSON line: medians, quartiles and the spread of the
           three, the image's bytes beside the arena's, the bytes each kernel moves (from the shapes) over its time, and ms
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

G, TIMEOUTS, HORIZON, POOL, BATCH = 65536, 0.01, 72, 4, 8
SLICES = ((0, 128), (32704, 128), (65408, 128))               # dump_range pieces: both ends and the middle


def need_gpu():
    import torch
    if not torch.cuda.is_available():
        sys.stderr.write("time_mp_snapshot: no GPU is visible; this tool measures device calls and has no fallback\n")
        sys.exit(2)
    return torch.device("cuda:0")


class Rig:
    """the headline cluster and its stream; tick inputs resident on the device (a pool of POOL ticks' batches and reply
    orders, the per-tick timer events as they come)"""

    def __init__(self, dev, n_ticks, groups=G):
        import torch
        from summerset_amd import workloads
        self.torch, self.dev, self.G, self.wl = torch, dev, groups, workloads
        self.st = workloads.headline_stream(groups, n_ticks, min(1.0, TIMEOUTS * n_ticks / HORIZON), n_ticks)
        self.pool = []
        for t in range(POOL):
            x = self.st.tick(t)
            self.pool.append({k: torch.from_numpy(x[k]).to(dev) for k in ("req_cnt", "req_val", "ackctl")})

    def cluster(self):
        return self.wl.headline_cluster(self.G)

    def tick_args(self, t):
        torch = self.torch
        e, p = self.st.tick_events(t), self.pool[t % POOL]
        fired = bool((e["timeout_rep"] != 0xFF).any())
        up = lambda a: torch.from_numpy(a).to(self.dev)   # noqa: E731
        return dict(timeout_rep=up(e["timeout_rep"]) if fired else None, timeout_src=up(e["timeout_src"]) if fired else None,
                    req_target=up(e["req_target"]), req_cnt=p["req_cnt"], req_val=p["req_val"], ackctl=p["ackctl"],
                    heartbeat=self.st.heartbeat(t))

    def run(self, engines, t0, t1, timed=False):
        """ticks [t0, t1) in batches of BATCH on every engine; timed: ms per tick of each batch (first engine)"""
        torch = self.torch
        out = []
        for ch in self.wl.batches(t0, t1, BATCH):
            args = [self.tick_args(t) for t in ch]
            torch.cuda.synchronize()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            for i, eng in enumerate(engines):
                if i == 0:
                    e0.record()
                eng.run_ticks(args)
                if i == 0:
                    e1.record()
            torch.cuda.synchronize()
            if timed:
                out.append(e0.elapsed_time(e1) / len(ch))
        return out

    def run_side_by_side(self, engines, t0, t1):
        """ticks [t0, t1) in batches of BATCH on every engine, each engine's batch between its own events, the order alternating
        from batch to batch: ms per tick of every batch, per engine"""
        torch = self.torch
        out = [[] for _ in engines]
        for n, ch in enumerate(self.wl.batches(t0, t1, BATCH)):
            args = [self.tick_args(t) for t in ch]
            torch.cuda.synchronize()
            marks = []
            for i in (range(len(engines)) if n % 2 == 0 else reversed(range(len(engines)))):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record(); engines[i].run_ticks(args); e1.record()
                marks.append((i, e0, e1))
            torch.cuda.synchronize()
            for i, e0, e1 in marks:
                out[i].append(e0.elapsed_time(e1) / len(ch))
        return out


def same_slices(a, b, R, what):
    import numpy as np
    for g0, n in SLICES:
        for r in range(R):
            x, y = a.dump(r, g0, n), b.dump(r, g0, n)
            for k in x:
                assert np.array_equal(x[k], y[k]), (what, g0, r, k)


def step_parity(dev, warm):
    rig = Rig(dev, warm + 8)
    a = rig.cluster()
    rig.run([a], 0, warm)
    snap = a.save_state()
    info = snap.info()
    b = rig.cluster()
    b.load_state(snap)
    same_slices(a, b, 5, "loaded")
    rig.run([a, b], warm, warm + 8)
    same_slices(a, b, 5, "8 ticks on")
    for r in range(5):
        assert a.counters(r) == b.counters(r), r
    assert a.counters(0)["commits"] > 0 and info["n_slots"] > 0
    print(json.dumps({"step": "parity", "ok": True, "groups": G, "warmup_ticks": warm, "slices": [list(s) for s in SLICES], "snapshot": info}), flush=True)


def step_time(dev, warm, reps):
    import numpy as np
    import torch
    from summerset_amd import _lib
    steady = 60
    note = lambda what: (sys.stderr.write("time_mp_snapshot: %s\n" % what), sys.stderr.flush())   # noqa: E731
    rig = Rig(dev, warm + 2 * steady)
    a, twin_cluster = rig.cluster(), rig.cluster()                  # the twin runs the same ticks and is never saved or loaded: the control
    rig.run([a, twin_cluster], 0, warm)
    note("warm-up done")
    before = rig.run([a, twin_cluster], warm, warm + steady, timed=True)
    note("%d ticks before the save done" % steady)
    keep = a.save_state()                                          # what the loads take
    info = keep.info()
    scratch = a.save_state()                                       # what the timed saves fill
    scratch.info()
    base, arena_bytes = a.debug_arena_view()
    twin = torch.empty(arena_bytes, dtype=torch.uint8, device=dev)
    hip = C.CDLL("libamdhip64.so")
    hip.hipMemcpyAsync.restype = C.c_int
    hip.hipMemcpyAsync.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int, C.c_void_p]
    st = _lib.stream_ptr(None)

    def save():
        a.save_state(scratch)

    def load():
        a.load_state(keep)

    def copy():
        rc = hip.hipMemcpyAsync(twin.data_ptr(), base, arena_bytes, 3, st)   # hipMemcpyDeviceToDevice
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
        assert scratch.info() == info                              # the state did not move: every save sees the one the loads restore
        if r >= 4:
            for what, e0, e1 in marks:
                us[what].append(e0.elapsed_time(e1) * 1e3)
    note("%d repetitions done" % reps)
    after, control = rig.run_side_by_side([a, twin_cluster], warm + steady, warm + 2 * steady)
    same_slices(a, twin_cluster, 5, "%d ticks after the loads" % steady)

    def stats(x, unit="us", nd=2):
        q1, med, q3 = (float(v) for v in np.percentile(x, [25, 50, 75]))
        return {"median_" + unit: round(med, nd), "q1_" + unit: round(q1, nd), "q3_" + unit: round(q3, nd), "iqr_" + unit: round(q3 - q1, nd),
                "min_" + unit: round(float(min(x)), nd), "n": len(x)}
    R, GR = 5, G * 5
    scal = GR * (1 + 3 * 8 + 6 * 4 + 4 * R + 4 + 4 + 4)            # leader, ballots, bars, peer_exec_bar, bal_lo / null_lb, outbox count and descriptor
    ring = info["n_slots"] * 16 + info["n_outbox"] * 20           # ballot, token and meta word per live slot; an outbox entry's four words
    nblock = (((G + 63) // 64 + 3) // 4)
    prefix = nblock * GR * 12 // 2                                # every block sums the counts in front of it: 12 B per (replica, group), half of them on average
    moved = {"save": {"reads": scal + ring, "writes": info["bytes"], "prefix_reads_l2": prefix},
             "load": {"reads": info["bytes"], "writes": scal + ring, "prefix_reads_l2": prefix},
             "arena_copy": {"reads": arena_bytes, "writes": arena_bytes}}
    out = {"step": "time", "workload": "MultiPaxos headline shape: %d groups x 5 replicas, S = 32, W = 512, %d warm-up + %d ticks, then save / load / "
                                       "arena copy" % (G, warm, steady), "device": torch.cuda.get_device_name(0), "reps": reps,
           "snapshot": info, "image_bytes": info["bytes"], "arena_bytes": arena_bytes, "calls": {}}
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
    sb, sa = stats(before, "ms_per_tick", 5), stats(after, "ms_per_tick", 5)
    out["ticks_before_save"], out["ticks_after_load"] = sb, sa
    tick_spread = max(sb["iqr_ms_per_tick"], sa["iqr_ms_per_tick"])
    out["after_load_within_spread_of_before"] = abs(sa["median_ms_per_tick"] - sb["median_ms_per_tick"]) <= tick_spread
    # the same ticks on a cluster that was never saved or loaded: what the later ticks cost whatever load did
    sc = stats(control, "ms_per_tick", 5)
    out["same_ticks_never_loaded"] = sc
    out["after_load_within_spread_of_never_loaded"] = abs(sa["median_ms_per_tick"] - sc["median_ms_per_tick"]) <= max(sa["iqr_ms_per_tick"], sc["iqr_ms_per_tick"])
    out["same_state_as_never_loaded"] = True
    print(json.dumps(out), flush=True)


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
    for step, limit in (("parity", 300), ("time", 420)):                     # the second only if the first succeeded
        rc = subprocess.run(["timeout", "-k", "10", str(limit), sys.executable, os.path.abspath(__file__), "--step", step, "--reps", str(args.reps),
                             "--warmup", str(args.warmup)]).returncode
        if rc != 0:
            sys.stderr.write("time_mp_snapshot: step %s ended with status %d; stopping\n" % (step, rc))
            sys.exit(rc)


if __name__ == "__main__":
    main()
