#!/usr/bin/env python3
"""Chosen groups out of and into a MultiPaxos cluster (`smr_mp_save_groups` / `smr_mp_load_groups` / `smr_mp_reset_groups`) beside
the whole-cluster calls (`smr_mp_save_state` / `smr_mp_load_state`), timed with device events in one process.

    python tools/time_mp_move_groups.py > profiles/mp_move_groups.log

Shape: the headline line's (`workloads.headline_cluster` / `headline_stream`: G = 65 536, R = 5, S = 32, W = 512, the bench's
timeout rate), after warm-up ticks; a second cluster of the same shape is the target.  Lists of n = 64, 1 024 and 16 384 groups,
each in two orders:
  ascending  n consecutive groups from a tile boundary: whole 64-group tiles, the cluster side as contiguous as the full call's
  random     a seeded sample of the cluster's groups in random order: the cluster side pays a line per element
The figure to read is us per listed group beside the full call's us per group.  A call's time is what lies between two events on
its stream: the list's host-to-device copy and the one kernel.

One child process under `timeout -k 10`: a parity check first (the groups loaded into the target give the source's
`dump_range` slices), then a warm-up pass of every call and >= 30 timed repetitions, the calls' order alternating within a
repetition.  One JSON line per list and one for the full calls: medians, quartiles, spread.
No device visible: an error (exit status 2), never a fallback."""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

SIZES, SEED, FIRST = (64, 1024, 16384), 0x6D6F7665, 4096


def lists(G, n):
    import numpy as np
    rng = np.random.default_rng(SEED + n)
    return {"ascending": np.arange(FIRST, FIRST + n, dtype=np.uint32), "random": rng.permutation(G)[:n].astype(np.uint32)}


def step_time(dev, warm, reps):
    import numpy as np
    import time_mp_snapshot as tms
    import torch
    from summerset_amd import MpSnapshot
    G, R = tms.G, 5
    note = lambda what: (sys.stderr.write("time_mp_move_groups: %s\n" % what), sys.stderr.flush())   # noqa: E731
    rig = tms.Rig(dev, warm)
    a, b = rig.cluster(), rig.cluster()
    rig.run([a], 0, warm)
    note("warm-up done")
    # parity: the first two tiles of an ascending list, through the target's dump_range slices
    asc = lists(G, 1024)["ascending"]
    snap = a.save_groups(asc)
    b.load_groups(snap, asc)
    for r in range(R):
        x, y = a.dump(r, FIRST, 128), b.dump(r, FIRST, 128)
        for k in x:
            assert np.array_equal(x[k], y[k]), ("loaded", r, k)
    b.reset_groups(asc)
    snap.close()
    print(json.dumps({"step": "parity", "ok": True, "groups": G, "warmup_ticks": warm}), flush=True)

    def stats(x):
        q1, med, q3 = (float(v) for v in np.percentile(x, [25, 50, 75]))
        return {"median_us": round(med, 2), "q1_us": round(q1, 2), "q3_us": round(q3, 2), "iqr_us": round(q3 - q1, 2), "min_us": round(float(min(x)), 2), "n": len(x)}

    def timed(calls):
        us = {k: [] for k, _ in calls}
        for r in range(4 + reps):                                  # four warm-up passes, then the timed ones
            order = calls[r % len(calls):] + calls[:r % len(calls)]
            if (r // len(calls)) % 2:
                order = order[::-1]
            torch.cuda.synchronize()
            marks = []
            for what, fn in order:
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record(); fn(); e1.record()
                marks.append((what, e0, e1))
            torch.cuda.synchronize()
            if r >= 4:
                for what, e0, e1 in marks:
                    us[what].append(e0.elapsed_time(e1) * 1e3)
        return {k: stats(v) for k, v in us.items()}

    # the full calls, at the code path they have always had
    keep, scratch = a.save_state(), a.save_state()
    info = keep.info()
    full = timed([("save_state", lambda: a.save_state(scratch)), ("load_state", lambda: a.load_state(keep))])
    for k in full:
        full[k]["us_per_group"] = round(full[k]["median_us"] / G, 5)
    print(json.dumps({"step": "full", "device": torch.cuda.get_device_name(0), "groups": G, "reps": reps, "snapshot": info, "calls": full}), flush=True)
    scratch.close()
    note("full calls done")
    for n in SIZES:
        for order, lst in lists(G, n).items():
            s = MpSnapshot(a, n)
            a.save_groups(lst, s)
            gi = s.info()
            kept = a.save_groups(lst)                              # what the timed loads take
            kept.info()
            res = timed([("save_groups", lambda: a.save_groups(lst, s)), ("load_groups", lambda: b.load_groups(kept, lst)),
                         ("reset_groups", lambda: b.reset_groups(lst))])
            assert s.info() == gi                                  # the source did not move
            for k, whole in (("save_groups", "save_state"), ("load_groups", "load_state"), ("reset_groups", None)):
                res[k]["us_per_group"] = round(res[k]["median_us"] / n, 5)
                if whole:
                    res[k]["full_call_us_per_group"] = full[whole]["us_per_group"]
                    res[k]["per_group_over_full_call"] = round(res[k]["us_per_group"] / full[whole]["us_per_group"], 2)
                    res[k]["full_call_over_this"] = round(full[whole]["median_us"] / res[k]["median_us"], 2)
            print(json.dumps({"step": "groups", "n": n, "order": order, "image": gi, "calls": res}), flush=True)
            s.close(); kept.close()
        note("n = %d done" % n)


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--step", choices=("time",), help="run in this process (default: a child under `timeout -k 10`)")
    ap.add_argument("--reps", type=int, default=33)
    ap.add_argument("--warmup", type=int, default=24)
    args = ap.parse_args()
    assert args.reps >= 30, "at least 30 repetitions"
    import torch
    if not torch.cuda.is_available():
        sys.stderr.write("time_mp_move_groups: no GPU is visible; this tool measures device calls and has no fallback\n")
        sys.exit(2)
    dev = torch.device("cuda:0")
    if args.step:
        return step_time(dev, args.warmup, args.reps)
    rc = subprocess.run(["timeout", "-k", "10", "540", sys.executable, os.path.abspath(__file__), "--step", "time", "--reps", str(args.reps),
                         "--warmup", str(args.warmup)]).returncode
    if rc != 0:
        sys.stderr.write("time_mp_move_groups: ended with status %d\n" % rc)
        sys.exit(rc)


if __name__ == "__main__":
    main()
