#!/usr/bin/env python3
"""Chosen groups out of and into Raft replica objects (`smr_raft_save_groups` / `smr_raft_load_groups` / `smr_raft_reset_groups`
and their cluster forms) beside the whole-object calls (`smr_raft_save_state` / `smr_raft_load_state`,
`smr_raft_cluster_save_state` / `_load_state`), timed with device events in one process.

    python tools/time_raft_move_groups.py > profiles/raft_move_groups.log

Shape: config 2's, the Raft leg's (`tools/time_raft_snapshot.py::RaftRig`: G = 65 536, R = 5, W = 512, S = 32 appends and four
replies per group and tick; leader objects, their rings full after the warm-up ticks).  R objects (replica ids 0 .. R - 1) are the
co-located cluster the cluster forms work on, R more of the same shape the targets; the single calls work on the first of each.
Lists of n = 64, 1 024 and 16 384 groups, each in two orders:
  ascending  n consecutive groups from a tile boundary: whole 64-group tiles, the replica side as contiguous as the full call's
  random     a seeded sample of the object's groups in random order: the replica side pays a line per element
The figure to read is us per listed group beside the full call's us per group.  A call's time is what lies between two events on
its stream: the list's host-to-device copy and the one kernel.

One child process under `timeout -k 10`: a parity check first (the groups loaded into the targets give the sources' dump
columns), then warm-up passes of every call and >= 30 timed repetitions, the calls' order alternating within a repetition.  One
JSON line per list and one for the full calls: medians, quartiles, spread.
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
    import time_raft_snapshot as trs
    import torch
    from summerset_amd import (RaftLeaderGroup, RaftSnapshot, load_cluster_groups, load_cluster_state, reset_cluster_groups, save_cluster_groups,
                               save_cluster_state)
    note = lambda what: (sys.stderr.write("time_raft_move_groups: %s\n" % what), sys.stderr.flush())   # noqa: E731
    rig = trs.RaftRig(dev, warm)
    G, R, W = rig.G, rig.R, rig.W
    new = lambda: [RaftLeaderGroup(G, R, leader_id=r, window=W, term=2) for r in range(R)]   # noqa: E731
    src, dst = new(), new()
    for t in range(warm):
        for x in src:
            rig.tick(x, t)
    note("warm-up done")
    # parity: an ascending and a random list through the cluster forms, by the targets' dump columns
    for lst in lists(G, 1024).values():
        snaps = save_cluster_groups(src, lst)
        load_cluster_groups(dst, snaps, lst)
        for a, b in list(zip(src, dst))[::R - 1]:                   # (the first and the last replica: a dump of this shape is 268 MB)
            for x, y in ((a.dump(), b.dump()), (a.dump_votes(), b.dump_votes())):
                for k in x:
                    assert np.array_equal(x[k][..., lst], y[k][..., lst]), ("loaded", a.me, k)
        reset_cluster_groups(dst, lst)
        for s in snaps:
            s.close()
    print(json.dumps({"step": "parity", "ok": True, "groups": G, "replicas": R, "window": W, "warmup_ticks": warm}), flush=True)

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

    # the full calls, at the code path they have always had: one object, and the R objects in one launch
    keep, scratch = save_cluster_state(src), save_cluster_state(src)
    info = keep[0].info()
    full = timed([("save_state", lambda: src[0].save_state(scratch[0])), ("load_state", lambda: src[0].load_state(keep[0])),
                  ("cluster_save_state", lambda: save_cluster_state(src, scratch)), ("cluster_load_state", lambda: load_cluster_state(src, keep))])
    for k in full:
        full[k]["us_per_group"] = round(full[k]["median_us"] / G, 5)
    print(json.dumps({"step": "full", "device": torch.cuda.get_device_name(0), "groups": G, "replicas": R, "reps": reps, "snapshot": info, "calls": full}), flush=True)
    for s in scratch:
        s.close()
    note("full calls done")
    whole = {"save_groups": "save_state", "load_groups": "load_state", "cluster_save_groups": "cluster_save_state", "cluster_load_groups": "cluster_load_state"}
    for n in SIZES:
        for order, lst in lists(G, n).items():
            s = [RaftSnapshot(x, n) for x in src]
            save_cluster_groups(src, lst, s)
            gi = s[0].info()
            kept = save_cluster_groups(src, lst)                   # what the timed loads take
            for k in kept:
                k.info()
            res = timed([("save_groups", lambda: src[0].save_groups(lst, s[0])), ("load_groups", lambda: dst[0].load_groups(kept[0], lst)),
                         ("reset_groups", lambda: dst[0].reset_groups(lst)),
                         ("cluster_save_groups", lambda: save_cluster_groups(src, lst, s)), ("cluster_load_groups", lambda: load_cluster_groups(dst, kept, lst)),
                         ("cluster_reset_groups", lambda: reset_cluster_groups(dst, lst))])
            assert s[0].info() == gi                               # the source did not move
            for k in res:
                res[k]["us_per_group"] = round(res[k]["median_us"] / n, 5)
                if k in whole:
                    res[k]["full_call_us_per_group"] = full[whole[k]]["us_per_group"]
                    res[k]["per_group_over_full_call"] = round(res[k]["us_per_group"] / full[whole[k]]["us_per_group"], 2)
                    res[k]["full_call_over_this"] = round(full[whole[k]]["median_us"] / res[k]["median_us"], 2)
            print(json.dumps({"step": "groups", "n": n, "order": order, "image": gi, "calls": res}), flush=True)
            for x in s + kept:
                x.close()
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
        sys.stderr.write("time_raft_move_groups: no GPU is visible; this tool measures device calls and has no fallback\n")
        sys.exit(2)
    dev = torch.device("cuda:0")
    if args.step:
        return step_time(dev, args.warmup, args.reps)
    rc = subprocess.run(["timeout", "-k", "10", "540", sys.executable, os.path.abspath(__file__), "--step", "time", "--reps", str(args.reps),
                         "--warmup", str(args.warmup)]).returncode
    if rc != 0:
        sys.stderr.write("time_raft_move_groups: ended with status %d\n" % rc)
        sys.exit(rc)


if __name__ == "__main__":
    main()
