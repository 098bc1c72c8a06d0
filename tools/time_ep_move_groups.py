#!/usr/bin/env python3
"""Chosen groups out of and into EPaxos replicas (`smr_ep_cluster_save_groups` / `_load_groups` / `_reset_groups`) beside the
whole-object calls (`smr_ep_cluster_save_state` / `_load_state`), timed with device events in one process.

    python tools/time_ep_move_groups.py > profiles/ep_move_groups.log
    python tools/time_ep_move_groups.py --whole-only           # the whole-object calls alone: runs on a commit without the group calls

Shape: the bench's EPaxos leg, the one tools/time_ep_snapshot.py uses (G = 65 536, R = 5, window 32, 64 keys, execution on, the
five replicas seated in an smr_ep_cluster and ticked by its one-launch tick; after 40 ticks every row has wrapped).  The five
replicas are the sources, five unseated replicas of the same shape the targets of the loads and resets.  Lists of n = 64, 1 024
and 16 384 groups as seeded random samples in random order, and the full ascending list (n = G), whose image is the whole-object
image but for the counters: its time beside the whole-object call's is what the list's indirection costs.
A call's time is what lies between two events on its stream: the list's copy and the one kernel over the five objects.

One child process under `timeout -k 10`: a parity check first (a random list saved and loaded: the targets' dump columns are the
sources'), then four warm-up passes of every call and >= 30 timed repetitions, the calls' order alternating within a
repetition; medians with quartiles and minima.  One JSON line per list and one for the whole-object calls.
No device visible: an error (exit status 2), never a fallback."""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

SIZES, SEED = (64, 1024, 16384), 0x6D6F7665


def step_time(G, ticks, reps, whole_only):
    import numpy as np
    import time_ep_snapshot as tes
    import torch
    from summerset_amd import EPaxosReplicaGroup, EPaxosSnapshot, epaxos
    note = lambda what: (sys.stderr.write("time_ep_move_groups: %s\n" % what), sys.stderr.flush())   # noqa: E731
    R, W, K = tes.R, tes.W, tes.K
    _, src, cl = tes.cluster(G, ticks)
    assert int(src[0].dump()["len"].min()) > W, "the rings have not wrapped: more --ticks"
    note("warm-up ticks done")

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

    dst = [EPaxosReplicaGroup(G, R, me=r, window=W, n_keys=K, execute=True) for r in range(R)]
    keep, scratch = epaxos.save_cluster_state(src), epaxos.save_cluster_state(src)
    info = keep[0].info()
    # (a load into the seated sources writes the cluster's shared per-key table, one into the unseated targets their private ones)
    full = timed([("cluster_save_state", lambda: epaxos.save_cluster_state(src, scratch)), ("cluster_load_state", lambda: epaxos.load_cluster_state(src, keep)),
                  ("cluster_load_state_unseated", lambda: epaxos.load_cluster_state(dst, keep))])
    for k in full:
        full[k]["us_per_group"] = round(full[k]["median_us"] / G, 5)
    print(json.dumps({"step": "full", "device": torch.cuda.get_device_name(0), "groups": G, "replicas": R, "window": W, "n_keys": K, "reps": reps,
                      "warmup_ticks": ticks, "replica_image": info, "calls": full}), flush=True)
    for s in scratch:
        s.close()
    note("whole-object calls done")
    if whole_only:
        return
    rng = np.random.default_rng(SEED)
    lst = rng.permutation(G)[:1024].astype(np.uint32)             # parity: by the targets' dump columns
    rs = epaxos.save_cluster_groups(src, lst)
    epaxos.load_cluster_groups(dst, rs, lst)
    for a, b in list(zip(src, dst))[::R - 1]:
        for x, y in ((a.dump(), b.dump()), (a.exec_dump(), b.exec_dump())):
            for k in x:
                if k != "counters":
                    xa, ya = (x[k][:, :, lst], y[k][:, :, lst]) if k == "deps" else (x[k][..., lst], y[k][..., lst])
                    assert np.array_equal(xa, ya), ("loaded", a.me, k)
    epaxos.reset_cluster_groups(dst, lst)
    assert all(not d.dump()["len"][:, lst].any() for d in dst[::R - 1])
    for s in rs:
        s.close()
    print(json.dumps({"step": "parity", "ok": True, "groups": G, "replicas": R, "window": W}), flush=True)
    whole = {"cluster_save_groups": "cluster_save_state", "cluster_load_groups": "cluster_load_state_unseated", "cluster_load_groups_seated": "cluster_load_state"}
    for n, order in [(min(n, G), "random") for n in SIZES] + [(G, "ascending")]:
        lst = np.arange(G, dtype=np.uint32) if order == "ascending" else np.random.default_rng(SEED + n).permutation(G)[:n].astype(np.uint32)
        s, kept = [EPaxosSnapshot(x, n) for x in src], epaxos.save_cluster_groups(src, lst)
        gi = kept[0].info()
        calls = [("cluster_save_groups", lambda: epaxos.save_cluster_groups(src, lst, s)), ("cluster_load_groups", lambda: epaxos.load_cluster_groups(dst, kept, lst)),
                 ("cluster_reset_groups", lambda: epaxos.reset_cluster_groups(dst, lst))]
        if order == "ascending":                                   # the sources' own state back into them: what cluster_load_state does
            calls.append(("cluster_load_groups_seated", lambda: epaxos.load_cluster_groups(src, kept, lst)))
        res = timed(calls)
        assert s[0].info() == gi                                   # the sources did not move
        for k in res:
            res[k]["us_per_group"] = round(res[k]["median_us"] / n, 5)
            if k in whole:
                res[k]["full_call_us"] = full[whole[k]]["median_us"]
                res[k]["share_of_full_call"] = round(res[k]["median_us"] / full[whole[k]]["median_us"], 4)
                res[k]["per_group_over_full_call"] = round(res[k]["us_per_group"] / full[whole[k]]["us_per_group"], 2)
        print(json.dumps({"step": "groups", "n": n, "order": order, "replica_image": gi, "calls": res}), flush=True)
        for x in s + kept:
            x.close()
        note("n = %d done" % n)
    cl.close()


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--step", choices=("time",), help="run in this process (default: a child under `timeout -k 10`)")
    ap.add_argument("--groups", type=int, default=65536)
    ap.add_argument("--ticks", type=int, default=40)
    ap.add_argument("--reps", type=int, default=31)
    ap.add_argument("--whole-only", action="store_true", help="only the whole-object calls (what an earlier commit has)")
    args = ap.parse_args()
    assert args.reps >= 30, "at least 30 repetitions"
    import torch
    if not torch.cuda.is_available():
        sys.stderr.write("time_ep_move_groups: no GPU is visible; this tool measures device calls and has no fallback\n")
        sys.exit(2)
    if args.step:
        return step_time(args.groups, args.ticks, args.reps, args.whole_only)
    cmd = ["timeout", "-k", "10", "540", sys.executable, os.path.abspath(__file__), "--step", "time", "--reps", str(args.reps), "--groups", str(args.groups),
           "--ticks", str(args.ticks)] + (["--whole-only"] if args.whole_only else [])
    rc = subprocess.run(cmd).returncode
    if rc != 0:
        sys.stderr.write("time_ep_move_groups: ended with status %d\n" % rc)
        sys.exit(rc)


if __name__ == "__main__":
    main()
