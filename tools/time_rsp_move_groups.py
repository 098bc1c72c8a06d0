#!/usr/bin/env python3
"""Chosen groups out of and into RSPaxos replicas with their payload stores (`smr_rsp_cluster_save_groups` / `_load_groups` /
`_reset_groups` and `smr_rsp_pstore_save_groups` / `_load_groups` / `_reset_groups`) beside the whole-object calls
(`smr_rsp_cluster_save_state` / `_load_state`, `smr_rsp_pstore_save` / `_load`), timed with device events in one process.

    python tools/time_rsp_move_groups.py > profiles/rsp_move_groups.log
    python tools/time_rsp_move_groups.py --whole-only          # the whole-object calls alone: runs on a commit without the group calls

Shape: config 4's, the one tools/time_rsp_snapshot.py uses (`workloads.config4_payload_cluster`: G = 16 384, R = 5, the store's
window of 16, L = 4113; the rings wrapped after the warm-up ticks).  The five replicas and their five stores are the sources, five
more of each the targets of the loads and resets.  Lists of n = 64, 1 024, 16 384 (= G) groups, each in two orders:
  ascending  n consecutive groups from a tile boundary
  random     a seeded sample of the object's groups in random order
A call's time is what lies between two events on its stream: for the replicas the list's copy and the one kernel over the five
objects, for the stores per object the list's copy, the head launch and the byte launch.  Which of ONE store's two launches
dominates is read from a save of the same list out of an EMPTY store of the same shape beside it: its head launch does the
same work per cell, its byte launch finds no shard (`head_share` = that time over the full store's; `byte_launch_us` = the rest).
The byte figures are a MODEL, not counters: a store's save or load reads and writes the image's shard bytes once each; the rate
(`model_GBs`, `of_hbm`) is that sum over the five stores' WHOLE time -- list copy, head launch and byte launch -- beside
DESIGN.md 7's HBM rate: the call's rate, not the byte kernel's, whose own time comes from a kernel trace.

One child process under `timeout -k 10`: a parity check first, then four warm-up passes of every call and >= 30 timed
repetitions, the calls' order alternating within a repetition.  One JSON line per list and one for the whole-object calls.
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
HBM_GBS = 8000.0                                                            # the rate DESIGN.md 7 holds the byte kernels against (MI355X peak)


def lists(G, n):
    import numpy as np
    rng = np.random.default_rng(SEED + n)
    first = FIRST if FIRST + n <= G else 0
    return {"ascending": np.arange(first, first + n, dtype=np.uint32), "random": rng.permutation(G)[:n].astype(np.uint32)}


def step_time(dev, G, ticks, reps, whole_only):
    import numpy as np
    import time_rsp_snapshot as trs
    import torch
    from summerset_amd import PayloadStoreSnapshot, RSPaxosPayloadStore, RSPaxosReplicaGroup, RSPaxosSnapshot, workloads as wl
    from summerset_amd.rspaxos import load_cluster_state, save_cluster_state
    note = lambda what: (sys.stderr.write("time_rsp_move_groups: %s\n" % what), sys.stderr.flush())   # noqa: E731
    _, src, stores = trs.cluster(G, ticks)
    R, W, L, ft = src[0].R, src[0].W, wl.CONFIG4["L"], wl.CONFIG4["ft"]
    assert int(src[0].dump()["len"].max()) > W, "the rings have not wrapped: more --ticks"
    dst = [RSPaxosReplicaGroup(G, R, me=r, window=W, fault_tolerance=ft) for r in range(R)]
    dstores = [RSPaxosPayloadStore(G, R, W, max_data_len=L) for _ in range(R)]
    empty = RSPaxosPayloadStore(G, R, W, max_data_len=L)
    note("warm-up done")

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

    def rate(shard_bytes, us):
        return round(2 * shard_bytes / (us * 1e-6) / 1e9, 1)

    # the whole-object calls: the five replicas in one launch, the five stores one after the other; one object of each too
    keep, scratch = save_cluster_state(src), save_cluster_state(src)
    skeep, sscratch = [s.save() for s in stores], [s.save() for s in stores]
    rinfo, sinfo = keep[0].info(), [s.info() for s in skeep]
    sbytes = sum(i["shard_bytes"] for i in sinfo)
    full = timed([("cluster_save_state", lambda: save_cluster_state(src, scratch)), ("cluster_load_state", lambda: load_cluster_state(src, keep)),
                  ("stores_save", lambda: [s.save(x) for s, x in zip(stores, sscratch)]), ("stores_load", lambda: [s.load(x) for s, x in zip(stores, skeep)]),
                  ("save_state", lambda: src[0].save_state(scratch[0])), ("load_state", lambda: src[0].load_state(keep[0])),
                  ("store_save", lambda: stores[0].save(sscratch[0])), ("store_load", lambda: stores[0].load(skeep[0]))])
    for k in full:
        full[k]["us_per_group"] = round(full[k]["median_us"] / G, 5)
    for k in ("stores_save", "stores_load"):
        full[k]["shard_bytes"] = sbytes
        full[k]["model_GBs"] = rate(sbytes, full[k]["median_us"])
        full[k]["of_hbm"] = round(full[k]["model_GBs"] / HBM_GBS, 3)
    full["store_save"]["model_GBs"] = rate(sinfo[0]["shard_bytes"], full["store_save"]["median_us"])
    full["store_load"]["model_GBs"] = rate(sinfo[0]["shard_bytes"], full["store_load"]["median_us"])
    print(json.dumps({"step": "full", "device": torch.cuda.get_device_name(0), "groups": G, "replicas": R, "window": W, "L": L, "reps": reps,
                      "replica_image": rinfo, "store_images": sinfo, "hbm_GBs": HBM_GBS, "calls": full}), flush=True)
    for s in scratch + sscratch:
        s.close()
    note("whole-object calls done")
    if whole_only:
        return
    from summerset_amd.rspaxos import load_cluster_groups, reset_cluster_groups, save_cluster_groups
    # parity: an ascending and a random list, by the targets' dump columns, headers, alias bytes and sampled rows
    for lst in lists(G, 1024).values():
        rs = save_cluster_groups(src, lst)
        load_cluster_groups(dst, rs, lst)
        for a, b in list(zip(src, dst))[::R - 1]:
            x, y = a.dump(), b.dump()
            for k in x:
                if k != "counters":
                    assert np.array_equal(x[k][..., lst], y[k][..., lst]), ("loaded", a.me, k)
        ps = [s.save_groups(lst) for s in stores]
        for d, p in zip(dstores, ps):
            d.load_groups(p, lst)
        sl = (L + stores[0].d - 1) // stores[0].d
        for a, b in list(zip(stores, dstores))[::R - 1]:
            assert np.array_equal(a.voted_alias()[:, lst], b.voted_alias()[:, lst])
            for p in (0, 1):
                x, y = a.dump(p), b.dump(p)
                assert all(np.array_equal(x[k][:, lst], y[k][:, lst]) for k in x), ("store", p)
            for w in (0, W - 1):
                m = (a.dump(0)["avail"][w][lst][None, :, None] >> np.arange(R)[:, None, None]) & 1
                assert np.array_equal(a.read_row(w, 0)[:, lst, :sl] * m, b.read_row(w, 0)[:, lst, :sl] * m), ("rows", w)
        reset_cluster_groups(dst, lst)
        for d in dstores:
            d.reset_groups(lst)
        assert all((d.dump(0)["tok"][:, lst] == 0xFFFFFFFF).all() for d in dstores)
        for s in rs + ps:
            s.close()
    print(json.dumps({"step": "parity", "ok": True, "groups": G, "replicas": R, "window": W, "warmup_ticks": ticks}), flush=True)
    whole = {"cluster_save_groups": "cluster_save_state", "cluster_load_groups": "cluster_load_state", "stores_save_groups": "stores_save",
             "stores_load_groups": "stores_load", "store_save_groups": "store_save"}
    for n in SIZES:
        n = min(n, G)
        for order, lst in lists(G, n).items():
            s, kept = [RSPaxosSnapshot(x, n) for x in src], save_cluster_groups(src, lst)
            ss, skept = [PayloadStoreSnapshot(x, n) for x in stores], [x.save_groups(lst) for x in stores]
            se = PayloadStoreSnapshot(empty, n)
            gi, si = kept[0].info(), [x.info() for x in skept]
            gb = sum(i["shard_bytes"] for i in si)
            res = timed([("cluster_save_groups", lambda: save_cluster_groups(src, lst, s)), ("cluster_load_groups", lambda: load_cluster_groups(dst, kept, lst)),
                         ("cluster_reset_groups", lambda: reset_cluster_groups(dst, lst)),
                         ("stores_save_groups", lambda: [x.save_groups(lst, y) for x, y in zip(stores, ss)]),
                         ("stores_load_groups", lambda: [x.load_groups(y, lst) for x, y in zip(dstores, skept)]),
                         ("stores_reset_groups", lambda: [x.reset_groups(lst) for x in dstores]),
                         ("store_save_groups", lambda: stores[0].save_groups(lst, ss[0])),
                         ("store_save_groups_of_an_empty_store", lambda: empty.save_groups(lst, se))])
            assert [x.info() for x in ss] == si                    # the sources did not move
            for k in res:
                res[k]["us_per_group"] = round(res[k]["median_us"] / n, 5)
                if k in whole:
                    res[k]["full_call_us_per_group"] = full[whole[k]]["us_per_group"]
                    res[k]["per_group_over_full_call"] = round(res[k]["us_per_group"] / full[whole[k]]["us_per_group"], 2)
                    res[k]["full_call_over_this"] = round(full[whole[k]]["median_us"] / res[k]["median_us"], 2)
            for k in ("stores_save_groups", "stores_load_groups"):
                res[k]["shard_bytes"] = gb
                res[k]["model_GBs"] = rate(gb, res[k]["median_us"])
                res[k]["of_hbm"] = round(res[k]["model_GBs"] / HBM_GBS, 4)
            head = res["store_save_groups_of_an_empty_store"]["median_us"]     # the list's copy + the head launch + an idle byte launch
            res["store_save_groups"]["head_share"] = round(head / res["store_save_groups"]["median_us"], 3)
            res["store_save_groups"]["byte_launch_us"] = round(res["store_save_groups"]["median_us"] - head, 2)
            print(json.dumps({"step": "groups", "n": n, "order": order, "replica_image": gi, "store_shard_bytes": gb, "calls": res}), flush=True)
            for x in s + kept + ss + skept + [se]:
                x.close()
        note("n = %d done" % n)


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--step", choices=("time",), help="run in this process (default: a child under `timeout -k 10`)")
    ap.add_argument("--groups", type=int, default=16384)
    ap.add_argument("--ticks", type=int, default=40)
    ap.add_argument("--reps", type=int, default=31)
    ap.add_argument("--whole-only", action="store_true", help="only the whole-object calls (what an earlier commit has)")
    args = ap.parse_args()
    assert args.reps >= 30, "at least 30 repetitions"
    import torch
    if not torch.cuda.is_available():
        sys.stderr.write("time_rsp_move_groups: no GPU is visible; this tool measures device calls and has no fallback\n")
        sys.exit(2)
    dev = torch.device("cuda:0")
    if args.step:
        return step_time(dev, args.groups, args.ticks, args.reps, args.whole_only)
    cmd = ["timeout", "-k", "10", "540", sys.executable, os.path.abspath(__file__), "--step", "time", "--reps", str(args.reps), "--groups", str(args.groups),
           "--ticks", str(args.ticks)] + (["--whole-only"] if args.whole_only else [])
    rc = subprocess.run(cmd).returncode
    if rc != 0:
        sys.stderr.write("time_rsp_move_groups: ended with status %d\n" % rc)
        sys.exit(rc)


if __name__ == "__main__":
    main()
