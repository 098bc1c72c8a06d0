#!/usr/bin/env python3
"""Times save / load of an EPaxos cluster's replicas beside the copy a wholesale checkpoint would make.

At the bench's EPaxos shape (`bench.py`'s epaxos_cluster_leg: 65 536 groups x 5 replicas, window 32, 64 keys, execution on),
after enough one-launch ticks that every row has wrapped: `smr_ep_cluster_save_state` / `smr_ep_cluster_load_state` of the five
replicas (one launch each) beside a device-to-device copy of the same five replicas' arenas (`smr_ep_debug_arena_view`).
Every device step is a child process of its own under `timeout -k 10`; the parity step runs first (a second set of replicas
loaded from the images dumps what the saved set dumps) and the timing step only if it passed.  Timing: three warm-up rounds,
then `--regions` regions of `--reps` back-to-back calls each between two device events, the three kinds alternating in order
from region to region; reported per call as the median over the regions with the range.  The copy at the same commit is the
yardstick; no threshold is fixed in advance.  Writes profiles/ep_snapshot_vs_arena_copy.log (and prints it).  The byte figures
are a MODEL, not counters: a save or load is taken to read the live cells' record words and write the image (or the reverse), a
copy to read and write the arenas' size.

    python tools/time_ep_snapshot.py [--groups G] [--ticks T] [--reps N] [--regions M]
"""
import argparse
import ctypes as C
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
LOG = os.path.join(ROOT, "profiles", "ep_snapshot_vs_arena_copy.log")
R, W, K = 5, 32, 64


def cluster(G, ticks):
    import numpy as np
    import torch
    from summerset_amd import EPaxosReplicaGroup
    from summerset_amd.ep_cluster import EPaxosCluster
    dev = torch.device("cuda:0")
    reps = [EPaxosReplicaGroup(G, R, me=r, window=W, n_keys=K, execute=True) for r in range(R)]
    cl = EPaxosCluster(reps)
    rng = np.random.default_rng(0x5EED5EED)
    zipf = 1.0 / np.arange(1, K + 1) ** 0.99
    zipf /= zipf.sum()
    out = cl.new_outputs(dev)
    for t in range(ticks):
        cl.tick([torch.from_numpy(rng.choice(K, G, p=zipf).astype(np.uint8)).to(dev) for _ in range(R)], out=out)
    torch.cuda.synchronize()
    return dev, reps, cl


def step_parity(a):
    import numpy as np
    from summerset_amd import EPaxosReplicaGroup, epaxos
    dev, reps, cl = cluster(a.groups, a.ticks)
    assert int(reps[0].dump()["len"].min()) > W, "the rings have not wrapped: more --ticks"
    fresh = [EPaxosReplicaGroup(a.groups, R, me=r, window=W, n_keys=K, execute=True) for r in range(R)]
    snaps = epaxos.save_cluster_state(reps)
    epaxos.load_cluster_state(fresh, snaps)
    for r in range(R):
        for x, y in ((reps[r].dump(), fresh[r].dump()), (reps[r].exec_dump(), fresh[r].exec_dump())):
            assert all(np.array_equal(x[k], y[k]) for k in x), ("replica", r)
    print(json.dumps(dict(step="parity", ok=True, replica0=snaps[0].info())))


def step_time(a):
    import torch
    from summerset_amd import _lib, epaxos
    dev, reps, cl = cluster(a.groups, a.ticks)
    Lb = _lib.load()
    snaps = epaxos.save_cluster_state(reps)
    infos = [s.info() for s in snaps]
    allocs = []
    for e in reps:
        base, n = C.c_void_p(), C.c_uint64()
        _lib.check(Lb.smr_ep_debug_arena_view(e._h, C.byref(base), C.byref(n)))
        allocs.append((base.value, n.value))
    twins = [torch.empty(n, dtype=torch.uint8, device=dev) for _, n in allocs]
    hip = C.CDLL("libamdhip64.so")
    hip.hipMemcpyAsync.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int, C.c_void_p]
    stream = _lib.stream_ptr(None)

    def copy():
        for (b, n), t in zip(allocs, twins):
            assert hip.hipMemcpyAsync(t.data_ptr(), b, n, 3, stream) == 0      # hipMemcpyDeviceToDevice
    fns = dict(save=lambda: epaxos.save_cluster_state(reps, snaps), load=lambda: epaxos.load_cluster_state(reps, snaps), copy=copy)
    for _ in range(3):
        for fn in fns.values():
            fn()
    torch.cuda.synchronize()
    res = dict(save=[], load=[], copy=[])
    for i in range(a.regions):
        for name in (("save", "load", "copy") if i % 2 == 0 else ("copy", "load", "save")):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(a.reps):
                fns[name]()
            e1.record()
            torch.cuda.synchronize()
            res[name].append(e0.elapsed_time(e1) * 1e3 / a.reps)              # us per call
    med = lambda v: sorted(v)[len(v) // 2]
    copy_bytes = sum(n for _, n in allocs)
    image_bytes = sum(i["bytes"] for i in infos)
    cells = sum(i["n_cells"] for i in infos)
    # per live cell 48 B of record words in the planes (64 at populations 7-8) against 64 B in the image; the rest of the image
    # (reply records, the per-key table, scalars) is taken as read once and written once
    plane_bytes = cells * 48
    print(json.dumps(dict(step="time", groups=a.groups, population=R, window=W, n_keys=K, reps_per_region=a.reps, regions=a.regions,
                          image_bytes=image_bytes, n_cells=cells, copy_bytes=copy_bytes,
                          **{k + "_us": dict(median=med(v), min=min(v), max=max(v)) for k, v in res.items()},
                          model_save_bytes_read_written=[plane_bytes + image_bytes - cells * 64, image_bytes],
                          model_load_bytes_read_written=[image_bytes, plane_bytes + cells * 4 + image_bytes - cells * 64],
                          model_copy_bytes_read_written=[copy_bytes, copy_bytes],
                          save_over_copy=med(res["save"]) / med(res["copy"]), load_over_copy=med(res["load"]) / med(res["copy"]))))


def child(args, limit):
    cmd = ["timeout", "-k", "10", str(limit), sys.executable, os.path.abspath(__file__)] + args
    p = subprocess.run(cmd, capture_output=True, text=True)
    lines = [ln for ln in p.stdout.splitlines() if ln.startswith("{")]
    return p.returncode, (json.loads(lines[-1]) if lines else None), p.stderr[-2000:]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--groups", type=int, default=65536)
    ap.add_argument("--ticks", type=int, default=W + 8)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--regions", type=int, default=7)
    ap.add_argument("--step", choices=["parity", "time"])
    a = ap.parse_args()
    if a.step == "parity":
        return step_parity(a)
    if a.step == "time":
        return step_time(a)
    common = ["--groups", str(a.groups), "--ticks", str(a.ticks), "--reps", str(a.reps), "--regions", str(a.regions)]
    rc, par, err = child(common + ["--step", "parity"], 240)
    out = [json.dumps(par) if par else "parity step failed (exit %d): %s" % (rc, err)]
    if rc == 0 and par and par.get("ok"):                                     # nothing more on the device after a step that failed
        rc, res, err = child(common + ["--step", "time"], 240)
        out.append(json.dumps(res) if res else "time: failed (exit %d): %s" % (rc, err))
    text = "\n".join(out) + "\n"
    with open(LOG, "w") as f:
        f.write(text)
    sys.stdout.write(text)
    return 0 if rc == 0 else 1


if __name__ == "__main__":
    sys.exit(main())
