#!/usr/bin/env python3
"""Times save / load of an RSPaxos replica and of its payload store beside the copies a wholesale checkpoint would make.

At `workloads.config4_payload_cluster`'s shape, after enough ticks that the rings have wrapped:
  * `smr_rsp_save_state` / `smr_rsp_load_state` of the leader replica -- at THIS cluster's window (16, the store's), not the
    engines' benchmark window of 64 -- beside a device-to-device copy of its arena (`smr_rsp_debug_arena_view`);
  * `smr_rsp_pstore_save` / `smr_rsp_pstore_load` of the leader's store and of one follower's, beside device-to-device copies
    of the store's three allocations (`smr_rsp_pstore_debug_allocs`).
Every device step is a child process of its own under `timeout -k 10`; the parity step runs first (a loaded replica dumps what
the saved one dumps, a loaded store holds the saved one's headers, alias bytes, counters and sampled rows) and the timing steps
only if it passed; inside a repetition the order of snapshot and copy alternates.  The copy at the same commit is the
yardstick; no threshold is fixed in advance.  Writes the median, the range, the bytes read and written and the ratio to the
copy into profiles/rsp_snapshot_vs_arena_copy.log (and prints them).  The byte figures are a MODEL, not counters: a save or
load is taken to read and write the image's size once each (the kernels also read the per-group counts in front of each block
again, and the replica's ring arrays are 55 B per instance against the record's 56), a copy the allocations' size.

    python tools/time_rsp_snapshot.py [--groups G] [--ticks T] [--reps N]
"""
import argparse
import ctypes as C
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
LOG = os.path.join(ROOT, "profiles", "rsp_snapshot_vs_arena_copy.log")


def cluster(G, ticks):
    """config 4's engines and stores after `ticks` steady ticks (every group appends every tick)"""
    import torch
    from summerset_amd import workloads as wl
    dev = torch.device("cuda:0")
    reps, loop, stores = wl.config4_payload_cluster(G=G)
    L = wl.CONFIG4["L"]
    src = torch.randint(0, 256, (G, L), dtype=torch.uint8, device=dev)
    ones = torch.ones(G, dtype=torch.int32, device=dev)
    for t in range(ticks):
        slot = torch.full((G,), t, dtype=torch.int32, device=dev)
        val = torch.arange(G, dtype=torch.int32, device=dev) + 1 + t * G
        wl.config4_payload_tick(reps, loop, stores, slot, src, val, None, t % 3 == 2, ones)
    torch.cuda.synchronize()
    return dev, reps, stores


def step_parity(a):
    import numpy as np
    import torch
    from summerset_amd import RSPaxosPayloadStore, RSPaxosReplicaGroup, workloads as wl
    dev, reps, stores = cluster(a.groups, a.ticks)
    W = reps[0].W
    assert int(reps[0].dump()["len"].max()) > W, "the rings have not wrapped: more --ticks"
    out = {}
    for q in (0, 1):
        fresh = RSPaxosReplicaGroup(a.groups, reps[q].R, me=q, window=W, fault_tolerance=wl.CONFIG4["ft"])
        snap = reps[q].save_state()
        fresh.load_state(snap)
        x, y = reps[q].dump(), fresh.dump()
        assert all(np.array_equal(x[k], y[k]) for k in x), ("replica", q)
        out["replica%d" % q] = snap.info()
        st = RSPaxosPayloadStore(a.groups, reps[q].R, stores[q].W, max_data_len=wl.CONFIG4["L"] + 100)
        ps = stores[q].save()
        st.load(ps)
        assert st.counters() == stores[q].counters() and np.array_equal(st.voted_alias(), stores[q].voted_alias()), ("store", q)
        for p in (0, 1):
            x, y = stores[q].dump(p), st.dump(p)
            assert all(np.array_equal(x[k], y[k]) for k in x), ("store", q, p)
        sl = (wl.CONFIG4["L"] + st.d - 1) // st.d
        for w in (0, stores[q].W - 1):
            assert np.array_equal(stores[q].read_row(w, 0)[:, :, :sl] * (stores[q].dump(0)["avail"][w][None, :, None] != 0),
                                  st.read_row(w, 0)[:, :, :sl] * (st.dump(0)["avail"][w][None, :, None] != 0)), ("rows", q, w)
        out["store%d" % q] = ps.info()
        st.close(); ps.close(); fresh.close(); snap.close()
    print(json.dumps(dict(step="parity", ok=True, **out)))


def _time(fn, torch):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record(); fn(); e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3                                          # us


def step_time(a):
    import torch
    from summerset_amd import _lib
    dev, reps, stores = cluster(a.groups, a.ticks)
    Lb = _lib.load()
    q = {"replica": 0, "leader_store": 0, "follower_store": 1}[a.what]
    if a.what == "replica":
        obj, snap = reps[q], reps[q].save_state()
        base, n = C.c_void_p(), C.c_uint64()
        _lib.check(Lb.smr_rsp_debug_arena_view(obj._h, C.byref(base), C.byref(n)))
        allocs = [(base.value, n.value)]
        save, load = (lambda: obj.save_state(snap)), (lambda: obj.load_state(snap))
    else:
        obj, snap = stores[q], stores[q].save()
        bases, ns = (C.c_void_p * 3)(), (C.c_uint64 * 3)()
        _lib.check(Lb.smr_rsp_pstore_debug_allocs(obj._h, bases, ns))
        allocs = [(bases[i], ns[i]) for i in range(3) if ns[i]]
        save, load = (lambda: obj.save(snap)), (lambda: obj.load(snap))
    info = snap.info()
    twins = [torch.empty(n, dtype=torch.uint8, device=dev) for _, n in allocs]
    hip = C.CDLL("libamdhip64.so")
    hip.hipMemcpyAsync.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int, C.c_void_p]
    stream = _lib.stream_ptr(None)

    def copy():
        for (b, n), t in zip(allocs, twins):
            assert hip.hipMemcpyAsync(t.data_ptr(), b, n, 3, stream) == 0      # hipMemcpyDeviceToDevice
    for fn in (save, load, copy):
        fn()
    torch.cuda.synchronize()
    res = dict(save=[], load=[], copy=[])
    for i in range(a.reps):
        order = ("save", "load", "copy") if i % 2 == 0 else ("copy", "load", "save")
        for name in order:
            res[name].append(_time(dict(save=save, load=load, copy=copy)[name], torch))
    med = lambda v: sorted(v)[len(v) // 2]
    copy_bytes = sum(n for _, n in allocs)
    print(json.dumps(dict(step="time", what=a.what, image_bytes=info["bytes"], copy_bytes=copy_bytes, reps=a.reps,
                          **{k + "_us": dict(median=med(v), min=min(v), max=max(v)) for k, v in res.items()},
                          window=int(obj.W), model_save_bytes_read_written=[info["bytes"], info["bytes"]], model_copy_bytes_read_written=[copy_bytes, copy_bytes],
                          save_over_copy=med(res["save"]) / med(res["copy"]), load_over_copy=med(res["load"]) / med(res["copy"]))))


def child(args, limit):
    cmd = ["timeout", "-k", "10", str(limit), sys.executable, os.path.abspath(__file__)] + args
    p = subprocess.run(cmd, capture_output=True, text=True)
    lines = [ln for ln in p.stdout.splitlines() if ln.startswith("{")]
    return p.returncode, (json.loads(lines[-1]) if lines else None), p.stderr[-2000:]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--groups", type=int, default=16384)
    ap.add_argument("--ticks", type=int, default=80)
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--step", choices=["parity", "time"])
    ap.add_argument("--what", choices=["replica", "leader_store", "follower_store"])
    a = ap.parse_args()
    if a.step == "parity":
        return step_parity(a)
    if a.step == "time":
        return step_time(a)
    common = ["--groups", str(a.groups), "--ticks", str(a.ticks), "--reps", str(a.reps)]
    rc, par, err = child(common + ["--step", "parity"], 300)
    out = [json.dumps(par) if par else "parity step failed (exit %d): %s" % (rc, err)]
    if rc == 0 and par and par.get("ok"):
        for what in ("replica", "leader_store", "follower_store"):
            rc, res, err = child(common + ["--step", "time", "--what", what], 300)
            out.append(json.dumps(res) if res else "%s: failed (exit %d): %s" % (what, rc, err))
            if rc != 0:                                                       # nothing more on the device after a step that failed
                break
    text = "\n".join(out) + "\n"
    with open(LOG, "w") as f:
        f.write(text)
    sys.stdout.write(text)
    return 0 if rc == 0 else 1


if __name__ == "__main__":
    sys.exit(main())
