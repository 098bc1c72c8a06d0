#!/usr/bin/env python3
"""A MultiPaxos cluster's state out of its WAL bytes (`smr_mp_snapshot_from_wal` + `smr_mp_load_state`) beside the two things it
can be held against, for the SAME state, timed with device events in one process: `smr_mp_save_state` + `smr_mp_load_state` of the
cluster that replay produced (what a checkpoint of a live cluster costs), and one device-to-device `hipMemcpyAsync` of the WAL
bytes (what merely touching the input costs).

    python tools/time_mp_wal_replay.py > profiles/mp_wal_replay.log

Shapes: 16 384 and 65 536 groups x 5 replicas, 32 entries per log (1 PrepareBal, 20 AcceptData, 11 CommitSlot: a log of 20
slots, 11 of them executed), request values of 16 B and of 4 KiB; W = 64.  Every log holds the same bytes (the walk's cost does not
depend on the values of slots, ballots and tokens; their widths are those of a young cluster: one-byte slots, three-byte ballots).

Each shape is a process of its own under `timeout -k 10`, the next only if the one before succeeded, nothing retried.  A shape
first checks the loaded state (bars, ballots, statuses and tokens of slices at both ends and the middle, `consumed`, `counts`),
then times >= 30 repetitions of the three, the order alternating within a repetition.  One JSON line per shape: medians, quartiles
and spread, the WAL's bytes beside the image's.  No device visible: an error (exit status 2), never a fallback."""
import argparse
import ctypes as C
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

R, W, N_ACCEPT, N_COMMIT, BALLOT = 5, 64, 20, 11, 256 + 3
SHAPES = [(16384, 16), (16384, 4096), (65536, 16), (65536, 4096)]


def need_gpu():
    import torch
    if not torch.cuda.is_available():
        sys.stderr.write("time_mp_wal_replay: no GPU is visible; this tool measures device calls and has no fallback\n")
        sys.exit(2)
    return torch.device("cuda:0")


def one_log(value_bytes):
    """(the log's bytes, its journal): 32 entries"""
    from summerset_amd import wire
    out, toks = [wire.wal_prepare_bal(0, BALLOT)], []
    for s in range(N_ACCEPT):
        out.append(wire.wal_accept_data(s, BALLOT, wire.reqbatch([(7, 100 + s, ("put", "key%02d" % s, "v" * value_bytes))])))
        toks.append(1000 + s)
    out += [wire.wal_commit_slot(s) for s in range(N_COMMIT)]
    assert len(out) == 32
    return b"".join(out), toks


def step(dev, G, value_bytes, reps):
    import numpy as np
    import torch
    from summerset_amd import MpSnapshot, MultiPaxosCluster, _lib
    log, toks = one_log(value_bytes)
    n_logs = G * R
    buf = torch.from_numpy(np.frombuffer(log, np.uint8).copy()).to(dev).repeat(n_logs)
    off = torch.arange(n_logs + 1, dtype=torch.int64, device=dev) * len(log)
    tok = torch.tensor(toks, dtype=torch.int32, device=dev).repeat(n_logs)
    toff = torch.arange(n_logs + 1, dtype=torch.int64, device=dev) * len(toks)
    eng = MultiPaxosCluster(G, R, W, outbox_cap=W + 4)
    snap, consumed, status, counts = MpSnapshot.from_wal(eng, (buf, off), (tok, toff), device=dev)
    eng.load_state(snap)
    # the state, before anything is timed
    assert bool((consumed == len(log)).all()) and not bool(status.any()) and counts.tolist() == [32 * n_logs, 0, 0, 0]
    info = snap.info()
    assert info["n_slots"] == N_ACCEPT * n_logs and info["max_live"] == N_ACCEPT
    for g0 in (0, (G // 2) & ~63, G - 64):
        for r in range(R):
            d = eng.dump(r, g0, 64)
            assert (d["log_len"] == N_ACCEPT).all() and (d["accept_bar"] == N_ACCEPT).all() and (d["commit_bar"] == N_COMMIT).all()
            assert (d["exec_bar"] == N_COMMIT).all() and (d["bal_max_seen"] == BALLOT).all() and (d["bal_prepared"] == BALLOT).all()
            assert (d["leader"] == 0xFF).all() and (d["s_status"][:N_COMMIT] == 4).all() and (d["s_status"][N_COMMIT:N_ACCEPT] == 2).all()
            assert (d["s_reqs"][:N_ACCEPT] == np.arange(1000, 1000 + N_ACCEPT, dtype=np.uint32)[:, None]).all() and (d["s_bal"][:N_ACCEPT] == BALLOT).all()
    keep = eng.save_state()                                          # the same state as a checkpoint of the live cluster
    assert keep.export() == snap.export() if G <= 16384 and value_bytes == 16 else True
    twin = torch.empty_like(buf)
    hip = C.CDLL("libamdhip64.so")
    hip.hipMemcpyAsync.restype = C.c_int
    hip.hipMemcpyAsync.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int, C.c_void_p]
    st = _lib.stream_ptr(None)

    def replay():
        MpSnapshot.from_wal(eng, (buf, off), (tok, toff), device=dev, snap=snap)
        eng.load_state(snap)

    def checkpoint():
        eng.save_state(keep)
        eng.load_state(keep)

    def copy():
        rc = hip.hipMemcpyAsync(twin.data_ptr(), buf.data_ptr(), buf.numel(), 3, st)   # hipMemcpyDeviceToDevice
        assert rc == 0, rc
    calls = [("from_wal_load", replay), ("save_load", checkpoint), ("wal_copy", copy)]
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
        if r >= 4:
            for what, e0, e1 in marks:
                us[what].append(e0.elapsed_time(e1) * 1e3)
    assert snap.info() == info

    def stats(x):
        q1, med, q3 = (float(v) for v in np.percentile(x, [25, 50, 75]))
        return {"median_us": round(med, 1), "q1_us": round(q1, 1), "q3_us": round(q3, 1), "iqr_us": round(q3 - q1, 1), "min_us": round(float(min(x)), 1), "n": len(x)}
    out = {"groups": G, "replicas": R, "window": W, "entries_per_log": 32, "value_bytes": value_bytes, "device": torch.cuda.get_device_name(0), "reps": reps,
           "wal_bytes": int(buf.numel()), "log_bytes": len(log), "image_bytes": info["bytes"], "n_slots": info["n_slots"],
           "note": "from_wal_load: smr_mp_snapshot_from_wal (offset read-back and two launches) + smr_mp_load_state (header read-back, one launch); "
                   "save_load: smr_mp_save_state + smr_mp_load_state of the same state; wal_copy: one hipMemcpyAsync of the WAL bytes, device to device",
           "calls": {k: stats(us[k]) for k, _ in calls}}
    c = out["calls"]
    c["from_wal_load"]["wal_gb_per_s"] = round(buf.numel() / (c["from_wal_load"]["median_us"] * 1e-6) / 1e9, 1)
    c["from_wal_load"]["entries_per_us"] = round(32 * n_logs / c["from_wal_load"]["median_us"], 1)
    c["from_wal_load"]["over_save_load"] = round(c["from_wal_load"]["median_us"] / c["save_load"]["median_us"], 2)
    c["from_wal_load"]["over_wal_copy"] = round(c["from_wal_load"]["median_us"] / c["wal_copy"]["median_us"], 2)
    print(json.dumps(out), flush=True)


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--shape", help="G,value_bytes: run one shape in this process (default: all, each a child under `timeout -k 10`)")
    ap.add_argument("--reps", type=int, default=30)
    args = ap.parse_args()
    assert args.reps >= 30, "at least 30 repetitions"
    if args.shape:
        g, v = (int(x) for x in args.shape.split(","))
        return step(need_gpu(), g, v, args.reps)
    need_gpu()
    for g, v in SHAPES:                                              # the next only if the one before succeeded
        rc = subprocess.run(["timeout", "-k", "10", "240", sys.executable, os.path.abspath(__file__), "--shape", "%d,%d" % (g, v), "--reps", str(args.reps)]).returncode
        if rc != 0:
            sys.stderr.write("time_mp_wal_replay: shape %d,%d ended with status %d; stopping\n" % (g, v, rc))
            sys.exit(rc)


if __name__ == "__main__":
    main()
