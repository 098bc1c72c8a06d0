#!/usr/bin/env python3
"""The string store's state out of and into the device-resident snapshot (`smr_skv_save_state` / `_load_state`, `smr_skv_save_groups` /
`_load_groups`) beside a wholesale `hipMemcpy` of the store's one allocation, timed with device events in one process.

    python tools/time_kv_snapshot.py > profiles/kv_snapshot.log

Shape: the string store's default geometry (slots = 256, heap_bytes = 64 KiB) at G = 16 384 groups, every group holding the same
keys (the image's size and the kernels' work do not depend on which), at three fill levels:
  few      4 keys of 8 bytes with 24-byte values
  half     128 keys (half the table) of 8 bytes with 16-byte values
  dead     8 keys whose 720-byte values were overwritten ten times: 90 % of heap_used is dead bytes
Per level: a whole save and a whole load (into a second store), 64 listed groups (a seeded random sample) out and in, and the
copy of the arena (`smr_skv_debug_arena`: tables and heaps, 1.1 GB) as the yardstick.  A call's time is what lies between two
events on its stream: for a save the rank, head and byte launches (the list's copy in front for listed groups), for a load the
sizes, head and byte launches.  Which part of a save is the rank launch is not in these figures: it comes from a kernel trace
of this tool (`rocprofv3 --kernel-trace --stats -- python tools/time_kv_snapshot.py --step time --level half --list 0`).
The byte figures are a MODEL, not counters: a save reads the live bytes and writes the image, a load the reverse.

One child process under `timeout -k 10`: a parity check per level first (Gets on the loaded store answer the pairs), then four
warm-up passes of every call and >= 30 timed repetitions, the calls' order alternating.  One JSON line per level.
No device visible: an error (exit status 2), never a fallback."""
import argparse
import ctypes as C
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SEED = 0x6B767373
LEVELS = {"few": dict(keys=4, vlen=24, overwrites=0), "half": dict(keys=128, vlen=16, overwrites=0), "dead": dict(keys=8, vlen=720, overwrites=9)}


def fill(sm, dev, keys, vlen, overwrites):
    """every group Puts the same `keys` keys (8 bytes each) 1 + overwrites times; -> the pairs it ends up holding"""
    import numpy as np
    import torch
    rng = np.random.default_rng(SEED)
    G = sm.G
    names = [b"key%05d" % i for i in range(keys)]
    pairs = {}
    for rnd in range(1 + overwrites):
        blob = bytearray()
        ko, vo = [], []
        for k in names:
            v = rng.integers(0, 256, vlen, dtype=np.uint8).tobytes()
            ko.append(len(blob)); blob += k
            vo.append(len(blob)); blob += v
            pairs[k] = v
        col = lambda x: torch.from_numpy(np.ascontiguousarray(np.broadcast_to(np.asarray(x, np.int32)[:, None], (keys, G)))).to(dev)   # noqa: E731
        kind = torch.ones((keys, G), dtype=torch.uint8, device=dev)
        payload = torch.from_numpy(np.frombuffer(bytes(blob), np.uint8).copy()).to(dev)
        st, _, _ = sm.execute(kind, payload, col(ko), col([8] * keys), col(vo), col([vlen] * keys))
        assert not bool((st == 2).any()), "the fill ran a heap or a table full"
    return pairs


def parity(sm, dev, pairs, groups):
    """Gets of every key on the loaded store answer the pairs, read back for `groups`"""
    import numpy as np
    import torch
    names = sorted(pairs)
    blob = b"".join(names)
    G, n = sm.G, len(names)
    col = lambda x: torch.from_numpy(np.ascontiguousarray(np.broadcast_to(np.asarray(x, np.int32)[:, None], (n, G)))).to(dev)   # noqa: E731
    st, off, ln = sm.execute(torch.zeros((n, G), dtype=torch.uint8, device=dev), torch.from_numpy(np.frombuffer(blob, np.uint8).copy()).to(dev),
                             col([8 * i for i in range(n)]), col([8] * n), col([0] * n), col([0] * n))
    st, off, ln = st.cpu().numpy(), off.cpu().numpy(), ln.cpu().numpy()
    assert (st == 1).all() and (ln == len(pairs[names[0]])).all()
    for g in groups:
        for i in (0, n // 2, n - 1):
            assert sm.heap_bytes_of(int(g), int(off[i, g]), int(ln[i, g])) == pairs[names[i]], (g, i)


def step_time(dev, G, reps, n_list, levels, slots=256):
    import numpy as np
    import torch
    from summerset_amd import StringKvSnapshot, StringKvStateMachine, _lib
    note = lambda what: (sys.stderr.write("time_kv_snapshot: %s\n" % what), sys.stderr.flush())   # noqa: E731
    hip = C.CDLL("libamdhip64.so")
    hip.hipMemcpyAsync.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int, C.c_void_p]

    def stats(x):
        q1, med, q3 = (float(v) for v in np.percentile(x, [25, 50, 75]))
        return {"median_us": round(med, 2), "q1_us": round(q1, 2), "q3_us": round(q3, 2), "min_us": round(float(min(x)), 2), "n": len(x)}

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

    lst = np.random.default_rng(SEED).permutation(G)[:n_list].astype(np.uint32)
    for level, shape in LEVELS.items():
        if level not in levels:
            continue
        src, dst = StringKvStateMachine(G, slots), StringKvStateMachine(G, slots)
        if level == "half":
            shape = dict(shape, keys=slots // 2)                   # (half the table, whatever --slots)
        pairs = fill(src, dev, **shape)
        base, arena_bytes, _ = src.debug_arena()
        twin = torch.empty(arena_bytes, dtype=torch.uint8, device=dev)
        stream = _lib.stream_ptr(None)
        whole, keep = StringKvSnapshot(src), src.save_state()
        part, pkeep = (StringKvSnapshot(src, n_list), src.save_groups(lst)) if n_list else (None, None)
        dst.load_state(keep)
        parity(dst, dev, pairs, [0, G // 2, G - 1])
        st = src.stats()
        info, ginfo = keep.info(), pkeep.info() if n_list else None
        live = sum(len(k) + len(v) for k, v in pairs.items())

        def copy():
            assert hip.hipMemcpyAsync(twin.data_ptr(), base, arena_bytes, 3, stream) == 0          # hipMemcpyDeviceToDevice
        calls = [("save_state", lambda: src.save_state(whole)), ("load_state", lambda: dst.load_state(keep)), ("arena_copy", copy)]
        if n_list:                                                 # (--list 0: the whole-object calls alone, for a kernel trace)
            calls += [("save_groups", lambda: src.save_groups(lst, part)), ("load_groups", lambda: dst.load_groups(pkeep, lst))]
        res = timed(calls)
        assert whole.info() == info
        for k in ("save_state", "load_state"):
            res[k]["model_GBs"] = round((G * live + info["bytes"]) / (res[k]["median_us"] * 1e-6) / 1e9, 1)
            res[k]["over_arena_copy"] = round(res[k]["median_us"] / res["arena_copy"]["median_us"], 3)
        res["arena_copy"]["GBs_read_plus_written"] = round(2 * arena_bytes / (res["arena_copy"]["median_us"] * 1e-6) / 1e9, 1)
        print(json.dumps({"step": "level", "level": level, "device": torch.cuda.get_device_name(0), "groups": G, "slots": src.slots, "heap_bytes": src.heap_bytes,
                          "keys_per_group": shape["keys"], "live_bytes_per_group": live, "heap_used_per_group": int(st["heap_used"][0]),
                          "dead_share": round(1 - live / int(st["heap_used"][0]), 3), "image": info, "list": n_list, "list_image": ginfo,
                          "arena_bytes": arena_bytes, "reps": reps, "calls": res}), flush=True)
        for x in (whole, keep, part, pkeep, src, dst):
            if x is not None:
                x.close()
        del twin
        note("%s done" % level)


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--step", choices=("time",), help="run in this process (default: a child under `timeout -k 10`)")
    ap.add_argument("--groups", type=int, default=16384)
    ap.add_argument("--list", type=int, default=64)
    ap.add_argument("--reps", type=int, default=31)
    ap.add_argument("--slots", type=int, default=256, help="another table size (the rank launch's share at 1024: DESIGN.md 7)")
    ap.add_argument("--level", choices=tuple(LEVELS) + ("all",), default="all")
    args = ap.parse_args()
    assert args.reps >= 30, "at least 30 repetitions"
    import torch
    if not torch.cuda.is_available():
        sys.stderr.write("time_kv_snapshot: no GPU is visible; this tool measures device calls and has no fallback\n")
        sys.exit(2)
    if args.step:
        return step_time(torch.device("cuda:0"), args.groups, args.reps, args.list, tuple(LEVELS) if args.level == "all" else (args.level,), args.slots)
    cmd = ["timeout", "-k", "10", "540", sys.executable, os.path.abspath(__file__), "--step", "time", "--reps", str(args.reps), "--groups", str(args.groups),
           "--list", str(args.list), "--level", args.level, "--slots", str(args.slots)]
    rc = subprocess.run(cmd).returncode
    if rc != 0:
        sys.stderr.write("time_kv_snapshot: ended with status %d\n" % rc)
        sys.exit(rc)


if __name__ == "__main__":
    main()
