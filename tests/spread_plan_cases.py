"""The static plans of layout L2 do not move: for every case, rank and exchange the split sizes and a SHA-256 over the sorted
(message, send offset) and (message, receive offset) pairs, against tests/golden/spread_plan_digests.json.  A plan is host
arithmetic, so the cases need no device: the engines behind the job objects are the emulator build's (`hostsim.patched()`), which
is also where the sizes that come from the library (`smr_mp_image_bytes`, `smr_rs_shard_len`) are asked.  The bodies of
tests/test_spread_plan_digests.py; tools/make_spread_plan_digests.py writes the file.

The shapes: worlds 1, 2, 3 and 8; group counts that do not divide by the world; (8, 5), where blocks 5 to 7 have no groups; a
`data_len` of 100, where neither an RSPaxos header nor a shard is a multiple of 16 bytes."""
import hashlib
import json
import os

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "spread_plan_digests.json")

_SHAPES = [(1, 70), (2, 130), (3, 100), (8, 5), (8, 21)]
EP_CASES = [(5, w, g, o) for w, g in _SHAPES for o in (False, True)] + [(3, 2, 60, False)]           # (R, world, G, ordered)
RSP_CASES = [(5, w, g, 100) for w, g in _SHAPES] + [(5, 2, 130, 4096), (3, 2, 60, 100)]             # (R, world, G, data_len)
MP_CASES = [(5, w, g) for w, g in [(2, 130), (3, 100), (4, 21), (8, 21)]] + [(3, 2, 60)]             # (R, world, G)
MP_W, MP_S = 16, 4


def ep_id(c):
    return "epaxos R%d world%d G%d %s" % (c[0], c[1], c[2], "ordered" if c[3] else "together")


def rsp_id(c):
    return "rspaxos R%d world%d G%d L%d" % c


def mp_id(c):
    return "multipaxos R%d world%d G%d" % c


def ep_ranks(c):
    from summerset_amd import spread_ep
    R, world, G, ordered = c
    return [spread_ep.SpreadEPaxos(G, R, r, world, "cpu", ordered=ordered) for r in range(world)]


def rsp_ranks(c):
    from summerset_amd import spread_rsp
    R, world, G, L = c
    return [spread_rsp.SpreadRSPaxos(G, R, 8, r, world, "cpu", L) for r in range(world)]


def mp_ranks(c):
    from summerset_amd import spread_mp
    R, world, G = c
    return [spread_mp.SpreadMultiPaxos(G, R, MP_W, r, world, "cpu", MP_S, outbox_cap=MP_W + 4) for r in range(world)]


def _sha(pairs):
    return hashlib.sha256(json.dumps(sorted((list(k), int(o)) for k, o in pairs)).encode()).hexdigest()


def _name(k):
    return k if isinstance(k, str) else "%s/%d" % k


def _offsets(p):
    """(send pairs, receive pairs, dup_of or None) of one plan.  MultiPaxos: a message's key is (src, dst, block, kind, replica,
    other); the commit the digests were recorded on kept its messages as objects in p["send"] / p["recv"]"""
    if "soff" in p:
        return list(p["soff"].items()), list(p["roff"].items()), p.get("dup_of")
    key = lambda m: (m.src, m.dst, m.block, m.kind, m.rep, m.other)   # noqa: E731
    return ([(key(m), m.soff) for m in p["send"]], [(key(m), m.roff) for m in p["recv"]],
            {key(m): (None if m.dup_of is None else m.dup_of.soff) for m in p["send"]})


def record(ranks):
    """{rank: {exchange: dict(in_split, out_split, n_send, n_recv, send, recv[, dup_of])}} of a job's rank objects"""
    out = {}
    for r, obj in enumerate(ranks):
        out[str(r)] = {}
        for k, p in obj._plans.items():
            send, recv, dup = _offsets(p)
            d = dict(in_split=[int(x) for x in p["in_split"]], out_split=[int(x) for x in p["out_split"]],
                     n_send=int(p.get("n_send", sum(p["in_split"]))), n_recv=int(p.get("n_recv", sum(p["out_split"]))),
                     send=_sha(send), recv=_sha(recv))
            if dup is not None:                                   # per send message, by send offset: the offset it is a copy of
                at = dict(send)
                d["dup_of"] = [[int(at[m]), None if o is None else int(o)] for m, o in sorted(dup.items(), key=lambda x: at[x[0]])]
            out[str(r)][_name(k)] = d
    return out


def close(ranks):
    for obj in ranks:
        for fn in ("close_library_tick", "close"):
            if hasattr(obj, fn):
                getattr(obj, fn)()


CASES = {}
for _c in EP_CASES:
    CASES[ep_id(_c)] = (ep_ranks, _c)
for _c in RSP_CASES:
    CASES[rsp_id(_c)] = (rsp_ranks, _c)
for _c in MP_CASES:
    CASES[mp_id(_c)] = (mp_ranks, _c)


def golden():
    with open(GOLDEN) as f:
        return json.load(f)


def same_as_recorded(name):
    make, c = CASES[name]
    ranks = make(c)
    try:
        got = record(ranks)
    finally:
        close(ranks)
    want = golden()["cases"][name]
    for r in want:
        for k in want[r]:
            assert got[r][k] == want[r][k], (name, "rank", r, k, got[r][k], want[r][k])
    assert got == want, name


def library_splits(obj, fn):
    """[(in_split, out_split)] per exchange, from the library's plan of `obj` (after use_library_tick); fn = smr_*_spread_buffers"""
    import ctypes as C
    from summerset_amd import _lib
    out = []
    for k in range(len(obj._plans)):
        sp, rp = C.c_void_p(), C.c_void_p()
        sb, rb = (C.c_uint64 * obj.world)(), (C.c_uint64 * obj.world)()
        _lib.check(fn(obj._lib_h, k, C.byref(sp), sb, C.byref(rp), rb))
        out.append(([int(x) for x in sb], [int(x) for x in rb]))
    return out


def library_splits_agree(name):
    """the C++ plan builder (csrc/ep_spread.hip, csrc/rsp_spread.hip) and the Python one give every exchange the same split sizes:
    the exchanges of `obj._plans` are in the library's exchange order"""
    make, c = CASES[name]
    ranks = make(c)
    try:
        for obj in ranks:
            mine = [(p["in_split"], p["out_split"]) for p in obj._plans.values()]    # (before the library's buffers replace any)
            obj.use_library_tick()
            fn = obj._L.smr_ep_spread_buffers if make is ep_ranks else obj._L.smr_rsp_spread_buffers
            assert library_splits(obj, fn) == [([int(x) for x in a], [int(x) for x in b]) for a, b in mine], (name, obj.rank)
    finally:
        close(ranks)
