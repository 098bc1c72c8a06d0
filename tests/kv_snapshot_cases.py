"""Save, load, chosen groups and compaction of the two device-resident state machines (`smr_skv_*`, `smr_kv_*`; csrc/skv_snapshot.h,
csrc/kv_snapshot.h): the bodies, run by tests/test_kv_snapshot.py on the emulator (`dev` = "cpu" under `hostsim.patched()`) and by
tests/test_zzzz_kv_snapshot_gpu.py on the device.

Nothing here compares the code under test against itself.  The checker of the string store is a Python dict per group (as in
tests/test_zz_skv_gpu.py); `model_image(dicts, full)` builds the bytes an export must equal out of the format the header documents,
with its own FNV-1a; the token table's checker is a numpy array."""
import contextlib
import ctypes as C
import struct

import numpy as np

GET, PUT, NOP = 0, 1, 0xFF
EMPTY = 0xFFFFFFFF
SKV_MAGIC, KV_MAGIC = 0x564B5353, 0x564B4B53
TABLE = ("hash", "koff", "klen", "voff", "vlen")

SKV_SYMBOLS = ["smr_skv_snapshot_create", "smr_skv_snapshot_create_groups", "smr_skv_snapshot_destroy", "smr_skv_snapshot_info_get",
               "smr_skv_snapshot_export", "smr_skv_snapshot_import", "smr_skv_save_state", "smr_skv_load_state", "smr_skv_save_groups",
               "smr_skv_load_groups", "smr_skv_reset_groups"]
KV_SYMBOLS = [n.replace("smr_skv", "smr_kv") for n in SKV_SYMBOLS]


def symbols(lib):
    import summerset_amd
    from summerset_amd import _lib
    names = {n for n, _, _ in _lib.SYMBOLS}
    for n in SKV_SYMBOLS + KV_SYMBOLS:
        assert n in names and getattr(lib, n), n
    for n in ("move_kv_groups", "move_skv_groups", "KvSnapshot", "StringKvSnapshot"):
        assert hasattr(summerset_amd, n), n
    for cls in (summerset_amd.KvStateMachine, summerset_amd.StringKvStateMachine):
        for n in ("save_state", "load_state", "save_groups", "load_groups", "reset_groups"):
            assert hasattr(cls, n), (cls, n)
    assert hasattr(summerset_amd.StringKvStateMachine, "compact") and hasattr(summerset_amd.StringKvSnapshot, "items")


# ---- the models ----------------------------------------------------------------------------------------------------------------
def fnv1a(key):
    h = 0xCBF29CE484222325
    for b in key:
        h = ((h ^ b) * 0x100000001B3) & 0xFFFFFFFFFFFFFFFF
    return h


def _a8(x):
    return (x + 7) & ~7


def _a16(x):
    return (x + 15) & ~15


def model_image(dicts, full=None):
    """the image of these maps, from the documented format: header, n_keys, full, records, bytes; tile-major over 64 positions,
    then rank (ascending (hash, klen, key bytes)), then position"""
    n = len(dicts)
    full = [0] * n if full is None else [int(x) for x in full]
    ranked = [sorted(d.items(), key=lambda kv: (fnv1a(kv[0]), len(kv[0]), kv[0])) for d in dicts]
    recs, blob = bytearray(), bytearray()
    n_rec = 0
    for t0 in range(0, n, 64):
        tile = ranked[t0:t0 + 64]
        for k in range(max(len(r) for r in tile)):
            for r in tile:
                if k < len(r):
                    key, val = r[k]
                    recs += struct.pack("<QII", fnv1a(key), len(key), len(val))
                    run = key + val
                    blob += run + b"\0" * (_a16(len(run)) - len(run))
                    n_rec += 1
    nk = np.array([len(d) for d in dicts], "<u4").tobytes()
    nk += b"\0" * (_a8(len(nk)) - len(nk))
    fl = bytes(full) + b"\0" * (_a8(n) - n)
    fixed = 64 + len(nk) + len(fl)
    pad = _a16(fixed + len(recs)) - (fixed + len(recs))
    total = fixed + len(recs) + pad + len(blob)
    max_keys = max([len(d) for d in dicts] + [0])
    max_bytes = max([sum(len(k) + len(v) for k, v in d.items()) for d in dicts] + [0])
    hdr = struct.pack("<IIIIIIQQQQQ", SKV_MAGIC, 1, n, max_keys, max_bytes, 0, total, n_rec, len(blob), 0, 0)
    assert len(hdr) == 64
    return hdr + nk + fl + bytes(recs) + b"\0" * pad + bytes(blob)


def kv_model_image(table):
    """the token table's image: header, then u32 kv[K][n] padded to 8"""
    table = np.ascontiguousarray(table, "<u4")
    K, n = table.shape
    body = table.tobytes()
    body += b"\0" * (_a8(len(body)) - len(body))
    return struct.pack("<IIIIQ", KV_MAGIC, 1, n, K, 64 + len(body)) + b"\0" * 40 + body


def live_bytes(d):
    return sum(len(k) + len(v) for k, v in d.items())


# ---- driving a string store --------------------------------------------------------------------------------------------------
def submit(sm, dev, rows, stream=None):
    """rows: list of lists (one entry per group) of ("get", key) | ("put", key, value) | None; enqueues, returns the result tensors"""
    import torch
    G = sm.G
    blob, kind = bytearray(), np.full((len(rows), G), NOP, np.uint8)
    ko, kl, vo, vl = (np.zeros((len(rows), G), np.int32) for _ in range(4))
    for i, row in enumerate(rows):
        for g, c in enumerate(row):
            if c is None:
                continue
            kind[i, g] = PUT if c[0] == "put" else GET
            ko[i, g], kl[i, g] = len(blob), len(c[1]); blob += c[1]
            if c[0] == "put":
                vo[i, g], vl[i, g] = len(blob), len(c[2]); blob += c[2]
    t = lambda a: torch.from_numpy(a).to(dev)                    # noqa: E731
    payload = torch.from_numpy(np.frombuffer(bytes(blob) or b"\0", np.uint8).copy()).to(dev)
    return sm.execute(t(kind), payload, t(ko), t(kl), t(vo), t(vl), stream=stream) + (payload,)


def heap_of(sm):
    """the whole heap, uint8 [G, heap_bytes] (small stores only)"""
    offs = sm.debug_arena()[2]
    return sm.debug_read(offs[5], sm.G * sm.heap_bytes).reshape(sm.G, sm.heap_bytes)


def collect(sm, res, values=True):
    """the results as Python values: None / bytes / "FULL" (values = False: the length instead of the bytes)"""
    st, off, ln = (x.cpu().numpy() for x in res[:3])
    heap = heap_of(sm) if values else None
    out = []
    for i in range(st.shape[0]):
        out.append([None if st[i, g] == 0 else ("FULL" if st[i, g] == 2 else (bytes(heap[g, off[i, g]:off[i, g] + ln[i, g]]) if values else int(ln[i, g])))
                    for g in range(sm.G)])
    return out


def run(sm, dev, rows):
    return collect(sm, submit(sm, dev, rows))


def apply(model, rows, where=None):
    """what the dicts answer to `rows` (and become); where[g]: the model of position g (None: no model there)"""
    out = []
    for row in rows:
        r = []
        for g, c in enumerate(row):
            m = model[g] if where is None else (None if where[g] is None else model[where[g]])
            if c is None or m is None:
                r.append(None)
                continue
            r.append(m.get(c[1]))
            if c[0] == "put":
                m[c[1]] = c[2]
        out.append(r)
    return out


def fill(sm, dev, dicts, order=None):
    """Puts that leave group g holding dicts[g], one key a row (order: a permutation of each group's keys)"""
    keys = [list(d) if order is None else order(list(d)) for d in dicts]
    rows = [[("put", k[i], dicts[g][k[i]]) if i < len(k) else None for g, k in enumerate(keys)] for i in range(max(len(k) for k in keys))]
    if rows:
        got = run(sm, dev, rows)
        assert all(x is None for r in got for x in r)
    return sm


def gets_equal(sm, dev, dicts, what, where=None, extra=(b"no such key",)):
    """a Get of every key of its model (and of keys it does not hold) answers what the model holds"""
    n = len(dicts) if where is None else sm.G
    mod = lambda g: dicts[g] if where is None else (None if where[g] is None else dicts[where[g]])   # noqa: E731
    keys = [sorted(mod(g)) + list(extra) if mod(g) is not None else [] for g in range(n)]
    rows = [[("get", k[i]) if i < len(k) else None for k in keys] for i in range(max(len(k) for k in keys))]
    got = run(sm, dev, rows)
    for i, row in enumerate(rows):
        for g, c in enumerate(row):
            want = None if c is None else mod(g).get(c[1])
            assert got[i][g] == want, (what, i, g, c, got[i][g], want)


def raw(sm):
    """every array of the store, read raw"""
    _, n, offs = sm.debug_arena()
    G, S = sm.G, sm.slots
    out = {"hash": np.frombuffer(sm.debug_read(offs[0], 8 * S * G).tobytes(), "<u8").reshape(S, G)}
    for k, name in enumerate(TABLE[1:], 1):
        out[name] = np.frombuffer(sm.debug_read(offs[k], 4 * S * G).tobytes(), "<u4").reshape(S, G)
    out["heap"] = heap_of(sm)
    out["heap_used"] = np.frombuffer(sm.debug_read(offs[6], 4 * G).tobytes(), "<u4")
    out["full"] = sm.debug_read(offs[7], G).copy()
    out["n_keys"] = np.frombuffer(sm.debug_read(offs[8], 4 * G).tobytes(), "<u4")
    return out


def raw_equal(a, b, groups, what, heap=True):
    for n in a:
        if n == "heap" and not heap:
            continue
        x, y = (a[n][groups] if n == "heap" else a[n][..., groups]), (b[n][groups] if n == "heap" else b[n][..., groups])
        assert np.array_equal(x, y), (what, n)


def as_new(r, fresh, groups, what):
    """the listed groups are what a new store holds (heap bytes are not state)"""
    for n in TABLE + ("heap_used", "n_keys", "full"):
        assert np.array_equal(r[n][..., groups], fresh[n][..., np.arange(len(groups)) % fresh[n].shape[-1]]), (what, n)


def _close(xs):
    for x in xs:
        x.close()


def _rng_dicts(rng, n, pool, most, vmax=24):
    out = []
    for _ in range(n):
        ks = rng.permutation(len(pool))[:int(rng.integers(0, most + 1))]
        out.append({pool[k]: rng.integers(0, 256, int(rng.integers(0, vmax + 1)), dtype=np.uint8).tobytes() for k in ks})
    return out


def _pool(rng, n=26):
    alnum = np.frombuffer(b"ABCDEFGHIJKLMNOPQRSTUVWXYZabcdefghijklmnopqrstuvwxyz0123456789", np.uint8)
    keys = {b""}
    while len(keys) < n:
        keys.add(alnum[rng.integers(0, 62, int(rng.integers(1, 12)))].tobytes())
    return sorted(keys)


# ---- 2: identity at every boundary --------------------------------------------------------------------------------------------
def identity_at_every_boundary(dev, G=130, slots=(32, 64), heap=(4096, 3072), rows=4, sizes=(None, 1, 63, 64, 65, 130)):
    """random Put / Get / none rows from a 26-key pool (b"" among them) in several calls; after each call the state goes into a
    second store -- whole, then through lists of 1, 63, 64, 65 and 130 groups in a shuffled order -- and both stores take the
    same next commands: every result equals the dict model, n_keys too, and a loaded group's heap_used is sum(klen + vlen)"""
    from summerset_amd import StringKvStateMachine
    rng = np.random.default_rng(101)
    pool = _pool(rng)
    a, b = StringKvStateMachine(G, slots[0], heap[0]), StringKvStateMachine(G, slots[1], heap[1])
    model = [dict() for _ in range(G)]
    for call, n in enumerate(sizes):
        cmds = []
        for _ in range(rows):
            row = []
            for g in range(G):
                u, k = rng.random(), pool[int(rng.integers(len(pool)))]
                row.append(None if u < 0.15 else (("get", k) if u < 0.45 else ("put", k, rng.integers(0, 256, int(rng.integers(0, 30)), dtype=np.uint8).tobytes())))
            cmds.append(row)
        shadow = [dict(m) for m in model]
        want = apply(model, cmds)
        assert run(a, dev, cmds) == want, ("source", call)
        if call:
            assert apply(shadow, cmds) == want and run(b, dev, cmds) == want, ("loaded side", call)
        if n is None:
            snap = a.save_state()
            b.load_state(snap)
            lst = np.arange(G)
        else:
            lst = rng.permutation(G)[:n]
            snap = a.save_groups(lst)
            b.load_groups(snap, lst)
        assert snap.export() == model_image([model[g] for g in lst]), call
        sa, sb = a.stats(), b.stats()
        assert [int(x) for x in sa["n_keys"]] == [len(m) for m in model] == [int(x) for x in sb["n_keys"]], call
        assert [int(sb["heap_used"][g]) for g in lst] == [live_bytes(model[g]) for g in lst], call
        assert not sa["full"].any() and not sb["full"].any()
        snap.close()
    gets_equal(b, dev, model, "at the end")
    _close([a, b])


# ---- 3: canonical bytes -------------------------------------------------------------------------------------------------------
def canonical_bytes(dev, G=70):
    """the same maps built three ways -- slots 16 / 64, different heap_bytes, every key overwritten 20 times and inserted in another
    order -- export the same bytes, and those are model_image's; items() gives the dicts back"""
    from summerset_amd import StringKvStateMachine
    rng = np.random.default_rng(103)
    dicts = _rng_dicts(rng, G, _pool(rng), 12)
    dicts[5], dicts[64] = {}, {b"": b""}
    a = fill(StringKvStateMachine(G, 16, 1024), dev, dicts)
    b = fill(StringKvStateMachine(G, 64, 4096), dev, dicts, order=lambda k: k[::-1])
    c = StringKvStateMachine(G, 32, 8192)
    for r in range(20):                                          # 19 other values first, each key's in another order every round
        junk = [{k: bytes([r]) * ((r + len(k)) % 23) for k in d} for d in dicts]
        c = fill_over(c, dev, junk if r < 19 else dicts, np.random.default_rng(r))
    sa, sb, sc = a.save_state(), b.save_state(), c.save_state()
    want = model_image(dicts)
    assert sa.export() == want and sb.export() == want and sc.export() == want
    assert sa.items() == dicts and not sa.full_flags().any()
    i = sa.info()
    assert i["bytes"] == len(want) and i["n_records"] == sum(len(d) for d in dicts) and i["n_groups"] == G
    assert i["max_keys"] == max(len(d) for d in dicts) and i["max_group_bytes"] == max(live_bytes(d) for d in dicts)
    assert int(c.stats()["heap_used"].sum()) > 3 * sum(live_bytes(d) for d in dicts)   # c's heaps are mostly dead bytes
    _close([a, b, c, sa, sb, sc])


def fill_over(sm, dev, dicts, rng):
    """Puts of every pair in a random key order per group; earlier values are overwritten (the result is the old value or None)"""
    keys = [[list(d)[j] for j in rng.permutation(len(d))] for d in dicts]
    rows = [[("put", k[i], dicts[g][k[i]]) if i < len(k) else None for g, k in enumerate(keys)] for i in range(max(len(k) for k in keys))]
    got = run(sm, dev, rows)
    assert not any(x == "FULL" for r in got for x in r)
    return sm


# ---- 4: record sizes around the pad -------------------------------------------------------------------------------------------
def record_sizes_around_the_pad(dev, G=130, slots=8):
    """klen + vlen = 0, 1, 15, 16, 17, 31, 32, 33 with empty keys and empty values; a group with no keys between groups that hold
    some; a tile whose groups hold 0 .. slots keys; whole and through a list, out and back in"""
    from summerset_amd import StringKvStateMachine
    pairs = []                                                   # (klen, vlen): the key's first byte tells them apart
    for total in (0, 1, 15, 16, 17, 31, 32, 33):
        pairs += sorted({(0, total), (total, 0), (total // 2, total - total // 2), (1 if total else 0, max(total - 1, 0))})
    assert {k + v for k, v in pairs} == {0, 1, 15, 16, 17, 31, 32, 33}
    dicts = []
    for g in range(G):
        n = g % (slots + 1) if g < 64 else (0 if g % 3 == 1 else 1 + (g * 7) % slots)   # tile 0: 0 .. slots keys; then empty groups in between
        d, j = {}, g
        while len(d) < n:
            kl, vl = pairs[j % len(pairs)]
            j += 1
            key = bytes([(65 + j + i) & 0xFF for i in range(kl)])
            if key not in d:
                d[key] = bytes([(g + 3 * i) & 0xFF for i in range(vl)])
        dicts.append(d)
    assert {len(d) for d in dicts[:64]} == set(range(slots + 1)) and any(b"" in d for d in dicts) and any(b"" in d.values() for d in dicts)
    a = fill(StringKvStateMachine(G, slots, 512), dev, dicts)
    snap = a.save_state()
    assert snap.export() == model_image(dicts)
    b = StringKvStateMachine(G, 2 * slots, 384)
    b.load_state(snap)
    gets_equal(b, dev, dicts, "whole", extra=(b"zz", b""))
    lst = np.random.default_rng(5).permutation(G)[:77]
    gs = b.save_groups(lst)
    assert gs.export() == model_image([dicts[g] for g in lst]) and gs.items() == [dicts[g] for g in lst]
    c = StringKvStateMachine(77, slots, 300)
    c.load_state(gs)                                             # a group image is the whole image of a 77-group store
    gets_equal(c, dev, [dicts[g] for g in lst], "interchange", extra=(b"zz", b""))
    assert [int(x) for x in c.stats()["heap_used"]] == [live_bytes(dicts[g]) for g in lst]
    _close([a, b, c, snap, gs])


# ---- 5: a full table ----------------------------------------------------------------------------------------------------------
def full_table(dev, slots=8):
    """n_keys == slots saved and loaded into a store of the same slots (probes wrap); later Gets find every key; a Put of a new key
    sets full; a group that is full already stays full through save / load and refuses"""
    from summerset_amd import StringKvStateMachine
    G = 4
    dicts = [{bytes([97 + i]) * (1 + g): bytes([i, g]) for i in range(slots)} for g in range(2)] + [{b"q": b"1"}, {b"x": b"y", b"": b"e"}]
    a = fill(StringKvStateMachine(G, slots, 256), dev, dicts)
    # group 2 becomes full: its heap cannot take 300 bytes
    assert run(a, dev, [[None, None, ("put", b"big", b"v" * 300), None]]) == [[None, None, "FULL", None]]
    assert a.stats()["full"].tolist() == [0, 0, 1, 0] and a.stats()["n_keys"].tolist() == [slots, slots, 1, 2]
    snap = a.save_state()
    assert snap.export() == model_image(dicts, [0, 0, 1, 0]) and snap.full_flags().tolist() == [0, 0, 1, 0]
    b = StringKvStateMachine(G, slots, 200)
    b.load_state(snap)
    r = raw(b)
    assert (r["klen"][:, :2] != EMPTY).all()                     # every entry taken: the probes wrapped
    for g in range(2):                                           # ... each record at the first free entry from hash & mask, in rank order
        taken = []
        for key in sorted(dicts[g], key=lambda k: (fnv1a(k), len(k), k)):
            s = fnv1a(key) & (slots - 1)
            while s in taken:
                s = (s + 1) & (slots - 1)
            taken.append(s)
            assert int(r["hash"][s, g]) == fnv1a(key) and int(r["klen"][s, g]) == len(key), (g, key)
    st = b.stats()
    assert st["full"].tolist() == [0, 0, 1, 0] and st["n_keys"].tolist() == [slots, slots, 1, 2]
    rows = [[("get", k) for k in (list(dicts[0])[i], list(dicts[1])[i])] + [("get", b"q"), ("get", b"x" if i % 2 else b"")] for i in range(slots)]
    got = run(b, dev, rows)
    for i, row in enumerate(rows):
        assert got[i][:2] == [dicts[0][row[0][1]], dicts[1][row[1][1]]] and got[i][2] == "FULL" and got[i][3] == dicts[3][row[3][1]], i
    got = run(b, dev, [[("put", b"new key", b"v"), ("put", list(dicts[1])[0], b"w"), ("get", b"q"), ("put", b"n", b"m")]])
    assert got == [["FULL", dicts[1][list(dicts[1])[0]], "FULL", None]]   # a ninth key: refused; an overwrite and group 3 go on
    assert b.stats()["full"].tolist() == [1, 0, 1, 0]
    _close([a, b, snap])


# ---- 6: compaction ------------------------------------------------------------------------------------------------------------
def compaction(dev, heap=256):
    """a group's heap filled by overwrites to within one value of heap_bytes, not full: after compact its heap_used is the live size
    and the next Puts succeed where they set full in a store that was not compacted; the neighbours are unchanged"""
    from summerset_amd import StringKvStateMachine
    G, val = 5, 40
    stores = [StringKvStateMachine(G, 8, heap) for _ in range(2)]   # [1]: the control, never compacted
    model = [{b"n%d" % g: b"neighbour %d" % g} for g in range(G)]
    model[2] = {}
    n_over = (heap - 1) // val
    for sm in stores:
        fill(sm, dev, model)
        rows = [[None, None, ("put", b"k", bytes([i]) * val), ("put", b"n3", b"v%d" % i) if i == 1 else None, None] for i in range(n_over)]
        run(sm, dev, rows)
    model[2][b"k"] = bytes([n_over - 1]) * val
    model[3][b"n3"] = b"v1"
    a, ctl = stores
    st0, r0 = a.stats(), raw(a)
    assert int(st0["heap_used"][2]) == 1 + val * n_over and heap - int(st0["heap_used"][2]) < val and not st0["full"].any()
    snap = a.compact([2])
    st1, r1 = a.stats(), raw(a)
    assert int(st1["heap_used"][2]) == 1 + val == live_bytes(model[2]) and int(st1["n_keys"][2]) == 1 and not st1["full"].any()
    rest = [0, 1, 3, 4]
    raw_equal(r1, r0, rest, "beside a compaction")
    more = [[None, None, ("put", b"k", bytes([100 + i]) * val), None, None] for i in range(3)]
    got, got_ctl = run(a, dev, more), run(ctl, dev, more)
    assert [r[2] for r in got] == [bytes([n_over - 1]) * val, bytes([100]) * val, bytes([101]) * val]
    assert [r[2] for r in got_ctl] == ["FULL"] * 3 and ctl.stats()["full"].tolist() == [0, 0, 1, 0, 0]
    model[2][b"k"] = bytes([102]) * val
    gets_equal(a, dev, model, "after the compaction")
    assert not a.stats()["full"].any()
    a.compact([2, 0], None)                                      # again, with a neighbour: nothing changes for the maps
    gets_equal(a, dev, model, "after the second compaction")
    _close(stores + [snap])


# ---- 7: a move changes object and position ------------------------------------------------------------------------------------
def move_between_stores(dev, GA=70, GB=50, n_models=80, rounds=4):
    """two stores of different geometry; between command batches random lists of groups move between them with move_skv_groups, to
    other positions; the host keeps the table of which model sits where; every result equals the model throughout, and the source
    groups are as new after the reset, read raw"""
    from summerset_amd import StringKvStateMachine, move_skv_groups
    rng = np.random.default_rng(107)
    pool = _pool(rng, 12)
    st = [StringKvStateMachine(GA, 16, 2048), StringKvStateMachine(GB, 32, 3000)]
    fresh = [raw(StringKvStateMachine(4, 16, 64)), raw(StringKvStateMachine(4, 32, 64))]
    where = [[None] * GA, [None] * GB]                           # where[s][position] = model id
    for m in range(n_models):
        s = 0 if m < 50 else 1
        where[s][[p for p in rng.permutation(len(where[s])) if where[s][p] is None][0]] = m
    model = [dict() for _ in range(n_models)]
    for rnd in range(rounds):
        for s in (0, 1):
            cmds = []
            for _ in range(3):
                row = []
                for p in range(st[s].G):
                    u, k = rng.random(), pool[int(rng.integers(len(pool)))]
                    row.append(None if where[s][p] is None or u < 0.1 else (("get", k) if u < 0.4 else ("put", k, rng.integers(0, 256, int(rng.integers(0, 20)), dtype=np.uint8).tobytes())))
                cmds.append(row)
            assert run(st[s], dev, cmds) == apply(model, cmds, where[s]), (rnd, s)
        src, dst = rnd % 2, 1 - rnd % 2
        free = [p for p in rng.permutation(st[dst].G) if where[dst][p] is None]
        held = [p for p in rng.permutation(st[src].G) if where[src][p] is not None]
        k = min(len(free), len(held), 17)
        sp, dp = held[:k], free[:k]
        snap = move_skv_groups(st[src], sp, st[dst], dp)
        assert snap.items() == [model[where[src][p]] for p in sp]
        for p, q in zip(sp, dp):
            where[dst][q], where[src][p] = where[src][p], None
        as_new(raw(st[src]), fresh[src], np.array(sp), ("source after the move", rnd))
        snap.close()
    for s in (0, 1):
        gets_equal(st[s], dev, model, ("at the end", s), where=where[s])
        n = st[s].stats()["n_keys"]
        assert [int(x) for x in n] == [0 if m is None else len(model[m]) for m in where[s]]
    _close(st)


# ---- 8: neighbours untouched --------------------------------------------------------------------------------------------------
def _view(addr, n):
    return np.ctypeslib.as_array((C.c_uint8 * n).from_address(addr))


def neighbours_untouched(dev, G=70, k=23, zones=None):
    """raw copies of every table array, heap_used, n_keys, full and the heap strips of the unlisted groups are identical before and
    after a load_groups and a reset_groups.  zones (the emulator's red_zones): a save and a load of a run of groups inside red zones
    around the image in the snapshot's buffer and around the listed groups' heap strips, with zero hits"""
    from summerset_amd import StringKvSnapshot, StringKvStateMachine
    rng = np.random.default_rng(109)
    pool = _pool(rng, 10)
    da, db = _rng_dicts(rng, G, pool, 8), _rng_dicts(rng, G, pool, 8)
    a, b = fill(StringKvStateMachine(G, 16, 1024), dev, da), fill(StringKvStateMachine(G, 8, 512), dev, db)
    fill_over(a, dev, da, rng)                                   # dead bytes in a's heaps
    r0 = raw(a)
    la, lb = rng.permutation(G)[:k], rng.permutation(G)[:k]
    snap = b.save_groups(lb)
    a.load_groups(snap, la)
    r1 = raw(a)
    rest = np.setdiff1d(np.arange(G), la)
    raw_equal(r1, r0, rest, "beside a load")
    for x, g in enumerate(la):
        da[g] = dict(db[lb[x]])
        used = int(r1["heap_used"][g])
        assert used == live_bytes(da[g]) and np.array_equal(r1["heap"][g, used:], r0["heap"][g, used:]), "bytes behind heap_used were touched"
    lc = rng.permutation(G)[:k]
    a.reset_groups(lc)
    r2 = raw(a)
    raw_equal(r2, r1, np.setdiff1d(np.arange(G), lc), "beside a reset")
    assert np.array_equal(r2["heap"], r1["heap"]), "a reset touched heap bytes"
    as_new(r2, raw(StringKvStateMachine(4, 16, 64)), lc, "reset is create")
    for g in lc:
        da[g] = {}
    gets_equal(a, dev, da, "after load and reset")
    if zones is not None:
        g0, n = 21, 30
        run_of = g0 + rng.permutation(n)                         # a run of groups, in a shuffled order: one window of the heap
        gs = StringKvSnapshot(a, n)
        base, _, offs = a.debug_arena()
        heap = _view(base + offs[5], G * a.heap_bytes)
        p, nb = C.c_void_p(), C.c_uint64()
        from summerset_amd import _lib
        _lib.check(_lib.load().smr_skv_snapshot_debug_buffer(gs._h, C.byref(p), C.byref(nb)))
        buf = _view(p.value, nb.value)
        img = model_image([da[g] for g in run_of])
        n_rec = sum(len(da[g]) for g in run_of)
        used = _a16(64 + _a8(4 * n) + _a8(n)) + 16 * n * a.slots + (len(img) - _a16(64 + _a8(4 * n) + _a8(n) + 16 * n_rec))   # records at capacity
        assert used < nb.value
        with zones(buf, 0, used, (heap, g0 * a.heap_bytes, (g0 + n) * a.heap_bytes)) as hits:
            a.save_groups(run_of, gs)
        assert hits.count == 0, hits.first
        assert gs.export() == img
        with zones(buf, 0, used, (heap, g0 * a.heap_bytes, (g0 + n) * a.heap_bytes)) as hits:
            a.load_groups(gs, run_of[::-1])
        assert hits.count == 0, hits.first
        saved = [dict(da[g]) for g in run_of]
        for x, g in enumerate(run_of[::-1]):
            da[g] = saved[x]
        gets_equal(a, dev, da, "after the load inside red zones")
        gs.close()
    _close([a, b, snap])


# ---- 9: list shapes -----------------------------------------------------------------------------------------------------------
def list_shapes(dev, G=400, n=330):
    """330 list entries: six tiles, two blocks of the head launch"""
    from summerset_amd import StringKvStateMachine
    rng = np.random.default_rng(113)
    dicts = _rng_dicts(rng, G, _pool(rng, 8), 4, vmax=12)
    a = fill(StringKvStateMachine(G, 8, 256), dev, dicts)
    src, dst = rng.permutation(G)[:n], rng.permutation(G)[:n]
    snap = a.save_groups(src)
    assert snap.export() == model_image([dicts[g] for g in src])
    b = StringKvStateMachine(G, 8, 128)
    b.load_groups(snap, dst)
    want = [{} for _ in range(G)]
    for s, d in zip(src, dst):
        want[d] = dicts[s]
    gets_equal(b, dev, want, "330 entries")
    assert [int(x) for x in b.stats()["n_keys"]] == [len(d) for d in want]
    _close([a, b, snap])


def _bulk(sm, dev, kind, blob, ko, kl, vo, vl):
    """one row of commands from arrays [G]; -> state, off, len as numpy"""
    import torch
    t = lambda a, dt: torch.from_numpy(np.ascontiguousarray(a, dt)[None, :]).to(dev)   # noqa: E731
    payload = torch.from_numpy(np.frombuffer(blob, np.uint8).copy()).to(dev) if isinstance(blob, bytes) else blob
    st, off, ln = sm.execute(t(kind, np.uint8), payload, t(ko, np.int32), t(kl, np.int32), t(vo, np.int32), t(vl, np.int32))
    return st.cpu().numpy()[0], off.cpu().numpy()[0], ln.cpu().numpy()[0]


def permutation_onto_itself(dev, G=66000):
    """DEVICE ONLY (66 000 lanes are too many fibers for the emulator): a permutation of a 66 000-group store -- 1 032 tiles for
    1 024 wavefronts, so wavefronts take two tiles -- with slots = 8 and heap_bytes = 256, moved onto itself in reversed order"""
    from summerset_amd import StringKvStateMachine
    a = StringKvStateMachine(G, 8, 256)
    ids = np.arange(G, dtype="<u4")
    blob = b"ab" + ids.tobytes()
    ones, zeros = np.ones(G), np.zeros(G)
    for key in (0, 1):                                           # "a" -> the group's id (4 bytes), "b" -> the first 1 + g % 4 bytes of it
        st, _, _ = _bulk(a, dev, ones * PUT, blob, zeros + key, ones, 2 + 4 * ids, (ones * 4) if key == 0 else 1 + ids % 4)
        assert not st.any()
    lst = np.random.default_rng(127).permutation(G)
    snap = a.save_groups(lst)
    i = snap.info()
    assert i["n_records"] == 2 * G and i["byte_bytes"] == 32 * G and i["max_keys"] == 2 and i["max_group_bytes"] == 10
    a.load_groups(snap, lst[::-1])                               # group lst[::-1][x] now holds what lst[x] held
    came_from = np.empty(G, np.int64)
    came_from[lst[::-1]] = lst
    heap = heap_of(a)
    for key in (0, 1):
        st, off, ln = _bulk(a, dev, ones * GET, blob, zeros + key, ones, zeros, zeros)
        want_len = 4 if key == 0 else 1 + came_from % 4
        assert (st == 1).all() and (ln == want_len).all()
        got = np.zeros((G, 4), np.uint8)
        for j in range(4):
            got[:, j] = np.where(j < ln, heap[np.arange(G), np.minimum(off + j, 255)], 0)
        want = came_from.astype("<u4").view(np.uint8).reshape(G, 4).copy()
        want[np.arange(4)[None, :] >= np.broadcast_to(want_len, (G,))[:, None]] = 0
        assert np.array_equal(got, want), key
    st = a.stats()
    assert (st["n_keys"] == 2).all() and np.array_equal(st["heap_used"], 2 + 4 + 1 + came_from % 4) and not st["full"].any()
    _close([a, snap])


# ---- 10: past 4 GiB -----------------------------------------------------------------------------------------------------------
def past_4gib(dev, G=70000, heap=66000, vlen=65000):
    """DEVICE ONLY (9 GiB of heaps): 70 000 groups of heap_bytes = 66 000, slots = 2; every group Puts one key whose value is the
    same 65 000-byte run of one seeded payload buffer; the first group, the last group and the first group whose strip starts
    beyond 4 GiB Put a second, short value; save, load into a second store, read back those three groups and 20 seeded others;
    the image is larger than 2^32 bytes and its size is the model's arithmetic"""
    import torch
    from summerset_amd import StringKvStateMachine
    rng = np.random.default_rng(131)
    run_bytes = rng.integers(0, 256, vlen, dtype=np.uint8).tobytes()
    shorts = [b"first", b"the last group", b"beyond four GiB"]
    blob = b"kx" + run_bytes + b"".join(shorts)
    payload = torch.from_numpy(np.frombuffer(blob, np.uint8).copy()).to(dev)
    far = -(-(1 << 32) // heap)                                  # the first group whose strip starts at or beyond 2^32
    assert (far - 1) * heap < (1 << 32) <= far * heap < (G - 1) * heap
    special = [0, G - 1, far]
    a, b = StringKvStateMachine(G, 2, heap), StringKvStateMachine(G, 2, heap)
    ones, zeros = np.ones(G), np.zeros(G)
    st, _, _ = _bulk(a, dev, ones * PUT, payload, zeros, ones, zeros + 2, zeros + vlen)
    assert not st.any()
    kind, vo, vl = np.full(G, NOP), np.zeros(G), np.zeros(G)
    at = 2 + vlen
    for g, s in zip(special, shorts):
        kind[g], vo[g], vl[g] = PUT, at, len(s)
        at += len(s)
    st, _, _ = _bulk(a, dev, kind, payload, zeros + 1, ones, vo, vl)
    assert not st.any()
    snap = a.save_state()
    b.load_state(snap)
    i = snap.info()
    fixed = 64 + _a8(4 * G) + _a8(G)
    n_rec = G + 3
    byte_bytes = G * _a16(1 + vlen) + sum(_a16(1 + len(s)) for s in shorts)
    assert i["bytes"] == _a16(fixed + 16 * n_rec) + byte_bytes and i["bytes"] > (1 << 32)
    assert i["n_records"] == n_rec and i["byte_bytes"] == byte_bytes and i["max_keys"] == 2 and i["max_group_bytes"] == 1 + vlen + 1 + max(len(s) for s in shorts)
    for key in (0, 1):
        st, off, ln = _bulk(b, dev, ones * GET, payload, zeros + key, ones, zeros, zeros)
        if key == 0:
            assert (st == 1).all() and (ln == vlen).all()
            for g in special + [int(x) for x in rng.integers(0, G, 20)]:
                assert b.heap_bytes_of(g, off[g], ln[g]) == run_bytes, g
        else:
            assert sorted(np.nonzero(st)[0].tolist()) == sorted(special)
            for g, s in zip(special, shorts):
                assert b.heap_bytes_of(g, off[g], ln[g]) == s, g
    sb = b.stats()
    assert (sb["n_keys"] == 1 + np.isin(np.arange(G), special)).all() and not sb["full"].any()
    assert int(sb["heap_used"][far]) == 1 + vlen + 1 + len(shorts[2]) and int(sb["heap_used"][1]) == 1 + vlen
    _close([a, b, snap])


# ---- 11: refusals -------------------------------------------------------------------------------------------------------------
def _refused(fn, word=None, code=None):
    from summerset_amd import SummersetError
    try:
        fn()
    except SummersetError as e:
        assert word is None or word in e.msg, (word, e.msg)
        assert code is None or e.code == code, (code, e.code, e.msg)
        return
    raise AssertionError("not refused (%s)" % word)


def refusals(dev, G=40, n=7):
    """every refusal of the header's list, each leaving store and snapshot byte-identical"""
    from summerset_amd import StringKvSnapshot, StringKvStateMachine, _lib
    L = _lib.load()
    ARG, STATE = _lib.SMR_ERR_ARG, _lib.SMR_ERR_STATE
    rng = np.random.default_rng(137)
    dicts = _rng_dicts(rng, G, _pool(rng, 10), 8)
    dicts[3] = {bytes([65 + i]): b"0123456789" * 5 for i in range(8)}          # eight keys, 408 bytes: the group that does not fit below
    a = fill(StringKvStateMachine(G, 16, 1024), dev, dicts)
    lst = np.arange(3, 3 + n)
    good = a.save_groups(lst)
    img0, r0 = good.export(), raw(a)

    def unchanged(what):
        r1 = raw(a)
        raw_equal(r1, r0, np.arange(G), what)
        assert good.export() == img0, what
    null, sp = C.c_void_p(None), C.c_void_p(0)
    gl = np.ascontiguousarray(lst, np.uint32)
    glp = gl.ctypes.data_as(C.c_void_p)
    for call in (lambda: L.smr_skv_save_state(null, good._h, sp), lambda: L.smr_skv_save_state(a._h, null, sp), lambda: L.smr_skv_load_state(null, good._h, sp),
                 lambda: L.smr_skv_load_state(a._h, null, sp), lambda: L.smr_skv_save_groups(null, glp, n, good._h, sp),
                 lambda: L.smr_skv_save_groups(a._h, None, n, good._h, sp), lambda: L.smr_skv_save_groups(a._h, glp, n, null, sp),
                 lambda: L.smr_skv_load_groups(null, good._h, glp, n, sp), lambda: L.smr_skv_load_groups(a._h, null, glp, n, sp),
                 lambda: L.smr_skv_load_groups(a._h, good._h, None, n, sp), lambda: L.smr_skv_reset_groups(null, glp, n, sp),
                 lambda: L.smr_skv_reset_groups(a._h, None, n, sp), lambda: L.smr_skv_snapshot_create(null, C.byref(C.c_void_p())),
                 lambda: L.smr_skv_snapshot_create(a._h, None), lambda: L.smr_skv_snapshot_import(good._h, None, 64),
                 lambda: L.smr_skv_snapshot_info_get(good._h, None), lambda: L.smr_skv_snapshot_export(good._h, None, 1 << 20)):
        _refused(lambda: _lib.check(int(call())), "null argument", ARG)
    unchanged("null arguments")
    for bad, word in (([], "a list of 0"), (list(range(G + 1)), "a list of"), ([0, G], "is group"), ([0, 2**32 - 1], "is group"), ([4, 5, 4], "listed twice")):
        k = len(bad)
        if 0 < k <= G:
            s = StringKvSnapshot(a, k)
            s.import_(a.save_groups(np.arange(k)).export())
        else:
            s = good                                             # (no snapshot of 0 or G + 1 groups can be made: below)
        _refused(lambda: a.save_groups(bad, s), word if 0 < k <= G else None, ARG)
        _refused(lambda: a.load_groups(s, bad), word if 0 < k <= G else None, ARG)
        _refused(lambda: a.reset_groups(bad), word, ARG)
        unchanged(("list", word))
    for k in (0, G + 1):
        _refused(lambda: StringKvSnapshot(a, k), "a snapshot of", ARG)
    other = np.arange(n + 1)                                     # a list length that is not the snapshot's n_groups
    _refused(lambda: a.save_groups(other, good), "made for", ARG)
    _refused(lambda: a.load_groups(good, other), "made for", ARG)
    whole = a.save_state()
    _refused(lambda: a.load_groups(whole, lst), "made for", ARG)
    _refused(lambda: a.load_state(good), "another n_groups", ARG)
    _refused(lambda: a.save_state(good), "another n_groups", ARG)
    empty = StringKvSnapshot(a, n)                               # a load before any save
    _refused(lambda: a.load_groups(empty, lst), "nothing saved", STATE)
    _refused(lambda: a.load_state(StringKvSnapshot(a)), "nothing saved", STATE)
    _refused(lambda: empty.info(), "nothing saved", STATE)
    unchanged("another n, an empty snapshot")
    small = StringKvStateMachine(G, 4, 1024)                     # max_keys > slots
    tight = StringKvStateMachine(G, 16, 400)                     # max_group_bytes > heap_bytes
    fill(small, dev, [{b"s": b"t"}] * G); fill(tight, dev, [{b"s": b"t"}] * G)
    rs, rt = raw(small), raw(tight)
    assert good.info()["max_keys"] == 8 and good.info()["max_group_bytes"] == 408
    _refused(lambda: small.load_groups(good, lst), "does not fit 4 slots", ARG)
    _refused(lambda: tight.load_groups(good, lst), "does not fit heap_bytes 400", ARG)
    raw_equal(raw(small), rs, np.arange(G), "max_keys > slots"); raw_equal(raw(tight), rt, np.arange(G), "max_group_bytes > heap_bytes")
    # import: every way an image can be wrong; the snapshot keeps what it held
    tgt = StringKvSnapshot(a, n)
    tgt.import_(img0)
    assert (4 * n) % 8 == 4 and n % 8                            # (both fixed arrays end in pad bytes)
    hdr = lambda **kw: _patch_hdr(img0, **kw)                    # noqa: E731
    fixed = 64 + _a8(4 * n) + _a8(n)
    n_rec = good.info()["n_records"]
    o_bytes = _a16(fixed + 16 * n_rec)
    rec = lambda i: struct.unpack_from("<QII", img0, fixed + 16 * i)   # noqa: E731
    first_pad = next(i for i in range(n_rec) if (rec(i)[1] + rec(i)[2]) % 16)    # (record i's run has pad bytes)
    pad_at = o_bytes + sum(_a16(rec(j)[1] + rec(j)[2]) for j in range(first_pad)) + rec(first_pad)[1] + rec(first_pad)[2]
    swapped = bytearray(img0)                                    # group 3 (position 0) holds eight keys: its ranks 0 and 1 are records 0 and r1
    nk0 = np.frombuffer(img0, "<u4", n, 64)
    r1 = int((nk0 > 0).sum())
    assert nk0[0] == 8 and rec(0)[1:] == rec(r1)[1:] == (1, 50)
    swapped[fixed:fixed + 16], swapped[fixed + 16 * r1:fixed + 16 * r1 + 16] = img0[fixed + 16 * r1:fixed + 16 * r1 + 16], img0[fixed:fixed + 16]
    r0b, rnb = _run_at(img0, fixed, o_bytes, 0), _run_at(img0, fixed, o_bytes, r1)
    swapped[r0b[0]:r0b[1]], swapped[rnb[0]:rnb[1]] = img0[rnb[0]:rnb[1]], img0[r0b[0]:r0b[1]]   # (their bytes too: the hashes still match)
    one_more = bytearray(img0)
    struct.pack_into("<I", one_more, 64 + 4 * 2, np.frombuffer(img0, "<u4", n, 64)[2] + 1)
    for bad, word in ((img0[:-1], "truncated"), (img0[:40], "shorter than its header"), (img0[:fixed + 8], "truncated"),
                      (hdr(magic=SKV_MAGIC ^ 1), "magic"), (hdr(version=2), "version"),
                      (_poke(img0, pad_at, 1), "padding is not zero"), (_poke(img0, 64 + 4 * n, 1), "padding is not zero"),
                      (_poke(img0, 64 + _a8(4 * n) + n, 1), "padding is not zero"), (_poke(img0, 64 + _a8(4 * n), 2), "neither 0 nor 1"),
                      (bytes(swapped), "rank order"), (bytes(one_more), "n_keys"),
                      (hdr(max_keys=9), None), (hdr(max_group_bytes=409), None), (hdr(n_groups=n + 1), "another n_groups"),
                      (_poke(img0, fixed + 8, rec(0)[1] + 1), None)):
        _refused(lambda: tgt.import_(bad), word, ARG)
        assert tgt.export() == img0, word
    _refused(lambda: _lib.check(int(L.smr_skv_snapshot_export(good._h, (C.c_uint8 * 8)(), 8))), "the image takes", ARG)
    unchanged("imports")
    _close([a, small, tight, good, whole, empty, tgt])


def _patch_hdr(img, **kw):
    names = ("magic", "version", "n_groups", "max_keys", "max_group_bytes")
    f = list(struct.unpack_from("<IIIII", img, 0))
    for k, v in kw.items():
        f[names.index(k)] = v
    return struct.pack("<IIIII", *f) + img[20:]


def _poke(img, at, value):
    b = bytearray(img)
    b[at] = value & 0xFF
    return bytes(b)


def _run_at(img, fixed, o_bytes, i):
    """[start, end) of record i's padded run"""
    lens = [sum(struct.unpack_from("<II", img, fixed + 16 * j + 8)) for j in range(i + 1)]
    start = o_bytes + sum(_a16(x) for x in lens[:-1])
    return start, start + _a16(lens[-1])


# ---- 12: stream order ---------------------------------------------------------------------------------------------------------
def stream_order(dev, G=70, k=40):
    """on one non-default stream: save, execute, load, execute back to back with no host synchronisation of the test's own; the
    listed groups end as the saved state plus the last commands, the others as everything in order"""
    import torch
    from summerset_amd import StringKvSnapshot, StringKvStateMachine
    rng = np.random.default_rng(139)
    pool = _pool(rng, 10)
    model = _rng_dicts(rng, G, pool, 6)
    a = fill(StringKvStateMachine(G, 16, 2048), dev, model)
    lst = rng.permutation(G)[:k]
    snap = StringKvSnapshot(a, k)
    mk = lambda: [[("put", pool[int(rng.integers(len(pool)))], rng.integers(0, 256, int(rng.integers(1, 20)), dtype=np.uint8).tobytes()) if rng.random() < 0.7  # noqa: E731
                   else ("get", pool[int(rng.integers(len(pool)))]) for _ in range(G)] for _ in range(3)]
    c1, c2 = mk(), mk()
    side = None if str(dev) == "cpu" else torch.cuda.Stream()    # one non-default stream (the emulator has the null stream alone)
    stream = None if side is None else side.cuda_stream
    if side is not None:
        torch.cuda.synchronize()
    with (torch.cuda.stream(side) if side is not None else contextlib.nullcontext()):
        a.save_groups(lst, snap, stream=stream)
        r1 = submit(a, dev, c1, stream=stream)
        a.load_groups(snap, lst, stream=stream)
        r2 = submit(a, dev, c2, stream=stream)
    if side is not None:
        side.synchronize()
    assert snap.items() == [model[g] for g in lst]               # the image is the state at the save point
    saved = {int(g): dict(model[g]) for g in lst}
    want1 = apply(model, c1)
    got1 = collect(a, r1, values=False)                          # (off, len) of the listed groups' results are no longer valid: lengths only
    for i in range(3):
        assert [None if w is None else len(w) for w in want1[i]] == got1[i], i
    for g, d in saved.items():
        model[g] = d
    assert collect(a, r2) == apply(model, c2)
    gets_equal(a, dev, model, "at the end")
    _close([a, snap])


# ---- 13: the token table ------------------------------------------------------------------------------------------------------
def _kv_exec(t, dev, kind, key, val):
    import torch
    f = lambda a, dt: torch.from_numpy(np.ascontiguousarray(a, dt)).to(dev)   # noqa: E731
    return t.execute(f(kind, np.uint8), f(key, np.uint8), f(val, np.int32)).cpu().numpy().astype(np.uint32)


def _kv_step(t, dev, model, rng, rows=3):
    """random commands on the table and on the numpy model [K, G]; the results agree"""
    K, G = model.shape
    kind = rng.choice(np.array([GET, PUT, NOP], np.uint8), (rows, G), p=[0.3, 0.6, 0.1])
    key = rng.integers(0, K, (rows, G)).astype(np.uint8)
    val = rng.integers(1, 1 << 31, (rows, G)).astype(np.int32)
    got = _kv_exec(t, dev, kind, key, val)
    cols = np.arange(G)
    for i in range(rows):
        want = np.where(kind[i] <= 1, model[key[i], cols], 0)
        assert np.array_equal(got[i], want), i
        put = kind[i] == PUT
        model[key[i][put], cols[put]] = val[i][put].astype(np.uint32)


def token_table(dev, G=130, K=5):
    """identity over lists of 1, 63, 64, 65 and 130; a move between two tables with a position change against a numpy model; the
    export equals kv_model_image; neighbours untouched; reset equals create; the refusals, a different n_keys among them"""
    from summerset_amd import KvSnapshot, KvStateMachine, move_kv_groups
    rng = np.random.default_rng(149)
    a, b = KvStateMachine(G, K), KvStateMachine(G, K)
    ma, mb = np.zeros((K, G), np.uint32), np.zeros((K, G), np.uint32)
    for n in (None, 1, 63, 64, 65, 130):
        _kv_step(a, dev, ma, rng)
        if n is not None:
            _kv_step(b, dev, mb, rng)
        if n is None:
            snap = a.save_state()
            assert snap.export() == kv_model_image(ma) and np.array_equal(snap.table(), ma)
            b.load_state(snap)
            mb = ma.copy()
        else:
            lst = rng.permutation(G)[:n]
            snap = a.save_groups(lst)
            assert snap.export() == kv_model_image(ma[:, lst]) and snap.info() == dict(bytes=64 + _a8(4 * K * n), n_groups=n, n_keys=K)
            before = b.dump()
            b.load_groups(snap, lst)
            mb[:, lst] = ma[:, lst]
            after = b.dump()
            rest = np.setdiff1d(np.arange(G), lst)
            assert np.array_equal(after[:, rest], before[:, rest]) and np.array_equal(after, mb), n
        snap.close()
    # a move to other positions of a smaller table, and the source's groups as new
    c = KvStateMachine(77, K)
    mc = np.zeros((K, 77), np.uint32)
    _kv_step(c, dev, mc, rng)
    src, dst = rng.permutation(G)[:33], rng.permutation(77)[:33]
    before = a.dump()
    snap = move_kv_groups(a, src, c, dst)
    mc[:, dst] = ma[:, src]
    ma[:, src] = 0
    assert np.array_equal(c.dump(), mc) and np.array_equal(a.dump(), ma)
    assert np.array_equal(a.dump()[:, src], KvStateMachine(33, K).dump())          # reset is create
    rest = np.setdiff1d(np.arange(G), src)
    assert np.array_equal(a.dump()[:, rest], before[:, rest])
    _kv_step(a, dev, ma, rng); _kv_step(c, dev, mc, rng)
    whole = KvSnapshot(KvStateMachine(33, K))                     # a group image is the whole image of a 33-group table
    whole.import_(snap.export())
    d = KvStateMachine(33, K)
    d.load_state(whole)
    assert np.array_equal(d.dump(), snap.table())
    # refusals
    from summerset_amd import _lib
    from summerset_amd._lib import SMR_ERR_ARG as ARG, SMR_ERR_STATE as STATE
    img0, a0 = snap.export(), a.dump()
    L, null, sp = _lib.load(), C.c_void_p(None), C.c_void_p(0)
    gl = np.arange(33, dtype=np.uint32)
    glp = gl.ctypes.data_as(C.c_void_p)
    for call in (lambda: L.smr_kv_save_state(null, snap._h, sp), lambda: L.smr_kv_save_state(a._h, null, sp), lambda: L.smr_kv_load_state(null, snap._h, sp),
                 lambda: L.smr_kv_load_state(a._h, null, sp), lambda: L.smr_kv_save_groups(null, glp, 33, snap._h, sp),
                 lambda: L.smr_kv_save_groups(a._h, None, 33, snap._h, sp), lambda: L.smr_kv_save_groups(a._h, glp, 33, null, sp),
                 lambda: L.smr_kv_load_groups(null, snap._h, glp, 33, sp), lambda: L.smr_kv_load_groups(a._h, null, glp, 33, sp),
                 lambda: L.smr_kv_load_groups(a._h, snap._h, None, 33, sp), lambda: L.smr_kv_reset_groups(null, glp, 33, sp),
                 lambda: L.smr_kv_reset_groups(a._h, None, 33, sp), lambda: L.smr_kv_snapshot_create(null, C.byref(C.c_void_p())),
                 lambda: L.smr_kv_snapshot_create(a._h, None), lambda: L.smr_kv_snapshot_create_groups(null, 3, C.byref(C.c_void_p())),
                 lambda: L.smr_kv_snapshot_import(snap._h, None, 64), lambda: L.smr_kv_snapshot_import(null, img0, len(img0)),
                 lambda: L.smr_kv_snapshot_info_get(snap._h, None), lambda: L.smr_kv_snapshot_export(snap._h, None, 1 << 20)):
        _refused(lambda: _lib.check(int(call())), "null argument", ARG)
    assert snap.export() == img0 and np.array_equal(a.dump(), a0)
    for bad, word in (([], "a list of 0"), (list(range(G + 1)), "a list of"), ([0, G], "is group"), ([4, 5, 4], "listed twice")):
        _refused(lambda: a.reset_groups(bad), word, ARG)
        if 0 < len(bad) <= G:
            s = KvSnapshot(a, len(bad))
            _refused(lambda: a.save_groups(bad, s), word, ARG)
    _refused(lambda: a.save_groups(np.arange(34), snap), "made for", ARG)
    _refused(lambda: a.load_groups(snap, np.arange(32)), "made for", ARG)
    _refused(lambda: a.load_groups(KvSnapshot(a, 33), np.arange(33)), "nothing saved", STATE)
    other = KvStateMachine(G, K + 1)                              # a different n_keys
    o0 = other.dump()
    _refused(lambda: other.load_groups(snap, np.arange(33)), "another n_keys", ARG)
    _refused(lambda: other.save_groups(np.arange(33), snap), "another n_keys", ARG)
    _refused(lambda: KvSnapshot(other, 33).import_(img0), "another n_groups / n_keys", ARG)
    _refused(lambda: a.load_state(snap), "made for another", ARG)
    for bad, word in ((img0[:-1], "truncated"), (img0[:30], "shorter than its header"), (struct.pack("<I", KV_MAGIC ^ 1) + img0[4:], "magic"),
                      (img0[:4] + struct.pack("<I", 2) + img0[8:], "version"), (_poke(img0, len(img0) - 1, 1), "padding is not zero")):
        assert (4 * K * 33) % 8 == 4
        _refused(lambda: snap.import_(bad), word, ARG)
        assert snap.export() == img0
    assert np.array_equal(a.dump(), a0) and np.array_equal(other.dump(), o0)
    _close([a, b, c, d, other, snap, whole])
