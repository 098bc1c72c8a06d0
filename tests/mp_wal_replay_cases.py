"""A MultiPaxos cluster's state rebuilt from its WAL bytes (smr_mp_snapshot_from_wal, `MpSnapshot.from_wal`,
`MultiPaxosCluster.recover_from_wal`): the bodies of tests/test_mp_wal_replay.py (emulator, dev = "cpu", inside hostsim.red_zones)
and tests/test_zzzz_mp_wal_replay_gpu.py (device).

The expected state comes from `Replica`, a literal restatement of `recover_apply_entry` (multipaxos/recovery.rs:10-116, release
build) fed by `wire.wal_decode` run sequentially over each log (`expect_log`: storage.rs:240-267's end of log, and where the C-ABI
says a log stops).  It is test infrastructure and never the code under test.

Shapes: G = 130 (two full tiles and a partial one), R = 5, W in {16, 64}, 0 to 40 entries per log."""
import numpy as np

NO_REP = 0xFF
NULL, PREPARING, ACCEPTING, COMMITTED, EXECUTED = range(5)            # Status, mod.rs:168-174
ST_OK, ST_MALFORMED, ST_ORDER, ST_TOKEN, ST_RANGE = range(5)          # SMR_WAL_ST_*
G0, R0 = 130, 5
LEAD = 32                                                             # bytes (tokens: words / 4) of poisoned room around the inputs


# ---- the restatement -------------------------------------------------------------------------------------------------------
class Replica:
    """what recover_from_snapshot leaves (snapshot.rs:212-216) and recover_apply_entry (recovery.rs:10-116) makes of it"""

    def __init__(self, s0=0):
        self.start_slot = self.accept_bar = self.commit_bar = self.exec_bar = self.snap_bar = s0       # snapshot.rs:212-216
        self.insts = []
        self.bal_prep_sent = self.bal_prepared = self.bal_max_seen = 0
        self.voted_differs = 0                                        # (coverage: slots whose voted != (bal, reqs) at some point)

    @staticmethod
    def null_instance():
        return dict(bal=0, status=NULL, reqs=0, voted=(0, 0))         # mod.rs null_instance: no leader_bk / replica_bk, not external

    def _pad(self, slot):
        while self.start_slot + len(self.insts) <= slot:              # recovery.rs:20-22, 42-44
            self.insts.append(self.null_instance())

    def prepare_bal(self, slot, ballot):
        if slot < self.start_slot:                                    # :16-18
            return False
        self._pad(slot)
        inst = self.insts[slot - self.start_slot]                     # :24
        inst["bal"] = ballot                                          # :25
        inst["status"] = PREPARING                                    # :26
        if inst["voted"] != (0, 0) and inst["voted"] != (inst["bal"], inst["reqs"]):
            self.voted_differs += 1
        self.bal_prep_sent = max(self.bal_prep_sent, ballot)          # :28-30
        self.bal_max_seen = max(self.bal_max_seen, ballot)            # :31-33
        self.bal_prepared = 0                                         # :34
        return True

    def accept_data(self, slot, ballot, reqs):
        if slot < self.start_slot:                                    # :38-40
            return False
        self._pad(slot)
        inst = self.insts[slot - self.start_slot]                     # :46
        inst["bal"] = ballot                                          # :47
        inst["status"] = ACCEPTING                                    # :48
        inst["reqs"] = reqs                                           # :49
        inst["voted"] = (ballot, reqs)                                # :51
        self.bal_prep_sent = max(self.bal_prep_sent, ballot)          # :54-56
        self.bal_prepared = max(self.bal_prepared, ballot)            # :58-60
        self.bal_max_seen = max(self.bal_max_seen, ballot)            # :61-63
        if slot == self.accept_bar:                                   # :66-75
            while self.accept_bar < self.start_slot + len(self.insts):
                if self.insts[self.accept_bar - self.start_slot]["status"] < ACCEPTING:
                    break
                self.accept_bar += 1
        return True

    def commit_slot(self, slot):
        if slot < self.start_slot:                                    # :79-81
            return False
        self.insts[slot - self.start_slot]["status"] = COMMITTED      # :84 (the debug_assert of :82 is not in a release build)
        if slot == self.commit_bar:                                   # :87-111
            while self.commit_bar < self.accept_bar:
                inst = self.insts[self.commit_bar - self.start_slot]
                if inst["status"] < COMMITTED:
                    break
                self.commit_bar += 1                                  # :107
                self.exec_bar += 1                                    # :108
                inst["status"] = EXECUTED                             # :109
        return True

    def log_len(self):
        return self.start_slot + len(self.insts)


def expect_log(log, toks, s0, max_span):
    """one log, sequentially: (Replica, consumed, status, applied, ignored, cut tail)"""
    from summerset_amd import SummersetError, wire
    ref, p, k, applied, ignored = Replica(s0), 0, 0, 0, 0
    while True:
        try:
            n, e = wire.wal_decode(log[p:])
        except SummersetError:
            return ref, p, ST_MALFORMED, applied, ignored, 0
        if n == 0:                                                    # storage.rs:245-267: the final Truncate goes to p
            return ref, p, ST_OK, applied, ignored, int(p < len(log))
        kind, slot, tok = e["kind"], e["slot"], 0
        if kind == wire.WAL_ACCEPT_DATA:
            nonempty = e["reqs"][0] != 0                              # the Vec's length varint
            if k >= len(toks) or (toks[k] != 0) != nonempty:
                return ref, p, ST_TOKEN, applied, ignored, 0
            tok, k = toks[k], k + 1
        if slot < s0:
            ignored += 1
        else:
            if kind == wire.WAL_COMMIT_SLOT:
                if slot >= ref.log_len():                             # recovery.rs:84 indexes out of range
                    return ref, p, ST_ORDER, applied, ignored, 0
                ref.commit_slot(slot)
            else:
                if slot + 1 >= 1 << 32 or slot - s0 >= max_span:
                    return ref, p, ST_RANGE, applied, ignored, 0
                ref.prepare_bal(slot, e["ballot"]) if kind == wire.WAL_PREPARE_BAL else ref.accept_data(slot, e["ballot"], tok)
            applied += 1
        p += n


def expected_dumps(refs, G, R, W, n_live=None):
    """the restatement's replicas as smr_mp_dump's arrays (slot arrays [W][G] at slot % W, zero outside the log); n_live: of the
    first n_live logs-per-group only (the i-th live replica's, in order)"""
    from summerset_amd import _lib
    from summerset_amd.multipaxos import _DUMP_T
    out = []
    for r in range(R if n_live is None else n_live):
        d = {}
        for name in _lib.MP_DUMP_FIELDS:
            shape = (R, G) if name == "peer_exec_bar" else ((W, G) if name.startswith("s_") else (G,))
            d[name] = np.zeros(shape, _DUMP_T.get(name, np.uint32))
        d["leader"][:] = NO_REP
        for g in range(G):
            x = refs[r * G + g]
            d["bal_prep_sent"][g], d["bal_prepared"][g], d["bal_max_seen"][g] = x.bal_prep_sent, x.bal_prepared, x.bal_max_seen
            d["start_slot"][g], d["log_len"][g], d["accept_bar"][g] = x.start_slot, x.log_len(), x.accept_bar
            d["commit_bar"][g], d["exec_bar"][g], d["snap_bar"][g] = x.commit_bar, x.exec_bar, x.snap_bar
            for k, inst in enumerate(x.insts):
                w = (x.start_slot + k) % W
                d["s_bal"][w, g], d["s_status"][w, g], d["s_reqs"][w, g] = inst["bal"], inst["status"], inst["reqs"]
                d["s_vbal"][w, g], d["s_vreqs"][w, g] = inst["voted"]
        out.append(d)
    return out


# ---- logs ------------------------------------------------------------------------------------------------------------------
def _reqs(tok, big=False):
    """some ReqBatch bytes for a token: 0 = the empty batch; big: a 4 KiB value"""
    from summerset_amd import wire
    if tok == 0:
        return wire.reqbatch([])
    return wire.reqbatch([(tok & 0xFF, tok, ("put", "k%d" % (tok % 7), "v" * (4096 if big else 16)))])


def frames(entries):
    """[("P", slot, ballot) | ("A", slot, ballot, token[, big]) | ("C", slot)] -> (the log's bytes, its journal)"""
    from summerset_amd import wire
    out, toks = [], []
    for e in entries:
        if e[0] == "P":
            out.append(wire.wal_prepare_bal(e[1], e[2]))
        elif e[0] == "A":
            out.append(wire.wal_accept_data(e[1], e[2], _reqs(e[3], len(e) > 4 and e[4])))
            toks.append(e[3])
        else:
            out.append(wire.wal_commit_slot(e[1]))
    return b"".join(out), toks


def random_valid_log(rng, s0, span, n):
    """what one replica of a group writes, as leader or follower: Prepare rounds at rising ballots over the slots that are not
    committed yet, Accepts out of order, re-Accepts at higher ballots over voted slots, commits behind them"""
    ref, ents, bal = Replica(s0), [], 0
    step = [1, 200, 1 << 16, 1 << 33][int(rng.integers(0, 4))]
    for _ in range(n):
        c, hi = rng.random(), min(ref.log_len() + 2, s0 + span)
        open_ = [s for s in range(ref.commit_bar, hi) if s >= ref.log_len() or ref.insts[s - s0]["status"] < COMMITTED]
        ready = [s for s in range(ref.commit_bar, ref.accept_bar) if ref.insts[s - s0]["status"] == ACCEPTING]
        if c < 0.25 and ready:
            s = ready[0] if rng.random() < 0.6 else ready[int(rng.integers(0, len(ready)))]
            ents.append(("C", s)); ref.commit_slot(s)
        elif c < 0.4 and open_:
            bal += int(rng.integers(1, 4)) * step
            s = open_[int(rng.integers(0, len(open_)))]
            ents.append(("P", s, bal)); ref.prepare_bal(s, bal)
        elif open_:
            if bal == 0 or rng.random() < 0.1:
                bal += step
            s = open_[int(rng.integers(0, min(len(open_), 4)))]
            tok = 0 if rng.random() < 0.1 else int(rng.integers(1, 1 << 32))
            ents.append(("A", s, bal, tok)); ref.accept_data(s, bal, tok)
    return ents, ref


def random_valid_logs(rng, G, R, span, s0=None):
    logs, toks, differs = [], [], 0
    for l in range(G * R):
        ents, ref = random_valid_log(rng, 0 if s0 is None else int(s0[l]), span, int(rng.integers(0, 41)))
        differs += ref.voted_differs
        b, t = frames(ents)
        logs.append(b); toks.append(t)
    return logs, toks, differs


# ---- running the call --------------------------------------------------------------------------------------------------------
class _NoZones:
    count, first = 0, ""

    def __enter__(self):
        return self

    def __exit__(self, *a):
        return False


def from_wal(dev, like, logs, toks, s0=None, n_groups=None, max_span=None, zones=None, lead=LEAD):
    """`MpSnapshot.from_wal` over inputs that sit in the middle of larger buffers (`lead` bytes of 0xAB in front and behind);
    zones: hostsim.red_zones, which poisons that room for the kernels -- the device simply never reads it"""
    import torch
    from summerset_amd import MpSnapshot
    raw = b"".join(logs)
    buf = np.full(len(raw) + 2 * lead, 0xAB, np.uint8)
    buf[lead:lead + len(raw)] = np.frombuffer(raw, np.uint8)
    off = lead + np.concatenate([[0], np.cumsum([len(b) for b in logs])]).astype(np.int64)
    flat = np.asarray([x for t in toks for x in t], dtype=np.int64)
    tk = np.full(len(flat) + 2 * (lead // 4), 0xABABABAB, np.uint32)
    tk[lead // 4:lead // 4 + len(flat)] = flat.astype(np.uint32)
    toff = lead // 4 + np.concatenate([[0], np.cumsum([len(t) for t in toks])]).astype(np.int64)
    tb, tt = torch.from_numpy(buf).to(dev), torch.from_numpy(tk.view(np.int32)).to(dev)
    ctx = _NoZones() if zones is None else zones(tb, lead, lead + len(raw), (tt, lead, lead + 4 * len(flat)))
    with ctx as hits:
        # (the tuple form's length is the whole tensor: the logs' own offsets are what bounds the walk)
        snap, consumed, status, counts = MpSnapshot.from_wal(like, (tb, torch.from_numpy(off).to(dev)), (tt, torch.from_numpy(toff).to(dev)),
                                                             s0, n_groups, max_span, device=dev)
        info = snap.info()                                            # (synchronises)
    assert hits.count == 0, "the walk left its logs: " + hits.first
    return snap, consumed.cpu().numpy(), status.cpu().numpy(), counts.cpu().numpy(), info


def _cluster(G, R, W, **kw):
    from summerset_amd import MultiPaxosCluster
    return MultiPaxosCluster(G, R, W, outbox_cap=W + 4, **kw)


def _same_dumps(eng, want, what):
    for r, x in enumerate(want):
        a = eng.dump(r)
        for n in x:
            if not np.array_equal(a[n], x[n]):
                bad = np.argwhere(a[n] != x[n])[:4]
                raise AssertionError("%s rep %d: %s differs at %s: %s, expected %s" % (what, r, n, bad.tolist(), a[n][tuple(bad.T)], x[n][tuple(bad.T)]))


def check_against_model(dev, logs, toks, what, G=G0, R=R0, W=16, s0=None, max_span=None, zones=None, expect_status=None):
    """the call against the restatement: consumed, status, counts, info, and the dump of a fresh cluster loaded from the image"""
    span = W if max_span is None else max_span
    exp = [expect_log(logs[l], toks[l], 0 if s0 is None else int(s0[l]), span) for l in range(G * R)]
    like = _cluster(G, R, W)
    snap, consumed, status, counts, info = from_wal(dev, like, logs, toks, s0, None, max_span, zones)
    assert np.array_equal(consumed, [e[1] for e in exp]), what + ": consumed"
    assert np.array_equal(status, [e[2] for e in exp]), what + ": status"
    if expect_status is not None:
        assert {l: int(s) for l, s in enumerate(status) if s} == expect_status, what + ": which logs stopped, and why"
    assert counts.tolist() == [sum(e[3] for e in exp), sum(e[4] for e in exp), sum(e[2] != 0 for e in exp), sum(e[5] for e in exp)], what + ": counts"
    refs = [e[0] for e in exp]
    assert info["n_slots"] == sum(len(x.insts) for x in refs) and info["max_live"] == max(len(x.insts) for x in refs), what + ": info"
    assert info["n_outbox"] == 0 and info["max_outbox"] == 0 and info["n_groups"] == G and info["population"] == R
    like.load_state(snap)
    _same_dumps(like, expected_dumps(refs, G, R, W), what)
    for r in range(R):
        assert like.counters(r) == {"commits": 0, "redirects": 0, "rejects": 0}
    return snap, like, refs, (consumed, status, counts)


def symbols(lib):
    from summerset_amd import _lib
    names = {n for n, _, _ in _lib.SYMBOLS}
    for n in ("smr_mp_snapshot_from_wal", "smr_wal_decode"):
        assert n in names and getattr(lib, n)


# ---- 1. random valid logs ----------------------------------------------------------------------------------------------------
def random_logs(dev, W, zones=None, seed=11):
    rng = np.random.default_rng(seed + W)
    s0 = np.where(rng.random(G0 * R0) < 0.3, rng.integers(1, 5000, G0 * R0), 0)
    logs, toks, differs = random_valid_logs(rng, G0, R0, 16, s0)
    assert differs > 0, "no slot whose voted != (bal, reqs): the generator lost its re-Prepare over a voted slot"
    assert any(len(b) == 0 for b in logs) and max(len(t) for t in toks) > 8
    _, _, refs, _ = check_against_model(dev, logs, toks, "random valid logs, W = %d" % W, W=W, s0=s0, max_span=16, zones=zones)
    live = [x for x in refs if x.insts]
    assert any(i["voted"] != (i["bal"], i["reqs"]) and i["voted"] != (0, 0) for x in live for i in x.insts), "voted != (bal, reqs) in the final state"
    assert any(x.accept_bar < x.log_len() for x in live) and any(x.exec_bar > x.start_slot for x in live)


# ---- 2. canonical bytes --------------------------------------------------------------------------------------------------------
def canonical_bytes(dev, zones=None, seed=5):
    rng = np.random.default_rng(seed)
    logs, toks, _ = random_valid_logs(rng, G0, R0, 16)
    images = []
    for W in (16, 64):
        eng = _cluster(G0, R0, W)
        snap, _, status, _, _ = from_wal(dev, eng, logs, toks, max_span=16, zones=zones)
        assert not status.any()
        img = snap.export()
        eng.load_state(snap)
        assert eng.save_state().export() == img, "W = %d: export(from_wal) != export(save_state(load_state(from_wal)))" % W
        images.append(img)
    assert images[0] == images[1], "the same logs through W = 16 and W = 64 clusters export different bytes"


# ---- 3. order-dependent bars -----------------------------------------------------------------------------------------------
def order_cases():
    """(name, entries, start_slot, what the restatement must show: accept_bar, commit_bar, statuses)"""
    return [
        ("accept 1 then 0", [("A", 1, 5, 11), ("A", 0, 5, 10)], 0, (2, 0, [ACCEPTING, ACCEPTING])),
        ("a PrepareBal in the gap", [("A", 0, 5, 10), ("P", 1, 5), ("A", 2, 5, 12)], 0, (1, 0, [ACCEPTING, PREPARING, ACCEPTING])),
        ("the gap closes later", [("A", 0, 5, 10), ("A", 2, 5, 12), ("P", 1, 6), ("A", 1, 6, 11)], 0, (3, 0, [ACCEPTING] * 3)),
        ("commit ahead, then the release", [("A", 0, 5, 10), ("A", 1, 5, 11), ("A", 2, 5, 12), ("C", 1), ("C", 2), ("C", 0)], 0,
         (3, 3, [EXECUTED] * 3)),
        ("commit not below accept_bar", [("A", 0, 5, 10), ("P", 1, 5), ("A", 2, 5, 12), ("C", 2), ("C", 0)], 0,
         (1, 1, [EXECUTED, PREPARING, COMMITTED])),
        ("commit of a padded null", [("A", 3, 5, 13), ("C", 1)], 0, (0, 0, [NULL, COMMITTED, NULL, ACCEPTING])),
        ("PrepareBal over a Committed slot", [("A", 0, 5, 10), ("A", 1, 5, 11), ("C", 1), ("P", 1, 9), ("C", 0)], 0,
         (2, 1, [EXECUTED, PREPARING])),
        ("below start_slot", [("A", 3, 5, 13), ("P", 9, 7), ("C", 2), ("A", 10, 7, 20), ("A", 12, 7, 0), ("C", 10), ("A", 11, 7, 21)], 10,
         (13, 11, [EXECUTED, ACCEPTING, ACCEPTING])),
    ]


def order_dependent_bars(dev, zones=None):
    rng = np.random.default_rng(3)
    logs, toks, _ = random_valid_logs(rng, G0, R0, 16)
    s0 = np.zeros(G0 * R0, np.int64)
    where = {}
    for j, (name, ents, start, _) in enumerate(order_cases()):
        l = 37 + 61 * j                                               # spread over the tiles and replicas
        logs[l], toks[l] = frames(ents)
        s0[l], where[l] = start, name
    _, _, refs, (_, status, _) = check_against_model(dev, logs, toks, "order-dependent bars", s0=s0, zones=zones)
    assert not status.any()
    for (l, name), (_, _, _, (abar, cbar, sts)) in zip(sorted(where.items()), order_cases()):
        x = refs[l]
        assert (x.accept_bar, x.commit_bar, x.exec_bar, [i["status"] for i in x.insts]) == (abar, cbar, cbar, sts), name


# ---- 4. framing ----------------------------------------------------------------------------------------------------------------
def framing(dev, zones=None):
    from summerset_amd import wire
    logs, toks = [], []
    wide = [250, 251, 1 << 16, (1 << 16) - 1, 1 << 32, 1 << 63, (1 << 64) - 1]
    slots = [0, 7, 250, 251, 300]
    # the wider slots, applied: a log that starts just below a width's boundary runs across it.  3 -> 5 bytes at 2^16 (what every
    # cluster past 65 535 slots writes), 5-byte slots around 2^31, and the last slot the image can hold (log_len = 2^32 - 1);
    # 2^32 and 2^63 cannot be held and are `statuses`'
    far = {9: (1 << 16) - 5, 10: (1 << 31) - 3, 11: (1 << 32) - 14}
    s0 = np.zeros(G0 * R0, np.int64)
    for l in range(G0 * R0):
        k = l % 13
        if k in far:
            a = s0[l] = far[k] + (l // 13) % 3
            a = int(a)
            ents = [("A", 250, 9, 1), ("P", a - 1, 9), ("C", 3),                          # below start_slot, in three widths
                    ("A", a + 1, 5, 21), ("A", a, 5, 20), ("C", a), ("P", a + 9, wide[l % len(wide)]), ("A", a + 6, 7, 26, l % 2 == 0),
                    ("A", a + 2, 5, 22), ("A", a + 3, 5, 0), ("C", a + 2), ("C", a + 1), ("A", a + 10, 1 << 33, 30), ("P", a + 4, 300)]
            assert a + 10 <= (1 << 32) - 2
            b, t = frames(ents)
            logs.append(b); toks.append(t)
        elif k == 0:
            logs.append(b""); toks.append([])                        # empty logs
        elif k == 1:                                                  # eleven bytes a frame: the next log starts at every offset mod 16
            b, t = frames([("P", 0, 1)] * (1 + l % 3))
            assert len(b) % 11 == 0
            logs.append(b); toks.append(t)
        elif k in (2, 3):                                             # every varint width, slot and ballot
            ents = []
            for j, s in enumerate(slots):
                ents += [("P", s, wide[(l + j) % len(wide)]), ("A", s, wide[(l + j + 1) % len(wide)], j + 1)]
            b, t = frames(ents)
            logs.append(b); toks.append(t)
        elif k == 4:                                                  # an empty reqs and a 4 KiB one
            b, t = frames([("A", 0, 3, 0), ("A", 1, 3, 77, True), ("A", 2, 3, 78), ("C", 0), ("C", 1)])
            assert len(b) > 4096
            logs.append(b); toks.append(t)
        elif k in (5, 6):                                             # a tail cut at each of 0..7 header bytes
            b, t = frames([("A", 0, 3, 5), ("C", 0), ("A", 1, 4, 6)])
            nxt = wire.wal_prepare_bal(2, 9)
            logs.append(b + nxt[:(l // 13) % 8]); toks.append(t)
        elif k == 7:                                                  # a tail cut inside a body (and the journal knows the frame)
            b, t = frames([("A", 0, 3, 5), ("A", 1, 3, 6)])
            cut = 9 + (l // 13) % (len(b) // 2 - 10)
            logs.append(b[:len(b) // 2 + cut]); toks.append(t)
        elif k == 8:                                                  # trailing bytes inside a frame
            out, t = [], [4]
            for f in (wire.wal_prepare_bal(0, 2), wire.wal_accept_data(0, 2, _reqs(4)), wire.wal_commit_slot(0)):
                body = f[8:] + b"\xfe\xff\x00junk"[:1 + l % 7]
                out.append(len(body).to_bytes(8, "big") + body)
            logs.append(b"".join(out)); toks.append(t)
        else:
            b, t = frames([("A", 0, 1, 9), ("A", 1, 1, 10), ("C", 0)][:k - 8])
            logs.append(b); toks.append(t)
    offs = np.concatenate([[0], np.cumsum([len(b) for b in logs])])[:-1]
    assert {int(o) % 16 for o, b in zip(offs, logs) if b} == set(range(16)), "logs that start at every offset mod 16"
    _, _, refs, (consumed, status, counts) = check_against_model(dev, logs, toks, "framing", W=512, s0=s0, zones=zones)
    assert not status.any()
    for l in (9, 10, 11, 9 + 13, 11 + 26):                            # (what the model made of them: the test's own footing)
        x, a = refs[l], int(s0[l])
        assert (x.start_slot, x.log_len(), x.accept_bar, x.commit_bar, x.exec_bar) == (a, a + 11, a + 4, a + 3, a + 3), l
        assert [i["status"] for i in x.insts] == [EXECUTED] * 3 + [ACCEPTING, PREPARING, NULL, ACCEPTING, NULL, NULL, PREPARING, ACCEPTING], l
    assert max(x.log_len() for x in refs) == (1 << 32) - 1 and counts[1] == 3 * sum(l % 13 in far for l in range(G0 * R0))
    cut = [l for l in range(G0 * R0) if l % 13 in (5, 6, 7) and not (l % 13 != 7 and (l // 13) % 8 == 0)]
    assert counts[3] == len(cut) and all(consumed[l] < len(logs[l]) for l in cut)
    assert refs[2].insts[300]["bal"] in wide and refs[4].insts[1]["reqs"] == 77


# ---- 5. statuses -----------------------------------------------------------------------------------------------------------------
def statuses(dev, zones=None):
    from summerset_amd import wire
    rng = np.random.default_rng(8)
    logs, toks, _ = random_valid_logs(rng, G0, R0, 16)
    head = [("A", 0, 3, 5), ("A", 1, 3, 6), ("C", 0)]
    hb, ht = frames(head)
    tail = wire.wal_accept_data(2, 3, _reqs(7))                      # what would follow, were the log not stopped
    bad = {
        40: (hb + (10 ** 12 + 1).to_bytes(8, "big") + b"\x00" * 5 + tail, ht + [7], ST_MALFORMED),
        41: (hb + (3).to_bytes(8, "big") + b"\x03\x00\x00" + tail, ht + [7], ST_MALFORMED),           # an unknown variant
        170: (hb + (2).to_bytes(8, "big") + b"\x00\xfb" + tail, ht + [7], ST_MALFORMED),              # a slot that does not parse in the frame
        171: (hb + (0).to_bytes(8, "big") + tail, ht + [7], ST_MALFORMED),                            # an empty frame
        300: (hb + wire.wal_commit_slot(2) + tail, ht + [7], ST_ORDER),                               # CommitSlot beyond the log
        301: (hb + wire.wal_commit_slot(1 << 40) + tail, ht + [7], ST_ORDER),
        430: (hb + tail + tail, ht + [7], ST_TOKEN),                                                  # a short journal
        431: (hb + tail, ht + [0], ST_TOKEN),                                                         # a zero token, a non-empty batch
        432: (hb + wire.wal_accept_data(2, 3, _reqs(0)) + tail, ht + [9, 7], ST_TOKEN),               # a token, an empty batch
        560: (hb + wire.wal_prepare_bal(1 << 32, 3) + tail, ht + [7], ST_RANGE),                      # a slot >= 2^32
        561: (hb + wire.wal_accept_data((1 << 32) - 1, 3, _reqs(7)) + tail, ht + [7, 7], ST_RANGE),   # log_len would not fit
        562: (hb + wire.wal_accept_data(16, 3, _reqs(7)) + tail, ht + [7, 7], ST_RANGE),              # a span >= max_span
        649: (hb + wire.wal_prepare_bal(16, 3), ht, ST_RANGE),
    }
    for l, (b, t, _) in bad.items():
        logs[l], toks[l] = b, t
    want = {l: st for l, (_, _, st) in bad.items()}
    _, _, refs, (consumed, status, counts) = check_against_model(dev, logs, toks, "statuses", zones=zones, expect_status=want)
    for l, (b, _, st) in bad.items():                                 # stopped in front of the frame, the prefix kept
        where = len(hb) + (len(tail) if l == 430 else 0)
        x = refs[l]
        assert consumed[l] == where, (l, st)
        assert (x.accept_bar, x.commit_bar, x.log_len()) == ((3, 1, 3) if l == 430 else (2, 1, 2)), (l, st)
    assert counts[2] == len(bad)


def refusals(dev, zones=None):
    """refused arguments leave the snapshot's bytes unchanged (zones: nothing outside the logs and the journal is read on the way
    to a refusal either)"""
    import ctypes as C

    import torch
    from summerset_amd import SummersetError, _lib
    from summerset_amd._lib import stream_ptr
    rng = np.random.default_rng(2)
    G, R, W = 70, 3, 16
    logs, toks, _ = random_valid_logs(rng, G, R, 16)
    eng = _cluster(G, R, W)
    snap, _, _, _, _ = from_wal(dev, eng, logs, toks, zones=zones)
    before = snap.export()
    n = G * R
    raw = b"".join(logs)
    flat = np.asarray([x for t in toks for x in t], dtype=np.int64).astype(np.uint32)
    # the buffer the call is told about is `whole`'s first len(raw) bytes; LEAD more bytes (tokens: LEAD // 4 more) lie behind
    whole = torch.from_numpy(np.concatenate([np.frombuffer(raw, np.uint8), np.full(LEAD, 0xAB, np.uint8)])).to(dev)
    wtok = torch.from_numpy(np.concatenate([flat, np.full(LEAD // 4, 0xABABABAB, np.uint32)]).view(np.int32)).to(dev)
    buf, tok = whole, wtok
    off = np.concatenate([[0], np.cumsum([len(b) for b in logs])]).astype(np.int64)
    toff = np.concatenate([[0], np.cumsum([len(t) for t in toks])]).astype(np.int64)
    consumed = torch.full((n,), -7, dtype=torch.int64, device=dev)
    status = torch.full((n,), -7, dtype=torch.int32, device=dev)
    counts = torch.full((4,), -7, dtype=torch.int64, device=dev)

    def call(o=off, to=toff, blen=len(raw), span=W, b=buf, outs=None, t=tok):
        od, td = torch.from_numpy(np.ascontiguousarray(o)).to(dev), torch.from_numpy(np.ascontiguousarray(to)).to(dev)
        c, s, k = outs if outs is not None else (consumed, status, counts)
        p = lambda x: None if x is None else x.data_ptr()
        return _lib.load().smr_mp_snapshot_from_wal(snap._h, p(b), blen, od.data_ptr(), p(t), td.data_ptr(), None, span, p(c), p(s), p(k),
                                                    stream_ptr(None))
    desc, tdesc = off.copy(), toff.copy()
    desc[5], tdesc[9] = desc[6] + 1, tdesc[10] + 1
    past = off.copy()
    past[-1] += 1
    from summerset_amd import MpSnapshot
    with (_NoZones() if zones is None else zones(whole, 0, len(raw), (wtok, 0, 4 * len(flat)))) as hits:
        for what, kw in [("descending offsets", dict(o=desc)), ("descending journal offsets", dict(to=tdesc)), ("an offset past buf_len", dict(o=past)),
                         ("buf_len short of the last offset", dict(blen=len(raw) - 1)), ("max_span 0", dict(span=0)), ("max_span above the room", dict(span=W + 1)),
                         ("null buffer", dict(b=None)), ("null consumed", dict(outs=(None, status, counts))), ("null status", dict(outs=(consumed, None, counts))),
                         ("null counts", dict(outs=(consumed, status, None))), ("null journal", dict(t=None))]:
            assert call(**kw) == _lib.SMR_ERR_ARG, what
            assert snap.export() == before, what + ": the snapshot changed"
            assert (consumed.cpu().numpy() == -7).all() and (status.cpu().numpy() == -7).all() and (counts.cpu().numpy() == -7).all(), what
        # the wrapper's own check: one log per (live replica, group), neither fewer nor -- which the library would read past the offsets for -- more
        for k in (n - 1, n - G, n + G):
            try:
                MpSnapshot.from_wal(eng, (logs + logs)[:k], (toks + toks)[:k], device=dev)
                raise AssertionError("%d logs were taken for %d" % (k, n))
            except ValueError:
                pass
        assert call() == 0 and snap.export() == before               # and the same call with nothing wrong goes through
    assert hits.count == 0, "a refused or a good call left its logs: " + hits.first
    eng.load_state(snap)


# ---- 6. listed groups ------------------------------------------------------------------------------------------------------------
def listed_groups(dev, zones=None):
    """create_groups(n = 7) + from_wal + load_groups into a running cluster"""
    rng = np.random.default_rng(21)
    G, R, W, n = G0, R0, 16, 7
    eng = _cluster(G, R, W)
    eng.preset_leader(1)
    import torch
    for t in range(6):                                                # a running cluster: a few ticks of client batches
        cnt = (rng.random(G) < 0.8).astype(np.uint32)
        val = rng.integers(1, 1 << 31, (1, G)).astype(np.uint32)
        eng.tick(req_target=torch.ones(G, dtype=torch.uint8, device=dev), req_cnt=torch.from_numpy(cnt.view(np.int32)).to(dev).view(torch.int32),
                 req_val=torch.from_numpy(val.view(np.int32)).to(dev), heartbeat=t % 3 == 2)
    before = [eng.dump(r) for r in range(R)]
    assert before[1]["log_len"].max() > 0
    groups = [129, 0, 64, 63, 5, 100, 77]
    s0 = rng.integers(0, 100, n * R)
    logs, toks, _ = random_valid_logs(rng, n, R, 16, s0)
    exp = [expect_log(logs[l], toks[l], int(s0[l]), W) for l in range(n * R)]
    snap, consumed, status, counts, info = from_wal(dev, eng, logs, toks, s0, n_groups=n, zones=zones)
    assert info["n_groups"] == n and not status.any() and np.array_equal(consumed, [e[1] for e in exp])
    eng.load_groups(snap, groups)
    want = expected_dumps([e[0] for e in exp], n, R, W)
    rest = np.setdiff1d(np.arange(G), groups)
    for r in range(R):
        a = eng.dump(r)
        for name in a:
            assert np.array_equal(a[name][..., groups], want[r][name]), "rep %d: %s of the recovered groups" % (r, name)
            assert np.array_equal(a[name][..., rest], before[r][name][..., rest]), "rep %d: %s of another group changed" % (r, name)
    # ... and through the one call
    eng2 = _cluster(G, R, W)
    eng2.recover_from_wal(logs, toks, s0, groups=groups, device=dev)
    for r in range(R):
        a = eng2.dump(r)
        for name in a:
            assert np.array_equal(a[name][..., groups], want[r][name])


# ---- 7. the recovered cluster goes on ----------------------------------------------------------------------------------------------
def coherent_cluster_logs(rng, G, R):
    """per group the logs of R replicas of ONE history: ballot b1's leader got tokens t[s] accepted on prefixes of different
    lengths, the common prefix K committed on all of them (the engine has no catch-up: a replica that recovers BEHIND the new
    leader's commit_bar -- holes, or slots still Accepting at the old ballot -- stays behind, as it does in a cluster that got
    there by running); then (half of the groups) ballot b2's quorum prepared and accepted the slots from K on -- a slot none of
    them had voted for with a NEW token, which is then the token of the highest ballot"""
    logs, toks, final = [None] * (G * R), [None] * (G * R), []
    for g in range(G):
        n = int(rng.integers(1, 9))
        b1, b2 = 256 + int(rng.integers(0, R)), 512 + int(rng.integers(0, R))
        t = [1000 + 16 * g + s for s in range(n)]
        K = int(rng.integers(0, n + 1))
        # What Paxos promises of a slot that is not committed yet is the value of the highest ballot any quorum can see: a vote
        # held by fewer than R - quorum + 1 replicas may or may not survive, depending on whose replies the next leader hears
        # first (the reference's too).  So every slot here ends with its highest-ballot vote on a majority: b1's prefix of m slots
        # on three replicas at least, and the one or two longer prefixes only where b2's quorum then votes over them
        m, second, quorum = int(rng.integers(K, n + 1)), rng.random() < 0.5, R // 2 + 1
        longer = [int(x) for x in rng.integers(m, n + 1, R - quorum)] if second else [m] * (R - quorum)
        a = sorted(longer + [m] + [int(x) for x in rng.integers(K, m + 1, quorum - 1)], reverse=True)
        order = rng.permutation(R)
        acc = {int(order[i]): a[i] for i in range(R)}
        ents = {r: [("A", s, b1, t[s]) for s in range(acc[r])] for r in range(R)}
        for r in range(R):
            if acc[r] > 2 and rng.random() < 0.5:                     # Accepts out of order
                ents[r][0], ents[r][1] = ents[r][1], ents[r][0]
            at = int(rng.integers(K, acc[r] + 1))                     # the commits behind their Accepts, some Accepts behind the commits
            ents[r][at:at] = [("C", s) for s in (range(K) if rng.random() < 0.5 else reversed(range(K)))]
        top = {s: (b1, t[s]) for s in range(max(acc.values()))}
        if second:
            q2 =[int(x) for x in order[R - (R // 2 + 1):]]           # the quorum of b2: the replicas with the shortest prefixes
            for s in range(K, n):
                tok = t[s] if any(acc[r] > s for r in q2) else 5000 + 16 * g + s
                for r in q2:
                    if s == K:
                        ents[r].append(("P", s, b2))
                    ents[r].append(("A", s, b2, tok))
                top[s] = (b2, tok)
        for r in range(R):
            logs[r * G + g], toks[r * G + g] = frames(ents[r])
        final.append((K, top))
    return logs, toks, final


def goes_on(dev, W=16, seed=4, zones=None):
    import torch
    rng = np.random.default_rng(seed)
    G, R = G0, R0
    logs, toks, final = coherent_cluster_logs(rng, G, R)
    eng = _cluster(G, R, W)
    snap, _, status, _, _ = from_wal(dev, eng, logs, toks, zones=zones)
    assert not status.any()
    eng.load_state(snap)
    rec = [eng.dump(r) for r in range(R)]
    one_call = _cluster(G, R, W)                                      # the same through `recover_from_wal`
    assert not one_call.recover_from_wal(logs, toks, device=dev)[2].cpu().numpy().any()
    for r in range(R):
        d = one_call.dump(r)
        assert all(np.array_equal(d[k], rec[r][k]) for k in d), r
    assert any(b == 512 for _, top in final for b, _ in ((v[0] & ~0xFF, v[1]) for v in top.values())), "no group went through a second ballot"
    assert any(top[s][1] >= 5000 for _, top in final for s in top), "no slot whose highest ballot carries a new token"

    def bars_hold(ds, when):
        for r, d in enumerate(ds):
            assert (d["exec_bar"] <= d["commit_bar"]).all() and (d["commit_bar"] <= d["accept_bar"]).all() and \
                (d["accept_bar"] <= d["log_len"]).all(), "%s rep %d: exec_bar <= commit_bar <= accept_bar <= log_len" % (when, r)
            assert not d["overflow"].any()
    # what every replica has ever shown Committed or Executed, by slot (the heartbeat round trims executed slots off the ring:
    # a slot that left stays on record); a token, once committed, never changes.  Logs stay below W slots: no row is reused
    ctok = [np.full((W, G), -1, np.int64) for _ in range(R)]

    def note(ds, when):
        bars_hold(ds, when)
        for r, d in enumerate(ds):
            assert d["log_len"].max() <= W
            m = d["s_status"] >= COMMITTED
            known = m & (ctok[r] >= 0)
            assert (d["s_reqs"][known] == ctok[r][known]).all(), "%s rep %d: a committed slot changed its token" % (when, r)
            ctok[r][m] = d["s_reqs"][m]
            assert (d["start_slot"] <= d["exec_bar"]).all()
    note(rec, "recovered")
    # the replica that times out: per group one that has seen the group's highest ballot.  (A candidate whose new ballot is below
    # what a quorum has promised is refused, as in the reference, and would only try again at its next timeout.)
    who = np.argmax(np.stack([d["bal_max_seen"] for d in rec]), axis=0).astype(np.uint8)
    assert len(set(who.tolist())) >= 3
    t0 = dict(timeout_rep=torch.from_numpy(who).to(dev), timeout_src=torch.full((G,), NO_REP, dtype=torch.uint8, device=dev))
    prev = None
    for tick in range(24):                                            # one replica times out, then ticks until quiet
        eng.tick(heartbeat=tick % 2 == 1, **(t0 if tick == 0 else {}))
        now = [eng.dump(r) for r in range(R)]
        note(now, "tick %d" % tick)
        if prev is not None and tick % 2 == 0 and all(np.array_equal(now[r][k], prev[r][k]) for r in range(R) for k in now[r]):
            break
        if tick % 2 == 0:
            prev = now
    else:
        raise AssertionError("not quiet after 24 ticks")
    for g, (K, top) in enumerate(final):
        for r in range(R):                                            # the committed prefix and its tokens are unchanged on every replica
            c0 = int(rec[r]["commit_bar"][g])
            assert now[r]["commit_bar"][g] >= c0
            for s in range(c0):
                assert ctok[r][s, g] == rec[r]["s_reqs"][s, g] == top[s][1], (g, r, s)
        for s, (_, tok) in top.items():                               # every recovered Accepting slot: Committed on a quorum, the highest ballot's token
            held = [r for r in range(R) if ctok[r][s, g] == tok]
            assert len(held) >= R // 2 + 1, "group %d slot %d: token %d committed on %s" % (g, s, tok, held)
            assert all(ctok[r][s, g] in (-1, tok) for r in range(R)), "group %d slot %d: two tokens committed" % (g, s)


# ---- a live mask below the population ------------------------------------------------------------------------------------------
def live_subset(dev, zones=None, mask=0b10110):
    """a block of a spread cluster: replicas 1, 2 and 4 of 5 live.  Log i * G + j is the i-th LIVE replica's log of group j; the
    image's scalars, SnapRep and records are indexed the same way; replicas 0 and 3 are left as they were"""
    rng = np.random.default_rng(17)
    G, R, W = 70, 5, 16
    live = [r for r in range(R) if (mask >> r) & 1]
    L = len(live)
    s0 = np.where(rng.random(G * L) < 0.3, rng.integers(1, 70000, G * L), 0)
    logs, toks, _ = random_valid_logs(rng, G, L, 16, s0)
    exp = [expect_log(logs[l], toks[l], int(s0[l]), W) for l in range(G * L)]
    eng = _cluster(G, R, W)
    eng.set_live(mask)
    assert eng.live_mask() == mask
    before = [eng.dump(r) for r in range(R)]
    snap, consumed, status, counts, info = from_wal(dev, eng, logs, toks, s0, zones=zones)
    assert np.array_equal(consumed, [e[1] for e in exp]) and not status.any()
    assert counts.tolist() == [sum(e[3] for e in exp), sum(e[4] for e in exp), 0, 0]
    assert info["live_mask"] == mask and info["population"] == R and info["n_slots"] == sum(len(e[0].insts) for e in exp)
    for k in (G * R, G * (L - 1)):                                    # one log per LIVE replica and group, not per replica
        try:
            from_wal(dev, eng, (logs + logs)[:k], (toks + toks)[:k])
            raise AssertionError("%d logs were taken for %d live replicas x %d groups" % (k, L, G))
        except ValueError:
            pass
    eng.load_state(snap)
    want = expected_dumps([e[0] for e in exp], G, R, W, n_live=L)
    for r in range(R):
        a = eng.dump(r)
        x = want[live.index(r)] if r in live else before[r]
        for name in x:
            assert np.array_equal(a[name], x[name]), "rep %d (%s): %s" % (r, "live" if r in live else "not live", name)
    img = snap.export()
    assert eng.save_state().export() == img                           # and it is the image a save of that cluster writes


# ---- 8. offsets past 4 GiB (device only) ---------------------------------------------------------------------------------------------
def past_4gib(dev):
    """one buffer whose last logs lie past 4 GiB: a zero-filled allocation, a handful of short logs at the end"""
    import torch
    from summerset_amd import MpSnapshot
    G, R, W = 3, 3, 16
    n = G * R
    rng = np.random.default_rng(6)
    logs, toks, _ = random_valid_logs(rng, G, R, 16)
    logs = [b if b else frames([("A", 0, 1, 3)])[0] for b in logs]
    toks = [t if t else [3] for t in toks]
    base = (1 << 32) + 12345
    total = base + sum(len(b) for b in logs)
    buf = torch.zeros(total, dtype=torch.uint8, device=dev)
    buf[base:] = torch.from_numpy(np.frombuffer(b"".join(logs), np.uint8).copy()).to(dev)
    off = np.concatenate([[0], np.cumsum([len(b) for b in logs])]).astype(np.int64) + base
    off[:4] = [0, 0, 0, 7]                                            # logs 0, 1: empty; log 2: seven zero bytes, a cut tail; log 3: 4 GiB of zero-length frames
    toff = np.concatenate([[0], np.cumsum([len(t) for t in toks])]).astype(np.int64)
    tok = torch.from_numpy(np.asarray([x for t in toks for x in t], dtype=np.int64).astype(np.uint32).view(np.int32)).to(dev)
    eng = _cluster(G, R, W)
    snap, consumed, status, counts = MpSnapshot.from_wal(eng, (buf, torch.from_numpy(off).to(dev)), (tok, torch.from_numpy(toff).to(dev)), device=dev)
    consumed, status, counts = consumed.cpu().numpy(), status.cpu().numpy(), counts.cpu().numpy()
    del buf
    exp = [expect_log(logs[l], toks[l], 0, W) for l in range(n)]
    assert status[:4].tolist() == [0, 0, 0, ST_MALFORMED] and consumed[:4].tolist() == [0, 0, 0, 0]   # (an empty frame is no WalEntry)
    assert np.array_equal(consumed[4:], [e[1] for e in exp[4:]]) and not status[4:].any()
    assert counts.tolist() == [sum(e[3] for e in exp[4:]), 0, 1, 1]
    refs = [Replica(0)] * 4 + [e[0] for e in exp[4:]]
    eng.load_state(snap)
    _same_dumps(eng, expected_dumps(refs, G, R, W), "past 4 GiB")
