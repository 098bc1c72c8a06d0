"""The Reed-Solomon entry points (summerset_amd/csrc/rs_kernels.hip) over every kernel instance, erasure pattern size and shard
layout, bit for bit.  Device-agnostic bodies: tests/test_rs_bounds.py runs them on the emulator build (tests/hostsim) with red
zones around every buffer, tests/test_zzzz_rs_edges_gpu.py on the device.

Ground truth is never the code under test: parity is the CPU oracle's (`oracle.rs_encode`, pinned in tests/test_oracle_rs.py), a
rebuilt shard is the codeword's own bytes from before the erasure.  Every call works inside a larger buffer filled with 0xCD, at
least 64 bytes of it on either side, and the WHOLE buffer is compared afterwards: a byte written outside the shards a call owns
fails the case, and on the device a stray access still lands in the test's own allocation.

`zones(buf, lo, hi, *more)` is tests/hostsim's `red_zones` on the emulator -- the kernels may touch bytes [lo, hi) of `buf` and
nothing else of it, loads included -- and `no_zones` on the device, where a read cannot be observed."""
import contextlib
import itertools
import math

import numpy as np

FILL, ERASED, SLACK = 0xCD, 0xEE, 64

# RS_DISPATCH picks the kernel instance <NOUT, NIN> by n_out (shards to make: p for encode / verify, the erased ones for
# reconstruct) in 1..2 | 3..4 | 5..8 and n_in (= d) in 1..4 | 5..8 | 9..16; the LUT kernel by n_out alone.
#   scheme   n_in bucket     n_out of encode / verify   reconstruct reaches (erasing 1..p shards)
#   (1,1)    4  (low edge)   2 (low)                    <2,4>
#   (1,8)    4  (low)        8 (high)                   <2,4> <4,4> <8,4>
#   (2,8)    4               8 (high)                   <2,4> <4,4> <8,4>
#   (3,2)    4               2 (high)                   <2,4>
#   (4,4)    4  (high edge)  4 (high)                   <2,4> <4,4>
#   (5,5)    8  (low)        8 (low: 5)                 <2,8> <4,8> <8,8>
#   (8,3)    8  (high)       4 (low: 3)                 <2,8> <4,8>
#   (8,8)    8  (high)       8 (high)                   <2,8> <4,8> <8,8>
#   (9,6)    16 (low)        8                          <2,16> <4,16> <8,16>
#   (12,8)   16              8                          <2,16> <4,16> <8,16>
#   (13,3)   16              4 (low: 3)                 <2,16> <4,16>      (bit 12 of the plane masks)
#   (16,1)   16 (high)       2 (low: 1)                 <2,16>             (bit 15 of the plane masks)
#   (16,8)   16 (high)       8 (high)                   <2,16> <4,16> <8,16>
SCHEMES = [(1, 1), (1, 8), (2, 8), (3, 2), (4, 4), (5, 5), (8, 3), (8, 8), (9, 6), (12, 8), (13, 3), (16, 1), (16, 8)]
SWEEP_SCHEMES = [(3, 2), (16, 8)]
LAYOUTS = ("packed", "strided", "stores")


def lengths(d):
    """data lengths of a scheme: one byte, one byte a shard, a shard of one block less / exactly / more than a byte, ragged"""
    return [1, d, 16 * d - 1, 16 * d, 16 * d + 1, 33 * d + 5]


def sweep_lengths(d):
    """shard_len = 17..32: every residue mod 16 behind one whole block, the last data shard d - 1 bytes short"""
    return [d * sl - (d - 1) for sl in range(17, 33)]


@contextlib.contextmanager
def no_zones(*_):
    yield None


def _guarded(zones, windows, fn):
    """`fn()` with the kernels confined to the windows [(buf, lo, hi), ...]; its return value"""
    flat = list(windows[0]) + list(windows[1:])
    with zones(*flat) as hits:
        rc = fn()
    assert hits is None or hits.count == 0, (hits.count, hits.first)
    return rc


class Geometry:
    """where shard k of codeword i lies: `off + i * cw_stride + k * shard_stride` in a buffer of `size` bytes"""

    def __init__(self, d, p, L, n, layout):
        self.d, self.p, self.t, self.L, self.n, self.layout = d, p, d + p, L, n, layout
        self.sl = sl = -(-L // d)
        if layout == "packed":              # (a) a codeword buffer with no rounding at all
            self.ss, self.cs, self.off = sl, (d + p) * sl, SLACK
        elif layout == "strided":           # (b) gaps behind every shard and every codeword, odd base address
            self.ss, self.off = sl + 3, SLACK + 1
            self.cs = (d + p) * self.ss + 7
        elif layout == "stores":            # (c) shard-major: store k holds shard k of every codeword
            self.ss, self.cs, self.off = n * sl, sl, SLACK
        else:
            raise ValueError(layout)
        self.span = (n - 1) * self.cs + (self.t - 1) * self.ss + sl
        self.size = self.off + self.span + SLACK
        self._idx = None

    def pos(self, i, k):
        return self.off + i * self.cs + k * self.ss

    def blank(self):
        return np.full(self.size, FILL, np.uint8)

    def place(self, img, shards, ks, value=None):
        """shards `ks` of every codeword into the image: from shards[n, t, sl], or filled with `value`"""
        if self._idx is None:
            self._idx = (self.off + np.arange(self.n)[:, None, None] * self.cs + np.arange(self.t)[None, :, None] * self.ss
                         + np.arange(self.sl)[None, None, :])
        ks = list(ks)
        img[self._idx[:, ks]] = shards[:, ks] if value is None else value
        return img


def _dev(arr, device):
    import torch
    t = torch.tensor(arr, device=device)                        # always a copy
    assert t.is_contiguous()
    return t


def _host(t):
    return t.cpu().numpy()


def codeword_shards(oracle, d, p, data):
    """[n, d + p, shard_len]: from_data's zero-padded split of every row, and the oracle's parity below it"""
    n, L = data.shape
    sl = -(-L // d)
    sh = np.zeros((n, d + p, sl), np.uint8)
    flat = np.zeros((n, d * sl), np.uint8)
    flat[:, :L] = data
    sh[:, :d] = flat.reshape(n, d, sl)
    for i in range(n):
        sh[i, d:] = oracle.rs_encode(d, p, data[i])
    return sh


def erasure_patterns(d, p):
    """tuples of erased shard ids, every size 1..p: all of a size where there are at most 10, else 6 drawn with a fixed seed;
    always the first p shards, the last p, and p shards across the data / parity boundary ((3,2): all 15 patterns)"""
    t = d + p
    rng = np.random.default_rng(1000 * d + p)
    pats = []
    for k in range(1, p + 1):
        if math.comb(t, k) <= 10:
            pats += list(itertools.combinations(range(t), k))
        else:
            pats += [tuple(sorted(int(x) for x in rng.choice(t, k, replace=False))) for _ in range(6)]
    lo = max(0, d - (p + 1) // 2)
    pats += [tuple(range(p)), tuple(range(t - p, t)), tuple(range(lo, lo + p))]
    return list(dict.fromkeys(pats))


def _source(g, data, device):
    """the serialized rows in a guarded buffer of their own: packed (stride L), or stride L + 5 from an odd address"""
    stride, off = (g.L + 5, SLACK + 1) if g.layout == "strided" else (g.L, SLACK)
    img = np.full(off + (g.n - 1) * stride + g.L + SLACK, FILL, np.uint8)
    for i in range(g.n):
        img[off + i * stride:off + i * stride + g.L] = data[i]
    t = _dev(img, device)
    return t, off, stride, (t, off, off + (g.n - 1) * stride + g.L)


def check_encode(device, oracle, zones, g, data, shards):
    """smr_rs_encode / smr_rs_encode_lut write the parity shards of the layout and nothing else; the one-pass from_data forms
    write every shard"""
    from summerset_amd import _lib
    lib, st = _lib.load(), _lib.stream_ptr(None)
    d, p, n, L, sl = g.d, g.p, g.n, g.L, g.sl
    src, soff, sstride, swin = _source(g, data, device)
    want_par = g.place(g.blank(), shards, range(d, g.t))
    for name in ("smr_rs_encode", "smr_rs_encode_lut"):
        out = _dev(g.blank(), device)
        rc = _guarded(zones, [swin, (out, g.pos(0, d), g.pos(n - 1, g.t - 1) + sl)],
                      lambda: getattr(lib, name)(src.data_ptr() + soff, L, sstride, n, d, p, out.data_ptr() + g.pos(0, d), g.cs, g.ss, st))
        assert rc == 0 and np.array_equal(_host(out), want_par), (name, d, p, L, g.layout)
    want = g.place(g.blank(), shards, range(g.t))
    if g.layout == "strided":
        # the one-pass form lays the shards of a codeword side by side: here with a padded cw_stride from an odd address
        h = Geometry(d, p, L, n, "packed")
        h.cs, h.off = g.t * sl + 7, SLACK + 1
        h.span = (n - 1) * h.cs + g.t * sl
        h.size = h.off + h.span + SLACK
        assert h.ss == sl and h._idx is None
        g, want = h, h.place(h.blank(), shards, range(h.t))
    out = _dev(g.blank(), device)
    assert (out.data_ptr() + g.off) % 2 == (1 if g.off != SLACK else 0)
    if g.layout == "stores":
        call = lambda: lib.smr_rs_from_data_encode_stores(src.data_ptr() + soff, L, sstride, n, d, p, out.data_ptr() + g.off, g.ss, g.cs, st)
    else:
        call = lambda: lib.smr_rs_from_data_encode(src.data_ptr() + soff, L, sstride, n, d, p, out.data_ptr() + g.off, g.cs, st)
    rc = _guarded(zones, [swin, (out, g.off, g.off + g.span)], call)
    assert rc == 0 and np.array_equal(_host(out), want), ("from_data", d, p, L, g.layout)
    assert np.array_equal(_host(src)[:soff], np.full(soff, FILL, np.uint8))            # (the source is only read)


def check_reconstruct(device, zones, g, shards, patterns=None):
    """every pattern, reconstruct_all and reconstruct_data: afterwards the buffer is what it was, with exactly the shards the call
    had to rebuild replaced by the original bytes -- present shards, erased parity under data_only, gaps and slack as they were"""
    from summerset_amd import _lib
    lib, st = _lib.load(), _lib.stream_ptr(None)
    full = g.place(g.blank(), shards, range(g.t))
    calls = 0
    for lost in (erasure_patterns(g.d, g.p) if patterns is None else patterns):
        before = g.place(full.copy(), None, lost, value=ERASED)
        mask = ((1 << g.t) - 1) & ~sum(1 << k for k in lost)
        for data_only in (0, 1):
            rebuilt = [k for k in lost if k < g.d or not data_only]
            want = g.place(before.copy(), shards, rebuilt)
            buf = _dev(before, device)
            rc = _guarded(zones, [(buf, g.off, g.off + g.span)],
                          lambda: lib.smr_rs_reconstruct(buf.data_ptr() + g.off, g.sl, g.ss, g.cs, g.n, g.d, g.p, mask, data_only, st))
            assert rc == 0, (g.d, g.p, g.L, g.layout, lost, data_only, lib.smr_last_error())
            got = _host(buf)
            if not np.array_equal(got, want):
                bad = np.nonzero(got != want)[0]
                raise AssertionError("reconstruct (%d,%d) L=%d %s lost=%s data_only=%d: %d bytes differ, first at buffer offset %d (shards start at %d)"
                                     % (g.d, g.p, g.L, g.layout, lost, data_only, bad.size, bad[0], g.off))
            calls += 1
    # one shard more than the code can lose: refused, nothing written.  (No pattern reaches the "too many missing shards" refusal
    # behind it: with p <= 8 a ninth missing shard leaves fewer than d, and "too few shards present" comes first.)
    lost = tuple(range(g.p + 1))
    before = g.place(full.copy(), None, lost, value=ERASED)
    buf = _dev(before, device)
    rc = _guarded(zones, [(buf, 0, 0)], lambda: lib.smr_rs_reconstruct(buf.data_ptr() + g.off, g.sl, g.ss, g.cs, g.n, g.d, g.p,
                                                                        ((1 << g.t) - 1) & ~((1 << (g.p + 1)) - 1), 0, st))
    assert rc == _lib.SMR_ERR_ARG and b"too few shards" in lib.smr_last_error() and np.array_equal(_host(buf), before)
    return calls


def check_verify(device, zones, g, shards):
    """clean: every codeword passes; one bit flipped at the corners of the shard set, each in a codeword of its own: exactly those
    fail; a flip in a gap byte (strided layout) fails nobody.  ok[] is written for the n codewords and nowhere else."""
    from summerset_amd import _lib
    lib, st = _lib.load(), _lib.stream_ptr(None)
    n, d, t, sl = g.n, g.d, g.t, g.sl
    assert n >= 4
    full = g.place(g.blank(), shards, range(t))

    def run(img):
        buf = _dev(img, device)
        ok = _dev(np.full(SLACK + n + SLACK, 7, np.uint8), device)
        rc = _guarded(zones, [(buf, g.off, g.off + g.span), (ok, SLACK, SLACK + n)],
                      lambda: lib.smr_rs_verify(buf.data_ptr() + g.off, sl, g.ss, g.cs, n, d, g.p, ok.data_ptr() + SLACK, st))
        assert rc == 0, lib.smr_last_error()
        assert np.array_equal(_host(buf), img)
        ok = _host(ok)
        assert (ok[:SLACK] == 7).all() and (ok[SLACK + n:] == 7).all()
        return ok[SLACK:SLACK + n]

    assert run(full).tolist() == [1] * n, (g.d, g.p, g.L, g.layout)
    bad = full.copy()
    flips = {0: g.pos(0, 0),                                    # first byte of shard 0, first codeword
             n // 2: g.pos(n // 2, d - 1) + sl - 1,             # last byte of the last data shard, a middle one
             n - 1: g.pos(n - 1, t - 1) + sl - 1,               # last byte of the last parity shard, the last one
             1: g.pos(1, t - 1)}                                # first byte of the last parity shard
    assert len(flips) == 4
    for bit, a in enumerate(flips.values()):
        bad[a] ^= 1 << (2 * bit + 1)
    assert run(bad).tolist() == [0 if i in flips else 1 for i in range(n)], (g.d, g.p, g.L, g.layout)
    if g.layout == "strided":
        gap = full.copy()
        for a in (g.pos(0, 0) + sl, g.pos(1, t - 1) + sl + 2, g.pos(n - 1, d - 1) + sl + 1, g.pos(n - 2, t - 1) + g.ss + 3):
            assert gap[a] == FILL
            gap[a] ^= 0x10
        assert run(gap).tolist() == [1] * n, (g.d, g.p, g.L)


def one_case(device, oracle, zones, d, p, L, layout, n=5, patterns=None):
    """encode, reconstruct and verify of n codewords of L bytes in one layout; the number of reconstruct calls made"""
    rng = np.random.default_rng([d, p, L, LAYOUTS.index(layout)])
    data = rng.integers(0, 256, (n, L), dtype=np.uint8)
    data[0, -1] = 0xFF                                          # (no zero where the padding begins)
    g = Geometry(d, p, L, n, layout)
    shards = codeword_shards(oracle, d, p, data)
    check_encode(device, oracle, zones, g, data, shards)
    calls = check_reconstruct(device, zones, g, shards, patterns)
    check_verify(device, zones, g, shards)
    return calls


def scheme_cases(device, oracle, zones, d, p, Ls=None, n=5):
    calls = 0
    for L in (lengths(d) if Ls is None else Ls):
        for layout in LAYOUTS:
            calls += one_case(device, oracle, zones, d, p, L, layout, n=n)
    return calls


def matrix_matches_oracle(oracle):
    from summerset_amd import rscoding
    for d, p in SCHEMES:
        assert np.array_equal(rscoding.rs_matrix(d, p), oracle.rs_matrix(d, p)), (d, p)


def error_paths(device, oracle, zones):
    """calls that must be refused with SMR_ERR_ARG before anything is launched or written"""
    from summerset_amd import _lib
    lib, st, ERR = _lib.load(), _lib.stream_ptr(None), _lib.SMR_ERR_ARG
    d, p, n, L = 3, 2, 4, 24
    rng = np.random.default_rng(77)
    data = rng.integers(0, 256, (n, L), dtype=np.uint8)
    g = Geometry(d, p, L, n, "packed")
    sl = g.sl
    shards = codeword_shards(oracle, d, p, data)
    full = g.place(g.blank(), shards, range(g.t))

    def refused(fn, *imgs):
        bufs = [_dev(i, device) for i in imgs]
        rc = _guarded(zones, [(b, 0, 0) for b in bufs], lambda: fn(*[b.data_ptr() for b in bufs]))
        assert rc == ERR, (rc, lib.smr_last_error())
        for b, i in zip(bufs, imgs):
            assert np.array_equal(_host(b), i)

    ok7 = np.full(SLACK + n + SLACK, 7, np.uint8)
    # null buffers
    refused(lambda okp: lib.smr_rs_verify(None, sl, g.ss, g.cs, n, d, p, okp + SLACK, st), ok7)
    refused(lambda b: lib.smr_rs_verify(b + g.off, sl, g.ss, g.cs, n, d, p, None, st), full)
    assert lib.smr_rs_reconstruct(None, sl, g.ss, g.cs, n, d, p, 0b11110, 0, st) == ERR
    # layouts whose shards overlap: (shard_stride, cw_stride)
    for ss, cs in ((sl - 1, g.cs),                                          # shards of a codeword run into each other
                   (sl, g.t * sl - 1),                                      # codewords run into each other ...
                   (sl + 3, (g.t - 1) * (sl + 3) + sl - 1),                 # ... by one byte, strided
                   (n * sl, sl - 1),                                        # shard-major: a store's shards overlap
                   ((n - 1) * sl + sl - 1, sl),                             # shard-major: the stores overlap by one byte
                   (0, 0)):
        refused(lambda b: lib.smr_rs_reconstruct(b + g.off, sl, ss, cs, n, d, p, 0b11110, 0, st), full)
        refused(lambda b, okp: lib.smr_rs_verify(b + g.off, sl, ss, cs, n, d, p, okp + SLACK, st), full, ok7)
    # ... while one codeword has no cw_stride to get wrong, and the two rules' own edges are taken
    one = Geometry(d, p, L, 1, "packed")
    sh1 = shards[:1]
    img = one.place(one.place(one.blank(), sh1, range(one.t)), None, (0,), value=ERASED)
    buf = _dev(img, device)
    rc = _guarded(zones, [(buf, one.off, one.off + one.span)],
                  lambda: lib.smr_rs_reconstruct(buf.data_ptr() + one.off, sl, sl, 0, 1, d, p, 0b11110, 0, st))
    assert rc == 0 and np.array_equal(_host(buf), one.place(one.blank(), sh1, range(one.t)))
    # one launch holds at most 0xFFFFFF blocks of 256 lanes: 2^24 codewords of 4096-byte shards are one block too many
    big, bsl = 1 << 24, 4096
    dummy = np.full(256, FILL, np.uint8)
    refused(lambda b: lib.smr_rs_reconstruct(b + SLACK, bsl, bsl, 5 * bsl, big, 3, 2, 0b11110, 0, st), dummy)
    refused(lambda b: lib.smr_rs_encode(b + SLACK, 3 * bsl, 3 * bsl, big, 3, 2, b + SLACK, 2 * bsl, bsl, st), dummy)
    refused(lambda b: lib.smr_rs_encode_lut(b + SLACK, 3 * bsl, 3 * bsl, big, 3, 2, b + SLACK, 2 * bsl, bsl, st), dummy)
    refused(lambda b, okp: lib.smr_rs_verify(b + SLACK, bsl, bsl, 5 * bsl, big, 3, 2, okp, st), dummy, np.full(big, 7, np.uint8))
