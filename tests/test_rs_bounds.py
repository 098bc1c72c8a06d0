"""The RS entry points on the emulator build of the engine (tests/hostsim): the shipped kernels and C-ABI, every lane a fiber,
with red zones around every buffer -- a kernel access outside the bytes the header allows a call to touch, a LOAD included, is
recorded and fails the test.  The bodies are tests/rs_cases.py; the device runs the same ones in tests/test_zzzz_rs_edges_gpu.py,
where only the written bytes can be checked."""
import numpy as np
import pytest

import rs_cases as c


@pytest.fixture(scope="module")
def sim():
    import hostsim
    hostsim.build()
    return hostsim


def test_red_zones_record_and_lift(sim):
    """the context manager itself: a load one byte past the window is a recorded hit with its text, the call still finishes, and
    afterwards the ranges are gone (the same call, unguarded, hits nothing and aborts nothing)"""
    import torch
    from summerset_amd import _lib
    size = 64 + 48 + 64
    buf = torch.full((size,), 0xCD, dtype=torch.uint8)
    ok = torch.full((3,), 7, dtype=torch.uint8)
    with sim.patched() as lib:
        def verify():
            return lib.smr_rs_verify(buf.data_ptr() + 64, 8, 8, 48, 1, 4, 2, ok.data_ptr(), _lib.stream_ptr(None))
        with sim.red_zones(buf, 64, 64 + 47) as hits:            # the window ends one byte short of the last shard
            assert verify() == 0
        assert hits.count >= 1 and "arena guard gap" in hits.first and "load" in hits.first, (hits.count, hits.first)
        with sim.red_zones(buf, 64, 64 + 48, (ok, 0, 1)) as hits:
            assert verify() == 0
        assert hits.count == 0 and hits.first == "", (hits.count, hits.first)
        with pytest.raises(ZeroDivisionError):
            with sim.red_zones(buf, 64, 64) as hits:
                1 / 0
        assert verify() == 0                                     # no range left behind: nothing records, nothing aborts
        with sim.red_zones(buf, 0, size) as hits:
            pass
        assert hits.count == 0


def test_reconstruct_reads_no_byte_behind_the_last_shard(sim, oracle):
    """(4+2) shards of 8 bytes, packed: 48-byte codewords, so a whole 16-byte load of a shard's only (partial) block runs 8 bytes
    past the shard -- for the last shard of the last codeword, past the buffer.  Shards 0 and 1 erased: the sources are shards
    2..5 and the last one is read.  Before the loads were bounded by the shards' real extent this recorded
    "load of 16 bytes ... runs into an arena guard gap" (lane 2, the last codeword)."""
    import torch
    from summerset_amd import _lib
    d, p, n, L = 4, 2, 3, 32
    data = np.random.default_rng(8).integers(0, 256, (n, L), dtype=np.uint8)
    g = c.Geometry(d, p, L, n, "packed")
    assert (g.sl, g.ss, g.cs, g.span) == (8, 8, 48, 144)
    sh = c.codeword_shards(oracle, d, p, data)
    want = g.place(g.blank(), sh, range(6))
    buf = torch.tensor(g.place(want.copy(), None, (0, 1), value=c.ERASED))
    with sim.patched() as lib:
        with sim.red_zones(buf, g.off, g.off + g.span) as hits:
            rc = lib.smr_rs_reconstruct(buf.data_ptr() + g.off, 8, 8, 48, n, d, p, 0b111100, 0, _lib.stream_ptr(None))
    assert hits.count == 0, (hits.count, hits.first)
    assert rc == 0 and np.array_equal(buf.numpy(), want)


def test_verify_reads_no_byte_behind_shard_major_stores(sim, oracle):
    """RS(3,2), five codewords of one-byte shards, shard-major: 25 bytes of stores.  Every lane's 16-byte load of a data shard
    started at offset 0..14 of 25 -- the one at offset 10 and the ones behind it left the stores."""
    import torch
    from summerset_amd import _lib
    d, p, n, L = 3, 2, 5, 2
    data = np.random.default_rng(9).integers(0, 256, (n, L), dtype=np.uint8)
    g = c.Geometry(d, p, L, n, "stores")
    assert (g.sl, g.ss, g.cs, g.span) == (1, 5, 1, 25)
    sh = c.codeword_shards(oracle, d, p, data)
    buf = torch.tensor(g.place(g.blank(), sh, range(5)))
    ok = torch.full((n,), 7, dtype=torch.uint8)
    with sim.patched() as lib:
        with sim.red_zones(buf, g.off, g.off + g.span, (ok, 0, n)) as hits:
            rc = lib.smr_rs_verify(buf.data_ptr() + g.off, 1, 5, 1, n, d, p, ok.data_ptr(), _lib.stream_ptr(None))
    assert hits.count == 0, (hits.count, hits.first)
    assert rc == 0 and ok.tolist() == [1] * n


def test_matrix_matches_the_oracle(sim, oracle):
    with sim.patched():
        c.matrix_matches_oracle(oracle)


@pytest.mark.parametrize("scheme", c.SCHEMES, ids=lambda s: "%d_%d" % s)
def test_scheme_in_every_layout(sim, oracle, scheme):
    """encode (xtime, LUT, one-pass), every erasure pattern size through reconstruct_all / reconstruct_data, verify -- six lengths,
    three layouts, every call confined to its bytes"""
    with sim.patched():
        calls = c.scheme_cases("cpu", oracle, sim.red_zones, *scheme)
    assert calls >= 2 * 18 * min(scheme[0] + scheme[1], 3)


@pytest.mark.parametrize("scheme", c.SWEEP_SCHEMES, ids=lambda s: "%d_%d" % s)
def test_every_shard_length_residue(sim, oracle, scheme):
    """shard_len 17..32: every length of a shard's last block"""
    d, p = scheme
    with sim.patched():
        c.scheme_cases("cpu", oracle, sim.red_zones, d, p, Ls=c.sweep_lengths(d))


def test_error_paths_launch_nothing(sim, oracle):
    with sim.patched():
        c.error_paths("cpu", oracle, sim.red_zones)
