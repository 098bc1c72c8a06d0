"""The RS kernels on the device at every <NOUT, NIN> instance, every size of erasure pattern and three shard layouts: the bodies
of tests/rs_cases.py (which the emulator runs inside red zones in tests/test_rs_bounds.py), against the CPU oracle and the
codewords' own bytes, bit for bit.  A load cannot be observed here and is not probed: what the device run shows is that every
instance computes the right bytes on gfx950, that stores stay inside the shards (every buffer is compared whole, filler
included) and that refused calls return without launching.  Stage 10: behind the rest of the suite under `pytest -x`."""
import numpy as np
import pytest

import rs_cases as c

pytestmark = [pytest.mark.gpu, pytest.mark.timeout(600), pytest.mark.stage(10)]


def test_matrix_matches_the_oracle(cuda, oracle):
    c.matrix_matches_oracle(oracle)


@pytest.mark.parametrize("scheme", c.SCHEMES, ids=lambda s: "%d_%d" % s)
def test_scheme_in_every_layout(cuda, oracle, scheme):
    """the emulator's six lengths, and 4099 / 65536 + 7 bytes: launches of several blocks, shards of hundreds of 16-byte columns"""
    d, p = scheme
    c.scheme_cases(cuda, oracle, c.no_zones, d, p, n=13)
    c.scheme_cases(cuda, oracle, c.no_zones, d, p, Ls=[4099, 65536 + 7], n=7)


@pytest.mark.parametrize("scheme", c.SWEEP_SCHEMES, ids=lambda s: "%d_%d" % s)
def test_every_shard_length_residue(cuda, oracle, scheme):
    d, p = scheme
    c.scheme_cases(cuda, oracle, c.no_zones, d, p, Ls=c.sweep_lengths(d), n=13)


def test_error_paths_launch_nothing(cuda, oracle):
    c.error_paths(cuda, oracle, c.no_zones)


def test_offsets_beyond_4_gib(cuda, oracle):
    """700 000 codewords of 4099 bytes through the shard-major one-pass encode: 2.9 GB of source, 4.8 GB of stores.  Shard 4's
    store begins at 4 * 700 000 * 1367 = 3.83e9 bytes and ends at 4.78e9: it runs across 2^32, its rows from 341 894 on -- row
    n - 1, where the bit is flipped, among them -- lie beyond it.  The 64-bit store offsets of every kernel of the family
    (from_data, verify, reconstruct)."""
    import torch
    from summerset_amd import RSCodewordBatch
    d, p, L, n = 3, 2, 4099, 700_000
    free, _ = torch.cuda.mem_get_info()
    assert free >= 12 * 10**9, "this case needs 12 GB of free device memory, %d bytes are free" % free
    g = torch.Generator(device=cuda).manual_seed(4099)
    src = torch.randint(0, 256, (n, L), dtype=torch.uint8, device=cuda, generator=g)
    cw = RSCodewordBatch.from_data_and_encode_stores(src, d, p)
    stores, sl = cw.stores, cw.shard_len
    try:
        assert sl == 1367 and stores.shape == (5, n, sl)
        assert 4 * n * sl < 2**32 < 4 * n * sl + (n - 1) * sl                   # shard 4's store straddles 2^32; its last row is beyond
        assert bool(cw.verify_parity().all())
        rows = sorted({0, n - 1} | {int(x) for x in np.random.default_rng(64).choice(n, 62, replace=False)})
        assert len(rows) >= 62
        idx = torch.tensor(rows, device=cuda)
        data = src[idx].cpu().numpy()
        got = stores[:, idx].cpu().numpy()                                      # [5, rows, sl]
        del src
        for j, i in enumerate(rows):
            padded = np.zeros(d * sl, np.uint8)
            padded[:L] = data[j]
            assert np.array_equal(got[:d, j].reshape(-1), padded), i
            assert np.array_equal(got[d:, j], oracle.rs_encode(d, p, data[j])), i
        stores[4, n - 1, sl - 1] ^= 0x04
        bad = (~cw.verify_parity()).nonzero().flatten().tolist()
        assert bad == [n - 1], bad[:10]
        stores[4, n - 1, sl - 1] ^= 0x04
        keep = stores.clone()
        cw.erase((0, 4))
        assert not torch.equal(stores, keep)
        cw.reconstruct_all()
        assert torch.equal(stores, keep)
        del keep
    finally:
        src = cw = stores = None
        torch.cuda.empty_cache()
