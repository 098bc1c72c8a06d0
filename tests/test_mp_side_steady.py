"""The side launch's steady step (mp_engine.hip: side_steady_tick) on the emulator build of the engine (tests/hostsim): the shipped
kernels and C-ABI, every lane a fiber, against the CPU oracle after every run_ticks call.  The bodies are
tests/mp_side_steady_cases.py; the device runs the same ones in tests/test_zzzz_mp_side_steady_gpu.py.

The emulator's side grid is 12 blocks (-DSTRAG_BATCH_BLOCKS=12, tests/hostsim), so a list of 22 groups and more puts several
groups on the lanes of one block, and G = 257 with a third of the groups listed (86 > 12 x STRAG_BATCH_K) takes a second pass."""
import pytest


@pytest.fixture(scope="module")
def sim():
    import hostsim
    hostsim.build()
    return hostsim


def test_symbol_is_exported_and_bound(sim):
    from summerset_amd import _lib
    assert "smr_mp_debug_side_steps" in {n for n, _, _ in _lib.SYMBOLS} and sim.load().smr_mp_debug_side_steps


@pytest.mark.parametrize("G,R,S,W,hb,batch", [(65, 3, 1, 32, 2, 8), (130, 5, 5, 64, 2, 3), (257, 7, 1, 32, 4, 8), (130, 5, 1, 64, 4, 1)])
def test_steady_and_listed(sim, oracle, G, R, S, W, hb, batch):
    import mp_side_steady_cases as c
    with sim.patched():
        c.steady_and_listed("cpu", oracle, G, R, S, W, hb, batch)


@pytest.mark.parametrize("G,R,S,W,ttl,hb,batches", [(130, 5, 5, 64, 4, 4, (8,)), (65, 3, 1, 32, 1, 2, (3,)), (65, 7, 5, 64, 0xFE, 2, (1, 3, 8)),
                                                   (130, 5, 5, 64, 0xFF, 4, (8,))])
def test_reply_loss(sim, oracle, G, R, S, W, ttl, hb, batches):
    import mp_side_steady_cases as c
    with sim.patched():
        c.reply_loss("cpu", oracle, G, R, S, W, ttl, hb, batches)


@pytest.mark.parametrize("G,R,S,W,ttl,hb", [(130, 5, 5, 64, 4, 4), (65, 3, 1, 32, 1, 2), (257, 5, 1, 32, 0xFE, 4), (65, 7, 32, 64, 4, 2),
                                            (65, 5, 33, 64, 0xFE, 4)])
def test_timeout_in_every_position_of_a_batch(sim, oracle, G, R, S, W, ttl, hb):
    import mp_side_steady_cases as c
    with sim.patched():
        c.timeout_in_every_position("cpu", oracle, G, R, S, W, ttl, hb)


@pytest.mark.parametrize("G,R,S,W,ttl,hb,batches", [(130, 5, 5, 64, 0xFE, 2, (8, 3, 1)), (65, 3, 1, 32, 4, 4, (3,)), (65, 7, 5, 64, 4, 2, (8,))])
def test_redirects_and_empty_batches(sim, oracle, G, R, S, W, ttl, hb, batches):
    import mp_side_steady_cases as c
    with sim.patched():
        c.redirects_and_empty_batches("cpu", oracle, G, R, S, W, ttl, hb, batches)


@pytest.mark.parametrize("G,R,S,W,ttl,hb,batches,reserve,frozen", [(65, 5, 3, 16, 0xFE, 8, (8,), None, False), (130, 5, 5, 32, 0xFE, 4, (3, 8), None, False),
                                                                  (65, 3, 32, 64, 4, 2, (8, 3), 0, True), (65, 7, 33, 64, 0xFE, 4, (1, 8), None, False)])
def test_window(sim, oracle, G, R, S, W, ttl, hb, batches, reserve, frozen):
    import mp_side_steady_cases as c
    with sim.patched():
        c.window("cpu", oracle, G, R, S, W, ttl, hb, batches, win_reserve=reserve, expect_frozen=frozen)


@pytest.mark.parametrize("G,R,S,W,ttl,hb", [(130, 5, 5, 64, 4, 4), (65, 3, 1, 32, 1, 2), (65, 7, 5, 64, 4, 2)])
def test_hand_back_to_the_bulk(sim, oracle, G, R, S, W, ttl, hb):
    import mp_side_steady_cases as c
    with sim.patched():
        c.hand_back("cpu", oracle, G, R, S, W, ttl, hb, (8,))


@pytest.mark.parametrize("G,R,S,W,ttl,hb", [(130, 5, 5, 64, 0xFE, 4), (65, 3, 1, 32, 4, 2)])
def test_save_and_load(sim, oracle, G, R, S, W, ttl, hb):
    import mp_side_steady_cases as c
    with sim.patched():
        c.save_and_load("cpu", oracle, G, R, S, W, ttl, hb)


@pytest.mark.parametrize("G,R,S,W,ttl,hb,batches", [(130, 5, 5, 64, 4, 4, (8,)), (257, 3, 1, 32, 0xFE, 2, (1, 3, 8)), (65, 7, 5, 64, 1, 4, (3,))])
def test_both_switch_settings(sim, oracle, G, R, S, W, ttl, hb, batches):
    import mp_side_steady_cases as c
    with sim.patched():
        c.both_settings("cpu", oracle, G, R, S, W, ttl, hb, batches)
