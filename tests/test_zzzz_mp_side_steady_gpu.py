"""The side launch's steady step (mp_engine.hip: side_steady_tick) on the device: tests/mp_side_steady_cases.py, the cases
tests/test_mp_side_steady.py runs on the emulator, at the same small shapes -- on the device's grid of 192 side blocks a listed
group has a block to itself, the emulator's 12 blocks are what puts several on one.  Bit-exact against the CPU oracle after
every run_ticks call; no case is skipped."""
import pytest

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("G,R,S,W,hb,batch", [(65, 3, 1, 32, 2, 8), (130, 5, 5, 64, 2, 3), (257, 7, 1, 32, 4, 8)])
def test_steady_and_listed(cuda, oracle, G, R, S, W, hb, batch):
    import mp_side_steady_cases as c
    c.steady_and_listed(cuda, oracle, G, R, S, W, hb, batch)


@pytest.mark.parametrize("G,R,S,W,ttl,hb,batches", [(130, 5, 5, 64, 4, 4, (8,)), (65, 7, 5, 64, 0xFE, 2, (1, 3, 8)), (130, 5, 5, 64, 0xFF, 4, (8,))])
def test_reply_loss(cuda, oracle, G, R, S, W, ttl, hb, batches):
    import mp_side_steady_cases as c
    c.reply_loss(cuda, oracle, G, R, S, W, ttl, hb, batches)


@pytest.mark.parametrize("G,R,S,W,ttl,hb", [(130, 5, 5, 64, 4, 4), (65, 3, 1, 32, 1, 2), (257, 5, 1, 32, 0xFE, 4), (65, 7, 32, 64, 4, 2),
                                            (65, 5, 33, 64, 0xFE, 4)])
def test_timeout_in_every_position_of_a_batch(cuda, oracle, G, R, S, W, ttl, hb):
    import mp_side_steady_cases as c
    c.timeout_in_every_position(cuda, oracle, G, R, S, W, ttl, hb)


@pytest.mark.parametrize("G,R,S,W,ttl,hb,batches", [(130, 5, 5, 64, 0xFE, 2, (8, 3, 1)), (65, 3, 1, 32, 4, 4, (3,))])
def test_redirects_and_empty_batches(cuda, oracle, G, R, S, W, ttl, hb, batches):
    import mp_side_steady_cases as c
    c.redirects_and_empty_batches(cuda, oracle, G, R, S, W, ttl, hb, batches)


@pytest.mark.parametrize("G,R,S,W,ttl,hb,batches,reserve,frozen", [(65, 5, 3, 16, 0xFE, 8, (8,), None, False), (65, 3, 32, 64, 4, 2, (8, 3), 0, True),
                                                                  (65, 7, 33, 64, 0xFE, 4, (1, 8), None, False)])
def test_window(cuda, oracle, G, R, S, W, ttl, hb, batches, reserve, frozen):
    import mp_side_steady_cases as c
    c.window(cuda, oracle, G, R, S, W, ttl, hb, batches, win_reserve=reserve, expect_frozen=frozen)


@pytest.mark.parametrize("G,R,S,W,ttl,hb", [(130, 5, 5, 64, 4, 4), (65, 3, 1, 32, 1, 2)])
def test_hand_back_to_the_bulk(cuda, oracle, G, R, S, W, ttl, hb):
    import mp_side_steady_cases as c
    c.hand_back(cuda, oracle, G, R, S, W, ttl, hb, (8,))


@pytest.mark.parametrize("G,R,S,W,ttl,hb", [(130, 5, 5, 64, 0xFE, 4), (65, 3, 1, 32, 4, 2)])
def test_save_and_load(cuda, oracle, G, R, S, W, ttl, hb):
    import mp_side_steady_cases as c
    c.save_and_load(cuda, oracle, G, R, S, W, ttl, hb)


@pytest.mark.parametrize("G,R,S,W,ttl,hb,batches", [(130, 5, 5, 64, 4, 4, (8,)), (257, 3, 1, 32, 0xFE, 2, (1, 3, 8)), (65, 7, 5, 64, 1, 4, (3,))])
def test_both_switch_settings(cuda, oracle, G, R, S, W, ttl, hb, batches):
    import mp_side_steady_cases as c
    c.both_settings(cuda, oracle, G, R, S, W, ttl, hb, batches)
