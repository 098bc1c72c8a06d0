"""`smr_ep_cluster_tick` at the edges the Zipf schedules of test_zz_ep_cluster_gpu.py / test_zzz_ep_cluster_fused_gpu.py do not
reach -- always against the oracle cluster of tests/ep_cluster.py, bit for bit (every leader's outputs every tick, every replica's
dump() and exec_dump() at the end), one launch and launch by launch, in both orders of the leaders' steps:

* sequence numbers across 2^31, 2^32 - 1 (the sentinel of the 32-bit copy `sq32`), 2^32 and 2^63 (the sign of the binding's
  int64 tensors): a prelude through the handler-by-handler driver whose PreAcceptReplies carry a wide seq;
* the one-by-one launch's later passes (more listed lanes at a replica than its grid has: EPC_CL_MAX_BLOCKS);
* the execution walk outside LDS (R W > 512) and at the boundary (R W = 512);
* key and loss schedules that force the rare steps: a clique of R instances of one key, a key idle for more than W ticks, a
  silent replica, an isolated leader, an acceptor nobody hears, replies lost on their way back;
* populations 4 and 6, and the phase-major order on the step-by-step kernel (SMR_EP_PM_UNBATCHED).

Every body is a helper taking its sizes: tests/test_hostsim.py runs them small on the emulator build."""
import numpy as np
import pytest

import ep_cluster as ec
from test_zz_ep_cluster_gpu import run_fused_vs_driver

pytestmark = [pytest.mark.gpu, pytest.mark.timeout(1200)]

# base of the prelude's sequence numbers -> the boundaries the run must cross
WIDE = {2**31 - 3: (2**31,), 2**32 - 3: (2**32 - 1, 2**32), 2**63 - 3: (2**63,)}


def wide_seq_prelude(dev, base, R, G, K, span, seed, n_ticks=3):
    """ticks of the handler-by-handler driver (ep_cluster.tick on NumpyEngine / the oracles) whose PreAcceptReplies carry
    seq = base - off[g] (off < span, per group) from a seeded subset of the acceptors: the leaders commit those instances
    with that seq (fast path where the replies agree, slow path where they do not); a quarter of the groups stays narrow"""
    rng = np.random.default_rng(seed)
    off = rng.integers(0, span, G).astype(np.uint64)
    pick = rng.random((R, R, G)) < 0.6
    pick[:, :, rng.random(G) < 0.25] = False
    keys = [ec.same_key(rng, R, G, K) if t % 2 == 0 else ec.zipf_keys(rng, R, G, K) for t in range(n_ticks)]
    drop = [{(s, q): rng.random(G) < 0.1 for s in range(R) for q in range(R) if s != q} for _ in range(n_ticks)]
    via = ec.wide_seq_via(base, off, lambda s: pick[s])

    def run(sets, orcs):
        for reps in [[ec.NumpyEngine(e, dev) for e in s] for s in sets] + ([orcs] if orcs is not None else []):
            for t in range(n_ticks):
                ec.tick(reps, keys[t], drop[t], via=via)
    return run


def run_wide_seq(dev, oracle, base, G, W, phase_major, R=5, K=2, T=None, seed=3):
    """the prelude, then T >= 2W + 4 ticks of the cluster on K hot keys (cliques every other tick, loss): seq climbs across
    the boundaries of WIDE[base]; asserts that committed cells of the final dumps lie on both sides of each"""
    T = T or 2 * W + 4
    span = 4 * R * T
    rng0 = np.random.default_rng(seed)

    def schedule(rng, t):
        keys = ec.same_key(rng, R, G, K) if t % 2 else ec.zipf_keys(rng, R, G, K, p_propose=0.95)
        return keys, {(s, q): rng.random(G) < 0.08 for s in range(R) for q in range(R) if s != q and rng.random() < 0.5}
    info = {}
    slow = run_fused_vs_driver(dev, G, K, 0.0, T=T, R=R, W=W, oracle=oracle, phase_major=phase_major, seed=int(rng0.integers(1 << 20)),
                               schedule=schedule, prelude=wide_seq_prelude(dev, base, R, G, K, span, seed), info=info)
    seq = np.concatenate([d["seq"][d["status"] >= 3] for d in info["dumps"]]).astype(np.uint64)
    wide = seq[seq >= np.uint64(base - 2 * span)]
    for b in WIDE[base]:
        assert (wide < np.uint64(b)).any() and (wide >= np.uint64(b)).any(), (base, b, len(wide))
    return slow


def run_multi_pass(dev, oracle, G, cap_lanes, R=5, K=1, W=16, T=6, loss=0.1, seed=11):
    """phase-major one-launch ticks on a same-key clique in every group (every replica proposing): the lanes that leave the
    batched CommitNotice step go on their replica's list; asserts that some tick listed more than R x cap_lanes lanes in all --
    at least one replica's list longer than the one-by-one launch's grid covers in a pass (EPC_CL_MAX_BLOCKS x 2)"""
    def schedule(rng, t):
        keys = ec.same_key(rng, R, G, K)
        return keys, ({(s, q): rng.random(G) < loss for s in range(R) for q in range(R) if s != q} if loss else None)
    info = {}
    run_fused_vs_driver(dev, G, K, 0.0, T=T, R=R, W=W, oracle=oracle, phase_major=True, seed=seed, schedule=schedule, info=info)
    listed = max(st["commit_lanes_one_by_one"] for st in info["stats"])
    assert listed > R * cap_lanes, (listed, R * cap_lanes)
    return listed


def run_walk_outside_lds(dev, oracle, G, R, W, T=None, K=3, seed=21):
    """execution on, hot keys, phase major (the one-by-one launch keeps the walk in LDS only for R W <= 512) and leader major;
    T >= 2W + 4 is not needed for the walk: a few ticks list lanes"""
    T = T or 6
    listed = 0
    for pm in (False, True):
        def schedule(rng, t):
            keys = ec.same_key(rng, R, G, K) if t % 2 else ec.zipf_keys(rng, R, G, K)
            return keys, {(s, q): rng.random(G) < 0.1 for s in range(R) for q in range(R) if s != q}
        info = {}
        run_fused_vs_driver(dev, G, K, 0.0, T=T, R=R, W=W, oracle=oracle, phase_major=pm, seed=seed, schedule=schedule, info=info)
        if pm:
            listed = sum(st["commit_lanes_one_by_one"] for st in info["stats"])
    assert listed > 0                                            # the one-by-one launch walked (with R W > 512: in global memory)
    return listed


SCHEDULES = ("same_key", "idle_then_hot", "silent_rows", "isolated_leader", "deaf_acceptor", "lost_replies")


def run_schedule(dev, oracle, name, G, R=5, W=16, K=4, T=None, execute=True, phase_major=False, seed=31, unbatched=False):
    """one of SCHEDULES through the cluster tick against the oracle cluster; `lost_replies` runs its losses in a prelude through
    the handler-by-handler driver (the cluster's drop masks lose a PreAccept with its reply), then Zipf ticks on the cluster"""
    T = T or (2 * W + 6 if name == "idle_then_hot" else 8)
    if name == "idle_then_hot":                                  # two keys: each comes back after W + 2 idle ticks, by tick 2W + 4
        K = 2
    groups = (np.arange(G) % 3) != 0
    prelude = None

    def schedule(rng, t):
        drop = None
        if name == "same_key":
            keys = ec.same_key(rng, R, G, K)
        elif name == "idle_then_hot":
            keys = ec.idle_then_hot(rng, R, G, K, t, W)
        elif name == "silent_rows":
            keys = ec.silent_rows(ec.zipf_keys(rng, R, G, K), t, who=1, t0=2, n=3)
        elif name == "isolated_leader":
            keys = ec.zipf_keys(rng, R, G, K, p_propose=0.95)
            if 1 <= t < 4:
                drop = ec.isolated_leader(R, G, who=(t % R), groups=groups)
        elif name == "deaf_acceptor":
            keys = ec.zipf_keys(rng, R, G, K, p_propose=0.95)
            if t % 2 == 0:
                drop = ec.deaf_acceptor(R, G, who=R - 1, groups=groups)
        else:
            keys = ec.zipf_keys(rng, R, G, K)
        return keys, drop
    if name == "lost_replies":
        rng = np.random.default_rng(seed)
        lose = rng.random((3, R, R, G)) < 0.35
        pkeys = [ec.same_key(rng, R, G, K), ec.zipf_keys(rng, R, G, K), ec.same_key(rng, R, G, K)]

        def prelude(sets, orcs):
            for reps in [[ec.NumpyEngine(e, dev) for e in s] for s in sets] + ([orcs] if orcs is not None else []):
                for t in range(3):
                    ec.tick(reps, pkeys[t], via=ec.lost_replies(lambda s, t=t: lose[t, s]))
    return run_fused_vs_driver(dev, G, K, 0.0, T=T, R=R, W=W, oracle=oracle, phase_major=phase_major, seed=seed, schedule=schedule,
                               prelude=prelude, execute=execute, unbatched=unbatched)


# ---- on the device ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("base", sorted(WIDE))
@pytest.mark.parametrize("phase_major", [False, True])
def test_cluster_tick_wide_sequence_numbers(cuda, oracle, base, phase_major):
    run_wide_seq(cuda, oracle, base, G=1000, W=16, phase_major=phase_major)


def test_one_by_one_launch_second_pass_at_size(cuda, oracle):
    """65 536 groups, one key, every replica proposing: more lanes listed at a replica than 1024 blocks x 2 lanes cover in a
    pass, against oracle slices (the first, the last and seeded 512-group slices)"""
    import test_baseline_configs_gpu as tb
    listed = tb.run_epaxos_cluster_slices(cuda, oracle, G=65536, W=16, K=1, T=5, width=512, n_slices=3, phase_major=True,
                                          keys_fn=lambda rng, R, G, K: ec.same_key(rng, R, G, K))
    assert max(listed) > 5 * 2 * 1024, listed


@pytest.mark.parametrize("R,W", [(5, 128), (4, 128)])
def test_cluster_tick_walk_outside_lds(cuda, oracle, R, W):
    run_walk_outside_lds(cuda, oracle, G=1000, R=R, W=W)


@pytest.mark.parametrize("name", SCHEDULES)
def test_cluster_tick_rare_schedules(cuda, oracle, name):
    for execute in (True, False):
        for pm in (False, True):
            run_schedule(cuda, oracle, name, G=1000, execute=execute, phase_major=pm)


@pytest.mark.parametrize("R", [4, 6])
def test_cluster_tick_populations_4_and_6(cuda, oracle, R):
    for pm in (False, True):
        assert run_fused_vs_driver(cuda, 700, 6, 0.15, T=7, R=R, W=16, oracle=oracle, phase_major=pm) > 0
        run_schedule(cuda, oracle, "same_key", G=700, R=R, phase_major=pm)


def test_cluster_tick_phase_major_unbatched(cuda, oracle):
    assert run_fused_vs_driver(cuda, 700, 6, 0.15, oracle=oracle, phase_major=True, unbatched=True) > 0
    run_schedule(cuda, oracle, "same_key", G=700, phase_major=True, unbatched=True)
