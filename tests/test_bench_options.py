"""bench.py's own options on CPU: a plain run times exactly --steps ticks and measures nothing else, --full keeps the rest, the
tick events it makes resident are the stream's own, and --dump-outputs writes the engine's state (the emulator standing in for
the device)."""
import os
import sys

import numpy as np
import pytest


def _args(monkeypatch, *argv):
    import bench
    monkeypatch.setattr(sys, "argv", ["bench.py"] + list(argv))
    return bench.parse()


def test_plain_run_times_exactly_steps(monkeypatch):
    import bench
    a = _args(monkeypatch, "--gpus", "1", "--steps", "20", "--warmup", "5")
    assert not a.full and a.dump_outputs is None
    assert bench.timed_regions(a) == 1
    # the workload (its leader changes per tick) is the one --full draws for its nine regions: the plain run is its first region
    f = _args(monkeypatch, "--gpus", "1", "--steps", "20", "--warmup", "5", "--full")
    assert bench.timed_regions(f) == bench.n_regions(f) == 9
    assert bench.timeout_span(a) == bench.timeout_span(f) and bench.timeout_frac(a) == bench.timeout_frac(f)
    assert bench.timed_regions(_args(monkeypatch, "--steps", "60", "--full")) == 3
    assert bench.timed_regions(_args(monkeypatch, "--steps", "60", "--repeats", "5")) == 5
    assert _args(monkeypatch, "--dump-outputs", "out").dump_outputs == "out"


@pytest.mark.parametrize("G,n_ticks,frac,span", [(130, 40, 0.5, 30), (64, 12, 0.0, 72), (200, 25, 1.0, 20)])
def test_resident_events_are_the_streams(G, n_ticks, frac, span):
    import torch
    import bench
    from summerset_amd import workloads
    st = workloads.headline_stream(G, n_ticks, frac, span)
    fired, events = bench.resident_events(torch, st, n_ticks, torch.device("cpu"))
    assert len(fired) == len(events) == n_ticks
    for t in range(n_ticks):
        want = st.tick_events(t)
        assert fired[t] == bool((st.timeout_tick == t).any()), t
        assert events[t]["req_target"].dtype == torch.uint8
        assert np.array_equal(events[t]["req_target"].numpy(), want["req_target"]), t
        if fired[t]:
            for k in ("timeout_rep", "timeout_src"):
                assert events[t][k].dtype == torch.uint8 and np.array_equal(events[t][k].numpy(), want[k]), (t, k)
        else:
            assert events[t]["timeout_rep"] is None and events[t]["timeout_src"] is None
    if frac:
        assert any(fired)


def test_dump_outputs_on_the_emulator(tmp_path, monkeypatch):
    import torch
    import hostsim
    import bench
    from summerset_amd import workloads
    hostsim.build()
    G, W, n_ticks = 130, 16, 10
    with hostsim.patched():
        eng = workloads.headline_cluster(G, W=W)
        st = workloads.headline_stream(G, n_ticks, 0.5, n_ticks, S=4, W=W)
        fired, events = bench.resident_events(torch, st, n_ticks, torch.device("cpu"))
        pool = [{k: torch.from_numpy(v) for k, v in st.tick(t).items() if k in ("req_cnt", "req_val", "ackctl")} for t in range(2)]
        workloads.drive_headline(eng, lambda t: dict(pool[t % 2], heartbeat=st.heartbeat(t), req_target=events[t]["req_target"],
                                                     timeout_rep=events[t]["timeout_rep"], timeout_src=events[t]["timeout_src"]),
                                 0, n_ticks)
        monkeypatch.setattr(bench, "DUMP_BYTES", 1)                  # one block: the sample is seeded, not the first block
        one = bench.dump_outputs(eng, str(tmp_path / "one"))
        monkeypatch.setattr(bench, "DUMP_BYTES", 48 << 20)
        out = str(tmp_path / "all")
        arrays = bench.dump_outputs(eng, out, group_base=1000)
        states = [eng.dump(r) for r in range(eng.R)]
        counters = [eng.counters(r) for r in range(eng.R)]
        eng.close()
    files = sorted(os.listdir(out))
    assert files == sorted(k + ".npy" for k in arrays) and "counters.npy" in files and "sample_groups.npy" in files
    assert sum(os.path.getsize(os.path.join(out, f)) for f in files) < 64 << 20
    for f in files:
        a = np.load(os.path.join(out, f))
        assert a.dtype in (np.float32, np.float64) and np.array_equal(a, arrays[f[:-4]]), f
    assert np.array_equal(arrays["sample_groups"], np.arange(G) + 1000.0)      # every block fits: all 130 groups, in order
    assert arrays["counters"].tolist() == [[c["commits"], c["redirects"], c["rejects"]] for c in counters]
    assert arrays["counters"][:, 0].sum() > 0
    for name, a in arrays.items():
        if name in ("counters", "sample_groups"):
            continue
        assert a.shape[0] == 5 and a.shape[-1] == G, name
        for r in range(5):
            assert np.array_equal(a[r], states[r][name].astype(a.dtype)), (name, r)
    g = one["sample_groups"].astype(int)
    assert len(g) in (64, 2) and g[0] % 64 == 0
    assert np.array_equal(one["commit_bar"], arrays["commit_bar"][..., g])
