"""the default workload (as tools/pmc_probe.py drives it), 64 ticks in batches of 8: share of the side launch's group-ticks that took the steady step"""
import os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from summerset_amd import workloads
dev = torch.device("cuda")
G, R, S, W, H, T = 65536, 5, 32, 512, 4, 64
eng = workloads.headline_cluster(G, W=W, R=R, straggler_ticks=4)
st = workloads.headline_stream(G, T, 0.01, T, S=S, W=W, R=R, H=H)
pool = [{k: torch.from_numpy(v).to(dev) for k, v in st.tick(t).items() if k in ("req_cnt", "req_val", "ackctl")} for t in range(4)]
def tick_args(t):
    e = {k: torch.from_numpy(v).to(dev) for k, v in st.tick_events(t).items()}
    fired = bool((st.timeout_tick == t).any())
    return dict(timeout_rep=e["timeout_rep"] if fired else None, timeout_src=e["timeout_src"] if fired else None, req_target=e["req_target"],
                heartbeat=st.heartbeat(t), **pool[t % 4])
workloads.drive_headline(eng, tick_args, 0, T, batch=8)
torch.cuda.synchronize()
a, b = eng.debug_side_steps()
print("side group-ticks: steady step %d, round bodies %d, share %.3f" % (a, b, a / max(a + b, 1)))
