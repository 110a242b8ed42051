#!/usr/bin/env python3
"""Time the baseline-scheduler kernel (rlks_env_rule_actions) at c3's size (65,536 envs x
8 clusters x 256 nodes) beside the node step it runs ahead of, in one process: each is captured 64 times
into a HIP graph and replayed between device events, as bench.py's k_node_step leg times the step.
usage: rule_kernel_time.py [n_envs]   -> one JSON line"""
import json
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT / "rl-k8s-scheduler_amd"))

REPS = 64

if __name__ == "__main__":
    import torch

    from rlks import VecK8sMultiCloudEnv, _lib
    from rlks.env import NodeSpec
    from rlks.tables import synthetic_table

    n, C, nodes = (int(sys.argv[1]) if len(sys.argv) > 1 else 65536), 8, 256
    dev = torch.device("cuda", 0)
    spec = NodeSpec(C, nodes, arrival_rate=1.0, depart_prob="stationary", init_occupancy=0.5)
    venv = VecK8sMultiCloudEnv(n, table=synthetic_table(C, 100, seed=42), seed=42, nodes=spec, device=dev)
    venv.reset()
    acts = [torch.randint(0, C, (n,), dtype=torch.int32, device=dev) for _ in range(8)]
    out = torch.zeros(n, dtype=torch.int32, device=dev)
    for t in range(60):  # away from the reset state, as bench.py
        venv.step(acts[t % 8])
    venv.check_status()
    torch.cuda.synchronize()

    def graph(fn):
        g = torch.cuda.CUDAGraph()
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            with torch.cuda.graph(g, stream=side):
                cs = torch.cuda.current_stream().cuda_stream
                for t in range(REPS):
                    fn(t, cs)
        torch.cuda.synchronize()
        return g

    def timed(g, reps=5):
        g.replay()
        torch.cuda.synchronize()
        s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        s.record()
        for _ in range(reps):
            g.replay()
        e.record()
        torch.cuda.synchronize()
        return s.elapsed_time(e) / reps / REPS * 1e3  # us per launch

    res = {"n_envs": n, "clusters": C, "nodes": nodes, "launches_per_graph": REPS, "rule_us": {}}
    # the rules first: they leave the env in the state the warm-up steps gave it
    for name, rule in _lib.RULES.items():
        g = graph(lambda t, cs: _lib.call("rlks_env_rule_actions", venv.handle, rule, venv.obs.data_ptr(),
                                          out.data_ptr(), cs))
        res["rule_us"][name] = round(timed(g), 2)
    g = graph(lambda t, cs: _lib.call("rlks_env_step", venv.handle, acts[t % 8].data_ptr(), venv.obs.data_ptr(),
                                      venv.reward.data_ptr(), None, venv.terminated.data_ptr(), None, None, None,
                                      None, cs))
    res["node_step_us"] = round(timed(g), 2)
    print(json.dumps(res))
