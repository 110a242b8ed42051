#!/usr/bin/env python3
"""Time the action-mask kernels (rlks_env_action_mask, rlks_env_masked_sample) at c3's size
(65,536 envs x 8 clusters x 256 nodes) beside the "myopic_with_room" rule kernel and the two forms of a
rollout's sample + step, in one process: each is captured 64 times into a HIP graph and replayed between
device events, as tools/rule_kernel_time.py times the rule kernels.  With --rollout: also c3's rollout
(bench.py's PPO at 65,536 lanes, T steps) with action_mask="room" against None, alternating.
usage: action_mask_time.py [n_envs] [--rollout T]   -> one JSON line"""
import json
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT / "rl-k8s-scheduler_amd"))
sys.path.insert(0, str(ROOT))

REPS = 64

if __name__ == "__main__":
    import torch

    from rlks import VecK8sMultiCloudEnv, _lib
    from rlks.env import NodeSpec
    from rlks.tables import synthetic_table

    argv = sys.argv[1:]
    T = 0
    if "--rollout" in argv:
        i = argv.index("--rollout")
        T = int(argv[i + 1])
        del argv[i:i + 2]
    n, C, nodes = (int(argv[0]) if argv else 65536), 8, 256
    dev = torch.device("cuda", 0)
    spec = NodeSpec(C, nodes, arrival_rate=1.0, depart_prob="stationary", init_occupancy=0.5)
    venv = VecK8sMultiCloudEnv(n, table=synthetic_table(C, 100, seed=42), seed=42, nodes=spec, device=dev)
    venv.reset()
    acts = [torch.randint(0, C, (n,), dtype=torch.int32, device=dev) for _ in range(8)]
    out = torch.zeros(n, dtype=torch.int32, device=dev)
    logp = torch.zeros(n, dtype=torch.float32, device=dev)
    rew = torch.zeros(n, dtype=torch.float32, device=dev)
    done = torch.zeros(n, dtype=torch.uint8, device=dev)
    bits = torch.zeros(n, dtype=torch.int64, device=dev)
    logits = [torch.randn(n, C, device=dev) for _ in range(8)]
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

    res = {"n_envs": n, "clusters": C, "nodes": nodes, "launches_per_graph": REPS}
    # the kernels that do not step first: they leave the env in the state the warm-up steps gave it
    g = graph(lambda t, cs: _lib.call("rlks_env_rule_actions", venv.handle, _lib.RLKS_RULE_MYOPIC_WITH_ROOM,
                                      venv.obs.data_ptr(), out.data_ptr(), cs))
    res["rule_myopic_with_room_us"] = round(timed(g), 2)
    g = graph(lambda t, cs: _lib.call("rlks_env_action_mask", venv.handle, bits.data_ptr(), cs))
    res["action_mask_us"] = round(timed(g), 2)
    g = graph(lambda t, cs: _lib.call("rlks_env_masked_sample", venv.handle, logits[t % 8].data_ptr(), 1, out.data_ptr(),
                                      logp.data_ptr(), None, cs))
    res["masked_sample_us"] = round(timed(g), 2)
    res["full_lanes"] = int((~venv.action_mask().all(1)).sum())

    def masked_step(t, cs):
        _lib.call("rlks_env_masked_sample", venv.handle, logits[t % 8].data_ptr(), 1, out.data_ptr(), logp.data_ptr(), None, cs)
        _lib.call("rlks_env_step", venv.handle, out.data_ptr(), venv.obs.data_ptr(), None, rew.data_ptr(), done.data_ptr(),
                  None, None, None, None, cs)

    g = graph(masked_step)
    res["masked_sample_then_step_us"] = round(timed(g), 2)
    g = graph(lambda t, cs: _lib.call("rlks_env_sample_step", venv.handle, logits[t % 8].data_ptr(), 1, out.data_ptr(),
                                      logp.data_ptr(), venv.obs.data_ptr(), rew.data_ptr(), done.data_ptr(), cs))
    res["sample_step_us"] = round(timed(g), 2)
    venv.close()

    if T > 0:
        from bench import CONFIGS, env_setup
        from rlks.ppo import PPO, PPOConfig

        preset = CONFIGS["c3"]
        table, nspec = env_setup("c3")
        algos = {}
        for mask in (None, "room"):
            cfg = (PPOConfig().framework("torch")
                   .training(train_batch_size=n * T, sgd_minibatch_size=min(preset["minibatch"], n * T), num_sgd_iter=1,
                             lr=3e-4, action_mask=mask, model={"fcnet_hiddens": [preset["hidden"]] * 2})
                   .debugging(seed=42))
            cfg.num_envs, cfg.rollout_fragment_length, cfg.table, cfg.nodes = n, T, table, nspec
            algos[mask] = PPO(config=cfg, device=dev)
        ms = {None: [], "room": []}
        for rep in range(5):  # (the first pair is the warm-up)
            for mask, algo in algos.items():
                s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                s.record()
                algo.rollout(explore=True)
                e.record()
                torch.cuda.synchronize()
                if rep:
                    ms[mask].append(s.elapsed_time(e))
        res["rollout"] = {"T": T, "unmasked_ms": [round(x, 2) for x in ms[None]], "masked_ms": [round(x, 2) for x in ms["room"]]}
    print(json.dumps(res))
