#!/usr/bin/env python3
"""Time the rollout-metrics reduction (rlks_rollout_metrics) on synthetic rollout buffers
at c4's (T = 128, N = 131,072, A = C = 2) and c3's (N = 65,536, A = C = 8) sizes: the two launches
are captured 16 times into a HIP graph and replayed between device events.  Per size: the time per call
and the bytes the kernel must read over that time, as a fraction of the 6.29 TB/s a float4 copy
reaches on an MI355X (MI355X_MICROARCH.md).  "Must read" counts 17 B per sample (action, reward, value,
vtarg, done) plus the 4 C bytes of its utilisation columns; the obs rows' other columns share those
columns' cache lines, so the lines fetched are up to 12 C bytes per sample ("line_bytes").
With --train it also times a c4-sized PPO.train_step_no_sync with the flag off, on, off, on, off
(`--legs` of them, `--iters` iterations per leg after `--warmup`), so that drift between the off legs shows: two agents
with one seed, and then one agent (the flag-on one, its metrics launch skipped in the off legs), which
takes the two agents' different buffers out of the comparison.
usage: rollout_metrics_time.py [--train] [--iters K] [--legs L] [--warmup W]   -> one JSON line"""
import argparse
import ctypes as C_
import json
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT / "rl-k8s-scheduler_amd"))

REPS = 16
HBM_COPY_TBS = 6.29
SIZES = {"c4": (128, 131072, 2, 2), "c3": (128, 65536, 8, 8)}


def kernel_time(torch, _lib, dev, T, N, A, C):
    D = 3 * C
    g = torch.Generator(device=dev).manual_seed(1)
    f32 = dict(dtype=torch.float32, device=dev)
    buf = {"obs": torch.rand(T + 1, N, D, generator=g, **f32), "values": torch.randn(T + 1, N, generator=g, **f32),
           "actions": torch.randint(0, A, (T, N), generator=g, dtype=torch.int32, device=dev),
           "rewards": torch.randn(T, N, generator=g, **f32), "vtarg": torch.randn(T, N, generator=g, **f32),
           "dones": (torch.rand(T, N, generator=g, device=dev) < 0.01).to(torch.uint8)}
    bufs = _lib.RolloutBufs(buf["obs"].data_ptr(), None, buf["values"].data_ptr(), buf["actions"].data_ptr(), None,
                            buf["rewards"].data_ptr(), buf["dones"].data_ptr(), None, buf["vtarg"].data_ptr(), T, N, N)
    size = _lib.lib().rlks_rollout_metrics_size(A, C)
    wsb = C_.c_int64()
    _lib.call("rlks_rollout_metrics_workspace_bytes", T, N, A, C, C_.byref(wsb))
    ws = torch.empty(wsb.value // 8, dtype=torch.float64, device=dev)
    out = torch.zeros(size, dtype=torch.float64, device=dev)

    def call(cs):
        _lib.call("rlks_rollout_metrics", C_.byref(bufs), D, A, C, out.data_ptr(), ws.data_ptr(), wsb.value, cs)

    call(None)
    torch.cuda.synchronize()
    gr = torch.cuda.CUDAGraph()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        with torch.cuda.graph(gr, stream=side):
            for _ in range(REPS):
                call(torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    gr.replay()
    torch.cuda.synchronize()
    times = []
    for _ in range(5):
        s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        s.record()
        gr.replay()
        e.record()
        torch.cuda.synchronize()
        times.append(s.elapsed_time(e) / REPS * 1e3)  # us per call
    us = sorted(times)[len(times) // 2]
    n = T * N
    must, lines = n * (17 + 4 * C), n * (17 + 12 * C)
    return {"T": T, "N": N, "A": A, "C": C, "us_per_call": round(us, 2), "us_min_max": [round(min(times), 2), round(max(times), 2)],
            "must_read_bytes": must, "must_read_TBs": round(must / us / 1e6, 3),
            "frac_of_hbm_copy_rate": round(must / us / 1e6 / HBM_COPY_TBS, 3),
            "line_bytes": lines, "line_TBs": round(lines / us / 1e6, 3),
            "reward_sum": float(out[_lib.RLKS_RM_REWARD_SUM].item())}


def train_ab(torch, dev, iters, warmup, n_legs):
    """c4-sized train_step_no_sync (bench.py's c4: 131,072 lanes, T = 128, 65,536-row minibatches, 10
    epochs), flag off / on, alternating legs"""
    from rlks.ppo import PPO, PPOConfig

    envs, T, mb = 131072, 128, 65536

    def make(flag):
        cfg = (PPOConfig().environment("K8sMultiCloudEnv").framework("torch")
               .training(train_batch_size=envs * T, sgd_minibatch_size=mb, num_sgd_iter=10, lr=3e-4, gamma=0.99)
               .debugging(seed=42).reporting(rollout_metrics=flag))
        cfg.num_envs = envs
        cfg.rollout_fragment_length = T
        return PPO(config=cfg, device=dev)

    agents = {"off": make(False), "on": make(True)}
    for a in agents.values():
        for _ in range(warmup):
            a.train_step_no_sync()
    torch.cuda.synchronize()

    def legs_of(agent_of):
        legs = []
        for name in ["off" if k % 2 == 0 else "on" for k in range(n_legs)]:
            a, rm_out = agent_of(name), agents["on"].rm_out
            if a is agents["on"] and name == "off":
                a.rm_out = None  # the same agent and buffers, the metrics launch skipped
            s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            s.record()
            for _ in range(iters):
                a.train_step_no_sync()
            e.record()
            torch.cuda.synchronize()
            agents["on"].rm_out = rm_out
            legs.append({"flag": name, "ms_per_iteration": round(s.elapsed_time(e) / iters, 3)})
        off = [l["ms_per_iteration"] for l in legs if l["flag"] == "off"]
        on = [l["ms_per_iteration"] for l in legs if l["flag"] == "on"]
        ms = [l["ms_per_iteration"] for l in legs]
        # each on leg against the mean of the off legs before and after it: drift that is linear cancels
        nb = [round(ms[k] - (ms[k - 1] + ms[k + 1]) / 2, 3) for k in range(1, n_legs - 1, 2)]
        return {"legs": legs, "off_spread_ms": round(max(off) - min(off), 3),
                "on_minus_off_ms": round(sum(on) / len(on) - sum(off) / len(off), 3),
                "on_minus_neighbouring_off_ms": nb, "mean_of_those_ms": round(sum(nb) / len(nb), 3)}

    return {"lanes": envs, "T": T, "minibatch": mb, "iters_per_leg": iters,
            "two_agents": legs_of(lambda name: agents[name]), "one_agent": legs_of(lambda name: agents["on"])}


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--train", action="store_true")
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--legs", type=int, default=5, help="alternating off / on legs, odd: off first and last")
    args = ap.parse_args()
    import torch

    from rlks import _lib

    if not torch.cuda.is_available():
        raise SystemExit("rollout_metrics_time.py needs a HIP device")
    dev = torch.device("cuda", 0)
    res = {"launches_per_graph": REPS, "kernel": {k: kernel_time(torch, _lib, dev, *v) for k, v in SIZES.items()}}
    if args.train:
        res["train_step_c4"] = train_ab(torch, dev, args.iters, args.warmup, args.legs | 1)
    print(json.dumps(res))
