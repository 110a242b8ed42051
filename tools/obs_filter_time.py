#!/usr/bin/env python3
"""Time the observation filter (rlks_obs_filter_*, rlks_rollout_filtered).

kernels   apply at one rollout step's size and over a whole (T + 1)-row buffer, stats over a rollout's T N
          rows, at c4's (N = 131,072, D = 6), c3's (65,536, 24) and c5's (16,384, 192) sizes with T = 128:
          each call is captured 16 times into a HIP graph and replayed between device events.  Bytes: apply
          reads and writes 4 B per float, stats reads 4 B per float; the rate is given as a fraction of the
          6.29 TB/s a float4 copy reaches on an MI355X (MI355X_MICROARCH.md).
rollouts  PPO.rollout() of bench.py's c4 and c3 agents (T = 128) with the filter off and on: two agents with
          one seed, alternating legs off, on, off, ... of `--iters` rollouts each between device events after
          `--warmup` rollouts; the on leg includes the stats and merge launches.  Median and spread per flag.
--off-only  only the filter-off legs (one agent): run it with RLKS_LIB pointing at another build of the
          library, an earlier commit's say, to compare the unfiltered rollout across builds.
usage: obs_filter_time.py [--kernels] [--rollouts c4,c3] [--off-only] [--iters K] [--legs L] [--warmup W] -> one JSON line"""
import argparse
import ctypes as C_
import json
import os
import statistics
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT / "rl-k8s-scheduler_amd"))
sys.path.insert(0, str(ROOT))

REPS = 16
HBM_COPY_TBS = 6.29
T = 128
SIZES = {"c4": (131072, 6), "c3": (65536, 24), "c5": (16384, 192)}


def graph_time(torch, call):
    """median / min / max microseconds per call of `call(stream)`, REPS calls per graph replay"""
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
        times.append(s.elapsed_time(e) / REPS * 1e3)
    return sorted(times)[len(times) // 2], min(times), max(times)


def rate(us, nbytes):
    med, lo, hi = us
    return {"us_per_call": round(med, 2), "us_min_max": [round(lo, 2), round(hi, 2)], "bytes": nbytes,
            "TBs": round(nbytes / med / 1e6, 3), "frac_of_hbm_copy_rate": round(nbytes / med / 1e6 / HBM_COPY_TBS, 3)}


def kernel_times(torch, _lib, dev, N, D):
    from rlks.obs_filter import ObsFilter

    g = torch.Generator(device=dev).manual_seed(1)
    raw = torch.rand(T + 1, N, D, generator=g, dtype=torch.float32, device=dev)
    out = torch.empty_like(raw)
    f = ObsFilter(D, dev)
    f.reserve((T + 1) * N)
    f.stats(raw[0])
    f.merge()  # a state that is not the identity
    S, R, W = f.state.data_ptr(), f.record.data_ptr(), f.ws.data_ptr()

    def apply(rows, x, y):
        return lambda cs: _lib.call("rlks_obs_filter_apply", S, x.data_ptr(), y.data_ptr(), rows, D, cs)

    def stats(rows, x):
        return lambda cs: _lib.call("rlks_obs_filter_stats", S, x.data_ptr(), rows, D, R, W, f.ws.numel() * 8, cs)

    res = {"N": N, "D": D, "T": T,
           "apply_one_step": rate(graph_time(torch, apply(N, raw[1], out[1])), N * D * 8),
           "apply_whole_buffer": rate(graph_time(torch, apply((T + 1) * N, raw, out)), (T + 1) * N * D * 8),
           "stats_rollout": rate(graph_time(torch, stats(T * N, raw[1:])), T * N * D * 4),
           "merge": {"us_per_call": round(graph_time(torch, lambda cs: _lib.call("rlks_obs_filter_merge", S, R, D, cs))[0], 2)}}
    res["per_rollout_us"] = round((T + 1) * res["apply_one_step"]["us_per_call"] + res["stats_rollout"]["us_per_call"]
                                  + res["merge"]["us_per_call"], 1)
    return res


def make_agent(torch, dev, config, filtered):
    from bench import CONFIGS, env_setup
    from rlks.ppo import PPO, PPOConfig

    p = CONFIGS[config]
    table, nodes = env_setup(config)
    cfg = (PPOConfig().environment("K8sMultiCloudEnv").framework("torch")
           .training(train_batch_size=p["envs"] * T, sgd_minibatch_size=p["minibatch"], num_sgd_iter=1, lr=3e-4,
                     gamma=0.99, model={"fcnet_hiddens": [p["hidden"]] * 2})
           .debugging(seed=42))
    if filtered:
        cfg.rollouts(observation_filter="MeanStdFilter")
    cfg.num_envs = p["envs"]
    cfg.rollout_fragment_length = T
    cfg.table, cfg.nodes = table, nodes
    return PPO(config=cfg, device=dev)


def rollout_legs(torch, dev, config, flags, iters, warmup, n_legs):
    agents = {f: make_agent(torch, dev, config, f == "on") for f in set(flags)}
    for a in agents.values():
        for _ in range(warmup):
            a.rollout(explore=True)
    torch.cuda.synchronize()
    legs = []
    for k in range(n_legs):
        name = flags[k % len(flags)]
        s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        s.record()
        for _ in range(iters):
            agents[name].rollout(explore=True)
        e.record()
        torch.cuda.synchronize()
        legs.append({"filter": name, "ms_per_rollout": round(s.elapsed_time(e) / iters, 3)})
    out = {"lanes": agents[flags[0]].N, "T": T, "D": agents[flags[0]].D, "precision": agents[flags[0]].precision,
           "iters_per_leg": iters, "legs": legs}
    for f in set(flags):
        ms = [l["ms_per_rollout"] for l in legs if l["filter"] == f]
        out[f] = {"median_ms": round(statistics.median(ms), 3), "min_max_ms": [min(ms), max(ms)]}
    if "on" in out and "off" in out:
        out["on_minus_off_ms"] = round(out["on"]["median_ms"] - out["off"]["median_ms"], 3)
        out["raw_buffer_bytes"] = (T + 1) * out["lanes"] * out["D"] * 4
    for a in agents.values():
        a.stop()
    return out


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--kernels", action="store_true")
    ap.add_argument("--rollouts", default="", help="comma-separated bench configs, e.g. c4,c3")
    ap.add_argument("--off-only", action="store_true")
    ap.add_argument("--iters", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--legs", type=int, default=7)
    args = ap.parse_args()
    import torch

    from rlks import _lib

    if not torch.cuda.is_available():
        raise SystemExit("obs_filter_time.py needs a HIP device")
    if "RLKS_LIB" in os.environ and args.off_only:
        # another build's library may predate the filter: its entry points are not needed for the off legs
        _lib._OPTIONAL |= {n for n in _lib.SIGNATURES if "obs_filter" in n or n == "rlks_rollout_filtered"}
    dev = torch.device("cuda", 0)
    res = {"launches_per_graph": REPS, "lib": Path(os.environ.get("RLKS_LIB", "librlks.so")).name}
    if args.kernels:
        res["kernel"] = {k: kernel_times(torch, _lib, dev, *v) for k, v in SIZES.items()}
    flags = ["off"] if args.off_only else ["off", "on"]
    for config in [c for c in args.rollouts.split(",") if c]:
        res[f"rollout_{config}"] = rollout_legs(torch, dev, config, flags, args.iters, args.warmup,
                                                args.legs if args.off_only else args.legs | 1)
    print(json.dumps(res))
