#!/usr/bin/env python3
"""Throughput benchmark: env-steps/s of batched rollout + PPO policy update (BASELINE.json metric).

Workload (default "c4" = BASELINE.json configs[3], the config the metric's 1/2/4/8-GPU curve is
quoted on): per GPU 131,072 envs on the reference 2-cloud price/latency table (1,048,576 at 8
GPUs), T = 128 rollout steps per iteration (16.8M env-steps per GPU), GAE, then 10 SGD epochs of
65,536-row minibatches (256 per epoch) of RLlib's default PPO (FCNet [256, 256] tanh, separate
value net, Adam lr 3e-4, gamma 0.99).  A "step" is one full PPO iteration.  Synthetic data (the
env itself generates it); random-init weights; fp32-accurate arithmetic throughout.

  python bench.py --gpus N --steps K --warmup W [--config c2|c3|c4|c5] [--dump-outputs DIR] [--full]
  (--config picks another BASELINE.json workload — c2: 4,096 envs/GPU (configs[1]); c3: 65,536
   node-level envs x 8 clusters x 256 nodes; c5: 64 x 1,024 nodes with the Locust-fitted MMPP
   arrivals and the [2048, 2048] policy on the generic-width path; the default is c4)
  (N > 1: one rank per GPU over RCCL.  Either launched by torch.distributed.run (WORLD_SIZE set,
   and it must equal --gpus), or, with no launcher, this script starts the N ranks itself as child
   processes (launch_ranks) and exits with the worst rank's status.
   --scaling weak (default): every rank owns the config's per-GPU lanes and minibatch (c4: 131,072
   lanes and 65,536 rows; 1,048,576 lanes at 8 GPUs).  --scaling strong: the whole job's work is
   fixed at 8x the per-GPU figures (c4: 1,048,576 lanes, a 524,288-row global minibatch) and each
   of the N ranks owns 1/N of it, so one PPO iteration is the same computation at every N.)

Prints ONE JSON line on rank 0.  A plain run sets up, warms up, times the K steps and prints the line
(value, ms_per_step, config, finite); roofline, cpu_baseline, allreduce and kernels are null.
--dump-outputs DIR: after the timed steps, rank 0 writes what the last timed step left for its caller
(parameters, Adam moments, learner stats, the rollout and advantage buffers) as DIR/<name>.npy
(dump_outputs).  The seeds are fixed, so two runs with the same arguments start from identical inputs.
--full: also measures, with HIP events on the launch stream, the average duration of each kernel of
the SGD step (roofline of the dominant one), of the env step kernel and of the GAE scan, profiles the
gradient all-reduce (multi-rank), and times the CPU port (oracle/cpu_ppo.py) on the host cores as
cpu_baseline; --no-kernel-timing / --no-cpu-baseline drop a leg of it.
"""
from __future__ import annotations

import argparse
import ctypes as C
import json
import os
import sys
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent
sys.path.insert(0, str(ROOT / "rl-k8s-scheduler_amd"))

HBM_PEAK_GBS = 8000.0          # MI355X HBM3E spec (MI355X_MICROARCH.md)
FP32_MFMA_PEAK_TFLOPS = 157.3  # v_mfma_f32_32x32x2_f32 dense peak (MI355X_MICROARCH.md)
F16_MFMA_PEAK_TFLOPS = 2500.0  # dense fp16/bf16 MFMA peak (MI355X_MICROARCH.md)
# split-fp16: every fp32-accurate product is three f16 MFMA products, so the ceiling for the
# algorithmic (fp32) FLOPs is a third of the f16 peak
SF16_PEAK_TFLOPS = F16_MFMA_PEAK_TFLOPS / 3



def flops_per_row(name, D=6, H=256, A=2):
    """algorithmic (fp32) FLOPs per minibatch row of each SGD-step kernel, both nets"""
    fwd = lambda An: 2 * (D * H + H * H + H * An)  # noqa: E731  per net forward
    head = lambda An: 4 * H * An                    # noqa: E731  head backward: dout W3 and dW3
    return {
        "k_fwd_head_pi": fwd(A) + head(A),
        "k_fwd_head_vf": fwd(1) + head(1),
        "k_dw2": 2 * 2 * H * H,                     # dW2 = dZ2^T H1, both nets
        "k_dh1": 2 * 2 * H * H + 2 * 2 * D * H,     # dH1 = dZ2 W2 and dW1 = dZ1^T X, both nets
        # split-fp16 F1 (sgd_sf16.hip) as two kernels: forward + head backward (F1a), dH1 = dZ2 W2 +
        # dW1 = dZ1^T X (F1b); f1_total is the pair
        "f1_total": sum(fwd(An) + head(An) + 2 * H * H + 2 * D * H for An in (A, 1)),
        "k_sf_f1": sum(fwd(An) + head(An) + 2 * H * H + 2 * D * H for An in (A, 1)),  # fused F1 = F1a + F1b
        "k_sf_fwd": sum(fwd(An) + head(An) for An in (A, 1)),
        "k_sf_bwd": 2 * (2 * H * H + 2 * D * H),
        "k_sf_dw2": 2 * 2 * H * H,                  # dW2 = dZ2^T H1, both nets
        # generic-width path (wide_mlp.hip): the whole gradient (forward, head, dW2, dH1, dW1), both nets
        "wide_grad": sum(fwd(An) + head(An) + 4 * H * H + 2 * D * H for An in (A, 1)),
    }[name]


# BASELINE.json configs; "c1" is the reference's single-env CPU plumbing case
CONFIGS = {
    "c2": dict(envs=4096, clusters=2, nodes=0, hidden=256, minibatch=65536,
               text="c2: 4,096 envs/GPU x 2-cloud table, T=128 rollout + GAE + PPO update "
                    "(10 epochs x 8 minibatches of 65,536 rows/GPU, FCNet [256,256] tanh)",
               cpu=dict(n_envs=4096, T=128, minibatch=65536)),
    "c3": dict(envs=65536, clusters=8, nodes=256, hidden=256, minibatch=65536, arrivals="poisson",
               text="c3: 65,536 envs/GPU x 8 clusters x 256 nodes (Poisson(1) arrivals, first-fit, stationary "
                    "departures), T=128 rollout + GAE + PPO update (10 epochs x 128 minibatches of 65,536 rows, "
                    "FCNet [256,256] tanh, obs 24, 8 actions)",
               cpu=dict(n_envs=4096, T=32, minibatch=65536)),
    "c4": dict(envs=131072, clusters=2, nodes=0, hidden=256, minibatch=65536,
               text="c4: 131,072 envs/GPU (1,048,576 over 8 GPUs) x 2-cloud table, T=128 rollout + GAE + PPO "
                    "update (10 epochs x 256 minibatches of 65,536 rows/GPU, FCNet [256,256] tanh)",
               cpu=dict(n_envs=4096, T=128, minibatch=65536)),
    "c5": dict(envs=16384, clusters=64, nodes=1024, hidden=2048, minibatch=65536, arrivals="bursty",
               text="c5: 16,384 envs/GPU x 64 clusters x 1,024 nodes (bursty Locust-shaped arrivals, first-fit), "
                    "T=128 rollout + GAE + PPO update (10 epochs x 32 minibatches of 65,536 rows, FCNet "
                    "[2048,2048] tanh, obs 192, 64 actions)",
               cpu=dict(n_envs=256, T=16, minibatch=4096)),
}


def env_setup(name):
    """(table, NodeSpec or None) of a config"""
    from rlks.env import NodeSpec, bursty_trace
    from rlks.tables import load_table, synthetic_table

    c = CONFIGS[name]
    if not c["nodes"]:
        return load_table(), None
    tab = synthetic_table(c["clusters"], 100, seed=42)
    trace = bursty_trace() if c.get("arrivals") == "bursty" else None
    return tab, NodeSpec(c["clusters"], c["nodes"], arrival_rate=1.0, arrival_trace=trace, depart_prob="stationary",
                         init_occupancy=0.5)


ROOFLINE_KERNELS = ("k_fwd_head_pi", "k_fwd_head_vf", "k_dw2", "k_dh1", "k_sf_f1", "k_sf_fwd", "k_sf_bwd", "k_sf_dw2",
                    "wide_grad")


def algo_bytes_per_launch(name, rows, D=6, H=256, A=2):
    """algorithmic HBM bytes of one launch of a split-fp16 SGD kernel over `rows` minibatch rows
    (DESIGN.md "Algorithmic bytes"): only the step's own inputs the kernel must read, each once --
    F1a the row's record (fp32, mb_stride floats; both nets use the same bytes), F1b and F2 its obs
    columns (D floats).  The dZ2 hand-off F1a writes and F1b / F2 read back, the per-block weight-
    gradient partials and the weights (< 0.5 MB) are not algorithmic: they are the overhead
    traffic_over_algorithmic exposes."""
    rec = (D + A + 4 + 3) // 4 * 4 * 4
    per_row = {"k_sf_f1": rec, "k_sf_fwd": rec, "k_sf_bwd": 4 * D, "k_sf_dw2": 4 * D}.get(name)
    return None if per_row is None else per_row * rows


ENV_BYTES_PER_STEP = 4 + 8 + 24 + 4 + 1  # action, step r/w, obs, reward, done
# what the 2-cloud step kernel must move per env-step: action 4, step r/w 8, episode 4 (Philox
# counter), obs 24, reward 8 (the reference's float64), terminated 1
ENV_STEP_BYTES = 4 + 8 + 4 + 24 + 8 + 1
GAE_BYTES_PER_STEP = 17                  # r, V, done in; A, vtarg out


def parse():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--config", default="c4", choices=sorted(CONFIGS), help="BASELINE.json workload")
    ap.add_argument("--envs", type=int, default=None, help="lanes per GPU (default: the config's)")
    ap.add_argument("--rollout", type=int, default=128)
    ap.add_argument("--minibatch", type=int, default=None, help="rows per GPU per SGD step (default: the config's)")
    ap.add_argument("--epochs", type=int, default=10)
    ap.add_argument("--full", action="store_true",
                    help="after the timed steps also measure the per-kernel / roofline figures, the multi-rank "
                         "all-reduce profile and the CPU baseline (runs of their own; off by default)")
    ap.add_argument("--no-cpu-baseline", action="store_true", help="with --full: skip the CPU baseline")
    ap.add_argument("--no-kernel-timing", action="store_true", help="with --full: skip the kernel timings and roofline")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="write the last timed step's outputs as DIR/<name>.npy (rank 0; see dump_outputs)")
    ap.add_argument("--precision", default="auto", choices=("auto", "sf16", "fp32", "f16"),
                    help="SGD-step matrix arithmetic (f16: one-product throughput mode, below fp32: a secondary line)")
    ap.add_argument("--scaling", default="weak", choices=("weak", "strong"),
                    help="weak: per-GPU work fixed as N grows; strong: whole-job work fixed (8x the per-GPU config)")
    ap.add_argument("--dry-run", action="store_true",
                    help="launcher / rendezvous / timing plumbing only: every rank times an empty step on the "
                         "CPU (gloo) and rank 0 prints the JSON line; no GPU is touched (the launcher's CPU test)")
    return ap.parse_args()


STRONG_FACTOR = 8  # --scaling strong: the whole job = 8 x the config's per-GPU lanes and minibatch rows


def shard_sizes(args, preset, world):
    """(lanes, minibatch rows) per rank.  weak: the config's per-GPU figures (or --envs /
    --minibatch), whatever the world size.  strong: those figures x STRONG_FACTOR for the whole job
    (or --envs / --minibatch as whole-job totals), split evenly over the ranks."""
    envs = args.envs or preset["envs"]
    mb = args.minibatch or preset["minibatch"]
    if args.scaling == "weak":
        return envs, mb
    tot_envs = args.envs or STRONG_FACTOR * preset["envs"]
    tot_mb = args.minibatch or STRONG_FACTOR * preset["minibatch"]
    if tot_envs % world or tot_mb % world:
        raise SystemExit(f"--scaling strong: {tot_envs} lanes / {tot_mb} minibatch rows do not split over {world} ranks")
    return tot_envs // world, tot_mb // world


def _free_port():
    import socket

    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    return port


def visible_gpus():
    """GPUs this process may use, counted without any HIP call (the launcher parent must stay
    HIP-free: torch.cuda.device_count() falls back to hipGetDeviceCount, which initialises HIP, when
    amdsmi is unavailable).  A *_VISIBLE_DEVICES list, if set, is the count; otherwise the KFD topology's
    GPU nodes (gpu_id != 0) in sysfs.  None when neither says: the ranks then check for themselves."""
    for var in ("ROCR_VISIBLE_DEVICES", "HIP_VISIBLE_DEVICES", "CUDA_VISIBLE_DEVICES"):
        v = os.environ.get(var)
        if v is not None:
            return len([x for x in v.split(",") if x.strip() != ""])
    nodes = Path("/sys/class/kfd/kfd/topology/nodes")
    try:
        ids = [(d / "gpu_id").read_text().strip() for d in nodes.iterdir() if (d / "gpu_id").exists()]
    except OSError:
        return None
    n = sum(1 for i in ids if i not in ("", "0"))
    return n if ids else None


def launch_ranks(n, argv, timeout=None):
    """`bench.py --gpus N` with no torch.distributed launcher around it: start N fresh child
    processes of this script, one per GPU, with RANK / LOCAL_RANK / WORLD_SIZE / MASTER_ADDR /
    MASTER_PORT set (the contract's torch.distributed.run environment), and return the worst exit
    status.  This process makes no HIP call and does not import torch (a child is started, never
    exec'd: see the GPU box's rules); it counts devices from sysfs (visible_gpus).  When a rank fails,
    the others are stopped at once (they would wait at the next collective until RCCL's watchdog)."""
    import subprocess

    backend = os.environ.get("RLKS_DIST_BACKEND", "nccl")
    if "--dry-run" not in argv and backend == "nccl":
        have = visible_gpus()
        if have is not None and n > have:
            raise SystemExit(f"bench.py --gpus {n}: only {have} GPU(s) visible (RCCL needs one GPU per rank; "
                             "RLKS_DIST_BACKEND=gloo rehearses several ranks on fewer GPUs)")
    port = os.environ.get("MASTER_PORT") or str(_free_port())
    procs = []
    for r in range(n):
        env = dict(os.environ, RANK=str(r), LOCAL_RANK=str(r), WORLD_SIZE=str(n), LOCAL_WORLD_SIZE=str(n),
                   GROUP_RANK="0", MASTER_ADDR="127.0.0.1", MASTER_PORT=port)
        env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")  # RCCL on this pool's host driver (dmabuf IPC)
        procs.append(subprocess.Popen([sys.executable, str(Path(__file__).resolve()), *argv], env=env))
    t0 = time.monotonic()
    worst = 0
    try:
        while True:
            codes = [p.poll() for p in procs]  # every process polled in every pass (a list, not a generator)
            failed = [c for c in codes if c not in (None, 0)]
            if failed:
                worst = failed[0]
                break
            if all(c is not None for c in codes):
                break
            if timeout is not None and time.monotonic() - t0 > timeout:
                worst = 124
                break
            time.sleep(0.2)
    finally:
        for p in procs:
            if p.poll() is None:
                p.terminate()
        for p in procs:
            try:
                p.wait(timeout=30)
            except subprocess.TimeoutExpired:
                p.kill()
                p.wait()
    for p in procs:
        if p.returncode != 0 and worst == 0:
            worst = p.returncode
    return worst if worst >= 0 else 128 - worst


def kernel_timing(algo, torch, config="c2", reps=20):
    """average duration (ms) of each kernel, measured with HIP events on the launch stream"""
    from rlks import _lib

    s = torch.cuda.current_stream()
    out = {}

    def timed(fn, n=reps):
        fn()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(s)
        for _ in range(n):
            fn()
        e1.record(s)
        e1.synchronize()
        return e0.elapsed_time(e1) / n

    desc = C.byref(algo.params.desc)

    def phase(mask):
        return lambda: _lib.call("rlks_ppo_grad_phases", desc, C.byref(algo.coeffs), algo.params.flat.data_ptr(),
                                 algo.dyn.data_ptr(), algo.mbuf.data_ptr(), algo.mb, algo.grad.data_ptr(), None,
                                 algo.ws.data_ptr(), algo.ws.numel(), mask, s.cuda_stream)

    _lib.call("rlks_ppo_gather", desc, C.byref(algo.bufs), 1, 0, 0, algo.mb, algo.dyn.data_ptr(),
              algo.mbuf.data_ptr(), s.cuda_stream)
    D, H, A = algo.D, algo.H, algo.A
    if algo.precision == "wide":
        phases = ()  # generic-width path: one sequence of GEMM launches, timed as a whole below
        peak, peak_name = SF16_PEAK_TFLOPS, "frac_sf16_mfma"
    elif algo.precision in ("sf16", "f16"):
        phase(_lib.RLKS_PHASE_ALL)()  # weight splits + dZ2 in place for the per-phase timings
        # F1 = k_sf_fwd (F1a) + k_sf_bwd (F1b): each timed alone, and the pair
        f1 = (("k_sf_fwd", _lib.RLKS_PHASE_F1A), ("k_sf_bwd", _lib.RLKS_PHASE_F1B),
              ("f1_total", _lib.RLKS_PHASE_FWD_PI | _lib.RLKS_PHASE_FWD_VF))
        phases = (("k_sf_prep", _lib.RLKS_PHASE_PREP), *f1,
                  ("k_sf_dw2", _lib.RLKS_PHASE_DW2), ("k_reduce", _lib.RLKS_PHASE_REDUCE))
        peak, peak_name = SF16_PEAK_TFLOPS, "frac_sf16_mfma"
    else:
        phases = (("k_fwd_head_pi", _lib.RLKS_PHASE_FWD_PI), ("k_fwd_head_vf", _lib.RLKS_PHASE_FWD_VF),
                  ("k_dw2", _lib.RLKS_PHASE_DW2), ("k_dh1", _lib.RLKS_PHASE_DH1), ("k_reduce", _lib.RLKS_PHASE_REDUCE))
        peak, peak_name = FP32_MFMA_PEAK_TFLOPS, "frac_fp32_mfma"
    for name, mask in phases:
        ms = timed(phase(mask))
        rec = {"ms": ms}
        if name in ROOFLINE_KERNELS:
            tf = flops_per_row(name, D, H, A) * algo.mb / (ms * 1e-3) / 1e12
            rec.update({"tflops": tf, peak_name: tf / peak, "frac_fp32_mfma_peak": tf / FP32_MFMA_PEAK_TFLOPS})
        out[name] = rec
    if "f1_total" in out:
        tf = flops_per_row("f1_total", D, H, A) * algo.mb / (out["f1_total"]["ms"] * 1e-3) / 1e12
        out["f1_total"].update({"tflops": tf, peak_name: tf / peak})
        if f1_fused(desc):  # both nets' F1 phases = the fused kernel's launches
            tf = flops_per_row("k_sf_f1", D, H, A) * algo.mb / (out["f1_total"]["ms"] * 1e-3) / 1e12
            out["k_sf_f1"] = {"ms": out["f1_total"]["ms"], "tflops": tf, peak_name: tf / peak,
                              "frac_fp32_mfma_peak": tf / FP32_MFMA_PEAK_TFLOPS}
    if algo.precision in ("sf16", "f16"):
        # in-pipeline: every kernel of full gradients launched back to back as the SGD step runs them,
        # HIP events between the launches (rlks_ppo_grad_profile): the durations rocprofv3 sees, which
        # choose the roofline kernel (isolated repeats of one phase above are diagnostics only)
        ms5 = (C.c_double * 6)()
        _lib.call("rlks_ppo_grad_profile", desc, C.byref(algo.coeffs), algo.params.flat.data_ptr(), algo.dyn.data_ptr(),
                  algo.mbuf.data_ptr(), algo.mb, algo.grad.data_ptr(), None, algo.ws.data_ptr(), algo.ws.numel(), reps,
                  ms5, s.cuda_stream)
        fused = f1_fused(desc)  # F1 as one kernel (the library's default up to 4 actions)
        f1 = ("k_sf_f1",) if fused else ("k_sf_fwd", "k_sf_bwd")
        pipe = {"k_sf_prep": ms5[0], f1[0]: ms5[1], **({} if fused else {"k_sf_bwd": ms5[2]}),
                "k_sf_dw2": ms5[3], "k_reduce": ms5[4]}
        rec = {"ms": pipe, "event_bracket_ms": ms5[5],
               "method": f"{reps} full rlks_ppo_grad passes, each kernel launched between its own start / stop "
                         "events (hipExtLaunchKernelGGL), less the same bracket's time around an empty kernel"}
        for name in (*f1, "k_sf_dw2"):
            tf = flops_per_row(name, D, H, A) * algo.mb / (pipe[name] * 1e-3) / 1e12
            rec[name] = {"ms": pipe[name], "tflops": tf, peak_name: tf / peak}
        out["pipeline"] = rec
    ms = timed(lambda: _lib.call("rlks_ppo_grad", desc, C.byref(algo.coeffs), algo.params.flat.data_ptr(),
                                 algo.dyn.data_ptr(), algo.mbuf.data_ptr(), algo.mb, algo.grad.data_ptr(), None,
                                 algo.ws.data_ptr(), algo.ws.numel(), s.cuda_stream), n=reps if H <= 256 else 3)
    out["sgd_grad_total"] = {"ms": ms}
    # the per-SGD-step minibatch gather (a new epoch's permutation on every call, so that the
    # rows are not cache-resident from the previous call) and the once-per-iteration record pack
    ep = [100]

    def gather():
        ep[0] += 1
        if algo.packed is not None:
            _lib.call("rlks_ppo_gather_packed", desc, algo.packed.data_ptr(), algo.T, algo.N, 1, ep[0], 1, 0, 0,
                      algo.mb, algo.mbuf.data_ptr(), s.cuda_stream)
        else:
            _lib.call("rlks_ppo_gather", desc, C.byref(algo.bufs), 1, ep[0], 0, algo.mb, algo.dyn.data_ptr(),
                      algo.mbuf.data_ptr(), s.cuda_stream)

    out["k_gather" if algo.packed is None else "k_gather_packed"] = {"ms": timed(gather), "rows": algo.mb}
    if algo.packed is not None:
        out["k_pack"] = {"ms": timed(lambda: _lib.call("rlks_ppo_pack", desc, C.byref(algo.bufs),
                                                       algo.packed.data_ptr(), s.cuda_stream), n=5),
                         "samples": algo.T * algo.N}
    if algo.precision == "wide":
        tf = flops_per_row("wide_grad", D, H, A) * algo.mb / (ms * 1e-3) / 1e12
        out["wide_grad"] = {"ms": ms, "tflops": tf, peak_name: tf / peak, "frac_fp32_mfma_peak": tf / FP32_MFMA_PEAK_TFLOPS}
    b = algo.buf
    N, T = algo.N, algo.T
    if algo.env.cfg.nodes_per_cluster == 0:
        ms = timed(lambda: _lib.call("rlks_env_sample_step", algo.env.handle, b["logits"].data_ptr(), 1,
                                     b["actions"].data_ptr(), b["logp"].data_ptr(), b["obs"][1].data_ptr(),
                                     b["rewards"].data_ptr(), b["dones"].data_ptr(), s.cuda_stream))
        gbs = ENV_BYTES_PER_STEP * N / (ms * 1e-3) / 1e9
        out["k_sample_step"] = {"ms": ms, "GBps": gbs, "frac_hbm": gbs / HBM_PEAK_GBS, "lanes": N}
    ms = timed(lambda: _lib.call("rlks_gae", b["rewards"].data_ptr(), b["values"].data_ptr(), b["dones"].data_ptr(),
                                 0.99, 1.0, T, N, b["adv"].data_ptr(), b["vtarg"].data_ptr(), algo.gae_part.data_ptr(),
                                 s.cuda_stream))
    gbs = GAE_BYTES_PER_STEP * N * T / (ms * 1e-3) / 1e9
    out["k_gae"] = {"ms": ms, "GBps": gbs, "frac_hbm": gbs / HBM_PEAK_GBS}
    ms = timed(lambda: _lib.call("rlks_rollout_ws", algo.env.handle, desc, algo.params.flat.data_ptr(),
                                 C.byref(algo.bufs), 1, algo.ws.data_ptr(), algo.ws.numel(), s.cuda_stream), n=3)
    # both nets' forward of the (T + 1) N visited observations (logits of T N of them)
    flops = (T + 1) * N * (flops_per_row("k_fwd_head_pi", D, H, A) - 4 * H * A
                           + flops_per_row("k_fwd_head_vf", D, H, A) - 4 * H)
    out["rollout"] = {"ms": ms, "env_steps_per_s": T * N / (ms * 1e-3), "tflops": flops / (ms * 1e-3) / 1e12}
    if config == "c3":
        out["k_node_step_c3"] = node_env_timing(algo, torch, timed)
    if config not in ("c2", "c4"):
        return out
    # the standalone env step kernel at a size where HBM, not launch latency, bounds it: the plain
    # gymnasium step contract (trusted actions, no episode-return bookkeeping) through the ABI on
    # preallocated buffers, and VecK8sMultiCloudEnv.step as a whole (status memset + k_validate +
    # step with episode returns, info["step"] and final observations)
    from rlks import VecK8sMultiCloudEnv

    big = 1 << 24
    res = {"lanes": big}
    for track in (False, True):
        venv = VecK8sMultiCloudEnv(big, table=algo.table, seed=1, device=algo.device, track_returns=track)
        venv.reset()
        acts = torch.randint(0, 2, (big,), dtype=torch.int32, device=algo.device)
        if not track:
            ms = timed(lambda: _lib.call("rlks_env_step", venv.handle, acts.data_ptr(), venv.obs.data_ptr(),
                                         venv.reward.data_ptr(), None, venv.terminated.data_ptr(), None, None,
                                         venv.final_obs.data_ptr(), None, s.cuda_stream), n=20)
            alg = ENV_STEP_BYTES * big / (ms * 1e-3) / 1e9
            res.update({"ms": ms, "kernel": "k_env_step2", "bytes_per_step": ENV_STEP_BYTES,
                        "GBps": alg, "frac_hbm": alg / HBM_PEAK_GBS, "env_steps_per_s": big / (ms * 1e-3),
                        "GBps_survey_bytes": ENV_BYTES_PER_STEP * big / (ms * 1e-3) / 1e9})
        else:
            ms = timed(lambda: venv.step(acts), n=10)
            # + ep_ret 8 + 8, step_out 4, the validation pass's action read 4
            moved = ENV_STEP_BYTES + 24
            res["vecenv_step"] = {"ms": ms, "bytes_per_step": moved,
                                  "GBps": moved * big / (ms * 1e-3) / 1e9, "env_steps_per_s": big / (ms * 1e-3)}
        venv.close()
        del venv, acts
    out["k_env_step_16M"] = res
    out["k_node_step_c3"] = node_env_timing(algo, torch, timed)
    out["k_node_step_c3_churn"] = node_env_timing(algo, torch, timed, depart_prob=0.02)
    return out


def node_env_timing(algo, torch, timed, n=65536, C=8, nodes=256, depart_prob="stationary"):
    """BASELINE configs[2]: the node-level step kernel k_node_step (65,536 envs x 8 clusters x 256
    nodes, Poisson(1) arrivals, first-fit, per-pod departures realised as geometric skips:
    "stationary" = arrivals balance departures at the initial occupancy U(0, 50%); a float = that
    per-pod probability).

    Timed as a production driver runs it: ABI steps on preallocated buffers captured once into a
    HIP graph and replayed.  `ms` = the kernel alone (trusted actions: status = NULL);
    `ms_validated` = the full checked step (status memset + k_validate + k_node_step)."""
    from rlks import VecK8sMultiCloudEnv, _lib
    from rlks.env import NodeSpec
    from rlks.tables import synthetic_table

    spec = NodeSpec(C, nodes, arrival_rate=1.0, depart_prob=depart_prob, init_occupancy=0.5)
    venv = VecK8sMultiCloudEnv(n, table=synthetic_table(C, 100, seed=42), seed=42, nodes=spec, device=algo.device)
    venv.reset()
    acts = [torch.randint(0, C, (n,), dtype=torch.int32, device=algo.device) for _ in range(8)]
    for t in range(60):
        venv.step(acts[t % 8])
    venv.counters(enable=1)  # placement / departure statistics from an untimed eager pass
    cnt_steps = 32
    for t in range(cnt_steps):
        venv.step(acts[t % 8])
    cnt = venv.counters(enable=0).cpu().numpy().astype(np.float64) / (cnt_steps * n)  # per env-step
    venv.check_status()
    torch.cuda.synchronize()
    reps = 64

    def graph(checked):
        g = torch.cuda.CUDAGraph()
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            with torch.cuda.graph(g, stream=side):
                cs = torch.cuda.current_stream().cuda_stream
                for t in range(reps):
                    _lib.call("rlks_env_step", venv.handle, acts[t % 8].data_ptr(), venv.obs.data_ptr(),
                              venv.reward.data_ptr(), None, venv.terminated.data_ptr(), venv.truncated.data_ptr(),
                              venv.steps.data_ptr(), venv.final_obs.data_ptr(),
                              venv._status.data_ptr() if checked else None, cs)
        torch.cuda.synchronize()
        g.replay()
        torch.cuda.synchronize()
        return g

    g_kernel, g_checked = graph(False), graph(True)
    ms = timed(g_kernel.replay, n=5) / reps
    ms_checked = timed(g_checked.replay, n=5) / reps
    venv.check_status()
    checks, placed, rejected, departed, written, chunks = cnt
    # algorithmic bytes per env-step: the 8-node chunks the step reads (64 B each: those holding
    # departing pods, the first-fit chunks) and the nodes it writes back (8 B); the chunk pod totals
    # (2 B per chunk: at most a cluster's worth per departure and for the arrivals, and one write per
    # chunk read); used millicores of every cluster 4C (departure draws and obs); obs 12C; action 4,
    # step r/w 8, episode 4, ep_ret r/w 16, reward 8, done 1, trunc 1, step_out 4
    algo_bytes = (64 * chunks + 8 * written + 2 * (nodes // 8) * (departed + 1) + 2 * chunks + 4 * C + 12 * C
                  + 4 + 8 + 4 + 16 + 8 + 1 + 1 + 4)
    gbs = algo_bytes * n / (ms * 1e-3) / 1e9
    # SURVEY.md §8(d)'s per-env-step figure: the chosen cluster's nodes, 256 x 8 B + 8 B + 72 B obs +
    # the 41 B of the table env = 2,169 B at C = 8, N = 256
    survey_bytes = nodes * 8 + 8 + (12 * C - 24) + ENV_BYTES_PER_STEP
    res = {"kernel": "k_node_step", "depart_prob": spec.depart_prob, "ms": ms, "ms_validated": ms_checked, "envs": n, "clusters": C,
           "nodes": nodes, "env_steps_per_s": n / (ms * 1e-3), "env_steps_per_s_validated": n / (ms_checked * 1e-3),
           "node_checks_per_step": checks, "placed_per_step": placed, "rejected_per_step": rejected,
           "departed_per_step": departed, "nodes_written_per_step": written, "chunks_read_per_step": chunks,
           "bytes_per_step": algo_bytes, "GBps": gbs, "frac_hbm": gbs / HBM_PEAK_GBS,
           "survey_bytes_per_step": survey_bytes,
           "survey_bytes_note": "SURVEY §8(d)'s 2,169 B/env-step assumed a sweep of the chosen cluster's nodes; the "
                                "chunk-indexed step does not move those bytes, so no fraction is quoted on them"}
    pmc = pmc_traffic()
    if pmc and "k_node_step" in pmc and (n, C, nodes) == (65536, 8, 256) and depart_prob == "stationary":
        res["traffic"] = pmc["k_node_step"]["hbm_bytes_per_launch"]
        res["traffic_over_algorithmic"] = pmc["k_node_step"]["hbm_bytes_per_launch"] / (algo_bytes * n)
        res["traffic_source"] = pmc["k_node_step"]["source"]
    venv.close()
    return res


def cpu_threads() -> int:
    """host threads for the CPU baseline: the CPUs this process may run on (its affinity mask),
    capped by OMP_NUM_THREADS when set.  The GPU box sets OMP_NUM_THREADS to its per-GPU CPU share
    (16), while os.cpu_count() there reports the whole machine's CPUs, most of them not this job's."""
    n = len(os.sched_getaffinity(0)) if hasattr(os, "sched_getaffinity") else (os.cpu_count() or 1)
    omp = os.environ.get("OMP_NUM_THREADS", "")
    return max(1, min(n, int(omp))) if omp.isdigit() else max(1, n)


def mfma_calibration(torch, sf16_tflops, products=3):
    """what this chip's f16 MFMA pipes sustain on random operands, measured live in this process after
    the timed region (librlks_calib.so: one wave per SIMD on every CU, eight independent accumulators,
    back-to-back issue), for the two shapes the SGD kernels use, against the dominant kernel's f16
    MFMA rate (3 f16 products per fp32-accurate FLOP).  The 2.5 PF spec is not held under dense MFMA
    load on random data (MI355X_MICROARCH.md, DVFS give-back)."""
    lib = C.CDLL(str(ROOT / "rl-k8s-scheduler_amd" / "rlks" / "librlks_calib.so"))
    lib.rlks_calib_mfma_f16.argtypes = [C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p,
                                        C.POINTER(C.c_double)]
    dev = torch.device("cuda", torch.cuda.current_device())
    cus = torch.cuda.get_device_properties(dev).multi_processor_count
    g = torch.Generator(device=dev).manual_seed(11)
    rnd = (torch.rand(1 << 20, generator=g, device=dev) * 2 - 1).to(torch.float16)
    out = torch.empty(cus * 256, device=dev)
    s = torch.cuda.current_stream()
    res = {"cus": cus, "operands": "random fp16 in [-1, 1]"}
    for shape, name in ((0, "mfma_f32_16x16x32_f16"), (1, "mfma_f32_32x32x16_f16")):
        tf = C.c_double()
        rc = lib.rlks_calib_mfma_f16(shape, cus, 10000, 5, rnd.data_ptr(), out.data_ptr(), s.cuda_stream, C.byref(tf))
        res[name + "_tflops"] = tf.value if rc == 0 else None
    sustained = res["mfma_f32_16x16x32_f16_tflops"]
    res["kernel_f16_mfma_tflops"] = products * sf16_tflops
    res["frac_of_sustained_16x16x32"] = products * sf16_tflops / sustained if sustained else None
    res["sf16_ceiling_sustained_tflops"] = sustained / products if sustained else None
    return res


def f1_fused(desc):
    """Whether the library runs a whole split-fp16 gradient's F1 as one kernel (k_sf_f1).  An older
    variant library (RLKS_LIB, A/B runs) without the query fused it only under RLKS_F1_FUSED."""
    from rlks import _lib

    lib = _lib.lib()
    if hasattr(lib, "rlks_sf_f1_fused"):
        return bool(lib.rlks_sf_f1_fused(desc))
    return bool(os.environ.get("RLKS_F1_FUSED"))


def pmc_traffic():
    """per-launch HBM bytes of the dominant kernel from the committed rocprofv3 PMC summary, if any"""
    p = ROOT / "profiles" / "pmc_traffic.json"
    if p.exists():
        try:
            return json.loads(p.read_text())
        except Exception:
            return None
    return None


def dry_run(args, world, rank):
    """--dry-run: the multi-rank contract without a GPU (gloo on the CPU): barrier, an empty timed
    region, MAX over ranks, one JSON line from rank 0 with the shard sizes the real run would use"""
    import torch
    import torch.distributed as dist

    if world > 1:
        dist.init_process_group("gloo")
    fail = os.environ.get("RLKS_DRYRUN_FAIL_RANK")
    if fail is not None and int(fail) == rank:  # launcher test: this rank dies while the others wait
        sys.exit(3)
    preset = CONFIGS[args.config]
    envs, mb = shard_sizes(args, preset, world)
    for _ in range(args.warmup):
        pass
    if world > 1:
        dist.barrier()
    t0 = time.perf_counter()
    for _ in range(args.steps):
        time.sleep(0.001)
    if world > 1:
        dist.barrier()
    elapsed = time.perf_counter() - t0
    if world > 1:
        t = torch.tensor([elapsed], dtype=torch.float64)
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        elapsed = float(t.item())
    if rank == 0:
        print(json.dumps({"metric": METRIC, "value": None, "unit": "env-steps/s", "n_gpus": world, "steps": args.steps,
                          "warmup": args.warmup, "ms_per_step": elapsed / max(1, args.steps) * 1e3,
                          "higher_is_better": True, "scaling": args.scaling, "vs_baseline": None,
                          "data": "dry-run (launcher plumbing only; no GPU work)",
                          "config": {"name": args.config, "envs_per_gpu": envs, "minibatch_per_gpu": mb,
                                     "global_envs": envs * world, "global_minibatch": mb * world,
                                     "parallelism": f"dp{world}"}}), flush=True)
    if world > 1:
        dist.barrier()
        dist.destroy_process_group()


DUMP_MAX_ELEMS = 1 << 19  # per array: 2 MB of float32, so the ~16 arrays stay far below 64 MB in all
DUMP_SEED = 20240229


def dump_outputs(algo, torch, out_dir):
    """--dump-outputs: what train_step_no_sync left for its caller after the last timed step, one
    DIR/<name>.npy per array: the flat parameters, Adam moments and last gradient, the per-SGD-step
    learner stats and episode sums (float64), the dynamic scalars (KL coefficient, advantage mean /
    scale) and the rollout / advantage buffers the update read (float32; integer buffers converted).
    An array of more than DUMP_MAX_ELEMS elements is written as a fixed sample of that many of its
    flattened elements (sorted indices from numpy's default_rng(DUMP_SEED), the same for every run
    and build)."""
    out = Path(out_dir)
    out.mkdir(parents=True, exist_ok=True)
    arrays = {"params": algo.params.flat, "adam_m": algo.adam_m, "adam_v": algo.adam_v, "grad": algo.grad,
              "stats": algo.stats, "ep_stats": algo.ep_stats, "dyn": algo.dyn}
    arrays.update({f"rollout_{k}": v for k, v in algo.buf.items()})
    for name, t in arrays.items():
        flat = t.detach().reshape(-1)
        if flat.numel() > DUMP_MAX_ELEMS:
            idx = np.sort(np.random.default_rng(DUMP_SEED).integers(0, flat.numel(), DUMP_MAX_ELEMS))
            flat = flat[torch.from_numpy(idx).to(flat.device)]
        else:
            flat = flat.reshape(t.shape)
        a = flat.cpu().numpy()
        np.save(out / f"{name}.npy", a.astype(np.float64 if a.dtype == np.float64 else np.float32))


METRIC = "env-steps/sec (node), batched rollout+policy update, 1/2/4/8 GPUs; %HBM BW"


def main():
    args = parse()
    argv = sys.argv[1:]
    if "WORLD_SIZE" not in os.environ and args.gpus > 1:
        sys.exit(launch_ranks(args.gpus, argv))
    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local = int(os.environ.get("LOCAL_RANK", "0"))
    if world != args.gpus:
        raise SystemExit(f"bench.py: WORLD_SIZE {world} != --gpus {args.gpus}")
    if args.dry_run:
        return dry_run(args, world, rank)
    import torch
    import torch.distributed as dist

    # RLKS_DDP_FORCE=1 on one rank: a one-rank process group (RCCL) and the multi-rank SGD step with every
    # collective issued (rlks.distributed.forced): RCCL's all-reduce on hardware with one GPU
    forced = world == 1 and os.environ.get("RLKS_DDP_FORCE") == "1"
    if forced:
        os.environ.setdefault("MASTER_PORT", str(_free_port()))
        os.environ.setdefault("RANK", "0")
        os.environ.setdefault("WORLD_SIZE", "1")
    if world > 1 or forced:
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        # RCCL ("nccl") over xGMI, one GPU per rank.  RLKS_DIST_BACKEND=gloo is for rehearsing the
        # multi-rank path with several ranks on fewer GPUs (ranks share devices round-robin).
        backend = os.environ.get("RLKS_DIST_BACKEND", "nccl")
        if backend == "nccl" and local >= torch.cuda.device_count():
            raise SystemExit(f"rank {rank}: LOCAL_RANK {local} but only {torch.cuda.device_count()} HIP device(s)")
        device = local % max(1, torch.cuda.device_count()) if backend != "nccl" else local
        torch.cuda.set_device(device)
        if backend == "nccl":
            dist.init_process_group("nccl", device_id=torch.device("cuda", device))
        else:
            dist.init_process_group(backend)
    else:
        torch.cuda.set_device(0)
    dev = torch.device("cuda", torch.cuda.current_device())

    from rlks.ppo import PPO, PPOConfig

    preset = CONFIGS[args.config]
    envs, minibatch = shard_sizes(args, preset, world)
    H = preset["hidden"]
    table, nodes = env_setup(args.config)
    cfg = (PPOConfig().environment("K8sMultiCloudEnv").framework("torch")
           .training(train_batch_size=envs * args.rollout * world, sgd_minibatch_size=minibatch * world,
                     num_sgd_iter=args.epochs, lr=3e-4, gamma=0.99, sgd_precision=args.precision,
                     model={"fcnet_hiddens": [H, H]})
           .debugging(seed=42))
    cfg.num_envs = envs
    cfg.rollout_fragment_length = args.rollout
    if os.environ.get("RLKS_OVERLAP_ALLREDUCE") is not None:  # multi-rank A/B: 0 = one bucket after the gradient
        cfg.overlap_allreduce = os.environ["RLKS_OVERLAP_ALLREDUCE"] != "0"
    cfg.table, cfg.nodes = table, nodes
    algo = PPO(config=cfg, device=dev)

    for _ in range(args.warmup):
        algo.train_step_no_sync()
    torch.cuda.synchronize()
    if world > 1:
        dist.barrier()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(args.steps):
        algo.train_step_no_sync()
    torch.cuda.synchronize()
    if world > 1:
        dist.barrier()
    torch.cuda.synchronize()
    elapsed = time.perf_counter() - t0
    if world > 1:
        t = torch.tensor([elapsed], dtype=torch.float64, device=dev)
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        elapsed = float(t.item())
    steps_total = algo.samples * world * args.steps
    value = steps_total / elapsed
    ms_per_step = elapsed / args.steps * 1e3
    if args.dump_outputs and rank == 0:
        dump_outputs(algo, torch, args.dump_outputs)

    # --full, multi-rank: one more (untimed) iteration with events around every gradient all-reduce
    allreduce = algo.profile_allreduce() if args.full and algo.multi else None
    kernels = kernel_timing(algo, torch, args.config) if args.full and not args.no_kernel_timing else None
    # sanity: the policy is learning something finite
    st = algo.stats.cpu().numpy()
    finite = bool((st == st).all())

    result = None
    if rank == 0:
        roofline = None
        if kernels:
            # the dominant kernel as rocprofv3 --stats ranks them: largest share of GPU time (each
            # runs once per SGD step, so: the longest launch), timed in the pipeline where there is one
            if "pipeline" in kernels:
                # the kernel: the longest in the pipeline (kernel-bracketing events: they rank the kernels as
                # rocprofv3 does); its duration: 20 back-to-back launches of it alone (HIP events around the
                # batch), which matched rocprofv3's in-pipeline average within 1% on the boxes measured
                # (66.7 vs 66.7 µs, 68.8 vs 69.0 µs; profiles/r06_trace) -- the bracketed figure carries the
                # bracket's own few µs, reported beside it
                pk = {n: v for n, v in kernels["pipeline"].items() if isinstance(v, dict) and "tflops" in v}
                dom = max(pk, key=lambda n: pk[n]["ms"])
                k = kernels[dom] if dom in kernels and "tflops" in kernels[dom] else pk[dom]
            else:
                cands = [k for k in kernels if k in ROOFLINE_KERNELS]
                dom = max(cands, key=lambda k: kernels[k]["ms"])
                k = kernels[dom]
            peak = {"fp32": FP32_MFMA_PEAK_TFLOPS, "f16": F16_MFMA_PEAK_TFLOPS}.get(algo.precision, SF16_PEAK_TFLOPS)
            roofline = {"bound": "mfma", "kernel": dom, "achieved": k["tflops"], "peak": peak,
                        "unit": "TFLOP/s", "frac": k["tflops"] / peak, "traffic": None,
                        "flop_per_launch": flops_per_row(dom if dom in ROOFLINE_KERNELS else "k_sf_f1", algo.D, algo.H,
                                                         algo.A) * algo.mb,
                        "avg_launch_ms": k["ms"],
                        "peak_basis": ("fp32 MFMA dense peak" if algo.precision == "fp32" else
                                       "2.5 PF dense f16 MFMA (one product per FLOP)" if algo.precision == "f16" else
                                       "split-fp16: 2.5 PF dense f16 MFMA / 3 products per fp32-accurate FLOP")}
            if dom == "wide_grad":
                roofline["note"] = "generic-width path: the whole SGD-step gradient (a sequence of split-fp16 GEMM launches)"
            if "pipeline" in kernels:
                roofline["avg_launch_ms_method"] = ("20 back-to-back launches of the kernel (HIP events on its stream); "
                                                    "chosen as the longest kernel of the SGD step in the pipeline")
                roofline["avg_launch_ms_pipeline"] = kernels["pipeline"]["ms"][dom]
                roofline["pipeline_event_bracket_ms"] = kernels["pipeline"]["event_bracket_ms"]
                # both timings are the kernel plus an overhead of their own (back-to-back: the launches'
                # overlapping ramps and drains; in the pipeline: the start / stop events around it), so
                # the smaller is the tighter figure: the back-to-back one matched rocprofv3 within 1% for
                # F1a (profiles/r06_trace), the raw bracketed one within 0.2% for the fused F1
                # (131.7 vs 131.4 µs, 125.9 vs 125.7; profiles/r06_trace6, r06_trace7)
                raw = kernels["pipeline"]["ms"][dom] + kernels["pipeline"]["event_bracket_ms"]
                if raw < roofline["avg_launch_ms"]:
                    roofline["avg_launch_ms_back_to_back"] = roofline["avg_launch_ms"]
                    roofline["avg_launch_ms"] = raw
                    roofline["achieved"] = roofline["flop_per_launch"] / (raw * 1e-3) / 1e12
                    roofline["frac"] = roofline["achieved"] / peak
                    roofline["avg_launch_ms_method"] = (
                        "the kernel's in-pipeline start / stop event bracket (rlks_ppo_grad_profile, not less the "
                        "bracket's own cost), smaller than 20 back-to-back launches of it (avg_launch_ms_back_to_back); "
                        "chosen as the longest kernel of the SGD step in the pipeline")
            if algo.precision != "fp32" and not args.no_kernel_timing:
                roofline["calibration"] = mfma_calibration(torch, roofline["achieved"], 1 if algo.precision == "f16" else 3)
            pmc = pmc_traffic()
            ab = algo_bytes_per_launch(dom, algo.mb, algo.D, algo.H, algo.A)
            roofline["algorithmic_bytes_per_launch"] = ab
            if pmc and args.config in ("c2", "c4") and dom in pmc:
                roofline["traffic"] = pmc[dom]["hbm_bytes_per_launch"]
                roofline["traffic_source"] = pmc["source"]
                if ab:
                    roofline["traffic_over_algorithmic"] = roofline["traffic"] / ab
            if "pipeline" in kernels:  # the step's MFMA kernels side by side
                side = {}
                for n, v in kernels["pipeline"].items():
                    if not (isinstance(v, dict) and "tflops" in v):
                        continue
                    iso = kernels.get(n, {})
                    ms_k = iso.get("ms", v["ms"])
                    tf_k = iso.get("tflops", v["tflops"])
                    e = {"avg_launch_ms": ms_k, "avg_launch_ms_pipeline": v["ms"], "achieved": tf_k, "frac": tf_k / peak,
                         "algorithmic_bytes_per_launch": algo_bytes_per_launch(n, algo.mb, algo.D, algo.H, algo.A)}
                    if pmc and args.config in ("c2", "c4") and n in pmc:
                        e["traffic"] = pmc[n]["hbm_bytes_per_launch"]
                    side[n] = e
                roofline["kernels"] = side
            if pmc and args.config in ("c2", "c4") and algo.precision == "sf16":
                # the whole SGD step against its compulsory bytes: the minibatch records read once, the
                # parameters read by the weight split, and Adam (p, m, v read + written, the gradient
                # written and read): everything else is a hand-off between the step's own kernels
                step = [k for k in ("k_sf_split", "k_sf_fwd", "k_sf_bwd", "k_sf_dw2", "k_reduce") if k in pmc]
                if "k_sf_f1" in kernels.get("pipeline", {}).get("ms", {}) and "k_sf_f1" in pmc:
                    step = [k for k in ("k_sf_split", "k_sf_f1", "k_sf_dw2", "k_reduce") if k in pmc]
                moved = sum(pmc[k]["hbm_bytes_per_launch"] for k in step)
                P = algo.params.padded
                comp = algo.mb * algo.stride * 4 + P * 4 + (6 + 2) * P * 4
                roofline["sgd_step"] = {"traffic": moved, "kernels": step, "compulsory_bytes": comp,
                                        "traffic_over_compulsory": moved / comp,
                                        "floor_us_at_6p3TBps": moved / 6.3e12 * 1e6}
        cpu = None
        if args.full and not args.no_cpu_baseline and world == 1:
            sys.path.insert(0, str(ROOT / "oracle"))
            from cpu_ppo import time_cpu_iteration

            cc = preset["cpu"]
            c = time_cpu_iteration(n_envs=cc["n_envs"], T=cc["T"], minibatch=cc["minibatch"], epochs=args.epochs,
                                   threads=cpu_threads(), table=table, nodes=nodes, hidden=H, label=args.config)
            cpu = {"value": c["value"], "unit": "env-steps/s", "cores": c["cores"], "kind": "port",
                   "sample": c["sample"]}
        result = {
            "metric": METRIC,
            "value": value, "unit": "env-steps/s", "n_gpus": world, "steps": args.steps, "warmup": args.warmup,
            "ms_per_step": ms_per_step, "higher_is_better": True, "scaling": args.scaling, "vs_baseline": None,
            "dtype": {"fp32": "fp32", "f16": "fp16 operands, fp32 accumulation (throughput mode, below the reference's fp32)"}.get(
                algo.precision, "fp32 (split-fp16 MFMA, fp32-accurate)"), "data": "synthetic (env-generated rollouts, random-init FCNet)",
            "config": {"workload": preset["text"], "name": args.config,
                       "envs_per_gpu": envs, "rollout_steps": args.rollout, "minibatch_per_gpu": algo.mb,
                       "epochs": args.epochs, "global_batch": algo.samples * world, "global_envs": envs * world,
                       "global_minibatch": algo.mb * world, "sgd_precision": algo.precision,
                       "parallelism": f"dp{world}"},
            "roofline": roofline, "cpu_baseline": cpu, "allreduce": allreduce, "kernels": kernels, "finite": finite,
        }
        print(json.dumps(result), flush=True)
    if world > 1 or forced:
        dist.barrier()
        dist.destroy_process_group()
    return result


if __name__ == "__main__":
    main()
