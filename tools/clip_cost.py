"""Cost of global-norm clipping at the c4 shape: 131,072 lanes, T 128, 65,536-row minibatches, 10
epochs (2,560 SGD steps per iteration), through PPO.train_step_no_sync with grad_clip None and 40.0,
alternating; ms per iteration and the per-SGD-step difference (profiles/r09_grad_clip).  Prints one JSON
line; an argument names a file to write it to as well."""
import json
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT / "rl-k8s-scheduler_amd"))

import numpy as np  # noqa: E402
import torch  # noqa: E402

from rlks import _lib  # noqa: E402
from rlks.ppo import PPO, PPOConfig  # noqa: E402


def make(clip):
    N, T, mb, epochs = 131072, 128, 65536, 10
    cfg = (PPOConfig().environment("K8sMultiCloudEnv").framework("torch")
           .training(train_batch_size=N * T, sgd_minibatch_size=mb, num_sgd_iter=epochs, lr=3e-4, gamma=0.99,
                     grad_clip=clip).debugging(seed=1))
    cfg.num_envs = N
    cfg.rollout_fragment_length = T
    return PPO(config=cfg, device=torch.device("cuda", 0))


def timed(algo, n):
    st = torch.cuda.current_stream()
    out = []
    for _ in range(n):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(st)
        algo.train_step_no_sync()
        b.record(st)
        b.synchronize()
        out.append(a.elapsed_time(b))
    return out


def main():
    algos = {"none": make(None), "clip40": make(40.0)}
    for a in algos.values():
        timed(a, 1)  # warm-up
    ms = {k: [] for k in algos}
    for _ in range(3):  # alternating legs
        for k, a in algos.items():
            ms[k] += timed(a, 2)
    steps = algos["none"].stats.shape[0]
    norms = algos["clip40"].stats[:, _lib.RLKS_STAT_GRAD_GNORM].cpu().numpy()
    res = {"sgd_steps_per_iteration": int(steps), "ms_per_iteration": ms,
           "median_ms": {k: float(np.median(v)) for k, v in ms.items()},
           "us_per_sgd_step_difference": float((np.median(ms["clip40"]) - np.median(ms["none"])) * 1e3 / steps),
           "last_iteration_norm_min_median_max": [float(norms.min()), float(np.median(norms)), float(norms.max())],
           "last_iteration_clipped_fraction": float((norms > 40.0).mean()),
           "finite": bool(torch.isfinite(algos["clip40"].params.flat).all())}
    if len(sys.argv) > 1:
        Path(sys.argv[1]).write_text(json.dumps(res, indent=1))
    print(json.dumps(res))


if __name__ == "__main__":
    main()
