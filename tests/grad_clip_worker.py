"""One rank of tests/test_gpu_grad_clip_ranks.py (started as a fresh child process): torch.distributed
over gloo, every rank on device 0, the real PPO class with grad_clip set; writes its parameters and,
per iteration, the reported grad_gnorm and the per-step norms to <out>/rank<r>.npz."""
import json
import os
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]
sys.path[:0] = [str(ROOT / "rl-k8s-scheduler_amd")]


def main():
    out = Path(sys.argv[1])
    N, T, mb, epochs, iters = (int(x) for x in sys.argv[2:7])
    grad_clip = float(sys.argv[7])
    import numpy as np
    import torch
    import torch.distributed as dist

    rank, world = int(os.environ["RANK"]), int(os.environ["WORLD_SIZE"])
    torch.cuda.set_device(0)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        from rlks import _lib
        from rlks.ppo import PPO, PPOConfig

        cfg = (PPOConfig().environment("K8sMultiCloudEnv").framework("torch")
               .training(train_batch_size=N * T * world, sgd_minibatch_size=mb, num_sgd_iter=epochs, lr=3e-4,
                         gamma=0.99, grad_clip=grad_clip)
               .debugging(seed=13))
        cfg.num_envs = N
        cfg.rollout_fragment_length = T
        algo = PPO(config=cfg, device=torch.device("cuda", 0))
        assert algo.multi and algo.grad_clip == grad_clip
        gnorm, steps = [], []
        for _ in range(iters):
            r = algo.train()
            gnorm.append(r["info"]["learner"]["default_policy"]["learner_stats"]["grad_gnorm"])
            # (self.stats is sum-all-reduced over the ranks)
            steps.append((algo.stats[:, _lib.RLKS_STAT_GRAD_GNORM] / world).cpu().numpy())
        np.savez(out / f"rank{rank}.npz", params=algo.params.flat.cpu().numpy(), kl_coeff=np.float32(algo.dyn[2].item()),
                 gnorm=np.array(gnorm), steps=np.array(steps), meta=np.array(json.dumps({"world": world})))
    finally:
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
