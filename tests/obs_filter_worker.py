"""One rank of tests/test_gpu_obs_filter_ranks.py (started as a fresh child process): torch.distributed
over gloo, every rank on device 0, the real PPO class with observation_filter="MeanStdFilter"; writes its
filter state and its raw observations to <out>/rank<r>.npz."""
import os
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]
sys.path[:0] = [str(ROOT / "rl-k8s-scheduler_amd")]


def main():
    out = Path(sys.argv[1])
    N, T, iters = (int(x) for x in sys.argv[2:5])
    import numpy as np
    import torch
    import torch.distributed as dist

    rank, world = int(os.environ["RANK"]), int(os.environ["WORLD_SIZE"])
    torch.cuda.set_device(0)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        from rlks.ppo import PPO, PPOConfig

        cfg = (PPOConfig().environment("K8sMultiCloudEnv").framework("torch")
               .rollouts(observation_filter="MeanStdFilter")
               .training(train_batch_size=N * T * world, sgd_minibatch_size=256 * world, num_sgd_iter=1, lr=3e-4,
                         gamma=0.99)
               .debugging(seed=13))
        cfg.num_envs = N
        cfg.rollout_fragment_length = T
        algo = PPO(config=cfg, device=torch.device("cuda", 0))
        assert algo.multi and algo.obs_filter is not None
        raws, counts = [], []
        for _ in range(iters):
            r = algo.train()
            counts.append(r["info"]["learner"]["default_policy"]["obs_filter"]["count"])
            raws.append(algo.raw.cpu().numpy())
        np.savez(out / f"rank{rank}.npz", state=algo.obs_filter.state.cpu().numpy(), raw=np.stack(raws),
                 counts=np.array(counts), params=algo.params.flat.cpu().numpy())
    finally:
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
