"""Global-norm clipping on the data-parallel path: two gloo ranks on one GPU (fresh child processes,
tests/grad_clip_worker.py) with grad_clip set.  On more than one rank the norm is that of the
all-reduced gradient, so every rank clips by the same coefficient: both ranks end with identical
parameters and report an identical grad_gnorm, and the run equals one rank over both lane blocks
(num_lane_groups = 2) within test_two_ranks_equal_one_rank_with_two_lane_groups's bounds, 1e-5 of the
parameters' norm and 1e-3 of the update's (fp32 summation order: per-rank sums + all-reduce vs one
sum)."""
import os
import socket
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

HERE = Path(__file__).resolve().parent


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _run_ranks(out, N, T, mb, epochs, iters, world, grad_clip):
    out.mkdir(parents=True, exist_ok=True)
    port = _free_port()
    procs = []
    for r in range(world):
        env = dict(os.environ, RANK=str(r), WORLD_SIZE=str(world), LOCAL_RANK=str(r), MASTER_ADDR="127.0.0.1",
                   MASTER_PORT=str(port), HSA_ENABLE_IPC_MODE_LEGACY="0")
        procs.append(subprocess.Popen([sys.executable, str(HERE / "grad_clip_worker.py"), str(out), str(N), str(T),
                                       str(mb), str(epochs), str(iters), repr(grad_clip)], env=env))
    try:
        for p in procs:
            assert p.wait(timeout=100) == 0
    finally:
        for p in procs:
            if p.poll() is None:
                p.kill()
    return [np.load(out / f"rank{r}.npz") for r in range(world)]


def test_two_clipped_ranks_equal_one_rank_with_two_lane_groups(tmp_path):
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    from rlks import _lib
    from rlks.ppo import PPO, PPOConfig

    N, T, mb, epochs, iters, world = 512, 128, 4096, 2, 2, 2
    d = torch.device("cuda", 0)

    def single(grad_clip):
        cfg = (PPOConfig().environment("K8sMultiCloudEnv").framework("torch")
               .training(train_batch_size=N * T * world, sgd_minibatch_size=mb, num_sgd_iter=epochs, lr=3e-4,
                         gamma=0.99, grad_clip=grad_clip)
               .debugging(seed=13))
        cfg.num_envs = N * world
        cfg.rollout_fragment_length = T
        cfg.num_lane_groups = world
        return PPO(config=cfg, device=d)

    # the threshold: the median norm of the first iteration's SGD steps, so that the clip acts on
    # some steps and not on others
    probe = single(1e30)
    probe.train()
    clip = float(np.float32(np.median(probe.stats[:, _lib.RLKS_STAT_GRAD_GNORM].cpu().numpy())))

    ranks = _run_ranks(tmp_path, N, T, mb, epochs, iters, world, clip)
    assert np.array_equal(ranks[0]["params"].view(np.int32), ranks[1]["params"].view(np.int32))
    assert np.array_equal(ranks[0]["gnorm"], ranks[1]["gnorm"])
    assert np.array_equal(ranks[0]["steps"], ranks[1]["steps"])
    steps = ranks[0]["steps"]
    assert (steps > clip).any() and (steps <= clip).any(), (clip, steps)

    algo = single(clip)
    p0 = algo.params.flat.cpu().numpy().astype(np.float64)
    res = [algo.train() for _ in range(iters)]
    p1 = algo.params.flat.cpu().numpy().astype(np.float64)
    p2 = ranks[0]["params"].astype(np.float64)
    dn = np.linalg.norm(p2 - p1)
    print(f"clip {clip}: ||p_2rank - p_1rank|| / ||p|| = {dn / np.linalg.norm(p1):.2e}, / ||update|| = "
          f"{dn / np.linalg.norm(p1 - p0):.2e}")
    assert dn <= 1e-5 * np.linalg.norm(p1)
    assert dn <= 1e-3 * np.linalg.norm(p1 - p0)
    assert float(ranks[0]["kl_coeff"]) == float(algo.dyn[2].item())
    for g2, r in zip(ranks[0]["gnorm"], res):
        # (the same gradients up to summation order and the parameters' drift bounded above)
        assert g2 == pytest.approx(r["info"]["learner"]["default_policy"]["learner_stats"]["grad_gnorm"], rel=1e-3)
