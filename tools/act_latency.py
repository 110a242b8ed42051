#!/usr/bin/env python
"""Host wall-clock latency of one decision call, synchronisation included.

    python tools/act_latency.py --side server --out profiles/r16_serving/tree_1.json
    python tools/act_latency.py --side algo --pkg <a checkout's rl-k8s-scheduler_amd> --out .../parent_1.json

--side server   PolicyServer.act (PPO.server())
--side algo     PPO.compute_single_action at n = 1, PPO.compute_actions(...).cpu().numpy() at n > 1
--hidden        the hidden width (default: the config's 256); 128 is outside the act kernel's scope, so that
                --side server then times the fallback
--pkg           the package directory to import rlks from (default: this tree's), so that another
                checkout's build is timed by the same script on the same box
Grid: n in {1, 16, 256, 1024} x explore in {False, True} x {plain, filter + mask} at (D, A) = (6, 2) and
(24, 8).  Per cell: 200 warm-up calls, then time.perf_counter_ns around each of 2,000 calls; the record
holds the median and the 99th percentile in microseconds.  The plain cells run a table env's algorithm, the
filter + mask cells a node-level one (NodeSpec(C, 16), observation_filter="MeanStdFilter",
action_mask="room"); the env only supplies the configuration, every call gets the same seeded observations.
"""
import argparse
import json
import sys
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parents[1]
NS = (1, 16, 256, 1024)
SHAPES = ((6, 2), (24, 8))
WARMUP, CALLS = 200, 2000


def build(C_, variant, dev, hidden=None):
    from rlks.env import NodeSpec
    from rlks.ppo import PPO, PPOConfig
    from rlks.tables import load_table, synthetic_table

    cfg = (PPOConfig().framework("torch")
           .training(train_batch_size=256 * 8, sgd_minibatch_size=1024, num_sgd_iter=1, lr=3e-4)
           .debugging(seed=11))
    cfg.num_envs, cfg.rollout_fragment_length = 256, 8
    if hidden:
        cfg.training(model={"fcnet_hiddens": [hidden, hidden]})
    cfg.table = load_table() if C_ == 2 else synthetic_table(C_, 100, seed=7)
    if variant == "filter+mask":
        cfg.nodes = NodeSpec(C_, 16)
        cfg.training(action_mask="room")
        cfg.rollouts(observation_filter="MeanStdFilter")
    return PPO(config=cfg, device=dev)


def time_calls(fn, warmup=WARMUP, calls=CALLS):
    for _ in range(warmup):
        fn()
    t = np.empty(calls, np.int64)
    for i in range(calls):
        t0 = time.perf_counter_ns()
        fn()
        t[i] = time.perf_counter_ns() - t0
    return float(np.median(t)) / 1e3, float(np.percentile(t, 99)) / 1e3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--side", choices=("server", "algo"), required=True)
    ap.add_argument("--pkg", default=str(ROOT / "rl-k8s-scheduler_amd"))
    ap.add_argument("--out", required=True)
    ap.add_argument("--calls", type=int, default=CALLS)
    ap.add_argument("--hidden", type=int, default=None, help="e.g. 128: outside rlks_policy_act's scope, so that "
                    "--side server times the fallback (forward + rlks.sampling.sample_rows)")
    args = ap.parse_args()
    sys.path.insert(0, args.pkg)
    import torch

    dev = torch.device("cuda", 0)
    rows = []
    for D, A in SHAPES:
        for variant in ("plain", "filter+mask"):
            algo = build(A, variant, dev, args.hidden)
            assert (algo.D, algo.A) == (D, A)
            obs = np.random.default_rng(5).random((max(NS), D)).astype(np.float32)
            mask = None
            if variant == "filter+mask":
                mask = np.random.default_rng(3).random((max(NS), A)) < 0.5
                mask[:, 0] = True
            srv = algo.server(max_rows=max(NS)) if args.side == "server" else None
            for explore in (False, True):
                for n in NS:
                    o, m = obs[:n], (mask[:n] if mask is not None else None)
                    if srv is not None:
                        if n == 1:
                            fn = lambda: srv.act(o[0], explore=explore, action_mask=None if m is None else m[0])  # noqa: E731
                        else:
                            fn = lambda: srv.act(o, explore=explore, action_mask=m)  # noqa: E731
                    elif n == 1:
                        fn = lambda: algo.compute_single_action(o[0], explore=explore,  # noqa: E731
                                                                action_mask=None if m is None else m[0])
                    else:
                        fn = lambda: algo.compute_actions(o, explore=explore, action_mask=m).cpu().numpy()  # noqa: E731
                    med, p99 = time_calls(fn, calls=args.calls)
                    rows.append({"D": D, "A": A, "variant": variant, "explore": explore, "n": n,
                                 "median_us": round(med, 2), "p99_us": round(p99, 2)})
                    print(json.dumps(rows[-1]), flush=True)
            algo.stop()
    out = Path(args.out)
    out.parent.mkdir(parents=True, exist_ok=True)
    out.write_text(json.dumps({"side": args.side, "pkg": args.pkg, "warmup": WARMUP, "calls": args.calls,
                               "hidden": args.hidden, "fused": bool(srv.fused) if srv is not None else None,
                               "rows": rows}, indent=1))


if __name__ == "__main__":
    main()
