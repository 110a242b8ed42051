#!/usr/bin/env python3
"""A/B of PPO.rollout() on the node-level configs (c3: node_rollout, c5: wide_rollout) between two
builds of the library, same box, one call: which form of "sample + node step" a rollout loop should
launch.

  node_rollout_ab.py --parent <parent librlks.so> [--new <this tree's librlks.so>]
                     [--configs c3 c5] [--rollout 128] [--repeats 5] [--rounds 2] [--json out.json]

The library is chosen when a process loads it (RLKS_LIB), so each measurement is a fresh child of
this script; the two libraries alternate, parent first, `rounds` times per config, one child at a
time.  A child builds the config's PPO (bench.env_setup, bench.py's seed and shapes), runs two
rollouts to warm up, then `repeats` rollouts each between two device events, and prints the times.
Per library and config the repeats of all rounds are pooled: median, min, max.  A child also prints
checksums of the bits its last rollout left in each buffer; the buffers on which the two libraries
disagree are named.

Decision rule: a loop takes the new library's form if its median is not above the parent's median
by more than the parent's own min-max spread."""
import argparse
import json
import os
import statistics
import subprocess
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "rl-k8s-scheduler_amd"))


def child(config, T, repeats):
    import torch

    import bench
    from rlks.ppo import PPO, PPOConfig

    torch.cuda.set_device(0)
    preset = bench.CONFIGS[config]
    envs, H = preset["envs"], preset["hidden"]
    table, nodes = bench.env_setup(config)
    cfg = (PPOConfig().environment("K8sMultiCloudEnv").framework("torch")
           .training(train_batch_size=envs * T, sgd_minibatch_size=preset["minibatch"], num_sgd_iter=1, lr=3e-4,
                     gamma=0.99, model={"fcnet_hiddens": [H, H]})
           .debugging(seed=42))
    cfg.num_envs, cfg.rollout_fragment_length = envs, T
    cfg.table, cfg.nodes = table, nodes
    algo = PPO(config=cfg, device=torch.device("cuda", 0))
    for _ in range(2):
        algo.rollout(explore=True)
    torch.cuda.synchronize()
    ms = []
    for _ in range(repeats):
        s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        s.record()
        algo.rollout(explore=True)
        e.record()
        torch.cuda.synchronize()
        ms.append(s.elapsed_time(e))
    b = algo.buf
    # (checksums of the bits the last rollout left: the two libraries must agree on them)
    digest = {k: int(b[k].view(torch.uint8 if b[k].dtype == torch.uint8 else torch.int32).to(torch.int64).sum().item())
              for k in ("actions", "logp", "obs", "rewards", "dones", "logits", "values")}
    print("AB " + json.dumps({"config": config, "T": T, "envs": envs, "precision": algo.precision, "ms": ms,
                              "digest": digest}), flush=True)


def summary(ms):
    return {"median": statistics.median(ms), "min": min(ms), "max": max(ms), "n": len(ms)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent", help="the parent commit's librlks.so")
    ap.add_argument("--new", default=str(ROOT / "rl-k8s-scheduler_amd" / "rlks" / "librlks.so"))
    ap.add_argument("--configs", nargs="+", default=["c3", "c5"])
    ap.add_argument("--rollout", type=int, default=128)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=2)
    ap.add_argument("--timeout", type=int, default=240, help="seconds a child may take")
    ap.add_argument("--json")
    ap.add_argument("--child", help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.child:
        return child(a.child, a.rollout, a.repeats)
    if not a.parent:
        ap.error("--parent is required")
    libs = {"parent": str(Path(a.parent).resolve()), "new": str(Path(a.new).resolve())}
    out = {"libs": libs, "rollout": a.rollout, "configs": {}}
    for config in a.configs:
        runs = {"parent": [], "new": []}
        digests = {"parent": set(), "new": set()}
        for _ in range(a.rounds):
            for which in ("parent", "new"):
                env = dict(os.environ, RLKS_LIB=libs[which])
                p = subprocess.run([sys.executable, __file__, "--child", config, "--rollout", str(a.rollout),
                                    "--repeats", str(a.repeats)], env=env, capture_output=True, text=True,
                                   timeout=a.timeout)
                line = next((l for l in p.stdout.splitlines() if l.startswith("AB ")), None)
                if p.returncode != 0 or line is None:  # nothing more runs on the device after a failed child
                    sys.stderr.write(p.stdout[-2000:] + p.stderr[-4000:])
                    raise SystemExit(f"{config} / {which}: child exited with {p.returncode}")
                r = json.loads(line[3:])
                runs[which] += r["ms"]
                digests[which].add(json.dumps(r["digest"], sort_keys=True))
                print(f"{config} {which:6s} " + " ".join(f"{x:.3f}" for x in r["ms"]), flush=True)
        sp, sn = summary(runs["parent"]), summary(runs["new"])
        spread = sp["max"] - sp["min"]
        # the buffers whose bits differ: between the two libraries, or between two runs of one (none expected there)
        dp, dn = ([json.loads(x) for x in sorted(digests[w])] for w in ("parent", "new"))
        differ = sorted(k for k in dp[0] if len({d[k] for d in dp + dn}) > 1)
        rec = {"parent": sp, "new": sn, "parent_spread": spread, "ms": runs,
               "digests": {"parent": dp, "new": dn}, "repeatable": len(dp) == 1 and len(dn) == 1,
               "buffers_that_differ": differ, "switch": sn["median"] <= sp["median"] + spread}
        out["configs"][config] = rec
        print(f"{config}: parent median {sp['median']:.3f} ms [{sp['min']:.3f}, {sp['max']:.3f}], new median "
              f"{sn['median']:.3f} ms [{sn['min']:.3f}, {sn['max']:.3f}], buffers that differ: "
              f"{', '.join(differ) or 'none'}{'' if rec['repeatable'] else ' (runs of one library disagree)'} -> "
              f"{'switch' if rec['switch'] else 'keep'}", flush=True)
    if a.json:
        Path(a.json).write_text(json.dumps(out, indent=1) + "\n")
    print(json.dumps({c: {k: r[k] for k in ("parent", "new", "parent_spread", "buffers_that_differ", "switch")}
                      for c, r in out["configs"].items()}))


if __name__ == "__main__":
    main()
