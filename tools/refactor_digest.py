#!/usr/bin/env python3
"""SHA-256 digests of what the rollout, gradient and SGD-step kernels compute, for the library RLKS_LIB
selects: run once with the parent commit's librlks.so and once with the tree's, then compare the files.

  RLKS_LIB=<parent's librlks.so> RLKS_LIB_NAME=parent python tools/refactor_digest.py profiles/<change>/digest_parent.json
  python tools/refactor_digest.py profiles/<change>/digest_tree.json
  python tools/refactor_digest.py --compare profiles/<change>/digest_parent.json profiles/<change>/digest_tree.json

rollout: every buffer of one PPO.rollout on each rollout kernel path (the rows of
         tests/test_gpu_node_sample_step.py::test_rollout_replays_from_its_logits); logp itself goes to
         <output>.logp.npz beside the digests (not for committing), from which --compare gives the ulp
         distance where the digests differ
grad:    grad and stats of one rlks_ppo_grad at 256 rows (fp32, sf16, f16 at 2, 4 and 8 actions; wide at
         D = 48, H = 384, A = 16) on records with masked old logits, zero advantages (the surrogate's tie)
         and ratios on both sides of the clip range
sgd:     the parameters after the three rlks_ppo_sgd_step_next steps of one PPO.update (4 actions, sf16)"""
import ctypes as C
import hashlib
import json
import os
import sys
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parents[1]
for p in (ROOT / "rl-k8s-scheduler_amd", ROOT / "oracle", ROOT / "tests"):
    sys.path.insert(0, str(p))

PER_STEP_LANES = 16384 + 1  # above ppo.hip's SF_ROLL_FUSED_MAX_LANES: k_sf_fwd16 + k_sample_step per step
ROLLOUTS = {  # name: C, nodes, H, N, T, minibatch, table rows, sgd_precision, per-step path
    "node-sf16-8": (8, 16, 256, 520, 16, 8192, 100, "auto", False),
    "node-wide-16": (16, 32, 384, 136, 8, 1024, 100, "auto", False),
    "table-persistent-2": (2, None, 256, 96, 6, 256, 4, "auto", False),
    "table-persistent-8": (8, None, 256, 96, 6, 256, 4, "auto", False),
    "table-per-step-4": (4, None, 256, 96, 6, 256, 4, "auto", True),
    "table-fp32-4": (4, None, 256, 96, 6, 256, 4, "fp32", False),
    "table-wide-4": (4, None, 384, 136, 6, 256, 4, "auto", False),
}


def sha(x):
    return hashlib.sha256(np.ascontiguousarray(x.cpu().numpy() if hasattr(x, "cpu") else x).tobytes()).hexdigest()


def make_algo(torch, C_, nodes, H, N, T, mb, rows, prec, per_step):
    from rlks.env import NodeSpec
    from rlks.ppo import PPO, PPOConfig
    from rlks.tables import synthetic_table

    spec = None if nodes is None else NodeSpec(C_, nodes, arrival_rate=2.0, depart_prob=0.05, init_occupancy=0.5,
                                               reject_penalty=0.1)
    cfg = (PPOConfig().framework("torch")
           .training(train_batch_size=N * T, sgd_minibatch_size=mb, num_sgd_iter=1, lr=3e-4,
                     model={"fcnet_hiddens": [H, H]})
           .debugging(seed=5))
    cfg.num_envs, cfg.table, cfg.nodes, cfg.sgd_precision = N, synthetic_table(C_, rows, seed=7), spec, prec
    algo = PPO(config=cfg, device=torch.device("cuda", 0))
    if per_step:
        algo.bufs.global_lanes = PER_STEP_LANES
    return algo


def records(rows, D, A, seed):
    """packed minibatch records [obs D | logits_old A | adv | vtarg | logp_old | action | pad] that reach every
    branch of the loss row: rows 0 mod 4 carry a masked old logit (not the action's), rows 1 mod 4 a
    zero advantage (s1 == s2), and the old logits are far enough from a fresh policy's that ratios fall on
    both sides of the clip range"""
    rng = np.random.default_rng(seed)
    stride = (D + A + 4 + 3) // 4 * 4
    mb = np.zeros((rows, stride), np.float32)
    mb[:, :D] = rng.random((rows, D))
    lo = (rng.standard_normal((rows, A)) * 0.5).astype(np.float32)
    act = rng.integers(0, A, rows)
    masked = (act[::4] + 1 + rng.integers(0, A - 1, len(act[::4]))) % A
    lo[np.arange(0, rows, 4), masked] = np.float32(-1e30)
    mb[:, D:D + A] = lo
    mb[:, D + A] = rng.standard_normal(rows) * 3 + 0.5
    mb[1::4, D + A] = 0.0
    mb[:, D + A + 1] = rng.standard_normal(rows) * 2
    mb[:, D + A + 3] = act
    l64 = lo.astype(np.float64)
    mx = l64.max(1, keepdims=True)
    lsm = l64 - mx - np.log(np.exp(l64 - mx).sum(1, keepdims=True))
    mb[:, D + A + 2] = lsm[np.arange(rows), act]
    return mb


def grad_digest(torch, D, H, A, prec, rows=256):
    from rlks import _lib
    from rlks.policy import PolicyParams

    dev = torch.device("cuda", 0)
    p = PolicyParams(D, H, A, device=dev, seed=11 + A)
    p.desc.precision = prec
    mbt = torch.from_numpy(records(rows, D, A, 100 + A)).to(dev)
    dyn = torch.tensor([0.0, 1.0, 0.2, 1.0 / rows, 0, 0, 0, 0], dtype=torch.float32, device=dev)  # adv as stored: the ties stay ties
    co = _lib.PpoCoeffs(0.3, 10.0, 1.0, 0.01)
    wsb = C.c_int64()
    _lib.call("rlks_ppo_workspace_bytes", C.byref(p.desc), rows, C.byref(wsb))
    ws = torch.zeros(wsb.value, dtype=torch.uint8, device=dev)
    grad = torch.zeros(p.padded, device=dev)
    stats = torch.zeros(_lib.RLKS_STAT_SIZE, dtype=torch.float64, device=dev)
    _lib.call("rlks_ppo_grad", C.byref(p.desc), C.byref(co), p.flat.data_ptr(), dyn.data_ptr(), mbt.data_ptr(), rows,
              grad.data_ptr(), stats.data_ptr(), ws.data_ptr(), ws.numel(), None)
    torch.cuda.synchronize()
    assert torch.isfinite(grad).all() and float(grad.abs().max()) > 0
    return {"grad": sha(grad), "stats": sha(stats)}


def run(out):
    import torch
    from rlks import _lib

    res = {"lib": os.environ.get("RLKS_LIB_NAME", "tree"), "rollout": {}, "grad": {}, "sgd": {}}
    logp = {}
    for name, (C_, nodes, H, N, T, mb, rows, prec, per_step) in ROLLOUTS.items():
        algo = make_algo(torch, C_, nodes, H, N, T, mb, rows, prec, per_step)
        algo.rollout(explore=True)
        torch.cuda.synchronize()
        b = algo.buf
        res["rollout"][name] = {k: sha(b[k]) for k in ("logits", "values", "actions", "logp", "obs", "rewards", "dones")}
        logp[name] = b["logp"].cpu().numpy().view(np.uint32).ravel()
        print("rollout", name, res["rollout"][name]["logp"][:16], flush=True)
        algo.stop()
    precs = {"fp32": _lib.RLKS_PRECISION_FP32, "sf16": _lib.RLKS_PRECISION_SF16, "f16": _lib.RLKS_PRECISION_F16}
    for pname, prec in precs.items():
        for A in (2, 4, 8):
            res["grad"][f"{pname}-{A}"] = grad_digest(torch, 3 * A, 256, A, prec)
            print("grad", pname, A, res["grad"][f"{pname}-{A}"]["grad"][:16], flush=True)
    res["grad"]["wide-16"] = grad_digest(torch, 48, 384, 16, _lib.RLKS_PRECISION_WIDE)
    print("grad wide", res["grad"]["wide-16"]["grad"][:16], flush=True)
    # three SGD steps: 128 lanes x 6 steps = 3 minibatches of 256; the rollout on the per-step path, whose
    # logp does not depend on the library compared
    algo = make_algo(torch, 4, None, 256, 128, 6, 256, 100, "sf16", True)
    algo.rollout(explore=True)
    algo.advantages()
    algo.update()
    torch.cuda.synchronize()
    assert algo.adam_step == 3
    res["sgd"] = {"params": sha(algo.params.flat), "adam_m": sha(algo.adam_m), "adam_v": sha(algo.adam_v),
                  "stats": sha(algo.stats), "rollout_logp": sha(algo.buf["logp"])}
    print("sgd", res["sgd"]["params"][:16], flush=True)
    algo.stop()
    out.parent.mkdir(parents=True, exist_ok=True)
    out.write_text(json.dumps(res, indent=1) + "\n")
    np.savez(out.with_suffix(".logp.npz"), **logp)


def ulp_key(bits):
    """float32 bits -> integers whose difference is the distance in ulp (monotone over the reals)"""
    b = np.asarray(bits, np.uint32).astype(np.int64)
    return np.where(b & 0x80000000, 0x80000000 - b, b)


def compare(pa, pb):
    a, b = json.loads(Path(pa).read_text()), json.loads(Path(pb).read_text())
    print(f"{a['lib']} ({pa}) against {b['lib']} ({pb})")
    differ = []
    for sec in ("rollout", "grad"):
        for name in a[sec]:
            for k in a[sec][name]:
                if a[sec][name][k] != b[sec][name][k]:
                    differ.append(f"{sec}/{name}/{k}")
    differ += [f"sgd/{k}" for k in a["sgd"] if a["sgd"][k] != b["sgd"][k]]
    n = sum(len(v) for sec in ("rollout", "grad") for v in a[sec].values()) + len(a["sgd"])
    print(f"{n} digests compared, {len(differ)} differ: {', '.join(differ) if differ else 'none'}")
    la, lb = Path(pa).with_suffix(".logp.npz"), Path(pb).with_suffix(".logp.npz")
    if not (la.exists() and lb.exists()):
        print("no logp files beside the digests: no ulp distances")
        return differ
    la, lb = np.load(la), np.load(lb)
    for name in la.files:
        d = np.abs(ulp_key(la[name]) - ulp_key(lb[name]))
        print(f"logp {name:20s} {len(d)} values, {int((d > 0).sum())} differ, max {int(d.max())} ulp")
    return differ


if __name__ == "__main__":
    if sys.argv[1] == "--compare":
        compare(sys.argv[2], sys.argv[3])
    else:
        run(Path(sys.argv[1]))
