#!/usr/bin/env python3
"""SHA-256 digests of what the rollout, gather, gradient and SGD-step entries compute, for the library RLKS_LIB
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
sgd:     the parameters after the three rlks_ppo_sgd_step_next steps of one PPO.update (4 actions, sf16)
ws:      rlks_ppo_workspace_bytes, the two record strides and the debug entries' pointer offsets (fp32 at 128
         rows, sf16 at 256 rows, 2 / 4 / 8 actions; wide at 256 rows) -- plain numbers, not digests
gather:  the minibatches of rlks_ppo_pack + rlks_ppo_gather_packed and of rlks_ppo_gather_grouped (T = 6,
         N = 128, 256 rows, two epochs, 1 / 2 / 16 lane groups; 2, 4, 8 actions and the wide record)
step:    two consecutive SGD steps (the second with prev_fused = 1) through each step entry at 4 actions:
         parameters, Adam moments, gradient, stats and the next minibatch the first step gathered (1 lane
         group: inside the reduce's launch on sf16; 16: a launch of its own), then rlks_grad_global_norm"""
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

PER_STEP_LANES = 16384 + 1  # above workspace.h's SF_ROLL_FUSED_MAX_LANES: k_sf_fwd16 + k_sample_step per step
ROLLOUTS = {  # name: C, nodes, H, N, T, minibatch, table rows, sgd_precision, per-step path[, config attributes]
    "node-sf16-8": (8, 16, 256, 520, 16, 8192, 100, "auto", False),
    "node-wide-16": (16, 32, 384, 136, 8, 1024, 100, "auto", False),
    "table-persistent-2": (2, None, 256, 96, 6, 256, 4, "auto", False),
    "table-persistent-8": (8, None, 256, 96, 6, 256, 4, "auto", False),
    "table-per-step-4": (4, None, 256, 96, 6, 256, 4, "auto", True),
    "table-fp32-4": (4, None, 256, 96, 6, 256, 4, "fp32", False),
    "table-wide-4": (4, None, 384, 136, 6, 256, 4, "auto", False),
    "table-filtered-4": (4, None, 256, 96, 6, 256, 4, "auto", False, {"observation_filter": "MeanStdFilter"}),
    "node-masked-8": (8, 16, 256, 520, 16, 8192, 100, "auto", False, {"action_mask": "room"}),
}


def sha(x):
    return hashlib.sha256(np.ascontiguousarray(x.cpu().numpy() if hasattr(x, "cpu") else x).tobytes()).hexdigest()


def make_algo(torch, C_, nodes, H, N, T, mb, rows, prec, per_step, attrs=None):
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
    for k, v in (attrs or {}).items():
        setattr(cfg, k, v)
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


SHAPES = {  # path: (precision name, rows, [(D, H, A)])
    "fp32": ("FP32", 128, [(3 * A, 256, A) for A in (2, 4, 8)]),
    "sf16": ("SF16", 256, [(3 * A, 256, A) for A in (2, 4, 8)]),
    "wide": ("WIDE", 256, [(48, 384, 16)]),
}


def policy(torch, D, H, A, prec):
    from rlks import _lib
    from rlks.policy import PolicyParams

    p = PolicyParams(D, H, A, device=torch.device("cuda", 0), seed=11 + A)
    p.desc.precision = getattr(_lib, "RLKS_PRECISION_" + prec)
    return p


def workspace(torch, p, rows):
    from rlks import _lib

    wsb = C.c_int64()
    _lib.call("rlks_ppo_workspace_bytes", C.byref(p.desc), rows, C.byref(wsb))
    return torch.zeros(wsb.value, dtype=torch.uint8, device=p.flat.device)


def ws_digest(torch):
    from rlks import _lib

    res = {}
    for path, (prec, rows, shapes) in SHAPES.items():
        for D, H, A in shapes:
            p = policy(torch, D, H, A, prec)
            ws = workspace(torch, p, rows)
            r = {"bytes": ws.numel(), "minibatch_stride": _lib.lib().rlks_minibatch_stride(C.byref(p.desc)),
                 "packed_stride": _lib.lib().rlks_packed_stride(C.byref(p.desc))}
            entry, n = {"sf16": ("rlks_debug_sf_handoff", 4), "wide": ("rlks_debug_wide_bufs", 6)}.get(path, (None, 0))
            if entry:
                out = (C.c_void_p * n)()
                _lib.call(entry, C.byref(p.desc), rows, ws.data_ptr(), out)
                r["offsets"] = [v - ws.data_ptr() for v in out]
            res[f"{path}-{A}"] = r
    return res


GT, GN, GROWS = 6, 128, 256  # the gather's train batch: 3 minibatches of 256 rows


def rollout_arrays(torch, D, A, seed):
    """a train batch [GT][GN] of the six arrays a minibatch record is made of, as rlks_rollout_bufs"""
    from rlks import _lib

    rec = torch.from_numpy(records(GT * GN, D, A, seed)).cuda()
    keep = {"obs": rec[:, :D].contiguous(), "logits": rec[:, D:D + A].contiguous(), "adv": rec[:, D + A].contiguous(),
            "vtarg": rec[:, D + A + 1].contiguous(), "logp": rec[:, D + A + 2].contiguous(),
            "actions": rec[:, D + A + 3].to(torch.int32)}
    b = _lib.RolloutBufs(T=GT, N=GN, **{k: v.data_ptr() for k, v in keep.items()})
    return b, keep


def packed_records(torch, p, b):
    from rlks import _lib

    ps = _lib.lib().rlks_packed_stride(C.byref(p.desc))
    packed = torch.zeros(GT * GN, ps, device="cuda")
    _lib.call("rlks_ppo_pack", C.byref(p.desc), C.byref(b), packed.data_ptr(), None)
    return packed


def gather_digest(torch):
    from rlks import _lib

    res = {}
    for path in ("sf16", "wide"):
        for D, H, A in SHAPES[path][2]:
            p = policy(torch, D, H, A, SHAPES[path][0])
            b, keep = rollout_arrays(torch, D, A, 200 + A)
            stride = _lib.lib().rlks_minibatch_stride(C.byref(p.desc))
            packed = packed_records(torch, p, b) if path == "sf16" else None
            r = {} if packed is None else {"packed": sha(packed)}
            for groups in (1, 2, 16):
                for epoch in (0, 1):
                    for row0 in (0, 2 * GROWS):
                        mb = torch.zeros(GROWS, stride, device="cuda")
                        _lib.call("rlks_ppo_gather_grouped", C.byref(p.desc), C.byref(b), 77, epoch, groups, 0, row0, GROWS,
                                  None, mb.data_ptr(), None)
                        r[f"grouped-g{groups}-e{epoch}-r{row0}"] = sha(mb)
                        if packed is not None:
                            mb2 = torch.zeros(GROWS, stride, device="cuda")
                            _lib.call("rlks_ppo_gather_packed", C.byref(p.desc), packed.data_ptr(), GT, GN, 77, epoch, groups,
                                      0, row0, GROWS, mb2.data_ptr(), None)
                            r[f"packed-g{groups}-e{epoch}-r{row0}"] = sha(mb2)
            res[f"{path}-{A}"] = r
            del keep
    return res


ADAM = (3e-4, 0.9, 0.999, 1e-8)
GRAD_CLIP = 0.05  # well below these gradients' norm: the coefficient is not 1


def step_digest(torch, path, entry, groups):
    """two SGD steps through `entry` on the path's shape at 4 actions (wide: its own); step 1 gathers the
    next minibatch (not on the wide path, which has no packed records)"""
    from rlks import _lib

    prec, rows, shapes = SHAPES[path]
    D, H, A = shapes[len(shapes) // 2]
    p = policy(torch, D, H, A, prec)
    d, n = C.byref(p.desc), p.padded
    dev = p.flat.device
    b, keep = rollout_arrays(torch, D, A, 300 + A)
    packed = packed_records(torch, p, b) if path != "wide" else None
    mb = torch.from_numpy(records(rows, D, A, 100 + A)).to(dev)
    dyn = torch.tensor([0.0, 1.0, 0.2, 1.0 / rows, 0, 0, 0, 0], dtype=torch.float32, device=dev)
    co = C.byref(_lib.PpoCoeffs(0.3, 10.0, 1.0, 0.01))
    ws = workspace(torch, p, rows)
    grad, m, v = (torch.zeros(n, device=dev) for _ in range(3))
    stats = torch.zeros(_lib.RLKS_STAT_SIZE, dtype=torch.float64, device=dev)
    W = (ws.data_ptr(), ws.numel(), None)
    res = {}
    for step in (1, 2):
        x = None
        if step == 1 and packed is not None:
            x = C.byref(_lib.GatherNext(packed.data_ptr(), mb.data_ptr(), 77, rows, GT, GN, 0, groups, 0, rows))
        g = (d, co, p.flat.data_ptr(), dyn.data_ptr(), mb.data_ptr(), rows, grad.data_ptr(), stats.data_ptr())
        opt = (m.data_ptr(), v.data_ptr(), n, *ADAM, step)
        apply = (d, p.flat.data_ptr(), grad.data_ptr(), *opt)
        if entry == "sgd_step_next":
            _lib.call("rlks_ppo_sgd_step_next", *g, *opt, step - 1, x, *W)
        elif entry == "sgd_step_clip":
            _lib.call("rlks_ppo_sgd_step_clip", *g, *opt, step - 1, GRAD_CLIP, x, *W)
        else:
            if entry == "grad_step_part":
                _lib.call("rlks_ppo_grad_step_part", *g, step, step - 1, 1, None, *W)
                _lib.call("rlks_ppo_grad_step_part", *g, step, step - 1, 2, x, *W)
            else:
                _lib.call("rlks_ppo_grad_step_next", *g, step, step - 1, x, *W)
            if entry == "grad_step_next+apply_clip":
                _lib.call("rlks_ppo_adam_apply_clip", *apply, GRAD_CLIP, stats.data_ptr(), ws.data_ptr(), ws.numel(), rows,
                          None)
            else:
                _lib.call("rlks_ppo_adam_apply", *apply, ws.data_ptr(), ws.numel(), rows, None)
        torch.cuda.synchronize()
        assert torch.isfinite(p.flat).all() and float(grad.abs().max()) > 0
        res[f"step{step}"] = {"params": sha(p.flat), "adam_m": sha(m), "adam_v": sha(v), "grad": sha(grad),
                              "stats": sha(stats), "next_mb": sha(mb)}
    norm = torch.zeros(1, dtype=torch.float64, device=dev)
    _lib.call("rlks_grad_global_norm", d, grad.data_ptr(), n, norm.data_ptr(), *W)
    torch.cuda.synchronize()
    res["global_norm"] = sha(norm)
    del keep
    return res


STEPS = [("sf16", e, g) for e in ("sgd_step_next", "sgd_step_clip", "grad_step_next", "grad_step_part",
                                  "grad_step_next+apply_clip") for g in (1, 16)]
STEPS += [(path, e, 1) for path in ("fp32", "wide") for e in ("sgd_step_next", "sgd_step_clip")]


def compact(res):
    """the result as JSON with one line per case (an entry of a section), so that the file stays short"""
    secs = []
    for sec, v in res.items():
        if isinstance(v, dict) and all(isinstance(x, dict) for x in v.values()):
            cases = ",\n".join(f"  {json.dumps(k)}: {json.dumps(x)}" for k, x in v.items())
            secs.append(f" {json.dumps(sec)}: {{\n{cases}\n }}")
        else:
            secs.append(f" {json.dumps(sec)}: {json.dumps(v)}")
    return "{\n" + ",\n".join(secs) + "\n}\n"


def run(out):
    import torch
    from rlks import _lib

    res = {"lib": os.environ.get("RLKS_LIB_NAME", "tree"), "rollout": {}, "grad": {}, "sgd": {}}
    res["ws"] = ws_digest(torch)
    print("ws", {k: v["bytes"] for k, v in res["ws"].items()}, flush=True)
    res["gather"] = gather_digest(torch)
    print("gather", {k: len(v) for k, v in res["gather"].items()}, flush=True)
    res["step"] = {}
    for path, entry, groups in STEPS:
        res["step"][f"{path}-{entry}-g{groups}"] = step_digest(torch, path, entry, groups)
        print("step", path, entry, groups, res["step"][f"{path}-{entry}-g{groups}"]["step2"]["params"][:16], flush=True)
    logp = {}
    for name, row in ROLLOUTS.items():
        algo = make_algo(torch, *row)
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
    out.write_text(compact(res))
    np.savez(out.with_suffix(".logp.npz"), **logp)


def ulp_key(bits):
    """float32 bits -> integers whose difference is the distance in ulp (monotone over the reals)"""
    b = np.asarray(bits, np.uint32).astype(np.int64)
    return np.where(b & 0x80000000, 0x80000000 - b, b)


def compare(pa, pb):
    a, b = json.loads(Path(pa).read_text()), json.loads(Path(pb).read_text())
    print(f"{a['lib']} ({pa}) against {b['lib']} ({pb})")

    def leaves(x, path=""):
        if isinstance(x, dict):
            return {k2: v2 for k, v in x.items() for k2, v2 in leaves(v, f"{path}/{k}").items()}
        return {path[1:]: x}

    a.pop("lib"), b.pop("lib")
    la, lb = leaves(a), leaves(b)
    differ = sorted(k for k in la.keys() | lb.keys() if la.get(k) != lb.get(k))
    per = {sec: sum(1 for k in la if k.startswith(sec + "/")) for sec in a}
    print(f"{len(la)} values compared ({', '.join(f'{s} {n}' for s, n in per.items())}), {len(differ)} differ: "
          f"{', '.join(differ) if differ else 'none'}")
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
