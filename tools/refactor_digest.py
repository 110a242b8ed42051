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
         group: inside the reduce's launch on sf16; 16: a launch of its own), then rlks_grad_global_norm
decide:  what the Python decide paths return, through public entries only: compute_actions and
         compute_single_action (with the call counters), the server's fallback with full_fetch, evaluate,
         evaluate_nodes, evaluate_lanes, PPO.evaluate() with baselines, DecisionLog.collect and the estimate with
         the target passed as a PPO, a PolicyParams, a PolicyServer and a checkpoint.  Here the library is the same
         and the Python differs: copy this file into a checkout of the other commit and run it there too.

  python tools/refactor_digest.py --decide <out.json>      the decide group alone"""
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
    "table-fp32-128-2": (2, None, 256, 32776, 2, 128, 100, "fp32", False),  # past 32,768 lanes: 128-row tiles
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


# ---------------------------------------------------------------------------- decide
def decide_algo(torch, table, nodes=None, H=256, **attrs):
    from rlks.ppo import PPO, PPOConfig

    cfg = (PPOConfig().framework("torch")
           .training(train_batch_size=64 * 4, sgd_minibatch_size=256, num_sgd_iter=1, lr=3e-4,
                     model={"fcnet_hiddens": [H, H]})
           .debugging(seed=5))
    cfg.num_envs, cfg.table, cfg.nodes = 64, table, nodes
    for k, v in attrs.items():
        setattr(cfg, k, v)
    return PPO(config=cfg, device=torch.device("cuda", 0))


def decide_masks(A, n, seed):
    """bool [n, A]: random rows, row 0 without an allowed action, row 1 (n > 1) only the top bit (bit 63 at A = 64)"""
    m = np.random.default_rng(seed).random((n, A)) < 0.5
    m[0] = False
    if n > 1:
        m[1] = False
        m[1, A - 1] = True
    return m


def decide_digest(torch, tmp):
    """what the Python decide paths return (rlks.sampling, rlks.evaluation, rlks.offline), public entries only,
    so that the same file runs on a checkout from before the fold"""
    import dataclasses
    import warnings

    import rule_ref as rr
    from rlks.evaluation import evaluate, evaluate_lanes, evaluate_nodes
    from rlks.offline import DecisionLog, estimate, run_estimate, target_logp
    from rlks.policy import PolicyParams
    from rlks.tables import load_table, synthetic_table

    warnings.simplefilter("ignore", RuntimeWarning)  # save() of a node-level algorithm: env lanes are not kept
    dev = torch.device("cuda", 0)
    case = rr.CASES["J"]  # 3 clusters of 8 nodes that fill up (tests/test_action_mask_host.py::test_mask_cases_fill_up)
    jtab, jspec = synthetic_table(case.C, 100, seed=7), rr.node_spec(case)
    res = {}
    # compute_actions / compute_single_action
    algos = {"table-2": (decide_algo(torch, load_table()), False),
             "node-masked-8": (decide_algo(torch, synthetic_table(8, 100, seed=7), rr.node_spec(
                 dataclasses.replace(case, C=8, cpu=(300,) * 8, mem=(4096,) * 8)), action_mask="room"), True),
             "table-64-with-masks": (decide_algo(torch, synthetic_table(64, 8, seed=7)), True)}
    for name, (algo, with_mask) in algos.items():
        r = {"sample_calls": [algo.sample_calls]}
        obs = np.random.default_rng(5).random((300, algo.D)).astype(np.float32)
        for n in (300, 1):
            m = decide_masks(algo.A, n, 3) if with_mask else None
            for k, explore in enumerate((True, True, True, False)):
                r[f"n{n}-call{k}"] = sha(algo.compute_actions(obs[:n], explore=explore, action_mask=m))
                r["sample_calls"].append(algo.sample_calls)
        for row in (0, 1):
            m = decide_masks(algo.A, 2, 3)[row] if with_mask else None
            r[f"single-row{row}"] = [algo.compute_single_action(obs[row], explore=e, action_mask=m)
                                     for e in (True, True, True, False)]
            r["sample_calls"].append(algo.sample_calls)
        res[f"compute-{name}"] = r
        algo.stop()
    # the server's fallback (hidden 128: outside rlks_policy_act's scope)
    for name, attrs in (("plain", {}), ("masked", {"action_mask": "room"})):
        algo = decide_algo(torch, jtab, jspec, H=128, **attrs)
        srv = algo.server(max_rows=300)
        assert not srv.fused
        obs = np.random.default_rng(6).random((300, algo.D)).astype(np.float32)
        r = {"calls": [srv.calls]}
        for n in (300, 1):
            for mk in ((True,) if attrs else (False, True)):
                m = decide_masks(algo.A, n, 4) if mk else None
                for k, explore in enumerate((True, True, False)):
                    acts, info = srv.act(obs[:n], explore=explore, action_mask=m, full_fetch=True)
                    r[f"n{n}-mask{int(mk)}-call{k}"] = sha(acts) + "".join(sha(info[key])[:16] for key in sorted(info))
                    r["calls"].append(srv.calls)
        one, info = srv.act(obs[0], explore=True, action_mask=decide_masks(algo.A, 2, 4)[1], full_fetch=True)
        r["single"] = [one, info["action_logp"], info["vf_preds"], sha(info["action_dist_inputs"]), sha(info["action_prob"])]
        res[f"server-{name}"] = r
        srv.close()
        algo.stop()
    # evaluate
    params2 = PolicyParams(6, 256, 2, device=dev, seed=3)
    r = {}
    for pol in ("round_robin", "greedy", "cheapest", "myopic", "random", params2):
        e = evaluate(pol, 5, seed=42, device=dev)
        r[pol if isinstance(pol, str) else "params"] = {"rewards": sha(e.rewards), "actions": sha(e.actions), "names": list(e.names)}
    res["evaluate"] = r
    # evaluate_nodes / evaluate_lanes on the fill-up spec
    masked_algo = decide_algo(torch, jtab, jspec, action_mask="room")
    params3 = policy(torch, 9, 256, 3, "WIDE")  # 3 actions: the generic-width forward
    kw = dict(nodes=jspec, table=jtab, seed=11, device=dev)
    r, lanes = {}, {}
    for name, pol in (("myopic_with_room", "myopic_with_room"), ("least_loaded", "least_loaded"), ("params", params3),
                      ("masked-ppo", masked_algo)):
        e = evaluate_nodes(pol, 5, **kw)
        r[name] = {"rewards": sha(e.rewards), "actions": sha(e.actions), "choices": e.choices.tolist(),
                   "counts": [e.placed, e.rejected, e.departed], "mean_util": sha(e.mean_util), "extra": e.extra}
        if not isinstance(pol, str):
            for flag in (None, True, False):
                lanes[f"{name}-mask-{flag}"] = sha(evaluate_lanes(pol, 5, action_mask=flag, **kw))
                r[f"{name}-mask-{flag}"] = sha(evaluate_nodes(pol, 5, action_mask=flag, **kw).actions)
    assert r["masked-ppo-mask-True"] != r["masked-ppo-mask-False"], "the mask does not bite"
    res["evaluate_nodes"], res["evaluate_lanes"] = r, lanes
    # PPO.evaluate() with baselines
    table_algo = decide_algo(torch, load_table(), evaluation_baselines=["round_robin", "cheapest", "myopic"],
                             evaluation_duration=5)
    masked_algo.config.evaluation_baselines, masked_algo.config.evaluation_duration = ["myopic", "least_loaded"], 5
    res["ppo_evaluate"] = {"table": json.dumps(table_algo.evaluate(), sort_keys=True),
                           "node": json.dumps(masked_algo.evaluate(), sort_keys=True),
                           "node-unmasked": json.dumps(masked_algo.evaluate(action_mask=False), sort_keys=True)}
    # DecisionLog.collect and estimate() with the target given each way
    r, est = {}, {}
    # (4 clusters: a server built from a checkpoint forwards through the fused kernels, which take 2, 4 or 8
    # actions; nodes of one pod, so that clusters fill within the 6 steps)
    spec4 = rr.node_spec(dataclasses.replace(case, C=4, cpu=(100,) * 4, mem=(4096,) * 4))
    algo4 = decide_algo(torch, synthetic_table(4, 100, seed=7), spec4, action_mask="room")
    for name, algo, lanes_, nodes in (("table", table_algo, 4, None), ("node-masked", algo4, 8, spec4)):
        log = DecisionLog.collect(algo, 6, lanes=lanes_, table=algo.table, nodes=nodes, seed=9)
        r[name] = {k: sha(v) for k, v in log.to_numpy().items()}
        greedy = DecisionLog.collect(algo.params, 6, lanes=lanes_, table=algo.table, nodes=nodes, seed=9, explore=False)
        r[name + "-params-greedy"] = {k: sha(v) for k, v in greedy.to_numpy().items()}
        other = decide_algo(torch, algo.table, nodes, **({"action_mask": "room"} if nodes is not None else {}))
        other.params.flat.mul_(1.5)  # a target that is not the behaviour policy
        srv = other.server()
        for way, target in (("ppo", other), ("params", other.params), ("server", srv),
                            ("checkpoint", other.save(str(tmp / f"ckpt-{name}")))):
            lp = target_logp(target, log)
            rec, _ = run_estimate(lp, torch.as_tensor(log.logp, device=dev), torch.as_tensor(log.rewards, device=dev),
                                  torch.as_tensor(log.dones, device=dev), 0.99)
            est[f"{name}-{way}"] = {"logp": sha(lp), "record": sha(rec), "estimate": json.dumps(estimate(target, log),
                                                                                              sort_keys=True)}
        srv.close()
        other.stop()
    res["collect"], res["estimate"] = r, est
    for a in (masked_algo, table_algo, algo4):
        a.stop()
    return res


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


def run(out, only=None):
    import tempfile

    import torch
    from rlks import _lib

    res = {"lib": os.environ.get("RLKS_LIB_NAME", "tree")}
    with tempfile.TemporaryDirectory() as tmp:
        res["decide"] = decide_digest(torch, Path(tmp))
    print("decide", {k: len(v) for k, v in res["decide"].items()}, flush=True)
    if only == "decide":
        out.parent.mkdir(parents=True, exist_ok=True)
        out.write_text(compact(res))
        return
    res.update(rollout={}, grad={}, sgd={})
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
    elif sys.argv[1] == "--decide":
        run(Path(sys.argv[2]), only="decide")
    else:
        run(Path(sys.argv[1]))
