"""Off-policy evaluation of logged decisions: what would a policy have earned on the decisions
another one actually made?

    log = DecisionLog.collect(old_algo, 120, lanes=64)       # or DecisionLog.from_rollout(algo), or your own arrays
    log.save("decisions.npz")
    res = estimate("path/to/checkpoint_000010", DecisionLog.load("decisions.npz"), gamma=0.99)
    res["wis"]["v_target"], res["wis"]["v_behavior"], res["ess"]

RLlib's off-policy estimators ``ImportanceSampling`` and ``WeightedImportanceSampling`` restated (RLlib is not
part of the reference tree; tests/ope_ref.py pins the arithmetic): per episode the cumulative ratio
p_k = prod_{j <= k} pi_new(a_j | s_j) / pi_old(a_j | s_j) weighs the discounted rewards, WIS divides it by its
mean w_k over the episodes that reach step k.  Two deviations from RLlib: the cumulative log ratio enters exp()
as min(L_k, 700), where RLlib lets the product overflow (the steps this changes are counted in
``clamped_steps``), and a WIS term is 0.0 where every p_k at that step underflowed to 0, where RLlib divides.

The target's logits come from ``PolicyParams.forward`` (which applies an observation filter), its logp of the
logged actions from ``rlks_ope_logp`` and the estimate from ``rlks_ope_estimate``; ``summarise`` is the pure
numpy last step.  One rank: the WIS weights need the sum over every episode of the log.
"""
from __future__ import annotations

import ctypes as C
import os
from pathlib import Path

import numpy as np

from . import _lib
from ._lib import (RLKS_OPE_BAD_ROWS, RLKS_OPE_CLAMPED, RLKS_OPE_EPISODES, RLKS_OPE_MAX_LEN, RLKS_OPE_PEND_SQ,
                   RLKS_OPE_PEND_SUM, RLKS_OPE_SIZE, RLKS_OPE_STEPS, RLKS_OPE_VB_SQ, RLKS_OPE_VB_SUM, RLKS_OPE_VIS_SQ,
                   RLKS_OPE_VIS_SUM, RLKS_OPE_VWIS_SQ, RLKS_OPE_VWIS_SUM)
from .sampling import check_mask_width, mask_on, pack_mask, pack_mask_device, resolve_policy

METHODS = {"is": (RLKS_OPE_VIS_SUM, RLKS_OPE_VIS_SQ), "wis": (RLKS_OPE_VWIS_SUM, RLKS_OPE_VWIS_SQ)}
FORWARD_CHUNK = 1 << 20  # rows per target forward: bounds the logits buffer
_FIELDS = ("obs", "actions", "logp", "rewards", "dones")


def _is_tensor(x):
    return hasattr(x, "detach") and hasattr(x, "device")


def _host(x):
    return x.detach().cpu().numpy() if _is_tensor(x) else np.asarray(x)


def _dtype_name(x):
    return str(x.dtype).replace("torch.", "")


def _check_methods(methods):
    methods = (methods,) if isinstance(methods, str) else tuple(methods)
    bad = [m for m in methods if m not in METHODS]
    if bad or not methods:
        raise ValueError(f"unknown off-policy estimation method(s) {bad}; choose from {sorted(METHODS)}")
    return methods


class DecisionLog:
    """A time-major record of decisions: obs [T, N, D] float32 (raw, before any observation filter), actions
    [T, N] int32, logp [T, N] float32 (the behaviour policy's log-probability of the action), rewards [T, N]
    float32, dones [T, N] uint8 or bool, and optionally the action mask the behaviour policy decided under:
    bool [T, N, A] (True = allowed) or the packed words [T, N] (uint64; int64 for a device tensor), bit a of a
    word = action a allowed.  Arrays are numpy arrays or device tensors and are kept as given; the mask is kept
    as words.  Shapes and dtypes are validated, and on the host also the action range (>= 0, and < A where a
    bool mask or `n_actions` tells A)."""

    def __init__(self, obs, actions, logp, rewards, dones, action_mask=None, *, n_actions=None):
        if getattr(obs, "ndim", 0) != 3:
            raise ValueError(f"obs must be [T, N, D], got shape {list(np.shape(obs))}")
        T, N, D = (int(s) for s in obs.shape)
        if T < 1 or N < 1 or D < 1:
            raise ValueError(f"an empty log: obs has shape {[T, N, D]}")
        want = {"obs": ("float32",), "actions": ("int32",), "logp": ("float32",), "rewards": ("float32",),
                "dones": ("uint8", "bool")}
        given = dict(zip(_FIELDS, (obs, actions, logp, rewards, dones)))
        for name, x in given.items():
            if not hasattr(x, "shape") or not hasattr(x, "dtype"):
                raise ValueError(f"{name} must be a numpy array or a tensor")
            if name != "obs" and tuple(x.shape) != (T, N):
                raise ValueError(f"{name} must be [{T}, {N}] like obs' leading dimensions, got {list(x.shape)}")
            if _dtype_name(x) not in want[name]:
                raise ValueError(f"{name} must be {' or '.join(want[name])}, got {_dtype_name(x)}")
        if _dtype_name(dones) == "bool":
            if _is_tensor(dones):
                import torch

                dones = dones.to(torch.uint8)
            else:
                dones = dones.astype(np.uint8)
        self.T, self.N, self.D = T, N, D
        self.obs, self.actions, self.logp, self.rewards, self.dones = obs, actions, logp, rewards, dones
        self.n_actions = None if n_actions is None else int(n_actions)
        self.action_mask = None
        if action_mask is not None:
            self.action_mask = self._mask_words(action_mask)
        if not _is_tensor(actions):
            a = np.asarray(actions)
            if a.min() < 0 or (self.n_actions is not None and a.max() >= self.n_actions):
                top = "A" if self.n_actions is None else str(self.n_actions)
                raise ValueError(f"actions outside [0, {top}): min {int(a.min())}, max {int(a.max())}")

    def _mask_words(self, m):
        T, N = self.T, self.N
        name = _dtype_name(m)
        if name == "bool":
            if m.ndim != 3 or tuple(m.shape[:2]) != (T, N):
                raise ValueError(f"a bool action_mask must be [{T}, {N}, A], got {list(m.shape)}")
            A = int(m.shape[2])
            check_mask_width(A)
            if self.n_actions not in (None, A):
                raise ValueError(f"action_mask has {A} actions, n_actions says {self.n_actions}")
            self.n_actions = A
            if _is_tensor(m):
                return pack_mask_device(m)
            return pack_mask(m.reshape(T * N, A), T * N, A).reshape(T, N)
        if name not in ("uint64", "int64") or tuple(m.shape) != (T, N):
            raise ValueError(f"action_mask must be bool [{T}, {N}, A] or 64-bit words [{T}, {N}], got {name} "
                             f"{list(m.shape)}")
        return m if _is_tensor(m) else np.asarray(m).view(np.uint64)

    def to_numpy(self) -> dict:
        """the log's arrays on the host; the mask as uint64 words"""
        out = {k: np.ascontiguousarray(_host(getattr(self, k))) for k in _FIELDS}
        if self.action_mask is not None:
            out["action_mask"] = np.ascontiguousarray(_host(self.action_mask)).view(np.uint64)
        return out

    def save(self, path):
        """one .npz (numpy appends the suffix when `path` has none)"""
        arrays = self.to_numpy()
        if self.n_actions is not None:
            arrays["n_actions"] = np.int64(self.n_actions)
        np.savez(os.fspath(path), **arrays)

    @classmethod
    def load(cls, path) -> "DecisionLog":
        with np.load(os.fspath(path)) as z:
            missing = [k for k in _FIELDS if k not in z.files]
            if missing:
                raise ValueError(f"{path} is not a decision log: no {missing}")
            return cls(*(z[k] for k in _FIELDS), action_mask=z["action_mask"] if "action_mask" in z.files else None,
                       n_actions=int(z["n_actions"]) if "n_actions" in z.files else None)

    @classmethod
    def from_rollout(cls, algo) -> "DecisionLog":
        """a snapshot (copies, on the device) of a PPO's last rollout: call it after train() or rollout().  With
        an observation filter the raw observations are taken; with action_mask="room" the masks are recovered
        from the stored logits (masked where <= RLKS_MASKED_LOGIT_MAX)."""
        T, b = algo.T, algo.buf
        obs = (algo.raw if algo.raw is not None else b["obs"])[:T].clone()
        mask = None
        if algo.action_mask is not None:
            mask = b["logits"] > _lib.RLKS_MASKED_LOGIT_MAX
        return cls(obs, b["actions"].clone(), b["logp"].clone(), b["rewards"].clone(), b["dones"].clone(),
                   action_mask=mask, n_actions=algo.A)

    @classmethod
    def collect(cls, policy, steps, *, lanes, table=None, nodes=None, seed=0, explore=True) -> "DecisionLog":
        """`steps` decisions on each of `lanes` lanes of a fresh VecK8sMultiCloudEnv (Philox noise keyed by
        `seed`, auto-reset) under `policy`, a PPO or a PolicyParams: per step the forward, then sample_step, or,
        for a PPO with action_mask="room", the env's mask, masked_sample and step.  Everything stays on the
        device."""
        import torch

        from .env import VecK8sMultiCloudEnv
        from .evaluation import decider
        from .tables import load_table

        steps, lanes = int(steps), int(lanes)
        if steps < 1 or lanes < 1:
            raise ValueError("collect: steps and lanes must be positive")
        table = table if table is not None else load_table()
        pol = resolve_policy(policy, table)
        masked = mask_on(pol, None, nodes)
        A = table.n_clouds
        env = VecK8sMultiCloudEnv(lanes, table=table, seed=int(seed), noise="philox", autoreset=True, nodes=nodes,
                                  device=pol.params.flat.device)
        try:
            dev = env.device
            f32 = dict(dtype=torch.float32, device=dev)
            obs_l = torch.empty(steps, lanes, 3 * A, **f32)
            act_l = torch.empty(steps, lanes, dtype=torch.int32, device=dev)
            logp_l, rew_l = torch.empty(steps, lanes, **f32), torch.empty(steps, lanes, **f32)
            done_l = torch.empty(steps, lanes, dtype=torch.uint8, device=dev)
            mask_l = torch.empty(steps, lanes, dtype=torch.int64, device=dev) if masked else None
            decide, forward = decider(pol, env, explore=explore, masked=masked)
            obs = env.reset()
            for t in range(steps):
                obs_l[t].copy_(obs)
                if masked:
                    _lib.call("rlks_env_action_mask", env.handle, _lib.ptr(mask_l[t]), env.dev.stream)
                    a, lp = decide(obs, t)
                    obs, r, done, _, _ = env.step(a)  # r: f64 -> f32 below, as the rollout stores it
                else:  # the draw and the step in one launch
                    a, lp, obs, r, done = env.sample_step(forward(obs), explore=explore)
                act_l[t].copy_(a)
                logp_l[t].copy_(lp)
                rew_l[t].copy_(r)
                done_l[t].copy_(done)
            env.check_status()
            return cls(obs_l, act_l, logp_l, rew_l, done_l, action_mask=mask_l, n_actions=A)
        finally:
            env.close()


def _on(x, dev, dtype):
    import torch

    t = x if _is_tensor(x) else torch.from_numpy(np.ascontiguousarray(x))
    return t.to(device=dev, dtype=dtype).contiguous()


def target_logp(policy, log):
    """float32 [T, N] on the device: the policy's log-probability of every logged action, under the log's masks
    for a masked policy.  Forwards in row chunks of at most FORWARD_CHUNK rows, then rlks_ope_logp."""
    import torch

    if isinstance(policy, (str, Path)):  # a checkpoint written by PPO.save()
        from .serving import PolicyServer

        policy = PolicyServer.from_checkpoint(policy)
    params, extra, masked, _keep = resolve_policy(policy)
    if not isinstance(log, DecisionLog):
        raise ValueError("log must be a DecisionLog")
    if masked and log.action_mask is None:
        raise ValueError("this policy was trained with action_mask='room' and the log carries no action mask: a "
                         "masked policy evaluated unmasked would be a silent error")
    if log.D != params.D:
        raise ValueError(f"the log's observations have {log.D} columns, the policy {params.D}")
    if log.n_actions not in (None, params.A):
        raise ValueError(f"the log has {log.n_actions} actions, the policy {params.A}")
    if not _is_tensor(log.actions):
        a = np.asarray(log.actions)
        if a.max() >= params.A:
            raise ValueError(f"logged actions up to {int(a.max())}, the policy has {params.A} actions")
    dev = params.flat.device
    rows, A = log.T * log.N, params.A
    with torch.cuda.device(dev):
        obs = _on(log.obs, dev, torch.float32).view(rows, log.D)
        act = _on(log.actions, dev, torch.int32).view(rows)
        bits = None
        if masked:
            m = log.action_mask
            bits = _on(m if _is_tensor(m) else np.asarray(m).view(np.int64), dev, torch.int64).view(rows)
        out = torch.empty(rows, dtype=torch.float32, device=dev)
        chunk = min(rows, FORWARD_CHUNK)
        logits = torch.empty(chunk, A, dtype=torch.float32, device=dev)
        values = torch.empty(chunk, dtype=torch.float32, device=dev)
        stream = torch.cuda.current_stream(dev).cuda_stream
        for i in range(0, rows, chunk):
            m = min(chunk, rows - i)
            x = obs[i:i + m]
            if extra is not None:
                x = extra.apply(x)
            params.forward(x, logits[:m], values[:m])
            _lib.call("rlks_ope_logp", _lib.ptr(logits), _lib.ptr(act[i:i + m]),
                      _lib.ptr(bits[i:i + m]) if bits is not None else None, m, A, _lib.ptr(out[i:i + m]), stream)
    return out.view(log.T, log.N)


def run_estimate(logp_new, logp_old, rewards, dones, gamma, drop_truncated=False, per_episode=False):
    """rlks_ope_estimate on device tensors [T, N] -> (record float64 [RLKS_OPE_SIZE] on the host, ep_out float64
    [T, N, 4] on the device, NaN outside the counted segments' last steps, or None)"""
    import torch

    T, N = (int(s) for s in logp_new.shape)
    dev = logp_new.device
    with torch.cuda.device(dev):
        wsb = C.c_int64()
        _lib.call("rlks_ope_workspace_bytes", T, N, C.byref(wsb))
        ws = torch.empty(wsb.value // 8 + 1, dtype=torch.float64, device=dev)
        rec = torch.zeros(RLKS_OPE_SIZE, dtype=torch.float64, device=dev)
        ep = torch.full((T, N, 4), float("nan"), dtype=torch.float64, device=dev) if per_episode else None
        _lib.call("rlks_ope_estimate", _lib.ptr(logp_new), _lib.ptr(logp_old), _lib.ptr(rewards), _lib.ptr(dones), T, N,
                  float(gamma), int(bool(drop_truncated)), _lib.ptr(rec), _lib.ptr(ep), _lib.ptr(ws), ws.numel() * 8,
                  torch.cuda.current_stream(dev).cuda_stream)
        return rec.cpu().numpy(), ep


def _std(sq, s, n):
    m = s / n
    return float(np.sqrt(max(0.0, sq / n - m * m)))


def summarise(record, methods=("is", "wis")) -> dict:
    """the estimators' result from a record (double[RLKS_OPE_SIZE]); pure numpy.  Per method RLlib's keys:
    v_behavior and v_target (means over the episodes), their population standard deviations (numpy's ddof 0),
    v_gain = v_target / max(v_behavior, 1e-8) and v_delta = v_target - v_behavior; then the counts and
    ess = (sum p_end)^2 / sum p_end^2, the effective number of episodes behind the IS estimate.  ValueError for
    a record with BAD_ROWS > 0 (a logp that is not finite) or without an episode."""
    methods = _check_methods(methods)
    r = np.asarray(record, np.float64)
    if r.shape != (RLKS_OPE_SIZE,):
        raise ValueError(f"summarise: a record of {RLKS_OPE_SIZE} doubles, got shape {r.shape}")
    if r[RLKS_OPE_BAD_ROWS] > 0:
        raise ValueError(f"{int(r[RLKS_OPE_BAD_ROWS])} logged steps have a logp (target or behaviour) that is not "
                         "finite; the estimate is undefined")
    E = float(r[RLKS_OPE_EPISODES])
    if E <= 0:
        raise ValueError("no counted episode in the log (drop_truncated with no finished episode?)")
    vb, vb_std = float(r[RLKS_OPE_VB_SUM] / E), _std(r[RLKS_OPE_VB_SQ], r[RLKS_OPE_VB_SUM], E)
    out = {}
    for m in methods:
        s_sum, s_sq = METHODS[m]
        vt = float(r[s_sum] / E)
        out[m] = {"v_behavior": vb, "v_behavior_std": vb_std, "v_target": vt, "v_target_std": _std(r[s_sq], r[s_sum], E),
                  "v_gain": vt / max(vb, 1e-8), "v_delta": vt - vb}
    psq = float(r[RLKS_OPE_PEND_SQ])
    out.update(episodes=int(round(E)), steps=int(round(r[RLKS_OPE_STEPS])), max_len=int(round(r[RLKS_OPE_MAX_LEN])),
               clamped_steps=int(round(r[RLKS_OPE_CLAMPED])),
               ess=float(r[RLKS_OPE_PEND_SUM]) ** 2 / psq if psq > 0 else 0.0)
    return out


def estimate(policy, log, methods=("is", "wis"), gamma=0.99, drop_truncated=False, per_episode=False) -> dict:
    """{"is": {...}, "wis": {...}, "episodes", "steps", "max_len", "clamped_steps", "ess"} (summarise) for the
    target `policy` (a PPO, a PolicyServer, a PolicyParams or a checkpoint path) on the DecisionLog `log`.
    An episode is a lane's steps up to and including a done; the steps after a lane's last done form a
    truncated episode, counted unless drop_truncated.  per_episode adds "per_episode": {"v_behavior", "v_is",
    "v_wis", "p_end"}, float64 arrays over the counted episodes in (t_end, n) row-major order."""
    import torch

    methods = _check_methods(methods)
    gamma = float(gamma)
    if not (0.0 <= gamma <= 1.0):
        raise ValueError(f"gamma must be in [0, 1], got {gamma}")
    lp_new = target_logp(policy, log)
    dev = lp_new.device
    lp_old, rew = _on(log.logp, dev, torch.float32), _on(log.rewards, dev, torch.float32)
    dones = _on(log.dones, dev, torch.uint8)
    rec, ep = run_estimate(lp_new, lp_old, rew, dones, gamma, drop_truncated, per_episode)
    out = summarise(rec, methods)
    if per_episode:
        ends = dones != 0
        if not drop_truncated:
            ends[-1] = True
        rows = ep[ends].cpu().numpy()  # boolean indexing walks (t, n) in row-major order
        out["per_episode"] = {k: rows[:, j].copy() for j, k in enumerate(("v_behavior", "v_is", "v_wis", "p_end"))}
    return out
