"""The policy side of a decision, written once: what a policy object is (resolve_policy, mask_on), how an
action mask becomes 64-bit words and back (pack_mask on the host, pack_mask_device / unpack_mask on tensors)
and how rows of logits are drawn outside an env (sample_rows).  PPO.compute_actions,
PolicyServer.act's fallback, rlks.evaluation and rlks.offline all come here.
"""
from __future__ import annotations

from typing import Any, NamedTuple

import numpy as np

from . import _lib

# Philox counter word 0 of policy-side draws (compute_actions, compute_single_action, PolicyServer.act): no
# env lane has this id, so these draws never repeat a rollout draw under the same key
SAMPLER_ID = 0xFFFFFFFF


def check_mask_width(A):
    if A > 64:
        raise ValueError(f"action_mask supports at most 64 actions, got {A}")


def pack_mask(mask, n, A):
    """bool [A] or [n, A] (True = allowed) -> uint64 [n], bit a of row i = mask[i, a]"""
    check_mask_width(A)
    m = np.asarray(mask, dtype=bool)
    if m.shape == (A,):
        m = np.broadcast_to(m, (n, A))
    if m.shape != (n, A):
        raise ValueError(f"action_mask must be [{A}] or [{n}, {A}], got {list(m.shape)}")
    return np.bitwise_or.reduce(np.left_shift(m.astype(np.uint64), np.arange(A, dtype=np.uint64)[None, :]), axis=1,
                                dtype=np.uint64)


def pack_mask_device(m):
    """pack_mask on a tensor: bool [..., A] -> int64 [...] on m's device (bit 63 through the int64's sign bit)"""
    import torch

    A = m.shape[-1]
    check_mask_width(A)
    w = torch.ones(A, dtype=torch.int64, device=m.device) << torch.arange(A, device=m.device)
    return (m.to(torch.int64) * w).sum(-1).contiguous()


def unpack_mask(bits, A):
    """the inverse: int64 [...] -> bool [..., A]"""
    import torch

    return ((bits[..., None] >> torch.arange(A, device=bits.device)) & 1).to(torch.bool)


def sample_rows(logits, *, seed, call, explore, bits=None, want_logp=False, stream):
    """TorchCategorical sample (explore) or argmax of logits [n, A] on the device sampler
    (rlks_sample_categorical, or rlks_sample_categorical_masked under `bits`, the mask words [n] as an int64
    device tensor or as pack_mask's uint64 array: a row without an allowed action counts as all allowed).
    Row i draws Philox({SAMPLER_ID, i, call, ACTION}, key = seed): the caller owns the counter `call` and
    advances it once per exploring call.
    -> (actions int32 [n], logp float32 [n] or None), device tensors"""
    import torch

    n, A = logits.shape
    dev = logits.device
    logits = logits.contiguous()
    act = torch.empty(n, dtype=torch.int32, device=dev)
    logp = torch.empty(n, dtype=torch.float32, device=dev) if want_logp else None
    ids = None
    if explore:
        idh = np.zeros((n, 3), np.uint32)
        idh[:, 0] = SAMPLER_ID
        idh[:, 1] = np.arange(n, dtype=np.uint32)
        idh[:, 2] = call & 0xFFFFFFFF
        ids = torch.from_numpy(idh.view(np.int32)).to(dev)
    if isinstance(bits, np.ndarray):  # last, so that the host work above runs beside the forward still in flight
        bits = torch.from_numpy(bits.view(np.int64)).to(dev)
    tail = (_lib.ptr(ids), seed & 0xFFFFFFFFFFFFFFFF, int(bool(explore)), _lib.ptr(act), _lib.ptr(logp), stream)
    if bits is not None:
        _lib.call("rlks_sample_categorical_masked", _lib.ptr(logits), _lib.ptr(bits), n, A, *tail)
    else:
        _lib.call("rlks_sample_categorical", _lib.ptr(logits), n, A, *tail)
    return act, logp


class Policy(NamedTuple):
    """resolve_policy's record"""
    params: Any   # PolicyParams
    filter: Any   # an ObsFilter to apply before params.forward (which applies params.obs_filter itself), or None
    masked: bool  # trained with action_mask="room": deciding unmasked would be a silent error
    keep: Any     # the object given: holds what the fields borrow


def resolve_policy(policy, table=None) -> Policy:
    """a PPO, a PolicyServer or a PolicyParams -> Policy.  What a string means is the caller's business
    (a rule name in rlks.evaluation, a checkpoint in rlks.offline).  With `table`, the policy must fit it."""
    from .serving import PolicyServer

    if isinstance(policy, PolicyServer):
        p = policy.params
        extra = policy.obs_filter if (policy.obs_filter is not None and p.obs_filter is None) else None
        pol = Policy(p, extra, policy.masked, policy)
    else:
        p = getattr(policy, "params", policy)
        if not hasattr(p, "forward") or not hasattr(p, "flat"):
            raise ValueError("policy must be a PPO, a PolicyServer, a PolicyParams or a checkpoint path")
        pol = Policy(p, None, getattr(policy, "action_mask", None) is not None, policy)
    if table is not None and (p.D != 3 * table.n_clouds or p.A != table.n_clouds):
        raise ValueError("policy shape does not match the table's clouds")
    return pol


def mask_on(pol, action_mask, nodes):
    """whether a run decides under the env's action mask.  pol: a Policy, or None for a
    rule; action_mask: None = the policy's own setting (off for bare parameters and rules)"""
    on = (pol is not None and pol.masked) if action_mask is None else bool(action_mask)
    if on and pol is None:
        raise ValueError("action_mask applies to a policy, not to a rule")
    if on and nodes is None:
        raise ValueError("action_mask needs a node-level env: a table env has room everywhere")
    return on
