"""Host side of the per-iteration rollout metrics (PPOConfig.reporting(rollout_metrics=True),
DESIGN.md §20): pure numpy, no device use.

The device leaves one record per rank and iteration (rlks_rollout_metrics, include/rlks.h):
double[RLKS_RM_FIXED + A + C] = the RLKS_RM_* slots, A action counts, C sums of the utilisation
columns.  combine() merges the ranks' records, summarise() turns a record (and, on node-level envs,
the iteration's pod-counter deltas) into result["custom_metrics"], RLlib's key for user metrics.

vf_explained_var_rollout is not RLlib's vf_explained_var: RLlib's is a per-minibatch figure from
inside the loss, with the value net as it is at that SGD step; this one is taken once over the whole
train batch with the values the rollout recorded, before any SGD step of the iteration.
"""
from __future__ import annotations

import numpy as np

from ._lib import (RLKS_RM_DONES, RLKS_RM_FIXED, RLKS_RM_RESID_SQ, RLKS_RM_RESID_SUM, RLKS_RM_REWARD_MAX,
                   RLKS_RM_REWARD_MIN, RLKS_RM_REWARD_SUM, RLKS_RM_ROWS, RLKS_RM_VALUE_SUM, RLKS_RM_VTARG_SQ,
                   RLKS_RM_VTARG_SUM)

# rlks_env_counters slots
COUNTER_PLACED, COUNTER_REJECTED, COUNTER_DEPARTED = 1, 2, 3


def record_size(A: int, C: int) -> int:
    return RLKS_RM_FIXED + int(A) + int(C)


def combine(parts):
    """one record from the ranks' records, in the order given: sums and counts added, min / max taken"""
    parts = [np.asarray(p, np.float64) for p in parts]
    if not parts or any(p.shape != parts[0].shape or p.ndim != 1 for p in parts):
        raise ValueError("combine: records of one size, at least one")
    out = parts[0].copy()
    for p in parts[1:]:
        lo, hi = min(out[RLKS_RM_REWARD_MIN], p[RLKS_RM_REWARD_MIN]), max(out[RLKS_RM_REWARD_MAX], p[RLKS_RM_REWARD_MAX])
        out += p
        out[RLKS_RM_REWARD_MIN], out[RLKS_RM_REWARD_MAX] = lo, hi
    return out


def _variance(sq, s, n):
    """population variance from sum x^2, sum x and the count, never below 0"""
    m = s / n
    return max(0.0, sq / n - m * m)


def summarise(record, A: int, C: int, counters=None) -> dict:
    """result["custom_metrics"] from a record; counters: this iteration's deltas of the six node
    counters (rlks_env_counters, integers) on a node-level env, else None"""
    r = np.asarray(record, np.float64)
    A, C = int(A), int(C)
    if r.shape != (record_size(A, C),):
        raise ValueError(f"summarise: a record of {record_size(A, C)} doubles, got shape {r.shape}")
    n = float(r[RLKS_RM_ROWS])
    if n <= 0:
        raise ValueError("summarise: an empty record")
    counts = [int(round(x)) for x in r[RLKS_RM_FIXED:RLKS_RM_FIXED + A]]
    var_t = _variance(r[RLKS_RM_VTARG_SQ], r[RLKS_RM_VTARG_SUM], n)
    var_r = _variance(r[RLKS_RM_RESID_SQ], r[RLKS_RM_RESID_SUM], n)
    out = {
        "reward_mean": float(r[RLKS_RM_REWARD_SUM] / n),
        "reward_min": float(r[RLKS_RM_REWARD_MIN]),
        "reward_max": float(r[RLKS_RM_REWARD_MAX]),
        "dones": int(round(r[RLKS_RM_DONES])),
        "action_count": counts,
        "action_share": [c / n for c in counts],
        "utilisation_mean": [float(x / n) for x in r[RLKS_RM_FIXED + A:]],
        "value_mean": float(r[RLKS_RM_VALUE_SUM] / n),
        "vtarg_mean": float(r[RLKS_RM_VTARG_SUM] / n),
        "vf_explained_var_rollout": max(-1.0, 1.0 - var_r / var_t) if var_t > 0 else float("nan"),
    }
    if counters is not None:
        placed, rejected, departed = (int(counters[i]) for i in (COUNTER_PLACED, COUNTER_REJECTED, COUNTER_DEPARTED))
        arrived = placed + rejected
        out.update(pods_placed=placed, pods_rejected=rejected, pods_departed=departed,
                   rejection_rate=rejected / arrived if arrived else float("nan"))
    return out
