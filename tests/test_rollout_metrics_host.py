"""CPU tests of the rollout metrics' host side (rlks.rollout_metrics): summarise and
combine on records a person can check, the NaN and floor cases, the config flag's round trip and the
header's declarations.  No device."""
import json
import math
import re

import numpy as np
import pytest

from conftest import ROOT
from rollout_metrics_ref import EXACT, reference, sum_bound

from rlks import _lib as L
from rlks.rollout_metrics import combine, record_size, summarise


def _record(A, C, **slots):
    r = np.zeros(L.RLKS_RM_FIXED + A + C)
    for k, v in slots.items():
        r[getattr(L, "RLKS_RM_" + k)] = v
    return r


def test_summarise_six_samples_by_hand():
    """rewards 1 -2 3 .5 4 -.5; values 1.5 .5 2 3 3 1; vtarg 2 0 2 4 3 1 (resid .5 -.5 0 1 0 0);
    actions 0 0 1 0 1 0; dones 0 0 1 0 0 1; utilisation columns summing to 1.5 and 3"""
    A = C = 2
    r = _record(A, C, ROWS=6, REWARD_SUM=6.0, REWARD_MIN=-2.0, REWARD_MAX=4.0, DONES=2, VALUE_SUM=11.0,
                VTARG_SUM=12.0, VTARG_SQ=34.0, RESID_SUM=1.0, RESID_SQ=1.5)
    r[L.RLKS_RM_FIXED:] = [4, 2, 1.5, 3.0]
    assert record_size(A, C) == len(r) == 14
    m = summarise(r, A, C)
    assert m["reward_mean"] == 1.0 and m["reward_min"] == -2.0 and m["reward_max"] == 4.0
    assert m["dones"] == 2 and isinstance(m["dones"], int)
    assert m["action_count"] == [4, 2] and all(isinstance(c, int) for c in m["action_count"])
    assert m["action_share"] == [4 / 6, 2 / 6]
    assert m["utilisation_mean"] == [0.25, 0.5]
    assert m["value_mean"] == 11 / 6 and m["vtarg_mean"] == 2.0
    # Var(vtarg) = 34/6 - 2^2 = 5/3; Var(resid) = 1.5/6 - (1/6)^2 = 2/9; 1 - (2/9) / (5/3) = 13/15
    assert m["vf_explained_var_rollout"] == pytest.approx(13 / 15, rel=1e-14)
    assert "pods_placed" not in m and "rejection_rate" not in m
    # node counters: [checks, placed, rejected, departed, write-backs, reads]
    m = summarise(r, A, C, counters=np.array([100, 30, 10, 7, 5, 6], np.int64))
    assert (m["pods_placed"], m["pods_rejected"], m["pods_departed"]) == (30, 10, 7)
    assert m["rejection_rate"] == 0.25
    json.dumps(m)  # plain Python numbers and lists
    with pytest.raises(ValueError):
        summarise(r, 3, 2)


def test_nan_cases_and_the_floor():
    A = C = 2
    # a constant vtarg: Var(vtarg) = 16/4 - 2^2 = 0 exactly
    flat = _record(A, C, ROWS=4, VTARG_SUM=8.0, VTARG_SQ=16.0, RESID_SUM=1.0, RESID_SQ=3.0)
    assert math.isnan(summarise(flat, A, C)["vf_explained_var_rollout"])
    # no arrivals: placed + rejected = 0
    m = summarise(flat, A, C, counters=[0, 0, 0, 5, 0, 0])
    assert math.isnan(m["rejection_rate"]) and m["pods_departed"] == 5
    # Var(resid) = 100 >> Var(vtarg) = 1: 1 - 100 is floored at -1
    bad = _record(A, C, ROWS=4, VTARG_SUM=0.0, VTARG_SQ=4.0, RESID_SUM=0.0, RESID_SQ=400.0)
    assert summarise(bad, A, C)["vf_explained_var_rollout"] == -1.0
    # a perfect fit: resid = 0
    good = _record(A, C, ROWS=4, VTARG_SUM=0.0, VTARG_SQ=4.0)
    assert summarise(good, A, C)["vf_explained_var_rollout"] == 1.0


def _buffers(rng, T, N, A, C):
    D = 3 * C
    rewards = (rng.standard_normal((T, N)) * 50).astype(np.float32)
    rewards.ravel()[rng.integers(0, T * N, 4)] = [5000.0, -5000.0, 4765.0, -0.0]
    values = (rng.standard_normal((T + 1, N)) * 30 + 100).astype(np.float32)
    vtarg = (values[:T] + rng.standard_normal((T, N)).astype(np.float32) * 20).astype(np.float32)
    return dict(actions=rng.integers(0, A, (T, N)).astype(np.int32), rewards=rewards, values=values, vtarg=vtarg,
                dones=(rng.random((T, N)) < 0.1).astype(np.uint8), obs=rng.random((T + 1, N, D)).astype(np.float32))


def test_combine_of_two_halves_is_the_whole():
    rng = np.random.default_rng(3)
    T, N, A, C = 10, 37, 5, 3
    b = _buffers(rng, T, N, A, C)
    whole, ab = reference(**b, A=A, C=C)
    h = T // 2
    # values / obs carry one more row than the others: the half's last row is not read
    lo = {k: v[:h + 1] if k in ("values", "obs") else v[:h] for k, v in b.items()}
    hi = {k: v[h:] for k, v in b.items()}
    both = combine([reference(**lo, A=A, C=C)[0], reference(**hi, A=A, C=C)[0]])
    exact = list(EXACT) + list(range(L.RLKS_RM_FIXED, L.RLKS_RM_FIXED + A))
    for s in range(len(whole)):
        if s in exact:
            assert both[s] == whole[s], s
        else:  # two roundings more than one np.sum: within the bound of any summation order
            assert abs(both[s] - whole[s]) <= sum_bound(T * N, ab[s]), s
    assert both[L.RLKS_RM_ROWS] == T * N and both[L.RLKS_RM_FIXED:L.RLKS_RM_FIXED + A].sum() == T * N
    one = reference(**lo, A=A, C=C)[0]
    np.testing.assert_array_equal(combine([one]), one)
    with pytest.raises(ValueError):
        combine([one, one[:-1]])


def test_config_flag_round_trips():
    from rlks.ppo import PPOConfig

    assert PPOConfig().rollout_metrics is False
    c = PPOConfig().reporting(rollout_metrics=True)
    assert c.rollout_metrics is True
    d = json.loads(json.dumps(c.to_dict()))
    assert d["rollout_metrics"] is True
    assert PPOConfig.from_dict(d).rollout_metrics is True
    assert PPOConfig.from_dict(json.loads(json.dumps(PPOConfig().to_dict()))).rollout_metrics is False
    # the other reporting arguments are untouched by it
    assert PPOConfig().reporting(rollout_metrics=True, json_lines="x.jsonl").metrics_json_lines == "x.jsonl"


def test_header_declares_the_entry_points_and_slots():
    h = (ROOT / "include" / "rlks.h").read_text()
    for name in ("rlks_rollout_metrics_size", "rlks_rollout_metrics_workspace_bytes", "rlks_rollout_metrics"):
        assert re.search(r"^int " + name + r"\(", h, flags=re.M), name
        assert name in L.SIGNATURES
    t = (ROOT / "include" / "rlks_types.h").read_text()
    names = ["ROWS", "REWARD_SUM", "REWARD_MIN", "REWARD_MAX", "DONES", "VALUE_SUM", "VTARG_SUM", "VTARG_SQ",
             "RESID_SUM", "RESID_SQ", "FIXED"]
    for i, n in enumerate(names):  # the enum's values and their Python mirror
        assert re.search(rf"RLKS_RM_{n} = {i}\b", t), n
        assert getattr(L, "RLKS_RM_" + n) == i


def test_json_lines_line_keeps_custom_metrics():
    from rlks.metrics import JsonLinesReporter

    cm = {"action_share": [0.25, 0.75], "action_count": [1, 3], "vf_explained_var_rollout": float("nan")}
    line = JsonLinesReporter.__new__(JsonLinesReporter).line({"training_iteration": 1, "custom_metrics": cm})
    back = json.loads(json.dumps(line))
    assert back["custom_metrics"]["action_share"] == [0.25, 0.75] and back["custom_metrics"]["action_count"] == [1, 3]
    assert back["custom_metrics"]["vf_explained_var_rollout"] is None  # the reporter's NaN -> null rule
    assert "custom_metrics" not in JsonLinesReporter.__new__(JsonLinesReporter).line({"training_iteration": 1})
