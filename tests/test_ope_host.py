"""CPU tests of the off-policy evaluation surface (rlks.offline): the numpy restatement on the
worked example and on a bandit whose answer is known, summarise(), DecisionLog's round trip and validation, and
the three C declarations against the ctypes signature table."""
import ctypes as C
import re

import numpy as np
import pytest

import ope_ref
from conftest import ROOT
from rlks import _lib as L
from rlks.offline import DecisionLog, summarise


def split_log(ratio):
    """f32 logp_new, logp_old with logp_new - logp_old = log(ratio) to 2^-48 relative: the high and (negated)
    low f32 parts of the f64 logarithm"""
    lr = np.log(np.asarray(ratio, np.float64))
    hi = lr.astype(np.float32)
    lo = (lr - hi.astype(np.float64)).astype(np.float32)
    return hi, -lo


# the worked example: T = 3, N = 2, gamma = 0.5
RATIO = [[2, .5], [.25, 2], [4, .5]]
REWARD = np.array([[1, 2], [4, -2], [8, 4]], np.float32)
DONES = np.array([[0, 0], [1, 0], [0, 1]], np.uint8)
# a log ratio is held to 2^-48 relative (two f32 parts), |L| <= log 4 over at most 3 steps, values up to 32: the
# error through exp stays below 32 * 3 * 1.4 * 2^-48 ~ 5e-13
EX_TOL = 5e-13


def worked(drop):
    ln, lo = split_log(RATIO)
    return ope_ref.reference(ln, lo, REWARD, DONES, 0.5, drop_truncated=drop)


def test_worked_example_all_segments():
    ref = worked(False)
    # (t_end N + n) ascending: lane 0 t = 0..1, then lane 0 t = 2 (truncated), then lane 1 t = 0..2
    assert ref["ep_index"].tolist() == [2, 4, 5]
    want = np.array([[3, 3, 2.2564102564102570, 0.5], [8, 32, 14.769230769230770, 4], [2, 0.5, 0.12820512820512830, 0.5]])
    assert np.all(np.abs(ref["ep"] - want) <= EX_TOL), ref["ep"] - want
    assert np.all(np.abs(ref["S"] / ref["c"] - np.array([6.5 / 3, 1.5 / 2, 0.5 / 1])) <= EX_TOL)
    rec = ref["record"]
    assert (rec[L.RLKS_OPE_EPISODES], rec[L.RLKS_OPE_STEPS], rec[L.RLKS_OPE_MAX_LEN]) == (3, 6, 3)
    assert rec[L.RLKS_OPE_CLAMPED] == 0 and rec[L.RLKS_OPE_BAD_ROWS] == 0
    out = summarise(rec)
    assert out["episodes"] == 3 and out["steps"] == 6 and out["max_len"] == 3 and out["clamped_steps"] == 0
    assert abs(out["is"]["v_behavior"] - 13 / 3) <= EX_TOL and abs(out["is"]["v_target"] - 35.5 / 3) <= EX_TOL
    assert abs(out["wis"]["v_target"] - want[:, 2].sum() / 3) <= EX_TOL
    assert abs(out["is"]["v_behavior_std"] - np.std([3, 8, 2])) <= EX_TOL
    assert abs(out["is"]["v_target_std"] - np.std([3, 32, 0.5])) <= 10 * EX_TOL
    assert abs(out["wis"]["v_delta"] - (out["wis"]["v_target"] - 13 / 3)) <= EX_TOL
    assert abs(out["is"]["v_gain"] - (35.5 / 3) / (13 / 3)) <= EX_TOL
    assert abs(out["ess"] - 5.0 ** 2 / (0.25 + 16 + 0.25)) <= EX_TOL
    assert set(summarise(rec, methods=("wis",))) == {"wis", "episodes", "steps", "max_len", "clamped_steps", "ess"}


def test_worked_example_drop_truncated():
    ref = worked(True)
    assert ref["ep_index"].tolist() == [2, 5]
    want = np.array([[3, 3, 2.9333333333333336, 0.5], [2, 0.5, 0.4666666666666668, 0.5]])
    assert np.all(np.abs(ref["ep"] - want) <= EX_TOL), ref["ep"] - want
    rec = ref["record"]
    assert (rec[L.RLKS_OPE_EPISODES], rec[L.RLKS_OPE_STEPS], rec[L.RLKS_OPE_MAX_LEN]) == (2, 5, 3)


def test_bandit_is_and_wis_find_the_target_value():
    """T = 1, every done set: uniform behaviour over 2 actions, target (0.2, 0.8), rewards 1 | 3 + N(0, 1):
    the target earns 0.2 * 1 + 0.8 * 3 = 2.6"""
    N = 65536
    rng = np.random.default_rng(7)
    a = rng.integers(0, 2, N)
    r = (np.array([1.0, 3.0])[a] + rng.standard_normal(N)).astype(np.float32)[None, :]
    ln = np.log(np.array([0.2, 0.8]))[a].astype(np.float32)[None, :]
    lo = np.full((1, N), np.log(0.5), np.float32)
    ref = ope_ref.reference(ln, lo, r, np.ones((1, N), np.uint8), 0.99)
    out = summarise(ref["record"])
    assert out["episodes"] == N and out["max_len"] == 1
    for m in ("is", "wis"):
        se = out[m]["v_target_std"] / np.sqrt(N)
        print(m, out[m]["v_target"], "standard error", se)
        assert abs(out[m]["v_target"] - 2.6) <= 5 * se, (m, out[m], se)
    assert abs(out["is"]["v_behavior"] - 2.0) <= 5 * out["is"]["v_behavior_std"] / np.sqrt(N)
    assert 0.5 * N < out["ess"] < N  # ratios 0.4 and 1.6: ess = N (E p)^2 / E p^2 = N / 1.36


def test_extremes_in_the_restatement():
    """lr = -40 for 30 steps: exp(L_k) underflows to 0 from L = -760 on, there S_k == 0 and the WIS terms are 0.0,
    not NaN; lr = +40: the clamp at RLKS_OPE_LMAX bites from L = 720 on and everything per episode stays finite"""
    T = 30
    one = np.ones((T, 1), np.float32)
    d = np.zeros((T, 1), np.uint8)
    lo = ope_ref.reference(-40 * one, 0 * one, one, d, 1.0)
    assert lo["S"][-1] == 0.0 and np.all(np.isfinite(lo["ep"])) and lo["record"][L.RLKS_OPE_CLAMPED] == 0
    hi = ope_ref.reference(40 * one, 0 * one, one, d, 1.0)
    assert hi["record"][L.RLKS_OPE_CLAMPED] == 13 and np.all(np.isfinite(hi["ep"]))
    assert hi["ep"][0, 3] == np.exp(L.RLKS_OPE_LMAX)


def test_summarise_rejects_empty_and_bad_records():
    rec = worked(False)["record"]
    empty = np.zeros(L.RLKS_OPE_SIZE)
    with pytest.raises(ValueError, match="no counted episode"):
        summarise(empty)
    bad = rec.copy()
    bad[L.RLKS_OPE_BAD_ROWS] = 2
    with pytest.raises(ValueError, match="not finite"):
        summarise(bad)
    with pytest.raises(ValueError, match="unknown off-policy"):
        summarise(rec, methods=("dr",))
    with pytest.raises(ValueError):
        summarise(rec[:-1])


def make_log(T=5, N=3, D=6, A=2, mask=None, seed=0):
    rng = np.random.default_rng(seed)
    return DecisionLog(rng.random((T, N, D), dtype=np.float32), rng.integers(0, A, (T, N)).astype(np.int32),
                       -rng.random((T, N), dtype=np.float32), rng.standard_normal((T, N)).astype(np.float32),
                       (rng.random((T, N)) < 0.3).astype(np.uint8), action_mask=mask)


def test_decision_log_round_trip(tmp_path):
    rng = np.random.default_rng(1)
    m = rng.random((5, 3, 2)) < 0.7
    log = make_log(mask=m)
    assert log.n_actions == 2 and log.action_mask.dtype == np.uint64
    assert np.array_equal(log.action_mask, m[..., 0].astype(np.uint64) | (m[..., 1].astype(np.uint64) << np.uint64(1)))
    log.save(tmp_path / "log.npz")
    back = DecisionLog.load(tmp_path / "log.npz")
    a, b = log.to_numpy(), back.to_numpy()
    assert set(a) == set(b) == {"obs", "actions", "logp", "rewards", "dones", "action_mask"}
    for k in a:
        assert a[k].dtype == b[k].dtype and a[k].tobytes() == b[k].tobytes(), k
    assert (back.T, back.N, back.D, back.n_actions) == (5, 3, 6, 2)
    plain = make_log()
    plain.save(tmp_path / "plain.npz")
    assert DecisionLog.load(tmp_path / "plain.npz").action_mask is None
    # bool dones are taken as bytes; packed words are taken as they are
    w = DecisionLog(a["obs"], a["actions"], a["logp"], a["rewards"], a["dones"].astype(bool), action_mask=a["action_mask"])
    assert w.dones.dtype == np.uint8 and np.array_equal(w.action_mask, a["action_mask"])


def test_decision_log_validation():
    a = make_log().to_numpy()
    args = lambda **kw: [kw.get(k, a[k]) for k in ("obs", "actions", "logp", "rewards", "dones")]  # noqa: E731
    with pytest.raises(ValueError, match=r"obs must be \[T, N, D\]"):
        DecisionLog(*args(obs=a["obs"][0]))
    with pytest.raises(ValueError, match="actions must be"):
        DecisionLog(*args(actions=a["actions"][:-1]))
    with pytest.raises(ValueError, match="logp must be float32"):
        DecisionLog(*args(logp=a["logp"].astype(np.float64)))
    with pytest.raises(ValueError, match="actions must be int32"):
        DecisionLog(*args(actions=a["actions"].astype(np.int64)))
    with pytest.raises(ValueError, match="dones must be"):
        DecisionLog(*args(dones=a["dones"].astype(np.int32)))
    neg = a["actions"].copy()
    neg[0, 0] = -1
    with pytest.raises(ValueError, match="actions outside"):
        DecisionLog(*args(actions=neg))
    with pytest.raises(ValueError, match="actions outside"):
        DecisionLog(*args(), n_actions=1)
    with pytest.raises(ValueError, match="bool action_mask"):
        DecisionLog(*args(), action_mask=np.ones((5, 3), bool))
    with pytest.raises(ValueError, match="at most 64"):
        DecisionLog(*args(), action_mask=np.ones((5, 3, 65), bool))
    with pytest.raises(ValueError, match="action_mask must be"):
        DecisionLog(*args(), action_mask=np.ones((5, 3), np.float32))


C_TYPES = {"int": C.c_int, "int64_t": C.c_int64, "double": C.c_double}


def test_header_declarations_match_signatures():
    """the three entries as include/rlks.h declares them against _lib.SIGNATURES (the ABI test checks that the
    library exports every declared name)"""
    txt = re.sub(r"/\*.*?\*/", "", (ROOT / "include" / "rlks.h").read_text(), flags=re.S)
    for name in ("rlks_ope_logp", "rlks_ope_workspace_bytes", "rlks_ope_estimate"):
        m = re.search(r"^int\s+" + name + r"\s*\(([^)]*)\)\s*;", txt, flags=re.M)
        assert m, name
        want = []
        for arg in m.group(1).split(","):
            words = arg.replace("*", " * ").split()
            if "*" in words:
                want.append(C.POINTER(C.c_int64) if words[0] == "int64_t" else C.c_void_p)
            else:
                want.append(C_TYPES[[w for w in words if w != "const"][0]])
        assert L.SIGNATURES[name] == want, (name, L.SIGNATURES[name], want)
    assert (L.RLKS_OPE_SIZE, L.RLKS_OPE_LMAX) == (13, 700.0)
    enum = re.search(r"enum\s*\{\s*RLKS_OPE_EPISODES.*?\}", (ROOT / "include" / "rlks_types.h").read_text(), flags=re.S)
    txt = re.sub(r"/\*.*?\*/", "", enum.group(0), flags=re.S)
    for name, val in re.findall(r"(RLKS_OPE_[A-Z_]+)\s*=\s*(\d+)", txt):
        assert getattr(L, name) == int(val), name
