"""rlks_env_rule_actions: the baseline schedulers decided on the device.  The cases,
the numpy restatement of the rules and the C oracle's run of each case under each rule are in
tests/rule_ref.py.

A device env stepped by rule_actions + step must equal the oracle stepped by the restatement: actions,
observation bits, float64 rewards and terminations after every step, the six node counters at the end."""
import ctypes as C

import numpy as np
import pytest

import node_regimes as nr
import oracle
import rule_ref as rr

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

RULE_NAMES = sorted(rr.RULES, key=rr.RULES.get)


def _dev():
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    return torch.device("cuda", 0)


def _u32(x):
    x = x.cpu().numpy() if hasattr(x, "cpu") else np.asarray(x)
    return x.view(np.uint32)


def _u64(x):
    x = x.cpu().numpy() if hasattr(x, "cpu") else np.asarray(x)
    return x.view(np.uint64)


def _make_env(case, d, **kw):
    from rlks import VecK8sMultiCloudEnv

    return VecK8sMultiCloudEnv(case.n, table=nr.table(case), seed=nr.SEED, nodes=rr.node_spec(case),
                               env_offset=nr.ENV_OFFSET, device=d, **kw)


def test_rule_numbers_match_the_header():
    from rlks import _lib

    assert _lib.RULES == rr.RULES
    for name, num in rr.RULES.items():
        assert getattr(_lib, "RLKS_RULE_" + name.upper()) == num


@pytest.mark.parametrize("rule", RULE_NAMES)
@pytest.mark.parametrize("name", sorted(rr.CASES))
def test_node_env_follows_the_oracle(name, rule):
    case = rr.CASES[name]
    rr.check_guards(name)             # the case is in its regimes, before the device is touched
    exp = rr.oracle_run(name, rule)   # the oracle stepped by the numpy rule
    d = _dev()
    X = _make_env(case, d)
    X.counters(enable=1)
    np.testing.assert_array_equal(_u32(X.reset()), exp.obs_reset.view(np.uint32))
    for t in range(case.steps):
        a = X.rule_actions(rule if t % 2 else rr.RULES[rule])  # by name and by number
        assert a.dtype == torch.int32 and a.shape == (case.n,)
        np.testing.assert_array_equal(a.cpu().numpy(), exp.actions[t], err_msg=f"actions at step {t}")
        obs, rew, term, _, _ = X.step(a)
        np.testing.assert_array_equal(_u32(obs), exp.obs[t].view(np.uint32), err_msg=f"obs after step {t}")
        np.testing.assert_array_equal(_u64(rew), exp.rew[t].view(np.uint64), err_msg=f"reward at step {t}")
        np.testing.assert_array_equal(term.cpu().numpy(), exp.term[t], err_msg=f"terminated at step {t}")
    X.check_status()
    np.testing.assert_array_equal(X.counters().cpu().numpy(), exp.counters)
    X.close()


@pytest.mark.parametrize("rule", RULE_NAMES)
@pytest.mark.parametrize("noise,n,C_", [("mt19937", rr.TABLE_CASE["n"], rr.TABLE_CASE["C"]), ("philox", 300, 7)])
def test_table_env_follows_the_oracle(noise, n, C_, rule):
    """table envs (nodes_per_cluster = 0): the two-cloud MT19937 env of the reference and the general
    step kernel at C = 7 (row stride 21, a ragged last workgroup); 120 steps, past the auto-reset"""
    from rlks import VecK8sMultiCloudEnv
    from rlks.tables import synthetic_table

    d = _dev()
    tab = synthetic_table(C_, nr.N_ROWS, seed=nr.TABLE_SEED)
    X = VecK8sMultiCloudEnv(n, table=tab, seed=nr.SEED, noise=noise, env_offset=nr.ENV_OFFSET, device=d)
    ora = oracle.OracleEnv(oracle.make_cfg(n, nr.N_ROWS, C_, noise_mode=1 if noise == "mt19937" else 0, seed=nr.SEED,
                                           autoreset=1, env_offset=nr.ENV_OFFSET), tab.cost, tab.latency)
    spec = rr.Spec(C_)
    eo = ora.reset()
    np.testing.assert_array_equal(_u32(X.reset()), eo.view(np.uint32))
    resets = 0
    for t in range(rr.STEPS):
        ea = rr.decide(ora, rule, eo, spec)
        a = X.rule_actions(rule)
        np.testing.assert_array_equal(a.cpu().numpy(), ea, err_msg=f"actions at step {t}")
        obs, rew, term, _, _ = X.step(a)
        eo, er, et, _, _, status = ora.step(ea)
        assert not status.any()
        eo = eo.copy()
        np.testing.assert_array_equal(_u32(obs), eo.view(np.uint32), err_msg=f"obs after step {t}")
        np.testing.assert_array_equal(_u64(rew), er.view(np.uint64), err_msg=f"reward at step {t}")
        np.testing.assert_array_equal(term.cpu().numpy(), et, err_msg=f"terminated at step {t}")
        resets += int(et.sum())
    assert resets == n
    X.close()


def test_golden_round_robin_and_greedy_traces(traces):
    """the reference env's own action traces (tools/make_goldens.py) for random.seed(0 / 7 / 42), one lane each"""
    from rlks import VecK8sMultiCloudEnv

    d = _dev()
    seeds = [0, 7, 42]
    for rule, pol in (("round_robin", "rr"), ("cheapest", "greedy")):
        X = VecK8sMultiCloudEnv(len(seeds), noise="mt19937", autoreset=False, device=d)
        X.seed(seeds)
        np.testing.assert_array_equal(_u32(X.reset()), np.stack([traces[f"s{s}_{pol}_obs"][0] for s in seeds]).view(np.uint32))
        for t in range(99):
            a = X.rule_actions(rule)
            np.testing.assert_array_equal(a.cpu().numpy(), [traces[f"s{s}_{pol}_action"][t] for s in seeds],
                                          err_msg=f"{pol} action at step {t}")
            obs, rew, _, _, _ = X.step(a)
            np.testing.assert_array_equal(_u32(obs), np.stack([traces[f"s{s}_{pol}_obs"][t + 1] for s in seeds]).view(np.uint32))
            np.testing.assert_array_equal(_u64(rew), np.array([traces[f"s{s}_{pol}_reward"][t] for s in seeds]).view(np.uint64))
        X.close()


@pytest.mark.parametrize("name", ["J", "K"])
def test_random_is_the_categorical_draw_from_zero_logits(name):
    from rlks import _lib

    case = rr.CASES[name]
    d = _dev()
    X = _make_env(case, d)
    X.reset()
    zeros = torch.zeros(case.n, case.C, dtype=torch.float32, device=d)
    want = torch.empty(case.n, dtype=torch.int32, device=d)
    seen = set()
    for t in range(rr.STEPS):  # (past the auto-reset: episode 2 draws differ from episode 1's)
        st, ep = X.lane_state()
        ids = torch.stack([torch.arange(case.n, dtype=torch.int32, device=d) + nr.ENV_OFFSET, ep, st], 1).contiguous()
        _lib.call("rlks_sample_categorical", _lib.ptr(zeros), case.n, case.C, _lib.ptr(ids), nr.SEED, 1, _lib.ptr(want),
                  None, X.dev.stream)
        a = X.rule_actions("random")
        assert torch.equal(a, want), f"step {t}"
        seen.update(a.cpu().numpy().tolist())
        X.step(a)
    assert seen == set(range(case.C))
    X.close()


def test_explicit_obs_and_lanes_past_the_last_row():
    """`obs` need not be the env's own; a lane past the last table row is decided like any other"""
    case = rr.CASES["J"]
    spec = rr.spec_of(case)
    d = _dev()
    X = _make_env(case, d, autoreset=False)
    X.reset()
    for _ in range(nr.N_ROWS):  # 99 steps end the episode, the 100th runs past the last row
        X.step(X.rule_actions("least_loaded"))
    with pytest.raises(IndexError):
        X.check_status()
    st, ep = (x.cpu().numpy() for x in X.lane_state())
    assert (st == nr.N_ROWS).all()
    used = X.node_state()[2].cpu().numpy()
    rng = np.random.default_rng(3)
    obs = rng.random((case.n, 3 * case.C)).astype(np.float32)
    obs[:5, :case.C] = 0.25            # ties: the lowest index
    obs[5:9, 2 * case.C:] = 0.5
    obs[9:12] = 0.0
    for rule in RULE_NAMES:
        got = X.rule_actions(rule, torch.from_numpy(obs.astype(np.float64)).to(d))  # (made float32, contiguous)
        np.testing.assert_array_equal(got.cpu().numpy(), rr.rule_actions(rule, obs, st, ep, used, spec), err_msg=rule)
    for bad in (torch.zeros(case.n, 3 * case.C + 1), torch.zeros(case.n - 1, 3 * case.C)):
        with pytest.raises(ValueError):
            X.rule_actions("myopic", bad.to(d))
    with pytest.raises(ValueError, match="unknown rule"):
        X.rule_actions("best_fit")
    X.close()


def test_null_pointers_and_unknown_rules_are_argument_errors():
    from rlks import _lib

    case = rr.CASES["L"]
    d = _dev()
    X = _make_env(case, d)
    X.reset()
    act = torch.full((case.n,), -7, dtype=torch.int32, device=d)
    fn = _lib.lib().rlks_env_rule_actions
    s = X.dev.stream
    assert fn(None, 0, _lib.ptr(X.obs), _lib.ptr(act), s) == -1       # RLKS_ERR_ARG
    assert fn(X.handle, 0, None, _lib.ptr(act), s) == -1
    assert fn(X.handle, 0, _lib.ptr(X.obs), None, s) == -1
    for rule in (-1, 6, 1 << 20):
        assert fn(X.handle, rule, _lib.ptr(X.obs), _lib.ptr(act), s) == -1
        assert b"unknown rule" in _lib.lib().rlks_last_error()
        with pytest.raises(_lib.RlksError, match="unknown rule"):
            X.rule_actions(rule)
    torch.cuda.synchronize()
    assert (act == -7).all()  # nothing was launched
    X.close()


def test_rule_and_step_replay_from_a_captured_graph():
    """asynchronous on the stream and capturable: rule + trusted step, captured once and replayed, walk
    the env exactly as the eager calls walk its twin"""
    from rlks import _lib

    case = rr.CASES["G"]
    d = _dev()
    X, Y = _make_env(case, d), _make_env(case, d)
    X.reset()
    Y.reset()
    act = torch.zeros(case.n, dtype=torch.int32, device=d)
    rule = rr.RULES["myopic_with_room"]

    def launch(E, stream):
        _lib.call("rlks_env_rule_actions", E.handle, rule, _lib.ptr(E.obs), _lib.ptr(act), stream)
        _lib.call("rlks_env_step", E.handle, _lib.ptr(act), _lib.ptr(E.obs), _lib.ptr(E.reward), None,
                  _lib.ptr(E.terminated), None, None, None, None, stream)

    side = torch.cuda.Stream(device=d)
    side.wait_stream(torch.cuda.current_stream(d))
    g = torch.cuda.CUDAGraph()
    with torch.cuda.stream(side):
        with torch.cuda.graph(g, stream=side):
            launch(X, side.cuda_stream)
    torch.cuda.current_stream(d).wait_stream(side)
    for t in range(12):
        g.replay()
        torch.cuda.synchronize()
        xa = act.clone()
        launch(Y, Y.dev.stream)
        torch.cuda.synchronize()
        assert torch.equal(xa, act), f"actions at replay {t}"
        assert torch.equal(X.obs, Y.obs) and torch.equal(X.reward, Y.reward), f"replay {t}"
    for a, b in zip(X.node_state(), Y.node_state()):
        assert torch.equal(a, b)
    X.close()
    Y.close()
