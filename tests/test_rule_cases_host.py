"""CPU checks of the baseline-scheduler cases (tests/rule_ref.py), by the C oracle and
the numpy restatement alone: every case is in the regimes it is there for, the room test on a
cluster's used millicores is the per-node one, and on the reference table the rules reproduce the
reference's goldens.  Also the host side of PPOConfig.evaluation(evaluation_baselines=...)."""
import json

import numpy as np
import pytest

import oracle
import rule_ref as rr

SEEDS = [0, 7, 42]


@pytest.mark.parametrize("name", sorted(rr.CASES))
def test_case_is_in_its_regimes(name):
    wr, ll, my = rr.check_guards(name)
    m = rr.MEASURED[name]
    # the recorded figures (a changed default shows here first; the floors are what the GPU tests rely on)
    assert (wr.differ, wr.no_room, wr.some_full, ll.ll_ties) == (m["differ"], m["no_room"], m["some_full"], m["ll_ties"])
    assert int(my.counters[2]) == m["myopic_rejected"]
    assert len(np.unique(np.concatenate(my.actions))) == m["myopic_actions"]
    if name != "K":  # every rule uses every action
        for rule in rr.RULES:
            used = np.unique(np.concatenate(rr.oracle_run(name, rule).actions))
            assert np.array_equal(used, np.arange(rr.CASES[name].C)), (name, rule, used)


@pytest.mark.parametrize("name", sorted(rr.CASES))
def test_used_cpu_room_test_is_the_per_node_one(name):
    """a cluster's nodes are equally sized: pods < nodes * pods-per-node <=> some node has free cpu
    and memory for one pod, on every state of every rule's run"""
    for rule in rr.RULES:
        assert rr.oracle_run(name, rule).room_mismatch == 0, (name, rule)


def _golden_episode(cost, lat, seed, rule):
    """one episode of the reference table (MT19937 noise, random.seed(seed)) under `rule`"""
    env = oracle.OracleEnv(oracle.make_cfg(1, 100, 2, noise_mode=1), cost, lat)
    env.seed(0, seed)
    spec = rr.Spec(2, seed=0, env_offset=0)
    obs = env.reset()
    acts, rews, obss = [], [], []
    for _ in range(99):
        st, ep = env.lane_counters()
        a = rr.rule_actions(rule, obs, st, ep, None, spec)
        obss.append(obs.copy())
        obs, r, term, _, _, status = env.step(a)
        assert not status.any()
        acts.append(int(a[0]))
        rews.append(float(r[0]))
    assert term[0]
    ret = 0.0
    for r in rews:  # ep_reward += reward, in step order
        ret += r
    return np.array(acts, np.int32), np.array(rews), ret, np.concatenate(obss)


@pytest.mark.parametrize("seed", SEEDS)
def test_cheapest_is_the_reference_greedy(golden_cost_lat, traces, traces_meta, seed):
    cost, lat = golden_cost_lat
    acts, rews, ret, _ = _golden_episode(cost, lat, seed, "cheapest")
    np.testing.assert_array_equal(acts, traces[f"s{seed}_greedy_action"])
    np.testing.assert_array_equal(rews.view(np.uint64), traces[f"s{seed}_greedy_reward"].view(np.uint64))
    assert ret == traces_meta["returns"]["greedy"] == 3725.338357358271
    rr_acts, _, rr_ret, _ = _golden_episode(cost, lat, seed, "round_robin")
    np.testing.assert_array_equal(rr_acts, traces[f"s{seed}_rr_action"])
    assert rr_ret == traces_meta["returns"]["rr"]


def test_myopic_is_the_per_step_maximum(golden_cost_lat, traces_meta):
    """the table env's reward depends on nothing the agent changes, so the myopic rule is its optimal
    policy: it takes the larger f64 reward at every step (the f32 observation flips no order and no
    step is tied), and its return is the golden upper bound"""
    cost, lat = golden_cost_lat
    acts, rews, ret, _ = _golden_episode(cost, lat, 42, "myopic")
    r = 100.0 * (0.6 * cost[:99] + 0.4 * lat[:99])  # the reward of either cloud at each step (:122)
    assert int((r[:, 0] == r[:, 1]).sum()) == 0                       # no ties
    assert int((acts != r.argmax(1)).sum()) == 0                      # no order flips
    np.testing.assert_array_equal(rews.view(np.uint64), r.max(1).view(np.uint64))
    acts_room, _, ret_room, _ = _golden_episode(cost, lat, 42, "myopic_with_room")
    assert np.array_equal(acts_room, acts) and ret_room == ret        # a table env always has room
    bound = traces_meta["per_step_max_return"]
    assert bound == 6245.5367107939965 and ret == 6245.536710793996   # (pairwise np.sum; the step-order sum)
    assert abs(ret - bound) <= 99 * 2.0 ** -53 * bound


def test_comparison_report_lines():
    from rlks.evaluation import EvalResult, NodeEvalResult, comparison_report

    acts = np.array([[0, 1], [1, 1]], np.int32)
    node = NodeEvalResult(np.array([110.0, 130.0]), acts, np.array([1, 3]), placed=30, rejected=10, departed=5,
                          mean_util=np.array([0.5, 0.25]))
    tab = EvalResult(np.array([100.0, 100.0]), acts)
    assert node.rejection_rate == 0.25
    assert NodeEvalResult(node.rewards, acts, node.choices, 0, 0, 0, node.mean_util).rejection_rate == 0.0
    lines = comparison_report({"table": tab, "policy": node}).splitlines()
    assert len(lines) == 2
    assert "return =     100.00" in lines[0] and "+0.00%" in lines[0] and "n/a" in lines[0] and "25.0% 75.0%" in lines[0]
    assert "return =     120.00" in lines[1] and "vs table =  +20.00%" in lines[1] and "25.00%" in lines[1]
    assert "-16.67%" in comparison_report({"table": tab, "policy": node}, baseline="policy").splitlines()[0]
    with pytest.raises(ValueError):
        comparison_report({"a": tab}, baseline="b")
    with pytest.raises(ValueError):
        comparison_report({})


def test_evaluation_baselines_config():
    from rlks.ppo import PPOConfig

    c = PPOConfig()
    assert c.evaluation_baselines is None and c.to_dict()["evaluation_baselines"] is None
    c = PPOConfig().evaluation(evaluation_interval=1, evaluation_duration=8,
                               evaluation_baselines=("myopic", "least_loaded"))
    assert c.evaluation_baselines == ["myopic", "least_loaded"]
    assert PPOConfig().evaluation(evaluation_baselines="random").evaluation_baselines == ["random"]
    for bad in (["myopic", "best_fit"], "greedy", [3]):
        with pytest.raises(ValueError, match="baseline"):
            PPOConfig().evaluation(evaluation_baselines=bad)
    # the round trip a checkpoint makes (algorithm_state.json)
    d = json.loads(json.dumps(c.to_dict()))
    assert d["evaluation_baselines"] == ["myopic", "least_loaded"]
    c2 = PPOConfig.from_dict(d)
    assert c2.evaluation_baselines == ["myopic", "least_loaded"] and c2.evaluation_interval == 1
    assert PPOConfig.from_dict(json.loads(json.dumps(PPOConfig().to_dict()))).evaluation_baselines is None
    d["evaluation_baselines"] = ["nope"]
    with pytest.raises(ValueError, match="baseline"):
        PPOConfig.from_dict(d)
    # .evaluation() without the argument leaves it
    assert c.evaluation(evaluation_duration=4).evaluation_baselines == ["myopic", "least_loaded"]
