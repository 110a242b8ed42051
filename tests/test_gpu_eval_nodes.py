"""The evaluation harness for node-level envs and the device baselines (rlks/evaluation.py, DESIGN.md
§19): evaluate_nodes against the C oracle's loop, the paired-arrivals property, the table env's golden
upper bound through evaluate("myopic"), and PPOConfig.evaluation(evaluation_baselines=...) in train()."""
import numpy as np
import pytest

import node_regimes as nr
import oracle
import rule_ref as rr

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

EVAL_SEED = 11


def _dev():
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    return torch.device("cuda", 0)


def _oracle_eval(case, rule, E, seed):
    """evaluate_nodes' loop in the C oracle: lane e = episode e, autoreset off, max_steps steps, float64
    returns summed in step order"""
    case = rr.dataclasses.replace(case, n=E)
    spec = rr.Spec(case.C, case.nodes, cpu=tuple(case.cpu), mem=tuple(case.mem), seed=seed, env_offset=0)
    ora = rr.make_oracle(case, autoreset=0, seed=seed, env_offset=0)
    obs = ora.reset()
    T = nr.N_ROWS - 1
    ret = np.zeros(E, np.float64)
    util = np.zeros((E, case.C), np.float64)
    acts = np.zeros((T, E), np.int32)
    for t in range(T):
        acts[t] = rr.decide(ora, rule, obs, spec)
        obs, r, term, _, _, status = ora.step(acts[t])
        assert not status.any()
        ret += r
        util += obs[:, 2 * case.C:]
    assert term.all()
    return ret, acts, ora.counters(), util.sum(0) / (T * E)


@pytest.fixture(scope="module")
def g_results():
    """case G (64 episodes) under two rules, evaluated once for the tests below"""
    from rlks.evaluation import evaluate_nodes

    d = _dev()
    case = rr.CASES["G"]
    kw = dict(nodes=rr.node_spec(case), table=nr.table(case), seed=EVAL_SEED, device=d)
    return {rule: evaluate_nodes(rule, 64, **kw) for rule in ("myopic_with_room", "least_loaded")}


def test_evaluate_nodes_equals_the_oracle_loop(g_results):
    case = rr.CASES["G"]
    res = g_results["myopic_with_room"]
    ret, acts, counters, util = _oracle_eval(case, "myopic_with_room", 64, EVAL_SEED)
    T = nr.N_ROWS - 1
    assert res.rewards.dtype == np.float64 and res.actions.dtype == np.int32 and res.actions.shape == (T, 64)
    np.testing.assert_array_equal(res.actions, acts)
    np.testing.assert_array_equal(res.rewards.view(np.uint64), ret.view(np.uint64))
    assert (res.placed, res.rejected, res.departed) == tuple(int(x) for x in counters[1:4])
    assert res.rejected > 0 and res.rejection_rate == res.rejected / (res.placed + res.rejected)
    assert res.choices.shape == (case.C,) and int(res.choices.sum()) == T * 64
    np.testing.assert_array_equal(res.choices, np.bincount(acts.reshape(-1), minlength=case.C))
    # (per lane the same float64 sums in step order; over the 64 lanes of positive terms the device's sum
    # and numpy's each have their own order: at most 63 roundings of 2^-53 on either side)
    np.testing.assert_allclose(res.mean_util, util, rtol=128 * 2.0 ** -53, atol=0)
    assert np.all((res.mean_util > 0) & (res.mean_util <= 1))


def test_two_rules_meet_the_same_arrivals(g_results):
    a, b = g_results["myopic_with_room"], g_results["least_loaded"]
    assert not np.array_equal(a.actions, b.actions)
    assert a.placed + a.rejected == b.placed + b.rejected > 0
    assert a.rejected != b.rejected


def test_comparison_report_of_device_results(g_results):
    from rlks.evaluation import comparison_report

    txt = comparison_report(g_results, baseline="least_loaded")
    lines = txt.splitlines()
    assert len(lines) == 2 and lines[0].startswith("myopic_with_room") and "vs least_loaded =" in lines[0]
    assert "+0.00%" in lines[1] and f"{g_results['least_loaded'].rejection_rate:.2%}" in lines[1]


def test_evaluate_myopic_reaches_the_golden_upper_bound(traces_meta, traces):
    from rlks.evaluation import comparison_report, evaluate

    d = _dev()
    bound = traces_meta["per_step_max_return"]
    res = evaluate("myopic", 5, seed=42, device=d)
    assert np.all(res.rewards == 6245.536710793996)              # the step-order float64 sum
    assert np.all(np.abs(res.rewards - bound) <= 99 * 2.0 ** -53 * bound)
    room = evaluate("myopic_with_room", 5, seed=42, device=d)     # a table env always has room
    assert np.array_equal(room.actions, res.actions) and np.array_equal(room.rewards, res.rewards)
    cheap, greedy = evaluate("cheapest", 3, seed=7, device=d), evaluate("greedy", 3, seed=7, device=d)
    assert np.array_equal(cheap.actions, greedy.actions) and np.all(cheap.rewards == traces_meta["returns"]["greedy"])
    assert np.array_equal(cheap.actions[:, 0], traces["s7_greedy_action"])
    ll, rnd = evaluate("least_loaded", 3, seed=7, device=d), evaluate("random", 3, seed=7, device=d)
    for r in (ll, rnd):  # no rule beats the myopic one here
        assert np.all(r.rewards < res.rewards[0]) and 0 < r.actions.sum() < r.actions.size
    assert np.array_equal(rnd.actions, evaluate("random", 3, seed=7, device=d).actions)
    assert not np.array_equal(rnd.actions, evaluate("random", 3, seed=8, device=d).actions)
    with pytest.raises(ValueError, match="unknown baseline"):
        evaluate("best_fit", 2, seed=1, device=d)
    txt = comparison_report({"greedy": greedy, "myopic": res})
    assert "n/a" in txt and txt.splitlines()[1].startswith("myopic")


def _algo(d, baselines):
    from rlks.env import NodeSpec
    from rlks.ppo import PPO, PPOConfig
    from rlks.tables import synthetic_table

    C_, N, T = 4, 128, 8
    tab = synthetic_table(C_, 100, seed=7)
    spec = NodeSpec(C_, 8, node_cpu_m=[300] * C_, node_mem_mi=[4096] * C_, arrival_rate=3.0, depart_prob=0.02,
                    init_occupancy=0.5, reject_penalty=0.25)
    cfg = (PPOConfig().framework("torch")
           .training(train_batch_size=N * T, sgd_minibatch_size=256, num_sgd_iter=1, lr=3e-4)
           .evaluation(evaluation_interval=1, evaluation_duration=16, evaluation_baselines=baselines)
           .debugging(seed=5))
    cfg.num_envs, cfg.table, cfg.nodes = N, tab, spec
    cfg.checkpoint_env_state = True  # (24 KB of node state here; off by default for node-level envs)
    return PPO(config=cfg, device=d), tab, spec


def test_train_reports_the_baselines_beside_the_policy(tmp_path):
    from rlks.evaluation import evaluate_nodes
    from rlks.ppo import PPO

    d = _dev()
    parent_keys = {"episode_reward_mean", "episode_reward_min", "episode_reward_max", "episodes_this_iter",
                   "episode_len_mean"}
    plain, _, _ = _algo(d, None)
    ev0 = plain.train()["evaluation"]
    assert set(ev0) == parent_keys

    algo, tab, spec = _algo(d, ["myopic", "least_loaded"])
    ev = algo.train()["evaluation"]
    assert set(ev) == parent_keys | {"baselines"} and list(ev["baselines"]) == ["myopic", "least_loaded"]
    seed = (algo.seed * 7919 + algo.iteration) & 0xFFFFFFFF
    for name in ("myopic", "least_loaded"):
        r = evaluate_nodes(name, 16, nodes=spec, table=tab, seed=seed, device=d)
        assert ev["baselines"][name] == {"episode_reward_mean": float(np.mean(r.rewards)),
                                         "rejection_rate": r.rejection_rate}
    assert ev["baselines"]["myopic"]["rejection_rate"] > 0
    own = evaluate_nodes(algo, 16, nodes=spec, table=tab, seed=seed, device=d)  # as evaluate_lanes runs the policy
    assert float(np.mean(own.rewards)) == ev["episode_reward_mean"]
    # the field travels with a checkpoint
    back = PPO.from_checkpoint(algo.save(str(tmp_path)), device=d)
    assert back.config.evaluation_baselines == ["myopic", "least_loaded"]
    for a in (plain, algo, back):
        a.stop()
