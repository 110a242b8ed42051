"""The shared decide path (rlks.sampling, rlks.evaluation.decider / run_episodes): evaluate_lanes on a node-level
env is evaluate_nodes' returns, and PPO.compute_actions and the server's fallback are one draw."""
import dataclasses

import numpy as np
import pytest

import action_mask_ref as am
import node_regimes as nr
import oracle
import rule_ref as rr

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

# rule_ref's fill-up case J (C = 3: not a power of two, 8 nodes: the fewest the library takes) with nodes of one
# pod, so that 8 pods fill a cluster and it happens within the 5 steps of a 6-row table (3 arrivals a step)
CASE = dataclasses.replace(rr.CASES["J"], cpu=(100,) * 3)
ROWS, EPISODES, SEED = 6, 5, 11


def _dev():
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    return torch.device("cuda", 0)


def _table():
    from rlks.tables import synthetic_table

    return synthetic_table(CASE.C, ROWS, seed=nr.TABLE_SEED)


def _algo(d, hidden, mask):
    from rlks.ppo import PPO, PPOConfig

    cfg = (PPOConfig().framework("torch")
           .training(train_batch_size=64 * 4, sgd_minibatch_size=256, num_sgd_iter=1, lr=3e-4, action_mask=mask,
                     model={"fcnet_hiddens": [hidden, hidden]})
           .debugging(seed=5))
    cfg.num_envs, cfg.table, cfg.nodes = 64, _table(), rr.node_spec(CASE)
    return PPO(config=cfg, device=d)


def _masked_lane_steps(actions, seed):
    """replay evaluate_nodes' actions in the C oracle: they obey the room mask; -> lane-steps with a masked cluster"""
    tab = _table()
    E = actions.shape[1]
    ora = oracle.OracleEnv(oracle.make_cfg(E, ROWS, CASE.C, noise_mode=0, seed=seed, autoreset=0, nodes=CASE.nodes,
                                           pod_cpu_m=nr.POD_CPU_M, pod_mem_mi=nr.POD_MEM_MI, arrival_mode=0,
                                           arrival_rate=CASE.rate, depart_prob=CASE.depart, init_occupancy=CASE.occ,
                                           reject_penalty=CASE.penalty),
                           tab.cost, tab.latency, np.array(CASE.cpu, np.int32), np.array(CASE.mem, np.int32), None)
    ora.reset()
    masked = 0
    for a in actions:
        m = am.room_mask(ora.node_state()[2], rr.spec_of(CASE))
        assert m[np.arange(E), a].all()
        masked += int((~m.all(1)).sum())
        ora.step(a)
    return masked


def test_evaluate_lanes_is_evaluate_nodes_rewards():
    from rlks import _lib
    from rlks.evaluation import evaluate_lanes, evaluate_nodes
    from rlks.policy import PolicyParams

    d = _dev()
    kw = dict(nodes=rr.node_spec(CASE), table=_table(), seed=SEED, device=d)
    params = PolicyParams(3 * CASE.C, 256, CASE.C, device=d, seed=3)
    params.desc.precision = _lib.RLKS_PRECISION_WIDE  # 3 actions: the generic-width forward
    algo = _algo(d, 256, "room")
    for policy in (params, algo):
        res = evaluate_nodes(policy, EPISODES, **kw)
        assert res.actions.shape == (ROWS - 1, EPISODES) and res.rewards.dtype == np.float64
        lanes = evaluate_lanes(policy, EPISODES, **kw)
        np.testing.assert_array_equal(lanes.view(np.uint64), res.rewards.view(np.uint64))
    # the algorithm's run was the masked one, and the mask had something to do
    assert _masked_lane_steps(res.actions, SEED) > 0
    for flag in (True, False):
        np.testing.assert_array_equal(evaluate_lanes(algo, EPISODES, action_mask=flag, **kw),
                                      evaluate_nodes(algo, EPISODES, action_mask=flag, **kw).rewards)
    np.testing.assert_array_equal(evaluate_lanes(algo, EPISODES, action_mask=True, **kw), lanes)
    algo.stop()


@pytest.mark.parametrize("mask", [None, "room"])
def test_compute_actions_and_the_server_fallback_share_the_draw(mask):
    d = _dev()
    algo = _algo(d, 128, mask)
    srv = algo.server(max_rows=65)
    assert not srv.fused and srv.masked == (mask is not None) and srv.seed == algo.seed
    rng = np.random.default_rng(9)
    obs = rng.random((65, algo.D)).astype(np.float32)
    m = None
    if mask is not None:
        m = rng.random((65, algo.A)) < 0.5
        m[0] = False                      # a row without an allowed action counts as all allowed
        m[1] = [False, False, True]
    drawn = []
    for call in (0, 1, 7):
        for n in (1, 65):
            algo.sample_calls = srv.calls = call
            mk = None if m is None else m[:n]
            a = algo.compute_actions(obs[:n], explore=True, action_mask=mk).cpu().numpy()
            s = srv.act(obs[:n], explore=True, action_mask=mk)
            assert algo.sample_calls == srv.calls == call + 1
            assert s.dtype == np.int32 and s.shape == (n,)
            np.testing.assert_array_equal(a, s)
            if mk is not None:
                ok = np.where(mk.any(1, keepdims=True), mk, True)
                assert ok[np.arange(n), a].all()
        drawn.append(a)
    assert not np.array_equal(drawn[0], drawn[1])  # the counter is part of the draw
    algo.sample_calls = srv.calls = 3
    g = algo.compute_actions(obs, explore=False, action_mask=m).cpu().numpy()
    np.testing.assert_array_equal(g, srv.act(obs, explore=False, action_mask=m))
    assert algo.sample_calls == srv.calls == 3  # argmax draws nothing
    assert algo.compute_single_action(obs[0], explore=False, action_mask=None if m is None else m[0]) == g[0]
    srv.close()
    algo.stop()
