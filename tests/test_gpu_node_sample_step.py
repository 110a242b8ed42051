"""rlks_env_sample_step on node-level envs: the Categorical draw folded into the node
step kernels.  Cases, logits and the oracle's runs are in tests/node_sample_cases.py.

The fused call must equal, bit for bit, the two calls it replaces (rlks_sample_categorical with the
lanes' own counters, then rlks_env_step with trusted actions) in actions, logp, observations,
rewards and terminations after every step and in the whole env state every 10th step; its
transitions must replay in the C oracle; and where C <= 8 its draws must be oracle.sample_actions'."""
import numpy as np
import pytest

import node_regimes as nr
import node_sample_cases as ns

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")


def _dev():
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    return torch.device("cuda", 0)


def _bits(x):
    x = x.cpu().numpy() if hasattr(x, "cpu") else np.asarray(x)
    return x.view(np.uint32) if x.dtype == np.float32 else x


def _make_env(case, d):
    from rlks import VecK8sMultiCloudEnv

    return VecK8sMultiCloudEnv(case.n, table=nr.table(case), seed=nr.SEED, nodes=ns.node_spec(case),
                               env_offset=nr.ENV_OFFSET, device=d)


class _Out:
    """the five outputs of one sample + step, owned by the test"""

    def __init__(self, n, D, d):
        self.actions = torch.full((n,), -7, dtype=torch.int32, device=d)
        self.logp = torch.full((n,), 7.0, dtype=torch.float32, device=d)
        self.obs = torch.zeros(n, D, dtype=torch.float32, device=d)
        self.reward = torch.full((n,), 7.0, dtype=torch.float32, device=d)
        self.done = torch.full((n,), 7, dtype=torch.uint8, device=d)

    def fields(self):
        return (("actions", self.actions), ("logp", self.logp), ("obs", self.obs), ("reward", self.reward),
                ("done", self.done))


def _fused(venv, lg, explore, out):
    from rlks import _lib

    _lib.call("rlks_env_sample_step", venv.handle, _lib.ptr(lg), int(explore), _lib.ptr(out.actions), _lib.ptr(out.logp),
              _lib.ptr(out.obs), _lib.ptr(out.reward), _lib.ptr(out.done), venv.dev.stream)


def _two_calls(venv, lg, explore, out, seed, env_offset):
    """rlks_sample_categorical keyed by the lanes' own (global lane, episode, step), then the trusted step"""
    from rlks import _lib

    st, ep = venv.lane_state()
    n = venv.num_envs
    ids = torch.stack([torch.arange(n, dtype=torch.int32, device=lg.device) + env_offset, ep, st], 1).contiguous()
    _lib.call("rlks_sample_categorical", _lib.ptr(lg), n, lg.shape[1], _lib.ptr(ids), seed, int(explore),
              _lib.ptr(out.actions), _lib.ptr(out.logp), venv.dev.stream)
    _lib.call("rlks_env_step", venv.handle, _lib.ptr(out.actions), _lib.ptr(out.obs), None, _lib.ptr(out.reward),
              _lib.ptr(out.done), None, None, None, None, venv.dev.stream)


def _same_outputs(x, y, what):
    for (name, a), (_, b) in zip(x.fields(), y.fields()):
        np.testing.assert_array_equal(_bits(a), _bits(b), err_msg=f"{name} {what}")


def _same_state(X, Y, what):
    for a, b, name in zip(X.node_state(), Y.node_state(), ("free cpu", "free mem", "used cpu")):
        assert torch.equal(a, b), f"{name} {what}"
    for a, b, name in zip(X.lane_state(), Y.lane_state(), ("step", "episode")):
        assert torch.equal(a, b), f"{name} {what}"
    assert torch.equal(X.counters(), Y.counters()), f"counters {what}"
    np.testing.assert_array_equal(X.episode_stats(clear=False).cpu().numpy().view(np.uint64),
                                  Y.episode_stats(clear=False).cpu().numpy().view(np.uint64),
                                  err_msg=f"episode stats {what}")


def _oracle_follows(ora, out, t):
    """the C oracle, fed the device's actions, gives the device's transition"""
    o, r, term, _, _, status = ora.step(out.actions.cpu().numpy())
    assert not status.any(), status
    np.testing.assert_array_equal(_bits(out.obs), o.view(np.uint32), err_msg=f"obs vs oracle at step {t}")
    np.testing.assert_array_equal(_bits(out.reward), r.astype(np.float32).view(np.uint32),
                                  err_msg=f"reward vs oracle at step {t}")
    np.testing.assert_array_equal(out.done.cpu().numpy(), term, err_msg=f"terminated vs oracle at step {t}")


def _oracle_end(ora, X):
    for g, e, name in zip(X.node_state(), ora.node_state(), ("free cpu", "free mem", "used cpu")):
        np.testing.assert_array_equal(g.cpu().numpy(), e, err_msg=f"{name} vs oracle at the end")
    np.testing.assert_array_equal(X.counters().cpu().numpy(), ora.counters())


@pytest.mark.parametrize("name", sorted(ns.CASES))
def test_fused_equals_sample_then_step(name):
    case = ns.CASES[name]
    exp = ns.check_guards(name)  # the oracle's own run, before the device is touched
    d = _dev()
    X, Y = _make_env(case, d), _make_env(case, d)
    ora = ns.make_oracle(case)
    X.counters(enable=1)
    Y.counters(enable=1)
    ox = X.reset().cpu().numpy()
    np.testing.assert_array_equal(ox.view(np.uint32), Y.reset().cpu().numpy().view(np.uint32))
    np.testing.assert_array_equal(ox.view(np.uint32), ora.reset().view(np.uint32))
    x, y = _Out(case.n, 3 * case.C, d), _Out(case.n, 3 * case.C, d)
    x.obs.copy_(X.obs)
    y.obs.copy_(Y.obs)
    excluded = 0
    for t in range(case.steps):
        lg_h = ns.logits(case, t)
        lg = torch.from_numpy(lg_h).to(d)
        if case.C <= 8:  # the draw restated on the host, before the lanes move on
            ea, margin = ns.sample(ora, case, lg_h)
        _fused(X, lg, 1, x)
        _two_calls(Y, lg, 1, y, nr.SEED, nr.ENV_OFFSET)
        _same_outputs(x, y, f"at step {t}")  # every lane, every draw
        if case.C <= 8:
            sure = margin >= ns.MARGIN_ULP
            excluded += int((~sure).sum())
            np.testing.assert_array_equal(x.actions.cpu().numpy()[sure], ea[sure], err_msg=f"draws vs host at step {t}")
            np.testing.assert_array_equal(ea, exp.actions[t])
        _oracle_follows(ora, x, t)
        if (t + 1) % nr.STATE_EVERY == 0 or t == case.steps - 1:
            _same_state(X, Y, f"after step {t}")
    assert excluded == 0  # (node_sample_cases.check_guards: no draw within 4 ulp of a boundary)
    _oracle_end(ora, X)


@pytest.mark.parametrize("name", ["A", "E", "P64"])
def test_fused_argmax(name):
    case = ns.CASES[name]
    d = _dev()
    X, Y = _make_env(case, d), _make_env(case, d)
    ora = ns.make_oracle(case)
    X.counters(enable=1)
    X.reset()
    Y.reset()
    ora.reset()
    x, y = _Out(case.n, 3 * case.C, d), _Out(case.n, 3 * case.C, d)
    for t in range(30):
        lg_h = ns.logits(case, t)
        lg = torch.from_numpy(lg_h).to(d)
        _fused(X, lg, 0, x)
        _two_calls(Y, lg, 0, y, nr.SEED, nr.ENV_OFFSET)
        a = x.actions.cpu().numpy()
        np.testing.assert_array_equal(a, lg_h.argmax(1).astype(np.int32), err_msg=f"argmax at step {t}")  # (first maximum)
        assert a[0] == 0 and a[1] == 1 % case.C
        _same_outputs(x, y, f"at step {t}")
        _oracle_follows(ora, x, t)
    _oracle_end(ora, X)


def test_python_sample_step():
    from rlks import VecK8sMultiCloudEnv, _lib
    from rlks.tables import synthetic_table

    d = _dev()
    # a 2-cloud table env (k_sample_step), 300 lanes: a ragged last workgroup
    tab = synthetic_table(2, 100, seed=7)
    P = VecK8sMultiCloudEnv(300, table=tab, seed=9, env_offset=5, device=d)
    Y = VecK8sMultiCloudEnv(300, table=tab, seed=9, env_offset=5, device=d)
    P.reset()
    Y.reset()
    y = _Out(300, 6, d)
    rng = np.random.default_rng(2)
    for t in range(110):
        lg = torch.from_numpy(rng.normal(0, 1.5, (300, 2)).astype(np.float32)).to(d)
        a, lp, obs, rew, done = P.sample_step(lg if t % 2 else lg.double())  # (made float32)
        assert (a.dtype, lp.dtype, obs.dtype, rew.dtype, done.dtype) == (torch.int32, torch.float32, torch.float32,
                                                                        torch.float32, torch.uint8)
        _two_calls(Y, lg, 1, y, 9, 5)
        for g, e, what in zip((a, lp, obs, rew, done), (y.actions, y.logp, y.obs, y.reward, y.done),
                              ("actions", "logp", "obs", "reward", "done")):
            np.testing.assert_array_equal(_bits(g), _bits(e), err_msg=f"table env {what} at step {t}")
    for s, e in zip(P.lane_state(), Y.lane_state()):
        assert torch.equal(s, e)
    # a node-level env: case D
    case = ns.CASES["D"]
    P, Y = _make_env(case, d), _make_env(case, d)
    P.reset()
    Y.reset()
    y = _Out(case.n, 3 * case.C, d)
    for t in range(case.steps):
        lg = torch.from_numpy(ns.logits(case, t)).to(d)
        a, lp, obs, rew, done = P.sample_step(lg, explore=True)
        assert obs is P.obs
        _two_calls(Y, lg, 1, y, nr.SEED, nr.ENV_OFFSET)
        for g, e, what in zip((a, lp, obs, rew, done), (y.actions, y.logp, y.obs, y.reward, y.done),
                              ("actions", "logp", "obs", "reward", "done")):
            np.testing.assert_array_equal(_bits(g), _bits(e), err_msg=f"case D {what} at step {t}")
    a, *_ = P.sample_step(torch.from_numpy(ns.logits(case, 0)).to(d), explore=False)
    np.testing.assert_array_equal(a.cpu().numpy(), ns.logits(case, 0).argmax(1))
    for bad in (torch.zeros(case.n, case.C + 1), torch.zeros(case.n - 1, case.C), torch.zeros(case.n * case.C)):
        with pytest.raises(ValueError):
            P.sample_step(bad.to(d))
    Q = VecK8sMultiCloudEnv(case.n, table=nr.table(case), seed=nr.SEED, nodes=ns.node_spec(case), autoreset=False,
                            device=d)
    Q.reset()
    with pytest.raises(_lib.RlksError, match="autoreset"):
        Q.sample_step(torch.zeros(case.n, case.C, device=d))


SF_ROLL_FUSED_MAX_LANES = 16384  # (workspace.h) above it a split-fp16 table rollout runs k_sf_fwd16 + k_sample_step per step


def _row(C, nodes, H, N, T, mb, rows=100, prec="auto", per_step=False, explore=True, id=None):
    return pytest.param(C, nodes, H, N, T, mb, rows, prec, per_step, explore, id=id)


@pytest.mark.parametrize("C,nodes,H,N,T,mb,rows,prec,per_step,explore", [
    _row(8, 16, 256, 520, 16, 8192, id="8-16-256-520-16-8192"),   # split-fp16, node_rollout
    _row(16, 32, 384, 136, 8, 1024, id="16-32-384-136-8-1024"),   # hidden 384: wide_rollout
    # table envs (nodes=None): every kernel that draws inside a rollout.  96 lanes are three full 32-row
    # tiles (test_gpu_table_rollout.py runs the ragged one); a 4-row table ends every episode after 3 steps,
    # so the counter's episode word moves
    _row(2, None, 256, 96, 6, 256, rows=4, id="table-persistent-2"),             # k_sf_roll
    _row(8, None, 256, 96, 6, 256, rows=4, id="table-persistent-8"),
    _row(2, None, 256, 96, 6, 256, rows=4, explore=False, id="table-persistent-2-argmax"),
    _row(4, None, 256, 96, 6, 256, rows=4, per_step=True, id="table-per-step-4"),  # k_sf_fwd16 + k_sample_step
    _row(4, None, 256, 96, 6, 256, rows=4, prec="fp32", id="table-fp32-4"),       # k_fwd_head<..., FWD_ROLLOUT>
    _row(4, None, 256, 96, 6, 256, rows=4, prec="fp32", explore=False, id="table-fp32-4-argmax"),
    _row(4, None, 384, 136, 6, 256, rows=4, id="table-wide-4"),                   # k_wide_sample
])
def test_rollout_replays_from_its_logits(C, nodes, H, N, T, mb, rows, prec, per_step, explore):
    """PPO.rollout's buffers are what a twin env gives when fed the rollout's own logits through
    rlks_sample_categorical + rlks_env_step, bit for bit.  Every rollout kernel draws with the one
    categorical() / categorical_row() of env_device.h, so this holds by the kernels' own arithmetic, on
    node-level and table envs alike.  Before the node-level rollouts moved to the fused step it failed
    for logp by 1 ulp in 59 of 136 lanes of a step, and before the draw was shared the table rows
    failed the same way on the persistent, fp32 and wide paths (profiles/r15_shared_rows): their
    samplers were built with FMA contraction, which rounds logf's last addition differently
    (DESIGN.md §18, §24)."""
    from rlks import VecK8sMultiCloudEnv
    from rlks.env import NodeSpec
    from rlks.ppo import PPO, PPOConfig
    from rlks.tables import synthetic_table

    d = _dev()
    tab = synthetic_table(C, rows, seed=7)
    spec = None if nodes is None else NodeSpec(C, nodes, arrival_rate=2.0, depart_prob=0.05, init_occupancy=0.5,
                                               reject_penalty=0.1)
    cfg = (PPOConfig().framework("torch")
           .training(train_batch_size=N * T, sgd_minibatch_size=mb, num_sgd_iter=1, lr=3e-4,
                     model={"fcnet_hiddens": [H, H]})
           .debugging(seed=5))
    cfg.num_envs, cfg.table, cfg.nodes, cfg.sgd_precision = N, tab, spec, prec
    algo = PPO(config=cfg, device=d)
    assert algo.T == T and algo.N == N
    assert algo.precision == ("wide" if H != 256 else "sf16" if prec == "auto" else prec)
    if per_step:
        algo.bufs.global_lanes = SF_ROLL_FUSED_MAX_LANES + 1
    algo.rollout(explore=explore)
    b = algo.buf
    twin = VecK8sMultiCloudEnv(N, table=tab, seed=5, nodes=spec, device=d)
    assert torch.equal(twin.reset(), b["obs"][0])
    y = _Out(N, 3 * C, d)
    for t in range(T):
        _two_calls(twin, b["logits"][t].contiguous(), explore, y, 5, 0)
        for g, e, what in zip((b["actions"][t], b["logp"][t], b["obs"][t + 1], b["rewards"][t], b["dones"][t]),
                              (y.actions, y.logp, y.obs, y.reward, y.done),
                              ("actions", "logp", "obs", "rewards", "dones")):
            np.testing.assert_array_equal(_bits(g), _bits(e), err_msg=f"{what}[{t}]")
    if rows < T:  # episodes ended inside the rollout
        assert b["dones"].any() and not b["dones"].all()
    if not explore:  # argmax: the lowest index of the maximum
        np.testing.assert_array_equal(b["actions"].cpu().numpy(), b["logits"].cpu().numpy().argmax(2))
