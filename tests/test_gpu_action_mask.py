"""Invalid-action masking on the device: rlks_env_action_mask, rlks_env_masked_sample,
rlks_sample_categorical_masked, the loss heads' select, the masked rollouts and the Python surface, held to
the restatements of tests/action_mask_ref.py (tied to the oracle by tests/test_action_mask_host.py)."""
import ctypes as C
import dataclasses

import numpy as np
import pytest

import action_mask_ref as am
import node_regimes as nr
import node_sample_cases as ns
import oracle
import rule_ref as rr

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

EPS32 = 2.0 ** -23
# logp = (l[a] - max) - logf(sum expf(l - max)) in float32 against the float64 log-softmax of the same
# float32 row: two subtractions, the sum and logf, each rounded at a magnitude of at most max(1, |logp|)
# (the sum is in [1, A], its log below |logp| + 1): 8 roundings' worth is a generous bound
LOGP_TOL = 8 * EPS32


def _dev():
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    return torch.device("cuda", 0)


def _u32(x):
    x = x.cpu().numpy() if hasattr(x, "cpu") else np.asarray(x)
    return x.view(np.uint32)


def _make_env(case, d, **kw):
    from rlks import VecK8sMultiCloudEnv

    kw.setdefault("seed", nr.SEED)
    kw.setdefault("env_offset", nr.ENV_OFFSET)
    return VecK8sMultiCloudEnv(case.n, table=nr.table(case), nodes=rr.node_spec(case), device=d, **kw)


def _bits(X):
    from rlks import _lib

    b = torch.full((X.num_envs,), -1, dtype=torch.int64, device=X.device)
    _lib.call("rlks_env_action_mask", X.handle, _lib.ptr(b), X.dev.stream)
    return b.cpu().numpy().view(np.uint64)


def _logp_close(lp, ref, what):
    lp = np.asarray(lp, np.float64)
    err = np.abs(lp - ref)
    assert (err <= LOGP_TOL * np.maximum(1.0, np.abs(ref))).all(), (what, float(err.max()))


# ----------------------------------------------------------------------------- 1. mask
@pytest.mark.parametrize("name", am.MASK_CASES)
def test_mask_follows_the_reference(name):
    case = rr.CASES[name]
    run = am.check_mask_guards(name)  # clusters fill, and somewhere no cluster has room
    d = _dev()
    X = _make_env(case, d)
    X.reset()
    full = np.uint64((1 << case.C) - 1)
    all_ones = 0
    for t in range(case.steps):
        bits = _bits(X)
        np.testing.assert_array_equal(bits, am.mask_bits(run.masks[t]), err_msg=f"mask before step {t}")
        if t % 10 == 0:
            m = X.action_mask()
            assert m.dtype == torch.bool and tuple(m.shape) == (case.n, case.C)
            np.testing.assert_array_equal(m.cpu().numpy(), run.masks[t])
        no_room = ~rr.has_room(X.node_state()[2].cpu().numpy(), rr.spec_of(case)).any(1)
        assert (bits[no_room] == full).all()
        all_ones += int(no_room.sum())
        X.step(torch.from_numpy(run.actions[t]).to(d))
    X.check_status()
    assert all_ones == run.no_room >= rr.FLOORS[name]["no_room"]
    X.close()


def test_mask_of_a_table_env_and_of_too_many_clusters():
    from rlks import VecK8sMultiCloudEnv, _lib
    from rlks.tables import synthetic_table

    d = _dev()
    X = VecK8sMultiCloudEnv(300, table=synthetic_table(3, 100, seed=7), seed=1, device=d)
    X.reset()
    assert bool(X.action_mask().all()) and (_bits(X) == np.uint64(7)).all()
    with pytest.raises(_lib.RlksError, match=r"\(-3\)"):  # RLKS_ERR_UNSUPPORTED
        _lib.call("rlks_env_set_action_masking", X.handle, 1)
    # all-true mask: the plain sampler's draw
    lg = torch.from_numpy(np.random.default_rng(0).normal(0, 1.5, (300, 3)).astype(np.float32)).to(d)
    before = lg.clone()
    a, lp = X.masked_sample(lg)
    assert torch.equal(lg, before)
    st, ep = X.lane_state()
    ids = torch.stack([torch.arange(300, dtype=torch.int32, device=d), ep, st], 1).contiguous()
    ea = torch.empty(300, dtype=torch.int32, device=d)
    elp = torch.empty(300, dtype=torch.float32, device=d)
    _lib.call("rlks_sample_categorical", _lib.ptr(lg), 300, 3, _lib.ptr(ids), 1, 1, _lib.ptr(ea), _lib.ptr(elp), X.dev.stream)
    assert torch.equal(a, ea) and torch.equal(lp.view(torch.int32), elp.view(torch.int32))
    X.close()
    W = VecK8sMultiCloudEnv(8, table=synthetic_table(65, 100, seed=7), seed=1, device=d)
    W.reset()
    with pytest.raises(_lib.RlksError, match=r"\(-3\)"):
        W.action_mask()
    with pytest.raises(_lib.RlksError, match=r"\(-3\)"):
        W.masked_sample(torch.zeros(8, 65, device=d))
    W.close()
    # 64 clusters: the whole word
    V = VecK8sMultiCloudEnv(5, table=synthetic_table(64, 100, seed=7), seed=1, device=d)
    V.reset()
    assert (_bits(V) == np.uint64(2 ** 64 - 1)).all() and bool(V.action_mask().all())
    V.close()


# ----------------------------------------------------------------------------- 2. sampler
@pytest.mark.parametrize("name", am.MASK_CASES)
def test_masked_sample_follows_the_reference(name):
    from rlks import _lib

    case = rr.CASES[name]
    run = am.check_mask_guards(name)
    d = _dev()
    X = _make_env(case, d)
    X.reset()
    n, A = case.n, case.C
    gids = nr.ENV_OFFSET + np.arange(n)
    rows = np.arange(n)
    ea2 = torch.empty(n, dtype=torch.int32, device=d)
    elp2 = torch.empty(n, dtype=torch.float32, device=d)
    mask_out = torch.zeros(n, dtype=torch.int64, device=d)
    unsure = masked_entries = 0
    for t in range(case.steps):
        explore = t % 4 != 3
        lg_h = am.step_logits(case, t)
        m = run.masks[t]
        ml, ea, margin, elp = am.sample_masked(lg_h, m, gids, run.episodes[t], run.steps[t], nr.SEED, explore=explore)
        lg = torch.from_numpy(lg_h).to(d)
        if t % 2:
            a, lp = X.masked_sample(lg, explore=explore)
        else:  # the C entry with the mask output
            a = torch.empty(n, dtype=torch.int32, device=d)
            lp = torch.empty(n, dtype=torch.float32, device=d)
            _lib.call("rlks_env_masked_sample", X.handle, _lib.ptr(lg), int(explore), _lib.ptr(a), _lib.ptr(lp),
                      _lib.ptr(mask_out), X.dev.stream)
            np.testing.assert_array_equal(mask_out.cpu().numpy().view(np.uint64), am.mask_bits(m))
        np.testing.assert_array_equal(_u32(lg), ml.view(np.uint32), err_msg=f"masked logits at step {t}")
        a_h = a.cpu().numpy()
        assert m[rows, a_h].all(), f"an action on a masked cluster at step {t}"
        sure = margin >= ns.MARGIN_ULP
        unsure += int((~sure).sum())
        np.testing.assert_array_equal(a_h[sure], ea[sure], err_msg=f"actions at step {t}")
        _logp_close(lp.cpu().numpy()[sure], elp[sure], f"logp at step {t}")
        # and, to the bit, the plain sampler on the masked row with the lanes' own counters
        st, ep = X.lane_state()
        ids = torch.stack([torch.arange(n, dtype=torch.int32, device=d) + nr.ENV_OFFSET, ep, st], 1).contiguous()
        _lib.call("rlks_sample_categorical", _lib.ptr(lg), n, A, _lib.ptr(ids), nr.SEED, int(explore), _lib.ptr(ea2),
                  _lib.ptr(elp2), X.dev.stream)
        assert torch.equal(a, ea2) and torch.equal(lp.view(torch.int32), elp2.view(torch.int32)), t
        masked_entries += int((~m).sum())
        X.step(torch.from_numpy(run.actions[t]).to(d))
    assert masked_entries >= rr.FLOORS[name]["some_full"] - rr.FLOORS[name]["no_room"]
    assert unsure <= 1e-3 * n * case.steps  # a draw within 4 ulp of a CDF boundary: about 2^-20 of them
    X.close()


def test_roomy_masked_sample_is_sample_step():
    case = am.ROOMY
    d = _dev()
    X, Y = _make_env(case, d), _make_env(case, d)
    np.testing.assert_array_equal(_u32(X.reset()), _u32(Y.reset()))
    for t in range(40):
        lg_h = ns.logits(case, t)  # (with the sampler's edge rows: ties, -inf, underflow)
        lx, ly = torch.from_numpy(lg_h).to(d), torch.from_numpy(lg_h).to(d)
        a, lp = X.masked_sample(lx, explore=t % 5 != 4)
        ea, elp, eobs, _, _ = Y.sample_step(ly, explore=t % 5 != 4)
        np.testing.assert_array_equal(_u32(lx), lg_h.view(np.uint32), err_msg=f"logits at step {t}")
        assert torch.equal(a, ea), t
        np.testing.assert_array_equal(_u32(lp), _u32(elp), err_msg=f"logp at step {t}")
        obs, *_ = X.step(a)
        np.testing.assert_array_equal(_u32(obs), _u32(eobs), err_msg=f"obs after step {t}")
    assert bool(X.action_mask().all())
    X.close()
    Y.close()


# ----------------------------------------------------------------------------- 3. fallback
def test_fallback_is_the_highest_unmasked_action():
    from rlks import _lib

    d = _dev()
    masks = np.array([[1, 1, 1, 0], [1, 0, 1, 0], [1, 1, 0, 0], [0, 1, 0, 0], [1, 1, 1, 1], [0, 0, 0, 0]], bool)
    want = [2, 2, 1, 1, 3, 3]  # (a mask without a bit counts as all of them)
    n, A = masks.shape
    lg_h = np.random.default_rng(1).normal(0, 1.0, (n, A)).astype(np.float32)
    ids = torch.tensor([list(am.FALLBACK_IDS)] * n, dtype=torch.int64).to(torch.int32).to(d).contiguous()
    bits = torch.from_numpy(am.mask_bits(masks).view(np.int64)).to(d)
    lg = torch.from_numpy(lg_h).to(d)
    a = torch.empty(n, dtype=torch.int32, device=d)
    lp = torch.empty(n, dtype=torch.float32, device=d)
    _lib.call("rlks_sample_categorical_masked", _lib.ptr(lg), _lib.ptr(bits), n, A, _lib.ptr(ids), am.FALLBACK_SEED, 1,
              _lib.ptr(a), _lib.ptr(lp), None)
    np.testing.assert_array_equal(a.cpu().numpy(), want)
    eff = masks.copy()
    eff[~eff.any(1)] = True
    ml, ea, _, elp = am.sample_masked(lg_h, eff, *[np.full(n, v) for v in am.FALLBACK_IDS], am.FALLBACK_SEED)
    np.testing.assert_array_equal(ea, want)
    np.testing.assert_array_equal(_u32(lg), ml.view(np.uint32))
    _logp_close(lp.cpu().numpy(), elp, "logp")
    # the plain sampler's default for the same counter is A - 1
    lg = torch.from_numpy(lg_h).to(d)
    _lib.call("rlks_sample_categorical", _lib.ptr(lg), n, A, _lib.ptr(ids), am.FALLBACK_SEED, 1, _lib.ptr(a), None, None)
    np.testing.assert_array_equal(a.cpu().numpy(), np.full(n, A - 1))
    with pytest.raises(_lib.RlksError, match=r"\(-3\)"):
        _lib.call("rlks_sample_categorical_masked", _lib.ptr(lg), _lib.ptr(bits), 1, 65, _lib.ptr(ids), 1, 1, _lib.ptr(a),
                  None, None)


# ----------------------------------------------------------------------------- 4. loss
@pytest.mark.parametrize("name,D,H,A,rows,prec", am.LOSS_CASES)
def test_masked_loss_matches_the_reference(name, D, H, A, rows, prec):
    """rlks_ppo_grad on records with masked old logits against the masked float64 reference: the project's
    per-tensor norm-wise 1e-5, the stats sums to relative 1e-5, everything finite, and exact zeros in the
    always-masked action's W3 row and b3 entry.  Without the select in the loss heads this fails."""
    from rlks import _lib
    from rlks.policy import TENSOR_NAMES, PolicyParams

    d = _dev()
    p = PolicyParams(D, H, A, device=d, seed=3)
    p.desc.precision = {"sf16": _lib.RLKS_PRECISION_SF16, "fp32": _lib.RLKS_PRECISION_FP32,
                        "wide": _lib.RLKS_PRECISION_WIDE}[prec]
    assert p.wide() == (prec == "wide")
    if prec == "sf16":
        assert _lib.lib().rlks_sf_f1_fused(C.byref(p.desc)) == (1 if A <= 4 else 0)
    mb, mask = am.loss_minibatch(D, A, rows)
    klc, ent_c = 0.2, 0.01
    dyn = torch.tensor([0.1, 0.9, klc, 1.0 / rows, 0, 0, 0, 0], dtype=torch.float32, device=d)
    co = _lib.PpoCoeffs(0.3, 10.0, 1.0, ent_c)
    wsb = C.c_int64()
    _lib.call("rlks_ppo_workspace_bytes", C.byref(p.desc), rows, C.byref(wsb))
    ws = torch.empty(wsb.value, dtype=torch.uint8, device=d)
    grad = torch.zeros(p.padded, device=d)
    stats = torch.zeros(8, dtype=torch.float64, device=d)
    mbt = torch.from_numpy(mb).to(d)
    _lib.call("rlks_ppo_grad", C.byref(p.desc), C.byref(co), p.flat.data_ptr(), dyn.data_ptr(), mbt.data_ptr(), rows,
              grad.data_ptr(), stats.data_ptr(), ws.data_ptr(), ws.numel(), None)
    g = grad.cpu().numpy()
    st = stats.cpu().numpy()
    dh = dyn.cpu().numpy()
    eg, est = am.ppo_loss_grad_masked(p.flat.cpu().numpy(), p.offsets, D, H, A, mb, entropy_coeff=float(np.float32(ent_c)),
                                      kl_coeff=float(dh[2]), adv_mean=float(dh[0]), adv_inv_std=float(dh[1]))
    assert np.isfinite(g).all() and np.isfinite(st).all()
    for i, (tname, _, _) in enumerate(TENSOR_NAMES):
        n = int(np.prod(p.shapes[i]))
        a, b = g[p.offsets[i]: p.offsets[i] + n], eg[p.offsets[i]: p.offsets[i] + n]
        rel = np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-300)
        print(f"{name} {tname}: rel {rel:.3e}")
        assert np.linalg.norm(a - b) <= 1e-5 * np.linalg.norm(b) + 1e-12, (tname, rel)
    for k, j in (("policy_loss", 0), ("kl", 2), ("entropy", 3)):
        print(f"{name} {k}: device {st[j]!r} reference {est[k]!r}")
        assert abs(st[j] - est[k]) <= 1e-5 * abs(est[k]), (k, st[j], est[k])
    assert st[4] == rows
    w3 = g[p.offsets[4]: p.offsets[4] + A * H].reshape(A, H)
    assert (w3[am.LOSS_ALWAYS_MASKED] == 0.0).all() and g[p.offsets[5] + am.LOSS_ALWAYS_MASKED] == 0.0
    if A > 2:  # (at 2 actions one action is left: its probability is 1 and the policy gradient is zero)
        assert np.abs(w3).max() > 0


# ----------------------------------------------------------------------------- 5. rollout
def _algo(case, d, mask, filt=False, seed=am.ROLLOUT_SEED):
    from rlks.ppo import PPO, PPOConfig

    N, T = am.ROLLOUT_N, am.ROLLOUT_T
    cfg = (PPOConfig().framework("torch")
           .training(train_batch_size=N * T, sgd_minibatch_size=2048, num_sgd_iter=1, lr=3e-4, action_mask=mask)
           .debugging(seed=seed))
    if filt:
        cfg.rollouts(observation_filter="MeanStdFilter")
    cfg.num_envs, cfg.table, cfg.nodes = N, nr.table(case), rr.node_spec(case)
    algo = PPO(config=cfg, device=d)
    assert algo.T == T and algo.N == N
    return algo


def _check_rollout(algo, ora, spec, what):
    """the rollout's buffers against the oracle stepped by the stored actions; -> lane-steps with a masked cluster"""
    b = {k: v.cpu().numpy() for k, v in algo.buf.items()}
    raw = algo.raw.cpu().numpy() if algo.raw is not None else b["obs"]
    N = algo.N
    rows = np.arange(N)
    masked = 0
    for t in range(algo.T):
        m = am.room_mask(ora.node_state()[2], spec)
        lg = b["logits"][t]
        np.testing.assert_array_equal(lg <= am.MASKED_LOGIT_MAX, ~m, err_msg=f"{what}: masked logits at step {t}")
        assert (lg[~m] == am.MASKED_LOGIT).all() and np.isfinite(lg).all()
        a = b["actions"][t]
        assert m[rows, a].all(), f"{what}: a decision on a full cluster at step {t}"
        l64 = lg.astype(np.float64)
        mx = l64.max(1, keepdims=True)
        ref = (l64 - mx - np.log(np.exp(l64 - mx).sum(1, keepdims=True)))[rows, a]
        _logp_close(b["logp"][t], ref, f"{what}: logp at step {t}")
        o, r, term, _, _, status = ora.step(a)
        assert not status.any()
        np.testing.assert_array_equal(raw[t + 1].view(np.uint32), o.view(np.uint32), err_msg=f"{what}: obs[{t + 1}]")
        np.testing.assert_array_equal(b["rewards"][t].view(np.uint32), r.astype(np.float32).view(np.uint32))
        np.testing.assert_array_equal(b["dones"][t], term)
        masked += int((~m.all(1)).sum())
    return masked


@pytest.mark.parametrize("name,filt", [("G", False), ("J", False), ("G", True)])
def test_rollout_obeys_the_mask(name, filt):
    """G: the split-fp16 node rollout (4 actions); J: the generic-width rollout (3 actions); G again through
    rlks_rollout_filtered"""
    case = am.rollout_case(name)
    spec = rr.spec_of(case)
    d = _dev()
    algo = _algo(case, d, "room", filt)
    assert algo.precision == ("sf16" if name == "G" else "wide")
    ora = am.rollout_oracle(case, am.ROLLOUT_SEED)
    first = (algo.raw if filt else algo.buf["obs"])[0].cpu().numpy()
    np.testing.assert_array_equal(first.view(np.uint32), ora.reset().view(np.uint32))
    masked = 0
    for it in range(am.ROLLOUT_ITERS[name]):
        algo.rollout(explore=True)
        masked += _check_rollout(algo, ora, spec, f"{name} rollout {it}")
    print(f"{name} filter={filt}: {masked} lane-steps with a masked cluster")
    assert masked >= am.ROLLOUT_FLOORS[name] > 0, masked
    algo.stop()


@pytest.mark.parametrize("filt", [False, True])
def test_roomy_rollout_is_bit_identical_to_unmasked(filt):
    case = dataclasses.replace(am.ROOMY, n=am.ROLLOUT_N)
    d = _dev()
    X, Y = _algo(case, d, "room", filt), _algo(case, d, None, filt)
    for it in range(2):
        X.rollout(explore=True)
        Y.rollout(explore=True)
        for k in X.buf:
            if k in ("adv", "vtarg"):
                continue
            assert torch.equal(X.buf[k], Y.buf[k]), (k, it)
        assert float(X.buf["logits"].min()) > float(am.MASKED_LOGIT_MAX)
    rx, ry = X.train(), Y.train()
    assert torch.equal(X.params.flat, Y.params.flat)
    assert rx["info"]["learner"]["default_policy"]["learner_stats"] == ry["info"]["learner"]["default_policy"]["learner_stats"]
    X.stop()
    Y.stop()


# ----------------------------------------------------------------------------- 6. surface
EVAL_EPISODES = 64
# lane-steps (of 99 x 64) with a masked cluster along evaluate_nodes' greedy masked run of the surface test's
# policy, measured once with the oracle replay below; the floor is a tenth
EVAL_MEASURED = 4246
EVAL_FLOOR = EVAL_MEASURED // 10


def test_python_surface(tmp_path):
    from rlks.evaluation import evaluate_nodes
    from rlks.ppo import PPO, PPOConfig

    case = am.rollout_case("J")
    spec = rr.spec_of(case)
    d = _dev()
    algo = _algo(case, d, "room")
    for _ in range(2):
        r = algo.train()
        ls = r["info"]["learner"]["default_policy"]["learner_stats"]
        for k in ("policy_loss", "vf_loss", "kl", "entropy", "cur_kl_coeff", "cur_lr"):
            assert np.isfinite(ls[k]), (k, ls)
    assert bool(torch.isfinite(algo.params.flat).all())
    # evaluate_nodes(algo, ...) masks: the trace obeys the mask under the oracle's replay
    seed = 11
    res = evaluate_nodes(algo, EVAL_EPISODES, nodes=rr.node_spec(case), table=nr.table(case), seed=seed, device=d)
    tab = nr.table(case)
    ora = oracle.OracleEnv(oracle.make_cfg(EVAL_EPISODES, nr.N_ROWS, case.C, noise_mode=0, seed=seed, autoreset=0,
                                           nodes=case.nodes, pod_cpu_m=nr.POD_CPU_M, pod_mem_mi=nr.POD_MEM_MI,
                                           arrival_mode=0, arrival_rate=case.rate, depart_prob=case.depart,
                                           init_occupancy=case.occ, reject_penalty=case.penalty),
                           tab.cost, tab.latency, np.array(case.cpu, np.int32), np.array(case.mem, np.int32), None)
    ora.reset()
    rows = np.arange(EVAL_EPISODES)
    masked = 0
    ret = np.zeros(EVAL_EPISODES)
    for t in range(res.actions.shape[0]):
        m = am.room_mask(ora.node_state()[2], spec)
        assert m[rows, res.actions[t]].all(), f"evaluation decided on a full cluster at step {t}"
        masked += int((~m.all(1)).sum())
        _, r, _, _, _, status = ora.step(res.actions[t])
        assert not status.any()
        ret += r
    np.testing.assert_array_equal(ret, res.rewards)
    print(f"evaluate_nodes: {masked} lane-steps with a masked cluster")
    assert masked >= EVAL_FLOOR > 0, masked
    ev = algo.evaluate(episodes=8)
    assert np.isfinite(ev["episode_reward_mean"])
    off = evaluate_nodes(algo, EVAL_EPISODES, nodes=rr.node_spec(case), table=nr.table(case), seed=seed, device=d,
                         action_mask=False)
    assert off.actions.shape == res.actions.shape
    # compute_actions / compute_single_action under a caller's mask
    rng = np.random.default_rng(2)
    n = 200
    obs = rng.random((n, algo.D)).astype(np.float32)
    mask = rng.random((n, algo.A)) < 0.5
    mask[np.arange(n), rng.integers(0, algo.A, n)] = True
    lg, _ = algo.params.forward(torch.from_numpy(obs).to(d))
    greedy = algo.compute_actions(obs, explore=False, action_mask=mask).cpu().numpy()
    np.testing.assert_array_equal(greedy, am.mask_logits(lg.cpu().numpy(), mask).argmax(1))
    calls = algo.sample_calls
    drawn = algo.compute_actions(obs, explore=True, action_mask=torch.from_numpy(mask).to(d)).cpu().numpy()
    assert mask[np.arange(n), drawn].all() and algo.sample_calls == calls + 1
    one = np.array([False, False, True])
    assert algo.compute_single_action(obs[0], explore=True, action_mask=one) == 2
    for call in (lambda: algo.compute_actions(obs), lambda: algo.compute_single_action(obs[0], explore=False)):
        with pytest.raises(ValueError, match="action_mask"):
            call()
    assert algo.sample_calls == calls + 2
    with pytest.raises(ValueError, match="action_mask"):
        algo.compute_actions(obs, action_mask=mask[:5])
    # the setting travels through a checkpoint
    with pytest.warns(RuntimeWarning, match="env lanes"):  # (node-level envs: checkpoint_env_state is off by default)
        back = PPO.from_checkpoint(algo.save(tmp_path), device=d)
    assert back.action_mask == "room" and back.config.action_mask == "room"
    assert torch.equal(back.params.flat, algo.params.flat)
    with pytest.raises(ValueError, match="action_mask"):
        back.compute_actions(obs)
    np.testing.assert_array_equal(back.compute_actions(obs, explore=False, action_mask=mask).cpu().numpy(), greedy)
    back.stop()
    # an unmasked algorithm takes a mask too, and needs none
    cfg = algo.config.copy()
    cfg.action_mask = None
    plain = PPO(config=cfg, device=d)
    assert plain.compute_actions(obs).shape == (n,)
    assert mask[np.arange(n), plain.compute_actions(obs, action_mask=mask).cpu().numpy()].all()
    plain.stop()
    # the config errors, raised by PPO.__init__
    bad = algo.config.copy()
    bad.action_mask = "full"
    with pytest.raises(ValueError, match="action_mask"):
        PPO(config=bad, device=d)
    bad = PPOConfig().training(action_mask="room", sgd_minibatch_size=256)
    with pytest.raises(ValueError, match="node-level"):
        PPO(config=bad, device=d)
    algo.stop()
