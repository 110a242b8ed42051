"""GPU tests of the serving path: rlks.serving.PolicyServer over k_policy_act.
Fixtures: tests/serving_cases.py.  "Bit for bit" compares the float32 words as uint32."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import oracle
import serving_cases as sc
from parity import close_as_fp32

pytestmark = pytest.mark.gpu

INFO = ("action_logp", "action_dist_inputs", "action_prob", "vf_preds")


def _dev():
    return torch.device("cuda", 0)


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32) if a.dtype == np.float32 else a


def _same(a, b, what=""):
    np.testing.assert_array_equal(_bits(a), _bits(b), err_msg=what)


def _same_out(x, y, rows=None, what=""):
    """(actions, info) pairs equal bit for bit (rows: of x, against all of y)"""
    sel = (lambda v: v) if rows is None else (lambda v: v[rows])
    _same(sel(x[0]), y[0], what + " actions")
    for k in INFO:
        _same(sel(x[1][k]), y[1][k], f"{what} {k}")


@functools.lru_cache(maxsize=None)
def _policy(D, A):
    """the fixture policy on the device, its host parameters and the oracle's forwards of the 33 rows
    (computed once, shared, never written)"""
    from rlks.policy import PolicyParams

    flat, off = sc.fixture_flat(D, A)
    p = PolicyParams(D, sc.H, A, device=_dev(), seed=sc.PARAM_SEED)
    assert list(p.offsets) == off
    p.flat.copy_(torch.from_numpy(flat))
    obs = sc.observations(33, D)
    ref = {"l64v64": oracle.mlp_forward(flat, off, D, sc.H, A, obs),
           "band": oracle.mlp_forward_fp32_band(flat, off, D, sc.H, A, obs)}
    return p, flat, off, obs, ref


def _server(D, A, **kw):
    from rlks.serving import PolicyServer

    return PolicyServer(_policy(D, A)[0], **kw)


def _check_oracle(info, flat, off, D, A, obs, ref=None):
    l64, v64 = ref["l64v64"] if ref else oracle.mlp_forward(flat, off, D, sc.H, A, obs)
    lb, vb = ref["band"] if ref else oracle.mlp_forward_fp32_band(flat, off, D, sc.H, A, obs)
    close_as_fp32(info["action_dist_inputs"], l64, lb, what="logits")
    close_as_fp32(info["vf_preds"], v64, vb, what="values")
    close_as_fp32(info["action_prob"], sc.softmax(l64, np.float64), [sc.softmax(b, np.float32) for b in lb],
                  what="probs")


def _sampler(logits, call, seed, explore, mask_bits=None):
    """rlks_sample_categorical[_masked] on `logits` with ids {SAMPLER_ID, i, call}: (actions, logp, the
    row as drawn from)"""
    from rlks import _lib
    from rlks.serving import SAMPLER_ID

    d = _dev()
    n, A = logits.shape
    lg = torch.from_numpy(np.ascontiguousarray(logits)).to(d)
    ids = np.zeros((n, 3), np.uint32)
    ids[:, 0], ids[:, 1], ids[:, 2] = SAMPLER_ID, np.arange(n), call
    idt = torch.from_numpy(ids.view(np.int32)).to(d)
    act = torch.empty(n, dtype=torch.int32, device=d)
    lp = torch.empty(n, dtype=torch.float32, device=d)
    s = torch.cuda.current_stream(d).cuda_stream
    if mask_bits is None:
        _lib.call("rlks_sample_categorical", _lib.ptr(lg), n, A, _lib.ptr(idt), seed, int(explore), _lib.ptr(act),
                  _lib.ptr(lp), s)
    else:
        mt = torch.from_numpy(mask_bits.view(np.int64).copy()).to(d)
        _lib.call("rlks_sample_categorical_masked", _lib.ptr(lg), _lib.ptr(mt), n, A, _lib.ptr(idt), seed,
                  int(explore), _lib.ptr(act), _lib.ptr(lp), s)
    return act.cpu().numpy(), lp.cpu().numpy(), lg.cpu().numpy()


# ------------------------------------------------------------------------------------------- 1
@pytest.mark.parametrize("D,A", sc.POLICIES)
def test_forward_parity(D, A):
    """logits, values and probabilities of 33 rows against the f64 oracle, as close as the fp32 band"""
    p, flat, off, obs, ref = _policy(D, A)
    srv = _server(D, A, max_rows=33)
    assert srv.fused
    acts, info = srv.act(obs, explore=False, full_fetch=True)
    assert acts.dtype == np.int32 and acts.shape == (33,)
    assert info["action_dist_inputs"].shape == (33, A) and info["action_prob"].shape == (33, A)
    _check_oracle(info, flat, off, D, A, obs, ref)
    np.testing.assert_array_equal(acts, info["action_dist_inputs"].argmax(1))
    np.testing.assert_allclose(info["action_prob"].sum(1), 1.0, atol=1e-6)
    # without full_fetch: the same actions (the value net does not run), and the single-row forms
    np.testing.assert_array_equal(srv.act(obs, explore=False), acts)
    one = srv.act(obs[3], explore=False)
    assert isinstance(one, int) and one == acts[3]
    a1, i1 = srv.act(obs[3], explore=False, full_fetch=True)
    assert a1 == acts[3] and isinstance(i1["vf_preds"], float) and i1["action_prob"].shape == (A,)
    # returned arrays are copies, not views of the staging block
    keep = info["action_prob"].copy()
    srv.act(obs[::-1].copy(), explore=False, full_fetch=True)
    _same(info["action_prob"], keep)


# ------------------------------------------------------------------------------------------- 2
@pytest.mark.parametrize("D,A", sc.POLICIES)
def test_row_independence(D, A):
    """a row's outputs do not depend on n, on its place in its tile, on the other rows or on max_rows"""
    obs = _policy(D, A)[3]
    s33, s1024 = _server(D, A, max_rows=33), _server(D, A, max_rows=1024)
    full = s33.act(obs, explore=False, full_fetch=True)
    _same_out(s33.act(obs, explore=False, full_fetch=True), full, what="repeat")
    _same_out(s1024.act(obs, explore=False, full_fetch=True), full, what="max_rows 1024")
    for i in (0, 15, 16, 32):
        for s in (s33, s1024):
            _same_out(full, s.act(obs[i:i + 1], explore=False, full_fetch=True), rows=slice(i, i + 1), what=f"row {i}")
    for n in sc.ROWS:
        _same_out(full, s1024.act(obs[:n], explore=False, full_fetch=True), rows=slice(0, n), what=f"n = {n}")
    # a row moved to another place in another tile
    perm = np.random.default_rng(0).permutation(33)
    moved = s33.act(obs[perm], explore=False, full_fetch=True)
    _same_out(full, moved, rows=perm, what="permuted")


# ------------------------------------------------------------------------------------------- 3
@pytest.mark.parametrize("D,A", sc.POLICIES)
def test_draw_is_the_shared_draw(D, A):
    """actions and logp are rlks_sample_categorical's on the returned logits with ids {SAMPLER_ID, i,
    call}; the counter advances only when exploring"""
    obs = _policy(D, A)[3]
    seed = 77
    srv = _server(D, A, seed=seed, max_rows=64)
    want_call = 0
    seen = set()
    for explore in (True, True, False, True, False):
        assert srv.calls == want_call
        acts, info = srv.act(obs, explore=explore, full_fetch=True)
        ra, rl, _ = _sampler(info["action_dist_inputs"], want_call, seed, explore)
        _same(acts, ra, f"actions, explore={explore}, call {want_call}")
        _same(info["action_logp"], rl, f"logp, explore={explore}, call {want_call}")
        if explore:
            want_call += 1
            seen.add(tuple(acts))
    assert len(seen) == 3  # three calls, three different draws


def test_draw_matches_the_oracle_restatement():
    """300 rows against oracle.sample_actions; rows within 4 ulp of a CDF boundary are left out (under
    1e-2 of them): the rule and the cap of test_compute_single_action_samples_on_device_philox"""
    from rlks.serving import SAMPLER_ID

    D, A = 24, 8
    obs = sc.observations(300, D, seed=9)
    srv = _server(D, A, seed=77, max_rows=300)
    for call in (0, 1):
        acts, info = srv.act(obs, explore=True, full_fetch=True)
        ref, margin = oracle.sample_actions(info["action_dist_inputs"], np.full(300, SAMPLER_ID, np.uint32),
                                            np.arange(300, dtype=np.uint32), np.full(300, call, np.uint32), 77)
        close = margin < 4
        assert close.mean() < 1e-2
        np.testing.assert_array_equal(acts[~close], ref[~close])
        assert len(set(acts)) > A // 2
    # single observations: row 0 of call k
    one = [srv.act(o) for o in obs[:20]]
    lg = srv.act(obs[:20], explore=False, full_fetch=True)[1]["action_dist_inputs"]
    ref, margin = oracle.sample_actions(lg, np.full(20, SAMPLER_ID, np.uint32), np.zeros(20, np.uint32),
                                        np.arange(2, 22, dtype=np.uint32), 77)
    np.testing.assert_array_equal(np.array(one)[margin >= 4], ref[margin >= 4])


# ------------------------------------------------------------------------------------------- 4
def test_mask():
    from rlks.serving import PolicyServer, pack_mask

    D, A, n, seed = 24, 8, 33, 5
    p, _, _, obs, _ = _policy(D, A)
    plain = PolicyServer(p, seed=seed, max_rows=n)
    raw = plain.act(obs, explore=False, full_fetch=True)[1]["action_dist_inputs"]  # the unmasked logits
    m = sc.random_masks(n, A)
    m[0] = False                       # no bit set: counts as all set
    m[1] = False
    m[1, 5] = True                     # one bit
    m[2] = False
    m[2, raw[2].argmin()] = True       # the only allowed action has the smallest logit
    bits = pack_mask(m, n, A)
    allowed = m.copy()
    allowed[0] = True
    srv = PolicyServer(p, masked=True, seed=seed, max_rows=n)
    call = 0
    for explore in (True, False, True):
        acts, info = srv.act(obs, explore=explore, action_mask=m, full_fetch=True)
        ra, rl, rlog = _sampler(raw, call, seed, explore, mask_bits=bits)
        _same(info["action_dist_inputs"], rlog, "masked logits")
        _same(acts, ra, "actions")
        _same(info["action_logp"], rl, "logp")
        assert allowed[np.arange(n), acts].all()
        assert np.all(info["action_prob"][~allowed] == 0.0)
        assert np.all(info["action_dist_inputs"][~allowed] == np.float32(-1e30))
        _same(info["action_dist_inputs"][allowed], raw[allowed], "unmasked entries")
        np.testing.assert_allclose(info["action_prob"].sum(1), 1.0, atol=1e-6)
        assert acts[1] == 5 and acts[2] == raw[2].argmin()
        call += int(explore)
    # one mask row for every observation; a single observation with its mask
    a_all = srv.act(obs, explore=False, action_mask=m[1])
    assert np.all(a_all == 5)
    assert srv.act(obs[2], explore=False, action_mask=m[2]) == raw[2].argmin()
    with pytest.raises(ValueError, match="action_mask"):
        srv.act(obs)
    with pytest.raises(ValueError, match="action_mask must be"):
        srv.act(obs, action_mask=m[:5])
    with pytest.raises(ValueError, match="compute_actions"):
        srv.act(np.concatenate([obs, obs]), action_mask=m[1])
    with pytest.raises(ValueError, match="obs must be"):
        srv.act(obs[:, :5], action_mask=m)


# ------------------------------------------------------------------------------------------- 5
def test_filter_in_the_kernel_is_the_apply_kernel():
    """a server with the filter on raw rows == a server without one fed ObsFilter.apply(raw); the state
    is merged from data with a large offset and a narrow spread (column 0: 1000 + 1e-3 noise)"""
    from obs_filter_ref import case_data
    from rlks.obs_filter import ObsFilter
    from rlks.serving import PolicyServer

    for D, A in ((6, 2), (9, 3)):
        p = _policy(D, A)[0]
        f = ObsFilter(D, _dev())
        f.stats(torch.from_numpy(case_data(4097, D, seed=0, offset=True)).to(_dev()))
        f.merge()
        n_seen, mean, _, inv = f.numpy()
        assert n_seen == 4097 and abs(mean[0] - 1000.0) < 1e-2 and inv[0] > 100.0
        raw = case_data(33, D, seed=1, offset=True)
        filtered = f.apply(torch.from_numpy(raw).to(_dev())).cpu().numpy()
        assert np.abs(filtered[:, 0]).max() < 10.0  # standardised, so the forward sees O(1) inputs
        with_f = PolicyServer(p, obs_filter=f, seed=3, max_rows=33)
        without = PolicyServer(p, seed=3, max_rows=33)
        for explore in (False, True):
            _same_out(with_f.act(raw, explore=explore, full_fetch=True),
                      without.act(filtered, explore=explore, full_fetch=True), what=f"D={D} explore={explore}")
        _same_out(with_f.act(raw[7:8], explore=False, full_fetch=True),
                  without.act(filtered[7:8], explore=False, full_fetch=True), what="one row")


# ------------------------------------------------------------------------------------------- 6
def _cfg(N, T, mb, epochs=1, seed=11, **kw):
    from rlks.ppo import PPOConfig

    cfg = (PPOConfig().environment("K8sMultiCloudEnv").framework("torch")
           .training(train_batch_size=N * T, sgd_minibatch_size=mb, num_sgd_iter=epochs, lr=3e-4, gamma=0.99, **kw)
           .debugging(seed=seed))
    cfg.num_envs = N
    cfg.rollout_fragment_length = T
    return cfg


def test_live_weights_and_checkpoint(tmp_path):
    """PPO.server() reads the live parameters: it matches the oracle before train() and, without being
    rebuilt, on the new weights after it; a server from the saved checkpoint equals it bit for bit"""
    from rlks.ppo import PPO
    from rlks.serving import PolicyServer

    algo = PPO(config=_cfg(256, 8, 1024), device=_dev())
    srv = algo.server()
    assert srv.fused and srv.calls == 0 and srv.max_rows == 1024
    obs = sc.observations(33, 6)
    before = algo.params.flat.cpu().numpy().copy()
    _check_oracle(srv.act(obs, explore=False, full_fetch=True)[1], before, algo.params.offsets, 6, 2, obs)
    algo.train()
    after = algo.params.flat.cpu().numpy().copy()
    assert np.abs(after - before).max() > 1e-5
    out = srv.act(obs, explore=False, full_fetch=True)
    _check_oracle(out[1], after, algo.params.offsets, 6, 2, obs)
    calls = algo.sample_calls
    srv.act(obs)  # an exploring call: the server's own counter, not the algorithm's
    assert srv.calls == 1 and algo.sample_calls == calls
    path = algo.save(str(tmp_path))
    loaded = PolicyServer.from_checkpoint(path)
    assert loaded.fused and not loaded.masked and loaded.obs_filter is None and loaded.seed == 11
    assert loaded.explore == algo.config.explore and loaded.calls == 0
    _same_out(loaded.act(obs, explore=False, full_fetch=True), out, what="from_checkpoint")
    algo.stop()


def test_checkpoint_carries_filter_and_mask(tmp_path):
    from rlks.env import NodeSpec
    from rlks.ppo import PPO
    from rlks.serving import PolicyServer
    from rlks.tables import synthetic_table

    cfg = _cfg(256, 8, 1024, action_mask="room")
    cfg.rollouts(observation_filter="MeanStdFilter")
    cfg.table, cfg.nodes = synthetic_table(3, 100, seed=7), NodeSpec(3, 16)
    algo = PPO(config=cfg, device=_dev())
    algo.train()  # the filter's state now holds the first rollout's observations
    srv = algo.server(max_rows=64)
    assert srv.fused and srv.masked and srv.obs_filter is algo.obs_filter and (srv.D, srv.A) == (9, 3)
    path = algo.save(str(tmp_path))
    loaded = PolicyServer.from_checkpoint(path, max_rows=64)
    assert loaded.masked and loaded.obs_filter is not None and loaded.fused
    _same(loaded.obs_filter.state.cpu().numpy().view(np.uint64), algo.obs_filter.state.cpu().numpy().view(np.uint64))
    assert algo.obs_filter.numpy()[0] > 0
    obs = algo.current_obs()[:33].cpu().numpy()
    m = sc.random_masks(33, 3)
    for explore in (False, True):
        _same_out(loaded.act(obs, explore=explore, action_mask=m, full_fetch=True),
                  srv.act(obs, explore=explore, action_mask=m, full_fetch=True), what=f"explore={explore}")
    with pytest.raises(ValueError, match="action_mask"):
        loaded.act(obs)
    # and the existing path agrees on the greedy actions' masks
    acts = loaded.act(obs, explore=False, action_mask=m)
    assert m[np.arange(33), acts].all()
    algo.stop()


# ------------------------------------------------------------------------------------------- 7
def test_agrees_with_compute_actions():
    """greedy server.act == compute_actions(explore=False) on 1,024 fixture rows, near-ties left out (at
    most 1 %: test_serving_host proves the cap from the oracle alone)"""
    from rlks.ppo import PPO

    D, A = 6, 2
    flat, off = sc.fixture_flat(D, A)
    algo = PPO(config=_cfg(256, 8, 1024), device=_dev())
    assert list(algo.params.offsets) == off
    algo.params.flat.copy_(torch.from_numpy(flat).to(_dev()))
    obs = sc.observations(sc.AGREE_ROWS, D)
    srv = algo.server(max_rows=sc.AGREE_ROWS)
    got = srv.act(obs, explore=False)
    ref = algo.compute_actions(obs, explore=False).cpu().numpy()
    l64, _ = oracle.mlp_forward(flat, off, D, sc.H, A, obs)
    band, _ = oracle.mlp_forward_fp32_band(flat, off, D, sc.H, A, obs)
    tie = sc.near_ties(l64, band)
    assert tie.mean() <= sc.AGREE_MAX_LEFT_OUT
    np.testing.assert_array_equal(got[~tie], ref[~tie])
    np.testing.assert_array_equal(got[~tie], l64.argmax(1)[~tie])
    assert len(set(got)) == A
    algo.stop()


# ------------------------------------------------------------------------------------------- 8
def test_fallback_outside_the_kernels_scope():
    """hidden 384 (D = 48, A = 16): server.fused is False and act() is compute_actions' sequence, the
    same bits for the same seed and counter"""
    from rlks.env import NodeSpec
    from rlks.ppo import PPO
    from rlks.tables import synthetic_table

    cfg = _cfg(256, 8, 1024, model={"fcnet_hiddens": [384, 384]})
    cfg.table, cfg.nodes = synthetic_table(16, 100, seed=7), NodeSpec(16, 8)
    algo = PPO(config=cfg, device=_dev())
    srv = algo.server(max_rows=64)
    assert not srv.fused and (srv.D, srv.H, srv.A) == (48, 384, 16)
    obs = sc.observations(33, 48)
    for explore in (True, False, True):
        assert srv.calls == algo.sample_calls
        got, info = srv.act(obs, explore=explore, full_fetch=True)
        ref = algo.compute_actions(obs, explore=explore).cpu().numpy()
        _same(got, ref, f"explore={explore}")
        lg, v = algo.params.forward(torch.from_numpy(obs).to(_dev()))
        _same(info["action_dist_inputs"], lg.cpu().numpy())
        _same(info["vf_preds"], v.cpu().numpy())
    assert srv.calls == 2
    assert isinstance(srv.act(obs[0], explore=False), int)
    algo.stop()
