"""CPU checks of invalid-action masking: the config surface, the restatements of
tests/action_mask_ref.py tied to the oracle (with an all-true mask they are oracle.sample_actions and
oracle.ppo_loss_grad exactly), the committed fallback counter, and the regime guards of every case the
GPU tests use, computed from the oracle alone."""
import json

import numpy as np
import pytest

import action_mask_ref as am
import oracle
import rule_ref as rr


def _spec():
    return rr.node_spec(rr.CASES["J"])


def test_config_validation_and_round_trip():
    from rlks.ppo import PPOConfig, validate_action_mask

    c = PPOConfig()
    assert c.action_mask is None and c.to_dict()["action_mask"] is None
    assert validate_action_mask(None) is None and validate_action_mask(None, None, 96) is None
    assert validate_action_mask("room", _spec(), 3) == "room"
    for bad in ("none", "rooms", True, 1, ["room"]):
        with pytest.raises(ValueError, match="action_mask"):
            validate_action_mask(bad, _spec(), 3)
    with pytest.raises(ValueError, match="node-level"):
        validate_action_mask("room", None, 2)
    with pytest.raises(ValueError, match="64"):
        validate_action_mask("room", _spec(), 65)
    c = PPOConfig().training(action_mask="room", lr=1e-3)
    c.nodes = _spec()
    d = json.loads(json.dumps(c.to_dict()))  # the round trip a checkpoint makes (algorithm_state.json)
    assert d["action_mask"] == "room"
    c2 = PPOConfig.from_dict(d)
    assert c2.action_mask == "room" and c2.nodes.to_dict() == c.nodes.to_dict() and c2.lr == 1e-3
    assert PPOConfig.from_dict(json.loads(json.dumps(PPOConfig().to_dict()))).action_mask is None
    # a checkpoint from before the setting existed
    d.pop("action_mask")
    assert PPOConfig.from_dict(d).action_mask is None


def test_sentinel_matches_the_header():
    from conftest import ROOT
    from rlks import _lib

    txt = (ROOT / "include" / "rlks_types.h").read_text()
    assert "#define RLKS_MASKED_LOGIT (-1e30f)" in txt and "#define RLKS_MASKED_LOGIT_MAX (-1e29f)" in txt
    assert np.float32(_lib.RLKS_MASKED_LOGIT) == am.MASKED_LOGIT
    assert np.float32(_lib.RLKS_MASKED_LOGIT_MAX) == am.MASKED_LOGIT_MAX
    # finite, and far enough down that float32 exp() of (sentinel - any finite policy logit) is exactly 0
    assert np.isfinite(am.MASKED_LOGIT) and am.MASKED_LOGIT <= am.MASKED_LOGIT_MAX
    assert np.exp(np.float32(am.MASKED_LOGIT_MAX) - np.float32(-1e28)) == 0.0


def test_all_true_mask_is_the_oracle_sampler():
    rng = np.random.default_rng(3)
    n, A = 500, 5
    lg = rng.normal(0, 1.5, (n, A)).astype(np.float32)
    gids, ep, st = np.arange(n) + 3, rng.integers(0, 4, n), rng.integers(0, 99, n)
    ea, em = oracle.sample_actions(lg, gids, ep, st, 4)
    ml, a, m, lp = am.sample_masked(lg, np.ones((n, A), bool), gids, ep, st, 4)
    np.testing.assert_array_equal(ml.view(np.uint32), lg.view(np.uint32))
    np.testing.assert_array_equal(a, ea)
    np.testing.assert_array_equal(m, em)
    l64 = lg.astype(np.float64)
    np.testing.assert_allclose(lp, (l64 - np.log(np.exp(l64).sum(1, keepdims=True)))[np.arange(n), ea], rtol=0, atol=1e-12)
    _, g, _, _ = am.sample_masked(lg, np.ones((n, A), bool), gids, ep, st, 4, explore=False)
    np.testing.assert_array_equal(g, lg.argmax(1))


def test_masked_sampler_stays_on_the_mask():
    rng = np.random.default_rng(4)
    n, A = 2000, 6
    lg = rng.normal(0, 1.5, (n, A)).astype(np.float32)
    mask = rng.random((n, A)) < 0.5
    mask[np.arange(n), rng.integers(0, A, n)] = True
    for explore in (True, False):
        ml, a, _, lp = am.sample_masked(lg, mask, np.arange(n), np.zeros(n), np.arange(n) % 99, 9, explore=explore)
        assert mask[np.arange(n), a].all()
        assert (ml[~mask] == am.MASKED_LOGIT).all() and np.array_equal(ml[mask], lg[mask])
        assert np.isfinite(lp).all() and (lp <= 0).all()
    np.testing.assert_array_equal(am.mask_bits(mask), [sum(1 << c for c in range(A) if r[c]) for r in mask])


def test_all_true_mask_is_the_oracle_loss():
    D, H, A, rows = 6, 8, 3, 32
    shapes = [(H, D), (H,), (H, H), (H,), (A, H), (A,), (H, D), (H,), (H, H), (H,), (1, H), (1,)]
    off, o = [], 0
    for s in shapes:
        off.append(o)
        o += int(np.prod(s))
    flat = np.random.default_rng(0).standard_normal(o) * 0.5
    mb, mask = am.loss_minibatch(D, A, rows, masked=False)
    assert mask.all() and (mb[:, D:D + A] > am.MASKED_LOGIT_MAX).all()
    kw = dict(kl_coeff=0.3, entropy_coeff=0.01, adv_mean=0.1, adv_inv_std=1.5)
    eg, est = oracle.ppo_loss_grad(flat, off, D, H, A, mb, **kw)
    g, st = am.ppo_loss_grad_masked(flat, off, D, H, A, mb, **kw)
    np.testing.assert_array_equal(g, eg)
    assert st == est
    # masked: finite, and no gradient reaches the always-masked action's output weights
    mb, mask = am.loss_minibatch(D, A, rows)
    g, st = am.ppo_loss_grad_masked(flat, off, D, H, A, mb, **kw)
    assert np.isfinite(g).all() and all(np.isfinite(v) for v in st.values())
    w3 = g[off[4]:off[4] + A * H].reshape(A, H)
    assert (w3[am.LOSS_ALWAYS_MASKED] == 0).all() and g[off[5] + am.LOSS_ALWAYS_MASKED] == 0 and np.abs(w3).max() > 0


@pytest.mark.parametrize("name,D,H,A,rows,prec", am.LOSS_CASES)
def test_loss_minibatches_are_masked_as_described(name, D, H, A, rows, prec):
    mb, mask = am.loss_minibatch(D, A, rows)
    lo = mb[:, D:D + A]
    assert np.array_equal(lo <= am.MASKED_LOGIT_MAX, ~mask)
    assert not mask[:, am.LOSS_ALWAYS_MASKED].any() and mask.any(1).all()
    act = mb[:, D + A + 3].astype(int)
    assert mask[np.arange(rows), act].all()
    assert len(np.unique(act)) == A - 1                       # every unmasked action is taken somewhere
    if A > 2:                                                 # rows differ in what they mask
        assert len(np.unique(am.mask_bits(mask))) >= 3
    assert np.isfinite(mb).all()


def test_fallback_counter_draws_one():
    """the committed counter's float32 draw is exactly 1.0: no cumulative entry can exceed u = 1.0 * sum"""
    x = oracle.philox([*am.FALLBACK_IDS, oracle.PURPOSE_ACTION << 16], [am.FALLBACK_SEED & 0xFFFFFFFF, am.FALLBACK_SEED >> 32])
    assert int(x[0]) >= 0xFFFFFF80
    u = oracle.u53(x[:1], x[1:2])
    assert u[0] < 1.0 and np.float32(u[0]) == np.float32(1.0)
    # the unmasked draw defaults to A - 1, the masked one to the highest unmasked index
    lg = np.zeros((1, 4), np.float32)
    ids = [np.array([v]) for v in am.FALLBACK_IDS]
    a, _ = oracle.sample_actions(lg, *ids, am.FALLBACK_SEED)
    assert a[0] == 3
    for mask, want in (([1, 1, 1, 0], 2), ([1, 0, 1, 0], 2), ([1, 1, 0, 0], 1), ([1, 1, 1, 1], 3)):
        _, a, _, _ = am.sample_masked(lg, np.array([mask], bool), *ids, am.FALLBACK_SEED)
        assert a[0] == want, mask


@pytest.mark.parametrize("name", am.MASK_CASES)
def test_mask_cases_fill_up(name):
    run = am.check_mask_guards(name)
    case = rr.CASES[name]
    assert len(run.masks) == case.steps and all(m.any(1).all() for m in run.masks)
    # the mask is what "myopic_with_room" decided under: its action always has room by the mask
    for m, a in zip(run.masks, run.actions):
        assert m[np.arange(case.n), a].all()


def test_roomy_case_never_fills():
    """along any run of the roomy spec every cluster keeps room: here under the worst policy for it, every
    pod of every step sent to cluster 0"""
    case = am.ROOMY
    spec = rr.spec_of(case)
    ora = rr.make_oracle(case)
    ora.reset()
    for _ in range(case.steps):
        assert am.room_mask(ora.node_state()[2], spec).all() and rr.has_room(ora.node_state()[2], spec).all()
        ora.step(np.zeros(case.n, np.int32))


def test_table_spec_has_room_everywhere():
    assert am.room_mask(np.zeros((5, 3), np.int32), rr.Spec(3)).all()
