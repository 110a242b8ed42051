"""CPU tests of the clipping reference (tests/clip_ref.py) against torch.nn.utils.clip_grad_norm_, of
the config validation of grad_clip / grad_clip_by and of the lr / entropy-coefficient schedules
(rlks.schedules: no device code)."""
import numpy as np
import pytest

import clip_ref

torch = pytest.importorskip("torch")

D, H, A = 6, 256, 2
SHAPES = [(H, D), (H,), (H, H), (H,), (A, H), (A,), (H, D), (H,), (H, H), (H,), (1, H), (1,)]


def _flat(seed):
    """a padded flat gradient shaped like the 12 parameter tensors (64-float aligned, as
    rlks_mlp_layout) with junk in the padding, and its true-element mask"""
    rng = np.random.default_rng(seed)
    off, o = [], 0
    for s in SHAPES:
        off.append(o)
        o += -(-int(np.prod(s)) // 64) * 64
    g = np.full(o, 1e30, np.float32)
    for of, s in zip(off, SHAPES):
        n = int(np.prod(s))
        g[of: of + n] = (rng.standard_normal(n) * 10.0 ** rng.uniform(-3, 1)).astype(np.float32)
    return g, off, clip_ref.real_mask(off, SHAPES, o)


def _ulp_diff(a, b):
    ia = a.view(np.int32).astype(np.int64)
    ib = b.view(np.int32).astype(np.int64)
    return np.abs(np.where(ia < 0, -(ia & 0x7FFFFFFF), ia) - np.where(ib < 0, -(ib & 0x7FFFFFFF), ib))


@pytest.mark.parametrize("case", ["far_above", "far_below", "equal"])
def test_reference_matches_torch_clip_grad_norm(case):
    g, off, mask = _flat(7)
    norm = clip_ref.global_norm(g, mask)
    clip = {"far_above": norm / 37.0, "far_below": norm * 37.0, "equal": norm}[case]
    clip = float(np.float32(clip))
    ts = [torch.zeros(s, requires_grad=True) for s in SHAPES]
    for t, of, s in zip(ts, off, SHAPES):
        t.grad = torch.from_numpy(g[of: of + int(np.prod(s))].reshape(s).copy())
    total = torch.nn.utils.clip_grad_norm_(ts, clip)
    out, n, coef = clip_ref.clipped(g, clip, mask)
    print(f"{case}: norm {n!r} torch {float(total)!r} coef {coef!r}")
    assert abs(n - float(total)) <= 1e-6 * n  # torch sums in float32
    # (at the threshold clip / (norm + 1e-6) is within a float32 ulp of 1: coef is 1 or just below)
    assert coef < 1 if case == "far_above" else coef == 1 if case == "far_below" else 1 - 1e-6 < coef <= 1
    got = np.concatenate([t.grad.numpy().ravel() for t in ts])
    worst = int(_ulp_diff(out[mask], got).max())
    print(f"{case}: max ulp difference {worst}")
    assert worst <= 1
    assert np.array_equal(out[~mask], g[~mask])  # padding is neither counted nor scaled
    if case == "far_below":
        assert coef == 1 and np.array_equal(out, g)


def test_clip_coef_arithmetic():
    assert clip_ref.clip_coef(10.0, 40.0) == np.float32(1.0)
    assert clip_ref.clip_coef(80.0, 40.0) == np.float32(40.0 / (80.0 + 1e-6))
    assert clip_ref.clip_coef(0.0, 1e-3) == np.float32(1.0)  # a zero gradient is not scaled up
    # grad_clip is a float32 argument of the library
    assert clip_ref.clip_coef(1.0, 0.1) == np.float32(float(np.float32(0.1)) / (1.0 + 1e-6))


def test_config_validation():
    from rlks.ppo import PPO, PPOConfig
    from rlks.schedules import validate_grad_clip

    assert validate_grad_clip(None) is None and validate_grad_clip(40) == 40.0
    assert validate_grad_clip(0.5, "global_norm") == 0.5
    for bad in (0, -1.0, float("inf"), float("nan"), "40", True):
        with pytest.raises(ValueError):
            validate_grad_clip(bad)
    for by in ("value", "norm"):
        with pytest.raises(ValueError, match="global_norm"):
            validate_grad_clip(40.0, by)
        with pytest.raises(ValueError, match="global_norm"):
            validate_grad_clip(None, by)
    # the agent refuses them at construction, before it touches a device
    for kw in (dict(grad_clip=0.0), dict(grad_clip=float("nan")), dict(grad_clip=-3),
               dict(grad_clip=40.0, grad_clip_by="value"), dict(grad_clip_by="norm"), dict(lr_schedule=[[1, 3e-4]]),
               dict(entropy_coeff_schedule=[[0, 0.01], [0, 0.0]])):
        with pytest.raises(ValueError):
            PPO(config=PPOConfig().training(**kw), device="cpu")
    # the knobs are part of the saved config, unknown training() keys are still accepted
    c = PPOConfig().training(grad_clip=40.0, grad_clip_by="global_norm", lr_schedule=[[0, 3e-4], [1000, 1e-4]],
                             some_future_knob=1)
    d = c.to_dict()
    assert d["grad_clip"] == 40.0 and d["lr_schedule"] == [[0, 3e-4], [1000, 1e-4]]
    c2 = PPOConfig.from_dict(d)
    assert c2.grad_clip == 40.0 and c2.grad_clip_by == "global_norm" and c2.lr_schedule == [[0, 3e-4], [1000, 1e-4]]
    assert PPOConfig().grad_clip is None and PPOConfig().lr_schedule is None


def test_schedule_at_between_and_beyond_its_points():
    from rlks.schedules import schedule_value

    s = [[0, 3e-4], [1000, 1e-4], [3000, 0.0]]
    assert schedule_value(s, 0) == 3e-4
    assert schedule_value(s, 1000) == 1e-4
    assert schedule_value(s, 3000) == 0.0
    assert schedule_value(s, 500) == pytest.approx(2e-4, rel=1e-12)
    assert schedule_value(s, 250) == pytest.approx(2.5e-4, rel=1e-12)
    assert schedule_value(s, 2000) == pytest.approx(5e-5, rel=1e-12)
    assert schedule_value(s, 999) > schedule_value(s, 1000) > schedule_value(s, 1001)
    assert schedule_value(s, 3001) == 0.0 and schedule_value(s, 10**12) == 0.0
    assert schedule_value([[0, 0.01]], 0) == 0.01 and schedule_value([[0, 0.01]], 12345) == 0.01
    assert schedule_value([(0, 1.0), (4, 3.0)], 1) == 1.5  # tuples are fine


@pytest.mark.parametrize("bad", [[], None, 3e-4, [[1, 3e-4]], [[0, 3e-4], [0, 1e-4]], [[0, 3e-4], [500, 1e-4], [400, 0.0]],
                                 [[0, 3e-4, 1]], [[0]], [[0, "x"]], [[0, float("nan")]], [[-1, 1.0]], [[0, 1.0], [2.5, 0.0]],
                                 [0, 3e-4]])
def test_malformed_schedules(bad):
    from rlks.schedules import schedule_value, validate_schedule

    with pytest.raises(ValueError):
        validate_schedule(bad, "lr_schedule")
    with pytest.raises(ValueError):
        schedule_value(bad, 0)
