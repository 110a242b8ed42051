"""Host tests of observation_filter (no device): the config knob's validation and round trip, the numpy
restatement (tests/obs_filter_ref.py) against two-pass figures, and two sensitivity checks that keep its
bounds honest: an f32 accumulation breaks the record bound, an unshifted sum x^2 breaks the m2 bound."""
import numpy as np
import pytest

import obs_filter_ref as R


def test_config_accepts_the_two_filters_and_round_trips():
    from rlks.ppo import PPOConfig

    assert PPOConfig().observation_filter == "NoFilter"
    for name in ("NoFilter", "MeanStdFilter"):
        for method in ("rollouts", "env_runners"):
            cfg = getattr(PPOConfig(), method)(observation_filter=name)
            assert cfg.observation_filter == name
            d = cfg.to_dict()
            assert d["observation_filter"] == name
            assert PPOConfig.from_dict(d).observation_filter == name


@pytest.mark.parametrize("bad", ["ConcurrentMeanStdFilter", "meanstdfilter", "", None, 1, lambda shape: None])
def test_unknown_filter_raises(bad):
    """an RLlib config with a filter this package does not have must not train unfiltered in silence"""
    from rlks.ppo import PPOConfig

    with pytest.raises(ValueError):
        PPOConfig().rollouts(observation_filter=bad)
    with pytest.raises(ValueError):
        PPOConfig().env_runners(observation_filter=bad)
    cfg = PPOConfig()
    cfg.observation_filter = "NoFilter"
    assert cfg.rollouts(num_rollout_workers=2).observation_filter == "NoFilter"  # other keywords as before


def test_algorithm_validates_a_config_that_came_through_from_dict():
    """from_dict sets attributes without rollouts(): PPO.__init__ checks again, before it touches a device"""
    from rlks.ppo import PPO, PPOConfig

    d = PPOConfig().to_dict()
    d["observation_filter"] = "ConcurrentMeanStdFilter"
    cfg = PPOConfig.from_dict(d)
    with pytest.raises(ValueError, match="observation_filter"):
        PPO(config=cfg, device="cpu")


def test_fresh_state_is_the_identity():
    x = R.case_data(255, 6, seed=1)
    x[3, 2] = -0.0
    y = R.apply(R.fresh(6), x)
    assert y.tobytes() == x.tobytes()


def test_three_batches_merge_to_the_two_pass_figures():
    batches = [R.case_data(r, 24, seed=s) for r, s in ((1, 2), (1000, 3), (257, 4))]
    batches = [b[:, :23] for b in batches]  # (without the constant column: see the next test)
    st, tm, t2 = R.chain(batches)
    R.check_whole_state(st, 1258, batches, "three batches")
    # and the figures themselves, not only their bound: 1e-12 relative is far inside f64 for O(1) data
    allx = np.concatenate(batches).astype(np.float64)
    assert np.allclose(st[1], allx.mean(0), rtol=1e-12, atol=0)
    assert np.allclose(st[2] / (st[0] - 1), allx.var(0, ddof=1), rtol=1e-12, atol=0)
    y = R.apply(st, batches[1])
    z = (batches[1].astype(np.float64) - allx.mean(0)) / (allx.std(0, ddof=1) + 1e-8)
    assert np.abs(y - z).max() <= 4 * 2.0 ** -24 * np.abs(z).max()


def test_constant_column_never_gets_a_negative_m2():
    batches = [R.case_data(r, 6, seed=s) for r, s in ((255, 5), (4097, 6))]
    st, _, _ = R.chain(batches)
    assert (st[2] >= 0).all() and np.isfinite(st[3]).all()
    assert st[1][5] == 0.375 and st[2][5] <= 1e-20
    R.check_whole_state(st, 255 + 4097, batches, "constant column")


def test_merge_of_an_empty_record_is_a_no_op():
    st, _, _ = R.chain([R.case_data(100, 6, seed=7)])
    st2 = R.merge(st, (0.0, np.zeros(6), np.zeros(6)))
    assert R.pack(st2).tobytes() == R.pack(st).tobytes()


def test_f32_accumulation_violates_the_record_bound():
    """sensitivity: the record bound is tight enough to tell an f32 accumulator from an f64 one"""
    rows, D = R.CASES["odd_4097"]
    x = R.case_data(rows, D, seed=8)
    K = np.zeros(D)
    _, s1, s2, ab1, ab2 = R.record(x, K)
    d32 = x - K.astype(np.float32)[None]
    s1_32 = np.zeros(D, np.float32)
    s2_32 = np.zeros(D, np.float32)
    for r in range(rows):  # a running f32 sum, as a kernel with float accumulators would form it
        s1_32 += d32[r]
        s2_32 += d32[r] * d32[r]
    assert (np.abs(s1_32.astype(np.float64) - s1) > R.record_bound(rows, ab1))[:D - 1].all()
    assert (np.abs(s2_32.astype(np.float64) - s2) > R.record_bound(rows, ab2))[:D - 1].all()


def test_unshifted_sum_of_squares_violates_the_m2_bound():
    """sensitivity: on the offset column (1000 + 1e-3 noise, K ~ 1000) the textbook m2 = sum x^2 - n mean^2
    loses every digit the m2 bound asks for"""
    rows, D = R.CASES["offset"]
    first = R.case_data(rows, D, seed=9, offset=True)
    x = R.case_data(rows, D, seed=10, offset=True)
    st, _, _ = R.chain([first])
    assert abs(st[1][0] - 1000.0) < 1e-3
    rec = R.record(x, st[1])[:3]
    _, tol_m2 = R.merge_bounds(st, rec)
    good = R.merge(st, rec)
    # the same merge in extended precision from the same record: inside the bound
    L = np.longdouble
    na, nb = L(st[0]), L(rec[0])
    s1, s2 = rec[1].astype(L), rec[2].astype(L)
    ext = st[2].astype(L) + (s2 - s1 * (s1 / nb)) + (s1 / nb) ** 2 * (na * nb / (na + nb))
    assert abs(float(ext[0]) - good[2][0]) <= tol_m2[0]
    # the unshifted form of the batch's part: sum x^2 - nb mean_b^2, then the same combination
    xb = x.astype(np.float64)
    sx, sxx = xb.sum(0), (xb * xb).sum(0)
    mean_b = sx / rec[0]
    delta = mean_b - st[1]
    naive = (st[2] + (sxx - rec[0] * mean_b * mean_b)) + (delta * delta) * ((st[0] * rec[0]) / (st[0] + rec[0]))
    assert abs(naive[0] - good[2][0]) > 100 * tol_m2[0], (naive[0], good[2][0], tol_m2[0])
    # (on an O(1) column the two forms agree to the bound's order: the offset is what separates them)
    assert abs(naive[1] - good[2][1]) <= 100 * tol_m2[1]
