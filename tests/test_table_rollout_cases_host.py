"""CPU checks of the table-rollout cases (table_rollout_cases.py) that test_gpu_table_rollout.py runs on the
device: the LDS arithmetic and the form every case must resolve to, and that the weight regimes are what
their descriptions say (fp64 numpy and the oracle), so that a failure on the device is the kernels'."""
import numpy as np
import pytest

import oracle
import table_rollout_cases as tc

# The fused rollout kernels' own LDS (dynamic bytes without a table) and the table rows (C = A clouds) that
# still fit beside them under 160 KiB, as worked out by hand from the launchers' formulas.  The fp32 rows
# count 16 static bytes (k_fwd_head declares double sVx[2]); the compiler drops them from the rollout
# instantiations, which never read sVx, and with 0 static bytes only the 4-action 128-row count moves (567).
LDS_TABLE = [
    # form, A, own bytes, static, rows that fit, rows the env accepts
    (tc.SF16_PERSISTENT, 2, 75776, 0, 2752, 4096),
    (tc.SF16_PERSISTENT, 4, 81920, 0, 1280, 2048),
    (tc.SF16_PERSISTENT, 8, 96256, 0, 528, 1024),
    (tc.FP32_FUSED_32, 8, 110816, 16, 414, 1024),
    (tc.FP32_FUSED_128, 8, 152160, 16, 91, 1024),
    (tc.FP32_FUSED_128, 4, 127552, 16, 566, 2048),
    (tc.FP32_FUSED_128, 2, 115248, 16, 1518, 4096),
]


@pytest.mark.parametrize("form,A,own,static,fit,accepted", LDS_TABLE)
def test_lds_formulas_reproduce_the_budget_table(form, A, own, static, fit, accepted):
    assert tc.fused_lds(form, A, 0, A) == own
    assert tc.rows_that_fit(form, A, static) == fit
    assert tc.fused_lds(form, A, fit, A) + static <= tc.LDS_LIMIT < tc.fused_lds(form, A, fit + 1, A) + static
    assert accepted == tc.MAX_TABLE_BYTES // (2 * A * 8) and fit < accepted  # the env takes tables the kernel cannot


def test_lds_figures_of_the_budget_cases():
    assert tc.LDS_LIMIT == 163840
    assert tc.fwd_rollout_lds(8, 128, 100, 8) == 164960        # the standard 8-cloud table past 32,768 lanes
    assert tc.fwd_rollout_lds(8, 32, 100, 8) == 123616         # ... fits the 32-row form
    assert tc.sf_roll_lds(8, 600, 8) == 173056 and 2 * 600 * 8 * 8 == 76800
    assert tc.fwd_rollout_lds(8, 32, 450, 8) == 168416 and 2 * 450 * 8 * 8 == 57600
    assert tc.sf_roll_lds(2, 2752, 2) == tc.LDS_LIMIT          # exactly the limit
    assert tc.sf_roll_lds(8, 4, 8) == 96768                    # the largest launch the suite had before


@pytest.mark.parametrize("case", tc.ALL, ids=lambda c: c.id)
def test_cases_resolve_to_their_form(case):
    assert tc.resolve(case.prec, case.A, case.rows, case.lanes, case.job_lanes) == case.form
    assert 2 * case.rows * case.A * 8 <= tc.MAX_TABLE_BYTES  # rlks_env_create accepts the table
    if case.form in (tc.SF16_PERSISTENT, tc.FP32_FUSED_32, tc.FP32_FUSED_128):
        assert tc.fused_lds(case.form, case.A, case.rows, case.A) <= tc.LDS_LIMIT


def test_resolver_order_and_edges():
    from rlks import _lib

    assert [getattr(_lib, "RLKS_ROLLOUT_" + n) for n in ("SF16_PERSISTENT", "SF16_PER_STEP", "FP32_FUSED_32",
                                                         "FP32_FUSED_128", "FP32_PER_STEP", "WIDE", "NODE")] == \
        [tc.SF16_PERSISTENT, tc.SF16_PER_STEP, tc.FP32_FUSED_32, tc.FP32_FUSED_128, tc.FP32_PER_STEP, tc.WIDE, tc.NODE]
    # the shapes that ran before resolve as they ran: the replay test's rows, the agent test's, bench c2 / c4
    for A in (2, 8):
        assert tc.resolve("sf16", A, 4, 96) == tc.SF16_PERSISTENT
    assert tc.resolve("sf16", 4, 4, 96, tc.SF_ROLL_FUSED_MAX_LANES + 1) == tc.SF16_PER_STEP
    assert tc.resolve("fp32", 4, 4, 96) == tc.FP32_FUSED_32
    assert tc.resolve("sf16", 2, 100, 4096) == tc.SF16_PERSISTENT
    assert tc.resolve("sf16", 2, 100, 32768) == tc.SF16_PER_STEP
    assert tc.resolve("sf16", 2, 100, 131072) == tc.SF16_PER_STEP
    # the lane rule needs autoreset lanes, as it always did; the budget needs them too, or refuses
    assert tc.resolve("sf16", 2, 100, 32768, autoreset=False) == tc.SF16_PERSISTENT
    assert tc.resolve("sf16", 2, 2752, 72) == tc.SF16_PERSISTENT and tc.resolve("sf16", 2, 2753, 72) == tc.SF16_PER_STEP
    with pytest.raises(tc.Unsupported) as e:
        tc.resolve("sf16", 8, 600, 72, autoreset=False)
    assert e.value.args == (173056, 163840)
    with pytest.raises(tc.Unsupported):
        tc.resolve("fp32", 8, 450, 72, autoreset=False)
    # the kernels decide, not the desc: rlks_rollout runs the fp32 kernels under a split-fp16 desc too, and a
    # 450 x 8 table fits the persistent kernel (153,856 B) but not the fused fp32 step (168,416 B)
    assert tc.resolve("sf16", 8, 450, 72) == tc.SF16_PERSISTENT and tc.sf_roll_lds(8, 450, 8) == 153856
    assert tc.resolve("fp32", 8, 450, 72) == tc.FP32_PER_STEP
    # fp32: 128-row tiles past 32,768 lanes while they fit, else 32-row tiles, else per step
    assert tc.resolve("fp32", 8, 91, tc.N_BIG) == tc.FP32_FUSED_128
    assert tc.resolve("fp32", 8, 92, tc.N_BIG) == tc.FP32_FUSED_32
    assert tc.resolve("fp32", 8, 414, tc.N_BIG) == tc.FP32_FUSED_32
    assert tc.resolve("fp32", 8, 415, tc.N_BIG) == tc.FP32_PER_STEP
    assert tc.resolve("fp32", 2, 100, 32 * 1024) == tc.FP32_FUSED_32


@pytest.fixture(scope="module")
def forwards():
    """per (regime, A): the fp64 logits, values and hidden magnitudes on the observations a rollout visits"""
    out = {}
    for A in tc.ACTIONS:
        for regime in tc.REGIMES:
            flat, off = tc.fixture_flat(regime, A)
            obs = tc.observations(tc.table(regime, A), tc.N * (tc.T + 1))
            lg, v = oracle.mlp_forward(flat, off, 3 * A, tc.H, A, obs)
            out[regime, A] = (lg, v, tc.hidden_f64(flat, off, 3 * A, A, obs))
    return out


@pytest.mark.parametrize("A", tc.ACTIONS)
@pytest.mark.parametrize("regime", tc.REGIMES)
def test_few_outputs_lie_under_the_comparison_floor(forwards, regime, A):
    """close_as_fp32 leaves out elements under 1e-6 of the largest: at most 1% of them may be"""
    lg, v, _ = forwards[regime, A]
    for x in (lg, v):
        assert np.isfinite(x).all()
        assert (np.abs(x) <= 1e-6 * np.abs(x).max()).mean() <= 0.01
    if regime == "grown":  # the +3 / -3 logits lie far apart: a large negative logp (and at 2 actions one argmax)
        assert (lg.max(1) - lg.min(1)).min() > 5.0 and tc_logp_min(lg) < -5.0


def tc_logp_min(lg):
    z = lg - lg.max(1, keepdims=True)
    return (z - np.log(np.exp(z).sum(1, keepdims=True))).min()


@pytest.mark.parametrize("A", tc.ACTIONS)
@pytest.mark.parametrize("regime", tc.REGIMES)
def test_no_regime_shrinks_the_activations(forwards, regime, A):
    """the split kernels' tanh is 1e-7 absolute by design: every regime keeps median |h1| and |h2| of both nets
    at or above init's, so the relative bar of the device tests measures the kernels, not that choice"""
    base = forwards["init", A][2]
    for (h1, h2), (b1, b2) in zip(forwards[regime, A][2], base):
        assert np.median(h1) >= np.median(b1) and np.median(h2) >= np.median(b2)
        assert np.median(b1) > 0.05 and np.median(b2) > 0.05


@pytest.mark.parametrize("A", tc.ACTIONS)
def test_outlier_moves_both_exponents_by_six(A):
    D = 3 * A
    shp = tc.shapes(D, A)
    (f0, off), (f1, _) = tc.fixture_flat("init", A), tc.fixture_flat("outlier", A)
    (f2, _) = tc.fixture_flat("grown", A)
    for net in (0, 1):
        for j in (tc.W1, tc.W2):
            a, b, g = (np.abs(tc._t(f, off, shp, 6 * net + j)).max() for f in (f0, f1, f2))
            assert tc.sf_exp(b) - tc.sf_exp(a) == -6 and b == np.float32(64.0) * a
            assert tc.sf_exp(g) - tc.sf_exp(a) == -2
            assert (tc._t(f0, off, shp, 6 * net + j) != tc._t(f1, off, shp, 6 * net + j)).sum() == 1
        # k_sf_prep scales W1 together with b1 (W1a = [W1 | b1]): the exponent of that maximum moves alike
        wa = [max(np.abs(tc._t(f, off, shp, 6 * net + tc.W1)).max(), np.abs(tc._t(f, off, shp, 6 * net + tc.B1)).max())
              for f in (f0, f1)]
        assert tc.sf_exp(wa[1]) - tc.sf_exp(wa[0]) == -6


def test_raw_table_is_the_unscaled_synthetic_table():
    from rlks.tables import minmax_scale, synthetic_table

    for C in tc.ACTIONS:
        raw, ref = tc.raw_synthetic_table(C), synthetic_table(C, tc.ROWS, seed=tc.TABLE_SEED)
        np.testing.assert_array_equal(minmax_scale(raw.cost), ref.cost)
        np.testing.assert_array_equal(minmax_scale(raw.latency), ref.latency)
        assert 0.008 < raw.cost.min() and raw.cost.max() < 0.023 and 40 <= raw.latency.min() and raw.latency.max() <= 90
        # the per-tile observation exponent differs from the scaled table's, whose columns lie in [0, 1]
        assert tc.sf_exp(np.abs(tc.observations(raw, 32)).max()) < tc.sf_exp(np.abs(tc.observations(ref, 32)).max())
    big = tc.table("init", 2, 2753)
    np.testing.assert_array_equal(tc.head_rows(big, 2752).cost, big.cost[:2752])
