"""Shared cases of the table-env rollout tests (test_table_rollout_cases_host.py, test_gpu_table_rollout.py):
the weight regimes and their tables, the LDS arithmetic of the fused rollout kernels restated in Python, the
form each case must resolve to, and the case lists.  Plain data and numpy; nothing here needs a GPU.

Regimes (each rewrites the flat parameters of both nets, and names a table):
  init       PolicyParams' initialisation with every bias drawn N(0, 0.1) (init leaves them zero, and a kernel
             that dropped one would pass otherwise), on synthetic_table(C, rows, seed=7).
  grown      init with W1, b1, W2 and W3 of both nets times 4 and the policy head's b3 alternating +3 / -3: the
             hidden units saturate, both tensor exponents of the split move by 2, and the logits lie 6 apart, so
             logp is large and negative (and at 2 actions the argmax is unambiguous).
  outlier    init with one element of W1 and one of W2 in each net set to 64 x that tensor's max |w|: both
             exponents drop by exactly 6 and the rest of the tensor sits six binades lower in the split.
  raw_table  init weights on the same synthetic table before minmax_scale: costs ~ 1e-2, latencies ~ 40-90, so
             the per-tile observation scale changes and the columns lie four decades apart.
No regime shrinks the activations: the split kernels' tanh is 1e-7 absolute by design (sgd_sf16.hip), and a
regime with tiny activations would measure that choice, not a defect (the host test holds every regime to it).
"""
from dataclasses import dataclass

import numpy as np

H = 256
BK = 32                      # mlp_common.h: the k-chunk of k_fwd_head
LDS_LIMIT = 160 * 1024       # env_device.h MAX_LDS_BYTES
MAX_TABLE_BYTES = 128 * 1024
SF_ROLL_FUSED_MAX_LANES = 16384   # workspace.h
FWD_SMALL_MAX_ROWS = 32 * 1024    # mlp_common.h

# include/rlks_types.h RLKS_ROLLOUT_*
SF16_PERSISTENT, SF16_PER_STEP, FP32_FUSED_32, FP32_FUSED_128, FP32_PER_STEP, WIDE, NODE = range(7)
FORM_NAMES = {SF16_PERSISTENT: "sf16-persistent", SF16_PER_STEP: "sf16-per-step", FP32_FUSED_32: "fp32-fused-32",
              FP32_FUSED_128: "fp32-fused-128", FP32_PER_STEP: "fp32-per-step", WIDE: "wide", NODE: "node"}

REGIMES = ("init", "grown", "outlier", "raw_table")
ACTIONS = (2, 4, 8)
N, T, ROWS = 72, 8, 100      # two full 32-row tiles and one with 8 valid rows
N_BIG = 32 * 1024 + 8        # past the fp32 tile switch, ragged last tile
T_BIG = 2
SEED = 5                     # env and parameter seed
BIAS_SEED = 20260
TABLE_SEED = 7
GROW = 4.0
OUTLIER = 64.0
# where the outliers go in W1 and W2.  One hidden unit saturates and the medians of |h1| and |h2| move by a
# few parts in a thousand either way with the place; at this one they stay at or above init's for both nets
# at 2, 4 and 8 actions (at [3, 1] / [5, 7] the value net's median |h2| came out 0.5% and 0.2% under it at 4 and
# 8 actions, which the host test's activation condition does not allow)
OUTLIER_AT = ((100, 2), (200, 100))
W1, B1, W2, B2, W3, B3 = range(6)   # tensor j of net n is flat tensor 6 n + j (include/rlks.h)
BIASES = (1, 3, 5, 7, 9, 11)


class Unsupported(Exception):
    """no form fits: (bytes asked, limit)"""


# ----------------------------------------------------------------------------- LDS arithmetic
def sf_roll_lds(A, rows, clouds):
    """dynamic LDS of k_sf_roll<A, KD> (rollout_sf16.hip roll_lds_bytes): sH, sPart, sBW, sObs, both tables"""
    kd = 16 if 3 * A + 1 <= 16 else 32
    return 2 * 8 * 2 * 2 * 64 * 16 + 2 * 4 * A * 32 * 4 + 2 * (1 + A) * H * 4 + 32 * kd * 4 + 2 * rows * clouds * 8


def fwd_rollout_lds(A, tile_rows, rows, clouds):
    """dynamic LDS of k_fwd_head<A, 0, WM, WN, FWD_ROLLOUT, 3A> (mlp_fwd.hip fwd_lds_bytes): 32-row tiles are
    WM, WN = 1, 4 and 128-row tiles 4, 2"""
    wm, wn = {32: (1, 4), 128: (4, 2)}[tile_rows]
    bm, d = 32 * wm, 3 * A
    f = (2 * H * (BK + 1) + 2 * BK * bm + wn * bm * A + bm * A + 2 * (A + 4) + H + bm * (d + 1)
         + ((H * (d + 1) + 1) & ~1))
    return 4 * f + 8 * 2 * rows * clouds


def fused_lds(form, A, rows, clouds):
    if form == SF16_PERSISTENT:
        return sf_roll_lds(A, rows, clouds)
    return fwd_rollout_lds(A, {FP32_FUSED_32: 32, FP32_FUSED_128: 128}[form], rows, clouds)


def rows_that_fit(form, A, static=0):
    """the most table rows (C = A clouds) with which the fused kernel of `form` stays within LDS_LIMIT"""
    left = LDS_LIMIT - static - fused_lds(form, A, 0, A)
    return left // (2 * A * 8)


def resolve(precision, A, rows, lanes, job_lanes=None, autoreset=True, static=0):
    """rollout.hip rollout_form for a table env with C = A clouds.  `static`: the fused kernels' static LDS
    bytes (the device reports 0 for all of them)"""
    if precision == "sf16":
        job = job_lanes if job_lanes else lanes
        if job > SF_ROLL_FUSED_MAX_LANES and autoreset:
            return SF16_PER_STEP
        need = static + sf_roll_lds(A, rows, A)
        if need <= LDS_LIMIT:
            return SF16_PERSISTENT
        per_step = SF16_PER_STEP
    else:
        if lanes > FWD_SMALL_MAX_ROWS:
            need = static + fwd_rollout_lds(A, 128, rows, A)
            if need <= LDS_LIMIT:
                return FP32_FUSED_128
        need = static + fwd_rollout_lds(A, 32, rows, A)
        if need <= LDS_LIMIT:
            return FP32_FUSED_32
        per_step = FP32_PER_STEP
    if autoreset:
        return per_step
    raise Unsupported(need, LDS_LIMIT)


# ----------------------------------------------------------------------------- tables
def raw_synthetic_table(n_clouds, n_rows=ROWS, seed=TABLE_SEED):
    """rlks.tables.synthetic_table's recipe (the same draws in the same order) without the min-max scaling: the
    table a run gets whose data skipped normalize_data.py"""
    from rlks.tables import Table

    rng = np.random.RandomState(seed)
    if n_clouds == 2:
        cbase, lbase = np.array([0.0104, 0.0208]), np.array([70.0, 60.0])
    else:
        cbase = rng.uniform(0.009, 0.022, n_clouds)
        lbase = rng.uniform(50.0, 80.0, n_clouds)
    cost = np.stack([cbase[c] + rng.uniform(-0.001, 0.001, n_rows) for c in range(n_clouds)], axis=1)
    lat = np.stack([lbase[c] + rng.uniform(-10, 10, n_rows) for c in range(n_clouds)], axis=1)
    names = [f"c{c}" for c in range(n_clouds)]
    cols = ["step"] + [f"cost_{n}" for n in names] + [f"latency_{n}" for n in names]
    raw = np.concatenate([np.arange(n_rows, dtype=np.float64)[:, None], cost, lat], axis=1)
    return Table(np.ascontiguousarray(cost), np.ascontiguousarray(lat), cols, raw, f"raw synthetic(C={n_clouds})")


def table(regime, n_clouds, n_rows=ROWS):
    from rlks.tables import synthetic_table

    if regime == "raw_table":
        return raw_synthetic_table(n_clouds, n_rows)
    return synthetic_table(n_clouds, n_rows, seed=TABLE_SEED)


def head_rows(tab, n_rows):
    """the first n_rows rows of a table: the rows a rollout from reset visits are then the same"""
    from rlks.tables import Table

    return Table(np.ascontiguousarray(tab.cost[:n_rows]), np.ascontiguousarray(tab.latency[:n_rows]), tab.columns,
                 tab.raw[:n_rows], tab.source + f"[:{n_rows}]")


# ----------------------------------------------------------------------------- regimes
def shapes(D, A):
    return [(H, D), (H,), (H, H), (H,), (A, H), (A,), (H, D), (H,), (H, H), (H,), (1, H), (1,)]


def _t(flat, offsets, shp, i):
    """view of flat tensor i"""
    n = int(np.prod(shp[i]))
    return flat[offsets[i]: offsets[i] + n].reshape(shp[i])


def regime_flat(regime, flat, offsets, D, A):
    """a float32 copy of the freshly initialised flat parameters rewritten for `regime`"""
    out = np.array(flat, dtype=np.float32, copy=True)
    shp = shapes(D, A)
    rng = np.random.default_rng(BIAS_SEED + 1000 * D + A)
    for i in BIASES:
        _t(out, offsets, shp, i)[...] = (0.1 * rng.standard_normal(shp[i])).astype(np.float32)
    if regime == "grown":
        for net in (0, 1):
            for j in (W1, B1, W2, W3):
                _t(out, offsets, shp, 6 * net + j)[...] *= np.float32(GROW)
        _t(out, offsets, shp, B3)[...] = np.where(np.arange(A) % 2 == 0, 3.0, -3.0).astype(np.float32)
    elif regime == "outlier":
        for net in (0, 1):
            for j, at in ((W1, OUTLIER_AT[0]), (W2, OUTLIER_AT[1])):
                w = _t(out, offsets, shp, 6 * net + j)
                w[at] = np.float32(OUTLIER) * np.abs(w).max()
    elif regime not in ("init", "raw_table"):
        raise ValueError(regime)
    return out


def apply_regime(params, regime):
    """overwrite a PolicyParams' views (both nets) for `regime`; expects the constructor's weights"""
    import torch

    flat = regime_flat(regime, params.flat.cpu().numpy(), params.offsets, params.D, params.A)
    params.flat.copy_(torch.from_numpy(flat).to(params.flat.device))


def fixture_flat(regime, A):
    """(flat float32 [padded], offsets) of PolicyParams(3A, 256, A, seed=SEED) on the CPU in `regime`"""
    from rlks.policy import PolicyParams

    p = PolicyParams(3 * A, H, A, device=None, seed=SEED)
    return regime_flat(regime, p.flat.numpy(), p.offsets, 3 * A, A), list(p.offsets)


def sf_exp(mx):
    """sf_exp.h: the power-of-two exponent that brings max |x| under the fp16 range"""
    mx = np.float32(mx)
    if not (mx > 0) or not (mx <= np.float32(3.4e38)):
        return 0
    return int(min(max(15 - int(np.frexp(mx)[1]), -120), 120))


def observations(tab, n_rows, seed=SEED):
    """[n_rows x ...] observations a rollout from reset visits: table rows in order beside utilisations drawn
    U(0.1, 0.8) (the env's own draw is Philox; the distribution is what matters to the host conditions)"""
    C = tab.n_clouds
    rng = np.random.default_rng(seed)
    t = np.arange(n_rows) % tab.n_rows
    return np.concatenate([tab.cost[t], tab.latency[t], rng.uniform(0.1, 0.8, (n_rows, C))], axis=1).astype(np.float32)


def hidden_f64(flat, offsets, D, A, obs):
    """fp64 |h1| and |h2| of both nets: [(h1, h2) pi, (h1, h2) vf]"""
    shp = shapes(D, A)
    f = np.asarray(flat, np.float64)
    x = np.asarray(obs, np.float64)
    out = []
    for net in (0, 1):
        w1, b1, w2, b2 = (_t(f, offsets, shp, 6 * net + j) for j in (W1, B1, W2, B2))
        h1 = np.tanh(x @ w1.T + b1)
        out.append((np.abs(h1), np.abs(np.tanh(h1 @ w2.T + b2))))
    return out


# ----------------------------------------------------------------------------- cases
@dataclass(frozen=True)
class Case:
    id: str
    prec: str            # "sf16" / "fp32"
    A: int
    regime: str
    form: int            # the form rlks_rollout_form must name
    rows: int = ROWS
    lanes: int = N
    steps: int = T
    per_step: bool = False   # bufs.global_lanes = SF_ROLL_FUSED_MAX_LANES + 1
    explore: bool = True

    @property
    def job_lanes(self):
        return SF_ROLL_FUSED_MAX_LANES + 1 if self.per_step else self.lanes


_FORMS = (("persistent", "sf16", False, SF16_PERSISTENT), ("per-step", "sf16", True, SF16_PER_STEP),
          ("fp32", "fp32", False, FP32_FUSED_32))

# every regime x every small form x A
PARITY = [Case(f"{name}-{A}-{regime}", prec, A, regime, form, per_step=ps)
          for name, prec, ps, form in _FORMS for A in ACTIONS for regime in REGIMES]
# one grown case per form with the argmax draw
ARGMAX = [Case(f"{name}-4-grown-argmax", prec, 4, "grown", form, per_step=ps, explore=False)
          for name, prec, ps, form in _FORMS]
# the fp32 128-row tiles, and the A = 8 shape whose 128-row form is over budget (164,960 B)
BIG = ([Case(f"fp32-128-{A}-{regime}", "fp32", A, regime, FP32_FUSED_128, lanes=N_BIG, steps=T_BIG)
        for A in (2, 4) for regime in ("init", "grown")]
       + [Case(f"fp32-budget-32-8-{regime}", "fp32", 8, regime, FP32_FUSED_32, lanes=N_BIG, steps=T_BIG)
          for regime in ("init", "grown")])
BIG_HEAD, BIG_TAIL = 4096, 136   # lanes of a big case whose logits and values are compared
# tables too large for the fused form at 72 lanes
BUDGET = [Case("sf16-budget-per-step-8", "sf16", 8, "init", SF16_PER_STEP, rows=600),
          Case("fp32-budget-per-step-8", "fp32", 8, "init", FP32_PER_STEP, rows=450)]
ALL = PARITY + ARGMAX + BIG + BUDGET
