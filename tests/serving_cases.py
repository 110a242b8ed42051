"""Shared fixtures of the serving tests (test_serving_host.py, test_gpu_serving.py): the policies, their
adjusted weights, the observations and the near-tie rule.  Plain data and numpy; fixture_flat() builds the
stock initialisation through rlks.policy on the CPU.

Policies: PolicyParams(D, 256, A) for (6, 2), (24, 8) and (9, 3): in the last, D is no multiple of 4 and A is
odd and none of 2 / 4 / 8.  adjust() multiplies both heads' weights by 100, so that logit gaps are O(1) (a
fresh init has 0.01-norm head rows and near-ties everywhere), and sets every bias to a seeded N(0, 0.1)
draw: init leaves the biases zero, and a kernel that dropped one would pass otherwise.
"""
import numpy as np

H = 256
POLICIES = [(6, 2), (24, 8), (9, 3)]
ROWS = (1, 15, 16, 17, 33)  # below, at and above a 16-row tile, and a ragged third tile
PARAM_SEED = 11
BIAS_SEED = 20250
OBS_SEED = 5
HEAD_SCALE = 100.0
AGREE_ROWS = 1024      # test 7: rows compared with compute_actions
AGREE_GAP_FACTOR = 8.0  # a row may be left out when its f64 top-two gap < 8 x its largest band deviation
AGREE_MAX_LEFT_OUT = 0.01

W_HEADS = (4, 10)                 # pi.w3, vf.w3 (flat tensor indices, include/rlks.h)
BIASES = (1, 3, 5, 7, 9, 11)


def shapes(D, A):
    return [(H, D), (H,), (H, H), (H,), (A, H), (A,), (H, D), (H,), (H, H), (H,), (1, H), (1,)]


def adjust(flat, offsets, D, A, seed=BIAS_SEED):
    """a copy of the flat float32 parameters with the heads scaled and the biases drawn"""
    out = np.array(flat, dtype=np.float32, copy=True)
    shp = shapes(D, A)
    rng = np.random.default_rng(seed + 1000 * D + A)
    for i in W_HEADS:
        n = int(np.prod(shp[i]))
        out[offsets[i]: offsets[i] + n] *= np.float32(HEAD_SCALE)
    for i in BIASES:
        n = int(np.prod(shp[i]))
        out[offsets[i]: offsets[i] + n] = (0.1 * rng.standard_normal(n)).astype(np.float32)
    return out


def fixture_flat(D, A):
    """(flat float32 [padded], offsets): PolicyParams(D, 256, A, seed=PARAM_SEED) on the CPU, adjusted"""
    from rlks.policy import PolicyParams

    p = PolicyParams(D, H, A, device=None, seed=PARAM_SEED)
    return adjust(p.flat.numpy(), p.offsets, D, A), list(p.offsets)


def observations(n, D, seed=OBS_SEED):
    """seeded, uniform in [0, 1)"""
    return np.random.default_rng(seed + 7 * D).random((n, D)).astype(np.float32)


def random_masks(n, A, seed=3):
    """bool [n, A], about half the bits set, every row with at least one"""
    rng = np.random.default_rng(seed)
    m = rng.random((n, A)) < 0.5
    m[np.arange(n), rng.integers(0, A, n)] = True
    return m


def softmax(logits, dtype):
    lo = np.asarray(logits, dtype)
    e = np.exp(lo - lo.max(-1, keepdims=True))
    return e / e.sum(-1, keepdims=True)


def near_ties(logits64, band):
    """bool [n]: rows whose f64 top-two logit gap is below AGREE_GAP_FACTOR x the row's largest
    band-vs-f64 deviation (two fp32 evaluations may order such a row's best two either way)"""
    l64 = np.asarray(logits64, np.float64)
    top = np.sort(l64, axis=1)
    gap = top[:, -1] - top[:, -2]
    dev = np.max([np.abs(np.asarray(b, np.float64) - l64).max(1) for b in band], axis=0)
    return gap < AGREE_GAP_FACTOR * dev
