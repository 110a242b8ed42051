"""numpy f64 restatement of the rollout-metrics record (rlks_rollout_metrics, include/rlks.h; DESIGN.md
§20), with the definitions and the widening of the kernel: every f32 input becomes f64 before any
operation, squares and the residual are formed in f64, sums are np.sum in f64, min / max are taken on
the f32 values.  Also the sum of absolute values behind every summed slot, which the tests' error bound
needs, and that bound itself."""
import numpy as np

from rlks import _lib as L


def reference(actions, rewards, values, vtarg, dones, obs, A, C):
    """-> (record, abs_record): double[RLKS_RM_FIXED + A + C] each; abs_record holds sum |x| where the
    record holds sum x (0 in the min / max slots).  Shapes: actions / rewards / vtarg / dones [T][N],
    values [T+1][N] (row T is not read), obs [T+1][N][D] (rows t < T, columns 2C .. 3C)."""
    T, N = rewards.shape
    assert rewards.dtype == values.dtype == vtarg.dtype == obs.dtype == np.float32 and dones.dtype == np.uint8
    r = rewards.astype(np.float64).ravel()
    v = values[:T].astype(np.float64).ravel()
    t = vtarg.astype(np.float64).ravel()
    res = t - v
    util = obs[:T, :, 2 * C:3 * C].astype(np.float64).reshape(T * N, C)
    counts = np.bincount(actions.ravel().astype(np.int64), minlength=A)[:A]
    rec = np.zeros(L.RLKS_RM_FIXED + A + C, np.float64)
    ab = np.zeros_like(rec)
    rec[L.RLKS_RM_ROWS] = ab[L.RLKS_RM_ROWS] = T * N
    rec[L.RLKS_RM_REWARD_MIN] = np.float64(rewards.min())
    rec[L.RLKS_RM_REWARD_MAX] = np.float64(rewards.max())
    rec[L.RLKS_RM_DONES] = ab[L.RLKS_RM_DONES] = np.count_nonzero(dones)
    for slot, x in ((L.RLKS_RM_REWARD_SUM, r), (L.RLKS_RM_VALUE_SUM, v), (L.RLKS_RM_VTARG_SUM, t),
                    (L.RLKS_RM_VTARG_SQ, t * t), (L.RLKS_RM_RESID_SUM, res), (L.RLKS_RM_RESID_SQ, res * res)):
        rec[slot] = np.sum(x)
        ab[slot] = np.sum(np.abs(x))
    rec[L.RLKS_RM_FIXED:L.RLKS_RM_FIXED + A] = ab[L.RLKS_RM_FIXED:L.RLKS_RM_FIXED + A] = counts
    rec[L.RLKS_RM_FIXED + A:] = util.sum(0)
    ab[L.RLKS_RM_FIXED + A:] = np.abs(util).sum(0)
    return rec, ab


EXACT = (L.RLKS_RM_ROWS, L.RLKS_RM_REWARD_MIN, L.RLKS_RM_REWARD_MAX, L.RLKS_RM_DONES)


def sum_bound(n, abs_sum):
    """|fl(sum) - sum| <= (n - 1) u sum|x| + O(u^2) for f64 summation in any order (u = 2^-53; Higham,
    Accuracy and Stability of Numerical Algorithms, §4.2), rounded up to n u sum|x| and doubled, since the
    reference's own np.sum carries the same error: 2 n 2^-53 sum|x|"""
    return 2.0 * n * 2.0 ** -53 * abs_sum


def check_record(got, ref, ab, A, what=""):
    """counts, ROWS, DONES, min and max bit-equal; each sum within sum_bound of the reference"""
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    assert got.shape == ref.shape, (got.shape, ref.shape)
    n = ref[L.RLKS_RM_ROWS]
    exact = list(EXACT) + list(range(L.RLKS_RM_FIXED, L.RLKS_RM_FIXED + A))
    for s in exact:
        assert got[s].tobytes() == ref[s].tobytes(), (what, "slot", s, got[s], ref[s])
    for s in range(len(ref)):
        if s in exact:
            continue
        err, tol = abs(got[s] - ref[s]), sum_bound(n, ab[s])
        assert err <= tol, (what, "slot", s, got[s], ref[s], err, tol)
