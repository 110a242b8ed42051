"""numpy f64 restatement of the observation filter (rlks_obs_filter_*, include/rlks.h):
the batch record, Chan's merge and the filtered value, each operation rounded on its own as the device
forms it, and the error bounds the tests hold the device to.  u = 2^-53 throughout.

State: (count, mean[D], m2[D], inv[D]).  Record: (rows, s1[D], s2[D]) with s1 = sum (x - K), s2 =
sum (x - K)^2 and K = the state's mean.
"""
import numpy as np

from rollout_metrics_ref import sum_bound

U = 2.0 ** -53


def fresh(D):
    return 0.0, np.zeros(D), np.zeros(D), np.ones(D)


def pack(state):
    """the device layout double[1 + 3 D]"""
    n, mean, m2, inv = state
    return np.concatenate([[n], mean, m2, inv]).astype(np.float64)


def unpack(s):
    s = np.asarray(s, np.float64)
    D = (len(s) - 1) // 3
    return float(s[0]), s[1:1 + D].copy(), s[1 + D:1 + 2 * D].copy(), s[1 + 2 * D:].copy()


def record(x, K):
    """-> (rows, s1, s2, ab1, ab2): the record of x [rows][D] (float32) about the shift K [D], and the
    sums of the absolute terms behind s1 and s2 (the record bound's argument; s2's terms are their own
    absolute values).  The terms d = fl(x - K) and fl(d d) are what the device forms, bit for bit: only
    the order of the additions differs."""
    assert x.dtype == np.float32 and x.ndim == 2
    d = x.astype(np.float64) - np.asarray(K, np.float64)[None]
    sq = d * d
    return float(x.shape[0]), d.sum(0), sq.sum(0), np.abs(d).sum(0), sq.sum(0)


def record_bound(rows, ab):
    """Record: every slot is an f64 sum of `rows` terms that both sides form identically, so the two
    differ by their summation orders alone: |fl(sum) - sum| <= (rows - 1) u sum|term| for any order
    (Higham, Accuracy and Stability of Numerical Algorithms, §4.2), once for each side:
    rollout_metrics_ref.sum_bound(rows, sum|term|) = 2 rows u sum|term|."""
    return sum_bound(rows, np.asarray(ab, np.float64))


def inv_of(n, m2):
    m2 = np.asarray(m2, np.float64)
    return 1.0 / (np.sqrt(m2 / (n - 1.0)) + 1e-8) if n >= 2 else np.ones_like(m2)


def merge(state, rec):
    """Chan's update, the operations in the order of include/rlks.h; rows == 0 leaves the state as it is"""
    na, mean, m2, inv = state
    nb, s1, s2 = rec[0], np.asarray(rec[1], np.float64), np.asarray(rec[2], np.float64)
    if not nb > 0:
        return na, mean.copy(), m2.copy(), inv.copy()
    n = na + nb
    delta = s1 / nb
    mean_n = mean + delta * (nb / n)
    m2_n = (m2 + (s2 - s1 * delta)) + (delta * delta) * ((na * nb) / n)
    m2_n = np.where(m2_n > 0.0, m2_n, 0.0)
    return n, mean_n, m2_n, inv_of(n, m2_n)


def merge_bounds(state, rec):
    """Merge, given the same record on both sides (the device's own) -> (tol_mean, tol_m2).
    mean' = mean + (s1 / nb) (nb / n) is at most 4 correctly rounded operations on each side (a
    division, a division, a product, a sum; fused or not), each off by at most u times a magnitude that
    |mean| + |delta| bounds: 8 u (|mean| + |delta|).
    m2' = (m2 + (s2 - s1 delta)) + delta^2 (na nb / n) is at most 8 operations on each side, each off by
    at most u times a partial result that m2 + s2 + |s1 delta| + delta^2 na nb / n bounds: 16 u (...).
    The clamp at zero moves m2' towards the true value (m2 >= 0) and adds nothing."""
    na, mean, m2, _ = state
    nb, s1, s2 = rec[0], np.asarray(rec[1], np.float64), np.asarray(rec[2], np.float64)
    n = na + nb
    delta = s1 / nb
    return (8 * U * (np.abs(mean) + np.abs(delta)),
            16 * U * (m2 + s2 + np.abs(s1 * delta) + delta * delta * (na * nb / n)))


def inv_bound(inv):
    """inv = 1 / (sqrt(m2 / (n - 1)) + 1e-8) from the device's own m2' and count: a subtraction (exact
    for counts below 2^53), a division, a root, a sum and a division, four roundings without cancellation
    on each side, each moving the result by at most u of itself: 8 u inv"""
    return 8 * U * np.abs(inv)


def apply(state, x):
    """y = (float)(((double)x - mean[d]) * inv[d])"""
    _, mean, _, inv = state
    return ((x.astype(np.float64) - mean) * inv).astype(np.float32)


def chain(batches, state=None):
    """The reference run over `batches` (each [rows][D] float32), one record and merge per batch, and the
    tolerance of the resulting mean and m2 against exact arithmetic over the same rows, propagated merge
    by merge the way test_gpu_rollout_metrics._close_metrics.var_and_tol propagates a sum's bound into a
    variance.  -> (state, tol_mean[D], tol_m2[D]).

    With tm, t2 the tolerances before a merge, e1 = record_bound(nb, sum|x - K|) and e2 =
    record_bound(nb, sum (x - K)^2) those of the batch's record, ed = e1 / nb that of delta:
      mean'  exact arithmetic gives K na / n + mean_b nb / n, so the old error enters with na / n and the
             batch's with nb / n:  tm' = tm na / n + ed nb / n + 8 u (|mean| + |delta|)  (merge_bounds);
      m2'    the batch's own part s2 - s1^2 / nb moves by e2 + 2 |delta| e1 + e1^2 / nb; the cross term
             delta^2 na nb / n, delta = mean_b - K, moves by (2 |delta| (ed + tm) + (ed + tm)^2) na nb / n,
             tm being how far K is from the true mean of what was merged before; then the merge's own
             roundings, 16 u (m2 + s2 + |s1 delta| + delta^2 na nb / n)  (merge_bounds).
    The record bounds are already doubled (two summation orders), which here covers the device's and this
    reference's."""
    x0 = batches[0]
    D = x0.shape[1]
    st = fresh(D) if state is None else state
    tm, t2 = np.zeros(D), np.zeros(D)
    for x in batches:
        na, mean, m2, _ = st
        nb, s1, s2, ab1, ab2 = record(x, mean)
        if nb == 0:
            continue
        n = na + nb
        e1, e2 = record_bound(nb, ab1), record_bound(nb, ab2)
        ed = e1 / nb
        delta = np.abs(s1 / nb)
        bm, b2 = merge_bounds(st, (nb, s1, s2))
        t2 = t2 + (e2 + 2 * delta * e1 + e1 * e1 / nb) + (2 * delta * (ed + tm) + (ed + tm) ** 2) * (na * nb / n) + b2
        tm = tm * (na / n) + ed * (nb / n) + bm
        st = merge(st, (nb, s1, s2))
    return st, tm, t2


def two_pass(x):
    """mean and m2 of all rows by numpy's two passes, with their own error against exact arithmetic:
    the mean's sum within n u sum|x| (one summation order), so the mean within u sum|x| + u |mean|; m2 =
    sum (x - mean)^2 within n u m2 for the sum and, for a mean off by em, n em^2 (the first-order term
    2 em sum (x - mean) vanishes up to the same rounding, bounded by 2 em n u sum|x - mean| / n)."""
    x = np.asarray(x, np.float64)
    n = x.shape[0]
    mean = x.mean(0)
    dev = x - mean[None]
    m2 = (dev * dev).sum(0)
    em = U * np.abs(x).sum(0) + U * np.abs(mean)
    e2 = n * U * m2 + n * em * em + 2 * em * U * np.abs(dev).sum(0)
    return mean, m2, em, e2


def check_whole_state(state, rows_seen, batches, what=""):
    """the device state after merging `batches` in order against two_pass over all of their rows: the
    count exact, mean and m2 within chain()'s propagated bound plus two_pass's own error.  Non-vacuity
    first: on every column that varies, the standard deviation is more than 100 times its tolerance
    tol_m2 / (2 std (n - 1)) (d sqrt(m2 / (n - 1)) / d m2), and at least one column varies."""
    n, mean, m2, inv = state
    allx = np.concatenate([np.asarray(b, np.float32) for b in batches], 0)
    assert n == rows_seen == allx.shape[0], (what, n, rows_seen, allx.shape[0])
    _, tm, t2 = chain(batches)
    mean_t, m2_t, em, e2 = two_pass(allx)
    tm, t2 = tm + em, t2 + e2
    std = np.sqrt(m2_t / (n - 1.0))
    varies = std > 0
    assert varies.any(), what
    std_tol = t2[varies] / (2 * std[varies] * (n - 1.0))
    assert (std[varies] > 100 * std_tol).all(), (what, std[varies], std_tol)
    assert (np.abs(mean - mean_t) <= tm).all(), (what, "mean", np.abs(mean - mean_t).max(), tm.min())
    assert (np.abs(m2 - m2_t) <= t2).all(), (what, "m2", np.abs(m2 - m2_t).max(), t2.min())
    tol_inv = inv_bound(inv)
    assert (np.abs(inv - inv_of(n, m2)) <= tol_inv).all(), (what, "inv")


def case_data(rows, D, seed=0, offset=False):
    """the kernel tests' data: uniform float32 columns scaled differently per column, column D - 1
    constant; offset: column 0 is 1000 + 1e-3 noise (K ~ 1000 once a state has been merged from it)"""
    rng = np.random.default_rng(seed)
    x = (rng.random((rows, D)) * (1.0 + np.arange(D)[None] % 7) - 0.25 * (np.arange(D)[None] % 3)).astype(np.float32)
    x[:, D - 1] = np.float32(0.375)
    if offset:
        x[:, 0] = (1000.0 + 1e-3 * rng.standard_normal(rows)).astype(np.float32)
    return x


CASES = {"one_row": (1, 6), "odd_255": (255, 6), "odd_4097": (4097, 6), "c3": (1000, 24), "c5": (130, 192),
         "regime_e": (77, 288), "offset": (4097, 6)}
