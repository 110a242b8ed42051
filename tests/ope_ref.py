"""numpy f64 restatement of the off-policy estimators (rlks_ope_estimate, rlks_ope_logp; include/rlks.h,
DESIGN.md §28) and the error bounds the GPU tests hold the device to.  Nothing here is fitted to what the
device gives: every bound follows from the operation sequences and from two documented figures,

  * device exp (f64), expf and logf (f32): at most 1 ulp from the true value (ROCm documentation, HIP "Math
    API" reference, the tables of maximum ULP error of the single- and double-precision functions);
  * numpy's exp on the host (glibc): at most 1 ulp (glibc manual, "Known Maximum Errors in Math Functions"),

and from Higham, Accuracy and Stability of Numerical Algorithms, §4.2: a sum of n terms in any order errs by
at most (n - 1) u sum|x| + O(u^2).  As tests/rollout_metrics_ref.py does, sum bounds are rounded up to
n u sum|x| and doubled, since the restatement's own sum carries the same error.  Bounds are first order in u;
the second-order terms are below 1e-10 of them at the sizes the tests use.  The relative bound on p_k holds
for normal results; a subnormal p_k (below 2.2e-308) is within 1 ulp = 2^-1074 absolutely, which the IS and
p_end bounds add; the WIS bound does not cover segments whose p_k differ and are subnormal at the same step.

The estimate, per lane n of a time-major [T][N] log (every f32 widened to f64 first, every operation rounded on
its own, in this order):
    lr = logp_new - logp_old;  L_k = L_{k-1} + lr;  p_k = exp(min(L_k, LMAX));  g_k = g_{k-1} gamma, g_0 = 1;
    x_k = g_k r;  v_behavior = sum x_k;  v_is = sum p_k x_k;  w_k = S_k / c_k over the counted segments at step
    k;  v_wis = sum (p_k / w_k) x_k with 0.0 where S_k == 0;  p_end = p at the segment's last step.
"""
import numpy as np

from rlks import _lib as L

U = 2.0 ** -53        # f64 unit roundoff
U32 = 2.0 ** -24      # f32 unit roundoff; 1 ulp is at most 2 U32 relative
SUBNORMAL = 2.0 * 2.0 ** -1074  # 1 ulp of a subnormal f64 on each side
EXP_ULP = 1.0         # device exp / expf / logf and host exp: ulp bound taken for each
SLOTS_EXACT = (L.RLKS_OPE_EPISODES, L.RLKS_OPE_STEPS, L.RLKS_OPE_MAX_LEN, L.RLKS_OPE_CLAMPED, L.RLKS_OPE_BAD_ROWS)
VALUE_SLOTS = ((L.RLKS_OPE_VB_SUM, L.RLKS_OPE_VB_SQ), (L.RLKS_OPE_VIS_SUM, L.RLKS_OPE_VIS_SQ),
               (L.RLKS_OPE_VWIS_SUM, L.RLKS_OPE_VWIS_SQ), (L.RLKS_OPE_PEND_SUM, L.RLKS_OPE_PEND_SQ))


def counted_end(dones, drop_truncated):
    """t_end[n]: one past the last step of lane n inside a counted segment"""
    T, N = dones.shape
    if not drop_truncated:
        return np.full(N, T, np.int64)
    d = dones != 0
    last = T - 1 - np.argmax(d[::-1], axis=0)
    return np.where(d.any(axis=0), last + 1, 0).astype(np.int64)


def reference(logp_new, logp_old, rewards, dones, gamma, drop_truncated=False):
    """-> dict(record, record_bound: double[RLKS_OPE_SIZE]; ep_index: int64 [E] = t_end N + n ascending;
    ep, ep_bound: double [E][4] = v_behavior, v_is, v_wis, p_end; S, c: the rows' sums and counts).
    record_bound is 0 in the count slots: they are exact."""
    ln, lo, r = (np.asarray(a) for a in (logp_new, logp_old, rewards))
    d = np.asarray(dones)
    assert ln.dtype == lo.dtype == r.dtype == np.float32 and d.dtype == np.uint8
    T, N = ln.shape
    gamma = float(gamma)
    lr = ln.astype(np.float64) - lo.astype(np.float64)
    rr = r.astype(np.float64)
    t_end = counted_end(d, drop_truncated)
    lanes = np.arange(N)
    with np.errstate(over="ignore", invalid="ignore"):
        # walk one: p, k and the bound on p's relative error, then the rows
        p = np.zeros((T, N))
        relp = np.zeros((T, N))
        kk = np.zeros((T, N), np.int64)
        live = np.zeros((T, N), bool)
        k = np.zeros(N, np.int64)
        Lc = np.zeros(N)
        Labs = np.zeros(N)
        clamped = 0
        for t in range(T):
            on = t < t_end
            Lc = Lc + lr[t]
            Labs = Labs + np.abs(lr[t])
            clamped += int(np.count_nonzero(on & (Lc > L.RLKS_OPE_LMAX)))
            p[t] = np.exp(np.minimum(Lc, L.RLKS_OPE_LMAX))
            # L_k: a sum of k + 1 terms on both sides; its error passes through exp as a relative one;
            # then one exp on each side
            relp[t] = np.expm1(2.0 * (k + 1) * U * Labs) + 2.0 * EXP_ULP * 2.0 * U
            kk[t] = k
            live[t] = on
            end = d[t] != 0
            k = np.where(end, 0, k + 1)
            Lc = np.where(end, 0.0, Lc)
            Labs = np.where(end, 0.0, Labs)
        S = np.zeros(T)
        c = np.zeros(T, np.int64)
        relp_row = np.zeros(T)
        np.add.at(S, kk[live], p[live])
        np.add.at(c, kk[live], 1)
        np.maximum.at(relp_row, kk[live], relp[live])
        w = np.where(c > 0, S / np.maximum(c, 1), 0.0)
        # w_k: the row's sum (c_k non-negative terms, doubled), its terms' own error, one division a side
        relw = relp_row + 2.0 * c * U + 2.0 * U
        # walk two: the segments' values with their bounds
        bad = int(np.count_nonzero(live & ~(np.isfinite(ln) & np.isfinite(lo))))
        z = lambda: np.zeros(N)  # noqa: E731
        g, vb, vis, vw = np.ones(N), z(), z(), z()
        ax, apx, epx, aqx, eqx = z(), z(), z(), z(), z()
        k = np.zeros(N, np.int64)
        idx, vals, bnds, lens = [], [], [], []
        for t in range(T):
            on = t < t_end
            x = g * rr[t]
            px = p[t] * x
            wk, Sk = w[kk[t]], S[kk[t]]
            q = np.where(Sk == 0.0, 0.0, p[t] / np.where(Sk == 0.0, 1.0, wk))
            qx = np.where(Sk == 0.0, 0.0, q * x)
            vb, vis, vw = vb + x, vis + px, vw + qx
            ax += np.abs(x)
            apx += np.abs(px)
            epx += np.abs(px) * (relp[t] + 2.0 * U) + np.abs(x) * SUBNORMAL  # p's error, one product a side
            aqx += np.abs(qx)
            eqx += np.abs(qx) * (relp[t] + relw[kk[t]] + 4.0 * U)         # p's, w's, a division and a product a side
            end = (d[t] != 0) | (t == t_end - 1)
            close = on & end
            if close.any():
                n_ = lanes[close]
                ln_ = (k[close] + 1).astype(np.float64)
                idx.append(t * N + n_)
                lens.append(k[close] + 1)
                vals.append(np.stack([vb[close], vis[close], vw[close], p[t][close]], 1))
                bnds.append(np.stack([2.0 * ln_ * U * ax[close], epx[close] + 2.0 * ln_ * U * apx[close],
                                      eqx[close] + 2.0 * ln_ * U * aqx[close],
                                      p[t][close] * relp[t][close] + SUBNORMAL], 1))
            rst = d[t] != 0
            g = np.where(rst, 1.0, g * gamma)
            k = np.where(rst, 0, k + 1)
            for a in (vb, vis, vw, ax, apx, epx, aqx, eqx):
                a[rst] = 0.0
        rec = np.zeros(L.RLKS_OPE_SIZE)
        bnd = np.zeros(L.RLKS_OPE_SIZE)
        if idx:
            idx, lens = np.concatenate(idx), np.concatenate(lens)
            vals, bnds = np.concatenate(vals), np.concatenate(bnds)
        else:
            idx, lens, vals, bnds = np.zeros(0, np.int64), np.zeros(0, np.int64), np.zeros((0, 4)), np.zeros((0, 4))
        E = len(idx)
        rec[L.RLKS_OPE_EPISODES] = E
        rec[L.RLKS_OPE_STEPS] = lens.sum()
        rec[L.RLKS_OPE_MAX_LEN] = lens.max() if E else 0
        rec[L.RLKS_OPE_CLAMPED] = clamped
        rec[L.RLKS_OPE_BAD_ROWS] = bad
        for j, (s_sum, s_sq) in enumerate(VALUE_SLOTS):
            v, b = vals[:, j], bnds[:, j]
            rec[s_sum] = np.sum(v)
            rec[s_sq] = np.sum(v * v)
            bnd[s_sum] = np.sum(b) + 2.0 * E * U * np.sum(np.abs(v))
            # (v + e)^2 - v^2 = 2 v e + e^2, one square a side, then the sum
            bnd[s_sq] = np.sum(2.0 * np.abs(v) * b + b * b + 2.0 * U * v * v) + 2.0 * E * U * np.sum(v * v)
    return {"record": rec, "record_bound": bnd, "ep_index": idx, "ep": vals, "ep_bound": bnds, "S": S, "c": c}


def check_estimate(record, ref, ep_out=None, what="", sums=range(L.RLKS_OPE_VB_SUM, L.RLKS_OPE_SIZE)):
    """counts bit-equal, every sum (of the slots `sums`) and every per-episode entry within its bound, ep_out
    untouched (NaN, as the caller filled it) elsewhere -> the largest error / bound seen"""
    rec = np.asarray(record, np.float64)
    worst = 0.0
    for s in SLOTS_EXACT:
        assert rec[s].tobytes() == ref["record"][s].tobytes(), (what, "slot", s, rec[s], ref["record"][s])
    for s in sums:
        err, tol = abs(rec[s] - ref["record"][s]), ref["record_bound"][s]
        assert err <= tol, (what, "slot", s, rec[s], ref["record"][s], err, tol)
        worst = max(worst, err / tol if tol > 0 else 0.0)
    if ep_out is not None:
        flat = np.asarray(ep_out, np.float64).reshape(-1, 4)
        got = flat[ref["ep_index"]]
        err = np.abs(got - ref["ep"])
        assert np.all(err <= ref["ep_bound"]), (what, "ep_out", float(np.max(err - ref["ep_bound"])))
        rest = np.ones(len(flat), bool)
        rest[ref["ep_index"]] = False
        assert np.all(np.isnan(flat[rest])), (what, "ep_out written outside the counted segments' last steps")
        ok = ref["ep_bound"] > 0
        if ok.any():
            worst = max(worst, float(np.max(err[ok] / ref["ep_bound"][ok])))
    return worst


def masked_rows(logits, mask, A):
    """the rows rlks_ope_logp reads: float32 [rows][A], RLKS_MASKED_LOGIT outside the mask words (uint64 [rows]
    or None); a word without a bit among the low A counts as all of them"""
    lg = np.asarray(logits, np.float32).reshape(-1, A)
    if mask is None:
        return lg
    low = np.uint64((1 << A) - 1) if A < 64 else np.uint64(0xFFFFFFFFFFFFFFFF)
    m = np.asarray(mask, np.uint64) & low
    m = np.where(m == 0, low, m)
    bits = ((m[:, None] >> np.arange(A, dtype=np.uint64)[None, :]) & np.uint64(1)).astype(bool)
    return np.where(bits, lg, np.float32(L.RLKS_MASKED_LOGIT)).astype(np.float32)


def logp_reference(logits, actions, mask, A):
    """-> (logp f64 [rows], bound [rows]) for the f64 log-softmax of the same f32 rows at the given actions
    (NaN, bound 0 for an action outside [0, A)).  The device's sequence, u = 2^-24:
        d_a = fl(l_a - mx)              |error| <= u |d_a|
        e_a = expf(d_a)                 relative error <= 2 u (1 ulp) + u |d_a| (from d_a); absolute 2^-126 more
                                        where the result is subnormal (it may be flushed to 0)
        s = sum_a e_a, ascending        |error| <= sum e_a (rho_a + (A - 1) u);  s >= 1
        logf(s)                         relative error <= 2 u (1 ulp), after (error of s) / s
        (l_act - mx) - logf(s)          u |d_act|, then u |logp|"""
    x = masked_rows(logits, mask, A).astype(np.float64)
    rows = x.shape[0]
    act = np.asarray(actions, np.int64)
    ok = (act >= 0) & (act < A)
    a = np.where(ok, act, 0)
    mx = x.max(1, keepdims=True)
    dd = x - mx
    e = np.exp(dd)
    s = e.sum(1)
    da = dd[np.arange(rows), a]
    lp = da - np.log(s)
    rel_s = (e * (2.0 * EXP_ULP * U32 + U32 * np.abs(dd) + (A - 1) * U32)).sum(1) / s + A * 2.0 ** -126
    bound = U32 * np.abs(da) + rel_s + 2.0 * EXP_ULP * U32 * np.abs(np.log(s)) + U32 * np.abs(lp)
    return np.where(ok, lp, np.nan), np.where(ok, bound, 0.0)
