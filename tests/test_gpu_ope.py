"""GPU tests of off-policy evaluation (rlks_ope_logp, rlks_ope_estimate, rlks.offline): the logp
kernel against the draws, bit for bit, and against the f64 log-softmax within its forward bound; the estimator
against the numpy f64 restatement (tests/ope_ref.py) at the shapes where its indexing can go wrong, its extremes,
determinism and argument errors; DecisionLog.collect / from_rollout and estimate() end to end on a table env
and on a node-level env with action masks.

Tolerances are ope_ref's: derived from the operation sequences and the documented ulp bounds of exp, expf and
logf, not fitted.  Every test prints the largest error / bound it saw."""
import ctypes as C_

import numpy as np
import pytest

import ope_ref

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")


def _dev():
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    return torch.device("cuda", 0)


def _put(x, shift=0):
    """a device copy of x that starts `shift` elements past a 16-byte boundary"""
    src = torch.from_numpy(np.ascontiguousarray(x).ravel())
    flat = torch.zeros(src.numel() + shift, dtype=src.dtype, device=_dev())
    assert flat.data_ptr() % 16 == 0
    flat[shift:] = src.to(flat.device)
    return flat[shift:]


# ----------------------------------------------------------------------------- rlks_ope_logp
def _masks(rng, rows, A):
    """random words, every third row of the first ones a word with one bit, all bits, no bit among the low A"""
    m = rng.integers(0, 2 ** 63, rows, dtype=np.uint64) << np.uint64(1) | rng.integers(0, 2, rows, dtype=np.uint64)
    for i in range(min(rows, 12)):
        if i % 4 == 0:
            m[i] = np.uint64(1) << np.uint64(i % A)
        elif i % 4 == 1:
            m[i] = np.uint64(2 ** 64 - 1)
        elif i % 4 == 2:
            m[i] = np.uint64(0) if A == 64 else np.uint64(1) << np.uint64(A)  # nothing among the low A bits
    return m


def _ope_logp(logits, actions, mask, rows, A):
    from rlks import _lib

    out = torch.full((rows,), 7.0, dtype=torch.float32, device=_dev())
    _lib.call("rlks_ope_logp", _lib.ptr(logits), _lib.ptr(actions), _lib.ptr(mask), rows, A, _lib.ptr(out), None)
    return out.cpu().numpy()


@pytest.mark.parametrize("A", [2, 4, 8, 9, 64])
def test_logp_equals_the_draws_bit_for_bit(A):
    from rlks import _lib

    d = _dev()
    rng = np.random.default_rng(100 + A)
    for rows in (1, 130, 4100):
        lg_h = (rng.standard_normal((rows, A)) * 2).astype(np.float32)
        logits = _put(lg_h)
        ids = _put(rng.integers(0, 2 ** 31, (rows, 3)).astype(np.int32))
        kinds = [None, _masks(rng, rows, A)]
        if rows == 1:  # the one row under each kind of word
            kinds += [np.array([2 ** 64 - 1], np.uint64), np.array([0], np.uint64)]
        for mask_h in kinds:
            mask = None if mask_h is None else _put(mask_h.view(np.int64))
            for explore in (1, 0):
                act = torch.empty(rows, dtype=torch.int32, device=d)
                logp = torch.empty(rows, dtype=torch.float32, device=d)
                if mask is None:
                    _lib.call("rlks_sample_categorical", _lib.ptr(logits), rows, A, _lib.ptr(ids), 77, explore,
                              _lib.ptr(act), _lib.ptr(logp), None)
                else:  # the masked draw writes the masked row back: give it a copy
                    work = logits.clone()
                    _lib.call("rlks_sample_categorical_masked", _lib.ptr(work), _lib.ptr(mask), rows, A,
                              _lib.ptr(ids), 77, explore, _lib.ptr(act), _lib.ptr(logp), None)
                got = _ope_logp(logits, act, mask, rows, A)
                want = logp.cpu().numpy()
                assert got.tobytes() == want.tobytes(), (A, rows, mask_h is not None, explore,
                                                         int((got.view(np.uint32) != want.view(np.uint32)).sum()))
        assert np.array_equal(logits.cpu().numpy().reshape(rows, A), lg_h)  # the logits are only read


@pytest.mark.parametrize("A", [2, 9, 64])
def test_logp_of_every_action_within_its_bound(A):
    rows = 130
    rng = np.random.default_rng(200 + A)
    lg = (rng.standard_normal((rows, A)) * 3).astype(np.float32)
    lg[5] = 0.0
    lg[6, 0] = 100.0  # the other entries' exp are subnormal
    big = np.repeat(lg, A, axis=0)           # row i A + a: row i's logits, action a
    acts = np.tile(np.arange(A, dtype=np.int32), rows)
    worst = 0.0
    for mask_h in (None, _masks(rng, rows, A)):
        mrep = None if mask_h is None else np.repeat(mask_h, A)
        got = _ope_logp(_put(big), _put(acts), None if mrep is None else _put(mrep.view(np.int64)), rows * A, A)
        ref, bound = ope_ref.logp_reference(big, acts, mrep, A)
        err = np.abs(got.astype(np.float64) - ref)
        assert np.all(err <= bound), (A, mask_h is not None, float(np.max(err / bound)))
        worst = max(worst, float(np.max(err / bound)))
        if mask_h is not None:  # logged actions outside the mask: the sentinel's logp, p = exp(.) = 0
            assert (got < -1e29).sum() > 0 and np.all(np.exp(got[got < -1e29].astype(np.float64)) == 0.0)
    print(f"logp A={A}: largest error / bound {worst:.3f}")
    bad = np.array([-1, A, 2 ** 31 - 1, -2 ** 31], np.int32)
    got = _ope_logp(_put(lg[:4]), _put(bad), None, 4, A)
    assert np.all(np.isnan(got))
    got = _ope_logp(_put(lg[:4]), _put(bad), _put(_masks(rng, 4, A).view(np.int64)), 4, A)
    assert np.all(np.isnan(got))


# ----------------------------------------------------------------------------- rlks_ope_estimate
def _log(seed, T, N, dones="random"):
    """seeded inputs: lr uniform in +-0.7, rewards N(0, 50) with +-5,000 among them, 8% dones"""
    rng = np.random.default_rng(seed)
    lo = (-rng.random((T, N)) * 2).astype(np.float32)
    ln = (lo + rng.uniform(-0.7, 0.7, (T, N)).astype(np.float32)).astype(np.float32)
    r = (rng.standard_normal((T, N)) * 50).astype(np.float32)
    k = min(T * N, 4)
    r.ravel()[rng.choice(T * N, k, replace=False)] = np.array([5000, -5000, 4765, -4765], np.float32)[:k]
    if dones == "random":
        d = (rng.random((T, N)) < 0.08).astype(np.uint8)
        if T * N > 2:
            d.ravel()[rng.integers(0, T * N)] = 255  # any non-zero byte is a done
    else:
        d = np.full((T, N), dones, np.uint8)
    return ln, lo, r, d


def _estimate(ln, lo, r, d, gamma, drop, shift=0, repeat=1, ep=True):
    """the kernels on host arrays -> `repeat` (record, ep_out) pairs (numpy); ep_out and the workspace are
    NaN-filled before every call"""
    from rlks import _lib

    dev = _dev()
    T, N = ln.shape
    t = [_put(x, shift) for x in (ln, lo, r, d)]
    wsb = C_.c_int64()
    _lib.call("rlks_ope_workspace_bytes", T, N, C_.byref(wsb))
    assert 12 * T * N <= wsb.value <= 12 * T * N + 16 * T + 4 * N + 8 * 13 * (N // 256 + 1) + 6 * 256
    ws = torch.empty(wsb.value // 8, dtype=torch.float64, device=dev)
    outs = []
    for _ in range(repeat):
        ws.fill_(float("nan"))
        rec = torch.full((13,), float("nan"), dtype=torch.float64, device=dev)
        epo = torch.full((T, N, 4), float("nan"), dtype=torch.float64, device=dev) if ep else None
        _lib.call("rlks_ope_estimate", *(x.data_ptr() for x in t), T, N, float(gamma), int(drop), rec.data_ptr(),
                  _lib.ptr(epo), ws.data_ptr(), wsb.value, None)
        outs.append((rec.cpu().numpy(), epo.cpu().numpy() if ep else None))
    return outs


# T, N, dones: the smallest shapes at which each mechanism can go wrong
SHAPES = {
    "single": (1, 1, 0),             # one truncated segment; dropped, it leaves no episode
    "ragged_lanes": (3, 130, "random"),   # N no multiple of 64: a ragged last wave, one workgroup
    "ragged_steps": (75, 67, "random"),   # segments at many different steps k at one time t: ragged c_k
    "long_truncated": (300, 5, 0),   # one truncated segment per lane, longer than a workgroup has threads
    "one_lane": (4000, 1, "random"),  # a long log on one lane: 4,000 row workgroups over one column
    "many_lanes": (7, 4100, "random"),  # 17 workgroups: the partial records, a ragged last workgroup
    "all_done": (2, 64, 1),          # every step an episode
}
REFS = {}


def _ref(name, drop):
    """the shape's inputs and their reference, computed once"""
    if (name, drop) not in REFS:
        T, N, dones = SHAPES[name]
        x = _log(300 + len(name) + T, T, N, dones)
        REFS[(name, drop)] = (x, ope_ref.reference(*x, 0.97, drop_truncated=drop))
    return REFS[(name, drop)]


@pytest.mark.parametrize("drop", [False, True])
@pytest.mark.parametrize("name", list(SHAPES))
def test_estimate_matches_reference(name, drop):
    from rlks import _lib

    x, ref = _ref(name, drop)
    (rec, ep), = _estimate(*x, 0.97, drop)
    worst = ope_ref.check_estimate(rec, ref, ep, f"{name} drop={drop}")
    E = int(ref["record"][_lib.RLKS_OPE_EPISODES])
    print(f"{name} drop={drop}: {E} episodes, {int(np.count_nonzero(ref['c']))} distinct steps reached, "
          f"largest error / bound {worst:.3f}")
    if drop and name in ("single", "long_truncated"):  # nothing counted: zeros, no fault
        assert E == 0 and np.all(rec == 0.0)
    else:
        assert E > 0
    if name == "ragged_steps":
        assert len(np.unique(ref["c"][ref["c"] > 0])) > 8  # c_k is ragged indeed


def test_estimate_on_misaligned_buffers():
    """every input 4 bytes (the done bytes 1 byte) past a 16-byte boundary"""
    x, ref = _ref("ragged_lanes", False)
    (rec, ep), = _estimate(*x, 0.97, False, shift=1)
    ope_ref.check_estimate(rec, ref, ep, "shift")


def test_estimate_without_ep_out_and_twice_gives_the_same_bytes():
    x, ref = _ref("ragged_steps", False)
    (r1, e1), (r2, e2) = _estimate(*x, 0.97, False, repeat=2)
    assert r1.tobytes() == r2.tobytes() and e1.tobytes() == e2.tobytes()
    (r3, _), = _estimate(*x, 0.97, False, ep=False)
    assert r3.tobytes() == r1.tobytes()


def test_estimate_extremes():
    from rlks import _lib as L

    T = 30
    rng = np.random.default_rng(5)
    r = rng.uniform(-1, 1, (T, 2)).astype(np.float32)
    d = np.zeros((T, 2), np.uint8)
    zero = np.zeros((T, 2), np.float32)
    # lr = -40 on both lanes: from step 19 on every p underflows to 0, S_k == 0, the terms are 0.0
    x = (zero - 40, zero, r, d)
    ref = ope_ref.reference(*x, 1.0)
    assert ref["S"][-1] == 0.0
    (rec, ep), = _estimate(*x, 1.0, False)
    ope_ref.check_estimate(rec, ref, ep, "lr = -40")
    assert np.all(np.isfinite(rec)) and np.all(np.isfinite(ep[T - 1]))
    # lr = +40 on lane 0: L passes RLKS_OPE_LMAX at step 18; lane 1 holds w_k at (p_k + 1) / 2
    ln = zero.copy()
    ln[:, 0] = 40
    x = (ln, zero, r, d)
    ref = ope_ref.reference(*x, 1.0)
    (rec, ep), = _estimate(*x, 1.0, False)
    # squares of values near exp(700) overflow f64 (exp(700)^2 > 1.8e308): VIS_SQ and PEND_SQ are +inf on both sides
    finite = [s for s in range(L.RLKS_OPE_VB_SUM, L.RLKS_OPE_SIZE) if np.isfinite(ref["record"][s])]
    assert set(finite) >= {L.RLKS_OPE_VB_SUM, L.RLKS_OPE_VB_SQ, L.RLKS_OPE_VIS_SUM, L.RLKS_OPE_VWIS_SUM,
                           L.RLKS_OPE_VWIS_SQ, L.RLKS_OPE_PEND_SUM}
    ope_ref.check_estimate(rec, ref, ep, "lr = +40", sums=finite)
    assert rec[L.RLKS_OPE_CLAMPED] == 13 and np.all(np.isfinite(ep[T - 1])) and np.all(np.isfinite(rec[finite]))
    assert ep[T - 1, 0, 3] == np.exp(L.RLKS_OPE_LMAX) or abs(ep[T - 1, 0, 3] / np.exp(L.RLKS_OPE_LMAX) - 1) <= 2 ** -51


def test_estimate_counts_bad_rows():
    from rlks import _lib as L

    ln, lo, r, d = (a.copy() for a in _ref("ragged_lanes", False)[0])
    lo[0, 3] = np.nan
    lo[2, 129] = np.inf
    ln[1, 64] = -np.inf
    (rec, _), = _estimate(ln, lo, r, d, 0.97, False)
    assert rec[L.RLKS_OPE_BAD_ROWS] == 3
    assert rec[L.RLKS_OPE_STEPS] == 3 * 130


def test_argument_errors():
    from rlks import _lib

    dev = _dev()
    lib = _lib.lib()
    T, N = 3, 5
    f = torch.zeros(T * N + 4, dtype=torch.float32, device=dev)
    dn = torch.zeros(T * N, dtype=torch.uint8, device=dev)
    rec = torch.zeros(16, dtype=torch.float64, device=dev)
    wsb = C_.c_int64()
    _lib.call("rlks_ope_workspace_bytes", T, N, C_.byref(wsb))
    ws = torch.zeros(wsb.value // 8 + 1, dtype=torch.float64, device=dev)
    p, q, w = f.data_ptr(), rec.data_ptr(), ws.data_ptr()

    def est(ln=p, lo=p, r=p, d=dn.data_ptr(), T_=T, N_=N, gamma=0.9, rec_=q, ep=None, ws_=w, wb=wsb.value):
        return lib.rlks_ope_estimate(ln, lo, r, d, T_, N_, gamma, 0, rec_, ep, ws_, wb, None)

    assert est() == 0
    for kw in (dict(ln=None), dict(lo=None), dict(r=None), dict(d=None), dict(rec_=None), dict(ws_=None), dict(T_=0),
               dict(N_=0), dict(N_=-1), dict(gamma=1.5), dict(gamma=-0.1), dict(gamma=float("nan")),
               dict(gamma=float("inf")), dict(ln=p + 2), dict(r=p + 1), dict(rec_=q + 4), dict(ep=q + 4),
               dict(ws_=w + 4), dict(wb=wsb.value - 1), dict(wb=0)):
        assert est(**kw) == -1, kw
        assert b"rlks_ope_estimate" in lib.rlks_last_error()
    assert lib.rlks_ope_workspace_bytes(0, 1, C_.byref(wsb)) == -1 and lib.rlks_ope_workspace_bytes(1, 1, None) == -1
    a = torch.zeros(4, dtype=torch.int32, device=dev)
    m = torch.zeros(4, dtype=torch.int64, device=dev)
    big = torch.zeros(4 * 65, dtype=torch.float32, device=dev)
    assert lib.rlks_ope_logp(big.data_ptr(), a.data_ptr(), None, 4, 65, p, None) == 0
    assert lib.rlks_ope_logp(big.data_ptr(), a.data_ptr(), m.data_ptr(), 4, 65, p, None) == -3
    assert lib.rlks_ope_logp(p, a.data_ptr(), None, 0, 2, p, None) == 0
    for args in ((None, a.data_ptr(), None, 4, 2, p), (p, None, None, 4, 2, p), (p, a.data_ptr(), None, 4, 2, None),
                 (p, a.data_ptr(), None, -1, 2, p), (p, a.data_ptr(), None, 4, 0, p), (p + 2, a.data_ptr(), None, 4, 2, p),
                 (p, a.data_ptr(), m.data_ptr() + 4, 4, 2, p)):
        assert lib.rlks_ope_logp(*args, None) == -1, args
    torch.cuda.synchronize()


# ----------------------------------------------------------------------------- end to end
def _table_algo(d, seed=3):
    from rlks.ppo import PPO, PPOConfig

    cfg = (PPOConfig().framework("torch")
           .training(train_batch_size=256, sgd_minibatch_size=256, num_sgd_iter=1, lr=3e-4).debugging(seed=seed))
    cfg.num_envs = 64
    return PPO(config=cfg, device=d)


def test_end_to_end_table_env(tmp_path):
    from rlks.offline import DecisionLog, estimate, run_estimate, summarise, target_logp
    from rlks.policy import PolicyParams

    d = _dev()
    algo = _table_algo(d)
    T, N, gamma = 120, 64, 0.99
    log = DecisionLog.collect(algo, T, lanes=N, seed=11)
    h = log.to_numpy()
    assert h["obs"].shape == (T, N, 6) and h["dones"].sum() == N and h["dones"][98].all()  # episodes of 99 steps
    assert set(np.unique(h["actions"])) == {0, 1} and np.all(h["logp"] < 0)
    # the collecting policy as the target: the ratios are 1 up to the forward's rounding
    res = estimate(algo, log, gamma=gamma, per_episode=True)
    assert res["episodes"] == 2 * N and res["steps"] == T * N and res["max_len"] == 99 and res["clamped_steps"] == 0
    lp_new = target_logp(algo, log).cpu().numpy()
    m = float(np.max(np.abs(lp_new.astype(np.float64) - h["logp"].astype(np.float64))))
    absx = ope_ref.reference(h["logp"], h["logp"], np.abs(h["rewards"]), h["dones"], gamma)  # v_behavior = sum |x_k|
    lens = np.where(absx["ep_index"] // N == 98, 99, T - 99)
    pe = res["per_episode"]
    assert len(pe["v_is"]) == 2 * N
    slack = absx["ep"][:, 0] * (np.expm1(lens * m) + 4 * lens * ope_ref.U * np.exp(lens * m))
    print(f"table env: max |lr| {m:.3e}, max |v_is - v_behavior| {np.max(np.abs(pe['v_is'] - pe['v_behavior'])):.3e}")
    assert np.all(np.abs(pe["v_is"] - pe["v_behavior"]) <= slack)
    assert abs(res["is"]["v_delta"]) <= np.mean(slack) and abs(res["ess"] - 2 * N) <= 2 * N * np.expm1(4 * 99 * m)
    # a differently seeded policy as the target, against the restatement fed the same logp_new
    other = PolicyParams(6, 256, 2, device=d, seed=9)
    lp = target_logp(other, log)
    lp_h = lp.cpu().numpy()
    assert np.max(np.abs(lp_h - h["logp"])) > 1e-3
    ref = ope_ref.reference(lp_h, h["logp"], h["rewards"], h["dones"], gamma)
    dev = lambda k: torch.from_numpy(h[k]).to(d)  # noqa: E731
    rec, ep = run_estimate(lp, dev("logp"), dev("rewards"), dev("dones"), gamma, per_episode=True)
    worst = ope_ref.check_estimate(rec, ref, ep.cpu().numpy(), "table env")
    print(f"table env, other policy: largest error / bound {worst:.3f}")
    res2 = estimate(other, log, gamma=gamma, per_episode=True)
    pe2 = res2.pop("per_episode")
    assert res2 == summarise(rec)
    for j, k in enumerate(("v_behavior", "v_is", "v_wis", "p_end")):
        assert np.array_equal(pe2[k], ep.cpu().numpy().reshape(-1, 4)[ref["ep_index"], j])
    dropped = estimate(other, log, gamma=gamma, drop_truncated=True)
    assert dropped["episodes"] == N and dropped["steps"] == 99 * N
    # the live algorithm, its server and its checkpoint give the same bytes; a saved log too
    path = algo.save(tmp_path / "ckpt")
    log.save(tmp_path / "log.npz")
    live = estimate(algo, log, gamma=gamma)
    assert estimate(algo.server(), log, gamma=gamma) == live
    assert estimate(str(path), DecisionLog.load(tmp_path / "log.npz"), gamma=gamma) == live
    assert target_logp(path, log).cpu().numpy().tobytes() == lp_new.tobytes()
    with pytest.raises(ValueError, match="unknown off-policy"):
        estimate(algo, log, methods=("dm",))
    with pytest.raises(ValueError, match="no counted episode"):
        estimate(algo, DecisionLog(*(h[k][:50] for k in ("obs", "actions", "logp", "rewards", "dones"))),
                 drop_truncated=True)
    bad = h["logp"].copy()
    bad[0, 0] = -np.inf
    with pytest.raises(ValueError, match="not finite"):
        estimate(algo, DecisionLog(h["obs"], h["actions"], bad, h["rewards"], h["dones"]))


def test_end_to_end_node_env_with_masks():
    from rlks import _lib as L
    from rlks.env import NodeSpec
    from rlks.offline import DecisionLog, estimate
    from rlks.ppo import PPO, PPOConfig
    from rlks.tables import synthetic_table

    d = _dev()
    N, T, C = 64, 16, 3  # occupancy 1.0 and 40 arrivals a step fill clusters within the fragment: masks bite
    spec = NodeSpec(C, 16, node_cpu_m=[2000] * 3, node_mem_mi=[1024, 4096, 1024], arrival_rate=40.0, depart_prob=0.02,
                    init_occupancy=1.0, reject_penalty=0.25)
    cfg = (PPOConfig().framework("torch")
           .training(train_batch_size=N * T, sgd_minibatch_size=256, num_sgd_iter=1, lr=3e-4, action_mask="room")
           .debugging(seed=5))
    cfg.num_envs, cfg.table, cfg.nodes = N, synthetic_table(C, 100, seed=7), spec
    algo = PPO(config=cfg, device=d)
    assert algo.T == T and algo.A == C
    algo.train()
    log = DecisionLog.from_rollout(algo)
    h = log.to_numpy()
    lg = algo.buf["logits"].cpu().numpy()
    allowed = lg > L.RLKS_MASKED_LOGIT_MAX
    words = (allowed.astype(np.uint64) << np.arange(C, dtype=np.uint64)).sum(2).astype(np.uint64)
    assert np.array_equal(h["action_mask"], words) and (~allowed).sum() > 0 and allowed.any(2).all()
    assert allowed[np.arange(T)[:, None], np.arange(N)[None, :], h["actions"]].all()
    assert np.array_equal(h["logp"], algo.buf["logp"].cpu().numpy()) and log.n_actions == C
    res = estimate(algo, log, gamma=0.99)
    assert res["episodes"] == N and res["steps"] == N * T
    assert all(np.isfinite(res[m][k]) for m in ("is", "wis") for k in res[m]) and 0 < res["ess"] <= N * (1 + 1e-12)
    with pytest.raises(ValueError, match="action mask"):
        estimate(algo, DecisionLog(*(h[k] for k in ("obs", "actions", "logp", "rewards", "dones"))))
    # collect under the masked policy: the env's masks are logged and the decisions respect them
    col = DecisionLog.collect(algo, 6, lanes=32, table=cfg.table, nodes=spec, seed=2)
    c = col.to_numpy()
    bits = (c["action_mask"][..., None] >> np.arange(C, dtype=np.uint64)) & np.uint64(1)
    assert bits[np.arange(6)[:, None], np.arange(32)[None, :], c["actions"]].all()
    assert estimate(algo, col)["steps"] == 6 * 32
