"""GPU tests of the table-env rollouts in every form rlks_rollout_form can name for them:
the persistent split-fp16 kernel (k_sf_roll), the per-step split-fp16 form (k_sf_fwd16 + k_sample_step), the
fused fp32 step on 32- and 128-row tiles (k_fwd_head<..., FWD_ROLLOUT>) and the per-step fp32 form, under the
weight regimes and tables of table_rollout_cases.py.

Every case: the form the library names is the expected one; logits[t] (t < T) and values[t] (t <= T) pass
tests/parity.close_as_fp32 with its defaults against the fp64 oracle and its fp32 band; logp passes it against
log-softmax of the stored logits in fp64 and fp32; observations, rewards and dones are what the C oracle env
gives for the rollout's actions, bit for bit.  The error percentiles are printed before they are asserted
(`pytest -s`), which is where DESIGN.md §30's figures come from."""
import ctypes as C

import numpy as np
import pytest

import oracle
import table_rollout_cases as tc
from parity import QS, close_as_fp32, logp_of, rel_errors

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")


def _dev():
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    return torch.device("cuda", 0)


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view({1: np.uint8, 4: np.uint32, 8: np.uint64}[a.dtype.itemsize])


def _form(handle, desc, N, T, job_lanes=0):
    """rlks_rollout_form for these shapes (a host query: the buffers are never read)"""
    from rlks import _lib

    bufs = _lib.RolloutBufs(*([None] * 9), T, N, job_lanes)
    form = C.c_int32(-1)
    _lib.call("rlks_rollout_form", handle, C.byref(desc), C.byref(bufs), C.byref(form))
    return form.value


def _lds_bytes(desc, form, rows, clouds):
    from rlks import _lib

    out = C.c_int64()
    _lib.call("rlks_rollout_lds_bytes", C.byref(desc), form, rows, clouds, C.byref(out))
    return out.value


def _rollout(case, d, tab=None):
    """PPO.rollout of `case` from reset: (algo, host buffers, table)"""
    from rlks.ppo import PPO, PPOConfig

    tab = tab if tab is not None else tc.table(case.regime, case.A, case.rows)
    cfg = (PPOConfig().framework("torch")
           .training(train_batch_size=case.lanes * case.steps, sgd_minibatch_size=256 if case.prec == "sf16" else 128,
                     num_sgd_iter=1, lr=3e-4)
           .debugging(seed=tc.SEED))
    cfg.num_envs, cfg.table, cfg.sgd_precision = case.lanes, tab, case.prec
    algo = PPO(config=cfg, device=d)
    assert (algo.T, algo.N, algo.precision) == (case.steps, case.lanes, case.prec)
    tc.apply_regime(algo.params, case.regime)
    if case.per_step:
        algo.bufs.global_lanes = tc.SF_ROLL_FUSED_MAX_LANES + 1
    form = C.c_int32(-1)
    from rlks import _lib

    _lib.call("rlks_rollout_form", algo.env.handle, C.byref(algo.params.desc), C.byref(algo.bufs), C.byref(form))
    assert form.value == case.form, (tc.FORM_NAMES.get(form.value), tc.FORM_NAMES[case.form])
    algo.rollout(explore=case.explore)
    torch.cuda.synchronize()
    return algo, {k: v.cpu().numpy() for k, v in algo.buf.items()}, tab


def _report(cid, what, x, ref64, ref32):
    """print the percentiles of the kernel's and the fp32 band's relative errors, then hold them to close_as_fp32"""
    e, e32 = rel_errors(x, ref64, ref32)
    print(f"TABLE_ROLLOUT {cid} {what} n={e.size} kernel " + " ".join(f"{np.percentile(e, q):.3e}" for q in QS)
          + " band " + " ".join(f"{np.percentile(e32, q):.3e}" for q in QS))
    close_as_fp32(x, ref64, ref32, what=f"{cid} {what}")


def _check_forward(case, algo, b, lanes=None):
    """logits[t], t < T, and values[t], t <= T, of `lanes` (all) against the fp64 oracle and its fp32 band"""
    A, D, T = case.A, 3 * case.A, case.steps
    sel = np.arange(case.lanes) if lanes is None else lanes
    flat, off = algo.params.flat.cpu().numpy(), algo.params.offsets
    x = b["obs"][:, sel].reshape(-1, D)
    el, ev = oracle.mlp_forward(flat, off, D, tc.H, A, x)
    fl, fv = oracle.mlp_forward_fp32_band(flat, off, D, tc.H, A, x)
    n = T * len(sel)
    _report(case.id, "logits", b["logits"][:, sel].reshape(-1, A), el[:n], [f[:n] for f in fl])
    _report(case.id, "values", b["values"][:, sel].reshape(-1), ev, fv)
    return el[:n], ev


def _check_logp(case, b):
    lg, a = b["logits"], b["actions"]
    assert a.min() >= 0 and a.max() < case.A
    _report(case.id, "logp", b["logp"], logp_of(lg, a), logp_of(lg, a, np.float32))


def _check_replay(case, b, tab):
    """obs, rewards and dones are the C oracle env's for the rollout's actions, bit for bit"""
    ora = oracle.OracleEnv(oracle.make_cfg(case.lanes, tab.n_rows, tab.n_clouds, noise_mode=0, seed=tc.SEED,
                                           autoreset=1), tab.cost, tab.latency)
    np.testing.assert_array_equal(_bits(ora.reset()), _bits(b["obs"][0]))
    for t in range(case.steps):
        o, r, term, _, _, _ = ora.step(b["actions"][t])
        np.testing.assert_array_equal(_bits(o), _bits(b["obs"][t + 1]), err_msg=f"obs[{t + 1}]")
        np.testing.assert_array_equal(_bits(r.astype(np.float32)), _bits(b["rewards"][t]), err_msg=f"rewards[{t}]")
        np.testing.assert_array_equal(term, b["dones"][t], err_msg=f"dones[{t}]")


def _check_all(case, algo, b, tab, lanes=None):
    ref = _check_forward(case, algo, b, lanes)
    _check_logp(case, b)
    _check_replay(case, b, tab)
    return ref


def _buffers(T, N, A, d):
    """rollout buffers filled with sentinels, and their rlks_rollout_bufs"""
    from rlks import _lib

    f32 = dict(dtype=torch.float32, device=d)
    buf = {"obs": torch.full((T + 1, N, 3 * A), 7.0, **f32), "logits": torch.full((T, N, A), 7.0, **f32),
           "values": torch.full((T + 1, N), 7.0, **f32), "actions": torch.full((T, N), -7, dtype=torch.int32, device=d),
           "logp": torch.full((T, N), 7.0, **f32), "rewards": torch.full((T, N), 7.0, **f32),
           "dones": torch.full((T, N), 7, dtype=torch.uint8, device=d), "adv": torch.zeros(T, N, **f32),
           "vtarg": torch.zeros(T, N, **f32)}
    bufs = _lib.RolloutBufs(*(buf[k].data_ptr() for k in ("obs", "logits", "values", "actions", "logp", "rewards",
                                                          "dones", "adv", "vtarg")), T, N, 0)
    return buf, bufs


@pytest.mark.parametrize("case", tc.PARITY, ids=lambda c: c.id)
def test_rollout_forms_match_fp64_in_every_regime(case):
    """72 lanes (two full 32-row tiles and one with 8 valid rows) x 8 steps on the 100-row table"""
    algo, b, tab = _rollout(case, _dev())
    _check_all(case, algo, b, tab)


@pytest.mark.parametrize("case", tc.ARGMAX, ids=lambda c: c.id)
def test_argmax_rollouts_take_the_largest_logit(case):
    algo, b, tab = _rollout(case, _dev())
    np.testing.assert_array_equal(b["actions"], b["logits"].argmax(-1))
    _check_all(case, algo, b, tab)


@pytest.mark.parametrize("case", tc.BIG, ids=lambda c: c.id)
def test_fp32_rollout_past_the_tile_switch(case):
    """32,776 lanes: 128-row tiles at 2 and 4 actions; at 8 actions they would need 164,960 B of LDS with the
    100-row table, so the 32-row tiles run.  The last tile is ragged in both.  Forward of the first 4,096 and the
    last 136 lanes, transitions of all lanes."""
    algo, b, tab = _rollout(case, _dev())
    lanes = np.r_[np.arange(tc.BIG_HEAD), np.arange(case.lanes - tc.BIG_TAIL, case.lanes)]
    _check_all(case, algo, b, tab, lanes)


@pytest.mark.parametrize("case", tc.BUDGET, ids=lambda c: c.id)
def test_tables_over_the_fused_budget_run_per_step(case):
    """600 rows x 8 clouds (76,800 B; the persistent kernel would need 173,056 B) and 450 x 8 (57,600 B; the fused
    fp32 step 168,416 B): the per-step forms, whose LDS is the tables alone"""
    from rlks import _lib

    algo, b, tab = _rollout(case, _dev())
    fused = tc.SF16_PERSISTENT if case.prec == "sf16" else tc.FP32_FUSED_32
    assert _lds_bytes(algo.params.desc, fused, case.rows, case.A) > tc.LDS_LIMIT == 163840
    assert _lib.RLKS_ROLLOUT_SF16_PER_STEP == tc.SF16_PER_STEP and _lib.RLKS_ROLLOUT_FP32_PER_STEP == tc.FP32_PER_STEP
    _check_all(case, algo, b, tab)


def test_persistent_rollout_at_exactly_the_lds_limit():
    """split-fp16, 2 actions: the largest table whose persistent launch fits (the row count from the LDS formulas
    and the static bytes the runtime reports) runs persistent on exactly 160 KiB; one row more runs per step.
    The two tables share their rows, so both rollouts see the same observations: each is within the fp32 band
    of the fp64 oracle, and both replay in the oracle env."""
    from rlks import _lib

    d = _dev()
    desc = _lib.MlpDesc(6, tc.H, 2, _lib.RLKS_PRECISION_SF16)
    static = _lds_bytes(desc, tc.SF16_PERSISTENT, 1, 2) - tc.sf_roll_lds(2, 1, 2)
    assert static >= 0
    fit = tc.rows_that_fit(tc.SF16_PERSISTENT, 2, static)
    assert _lds_bytes(desc, tc.SF16_PERSISTENT, fit, 2) == tc.LDS_LIMIT  # exactly the limit
    assert 2 * (fit + 1) * 2 * 8 <= tc.MAX_TABLE_BYTES
    big = tc.table("init", 2, fit + 1)
    runs = []
    for rows, form, tab in ((fit, tc.SF16_PERSISTENT, tc.head_rows(big, fit)), (fit + 1, tc.SF16_PER_STEP, big)):
        case = tc.Case(f"sf16-limit-{tc.FORM_NAMES[form]}", "sf16", 2, "init", form, rows=rows)
        algo, b, _ = _rollout(case, d, tab)
        ref = _check_all(case, algo, b, tab)
        runs.append(b)
    np.testing.assert_array_equal(_bits(runs[0]["obs"]), _bits(runs[1]["obs"]))
    # the same observations and weights: the two forms differ only as two fp32-accurate evaluations do, each
    # no further from the fp64 oracle (one reference: the observations are equal) than close_as_fp32 lets a
    # kernel be from an fp32 evaluation, with the other form standing in for that evaluation
    for a, b, name in ((runs[0], runs[1], "persistent vs per-step"), (runs[1], runs[0], "per-step vs persistent")):
        _report("sf16-limit-" + name.replace(" ", "-"), "logits", a["logits"].reshape(-1, 2), ref[0], b["logits"].reshape(-1, 2))
        _report("sf16-limit-" + name.replace(" ", "-"), "values", a["values"].reshape(-1), ref[1], b["values"].reshape(-1))


def test_over_budget_without_autoreset_is_refused_before_any_launch():
    """600 rows x 8 clouds without autoreset lanes: the persistent kernel does not fit and the per-step form
    needs autoreset, so rlks_rollout_ws returns RLKS_ERR_UNSUPPORTED, naming the bytes, and launches nothing"""
    from rlks import VecK8sMultiCloudEnv, _lib
    from rlks.policy import PolicyParams

    d = _dev()
    A, N, T = 8, tc.N, tc.T
    env = VecK8sMultiCloudEnv(N, table=tc.table("init", A, 600), seed=tc.SEED, autoreset=False, device=d)
    p = PolicyParams(3 * A, tc.H, A, device=d, seed=tc.SEED)
    p.desc.precision = _lib.RLKS_PRECISION_SF16
    wsb = C.c_int64()
    _lib.call("rlks_ppo_workspace_bytes", C.byref(p.desc), 256, C.byref(wsb))
    ws = torch.full((wsb.value,), 0x5A, dtype=torch.uint8, device=d)
    buf, bufs = _buffers(T, N, A, d)
    buf["obs"][0] = env.reset()
    before = {k: v.clone() for k, v in buf.items()}
    torch.cuda.synchronize()
    lib = _lib.lib()
    rc = lib.rlks_rollout_ws(env.dev.handle, C.byref(p.desc), p.flat.data_ptr(), C.byref(bufs), 1, ws.data_ptr(),
                             ws.numel(), None)
    msg = lib.rlks_last_error().decode()
    print("TABLE_ROLLOUT refusal:", msg)
    assert rc == -3, (rc, msg)  # RLKS_ERR_UNSUPPORTED
    assert "173056" in msg and "163840" in msg and "autoreset" in msg
    form = C.c_int32(-1)
    assert lib.rlks_rollout_form(env.dev.handle, C.byref(p.desc), C.byref(bufs), C.byref(form)) == -3
    torch.cuda.synchronize()
    for k, v in buf.items():
        assert torch.equal(v, before[k]), k
    assert bool((ws == 0x5A).all())
    # the same env with a table that fits resolves persistent, as a table env without autoreset always did
    small = VecK8sMultiCloudEnv(N, table=tc.table("init", A, tc.ROWS), seed=tc.SEED, autoreset=False, device=d)
    assert _form(small.dev.handle, p.desc, N, T, tc.SF_ROLL_FUSED_MAX_LANES + 1) == tc.SF16_PERSISTENT


def test_rlks_rollout_decides_from_the_fp32_kernels_it_runs():
    """rlks_rollout runs the fp32 kernels for every fused-width desc, a split-fp16 one included, so its form
    comes from their LDS, not from k_sf_roll's.  450 rows x 8 clouds with a split-fp16 desc: the persistent
    kernel would fit (153,856 B), the fused fp32 step the entry would launch does not (168,416 B).  With
    autoreset lanes the entry runs the fp32 per-step form (parity, oracle replay); without them it refuses before
    any launch.  Past 32,768 lanes the entry keeps its 128-row tiles under a split-fp16 desc: bit for bit the
    rollout it gives under an fp32 desc."""
    from rlks import VecK8sMultiCloudEnv, _lib
    from rlks.policy import PolicyParams

    d = _dev()
    lib = _lib.lib()
    A, N, T = 8, tc.N, tc.T
    tab = tc.table("init", A, 450)
    p = PolicyParams(3 * A, tc.H, A, device=d, seed=tc.SEED)
    tc.apply_regime(p, "init")
    p.desc.precision = _lib.RLKS_PRECISION_SF16
    assert _lds_bytes(p.desc, tc.SF16_PERSISTENT, 450, A) == 153856 <= tc.LDS_LIMIT
    assert _lds_bytes(p.desc, tc.FP32_FUSED_32, 450, A) == 168416 > tc.LDS_LIMIT
    # without autoreset: refused, nothing launched
    env = VecK8sMultiCloudEnv(N, table=tab, seed=tc.SEED, autoreset=False, device=d)
    buf, bufs = _buffers(T, N, A, d)
    buf["obs"][0] = env.reset()
    before = {k: v.clone() for k, v in buf.items()}
    torch.cuda.synchronize()
    rc = lib.rlks_rollout(env.dev.handle, C.byref(p.desc), p.flat.data_ptr(), C.byref(bufs), 1, None)
    msg = lib.rlks_last_error().decode()
    assert rc == -3 and "168416" in msg and "163840" in msg, (rc, msg)
    torch.cuda.synchronize()
    for k, v in buf.items():
        assert torch.equal(v, before[k]), k
    # with autoreset: the fp32 per-step form
    env = VecK8sMultiCloudEnv(N, table=tab, seed=tc.SEED, device=d)
    buf, bufs = _buffers(T, N, A, d)
    buf["obs"][0] = env.reset()
    _lib.call("rlks_rollout", env.dev.handle, C.byref(p.desc), p.flat.data_ptr(), C.byref(bufs), 1, None)
    torch.cuda.synchronize()
    case = tc.Case("rlks_rollout-sf16-desc-per-step-8", "fp32", A, "init", tc.FP32_PER_STEP, rows=450)

    class _Algo:
        params = p

    b = {k: v.cpu().numpy() for k, v in buf.items()}
    _check_all(case, _Algo, b, tab)
    # the same shape through PPO's fp32 path (an fp32 desc) gives the same rollout, bit for bit
    _, ref, _ = _rollout(tc.BUDGET[1], d)
    for k in ("obs", "logits", "values", "actions", "logp", "rewards", "dones"):
        np.testing.assert_array_equal(_bits(b[k]), _bits(ref[k]), err_msg=k)
    # 32,776 lanes, 2 actions, 100 rows: 128-row tiles under either desc
    A, N, T = 2, tc.N_BIG, tc.T_BIG
    tab = tc.table("init", A)
    p = PolicyParams(3 * A, tc.H, A, device=d, seed=tc.SEED)
    tc.apply_regime(p, "init")
    outs = []
    for prec in (_lib.RLKS_PRECISION_SF16, _lib.RLKS_PRECISION_FP32):
        p.desc.precision = prec
        env = VecK8sMultiCloudEnv(N, table=tab, seed=tc.SEED, device=d)
        buf, bufs = _buffers(T, N, A, d)
        buf["obs"][0] = env.reset()
        _lib.call("rlks_rollout", env.dev.handle, C.byref(p.desc), p.flat.data_ptr(), C.byref(bufs), 1, None)
        torch.cuda.synchronize()
        outs.append({k: v.cpu().numpy() for k, v in buf.items()})
    for k in ("obs", "logits", "values", "actions", "logp", "rewards", "dones"):
        np.testing.assert_array_equal(_bits(outs[0][k]), _bits(outs[1][k]), err_msg=k)
    _, ref, _ = _rollout(tc.BIG[0], d)  # PPO's fp32 path at this shape: rlks_rollout_form names the 128-row tiles
    assert tc.BIG[0].form == tc.FP32_FUSED_128 and (tc.BIG[0].A, tc.BIG[0].regime) == (2, "init")
    np.testing.assert_array_equal(_bits(outs[0]["logits"]), _bits(ref["logits"]))


def test_shapes_that_ran_before_resolve_as_they_ran():
    """rlks_rollout_form on the shapes of test_rollout_replays_from_its_logits, of
    test_rollouts_carry_observations_and_sample_exactly and of bench.py's configurations (c3 and c5 with their
    cluster, node and hidden sizes on a few lanes: those forms do not depend on the lane count)"""
    from rlks import VecK8sMultiCloudEnv, _lib
    from rlks.env import NodeSpec
    from rlks.tables import load_table, synthetic_table

    d = _dev()
    SF, FP, WIDE = _lib.RLKS_PRECISION_SF16, _lib.RLKS_PRECISION_FP32, _lib.RLKS_PRECISION_WIDE
    per_step = tc.SF_ROLL_FUSED_MAX_LANES + 1
    rows = [
        # clouds, table rows, nodes, hidden, lanes, job lanes, precision, form
        (2, 4, None, 256, 96, 0, SF, tc.SF16_PERSISTENT),      # table-persistent-2 (and -argmax)
        (8, 4, None, 256, 96, 0, SF, tc.SF16_PERSISTENT),      # table-persistent-8
        (4, 4, None, 256, 96, per_step, SF, tc.SF16_PER_STEP),  # table-per-step-4
        (4, 4, None, 256, 96, 0, FP, tc.FP32_FUSED_32),        # table-fp32-4 (and -argmax)
        (4, 4, None, 384, 136, 0, WIDE, tc.WIDE),              # table-wide-4
        (8, 100, 16, 256, 520, 0, SF, tc.NODE),                # 8-16-256-520-16-8192
        (16, 100, 32, 384, 136, 0, WIDE, tc.WIDE),             # 16-32-384-136-8-1024
        (2, None, None, 256, 4096, 0, SF, tc.SF16_PERSISTENT),  # the agent test's c2 size; bench c2
        (2, None, None, 256, 32768, 0, SF, tc.SF16_PER_STEP),  # the agent test's per-step size
        (2, None, None, 256, 131072, 0, SF, tc.SF16_PER_STEP),  # bench c4
        (2, None, None, 256, 65536, 131072, SF, tc.SF16_PER_STEP),  # bench c4 on two ranks
        (8, 100, 256, 256, 64, 0, SF, tc.NODE),                # bench c3 (65,536 lanes there)
        (64, 100, 1024, 2048, 8, 0, WIDE, tc.WIDE),            # bench c5 (16,384 lanes there)
    ]
    for Cn, nrows, nodes, hid, N, job, prec, want in rows:
        tab = load_table() if nrows is None else synthetic_table(Cn, nrows, seed=7)
        spec = None if nodes is None else NodeSpec(Cn, nodes, arrival_rate=1.0, depart_prob=0.05, init_occupancy=0.5)
        env = VecK8sMultiCloudEnv(N, table=tab, seed=5, nodes=spec, device=d)
        desc = _lib.MlpDesc(3 * Cn, hid, Cn, prec)
        got = _form(env.dev.handle, desc, N, 16, job)
        assert got == want, (Cn, nrows, nodes, hid, N, job, tc.FORM_NAMES.get(got), tc.FORM_NAMES[want])
        del env
