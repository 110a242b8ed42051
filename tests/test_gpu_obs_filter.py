"""GPU tests of observation_filter="MeanStdFilter" (rlks_obs_filter_*, rlks_rollout_filtered, PPO; DESIGN.md
§21) against the numpy restatement tests/obs_filter_ref.py.

Tolerances (derived there, not tuned): apply bit-equal; the record within sum_bound(rows, sum|term|) per
slot; the merge, given the device's own record, within 8 u (|mean| + |delta|) / 16 u (m2 + s2 + |s1 delta| +
delta^2 na nb / n) / 8 u inv; a whole state against two-pass numpy within the bound propagated from those,
after a non-vacuity check.  Everything a rollout stores is compared bit for bit, except the forward's
logits and values, which are held to tests/parity.close_as_fp32 against the fp64 oracle."""
import ctypes as C_
import functools

import numpy as np
import pytest

import obs_filter_ref as R
import oracle
from parity import close_as_fp32
from rollout_metrics_ref import sum_bound

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

# csrc/workspace.h: above this many lanes the unfiltered split-fp16 table rollout runs the per-step kernels
SF_ROLL_FUSED_MAX_LANES = 16384
# csrc/obs_filter.hip: columns at most; stats: floats per workgroup, workgroups at most
OF_MAX_D, OF_PART_MIN_FLOATS, OF_PART_MAX_BLOCKS = 512, 16384, 1024

# beyond the issue's shapes: more partial records than stage two has chunk threads (64), and the grid caps
# of both kernels (1,024 stats workgroups; 2,048 apply workgroups x 1,024 floats)
GRID_CASES = {"blocks_69": (70001, 16), "grid_cap": (1048579, 17)}
ALL_CASES = {**R.CASES, **GRID_CASES}


def _dev():
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    return torch.device("cuda", 0)


def _lib():
    from rlks import _lib

    return _lib


@functools.lru_cache(maxsize=None)
def _case(name):
    """(x, state the case runs under): the state is merged (on the host) from another draw of the same
    data, so K is close to the columns' means: ~1000 on the offset column"""
    rows, D = ALL_CASES[name]
    off = name == "offset"
    x = R.case_data(rows, D, seed=21, offset=off)
    st, _, _ = R.chain([R.case_data(max(rows // 2, 3), D, seed=22, offset=off)])
    x.setflags(write=False)
    return x, st


def _put(a, d, shift=0):
    """a on the device, `shift` elements past a 16-byte boundary"""
    src = torch.from_numpy(np.array(a).ravel())  # (a copy: the cached cases are read-only)
    flat = torch.zeros(src.numel() + shift, dtype=src.dtype, device=d)
    assert flat.data_ptr() % 16 == 0
    flat[shift:] = src.to(d)
    return flat[shift:]


def _apply(state_t, x_t, y_t, rows, D):
    _lib().call("rlks_obs_filter_apply", state_t.data_ptr(), x_t.data_ptr(), y_t.data_ptr(), rows, D, None)


def _stats(state_t, x_t, rows, D, repeat=1):
    L = _lib()
    wsb = C_.c_int64()
    L.call("rlks_obs_filter_workspace_bytes", rows, D, C_.byref(wsb))
    nb = min(OF_PART_MAX_BLOCKS, max(1, -(-rows * D // OF_PART_MIN_FLOATS)))
    assert wsb.value == nb * 2 * D * 8
    ws = torch.empty(wsb.value // 8, dtype=torch.float64, device=x_t.device)
    outs = []
    for _ in range(repeat):
        ws.fill_(float("nan"))  # the workspace carries nothing from call to call
        rec = torch.full((1 + 2 * D,), float("nan"), dtype=torch.float64, device=x_t.device)
        L.call("rlks_obs_filter_stats", state_t.data_ptr(), x_t.data_ptr(), rows, D, rec.data_ptr(), ws.data_ptr(),
               wsb.value, None)
        outs.append(rec)
    return outs


# ----------------------------------------------------------------------------- kernels
def test_state_layout_and_init():
    L = _lib()
    d = _dev()
    for D in (1, 6, 288, OF_MAX_D):
        size = L.lib().rlks_obs_filter_size(D)
        assert size == 1 + 3 * D == L.RLKS_OF_VECS + L.RLKS_OF_NVEC * D
        s = torch.full((size,), float("nan"), dtype=torch.float64, device=d)
        L.call("rlks_obs_filter_init", s.data_ptr(), D, None)
        assert s.cpu().numpy().tobytes() == R.pack(R.fresh(D)).tobytes()


@pytest.mark.parametrize("name", list(ALL_CASES))
def test_apply_is_bit_equal(name):
    """out of place, in place, and from pointers 4 bytes past a 16-byte boundary (the 4-byte path)"""
    d = _dev()
    x, st = _case(name)
    rows, D = x.shape
    state = _put(R.pack(st), d)
    want = R.apply(st, x)
    for shift in (0, 1):
        xt = _put(x, d, shift)
        yt = _put(np.full(x.size, np.nan, np.float32), d, shift)
        _apply(state, xt, yt, rows, D)
        assert yt.cpu().numpy().tobytes() == want.tobytes(), (name, shift, "out of place")
        assert xt.cpu().numpy().tobytes() == x.tobytes()
        _apply(state, xt, xt, rows, D)
        assert xt.cpu().numpy().tobytes() == want.tobytes(), (name, shift, "in place")
    assert state.cpu().numpy().tobytes() == R.pack(st).tobytes()  # read, never written


@pytest.mark.parametrize("name", list(R.CASES))
def test_fresh_state_is_the_identity(name):
    d = _dev()
    x, _ = _case(name)
    x = x.copy()
    x.ravel()[::7] *= -1
    x.ravel()[0] = -0.0
    rows, D = x.shape
    state = _put(R.pack(R.fresh(D)), d)
    xt = _put(x, d)
    yt = torch.full_like(xt, float("nan"))
    _apply(state, xt, yt, rows, D)
    assert yt.cpu().numpy().tobytes() == x.tobytes()
    _apply(state, xt, xt, rows, D)
    assert xt.cpu().numpy().tobytes() == x.tobytes()


@pytest.mark.parametrize("name", list(ALL_CASES))
def test_stats_within_bound_and_reproducible(name):
    d = _dev()
    x, st = _case(name)
    rows, D = x.shape
    state = _put(R.pack(st), d)
    a, b = (r.cpu().numpy() for r in _stats(state, _put(x, d), rows, D, repeat=2))
    assert a.tobytes() == b.tobytes()
    n, s1, s2, ab1, ab2 = R.record(x, st[1])
    assert a[0] == n == rows
    e1, e2 = np.abs(a[1:1 + D] - s1), np.abs(a[1 + D:] - s2)
    print(f"{name}: max err / bound s1 {np.max(e1 / np.maximum(R.record_bound(rows, ab1), 1e-300)):.3g} "
          f"s2 {np.max(e2 / np.maximum(R.record_bound(rows, ab2), 1e-300)):.3g}")
    assert (e1 <= R.record_bound(rows, ab1)).all(), (name, "s1")
    assert (e2 <= R.record_bound(rows, ab2)).all(), (name, "s2")
    if name == "offset":  # K ~ 1000: the shifted sums are those of the 1e-3 noise
        assert abs(st[1][0] - 1000.0) < 1e-3 and a[1 + D] < rows * 1e-4


def test_stats_of_no_rows_is_a_record_of_zeros():
    d = _dev()
    _, st = _case("odd_255")
    state = _put(R.pack(st), d)
    x = torch.zeros(8, device=d)
    rec = _stats(state, x, 0, 6)[0].cpu().numpy()
    assert rec.tobytes() == np.zeros(13).tobytes()


@pytest.mark.parametrize("start", ["fresh", "merged"])
@pytest.mark.parametrize("name", list(R.CASES))
def test_merge_within_bounds(name, start):
    """the device merges its own record; the reference merges that same record"""
    L = _lib()
    d = _dev()
    x, st = _case(name)
    rows, D = x.shape
    if start == "fresh":
        st = R.fresh(D)
    state = _put(R.pack(st), d)
    rec = _stats(state, _put(x, d), rows, D)[0]
    L.call("rlks_obs_filter_merge", state.data_ptr(), rec.data_ptr(), D, None)
    n, mean, m2, inv = R.unpack(state.cpu().numpy())
    r = rec.cpu().numpy()
    host_rec = (r[0], r[1:1 + D], r[1 + D:])
    en, emean, em2, _ = R.merge(st, host_rec)
    tm, t2 = R.merge_bounds(st, host_rec)
    assert n == en == st[0] + rows
    assert (np.abs(mean - emean) <= tm).all(), (name, np.abs(mean - emean).max())
    assert (np.abs(m2 - em2) <= t2).all(), (name, np.abs(m2 - em2).max())
    assert (m2 >= 0).all() and np.isfinite(inv).all()
    assert (np.abs(inv - R.inv_of(n, m2)) <= R.inv_bound(inv)).all(), name
    if n < 2:
        assert (inv == 1.0).all()
    # rows = 0: a no-op
    before = state.cpu().numpy().tobytes()
    zero = torch.zeros(1 + 2 * D, dtype=torch.float64, device=d)
    L.call("rlks_obs_filter_merge", state.data_ptr(), zero.data_ptr(), D, None)
    assert state.cpu().numpy().tobytes() == before


def test_bad_arguments_are_refused():
    """argument errors only: RLKS_ERR_ARG (-1), and the outputs keep their sentinel"""
    L = _lib()
    lib = L.lib()
    d = _dev()
    D = 6
    assert lib.rlks_obs_filter_size(0) == -1 and lib.rlks_obs_filter_size(OF_MAX_D + 1) == -1
    assert lib.rlks_obs_filter_size(384) == 1 + 3 * 384  # the bound is at least 384
    state = _put(R.pack(R.fresh(D)), d)
    x = torch.ones(4 * D, device=d)
    y = torch.full((4 * D,), 7.0, device=d)
    rec = torch.full((1 + 2 * D,), 7.0, dtype=torch.float64, device=d)
    ws = torch.zeros(2 * D, dtype=torch.float64, device=d)
    big = _put(R.pack(R.fresh(OF_MAX_D + 1)), d)
    S, X, Y, RC, W = state.data_ptr(), x.data_ptr(), y.data_ptr(), rec.data_ptr(), ws.data_ptr()
    bad = [
        lib.rlks_obs_filter_init(None, D, None), lib.rlks_obs_filter_init(S, 0, None),
        lib.rlks_obs_filter_apply(None, X, Y, 4, D, None), lib.rlks_obs_filter_apply(S, None, Y, 4, D, None),
        lib.rlks_obs_filter_apply(S, X, None, 4, D, None), lib.rlks_obs_filter_apply(S, X, Y, -1, D, None),
        lib.rlks_obs_filter_apply(big.data_ptr(), X, Y, 0, OF_MAX_D + 1, None),
        lib.rlks_obs_filter_workspace_bytes(4, D, None), lib.rlks_obs_filter_workspace_bytes(-1, D, C_.byref(C_.c_int64())),
        lib.rlks_obs_filter_stats(None, X, 4, D, RC, W, 2 * D * 8, None),
        lib.rlks_obs_filter_stats(S, None, 4, D, RC, W, 2 * D * 8, None),
        lib.rlks_obs_filter_stats(S, X, 4, D, None, W, 2 * D * 8, None),
        lib.rlks_obs_filter_stats(S, X, 4, D, RC, None, 2 * D * 8, None),
        lib.rlks_obs_filter_stats(S, X, -1, D, RC, W, 2 * D * 8, None),
        lib.rlks_obs_filter_stats(S, X, 4, D, RC, W, 2 * D * 8 - 1, None),  # workspace too small
        lib.rlks_obs_filter_merge(None, RC, D, None), lib.rlks_obs_filter_merge(S, None, D, None),
        lib.rlks_obs_filter_merge(S, RC, OF_MAX_D + 1, None),
    ]
    assert bad == [-1] * len(bad), bad
    torch.cuda.synchronize()
    assert bool((y == 7.0).all()) and bool((rec == 7.0).all())
    assert state.cpu().numpy().tobytes() == R.pack(R.fresh(D)).tobytes()
    # rlks_rollout_filtered without a state or a raw buffer
    algo = _make("a", filtered=True)
    args = (algo.env.handle, C_.byref(algo.params.desc), algo.params.flat.data_ptr(), C_.byref(algo.bufs), 1,
            algo.ws.data_ptr(), algo.ws.numel())
    assert lib.rlks_rollout_filtered(*args, None, algo.raw.data_ptr(), None) == -1
    assert lib.rlks_rollout_filtered(*args, algo.obs_filter.state.data_ptr(), None, None) == -1
    algo.stop()


# ----------------------------------------------------------------------------- rollouts
N_LANES = 256
PATHS = {"a": 16, "b": 16, "c": 16, "d": 8, "e": 8}  # path -> T
SEED = 11


def _setup(path):
    """(table or None, NodeSpec or None) of a rollout path"""
    from rlks.env import NodeSpec
    from rlks.tables import synthetic_table

    if path == "d":  # node env on the fused 256-unit kernels: node_rollout
        return synthetic_table(4, 100, seed=3), NodeSpec(4, 16, arrival_rate=2.0, depart_prob=0.05, reject_penalty=0.1)
    if path == "e":  # tests/node_regimes.py regime A's spec: 3 clusters are no fused shape, wide_rollout
        return synthetic_table(3, 100, seed=7), NodeSpec(3, 16, node_cpu_m=[2000] * 3, node_mem_mi=[1024, 4096, 1024],
                                                         arrival_rate=8.0, depart_prob=0.02, init_occupancy=0.9,
                                                         reject_penalty=0.25)
    return None, None


def _make(path, filtered, epochs=2, **kw):
    from rlks.ppo import PPO, PPOConfig

    T = PATHS[path]
    train = dict(train_batch_size=N_LANES * T, sgd_minibatch_size=256, num_sgd_iter=epochs, lr=3e-4, gamma=0.99)
    if path == "b":
        train["sgd_precision"] = "fp32"
    if path == "c":
        train["model"] = {"fcnet_hiddens": [64, 64]}
    cfg = PPOConfig().environment("K8sMultiCloudEnv").framework("torch").training(**train).debugging(seed=SEED)
    if filtered:
        cfg.rollouts(observation_filter="MeanStdFilter")
    cfg.num_envs = N_LANES
    cfg.rollout_fragment_length = T
    cfg.table, cfg.nodes = _setup(path)
    for k, v in kw.items():
        setattr(cfg, k, v)
    algo = PPO(config=cfg, device=_dev())
    assert algo.precision == {"a": "sf16", "b": "fp32", "c": "wide", "d": "sf16", "e": "wide"}[path]
    assert (algo.obs_filter is not None) == filtered and algo.T == T
    return algo


def _host(algo):
    b = {k: v.cpu().numpy() for k, v in algo.buf.items()}
    if algo.raw is not None:
        b["raw"] = algo.raw.cpu().numpy()
    return b


@functools.lru_cache(maxsize=None)
def _two_rollouts(path):
    """two PPO.rollout() calls of a filtered algorithm, an SGD update between them, and the first
    rollout of its unfiltered twin: host copies, never written again"""
    f, u = _make(path, True), _make(path, False)
    if path == "a":  # the twin on the per-step kernels too, which a filtered rollout always takes
        u.bufs.global_lanes = SF_ROLL_FUSED_MAX_LANES + 1
    out = {"flat": [], "state": [], "host": []}
    u.rollout(explore=True)
    out["twin"] = _host(u)
    for it in range(2):
        if it:
            f.advantages()
            f.update()
            f.iteration += 1
        out["state"].append(f.obs_filter.numpy())   # what this rollout filters with
        out["flat"].append(f.params.flat.cpu().numpy())
        f.rollout(explore=True)
        out["host"].append(_host(f))
    out["state"].append(f.obs_filter.numpy())
    out["offsets"], out["dims"] = list(f.params.offsets), (f.D, f.H, f.A)
    f.stop()
    u.stop()
    return out


@pytest.mark.parametrize("path", list(PATHS))
def test_fresh_filter_rollout_equals_the_unfiltered_one(path):
    run = _two_rollouts(path)
    b, t = run["host"][0], run["twin"]
    n, mean, m2, inv = run["state"][0]
    assert n == 0 and not mean.any() and not m2.any() and (inv == 1).all()
    for k in ("obs", "logits", "values", "actions", "logp", "rewards", "dones"):
        assert b[k].tobytes() == t[k].tobytes(), (path, k)
    assert b["raw"].tobytes() == b["obs"].tobytes()
    assert len(np.unique(b["actions"])) == run["dims"][2]  # the policy explores every action


@pytest.mark.parametrize("path", list(PATHS))
def test_filtered_rollout_with_a_merged_state(path):
    """the second rollout: obs = apply(state, raw) bit for bit, the raw transitions are the env's own
    (replayed from the first step of the first rollout), logits and values are the forward of the
    filtered observations"""
    from test_gpu_agent import _oracle_env, _start, replay

    run = _two_rollouts(path)
    T = PATHS[path]
    D, H, A = run["dims"]
    st = run["state"][1]
    assert st[0] == (T + 1) * N_LANES and st[2].any()
    b = run["host"][1]
    for t in range(T + 1):
        assert R.apply(st, b["raw"][t]).tobytes() == b["obs"][t].tobytes(), (path, t)
    assert b["raw"].tobytes() != b["obs"].tobytes()
    tab, spec = _setup(path)
    if spec is None:
        ora = _start(_oracle_env(N_LANES, SEED))
        for h in run["host"]:
            n, amb, _ = replay(ora, {**h, "obs": h["raw"]}, SEED)
            assert amb <= 1e-3 * n
    else:
        from rlks import VecK8sMultiCloudEnv

        twin = VecK8sMultiCloudEnv(N_LANES, table=tab, seed=SEED, nodes=spec, device=_dev())
        obs = twin.reset()
        assert obs.cpu().numpy().tobytes() == run["host"][0]["raw"][0].tobytes()
        for h in run["host"]:
            for t in range(T):
                obs, r, term, _, _ = twin.step(torch.from_numpy(h["actions"][t]).to(twin.device))
                assert obs.cpu().numpy().tobytes() == h["raw"][t + 1].tobytes(), (path, t)
                assert r.to(torch.float32).cpu().numpy().tobytes() == h["rewards"][t].tobytes(), (path, t)
                assert term.cpu().numpy().tobytes() == h["dones"][t].tobytes(), (path, t)
        twin.check_status()
        twin.close()
    flat, off = run["flat"][1], run["offsets"]
    for t in (0, 1, T):
        x = b["obs"][t]
        el, ev = oracle.mlp_forward(flat, off, D, H, A, x)
        fl, fv = oracle.mlp_forward_fp32_band(flat, off, D, H, A, x)
        close_as_fp32(b["values"][t], ev[:, 0] if ev.ndim == 2 else ev, [v[:, 0] if v.ndim == 2 else v for v in fv],
                      what=f"{path} values[{t}]")
        if t < T:
            close_as_fp32(b["logits"][t], el, fl, what=f"{path} logits[{t}]")


@pytest.mark.parametrize("path", list(PATHS))
def test_two_consecutive_rollouts_carry_raw_and_count_every_row_once(path):
    run = _two_rollouts(path)
    T = PATHS[path]
    D = run["dims"][0]
    h1, h2 = run["host"]
    assert h2["raw"][0].tobytes() == h1["raw"][T].tobytes()
    assert h2["obs"][0].tobytes() == R.apply(run["state"][1], h2["raw"][0]).tobytes()
    final = run["state"][2]
    assert final[0] == (T + 1) * N_LANES + T * N_LANES
    batches = [h1["raw"].reshape(-1, D), h2["raw"][1:].reshape(-1, D)]
    R.check_whole_state(run["state"][1], (T + 1) * N_LANES, batches[:1], f"{path} first")
    R.check_whole_state(final, (2 * T + 1) * N_LANES, batches, f"{path} both")


def test_sgd_side_is_untouched():
    """a filtered algorithm's buffers, parameters, Adam state and dyn in an unfiltered twin: advantages()
    and update() leave bit-equal parameters and moments"""
    f, u = _make("a", True), _make("a", False)
    f.rollout()
    f.advantages()
    f.update()
    f.iteration += 1
    f.rollout()  # a rollout under a merged state: buf["obs"] is filtered
    assert not torch.equal(f.raw, f.buf["obs"])
    for k in f.buf:
        u.buf[k].copy_(f.buf[k])
    for a, b in ((u.params.flat, f.params.flat), (u.adam_m, f.adam_m), (u.adam_v, f.adam_v), (u.dyn, f.dyn)):
        a.copy_(b)
    u.adam_step, u.iteration, u._fused_prev = f.adam_step, f.iteration, False
    f._fused_prev = False
    for algo in (f, u):
        algo.advantages()
        algo.update()
    for a, b in ((u.params.flat, f.params.flat), (u.adam_m, f.adam_m), (u.adam_v, f.adam_v), (u.dyn, f.dyn),
                 (u.stats, f.stats)):
        assert torch.equal(a, b)
    f.stop()
    u.stop()


@pytest.mark.parametrize("path", ["a", "e"])
def test_train_two_iterations(path):
    T = PATHS[path]
    on = _make(path, True, rollout_metrics=True)
    C = on.A
    for it in range(2):
        res = on.train()
        pol = res["info"]["learner"]["default_policy"]
        assert all(np.isfinite(v) for v in pol["learner_stats"].values()), pol["learner_stats"]
        of = pol["obs_filter"]
        assert of["count"] == ((it + 1) * T + 1) * N_LANES and len(of["mean"]) == len(of["std"]) == on.D
        n, mean, m2, _ = on.obs_filter.numpy()
        assert of["mean"] == list(mean) and np.allclose(of["std"], np.sqrt(m2 / (n - 1)), rtol=1e-15)
        raw = on.raw.cpu().numpy()
        util = raw[:T, :, 2 * C:].astype(np.float64).reshape(T * N_LANES, C)
        for c in range(C):  # the metrics read the raw buffer: a utilisation, not a standardised one
            got = res["custom_metrics"]["utilisation_mean"][c]
            assert abs(got - util[:, c].mean()) <= 2 * sum_bound(T * N_LANES, np.abs(util[:, c]).mean()), (path, c)
            assert 0.0 <= got <= 1.0
    assert not torch.equal(on.raw, on.buf["obs"])
    on.stop()
    # the knob off: explicit "NoFilter" and the default config train alike, nothing new is allocated
    off, dflt = _make(path, False, observation_filter="NoFilter"), _make(path, False)
    assert off.obs_filter is None and off.raw is None and off.raw_bufs is None and off.params.obs_filter is None
    for _ in range(2):
        r1, r2 = off.train(), dflt.train()
        assert "obs_filter" not in r1["info"]["learner"]["default_policy"]
        assert r1["info"]["learner"]["default_policy"]["learner_stats"] == r2["info"]["learner"]["default_policy"][
            "learner_stats"]
    for a, b in ((off.params.flat, dflt.params.flat), (off.adam_m, dflt.adam_m), (off.adam_v, dflt.adam_v),
                 (off.buf["obs"], dflt.buf["obs"])):
        assert torch.equal(a, b)
    off.stop()
    dflt.stop()


@pytest.mark.parametrize("path", ["a", "e"])
def test_serving_filters_and_never_updates(path):
    from rlks.policy import PolicyParams

    f = _make(path, True)
    f.train()
    f.rollout()
    before = f.obs_filter.state.cpu().numpy().tobytes()
    st = f.obs_filter.numpy()
    raw = f.current_obs()
    assert raw.data_ptr() == f.raw[f.T].data_ptr()
    # the same weights without a filter, fed the filtered rows
    p = PolicyParams(f.D, f.H, f.A, device=f.device, seed=0)
    p.flat.copy_(f.params.flat)
    p.desc.precision = f.params.desc.precision
    rows = raw.cpu().numpy()
    filtered = torch.from_numpy(R.apply(st, rows)).to(f.device)
    for i in (0, 1, 100, 255):
        lg, _ = p.forward(filtered[i:i + 1])
        assert f.compute_single_action(rows[i], explore=False) == int(lg.argmax(1).item())
    lg, _ = p.forward(filtered)
    assert np.array_equal(f.compute_actions(raw, explore=False).cpu().numpy(), lg.argmax(1).cpu().numpy())
    ev = f.evaluate(episodes=4)
    assert np.isfinite(ev["episode_reward_mean"])
    assert f.obs_filter.state.cpu().numpy().tobytes() == before
    f.stop()


def test_checkpoint_resume_is_exact_and_mismatch_raises(tmp_path):
    from rlks.ppo import PPO

    a = _make("a", True)
    a.train()
    path = a.save(tmp_path)
    a.train()
    b = PPO.from_checkpoint(path, device=_dev())
    assert b.obs_filter is not None and b.config.observation_filter == "MeanStdFilter"
    b.train()
    for x, y in ((a.params.flat, b.params.flat), (a.adam_m, b.adam_m), (a.adam_v, b.adam_v),
                 (a.obs_filter.state, b.obs_filter.state), (a.raw, b.raw), (a.buf["obs"], b.buf["obs"]),
                 (a.buf["actions"], b.buf["actions"])):
        assert torch.equal(x, y)
    assert a.obs_filter.numpy()[0] == (2 * PATHS["a"] + 1) * N_LANES
    # across a filter mismatch, either way
    plain = _make("a", False)
    with pytest.raises(ValueError, match="observation filter"):
        plain.restore(path)
    plain.train()
    p2 = plain.save(tmp_path / "plain")
    with pytest.raises(ValueError, match="observation filter"):
        a.restore(p2)
    for algo in (a, b, plain):
        algo.stop()
