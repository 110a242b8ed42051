"""GPU tests of the per-iteration rollout metrics (rlks_rollout_metrics, PPOConfig.reporting(
rollout_metrics=True)): the kernel against the numpy f64 restatement on synthetic
buffers, its determinism, and train()'s result["custom_metrics"] end to end on a table env and on a
node-level env, beside a twin with the flag off.

Tolerance (tests/rollout_metrics_ref.py sum_bound, derived, not tuned): counts, ROWS, DONES, min and max
bit-equal; each sum within 2 n 2^-53 sum|x| of the reference: n 2^-53 sum|x| bounds f64 summation of n
terms in any order, doubled for the reference's own rounding."""
import ctypes as C_
import json

import numpy as np
import pytest

from rollout_metrics_ref import check_record, reference, sum_bound

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

# the kernel's grid bound (csrc/rollout_metrics.hip): RM_MAX_BLOCKS = 1024 workgroups x RM_TILE = 1024
# samples: one pass of the full grid covers 1,048,576 samples
GRID_BLOCKS, GRID_PASS = 1024, 1024 * 1024


def _dev():
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    return torch.device("cuda", 0)


def _buffers(seed, T, N, A, C, extreme=None, dones=None):
    """seeded host buffers: negative and large rewards (+-5,000 among N(0, 50)), values near the returns'
    scale; extreme = "first" / "last" puts the one largest |reward| into that sample"""
    rng = np.random.default_rng(seed)
    n = T * N
    rewards = (rng.standard_normal(n) * 50).astype(np.float32)
    if extreme is None:
        rewards[rng.integers(0, n, min(n, 6))] = np.array([5000, -5000, 4765, -4765, 0.0, -0.0], np.float32)[:min(n, 6)]
    else:
        rewards[0 if extreme == "first" else n - 1] = np.float32(-5000.0 if extreme == "first" else 5000.0)
    values = (rng.standard_normal((T + 1, N)) * 300 + 2000).astype(np.float32)
    vtarg = (values[:T] + (rng.standard_normal((T, N)) * 200).astype(np.float32)).astype(np.float32)
    d = (rng.random((T, N)) < 0.1).astype(np.uint8) if dones is None else np.full((T, N), dones, np.uint8)
    if dones is None and n > 2:
        d.ravel()[rng.integers(0, n)] = 255  # any non-zero byte is a done
    return dict(actions=rng.integers(0, A, (T, N)).astype(np.int32), rewards=rewards.reshape(T, N), values=values,
                vtarg=vtarg, dones=d, obs=rng.random((T + 1, N, 3 * C)).astype(np.float32))


def _run(b, A, C, shift=0, repeat=1):
    """the kernel on host buffers -> `repeat` records (numpy).  shift: every array starts `shift`
    elements into its allocation, so the 16-byte groups start after a scalar head of 4 - shift samples"""
    from rlks import _lib

    d = _dev()
    T, N = b["rewards"].shape

    def put(x, sh):
        src = torch.from_numpy(np.ascontiguousarray(x).ravel())
        flat = torch.zeros(src.numel() + sh, dtype=src.dtype, device=d)
        assert flat.data_ptr() % 16 == 0
        flat[sh:] = src.to(d)
        return flat[sh:]

    # the done bytes one further: past the scalar head they are then no aligned dword
    t = {k: put(v, shift + 1 if shift and k == "dones" else shift) for k, v in b.items()}
    # logits, logp and adv are not read: no buffers
    bufs = _lib.RolloutBufs(t["obs"].data_ptr(), None, t["values"].data_ptr(), t["actions"].data_ptr(), None,
                            t["rewards"].data_ptr(), t["dones"].data_ptr(), None, t["vtarg"].data_ptr(), T, N, N)
    size = _lib.lib().rlks_rollout_metrics_size(A, C)
    assert size == _lib.RLKS_RM_FIXED + A + C
    wsb = C_.c_int64()
    _lib.call("rlks_rollout_metrics_workspace_bytes", T, N, A, C, C_.byref(wsb))
    assert wsb.value == min(GRID_BLOCKS, -(-T * N // 1024)) * size * 8
    ws = torch.empty(wsb.value // 8, dtype=torch.float64, device=d)
    outs = []
    for _ in range(repeat):
        ws.fill_(float("nan"))  # the workspace carries nothing from call to call
        out = torch.full((size,), float("nan"), dtype=torch.float64, device=d)
        _lib.call("rlks_rollout_metrics", C_.byref(bufs), 3 * C, A, C, out.data_ptr(), ws.data_ptr(), wsb.value, None)
        outs.append(out.cpu().numpy())
    return outs


# T, N, A, C: the smallest shapes at which each mechanism can fail
SHAPES = {
    "single": (1, 1, 2, 2),
    "head_tail": (3, 130, 2, 2),      # T N = 390: not a multiple of 4 or of 64; 8-byte loads of the 2 columns
    "odd_rows": (5, 67, 8, 8),        # odd N: rows start at unaligned offsets; the 8-counter limit; 16-byte column loads
    "wide": (7, 64, 96, 96),          # more actions than a wave has lanes, D = 288: LDS histogram, column sums
    "wide_a_only": (6, 33, 9, 3),     # the first A past the register counters; odd C: 4-byte column loads
    "wide_c_only": (4, 70, 4, 9),     # the first C past the register sums, with register counters
    "ragged_chunks": (75, 4100, 2, 2),  # 301 records: stage two's chunks of 2, the last one of 1
    "strided": (129, 8192, 2, 2),    # T N = 1,056,768 > GRID_PASS: workgroups take a second pass; 1,024 records
}


@pytest.mark.parametrize("name", list(SHAPES))
def test_kernel_matches_reference(name):
    T, N, A, C = SHAPES[name]
    assert name != "strided" or GRID_PASS < T * N < GRID_PASS + GRID_PASS // 64
    b = _buffers(11, T, N, A, C)
    ref, ab = reference(**b, A=A, C=C)
    check_record(_run(b, A, C)[0], ref, ab, A, name)


@pytest.mark.parametrize("shift", [1, 2, 3])
def test_kernel_with_a_scalar_head(shift):
    """buffers that start 4, 8 or 12 bytes past a 16-byte boundary: a scalar head of 3, 2 or 1 samples,
    and done bytes that are no aligned dword"""
    T, N, A, C = 3, 130, 2, 2
    b = _buffers(12, T, N, A, C)
    ref, ab = reference(**b, A=A, C=C)
    check_record(_run(b, A, C, shift=shift)[0], ref, ab, A, f"shift {shift}")


@pytest.mark.parametrize("case", ["first", "last", "dones0", "dones1"])
def test_kernel_edge_values(case):
    """the extreme reward in the very first / very last sample; dones all 0 / all 1"""
    from rlks import _lib

    T, N, A, C = 3, 130, 2, 2
    kw = {"extreme": case} if case in ("first", "last") else {"dones": int(case[-1])}
    b = _buffers(13, T, N, A, C, **kw)
    ref, ab = reference(**b, A=A, C=C)
    got = _run(b, A, C)[0]
    check_record(got, ref, ab, A, case)
    if case == "first":
        assert got[_lib.RLKS_RM_REWARD_MIN] == -5000.0 == b["rewards"].ravel()[0]
    elif case == "last":
        assert got[_lib.RLKS_RM_REWARD_MAX] == 5000.0 == b["rewards"].ravel()[-1]
    else:
        assert got[_lib.RLKS_RM_DONES] == (0 if case == "dones0" else T * N)


@pytest.mark.parametrize("name", ["strided", "wide"])
def test_kernel_is_deterministic(name):
    T, N, A, C = SHAPES[name]
    a, b = _run(_buffers(14, T, N, A, C), A, C, repeat=2)
    assert a.tobytes() == b.tobytes()


def test_bad_arguments_are_refused():
    from rlks import _lib

    lib = _lib.lib()
    assert lib.rlks_rollout_metrics_size(0, 2) == -1 and lib.rlks_rollout_metrics_size(2, 0) == -1
    assert lib.rlks_rollout_metrics_size(4097, 2) == -3 and lib.rlks_rollout_metrics_size(2, 1025) == -3
    d = _dev()
    x = torch.zeros(64, device=d)
    bufs = _lib.RolloutBufs(x.data_ptr(), None, x.data_ptr(), x.data_ptr(), None, x.data_ptr(), x.data_ptr(), None,
                            x.data_ptr(), 1, 4, 4)
    out = torch.zeros(14, dtype=torch.float64, device=d)
    ws = torch.zeros(14, dtype=torch.float64, device=d)
    with pytest.raises(_lib.RlksError):  # an obs row of 5 columns cannot hold 3 C = 6
        _lib.call("rlks_rollout_metrics", C_.byref(bufs), 5, 2, 2, out.data_ptr(), ws.data_ptr(), 14 * 8, None)
    with pytest.raises(_lib.RlksError):  # workspace too small
        _lib.call("rlks_rollout_metrics", C_.byref(bufs), 6, 2, 2, out.data_ptr(), ws.data_ptr(), 13 * 8, None)
    torch.cuda.synchronize()


# ----------------------------------------------------------------------------- end to end
def _host(agent):
    return {k: agent.buf[k].cpu().numpy() for k in ("actions", "rewards", "values", "vtarg", "dones", "obs")}


def _close_metrics(got, ref_rec, ab, A, C):
    """custom_metrics against summarise(reference record): integers and min / max equal, means within the
    sums' bound over n, the explained variance within what those bounds leave of it"""
    from rlks import _lib as L
    from rlks.rollout_metrics import summarise

    exp = summarise(ref_rec, A, C)
    n = ref_rec[L.RLKS_RM_ROWS]
    tol = {s: sum_bound(n, ab[s]) for s in range(len(ref_rec))}
    for k in ("reward_min", "reward_max", "dones", "action_count", "action_share"):
        assert got[k] == exp[k], k
    for k, s in (("reward_mean", L.RLKS_RM_REWARD_SUM), ("value_mean", L.RLKS_RM_VALUE_SUM),
                 ("vtarg_mean", L.RLKS_RM_VTARG_SUM)):
        assert abs(got[k] - exp[k]) <= 2 * tol[s] / n, k  # 2x: the division's own rounding is far below
    for c in range(C):
        assert abs(got["utilisation_mean"][c] - exp["utilisation_mean"][c]) <= 2 * tol[L.RLKS_RM_FIXED + A + c] / n

    def var_and_tol(sq, s):
        # Var = sq / n - (s / n)^2: an error e_sq in sq and e_s in s moves it by at most
        # e_sq / n + 2 |mean| e_s / n + (e_s / n)^2
        m = ref_rec[s] / n
        return ref_rec[sq] / n - m * m, tol[sq] / n + 2 * abs(m) * tol[s] / n + (tol[s] / n) ** 2

    vt, et = var_and_tol(L.RLKS_RM_VTARG_SQ, L.RLKS_RM_VTARG_SUM)
    vr, er = var_and_tol(L.RLKS_RM_RESID_SQ, L.RLKS_RM_RESID_SUM)
    assert vt > 100 * et  # the batch's value targets do vary
    # 1 - vr / vt to first order in the two errors, doubled for the higher orders and the roundings
    assert abs(got["vf_explained_var_rollout"] - exp["vf_explained_var_rollout"]) <= 2 * (er + vr / vt * et) / vt
    return exp


def _same(a, b):
    return a == b or (a != a and b != b)


def test_train_reports_custom_metrics_table_env(tmp_path):
    """the smallest PPO the fused path takes (256 lanes, 256-row minibatches, 2 SGD iterations), two
    train() calls; 50-step fragments so that the second call ends the lanes' 99-step episodes.  Also
    the JSON line, and a twin with the flag off: the same training, no new key"""
    from rlks import _lib
    from rlks.ppo import PPO, PPOConfig
    from rlks.rollout_metrics import summarise

    d = _dev()
    N, T = 256, 50

    def make(flag):
        cfg = (PPOConfig().framework("torch")
               .training(train_batch_size=N * T, sgd_minibatch_size=256, num_sgd_iter=2, lr=3e-4, gamma=0.99)
               .debugging(seed=9))
        cfg.num_envs = N
        cfg.rollout_fragment_length = T
        if flag:
            cfg.reporting(rollout_metrics=True, json_lines=tmp_path / "m.jsonl")
        return PPO(config=cfg, device=d)

    on, off = make(True), make(False)
    assert on.precision == "sf16" and on.T == T and on.A == 2
    assert off.rm_out is None and off.rm_ws is None and off.rm_counters is None
    for it in range(2):
        r_on, r_off = on.train(), off.train()
        assert "custom_metrics" not in r_off
        assert _same(r_on["episode_reward_mean"], r_off["episode_reward_mean"])
    assert r_on["episodes_this_iter"] == N and np.isfinite(r_on["episode_reward_mean"])
    for a, b in ((on.params.flat, off.params.flat), (on.adam_m, off.adam_m), (on.adam_v, off.adam_v)):
        assert torch.equal(a, b)
    cm = r_on["custom_metrics"]
    ref, ab = reference(**_host(on), A=2, C=2)
    check_record(on.rollout_record, ref, ab, 2, "device record")
    assert cm == summarise(on.rollout_record, 2, 2)
    _close_metrics(cm, ref, ab, 2, 2)
    assert sum(cm["action_count"]) == T * N and cm["dones"] == N
    assert abs(sum(cm["action_share"]) - 1.0) <= 2 * 2.0 ** -53
    assert "pods_placed" not in cm
    # the JSON lines: one per train(), the nested lists as lists
    lines = [json.loads(x) for x in (tmp_path / "m.jsonl").read_text().splitlines()]
    assert len(lines) == 2
    share = lines[1]["custom_metrics"]["action_share"]
    assert isinstance(share, list) and len(share) == 2 and share == cm["action_share"]
    assert lines[1]["custom_metrics"]["action_count"] == cm["action_count"]
    on.stop()
    off.stop()


def test_train_reports_custom_metrics_node_env():
    """regime A's shape (tests/node_regimes.py: 3 clusters of 16 nodes, mixed node memory), the policy
    choosing every action; occupancy 1.0 and 24 arrivals a step fill clusters within the first fragment
    (the C oracle under uniform actions: 1,869 rejected and 43,018 departed after 16 steps).  The pod
    counts of each iteration are the deltas of a twin env stepped with the recorded actions"""
    from rlks import VecK8sMultiCloudEnv
    from rlks.env import NodeSpec
    from rlks.ppo import PPO, PPOConfig
    from rlks.tables import synthetic_table

    d = _dev()
    N, T, C = 256, 16, 3
    tab = synthetic_table(C, 100, seed=7)
    spec = NodeSpec(C, 16, node_cpu_m=[2000] * 3, node_mem_mi=[1024, 4096, 1024], arrival_rate=24.0, depart_prob=0.02,
                    init_occupancy=1.0, reject_penalty=0.25)
    cfg = (PPOConfig().framework("torch")
           .training(train_batch_size=N * T, sgd_minibatch_size=256, num_sgd_iter=2, lr=3e-4, gamma=0.99)
           .debugging(seed=5).reporting(rollout_metrics=True))
    cfg.num_envs, cfg.table, cfg.nodes = N, tab, spec
    agent = PPO(config=cfg, device=d)
    assert agent.T == T and agent.A == C
    twin = VecK8sMultiCloudEnv(N, table=tab, seed=5, nodes=spec, device=d)
    twin.counters(enable=1)
    twin.reset()
    seen = np.zeros(6, np.int64)
    for it in range(2):
        cm = agent.train()["custom_metrics"]
        b = _host(agent)
        assert len(np.unique(b["actions"])) == C  # the policy acts
        for t in range(T):
            obs, _, _, _, _ = twin.step(agent.buf["actions"][t])
            assert torch.equal(obs, agent.buf["obs"][t + 1])  # the twin is where the agent's env is
        twin.check_status()
        now = twin.counters().cpu().numpy()
        _, placed, rejected, departed, _, _ = (int(x) for x in now - seen)
        seen = now
        assert rejected >= 1 and departed >= 1 and placed >= 1  # a zero would let a swapped slot pass
        assert len({placed, rejected, departed}) == 3
        assert (cm["pods_placed"], cm["pods_rejected"], cm["pods_departed"]) == (placed, rejected, departed)
        assert cm["rejection_rate"] == rejected / (placed + rejected)
        ref, ab = reference(**b, A=C, C=C)
        check_record(agent.rollout_record, ref, ab, C, f"iteration {it}")
        _close_metrics(cm, ref, ab, C, C)
        util = b["obs"][:T, :, 2 * C:].astype(np.float64).reshape(T * N, C).mean(0)
        for c in range(C):
            assert abs(cm["utilisation_mean"][c] - util[c]) <= 2 * sum_bound(T * N, util[c])  # sum|u| / n = mean
        assert sum(cm["action_count"]) == T * N
    agent.stop()
    twin.close()
