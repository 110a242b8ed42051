"""Invalid-action masking restated in numpy and torch float64: the room mask, the masked
Categorical draw and the masked PPO loss, the oracle's runs the device tests follow, and the minibatches
of the loss test.  tests/test_gpu_action_mask.py holds the device to these; tests/test_action_mask_host.py
ties them to the oracle without a device (with an all-true mask they are oracle.sample_actions and
oracle.ppo_loss_grad exactly) and checks that every case is in the regime it is there for.

A floor is a condition on the inputs (a tenth of what the oracle gives, node_regimes.py's convention),
not a tolerance."""
import dataclasses
import functools

import numpy as np

import node_regimes as nr
import oracle
import rule_ref as rr

MASKED_LOGIT = np.float32(-1e30)      # include/rlks_types.h RLKS_MASKED_LOGIT
MASKED_LOGIT_MAX = np.float32(-1e29)  # RLKS_MASKED_LOGIT_MAX: a logit <= this counts as masked

MASK_CASES = ("G", "J", "L")  # rule_ref cases whose clusters fill up (rule_ref.FLOORS: some_full, no_room)

# A Philox counter whose draw f32(u53(words 0, 1)) is exactly 1.0 (u53 >= 1 - 2^-25: word 0 >= 0xFFFFFF80),
# found offline by scanning counter word 2 upwards from 0 with oracle.philox_batch under this key (about
# 2^-25 of the counters qualify); tests/test_action_mask_host.py re-derives the draw
FALLBACK_IDS = (7, 0, 1254616)  # Philox words 0, 1 = 0xffffff9b, 0x50704fd5
FALLBACK_SEED = 12345


# ----------------------------------------------------------------------------- mask
def room_mask(used_cpu, spec):
    """bool [n][C]: rule_ref.has_room, a row without room anywhere all True; a table spec all True"""
    used = np.asarray(used_cpu)
    if spec.nodes == 0:
        return np.ones((used.shape[0], spec.C), bool)
    room = rr.has_room(used, spec).copy()
    room[~room.any(1)] = True
    return room


def mask_bits(mask):
    """uint64 [n]: bit c = mask[:, c]"""
    m = np.asarray(mask, bool)
    return (m.astype(np.uint64) << np.arange(m.shape[1], dtype=np.uint64)[None, :]).sum(1, dtype=np.uint64)


def mask_logits(logits, mask):
    """float32 copy of logits with the entries outside the mask set to MASKED_LOGIT"""
    return np.where(np.asarray(mask, bool), np.asarray(logits, np.float32), MASKED_LOGIT).astype(np.float32)


# ----------------------------------------------------------------------------- sampler
def sample_masked(logits, mask, gids, episodes, steps, seed, explore=True):
    """oracle.sample_actions on the masked row, with the sampler's one difference: when no cumulative entry
    exceeds u the action is the highest unmasked index.  (A masked entry adds exp() = 0 to the running sum,
    so the scan never stops on one: a masked result can only be oracle.sample_actions' A - 1 default.)
    Greedy: the first maximum of the masked row.
    -> (masked logits float32, actions int32, margin (oracle.sample_actions'; inf when greedy),
        logp float64 = log-softmax of the masked row at the action)"""
    m = np.asarray(mask, bool)
    n, A = m.shape
    ml = mask_logits(logits, m)
    if explore:
        act, margin = oracle.sample_actions(ml, gids, episodes, steps, seed)
        highest = (A - 1 - np.argmax(m[:, ::-1], axis=1)).astype(np.int32)
        act = np.where(m[np.arange(n), act], act, highest).astype(np.int32)
    else:
        act, margin = ml.argmax(1).astype(np.int32), np.full(n, np.inf)
    l64 = ml.astype(np.float64)
    mx = l64.max(1, keepdims=True)
    lse = mx[:, 0] + np.log(np.exp(l64 - mx).sum(1))
    return ml, act, margin, l64[np.arange(n), act] - lse


# ----------------------------------------------------------------------------- loss
def ppo_loss_grad_masked(flat, off, D, H, A, mb, *, clip_param=0.3, vf_clip_param=10.0, vf_loss_coeff=1.0,
                         entropy_coeff=0.0, kl_coeff=0.2, adv_mean=0.0, adv_inv_std=1.0, count=None):
    """oracle.ppo_loss_grad (float64 autograd) with the loss heads' select: the new logit of an action whose
    old logit is <= MASKED_LOGIT_MAX is that old logit, not the network's output.
    -> (grad, stats dict of per-row sums)"""
    import torch

    rec = torch.as_tensor(np.asarray(mb, np.float64))
    rows = rec.shape[0]
    count = rows if count is None else count
    f = torch.tensor(np.asarray(flat, np.float64), requires_grad=True)
    x = rec[:, :D]
    lo = rec[:, D: D + A]
    adv = (rec[:, D + A] - adv_mean) * adv_inv_std
    vt = rec[:, D + A + 1]
    logp_old = rec[:, D + A + 2]
    act = rec[:, D + A + 3].long()
    outs = []
    for net in (0, 1):
        w1, b1, w2, b2, w3, b3 = oracle._net(torch, f, off, D, H, A, net)
        h1 = torch.tanh(x @ w1.T + b1)
        h2 = torch.tanh(h1 @ w2.T + b2)
        outs.append(h2 @ w3.T + b3)
    logits, value = torch.where(lo <= float(MASKED_LOGIT_MAX), lo, outs[0]), outs[1][:, 0]
    logp_all = torch.log_softmax(logits, dim=1)
    logp = logp_all.gather(1, act[:, None])[:, 0]
    ratio = torch.exp(logp - logp_old)
    surr = torch.min(adv * ratio, adv * torch.clamp(ratio, 1 - clip_param, 1 + clip_param))
    lpo = torch.log_softmax(lo, dim=1)
    kl = (lpo.exp() * (lpo - logp_all)).sum(1)
    ent = -(logp_all.exp() * logp_all).sum(1)
    vf = torch.clamp((value - vt) ** 2, 0, vf_clip_param)
    total = (-surr + vf_loss_coeff * vf - entropy_coeff * ent).sum() / count + kl_coeff * kl.sum() / count
    total.backward()
    stats = {"policy_loss": float((-surr).sum().detach()), "vf_loss": float(vf.sum().detach()),
             "kl": float(kl.sum().detach()), "entropy": float(ent.sum().detach()), "rows": rows}
    return f.grad.numpy(), stats


# the loss test's shapes: (name, D, H, A, rows, precision), one per policy loss head and F1 form
LOSS_CASES = (
    ("sf16-fused-2", 6, 256, 2, 256, "sf16"),
    ("sf16-fused-4", 12, 256, 4, 256, "sf16"),
    ("sf16-split-8", 24, 256, 8, 256, "sf16"),
    ("fp32-2", 6, 256, 2, 128, "fp32"),
    ("wide-3", 9, 64, 3, 256, "wide"),
)
LOSS_ALWAYS_MASKED = 1  # action 1 is masked in every row (every case has A >= 2)


def loss_minibatch(D, A, rows, seed=0, masked=True):
    """(records float32 [rows][D + A + 4], mask bool [rows][A]): observations in [0, 1), old logits N(0, 0.3)
    (near a fresh policy's, so that the ratios straddle the clip range) masked per row at random (action LOSS_ALWAYS_MASKED in every row, at least one action unmasked), the
    taken action uniform over the unmasked ones, logp_old the masked row's log-softmax at it"""
    rng = np.random.default_rng([11, seed, D, A, rows])
    mb = np.zeros((rows, D + A + 4), np.float32)
    mb[:, :D] = rng.random((rows, D))
    lo = (0.3 * rng.standard_normal((rows, A))).astype(np.float32)
    mask = np.ones((rows, A), bool)
    if masked:
        mask = rng.random((rows, A)) < 0.6
        mask[:, LOSS_ALWAYS_MASKED] = False
        keep = rng.integers(0, A - 1, rows)
        keep += keep >= LOSS_ALWAYS_MASKED   # a column other than the always-masked one
        mask[np.arange(rows), keep] = True
    lo = mask_logits(lo, mask)
    mb[:, D:D + A] = lo
    mb[:, D + A] = rng.standard_normal(rows)
    mb[:, D + A + 1] = rng.standard_normal(rows)
    pick = rng.random((rows, A)) * mask
    act = pick.argmax(1)
    mb[:, D + A + 3] = act
    l64 = lo.astype(np.float64)
    mx = l64.max(1, keepdims=True)
    lp = l64 - mx - np.log(np.exp(l64 - mx).sum(1, keepdims=True))
    mb[:, D + A + 2] = lp[np.arange(rows), act]
    return mb, mask


# ----------------------------------------------------------------------------- runs
def step_logits(case, t):
    """fresh seeded N(0, 1.5) logits [n][C] float32 of step t"""
    return np.random.default_rng([23, t]).normal(0, 1.5, (case.n, case.C)).astype(np.float32)


@dataclasses.dataclass
class MaskRun:
    masks: list      # per step, bool [n][C]: the mask before the step
    steps: list      # per step, the lanes' step counters before it
    episodes: list
    actions: list    # per step: the actions that stepped the oracle
    some_masked: int = 0   # lane-steps with a masked cluster
    no_room: int = 0       # lane-steps without room anywhere (an all-ones mask by the fallback)


@functools.lru_cache(maxsize=None)
def rule_run(name):
    """rule_ref's "myopic_with_room" run of case `name`, replayed through a fresh C oracle to read the
    used millicores, hence the mask, before every step; once a process, never written to again"""
    case = rr.CASES[name]
    spec = rr.spec_of(case)
    exp = rr.oracle_run(name, "myopic_with_room")
    ora = rr.make_oracle(case)
    ora.reset()
    run = MaskRun([], [], [], exp.actions)
    for t in range(case.steps):
        st, ep = ora.lane_counters()
        used = ora.node_state()[2]
        m = room_mask(used, spec)
        run.masks.append(m)
        run.steps.append(np.array(st))
        run.episodes.append(np.array(ep))
        run.some_masked += int((~m.all(1)).sum())
        run.no_room += int((~rr.has_room(used, spec).any(1)).sum())
        _, _, _, _, _, status = ora.step(exp.actions[t])
        assert not status.any(), status
    return run


def check_mask_guards(name):
    """clusters fill and the no-room fallback occurs along the run (rule_ref.FLOORS' own floors)"""
    run = rule_run(name)
    fl = rr.FLOORS[name]
    # a lane-step with some cluster full has a masked cluster unless no cluster has room
    assert run.some_masked + run.no_room >= fl["some_full"], (name, run.some_masked, run.no_room)
    assert run.some_masked >= fl["some_full"] - fl["no_room"] > 0, (name, run.some_masked)
    assert run.no_room >= fl["no_room"], (name, run.no_room)
    return run


# the roomy spec: nothing ever fills (24 nodes x 40 pods a cluster, empty at reset, one arrival a step)
ROOMY = nr._c(70, 4, 24, 4000, 4096, 1, 0.05, 0.0, 0.1, 100)


# ----------------------------------------------------------------------------- rollout replay
ROLLOUT_CASES = ("G", "J")
ROLLOUT_N, ROLLOUT_T, ROLLOUT_SEED = 256, 16, 5
# lane-steps (out of ROLLOUT_ITERS x T x N) with a masked cluster along PPO's rollouts, measured once with
# the oracle replay of tests/test_gpu_action_mask.py; the floor is a tenth
ROLLOUT_ITERS = {"G": 6, "J": 1}  # G starts empty: its clusters fill towards the end of the episode
ROLLOUT_MEASURED = {"G": 5037, "J": 227}
ROLLOUT_FLOORS = {k: v // 10 for k, v in ROLLOUT_MEASURED.items()}


def rollout_case(name):
    """rule_ref case `name` at ROLLOUT_N lanes"""
    return dataclasses.replace(rr.CASES[name], n=ROLLOUT_N)


def rollout_oracle(case, seed):
    tab = nr.table(case)
    cfg = oracle.make_cfg(case.n, nr.N_ROWS, case.C, noise_mode=0, seed=seed, autoreset=1, env_offset=0,
                          nodes=case.nodes, pod_cpu_m=nr.POD_CPU_M, pod_mem_mi=nr.POD_MEM_MI, arrival_mode=0,
                          arrival_rate=case.rate, depart_prob=case.depart, init_occupancy=case.occ,
                          reject_penalty=case.penalty)
    return oracle.OracleEnv(cfg, tab.cost, tab.latency, np.array(case.cpu, np.int32), np.array(case.mem, np.int32), None)
