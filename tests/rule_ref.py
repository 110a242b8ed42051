"""The baseline schedulers of rlks_env_rule_actions restated in numpy, the cases they
are tested on, and the C oracle's run of each case under each rule.  tests/test_gpu_rule_actions.py
and tests/test_gpu_eval_nodes.py hold the device to these; tests/test_rule_cases_host.py checks
without a device that every case is in the regimes it is there for.

Every rule is exact arithmetic (f32 compares, f64 products and sums rounded one by one, integers), so
the restatement and the device agree to the bit; "random" goes through oracle.sample_actions on an
all-zero logits row (every exp() is exactly 1: no draw's outcome depends on a rounding).

All cases: 100 rows, synthetic_table(C, 100, seed=7), seed 4, env_offset 3, 120 steps (past the
auto-reset), pod 100m / 64Mi, nodes 300m / 4096Mi (3 pods a node).

A floor is a condition on the inputs (about a tenth of what the oracle gives, node_regimes.py's
convention), not a tolerance."""
import dataclasses
import functools

import numpy as np

import node_regimes as nr
import node_sample_cases as ns
import oracle

RULES = {"round_robin": 0, "cheapest": 1, "myopic": 2, "least_loaded": 3, "myopic_with_room": 4, "random": 5}
STEPS = 120
W_COST, W_LAT = 0.6, 0.4  # oracle.make_cfg / rlks.env.make_cfg: reward = 100 * (0.6 cost + 0.4 latency)

CASES = {
    # p = 0, empty clusters fill up (node_regimes' G)
    "G": nr._c(64, 4, 24, 300, 4096, 3, 0.0, 0.0, 0.25, STEPS),
    # C = 3: observation row stride 9, a ragged last workgroup
    "J": nr._c(50, 3, 8, 300, 4096, 3, 0.02, 0.5, 0.25, STEPS),
    # C = 96: the lane-per-env step kernel
    "K": nr._c(40, 96, 8, 300, 4096, 12, 0.01, 1.0, 0.5, STEPS),
    "L": nr._c(70, 2, 8, 300, 4096, 2, 0.03, 0.5, 0.25, STEPS),
}
TABLE_CASE = dict(n=70, C=2)  # a table env (nodes_per_cluster = 0) with MT19937 noise

# lane-steps out of n * 120, measured with the C oracle: (myopic_with_room != myopic, no cluster with room,
# some cluster full) along the myopic_with_room run, least-loaded ties along the least_loaded run; and the
# pods "myopic" rejects, the actions it uses
MEASURED = {
    "G": dict(differ=906, no_room=207, some_full=1688, ll_ties=3243, myopic_rejected=2921, myopic_actions=4),
    "J": dict(differ=1427, no_room=636, some_full=3651, ll_ties=2003, myopic_rejected=6177, myopic_actions=3),
    "K": dict(differ=219, no_room=0, some_full=4276, ll_ties=3238, myopic_rejected=13512, myopic_actions=57),
    "L": dict(differ=1199, no_room=858, some_full=3283, ll_ties=2195, myopic_rejected=3501, myopic_actions=2),
}
# the floors (a tenth; K's "no room anywhere" is 0 and is not asked)
FLOORS = {
    "G": dict(differ=90, no_room=20, some_full=160, ll_ties=320, myopic_rejected=290),
    "J": dict(differ=140, no_room=60, some_full=360, ll_ties=200, myopic_rejected=610),
    "K": dict(differ=20, no_room=None, some_full=420, ll_ties=320, myopic_rejected=1350),
    "L": dict(differ=110, no_room=80, some_full=320, ll_ties=210, myopic_rejected=350),
}


@dataclasses.dataclass(frozen=True)
class Spec:
    """what a rule reads besides the lane's observation and counters"""
    C: int
    nodes: int = 0            # per cluster; 0: a table env
    pod_cpu: int = nr.POD_CPU_M
    pod_mem: int = nr.POD_MEM_MI
    cpu: tuple = ()           # node millicores / MiB per cluster
    mem: tuple = ()
    w_cost: float = W_COST
    w_lat: float = W_LAT
    seed: int = nr.SEED
    env_offset: int = nr.ENV_OFFSET


def spec_of(case):
    return Spec(case.C, case.nodes, cpu=tuple(case.cpu), mem=tuple(case.mem))


def _first_max(s, allowed=None):
    """lowest index of the maximum by strict > over the allowed columns of s [n][C]"""
    n, C = s.shape
    act = np.full(n, -1, np.int64)
    best = np.zeros(n, s.dtype)
    for c in range(C):
        ok = np.ones(n, bool) if allowed is None else allowed[:, c]
        take = ok & ((act < 0) | (s[:, c] > best))
        best = np.where(take, s[:, c], best)
        act = np.where(take, c, act)
    return act


def has_room(used_cpu, spec):
    """[n][C] bool: the cluster can take one more pod, from its used millicores (integers)"""
    pods = np.asarray(used_cpu, np.int64) // spec.pod_cpu
    cap = spec.nodes * np.minimum(np.array(spec.cpu, np.int64) // spec.pod_cpu,
                                  np.array(spec.mem, np.int64) // spec.pod_mem)
    return pods < cap[None, :]


def has_room_nodes(free_cpu, free_mem, spec):
    """the same from the node state [n][C][nodes]: some node has free cpu and memory for one pod"""
    return ((free_cpu >= spec.pod_cpu) & (free_mem >= spec.pod_mem)).any(-1)


def myopic_scores(obs, spec):
    o = np.asarray(obs, np.float32)
    C = spec.C
    # f64, the two products and the sum rounded separately (numpy never contracts)
    return np.float64(spec.w_cost) * o[:, :C].astype(np.float64) + np.float64(spec.w_lat) * o[:, C:2 * C].astype(np.float64)


def rule_actions(rule, obs, step, episode, used_cpu, spec):
    """int32 [n]: the decision of `rule` (a name or its number) for every lane, from obs [n][3C] float32,
    step / episode [n] and, for a node-level spec, used_cpu [n][C]"""
    rule = RULES[rule] if isinstance(rule, str) else int(rule)
    o = np.asarray(obs, np.float32)
    n, C = o.shape[0], spec.C
    assert o.shape == (n, 3 * C)
    if rule == 0:
        act = np.asarray(step, np.int64) % C
    elif rule == 1:
        act = _first_max(-o[:, :C])            # lowest index of the minimum (f32 negation is exact)
    elif rule == 2:
        act = _first_max(myopic_scores(o, spec))
    elif rule == 3:
        act = _first_max(-o[:, 2 * C:])
    elif rule == 4:
        s = myopic_scores(o, spec)
        act = _first_max(s)
        if spec.nodes > 0:
            room = has_room(used_cpu, spec)
            act = np.where(room.any(1), _first_max(s, room), act)
    elif rule == 5:
        act, _ = oracle.sample_actions(np.zeros((n, C), np.float32), spec.env_offset + np.arange(n), episode, step,
                                       spec.seed)
    else:
        raise ValueError(rule)
    return np.asarray(act, np.int32)


def make_oracle(case, autoreset=1, seed=nr.SEED, env_offset=nr.ENV_OFFSET):
    tab = nr.table(case)
    cfg = oracle.make_cfg(case.n, nr.N_ROWS, case.C, noise_mode=0, seed=seed, autoreset=autoreset, env_offset=env_offset,
                          nodes=case.nodes, pod_cpu_m=nr.POD_CPU_M, pod_mem_mi=nr.POD_MEM_MI, arrival_mode=0,
                          arrival_rate=case.rate, depart_prob=case.depart, init_occupancy=case.occ,
                          reject_penalty=case.penalty)
    return oracle.OracleEnv(cfg, tab.cost, tab.latency, np.array(case.cpu, np.int32), np.array(case.mem, np.int32), None)


node_spec = ns.node_spec  # the rlks.env.NodeSpec of a case


def decide(ora, rule, obs, spec):
    """the rule's actions for the oracle env's lanes as they stand"""
    st, ep = ora.lane_counters()
    used = ora.node_state()[2] if spec.nodes > 0 else None
    return rule_actions(rule, obs, st, ep, used, spec)


@dataclasses.dataclass
class Run:
    obs_reset: np.ndarray
    actions: list       # per step, int32 [n]
    obs: list           # per step, the observation after it
    rew: list           # float64
    term: list
    counters: np.ndarray
    # lane-steps: myopic_with_room != myopic, no cluster with room, some cluster full, utilisation minimum tied
    differ: int = 0
    no_room: int = 0
    some_full: int = 0
    ll_ties: int = 0
    room_mismatch: int = 0  # (lane, cluster) states where the used-cpu room test and the per-node one disagree


@functools.lru_cache(maxsize=None)
def oracle_run(name, rule):
    """Case `name` stepped through the C oracle by `rule`, once a process; nothing here is written to again."""
    case = CASES[name]
    spec = spec_of(case)
    ora = make_oracle(case)
    obs = ora.reset()
    run = Run(obs.copy(), [], [], [], [], None)
    for _ in range(case.steps):
        st, ep = ora.lane_counters()
        fc, fm, used = ora.node_state()
        room = has_room(used, spec)
        run.room_mismatch += int((room != has_room_nodes(fc, fm, spec)).sum())
        run.no_room += int((~room.any(1)).sum())
        run.some_full += int((~room.all(1)).sum())
        util = obs[:, 2 * spec.C:]
        run.ll_ties += int(((util == util.min(1, keepdims=True)).sum(1) > 1).sum())
        run.differ += int((rule_actions("myopic_with_room", obs, st, ep, used, spec)
                           != rule_actions("myopic", obs, st, ep, used, spec)).sum())
        a = rule_actions(rule, obs, st, ep, used, spec)
        obs, r, term, _, _, status = ora.step(a)
        assert not status.any(), status
        obs = obs.copy()
        run.actions.append(a)
        run.obs.append(obs)
        run.rew.append(r.copy())
        run.term.append(term.copy())
    run.counters = ora.counters()
    return run


def check_guards(name):
    """The case is in the regimes it is there for, by the oracle's state alone."""
    fl = FLOORS[name]
    wr, ll, my = oracle_run(name, "myopic_with_room"), oracle_run(name, "least_loaded"), oracle_run(name, "myopic")
    assert any(t.any() for t in wr.term), "the auto-reset must fall inside the run"
    assert wr.differ >= fl["differ"], (name, wr.differ)
    if fl["no_room"] is not None:
        assert wr.no_room >= fl["no_room"], (name, wr.no_room)
    assert wr.some_full >= fl["some_full"], (name, wr.some_full)
    assert ll.ll_ties >= fl["ll_ties"], (name, ll.ll_ties)
    assert int(my.counters[2]) >= fl["myopic_rejected"], (name, my.counters)
    return wr, ll, my
