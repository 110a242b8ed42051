"""The node step's saturated, extreme and wide-cluster regimes: the cases, the C
oracle's trajectory of each, and the guards that prove from the oracle's state alone that a case is
in the regime it is named for.  tests/test_gpu_nodes_regimes.py holds the device to the recorded
trajectories; tests/test_oracle_nodes.py checks the guards without a device.

A floor below is a condition on the inputs, about a tenth of what the oracle gives for the case, not
a tolerance: a case that misses one has left its regime (a changed default, say) and is adjusted
until the oracle meets the floor again."""
import functools
from dataclasses import dataclass, field

import numpy as np

import oracle

N_ROWS, TABLE_SEED, SEED, ENV_OFFSET = 100, 7, 4, 3
POD_CPU_M, POD_MEM_MI = 100, 64
STATE_EVERY = 10


@dataclass(frozen=True)
class Case:
    n: int
    C: int
    nodes: int
    cpu: tuple      # node millicores per cluster
    mem: tuple      # node MiB per cluster
    rate: float
    depart: float
    occ: float
    penalty: float
    steps: int
    # floors (None: not asked of this case)
    min_rejected: int = None
    min_skips: int = None          # full chunks below a chunk with room, summed over steps
    min_full_clusters: int = None  # most entirely full (env, cluster) pairs after one step
    extra: tuple = field(default=())  # further guards, by name (see check_guards)


def _c(n, C, nodes, cpu, mem, rate, depart, occ, penalty, steps, **kw):
    cpu = tuple(cpu) if isinstance(cpu, (list, tuple)) else (cpu,) * C
    mem = tuple(mem) if isinstance(mem, (list, tuple)) else (mem,) * C
    assert len(cpu) == C and len(mem) == C
    return Case(n, C, nodes, cpu, mem, float(rate), float(depart), float(occ), float(penalty), steps, **kw)


CASES = {
    # C not 2^k, mixed node sizes, one partly used group of chunk totals
    "A": _c(96, 3, 16, 2000, (1024, 4096, 1024), 8, 0.02, 0.9, 0.25, 150,
            min_rejected=700, min_skips=700, min_full_clusters=1),
    # 9 chunks: one whole group of totals and one partly used
    "B": _c(64, 5, 72, 400, 4096, 12, 0.03, 1.0, 0.5, 150,
            min_rejected=700, min_skips=3000, min_full_clusters=1),
    # more than 256 nodes, 33 chunks, more pods than the survival table has entries
    "C": _c(32, 6, 264, 200, 4096, 30, 0.05, 1.0, 0.5, 150,
            min_rejected=100, min_skips=11000, min_full_clusters=1, extra=("table_shorter_than_pods",)),
    # one chunk per cluster, a last workgroup with few envs
    "D": _c(100, 7, 8, [300 if c % 2 == 0 else 500 for c in range(7)], 4096, 2, 0.1, 0.5, 0.125, 150,
            min_rejected=15, min_full_clusters=1),
    # more than 64 clusters
    "E": _c(48, 96, 8, 300, 4096, 6, 0.1, 1.0, 0.5, 150,
            min_rejected=1700, min_full_clusters=1),
    # more than 64 clusters and a survival table of more than 4096 entries, 64 pods a node
    "F": _c(8, 65, 128, 6400, 4096, 40, 0.002, 1.0, 0.5, 110,
            min_skips=700, extra=("table_over_4096",)),
    # p = 0: nothing ever leaves, empty clusters fill up
    "G": _c(64, 4, 24, 300, 4096, 3, 0.0, 0.0, 0.25, 110,
            min_rejected=1100, min_skips=380, min_full_clusters=1, extra=("no_departures",)),
    # p = 1: every pod leaves every step
    "H": _c(64, 4, 16, 2000, 1024, 8, 1.0, 1.0, 0.0, 110, extra=("departed_over_placed",)),
    # no arrivals at all
    "I": _c(64, 4, 16, 2000, 1024, 0, 0.2, 1.0, 0.0, 110, extra=("no_arrivals",)),
}


def max_pods(case):
    return np.minimum(np.array(case.cpu) // POD_CPU_M, np.array(case.mem) // POD_MEM_MI)


def actions(case):
    """[steps][n] int32: lane i takes its hot cluster i % C with probability 0.8, a uniform one otherwise"""
    n, C = case.n, case.C
    rng = np.random.default_rng(1)
    return np.stack([np.where(rng.random(n) < 0.8, np.arange(n) % C, rng.integers(0, C, n)).astype(np.int32)
                     for _ in range(case.steps)])


def table(case):
    from rlks.tables import synthetic_table

    return synthetic_table(case.C, N_ROWS, seed=TABLE_SEED)


def state_steps(case):
    """the steps after which the whole node state is compared"""
    return [t for t in range(case.steps) if (t + 1) % STATE_EVERY == 0 or t == case.steps - 1]


@dataclass
class Trajectory:
    actions: np.ndarray
    state_created: tuple    # (free cpu, free mem, used cpu) after creation
    obs_reset: np.ndarray
    state_reset: tuple
    obs: list               # per step
    rew: list
    term: list
    states: dict            # step -> node state
    counters: np.ndarray
    skips: int
    full_clusters: int
    n_skip: int


@functools.lru_cache(maxsize=None)
def oracle_run(name):
    """Case `name` stepped through the C oracle, once a process; nothing here is written to again."""
    case = CASES[name]
    tab = table(case)
    cfg = oracle.make_cfg(case.n, N_ROWS, case.C, noise_mode=0, seed=SEED, autoreset=1, env_offset=ENV_OFFSET,
                          nodes=case.nodes, pod_cpu_m=POD_CPU_M, pod_mem_mi=POD_MEM_MI, arrival_mode=0,
                          arrival_rate=case.rate, depart_prob=case.depart, init_occupancy=case.occ,
                          reject_penalty=case.penalty)
    ora = oracle.OracleEnv(cfg, tab.cost, tab.latency, np.array(case.cpu, np.int32), np.array(case.mem, np.int32), None)
    acts = actions(case)
    created = ora.node_state()
    obs_reset = ora.reset()
    tr = Trajectory(acts, created, obs_reset, ora.node_state(), [], [], [], {}, None, 0, 0,
                    len(oracle.skip32(case.nodes * int(max_pods(case).max()), case.depart)))
    mp = max_pods(case)[None, :, None]
    cpu = np.array(case.cpu)[None, :, None]
    keep = set(state_steps(case))
    for t in range(case.steps):
        o, r, term, _, _, status = ora.step(acts[t])
        assert not status.any(), status
        tr.obs.append(o)
        tr.rew.append(r)
        tr.term.append(term)
        st = ora.node_state()
        if t in keep:
            tr.states[t] = st
        # chunks of 8 full nodes, and those of them that a first fit would pass on its way to room
        pods = (cpu - st[0]) // POD_CPU_M
        full = (pods == mp).reshape(case.n, case.C, case.nodes // 8, 8).all(-1)   # [n][C][chunks]
        room_above = np.flip(np.logical_or.accumulate(np.flip(~full, -1), -1), -1)  # a chunk with room at >= index
        tr.skips += int((full & room_above).sum())
        tr.full_clusters = max(tr.full_clusters, int(full.all(-1).sum()))
    tr.counters = ora.counters()
    return tr


def check_guards(name):
    """The case is in its regime, by the oracle's state alone."""
    case, tr = CASES[name], oracle_run(name)
    checks, placed, rejected, departed = (int(x) for x in tr.counters[:4])
    assert case.steps > N_ROWS - 1, "the auto-reset must fall inside the run"
    assert any(t.any() for t in tr.term)
    if case.min_rejected is not None:
        assert rejected >= case.min_rejected, (name, rejected)
    if case.min_skips is not None:
        assert tr.skips >= case.min_skips, (name, tr.skips)
    if case.min_full_clusters is not None:
        assert tr.full_clusters >= case.min_full_clusters, (name, tr.full_clusters)
    pods_max = case.nodes * int(max_pods(case).max())
    for g in case.extra:
        if g == "table_shorter_than_pods":
            assert tr.n_skip < pods_max, (tr.n_skip, pods_max)
        elif g == "table_over_4096":
            assert tr.n_skip > 4096, tr.n_skip
        elif g == "no_departures":
            assert departed == 0 and placed > 0
        elif g == "departed_over_placed":
            assert departed > placed > 0, (departed, placed)
        elif g == "no_arrivals":
            assert placed == 0 and rejected == 0 and checks == 0 and departed > 0, tr.counters
        else:
            raise KeyError(g)
    return tr
