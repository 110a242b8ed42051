"""Cases of the fused Categorical sample + node step (rlks_env_sample_step on node-level envs,
DESIGN.md §18): the envs, the logits of every step, and the C oracle's run of each case with the
actions oracle.sample_actions draws from those logits.  tests/test_gpu_node_sample_step.py holds the
device to these; tests/test_node_sample_cases_host.py checks without a device that every case does
what it is named for.

One case per dispatch form and lane layout of the sampling kernels: the work-list kernel with 2^cs
pair lanes an env (C = 2^cs, C < 2^cs with padded pair lanes and a logit row stride that is no
power of two, 1 to 64 envs a workgroup, a ragged last workgroup) and the two lane-per-env kernels
(C > 64).  A, D, E and F are tests/node_regimes.py's configurations with fewer steps.

A floor is a condition on the inputs (a tenth of what the oracle gives, node_regimes.py's
convention), not a tolerance."""
import dataclasses
import functools

import numpy as np

import node_regimes as nr
import oracle

MARGIN_ULP = 4  # draws closer than this to a CDF boundary may differ by exp() rounding (oracle.sample_actions)

CASES = {
    # wl, C = 2^k, 16 envs a workgroup, a ragged last workgroup
    "P8": nr._c(200, 8, 64, 400, 4096, 6, 0.05, 0.9, 0.25, 120),
    # wl, padded pair lanes (cs = 2), logit row stride 3
    "A": dataclasses.replace(nr.CASES["A"], steps=120, min_rejected=60, min_skips=None, min_full_clusters=None),
    # wl, cs = 3 with C = 7
    "D": dataclasses.replace(nr.CASES["D"], steps=120, min_rejected=None, min_skips=None, min_full_clusters=None),
    # wl, 64 envs a workgroup
    "P2": nr._c(70, 2, 16, 400, 4096, 3, 0.1, 0.5, 0.25, 120),
    # wl, 2 envs a workgroup, the last one half filled
    "P64": nr._c(7, 64, 8, 300, 4096, 6, 0.1, 1.0, 0.5, 120, min_rejected=40),
    # k_node_step<true>
    "E": dataclasses.replace(nr.CASES["E"], steps=120, min_rejected=500, min_skips=None, min_full_clusters=None),
    # k_node_step<false>
    "F": dataclasses.replace(nr.CASES["F"], steps=110, min_skips=None, extra=()),
}

# [placed, rejected, departed] the oracle counts for each case (recorded; the floors above are a tenth)
ORACLE_COUNTS = {
    "P8": (144269, 0, 358988), "A": (91882, 634, 88733), "D": (24118, 11, 27859), "P2": (25349, 0, 25605),
    "P64": (4731, 398, 14352), "E": (28726, 5839, 129172), "F": (35244, 0, 431450),
}


# the sampling kernel rlks_env_sample_step dispatches each case to (env.hip node_step_launch)
FORMS = {"P8": "wl", "A": "wl", "D": "wl", "P2": "wl", "P64": "wl", "E": "lane, table in LDS", "F": "lane"}


def form(case):
    if case.C <= 64:
        return "wl"
    n_skip = len(oracle.skip32(case.nodes * int(nr.max_pods(case).max()), case.depart))
    return "lane, table in LDS" if n_skip <= 4096 else "lane"


def logits(case, t):
    """[n][C] float32 logits of step t: a hot cluster per lane, and four rows at the sampler's edges"""
    n, C = case.n, case.C
    rng = np.random.default_rng([5, t])
    lg = rng.normal(0, 1.5, (n, C)).astype(np.float32)
    lg[np.arange(n), np.arange(n) % C] += np.float32(np.log(4 * max(C - 1, 1)))
    lg[0] = 0.0                      # every logit tied
    lg[1] = -1.0                     # two equal maxima
    lg[1, 1 % C] = lg[1, C - 1] = 2.0
    lg[2] = -np.inf                  # one cluster with all the mass
    lg[2, t % C] = 0.5
    lg[3] = np.where(np.arange(C) % 2 == 0, 80.0, -80.0)  # expf underflows to 0: flat stretches of the CDF
    return lg


def node_spec(case):
    from rlks.env import NodeSpec

    return NodeSpec(case.C, case.nodes, node_cpu_m=list(case.cpu), node_mem_mi=list(case.mem),
                    pod_cpu_m=nr.POD_CPU_M, pod_mem_mi=nr.POD_MEM_MI, arrival_rate=case.rate,
                    depart_prob=case.depart, init_occupancy=case.occ, reject_penalty=case.penalty)


def make_oracle(case):
    tab = nr.table(case)
    cfg = oracle.make_cfg(case.n, nr.N_ROWS, case.C, noise_mode=0, seed=nr.SEED, autoreset=1, env_offset=nr.ENV_OFFSET,
                          nodes=case.nodes, pod_cpu_m=nr.POD_CPU_M, pod_mem_mi=nr.POD_MEM_MI, arrival_mode=0,
                          arrival_rate=case.rate, depart_prob=case.depart, init_occupancy=case.occ,
                          reject_penalty=case.penalty)
    return oracle.OracleEnv(cfg, tab.cost, tab.latency, np.array(case.cpu, np.int32), np.array(case.mem, np.int32), None)


def sample(ora, case, lg):
    """(actions, margins) oracle.sample_actions draws for the oracle env's lanes as they stand"""
    st, ep = ora.lane_counters()
    return oracle.sample_actions(lg, nr.ENV_OFFSET + np.arange(case.n), ep, st, nr.SEED)


@dataclasses.dataclass
class Run:
    actions: list      # per step, int32 [n]
    margins: list      # per step, distance of the draw to the nearest CDF boundary (float32 ulp)
    resets: np.ndarray  # auto-resets of each lane
    counters: np.ndarray


@functools.lru_cache(maxsize=None)
def oracle_run(name):
    """Case `name` through the C oracle alone, its actions drawn by oracle.sample_actions; once a
    process, nothing here is written to again."""
    case = CASES[name]
    ora = make_oracle(case)
    ora.reset()
    run = Run([], [], np.zeros(case.n, np.int64), None)
    for t in range(case.steps):
        a, m = sample(ora, case, logits(case, t))
        _, _, term, _, _, status = ora.step(a)
        assert not status.any(), status
        run.actions.append(a)
        run.margins.append(m)
        run.resets += term
    run.counters = ora.counters()
    return run


def check_guards(name):
    """Every action is drawn, every lane auto-resets once, the saturated cases reject pods, and no
    draw is near enough to a CDF boundary for exp() rounding to decide it."""
    case, run = CASES[name], oracle_run(name)
    assert form(case) == FORMS[name], (name, form(case))
    drawn = np.unique(np.concatenate(run.actions))
    assert np.array_equal(drawn, np.arange(case.C)), (name, drawn)
    assert (run.resets == 1).all(), (name, run.resets)
    rejected = int(run.counters[2])
    if case.min_rejected is not None:
        assert rejected >= case.min_rejected, (name, rejected)
    assert min(float(m.min()) for m in run.margins) >= MARGIN_ULP, name
    return run
