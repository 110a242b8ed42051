"""GPU parity of the node-level env step against the C oracle where tests/test_gpu_nodes.py does not
go: clusters that fill up, so that first fit skips full chunks, rejects pods and
charges the penalty (rejections are covered here, not there); cluster counts that are no power of
two or exceed 64; one-chunk clusters, partly used groups of chunk totals, more than 256 nodes;
depart_prob of exactly 0 and 1, and no arrivals.  The cases and the guards that keep each in its
regime are in tests/node_regimes.py.

Per case, bit for bit: observations, f64 rewards and terminations after every step; every node's
free millicores / MiB and the per-cluster used millicores after creation, after reset(), every
10th step and after the last; all six counters at the end."""
import numpy as np
import pytest

import node_regimes as nr

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")


def _dev():
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    return torch.device("cuda", 0)


def _compare_state(venv, exp, what):
    got = [x.cpu().numpy() for x in venv.node_state()]
    for g, e, name in zip(got, exp, ("free cpu", "free mem", "used cpu")):
        np.testing.assert_array_equal(g, e, err_msg=f"{name} {what}")


@pytest.mark.parametrize("name", sorted(nr.CASES))
def test_node_regime_matches_oracle(name):
    from rlks import VecK8sMultiCloudEnv
    from rlks.env import NodeSpec

    case = nr.CASES[name]
    exp = nr.check_guards(name)  # the oracle's run, proven to be in the regime, before the device is touched
    d = _dev()
    spec = NodeSpec(case.C, case.nodes, node_cpu_m=list(case.cpu), node_mem_mi=list(case.mem),
                    pod_cpu_m=nr.POD_CPU_M, pod_mem_mi=nr.POD_MEM_MI, arrival_rate=case.rate,
                    depart_prob=case.depart, init_occupancy=case.occ, reject_penalty=case.penalty)
    assert spec.depart_prob == case.depart
    venv = VecK8sMultiCloudEnv(case.n, table=nr.table(case), seed=nr.SEED, nodes=spec, env_offset=nr.ENV_OFFSET,
                               device=d)
    venv.counters(enable=1)
    _compare_state(venv, exp.state_created, "after creation")
    np.testing.assert_array_equal(venv.reset().cpu().numpy().view(np.uint32), exp.obs_reset.view(np.uint32))
    _compare_state(venv, exp.state_reset, "after reset")
    acts = torch.from_numpy(exp.actions).to(d)
    for t in range(case.steps):
        obs, rew, term, _, _ = venv.step(acts[t])
        np.testing.assert_array_equal(obs.cpu().numpy().view(np.uint32), exp.obs[t].view(np.uint32),
                                      err_msg=f"obs at step {t}")
        np.testing.assert_array_equal(rew.cpu().numpy().view(np.uint64), exp.rew[t].view(np.uint64),
                                      err_msg=f"reward at step {t}")
        np.testing.assert_array_equal(term.cpu().numpy(), exp.term[t], err_msg=f"terminated at step {t}")
        if t in exp.states:
            _compare_state(venv, exp.states[t], f"after step {t}")
    np.testing.assert_array_equal(venv.counters().cpu().numpy(), exp.counters)
    venv.check_status()
