"""The cases of tests/node_sample_cases.py, by the C oracle alone (no device): each is dispatched to
the kernel form it is named for, draws every action, auto-resets every lane once, rejects pods where
it is meant to, keeps every draw at least 4 float32 ulp from a CDF boundary, and counts what was
recorded for it."""
import numpy as np
import pytest

import node_sample_cases as ns


@pytest.mark.parametrize("name", sorted(ns.CASES))
def test_case_guards(name):
    run = ns.check_guards(name)
    placed, rejected, departed = (int(x) for x in run.counters[1:4])
    print(f"{name}: placed {placed} rejected {rejected} departed {departed} "
          f"min margin {min(float(m.min()) for m in run.margins):.1f} ulp")
    assert (placed, rejected, departed) == ns.ORACLE_COUNTS[name]


def test_logit_rows_at_the_edges():
    for name, case in ns.CASES.items():
        for t in (0, 1, case.C, case.steps - 1):
            lg = ns.logits(case, t)
            C = case.C
            assert lg.dtype == np.float32 and lg.shape == (case.n, C)
            assert (lg[0] == 0).all()
            assert sorted(np.flatnonzero(lg[1] == 2.0)) == sorted({1 % C, C - 1}) and (np.delete(lg[1], [1 % C, C - 1]) == -1).all()
            assert np.flatnonzero(np.isfinite(lg[2])).tolist() == [t % C] and lg[2, t % C] == 0.5
            assert (np.exp(lg[3] - lg[3].max(), dtype=np.float32)[1::2] == 0).all()
            if case.n > 4:  # a lane's hot cluster outweighs the others together on average
                i = 4
                assert np.mean([ns.logits(case, s)[i].argmax() == i % C for s in range(20)]) > 0.3
