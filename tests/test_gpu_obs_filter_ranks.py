"""The observation filter on the data-parallel path: two gloo ranks on one GPU (fresh child processes,
tests/obs_filter_worker.py), 256 lanes each, 8 steps, one iteration.  Every rank takes the record of its
own raw observations about the same shift K (the states are equal on all ranks), the records are summed
by the all-reduce and every rank merges the sum: both ranks end with bit-identical filter state, its
count is the job's row count, and the state is within the whole-state bound (tests/obs_filter_ref.py) of
numpy over both ranks' rows."""
import os
import socket
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

import obs_filter_ref as R

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

HERE = Path(__file__).resolve().parent


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _run_ranks(out, N, T, iters, world):
    out.mkdir(parents=True, exist_ok=True)
    port = _free_port()
    procs = []
    for r in range(world):
        env = dict(os.environ, RANK=str(r), WORLD_SIZE=str(world), LOCAL_RANK=str(r), MASTER_ADDR="127.0.0.1",
                   MASTER_PORT=str(port), HSA_ENABLE_IPC_MODE_LEGACY="0")
        procs.append(subprocess.Popen([sys.executable, str(HERE / "obs_filter_worker.py"), str(out), str(N), str(T),
                                       str(iters)], env=env))
    try:
        for p in procs:
            assert p.wait(timeout=100) == 0
    finally:
        for p in procs:
            if p.poll() is None:
                p.kill()
    return [np.load(out / f"rank{r}.npz") for r in range(world)]


def test_two_ranks_share_one_filter_state(tmp_path):
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    N, T, world = 256, 8, 2
    ranks = _run_ranks(tmp_path, N, T, 1, world)
    assert ranks[0]["state"].tobytes() == ranks[1]["state"].tobytes()
    assert ranks[0]["raw"].tobytes() != ranks[1]["raw"].tobytes()  # each rank has lanes of its own
    rows = world * (T + 1) * N
    assert list(ranks[0]["counts"]) == list(ranks[1]["counts"]) == [rows]
    D = ranks[0]["raw"].shape[-1]
    # one merge of the summed record: for the bound, one batch of both ranks' rows
    both = np.concatenate([r["raw"][0].reshape(-1, D) for r in ranks])
    R.check_whole_state(R.unpack(ranks[0]["state"]), rows, [both], "two ranks")
    assert np.array_equal(ranks[0]["params"].view(np.int32), ranks[1]["params"].view(np.int32))
