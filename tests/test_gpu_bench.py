"""bench.py's plain run and --dump-outputs on the GPU: a plain run prints the headline line only (no
roofline / kernel / CPU-baseline / all-reduce legs, those are --full's), --steps sets ms_per_step's
divisor, and --dump-outputs writes the last timed step's outputs as float32 / float64 .npy files
within the 64 MB budget, from inputs that are the same in every run."""
import json
import os
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

ROOT = Path(__file__).resolve().parents[1]
SMALL = ("--gpus", "1", "--config", "c2", "--envs", "512", "--rollout", "16", "--minibatch", "4096", "--epochs", "1",
         "--steps", "2", "--warmup", "1")


def _bench(*args):
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_PORT")}
    r = subprocess.run([sys.executable, str(ROOT / "bench.py"), *SMALL, *args], cwd=ROOT, env=env, capture_output=True,
                       text=True, timeout=110)
    assert r.returncode == 0, r.stderr[-4000:]
    lines = [json.loads(ln) for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout
    return lines[0]


@pytest.fixture(scope="module")
def dumped(tmp_path_factory):
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    out = tmp_path_factory.mktemp("dump")
    return _bench("--dump-outputs", str(out)), out


def test_plain_run_prints_the_headline_line_only(dumped):
    j, _ = dumped
    assert j["steps"] == 2 and j["warmup"] == 1 and j["n_gpus"] == 1 and j["finite"]
    assert j["unit"] == "env-steps/s" and j["higher_is_better"] is True and j["dtype"].startswith("fp32")
    assert j["ms_per_step"] > 0
    assert j["value"] == pytest.approx(512 * 16 / (j["ms_per_step"] * 1e-3), rel=1e-6)
    for leg in ("roofline", "cpu_baseline", "allreduce", "kernels"):
        assert j[leg] is None, leg


def test_dump_outputs_writes_the_last_steps_arrays(dumped):
    _, out = dumped
    files = {p.stem: np.load(p) for p in out.glob("*.npy")}
    for name in ("params", "adam_m", "adam_v", "stats", "rollout_obs", "rollout_logits", "rollout_adv"):
        assert name in files, sorted(files)
    assert all(a.dtype in (np.float32, np.float64) for a in files.values())
    assert sum(a.nbytes for a in files.values()) <= 64 << 20
    assert all(np.isfinite(a).all() for a in files.values())
    assert files["rollout_obs"].shape == (17, 512, 6) and files["rollout_logits"].shape == (16, 512, 2)
    assert np.abs(files["adam_m"]).max() > 0 and np.abs(files["rollout_adv"]).max() > 0  # the update ran


def test_large_outputs_are_a_fixed_sample(tmp_path):
    sys.path.insert(0, str(ROOT))
    import bench

    if not torch.cuda.is_available():
        pytest.skip("no HIP device")

    class _P:
        flat = torch.arange(bench.DUMP_MAX_ELEMS * 3 + 5, dtype=torch.float32, device="cuda")

    small = torch.zeros(3, device="cuda")

    class _A:
        params = _P
        adam_m = adam_v = grad = dyn = small
        stats = ep_stats = torch.ones(2, 2, dtype=torch.float64, device="cuda")
        buf = {"dones": torch.ones(4, 2, dtype=torch.uint8, device="cuda")}

    d1, d2 = tmp_path / "a", tmp_path / "b"
    bench.dump_outputs(_A, torch, d1)
    bench.dump_outputs(_A, torch, d2)
    a, b = np.load(d1 / "params.npy"), np.load(d2 / "params.npy")
    assert a.shape == (bench.DUMP_MAX_ELEMS,) and a.dtype == np.float32 and np.array_equal(a, b)
    assert (np.diff(a) >= 0).all() and a.max() < _P.flat.numel()  # sorted element indices of the flat array
    assert np.load(d1 / "stats.npy").dtype == np.float64
    assert np.load(d1 / "rollout_dones.npy").dtype == np.float32
