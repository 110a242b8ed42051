"""The fused F1 kernel k_sf_f1 after DESIGN.md §25: the k-tile-major F1b finishes each k-tile's wave max, split
exponent and powers of two on the scalar unit, on bit patterns (csrc/sf_exp.h).  (§25 also tried H1 produced a
k-tile ahead in F1a's Z2 loop and the chain of F1b's k-tile 0 run behind the barrier that ends F1a's epilogue;
both passed these tests and measured slower, so they are not in the kernel.)  A maximum is exact in any order
and the integer forms give the floats' bits; every MFMA accumulator chain keeps its order and every element
sees the same VALU operations, so the whole gradient and the stats are the parent commit's to the byte.

Cases: those of tests/f1_ktile_cases.py (256 / 512 / 1,024 rows x A in {2, 4} plain, and the saturated /
zero-W2 / zero-tile regimes at 256 and 512 rows), plus 768 rows (three workgroups a net: an odd count).
Every case is computed once (split kernels, three fused runs, the float64 oracle and its fp32 band) and
shared by the tests:
  repeats            three fused runs bit-identical
  fused vs split     each tensor within 1e-6 of its norm of the split kernels' (RLKS_F1_SPLIT=1, which keep
                     the loop that produces H1 at the head of its own k-tile)
  per element        the band of tests/parity.py grad_close_as_fp32
  parent             sha256 of the whole gradient and of the stats equal to the parent commit's
                     (profiles/r16_f1a_ahead/parent_digests.json, written by tools/f1a_ahead_digests.py with the
                     parent's library); no margin
"""
import ctypes as C
import hashlib
import json
import os
from pathlib import Path

import numpy as np
import pytest

from f1_ktile_cases import ACTIONS, Case, all_cases, case_id
from parity import grad_close_as_fp32

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

PARENT = Path(__file__).resolve().parents[1] / "profiles" / "r16_f1a_ahead" / "parent_digests.json"
CASES = all_cases() + [("plain", 768, a) for a in ACTIONS]
IDS = [case_id(*c) for c in CASES]
_results = {}


def _result(regime, rows, A):
    """the case's gradients (split once, fused three times) and references, computed once a session"""
    key = (regime, rows, A)
    if key in _results:
        return _results[key]
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    from rlks import _lib

    saved = {k: os.environ.pop(k, None) for k in ("RLKS_F1_FUSED", "RLKS_F1_SPLIT")}
    try:
        c = Case(regime, rows, A, torch.device("cuda", 0))
        os.environ["RLKS_F1_SPLIT"] = "1"
        split = c.run()
        del os.environ["RLKS_F1_SPLIT"]
        assert _lib.lib().rlks_sf_f1_fused(C.byref(c.p.desc)) == 1  # the default form at these action counts
        fused = [c.run() for _ in range(3)]
    finally:
        os.environ.pop("RLKS_F1_SPLIT", None)
        for k, v in saved.items():
            if v is not None:
                os.environ[k] = v
    eg, est, eg32 = c.oracle()
    _results[key] = dict(case=c, split=split, fused=fused, eg=eg, est=est, eg32=eg32)
    return _results[key]


def _sha(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


@pytest.mark.parametrize("regime,rows,A", CASES, ids=IDS)
def test_f1a_ahead_repeats_and_matches_split(regime, rows, A):
    from rlks import _lib
    from rlks.policy import TENSOR_NAMES

    r = _result(regime, rows, A)
    c, (gs, ss), (gf, sf) = r["case"], r["split"], r["fused"][0]
    assert np.isfinite(gf).all() and np.isfinite(sf).all()
    assert np.any(gf != 0) and sf[_lib.RLKS_STAT_ROWS] == rows
    for g2, s2 in r["fused"][1:]:
        np.testing.assert_array_equal(g2.view(np.uint32), gf.view(np.uint32))
        np.testing.assert_array_equal(s2.view(np.uint64), sf.view(np.uint64))
    for i, (name, _, _) in enumerate(TENSOR_NAMES):
        o, n = c.p.offsets[i], int(np.prod(c.p.shapes[i]))
        a, b = gf[o:o + n].astype(np.float64), gs[o:o + n].astype(np.float64)
        print(f"{name}: |fused - split| / |split| = {np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-300):.3e}")
        assert np.linalg.norm(a - b) <= 1e-6 * np.linalg.norm(b) + 1e-12, name
    np.testing.assert_allclose(sf, ss, rtol=1e-6)


@pytest.mark.parametrize("regime,rows,A", CASES, ids=IDS)
def test_f1a_ahead_per_element(regime, rows, A):
    r = _result(regime, rows, A)
    c, (gf, _) = r["case"], r["fused"][0]
    grad_close_as_fp32(gf, r["eg"], r["eg32"], c.p.offsets, c.p.shapes, scale=r["est"]["scale"])


@pytest.mark.parametrize("regime,rows,A", CASES, ids=IDS)
def test_f1a_ahead_bytes_are_the_parents(regime, rows, A):
    r = _result(regime, rows, A)
    gf, sf = r["fused"][0]
    parent = json.loads(PARENT.read_text())["cases"][case_id(regime, rows, A)]
    print(f"grad {_sha(gf)} (parent {parent['grad']})  stats {_sha(sf)} (parent {parent['stats']})")
    assert _sha(gf) == parent["grad"]
    assert _sha(sf) == parent["stats"]
