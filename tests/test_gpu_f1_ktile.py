"""The k-tile-major F1b of the fused kernel k_sf_f1 (f1b_kt_body): up to 4 actions with three
products, dH1 is finished one k-tile a step, and each k-tile's dZ1 / dW1 epilogue and workgroup sum run
beside the next k-tiles' MFMAs.  dH1 and dZ1 keep the parent's bits (the accumulator chains are unchanged);
dZ1 is split at each k-tile's own power of two instead of the 16-row tile's, which can only add bits to dW1 / db1.

Shapes: 256 rows (one workgroup a net), 512 and 1,024 (several workgroups, both nets mixed over the grid),
A in {2, 4} with D = 3 A.  Cases (tests/f1_ktile_cases.py): the plain inputs at all three sizes, and at 256 and
512 rows three regimes in which a k-tile's exponent differs from its tile's (a saturated block of 16 hidden
units, a k-tile of zero W2 columns, a 16-row tile without any loss gradient).

Every case is computed once (split kernels, three fused runs, the float64 oracle and its fp32 band) and
shared by the tests:
  fused vs split     each tensor within 1e-6 of its norm of the split kernels' (RLKS_F1_SPLIT=1), the rule of
                     test_fused_f1_is_deterministic_and_matches_split_kernels; three fused runs bit-identical
  per element        against float64 in the band of tests/parity.py grad_close_as_fp32 (w1 / b1 of both nets are
                     checked tensor by tensor there: weights against their cancellation scale, biases relative)
  regimes            finite, and the same two bounds
  parent             max and p99 of the per-element error of w1 / b1 of both nets no larger than the parent
                     commit's on the same inputs (profiles/r14_f1_ktile/parent_w1_b1_err.json, written by
                     tools/f1_ktile_parent_err.py with the parent's library); no margin
"""
import ctypes as C
import json
import os
from pathlib import Path

import numpy as np
import pytest

from f1_ktile_cases import (ACTIONS, REGIME_ROWS, REGIMES, ROWS, W1_B1, Case, all_cases, case_id, w1_b1_digest,
                            w1_b1_errors)
from parity import grad_close_as_fp32

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

PARENT_ERR = Path(__file__).resolve().parents[1] / "profiles" / "r14_f1_ktile" / "parent_w1_b1_err.json"
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


def _fused_vs_split(r):
    from rlks import _lib
    from rlks.policy import TENSOR_NAMES

    c, (gs, ss), (gf, sf) = r["case"], r["split"], r["fused"][0]
    assert np.any(gf != 0) and sf[_lib.RLKS_STAT_ROWS] == c.rows
    for g2, s2 in r["fused"][1:]:
        np.testing.assert_array_equal(g2.view(np.uint32), gf.view(np.uint32))
        np.testing.assert_array_equal(s2.view(np.uint64), sf.view(np.uint64))
    for i, (name, _, _) in enumerate(TENSOR_NAMES):
        o, n = c.p.offsets[i], int(np.prod(c.p.shapes[i]))
        a, b = gf[o:o + n].astype(np.float64), gs[o:o + n].astype(np.float64)
        print(f"{name}: |fused - split| / |split| = {np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-300):.3e}")
        assert np.linalg.norm(a - b) <= 1e-6 * np.linalg.norm(b) + 1e-12, name
    np.testing.assert_allclose(sf, ss, rtol=1e-6)


def _per_element(r):
    c, (gf, _) = r["case"], r["fused"][0]
    assert np.isfinite(gf).all()
    for i, (mx, p99) in w1_b1_errors(gf, r["eg"], r["est"]["scale"], c.p.offsets, c.p.shapes).items():
        print(f"tensor {i}: per-element error max {mx:.3e} p99 {p99:.3e}")
    grad_close_as_fp32(gf, r["eg"], r["eg32"], c.p.offsets, c.p.shapes, scale=r["est"]["scale"])


@pytest.mark.parametrize("A", ACTIONS)
@pytest.mark.parametrize("rows", ROWS)
def test_ktile_fused_matches_split_and_repeats(rows, A):
    _fused_vs_split(_result("plain", rows, A))


@pytest.mark.parametrize("A", ACTIONS)
@pytest.mark.parametrize("rows", ROWS)
def test_ktile_w1_b1_per_element(rows, A):
    _per_element(_result("plain", rows, A))


@pytest.mark.parametrize("A", ACTIONS)
@pytest.mark.parametrize("rows", REGIME_ROWS)
@pytest.mark.parametrize("regime", REGIMES)
def test_ktile_scale_regimes(regime, rows, A):
    """a k-tile whose split exponent differs from its 16-row tile's: finite, and both bounds"""
    r = _result(regime, rows, A)
    for g, s in r["fused"] + [r["split"]]:
        assert np.isfinite(g).all() and np.isfinite(s).all()
    _fused_vs_split(r)
    _per_element(r)


@pytest.mark.parametrize("regime,rows,A", all_cases(), ids=[case_id(*c) for c in all_cases()])
def test_ktile_w1_b1_no_worse_than_parent(regime, rows, A):
    """the per-k-tile exponent can only add bits: max and p99 of the per-element error of w1 / b1 of both nets
    do not exceed the parent commit's on the same inputs (recorded; no margin).  The record also holds a digest of
    the parent's four tensors: where the tree's are byte-identical there is nothing to compare"""
    r = _result(regime, rows, A)
    c = r["case"]
    rec = json.loads(PARENT_ERR.read_text())
    parent = rec["cases"][case_id(regime, rows, A)]
    if w1_b1_digest(r["fused"][0][0], c.p.offsets, c.p.shapes) == rec["sha"][case_id(regime, rows, A)]:
        print("w1 / b1 of both nets byte-identical to the parent's")
        return  # the same tensors have the same error, whatever the last bits of this host's float64 oracle
    mine = w1_b1_errors(r["fused"][0][0], r["eg"], r["est"]["scale"], c.p.offsets, c.p.shapes)
    for i in W1_B1:
        pm, p99 = parent[str(i)]
        print(f"tensor {i}: max {mine[i][0]:.6e} (parent {pm:.6e})  p99 {mine[i][1]:.6e} (parent {p99:.6e})")
    for i in W1_B1:
        pm, p99 = parent[str(i)]
        assert mine[i][0] <= pm, f"tensor {i} max: {mine[i][0]:.6e} > parent {pm:.6e}"
        assert mine[i][1] <= p99, f"tensor {i} p99: {mine[i][1]:.6e} > parent {p99:.6e}"
