"""The fused F1 kernel (k_sf_f1) at grids below, at and just above one workgroup per CU.

Written for the persistent form of the kernel (min(CUs, items) workgroups walking the (net, tile group)
items with a static stride, both nets' constants resident in LDS), which was built, measured slower than
one workgroup per item and left out.  The shapes keep their value for the kernel as it
is: the tile's split Xa image, F1b's first W2^T half-chunk and its first dZ2 fragment now pass from F1a
to F1b inside the workgroup (LDS and registers), and whatever walks or re-orders the items later has to
give the same bits at these sizes.  With n_cu read from the device:
  256 rows               one item per net: two workgroups, far fewer than CUs
  768 rows               an odd item count per net (6 items)
  256 (n_cu / 2 + 1)     n_cu + 2 items: two more than CUs (a second round of exactly two workgroups)
  256 (n_cu + 1)         2 n_cu + 2 items: two full rounds and two workgroups of a third
and one launch per net (rlks_ppo_grad_phases, RLKS_PHASE_FWD_PI then RLKS_PHASE_FWD_VF).

For each shape and A in {2, 4}: three fused gradients bit for bit the same; equal to the split kernels'
(RLKS_F1_SPLIT=1) by the rule of test_fused_f1_is_deterministic_and_matches_split_kernels (each tensor
within 1e-6 of its norm: the workgroup sums add 16 waves' slots instead of 8); and per element against
the float64 oracle no worse than fp32 (tests/parity.py).

At 256 (n_cu + 1) rows on a 256-CU device F2 (k_sf_dw2r, not part of this kernel) cannot run: 2,056
32-row chunks split 8 ways are 257 per workgroup, one more than it takes (the parent commit refuses the
same call).  That shape therefore runs PREP | FWD | REDUCE without DW2, and dW2 / db2, which F1 does not
produce, take a plain fp32 evaluation's values in the oracle comparison (neutral there: they are
compared with themselves); everything F1 produces (dW1, db1, dW3, db3 of both nets, the stats) is
checked as at the other shapes.
"""
import ctypes as C

import numpy as np
import pytest

import oracle
from parity import grad_close_as_fp32

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

W2_B2 = (2, 3, 8, 9)  # dW2, db2 of the policy and the value net in rlks.policy.TENSOR_NAMES order (F2's)


def _dev():
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    return torch.device("cuda", 0)


def _n_cu():
    return torch.cuda.get_device_properties(0).multi_processor_count


def _setup(rows, A, d):
    from rlks import _lib
    from rlks.policy import PolicyParams

    D = 3 * A
    p = PolicyParams(D, 256, A, device=d, seed=rows + A)
    g = torch.Generator().manual_seed(rows + A + 1)
    for i in (1, 3, 5, 7, 9, 11):  # non-zero biases
        v = p.view(i)
        v.copy_((torch.randn(v.shape, generator=g) * 0.1).to(d))
    p.desc.precision = _lib.RLKS_PRECISION_SF16
    rng = np.random.default_rng(rows + 7 * A)
    stride = (D + A + 4 + 3) // 4 * 4
    mb = np.zeros((rows, stride), np.float32)
    mb[:, :D] = rng.random((rows, D))
    lg, vv = p.forward(torch.from_numpy(mb[:, :D].copy()).to(d))
    lo = lg.cpu().numpy() + rng.standard_normal((rows, A)).astype(np.float32) * 0.3
    mb[:, D:D + A] = lo
    mb[:, D + A] = rng.standard_normal(rows) * 3 + 0.5
    mb[:, D + A + 1] = vv.cpu().numpy() + rng.standard_normal(rows).astype(np.float32) * 4
    act = rng.integers(0, A, rows)
    mb[:, D + A + 3] = act
    lsm = lo - np.log(np.exp(lo - lo.max(1, keepdims=True)).sum(1, keepdims=True)) - lo.max(1, keepdims=True)
    mb[:, D + A + 2] = lsm[np.arange(rows), act]
    return p, mb


class _Grad:
    """one (params, minibatch) and the calls on it"""

    def __init__(self, rows, A):
        from rlks import _lib

        self.lib, self.d, self.rows, self.A = _lib, _dev(), rows, A
        self.p, self.mb = _setup(rows, A, self.d)
        self.mbt = torch.from_numpy(self.mb).to(self.d)
        self.dyn = torch.tensor([0.3, 0.7, 0.2, 1.0 / rows, 0, 0, 0, 0], dtype=torch.float32, device=self.d)
        self.co = _lib.PpoCoeffs(0.3, 10.0, 1.0, 0.01)
        wsb = C.c_int64()
        _lib.call("rlks_ppo_workspace_bytes", C.byref(self.p.desc), rows, C.byref(wsb))
        self.wsb = wsb.value

    def run(self, *phase_calls):
        """rlks_ppo_grad, or rlks_ppo_grad_phases once per entry of phase_calls, on a zeroed workspace"""
        p, L = self.p, self.lib
        ws = torch.zeros(self.wsb, dtype=torch.uint8, device=self.d)
        g = torch.zeros(p.padded, device=self.d)
        st = torch.zeros(8, dtype=torch.float64, device=self.d)
        args = (C.byref(p.desc), C.byref(self.co), p.flat.data_ptr(), self.dyn.data_ptr(), self.mbt.data_ptr(),
                self.rows, g.data_ptr(), st.data_ptr(), ws.data_ptr(), ws.numel())
        if not phase_calls:
            L.call("rlks_ppo_grad", *args, None)
        for ph in phase_calls:
            L.call("rlks_ppo_grad_phases", *args, ph, None)
        torch.cuda.synchronize()
        return g.cpu().numpy(), st.cpu().numpy()


def _shapes():
    n = _n_cu() if torch.cuda.is_available() else 256
    return {"one_item": 256, "odd_items": 768, "two_walk_two": 256 * (n // 2 + 1), "all_walk_two": 256 * (n + 1)}


@pytest.mark.parametrize("A", [2, 4])
@pytest.mark.parametrize("shape", ["one_item", "odd_items", "two_walk_two", "all_walk_two"])
def test_persistent_f1_walk(shape, A, monkeypatch):
    """three fused gradients bit for bit the same, equal to the split kernels' up to the order of the
    workgroup sums, and per element no worse than fp32 against the float64 oracle (module docstring)"""
    from rlks import _lib
    from rlks.policy import TENSOR_NAMES

    _dev()
    rows = _shapes()[shape]
    G = _Grad(rows, A)
    p = G.p
    # F2 takes at most 256 32-row chunks per workgroup (see the module docstring)
    tiles, splits = rows // 32, 1
    while splits * 2 <= 128 and tiles % (splits * 2) == 0:
        splits *= 2
    with_f2 = tiles // splits <= 256
    assert with_f2 or shape == "all_walk_two"
    calls = () if with_f2 else (_lib.RLKS_PHASE_PREP | _lib.RLKS_PHASE_FWD | _lib.RLKS_PHASE_REDUCE,)

    monkeypatch.delenv("RLKS_F1_FUSED", raising=False)
    monkeypatch.setenv("RLKS_F1_SPLIT", "1")
    gs, ss = G.run(*calls)
    monkeypatch.delenv("RLKS_F1_SPLIT")
    assert _lib.lib().rlks_sf_f1_fused(C.byref(p.desc)) == 1  # the default form at these action counts
    runs = [G.run(*calls) for _ in range(3)]
    gf, sf = runs[0]
    assert np.any(gf != 0) and sf[_lib.RLKS_STAT_ROWS] == rows
    for g2, s2 in runs[1:]:
        np.testing.assert_array_equal(g2.view(np.uint32), gf.view(np.uint32))
        np.testing.assert_array_equal(s2.view(np.uint64), sf.view(np.uint64))
    for i, (name, _, _) in enumerate(TENSOR_NAMES):
        o, n = p.offsets[i], int(np.prod(p.shapes[i]))
        a, b = gf[o:o + n].astype(np.float64), gs[o:o + n].astype(np.float64)
        print(f"{shape} A={A} {name}: |fused - split| / |split| = {np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-300):.3e}")
        assert np.linalg.norm(a - b) <= 1e-6 * np.linalg.norm(b) + 1e-12, name
    np.testing.assert_allclose(sf, ss, rtol=1e-6)

    D = 3 * A
    flat = p.flat.cpu().numpy()
    kw = dict(entropy_coeff=0.01, kl_coeff=0.2, adv_mean=0.3, adv_inv_std=0.7)
    eg, est = oracle.ppo_loss_grad(flat, p.offsets, D, 256, A, G.mb, scale=True, **kw)
    eg32 = oracle.ppo_loss_grad_fp32_band(flat, p.offsets, D, 256, A, G.mb, **kw)
    g = gf.copy()
    if not with_f2:
        first = np.asarray(eg32[0] if isinstance(eg32, (list, tuple)) else eg32)
        for i in W2_B2:
            o, n = p.offsets[i], int(np.prod(p.shapes[i]))
            assert not np.any(g[o:o + n])  # F2 did not run
            g[o:o + n] = first[o:o + n]
    grad_close_as_fp32(g, eg, eg32, p.offsets, p.shapes, scale=est["scale"])
    for k, j in (("policy_loss", 0), ("vf_loss", 1), ("kl", 2), ("entropy", 3)):
        assert abs(sf[j] - est[k]) <= 1e-5 * max(abs(est[k]), 1e-3 * rows), k


@pytest.mark.parametrize("A", [2, 4])
def test_value_net_alone_launch(A, monkeypatch):
    """k_sf_f1 launched once per net (RLKS_PHASE_FWD_PI, then RLKS_PHASE_FWD_VF: net0 = 1, one net, the
    Xa split for F2 written again by the value net's launch) gives the two-net launch's gradient and
    stats bit for bit: every workgroup writes its own tile group's partials whatever the grid.  768
    rows: three workgroups per launch"""
    from rlks import _lib

    _dev()
    monkeypatch.delenv("RLKS_F1_FUSED", raising=False)
    monkeypatch.delenv("RLKS_F1_SPLIT", raising=False)
    G = _Grad(768, A)
    g0, s0 = G.run()
    g1, s1 = G.run(_lib.RLKS_PHASE_PREP | _lib.RLKS_PHASE_FWD_PI, _lib.RLKS_PHASE_FWD_VF,
                   _lib.RLKS_PHASE_DW2 | _lib.RLKS_PHASE_REDUCE)
    assert np.any(g0 != 0) and s0[_lib.RLKS_STAT_ROWS] == 768
    np.testing.assert_array_equal(g1.view(np.uint32), g0.view(np.uint32))
    np.testing.assert_array_equal(s1.view(np.uint64), s0.view(np.uint64))
