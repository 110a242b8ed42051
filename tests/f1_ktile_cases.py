"""Inputs and error measures shared by tests/test_gpu_f1_ktile.py and tools/f1_ktile_parent_err.py
(the k-tile-major F1b of the fused kernel k_sf_f1).  Importing needs no GPU.

A case is (regime, rows, A) with D = 3 A:
  plain       the inputs of tests/test_gpu_f1_persistent.py
  saturated   hidden units [32, 48) of both nets (k-tile 2) pushed into tanh's tail by b1 = 15: 1 - H1^2 ~ 4e-13
              there, so that k-tile's dZ1 sits ~2^-40 below its 16-row tile's maximum
  zero_w2     columns [64, 80) of both nets' W2 zero: dH1, and so dZ1, of k-tile 4 is exactly zero
  zero_tile   rows [16, 32) (and [288, 304) from 512 rows on) with no loss gradient at all: the advantage equal
              to adv_mean with kl_coeff = entropy_coeff = 0, and the value target outside vf_clip_param, so
              those tiles' dZ2 is exactly zero (its split exponent is the largest one)
"""
import ctypes as C
import hashlib

import numpy as np

REGIMES = ("saturated", "zero_w2", "zero_tile")
ROWS = (256, 512, 1024)
REGIME_ROWS = (256, 512)
ACTIONS = (2, 4)
ADV_MEAN, ADV_INV_STD = 0.3, 0.7
W1_B1 = (0, 1, 6, 7)  # w1, b1 of the policy and the value net (rlks.policy.TENSOR_NAMES order)


def case_id(regime, rows, A):
    return f"{regime}-{rows}-A{A}"


def all_cases():
    return [("plain", r, a) for r in ROWS for a in ACTIONS] + \
           [(g, r, a) for g in REGIMES for r in REGIME_ROWS for a in ACTIONS]


class Case:
    """parameters, minibatch and loss coefficients of one case, and the library calls on them"""

    def __init__(self, regime, rows, A, dev):
        import torch
        from rlks import _lib
        from rlks.policy import PolicyParams

        self.torch, self.lib, self.d, self.rows, self.A, self.D = torch, _lib, dev, rows, A, 3 * A
        D = self.D
        p = PolicyParams(D, 256, A, device=dev, seed=rows + A)
        g = torch.Generator().manual_seed(rows + A + 1)
        for i in (1, 3, 5, 7, 9, 11):  # non-zero biases
            v = p.view(i)
            v.copy_((torch.randn(v.shape, generator=g) * 0.1).to(dev))
        if regime == "saturated":
            for net in (0, 1):
                p.view(6 * net + 1)[32:48] = 15.0
        if regime == "zero_w2":
            for net in (0, 1):
                p.view(6 * net + 2)[:, 64:80] = 0.0
        p.desc.precision = _lib.RLKS_PRECISION_SF16
        rng = np.random.default_rng(rows + 7 * A)
        stride = (D + A + 4 + 3) // 4 * 4
        mb = np.zeros((rows, stride), np.float32)
        mb[:, :D] = rng.random((rows, D))
        lg, vv = p.forward(torch.from_numpy(mb[:, :D].copy()).to(dev))
        vv = vv.cpu().numpy()
        lo = lg.cpu().numpy() + rng.standard_normal((rows, A)).astype(np.float32) * 0.3
        mb[:, D:D + A] = lo
        mb[:, D + A] = rng.standard_normal(rows) * 3 + 0.5
        mb[:, D + A + 1] = vv + rng.standard_normal(rows).astype(np.float32) * 4
        act = rng.integers(0, A, rows)
        mb[:, D + A + 3] = act
        lsm = lo - np.log(np.exp(lo - lo.max(1, keepdims=True)).sum(1, keepdims=True)) - lo.max(1, keepdims=True)
        mb[:, D + A + 2] = lsm[np.arange(rows), act]
        self.kl, self.ent = 0.2, 0.01
        if regime == "zero_tile":
            self.kl, self.ent = 0.0, 0.0
            for r0 in (16, 288):
                if r0 + 16 <= rows:
                    mb[r0:r0 + 16, D + A] = np.float32(ADV_MEAN)
                    mb[r0:r0 + 16, D + A + 1] = vv[r0:r0 + 16] + 100.0
        self.p, self.mb = p, mb
        self.mbt = torch.from_numpy(mb).to(dev)
        self.dyn = torch.tensor([ADV_MEAN, ADV_INV_STD, self.kl, 1.0 / rows, 0, 0, 0, 0], dtype=torch.float32, device=dev)
        self.co = _lib.PpoCoeffs(0.3, 10.0, 1.0, self.ent)
        wsb = C.c_int64()
        _lib.call("rlks_ppo_workspace_bytes", C.byref(p.desc), rows, C.byref(wsb))
        self.wsb = wsb.value

    def run(self):
        """one rlks_ppo_grad on a zeroed workspace -> (gradient, stats)"""
        torch, p = self.torch, self.p
        ws = torch.zeros(self.wsb, dtype=torch.uint8, device=self.d)
        g = torch.zeros(p.padded, device=self.d)
        st = torch.zeros(8, dtype=torch.float64, device=self.d)
        self.lib.call("rlks_ppo_grad", C.byref(p.desc), C.byref(self.co), p.flat.data_ptr(), self.dyn.data_ptr(),
                      self.mbt.data_ptr(), self.rows, g.data_ptr(), st.data_ptr(), ws.data_ptr(), ws.numel(), None)
        torch.cuda.synchronize()
        return g.cpu().numpy(), st.cpu().numpy()

    def oracle(self):
        """(float64 gradient, its stats with the cancellation scales, the fp32 band)"""
        import oracle

        flat, p = self.p.flat.cpu().numpy(), self.p
        kw = dict(entropy_coeff=self.ent, kl_coeff=self.kl, adv_mean=ADV_MEAN, adv_inv_std=ADV_INV_STD)
        eg, est = oracle.ppo_loss_grad(flat, p.offsets, self.D, 256, self.A, self.mb, scale=True, **kw)
        eg32 = oracle.ppo_loss_grad_fp32_band(flat, p.offsets, self.D, 256, self.A, self.mb, **kw)
        return eg, est, eg32


def w1_b1_errors(g, g64, scale, offsets, shapes):
    """{tensor index: (max, p99)} of the per-element error of dW1 / db1 of both nets, in the form
    tests/parity.py grad_close_as_fp32 takes them: a weight element against its own cancellation scale
    (|g - g64| / s over s > 0), a bias element relative (|g - g64| / |g64| over |g64| > 1e-6 max |g64|)"""
    out = {}
    for i in W1_B1:
        o, n = offsets[i], int(np.prod(shapes[i]))
        x, r = np.asarray(g[o:o + n], np.float64), np.asarray(g64[o:o + n], np.float64)
        if i in (0, 6):
            s = np.asarray(scale[o:o + n], np.float64)
            keep = s > 0
            e = np.abs(x - r)[keep] / s[keep]
        else:
            keep = np.abs(r) > 1e-6 * np.abs(r).max()
            e = np.abs(x - r)[keep] / np.abs(r[keep])
        out[i] = (float(e.max()), float(np.percentile(e, 99)))
    return out


def w1_b1_digest(g, offsets, shapes):
    """a digest of the four tensors' bytes: equal digests are byte-identical results"""
    h = hashlib.sha256()
    for i in W1_B1:
        o, n = offsets[i], int(np.prod(shapes[i]))
        h.update(np.ascontiguousarray(g[o:o + n]).tobytes())
    return h.hexdigest()[:16]
