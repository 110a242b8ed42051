"""observation_filter="MeanStdFilter": the running per-column mean / std of the observations, kept on
the device (rlks_obs_filter_*, include/rlks.h).

RLlib's MeanStdFilter standardises each observation as (x - mean) / (std + 1e-8) with the unbiased
running variance.  RLlib updates its local filter per observation and synchronises its workers once
per iteration; here the filter is frozen while a rollout runs and every raw observation of the rollout
is merged afterwards (batch-synchronous), so the first iteration runs the identity filter.  RLlib is
absent from the reference tree: parity unpinned, the arithmetic is pinned by tests/obs_filter_ref.py.
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _lib

FILTERS = ("NoFilter", "MeanStdFilter")


def validate_observation_filter(name):
    """"NoFilter" or "MeanStdFilter"; anything else (RLlib's "ConcurrentMeanStdFilter" and callables
    included) raises ValueError"""
    if not isinstance(name, str) or name not in FILTERS:
        raise ValueError(f"observation_filter must be one of {FILTERS}, got {name!r}")
    return name


class ObsFilter:
    """the device state double[1 + 3 D] = count, mean[D], m2[D], inv[D] and its launches, all on
    torch's current stream"""

    def __init__(self, D, device):
        import torch

        self.D = int(D)
        size = _lib.lib().rlks_obs_filter_size(self.D)
        _lib.check(min(size, 0), "rlks_obs_filter_size")
        self.device = torch.device(device)
        self.state = torch.empty(size, dtype=torch.float64, device=self.device)
        self.record = torch.zeros(_lib.RLKS_OFR_SUMS + 2 * self.D, dtype=torch.float64, device=self.device)
        self.ws = None
        _lib.call("rlks_obs_filter_init", _lib.ptr(self.state), self.D, self._stream())

    def _stream(self):
        import torch

        return torch.cuda.current_stream(self.device).cuda_stream

    def apply(self, x, out=None):
        """filter(x) for x [..., D] (contiguous float32 device tensor) into `out` (may be x); the state
        is read, never updated"""
        import torch

        if out is None:
            out = torch.empty_like(x)
        _lib.call("rlks_obs_filter_apply", _lib.ptr(self.state), _lib.ptr(x), _lib.ptr(out), x.numel() // self.D,
                  self.D, self._stream())
        return out

    def reserve(self, rows):
        """the stats workspace for up to `rows` rows"""
        import torch

        b = C.c_int64()
        _lib.call("rlks_obs_filter_workspace_bytes", int(rows), self.D, C.byref(b))
        if self.ws is None or self.ws.numel() * 8 < b.value:
            self.ws = torch.empty(max(1, b.value // 8), dtype=torch.float64, device=self.device)

    def stats(self, x):
        """self.record <- the batch record of x [rows, D]"""
        rows = x.numel() // self.D
        self.reserve(rows)
        _lib.call("rlks_obs_filter_stats", _lib.ptr(self.state), _lib.ptr(x), rows, self.D, _lib.ptr(self.record),
                  _lib.ptr(self.ws), self.ws.numel() * 8, self._stream())
        return self.record

    def merge(self, record=None):
        rec = self.record if record is None else record
        _lib.call("rlks_obs_filter_merge", _lib.ptr(self.state), _lib.ptr(rec), self.D, self._stream())

    # ---- host views (each synchronises)
    def numpy(self):
        """(count, mean[D], m2[D], inv[D]) as float64"""
        s = self.state.cpu().numpy()
        D, v = self.D, _lib.RLKS_OF_VECS
        return (float(s[_lib.RLKS_OF_COUNT]), s[v + _lib.RLKS_OF_MEAN * D: v + (_lib.RLKS_OF_MEAN + 1) * D].copy(),
                s[v + _lib.RLKS_OF_M2 * D: v + (_lib.RLKS_OF_M2 + 1) * D].copy(),
                s[v + _lib.RLKS_OF_INV * D: v + (_lib.RLKS_OF_INV + 1) * D].copy())

    def summary(self):
        """{"count", "mean", "std"}: std is the unbiased one the filter divides by (0 below two rows)"""
        n, mean, m2, _ = self.numpy()
        std = np.sqrt(m2 / (n - 1.0)) if n >= 2 else np.zeros_like(m2)
        return {"count": int(n), "mean": [float(x) for x in mean], "std": [float(x) for x in std]}

    def load(self, count, mean, m2, inv=None):
        """set the state from host (count, mean, m2); inv as saved, else by the merge's formula in
        float64"""
        import torch

        n = float(count)
        mean = np.asarray(mean, np.float64).reshape(self.D)
        m2 = np.asarray(m2, np.float64).reshape(self.D)
        if inv is not None:
            inv = np.asarray(inv, np.float64).reshape(self.D)
        else:
            inv = 1.0 / (np.sqrt(m2 / (n - 1.0)) + 1e-8) if n >= 2 else np.ones(self.D)
        s = np.concatenate([[n], mean, m2, inv]).astype(np.float64)
        self.state.copy_(torch.from_numpy(s).to(self.device))
