"""Serving a trained policy: observations in, decisions out, one kernel launch a call.

``PolicyServer.act`` is what the reference's evaluation loops call 10,000 times
(``compute_single_action``, eval_ppo.py:27, final_evaluation.py:48) without the trainer behind it: the
server holds a ``PolicyParams``, optionally an ``ObsFilter`` state, and one block of pinned, device-visible
host memory (rlks_host_alloc).  A call writes the observations and the packed mask words into the block
with numpy, launches ``rlks_policy_act`` on the block's device pointers, synchronises the stream and reads
the results out of the block: no torch op, no allocation and no explicit copy on the path.

    server = PolicyServer.from_checkpoint(path)        # no env, no rollout buffers, no Adam state
    action = server.act(obs)                           # obs [D] -> int
    actions, info = server.act(batch, full_fetch=True) # [n, D] -> int32 [n], RLlib's extra-fetch names

The draw is the shared one: row i of the server's k-th exploring call draws
Philox({SAMPLER_ID, i, k, ACTION}, key = seed), the scheme of ``rlks.sampling.sample_rows`` (which
``PPO.compute_actions`` calls with its own counter).  A policy outside the kernel's scope (hidden != 256,
obs_dim > 192, more than 64 actions) is served by ``params.forward`` + ``sample_rows``: ``server.fused`` is False.
"""
from __future__ import annotations

import ctypes as C
import json
from pathlib import Path

import numpy as np

from . import _lib
from .sampling import SAMPLER_ID, pack_mask, sample_rows  # (SAMPLER_ID and pack_mask: public names of this module too)


def check_inputs(D, A, max_rows, masked, obs, action_mask=None):
    """-> (obs float32 [n, D], mask words uint64 [n] or None, single).  ValueError for a wrong D, more
    rows than the staging block holds, a wrong mask shape, or a masked policy asked to act unmasked
    (the rule of PPO.compute_actions: a masked policy acting unmasked would be a silent error).  Host only."""
    if hasattr(obs, "detach"):
        obs = obs.detach().cpu().numpy()
    x = np.asarray(obs, dtype=np.float32)
    single = x.ndim == 1
    if single:
        x = x[None, :]
    if x.ndim != 2 or x.shape[1] != D:
        raise ValueError(f"obs must be [{D}] or [n, {D}], got {list(np.shape(obs))}")
    n = x.shape[0]
    if n > max_rows:
        raise ValueError(f"{n} rows exceed this server's max_rows = {max_rows}: build it with a larger max_rows, "
                         "or use PPO.compute_actions for bulk work")
    bits = None
    if action_mask is not None:
        bits = pack_mask(action_mask, n, A)
    elif masked:
        raise ValueError("this policy was trained with action_mask='room': pass action_mask (bool [A] or [n, A]); "
                         "a masked policy acting unmasked would be a silent error")
    return x, bits, single


def _align(o, a=16):
    return (o + a - 1) // a * a


class PolicyServer:
    """act() over a PolicyParams.  `obs_filter`: an rlks.obs_filter.ObsFilter whose state every
    observation goes through first (read, never updated).  `masked`: the policy was trained with
    action_mask="room", so act() must be given a mask.  `seed`: the draw's Philox key.  `max_rows`: the
    most rows one act() takes (the staging block's size).  `explore`: act()'s default."""

    def __init__(self, params, *, obs_filter=None, masked=False, seed=0, max_rows=1024, device=None, explore=True):
        import torch

        self.max_rows = int(max_rows)
        if self.max_rows < 1:
            raise ValueError(f"max_rows must be at least 1, got {max_rows}")
        self.params = params
        self.D, self.H, self.A = params.D, params.H, params.A
        if obs_filter is not None and obs_filter.D != self.D:
            raise ValueError(f"the observation filter has {obs_filter.D} columns, the policy {self.D}")
        self.obs_filter = obs_filter
        self.masked = bool(masked)
        self.seed = int(seed or 0) & 0xFFFFFFFFFFFFFFFF
        self.explore = bool(explore)
        self.calls = 0  # exploring act() calls so far: the draws' counter word 2
        if device is None:
            device = params.flat.device if params.flat.is_cuda else torch.device("cuda", torch.cuda.current_device())
        self.device = torch.device(device)
        self._torch = torch
        self._desc = _lib.MlpDesc(self.D, self.H, self.A, 0)
        self._fn = _lib.lib().rlks_policy_act
        # the staging block: obs | mask words | actions | logp | logits | probs | values, each 16-byte aligned
        R, D, A = self.max_rows, self.D, self.A
        sizes = [("obs", 4 * R * D), ("mask", 8 * R), ("actions", 4 * R), ("logp", 4 * R), ("logits", 4 * R * A),
                 ("probs", 4 * R * A), ("values", 4 * R)]
        off, o = {}, 0
        for name, b in sizes:
            off[name] = o
            o = _align(o + b)
        self._host, self._dev = C.c_void_p(), C.c_void_p()
        with torch.cuda.device(self.device):
            _lib.call("rlks_host_alloc", o, C.byref(self._host), C.byref(self._dev))
        raw = np.ctypeslib.as_array((C.c_ubyte * o).from_address(self._host.value))
        raw[:] = 0

        def view(name, dtype, shape):
            n = int(np.prod(shape)) * np.dtype(dtype).itemsize
            return raw[off[name]: off[name] + n].view(dtype).reshape(shape)

        self._obs = view("obs", np.float32, (R, D))
        self._mask = view("mask", np.uint64, (R,))
        self._actions = view("actions", np.int32, (R,))
        self._logp = view("logp", np.float32, (R,))
        self._logits = view("logits", np.float32, (R, A))
        self._probs = view("probs", np.float32, (R, A))
        self._values = view("values", np.float32, (R,))
        self._d = {name: C.c_void_p(self._dev.value + off[name]) for name, _ in sizes}
        # in scope?  The library decides (n = 0: the argument checks run, nothing is launched)
        rc = self._fn(C.byref(self._desc), params.flat.data_ptr(), None, self._d["obs"], None, 0, 0, 0, 0, 0,
                      self._d["actions"], None, None, None, None, None)
        if rc not in (0, -3):
            _lib.check(rc, "rlks_policy_act")
        self.fused = rc == 0

    def close(self):
        """free the staging block (also on garbage collection)"""
        h, self._host = getattr(self, "_host", None), None
        if h is not None and h.value:
            for k in ("_obs", "_mask", "_actions", "_logp", "_logits", "_probs", "_values"):
                setattr(self, k, None)
            _lib.lib().rlks_host_free(h)

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    @classmethod
    def from_checkpoint(cls, path, *, max_rows=1024, device=None):
        """a server from a checkpoint written by PPO.save(): algorithm_state.json (seed, explore,
        action_mask, the filter's name) and state.pt (weights/*, obs_filter/*).  Builds a PolicyParams and,
        with a filter, an ObsFilter: no env, no rollout buffers, no optimizer state."""
        import torch

        from .obs_filter import ObsFilter
        from .policy import TENSOR_NAMES, PolicyParams

        path = Path(path)
        meta = json.loads((path / "algorithm_state.json").read_text())
        cfg = meta["config"]
        sp = path / "state.pt"
        if not sp.exists():  # a multi-rank run: every rank holds the same weights and filter state
            sp = path / "state.rank0.pt"
        tensors = torch.load(sp, weights_only=True)
        sd = {k[len("weights/"):]: v for k, v in tensors.items() if k.startswith("weights/")}
        H, D = sd[TENSOR_NAMES[0][0]].shape
        A = sd[TENSOR_NAMES[4][0]].shape[0]
        if device is None:
            device = torch.device("cuda", torch.cuda.current_device())
        device = torch.device(device)
        with torch.cuda.device(device):
            params = PolicyParams(D, H, A, device=device, seed=0)
            for i, (name, _, _) in enumerate(TENSOR_NAMES):
                if tuple(sd[name].shape) != tuple(params.shapes[i]):
                    raise ValueError(f"checkpoint tensor {name} has shape {tuple(sd[name].shape)}, expected "
                                     f"{tuple(params.shapes[i])}")
            params.load_state_dict(sd)
            of = {k[len("obs_filter/"):]: v for k, v in tensors.items() if k.startswith("obs_filter/")}
            filt = None
            if of:
                filt = ObsFilter(D, device)
                filt.load(float(of["count"][0]), of["mean"].numpy(), of["m2"].numpy(), of["inv"].numpy())
                params.obs_filter = filt  # the fallback's params.forward filters too
        return cls(params, obs_filter=filt, masked=cfg.get("action_mask") is not None, seed=cfg.get("seed") or 0,
                   max_rows=max_rows, device=device, explore=bool(cfg.get("explore", True)))

    def act(self, obs, *, explore=None, action_mask=None, full_fetch=False):
        """obs [D] -> int, obs [n, D] -> int32 [n]; with full_fetch also info = {"action_logp",
        "action_dist_inputs" (the logits drawn from), "action_prob", "vf_preds"} (RLlib's names for
        compute_single_action(full_fetch=True)); the value net runs only then.  action_mask: bool [A] or
        [n, A], True = allowed, a row without a True counts as all True.  Returned arrays are copies."""
        x, bits, single = check_inputs(self.D, self.A, self.max_rows, self.masked, obs, action_mask)
        n = x.shape[0]
        explore = self.explore if explore is None else bool(explore)
        if not self.fused:
            acts, info = self._act_unfused(x, bits, explore, full_fetch)
        else:
            acts, info = self._act_fused(x, bits, n, explore, full_fetch)
        if single:
            acts = int(acts[0])
            if info is not None:
                info = {"action_logp": float(info["action_logp"][0]), "action_dist_inputs": info["action_dist_inputs"][0],
                        "action_prob": info["action_prob"][0], "vf_preds": float(info["vf_preds"][0])}
        return (acts, info) if full_fetch else acts

    def _act_fused(self, x, bits, n, explore, full_fetch):
        if n == 0:
            e = np.zeros(0, np.float32)
            return np.zeros(0, np.int32), ({"action_logp": e, "action_dist_inputs": np.zeros((0, self.A), np.float32),
                                            "action_prob": np.zeros((0, self.A), np.float32), "vf_preds": e.copy()}
                                           if full_fetch else None)
        self._obs[:n] = x
        if bits is not None:
            self._mask[:n] = bits
        d = self._d
        stream = self._torch.cuda.current_stream(self.device)
        f = self.obs_filter
        rc = self._fn(C.byref(self._desc), self.params.flat.data_ptr(), f.state.data_ptr() if f is not None else None,
                      d["obs"], d["mask"] if bits is not None else None, n, int(explore), self.seed, SAMPLER_ID,
                      self.calls & 0xFFFFFFFF, d["actions"], d["logp"] if full_fetch else None,
                      d["logits"] if full_fetch else None, d["probs"] if full_fetch else None,
                      d["values"] if full_fetch else None, stream.cuda_stream)
        if rc != 0:
            _lib.check(rc, "rlks_policy_act")
        if explore:
            self.calls += 1
        stream.synchronize()
        acts = self._actions[:n].copy()
        if not full_fetch:
            return acts, None
        return acts, {"action_logp": self._logp[:n].copy(), "action_dist_inputs": self._logits[:n].copy(),
                      "action_prob": self._probs[:n].copy(), "vf_preds": self._values[:n].copy()}

    def _act_unfused(self, x, bits, explore, full_fetch):
        """outside the kernel's scope: compute_actions' sequence, params.forward then sampling.sample_rows"""
        torch = self._torch
        with torch.cuda.device(self.device):
            o = torch.from_numpy(np.ascontiguousarray(x)).to(self.device)
            if self.obs_filter is not None and self.params.obs_filter is None:
                o = self.obs_filter.apply(o)
            logits, values = self.params.forward(o)
            act, logp = sample_rows(logits, seed=self.seed, call=self.calls, explore=explore, bits=bits,
                                    want_logp=True, stream=torch.cuda.current_stream(self.device).cuda_stream)
            if explore:
                self.calls += 1
            acts = act.cpu().numpy()
            if not full_fetch:
                return acts, None
            return acts, {"action_logp": logp.cpu().numpy(), "action_dist_inputs": logits.cpu().numpy(),
                          "action_prob": torch.softmax(logits, 1).cpu().numpy(), "vf_preds": values.cpu().numpy()}
