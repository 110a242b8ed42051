"""GPU tests of global-norm gradient clipping (include/rlks.h: rlks_grad_global_norm,
rlks_ppo_sgd_step_clip, rlks_ppo_adam_apply_clip; PPOConfig.grad_clip) and of the lr / entropy
schedules.

Step level, everything bit for bit: the reference of a case is rlks_ppo_grad, the device norm read
back (rlks_grad_global_norm), tests/clip_ref.clipped() on the host with that norm, rlks_adam_step.
The norm itself is checked against numpy's float64 norm to n_params * 2^-52 relative (the worst-case
rounding of a float64 sum of n exact terms).  Whole iteration: against clip_ref.ppo_iteration_clipped
in float64 with the bounds of test_gpu_agent.test_ppo_iteration_matches_fp64_oracle.
"""
import ctypes as C

import numpy as np
import pytest

import clip_ref

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

LR, B1, B2, EPS = 3e-3, 0.9, 0.999, 1e-8
STEPS = 5
SF16, FP32, WIDE = 1, 0, 2


def _dev():
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    return torch.device("cuda", 0)


def _bits(t):
    return t.view(torch.int32)


class Case:
    """a descriptor, STEPS minibatches (the recipe of test_fused_sgd_step_equals_grad_then_adam) and
    fresh optimizer states on it"""

    def __init__(self, d, M, A, prec=SF16, D=None, H=256):
        from rlks import _lib

        self.d, self.M, self.A, self.prec, self.H = d, M, A, prec, H
        self.D = D = 3 * A if D is None else D
        self.desc = _lib.MlpDesc(D, H, A, prec)
        self.stride = _lib.lib().rlks_minibatch_stride(C.byref(self.desc))
        self.co = _lib.PpoCoeffs(0.3, 10.0, 1.0, 0.0)
        self.dyn = torch.tensor([0.1, 1.3, 0.2, 1.0 / M, 0, 0, 0, 0], dtype=torch.float32, device=d)
        wsb = C.c_int64()
        _lib.call("rlks_ppo_workspace_bytes", C.byref(self.desc), M, C.byref(wsb))
        self.ws_bytes = wsb.value
        g = torch.Generator(device=d).manual_seed(A)
        self.mbs = []
        for _ in range(STEPS):
            mb = torch.zeros(M, self.stride, device=d)
            mb[:, :D] = torch.rand(M, D, generator=g, device=d)
            mb[:, D:D + A] = torch.randn(M, A, generator=g, device=d)
            mb[:, D + A] = torch.randn(M, generator=g, device=d)
            mb[:, D + A + 1] = torch.randn(M, generator=g, device=d) * 30
            mb[:, D + A + 2] = -torch.rand(M, generator=g, device=d) * 2
            mb[:, D + A + 3] = torch.randint(0, A, (M,), generator=g, device=d).float()
            self.mbs.append(mb)
        s = self.state()
        self.P = s["p"].padded
        self.n_real = s["p"].real
        self.mask = clip_ref.real_mask(s["p"].offsets, s["p"].shapes, self.P)
        self.scratch = torch.zeros(self.ws_bytes, dtype=torch.uint8, device=d)
        self.norm_out = torch.zeros(1, dtype=torch.float64, device=d)

    def state(self):
        from rlks.policy import PolicyParams

        d = self.d
        p = PolicyParams(self.D, self.H, self.A, device=d, seed=3)
        p.desc.precision = self.prec
        return dict(p=p, m=torch.zeros(p.padded, device=d), v=torch.zeros(p.padded, device=d),
                    g=torch.zeros(p.padded, device=d), ws=torch.zeros(self.ws_bytes, dtype=torch.uint8, device=d),
                    stats=torch.zeros(STEPS, 8, dtype=torch.float64, device=d))

    # ---- library calls on a state s, SGD step k (0-based; Adam step k + 1)
    def head(self, s, k):
        return (C.byref(self.desc), C.byref(self.co), s["p"].flat.data_ptr(), self.dyn.data_ptr(),
                self.mbs[k].data_ptr(), self.M, s["g"].data_ptr(), s["stats"][k].data_ptr())

    def grad(self, s, k):
        from rlks import _lib

        _lib.call("rlks_ppo_grad", *self.head(s, k), s["ws"].data_ptr(), s["ws"].numel(), None)

    def adam(self, s, k):
        from rlks import _lib

        _lib.call("rlks_adam_step", s["p"].flat.data_ptr(), s["g"].data_ptr(), s["m"].data_ptr(), s["v"].data_ptr(),
                  self.P, LR, B1, B2, EPS, k + 1, None)

    def norm(self, g):
        from rlks import _lib

        _lib.call("rlks_grad_global_norm", C.byref(self.desc), g.data_ptr(), self.P, self.norm_out.data_ptr(),
                  self.scratch.data_ptr(), self.scratch.numel(), None)
        return float(self.norm_out.item())

    def sgd_step(self, s, k):
        from rlks import _lib

        _lib.call("rlks_ppo_sgd_step", *self.head(s, k), s["m"].data_ptr(), s["v"].data_ptr(), self.P, LR, B1, B2, EPS,
                  k + 1, 1, s["ws"].data_ptr(), s["ws"].numel(), None)

    def sgd_step_clip(self, s, k, clip):
        from rlks import _lib

        # prev_fused = 1 from the first step on: step 1 has no predecessor (the tag fallback), later
        # steps read the maxima the clipped pass left
        _lib.call("rlks_ppo_sgd_step_clip", *self.head(s, k), s["m"].data_ptr(), s["v"].data_ptr(), self.P, LR, B1, B2,
                  EPS, k + 1, 1, clip, None, s["ws"].data_ptr(), s["ws"].numel(), None)

    def apply_clip(self, s, k, clip):
        from rlks import _lib

        _lib.call("rlks_ppo_adam_apply_clip", C.byref(self.desc), s["p"].flat.data_ptr(), s["g"].data_ptr(),
                  s["m"].data_ptr(), s["v"].data_ptr(), self.P, LR, B1, B2, EPS, k + 1, clip, s["stats"][k].data_ptr(),
                  s["ws"].data_ptr(), s["ws"].numel(), self.M, None)

    def pair_clip(self, s, k, clip):
        from rlks import _lib

        _lib.call("rlks_ppo_grad_step", *self.head(s, k), k + 1, 1, s["ws"].data_ptr(), s["ws"].numel(), None)
        self.apply_clip(s, k, clip)

    def parts_clip(self, s, k, clip):
        from rlks import _lib

        for part in (1, 2):
            _lib.call("rlks_ppo_grad_step_part", *self.head(s, k), k + 1, 1, part, None, s["ws"].data_ptr(),
                      s["ws"].numel(), None)
        self.apply_clip(s, k, clip)

    # ---- references (computed once per case and F1 form, shared, never modified)
    def norm1(self):
        """step 1's measured norm"""
        if not hasattr(self, "_norm1"):
            s = self.state()
            self.grad(s, 0)
            self._norm1 = self.norm(s["g"])
        return self._norm1

    def reference(self, clip):
        """per step: (params, m, v, clipped gradient) bits, and the norms / coefficients"""
        s = self.state()
        snaps, norms, coefs = [], [], []
        for k in range(STEPS):
            self.grad(s, k)
            n = self.norm(s["g"])
            gc, _, coef = clip_ref.clipped(s["g"].cpu().numpy(), clip, self.mask, norm=n)
            s["g"].copy_(torch.from_numpy(gc))
            self.adam(s, k)
            snaps.append({key: _bits(s[key] if key != "p" else s["p"].flat).clone() for key in ("p", "m", "v", "g")})
            norms.append(n)
            coefs.append(float(coef))
        return snaps, norms, coefs


_cases = {}


def case(M, A, prec=SF16, D=None, H=256, split=False):
    """(split: built and referenced under RLKS_F1_SPLIT=1, which the caller has set)"""
    key = (M, A, prec, D, H, split)
    if key not in _cases:
        _cases[key] = Case(_dev(), M, A, prec, D, H)
    return _cases[key]


def active_reference(c):
    if not hasattr(c, "_active"):
        clip = float(np.float32(0.5 * c.norm1()))
        c._active = (clip,) + c.reference(clip)
    return c._active


def check_against(c, s, k, snaps, norms, coefs, what):
    assert coefs[k] < 1.0, (what, k, coefs[k])
    n = float(s["stats"][k, 5].item())
    diff = {key: int((_bits(s[key] if key != "p" else s["p"].flat) != snaps[k][key]).sum()) for key in ("p", "m", "v", "g")}
    assert n == norms[k] and not any(diff.values()), (what, k, diff, n, norms[k])


SHAPES = [(256, 2), (256, 8), (2048, 2), (2048, 8)]


# ----------------------------------------------------------------------------- a. the norm
@pytest.mark.parametrize("M,A", SHAPES)
def test_norm(M, A):
    """rlks_grad_global_norm and the clipped step's stats[5] agree bit for bit (the gradient reduce's
    per-block partials and the one-partial pass sum in the same order), both within n * 2^-52 of
    numpy's float64 norm over the true elements; the layout's padding is never read"""
    c = case(M, A)
    s = c.state()
    c.grad(s, 0)
    n_dev = c.norm(s["g"])
    g = s["g"].cpu().numpy()
    n_np = clip_ref.global_norm(g, c.mask)
    s2 = c.state()
    c.sgd_step_clip(s2, 0, float(np.float32(2 * n_np)))  # (inactive: the gradient stays as summed)
    n_step = float(s2["stats"][0, 5].item())
    print(f"M={M} A={A}: norm {n_dev!r} step {n_step!r} numpy {n_np!r} rel {abs(n_dev - n_np) / n_np:.2e} "
          f"bound {c.n_real * 2.0 ** -52:.2e}")
    assert torch.equal(_bits(s["g"]), _bits(s2["g"]))
    assert n_dev == n_step
    assert abs(n_dev - n_np) <= c.n_real * 2.0 ** -52 * n_np
    assert abs(n_step - n_np) <= c.n_real * 2.0 ** -52 * n_np
    junk = s["g"].clone()
    junk[torch.from_numpy(~c.mask).to(junk.device)] = 1e30
    assert c.norm(junk) == n_dev
    assert torch.equal(_bits(junk[torch.from_numpy(c.mask).to(junk.device)]),
                       _bits(s["g"][torch.from_numpy(c.mask).to(junk.device)]))  # the norm pass writes nothing


# ----------------------------------------------------------------------------- b. inactive clip
@pytest.mark.parametrize("M,A", SHAPES)
def test_inactive_clip_is_the_unclipped_step(M, A):
    """An inactive clip (coef = 1.0f) leaves parameters, moments, gradient and stats[0..4] of
    rlks_ppo_sgd_step bit for bit over 5 consecutive steps, and stats[5] is the norm.

    The threshold is twice the LARGEST norm of the unclipped run's 5 steps, not twice step 1's: on
    these minibatches the norm does not stay below 2 x norm_1 (measured at 8 actions and 256 rows,
    even at a learning rate of 1e-5, where the parameters hardly move: 0.246, 0.472, 0.484, 0.537; at
    the tests' 3e-3 and 2 actions 0.84, 0.77, 2.29), so with 2 x norm_1 the clip acts from the second
    to fourth step on and no implementation could equal the unclipped step.  While the clip is inactive
    the two runs are the same trajectory, so the unclipped run's norms are the clipped run's; every
    step asserts that its norm stayed below the threshold."""
    c = case(M, A)
    a, b = c.state(), c.state()
    unclipped = []
    for k in range(STEPS):
        c.sgd_step(a, k)
        unclipped.append(c.norm(a["g"]))
    clip = float(np.float32(2.0 * max(unclipped)))
    assert clip >= 2.0 * c.norm1() * (1 - 1e-6)
    a = c.state()
    for k in range(STEPS):
        c.sgd_step(a, k)
        c.sgd_step_clip(b, k, clip)
        n = float(b["stats"][k, 5].item())
        print(f"M={M} A={A} step {k + 1}: norm {n!r} clip {clip!r}")
        assert n < clip and n == unclipped[k], (k, n, clip)  # (the premise: the clip stays inactive)
        assert c.norm(b["g"]) == n  # unclipped: the gradient buffer still holds the summed gradient
        for key in ("m", "v", "g"):
            assert torch.equal(_bits(a[key]), _bits(b[key])), (k, key)
        assert torch.equal(_bits(a["p"].flat), _bits(b["p"].flat)), k
        assert torch.equal(a["stats"][k, :5], b["stats"][k, :5]), k
        assert float(a["stats"][k, 5].item()) == 0.0 and float(b["stats"][k, 5].item()) == n, k


# ----------------------------------------------------------------------------- c. active clip
@pytest.mark.parametrize("M,A", SHAPES)
def test_active_clip_step_matches_reference(M, A):
    """grad_clip = 0.5 x step 1's norm over 5 steps: rlks_ppo_sgd_step_clip, and rlks_ppo_grad_step ->
    rlks_ppo_adam_apply_clip, equal the step-level reference in parameters, m, v and the clipped
    gradient, bit for bit, with coef < 1 at every step"""
    c = case(M, A)
    clip, snaps, norms, coefs = active_reference(c)
    s, r = c.state(), c.state()
    for k in range(STEPS):
        c.sgd_step_clip(s, k, clip)
        check_against(c, s, k, snaps, norms, coefs, "sgd_step_clip")
        c.pair_clip(r, k, clip)
        check_against(c, r, k, snaps, norms, coefs, "grad_step + adam_apply_clip")


@pytest.mark.parametrize("M,A", SHAPES)
def test_active_clip_two_part_gradient_matches_reference(M, A, monkeypatch):
    """the overlapped form's two rlks_ppo_grad_step_part calls -> rlks_ppo_adam_apply_clip, under
    RLKS_F1_SPLIT=1 (the two-part form always runs the two F1 kernels: so does its reference)"""
    monkeypatch.setenv("RLKS_F1_SPLIT", "1")
    c = case(M, A, split=True)
    clip, snaps, norms, coefs = active_reference(c)
    s = c.state()
    for k in range(STEPS):
        c.parts_clip(s, k, clip)
        check_against(c, s, k, snaps, norms, coefs, "grad_step_part x 2 + adam_apply_clip")


# ----------------------------------------------------------------------------- d. fp32 and wide
@pytest.mark.parametrize("prec,D,H,A", [(FP32, 6, 256, 2), (WIDE, 12, 512, 4)])
def test_active_clip_fp32_and_wide(prec, D, H, A):
    """the unfused paths (rlks_ppo_grad, the norm pass, the clipped Adam kernel) at 256 rows, against
    their own rlks_ppo_grad + host clip + rlks_adam_step"""
    c = case(256, A, prec, D, H)
    clip, snaps, norms, coefs = active_reference(c)
    s, r = c.state(), c.state()
    for k in range(STEPS):
        c.sgd_step_clip(s, k, clip)
        check_against(c, s, k, snaps, norms, coefs, "sgd_step_clip")
        c.grad(r, k)
        c.apply_clip(r, k, clip)
        check_against(c, r, k, snaps, norms, coefs, "grad + adam_apply_clip")


# ----------------------------------------------------------------------------- e. determinism
@pytest.mark.parametrize("M,A", [(2048, 2), (2048, 8)])
def test_clipped_step_is_deterministic(M, A):
    c = case(M, A)
    clip = active_reference(c)[0]
    runs = []
    for _ in range(3):
        s = c.state()
        for k in range(STEPS):
            c.sgd_step_clip(s, k, clip)
        runs.append(s)
    for s in runs[1:]:
        for key in ("m", "v", "g", "stats"):
            assert torch.equal(runs[0][key].view(torch.int32), s[key].view(torch.int32)), key
        assert torch.equal(_bits(runs[0]["p"].flat), _bits(s["p"].flat))


def test_clip_argument_is_checked():
    from rlks import _lib

    c = case(256, 2)
    s = c.state()
    for bad in (0.0, -1.0, float("inf"), float("nan")):
        with pytest.raises(_lib.RlksError):
            c.sgd_step_clip(s, 0, bad)
        with pytest.raises(_lib.RlksError):
            c.apply_clip(s, 0, bad)


# ----------------------------------------------------------------------------- agent level
def _cfg(N, T, mb, epochs=2, seed=11, **kw):
    from rlks.ppo import PPOConfig

    kw = {**dict(train_batch_size=N * T, sgd_minibatch_size=mb, num_sgd_iter=epochs, lr=3e-4, gamma=0.99), **kw}
    cfg = PPOConfig().environment("K8sMultiCloudEnv").framework("torch").training(**kw).debugging(seed=seed)
    cfg.num_envs = N
    cfg.rollout_fragment_length = T
    return cfg


def _stats(r):
    return r["info"]["learner"]["default_policy"]["learner_stats"]


# ----------------------------------------------------------------------------- f. whole iteration
def test_clipped_iteration_matches_fp64_reference():
    """One train() at N = 256, T = 16, minibatch 1,024, 2 epochs, seed 3 (8 Adam steps).  grad_clip =
    1e30 leaves the grad_clip = None run's parameters bit for bit and reports the 8 norms; grad_clip =
    their median against clip_ref.ppo_iteration_clipped in float64 over the same rollout, with the
    bounds of test_ppo_iteration_matches_fp64_oracle: ||dp|| <= 1e-5 ||p||, ||dp|| <= 1e-3 ||update||,
    |dp| <= 1e-5 |p| + 1e-9 for all but 1e-4 of the elements, m to 1e-4, the KL coefficient to 1e-6;
    some steps clipped and some not; grad_gnorm = the mean of the reference's norms to 1e-5."""
    from rlks import _lib
    from rlks.ppo import PPO

    d = _dev()
    N, T, mb, epochs, seed = 256, 16, 1024, 2, 3
    plain = PPO(config=_cfg(N, T, mb, epochs=epochs, seed=seed), device=d)
    r0 = plain.train()
    assert "grad_gnorm" not in _stats(r0)
    huge = PPO(config=_cfg(N, T, mb, epochs=epochs, seed=seed, grad_clip=1e30), device=d)
    r1 = huge.train()
    assert torch.equal(_bits(plain.params.flat), _bits(huge.params.flat))
    assert torch.equal(_bits(plain.adam_m), _bits(huge.adam_m)) and torch.equal(_bits(plain.adam_v), _bits(huge.adam_v))
    norms1 = huge.stats[:, _lib.RLKS_STAT_GRAD_GNORM].cpu().numpy()
    assert norms1.shape == (8,) and (norms1 > 0).all()
    assert _stats(r1)["grad_gnorm"] == pytest.approx(norms1.mean(), rel=1e-12)
    clip = float(np.float32(np.median(norms1)))

    algo = PPO(config=_cfg(N, T, mb, epochs=epochs, seed=seed, grad_clip=clip), device=d)
    p0 = algo.params.flat.cpu().numpy().astype(np.float64)
    r = algo.train()
    b = {k: v.cpu().numpy() for k, v in algo.buf.items()}
    real = clip_ref.real_mask(algo.params.offsets, algo.params.shapes, algo.params.padded)
    p_ref, m_ref, v_ref, klc, st, norms_ref = clip_ref.ppo_iteration_clipped(
        p0, algo.params.offsets, 6, 256, 2, b, grad_clip=clip, mask=real, perm_seed=algo.perm_seed(0), epochs=epochs,
        mb=mb, lr=3e-4)
    assert len(st) == 8 == algo.adam_step
    norms = algo.stats[:, _lib.RLKS_STAT_GRAD_GNORM].cpu().numpy()
    print("clip", clip, "norms", norms, "reference", np.array(norms_ref))
    assert (norms > clip).any() and (norms <= clip).any()
    p = algo.params.flat.cpu().numpy().astype(np.float64)
    p, p_ref, p0 = p[real], p_ref[real], p0[real]
    err = np.abs(p - p_ref)
    print(f"||dp||/||p|| {np.linalg.norm(p - p_ref) / np.linalg.norm(p_ref):.2e}, "
          f"||dp||/||update|| {np.linalg.norm(p - p_ref) / np.linalg.norm(p_ref - p0):.2e}, max {err.max():.2e}, "
          f"outliers {(err > 1e-5 * np.abs(p_ref) + 1e-9).mean():.2e}")
    assert np.linalg.norm(p - p_ref) <= 1e-5 * np.linalg.norm(p_ref)
    assert np.linalg.norm(p - p_ref) <= 1e-3 * np.linalg.norm(p_ref - p0)
    assert (err > 1e-5 * np.abs(p_ref) + 1e-9).mean() <= 1e-4
    m = algo.adam_m.cpu().numpy().astype(np.float64)[real]
    assert np.linalg.norm(m - m_ref[real]) <= 1e-4 * np.linalg.norm(m_ref[real])
    assert abs(float(algo.dyn[2].item()) - klc) <= 1e-6 * klc
    assert abs(_stats(r)["grad_gnorm"] - np.mean(norms_ref)) <= 1e-5 * np.mean(norms_ref)


# ----------------------------------------------------------------------------- g. resume
def test_resume_with_grad_clip_is_exact(tmp_path):
    """save -> from_checkpoint -> train() with grad_clip set equals the uninterrupted run bit for
    bit (the config dict carries grad_clip; no new state)"""
    from rlks import _lib
    from rlks.ppo import PPO

    d = _dev()
    N, T, mb = 256, 16, 1024
    probe = PPO(config=_cfg(N, T, mb, seed=21, grad_clip=1e30), device=d)
    probe.train()
    clip = float(np.float32(np.median(probe.stats[:, _lib.RLKS_STAT_GRAD_GNORM].cpu().numpy())))
    a = PPO(config=_cfg(N, T, mb, seed=21, grad_clip=clip), device=d)
    a.train()
    path = a.save(tmp_path)
    ra = a.train()
    b = PPO.from_checkpoint(path, device=d)
    assert b.grad_clip == clip
    rb = b.train()
    na = a.stats[:, _lib.RLKS_STAT_GRAD_GNORM].cpu().numpy()
    assert (na > clip).any()  # the clip acted in the compared iteration
    assert torch.equal(_bits(a.params.flat), _bits(b.params.flat))
    assert torch.equal(_bits(a.adam_m), _bits(b.adam_m)) and torch.equal(_bits(a.adam_v), _bits(b.adam_v))
    assert torch.equal(a.stats, b.stats)
    assert _stats(ra) == _stats(rb)


# ----------------------------------------------------------------------------- h. schedules
@pytest.mark.parametrize("knob,v0,v1", [("lr", 3e-4, 1e-4), ("entropy_coeff", 0.01, 0.0)])
def test_schedules_equal_setting_the_value_by_hand(knob, v0, v1):
    """two train() calls with a schedule from v0 at timestep 0 to v1 at N T (the second iteration's
    start) leave the parameters of a run that sets config.<knob> by hand before each call, bit for
    bit; cur_lr reports the value used"""
    from rlks.ppo import PPO

    d = _dev()
    N, T, mb = 256, 16, 1024
    sched = PPO(config=_cfg(N, T, mb, seed=5, **{knob + "_schedule": [[0, v0], [N * T, v1]]}), device=d)
    hand = PPO(config=_cfg(N, T, mb, seed=5), device=d)
    for v in (v0, v1):
        setattr(hand.config, knob, v)
        rs, rh = sched.train(), hand.train()
        if knob == "lr":
            assert _stats(rs)["cur_lr"] == v == _stats(rh)["cur_lr"]
        else:
            assert sched.coeffs.entropy_coeff == np.float32(v) == hand.coeffs.entropy_coeff
        assert torch.equal(_bits(sched.params.flat), _bits(hand.params.flat)), v
    assert sched.timesteps_total == 2 * N * T
    # the second iteration did use another value than the first
    const = PPO(config=_cfg(N, T, mb, seed=5, **{knob: v0}), device=d)
    const.train()
    const.train()
    assert not torch.equal(_bits(sched.params.flat), _bits(const.params.flat))
