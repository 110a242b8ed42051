"""Host reference of global-norm gradient clipping (test infrastructure; include/rlks.h states the
semantics): RLlib's old-API-stack torch policy (apply_grad_clipping) calls
torch.nn.utils.clip_grad_norm_ over every parameter of the one optimizer --

    norm = sqrt(sum g^2)                                 over the true elements of all 12 tensors
    coef = min(1, grad_clip / (norm + 1e-6))
    g   <- g * coef, then Adam on the clipped g

with the library's arithmetic: the sum in float64 (squares of float32 values are exact there),
coef = (float32) min(1.0, (double) grad_clip / (norm + 1e-6)) with grad_clip a float32 argument, and
g * coef one float32 multiplication, round to nearest.
"""
import numpy as np

import oracle


def real_mask(offsets, shapes, padded):
    """True at the true elements of the flat layout, False at its padding"""
    m = np.zeros(int(padded), bool)
    for o, shp in zip(offsets, shapes):
        m[int(o): int(o) + int(np.prod(shp))] = True
    return m


def global_norm(g, mask):
    """float64 norm of the float32 gradient over the true elements"""
    x = np.asarray(g, np.float32)[mask].astype(np.float64)
    return float(np.sqrt(np.sum(x * x)))


def clip_coef(norm, clip):
    return np.float32(min(1.0, float(np.float32(clip)) / (float(norm) + 1e-6)))


def clipped(g, clip, mask, norm=None):
    """(clipped float32 gradient, norm, coef): the true elements times coef, padding untouched.
    norm: the norm to clip by (default: global_norm(g, mask))"""
    g = np.asarray(g, np.float32)
    norm = global_norm(g, mask) if norm is None else float(norm)
    coef = clip_coef(norm, clip)
    out = g.copy()
    out[mask] = g[mask] * coef  # float32 x float32 -> float32, round to nearest
    return out, norm, coef


def ppo_iteration_clipped(flat, off, D, H, A, buf, *, grad_clip, mask, perm_seed, epochs, mb, lr, gamma=0.99, lam=1.0,
                          kl_coeff=0.2, kl_target=0.01, clip_param=0.3, vf_clip_param=10.0, vf_loss_coeff=1.0,
                          entropy_coeff=0.0, groups=1):
    """oracle.ppo_iteration's loop (from zero Adam state) in float64 with the clip between gradient
    and Adam.  Returns (params, adam_m, adam_v, new kl_coeff, per-step stats, per-step norms)."""
    T, N = buf["rewards"].shape
    S = T * N
    adv, vt = oracle.gae(buf["rewards"], buf["values"], buf["dones"], gamma, lam)
    a = adv.reshape(-1)
    mean, inv_std = a.mean(), 1.0 / max(1e-4, a.std())
    rec = np.concatenate([buf["obs"][:T].reshape(S, D), buf["logits"].reshape(S, A), a[:, None],
                          vt.reshape(S, 1), buf["logp"].reshape(S, 1), buf["actions"].reshape(S, 1)], axis=1)
    p = np.asarray(flat, np.float64).copy()
    m, v = np.zeros_like(p), np.zeros_like(p)
    clip = float(np.float32(grad_clip))
    step, stats, norms = 0, [], []
    for ep in range(epochs):
        order = oracle.minibatch_indices(perm_seed, ep, T, N, mb, groups)
        for b in range(order.shape[0]):
            g, st = oracle.ppo_loss_grad(p, off, D, H, A, rec[order[b]], clip_param=clip_param,
                                         vf_clip_param=vf_clip_param, vf_loss_coeff=vf_loss_coeff,
                                         entropy_coeff=entropy_coeff, kl_coeff=kl_coeff, adv_mean=mean,
                                         adv_inv_std=inv_std)
            norm = float(np.sqrt(np.sum(g[mask] ** 2)))
            g = g * min(1.0, clip / (norm + 1e-6))
            step += 1
            p, m, v = oracle.adam64(p, g, m, v, step, lr)
            stats.append(st)
            norms.append(norm)
    kl = np.mean([s["kl"] / s["rows"] for s in stats])
    if kl > 2.0 * kl_target:
        kl_coeff *= 1.5
    elif kl < 0.5 * kl_target:
        kl_coeff *= 0.5
    return p, m, v, kl_coeff, stats, norms
