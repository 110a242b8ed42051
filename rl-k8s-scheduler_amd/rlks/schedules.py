"""Host-side training schedules and the validation of the training knobs RLlib's PPOConfig takes.

`lr_schedule` and `entropy_coeff_schedule` (RLlib old-API-stack LearningRateSchedule /
EntropyCoeffSchedule over a PiecewiseSchedule; third-party, absent from the reference tree): a list
of [timestep, value] points, the first at timestep 0, timesteps strictly increasing, linear
interpolation between points, the last value held after the last point.  The agent evaluates them
at `timesteps_total` when an iteration starts.  No device code: importable without librlks.so.
"""
from __future__ import annotations

import math
import numbers


def _number(x) -> bool:
    return isinstance(x, numbers.Real) and not isinstance(x, bool)


def validate_schedule(schedule, name="schedule"):
    """the schedule as a list of (int timestep, float value); ValueError when malformed"""
    try:
        pts = [tuple(p) for p in schedule]
    except TypeError:
        raise ValueError(f"{name} must be a list of [timestep, value] points, got {schedule!r}") from None
    if not pts:
        raise ValueError(f"{name} must have at least one [timestep, value] point")
    out = []
    for p in pts:
        if len(p) != 2 or not _number(p[0]) or not _number(p[1]):
            raise ValueError(f"{name}: every point must be [timestep, value], got {p!r}")
        t, v = p
        if not math.isfinite(v) or not math.isfinite(t) or t != int(t) or t < 0:
            raise ValueError(f"{name}: timesteps must be non-negative integers and values finite, got {p!r}")
        out.append((int(t), float(v)))
    if out[0][0] != 0:
        raise ValueError(f"{name}: the first point must be at timestep 0, got {out[0][0]}")
    for (t0, _), (t1, _) in zip(out, out[1:]):
        if t1 <= t0:
            raise ValueError(f"{name}: timesteps must strictly increase, got {t0} then {t1}")
    return out


def schedule_value(schedule, timestep) -> float:
    """value of a validated-or-raw schedule at `timestep`: linear between points, the last value after"""
    pts = validate_schedule(schedule)
    t = int(timestep)
    if t < 0:
        raise ValueError(f"timestep must be >= 0, got {timestep}")
    for (t0, v0), (t1, v1) in zip(pts, pts[1:]):
        if t0 <= t < t1:
            return v0 + (v1 - v0) * ((t - t0) / (t1 - t0))
    return pts[-1][1]


def validate_grad_clip(grad_clip, grad_clip_by=None):
    """PPOConfig.grad_clip: None or a finite positive number; grad_clip_by: only RLlib's
    "global_norm" (its default) is implemented, "value" and "norm" are refused, not ignored"""
    if grad_clip_by is not None and grad_clip_by != "global_norm":
        raise ValueError(f"grad_clip_by={grad_clip_by!r} is not supported: only 'global_norm'")
    if grad_clip is None:
        return None
    if not _number(grad_clip) or not math.isfinite(grad_clip) or grad_clip <= 0:
        raise ValueError(f"grad_clip must be None or a finite positive number, got {grad_clip!r}")
    return float(grad_clip)
