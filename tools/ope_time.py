#!/usr/bin/env python3
"""Time the off-policy estimate's launches (rlks_ope_logp, rlks_ope_estimate) on synthetic logs at
c4's (T = 128, N = 131,072, A = 2) and c3's (N = 65,536, A = 8) sizes, episodes of 99 steps in lockstep as the
table env ends them: each entry is captured REPS times into a HIP graph and replayed between device events,
the median of 5 replays.  Per size: the time per call and the bytes the launches must move over that time, as
a fraction of the 6.29 TB/s a float4 copy reaches on an MI355X (MI355X_MICROARCH.md).

Bytes counted (per logged step unless said otherwise):
  logp      4 A + 4 read (the logits row, the action), 4 written
  estimate  13 read by each of the two walks (two logp, the reward, the done byte);
            columns: 12 written (the f64 sum and the u32 count), and 12 read back first where the lane had
            reached that step index before (every step of a lane's second and later episodes);
            rows: 12 read per (step index, lane) entry reached, 4 N per row for the lanes' reach;
            values: 16 read (S_k, w_k; cached: T rows), 32 written per episode with per-episode output (off here)
Then the whole rlks.offline.estimate() call, the target's forward included, as wall time (median of 3).
usage: ope_time.py [--no-wall]   -> one JSON line"""
import argparse
import ctypes as C_
import json
import sys
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT / "rl-k8s-scheduler_amd"))

REPS = 4
HBM_COPY_TBS = 6.29
EPISODE = 99
SIZES = {"c4": (128, 131072, 2), "c3": (128, 65536, 8)}


def graph_us(torch, call):
    """median over 5 replays of a graph of REPS calls, in us per call"""
    call(None)
    torch.cuda.synchronize()
    gr = torch.cuda.CUDAGraph()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        with torch.cuda.graph(gr, stream=side):
            for _ in range(REPS):
                call(torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    gr.replay()
    torch.cuda.synchronize()
    times = []
    for _ in range(5):
        s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        s.record()
        gr.replay()
        e.record()
        torch.cuda.synchronize()
        times.append(s.elapsed_time(e) / REPS * 1e3)
    return sorted(times)[2], min(times), max(times)


def rate(nbytes, us):
    tbs = nbytes / us / 1e6
    return {"bytes": int(nbytes), "TBs": round(tbs, 3), "frac_of_hbm_copy_rate": round(tbs / HBM_COPY_TBS, 3)}


def one_size(torch, _lib, dev, T, N, A, wall):
    g = torch.Generator(device=dev).manual_seed(1)
    f32 = dict(dtype=torch.float32, device=dev)
    rows = T * N
    logits = torch.randn(rows, A, generator=g, **f32)
    actions = torch.randint(0, A, (rows,), generator=g, dtype=torch.int32, device=dev)
    lp_new = torch.empty(rows, **f32)
    lp_old = -torch.rand(T, N, generator=g, **f32) - 0.3
    rewards = torch.randn(T, N, generator=g, **f32)
    dones = torch.zeros(T, N, dtype=torch.uint8, device=dev)
    dones[EPISODE - 1::EPISODE] = 1
    wsb = C_.c_int64()
    _lib.call("rlks_ope_workspace_bytes", T, N, C_.byref(wsb))
    ws = torch.empty(wsb.value // 8 + 1, dtype=torch.float64, device=dev)
    rec = torch.zeros(_lib.RLKS_OPE_SIZE, dtype=torch.float64, device=dev)

    def logp(cs):
        _lib.call("rlks_ope_logp", logits.data_ptr(), actions.data_ptr(), None, rows, A, lp_new.data_ptr(), cs)

    def est(cs):
        _lib.call("rlks_ope_estimate", lp_new.data_ptr(), lp_old.data_ptr(), rewards.data_ptr(), dones.data_ptr(), T, N,
                  0.99, 0, rec.data_ptr(), None, ws.data_ptr(), wsb.value, cs)

    us_l, lo_l, hi_l = graph_us(torch, logp)
    us_e, lo_e, hi_e = graph_us(torch, est)
    reached = N * min(T, EPISODE)          # (step index, lane) entries a lane reaches
    again = rows - reached                 # steps that add to an entry reached before
    b_logp = rows * (4 * A + 4 + 4)
    b_est = rows * (13 + 12 + 13 + 16) + again * 12 + reached * 12 + T * N * 4
    out = {"T": T, "N": N, "A": A, "workspace_bytes": wsb.value,
           "logp": {"us_per_call": round(us_l, 1), "us_min_max": [round(lo_l, 1), round(hi_l, 1)], **rate(b_logp, us_l)},
           "estimate": {"us_per_call": round(us_e, 1), "us_min_max": [round(lo_e, 1), round(hi_e, 1)],
                        **rate(b_est, us_e), "input_bytes": rows * 13},
           "episodes": float(rec[_lib.RLKS_OPE_EPISODES].item()), "v_is_sum": float(rec[_lib.RLKS_OPE_VIS_SUM].item())}
    if wall:
        from rlks.offline import DecisionLog, estimate
        from rlks.policy import PolicyParams

        del logits, ws
        params = PolicyParams(3 * A, 256, A, device=dev, seed=2)
        log = DecisionLog(torch.rand(T, N, 3 * A, generator=g, **f32), actions.view(T, N), lp_old, rewards, dones)
        estimate(params, log)
        ms = []
        for _ in range(3):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            estimate(params, log)
            torch.cuda.synchronize()
            ms.append((time.perf_counter() - t0) * 1e3)
        out["estimate_call_wall_ms"] = {"median": round(sorted(ms)[1], 2), "min_max": [round(min(ms), 2), round(max(ms), 2)]}
    return out


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--no-wall", action="store_true", help="skip the whole-call wall time")
    args = ap.parse_args()
    import torch

    from rlks import _lib

    if not torch.cuda.is_available():
        raise SystemExit("ope_time.py needs a HIP device")
    dev = torch.device("cuda", 0)
    print(json.dumps({"launches_per_graph": REPS, "hbm_copy_TBs": HBM_COPY_TBS,
                      "sizes": {k: one_size(torch, _lib, dev, *v, wall=not args.no_wall) for k, v in SIZES.items()}}))
