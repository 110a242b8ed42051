#!/usr/bin/env python
"""k_policy_act's own duration per launch shape, from a kernel trace.

    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -o act -- python tools/act_kernel_time.py --run
    python tools/act_kernel_time.py --summarise DIR --out profiles/r16_serving/kernel_time.json

--run        the workload: PolicyServer.act on seeded observations, CALLS calls per cell, the cells in the
             fixed order (D, A) in {(6, 2), (24, 8)} x full_fetch in {False, True} x n in {1, 16, 256, 1024}
             (greedy, no filter, no mask; full_fetch adds the value net's blocks)
--summarise  reads the trace's *kernel_trace.csv, takes the k_policy_act dispatches in order, CALLS per cell,
             and writes each cell's median and maximum duration in microseconds (the first 20 of a cell are
             left out as warm-up)
"""
import argparse
import csv
import json
import sys
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parents[1]
NS = (1, 16, 256, 1024)
SHAPES = ((6, 2), (24, 8))
CALLS, SKIP = 300, 20


def cells():
    return [(D, A, ff, n) for D, A in SHAPES for ff in (False, True) for n in NS]


def run():
    sys.path.insert(0, str(ROOT / "rl-k8s-scheduler_amd"))
    import torch

    from rlks.policy import PolicyParams
    from rlks.serving import PolicyServer

    dev = torch.device("cuda", 0)
    for D, A in SHAPES:
        srv = PolicyServer(PolicyParams(D, 256, A, device=dev, seed=11), max_rows=max(NS))
        assert srv.fused
        obs = np.random.default_rng(5).random((max(NS), D)).astype(np.float32)
        for ff in (False, True):
            for n in NS:
                for _ in range(CALLS):
                    srv.act(obs[:n], explore=False, full_fetch=ff)
        srv.close()


def summarise(d, out):
    files = sorted(Path(d).rglob("*kernel_trace.csv"))
    assert files, f"no kernel trace under {d}"
    dur = []
    for f in files:
        with open(f, newline="") as fh:
            for r in csv.DictReader(fh):
                if "k_policy_act" in r["Kernel_Name"]:
                    dur.append((int(r["Start_Timestamp"]), int(r["End_Timestamp"]) - int(r["Start_Timestamp"]),
                                int(r["Grid_Size_X"]), int(r["Grid_Size_Y"])))
    dur.sort()
    cs = cells()
    assert len(dur) == CALLS * len(cs), (len(dur), CALLS * len(cs))
    rows = []
    for i, (D, A, ff, n) in enumerate(cs):
        part = dur[i * CALLS:(i + 1) * CALLS]
        grids = sorted({(p[2], p[3]) for p in part})
        assert len(grids) == 1 and grids[0][1] == (2 if ff else 1), (D, A, ff, n, grids)  # the cell's own launches
        t = np.array([p[1] for p in part[SKIP:]], np.float64) / 1e3
        rows.append({"D": D, "A": A, "full_fetch": ff, "n": n, "blocks": [-(-n // 16), 2 if ff else 1],
                     "traced_grid": list(grids[0]),
                     "median_us": round(float(np.median(t)), 2), "max_us": round(float(t.max()), 2)})
        print(json.dumps(rows[-1]))
    Path(out).parent.mkdir(parents=True, exist_ok=True)
    Path(out).write_text(json.dumps({"kernel": "k_policy_act", "calls": CALLS, "skipped": SKIP, "rows": rows}, indent=1))


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--run", action="store_true")
    ap.add_argument("--summarise", metavar="DIR")
    ap.add_argument("--out", default="profiles/r16_serving/kernel_time.json")
    a = ap.parse_args()
    if a.run:
        run()
    elif a.summarise:
        summarise(a.summarise, a.out)
    else:
        ap.error("--run or --summarise DIR")
