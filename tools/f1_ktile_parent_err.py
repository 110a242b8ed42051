#!/usr/bin/env python3
"""Per-element error of dW1 / db1 (both nets) of the fused F1 kernel on the cases of tests/f1_ktile_cases.py,
for the library RLKS_LIB selects: max and p99 per tensor against the float64 oracle.

  RLKS_LIB=<parent commit's librlks.so> python tools/f1_ktile_parent_err.py profiles/r14_f1_ktile/parent_w1_b1_err.json

tests/test_gpu_f1_ktile.py holds the tree to the figures recorded there (no margin).  The file also keeps a
digest of the four tensors per case: run the tool once per library and compare the files to tell
byte-identical results from merely equal error figures."""
import json
import os
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]
for p in (ROOT / "rl-k8s-scheduler_amd", ROOT / "oracle", ROOT / "tests"):
    sys.path.insert(0, str(p))


def main():
    import torch
    from f1_ktile_cases import W1_B1, Case, all_cases, case_id, w1_b1_digest, w1_b1_errors

    out = Path(sys.argv[1])
    os.environ.pop("RLKS_F1_SPLIT", None)
    res = {"lib": Path(os.environ.get("RLKS_LIB", "librlks.so")).name, "cases": {}, "sha": {}}
    for regime, rows, A in all_cases():
        c = Case(regime, rows, A, torch.device("cuda", 0))
        g, _ = c.run()
        eg, est, _ = c.oracle()
        e = w1_b1_errors(g, eg, est["scale"], c.p.offsets, c.p.shapes)
        res["cases"][case_id(regime, rows, A)] = {str(i): list(e[i]) for i in W1_B1}
        # a digest of the four tensors, to tell byte-identical results from merely equal error figures
        res["sha"][case_id(regime, rows, A)] = w1_b1_digest(g, c.p.offsets, c.p.shapes)
        print(case_id(regime, rows, A), res["cases"][case_id(regime, rows, A)], res["sha"][case_id(regime, rows, A)], flush=True)
    out.parent.mkdir(parents=True, exist_ok=True)
    out.write_text(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
