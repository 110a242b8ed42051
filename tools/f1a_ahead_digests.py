#!/usr/bin/env python3
"""sha256 of the whole gradient and of the stats of the fused F1 kernel on the cases of
tests/test_gpu_f1a_ahead.py (tests/f1_ktile_cases.py's, plus 768 rows), for the library RLKS_LIB selects.

  RLKS_LIB=<parent commit's librlks.so> python tools/f1a_ahead_digests.py profiles/r16_f1a_ahead/parent_digests.json

tests/test_gpu_f1a_ahead.py holds the tree to the digests recorded there: the change reorders independent
work only, so equality gets no margin."""
import hashlib
import json
import os
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]
for p in (ROOT / "rl-k8s-scheduler_amd", ROOT / "oracle", ROOT / "tests"):
    sys.path.insert(0, str(p))

EXTRA_ROWS = 768  # three workgroups a net: an odd count


def cases():
    from f1_ktile_cases import ACTIONS, all_cases

    return all_cases() + [("plain", EXTRA_ROWS, a) for a in ACTIONS]


def digests(g, st):
    """(gradient, stats) -> their sha256 over the arrays' bytes"""
    import numpy as np

    return {"grad": hashlib.sha256(np.ascontiguousarray(g).tobytes()).hexdigest(),
            "stats": hashlib.sha256(np.ascontiguousarray(st).tobytes()).hexdigest()}


def main():
    import torch
    from f1_ktile_cases import Case, case_id

    out = Path(sys.argv[1])
    os.environ.pop("RLKS_F1_SPLIT", None)
    res = {"lib": Path(os.environ.get("RLKS_LIB", "librlks.so")).name, "cases": {}}
    for regime, rows, A in cases():
        c = Case(regime, rows, A, torch.device("cuda", 0))
        res["cases"][case_id(regime, rows, A)] = digests(*c.run())
        print(case_id(regime, rows, A), res["cases"][case_id(regime, rows, A)], flush=True)
    out.parent.mkdir(parents=True, exist_ok=True)
    out.write_text(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
