#!/usr/bin/env python3
"""Digests of the device code in a directory of per-unit assembly listings (`make -C csrc asm`), one
record per kernel; needs no GPU.

  python tools/kernel_digest.py <dir of .s files> <out.json>
  python tools/kernel_digest.py --compare a.json b.json

A record holds the SHA-256 of the kernel's instruction lines and, from the unit's kernel metadata, the
VGPR, AGPR and SGPR counts, the LDS bytes and the scratch bytes.  The instruction lines are the body
between the kernel's label and the end of its function (the instructions, then the directives of the
kernel descriptor the listing puts before the function's end), with comments, blank lines and alignment
directives dropped and the local block labels .LBB<f>_<n> renumbered in order of first appearance (<f>
is the function's position in its unit, which moves when a kernel changes place or unit).  Whatever is
there is hashed; nothing is searched for.  --compare matches kernels by name, whatever unit they are in,
and lists those added, removed or changed (exit status 1 if there are any)."""
import hashlib
import json
import re
import sys
from pathlib import Path

LABEL = re.compile(r"\.LBB\d+_\d+")
META = {".vgpr_count": "vgpr", ".agpr_count": "agpr", ".sgpr_count": "sgpr", ".group_segment_fixed_size": "lds",
        ".private_segment_fixed_size": "scratch"}


def metadata(lines):
    """kernel name -> {vgpr, agpr, sgpr, lds, scratch} from the amdhsa.kernels list (one '  - ' item per kernel)"""
    out, cur = {}, None
    start = lines.index("amdhsa.kernels:") + 1 if "amdhsa.kernels:" in lines else len(lines)
    for ln in lines[start:]:
        if not ln.startswith("  "):
            break
        if ln.startswith("  - "):
            cur = {}
        m = re.match(r"  [- ] (\.\w+):\s*(\S+)$", ln)
        if m and m.group(1) == ".name":
            out[m.group(2)] = cur
        elif m and m.group(1) in META:
            cur[META[m.group(1)]] = int(m.group(2))
    return out


def body_digest(lines, name):
    i = next(k for k, ln in enumerate(lines) if ln.startswith(name + ":")) + 1
    seen, text = {}, []
    for ln in lines[i:]:
        if ln.startswith(".Lfunc_end"):
            break
        ln = ln.split(";", 1)[0].strip()
        if not ln or ln.startswith(".p2align"):
            continue
        text.append(LABEL.sub(lambda m: seen.setdefault(m.group(0), f".L{len(seen)}"), ln))
    return hashlib.sha256("\n".join(text).encode()).hexdigest(), len(text)


def digest(src, out):
    recs = []
    for f in sorted(Path(src).glob("*.s")):
        lines = f.read_text().splitlines()
        for name, regs in metadata(lines).items():
            sha, n = body_digest(lines, name)
            recs.append({"unit": f.stem, "kernel": name, "sha256": sha, "lines": n, **regs})
    Path(out).write_text("[\n" + ",\n".join(json.dumps(r) for r in recs) + "\n]\n")  # one kernel a line
    print(f"{len(recs)} kernels in {len(list(Path(src).glob('*.s')))} units -> {out}")


def compare(pa, pb):
    a, b = ({r["kernel"]: r for r in json.loads(Path(p).read_text())} for p in (pa, pb))
    keys = ("sha256", "vgpr", "agpr", "sgpr", "lds", "scratch")
    diff = [f"removed {k} ({a[k]['unit']})" for k in a if k not in b]
    diff += [f"added   {k} ({b[k]['unit']})" for k in b if k not in a]
    for k in a:
        if k in b and any(a[k][f] != b[k][f] for f in keys):
            what = ", ".join(f"{f} {a[k][f]} -> {b[k][f]}" if f != "sha256" else "instructions"
                             for f in keys if a[k][f] != b[k][f])
            diff.append(f"changed {k} ({a[k]['unit']} -> {b[k]['unit']}): {what}")
    moved = sum(1 for k in a if k in b and a[k]["unit"] != b[k]["unit"])
    print(f"{pa}: {len(a)} kernels, {pb}: {len(b)} kernels, {moved} in another unit; "
          f"{len(diff)} added, removed or changed")
    print("\n".join(diff))
    return 1 if diff else 0


if __name__ == "__main__":
    if len(sys.argv) == 4 and sys.argv[1] == "--compare":
        sys.exit(compare(sys.argv[2], sys.argv[3]))
    if len(sys.argv) != 3:
        sys.exit(__doc__)
    digest(sys.argv[1], sys.argv[2])
