"""The split-fp16 scale exponent on a bit pattern (csrc/sf_exp.h: sf_exp_bits, pow2_bits), which the
k-tile-major F1b finishes on the scalar unit, against the float forms it replaces there:
sf_exp over all 256 biased exponents x mantissas {0, 1, 0x400000, 0x7fffff} and the three patterns around
3.4e38f (0x7f7fc99e, the last one with a non-zero exponent), and ldexpf(1, e) over every e from
-400 to 400 (the overflow to infinity, the denormals and the underflow to zero included).  Host only: the header
is compiled on its own."""
import subprocess
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]

PROG = r"""
#include <stdio.h>
#include <string.h>
#include "sf_exp.h"
static float f_of(unsigned u) { float f; memcpy(&f, &u, 4); return f; }
static unsigned u_of(float f) { unsigned u; memcpy(&u, &f, 4); return u; }
int main(void) {
  const unsigned mant[4] = {0u, 1u, 0x400000u, 0x7fffffu};
  int n = 0, bad = 0;
  for (unsigned be = 0; be < 256; ++be)
    for (int j = 0; j < 4; ++j, ++n) {
      const unsigned u = (be << 23) | mant[j];
      if (sf_exp_bits(u) != sf_exp(f_of(u))) {
        printf("sf_exp %08x: bits %d float %d\n", u, sf_exp_bits(u), sf_exp(f_of(u)));
        ++bad;
      }
    }
  const unsigned edge[3] = {0x7f7fc99du, 0x7f7fc99eu, 0x7f7fc99fu};  /* 3.4e38f and its two neighbours */
  for (int j = 0; j < 3; ++j, ++n)
    if (sf_exp_bits(edge[j]) != sf_exp(f_of(edge[j])) || (sf_exp_bits(edge[j]) == 0) != (j == 2)) {
      printf("sf_exp %08x: bits %d float %d\n", edge[j], sf_exp_bits(edge[j]), sf_exp(f_of(edge[j])));
      ++bad;
    }
  for (int e = -400; e <= 400; ++e, ++n)
    if (pow2_bits(e) != u_of(ldexpf(1.f, e))) {
      printf("pow2 %d: bits %08x float %08x\n", e, pow2_bits(e), u_of(ldexpf(1.f, e)));
      ++bad;
    }
  printf("checked %d bad %d\n", n, bad);
  return bad != 0;
}
"""


def test_sf_exp_bits_equals_sf_exp(tmp_path):
    (tmp_path / "t.c").write_text(PROG)
    subprocess.run(["gcc", "-O1", "-I", str(ROOT / "rl-k8s-scheduler_amd/csrc"), str(tmp_path / "t.c"), "-o",
                    str(tmp_path / "t"), "-lm"], check=True)
    r = subprocess.run([str(tmp_path / "t")], capture_output=True, text=True)
    print(r.stdout)
    assert r.returncode == 0, r.stdout
    assert "checked 1828 bad 0" in r.stdout
