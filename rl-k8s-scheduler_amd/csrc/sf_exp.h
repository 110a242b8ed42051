// The split-fp16 scale exponent, on the float and on its bit pattern (host and device: tests/test_sf_exp_bits.py
// compiles this header on its own and compares the two forms).
#pragma once
#include <math.h>
#if defined(__HIPCC__) || defined(__CUDACC__)
#define RLKS_HD __host__ __device__ __forceinline__
#else
#define RLKS_HD static inline
#endif

// exponent e with mx 2^e in [2^14, 2^15), clamped to +-120; 0 for mx = 0 / non-finite (and above 3.4e38)
RLKS_HD int sf_exp(float mx) {
  if (!(mx > 0.f) || !(mx <= 3.4e38f)) return 0;
  int e;
  (void)frexpf(mx, &e);
  const int r = 15 - e;
  return r < -120 ? -120 : (r > 120 ? 120 : r);
}

// sf_exp on the bit pattern u of a float whose sign bit is clear (a maximum of absolute values), in integer
// arithmetic: a wave-uniform u keeps it on the scalar unit.  A denormal's frexp exponent is at most -126, so
// it clamps to 120; 0x7f7fc99e is 3.4e38f, above which (infinity and NaN included) sf_exp gives 0.
// Written as selects, not branches: the scalar unit runs it beside the vector work of other waves.
RLKS_HD int sf_exp_bits(unsigned u) {
  const int r = 15 - ((int)(u >> 23) - 126);  // (>= -114 with the sign bit clear; a denormal's 141 clamps to 120)
  const int rc = r > 120 ? 120 : r;
  return (u == 0u || u > 0x7f7fc99eu) ? 0 : rc;
}

// bit pattern of ldexpf(1.f, e) for any e: infinity above 127, a denormal down to -149, 0 below
RLKS_HD unsigned pow2_bits(int e) {
  const unsigned nrm = (unsigned)(e + 127) << 23, den = 1u << ((e + 149) & 31);
  const unsigned v = e >= -126 ? nrm : den;
  const unsigned w = e < -149 ? 0u : v;
  return e > 127 ? 0x7f800000u : w;
}
