// obs_filter.h — the observation filter as the rollout loops see it (obs_filter.hip).
#pragma once

#include "rlks_internal.h"

namespace rlks {

// One filtered element, y = (float)(((double)x - mean[c]) * inv[c]): the apply kernel's arithmetic, and
// the serving kernel's (policy_act.hip) on the rows it loads, so both give the same bits.  sm / si: the
// state's mean and inv vectors (global or LDS).  A subtract then a multiply: nothing an FMA could fuse.
__device__ __forceinline__ float of_one(float x, const double* sm, const double* si, int c, int D) {
  if (!dcheck((unsigned)c < (unsigned)D, DC_FILTER_COL, c)) c = 0;
  return (float)(((double)x - sm[c]) * si[c]);
}

// Optional argument of the rollout host loops (rlks_rollout_filtered): with a tap, the env's
// observation output of step t goes to raw[t + 1] and one apply launch writes bufs->obs[t + 1] =
// filter(raw[t + 1]) before the next forward reads it.  Without one (nullptr) the loops issue exactly
// the launches of the unfiltered entries.
struct ObsTap {
  const double* state;  // double[rlks_obs_filter_size(D)]
  float* raw;           // [T + 1][N][D]
};

// where the env writes the observations of time row t ([N][D])
inline float* tap_obs_out(const ObsTap* tap, const rlks_rollout_bufs* b, int D, int t) {
  return (tap ? tap->raw : b->obs) + (size_t)t * b->N * D;
}
// bufs->obs[t] = filter(raw[t]): one launch with a tap, nothing without
inline int tap_apply(const ObsTap* tap, const rlks_rollout_bufs* b, int D, int t, hipStream_t s) {
  if (!tap) return RLKS_OK;
  const size_t o = (size_t)t * b->N * D;
  return rlks_obs_filter_apply(tap->state, tap->raw + o, b->obs + o, b->N, D, s);
}

}  // namespace rlks
