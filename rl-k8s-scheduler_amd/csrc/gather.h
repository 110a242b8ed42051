// gather.h — the minibatch permutation and gather as the kernels of gather.hip and the reduce-plus-gather
// kernels of ppo.hip see them.
#pragma once

#include "mlp_common.h"

namespace rlks {

// ----------------------------------------------------------------------------- gather
// Balanced Feistel bijection on [0, 2^(2*half)) with per-epoch round keys, cycle-walked into
// [0, S): a fresh uniform-looking permutation of the train batch every epoch with no sort.
struct Perm {
  uint32_t key[4];
  uint32_t half, mask;
  uint64_t S;
};

__device__ __forceinline__ uint32_t mix32(uint32_t x) {
  x ^= x >> 16; x *= 0x7feb352du;
  x ^= x >> 15; x *= 0x846ca68bu;
  x ^= x >> 16;
  return x;
}

__device__ __forceinline__ uint64_t perm_apply(const Perm& P, uint64_t x) {
  do {
    uint32_t L = (uint32_t)(x >> P.half), R = (uint32_t)x & P.mask;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const uint32_t nl = R;
      R = (L ^ mix32(R ^ P.key[r])) & P.mask;
      L = nl;
    }
    x = ((uint64_t)L << P.half) | R;
  } while (x >= P.S);
  return x;
}

constexpr int MAX_GROUPS = 64;
struct GatherArgs {
  rlks_rollout_bufs b;
  Perm perm[MAX_GROUPS];  // one bijection of [0, T * Ng) per lane group
  int64_t row0g;          // first row of this minibatch within each group's permutation
  int rows, rows_g, Ng, D, A, stride;
  float* mb;
  const float* packed;    // rlks_ppo_pack records [T N][pstride] (gather_packed), else null
  int pstride;
};

// source index t * N + n of minibatch row i: rows [k rows_g, (k+1) rows_g) come from lane group
// k, whose permutation p -> (t = p / Ng, lane k Ng + p mod Ng).  groups: the entries of `perm`
// (debug checks: the group index against it, and the permutation's input against its domain --
// its output is in [0, S) by construction)
__device__ __forceinline__ int64_t gather_src(const Perm* perm, int64_t row0g, int rows_g, int Ng, int N, uint32_t i,
                                              int groups) {
  uint32_t k = i / (uint32_t)rows_g;
  uint64_t ii = i - k * (uint32_t)rows_g;
  if (!dcheck(k < (uint32_t)groups, DC_GATHER_GROUP, k)) k = 0;
  if (!dcheck((uint64_t)row0g + ii < perm[k].S, DC_GATHER_SRC, (long long)(row0g + ii))) ii = 0;
  const uint64_t p = perm_apply(perm[k], (uint64_t)(row0g + ii));
  uint64_t t, nl;
  if (p >> 32) {
    t = p / (uint64_t)Ng;
    nl = p - t * (uint64_t)Ng;
  } else {  // 32-bit division (every train batch below 2^32 rows per group)
    const uint32_t t32 = (uint32_t)p / (uint32_t)Ng;
    t = t32;
    nl = (uint32_t)p - t32 * (uint32_t)Ng;
  }
  return (int64_t)(t * (uint64_t)N + (uint64_t)k * Ng + nl);
}
__device__ __forceinline__ int64_t gather_src(const GatherArgs& g, uint32_t i) {
  return gather_src(g.perm, g.row0g, g.rows_g, g.Ng, g.b.N, i, (g.rows + g.rows_g - 1) / g.rows_g);
}

// minibatch rows from packed records: PS / 4 consecutive threads per row, thread q moving the
// record's 16-byte piece q, so that every load instruction reads whole 64-byte lines (one line
// per row for PS = 16) and the stores are contiguous
template <int S, int PS>
__device__ __forceinline__ void gather_packed_elem(const Perm* perm, int64_t row0g, int rows_g, int Ng, int N, int rows,
                                                   const float* packed, float* mb, uint32_t e) {
  constexpr int TPR = PS / 4;
  const uint32_t i = e / TPR, q = e % TPR;
  if (i >= (uint32_t)rows) return;
  const int64_t tn = gather_src(perm, row0g, rows_g, Ng, N, i, (rows + rows_g - 1) / rows_g);
  const float4 v = reinterpret_cast<const float4*>(packed + tn * PS)[q];
  if (4 * q < (uint32_t)S) reinterpret_cast<float4*>(mb + (size_t)i * S)[q] = v;
}

// The next SGD step's packed gather, run by extra blocks of this step's reduce (single rank): the
// reduce reads only gradient partials, and every kernel reading the minibatch buffer has finished
// when it starts, so the gather may rewrite that buffer; one launch instead of two, and the gather's
// latency-bound reads hide under the reduce's streaming.
constexpr int NEXT_GROUPS = 8;
struct NextGather {
  Perm perm[NEXT_GROUPS];
  int64_t row0g;
  int rows, rows_g, Ng, N;
  float* mb;
  const float* packed;
  int blk0;  // blocks [0, blk0) reduce, the rest gather
};

// The narrow record shapes (2, 4 or 8 clouds): minibatch stride S, packed stride PS.  with_record calls
// f(Rec<S, PS>{}) for the shape of `stride`, the one place the kernels' template instances are chosen;
// false (f not called): a wide record.
template <int S_, int PS_>
struct Rec {
  static constexpr int S = S_, PS = PS_;
};
template <class F>
inline bool with_record(int stride, F&& f) {
  if (stride == 12) f(Rec<12, 16>{});
  else if (stride == 20) f(Rec<20, 32>{});
  else if (stride == 36) f(Rec<36, 48>{});
  else return false;
  return true;
}

// the permutations and row split of one gather call, checked (gather.hip; g.b and g.packed are the caller's)
int gather_args(const rlks_mlp_desc* d, int T, int N, uint64_t perm_seed, int epoch, int groups, int group0,
                int64_t row0, int rows, float* mb, GatherArgs& g);

}  // namespace rlks
