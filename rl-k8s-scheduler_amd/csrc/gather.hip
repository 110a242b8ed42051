// gather.hip — minibatch records: the per-epoch permutation, the gather from the rollout arrays, the
// packed sample records and the gather from them (include/rlks.h, section K4).
#include "gather.h"

namespace rlks {

// element j of sample tn's record [obs D | logits A | adv | vtarg | logp | action | 0...]; J: the caller's
// index type (int, or k_gather's uint32_t), which the address arithmetic keeps so each kernel's code stays as it was
template <typename J>
__device__ __forceinline__ float rec_field(const rlks_rollout_bufs& b, int D, int A, int64_t tn, J j) {
  float v = 0.f;
  if ((int)j < D) v = b.obs[tn * D + j];
  else if ((int)j < D + A) v = b.logits[tn * A + (j - D)];
  else if ((int)j == D + A) v = b.adv[tn];
  else if ((int)j == D + A + 1) v = b.vtarg[tn];
  else if ((int)j == D + A + 2) v = b.logp[tn];
  else if ((int)j == D + A + 3) v = (float)b.actions[tn];
  return v;
}

// narrow records (stride 12 / 20 / 36: 2, 4 or 8 clouds): one thread per row computes the row's permuted source
// once, loads its fields (obs and logits contiguous, four scalars) and writes the record as
// 16-byte stores; consecutive threads write consecutive records
template <int S>
__global__ __launch_bounds__(256) void k_gather_rows(GatherArgs g) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= (uint32_t)g.rows) return;
  const int64_t tn = gather_src(g, i);
  float rec[S];
#pragma unroll
  for (int j = 0; j < S; ++j) rec[j] = rec_field(g.b, g.D, g.A, tn, j);
  float4* dst = reinterpret_cast<float4*>(g.mb + (size_t)i * S);
#pragma unroll
  for (int q = 0; q < S / 4; ++q) {
    dst[q] = make_float4(rec[4 * q], rec[4 * q + 1], rec[4 * q + 2], rec[4 * q + 3]);
  }
}

// wide records: one thread per record element (row i = e / stride, field j), so the record
// stores are fully coalesced and each row's fields are read contiguously; the row's permuted
// source index is recomputed per element
__global__ void k_gather(GatherArgs g) {
  const uint32_t e = blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= (uint32_t)g.rows * (uint32_t)g.stride) return;
  const uint32_t i = e / (uint32_t)g.stride, j = e - i * (uint32_t)g.stride;
  const int64_t tn = gather_src(g, i);  // (named, and ahead of D and A: as one expression the kernel's code changes)
  const int D = g.D, A = g.A;
  g.mb[(size_t)e] = rec_field(g.b, D, A, tn, j);
}

// Sample records in rollout order, one 64-byte-aligned record per sample (c2 / c4: exactly one
// 64-byte line), so that a minibatch gather reads one line per row instead of one line from each
// of the six rollout arrays (obs, logits, adv, vtarg, logp, action): one thread per sample, 16-byte
// streaming stores.
template <int PS>
__global__ __launch_bounds__(256) void k_pack(rlks_rollout_bufs b, int D, int A, float* __restrict__ packed) {
  constexpr int TPR = PS / 4;  // threads per record, thread q writes floats [4q, 4q + 4)
  const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const int64_t tn = e / TPR;
  const int q = (int)(e % TPR);
  if (tn >= (int64_t)b.T * b.N) return;
  float rec[4];
#pragma unroll
  for (int c = 0; c < 4; ++c) rec[c] = rec_field(b, D, A, tn, 4 * q + c);
  typedef float f32x4 __attribute__((ext_vector_type(4)));
  __builtin_nontemporal_store(f32x4{rec[0], rec[1], rec[2], rec[3]}, reinterpret_cast<f32x4*>(packed + tn * PS) + q);
}

template <int S, int PS>
__global__ __launch_bounds__(256) void k_gather_packed(GatherArgs g) {
  gather_packed_elem<S, PS>(g.perm, g.row0g, g.rows_g, g.Ng, g.b.N, g.rows, g.packed, g.mb,
                            blockIdx.x * blockDim.x + threadIdx.x);
}

static Perm make_perm(uint64_t seed, int epoch, uint64_t S) {
  Perm P{};
  uint32_t bits = 2;
  while ((1ull << bits) < S) ++bits;
  if (bits & 1) ++bits;
  P.half = bits / 2;
  P.mask = (P.half >= 32) ? 0xffffffffu : ((1u << P.half) - 1u);
  P.S = S;
  uint64_t z = seed ^ (0x9E3779B97F4A7C15ull * (uint64_t)(epoch + 1));
  for (int r = 0; r < 4; ++r) {  // splitmix64 round keys
    z += 0x9E3779B97F4A7C15ull;
    uint64_t x = z;
    x = (x ^ (x >> 30)) * 0xBF58476D1CE4E5B9ull;
    x = (x ^ (x >> 27)) * 0x94D049BB133111EBull;
    P.key[r] = (uint32_t)(x ^ (x >> 31));
  }
  return P;
}

int gather_args(const rlks_mlp_desc* d, int T, int N, uint64_t perm_seed, int epoch, int groups, int group0,
                int64_t row0, int rows, float* mb, GatherArgs& g) {
  RLKS_REQUIRE(groups >= 1 && groups <= MAX_GROUPS && group0 >= 0 && N % groups == 0 && rows % groups == 0 &&
                   row0 % groups == 0, RLKS_ERR_ARG,
               "rlks_ppo_gather: groups must divide the lanes, the rows and row0 (at most 64 groups)");
  const int Ng = N / groups;
  const uint64_t Sg = (uint64_t)T * (uint64_t)Ng;
  RLKS_REQUIRE(row0 >= 0 && (uint64_t)(row0 + rows) / groups <= Sg, RLKS_ERR_ARG, "rlks_ppo_gather: rows out of range");
  g = GatherArgs{};
  // group k's key: perm_seed for global group 0 (the single-group gather), else perm_seed offset by
  // an odd 64-bit multiple of the global group id
  for (int k = 0; k < groups; ++k)
    g.perm[k] = make_perm(perm_seed + 0x632BE59BD9B4E019ull * (uint64_t)(group0 + k), epoch, Sg);
  g.row0g = row0 / groups;
  g.rows_g = rows / groups;
  g.Ng = Ng;
  g.rows = rows;
  g.D = d->obs_dim;
  g.A = d->n_actions;
  g.stride = mb_stride(d->obs_dim, d->n_actions);
  g.mb = mb;
  RLKS_REQUIRE((int64_t)rows * g.stride < (int64_t)1 << 31, RLKS_ERR_UNSUPPORTED,
               "rlks_ppo_gather: at most 2^31 record elements per call");
  return RLKS_OK;
}

}  // namespace rlks

using namespace rlks;

extern "C" {

int rlks_minibatch_stride(const rlks_mlp_desc* d) { return d ? mb_stride(d->obs_dim, d->n_actions) : 0; }

int rlks_ppo_gather(const rlks_mlp_desc* d, const rlks_rollout_bufs* b, uint64_t perm_seed, int epoch,
                    int64_t row0, int rows, const float* dyn, float* mb, void* stream) {
  return rlks_ppo_gather_grouped(d, b, perm_seed, epoch, 1, 0, row0, rows, dyn, mb, stream);
}

int rlks_ppo_gather_grouped(const rlks_mlp_desc* d, const rlks_rollout_bufs* b, uint64_t perm_seed, int epoch,
                            int groups, int group0, int64_t row0, int rows, const float* dyn, float* mb,
                            void* stream) {
  RLKS_REQUIRE(d && b && mb && rows >= 0, RLKS_ERR_ARG, "rlks_ppo_gather: bad argument");
  (void)dyn;  // advantages are standardised inside the loss kernel from dyn
  GatherArgs g;
  if (int rc = gather_args(d, b->T, b->N, perm_seed, epoch, groups, group0, row0, rows, mb, g)) return rc;
  if (rows == 0) return RLKS_OK;
  g.b = *b;
  hipStream_t s = (hipStream_t)stream;
  if (!with_record(g.stride, [&](auto r) {
        hipLaunchKernelGGL(k_gather_rows<decltype(r)::S>, dim3(cdiv(rows, 256)), dim3(256), 0, s, g);
      }))
    hipLaunchKernelGGL(k_gather, dim3(cdiv(rows * g.stride, 256)), dim3(256), 0, s, g);
  RLKS_LAUNCHED();
  return RLKS_OK;
}

int rlks_packed_stride(const rlks_mlp_desc* d) {
  int ps = 0;
  if (d) with_record(mb_stride(d->obs_dim, d->n_actions), [&](auto r) { ps = decltype(r)::PS; });
  return ps;
}

int rlks_ppo_pack(const rlks_mlp_desc* d, const rlks_rollout_bufs* b, float* packed, void* stream) {
  RLKS_REQUIRE(d && b && packed && b->T > 0 && b->N > 0, RLKS_ERR_ARG, "rlks_ppo_pack: bad argument");
  const int ps = rlks_packed_stride(d);
  RLKS_REQUIRE(ps > 0, RLKS_ERR_UNSUPPORTED, "rlks_ppo_pack: records of 2, 4 or 8 clouds (obs 6 / 12 / 24) only");
  const int64_t n = (int64_t)b->T * b->N;
  const dim3 grid(cdiv(n * (ps / 4), 256));
  hipStream_t s = (hipStream_t)stream;
  const int D = d->obs_dim, A = d->n_actions;
  with_record(mb_stride(D, A), [&](auto r) {
    hipLaunchKernelGGL(k_pack<decltype(r)::PS>, grid, dim3(256), 0, s, *b, D, A, packed);
  });
  RLKS_LAUNCHED();
  return RLKS_OK;
}

int rlks_ppo_gather_packed(const rlks_mlp_desc* d, const float* packed, int T, int N, uint64_t perm_seed, int epoch,
                           int groups, int group0, int64_t row0, int rows, float* mb, void* stream) {
  RLKS_REQUIRE(d && packed && mb && rows >= 0 && T > 0 && N > 0, RLKS_ERR_ARG, "rlks_ppo_gather_packed: bad argument");
  const int ps = rlks_packed_stride(d);
  RLKS_REQUIRE(ps > 0, RLKS_ERR_UNSUPPORTED, "rlks_ppo_gather_packed: records of 2, 4 or 8 clouds only");
  GatherArgs g;
  if (int rc = gather_args(d, T, N, perm_seed, epoch, groups, group0, row0, rows, mb, g)) return rc;
  if (rows == 0) return RLKS_OK;
  g.b.T = T;
  g.b.N = N;
  g.packed = packed;
  g.pstride = ps;
  hipStream_t s = (hipStream_t)stream;
  const dim3 rg(cdiv((int64_t)rows * ps / 4, 256));
  with_record(g.stride, [&](auto r) {
    using R = decltype(r);
    hipLaunchKernelGGL((k_gather_packed<R::S, R::PS>), rg, dim3(256), 0, s, g);
  });
  RLKS_LAUNCHED();
  return RLKS_OK;
}

}  // extern "C"
