// rollout_metrics.hip — per-iteration rollout metrics: one streaming reduction over
// what a rollout and rlks_gae left in the rollout buffers.
//
// The reference's training scripts print RLlib's episode_reward_mean and nothing about what the policy
// did (train_ppo.py:29-30); RLlib's slot for such figures is result["custom_metrics"].  Everything
// they need is in HBM after a rollout: actions, rewards, dones, values, vtarg and the utilisation
// third of each obs row.  HBM-bound: 17 B per sample of the flat arrays plus the obs rows' lines.
//
// Order (the same bits on every run, whichever workgroup finishes first):
//   stage one  k_rollout_metrics_part: a bounded grid strides over T N; sample -> (workgroup, wave,
//              lane) is a function of T N and the buffers' 16-byte phase alone; each lane adds its
//              samples in index order, lanes meet by xor butterflies, the workgroup's waves are added in
//              wave order, and the workgroup writes one partial record into the workspace;
//   stage two  k_rollout_metrics_final: the records are added in index order on three levels: chunks of
//              ceil(records / 256) consecutive records, groups of 8 chunks, then the groups.
// No floating-point atomics; the action histogram of A > 8 uses integer LDS atomics (exact).
#include <hip/hip_runtime.h>

#include "rlks_internal.h"

namespace rlks {

constexpr int RM_BLOCK = 256;
constexpr int RM_WAVES = RM_BLOCK / 64;
constexpr int RM_TILE = RM_BLOCK * 4;  // samples per workgroup and pass: one 16-byte load per lane and array
// grid bound: 4 workgroups (16 waves) per CU; one pass of the full grid covers RM_MAX_BLOCKS * RM_TILE
// = 1,048,576 samples, larger rollouts stride
constexpr int RM_MAX_BLOCKS = 1024;
constexpr int RM_SMALL = 8;  // up to 8 actions / clusters: per-lane register counters and sums
constexpr int RM_MAX_A = 4096, RM_MAX_C = 1024;  // LDS: 4 A + 32 C bytes
constexpr int RM_SH = RLKS_RM_FIXED + 2 * RM_SMALL;

struct RmArgs {
  const int32_t* actions;
  const float* rewards;
  const float* values;
  const float* vtarg;
  const uint8_t* dones;
  const float* obs;
  long long n;       // T N
  long long head;    // scalar samples before the first 16-byte group
  long long groups;  // 16-byte groups of 4 samples: [head, head + 4 groups)
  int D, A, C;
  int dones_u32;     // dones + head is 4-byte aligned: a group's done bytes are one dword
};

struct RmAcc {
  double rsum, vsum, tsum, tsq, dsum, dsq;
  float rmin, rmax;
  uint32_t dones, rows;
  uint32_t ac[RM_SMALL];
  double us[RM_SMALL];
};

template <bool SA>
__device__ __forceinline__ void rm_sample(RmAcc& a, uint32_t* hist, int A, int act, float r, float v, float vt) {
  const double rd = (double)r, vd = (double)v, td = (double)vt, res = td - vd;
  a.rsum += rd;
  a.vsum += vd;
  a.tsum += td;
  a.tsq += td * td;
  a.dsum += res;
  a.dsq += res * res;
  a.rmin = fminf(a.rmin, r);
  a.rmax = fmaxf(a.rmax, r);
  a.rows += 1u;
  if (SA) {
#pragma unroll
    for (int k = 0; k < RM_SMALL; ++k) a.ac[k] += (act == k) ? 1u : 0u;
  } else if ((unsigned)act < (unsigned)A) {
    atomicAdd(&hist[act], 1u);
  }
}

// the utilisation columns of obs row i (up to 8 clusters), W floats per load: the columns start 8 C
// bytes into a row of 4 D bytes, so 16-byte loads need C and D to be multiples of 4 (c3: C = 8, D = 24),
// 8-byte loads even C and D (c4: C = 2, D = 6)
template <int W>
__device__ __forceinline__ void rm_util(RmAcc& a, const RmArgs& p, long long i) {
  const float* __restrict__ row = p.obs + (size_t)i * p.D + 2 * p.C;
  if (W == 4) {
#pragma unroll
    for (int c = 0; c < RM_SMALL; c += 4)
      if (c < p.C) {
        const float4 u = *reinterpret_cast<const float4*>(row + c);
        a.us[c] += (double)u.x;
        a.us[c + 1] += (double)u.y;
        a.us[c + 2] += (double)u.z;
        a.us[c + 3] += (double)u.w;
      }
  } else if (W == 2) {
#pragma unroll
    for (int c = 0; c < RM_SMALL; c += 2)
      if (c < p.C) {
        const float2 u = *reinterpret_cast<const float2*>(row + c);
        a.us[c] += (double)u.x;
        a.us[c + 1] += (double)u.y;
      }
  } else {
#pragma unroll
    for (int c = 0; c < RM_SMALL; ++c)
      if (c < p.C) a.us[c] += (double)row[c];
  }
}

// SA: up to 8 actions (register counters); W: floats per load of the utilisation columns for up to 8
// clusters (register sums), 0 for more clusters (per-wave column sums in LDS)
template <bool SA, int W>
__global__ __launch_bounds__(RM_BLOCK) void k_rollout_metrics_part(RmArgs p, double* __restrict__ part) {
  // !SC: [RM_WAVES][C] utilisation sums; then !SA: [A] action histogram
  constexpr bool SC = W > 0;
  extern __shared__ double rm_dyn[];
  __shared__ double sh[RM_WAVES][RM_SH];
  double* const wutil = rm_dyn;
  uint32_t* const hist = (uint32_t*)(rm_dyn + (SC ? 0 : RM_WAVES * p.C));
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  if (!SA) {
    for (int k = threadIdx.x; k < p.A; k += RM_BLOCK) hist[k] = 0u;
    __syncthreads();
  }
  RmAcc a;
  a.rsum = a.vsum = a.tsum = a.tsq = a.dsum = a.dsq = 0.0;
  a.rmin = INFINITY;
  a.rmax = -INFINITY;
  a.dones = a.rows = 0u;
#pragma unroll
  for (int k = 0; k < RM_SMALL; ++k) { a.ac[k] = 0u; a.us[k] = 0.0; }

  // 16-byte groups: a wave takes 64 consecutive groups (256 samples) per pass
  const long long tiles = (p.groups + 63) / 64, vend = p.head + 4 * p.groups;
  for (long long q = (long long)blockIdx.x * RM_WAVES + wave; q < tiles; q += (long long)gridDim.x * RM_WAVES) {
    const long long g = q * 64 + lane;
    if (g < p.groups) {
      const long long i = p.head + 4 * g;
      const int4 a4 = *reinterpret_cast<const int4*>(p.actions + i);
      const float4 r4 = *reinterpret_cast<const float4*>(p.rewards + i);
      const float4 v4 = *reinterpret_cast<const float4*>(p.values + i);
      const float4 t4 = *reinterpret_cast<const float4*>(p.vtarg + i);
      uint32_t d4;
      if (p.dones_u32) {
        d4 = *reinterpret_cast<const uint32_t*>(p.dones + i);
      } else {
        d4 = (uint32_t)p.dones[i] | ((uint32_t)p.dones[i + 1] << 8) | ((uint32_t)p.dones[i + 2] << 16) |
             ((uint32_t)p.dones[i + 3] << 24);
      }
      rm_sample<SA>(a, hist, p.A, a4.x, r4.x, v4.x, t4.x);
      rm_sample<SA>(a, hist, p.A, a4.y, r4.y, v4.y, t4.y);
      rm_sample<SA>(a, hist, p.A, a4.z, r4.z, v4.z, t4.z);
      rm_sample<SA>(a, hist, p.A, a4.w, r4.w, v4.w, t4.w);
      a.dones += ((d4 & 0xffu) ? 1u : 0u) + ((d4 & 0xff00u) ? 1u : 0u) + ((d4 & 0xff0000u) ? 1u : 0u) +
                 ((d4 & 0xff000000u) ? 1u : 0u);
    }
    if (SC) {
      // the same 256 samples' obs rows, consecutive rows on consecutive lanes
      const long long base = p.head + q * 256;
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const long long i = base + j * 64 + lane;
        if (i < vend) rm_util<W>(a, p, i);
      }
    }
  }
  // scalar head [0, head) and tail [vend, n), strided over all threads of the grid
  const long long n_sc = p.head + (p.n - vend);
  for (long long s = (long long)blockIdx.x * RM_BLOCK + threadIdx.x; s < n_sc; s += (long long)gridDim.x * RM_BLOCK) {
    const long long i = s < p.head ? s : vend + (s - p.head);
    rm_sample<SA>(a, hist, p.A, p.actions[i], p.rewards[i], p.values[i], p.vtarg[i]);
    a.dones += p.dones[i] ? 1u : 0u;
    if (SC) rm_util<W>(a, p, i);
  }
  if (!SC) {
    // more than 8 clusters: the workgroup takes a contiguous range of rows, wave w its rows w, w + 4, ...,
    // a lane one column at a time (a row's columns are contiguous: 256-byte reads)
    const long long chunk = (p.n + gridDim.x - 1) / gridDim.x;
    const long long lo = (long long)blockIdx.x * chunk, hi = lo + chunk < p.n ? lo + chunk : p.n;
    for (int c0 = 0; c0 < p.C; c0 += 64) {
      const int c = c0 + lane;
      if (c < p.C) {
        const float* __restrict__ col = p.obs + 2 * p.C + c;
        double s = 0.0;
        for (long long i = lo + wave; i < hi; i += RM_WAVES) s += (double)col[(size_t)i * p.D];
        wutil[wave * p.C + c] = s;
      }
    }
  }

  // lanes meet by butterflies (every lane ends with the same bits), waves through LDS
  a.rsum = wave_sum(a.rsum);
  a.vsum = wave_sum(a.vsum);
  a.tsum = wave_sum(a.tsum);
  a.tsq = wave_sum(a.tsq);
  a.dsum = wave_sum(a.dsum);
  a.dsq = wave_sum(a.dsq);
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    a.rmin = fminf(a.rmin, __shfl_xor(a.rmin, o, 64));
    a.rmax = fmaxf(a.rmax, __shfl_xor(a.rmax, o, 64));
  }
  const unsigned long long rows = wave_sum_u64((unsigned long long)a.rows);
  const unsigned long long dones = wave_sum_u64((unsigned long long)a.dones);
  unsigned long long ac[RM_SMALL];
#pragma unroll
  for (int k = 0; k < RM_SMALL; ++k) {
    ac[k] = SA ? wave_sum_u64((unsigned long long)a.ac[k]) : 0ull;
    a.us[k] = SC ? wave_sum(a.us[k]) : 0.0;
  }
  if (lane == 0) {
    double* w = sh[wave];
    w[RLKS_RM_ROWS] = (double)rows;
    w[RLKS_RM_REWARD_SUM] = a.rsum;
    w[RLKS_RM_REWARD_MIN] = (double)a.rmin;
    w[RLKS_RM_REWARD_MAX] = (double)a.rmax;
    w[RLKS_RM_DONES] = (double)dones;
    w[RLKS_RM_VALUE_SUM] = a.vsum;
    w[RLKS_RM_VTARG_SUM] = a.tsum;
    w[RLKS_RM_VTARG_SQ] = a.tsq;
    w[RLKS_RM_RESID_SUM] = a.dsum;
    w[RLKS_RM_RESID_SQ] = a.dsq;
#pragma unroll
    for (int k = 0; k < RM_SMALL; ++k) {
      w[RLKS_RM_FIXED + k] = (double)ac[k];
      w[RLKS_RM_FIXED + RM_SMALL + k] = a.us[k];
    }
  }
  __syncthreads();
  // the workgroup's record: its waves in wave order
  const int S = RLKS_RM_FIXED + p.A + p.C;
  double* __restrict__ rec = part + (size_t)blockIdx.x * S;
  for (int s = threadIdx.x; s < S; s += RM_BLOCK) {
    double v;
    if (s < RLKS_RM_FIXED) {
      v = sh[0][s];
      for (int w = 1; w < RM_WAVES; ++w)
        v = s == RLKS_RM_REWARD_MIN ? fmin(v, sh[w][s]) : s == RLKS_RM_REWARD_MAX ? fmax(v, sh[w][s]) : v + sh[w][s];
    } else if (s < RLKS_RM_FIXED + p.A) {
      const int k = s - RLKS_RM_FIXED;
      if (SA) {
        v = sh[0][RLKS_RM_FIXED + k];
        for (int w = 1; w < RM_WAVES; ++w) v += sh[w][RLKS_RM_FIXED + k];
      } else {
        v = (double)hist[k];
      }
    } else {
      const int c = s - RLKS_RM_FIXED - p.A;
      if (SC) {
        v = sh[0][RLKS_RM_FIXED + RM_SMALL + c];
        for (int w = 1; w < RM_WAVES; ++w) v += sh[w][RLKS_RM_FIXED + RM_SMALL + c];
      } else {
        v = wutil[c];
        for (int w = 1; w < RM_WAVES; ++w) v += wutil[w * p.C + c];
      }
    }
    rec[s] = v;
  }
}

__device__ __forceinline__ double rm_merge(int slot, double a, double b) {
  return slot == RLKS_RM_REWARD_MIN ? fmin(a, b) : slot == RLKS_RM_REWARD_MAX ? fmax(a, b) : a + b;
}

// Stage two, RM_FIN_SLOTS slots per workgroup, the nb records merged in index order on three levels:
// chunk c = records [c R, (c + 1) R), R = ceil(nb / 256) <= 4, by one thread per (chunk, slot), every load
// of the thread in flight at once and neighbouring threads on neighbouring slots; groups of 8 chunks by
// one thread per (group, slot); the 32 groups by one thread per slot.  (One thread per slot over all nb
// records waits for memory nb / 8 times in a row: 0.3 ms at 1,024 records.)
constexpr int RM_FIN_SLOTS = 8;
constexpr int RM_FIN_R = RM_MAX_BLOCKS / RM_BLOCK;  // records per chunk, at most
constexpr int RM_FIN_GROUP = 8, RM_FIN_GROUPS = RM_BLOCK / RM_FIN_GROUP;
static_assert(RM_FIN_R * RM_BLOCK == RM_MAX_BLOCKS && RM_BLOCK % RM_FIN_SLOTS == 0, "stage two covers every record");
__global__ __launch_bounds__(RM_BLOCK) void k_rollout_metrics_final(const double* __restrict__ part, int nb, int S,
                                                                    double* __restrict__ out) {
  __shared__ double shc[RM_BLOCK][RM_FIN_SLOTS];
  __shared__ double shg[RM_FIN_GROUPS][RM_FIN_SLOTS];
  const int R = (nb + RM_BLOCK - 1) / RM_BLOCK, K = (nb + R - 1) / R;  // K <= 256 chunks, none empty
  const int j = threadIdx.x % RM_FIN_SLOTS, q = threadIdx.x / RM_FIN_SLOTS, s = blockIdx.x * RM_FIN_SLOTS + j;
  const bool live = s < S;
  const int sl = live ? s : S - 1;
  // chunks q, q + 32, ...: loads first (indices clamped into the records, so none is conditional)
  double v[RM_FIN_SLOTS][RM_FIN_R];
#pragma unroll
  for (int it = 0; it < RM_FIN_SLOTS; ++it) {
    const int c = it * (RM_BLOCK / RM_FIN_SLOTS) + q;
#pragma unroll
    for (int k = 0; k < RM_FIN_R; ++k) {
      const int b = c * R + k < nb ? c * R + k : nb - 1;
      v[it][k] = part[(size_t)b * S + sl];
    }
  }
#pragma unroll
  for (int it = 0; it < RM_FIN_SLOTS; ++it) {
    const int c = it * (RM_BLOCK / RM_FIN_SLOTS) + q;
    double x = v[it][0];
#pragma unroll
    for (int k = 1; k < RM_FIN_R; ++k)
      if (k < R && c * R + k < nb) x = rm_merge(s, x, v[it][k]);
    shc[c][j] = x;  // chunks c >= K are not read below
  }
  __syncthreads();
  if (q * RM_FIN_GROUP < K) {  // group q = chunks [8 q, 8 q + 8)
    double x = shc[q * RM_FIN_GROUP][j];
#pragma unroll
    for (int k = 1; k < RM_FIN_GROUP; ++k)
      if (q * RM_FIN_GROUP + k < K) x = rm_merge(s, x, shc[q * RM_FIN_GROUP + k][j]);
    shg[q][j] = x;
  }
  __syncthreads();
  if (q == 0 && live) {
    double x = shg[0][j];
#pragma unroll
    for (int g = 1; g < RM_FIN_GROUPS; ++g)
      if (g * RM_FIN_GROUP < K) x = rm_merge(s, x, shg[g][j]);
    out[s] = x;
  }
}

static int rm_blocks(long long n) {
  const long long b = (n + RM_TILE - 1) / RM_TILE;
  return (int)(b < 1 ? 1 : b > RM_MAX_BLOCKS ? RM_MAX_BLOCKS : b);
}

}  // namespace rlks

using namespace rlks;

extern "C" {

int rlks_rollout_metrics_size(int A, int C) {
  RLKS_REQUIRE(A >= 1 && C >= 1, RLKS_ERR_ARG, "rlks_rollout_metrics: A and C must be positive");
  RLKS_REQUIRE(A <= RM_MAX_A && C <= RM_MAX_C, RLKS_ERR_UNSUPPORTED,
               "rlks_rollout_metrics: at most 4096 actions and 1024 clusters");
  return RLKS_RM_FIXED + A + C;
}

int rlks_rollout_metrics_workspace_bytes(int T, int N, int A, int C, int64_t* bytes) {
  RLKS_REQUIRE(bytes && T > 0 && N > 0, RLKS_ERR_ARG, "rlks_rollout_metrics_workspace_bytes: bad argument");
  const int S = rlks_rollout_metrics_size(A, C);
  if (S < 0) return S;
  *bytes = (int64_t)rm_blocks((long long)T * N) * S * (int64_t)sizeof(double);
  return RLKS_OK;
}

int rlks_rollout_metrics(const rlks_rollout_bufs* b, int D, int A, int C, double* out, void* workspace,
                         int64_t workspace_bytes, void* stream) {
  RLKS_REQUIRE(b && out && workspace, RLKS_ERR_ARG, "rlks_rollout_metrics: null argument");
  RLKS_REQUIRE(b->obs && b->values && b->actions && b->rewards && b->dones && b->vtarg, RLKS_ERR_ARG,
               "rlks_rollout_metrics: obs, values, actions, rewards, dones and vtarg are required");
  RLKS_REQUIRE(b->T > 0 && b->N > 0, RLKS_ERR_ARG, "rlks_rollout_metrics: T and N must be positive");
  const int S = rlks_rollout_metrics_size(A, C);
  if (S < 0) return S;
  RLKS_REQUIRE(D >= 3 * C, RLKS_ERR_ARG, "rlks_rollout_metrics: an obs row holds 3 C columns");
  RmArgs p{};
  p.actions = b->actions;
  p.rewards = b->rewards;
  p.values = b->values;
  p.vtarg = b->vtarg;
  p.dones = b->dones;
  p.obs = b->obs;
  p.n = (long long)b->T * b->N;
  p.D = D;
  p.A = A;
  p.C = C;
  const int nb = rm_blocks(p.n);
  RLKS_REQUIRE(((uintptr_t)workspace & 7) == 0 && workspace_bytes >= (int64_t)nb * S * (int64_t)sizeof(double),
               RLKS_ERR_ARG, "rlks_rollout_metrics: workspace too small or misaligned");
  // 16-byte loads where the four arrays share their 16-byte phase; everything else is the scalar path
  const uintptr_t pa = (uintptr_t)p.actions, pr = (uintptr_t)p.rewards, pv = (uintptr_t)p.values,
                  pt = (uintptr_t)p.vtarg;
  if ((((pa ^ pr) | (pa ^ pv) | (pa ^ pt)) & 15) == 0 && (pa & 3) == 0) {
    p.head = (long long)(((16 - (pa & 15)) & 15) / 4);
    if (p.head > p.n) p.head = p.n;
    p.groups = (p.n - p.head) / 4;
  }
  p.dones_u32 = (((uintptr_t)p.dones + (uintptr_t)p.head) & 3) == 0;
  hipStream_t s = (hipStream_t)stream;
  double* part = (double*)workspace;
  const bool sa = A <= RM_SMALL, sc = C <= RM_SMALL;
  // floats per load of a row's utilisation columns (obs + 2 C, rows 4 D bytes apart)
  const uintptr_t pu = (uintptr_t)(p.obs + 2 * C);
  const int W = !sc ? 0 : (C % 4 == 0 && D % 4 == 0 && (pu & 15) == 0) ? 4 : (C % 2 == 0 && D % 2 == 0 && (pu & 7) == 0) ? 2 : 1;
  const size_t lds = (sc ? 0 : (size_t)RM_WAVES * C * sizeof(double)) + (sa ? 0 : (size_t)A * sizeof(uint32_t));
#define RM_LAUNCH(SA_, W_) \
  hipLaunchKernelGGL((k_rollout_metrics_part<SA_, W_>), dim3(nb), dim3(RM_BLOCK), lds, s, p, part)
  if (sa) {
    if (W == 4) RM_LAUNCH(true, 4);
    else if (W == 2) RM_LAUNCH(true, 2);
    else if (W == 1) RM_LAUNCH(true, 1);
    else RM_LAUNCH(true, 0);
  } else {
    if (W == 4) RM_LAUNCH(false, 4);
    else if (W == 2) RM_LAUNCH(false, 2);
    else if (W == 1) RM_LAUNCH(false, 1);
    else RM_LAUNCH(false, 0);
  }
#undef RM_LAUNCH
  RLKS_LAUNCHED();
  hipLaunchKernelGGL(k_rollout_metrics_final, dim3(cdiv(S, RM_FIN_SLOTS)), dim3(RM_BLOCK), 0, s, part, nb, S, out);
  RLKS_LAUNCHED();
  return RLKS_OK;
}

}  // extern "C"
