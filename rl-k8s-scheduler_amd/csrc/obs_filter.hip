// obs_filter.hip — observation_filter="MeanStdFilter" (DESIGN.md §21): running mean / standard
// deviation per observation column, kept on the device.
//
// RLlib's MeanStdFilter standardises every observation as (x - mean) / (std + 1e-8) with the unbiased
// running variance; RLlib is absent from the reference tree, so the arithmetic is this project's own
// specification (include/rlks.h) and is pinned by tests/obs_filter_ref.py.
//
//   apply   y = (float)(((double)x - mean[d]) * inv[d]): a streaming kernel, 16-byte loads and stores
//           where both pointers allow them, the column carried along the flat index, the mean / inv
//           table in LDS.  In place (y == x) is allowed: an element is read and written by one thread.
//   stats   the batch record [rows, s1[D], s2[D]], s1 = sum (x - K), s2 = sum (x - K)^2 in f64 with
//           K = the state's mean: stage one, a grid that depends on (rows, D) alone, every workgroup a
//           contiguous block of rows and every thread one column of it in row order (consecutive
//           threads read consecutive floats); a workgroup's threads of one column are added in thread
//           order into one partial per workgroup; stage two adds the partials in index order on two
//           levels.  No floating-point atomics: the same bits on every run.
//   merge   Chan's update of (count, mean, m2) by the record, one workgroup.
// This translation unit is compiled with -ffp-contract=off: every product and sum is rounded on its
// own, as the numpy restatement forms them.
#include <hip/hip_runtime.h>

#include "obs_filter.h"

namespace rlks {

constexpr int OF_MAX_D = 512;  // columns: LDS tables of 2 x 4 KB; two column slots per stats thread
constexpr int OF_BLOCK = 256;
constexpr int OF_APPLY_MAX_BLOCKS = 2048;  // 8 workgroups per CU, larger inputs stride
constexpr int OF_PART_MAX_BLOCKS = 1024;   // stats stage one: partial records at most
constexpr int OF_PART_MIN_FLOATS = 16384;  // stats: floats per workgroup before a second one is used
constexpr int OF_UNROLL = 8;               // stats: loads in flight per thread
constexpr int OF_FIN_SLOTS = 4, OF_FIN_Q = OF_BLOCK / OF_FIN_SLOTS;

template <bool VEC>
__global__ __launch_bounds__(OF_BLOCK) void k_obs_filter_apply(const double* __restrict__ state, const float* x,
                                                               float* y, long long total, int D) {
  __shared__ double sm[OF_MAX_D], si[OF_MAX_D];
  for (int d = threadIdx.x; d < D; d += OF_BLOCK) {
    sm[d] = state[RLKS_OF_VECS + RLKS_OF_MEAN * D + d];
    si[d] = state[RLKS_OF_VECS + RLKS_OF_INV * D + d];
  }
  __syncthreads();
  const long long tid = (long long)blockIdx.x * OF_BLOCK + threadIdx.x, stride = (long long)gridDim.x * OF_BLOCK;
  if (VEC) {
    const long long groups = total / 4;
    int col = (int)((4 * tid) % D);
    const int adv = (int)((4 * stride) % D);
    for (long long g = tid; g < groups; g += stride) {
      dcheck(4 * g + 3 < total, DC_FILTER_IDX, g);
      const float4 v = reinterpret_cast<const float4*>(x)[g];
      float4 o;
      int c = col;
      o.x = of_one(v.x, sm, si, c, D);
      c = c + 1 == D ? 0 : c + 1;
      o.y = of_one(v.y, sm, si, c, D);
      c = c + 1 == D ? 0 : c + 1;
      o.z = of_one(v.z, sm, si, c, D);
      c = c + 1 == D ? 0 : c + 1;
      o.w = of_one(v.w, sm, si, c, D);
      reinterpret_cast<float4*>(y)[g] = o;
      col += adv;
      if (col >= D) col -= D;
    }
    const long long i = 4 * groups + tid;  // the last total % 4 floats
    if (i < total) y[i] = of_one(x[i], sm, si, (int)(i % D), D);
  } else {
    int col = (int)(tid % D);
    const int adv = (int)(stride % D);
    for (long long i = tid; i < total; i += stride) {
      y[i] = of_one(x[i], sm, si, col, D);
      col += adv;
      if (col >= D) col -= D;
    }
  }
}

// Stage one.  D <= 256: P = D floor(256 / D) threads are live, thread j takes column j % D of the rows
// lo + j / D, + RP, + 2 RP, ... (RP = 256 / D rows per pass, one contiguous run of P floats).  D > 256:
// one row per pass, thread j its columns j and j + 256.  part[block][2 D] = s1[D], s2[D].
__global__ __launch_bounds__(OF_BLOCK) void k_obs_filter_part(const double* __restrict__ state,
                                                              const float* __restrict__ x, long long rows, int D,
                                                              double* __restrict__ part) {
  __shared__ double sh[2][OF_BLOCK];
  const bool narrow = D <= OF_BLOCK;
  const int RP = narrow ? OF_BLOCK / D : 1, P = narrow ? D * RP : OF_BLOCK;
  const int j = threadIdx.x, rsub = narrow ? j / D : 0, c0 = j - rsub * D;
  const long long chunk = (rows + gridDim.x - 1) / gridDim.x;
  const long long lo = (long long)blockIdx.x * chunk, hi = lo + chunk < rows ? lo + chunk : rows;
  double* __restrict__ rec = part + (size_t)blockIdx.x * 2 * D;
  for (int k = 0; k < (narrow ? 1 : OF_MAX_D / OF_BLOCK); ++k) {
    const int col = c0 + k * OF_BLOCK;
    const bool live = j < P && col < D;
    double s1 = 0.0, s2 = 0.0;
    if (live) {
      const double K = state[RLKS_OF_VECS + RLKS_OF_MEAN * D + col];
      const float* __restrict__ p = x + col;
      long long r = lo + rsub;
      for (; r + (long long)(OF_UNROLL - 1) * RP < hi; r += (long long)OF_UNROLL * RP) {
        float v[OF_UNROLL];
#pragma unroll
        for (int u = 0; u < OF_UNROLL; ++u) v[u] = p[(size_t)(r + (long long)u * RP) * D];
#pragma unroll
        for (int u = 0; u < OF_UNROLL; ++u) {
          const double d = (double)v[u] - K;
          s1 += d;
          s2 += d * d;
        }
      }
      for (; r < hi; r += RP) {
        dcheck(r >= 0 && r < rows, DC_FILTER_IDX, r);
        const double d = (double)p[(size_t)r * D] - K;
        s1 += d;
        s2 += d * d;
      }
    }
    if (narrow) {
      sh[0][j] = s1;
      sh[1][j] = s2;
      __syncthreads();
      if (j < D) {  // the column's threads in thread order
        double a = sh[0][j], b = sh[1][j];
        for (int q = 1; q < RP; ++q) {
          a += sh[0][q * D + j];
          b += sh[1][q * D + j];
        }
        rec[j] = a;
        rec[D + j] = b;
      }
    } else if (live) {
      rec[col] = s1;
      rec[D + col] = s2;
    }
  }
}

// Stage two, OF_FIN_SLOTS slots per workgroup: thread (q, slot) adds the partials [q R, (q + 1) R), R =
// ceil(nb / 64), in index order; thread (0, slot) then adds the 64 sums in order.
__global__ __launch_bounds__(OF_BLOCK) void k_obs_filter_final(const double* __restrict__ part, int nb, int S,
                                                               long long rows, double* __restrict__ record) {
  __shared__ double shq[OF_FIN_Q][OF_FIN_SLOTS];
  const int jj = threadIdx.x % OF_FIN_SLOTS, q = threadIdx.x / OF_FIN_SLOTS, s = blockIdx.x * OF_FIN_SLOTS + jj;
  const int R = (nb + OF_FIN_Q - 1) / OF_FIN_Q;
  double a = 0.0;
  if (s < S) {
    const int b0 = q * R, b1 = b0 + R < nb ? b0 + R : nb;
    for (int b = b0; b < b1; ++b) a += part[(size_t)b * S + s];
  }
  shq[q][jj] = a;
  __syncthreads();
  if (q == 0 && s < S) {
    double v = shq[0][jj];
    for (int k = 1; k < OF_FIN_Q; ++k) v += shq[k][jj];
    record[RLKS_OFR_SUMS + s] = v;
  }
  if (blockIdx.x == 0 && threadIdx.x == 0) record[RLKS_OFR_ROWS] = (double)rows;
}

__device__ __forceinline__ double of_inv(double n, double m2) {
  return n >= 2.0 ? 1.0 / (sqrt(m2 / (n - 1.0)) + 1e-8) : 1.0;
}

__global__ __launch_bounds__(OF_BLOCK) void k_obs_filter_init(double* __restrict__ state, int D) {
  for (int i = threadIdx.x; i < RLKS_OF_VECS + RLKS_OF_NVEC * D; i += OF_BLOCK)
    state[i] = i >= RLKS_OF_VECS + RLKS_OF_INV * D ? 1.0 : 0.0;
}

__global__ __launch_bounds__(OF_BLOCK) void k_obs_filter_merge(double* __restrict__ state,
                                                               const double* __restrict__ record, int D) {
  const double na = state[RLKS_OF_COUNT], nb = record[RLKS_OFR_ROWS];
  __syncthreads();  // every thread holds the old count before thread 0 replaces it
  if (!(nb > 0.0)) return;
  const double n = na + nb;
  for (int d = threadIdx.x; d < D; d += OF_BLOCK) {
    double* mean = state + RLKS_OF_VECS + RLKS_OF_MEAN * D + d;
    double* m2 = state + RLKS_OF_VECS + RLKS_OF_M2 * D + d;
    const double s1 = record[RLKS_OFR_SUMS + d], s2 = record[RLKS_OFR_SUMS + D + d];
    const double delta = s1 / nb;
    const double m2n = (*m2 + (s2 - s1 * delta)) + (delta * delta) * ((na * nb) / n);
    *mean = *mean + delta * (nb / n);
    // a column that does not vary has m2 = 0 up to rounding: never the root of a negative number
    *m2 = m2n > 0.0 ? m2n : 0.0;
    state[RLKS_OF_VECS + RLKS_OF_INV * D + d] = of_inv(n, *m2);
  }
  if (threadIdx.x == 0) state[RLKS_OF_COUNT] = n;
}

static int of_part_blocks(long long rows, int D) {
  const long long b = (rows * D + OF_PART_MIN_FLOATS - 1) / OF_PART_MIN_FLOATS;
  return (int)(b < 1 ? 1 : b > OF_PART_MAX_BLOCKS ? OF_PART_MAX_BLOCKS : b);
}

}  // namespace rlks

using namespace rlks;

extern "C" {

int rlks_obs_filter_size(int D) {
  RLKS_REQUIRE(D >= 1 && D <= OF_MAX_D, RLKS_ERR_ARG, "rlks_obs_filter: 1 <= D <= 512 columns");
  return RLKS_OF_VECS + RLKS_OF_NVEC * D;
}

int rlks_obs_filter_init(double* state, int D, void* stream) {
  RLKS_REQUIRE(state && ((uintptr_t)state & 7) == 0, RLKS_ERR_ARG, "rlks_obs_filter_init: null or misaligned state");
  if (int n = rlks_obs_filter_size(D); n < 0) return n;
  hipLaunchKernelGGL(k_obs_filter_init, dim3(1), dim3(OF_BLOCK), 0, (hipStream_t)stream, state, D);
  RLKS_LAUNCHED();
  return RLKS_OK;
}

int rlks_obs_filter_apply(const double* state, const float* x, float* y, int64_t rows, int D, void* stream) {
  RLKS_REQUIRE(state && x && y && rows >= 0, RLKS_ERR_ARG, "rlks_obs_filter_apply: null argument or rows < 0");
  RLKS_REQUIRE((((uintptr_t)x | (uintptr_t)y) & 3) == 0 && ((uintptr_t)state & 7) == 0, RLKS_ERR_ARG,
               "rlks_obs_filter_apply: misaligned argument");
  if (int n = rlks_obs_filter_size(D); n < 0) return n;
  if (rows == 0) return RLKS_OK;
  const long long total = (long long)rows * D;
  const bool vec = (((uintptr_t)x | (uintptr_t)y) & 15) == 0;
  const long long items = vec ? (total + 3) / 4 : total;
  const long long nbl = (items + OF_BLOCK - 1) / OF_BLOCK;
  const int nb = (int)(nbl > OF_APPLY_MAX_BLOCKS ? OF_APPLY_MAX_BLOCKS : nbl);
  hipStream_t s = (hipStream_t)stream;
  if (vec) hipLaunchKernelGGL((k_obs_filter_apply<true>), dim3(nb), dim3(OF_BLOCK), 0, s, state, x, y, total, D);
  else hipLaunchKernelGGL((k_obs_filter_apply<false>), dim3(nb), dim3(OF_BLOCK), 0, s, state, x, y, total, D);
  RLKS_LAUNCHED();
  return RLKS_OK;
}

int rlks_obs_filter_workspace_bytes(int64_t rows, int D, int64_t* bytes) {
  RLKS_REQUIRE(bytes && rows >= 0, RLKS_ERR_ARG, "rlks_obs_filter_workspace_bytes: null argument or rows < 0");
  if (int n = rlks_obs_filter_size(D); n < 0) return n;
  *bytes = (int64_t)of_part_blocks(rows, D) * 2 * D * (int64_t)sizeof(double);
  return RLKS_OK;
}

int rlks_obs_filter_stats(const double* state, const float* x, int64_t rows, int D, double* record, void* workspace,
                          int64_t ws_bytes, void* stream) {
  RLKS_REQUIRE(state && x && record && workspace && rows >= 0, RLKS_ERR_ARG,
               "rlks_obs_filter_stats: null argument or rows < 0");
  if (int n = rlks_obs_filter_size(D); n < 0) return n;
  const int nb = of_part_blocks(rows, D);
  RLKS_REQUIRE((((uintptr_t)workspace | (uintptr_t)record | (uintptr_t)state) & 7) == 0 && ((uintptr_t)x & 3) == 0 &&
                   ws_bytes >= (int64_t)nb * 2 * D * (int64_t)sizeof(double),
               RLKS_ERR_ARG, "rlks_obs_filter_stats: workspace too small or misaligned argument");
  hipStream_t s = (hipStream_t)stream;
  double* part = (double*)workspace;
  hipLaunchKernelGGL(k_obs_filter_part, dim3(nb), dim3(OF_BLOCK), 0, s, state, x, (long long)rows, D, part);
  RLKS_LAUNCHED();
  hipLaunchKernelGGL(k_obs_filter_final, dim3(cdiv(2 * D, OF_FIN_SLOTS)), dim3(OF_BLOCK), 0, s, part, nb, 2 * D,
                     (long long)rows, record);
  RLKS_LAUNCHED();
  return RLKS_OK;
}

int rlks_obs_filter_merge(double* state, const double* record, int D, void* stream) {
  RLKS_REQUIRE(state && record && (((uintptr_t)state | (uintptr_t)record) & 7) == 0, RLKS_ERR_ARG,
               "rlks_obs_filter_merge: null or misaligned argument");
  if (int n = rlks_obs_filter_size(D); n < 0) return n;
  hipLaunchKernelGGL(k_obs_filter_merge, dim3(1), dim3(OF_BLOCK), 0, (hipStream_t)stream, state, record, D);
  RLKS_LAUNCHED();
  return RLKS_OK;
}

}  // extern "C"
