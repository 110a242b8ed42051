// ope.hip — off-policy evaluation of logged decisions: the target policy's logp of the logged
// actions (rlks_ope_logp) and RLlib's ImportanceSampling / WeightedImportanceSampling estimators over a
// time-major [T][N] decision log (rlks_ope_estimate); include/rlks.h states the arithmetic.
//
// The estimate is a segmented scan over time per lane (L_k and g_k are running values of a segment) with one
// cross-lane sum per step index k: S_k adds p_k over segments that sit at step k at different times t in
// different lanes.  Order (the same bits on every call, whichever workgroup finishes first):
//   k_ope_columns  thread n walks its lane and adds p_k into W[k][n], its own column, in program order; rows
//                  the lane has not reached yet are written, not added to, and reached[n] counts them, so the
//                  workspace needs no clearing and nothing left in it is ever read;
//   k_ope_rows     workgroup k sums row k over the lanes that reached it: thread i its lanes i, i + 256, .. in
//                  that order, lanes by xor butterflies, waves in wave order;
//   k_ope_values   the walk again, now with w_k; per lane the record's sums in segment order, then the
//                  workgroup's lanes as above: one partial record per workgroup;
//   k_ope_final    the partial records: thread i records i, i + 256, .., then as above.
// [t][n] rows are read across lanes (coalesced); no floating-point atomics, no atomics at all.  The file is
// built without FMA contraction: every operation rounds on its own, as tests/ope_ref.py restates it.
#include <hip/hip_runtime.h>

#include "env_device.h"

namespace rlks {

constexpr int OPE_BLOCK = 256;
constexpr int OPE_WAVES = OPE_BLOCK / 64;

struct OpeArgs {
  const float* lnew;
  const float* lold;
  const float* rew;
  const uint8_t* dones;
  int T, N;
  double gamma;
  int drop;
};

// one past the last step of lane n that lies in a counted segment: T, or with drop_truncated one past the
// lane's last done
__device__ __forceinline__ int ope_t_end(const OpeArgs& a, int n) {
  int t_end = a.T;
  if (a.drop)
    while (t_end > 0 && !a.dones[(size_t)(t_end - 1) * a.N + n]) --t_end;
  return t_end;
}

// index of step t of lane n
__device__ __forceinline__ size_t ope_at(const OpeArgs& a, int t, int n) {
  size_t i = (size_t)t * a.N + n;
  if (!dcheck(t >= 0 && t < a.T && n < a.N, DC_OPE_STEP, (long long)i)) i = (size_t)n;
  return i;
}

// L_k = L_{k-1} + lr and p_k = exp(min(L_k, LMAX)); both walks call this one function
__device__ __forceinline__ double ope_ratio(double& L, float ln, float lo, bool& clamped) {
  const double lr = (double)ln - (double)lo;
  L = L + lr;
  clamped = L > RLKS_OPE_LMAX;
  return exp(fmin(L, RLKS_OPE_LMAX));
}

__global__ __launch_bounds__(OPE_BLOCK) void k_ope_columns(OpeArgs a, double* __restrict__ W, uint32_t* __restrict__ Cn,
                                                           int32_t* __restrict__ reached) {
  const int n = blockIdx.x * OPE_BLOCK + threadIdx.x;
  if (n >= a.N) return;
  const int t_end = ope_t_end(a, n);
  int k = 0, hi = 0;  // rows [0, hi) of this column hold sums of this call
  double L = 0.0;
  for (int t = 0; t < t_end; ++t) {
    const size_t i = ope_at(a, t, n);
    bool cl;
    const double p = ope_ratio(L, a.lnew[i], a.lold[i], cl);
    size_t c = (size_t)k * a.N + n;
    if (!dcheck(k <= t, DC_OPE_COL, (long long)c)) c = i;
    if (k < hi) {
      W[c] = W[c] + p;
      Cn[c] = Cn[c] + 1u;
    } else {
      W[c] = p;
      Cn[c] = 1u;
      hi = k + 1;
    }
    if (a.dones[i]) {
      k = 0;
      L = 0.0;
    } else {
      k += 1;
    }
  }
  reached[n] = hi;
}

__global__ __launch_bounds__(OPE_BLOCK) void k_ope_rows(const double* __restrict__ W, const uint32_t* __restrict__ Cn,
                                                        const int32_t* __restrict__ reached, int T, int N,
                                                        double* __restrict__ srow, double* __restrict__ wrow) {
  __shared__ double sh_s[OPE_WAVES];
  __shared__ unsigned long long sh_c[OPE_WAVES];
  int k = blockIdx.x;
  if (!dcheck(k < T, DC_OPE_ROW, k)) k = T - 1;
  double s = 0.0;
  unsigned long long c = 0ull;
  for (int n = threadIdx.x; n < N; n += OPE_BLOCK)
    if (k < reached[n]) {
      const size_t i = (size_t)k * N + n;
      s = s + W[i];
      c += Cn[i];
    }
  s = wave_sum(s);
  c = wave_sum_u64(c);
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  if (lane == 0) {
    sh_s[wave] = s;
    sh_c[wave] = c;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    double S = sh_s[0];
    unsigned long long cnt = sh_c[0];
    for (int w = 1; w < OPE_WAVES; ++w) {
      S = S + sh_s[w];
      cnt += sh_c[w];
    }
    srow[k] = S;
    wrow[k] = cnt ? S / (double)cnt : 0.0;  // a row no counted segment reaches is never read
  }
}

// slots of the partial records: the record's own
__device__ __forceinline__ double ope_merge(int slot, double a, double b) {
  return slot == RLKS_OPE_MAX_LEN ? fmax(a, b) : a + b;
}
__device__ __forceinline__ double ope_wave_merge(int slot, double v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = ope_merge(slot, v, __shfl_xor(v, o, 64));
  return v;
}

__global__ __launch_bounds__(OPE_BLOCK) void k_ope_values(OpeArgs a, const double* __restrict__ srow,
                                                          const double* __restrict__ wrow, double* __restrict__ ep_out,
                                                          double* __restrict__ part) {
  __shared__ double sh[OPE_WAVES][RLKS_OPE_SIZE];
  const int n = blockIdx.x * OPE_BLOCK + threadIdx.x;
  double acc[RLKS_OPE_SIZE];
#pragma unroll
  for (int s = 0; s < RLKS_OPE_SIZE; ++s) acc[s] = 0.0;
  unsigned long long episodes = 0ull, steps = 0ull, clamped = 0ull, bad = 0ull;
  int maxlen = 0;
  if (n < a.N) {
    const int t_end = ope_t_end(a, n);
    int k = 0;
    double L = 0.0, g = 1.0, vb = 0.0, vis = 0.0, vw = 0.0;
    for (int t = 0; t < t_end; ++t) {
      const size_t i = ope_at(a, t, n);
      const float ln = a.lnew[i], lo = a.lold[i];
      const bool done = a.dones[i] != 0;
      bad += (__builtin_isfinite(ln) && __builtin_isfinite(lo)) ? 0ull : 1ull;
      bool cl;
      const double p = ope_ratio(L, ln, lo, cl);
      clamped += cl ? 1ull : 0ull;
      const double x = g * (double)a.rew[i];
      int kr = k;
      if (!dcheck(k <= t, DC_OPE_ROW, k)) kr = t;
      const double S = srow[kr], w = wrow[kr];
      vb = vb + x;
      vis = vis + p * x;
      vw = vw + (S == 0.0 ? 0.0 : (p / w) * x);
      if (done || t == t_end - 1) {
        if (ep_out) {
          size_t e = i;
          if (!dcheck(e < (size_t)a.T * a.N, DC_OPE_EP, (long long)e)) e = (size_t)n;
          double* o = ep_out + 4 * e;
          o[0] = vb;
          o[1] = vis;
          o[2] = vw;
          o[3] = p;
        }
        acc[RLKS_OPE_VB_SUM] = acc[RLKS_OPE_VB_SUM] + vb;
        acc[RLKS_OPE_VB_SQ] = acc[RLKS_OPE_VB_SQ] + vb * vb;
        acc[RLKS_OPE_VIS_SUM] = acc[RLKS_OPE_VIS_SUM] + vis;
        acc[RLKS_OPE_VIS_SQ] = acc[RLKS_OPE_VIS_SQ] + vis * vis;
        acc[RLKS_OPE_VWIS_SUM] = acc[RLKS_OPE_VWIS_SUM] + vw;
        acc[RLKS_OPE_VWIS_SQ] = acc[RLKS_OPE_VWIS_SQ] + vw * vw;
        acc[RLKS_OPE_PEND_SUM] = acc[RLKS_OPE_PEND_SUM] + p;
        acc[RLKS_OPE_PEND_SQ] = acc[RLKS_OPE_PEND_SQ] + p * p;
        episodes += 1ull;
        steps += (unsigned long long)(k + 1);
        maxlen = max(maxlen, k + 1);
        k = 0;
        L = 0.0;
        g = 1.0;
        vb = vis = vw = 0.0;
      } else {
        k += 1;
        g = g * a.gamma;
      }
    }
  }
  // counts are exact in u64 and, below 2^53, as doubles
  acc[RLKS_OPE_EPISODES] = (double)wave_sum_u64(episodes);
  acc[RLKS_OPE_STEPS] = (double)wave_sum_u64(steps);
  acc[RLKS_OPE_CLAMPED] = (double)wave_sum_u64(clamped);
  acc[RLKS_OPE_BAD_ROWS] = (double)wave_sum_u64(bad);
  acc[RLKS_OPE_MAX_LEN] = ope_wave_merge(RLKS_OPE_MAX_LEN, (double)maxlen);
#pragma unroll
  for (int s = RLKS_OPE_VB_SUM; s < RLKS_OPE_SIZE; ++s) acc[s] = wave_sum(acc[s]);
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  if (lane == 0) {
#pragma unroll
    for (int s = 0; s < RLKS_OPE_SIZE; ++s) sh[wave][s] = acc[s];
  }
  __syncthreads();
  if (threadIdx.x < RLKS_OPE_SIZE) {
    const int s = threadIdx.x;
    double v = sh[0][s];
    for (int w = 1; w < OPE_WAVES; ++w) v = ope_merge(s, v, sh[w][s]);
    part[(size_t)blockIdx.x * RLKS_OPE_SIZE + s] = v;
  }
}

__global__ __launch_bounds__(OPE_BLOCK) void k_ope_final(const double* __restrict__ part, int nb,
                                                         double* __restrict__ record) {
  __shared__ double sh[RLKS_OPE_SIZE][OPE_WAVES];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  for (int s = 0; s < RLKS_OPE_SIZE; ++s) {
    double v = 0.0;
    for (int b = threadIdx.x; b < nb; b += OPE_BLOCK) {
      int br = b;
      if (!dcheck(b < nb, DC_OPE_PART, b)) br = 0;
      v = ope_merge(s, v, part[(size_t)br * RLKS_OPE_SIZE + s]);
    }
    v = ope_wave_merge(s, v);
    if (lane == 0) sh[s][wave] = v;
  }
  __syncthreads();
  if (threadIdx.x < RLKS_OPE_SIZE) {
    const int s = threadIdx.x;
    double v = sh[s][0];
    for (int w = 1; w < OPE_WAVES; ++w) v = ope_merge(s, v, sh[s][w]);
    record[s] = v;
  }
}

// one thread per row; a row's A logits are contiguous
__global__ __launch_bounds__(OPE_BLOCK) void k_ope_logp(const float* __restrict__ logits, const int32_t* __restrict__ actions,
                                                        const uint64_t* __restrict__ mask, long long rows, int A,
                                                        float* __restrict__ logp) {
  long long i = (long long)blockIdx.x * OPE_BLOCK + threadIdx.x;
  if (i >= rows) return;
  if (!dcheck(i >= 0, DC_OPE_LOGIT, i)) i = 0;
  logp[i] = categorical_logp(logits + (size_t)i * A, A, mask != nullptr, mask ? mask[i] : 0ull, actions[i]);
}

struct OpeWs {
  double* W;
  uint32_t* Cn;
  int32_t* reached;
  double* srow;
  double* wrow;
  double* part;
  int64_t bytes;
};

static OpeWs ope_layout(void* base, int T, int N) {
  WsCursor c{(char*)base};
  const int64_t tn = (int64_t)T * N;
  OpeWs w;
  w.W = c.take<double>(tn * (int64_t)sizeof(double));
  w.Cn = c.take<uint32_t>(tn * (int64_t)sizeof(uint32_t));
  w.reached = c.take<int32_t>((int64_t)N * (int64_t)sizeof(int32_t));
  w.srow = c.take<double>((int64_t)T * (int64_t)sizeof(double));
  w.wrow = c.take<double>((int64_t)T * (int64_t)sizeof(double));
  w.part = c.take<double>((int64_t)cdiv(N, OPE_BLOCK) * RLKS_OPE_SIZE * (int64_t)sizeof(double));
  w.bytes = c.o;
  return w;
}

}  // namespace rlks

using namespace rlks;

extern "C" {

int rlks_ope_logp(const float* logits, const int32_t* actions, const uint64_t* mask, int64_t rows, int A, float* logp_out,
                  void* stream) {
  RLKS_REQUIRE(logits && actions && logp_out && rows >= 0 && A >= 1, RLKS_ERR_ARG, "rlks_ope_logp: bad argument");
  RLKS_REQUIRE((((uintptr_t)logits | (uintptr_t)actions | (uintptr_t)logp_out) & 3) == 0 && ((uintptr_t)mask & 7) == 0,
               RLKS_ERR_ARG, "rlks_ope_logp: misaligned pointer");
  RLKS_REQUIRE(!mask || A <= 64, RLKS_ERR_UNSUPPORTED, "rlks_ope_logp: at most 64 actions with a mask (a 64-bit mask)");
  const int64_t blocks = (rows + OPE_BLOCK - 1) / OPE_BLOCK;
  RLKS_REQUIRE(blocks <= 0x7fffffffll, RLKS_ERR_UNSUPPORTED, "rlks_ope_logp: too many rows for one launch");
  if (rows == 0) return RLKS_OK;
  hipLaunchKernelGGL(k_ope_logp, dim3((unsigned)blocks), dim3(OPE_BLOCK), 0, (hipStream_t)stream, logits, actions, mask,
                     (long long)rows, A, logp_out);
  RLKS_LAUNCHED();
  return RLKS_OK;
}

int rlks_ope_workspace_bytes(int T, int N, int64_t* bytes) {
  RLKS_REQUIRE(bytes && T > 0 && N > 0, RLKS_ERR_ARG, "rlks_ope_workspace_bytes: bad argument");
  *bytes = ope_layout(nullptr, T, N).bytes;
  return RLKS_OK;
}

int rlks_ope_estimate(const float* logp_new, const float* logp_old, const float* rewards, const uint8_t* dones, int T,
                      int N, double gamma, int drop_truncated, double* record, double* ep_out, void* workspace,
                      int64_t workspace_bytes, void* stream) {
  RLKS_REQUIRE(logp_new && logp_old && rewards && dones && record && workspace, RLKS_ERR_ARG,
               "rlks_ope_estimate: null argument");
  RLKS_REQUIRE(T > 0 && N > 0, RLKS_ERR_ARG, "rlks_ope_estimate: T and N must be positive");
  RLKS_REQUIRE(gamma == gamma && gamma >= 0.0 && gamma <= 1.0, RLKS_ERR_ARG,
               "rlks_ope_estimate: gamma must be finite and in [0, 1]");
  RLKS_REQUIRE((((uintptr_t)logp_new | (uintptr_t)logp_old | (uintptr_t)rewards) & 3) == 0 &&
                   (((uintptr_t)record | (uintptr_t)ep_out | (uintptr_t)workspace) & 7) == 0,
               RLKS_ERR_ARG, "rlks_ope_estimate: misaligned pointer");
  const OpeWs w = ope_layout(workspace, T, N);
  RLKS_REQUIRE(workspace_bytes >= w.bytes, RLKS_ERR_ARG, "rlks_ope_estimate: workspace too small");
  const OpeArgs a{logp_new, logp_old, rewards, dones, T, N, gamma, drop_truncated ? 1 : 0};
  hipStream_t s = (hipStream_t)stream;
  const int nb = (int)cdiv(N, OPE_BLOCK);
  hipLaunchKernelGGL(k_ope_columns, dim3(nb), dim3(OPE_BLOCK), 0, s, a, w.W, w.Cn, w.reached);
  RLKS_LAUNCHED();
  hipLaunchKernelGGL(k_ope_rows, dim3(T), dim3(OPE_BLOCK), 0, s, w.W, w.Cn, w.reached, T, N, w.srow, w.wrow);
  RLKS_LAUNCHED();
  hipLaunchKernelGGL(k_ope_values, dim3(nb), dim3(OPE_BLOCK), 0, s, a, w.srow, w.wrow, ep_out, w.part);
  RLKS_LAUNCHED();
  hipLaunchKernelGGL(k_ope_final, dim3(1), dim3(OPE_BLOCK), 0, s, w.part, nb, record);
  RLKS_LAUNCHED();
  return RLKS_OK;
}

}  // extern "C"
