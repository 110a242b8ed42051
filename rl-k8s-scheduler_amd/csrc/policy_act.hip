// policy_act.hip — serving: n raw observations to decisions in one launch.
//
//   rlks_policy_act   k_policy_act: (filter) -> policy MLP -> (mask) -> argmax / Categorical draw -> probs,
//                     and the value net on the same tile when values are asked for
//   rlks_host_alloc / rlks_host_free   pinned, device-visible host memory for the caller's staging block
//
// Grid (ceil(n / 16), nets), 256 threads (4 waves).  blockIdx.y = 0 is the policy net, 1 the value net.
// Per 16-row tile:
//   load     X[16][D] into LDS, through of_one() (obs_filter.h) with a filter state; rows past n are zeros
//   layer 1  thread j owns hidden unit j: z[m] = b1[j], then z[m] = fmaf(X[m][d], W1[j][d], z[m]) for
//            d = 0 .. D - 1 (its W1 row read once), H1[m][j] = fast_tanh(z[m]) into LDS
//   layer 2  Z2 = H1 W2^T on v_mfma_f32_16x16x4_f32 (exact fp32).  Wave w owns the column tiles 4 w .. 4 w + 3.
//            k-block kb = 0 .. 15 covers k = 16 kb .. 16 kb + 15; lane (i = l & 15, g = l >> 4) holds
//            H1[i][16 kb + 4 g .. + 3] (one 16-byte LDS read) and, per column tile, W2[col][16 kb + 4 g .. + 3]
//            (one 16-byte global load, [out][in] row-major as stored); MFMA step s = 0 .. 3 takes component s of
//            both, so slot g of step s carries k = 16 kb + 4 g + s on the A and the B side alike.  The B
//            fragments of block kb + 1 are loaded ahead of block kb's 16 MFMAs.  Every output therefore adds
//            its 256 products in one fixed order: kb ascending, s ascending, the instruction's four slots.
//            H2 = fast_tanh(Z2 + b2) into a second LDS array (H1 is still being read by other waves)
//   head     out[m][a] = ((p0 + p1) + (p2 + p3)) + b3[a], p_q = the fmaf chain from 0 over k = 64 q .. 64 q + 63
//            ascending; thread (m = t & 15, q = (t >> 4) & 3) computes p_q for a = t >> 6, + 4, ...
//   rows     thread m < 16 with a live row: policy tile: the optional mask, the shared draw (categorical /
//            categorical_masked, env_device.h) with counter action_ctr(sampler_id, row, call) under key = seed,
//            then the softmax of the row as drawn from; value tile: values[row]
// Everything written for a row depends on that row, the parameters, the filter state, its mask word and
// (exploring) seed, call and the row's index alone: not on n, on the row's place in its tile or on other rows
// (an MFMA computes every output row from that row of A alone; the dead rows are zeros and are never stored).
// No atomics.  Plain C++ stores.
//
// Contraction: the file is built with the library's default flags, so fast_tanh() here is the instruction
// sequence k_fwd_head runs.  Layer 1 and the head are written as explicit fmaf; the draw and the softmax
// carry their own contract(off) scope; of_one() is a subtract and a multiply, which no FMA can fuse.
#include <hip/hip_runtime.h>

#include "mlp_common.h"
#include "obs_filter.h"

namespace rlks {

using f32x4 = __attribute__((ext_vector_type(4))) float;

constexpr int ACT_ROWS = 16;      // rows per tile: the MFMA's M
constexpr int ACT_BLOCK = 256;    // = HID: one thread per hidden unit in layer 1
constexpr int ACT_DMAX = 192;     // observation columns (sX: 12 KB)
constexpr int ACT_AMAX = 64;      // actions: the mask word's bits
constexpr int ACT_HS = HID + 4;   // LDS row stride of H1 / H2: 16-byte aligned rows, rows 4 banks apart
constexpr int ACT_LS = ACT_AMAX + 1;  // LDS row stride of the finished logits rows (one thread per row)
static_assert(ACT_BLOCK == HID, "layer 1 maps one thread to one hidden unit");
static_assert(ACT_ROWS * ACT_AMAX * 4 <= ACT_ROWS * ACT_HS, "the head's partials reuse H1's array");
static_assert(ACT_ROWS * ACT_LS <= ACT_ROWS * ACT_DMAX, "the logits rows reuse X's array");

struct ActArgs {
  NetPtrs P[2];          // policy, value
  const double* fstate;  // filter state or NULL
  const float* obs;      // [n][D] raw
  const uint64_t* mask;  // [n] or NULL
  int n, D, A, explore;
  uint32_t k0, k1, sampler, call;
  int32_t* actions;
  float *logp, *logits, *probs, *values;
};

// softmax of the row l[0..A) into p, every operation rounded on its own (as the draw's sums are)
__device__ __forceinline__ void softmax_row(const float* l, int A, float* __restrict__ p) {
#pragma clang fp contract(off)
  float mx = l[0];
  for (int a = 1; a < A; ++a)
    if (l[a] > mx) mx = l[a];
  float s = 0.f;
  for (int a = 0; a < A; ++a) s += __builtin_expf(l[a] - mx);
  for (int a = 0; a < A; ++a) p[a] = __fdiv_rn(__builtin_expf(l[a] - mx), s);
}

__device__ __forceinline__ float comp(const float4& v, int s) { return s == 0 ? v.x : s == 1 ? v.y : s == 2 ? v.z : v.w; }

__global__ __launch_bounds__(ACT_BLOCK) void k_policy_act(ActArgs g) {
  __shared__ __attribute__((aligned(16))) float sX[ACT_ROWS * ACT_DMAX];  // X, later the logits rows
  __shared__ __attribute__((aligned(16))) float sH1[ACT_ROWS * ACT_HS];   // H1, later the head's partials
  __shared__ __attribute__((aligned(16))) float sH2[ACT_ROWS * ACT_HS];
  float* sPart = sH1;  // [16][A][4]
  float* sOut = sX;    // [16][ACT_LS]

  const int net = blockIdx.y;
  const NetPtrs P = net ? g.P[1] : g.P[0];
  const int tid = threadIdx.x, l = tid & 63, w = tid >> 6;
  const int li = l & 15, lg = l >> 4;
  const int row0 = blockIdx.x * ACT_ROWS;
  const int D = g.D;

  // this lane's W2 fragments: column 64 w + 16 t + li (tile t), floats 16 kb + 4 lg .. + 3 of its row
  const float* wfrag = P.w2 + (size_t)(64 * w + li) * HID + 4 * lg;
  dcheck(64 * w + 48 + li < HID && 4 * lg + 16 * 15 + 3 < HID, DC_ACT_W2, 64 * w + li);
  float4 bc[4], bn[4];
#pragma unroll
  for (int t = 0; t < 4; ++t) bc[t] = *reinterpret_cast<const float4*>(wfrag + (size_t)t * 16 * HID);

  // ---- load (and filter) the tile's rows
  for (int e = tid; e < ACT_ROWS * D; e += ACT_BLOCK) {
    const int m = e / D, d = e - m * D;
    const int row = row0 + m;
    float x = 0.f;
    if (row < g.n) {
      x = g.obs[(size_t)row * D + d];
      if (g.fstate)
        x = of_one(x, g.fstate + RLKS_OF_VECS + RLKS_OF_MEAN * D, g.fstate + RLKS_OF_VECS + RLKS_OF_INV * D, d, D);
    }
    sX[m * D + d] = x;  // m * D + d = e < 16 D <= 16 ACT_DMAX
  }
  __syncthreads();

  // ---- layer 1: hidden unit tid
  {
    float z[ACT_ROWS];
    const float b = P.b1[tid];
#pragma unroll
    for (int m = 0; m < ACT_ROWS; ++m) z[m] = b;
    const float* wr = P.w1 + (size_t)tid * D;
#pragma unroll 4
    for (int d = 0; d < D; ++d) {
      const float wv = wr[d];
#pragma unroll
      for (int m = 0; m < ACT_ROWS; ++m) z[m] = fmaf(sX[m * D + d], wv, z[m]);
    }
#pragma unroll
    for (int m = 0; m < ACT_ROWS; ++m) sH1[m * ACT_HS + tid] = fast_tanh(z[m]);
  }
  __syncthreads();

  // ---- layer 2: 4 column tiles per wave, 16 k-blocks of 4 MFMA steps
  f32x4 acc[4];
#pragma unroll
  for (int t = 0; t < 4; ++t) acc[t] = f32x4{0.f, 0.f, 0.f, 0.f};
  const float* afrag = sH1 + li * ACT_HS + 4 * lg;
#pragma unroll
  for (int kb = 0; kb < HID / 16; ++kb) {
    if (kb + 1 < HID / 16) {
#pragma unroll
      for (int t = 0; t < 4; ++t)
        bn[t] = *reinterpret_cast<const float4*>(wfrag + (size_t)t * 16 * HID + 16 * (kb + 1));
    }
    const float4 a = *reinterpret_cast<const float4*>(afrag + 16 * kb);
#pragma unroll
    for (int s = 0; s < 4; ++s)
#pragma unroll
      for (int t = 0; t < 4; ++t)
        acc[t] = __builtin_amdgcn_mfma_f32_16x16x4f32(comp(a, s), comp(bc[t], s), acc[t], 0, 0, 0);
#pragma unroll
    for (int t = 0; t < 4; ++t) bc[t] = bn[t];
  }
  // accumulator register r of lane l: row 4 (l >> 4) + r, column l & 15 of the tile
#pragma unroll
  for (int t = 0; t < 4; ++t) {
    const int col = 64 * w + 16 * t + li;
    const float bb = P.b2[col];
#pragma unroll
    for (int r = 0; r < 4; ++r) sH2[(4 * lg + r) * ACT_HS + col] = fast_tanh(acc[t][r] + bb);
  }
  __syncthreads();  // H2 complete; every wave is done reading H1, whose array the partials take over

  // ---- head: quarter sums of the 256-long dot products
  const int A = net ? 1 : g.A;
  {
    const int m = tid & 15, q = (tid >> 4) & 3;
    const float* hr = sH2 + m * ACT_HS + 64 * q;
    for (int a = tid >> 6; a < A; a += 4) {
      const float* wr = P.w3 + (size_t)a * HID + 64 * q;
      float s = 0.f;
#pragma unroll
      for (int k = 0; k < 64; k += 4) {
        const float4 h = *reinterpret_cast<const float4*>(hr + k);
        const float4 wv = *reinterpret_cast<const float4*>(wr + k);
        s = fmaf(h.x, wv.x, s);
        s = fmaf(h.y, wv.y, s);
        s = fmaf(h.z, wv.z, s);
        s = fmaf(h.w, wv.w, s);
      }
      int slot = (m * A + a) * 4 + q;
      if (!dcheck(slot < ACT_ROWS * ACT_AMAX * 4 && a < ACT_AMAX, DC_ACT_HEAD, a)) slot = 0;
      sPart[slot] = s;
    }
  }
  __syncthreads();

  // ---- one thread per live row
  if (tid >= ACT_ROWS) return;
  const int row = row0 + tid;
  if (row >= g.n) return;
  dcheck(row >= 0 && row < g.n, DC_ACT_ROW, row);
  const float* part = sPart + (size_t)tid * A * 4;
  if (net) {
    g.values[row] = ((part[0] + part[1]) + (part[2] + part[3])) + P.b3[0];
    return;
  }
  dcheck(A >= 1 && A <= ACT_AMAX, DC_ACT_LDS, A);
  float* lrow = sOut + tid * ACT_LS;
  for (int a = 0; a < A; ++a) lrow[a] = ((part[4 * a] + part[4 * a + 1]) + (part[4 * a + 2] + part[4 * a + 3])) + P.b3[a];
  const u32x4 ctr = action_ctr(g.sampler, (uint32_t)row, g.call);
  float lp;
  int act;
  if (g.mask) act = categorical_masked(lrow, A, g.mask[row], g.explore != 0, ctr, g.k0, g.k1, lp);
  else act = categorical(lrow, A, g.explore != 0, ctr, g.k0, g.k1, lp);
  g.actions[row] = act;
  if (g.logp) g.logp[row] = lp;
  if (g.logits)
    for (int a = 0; a < A; ++a) g.logits[(size_t)row * A + a] = lrow[a];
  if (g.probs) softmax_row(lrow, A, g.probs + (size_t)row * A);
}

}  // namespace rlks

using namespace rlks;

extern "C" {

int rlks_policy_act(const rlks_mlp_desc* desc, const float* params_dev, const double* filter_state, const float* obs,
                    const uint64_t* mask, int n, int explore, unsigned long long seed, uint32_t sampler_id,
                    uint32_t call, int32_t* actions, float* logp, float* logits, float* probs, float* values,
                    void* stream) {
  RLKS_REQUIRE(desc && params_dev && obs && actions, RLKS_ERR_ARG,
               "rlks_policy_act: null desc, params, obs or actions");
  RLKS_REQUIRE(n >= 0, RLKS_ERR_ARG, "rlks_policy_act: n < 0");
  RLKS_REQUIRE(!mask || desc->n_actions <= ACT_AMAX, RLKS_ERR_UNSUPPORTED,
               "rlks_policy_act: at most 64 actions with a mask (a 64-bit mask)");
  RLKS_REQUIRE(desc->hidden == HID && desc->obs_dim >= 1 && desc->obs_dim <= ACT_DMAX && desc->n_actions >= 1 &&
                   desc->n_actions <= ACT_AMAX,
               RLKS_ERR_UNSUPPORTED, "rlks_policy_act: built for hidden 256, 1 <= obs_dim <= 192, 1 <= n_actions <= 64");
  RLKS_REQUIRE(((uintptr_t)params_dev & 15) == 0 &&
                   (((uintptr_t)obs | (uintptr_t)actions | (uintptr_t)logp | (uintptr_t)logits | (uintptr_t)probs |
                     (uintptr_t)values) & 3) == 0 &&
                   (((uintptr_t)filter_state | (uintptr_t)mask) & 7) == 0,
               RLKS_ERR_ARG, "rlks_policy_act: misaligned argument (params 16, floats 4, filter state and mask 8 bytes)");
  if (n == 0) return RLKS_OK;
  const Layout L = make_layout(desc->obs_dim, desc->hidden, desc->n_actions);
  ActArgs a;
  a.P[0] = net_ptrs_host(params_dev, L, 0);
  a.P[1] = net_ptrs_host(params_dev, L, 1);
  a.fstate = filter_state;
  a.obs = obs;
  a.mask = mask;
  a.n = n;
  a.D = desc->obs_dim;
  a.A = desc->n_actions;
  a.explore = explore ? 1 : 0;
  a.k0 = (uint32_t)seed;
  a.k1 = (uint32_t)(seed >> 32);
  a.sampler = sampler_id;
  a.call = call;
  a.actions = actions;
  a.logp = logp;
  a.logits = logits;
  a.probs = probs;
  a.values = values;
  hipLaunchKernelGGL(k_policy_act, dim3(cdiv(n, ACT_ROWS), values ? 2 : 1), dim3(ACT_BLOCK), 0, (hipStream_t)stream, a);
  RLKS_LAUNCHED();
  return RLKS_OK;
}

int rlks_host_alloc(size_t bytes, void** host_ptr, void** dev_ptr) {
  RLKS_REQUIRE(bytes > 0 && host_ptr && dev_ptr, RLKS_ERR_ARG, "rlks_host_alloc: zero bytes or null argument");
  void *h = nullptr, *d = nullptr;
  RLKS_HIP(hipHostMalloc(&h, bytes, hipHostMallocMapped));
  if (hipError_t e = hipHostGetDevicePointer(&d, h, 0); e != hipSuccess) {
    (void)hipHostFree(h);
    return fail(RLKS_ERR_HIP, std::string("hipHostGetDevicePointer: ") + hipGetErrorString(e));
  }
  *host_ptr = h;
  *dev_ptr = d;
  return RLKS_OK;
}

int rlks_host_free(void* host_ptr) {
  if (!host_ptr) return RLKS_OK;
  RLKS_HIP(hipHostFree(host_ptr));
  return RLKS_OK;
}

}  // extern "C"
