// reduce.h — the gradient reduce as device code: the fixed-order f64 sum of partials with the optional
// fused Adam, global-norm partials and clip (reduce_block<MODE>), and its host-side task list (Reducer).
// Header only: reduce_block is inlined into the kernels of ppo.hip that combine it with a gather.
#pragma once

#include "sgd_sf16.h"

namespace rlks {

// ----------------------------------------------------------------------------- reduce
// out[i] = sum_p part[p * pstride + i] (i < len, p < P) in a fixed order with f64 accumulation.
// A block = 256 threads = OPB output vectors x G partial-groups; a vector is 4 consecutive outputs
// (one 16-byte load per partial) when the task's length and stride allow it, else 1.  G is chosen
// per task so that every thread sums about 16 partials.
struct RedTask {
  const float* part;
  float* out;        // float output ...
  double* out64;     // ... or double output (stats)
  int64_t pstride;
  int P, len, G, V;
  int blk0;
  int mslot;         // fused Adam: -1, or the max |w| slot (net * 2 + 0: W2, + 1: W1a) of the output
  int mbase;         // first entry of this task's blocks in the slot
  int kq;            // 0: output vector iv at element 4 iv; 1 (k_sf_dw2r's [k / 4][n][4] partials of a
                     // [256][256] weight): at n * 256 + 4 (iv >> 8), n = iv & 255
};
constexpr int MAX_TASKS = 20;
// torch.optim.Adam (single-tensor path) on element i: exp_avg.lerp_(g, 1-b1); exp_avg_sq =
// b2*v + (1-b2)*g*g; p -= (lr / (1 - b1^t)) * m / (sqrt(v) / sqrt(1 - b2^t) + eps).  Shared by
// k_adam and the fused reduce so that both paths compute the same bits; every rounding is spelled out
// (__fmul_rn / __fadd_rn / fmaf) so that no inlining context contracts them differently (an -fno-slp-vectorize
// build fused m + w1 (g - m) into an fma in one kernel and not in the other, profiles/r06_noslp).
struct AdamCo {
  float w1, b2, omb2, step_size, bc2_sqrt, eps;
};
__device__ __forceinline__ float adam_elem(float* __restrict__ p, float* __restrict__ m, float* __restrict__ v,
                                           int64_t i, float gi, const AdamCo& c) {
  const float mi = __fadd_rn(m[i], __fmul_rn(c.w1, __fsub_rn(gi, m[i])));
  const float vi = fmaf(gi, __fmul_rn(c.omb2, gi), __fmul_rn(c.b2, v[i]));
  m[i] = mi;
  v[i] = vi;
  const float denom = __fadd_rn(__fdiv_rn(sqrtf(vi), c.bc2_sqrt), c.eps);
  const float pn = fmaf(-c.step_size, __fdiv_rn(mi, denom), p[i]);
  p[i] = pn;
  return pn;
}

struct RedArgs {
  RedTask t[MAX_TASKS];
  int ntasks;
  double* stats;     // optional: stats[4] = rows, stats[5..7] = 0 (the sums come from tasks)
  double rows;
  // fused Adam (p != null): every parameter-gradient output element is also applied to its
  // parameter (index = out - grad), and the new |w| maxima of W2 / W1a go to the split's slots
  float *p, *m, *v;
  const float* grad;
  AdamCo co;
  float* slot[4];     // [net * 2 + 0] W2, [net * 2 + 1] W1a: per-block max entries (task mbase + block)
  unsigned* tag[2];   // set to tag_val: the slots hold the maxima of Adam step tag_val
  unsigned tag_val;
};

// ----------------------------------------------------------------------------- global-norm clipping
// RLlib's torch policy clips by global norm (ray/rllib/utils/torch_utils.py apply_grad_clipping ->
// torch.nn.utils.clip_grad_norm_ over every parameter of the one optimizer): norm = sqrt(sum g^2),
// coef = min(1, grad_clip / (norm + 1e-6)), g <- g coef, then Adam on the clipped g.  RLlib and torch
// are third-party and absent here: the semantics are restated in tests/clip_ref.py.
//
// The sum of squares is an f64 sum in one fixed order that does not depend on how a kernel tiles the
// gradient: per tensor, the zero-padded binary tree over the output-vector index (neighbours first:
// x[i] + x[i ^ 1], then pairs of pairs, ...), then the tensors in task order.  A reduce block owns an
// aligned power-of-two run of vectors, so its partial is one node of that tree whatever its size
// (adding the +0.0 of a missing leaf is exact), and k_norm_finish continues the tree over the blocks.
// The gradient reduce of the fused step (many partials, small blocks) and the one-partial pass over an
// all-reduced gradient (1,024-element blocks) therefore give the same bits.  No atomics, no grid sync.
struct NrmArgs {
  double* part;       // RED_NRM / RED_NRM_ONLY: [reduce blocks] the block's sum of squares of its outputs
  const float* coef;  // RED_CLIP: the clip coefficient k_norm_finish left
};
enum RedMode {
  RED_PLAIN = 0,     // the reduce as it always was
  RED_NRM = 1,       // + one norm partial per block
  RED_NRM_ONLY = 2,  // one partial in place: norm partials only, nothing is written back
  RED_CLIP = 3       // one partial in place: g <- g coef, written back, then the fused Adam
};

// g coef as one rounded fp32 product (IEEE round to nearest).  The pragma keeps it one: with hipcc's
// default contraction the compiler would fold it into the Adam arithmetic that consumes it
// (g coef - m as one fma), and the clipped step would differ from Adam on the stored clipped gradient.
__device__ __forceinline__ float clip_mul(float g, float coef) {
#pragma clang fp contract(off)
  return g * coef;
}

__device__ __forceinline__ double tree64(double v) {
#pragma unroll
  for (int off = 1; off < 64; off <<= 1) v += __shfl_xor(v, off, 64);
  return v;
}
// the 256 threads' values summed as the binary tree over threadIdx.x (every thread gets the sum)
__device__ __forceinline__ double block_tree256(double v) {
  __shared__ double w[4];
  v = tree64(v);
  if ((threadIdx.x & 63) == 0) w[threadIdx.x >> 6] = v;
  __syncthreads();
  return (w[0] + w[1]) + (w[2] + w[3]);
}

template <int MODE>
__device__ __forceinline__ void reduce_block(const RedArgs& g, const int bx, const NrmArgs& c) {
  __shared__ double sh[4][256];
  int ti = 0;
  while (ti + 1 < g.ntasks && bx >= g.t[ti + 1].blk0) ++ti;
  const RedTask T = g.t[ti];
  const int opb = 256 / T.G;
  const int o = threadIdx.x % opb, grp = threadIdx.x / opb;
  const int iv = (bx - T.blk0) * opb + o;  // output vector
  double s[4] = {0.0, 0.0, 0.0, 0.0};
  // the partials of a thread RB loads at a time, summed in the same (increasing p) order: one
  // dependent load round trip per RB partials instead of per partial (c4 reduce + next gather
  // 17.5 -> 14.2-14.5 us at RB = 4 or 8, ~5.6 TB/s; profiles/r04c/reduce_batched_loads*.txt)
  constexpr int RB = 8;
  if (T.V == 4) {
    if (4 * iv < T.len) {
      // (kq 2, norm-only pass: the vector read where kq 1 writes it, so that a [256][256] weight's
      // vectors are numbered as in the gradient reduce and the norm's tree is the same)
      const float* base = T.part + ((MODE == RED_NRM_ONLY && T.kq == 2) ? (iv & 255) * 256 + 4 * (iv >> 8) : 4 * iv);
      int p = grp;
      for (; p + (RB - 1) * T.G < T.P; p += RB * T.G) {
        float4 v[RB];
#pragma unroll
        for (int q = 0; q < RB; ++q) v[q] = *reinterpret_cast<const float4*>(base + (int64_t)(p + q * T.G) * T.pstride);
#pragma unroll
        for (int q = 0; q < RB; ++q) {
          s[0] += (double)v[q].x; s[1] += (double)v[q].y; s[2] += (double)v[q].z; s[3] += (double)v[q].w;
        }
      }
      for (; p < T.P; p += T.G) {
        const float4 v = *reinterpret_cast<const float4*>(base + (int64_t)p * T.pstride);
        s[0] += (double)v.x; s[1] += (double)v.y; s[2] += (double)v.z; s[3] += (double)v.w;
      }
    }
  } else if (iv < T.len) {
    int p = grp;
    for (; p + (RB - 1) * T.G < T.P; p += RB * T.G) {
      float v[RB];
#pragma unroll
      for (int q = 0; q < RB; ++q) v[q] = T.part[(int64_t)(p + q * T.G) * T.pstride + iv];
#pragma unroll
      for (int q = 0; q < RB; ++q) s[0] += (double)v[q];
    }
    for (; p < T.P; p += T.G) s[0] += (double)T.part[(int64_t)p * T.pstride + iv];
  }
#pragma unroll
  for (int j = 0; j < 4; ++j) sh[j][threadIdx.x] = s[j];
  // groups summed pairwise in a fixed tree order: log2 G LDS steps (the G group values summed
  // serially by each output's thread: 35 us instead of 19 us per c4 reduce, a few threads per
  // block doing G dependent LDS reads each)
  for (int h = T.G / 2; h >= 1; h /= 2) {
    __syncthreads();
    if (grp < h)
#pragma unroll
      for (int j = 0; j < 4; ++j) sh[j][threadIdx.x] += sh[j][threadIdx.x + h * opb];
  }
  __syncthreads();
  float wmax = 0.f;
  double sq = 0.0;  // RED_NRM*: this thread's leaf of the norm's tree (its vector's sum of squares)
  if (grp == 0) {
    double t[4] = {0.0, 0.0, 0.0, 0.0};
    for (int j = 0; j < T.V; ++j) t[j] = sh[j][o];
    const int i0 = T.kq ? (iv & 255) * 256 + 4 * (iv >> 8) : T.V * iv;
    if (T.out64) {
      for (int j = 0; j < T.V && i0 + j < T.len; ++j) T.out64[i0 + j] = t[j];
    } else if (T.V == 4 && i0 + 3 < T.len) {
      float4 gv = make_float4((float)t[0], (float)t[1], (float)t[2], (float)t[3]);
      if (MODE == RED_NRM || MODE == RED_NRM_ONLY)
        sq = ((double)gv.x * (double)gv.x + (double)gv.y * (double)gv.y) +
             ((double)gv.z * (double)gv.z + (double)gv.w * (double)gv.w);
      if (MODE == RED_CLIP) {
        const float cf = *c.coef;
        gv = make_float4(clip_mul(gv.x, cf), clip_mul(gv.y, cf), clip_mul(gv.z, cf), clip_mul(gv.w, cf));
      }
      if (MODE != RED_NRM_ONLY) *reinterpret_cast<float4*>(T.out + i0) = gv;
      if (g.p) {  // Adam on the four parameters (16-byte aligned: tensors start on 64-float boundaries)
        const int64_t pi = (T.out - g.grad) + i0;
        float4 pv = *reinterpret_cast<const float4*>(g.p + pi), mv = *reinterpret_cast<const float4*>(g.m + pi),
               vv = *reinterpret_cast<const float4*>(g.v + pi);
        float* pp = &pv.x; float* mm = &mv.x; float* vq = &vv.x;
        const float gg[4] = {gv.x, gv.y, gv.z, gv.w};
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          wmax = fmaxf(wmax, fabsf(adam_elem(pp, mm, vq, j, gg[j], g.co)));
        }
        *reinterpret_cast<float4*>(g.p + pi) = pv;
        *reinterpret_cast<float4*>(g.m + pi) = mv;
        *reinterpret_cast<float4*>(g.v + pi) = vv;
      }
    } else {
      double e2[4] = {0.0, 0.0, 0.0, 0.0};
      for (int j = 0; j < T.V && i0 + j < T.len; ++j) {
        float gj = (float)t[j];
        if (MODE == RED_NRM || MODE == RED_NRM_ONLY) e2[j] = (double)gj * (double)gj;
        if (MODE == RED_CLIP) gj = clip_mul(gj, *c.coef);
        if (MODE != RED_NRM_ONLY) T.out[i0 + j] = gj;
        if (g.p) wmax = fmaxf(wmax, fabsf(adam_elem(g.p, g.m, g.v, (T.out - g.grad) + i0 + j, gj, g.co)));
      }
      if (MODE == RED_NRM || MODE == RED_NRM_ONLY) sq = (e2[0] + e2[1]) + (e2[2] + e2[3]);
    }
  }
  if (g.p && T.mslot >= 0) {  // block-uniform: this block's max |w_new| -> the slot
    __shared__ float smax[4];
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) wmax = fmaxf(wmax, __shfl_xor(wmax, off, 64));
    if ((threadIdx.x & 63) == 0) smax[threadIdx.x >> 6] = wmax;
    __syncthreads();
    if (threadIdx.x == 0)
      g.slot[T.mslot][T.mbase + bx - T.blk0] = fmaxf(fmaxf(smax[0], smax[1]), fmaxf(smax[2], smax[3]));
  }
  if (g.stats && bx == 0 && threadIdx.x == 0) {
    g.stats[RLKS_STAT_ROWS] = g.rows;
    g.stats[5] = g.stats[6] = g.stats[7] = 0.0;
  }
  if (g.p && bx == 0 && threadIdx.x == 0) {
    *g.tag[0] = g.tag_val;
    *g.tag[1] = g.tag_val;
  }
  if (MODE == RED_NRM || MODE == RED_NRM_ONLY) {  // grp 0 is threads [0, opb): the rest add +0.0
    const double bs = block_tree256(sq);
    if (threadIdx.x == 0) c.part[bx] = bs;
  }
}

// what k_norm_finish (ppo.hip) sums: per tensor k the nb[k] block partials from blk0[k] on, in chunks of
// 64 numbered through all tensors by c0[k]
constexpr int NRM_MAX_CHUNKS = 4096;  // level-0 sums held in LDS (64 partials each)
constexpr int NRM_MAX_NB = 65536;     // partials per tensor (64 x 64 x 16)
struct NrmPlan {
  int n;
  int blk0[RLKS_N_TENSORS], nb[RLKS_N_TENSORS], c0[RLKS_N_TENSORS + 1];
};

struct Reducer {
  RedArgs a{};
  int blocks = 0;
  int mnext[4] = {0, 0, 0, 0};  // next free entry per max slot
  int nblk[MAX_TASKS] = {};
  // the parameter-gradient tasks' blocks, for k_norm_finish (the stats tasks are not part of the norm)
  bool plan(NrmPlan& pl) const {
    pl = NrmPlan{};
    for (int i = 0; i < a.ntasks; ++i) {
      if (a.t[i].out64) continue;
      if (pl.n == RLKS_N_TENSORS || nblk[i] > NRM_MAX_NB) return false;
      pl.blk0[pl.n] = a.t[i].blk0;
      pl.nb[pl.n] = nblk[i];
      pl.c0[pl.n + 1] = pl.c0[pl.n] + (int)cdiv(nblk[i], 64);
      ++pl.n;
    }
    return pl.c0[pl.n] <= NRM_MAX_CHUNKS;
  }
  void add(const float* part, float* out, double* out64, int64_t pstride, int P, int len, int mslot = -1) {
    RedTask& t = a.t[a.ntasks++];
    t.mslot = mslot;
    t.mbase = 0;
    t.kq = 0;
    int G = 1;
    constexpr int PPT = 32;  // partials per thread (c4 reduce: 16 -> 19.0 us, 32 -> 19.0 us, 8 -> 23.9 us)
    while (G < 256 && G * PPT < P) G *= 2;
    const bool vec = len % 4 == 0 && pstride % 4 == 0 && ((uintptr_t)part & 15) == 0;
    t.part = part; t.out = out; t.out64 = out64; t.pstride = pstride; t.P = P; t.len = len; t.G = G;
    t.V = vec ? 4 : 1;
    t.blk0 = blocks;
    const int nb = (int)cdiv(cdiv(len, t.V), 256 / G);
    nblk[a.ntasks - 1] = nb;
    blocks += nb;
    if (mslot >= 0) {
      t.mbase = mnext[mslot];
      mnext[mslot] += nb;
    }
  }
  // Fused Adam step `step` on every parameter as its gradient is summed (the tasks are all added); the
  // new W2 / W1a maxima go to the slots of the step's parity and are tagged step + 1 (tag of step s =
  // s + 1, 0: none), which step + 1's prep expects: the slots are complete when the reduce is, and the
  // next prep is a later launch.  false: a weight has more reduce blocks than a slot holds.
  bool adam(float* p, float* m, float* v, const float* grad, const AdamCo& co, int step, const SfNetW (&w)[2]) {
    for (int k = 0; k < 4; ++k)
      if (mnext[k] > SF_PMAX) return false;
    a.p = p; a.m = m; a.v = v; a.grad = grad; a.co = co;
    const int par = step & 1;
    for (int net = 0; net < 2; ++net) {
      a.slot[2 * net] = w[net].pmax + (par * 2 + 0) * SF_PMAX;
      a.slot[2 * net + 1] = w[net].pmax + (par * 2 + 1) * SF_PMAX;
      a.tag[net] = w[net].tag + par;
    }
    a.tag_val = (unsigned)step + 1u;
    return true;
  }
};

}  // namespace rlks
