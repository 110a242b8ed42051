// ppo.hip — host API of the policy/value MLP and the PPO update (include/rlks.h, section K4):
// layout, forward, gradient orchestration (F1 -> F2 -> F3 -> reduce), global-norm clipping, Adam, the
// SGD-step entries and the KL-coefficient update.  The reduce's device code is reduce.h, the minibatch
// gather gather.h / gather.hip, the workspace layouts workspace.h, the rollout loops rollout.hip.
//
// Reference: RLlib PPO behind train_ppo.py:9-31 (train_batch_size 4000, sgd_minibatch_size 256,
// num_sgd_iter 10, lr 3e-4, gamma 0.99) and train_final.py:6-20.  RLlib is third-party and absent
// from /root/reference: the restated semantics are pinned against oracle/oracle.py.
#include <cmath>

#include "gather.h"
#include "reduce.h"
#include "workspace.h"

namespace rlks {

// ----------------------------------------------------------------------------- kernels

__global__ __launch_bounds__(256) void k_reduce(RedArgs g) { reduce_block<RED_PLAIN>(g, (int)blockIdx.x, NrmArgs{}); }
template <int MODE>
__global__ __launch_bounds__(256) void k_reduce_clip(RedArgs g, NrmArgs c) {
  reduce_block<MODE>(g, (int)blockIdx.x, c);
}

// The norm's tree continued over the reduce blocks' partials, one 256-thread block: per tensor k the
// nb[k] partials from blk0[k] on, 64 at a time per wave (level 0: from memory, all tensors' chunks
// numbered through by c0[k]; level 1: over level 0's sums), then up to 16 level-1 sums per tensor by
// one thread, then the tensors in order.  norm = sqrt(S), coef = (float)min(1, clip / (norm + 1e-6)).
__global__ __launch_bounds__(256) void k_norm_finish(NrmPlan pl, const double* __restrict__ part, float clip,
                                                     double* __restrict__ norm_ws, float* __restrict__ coef_ws,
                                                     double* __restrict__ norm_out, double* __restrict__ stats) {
  __shared__ double l0[NRM_MAX_CHUNKS];
  __shared__ double l1[RLKS_N_TENSORS][16];
  __shared__ double ts[RLKS_N_TENSORS];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  for (int ch = wave; ch < pl.c0[pl.n]; ch += 4) {
    int k = 0;
    while (k + 1 < pl.n && ch >= pl.c0[k + 1]) ++k;
    const int i = (ch - pl.c0[k]) * 64 + lane;
    const double v = tree64(i < pl.nb[k] ? part[pl.blk0[k] + i] : 0.0);
    if (lane == 0) l0[ch] = v;
  }
  __syncthreads();
  for (int k = wave; k < pl.n; k += 4) {
    const int n1 = pl.c0[k + 1] - pl.c0[k];
    for (int c2 = 0; c2 < 16; ++c2) {
      const int i = c2 * 64 + lane;
      const double v = c2 * 64 < n1 ? tree64(i < n1 ? l0[pl.c0[k] + i] : 0.0) : 0.0;  // (wave-uniform)
      if (lane == 0) l1[k][c2] = v;
    }
  }
  __syncthreads();
  if ((int)threadIdx.x < pl.n) {
    const double* e = l1[threadIdx.x];
    ts[threadIdx.x] = (((e[0] + e[1]) + (e[2] + e[3])) + ((e[4] + e[5]) + (e[6] + e[7]))) +
                      (((e[8] + e[9]) + (e[10] + e[11])) + ((e[12] + e[13]) + (e[14] + e[15])));
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    double S = 0.0;
    for (int k = 0; k < pl.n; ++k) S += ts[k];
    const double norm = sqrt(S);
    if (norm_ws) *norm_ws = norm;
    if (coef_ws) *coef_ws = (float)fmin(1.0, (double)clip / (norm + 1e-6));
    if (norm_out) *norm_out = norm;
    if (stats) stats[RLKS_STAT_GRAD_GNORM] = norm;
  }
}

// the reduce with the next SGD step's packed gather in its extra blocks (NextGather, gather.h)
template <int S, int PS>
__global__ __launch_bounds__(256) void k_reduce_gather(RedArgs g, NextGather n) {
  if ((int)blockIdx.x < n.blk0) {
    reduce_block<RED_PLAIN>(g, (int)blockIdx.x, NrmArgs{});
    return;
  }
  gather_packed_elem<S, PS>(n.perm, n.row0g, n.rows_g, n.Ng, n.N, n.rows, n.packed, n.mb,
                            ((uint32_t)blockIdx.x - (uint32_t)n.blk0) * 256u + threadIdx.x);
}
// the same with the norm partials of the clipped step (rlks_ppo_sgd_step_clip)
template <int S, int PS>
__global__ __launch_bounds__(256) void k_reduce_gather_nrm(RedArgs g, NextGather n, NrmArgs c) {
  if ((int)blockIdx.x < n.blk0) {
    reduce_block<RED_NRM>(g, (int)blockIdx.x, c);
    return;
  }
  gather_packed_elem<S, PS>(n.perm, n.row0g, n.rows_g, n.Ng, n.N, n.rows, n.packed, n.mb,
                            ((uint32_t)blockIdx.x - (uint32_t)n.blk0) * 256u + threadIdx.x);
}

// fp32 path: per-net stat sums -> RLKS_STAT_* layout
__global__ void k_stats_finish(double* __restrict__ st, const double* __restrict__ s_pi,
                               const double* __restrict__ s_vf, int rows) {
  if (threadIdx.x) return;
  st[RLKS_STAT_POLICY_LOSS] = s_pi[0];
  st[RLKS_STAT_VF_LOSS] = s_vf[1];
  st[RLKS_STAT_KL] = s_pi[2];
  st[RLKS_STAT_ENTROPY] = s_pi[3];
  st[RLKS_STAT_ROWS] = (double)rows;
  st[5] = st[6] = st[7] = 0.0;
}

// ----------------------------------------------------------------------------- Adam
// torch.optim.Adam (single-tensor path): exp_avg.lerp_(g, 1-b1); exp_avg_sq = b2*v + (1-b2)*g*g;
// p -= (lr / (1 - b1^t)) * m / (sqrt(v) / sqrt(1 - b2^t) + eps)
__global__ void k_adam(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ m,
                       float* __restrict__ v, int64_t n, AdamCo co) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  (void)adam_elem(p, m, v, i, g[i], co);
}

// the same on the clipped gradient g coef (k_norm_finish's coefficient), which replaces g
__global__ void k_adam_clip(float* __restrict__ p, float* __restrict__ g, float* __restrict__ m,
                            float* __restrict__ v, int64_t n, AdamCo co, const float* __restrict__ coef) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const float gi = clip_mul(g[i], *coef);
  g[i] = gi;
  (void)adam_elem(p, m, v, i, gi, co);
}

// RLlib PPO update_kl
__global__ void k_kl_update(float* __restrict__ dyn, const double* __restrict__ kc, float target) {
  if (threadIdx.x) return;
  const double kl = kc[1] > 0 ? kc[0] / kc[1] : 0.0;
  float c = dyn[RLKS_DYN_KL_COEFF];
  if (kl > 2.0 * target) c *= 1.5f;
  else if (kl < 0.5 * target) c *= 0.5f;
  dyn[RLKS_DYN_KL_COEFF] = c;
}

__global__ void k_empty() {}  // (rlks_ppo_grad_profile: the event bracket's own time)

// ----------------------------------------------------------------------------- norm / clip plumbing
// One parameter-gradient task per tensor over the flat gradient g as a single partial, summed in
// place (each element read and written by one thread): the reducer of the Adam pass after an
// all-reduce, of the clipped Adam pass and of the norm pass.  slots: the W2 / W1a tasks feed the next
// operand split's max |w| slots (fused Adam).  norm_order: a [256][256] W2 takes the vector numbering
// of the gradient reduce (kq 2; reduce_block<RED_NRM_ONLY> only).
static void flat_tasks(Reducer& R, const rlks_mlp_desc* d, const Layout& L, float* g, bool slots, bool norm_order) {
  const int D = d->obs_dim, A = d->n_actions, H = d->hidden;
  for (int net = 0; net < 2; ++net) {
    const int An = net == 0 ? A : 1;
    const int64_t* o = L.off + 6 * net;
    R.add(g + o[0], g + o[0], nullptr, 0, 1, H * D, slots ? 2 * net + 1 : -1);
    R.add(g + o[1], g + o[1], nullptr, 0, 1, H, slots ? 2 * net + 1 : -1);
    R.add(g + o[2], g + o[2], nullptr, 0, 1, H * H, slots ? 2 * net : -1);
    if (norm_order) R.a.t[R.a.ntasks - 1].kq = 2;
    R.add(g + o[3], g + o[3], nullptr, 0, 1, H);
    R.add(g + o[4], g + o[4], nullptr, 0, 1, An * H);
    R.add(g + o[5], g + o[5], nullptr, 0, 1, An);
  }
}
// the fused 256-unit kernels' gradient reduce numbers W2's vectors in k_sf_dw2r's partial order
static bool norm_order(const rlks_mlp_desc* d) { return is_sf(d) && !is_wide(d); }

// The clip's scratch, behind the gradient workspace of `rows` rows (rlks_ppo_workspace_bytes counts
// it): the reduce blocks' norm partials, then the norm (f64) and the coefficient (f32), taken from c.
struct NrmWs {
  double* part;
  double* norm;
  float* coef;
  int cap;  // partials
};
static NrmWs nrm_ws(const rlks_mlp_desc* d, WsCursor& c) {
  const Layout L = make_layout(d->obs_dim, d->hidden, d->n_actions);
  NrmWs w{};
  if (norm_order(d)) {
    // the fused step's gradient reduce: at most one block per output vector
    w.cap = (int)(L.padded / 4) + 64;
  } else {
    Reducer R;
    flat_tasks(R, d, L, nullptr, false, false);
    w.cap = R.blocks;
  }
  w.part = c.take<double>(8LL * w.cap);
  w.norm = c.take<double>(8 + 4);  // the norm and, 8 bytes on, the coefficient
  w.coef = w.norm ? (float*)(w.norm + 1) : nullptr;
  return w;
}

// sum g^2 of the block partials the plan names -> norm, coefficient (and norm_out / stats[GRAD_GNORM])
static int norm_finish(const Reducer& R, const NrmWs& n, float clip, double* norm_out, double* stats, hipStream_t s) {
  NrmPlan pl;
  RLKS_REQUIRE(R.blocks <= n.cap && R.plan(pl), RLKS_ERR_UNSUPPORTED, "grad_clip: too many reduce blocks for the norm");
  hipLaunchKernelGGL(k_norm_finish, dim3(1), dim3(256), 0, s, pl, n.part, clip, n.norm, n.coef, norm_out, stats);
  RLKS_LAUNCHED();
  return RLKS_OK;
}

// the norm of the flat gradient g (one partial, nothing written back) -> n.norm / n.coef, norm_out, stats
static int norm_pass(const rlks_mlp_desc* d, const float* g, const NrmWs& n, float clip, double* norm_out,
                     double* stats, hipStream_t s) {
  const Layout L = make_layout(d->obs_dim, d->hidden, d->n_actions);
  Reducer R;
  flat_tasks(R, d, L, const_cast<float*>(g), false, norm_order(d));
  RLKS_REQUIRE(R.blocks <= n.cap, RLKS_ERR_UNSUPPORTED, "grad_clip: too many reduce blocks for the norm");
  hipLaunchKernelGGL(k_reduce_clip<RED_NRM_ONLY>, dim3(R.blocks), dim3(256), 0, s, R.a, NrmArgs{n.part, nullptr});
  RLKS_LAUNCHED();
  return norm_finish(R, n, clip, norm_out, stats, s);
}

static bool clip_ok(float c) { return std::isfinite(c) && c > 0.f; }

// the gradient workspace of `rows` rows alone, without the clip's scratch behind it
static int grad_ws_bytes(const rlks_mlp_desc* d, int rows, int64_t* bytes) {
  if (int rc = check_desc(d)) return rc;
  const bool wide = is_wide(d), sf = is_sf(d);
  RLKS_REQUIRE(bytes && rows > 0 && rows % (wide ? 1 : sf ? 256 : GB) == 0, RLKS_ERR_ARG,
               wide ? "rlks_ppo_workspace_bytes: bad argument"
               : sf ? "rlks_ppo_workspace_bytes: split-fp16 rows must be a positive multiple of 256"
                    : "rlks_ppo_workspace_bytes: rows must be a positive multiple of 128");
  const int D = d->obs_dim, A = d->n_actions;
  *bytes = wide ? wide_ws_layout(D, d->hidden, A, rows, nullptr).bytes
           : sf ? sf_ws_layout(D, A, rows, nullptr).bytes : ws_layout(D, A, rows, nullptr).bytes;
  return RLKS_OK;
}

// the clip's scratch inside the caller's workspace of `rows` gradient rows
static int nrm_ws_at(const rlks_mlp_desc* d, int rows, void* workspace, int64_t ws_bytes, NrmWs& n) {
  int64_t gb = 0;
  if (int rc = grad_ws_bytes(d, rows, &gb)) return rc;
  WsCursor c{(char*)workspace};
  c.take<char>(gb);
  n = nrm_ws(d, c);
  RLKS_REQUIRE(ws_bytes >= c.o, RLKS_ERR_ARG, "grad_clip: workspace too small (rlks_ppo_workspace_bytes)");
  return RLKS_OK;
}

// SGD step with Adam fused into the gradient reduction (single rank: no gradient all-reduce between
// them).  step: the Adam step performed (1-based); prev_fused: the previous SGD step on these
// parameters was fused, so its reduce left this step's weight maxima in the split's slots.
struct FusedAdam {
  float *p, *m, *v;
  AdamCo co;
  int step, prev_fused;
  bool apply = true;  // false: the prep uses the previous step's maxima, the reduce only sums (an
                      // all-reduce follows; rlks_ppo_adam_apply then applies Adam)
  int64_t n = 0;      // parameter count, for the unfused Adam pass of the fp32 / wide paths (sgd_step)
  float clip = 0.f;   // > 0 (with apply): global-norm clipping, Adam as a pass of its own after the norm
};

// What the gradient and SGD-step entry points share; the step entries are argument adapters over sgd_step_any.
struct StepArgs {
  const rlks_mlp_desc* d;
  const rlks_ppo_coeffs* co;
  const float *params, *dyn, *mb;
  int M;
  float* grad;
  double* stats;
  void* workspace; int64_t ws_bytes;
  void* stream;
};

// ----------------------------------------------------------------------------- gradient drivers
// The reduce at the end of a split-fp16 gradient, one launch: R's tasks, with the next step's packed
// gather nx (or null / no rows) in extra blocks after the reduce's, and with one norm partial per
// block when nrm is given (the clipped step).
static int launch_reduce(const Reducer& R, int stride, const NextGather* nx, const NrmWs* nrm, hipStream_t s) {
  const NrmArgs c{nrm ? nrm->part : nullptr, nullptr};
  if (nx && nx->rows > 0) {
    NextGather n = *nx;
    n.blk0 = R.blocks;
    const bool narrow = with_record(stride, [&](auto r) {
      using Rc = decltype(r);
      const dim3 grid(R.blocks + (int)cdiv((int64_t)n.rows * Rc::PS / 4, 256));
      if (nrm) hipLaunchKernelGGL((k_reduce_gather_nrm<Rc::S, Rc::PS>), grid, dim3(256), 0, s, R.a, n, c);
      else hipLaunchKernelGGL((k_reduce_gather<Rc::S, Rc::PS>), grid, dim3(256), 0, s, R.a, n);
    });
    RLKS_REQUIRE(narrow, RLKS_ERR_UNSUPPORTED, "rlks_ppo_*_next: records of 2, 4 or 8 clouds only");
  } else if (nrm) {
    hipLaunchKernelGGL(k_reduce_clip<RED_NRM>, dim3(R.blocks), dim3(256), 0, s, R.a, c);
  } else {
    launch_timed(KEV_REDUCE, k_reduce, dim3(R.blocks), dim3(256), 0, s, R.a);
  }
  RLKS_LAUNCHED();
  return RLKS_OK;
}

// What sf_grad takes beside the step's arguments.  part: 0 = the whole gradient; 1 = the weight split,
// F1a, F2 and the reduce of W2 / b2 / W3 / b3 and the stats; 2 = F1b and the reduce of W1 / b1
// (rlks_ppo_grad_step_part: the caller all-reduces part 1's buckets while part 2 runs)
struct GradOpts {
  int phases = RLKS_PHASE_ALL;
  int part = 0;
  const FusedAdam* fa = nullptr;   // the prep's parity / maxima, and Adam in the reduce when fa->apply
  const NextGather* nx = nullptr;  // the next step's gather in the reduce's launch
  const NrmWs* nrm = nullptr;      // the clipped step: norm partials in the reduce, then the norm for `clip`
  float clip = 0.f;
};

static int sf_grad(const StepArgs& st, const GradOpts& o) {
  const rlks_mlp_desc* d = st.d;
  const FusedAdam* fa = o.fa;
  const int M = st.M, part = o.part;
  int phases = o.phases;
  float* const grad = st.grad;
  double* const stats = st.stats;
  hipStream_t s = (hipStream_t)st.stream;
  RLKS_REQUIRE(M > 0 && M % 256 == 0, RLKS_ERR_ARG, "rlks_ppo_grad: split-fp16 rows must be a positive multiple of 256");
  const int D = d->obs_dim, A = d->n_actions, H = HID;
  const SfWs w = sf_ws_layout(D, A, M, (char*)st.workspace);
  RLKS_REQUIRE(st.ws_bytes >= w.bytes, RLKS_ERR_ARG, "rlks_ppo_grad: workspace too small");
  const Layout L = make_layout(D, H, A);
  const bool f_pi = phases & (RLKS_PHASE_FWD | RLKS_PHASE_FWD_PI), f_vf = phases & (RLKS_PHASE_FWD | RLKS_PHASE_FWD_VF);
  if (part == 2) phases &= ~(RLKS_PHASE_PREP | RLKS_PHASE_DW2);
  if ((phases & (RLKS_PHASE_FWD | RLKS_PHASE_PREP)) && part != 2) {
    const int parity = fa ? ((fa->step - 1) & 1) : 0;
    if (int rc = sf_prep(d, w, st.params, s, false, parity, fa && fa->prev_fused, fa ? (unsigned)fa->step : 0u))
      return rc;
  }
  SfArgs a{};
  a.x = st.mb; a.x_stride = mb_stride(D, A); a.M = M; a.D = D; a.A_pi = A;
  a.tiles_per_split = w.tiles_per_split; a.co = *st.co; a.dyn = st.dyn; a.xsp = w.xsp;
  a.products = d->precision == RLKS_PRECISION_F16 ? 1 : 3;
  sf_nets(a.n, w, st.params, L);
  // F1 (forward, loss, dZ2, dH1 -> dW1 / db1, dW3 / db3) per net; F2 (dW2, db2) for both.  F1's form is
  // decided here, once, for the launch and for the reducer's partial count alike:
  //   part 1 / 2 (the overlapped multi-rank form, F1b under the all-reduce): that part's split kernel;
  //   F1A / F1B without a FWD bit (profiling: each half reads what a full F1 left in the workspace): the
  //     split kernels asked for, both nets;
  //   else (rlks_ppo_grad, the fused-Adam SGD step, the multi-rank step's one-bucket form; also a call
  //     that only reduces): the fused kernel where sf_f1_fused says so, else both split kernels.
  const int f1ab = phases & (RLKS_PHASE_F1A | RLKS_PHASE_F1B);
  SfF1Form f1;
  if (part != 0) f1 = part == 1 ? SF_F1_A : SF_F1_B;
  else if (f1ab && !(f_pi || f_vf)) f1 = SfF1Form((f1ab & RLKS_PHASE_F1A ? SF_F1_A : 0) | (f1ab & RLKS_PHASE_F1B ? SF_F1_B : 0));
  else f1 = sf_f1_fused(A) ? SF_F1_FUSED : SF_F1_SPLIT;
  if (f_pi || f_vf) {
    if (int rc = launch_sf_f1(a, f_pi ? 0 : 1, (f_pi && f_vf) ? 2 : 1, A, s, f1)) return rc;
  } else if (f1ab) {
    if (int rc = launch_sf_f1(a, 0, 2, A, s, f1)) return rc;
  }
  if (phases & RLKS_PHASE_DW2)
    if (int rc = launch_sf_dw2(a, w.splits, s)) return rc;
  if (!(phases & RLKS_PHASE_REDUCE)) return RLKS_OK;
  const int f1p = sf_f1_parts(M, f1);  // the fused kernel has half the split kernels' workgroups
  Reducer R;
  for (int net = 0; net < 2; ++net) {
    const int An = net == 0 ? A : 1;
    const int64_t* o = L.off + 6 * net;
    const SfNet& n = w.n[net];
    if (part != 1) {
      R.add(n.part_w1, grad + o[0], nullptr, (int64_t)H * D, f1p, H * D, 2 * net + 1);
      R.add(n.part_b1, grad + o[1], nullptr, H, f1p, H, 2 * net + 1);
    }
    if (part != 2) {
      R.add(n.part_w2, grad + o[2], nullptr, SF_W2_PSTRIDE, w.splits, H * H, 2 * net);
      R.a.t[R.a.ntasks - 1].kq = 1;  // k_sf_dw2r's partial order
      R.add(n.part_b2, grad + o[3], nullptr, H, w.splits, H);
      R.add(n.part_w3, grad + o[4], nullptr, (int64_t)An * H, f1p, An * H);
      if (net == 0) R.add(n.part_b3, grad + o[5], nullptr, An, f1p, An);
      else R.add(n.part_b3, grad + o[5], nullptr, 1, 2 * f1p, 1);  // every hi and lo, in f64
    }
  }
  if (stats && part != 2) {  // per-block columns [policy loss, vf loss, kl, entropy] -> RLKS_STAT_* directly
    const int tiles = f1p;
    R.add(w.n[0].part_stat + 0, nullptr, stats + RLKS_STAT_POLICY_LOSS, 4, tiles, 1);
    R.add(w.n[1].part_stat + 1, nullptr, stats + RLKS_STAT_VF_LOSS, 4, tiles, 1);
    R.add(w.n[0].part_stat + 2, nullptr, stats + RLKS_STAT_KL, 4, tiles, 1);
    R.add(w.n[0].part_stat + 3, nullptr, stats + RLKS_STAT_ENTROPY, 4, tiles, 1);
    R.a.stats = stats;
    R.a.rows = (double)M;
  }
  if (fa && fa->apply) {  // Adam on every parameter as its gradient is summed; W2 / W1a maxima -> the next prep
    RLKS_REQUIRE(part == 0, RLKS_ERR_ARG, "sf_grad: fused Adam needs the whole gradient");
    RLKS_REQUIRE(R.adam(fa->p, fa->m, fa->v, grad, fa->co, fa->step, w.w), RLKS_ERR_UNSUPPORTED,
                 "rlks_ppo_sgd_step: too many reduce blocks per weight");
  }
  if (o.nrm) {  // the clipped step: the same reduce (and gather) with one norm partial per block, then the norm
    RLKS_REQUIRE(part == 0 && !(fa && fa->apply), RLKS_ERR_ARG, "sf_grad: the norm needs the whole, unapplied gradient");
    RLKS_REQUIRE(R.blocks <= o.nrm->cap, RLKS_ERR_UNSUPPORTED, "grad_clip: too many reduce blocks for the norm");
  }
  if (int rc = launch_reduce(R, mb_stride(D, A), o.nx, o.nrm, s)) return rc;
  return o.nrm ? norm_finish(R, *o.nrm, o.clip, nullptr, stats, s) : RLKS_OK;
}

static AdamCo adam_co(float lr, float beta1, float beta2, float eps, int step) {
  const double bc1 = 1.0 - std::pow((double)beta1, step);
  const double bc2 = 1.0 - std::pow((double)beta2, step);
  return AdamCo{1.f - beta1, beta2, 1.f - beta2, (float)(lr / bc1), (float)std::sqrt(bc2), eps};
}

// Adam as a pass of its own over g; coef (or null): on the clipped gradient g coef, which replaces g
static int adam_pass(float* p, float* g, float* m, float* v, int64_t n, const AdamCo& co, const float* coef,
                     void* stream) {
  RLKS_REQUIRE(p && g && m && v && n >= 0, RLKS_ERR_ARG,
               coef ? "rlks_ppo_adam_apply_clip: bad argument" : "rlks_adam_step: bad argument");
  if (n == 0) return RLKS_OK;
  const dim3 grid(cdiv(n, 256));
  if (coef) hipLaunchKernelGGL(k_adam_clip, grid, dim3(256), 0, (hipStream_t)stream, p, g, m, v, n, co, coef);
  else hipLaunchKernelGGL(k_adam, grid, dim3(256), 0, (hipStream_t)stream, p, g, m, v, n, co);
  RLKS_LAUNCHED();
  return RLKS_OK;
}

// Adam over the flat gradient as a reduce over one partial that also leaves the new weights' maxima
// and the step tag (rlks_ppo_adam_apply); coef: first g <- g coef, written back (the clipped pass)
static int sf_adam_apply(const rlks_mlp_desc* d, float* params, float* grad, float* adam_m, float* adam_v,
                         const AdamCo& co, int step, void* workspace, int64_t ws_bytes, int rows, const float* coef,
                         hipStream_t s) {
  RLKS_REQUIRE(rows > 0 && rows % 256 == 0, RLKS_ERR_ARG, "rlks_ppo_adam_apply: rows as in rlks_ppo_grad_step");
  const SfWs w = sf_ws_layout(d->obs_dim, d->n_actions, rows, (char*)workspace);
  RLKS_REQUIRE(ws_bytes >= w.bytes, RLKS_ERR_ARG, "rlks_ppo_adam_apply: workspace too small");
  const Layout L = make_layout(d->obs_dim, HID, d->n_actions);
  Reducer R;
  flat_tasks(R, d, L, grad, true, false);
  RLKS_REQUIRE(R.adam(params, adam_m, adam_v, grad, co, step, w.w), RLKS_ERR_UNSUPPORTED,
               "rlks_ppo_adam_apply: too many blocks per weight");
  if (coef) hipLaunchKernelGGL(k_reduce_clip<RED_CLIP>, dim3(R.blocks), dim3(256), 0, s, R.a, NrmArgs{nullptr, coef});
  else hipLaunchKernelGGL(k_reduce, dim3(R.blocks), dim3(256), 0, s, R.a);
  RLKS_LAUNCHED();
  return RLKS_OK;
}

// gradient only: the prep reads the previous step's maxima when prev_fused, the reduce only sums
static FusedAdam grad_only(int step, int prev_fused) {
  return FusedAdam{nullptr, nullptr, nullptr, AdamCo{}, step, prev_fused ? 1 : 0, false};
}

// the next step's gather as extra reduce blocks (fused = true), or false: the caller gathers with
// rlks_ppo_gather_packed after the step (wide / fp32 paths, more than NEXT_GROUPS lane groups)
static int next_gather(const rlks_mlp_desc* d, const rlks_gather_next* x, NextGather& n, bool& fused) {
  RLKS_REQUIRE(x->packed_dev && x->mb_dev && x->rows >= 0 && x->T > 0 && x->N > 0, RLKS_ERR_ARG,
               "rlks_ppo_*_next: bad gather argument");
  RLKS_REQUIRE(rlks_packed_stride(d) > 0, RLKS_ERR_UNSUPPORTED, "rlks_ppo_*_next: records of 2, 4 or 8 clouds only");
  GatherArgs g;
  if (int rc = gather_args(d, x->T, x->N, x->perm_seed, x->epoch, x->groups, x->group0, x->row0, x->rows, x->mb_dev, g))
    return rc;
  fused = is_sf(d) && !is_wide(d) && x->groups <= NEXT_GROUPS;
  n = NextGather{};
  for (int k = 0; k < x->groups && k < NEXT_GROUPS; ++k) n.perm[k] = g.perm[k];
  n.row0g = g.row0g; n.rows = g.rows; n.rows_g = g.rows_g; n.Ng = g.Ng; n.N = x->N;
  n.mb = x->mb_dev; n.packed = x->packed_dev;
  return RLKS_OK;
}

static int gather_after(const rlks_mlp_desc* d, const rlks_gather_next* x, void* stream) {
  return rlks_ppo_gather_packed(d, x->packed_dev, x->T, x->N, x->perm_seed, x->epoch, x->groups, x->group0, x->row0,
                                x->rows, x->mb_dev, stream);
}

// One SGD step: the gradient of `part` (sf_grad: 0 = whole), Adam in its reduce when fa.apply, and the
// next step's gather x (or null; taken by part 0 and part 2) in the reduce's launch where that form
// exists, else as a call of its own after the step.  Off the split-fp16 kernels nothing is fused:
// the gradient (all of it in part 1), then Adam as a pass of its own, then the gather.
// bad_arg: the entry point's message for a null argument or step < 1.
static int sgd_step_any(const StepArgs& a, const char* bad_arg, const FusedAdam& fa, const rlks_gather_next* x,
                        int part) {
  if (int rc = check_desc(a.d)) return rc;
  RLKS_REQUIRE(a.co && a.params && a.dyn && a.mb && a.grad && a.workspace && fa.step >= 1 &&
                   (!fa.apply || (fa.m && fa.v)), RLKS_ERR_ARG, bad_arg);
  if (part == 1) x = nullptr;
  const bool clip = fa.apply && fa.clip > 0.f;
  NrmWs nw{};
  if (clip) {
    RLKS_REQUIRE(part == 0, RLKS_ERR_ARG, bad_arg);
    if (int rc = nrm_ws_at(a.d, a.M, a.workspace, a.ws_bytes, nw)) return rc;
  }
  if (!is_sf(a.d) || is_wide(a.d)) {
    if (part != 2) {
      if (int rc = rlks_ppo_grad(a.d, a.co, a.params, a.dyn, a.mb, a.M, a.grad, a.stats, a.workspace, a.ws_bytes, a.stream))
        return rc;
      // clipped: the norm of the gradient first, then Adam on g coef
      if (clip)
        if (int rc = norm_pass(a.d, a.grad, nw, fa.clip, nullptr, a.stats, (hipStream_t)a.stream)) return rc;
      if (fa.apply)
        if (int rc = adam_pass(fa.p, a.grad, fa.m, fa.v, fa.n, fa.co, clip ? nw.coef : nullptr, a.stream)) return rc;
    }
    return x ? gather_after(a.d, x, a.stream) : RLKS_OK;
  }
  NextGather n;
  bool fused = false;
  if (x)
    if (int rc = next_gather(a.d, x, n, fused)) return rc;
  // clipped: the gradient as the multi-rank step computes it (the reduce only sums; the next gather stays
  // in its launch) with the norm partials, the norm, then the clipped Adam pass as a launch of its own
  const FusedAdam g = grad_only(fa.step, fa.prev_fused);
  GradOpts o;
  o.part = part; o.fa = clip ? &g : &fa; o.nx = fused ? &n : nullptr;
  if (clip) { o.nrm = &nw; o.clip = fa.clip; }
  if (int rc = sf_grad(a, o)) return rc;
  if (clip)
    if (int rc = sf_adam_apply(a.d, fa.p, a.grad, fa.m, fa.v, fa.co, fa.step, a.workspace, a.ws_bytes, a.M, nw.coef,
                               (hipStream_t)a.stream))
      return rc;
  return (x && !fused) ? gather_after(a.d, x, a.stream) : RLKS_OK;
}

}  // namespace rlks

using namespace rlks;

extern "C" {

int rlks_mlp_layout(const rlks_mlp_desc* d, int64_t* offsets, int64_t* padded, int64_t* real) {
  RLKS_REQUIRE(d && d->obs_dim > 0 && d->hidden > 0 && d->n_actions > 0, RLKS_ERR_ARG, "rlks_mlp_layout: bad desc");
  const Layout L = make_layout(d->obs_dim, d->hidden, d->n_actions);
  if (offsets)
    for (int i = 0; i < RLKS_N_TENSORS; ++i) offsets[i] = L.off[i];
  if (padded) *padded = L.padded;
  if (real) *real = L.real;
  return RLKS_OK;
}

int rlks_policy_forward(const rlks_mlp_desc* d, const float* params, const float* obs, int n, float* logits,
                        float* values, void* stream) {
  if (int rc = check_desc(d)) return rc;
  RLKS_REQUIRE(!is_wide(d), RLKS_ERR_UNSUPPORTED, "rlks_policy_forward: this MLP needs rlks_policy_forward_ws");
  RLKS_REQUIRE(params && obs && n >= 0, RLKS_ERR_ARG, "rlks_policy_forward: bad argument");
  if (n == 0) return RLKS_OK;
  const Layout L = make_layout(d->obs_dim, d->hidden, d->n_actions);
  return forward_fp32(params, L, obs, n, d->obs_dim, d->n_actions, logits, values, (hipStream_t)stream);
}

int rlks_policy_forward_ws(const rlks_mlp_desc* d, const float* params, const float* obs, int n, float* logits,
                           float* values, void* workspace, int64_t ws_bytes, void* stream) {
  if (int rc = check_desc(d)) return rc;
  if (!is_wide(d)) return rlks_policy_forward(d, params, obs, n, logits, values, stream);
  RLKS_REQUIRE(params && obs && n >= 0 && workspace, RLKS_ERR_ARG, "rlks_policy_forward_ws: bad argument");
  if (n == 0) return RLKS_OK;
  const WideWs w = wide_ws_layout(d->obs_dim, d->hidden, d->n_actions, n, (char*)workspace);
  RLKS_REQUIRE(ws_bytes >= w.bytes, RLKS_ERR_ARG, "rlks_policy_forward_ws: workspace too small");
  return wide_forward(d, params, obs, d->obs_dim, n, w, logits, values, (hipStream_t)stream);
}

int rlks_ppo_workspace_bytes(const rlks_mlp_desc* d, int rows, int64_t* bytes) {
  if (int rc = grad_ws_bytes(d, rows, bytes)) return rc;
  WsCursor c{nullptr};
  c.take<char>(*bytes);
  (void)nrm_ws(d, c);
  *bytes = c.o;
  return RLKS_OK;
}

int rlks_grad_global_norm(const rlks_mlp_desc* d, const float* grad, int64_t n_params, double* norm_dev,
                          void* workspace, int64_t ws_bytes, void* stream) {
  if (int rc = check_desc(d)) return rc;
  RLKS_REQUIRE(grad && norm_dev && workspace, RLKS_ERR_ARG, "rlks_grad_global_norm: null argument");
  RLKS_REQUIRE(n_params == make_layout(d->obs_dim, d->hidden, d->n_actions).padded, RLKS_ERR_ARG,
               "rlks_grad_global_norm: n_params must be the padded layout size");
  WsCursor c{(char*)workspace};
  const NrmWs n = nrm_ws(d, c);
  RLKS_REQUIRE(ws_bytes >= c.o, RLKS_ERR_ARG, "rlks_grad_global_norm: workspace too small");
  return norm_pass(d, grad, n, 1.f, norm_dev, nullptr, (hipStream_t)stream);
}

int rlks_debug_sf_handoff(const rlks_mlp_desc* d, int rows, void* ws, void** out) {
  if (int rc = check_desc(d)) return rc;
  RLKS_REQUIRE(out && ws && rows > 0 && rows % 256 == 0 && is_sf(d) && !is_wide(d),
               RLKS_ERR_ARG, "rlks_debug_sf_handoff: split-fp16 descriptor, rows % 256 == 0");
  const SfWs w = sf_ws_layout(d->obs_dim, d->n_actions, rows, (char*)ws);
  for (int net = 0; net < 2; ++net) {
    out[net] = w.n[net].dz2s;
    out[2 + net] = w.n[net].tile_edz;
  }
  return RLKS_OK;
}

int rlks_debug_wide_bufs(const rlks_mlp_desc* d, int rows, void* ws, void** out) {
  if (int rc = check_desc(d)) return rc;
  RLKS_REQUIRE(out && ws && rows > 0 && is_wide(d), RLKS_ERR_ARG, "rlks_debug_wide_bufs: wide descriptor");
  const WideWs w = wide_ws_layout(d->obs_dim, d->hidden, d->n_actions, rows, (char*)ws);
  for (int net = 0; net < 2; ++net) {
    out[3 * net] = w.n[net].h2;
    out[3 * net + 1] = w.n[net].out;
    out[3 * net + 2] = w.n[net].dout;
  }
  return RLKS_OK;
}

int rlks_ppo_grad_phases(const rlks_mlp_desc* d, const rlks_ppo_coeffs* co, const float* params, const float* dyn,
                         const float* mb, int M, float* grad, double* stats, void* workspace, int64_t ws_bytes,
                         int phases, void* stream) {
  if (int rc = check_desc(d)) return rc;
  if (is_wide(d)) {
    RLKS_REQUIRE(co && params && dyn && mb && grad && workspace && M > 0, RLKS_ERR_ARG, "rlks_ppo_grad: bad argument");
    const WideWs w = wide_ws_layout(d->obs_dim, d->hidden, d->n_actions, M, (char*)workspace);
    RLKS_REQUIRE(ws_bytes >= w.bytes, RLKS_ERR_ARG, "rlks_ppo_grad: workspace too small");
    (void)phases;
    return wide_grad(d, co, params, dyn, mb, M, grad, stats, w, (hipStream_t)stream);
  }
  RLKS_REQUIRE(co && params && dyn && mb && grad && workspace, RLKS_ERR_ARG, "rlks_ppo_grad: null argument");
  if (is_sf(d)) {
    GradOpts o;
    o.phases = phases;
    return sf_grad({d, co, params, dyn, mb, M, grad, stats, workspace, ws_bytes, stream}, o);
  }
  RLKS_REQUIRE(M > 0 && M % GB == 0, RLKS_ERR_ARG, "rlks_ppo_grad: rows must be a positive multiple of 128");
  const int D = d->obs_dim, A = d->n_actions, H = HID;
  const Ws w = ws_layout(D, A, M, (char*)workspace);
  RLKS_REQUIRE(ws_bytes >= w.bytes, RLKS_ERR_ARG, "rlks_ppo_grad: workspace too small");
  hipStream_t s = (hipStream_t)stream;
  const Layout L = make_layout(D, H, A);
  const int stride = mb_stride(D, A);

  for (int net = 0; net < 2; ++net)
    if ((phases & RLKS_PHASE_FWD) || (phases & (net ? RLKS_PHASE_FWD_VF : RLKS_PHASE_FWD_PI))) {
      FwdArgs f{};
      f.P = net_ptrs_host(params, L, net);
      f.x = mb; f.x_stride = stride; f.M = M; f.D = D; f.A_pi = A;
      f.co = *co; f.dyn = dyn;
      const NetWs& n = w.n[net];
      f.dz2 = n.dz2; f.part_b2 = n.part_b2; f.part_w3 = n.part_w3; f.part_b3 = n.part_b3; f.part_stat = n.part_stat;
      if (int rc = launch_fwd_head(f, net, A, FWD_TRAIN, s)) return rc;
    }
  Dw2Args a2{};
  Dh1Args a1{};
  a2.x = a1.x = mb; a2.x_stride = a1.x_stride = stride; a2.M = a1.M = M; a2.rows_per_split = M / w.splits;
  for (int net = 0; net < 2; ++net) {
    a2.P[net] = a1.P[net] = net_ptrs_host(params, L, net);
    a2.dz2[net] = a1.dz2[net] = w.n[net].dz2;
    a2.part[net] = w.n[net].part_w2;
    a1.part_w1[net] = w.n[net].part_w1;
    a1.part_b1[net] = w.n[net].part_b1;
  }
  if (phases & RLKS_PHASE_DW2)
    if (int rc = launch_dw2(a2, D, w.splits, s)) return rc;
  if (phases & RLKS_PHASE_DH1)
    if (int rc = launch_dh1(a1, D, s)) return rc;
  if (!(phases & RLKS_PHASE_REDUCE)) return RLKS_OK;
  Reducer R;
  for (int net = 0; net < 2; ++net) {
    const int An = net == 0 ? A : 1;
    const int64_t* o = L.off + 6 * net;
    const NetWs& n = w.n[net];
    R.add(n.part_w1, grad + o[0], nullptr, (int64_t)H * D, w.tiles, H * D);
    R.add(n.part_b1, grad + o[1], nullptr, H, w.tiles, H);
    R.add(n.part_w2, grad + o[2], nullptr, (int64_t)H * H, w.splits, H * H);
    R.add(n.part_b2, grad + o[3], nullptr, H, w.tiles, H);
    R.add(n.part_w3, grad + o[4], nullptr, (int64_t)An * H, w.tiles, An * H);
    if (net == 0) R.add(n.part_b3, grad + o[5], nullptr, An, w.tiles, An);
    else R.add(n.part_b3, grad + o[5], nullptr, 1, 2 * w.tiles, 1);  // every hi and lo, in f64
    if (stats) R.add(n.part_stat, nullptr, w.stat64 + 4 * net, 4, w.tiles, 4);
  }
  hipLaunchKernelGGL(k_reduce, dim3(R.blocks), dim3(256), 0, s, R.a);
  RLKS_LAUNCHED();
  if (stats) {
    hipLaunchKernelGGL(k_stats_finish, dim3(1), dim3(64), 0, s, stats, w.stat64, w.stat64 + 4, M);
    RLKS_LAUNCHED();
  }
  return RLKS_OK;
}

int rlks_sf_f1_fused(const rlks_mlp_desc* d) {
  if (!d || !is_sf(d) || is_wide(d)) return 0;
  return sf_f1_fused(d->n_actions) ? 1 : 0;
}

int rlks_ppo_grad(const rlks_mlp_desc* d, const rlks_ppo_coeffs* co, const float* params, const float* dyn,
                  const float* mb, int M, float* grad, double* stats, void* workspace, int64_t ws_bytes,
                  void* stream) {
  return rlks_ppo_grad_phases(d, co, params, dyn, mb, M, grad, stats, workspace, ws_bytes, RLKS_PHASE_ALL, stream);
}

int rlks_ppo_grad_profile(const rlks_mlp_desc* d, const rlks_ppo_coeffs* co, const float* params, const float* dyn,
                          const float* mb, int M, float* grad, double* stats, void* workspace, int64_t ws_bytes,
                          int reps, double* ms_out, void* stream) {
  if (int rc = check_desc(d)) return rc;
  RLKS_REQUIRE(is_sf(d) && !is_wide(d) && reps > 0 && ms_out && co && params && dyn && mb && grad && workspace,
               RLKS_ERR_ARG, "rlks_ppo_grad_profile: split-fp16 descriptor, reps > 0");
  hipStream_t s = (hipStream_t)stream;
  hipEvent_t ev[2 * KEV_N];
  for (int i = 0; i < 2 * KEV_N; ++i)
    if (hipEventCreate(&ev[i]) != hipSuccess) return fail(RLKS_ERR_HIP, "rlks_ppo_grad_profile: event");
  for (int k = 0; k <= KEV_N; ++k) ms_out[k] = 0.0;
  // one untimed pass, then reps timed ones, each read back before its events are reused; a kernel
  // the pass does not launch (F1b under the fused F1) keeps its events unrecorded and reads 0
  const StepArgs a{d, co, params, dyn, mb, M, grad, stats, workspace, ws_bytes, stream};
  int rc = sf_grad(a, GradOpts{});
  for (int r = 0; r < reps && rc == RLKS_OK; ++r) {
    g_kernel_events = ev;
    rc = sf_grad(a, GradOpts{});
    g_kernel_events = nullptr;
    if (rc) break;
    if (hipStreamSynchronize(s) != hipSuccess) { rc = fail(RLKS_ERR_HIP, "rlks_ppo_grad_profile: sync"); break; }
    for (int k = 0; k < KEV_N; ++k) {
      float ms = 0.f;
      if (hipEventElapsedTime(&ms, ev[2 * k], ev[2 * k + 1]) == hipSuccess) ms_out[k] += ms / reps;
      else (void)hipGetLastError();  // (an unrecorded pair: clear the error before the next pass's launch checks)
    }
  }
  g_kernel_events = nullptr;
  // the event bracket's own cost: the same start / stop pair around an empty kernel (one wave), read
  // like the others and subtracted from each kernel's figure (ms_out[KEV_N] reports it)
  double ovh = 0.0;
  for (int r = 0; r < reps && rc == RLKS_OK; ++r) {
    hipExtLaunchKernelGGL(k_empty, dim3(1), dim3(64), 0u, s, ev[0], ev[1], 0u);
    if (hipStreamSynchronize(s) != hipSuccess) { rc = fail(RLKS_ERR_HIP, "rlks_ppo_grad_profile: sync"); break; }
    float ms = 0.f;
    if (hipEventElapsedTime(&ms, ev[0], ev[1]) == hipSuccess) ovh += ms / reps;
  }
  for (int k = 0; k < KEV_N; ++k)
    if (ms_out[k] > 0.0) ms_out[k] = ms_out[k] > ovh ? ms_out[k] - ovh : 0.0;
  ms_out[KEV_N] = ovh;
  (void)hipGetLastError();  // (an unrecorded event's elapsed-time query)
  for (int i = 0; i < 2 * KEV_N; ++i) (void)hipEventDestroy(ev[i]);
  return rc;
}

int rlks_adam_step(float* p, const float* g, float* m, float* v, int64_t n, float lr, float beta1, float beta2,
                   float eps, int step, void* stream) {
  RLKS_REQUIRE(step >= 1, RLKS_ERR_ARG, "rlks_adam_step: bad argument");
  return adam_pass(p, const_cast<float*>(g), m, v, n, adam_co(lr, beta1, beta2, eps, step), nullptr, stream);
}

int rlks_ppo_sgd_step_clip(const rlks_mlp_desc* d, const rlks_ppo_coeffs* co, float* params, const float* dyn,
                           const float* mb, int M, float* grad, double* stats, float* adam_m, float* adam_v,
                           int64_t n_params, float lr, float beta1, float beta2, float eps, int step, int prev_fused,
                           float grad_clip, const rlks_gather_next* x, void* workspace, int64_t ws_bytes,
                           void* stream) {
  RLKS_REQUIRE(clip_ok(grad_clip), RLKS_ERR_ARG, "rlks_ppo_sgd_step_clip: grad_clip must be finite and > 0");
  if (int rc = check_desc(d)) return rc;
  RLKS_REQUIRE(n_params == make_layout(d->obs_dim, d->hidden, d->n_actions).padded, RLKS_ERR_ARG,
               "rlks_ppo_sgd_step_clip: n_params must be the padded layout size");
  const FusedAdam fa{params, adam_m, adam_v, adam_co(lr, beta1, beta2, eps, step), step, prev_fused ? 1 : 0, true,
                     n_params, grad_clip};
  return sgd_step_any({d, co, params, dyn, mb, M, grad, stats, workspace, ws_bytes, stream},
                      "rlks_ppo_sgd_step_clip: bad argument", fa, x, 0);
}

int rlks_ppo_sgd_step_next(const rlks_mlp_desc* d, const rlks_ppo_coeffs* co, float* params, const float* dyn,
                           const float* mb, int M, float* grad, double* stats, float* adam_m, float* adam_v,
                           int64_t n_params, float lr, float beta1, float beta2, float eps, int step, int prev_fused,
                           const rlks_gather_next* x, void* workspace, int64_t ws_bytes, void* stream) {
  const FusedAdam fa{params, adam_m, adam_v, adam_co(lr, beta1, beta2, eps, step), step, prev_fused ? 1 : 0, true,
                     n_params};
  return sgd_step_any({d, co, params, dyn, mb, M, grad, stats, workspace, ws_bytes, stream},
                      "rlks_ppo_sgd_step: bad argument", fa, x, 0);
}

int rlks_ppo_sgd_step(const rlks_mlp_desc* d, const rlks_ppo_coeffs* co, float* params, const float* dyn,
                      const float* mb, int M, float* grad, double* stats, float* adam_m, float* adam_v, int64_t n_params,
                      float lr, float beta1, float beta2, float eps, int step, int prev_fused, void* workspace,
                      int64_t ws_bytes, void* stream) {
  return rlks_ppo_sgd_step_next(d, co, params, dyn, mb, M, grad, stats, adam_m, adam_v, n_params, lr, beta1, beta2, eps,
                                step, prev_fused, nullptr, workspace, ws_bytes, stream);
}

// The multi-rank form of rlks_ppo_sgd_step: the gradient (its prep reading the previous step's
// maxima when prev_fused), then, after the caller's all-reduce, Adam as a reduce over one partial
// (the summed gradient) that also leaves the new maxima and the step tag, so no SGD step needs the
// separate weight-max pass.  Same arithmetic as k_adam / the fused reduce: bit-identical parameters.
int rlks_ppo_grad_step_next(const rlks_mlp_desc* d, const rlks_ppo_coeffs* co, const float* params, const float* dyn,
                            const float* mb, int M, float* grad, double* stats, int step, int prev_fused,
                            const rlks_gather_next* x, void* workspace, int64_t ws_bytes, void* stream) {
  return sgd_step_any({d, co, params, dyn, mb, M, grad, stats, workspace, ws_bytes, stream},
                      "rlks_ppo_grad_step: bad argument", grad_only(step, prev_fused), x, 0);
}

int rlks_ppo_grad_step(const rlks_mlp_desc* d, const rlks_ppo_coeffs* co, const float* params, const float* dyn,
                       const float* mb, int M, float* grad, double* stats, int step, int prev_fused, void* workspace,
                       int64_t ws_bytes, void* stream) {
  return rlks_ppo_grad_step_next(d, co, params, dyn, mb, M, grad, stats, step, prev_fused, nullptr, workspace, ws_bytes,
                                 stream);
}

int rlks_ppo_grad_step_part(const rlks_mlp_desc* d, const rlks_ppo_coeffs* co, const float* params, const float* dyn,
                            const float* mb, int M, float* grad, double* stats, int step, int prev_fused, int part,
                            const rlks_gather_next* x, void* workspace, int64_t ws_bytes, void* stream) {
  if (int rc = check_desc(d)) return rc;  // (ahead of the part check, as it always was)
  RLKS_REQUIRE(part == 1 || part == 2, RLKS_ERR_ARG, "rlks_ppo_grad_step_part: part must be 1 or 2");
  return sgd_step_any({d, co, params, dyn, mb, M, grad, stats, workspace, ws_bytes, stream},
                      "rlks_ppo_grad_step_part: bad argument", grad_only(step, prev_fused), x, part);
}

int rlks_ppo_adam_apply(const rlks_mlp_desc* d, float* params, const float* grad, float* adam_m, float* adam_v,
                        int64_t n_params, float lr, float beta1, float beta2, float eps, int step, void* workspace,
                        int64_t ws_bytes, int rows, void* stream) {
  if (int rc = check_desc(d)) return rc;
  RLKS_REQUIRE(params && grad && adam_m && adam_v && workspace && step >= 1, RLKS_ERR_ARG,
               "rlks_ppo_adam_apply: bad argument");
  if (!is_sf(d) || is_wide(d))
    return rlks_adam_step(params, grad, adam_m, adam_v, n_params, lr, beta1, beta2, eps, step, stream);
  RLKS_REQUIRE(n_params == make_layout(d->obs_dim, HID, d->n_actions).padded, RLKS_ERR_ARG,
               "rlks_ppo_adam_apply: n_params must be the padded layout size");
  // one partial, summed in place (each element read and written by one thread)
  return sf_adam_apply(d, params, const_cast<float*>(grad), adam_m, adam_v, adam_co(lr, beta1, beta2, eps, step), step,
                       workspace, ws_bytes, rows, nullptr, (hipStream_t)stream);
}

int rlks_ppo_adam_apply_clip(const rlks_mlp_desc* d, float* params, float* grad, float* adam_m, float* adam_v,
                             int64_t n_params, float lr, float beta1, float beta2, float eps, int step,
                             float grad_clip, double* stats, void* workspace, int64_t ws_bytes, int rows,
                             void* stream) {
  if (int rc = check_desc(d)) return rc;
  RLKS_REQUIRE(params && grad && adam_m && adam_v && workspace && step >= 1, RLKS_ERR_ARG,
               "rlks_ppo_adam_apply_clip: bad argument");
  RLKS_REQUIRE(clip_ok(grad_clip), RLKS_ERR_ARG, "rlks_ppo_adam_apply_clip: grad_clip must be finite and > 0");
  RLKS_REQUIRE(n_params == make_layout(d->obs_dim, d->hidden, d->n_actions).padded, RLKS_ERR_ARG,
               "rlks_ppo_adam_apply_clip: n_params must be the padded layout size");
  NrmWs nw;
  if (int rc = nrm_ws_at(d, rows, workspace, ws_bytes, nw)) return rc;
  hipStream_t s = (hipStream_t)stream;
  // the norm of the (all-reduced) gradient, then Adam on g coef
  if (int rc = norm_pass(d, grad, nw, grad_clip, nullptr, stats, s)) return rc;
  const AdamCo co = adam_co(lr, beta1, beta2, eps, step);
  if (!is_sf(d) || is_wide(d)) return adam_pass(params, grad, adam_m, adam_v, n_params, co, nw.coef, stream);
  return sf_adam_apply(d, params, grad, adam_m, adam_v, co, step, workspace, ws_bytes, rows, nw.coef, s);
}

int rlks_kl_update(float* dyn, const double* kc, float target, void* stream) {
  RLKS_REQUIRE(dyn && kc, RLKS_ERR_ARG, "rlks_kl_update: null argument");
  hipLaunchKernelGGL(k_kl_update, dim3(1), dim3(64), 0, (hipStream_t)stream, dyn, kc, target);
  RLKS_LAUNCHED();
  return RLKS_OK;
}

}  // extern "C"
