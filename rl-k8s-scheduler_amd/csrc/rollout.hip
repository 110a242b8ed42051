// rollout.hip — the rollout host loops (include/rlks.h, section K4): the fp32, split-fp16 and wide
// table rollouts and the node-level rollout, with the optional observation filter between env and policy.
#include "workspace.h"

namespace rlks {

// The env / policy / buffer shape check every rollout branch starts with; `who` is the entry the
// messages name.  need_autoreset: the wide branch checks the lanes' autoreset together with the shapes.
static int check_shapes(const char* who, rlks_env* env, const rlks_mlp_desc* d, const rlks_rollout_bufs* b,
                        bool need_autoreset, rlks_env_cfg& cfg) {
  rlks_env_config(env, &cfg);
  RLKS_REQUIRE(cfg.n_envs == b->N && 3 * cfg.n_clouds == d->obs_dim && cfg.n_clouds == d->n_actions &&
                   (!need_autoreset || cfg.autoreset), RLKS_ERR_ARG,
               std::string(who) + ": env / policy / buffer shapes disagree" +
                   (need_autoreset ? " (autoreset lanes required)" : ""));
  return RLKS_OK;
}

// The argument check before it; need_ws: the branch needs a workspace.
static int check_rollout(const char* who, rlks_env* env, const rlks_mlp_desc* d, const float* params,
                         const rlks_rollout_bufs* b, bool need_ws, const void* workspace, bool need_autoreset,
                         rlks_env_cfg& cfg) {
  RLKS_REQUIRE(env && params && b && b->T > 0 && b->N > 0 && (!need_ws || workspace), RLKS_ERR_ARG,
               std::string(who) + ": bad argument");
  return check_shapes(who, env, d, b, need_autoreset, cfg);
}

// hipDeviceAttributeMaxSharedMemoryPerBlock of the current device, read once (0: the read failed).  The
// forms are chosen against MAX_LDS_BYTES (env_device.h); this figure goes into the over-budget message
static int device_lds_bytes() {
  static const int bytes = [] {
    int dev = 0, v = 0;
    const bool ok = hipGetDevice(&dev) == hipSuccess &&
                    hipDeviceGetAttribute(&v, hipDeviceAttributeMaxSharedMemoryPerBlock, dev) == hipSuccess;
    return ok ? v : 0;
  }();
  return bytes;
}

// The one place that decides a rollout's form (RLKS_ROLLOUT_*): rlks_rollout_form and the
// fp32 and split-fp16 host loops below go through it, and every launch of a fused table rollout kernel
// follows it (the wide branch of rollout_ws returns before it: wide_rollout stages no table).  A fused
// form is taken only while its LDS (sf_roll_lds / fwd_rollout_lds: the launchers' own counts) fits
// MAX_LDS_BYTES.  That test reads the kernels the entry runs, A, the table's size and the autoreset flag
// alone; the lane rules beside it (job_lanes, the 128-row tiles above FWD_SMALL_MAX_ROWS) are the ones that
// were always there.
// sf_kernels: the entry runs the split-fp16 kernels (rollout_ws with a split-fp16 desc); false: the fp32
// kernels, whatever the desc's precision says (rollout_fp32 is rlks_rollout's body, and that entry runs
// k_fwd_head for every fused-width desc).  `tap`: a filtered rollout (per-step on split-fp16 at every lane
// count; on the fp32 kernels the filter stands between the per-step launches of either form).
static int rollout_form(const char* who, const rlks_env_cfg& cfg, const rlks_mlp_desc* d, const rlks_rollout_bufs* b,
                        bool sf_kernels, bool tap, int32_t& form) {
  if (is_wide(d)) return form = RLKS_ROLLOUT_WIDE, RLKS_OK;
  if (cfg.nodes_per_cluster > 0) return form = RLKS_ROLLOUT_NODE, RLKS_OK;
  const int A = d->n_actions, R = cfg.n_rows, C = cfg.n_clouds;
  int64_t need = 0;
  auto over = [&](const char* kernel, int32_t per_step) {
    if (cfg.autoreset) return form = per_step, RLKS_OK;
    return fail(RLKS_ERR_UNSUPPORTED,
                std::string(who) + ": " + kernel + " with this " + std::to_string(R) + " x " + std::to_string(C) +
                    " table asks for " + std::to_string(need) + " B of LDS, the limit is " +
                    std::to_string(MAX_LDS_BYTES) + " B a workgroup (the device reports " +
                    std::to_string(device_lds_bytes()) + " B), and the per-step form needs autoreset lanes");
  };
  if (sf_kernels) {
    // by the whole job's lane count: W ranks of N lanes and one rank of W N lanes (num_lane_groups = W)
    // run the same forward kernel, so their logits, and hence their sampled actions, agree bit for bit
    const int64_t job_lanes = b->global_lanes > 0 ? b->global_lanes : b->N;
    if (tap || (job_lanes > SF_ROLL_FUSED_MAX_LANES && cfg.autoreset)) return form = RLKS_ROLLOUT_SF16_PER_STEP, RLKS_OK;
    if (int rc = sf_roll_lds(A, R, C, &need)) return rc;
    if (need <= MAX_LDS_BYTES) return form = RLKS_ROLLOUT_SF16_PERSISTENT, RLKS_OK;
    return over("the persistent split-fp16 rollout", RLKS_ROLLOUT_SF16_PER_STEP);
  }
  if (b->N > FWD_SMALL_MAX_ROWS) {
    if (int rc = fwd_rollout_lds(A, 128, R, C, &need)) return rc;
    if (need <= MAX_LDS_BYTES) return form = RLKS_ROLLOUT_FP32_FUSED_128, RLKS_OK;
  }
  if (int rc = fwd_rollout_lds(A, 32, R, C, &need)) return rc;
  if (need <= MAX_LDS_BYTES) return form = RLKS_ROLLOUT_FP32_FUSED_32, RLKS_OK;
  return over("the fused fp32 rollout step", RLKS_ROLLOUT_FP32_PER_STEP);
}

// Node-level envs (nodes_per_cluster > 0): the node sweep has its own workgroup shape (k_node_step:
// 64 envs x W waves), so a rollout step is two launches on the stream: forward of both nets on
// obs[t] (logits[t], values[t]) -> the sampling node step (rlks_env_sample_step: actions[t], logp[t],
// obs[t + 1], f32 rewards[t], dones[t]); then the bootstrap V(obs[T]).  `w` = the split-fp16
// weights (SF16) or nullptr (fp32 kernels).
static int node_rollout(const char* who, rlks_env* env, const rlks_env_cfg& cfg, const rlks_mlp_desc* d,
                        const float* params, const rlks_rollout_bufs* b, int explore, const SfWs* w, hipStream_t s,
                        const ObsTap* tap) {
  RLKS_REQUIRE(cfg.autoreset, RLKS_ERR_ARG, std::string(who) + ": node-level rollout needs autoreset lanes");
  const int N = b->N, D = d->obs_dim, A = d->n_actions;
  const Layout L = make_layout(D, HID, A);
  SfFwdArgs r{};
  if (w) {
    if (int rc = sf_prep(d, *w, params, s, true)) return rc;
    sf_nets(r.n, *w, params, L);
    r.M = N; r.D = D;
  }
  auto forward = [&](const float* x, float* logits, float* values) -> int {
    if (!w) return forward_fp32(params, L, x, N, D, A, logits, values, s);
    SfFwdArgs a = r;  // 16-row tiles of both nets (sgd_sf16.hip k_sf_fwd16)
    a.x = x;
    a.out[0] = logits;
    a.out[1] = values;
    return launch_sf_fwd16(a, A, s);
  };
  if (int rc = tap_apply(tap, b, D, 0, s)) return rc;
  for (int t = 0; t < b->T; ++t) {
    const size_t tN = (size_t)t * N;
    if (int rc = forward(b->obs + tN * D, b->logits + tN * A, b->values + tN)) return rc;
    if (env->action_masking) {
      // rlks_env_set_action_masking: the masked draw on logits[t] in place, then the trusted-actions node
      // step: two launches for the sampling node step's one
      if (int rc = rlks_env_masked_sample(env, b->logits + tN * A, explore, b->actions + tN, b->logp + tN, nullptr, s))
        return rc;
      if (int rc = rlks_env_step(env, b->actions + tN, tap_obs_out(tap, b, D, t + 1), nullptr, b->rewards + tN,
                                 b->dones + tN, nullptr, nullptr, nullptr, nullptr, s))
        return rc;
    } else if (int rc = rlks_env_sample_step(env, b->logits + tN * A, explore, b->actions + tN, b->logp + tN,
                                             tap_obs_out(tap, b, D, t + 1), b->rewards + tN, b->dones + tN, s)) {
      return rc;
    }
    if (int rc = tap_apply(tap, b, D, t + 1, s)) return rc;
  }
  return forward(b->obs + (size_t)b->T * N * D, nullptr, b->values + (size_t)b->T * N);
}

// The rollout entries share their host loops; `tap` (obs_filter.h) is rlks_rollout_filtered's filter
// between the env and the policy, nullptr for the unfiltered entries, which then issue exactly the
// launches they always did.
static int rollout_fp32(rlks_env* env, const rlks_mlp_desc* d, const float* params, const rlks_rollout_bufs* b,
                        int explore, const ObsTap* tap, void* stream) {
  if (int rc = check_desc(d)) return rc;
  RLKS_REQUIRE(!is_wide(d), RLKS_ERR_UNSUPPORTED, "rlks_rollout: this MLP / env needs rlks_rollout_ws");
  rlks_env_cfg cfg;
  if (int rc = check_rollout("rlks_rollout", env, d, params, b, false, nullptr, false, cfg)) return rc;
  hipStream_t s = (hipStream_t)stream;
  int32_t form;
  if (int rc = rollout_form("rlks_rollout", cfg, d, b, false, tap != nullptr, form)) return rc;
  if (form == RLKS_ROLLOUT_NODE) return node_rollout("rlks_rollout", env, cfg, d, params, b, explore, nullptr, s, tap);
  const int N = b->N, D = d->obs_dim, A = d->n_actions;
  const Layout L = make_layout(D, d->hidden, A);
  if (int rc = tap_apply(tap, b, D, 0, s)) return rc;
  if (form == RLKS_ROLLOUT_FP32_PER_STEP) {
    // per step: the policy forward, then the fused sample + env step (k_sample_step, auto-reset lanes),
    // whose LDS is the tables alone
    for (int t = 0; t < b->T; ++t) {
      const size_t tN = (size_t)t * N;
      if (int rc = forward_fp32(params, L, b->obs + tN * D, N, D, A, b->logits + tN * A, nullptr, s)) return rc;
      if (int rc = rlks_env_sample_step(env, b->logits + tN * A, explore, b->actions + tN, b->logp + tN,
                                        tap_obs_out(tap, b, D, t + 1), b->rewards + tN, b->dones + tN, s))
        return rc;
      if (int rc = tap_apply(tap, b, D, t + 1, s)) return rc;
    }
  } else {
    // per step: policy forward fused with sampling and the env step (one launch, pi net only)
    const int tile_rows = form == RLKS_ROLLOUT_FP32_FUSED_128 ? 128 : 32;
    FwdArgs f{};
    f.P = net_ptrs_host(params, L, 0);
    f.x_stride = D; f.M = N; f.D = D; f.A_pi = A;
    f.env = view(env); f.tab_cost = env->d_cost; f.tab_lat = env->d_lat; f.explore = explore;
    for (int t = 0; t < b->T; ++t) {
      const size_t tN = (size_t)t * N;
      f.x = b->obs + tN * D; f.out = b->logits + tN * A; f.obs_next = tap_obs_out(tap, b, D, t + 1);
      f.logp = b->logp + tN; f.actions = b->actions + tN; f.rewards = b->rewards + tN; f.dones = b->dones + tN;
      if (int rc = launch_fwd_rollout(f, A, tile_rows, s)) return rc;
      if (int rc = tap_apply(tap, b, D, t + 1, s)) return rc;
    }
  }
  // values of every visited observation (incl. the bootstrap obs[T]) in one batched pass
  return forward_fp32(params, L, b->obs, (b->T + 1) * N, D, A, nullptr, b->values, s);
}

static int rollout_ws(rlks_env* env, const rlks_mlp_desc* d, const float* params, const rlks_rollout_bufs* b,
                      int explore, void* workspace, int64_t ws_bytes, const ObsTap* tap, void* stream) {
  if (int rc = check_desc(d)) return rc;
  rlks_env_cfg cfg;
  if (is_wide(d)) {
    if (int rc = check_rollout("rlks_rollout_ws", env, d, params, b, true, workspace, true, cfg)) return rc;
    const WideWs w = wide_ws_layout(d->obs_dim, d->hidden, d->n_actions, b->N, (char*)workspace);
    RLKS_REQUIRE(ws_bytes >= w.bytes, RLKS_ERR_ARG, "rlks_rollout_ws: workspace too small");
    return wide_rollout(env, d, params, b, explore, w, (hipStream_t)stream, tap);
  }
  if (!is_sf(d)) return rollout_fp32(env, d, params, b, explore, tap, stream);
  if (int rc = check_rollout("rlks_rollout_ws", env, d, params, b, true, workspace, false, cfg)) return rc;
  const int N = b->N, D = d->obs_dim, A = d->n_actions;
  const SfWs w = sf_ws_layout(D, A, 0, (char*)workspace);
  RLKS_REQUIRE(ws_bytes >= w.weight_bytes, RLKS_ERR_ARG, "rlks_rollout_ws: workspace too small");
  hipStream_t s = (hipStream_t)stream;
  int32_t form;
  if (int rc = rollout_form("rlks_rollout_ws", cfg, d, b, true, tap != nullptr, form)) return rc;
  if (form == RLKS_ROLLOUT_NODE) return node_rollout("rlks_rollout_ws", env, cfg, d, params, b, explore, &w, s, tap);
  RLKS_REQUIRE(!tap || cfg.autoreset, RLKS_ERR_ARG, "rlks_rollout_filtered: autoreset lanes required");
  if (int rc = sf_prep(d, w, params, s, true)) return rc;
  const Layout L = make_layout(D, HID, A);
  if (form == RLKS_ROLLOUT_SF16_PER_STEP) {
    // per step: the 16-row forward of both nets (k_sf_fwd16), then the fused sample + env step
    // (k_sample_step, auto-reset lanes); V(obs[T]) by one more forward.  Filtered rollouts take this
    // branch at every lane count: the persistent kernel below reads and writes one buffer inside a
    // single launch, so no filter can stand between its env and its forward
    SfFwdArgs f{};
    sf_nets(f.n, w, params, L);
    f.M = N; f.D = D;
    if (int rc = tap_apply(tap, b, D, 0, s)) return rc;
    for (int t = 0; t <= b->T; ++t) {
      const size_t tN = (size_t)t * N;
      f.x = b->obs + tN * D;
      f.out[0] = t < b->T ? b->logits + tN * A : nullptr;
      f.out[1] = b->values + tN;
      if (int rc = launch_sf_fwd16(f, A, s)) return rc;
      if (t == b->T) break;
      if (int rc = rlks_env_sample_step(env, b->logits + tN * A, explore, b->actions + tN, b->logp + tN,
                                        tap_obs_out(tap, b, D, t + 1), b->rewards + tN, b->dones + tN, s))
        return rc;
      if (int rc = tap_apply(tap, b, D, t + 1, s)) return rc;
    }
    return RLKS_OK;
  }
  SfRollArgs a{};
  for (int net = 0; net < 2; ++net) {
    const NetPtrs P = net_ptrs_host(params, L, net);
    a.n[net] = SfRollNet{w.w[net].w1h, w.w[net].w1l, w.w[net].w2rh, w.w[net].w2rl, P.b2, P.w3, P.b3, w.w[net].sc};
  }
  a.M = N; a.D = D; a.A = A; a.T = b->T;
  a.env = view(env); a.tab_cost = env->d_cost; a.tab_lat = env->d_lat; a.explore = explore;
  // one launch: per step both nets' forward of obs[t] (logits[t], values[t]), sample, env step ->
  // obs[t + 1]; step T writes the bootstrap V(obs[T])
  a.x = b->obs; a.logits = b->logits; a.values = b->values; a.logp = b->logp;
  a.actions = b->actions; a.rewards = b->rewards; a.dones = b->dones;
  return launch_sf_roll(a, s);
}

}  // namespace rlks

using namespace rlks;

extern "C" {

int rlks_rollout(rlks_env* env, const rlks_mlp_desc* d, const float* params, const rlks_rollout_bufs* b,
                 int explore, void* stream) {
  return rollout_fp32(env, d, params, b, explore, nullptr, stream);
}

int rlks_rollout_ws(rlks_env* env, const rlks_mlp_desc* d, const float* params, const rlks_rollout_bufs* b,
                    int explore, void* workspace, int64_t ws_bytes, void* stream) {
  return rollout_ws(env, d, params, b, explore, workspace, ws_bytes, nullptr, stream);
}

int rlks_rollout_filtered(rlks_env* env, const rlks_mlp_desc* d, const float* params, const rlks_rollout_bufs* b,
                          int explore, void* workspace, int64_t ws_bytes, const double* state, float* raw,
                          void* stream) {
  RLKS_REQUIRE(state && raw && d && b && b->obs, RLKS_ERR_ARG, "rlks_rollout_filtered: null argument");
  if (int n = rlks_obs_filter_size(d->obs_dim); n < 0) return n;
  const ObsTap tap{state, raw};
  return rollout_ws(env, d, params, b, explore, workspace, ws_bytes, &tap, stream);
}

int rlks_rollout_form(rlks_env* env, const rlks_mlp_desc* d, const rlks_rollout_bufs* b, int32_t* form) {
  RLKS_REQUIRE(env && d && b && form && b->N > 0, RLKS_ERR_ARG, "rlks_rollout_form: bad argument");
  if (int rc = check_desc(d)) return rc;
  rlks_env_cfg cfg;
  if (int rc = check_shapes("rlks_rollout_form", env, d, b, is_wide(d), cfg)) return rc;
  return rollout_form("rlks_rollout_form", cfg, d, b, is_sf(d), false, *form);
}

int rlks_rollout_lds_bytes(const rlks_mlp_desc* d, int32_t form, int32_t n_rows, int32_t n_clouds, int64_t* bytes) {
  RLKS_REQUIRE(d && bytes && n_rows > 0 && n_clouds > 0, RLKS_ERR_ARG, "rlks_rollout_lds_bytes: bad argument");
  if (int rc = check_desc(d)) return rc;
  switch (form) {
    case RLKS_ROLLOUT_SF16_PERSISTENT: return sf_roll_lds(d->n_actions, n_rows, n_clouds, bytes);
    case RLKS_ROLLOUT_FP32_FUSED_32: return fwd_rollout_lds(d->n_actions, 32, n_rows, n_clouds, bytes);
    case RLKS_ROLLOUT_FP32_FUSED_128: return fwd_rollout_lds(d->n_actions, 128, n_rows, n_clouds, bytes);
    default: return fail(RLKS_ERR_UNSUPPORTED, "rlks_rollout_lds_bytes: not a fused table rollout form");
  }
}

}  // extern "C"
