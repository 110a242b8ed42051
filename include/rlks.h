/*
 * rlks.h — C ABI of librlks.so, the MI355X (gfx950) rollout-and-training engine for the
 * rl_scheduler multi-cloud pod scheduler.
 *
 * Drop-in boundary.  The reference's hot path sits behind the gymnasium Env API
 * (K8sMultiCloudEnv, /root/reference/rl_scheduler/env/k8s_multi_cloud_env.py:36-157) and behind
 * RLlib's PPO Algorithm surface (train(), compute_single_action(), save()/from_checkpoint(),
 * /root/reference/rl_scheduler/agent/train_ppo.py:9-31, eval_ppo.py:17-27,
 * final_evaluation.py:32-48).  The Python host package (rl-k8s-scheduler_amd/rlks) keeps that
 * surface and binds the entry points below with ctypes; INTEGRATION.md shows the binding.
 *
 * Conventions
 *  - Every function returns 0 (RLKS_OK) or a negative RLKS_ERR_* code; rlks_last_error() gives
 *    the message (thread-local).
 *  - Pointers named *_dev are device (HBM) pointers owned by the caller (torch tensors);
 *    *_host pointers are host memory.  `stream` is a hipStream_t (NULL = legacy default stream).
 *  - All device work is enqueued asynchronously on `stream`; no function synchronises the
 *    device except rlks_env_create/destroy, so every call can be captured in a hipGraph.
 *  - Handles are not re-entrant: one handle per GPU per host thread.
 */
#ifndef RLKS_H
#define RLKS_H

#include <stddef.h>
#include <stdint.h>

#include "rlks_types.h"

#ifdef __cplusplus
extern "C" {
#endif

#define RLKS_OK 0
#define RLKS_ERR_ARG (-1)
#define RLKS_ERR_HIP (-2)
#define RLKS_ERR_UNSUPPORTED (-3)
#define RLKS_ERR_STATE (-4)

const char* rlks_last_error(void);
const char* rlks_version(void);

/* Debug build only (make -C csrc debug -> librlks_debug.so): device-side bounds checks that count
 * instead of faulting.  out[3] = {violations since the last call, first site (rlks_internal.h
 * DcheckSite), its value}; synchronises the device and clears the counters.  RLKS_ERR_UNSUPPORTED
 * in the product library. */
int rlks_debug_checks(unsigned long long* out);

/* ============================================================== environment (K1 + K2) ==== */
typedef struct rlks_env rlks_env;

/* K8sMultiCloudEnv.__init__ (:46-66): tables are [n_rows][n_clouds] float64 host arrays with the
 * exact bits pandas parsed from data/processed/normalized_rl_data.csv (:58).  Allocates the SoA
 * lane state (step, episode, optional MT19937 state) in HBM.  Synchronises. */
int rlks_env_create(const rlks_env_cfg* cfg, const double* cost_host, const double* lat_host,
                    rlks_env** out);
/* Same, with the node-level extension when cfg->nodes_per_cluster > 0: node_cpu_m
 * and node_mem_mi are per-cluster node capacities [n_clouds]; arrival_trace [n_trace] gives the
 * per-step Poisson rate for arrival_mode 1 (bursty), indexed by step mod n_trace. */
int rlks_env_create_ext(const rlks_env_cfg* cfg, const double* cost_host, const double* lat_host,
                        const int32_t* node_cpu_m_host, const int32_t* node_mem_mi_host,
                        const double* arrival_trace_host, int n_trace, rlks_env** out);
int rlks_env_destroy(rlks_env* env);
int rlks_env_config(const rlks_env* env, rlks_env_cfg* out);

/* random.seed(seed) (:109-110) for the lanes in mask (NULL = all), MT19937 mode only:
 * keys_dev[lane * key_stride + j] are the 32-bit words of abs(seed), little-endian (CPython
 * random_seed); keylen_dev[lane] is the word count (>= 1). */
int rlks_env_seed(rlks_env* env, const uint8_t* mask_dev, const uint32_t* keys_dev,
                  const int32_t* keylen_dev, int key_stride, void* stream);

/* Advance each masked lane's MT19937 stream by n_draws_dev[lane] random() calls (int64 per lane;
 * MT19937 mode only).  Batched evaluation uses it to give lane e the stream position of episode e
 * of the reference's sequential loop (final_evaluation.py:42-49, one process-global generator). */
int rlks_env_mt_discard(rlks_env* env, const uint8_t* mask_dev, const int64_t* n_draws_dev, void* stream);
/* Lane's MT19937 state as CPython's random.getstate()[1] lays it out: 624 words then the position
 * (0..624), copied to (to_env = 0) or from (to_env = 1) words_dev[625] (MT19937 mode only).  The
 * drop-in env's "global" noise stream keeps the lane in step with the process-global `random`
 * module this way: the reference draws its cpu noise from it (k8s_multi_cloud_env.py:87) and
 * reseeds it in reset (:109-111). */
int rlks_env_mt_words(rlks_env* env, int lane, uint32_t* words_dev, int to_env, void* stream);

/* reset() (:106-112) for the lanes in mask (NULL = all): current_step = 0, obs of row 0. */
int rlks_env_reset(rlks_env* env, const uint8_t* mask_dev, float* obs_dev, void* stream);

/* step(action) (:115-144) for all lanes.  status_dev[0] = invalid actions (when > 0 NO lane
 * steps: the reference asserts before any change, :116); status_dev[1] = lanes that ran past the
 * last table row (the reference's IndexError, :91).  reward64 is bit-exact f64 (no FMA);
 * reward32 its f32 rounding; one of the two reward pointers, truncated, step_out and final_obs
 * may be NULL.  Node-level envs (nodes_per_cluster > 0)
 * run the node sweep (departures, arrivals, first-fit) in the same call.
 * status_dev == NULL declares the actions trusted (produced by rlks sampling): no validation
 * launch and no status report. */
int rlks_env_step(rlks_env* env, const int32_t* actions_dev, float* obs_dev, double* reward64_dev,
                  float* reward32_dev, uint8_t* terminated_dev, uint8_t* truncated_dev,
                  int32_t* step_out_dev, float* final_obs_dev, int32_t* status_dev, void* stream);

/* Fused action sampling + step for the rollout (RLlib sampler + TorchCategorical): action =
 * Categorical(logits) via Philox (explore != 0) or argmax (explore == 0, compute_single_action
 * explore=False); logp of the chosen action; env step; auto-reset; episode-return tracking.
 * logits_dev is [n_envs][n_clouds] (row stride n_clouds); lane i's draw is Philox4x32-10 of the
 * counter {env_offset + i, episode[i], step[i], RLKS_PURPOSE_ACTION << 16} under the env's seed,
 * with the episode and step the lane has before the step: the same actions and logp, bit for bit,
 * as rlks_sample_categorical with those ids followed by rlks_env_step(status = NULL).
 * Table and node-level envs alike, one launch each: a node-level env (nodes_per_cluster > 0) runs
 * the sampling form of the node step rlks_env_step would dispatch to, with its
 * episode log, counters and auto-reset.  reward_dev is the f32 reward, done_dev = terminated,
 * obs_next_dev the next observation (the next episode's first one on auto-reset).  A lane past the
 * last table row still gets its action and logp, reward 0, done 0 and no observation.
 * The env must have autoreset lanes (RLKS_ERR_STATE otherwise); every pointer is required
 * (RLKS_ERR_ARG).  Asynchronous on `stream` and capturable. */
int rlks_env_sample_step(rlks_env* env, const float* logits_dev, int explore, int32_t* actions_dev,
                         float* logp_dev, float* obs_next_dev, float* reward_dev, uint8_t* done_dev,
                         void* stream);

/* Baseline schedulers: actions_dev[lane] = the cluster rule `rule` (RLKS_RULE_*)
 * picks for each lane from what a scheduler sees before the step: the lane's observation row
 * obs_dev[lane][3 n_clouds] = [cost, lat, util] (normally the env's current observation), its step
 * and episode counters, the env's constants and, on a node-level env, its clusters' used millicores.
 *   ROUND_ROBIN       step % C
 *   CHEAPEST          lowest index of the minimum f32 obs[c]
 *   MYOPIC            lowest index of the maximum (strict >) of s_c = w_cost * (double)obs[c] +
 *                     w_lat * (double)obs[C + c], in f64 with the products and the sum rounded separately:
 *                     the cluster of the largest immediate reward, as far as the f32 observation shows it
 *   LEAST_LOADED      lowest index of the minimum f32 obs[2C + c]
 *   MYOPIC_WITH_ROOM  MYOPIC over the clusters that can take one more pod, used_cpu[c] / pod_cpu_m <
 *                     nodes_per_cluster * min(node_cpu[c] / pod_cpu_m, node_mem[c] / pod_mem_mi) in integers
 *                     (a cluster's nodes are equally sized: some node has room); over all clusters when
 *                     none has room; on a table env every cluster has room
 *   RANDOM            the action rlks_sample_categorical draws from an all-zero logits row with ids
 *                     {env_offset + lane, episode, step} under the env's seed.  This is
 *                     rlks_env_sample_step's counter: a lane must not use both for the same step, or
 *                     the two draws are one.
 * All rules are exact.  A lane past the last table row is decided like any other.  Table and node-level
 * envs, any n_clouds, with or without autoreset.  One launch, asynchronous on `stream` and capturable:
 * no validation launch, no host read.  A NULL pointer or an unknown rule: RLKS_ERR_ARG. */
int rlks_env_rule_actions(rlks_env* env, int rule, const float* obs_dev, int32_t* actions_dev, void* stream);

/* TorchCategorical sample (explore != 0) or argmax of rows i < n of logits_dev[n][A]: the draw of
 * row i is Philox4x32-10 of the counter {ids[3i], ids[3i + 1], ids[3i + 2], RLKS_PURPOSE_ACTION << 16}
 * under key = seed, turned into an action exactly as rlks_env_sample_step does (ids may be NULL
 * when explore = 0); logp_dev (may be NULL) gets log pi(action).  compute_single_action(obs) with
 * exploration (eval_ppo.py:27) keys its draw by (config seed, call counter). */
int rlks_sample_categorical(const float* logits_dev, int n, int A, const uint32_t* ids_dev, unsigned long long seed,
                            int explore, int32_t* actions_dev, float* logp_dev, void* stream);

/* ---- invalid-action masking (room(), mask() and the sentinel: rlks_types.h).  Every entry
 * is asynchronous on `stream`, reads nothing on the host and is capturable.  n_clouds (or A) > 64:
 * RLKS_ERR_UNSUPPORTED; a NULL required pointer: RLKS_ERR_ARG.
 *
 * rlks_env_action_mask: mask_dev[lane] = mask(lane) for every lane, table and node-level envs alike. */
int rlks_env_action_mask(rlks_env* env, uint64_t* mask_dev, void* stream);
/* One launch: computes the lane's mask, overwrites logits_dev[lane][c] (in/out, [n_envs][n_clouds]) of the
 * clusters without room with RLKS_MASKED_LOGIT, then draws the action from the masked row with
 * rlks_env_sample_step's arithmetic and Philox counter {env_offset + lane, episode, step,
 * RLKS_PURPOSE_ACTION << 16} under the env's key (explore != 0) or takes the argmax, lowest index of the
 * maximum (explore == 0); logp_dev = log pi(action) of the masked distribution; mask_out_dev (may be NULL)
 * gets the mask.  The env is not stepped: follow with rlks_env_step(status = NULL).  One difference from the
 * unmasked draw: when no cumulative entry exceeds u (f32(u53) rounds to 1.0, about 2^-25 of the draws) the
 * action is the highest-index unmasked cluster, not n_clouds - 1.  When every cluster has room, logits,
 * actions and logp are bit for bit rlks_env_sample_step's. */
int rlks_env_masked_sample(rlks_env* env, float* logits_dev, int explore, int32_t* actions_dev, float* logp_dev,
                           uint64_t* mask_out_dev, void* stream);
/* The same draw under the caller's masks mask_dev[n] (bit a set = action a allowed) with
 * rlks_sample_categorical's counter convention; logits_dev[n][A] is masked in place.  A row whose mask has
 * no bit among the low A is treated as unmasked (the masks live on the device: rejecting such a row would
 * cost a host read). */
int rlks_sample_categorical_masked(float* logits_dev, const uint64_t* mask_dev, int n, int A, const uint32_t* ids_dev,
                                   unsigned long long seed, int explore, int32_t* actions_dev, float* logp_dev,
                                   void* stream);
/* on != 0: the rollouts of a node-level env (rlks_rollout, rlks_rollout_ws, rlks_rollout_filtered) run, per
 * step, the forward, rlks_env_masked_sample on bufs->logits[t] in place and rlks_env_step with trusted
 * actions instead of the forward and rlks_env_sample_step: the same number of launches; bufs->logits then
 * holds the masked rows, which the gather and pack kernels carry into the minibatch records unchanged and
 * the loss heads recognise (rlks_ppo_grad below).  The flag is read when a rollout is enqueued.  A table
 * env: RLKS_ERR_UNSUPPORTED. */
int rlks_env_set_action_masking(rlks_env* env, int on);

/* Sum of completed-episode returns and their count over all lanes (double[2]); clear != 0
 * zeroes the accumulators (PPO result "episode_reward_mean", train_ppo.py:29-30). */
int rlks_env_episode_stats(rlks_env* env, double* out_dev, int clear, void* stream);

/* Completed-episode log since the last clear: returns_dev[RLKS_EPLOG_CAP] (float64) and
 * keys_dev[RLKS_EPLOG_CAP] (int64: episode << 32 | global lane) of the first RLKS_EPLOG_CAP
 * episodes, count_dev[0] (uint32) = all episodes completed (may exceed the capacity).  Sorting by
 * key gives completion order.  Feeds RLlib's 100-episode smoothing of episode_reward_mean
 * (metrics_num_episodes_for_smoothing; train_ppo.py:29-30 prints it).  Any pointer may be NULL. */
int rlks_env_episode_log(rlks_env* env, double* returns_dev, long long* keys_dev, unsigned* count_dev,
                         int clear, void* stream);

/* Snapshot of every per-lane state a resumed run needs (step / episode counters, episode returns,
 * MT19937 words, node free cpu / mem and per-cluster used cpu): rlks_env_state_bytes gives the
 * size; save / load copy it to / from a device buffer of that size, asynchronously on `stream`.
 * Checkpoint / resume (agent.save() each iteration, train_ppo.py:31;
 * PPO.from_checkpoint, eval_ppo.py:17).  Philox draws are keyed by (lane, episode, step), so the
 * counters restore the random streams too. */
int rlks_env_state_bytes(const rlks_env* env, int64_t* bytes);
int rlks_env_save_state(const rlks_env* env, void* dst_dev, void* stream);
int rlks_env_load_state(rlks_env* env, const void* src_dev, void* stream);

/* node-level extension: free millicores / MiB per node as [n_envs][n_clouds][nodes] and the
 * per-cluster used millicores [n_envs][n_clouds] (any pointer may be NULL) */
int rlks_env_node_state(rlks_env* env, int32_t* free_cpu_dev, int32_t* free_mem_dev, int32_t* used_cpu_dev,
                        void* stream);
/* node counters {node checks by first fit, pods placed, pods rejected, pods departed, node
 * write-backs, node reads} (u64[6]) copied to out_dev when non-NULL; enable = 1 / 0 turns counting on (zeroed) / off, -1
 * leaves it unchanged.  The flag is read when a step is launched (a captured graph keeps it). */
int rlks_env_counters(rlks_env* env, int enable, unsigned long long* out_dev, void* stream);

/* copy lane counters (current_step, episode index) into caller buffers (either may be NULL) */
int rlks_env_lane_state(rlks_env* env, int32_t* steps_dev, int32_t* episodes_dev, void* stream);

/* ============================================================== RNG test surface ========= */
/* Philox4x32-10 of n counters ctr_dev[n][4] under key_dev[2] -> out_dev[n][4] */
int rlks_philox4x32_10(const uint32_t* ctr_dev, const uint32_t* key_dev, uint32_t* out_dev, int n,
                       void* stream);
/* n draws of CPython random.random() after random.seed(key words) -> out_dev[n] (one lane) */
int rlks_mt_random(const uint32_t* key_dev, int keylen, double* out_dev, int n, void* stream);

/* ============================================================== advantages (K3) ========== */
/* RLlib compute_advantages (use_gae=True) over a time-major [T][N] rollout:
 *   delta_t = r_t + gamma * V_{t+1} * (1 - done_t) - V_t,  A_t = delta_t + gamma*lam*(1-done_t)*A_{t+1}
 *   vtarg_t = A_t + V_t;  values_dev is [T+1][N] (row T = bootstrap V(s_T)).
 * partials_dev (may be NULL) receives per-block [sum A, sum A^2] for standardisation. */
int rlks_gae(const float* rewards_dev, const float* values_dev, const uint8_t* dones_dev, float gamma,
             float lam, int T, int N, float* adv_dev, float* vtarg_dev, double* partials_dev,
             void* stream);
int rlks_gae_partials_count(int N);
/* sums_dev[3] = {sum A, sum A^2, count} from the partials (deterministic order) */
int rlks_adv_stats(const double* partials_dev, int n_partials, double count, double* sums_dev,
                   void* stream);
/* dyn_dev[ADV_MEAN], dyn_dev[ADV_INVSTD] from (possibly all-reduced) sums (numpy std, ddof=0) */
int rlks_adv_finalize(const double* sums_dev, float* dyn_dev, void* stream);

/* ============================================================== policy / value MLP (K4) == */
/* Flat parameter buffer layout (fp32, torch [out][in] weights, each tensor 64-float aligned).
 * Tensor indices (offsets12[i]):
 *   0 pi.w1 [H][D]  1 pi.b1 [H]  2 pi.w2 [H][H]  3 pi.b2 [H]  4 pi.w3 [A][H]  5 pi.b3 [A]
 *   6 vf.w1 [H][D]  7 vf.b1 [H]  8 vf.w2 [H][H]  9 vf.b2 [H] 10 vf.w3 [1][H] 11 vf.b3 [1]
 * stored in the order 0 1 6 7 2 3 4 5 8 9 10 11 (both nets' first layers first: the two gradient
 * buckets of rlks_ppo_grad_step_part are [0, offsets12[2]) and [offsets12[2], padded)).
 * (RLlib FCNet with vf_share_layers=False: _hidden_layers/_logits/_value_branch_separate/
 *  _value_branch.) */
#define RLKS_N_TENSORS 12
int rlks_mlp_layout(const rlks_mlp_desc* desc, int64_t* offsets12, int64_t* padded_count,
                    int64_t* real_count);

/* logits_dev[n][A], values_dev[n] = FCNet forward of obs_dev[n][D] (either output may be NULL) */
int rlks_policy_forward(const rlks_mlp_desc* desc, const float* params_dev, const float* obs_dev,
                        int n, float* logits_dev, float* values_dev, void* stream);

/* ---- serving: one launch from n raw observations to decisions.
 * one launch: raw obs -> (filter) -> policy MLP -> (mask) -> argmax / Categorical draw -> probs; optionally the value.
 * Every pointer is one the device can dereference: device memory or rlks_host_alloc'd memory.
 *   filter_state  NULL, or an rlks_obs_filter state for obs_dim columns: every loaded element goes through
 *                 rlks_obs_filter_apply's arithmetic first (the same bits)
 *   mask          NULL, or uint64_t[n], bit a set = action a allowed, with rlks_sample_categorical_masked's
 *                 rules (a row without a bit among the low A counts as unmasked; masked logits become
 *                 RLKS_MASKED_LOGIT)
 *   the draw      row i: rlks_sample_categorical[_masked] on the row's logits with ids {sampler_id, i, call}
 *                 under key = seed, bit for bit (explore = 0: the argmax, lowest index of the maximum)
 *   outputs       actions[n] (required); any of logp[n] = log pi(action), logits[n][A] = the row as drawn
 *                 from, probs[n][A] = its softmax (exact zeros where masked), values[n] may be NULL; the
 *                 value net runs only when values is given
 * What is written for row i depends on that row, the parameters, the filter state, its mask word and (when
 * exploring) seed, call and i alone: not on n nor on the other rows.  No atomics: the same bits on every run.
 * Scope: hidden 256, 1 <= obs_dim <= 192, 1 <= n_actions <= 64; anything else RLKS_ERR_UNSUPPORTED (use
 * rlks_policy_forward[_ws] + rlks_sample_categorical).  A null desc, params, obs or actions, n < 0 or a
 * misaligned pointer (params 16 bytes, floats 4, filter state and mask 8): RLKS_ERR_ARG.  Errors are found
 * before any HIP call; n == 0 returns RLKS_OK without a launch.  Asynchronous on `stream`, capturable. */
int rlks_policy_act(const rlks_mlp_desc* desc, const float* params_dev, const double* filter_state /* NULL */,
                    const float* obs, const uint64_t* mask /* NULL */, int n, int explore,
                    unsigned long long seed, uint32_t sampler_id, uint32_t call,
                    int32_t* actions, float* logp, float* logits, float* probs, float* values, void* stream);
/* device-visible pinned host memory (hipHostMalloc mapped + hipHostGetDevicePointer) for zero-copy staging */
int rlks_host_alloc(size_t bytes, void** host_ptr, void** dev_ptr);
int rlks_host_free(void* host_ptr);

/* Rollout buffers, time-major, device pointers */
typedef struct rlks_rollout_bufs {
  float* obs;       /* [T+1][N][D] */
  float* logits;    /* [T][N][A] */
  float* values;    /* [T+1][N] */
  int32_t* actions; /* [T][N] */
  float* logp;      /* [T][N] */
  float* rewards;   /* [T][N] */
  uint8_t* dones;   /* [T][N] */
  float* adv;       /* [T][N] */
  float* vtarg;     /* [T][N] */
  int32_t T;
  int32_t N;
  int32_t global_lanes; /* lanes of the whole data-parallel job (0: N).  The split-fp16 rollout picks
                           its forward kernel from this count, not from N, so that a lane's rollout
                           does not depend on how the job's lanes are split over ranks. */
} rlks_rollout_bufs;

/* T steps of (policy forward -> sample -> env step) into bufs, then the bootstrap values
 * V(obs[T]).  obs[0] must hold the current observations.  On every rollout path (this one,
 * rlks_rollout_ws at any precision and lane count, node-level or table env) actions[t] and logp[t] are
 * bit for bit what rlks_sample_categorical gives for logits[t] and the lanes' own counters (global lane,
 * episode, step), or rlks_sample_categorical_masked with the lanes' room masks under action masking:
 * one draw function serves all of them. */
int rlks_rollout(rlks_env* env, const rlks_mlp_desc* desc, const float* params_dev,
                 const rlks_rollout_bufs* bufs, int explore, void* stream);
/* Policy / value forward with a workspace (rlks_ppo_workspace_bytes for >= n rows): required for
 * the generic-width path (RLKS_PRECISION_WIDE or shapes outside the fused kernels). */
int rlks_policy_forward_ws(const rlks_mlp_desc* desc, const float* params_dev, const float* obs_dev, int n,
                           float* logits_dev, float* values_dev, void* workspace, int64_t ws_bytes, void* stream);
/* Generic split-fp16 GEMM of the wide-MLP path (config c5); see rlks_gemm_desc. */
int rlks_gemm_sf16(const rlks_gemm_desc* desc, void* stream);
/* atomicMax of max |x| over x[rows][cols] (row stride ld) into *slot (caller zeroes the slot). */
int rlks_absmax(const float* x, int rows, int cols, int ld, uint32_t* slot, void* stream);
/* Same rollout; with desc->precision == RLKS_PRECISION_SF16 it runs the split-fp16 step kernel
 * (both nets' forward + sample + env step per launch, values written per step, V(obs[T]) last)
 * with the split weights in `workspace` (an rlks_ppo_workspace_bytes-sized buffer: the SGD step's
 * workspace can be shared).  Other precisions fall through to rlks_rollout.  actions and logp are
 * rlks_sample_categorical's on the stored logits here too (see rlks_rollout). */
int rlks_rollout_ws(rlks_env* env, const rlks_mlp_desc* desc, const float* params_dev,
                    const rlks_rollout_bufs* bufs, int explore, void* workspace, int64_t ws_bytes,
                    void* stream);
/* The form (RLKS_ROLLOUT_*) rlks_rollout_ws runs for this env, policy and buffers: a host query, nothing is
 * launched.  The rollout entries decide with the same function, so the answer is what they run.  rlks_rollout
 * runs the fp32 kernels for every desc of the fused widths, whatever its precision: its form is the one this
 * query names for the same desc with RLKS_PRECISION_FP32.  A table
 * env's fused forms are taken only while their LDS (own buffers + both tables) fits a workgroup's 160 KiB;
 * that part of the choice depends on the kernels the entry runs, n_actions, the table's size and the env's autoreset
 * flag alone, so the ranks of one job resolve alike.  The per-step forms need autoreset lanes: without
 * them an over-budget shape is RLKS_ERR_UNSUPPORTED, the message naming the bytes asked and the limit. */
int rlks_rollout_form(rlks_env* env, const rlks_mlp_desc* desc, const rlks_rollout_bufs* bufs, int32_t* form);
/* LDS bytes per workgroup of the fused rollout kernel of `form` (RLKS_ROLLOUT_SF16_PERSISTENT,
 * RLKS_ROLLOUT_FP32_FUSED_32 / _128) with a table env of n_rows x n_clouds: its launcher's dynamic bytes plus
 * the static bytes hipFuncGetAttributes reports. */
int rlks_rollout_lds_bytes(const rlks_mlp_desc* desc, int32_t form, int32_t n_rows, int32_t n_clouds,
                           int64_t* bytes);

/* Minibatch rows per packed record: [obs D | logits_old A | adv | vtarg | logp_old | action] */
int rlks_minibatch_stride(const rlks_mlp_desc* desc);
/* Gather minibatch rows [row0, row0+rows) of epoch `epoch`'s permutation of the T*N samples
 * (Philox-keyed Feistel bijection, no sort) into mb_dev; advantages standardised with dyn. */
int rlks_ppo_gather(const rlks_mlp_desc* desc, const rlks_rollout_bufs* bufs, uint64_t perm_seed,
                    int epoch, int64_t row0, int rows, const float* dyn_dev, float* mb_dev,
                    void* stream);
/* Same over `groups` equal blocks of lanes (global block ids group0 .. group0 + groups - 1): block
 * k has its own permutation of its T * (N / groups) samples and supplies rows / groups rows of every
 * minibatch (rows [k rows/groups, (k+1) rows/groups) of mb_dev, row0 / groups onwards in its
 * order).  A run on W ranks with one block each then draws exactly the minibatches of a
 * single-rank run over all lanes with W blocks: training is independent of the world size up to
 * fp32 summation order.  groups (<= 64) must divide N, rows and row0.  groups = 1, group0 = 0 is
 * rlks_ppo_gather. */
int rlks_ppo_gather_grouped(const rlks_mlp_desc* desc, const rlks_rollout_bufs* bufs, uint64_t perm_seed,
                            int epoch, int groups, int group0, int64_t row0, int rows, const float* dyn_dev,
                            float* mb_dev, void* stream);
/* Floats per sample record of rlks_ppo_pack: the minibatch record padded to a 64-byte multiple
 * (16 / 32 / 48 for obs 6 / 12 / 24); 0 for shapes the packed path does not cover. */
int rlks_packed_stride(const rlks_mlp_desc* desc);
/* The rollout's T*N samples as records [T*N][rlks_packed_stride] in rollout order (after GAE):
 * one aligned record per sample, so that each minibatch row is one random line read. */
int rlks_ppo_pack(const rlks_mlp_desc* desc, const rlks_rollout_bufs* bufs, float* packed_dev, void* stream);
/* rlks_ppo_gather_grouped from packed records: the same rows, permutation and record bytes. */
int rlks_ppo_gather_packed(const rlks_mlp_desc* desc, const float* packed_dev, int T, int N, uint64_t perm_seed,
                           int epoch, int groups, int group0, int64_t row0, int rows, float* mb_dev, void* stream);

/* Gradient of the RLlib PPO loss (mean over `rows`*world rows via dyn[INV_COUNT]) w.r.t. the
 * flat parameters -> grad_dev (padded_count floats).  stats_dev (double[RLKS_STAT_SIZE]) gets
 * the sums for reporting and the KL update.  workspace from rlks_ppo_workspace_bytes (the gradient's
 * scratch for `rows` rows, then the gradient-clipping entry points' norm scratch).
 * Masked actions (rlks_env_masked_sample): where a record's old logit is <= RLKS_MASKED_LOGIT_MAX, the
 * policy heads use that old logit in place of the network's output for the action, so its probability,
 * KL, entropy and gradient terms are exact zeros.  A record without such an entry is computed as ever. */
int rlks_ppo_workspace_bytes(const rlks_mlp_desc* desc, int rows, int64_t* bytes);
/* Diagnostics (tools/f1b_isolate.py): the split-fp16 step's dZ2 hand-off inside `workspace` for `rows`
 * minibatch rows: out[net] = dZ2 planes ([rows / 16 tiles][8][hi, lo][64][8] fp16, sgd_sf16.hip F1a),
 * out[2 + net] = the tiles' int32 split exponents. */
int rlks_debug_sf_handoff(const rlks_mlp_desc* desc, int rows, void* workspace_dev, void** out);
/* Diagnostics (tools/wide_b2_isolate.py): the generic-width step's per-net forward and loss buffers
 * inside `workspace` after rlks_ppo_grad: out[3 net] = H2 [rows][hidden], out[3 net + 1] = head
 * outputs [rows][A or 1], out[3 net + 2] = dL/d outputs [rows][A or 1] (float32). */
int rlks_debug_wide_bufs(const rlks_mlp_desc* desc, int rows, void* workspace_dev, void** out);
int rlks_ppo_grad(const rlks_mlp_desc* desc, const rlks_ppo_coeffs* coeffs, const float* params_dev,
                  const float* dyn_dev, const float* mb_dev, int rows, float* grad_dev,
                  double* stats_dev, void* workspace_dev, int64_t workspace_bytes, void* stream);

/* Same, launching only the phases in `phases` (profiling / benchmarking: each phase reads what the
 * previous phases left in the workspace).  Split-fp16: F1A / F1B without a FWD bit run the split F1
 * kernels and a REDUCE in the same call sums their partials; a call with REDUCE and no F1 phase sums
 * the partials of the default F1 form (rlks_sf_f1_fused). */
#define RLKS_PHASE_FWD 1    /* F1: forward + head + loss + dZ2 */
#define RLKS_PHASE_DW2 2    /* F2: dW2 = dZ2^T H1 (split over rows) */
#define RLKS_PHASE_DH1 4    /* F3: dH1 = dZ2 W2 -> dZ1 -> dW1, db1 partials */
#define RLKS_PHASE_REDUCE 8 /* fixed-order reduction of all partials (+ stats) */
#define RLKS_PHASE_ALL 15
#define RLKS_PHASE_FWD_PI 16 /* F1 of the policy net only (profiling) */
#define RLKS_PHASE_FWD_VF 32 /* F1 of the value net only (profiling) */
#define RLKS_PHASE_PREP 64   /* split-fp16: weight split/permute (implied by RLKS_PHASE_FWD) */
#define RLKS_PHASE_F1A 128   /* split-fp16, split F1: k_sf_fwd only, both nets (profiling) */
#define RLKS_PHASE_F1B 256   /* split-fp16, split F1: k_sf_bwd only, both nets (profiling) */
int rlks_ppo_grad_phases(const rlks_mlp_desc* desc, const rlks_ppo_coeffs* coeffs, const float* params_dev,
                         const float* dyn_dev, const float* mb_dev, int rows, float* grad_dev, double* stats_dev,
                         void* workspace_dev, int64_t workspace_bytes, int phases, void* stream);

/* In-pipeline kernel timing of the split-fp16 gradient (bench.py roofline): `reps` full rlks_ppo_grad
 * passes on `stream` (after one untimed pass), each kernel launched with a start / stop event pair
 * (hipExtLaunchKernelGGL: the kernel's own duration, as rocprofv3 measures it); ms_out[6] = average ms
 * of the weight split (k_sf_split), F1a (k_sf_fwd; or the fused k_sf_f1, see rlks_sf_f1_fused), F1b
 * (k_sf_bwd; 0 when fused), F2 (k_sf_dw2r) and the reduce (k_reduce), each less the event bracket's own
 * cost, which ms_out[5] reports (the same bracket around an empty kernel).  Synchronises the stream. */
int rlks_ppo_grad_profile(const rlks_mlp_desc* desc, const rlks_ppo_coeffs* coeffs, const float* params_dev,
                          const float* dyn_dev, const float* mb_dev, int rows, float* grad_dev, double* stats_dev,
                          void* workspace_dev, int64_t workspace_bytes, int reps, double* ms_out, void* stream);

/* 1 if a whole split-fp16 gradient of this descriptor runs F1 as one kernel (k_sf_f1: the default up to
 * 4 actions; RLKS_F1_FUSED=1 / RLKS_F1_SPLIT=1 in the environment force either form, any other value is
 * as unset), else 0 (bench.py
 * names the kernels it times and profiles by it).  Not a reference interface: build introspection. */
int rlks_sf_f1_fused(const rlks_mlp_desc* desc);

/* torch.optim.Adam step (lerp form of exp_avg, bias-corrected), in place on n floats */
int rlks_adam_step(float* params_dev, const float* grad_dev, float* m_dev, float* v_dev, int64_t n,
                   float lr, float beta1, float beta2, float eps, int step, void* stream);
/* One SGD step on one rank: the PPO gradient of the minibatch (as rlks_ppo_grad; `grad` still
 * receives it) with Adam (as rlks_adam_step, step `step`) applied inside the gradient reduction,
 * which also leaves the new weights' max |w| for the next step's operand split (prev_fused = 1 on
 * the step after a fused one: the weight-max pass is skipped, with a device-side check that falls
 * back to scanning the weights).  Replaces rlks_ppo_grad + rlks_adam_step when no gradient
 * all-reduce sits between them; other precisions run exactly those two calls. */
int rlks_ppo_sgd_step(const rlks_mlp_desc* desc, const rlks_ppo_coeffs* coeffs, float* params_dev,
                      const float* dyn_dev, const float* mb_dev, int rows, float* grad_dev, double* stats_dev,
                      float* adam_m_dev, float* adam_v_dev, int64_t n_params, float lr, float beta1, float beta2,
                      float eps, int step, int prev_fused, void* workspace, int64_t ws_bytes, void* stream);

/* rlks_ppo_sgd_step followed by the next step's rlks_ppo_gather_packed (the arguments below) into
 * next->mb_dev, which may be this step's own mb_dev: the gather runs inside the step's last launch
 * (its gradient reduction), after every read of the minibatch.  Same rows and bytes as the two
 * calls; next == NULL is rlks_ppo_sgd_step.  (Reference: RLlib's minibatch loop,
 * sgd_minibatch_size at rl_scheduler/agent/train_ppo.py:16, draws minibatch k+1 after SGD step k.) */
typedef struct rlks_gather_next {
  const float* packed_dev; /* rlks_ppo_pack records [T N] */
  float* mb_dev;
  uint64_t perm_seed;
  int64_t row0;
  int T, N, epoch, groups, group0, rows;
} rlks_gather_next;
int rlks_ppo_sgd_step_next(const rlks_mlp_desc* desc, const rlks_ppo_coeffs* coeffs, float* params_dev,
                           const float* dyn_dev, const float* mb_dev, int rows, float* grad_dev, double* stats_dev,
                           float* adam_m_dev, float* adam_v_dev, int64_t n_params, float lr, float beta1, float beta2,
                           float eps, int step, int prev_fused, const rlks_gather_next* next, void* workspace,
                           int64_t ws_bytes, void* stream);

/* The same SGD step across ranks (reference: RLlib's multi-GPU learner, one gradient all-reduce per
 * minibatch): rlks_ppo_grad_step writes the rank's gradient (as rlks_ppo_grad; its operand split
 * reads the maxima the previous rlks_ppo_adam_apply left when prev_fused = 1); the caller all-reduces
 * grad_dev; rlks_ppo_adam_apply then applies Adam step `step` in place (as rlks_adam_step,
 * bit-identical) and leaves the new weights' maxima for the next step.  `rows` / the workspace are
 * those of the gradient call; n_params = the padded layout size.  Other precisions run
 * rlks_ppo_grad / rlks_adam_step. */
int rlks_ppo_grad_step(const rlks_mlp_desc* desc, const rlks_ppo_coeffs* coeffs, const float* params_dev,
                       const float* dyn_dev, const float* mb_dev, int rows, float* grad_dev, double* stats_dev,
                       int step, int prev_fused, void* workspace, int64_t ws_bytes, void* stream);
/* rlks_ppo_grad_step + the next step's gather, as rlks_ppo_sgd_step_next (the gather blocks ride
 * in the gradient-reduce launch, before the caller's all-reduce). */
int rlks_ppo_grad_step_next(const rlks_mlp_desc* desc, const rlks_ppo_coeffs* coeffs, const float* params_dev,
                            const float* dyn_dev, const float* mb_dev, int rows, float* grad_dev, double* stats_dev,
                            int step, int prev_fused, const rlks_gather_next* next, void* workspace,
                            int64_t ws_bytes, void* stream);
/* rlks_ppo_grad_step_next in two parts, so that the caller's all-reduce of part 1's gradient buckets
 * runs under part 2's kernels: part 1 = the weight split, the forward / loss kernel (F1a), dW2 / db2
 * (F2) and the reduce of W2, b2, W3, b3 (both nets) and the stats; part 2 = the dH1 / dW1 kernel
 * (F1b) and the reduce of W1, b1 (+ the next gather, `next` is read by part 2 only).  The gradient
 * equals rlks_ppo_grad_step's bit for bit.  Buckets (offsets of rlks_mlp_layout, storage order
 * above): part 1 = [off[2], padded), part 2 = [off[0], off[2]), one contiguous range each.  Other
 * precisions: the whole gradient in part 1, part 2 only gathers. */
int rlks_ppo_grad_step_part(const rlks_mlp_desc* desc, const rlks_ppo_coeffs* coeffs, const float* params_dev,
                            const float* dyn_dev, const float* mb_dev, int rows, float* grad_dev, double* stats_dev,
                            int step, int prev_fused, int part, const rlks_gather_next* next, void* workspace,
                            int64_t ws_bytes, void* stream);
int rlks_ppo_adam_apply(const rlks_mlp_desc* desc, float* params_dev, const float* grad_dev, float* adam_m_dev,
                        float* adam_v_dev, int64_t n_params, float lr, float beta1, float beta2, float eps, int step,
                        void* workspace, int64_t ws_bytes, int rows, void* stream);

/* ---- global-norm gradient clipping (PPOConfig.training(grad_clip=c), grad_clip_by "global_norm").
 * Restates RLlib's old-API-stack torch policy (ray/rllib/utils/torch_utils.py apply_grad_clipping,
 * one optimizer over every parameter of both nets) and torch.nn.utils.clip_grad_norm_ (norm_type 2);
 * both are third-party and absent from the reference tree, the arithmetic is pinned by
 * tests/clip_ref.py.  Per SGD step, over the true elements of the 12 tensors (layout padding is never
 * read):
 *   S = sum g^2 in f64 (squares of fp32 values are exact), one fixed summation order that does not
 *       depend on the kernel that produced g;  norm = sqrt(S);
 *   coef = (float) fmin(1.0, (double) grad_clip / (norm + 1e-6));  g <- g * coef (fp32, round to nearest);
 *   Adam (rlks_adam_step's arithmetic) on the clipped g, which grad_dev holds afterwards, as torch
 *   leaves p.grad.  stats_dev[RLKS_STAT_GRAD_GNORM] = norm (before clipping).
 * grad_clip must be finite and > 0 (RLKS_ERR_ARG).  The workspace is the step's own,
 * rlks_ppo_workspace_bytes(desc, rows) bytes: the norm's scratch lies behind the gradient's. */

/* The norm alone (a test surface, like rlks_absmax): *norm_dev (double) = the global norm of the flat
 * gradient grad_dev (n_params = padded_count).  workspace: any scratch of at least
 * rlks_ppo_workspace_bytes(desc, any valid rows) bytes, overwritten from its start -- not the
 * workspace of a run between two of its SGD steps. */
int rlks_grad_global_norm(const rlks_mlp_desc* desc, const float* grad_dev, int64_t n_params, double* norm_dev,
                          void* workspace, int64_t ws_bytes, void* stream);
/* rlks_ppo_sgd_step_next with clipping (next may be NULL).  Split-fp16: the gradient launches of
 * rlks_ppo_grad_step_next, whose reduce also leaves one norm partial per block, the norm, then the
 * clipped Adam pass of rlks_ppo_adam_apply_clip; other precisions: rlks_ppo_grad, the norm, Adam. */
int rlks_ppo_sgd_step_clip(const rlks_mlp_desc* desc, const rlks_ppo_coeffs* coeffs, float* params_dev,
                           const float* dyn_dev, const float* mb_dev, int rows, float* grad_dev, double* stats_dev,
                           float* adam_m_dev, float* adam_v_dev, int64_t n_params, float lr, float beta1, float beta2,
                           float eps, int step, int prev_fused, float grad_clip, const rlks_gather_next* next,
                           void* workspace, int64_t ws_bytes, void* stream);
/* rlks_ppo_adam_apply with clipping, after the caller's all-reduce(s) of rlks_ppo_grad_step[_next /
 * _part]: the norm of the all-reduced gradient (every rank computes the same bits), then Adam on
 * g * coef with the next step's weight maxima and step tag as rlks_ppo_adam_apply leaves them.
 * stats_dev (may be NULL): the step's stats row, [RLKS_STAT_GRAD_GNORM] is written. */
int rlks_ppo_adam_apply_clip(const rlks_mlp_desc* desc, float* params_dev, float* grad_dev, float* adam_m_dev,
                             float* adam_v_dev, int64_t n_params, float lr, float beta1, float beta2, float eps,
                             int step, float grad_clip, double* stats_dev, void* workspace, int64_t ws_bytes, int rows,
                             void* stream);

/* RLlib update_kl: kl = stats_sum[0] / stats_sum[1]; x1.5 if kl > 2*target, x0.5 if < target/2 */
int rlks_kl_update(float* dyn_dev, const double* kl_sum_count_dev, float kl_target, void* stream);

/* ============================================================== rollout metrics =========== */
/* What the policy did during one rollout, reduced on the device (PPOConfig.reporting(rollout_metrics=True),
 * DESIGN.md §20): out_dev = double[RLKS_RM_FIXED + A + C], the RLKS_RM_* slots of rlks_types.h, then A
 * action counts, then C sums of the utilisation columns obs[t][n][2C + c] (t < T; D = the obs row
 * length, D >= 3 C).  Reads bufs->actions / rewards / dones / vtarg, values[0..T) and those obs columns;
 * adv, logits and logp are not read.  vtarg must be valid: call it after rlks_gae.
 * Arithmetic: every f32 input is widened to f64 first, squares and the residual are formed in f64, all
 * sums are f64, min / max are taken on the f32 values.  Order: stage one writes one partial record per
 * workgroup of a bounded grid into the workspace (sample -> workgroup, wave and lane is a function of
 * T N alone; lanes meet by cross-lane butterflies, waves in index order), stage two sums the records in
 * index order.  No floating-point atomics: the same inputs give the same bits on every run.
 * rlks_rollout_metrics_size: the doubles in out_dev (negative RLKS_ERR_* for bad A / C).  The workspace
 * is rlks_rollout_metrics_workspace_bytes(T, N, A, C) bytes, 8-byte aligned, and holds nothing between
 * calls.  A <= 4096, C <= 1024 (RLKS_ERR_UNSUPPORTED beyond).  Two launches, asynchronous on `stream`
 * and capturable. */
int rlks_rollout_metrics_size(int A, int C);
int rlks_rollout_metrics_workspace_bytes(int T, int N, int A, int C, int64_t* bytes);
int rlks_rollout_metrics(const rlks_rollout_bufs* bufs, int D, int A, int C, double* out_dev,
                         void* workspace_dev, int64_t workspace_bytes, void* stream);

/* ============================================================== observation filter ======== */
/* PPOConfig.rollouts(observation_filter="MeanStdFilter"): RLlib's (x - mean) / (std + 1e-8)
 * per observation column with the unbiased running variance, no clipping.  RLlib is absent from the
 * reference tree; the arithmetic below is the specification, restated in numpy by tests/obs_filter_ref.py.
 * State: double[rlks_obs_filter_size(D)], the RLKS_OF_* layout of rlks_types.h; observations are row-major
 * [rows][D].  1 <= D <= 512 (2 x 4 KB of LDS tables; the largest env here has D = 288); beyond that, for a
 * null or misaligned pointer (floats 4-byte, doubles 8-byte aligned), rows < 0 or a workspace that is too
 * small: RLKS_ERR_ARG and nothing is launched.  Every entry is asynchronous on `stream` and capturable.
 *   init    count = 0, mean = 0, m2 = 0, inv = 1: the identity filter.
 *   apply   y = (float)(((double)x - mean[d]) * inv[d]): one f64 subtract, one f64 multiply, one
 *           conversion, never contracted.  y_dev == x_dev (in place) is allowed, any other overlap is not.
 *           Reads the state, never writes it.  16-byte accesses when x_dev and y_dev are 16-byte aligned.
 *   stats   record_dev = double[RLKS_OFR_SUMS + 2 D] = {rows, s1[D], s2[D]} over x_dev[rows][D], s1[d] =
 *           sum (x - K[d]), s2[d] = sum (x - K[d])^2 in f64, K = the state's mean read on the device (the
 *           shift keeps m2 free of the sum x^2 - n mean^2 cancellation).  Two launches; the grid and the
 *           order of every addition depend on (rows, D) alone and there are no floating-point atomics: the
 *           same input gives the same bits on every run.  The workspace (8-byte aligned) holds nothing
 *           between calls.  rows = 0 gives a record of zeros.
 *   merge   Chan's update with na = count, nb = record[0], n = na + nb, in f64, every operation rounded on
 *           its own:  delta = s1 / nb;  mean' = mean + delta * (nb / n);
 *           m2' = max(0, (m2 + (s2 - s1 * delta)) + (delta * delta) * ((na * nb) / n));
 *           inv' = 1 / (sqrt(m2' / (n - 1)) + 1e-8) when n >= 2, else 1;  count' = n.
 *           nb = 0 leaves the state unchanged.  The record is taken as handed over: several ranks sum their
 *           records (all-reduce) first, K being the same on all of them.  One workgroup. */
int rlks_obs_filter_size(int D); /* doubles in the state; negative RLKS_ERR_* for a bad D */
int rlks_obs_filter_init(double* state_dev, int D, void* stream);
int rlks_obs_filter_apply(const double* state_dev, const float* x_dev, float* y_dev, int64_t rows, int D,
                          void* stream);
int rlks_obs_filter_workspace_bytes(int64_t rows, int D, int64_t* bytes);
int rlks_obs_filter_stats(const double* state_dev, const float* x_dev, int64_t rows, int D, double* record_dev,
                          void* workspace_dev, int64_t workspace_bytes, void* stream);
int rlks_obs_filter_merge(double* state_dev, const double* record_dev, int D, void* stream);

/* rlks_rollout_ws with the filter between the env and the policy: the same dispatch and the same
 * launches, except that the env's observation output of step t goes to raw_dev[t + 1] (raw_dev is
 * float[T + 1][N][D]) and one rlks_obs_filter_apply launch per step writes bufs->obs[t + 1] =
 * filter(raw[t + 1]) before the next forward reads it.  The caller provides raw[0]; the entry filters it
 * into bufs->obs[0] first.  The state is read, never updated: the filter is frozen while a rollout runs.
 * A split-fp16 table rollout takes the per-step kernels at every lane count (the persistent T-step
 * kernel keeps its observations to itself).  workspace may be NULL for the fp32 kernels, as for
 * rlks_rollout. */
int rlks_rollout_filtered(rlks_env* env, const rlks_mlp_desc* desc, const float* params_dev,
                          const rlks_rollout_bufs* bufs, int explore, void* workspace, int64_t ws_bytes,
                          const double* state_dev, float* raw_dev, void* stream);

/* ============================================================== off-policy evaluation ===== */
/* What a target policy would have earned on logged decisions (rlks.offline.estimate): RLlib's
 * ImportanceSampling and WeightedImportanceSampling estimators restated (RLlib is absent from the reference
 * tree; tests/ope_ref.py pins the arithmetic).  Every entry is asynchronous on `stream`, reads nothing on the
 * host and is capturable; there are no floating-point atomics, and every addition's place depends on (T, N)
 * alone: the same buffers give the same bytes on every call.
 *
 * rlks_ope_logp: logp_out_dev[i] = log softmax(logits_dev[i])[actions_dev[i]] = l[a] - mx - log(sum exp(l - mx)),
 * rows i < rows of logits_dev[rows][A] (read only), by the operation sequence of rlks_sample_categorical's
 * draw, so the logp of an action that draw chose comes back bit for bit.  mask_dev (may be NULL): uint64_t[rows]
 * with rlks_sample_categorical_masked's rules (entries outside the mask read as RLKS_MASKED_LOGIT, a mask
 * without a bit among the low A counts as all of them) and that draw's bits; A > 64 with a mask:
 * RLKS_ERR_UNSUPPORTED.  An action outside [0, A) gives NaN.  rows = 0 launches nothing.
 *
 * rlks_ope_estimate: inputs time-major [T][N]: logp_new (target policy), logp_old (behaviour policy, as
 * logged), rewards (f32) and dones (u8).  In lane n a segment starts at t = 0 and after every non-zero done;
 * it ends at its done step or at T - 1 (then it is truncated).  Every segment is counted, with
 * drop_truncated != 0 only those ending in a done; an uncounted segment contributes to nothing.  Per step
 * k = t - start of a counted segment, every f32 widened to f64 first and every operation rounded on its own:
 *   lr = logp_new - logp_old;  L_k = L_{k-1} + lr (L_{-1} = 0);  p_k = exp(min(L_k, RLKS_OPE_LMAX));
 *   g_k = g_{k-1} * gamma (g_0 = 1);  x_k = g_k * r;
 *   v_behavior = sum_k x_k;  v_is = sum_k p_k x_k   (ascending k, from 0.0);
 *   S_k = sum of p_k over the counted segments that reach step k, c_k = their number, w_k = S_k / c_k;
 *   v_wis = sum_k (p_k / w_k) x_k, a term being 0.0 where S_k == 0;  p_end = p at the segment's last step.
 * record_dev = double[RLKS_OPE_SIZE] (rlks_types.h).  ep_out_dev (may be NULL): double[T][N][4]; at (t_end, n)
 * of every counted segment {v_behavior, v_is, v_wis, p_end}, untouched elsewhere.  Four launches:
 *   columns  one thread per lane walks t = 0 .. and adds p_k into its own column of a [T][N] f64 matrix (and 1
 *            into a u32 one) in program order, noting the rows it reached;
 *   rows     one workgroup per k: S_k and c_k over n (thread i adds lanes i, i + 256, .. in that order, lanes
 *            meet by xor butterflies, waves in wave order), then w_k;
 *   values   the walk again with w_k: the segments' values, ep_out, and per lane the record's sums in segment
 *            order; a workgroup's lanes meet as above and leave one partial record;
 *   final    one workgroup adds the partial records (thread i: records i, i + 256, .., then as above).
 * The workspace is rlks_ope_workspace_bytes(T, N) bytes (12 T N and a little), 8-byte aligned, and holds
 * nothing between calls.  RLKS_ERR_ARG: a null pointer, T or N < 1, gamma not finite or outside [0, 1], a
 * misaligned pointer (floats 4 bytes, doubles and the workspace 8), a workspace that is too small. */
int rlks_ope_logp(const float* logits_dev, const int32_t* actions_dev, const uint64_t* mask_dev /* NULL */,
                  int64_t rows, int A, float* logp_out_dev, void* stream);
int rlks_ope_workspace_bytes(int T, int N, int64_t* bytes);
int rlks_ope_estimate(const float* logp_new_dev, const float* logp_old_dev, const float* rewards_dev,
                      const uint8_t* dones_dev, int T, int N, double gamma, int drop_truncated, double* record_dev,
                      double* ep_out_dev /* NULL */, void* workspace_dev, int64_t workspace_bytes, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* RLKS_H */
