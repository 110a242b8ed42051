/*
 * rlks_types.h — plain-C types shared by the HIP library (librlks.so) and the CPU oracle.
 *
 * The environment model is the reference's K8sMultiCloudEnv
 * (/root/reference/rl_scheduler/env/k8s_multi_cloud_env.py:36-157), generalised to C clouds
 * and batched over n_envs independent lanes.  With n_clouds = 2 and nodes_per_cluster = 0
 * it is the reference env exactly.  nodes_per_cluster > 0 enables
 * the node-level extension specified in DESIGN.md §4 (no reference exists).
 */
#ifndef RLKS_TYPES_H
#define RLKS_TYPES_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* cpu-noise / randomness source for the observation's utilisation entries */
enum {
  RLKS_NOISE_PHILOX = 0,   /* Philox4x32-10, key = seed, counter = (env, episode, t, purpose) */
  RLKS_NOISE_MT19937 = 1   /* per-lane CPython MT19937 (random.seed / random.random), bit-exact */
};

/* completed-episode log capacity (rlks_env_episode_log): RLlib smooths episode_reward_mean over at
 * least the last 100 episodes (metrics_num_episodes_for_smoothing), so 100+ individual returns per
 * iteration are all a host ever needs */
enum { RLKS_EPLOG_CAP = 128 };

/* Philox counter purposes (ctr[3] high half) */
enum {
  RLKS_PURPOSE_OBS = 1,
  RLKS_PURPOSE_ACTION = 2,
  RLKS_PURPOSE_ARRIVAL = 3,
  RLKS_PURPOSE_DEPART = 4,
  RLKS_PURPOSE_OCCUPANCY = 5
};

/* Baseline schedulers of rlks_env_rule_actions: one decision per lane from its
 * observation row [cost[C], lat[C], util[C]], its step and episode and, on node-level envs, its
 * clusters' used millicores.  Ties go to the lowest index. */
enum {
  RLKS_RULE_ROUND_ROBIN = 0,      /* step % C (train_and_compare.py:65 at C = 2) */
  RLKS_RULE_CHEAPEST = 1,         /* argmin of the f32 cost (normal_scheduler_step, :156-157, at C = 2) */
  RLKS_RULE_MYOPIC = 2,           /* argmax of w_cost * cost + w_lat * lat in f64: the immediate reward */
  RLKS_RULE_LEAST_LOADED = 3,     /* argmin of the f32 utilisation */
  RLKS_RULE_MYOPIC_WITH_ROOM = 4, /* MYOPIC over the clusters with room for one more pod (all, if none has) */
  RLKS_RULE_RANDOM = 5            /* uniform: rlks_sample_categorical's draw from all-zero logits */
};

/* Invalid-action masking on node-level envs (rlks_env_action_mask, rlks_env_masked_sample).
 *   room(lane, c) = used_cpu[c][lane] / pod_cpu_m <
 *                   nodes_per_cluster * min(node_cpu[c] / pod_cpu_m, node_mem[c] / pod_mem_mi),
 *                   every term an integer: the RLKS_RULE_MYOPIC_WITH_ROOM predicate.
 *   mask(lane)    = uint64_t, bit c set when room(lane, c); when no cluster has room, all n_clouds low bits
 *                   (nothing to choose between: the rule's fallback).  A table env has room everywhere.
 * The logit of a cluster without room is overwritten with RLKS_MASKED_LOGIT, and a logit counts as masked
 * when it is <= RLKS_MASKED_LOGIT_MAX.  The sentinel is finite on purpose: with -inf the KL and entropy
 * terms of the PPO loss become 0 * inf = NaN; with -1e30f a masked action gets expf(...) == 0 and its KL,
 * entropy and gradient terms come out as exact zeros through the loss heads' existing arithmetic.  The
 * logits of clusters with room are expected above RLKS_MASKED_LOGIT_MAX (any finite policy output is). */
#define RLKS_MASKED_LOGIT (-1e30f)
#define RLKS_MASKED_LOGIT_MAX (-1e29f)

typedef struct rlks_env_cfg {
  int32_t n_envs;        /* lanes */
  int32_t n_rows;        /* T: table rows (reference: 100, normalized_rl_data.csv) */
  int32_t n_clouds;      /* C: clusters / actions (reference: 2, :51) */
  int32_t max_steps;     /* episode length; reference: len(table) - 1 = 99 (:66) */
  int32_t noise_mode;    /* RLKS_NOISE_* */
  int32_t autoreset;     /* 1: terminated lanes reset inside step (vector-env semantics) */
  int32_t env_offset;    /* global id of lane 0 (multi-GPU shard base; Philox counter word 0) */
  int32_t skip_returns;  /* 1: no episode-return bookkeeping in the step (ep_ret / ret_sum / ep_cnt /
                            episode log untouched): the plain gymnasium step contract */
  uint64_t seed;         /* Philox key; also the default MT seed when none is given */
  double cpu_lo;         /* random.uniform(0.1, 0.8) (:87) */
  double cpu_hi;
  double w_cost;         /* reward = scale * (w_cost * cost + w_lat * latency)  (:122) */
  double w_lat;
  double scale;
  /* ---- node-level extension; nodes_per_cluster == 0 disables it ---- */
  int32_t nodes_per_cluster; /* N nodes per cluster */
  int32_t pod_cpu_m;         /* pod request, millicores (simple-service.yaml:27: 100m) */
  int32_t pod_mem_mi;        /* pod request, MiB (simple-service.yaml:28: 64Mi) */
  int32_t arrival_mode;      /* 0: Poisson(arrival_rate); 1: bursty trace (per-step rates) */
  double arrival_rate;       /* mean pod arrivals per step */
  double depart_prob;        /* per-step probability that a running pod leaves (every pod) */
  double init_occupancy;     /* initial pods per node ~ U(0, init_occupancy * max_pods) */
  double reject_penalty;     /* subtracted from reward per rejected pod (0: reference reward) */
} rlks_env_cfg;

/* Multi-layer-perceptron policy/value description (RLlib FCNet, vf_share_layers=False) */
typedef struct rlks_mlp_desc {
  int32_t obs_dim;   /* D  (reference: 6) */
  int32_t hidden;    /* H  (reference: fcnet_hiddens [256, 256]) */
  int32_t n_actions; /* A  (reference: 2) */
  int32_t precision; /* RLKS_PRECISION_*: how the SGD step's matrix products are computed */
} rlks_mlp_desc;

/* SGD-step matrix arithmetic.  Both meet the 1e-5 relative gradient bar against the fp64 oracle:
 * FP32 runs v_mfma_f32_32x32x2_f32 (bitwise an fmaf chain); SF16 splits every operand into two
 * scaled fp16 halves and accumulates three v_mfma_f32_32x32x16_f16 products in fp32 (error
 * <= ~2^-21 per product, measured below the fp32 chain's) at 16x the fp32 matrix rate. */
enum {
  RLKS_PRECISION_FP32 = 0,
  RLKS_PRECISION_SF16 = 1,
  RLKS_PRECISION_WIDE = 2, /* generic split-fp16 GEMM path (wide_mlp.hip): any width, node envs;
                              chosen automatically when the fused 256-unit kernels do not fit */
  RLKS_PRECISION_F16 = 3   /* throughput mode: the split-fp16 SGD kernels with one product (fp16
                              operands hi x hi, fp32 accumulation) instead of three -- below the
                              reference's fp32, a secondary figure only; rollouts as RLKS_PRECISION_SF16 */
};

/* The form a rollout runs in (rlks_rollout_form).  A table env's rollout kernels stage the
 * env's two tables in LDS beside their own buffers; a form that would ask for more than a workgroup's
 * 160 KiB is passed over for the next one.  The per-step forms hold the tables alone. */
enum {
  RLKS_ROLLOUT_SF16_PERSISTENT = 0, /* k_sf_roll: the whole rollout in one launch */
  RLKS_ROLLOUT_SF16_PER_STEP = 1,   /* per step k_sf_fwd16, then rlks_env_sample_step */
  RLKS_ROLLOUT_FP32_FUSED_32 = 2,   /* per step k_fwd_head<..., FWD_ROLLOUT> on 32-row tiles; values in one pass */
  RLKS_ROLLOUT_FP32_FUSED_128 = 3,  /* the same on 128-row tiles (more than 32,768 lanes) */
  RLKS_ROLLOUT_FP32_PER_STEP = 4,   /* per step the fp32 policy forward, then rlks_env_sample_step */
  RLKS_ROLLOUT_WIDE = 5,            /* generic-width path (wide_mlp.hip) */
  RLKS_ROLLOUT_NODE = 6             /* node-level env: forward of both nets, then the sampling node step */
};

/* One split-fp16 GEMM (fp32 in / fp32 out, fp32-accurate): C = epi(op(A) op(B)), op = transpose
 * when trans_*; operand scales come from max|x| slots (uint bits of a non-negative float). */
enum {
  RLKS_GEMM_STORE = 0,     /* C = acc */
  RLKS_GEMM_TANH_BIAS = 1, /* C = tanh(acc + bias[n]) */
  RLKS_GEMM_BIAS = 2,      /* C = acc + bias[n] */
  RLKS_GEMM_DTANH = 3      /* C = acc * (1 - aux[m][n]^2) */
};
typedef struct rlks_gemm_desc {
  const float* a;
  const float* b;
  float* c;
  const float* bias;
  const float* aux;
  int32_t m, n, k, lda, ldb, ldc, ldaux;
  int32_t trans_a, trans_b, epilogue, accumulate, reserved;
  const uint32_t* a_max;
  const uint32_t* b_max;
  uint32_t* c_max;         /* optional (NULL): atomicMax of |C| */
} rlks_gemm_desc;

/* PPO loss coefficients that stay fixed for a run (RLlib PPOConfig names and defaults) */
typedef struct rlks_ppo_coeffs {
  float clip_param;      /* 0.3 */
  float vf_clip_param;   /* 10.0 */
  float vf_loss_coeff;   /* 1.0 */
  float entropy_coeff;   /* 0.0 */
} rlks_ppo_coeffs;

/* Device-resident per-iteration scalars (float[RLKS_DYN_SIZE]); kernels read them so that no
 * host round trip is needed between rollout, advantage standardisation and the SGD steps. */
enum {
  RLKS_DYN_ADV_MEAN = 0,    /* mean of the train batch's advantages */
  RLKS_DYN_ADV_INVSTD = 1,  /* 1 / max(1e-4, std)  (RLlib standardize_fields) */
  RLKS_DYN_KL_COEFF = 2,    /* adaptive KL coefficient (initial 0.2) */
  RLKS_DYN_INV_COUNT = 3,   /* 1 / global minibatch rows: the loss is a mean */
  RLKS_DYN_SIZE = 8
};

/* Per-minibatch loss statistics written by rlks_ppo_grad (double[RLKS_STAT_SIZE], sums) */
enum {
  RLKS_STAT_POLICY_LOSS = 0, /* sum of -surrogate */
  RLKS_STAT_VF_LOSS = 1,     /* sum of clipped squared error */
  RLKS_STAT_KL = 2,          /* sum of KL(old || new) */
  RLKS_STAT_ENTROPY = 3,     /* sum of entropy */
  RLKS_STAT_ROWS = 4,        /* rows */
  RLKS_STAT_GRAD_GNORM = 5,  /* global norm of the gradient before clipping (the *_clip entry points of
                                rlks.h; every other entry point writes 0.0) */
  RLKS_STAT_SIZE = 8
};

/* Per-iteration rollout metrics record written by rlks_rollout_metrics (double[RLKS_RM_FIXED + A + C],
 * DESIGN.md §20): sums are f64 sums of the f32 inputs widened first, min / max are taken on the f32
 * values, counts are exact integers held in doubles.  After the fixed slots: A action counts, then the C
 * sums of the utilisation columns obs[t][n][2C + c], t < T. */
enum {
  RLKS_RM_ROWS = 0,        /* samples read = T N */
  RLKS_RM_REWARD_SUM = 1,
  RLKS_RM_REWARD_MIN = 2,
  RLKS_RM_REWARD_MAX = 3,
  RLKS_RM_DONES = 4,       /* steps with a non-zero done byte */
  RLKS_RM_VALUE_SUM = 5,   /* values[0..T) */
  RLKS_RM_VTARG_SUM = 6,
  RLKS_RM_VTARG_SQ = 7,
  RLKS_RM_RESID_SUM = 8,   /* resid = (double)vtarg - (double)values */
  RLKS_RM_RESID_SQ = 9,
  RLKS_RM_FIXED = 10
};

/* Observation-filter state (rlks_obs_filter_*): double[RLKS_OF_VECS + RLKS_OF_NVEC * D] =
 * the row count, then three vectors over the D observation columns; vector v of column d lies at
 * [RLKS_OF_VECS + v * D + d].  A fresh state is count 0, mean 0, m2 0, inv 1: the identity. */
enum {
  RLKS_OF_COUNT = 0, /* observations merged so far (an integer held in a double) */
  RLKS_OF_VECS = 1,  /* the first vector starts here */
  RLKS_OF_MEAN = 0,  /* running mean */
  RLKS_OF_M2 = 1,    /* sum of squared deviations from the mean */
  RLKS_OF_INV = 2,   /* 1 / (sqrt(m2 / (count - 1)) + 1e-8) when count >= 2, else 1 */
  RLKS_OF_NVEC = 3
};
/* Batch record of rlks_obs_filter_stats: double[RLKS_OFR_SUMS + 2 D] = rows, then s1[D] = sum (x - K[d])
 * and s2[D] = sum (x - K[d])^2 with K = the state's mean when the record was taken.  Plain sums: the
 * records of several ranks with equal states add. */
enum {
  RLKS_OFR_ROWS = 0,
  RLKS_OFR_SUMS = 1
};

/* Off-policy evaluation record written by rlks_ope_estimate (double[RLKS_OPE_SIZE]), over the
 * counted segments of a decision log: counts are exact integers held in doubles; per segment v_behavior =
 * sum x_k, v_is = sum p_k x_k, v_wis = sum (p_k / w_k) x_k and p_end = p at its last step, all f64; the *_SUM
 * slots add them over the segments, the *_SQ slots their squares (formed in f64). */
enum {
  RLKS_OPE_EPISODES = 0,  /* counted segments */
  RLKS_OPE_STEPS = 1,     /* their steps */
  RLKS_OPE_MAX_LEN = 2,   /* the longest one's steps */
  RLKS_OPE_CLAMPED = 3,   /* steps with L_k > RLKS_OPE_LMAX */
  RLKS_OPE_BAD_ROWS = 4,  /* steps whose logp_new or logp_old is not finite: the other slots are then unspecified */
  RLKS_OPE_VB_SUM = 5,
  RLKS_OPE_VB_SQ = 6,
  RLKS_OPE_VIS_SUM = 7,
  RLKS_OPE_VIS_SQ = 8,
  RLKS_OPE_VWIS_SUM = 9,
  RLKS_OPE_VWIS_SQ = 10,
  RLKS_OPE_PEND_SUM = 11,
  RLKS_OPE_PEND_SQ = 12,
  RLKS_OPE_SIZE = 13
};
/* the cumulative log ratio L_k enters exp() as min(L_k, RLKS_OPE_LMAX): exp(700) ~ 1.0e304 is finite in f64 */
#define RLKS_OPE_LMAX 700.0

#ifdef __cplusplus
}
#endif
#endif /* RLKS_TYPES_H */
