// action_mask.hip — invalid-action masking for node-level envs: the room mask of every
// lane (rlks_env_action_mask), the masked Categorical draw ahead of the unchanged, trusted-actions node
// step (rlks_env_masked_sample) and the same draw under a caller's mask (rlks_sample_categorical_masked).
//
// A kernel of its own, like rules.hip: k_node_step_wl has no register to spare, and the room predicate is
// has_room() (env_device.h), which k_rule_actions<RLKS_RULE_MYOPIC_WITH_ROOM> evaluates too.  The masked
// draw follows categorical() (env_device.h) operation for operation on the masked row, so a row without a
// masked entry gives that function's bits; it differs in its fallback index and in writing the masked row
// back, so it stays a function of its own (categorical_masked(), beside categorical() in env_device.h: the
// serving kernel, policy_act.hip, draws with it too).  The file is built without FMA contraction, as env.hip is.
#include <hip/hip_runtime.h>

#include "env_device.h"

namespace rlks {

// mask(lane): bit c = cluster c can take one more pod; every cluster when none can (nothing to choose
// between: the rule's fallback) and on a table env.  C <= 64 (the entry points check it).
__device__ __forceinline__ uint64_t room_mask(const EnvView& v, int lane) {
  const int C = v.C;
  if (v.nodes <= 0) return low_bits(C);
  uint64_t m = 0;
  for (int c = 0; c < C; ++c)
    if (has_room(v, lane, c)) m |= 1ull << c;
  return m ? m : low_bits(C);
}

// One thread per lane; used_cpu is cluster-major [C][N] (coalesced), the logits row is C contiguous
// floats of the lane; a thread past the last lane does nothing (ragged last workgroup).
__global__ void __launch_bounds__(ENV_BLOCK) k_action_mask(EnvView v, uint64_t* __restrict__ mask) {
  const int lane = blockIdx.x * blockDim.x + threadIdx.x;
  if (lane >= v.N) return;
  mask[lane] = room_mask(v, lane);
}

__global__ void __launch_bounds__(ENV_BLOCK) k_masked_sample(EnvView v, float* __restrict__ logits, int explore,
                                                             int32_t* __restrict__ actions, float* __restrict__ logp,
                                                             uint64_t* __restrict__ mask_out) {
  const int lane = blockIdx.x * blockDim.x + threadIdx.x;
  if (lane >= v.N) return;
  const uint64_t m = room_mask(v, lane);
  float lp;
  actions[lane] = categorical_masked(logits + (size_t)lane * v.C, v.C, m, explore != 0,
                                     action_ctr(v, lane, v.episode[lane], v.step[lane]), v.k0, v.k1, lp);
  logp[lane] = lp;
  if (mask_out) mask_out[lane] = m;
}

// rows i < n: ctr = {ids[3i], ids[3i + 1], ids[3i + 2], ACTION << 16} (k_sample_categorical's)
__global__ void __launch_bounds__(256) k_sample_categorical_masked(float* __restrict__ logits,
                                                                   const uint64_t* __restrict__ mask, int n, int A,
                                                                   const uint32_t* __restrict__ ids, uint32_t k0,
                                                                   uint32_t k1, int explore,
                                                                   int32_t* __restrict__ actions,
                                                                   float* __restrict__ logp) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  float lp;
  u32x4 ctr = action_ctr(0u, 0u, 0u);
  if (explore) ctr = action_ctr(ids[3 * i], ids[3 * i + 1], ids[3 * i + 2]);  // ids may be NULL for argmax
  actions[i] = categorical_masked(logits + (size_t)i * A, A, mask[i], explore != 0, ctr, k0, k1, lp);
  if (logp) logp[i] = lp;
}

}  // namespace rlks

using namespace rlks;

extern "C" {

int rlks_env_action_mask(rlks_env* e, uint64_t* mask, void* stream) {
  RLKS_REQUIRE(e && mask, RLKS_ERR_ARG, "rlks_env_action_mask: null argument");
  RLKS_REQUIRE(e->cfg.n_clouds <= 64, RLKS_ERR_UNSUPPORTED, "rlks_env_action_mask: at most 64 clusters (a 64-bit mask)");
  hipLaunchKernelGGL(k_action_mask, dim3(cdiv(e->cfg.n_envs, ENV_BLOCK)), dim3(ENV_BLOCK), 0, (hipStream_t)stream,
                     view(e), mask);
  RLKS_LAUNCHED();
  return RLKS_OK;
}

int rlks_env_masked_sample(rlks_env* e, float* logits, int explore, int32_t* actions, float* logp, uint64_t* mask_out,
                           void* stream) {
  RLKS_REQUIRE(e && logits && actions && logp, RLKS_ERR_ARG, "rlks_env_masked_sample: null argument");
  RLKS_REQUIRE(e->cfg.n_clouds <= 64, RLKS_ERR_UNSUPPORTED,
               "rlks_env_masked_sample: at most 64 clusters (a 64-bit mask)");
  hipLaunchKernelGGL(k_masked_sample, dim3(cdiv(e->cfg.n_envs, ENV_BLOCK)), dim3(ENV_BLOCK), 0, (hipStream_t)stream,
                     view(e), logits, explore, actions, logp, mask_out);
  RLKS_LAUNCHED();
  return RLKS_OK;
}

int rlks_sample_categorical_masked(float* logits, const uint64_t* mask, int n, int A, const uint32_t* ids,
                                   unsigned long long seed, int explore, int32_t* actions, float* logp, void* stream) {
  RLKS_REQUIRE(logits && mask && actions && n >= 0 && A >= 1 && (ids || !explore), RLKS_ERR_ARG,
               "rlks_sample_categorical_masked: bad argument");
  RLKS_REQUIRE(A <= 64, RLKS_ERR_UNSUPPORTED, "rlks_sample_categorical_masked: at most 64 actions (a 64-bit mask)");
  if (n == 0) return RLKS_OK;
  hipLaunchKernelGGL(k_sample_categorical_masked, dim3(cdiv(n, 256)), dim3(256), 0, (hipStream_t)stream, logits, mask, n,
                     A, ids, (uint32_t)seed, (uint32_t)(seed >> 32), explore, actions, logp);
  RLKS_LAUNCHED();
  return RLKS_OK;
}

int rlks_env_set_action_masking(rlks_env* e, int on) {
  RLKS_REQUIRE(e, RLKS_ERR_ARG, "rlks_env_set_action_masking: null env");
  RLKS_REQUIRE(e->cfg.nodes_per_cluster > 0, RLKS_ERR_UNSUPPORTED,
               "rlks_env_set_action_masking: a table env has room everywhere (node-level envs only)");
  RLKS_REQUIRE(!on || e->cfg.n_clouds <= 64, RLKS_ERR_UNSUPPORTED,
               "rlks_env_set_action_masking: at most 64 clusters (a 64-bit mask)");
  e->action_masking = on ? 1 : 0;
  return RLKS_OK;
}

}  // extern "C"
