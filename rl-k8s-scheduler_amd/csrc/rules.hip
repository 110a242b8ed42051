// rules.hip — baseline schedulers on the device (rlks_env_rule_actions): one decision
// per lane from what a scheduler sees before the step, so that a baseline policy steps a batched env
// without a host round trip.
//
// Reference: the two baselines the reference's scripts print beside the agent,
//   rl_scheduler/agent/train_and_compare.py:65 (round robin, step % 2) and
//   rl_scheduler/env/k8s_multi_cloud_env.py:156-157 (normal_scheduler_step: the cheaper
//   cloud), generalised to C clusters, and the filter-then-score rules of a pod scheduler over the
//   node-level extension (no reference exists).
// A kernel of its own ahead of the unchanged step kernels (env.hip): k_node_step_wl has no register
// to spare.  Every rule is exact arithmetic on the lane's observation row (f32 compares; f64 products
// and sums rounded separately, as the reward's), its step and episode counters and, for a node-level
// env, its clusters' used millicores (integers): tests/rule_ref.py restates them in numpy to the bit.
#include <hip/hip_runtime.h>

#include "env_device.h"

namespace rlks {

// One thread per lane.  obs is row-major [N][3C] = [cost[C], lat[C], util[C]] (row stride 3C), used_cpu
// is cluster-major [C][N]; a thread past the last lane does nothing (ragged last workgroup).  No
// arrays: the running best of each rule is a register.
template <int RULE>
__global__ void __launch_bounds__(ENV_BLOCK) k_rule_actions(EnvView v, const float* __restrict__ obs,
                                                            int32_t* __restrict__ actions) {
  const int lane = blockIdx.x * blockDim.x + threadIdx.x;
  if (lane >= v.N) return;
  const int C = v.C;
  const float* o = obs + (size_t)lane * 3 * C;
  int act = 0;
  if constexpr (RULE == RLKS_RULE_ROUND_ROBIN) {
    act = v.step[lane] % C;
  } else if constexpr (RULE == RLKS_RULE_CHEAPEST || RULE == RLKS_RULE_LEAST_LOADED) {
    // the lowest index of the minimum (strict <)
    const float* x = o + (RULE == RLKS_RULE_CHEAPEST ? 0 : 2 * C);
    float best = x[0];
    for (int c = 1; c < C; ++c) {
      const float y = x[c];
      if (y < best) { best = y; act = c; }
    }
  } else if constexpr (RULE == RLKS_RULE_MYOPIC || RULE == RLKS_RULE_MYOPIC_WITH_ROOM) {
    // s_c = w_cost * cost_c + w_lat * lat_c in f64, the lowest index of the maximum (strict >); with
    // room: over the clusters that can take one more pod, over all of them when none can
    const bool filter = RULE == RLKS_RULE_MYOPIC_WITH_ROOM && v.nodes > 0;
    int act_room = -1;
    double best = 0.0, best_room = 0.0;
    for (int c = 0; c < C; ++c) {
      const double s = __dadd_rn(__dmul_rn(v.w_cost, (double)o[c]), __dmul_rn(v.w_lat, (double)o[C + c]));
      if (c == 0 || s > best) { best = s; act = c; }
      if (filter && has_room(v, lane, c) && (act_room < 0 || s > best_room)) { best_room = s; act_room = c; }
    }
    if (act_room >= 0) act = act_room;
  } else {  // RLKS_RULE_RANDOM
    // categorical() (env_device.h) on an all-zero logits row: max 0, every expf(0 - 0) = 1, their sum in
    // index order = (float)C exactly, u = f32(u53) * C, the first a with u < a + 1 (else C - 1), i.e.
    // floor(u) capped at C - 1 (u53 can round to 1.0f)
    const u32x4 x = philox4x32_10(action_ctr(v, lane, v.episode[lane], v.step[lane]), v.k0, v.k1);
    const float u = (float)u53(x.x, x.y) * (float)C;
    act = min((int)u, C - 1);
  }
  actions[lane] = act;
}

}  // namespace rlks

using namespace rlks;

extern "C" int rlks_env_rule_actions(rlks_env* e, int rule, const float* obs, int32_t* actions, void* stream) {
  RLKS_REQUIRE(e && obs && actions, RLKS_ERR_ARG, "rlks_env_rule_actions: null argument");
  const dim3 grid(cdiv(e->cfg.n_envs, ENV_BLOCK)), blk(ENV_BLOCK);
  hipStream_t s = (hipStream_t)stream;
  switch (rule) {
#define RLKS_RULE_CASE(R) \
  case R: hipLaunchKernelGGL(k_rule_actions<R>, grid, blk, 0, s, view(e), obs, actions); break;
    RLKS_RULE_CASE(RLKS_RULE_ROUND_ROBIN)
    RLKS_RULE_CASE(RLKS_RULE_CHEAPEST)
    RLKS_RULE_CASE(RLKS_RULE_MYOPIC)
    RLKS_RULE_CASE(RLKS_RULE_LEAST_LOADED)
    RLKS_RULE_CASE(RLKS_RULE_MYOPIC_WITH_ROOM)
    RLKS_RULE_CASE(RLKS_RULE_RANDOM)
#undef RLKS_RULE_CASE
    default: return fail(RLKS_ERR_ARG, "rlks_env_rule_actions: unknown rule");
  }
  RLKS_LAUNCHED();
  return RLKS_OK;
}
