// workspace.h — what the gradient side (ppo.hip) and the rollout side (rollout.hip) share on the host:
// the descriptor checks, the workspace layouts of the fused fp32 and split-fp16 paths (the wide path's
// is wide_mlp.h's), the weight-split prep and the two nets' argument blocks.  Defined in workspace.hip.
#pragma once

#include "sgd_sf16.h"
#include "wide_mlp.h"

namespace rlks {

bool is_wide(const rlks_mlp_desc* d);
// the split-fp16 fused kernels (fp32-accurate, or the one-product throughput mode)
bool is_sf(const rlks_mlp_desc* d);
// the fused kernels (mlp_fwd / mlp_bwd / sgd_sf16 / rollout_sf16) cover hidden 256, obs < 32 and
// 2 / 4 / 8 actions; everything else runs on the generic-width path (wide_mlp.hip)
int check_desc(const rlks_mlp_desc* d);

// fp32 path
struct NetWs {
  float *dz2, *part_b2, *part_w3, *part_b3, *part_stat, *part_w2, *part_w1, *part_b1;
};
struct Ws {
  NetWs n[2];
  double* stat64;  // [2][4]
  int64_t bytes;
  int tiles, splits;
};
int pick_splits(int M);
Ws ws_layout(int D, int A, int M, char* base);

// split-fp16 path: pre-split weights, dZ2^T, per-F1-block and per-F2-split partials
struct SfWs {
  SfNetW w[2];
  SfNet n[2];
  double* stat64;
  float* pmax_roll[2];  // the rollout's weight-max slots (the SGD steps' pmax keeps its parity state)
  _Float16* xsp;        // F1a's Xa split for F2 (SfArgs::xsp)
  int64_t bytes, weight_bytes;
  int blocks, splits, tiles_per_split;
  int fa_parts;  // F1's dW3 / db3 / stats partials per net (the split kernels' count: the allocation)
};
SfWs sf_ws_layout(int D, int A, int M, char* base);

// Weight splits for the split-fp16 kernels.  rollout: also the rollout's fragment-order copy of W2,
// with the max |w| slots of its own.  SGD step: `parity` selects the max slots (see SfPrepArgs);
// skip_wmax when the previous fused SGD step left this step's maxima there.
int sf_prep(const rlks_mlp_desc* d, const SfWs& w, const float* params, hipStream_t s, bool rollout, int parity = 0,
            bool skip_wmax = false, unsigned expect_tag = 0);

// both nets' split-fp16 argument blocks: the workspace's SfNet, b2 / w3 / b3 from the flat parameters
void sf_nets(SfNet (&n)[2], const SfWs& w, const float* params, const Layout& L);

// fp32 forward (k_fwd_head) of both nets on x [M][D]: logits [M][A] and / or values [M] (null: skipped)
int forward_fp32(const float* params, const Layout& L, const float* x, int M, int D, int A, float* logits,
                 float* values, hipStream_t s);

// 2-cloud split-fp16 rollouts: up to this many lanes one persistent k_sf_roll launch runs the whole
// rollout (each workgroup loops over the T steps of its 32 lanes: a latency design, c2's 4,096 lanes
// are 128 workgroups); above it each step is k_sf_fwd16 + k_sample_step over all lanes (c4: 131,072
// lanes, 24.5 -> 14.5 ms per rollout, profiles/r04c)
constexpr int SF_ROLL_FUSED_MAX_LANES = 16384;

}  // namespace rlks
