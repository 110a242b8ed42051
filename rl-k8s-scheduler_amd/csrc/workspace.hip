// workspace.hip — descriptor checks, workspace layouts and the per-net argument blocks (workspace.h).
#include "workspace.h"

namespace rlks {

bool is_wide(const rlks_mlp_desc* d) { return d->precision == RLKS_PRECISION_WIDE || wide_needed(d); }
bool is_sf(const rlks_mlp_desc* d) {
  return d->precision == RLKS_PRECISION_SF16 || d->precision == RLKS_PRECISION_F16;
}

int check_desc(const rlks_mlp_desc* d) {
  RLKS_REQUIRE(d, RLKS_ERR_ARG, "null mlp desc");
  RLKS_REQUIRE(d->precision == RLKS_PRECISION_FP32 || d->precision == RLKS_PRECISION_SF16 ||
                   d->precision == RLKS_PRECISION_WIDE || d->precision == RLKS_PRECISION_F16, RLKS_ERR_ARG,
               "unknown precision");
  RLKS_REQUIRE(d->obs_dim > 0 && d->hidden > 0 && d->hidden % 32 == 0 && d->hidden <= 8192 && d->n_actions > 0 &&
                   d->n_actions <= 64, RLKS_ERR_UNSUPPORTED,
               "MLP: hidden must be a multiple of 32 (<= 8192), 1 <= n_actions <= 64");
  if (!is_wide(d))
    RLKS_REQUIRE(d->obs_dim <= DMAX && (d->n_actions == 2 || d->n_actions == 4 || d->n_actions == 8),
                 RLKS_ERR_UNSUPPORTED, "fused MLP kernels: obs_dim in [1, 32], 2, 4 or 8 actions");
  return RLKS_OK;
}

int pick_splits(int M) {
  // F2 grid = 4 tiles x 2 nets x S: about four workgroups per CU, >= 4 chunks of rows per split
  int s = 1;
  while (s * 2 * 8 <= 1024 && (M / (s * 2)) % BK == 0 && M / (s * 2) >= 4 * BK) s *= 2;
  return s;
}

Ws ws_layout(int D, int A, int M, char* base) {
  Ws w{};
  w.tiles = M / GB;
  w.splits = pick_splits(M);
  WsCursor c{base};
  for (int net = 0; net < 2; ++net) {
    const int An = net == 0 ? A : 1;
    NetWs& n = w.n[net];
    n.dz2 = c.take<float>(4LL * M * HID);
    n.part_b2 = c.take<float>(4LL * w.tiles * HID);
    n.part_w3 = c.take<float>(4LL * w.tiles * An * HID);
    n.part_b3 = c.take<float>(4LL * w.tiles * (net == 0 ? A : 2));  // value net: [tile][hi, lo] (vf_row)
    n.part_stat = c.take<float>(4LL * w.tiles * 4);
    n.part_w2 = c.take<float>(4LL * w.splits * HID * HID);
    n.part_w1 = c.take<float>(4LL * w.tiles * HID * D);
    n.part_b1 = c.take<float>(4LL * w.tiles * HID);
  }
  w.stat64 = c.take<double>(8 * 8);
  w.bytes = c.o;
  return w;
}

SfWs sf_ws_layout(int D, int A, int M, char* base) {
  SfWs w{};
  const int KD = sf_kd(D), tiles = M / 32;  // F2's 32-row tiles
  w.blocks = M / (16 * SF_F1_W);  // F1 workgroups of SF_F1_W x 16 rows
  w.fa_parts = sf_f1_parts(M, SF_F1_SPLIT);
  w.splits = 1;
  constexpr int F2_MAX_SPLITS = 128;  // F2 row splits per net (one 512-thread workgroup each)
  while (w.splits * 2 <= F2_MAX_SPLITS && tiles % (w.splits * 2) == 0) w.splits *= 2;
  w.tiles_per_split = tiles > 0 ? tiles / w.splits : 0;
  WsCursor c{base};
  // split weights of both nets first: their offsets do not depend on M (the rollout shares them)
  for (int net = 0; net < 2; ++net) {
    SfNetW& W = w.w[net];
    SfNet& n = w.n[net];
    W.w1h = c.take<_Float16>(2LL * HID * KD);
    W.w1l = c.take<_Float16>(2LL * HID * KD);
    W.w2ph = c.take<_Float16>(2LL * HID * HID);
    W.w2pl = c.take<_Float16>(2LL * HID * HID);
    W.w2th = c.take<_Float16>(2LL * HID * HID);
    W.w2tl = c.take<_Float16>(2LL * HID * HID);
    W.w2rh = c.take<_Float16>(2LL * HID * HID);
    W.w2rl = c.take<_Float16>(2LL * HID * HID);
    W.sc = c.take<float>(4 * 8);
    W.pmax = c.take<float>(4LL * 4 * SF_PMAX);
    W.tag = c.take<unsigned>(4 * 2);
    w.pmax_roll[net] = c.take<float>(4LL * 4 * SF_PMAX);
    n.w1h = W.w1h; n.w1l = W.w1l; n.w2ph = W.w2ph; n.w2pl = W.w2pl; n.w2th = W.w2th; n.w2tl = W.w2tl;
    n.sc = W.sc;
  }
  w.weight_bytes = c.o;
  for (int net = 0; net < 2; ++net) {
    const int An = net == 0 ? A : 1;
    SfNet& n = w.n[net];
    n.dz2s = c.take<_Float16>(4LL * M * HID);
    n.tile_edz = c.take<int>(4LL * (M / 16));
    n.tile_ex = c.take<int>(4LL * (M / 16));
    n.part_w1 = c.take<float>(4LL * w.blocks * HID * D);
    n.part_b1 = c.take<float>(4LL * w.blocks * HID);
    n.part_w3 = c.take<float>(4LL * w.fa_parts * An * HID);
    n.part_b3 = c.take<float>(4LL * w.fa_parts * (net == 0 ? A : 2));  // value net: [part][hi, lo] (vf_row)
    n.part_stat = c.take<float>(4LL * w.fa_parts * 4);
    n.part_w2 = c.take<float>(4LL * w.splits * SF_W2_PSTRIDE);
    n.part_b2 = c.take<float>(4LL * w.splits * HID);
  }
  w.stat64 = c.take<double>(8 * 8);
  w.xsp = c.take<_Float16>(2LL * 2 * M * KD);
  w.bytes = c.o;
  return w;
}

int sf_prep(const rlks_mlp_desc* d, const SfWs& w, const float* params, hipStream_t s, bool rollout, int parity,
            bool skip_wmax, unsigned expect_tag) {
  const int D = d->obs_dim;
  const Layout L = make_layout(D, HID, d->n_actions);
  SfPrepArgs pa{};
  pa.D = D;
  pa.KD = sf_kd(D);
  pa.parity = rollout ? 0 : parity;
  pa.skip_wmax = rollout ? 0 : (skip_wmax ? 1 : 0);
  pa.write_roll = rollout ? 1 : 0;
  pa.expect_tag = expect_tag;
  for (int net = 0; net < 2; ++net) {
    pa.n[net] = w.w[net];
    if (rollout) pa.n[net].pmax = w.pmax_roll[net];
    const NetPtrs P = net_ptrs_host(params, L, net);
    pa.n[net].w1 = P.w1; pa.n[net].b1 = P.b1; pa.n[net].w2 = P.w2;
  }
  return launch_sf_prep(pa, s);
}

void sf_nets(SfNet (&n)[2], const SfWs& w, const float* params, const Layout& L) {
  for (int net = 0; net < 2; ++net) {
    const NetPtrs P = net_ptrs_host(params, L, net);
    n[net] = w.n[net];
    n[net].b2 = P.b2; n[net].w3 = P.w3; n[net].b3 = P.b3;
  }
}

int forward_fp32(const float* params, const Layout& L, const float* x, int M, int D, int A, float* logits,
                 float* values, hipStream_t s) {
  for (int net = 0; net < 2; ++net) {
    float* out = net == 0 ? logits : values;
    if (!out) continue;
    FwdArgs f{};
    f.P = net_ptrs_host(params, L, net);
    f.x = x; f.x_stride = D; f.M = M; f.D = D; f.A_pi = A; f.out = out;
    if (int rc = launch_fwd_head(f, net, A, FWD_ONLY, s)) return rc;
  }
  return RLKS_OK;
}

}  // namespace rlks
