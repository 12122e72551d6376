// One environment step of an off-policy generator (DQN / TD3 / DDPG) under a learned reward, for gfx950, in ONE launch:
// the step's n transitions are read once (from a pinned, device-mapped host record or from device memory), relabelled with
// the discriminator's reward and written to (a) rows ring_row .. ring_row + n - 1 of the learner's replay table, (b) the
// same rows of the trainer's per-round tile and (c) a pinned host array of rewards.
//
// The reward is the reference's default stack [state | action | next_state | done] (D <= 64) -> 32 -> 32 -> 1, ReLU, with the
// input RunningNorm in eval mode ((x - mean) * (1 / sqrt(var + eps)), as disc32_rows_kernel forms it) and an output
// activation. The kernel is latency bound: n is 1 .. 1024 rows and a row costs 32 * (D + 33) fused multiply-adds, while its
// inputs come over PCIe. On gfx950 the fp32 MFMA runs at the vector rate, so the matrix cores would buy nothing for a 16-row
// block and cost a fragment shuffle; the dots are VALU fmaf chains. One 512-thread workgroup takes OP_ROWS = 16 rows: thread
// (r, j) = (tid / 32, tid % 32) owns hidden unit j of row r, every sum is one chain per output in a fixed order of k, so a
// row's reward depends on neither the other rows nor n. No atomics, no waiting on host memory; every store is a plain
// vector store.
#include "common.h"
#include "../../include/imitation_hip.h"

bool ia_disc32_shape_ok(const ia_mlp_desc* d, int ldx);   // airl_fused.hip

namespace {

constexpr int OP_ROWS = 16, OP_H = 32, OP_DMAX = 64, OP_THREADS = OP_ROWS * OP_H;
constexpr int OP_XS = OP_DMAX + 1, OP_HS = OP_H + 1;      // odd LDS strides

struct StepArgs {
  const float *obs, *next_obs; const int64_t* act_i64; const float *act_f32, *ring_act_in; const uint8_t* dones;
  const float* ring_done_in;
  int n, od, ad, us, ua, un, ud, D;
  const float *P, *mean, *var; float eps; int out_act, has_net;
  const float* rewards_in;
  float *ring_obs, *ring_next; int64_t* ring_act_i64; float *ring_act_f32, *ring_reward, *ring_done; long long ring_row;
  float *tile_obs, *tile_next; int64_t* tile_act_i64; float* tile_act_f32; uint8_t* tile_dones; long long tile_row;
  float* rewards_host;
};

__global__ __launch_bounds__(OP_THREADS) void offpolicy_step_kernel(const StepArgs g) {
  __shared__ float W1s[OP_DMAX * OP_HS];                  // [k][j]: W1[j][k]
  __shared__ float W2s[OP_H * OP_HS];                     // [k][j]: W2[j][k]
  __shared__ float vec[3 * OP_H + 1];                     // b1, b2, w3, b3
  __shared__ float nm[OP_DMAX], ni[OP_DMAX];              // mean, 1 / sqrt(var + eps)
  __shared__ float X[OP_ROWS * OP_XS];                    // raw, then normalised inputs of the block's rows
  __shared__ float H1[OP_ROWS * OP_HS], H2[OP_ROWS * OP_HS];
  const int tid = threadIdx.x;
  const int i0 = blockIdx.x * OP_ROWS;
  const int rows = min(OP_ROWS, g.n - i0);
  const int od = g.od, ad = g.ad, D = g.D;
  const bool tile = g.tile_obs != nullptr;
  const int off_a = g.us ? od : 0, off_n = off_a + (g.ua ? ad : 0), off_d = off_n + (g.un ? od : 0);

  // ---- the weights into LDS (device memory; their loads are in flight while the rows cross PCIe)
  if (g.has_net) {
    for (int e = tid; e < OP_H * D; e += OP_THREADS) {
      const int j = e / D, k = e - j * D;
      W1s[k * OP_HS + j] = g.P[e];
    }
    const float* P2 = g.P + OP_H * D + OP_H;
    for (int e = tid; e < OP_H * OP_H; e += OP_THREADS) W2s[(e & (OP_H - 1)) * OP_HS + (e >> 5)] = P2[e];
    if (tid < OP_H) {
      vec[tid] = g.P[OP_H * D + tid];
      vec[OP_H + tid] = P2[OP_H * OP_H + tid];
      vec[2 * OP_H + tid] = P2[OP_H * OP_H + OP_H + tid];
    }
    if (tid == 0) vec[3 * OP_H] = P2[OP_H * OP_H + 2 * OP_H];
    if (tid < D) {
      const bool hn = g.mean != nullptr;
      nm[tid] = hn ? g.mean[tid] : 0.f;
      ni[tid] = hn ? 1.f / sqrtf(g.var[tid] + g.eps) : 1.f;
    }
  }

  // ---- the rows: read once, stored to the ring and the tile as they are, and into the input tile
  const int n_obs = rows * od;
  for (int e = tid; e < n_obs; e += OP_THREADS) {
    const int r = e / od, k = e - r * od;
    const long long src = (long long)i0 * od + e;
    const float v = g.obs[src], w = g.next_obs[src];
    g.ring_obs[(g.ring_row + i0) * od + e] = v;
    g.ring_next[(g.ring_row + i0) * od + e] = w;
    if (tile) {
      g.tile_obs[(g.tile_row + i0) * od + e] = v;
      g.tile_next[(g.tile_row + i0) * od + e] = w;
    }
    if (g.has_net) {
      if (g.us) X[r * OP_XS + k] = v;
      if (g.un) X[r * OP_XS + off_n + k] = w;
    }
  }
  if (g.act_i64 != nullptr) {
    if (tid < rows) {
      const long long a = g.act_i64[i0 + tid];
      g.ring_act_i64[g.ring_row + i0 + tid] = a;
      if (tile) g.tile_act_i64[g.tile_row + i0 + tid] = a;
      if (g.has_net && g.ua)
        for (int j = 0; j < ad; ++j) X[tid * OP_XS + off_a + j] = a == j ? 1.f : 0.f;   // one-hot
    }
  } else {
    for (int e = tid; e < rows * ad; e += OP_THREADS) {
      const int r = e / ad, k = e - r * ad;
      const long long src = (long long)i0 * ad + e;
      const float v = g.act_f32[src];
      g.ring_act_f32[(g.ring_row + i0) * ad + e] = g.ring_act_in != nullptr ? g.ring_act_in[src] : v;
      if (tile) g.tile_act_f32[(g.tile_row + i0) * ad + e] = v;
      if (g.has_net && g.ua) X[r * OP_XS + off_a + k] = v;
    }
  }
  if (tid < rows) {
    const uint8_t d = g.dones[i0 + tid];
    g.ring_done[g.ring_row + i0 + tid] = g.ring_done_in[i0 + tid];
    if (tile) g.tile_dones[g.tile_row + i0 + tid] = d;
    if (g.has_net && g.ud) X[tid * OP_XS + off_d] = d ? 1.f : 0.f;
  }
  if (!g.has_net) {   // (kernel argument: uniform) another reward net's device-resident prediction
    if (tid < rows) {
      const float rew = g.rewards_in[i0 + tid];
      g.ring_reward[g.ring_row + i0 + tid] = rew;
      if (g.rewards_host != nullptr) g.rewards_host[i0 + tid] = rew;
    }
    return;
  }
  __syncthreads();

  // ---- normalise, then the three layers, every sum in the order disc32_rows_kernel (airl_fused.hip) walks it on the
  // 32x32x2 matrix instruction -- bias first, then per group of eight inputs k, k + 4, k + 1, k + 5, ... as one fmaf chain
  // (columns past D carry zeros there as here); the output layer as two 16-term sums of rounded products -- so that this
  // launch and the tile relabelling (`ia_disc_fused_predict`) agree on a row's reward.
  const int C8 = (D + 7) >> 3;
  for (int e = tid; e < rows * 8 * C8; e += OP_THREADS) {
    const int r = e / (8 * C8), k = e - r * (8 * C8);
    X[r * OP_XS + k] = k < D ? (X[r * OP_XS + k] - nm[k]) * ni[k] : 0.f;
  }
  for (int e = tid; e < (8 * C8 - D) * OP_H; e += OP_THREADS) W1s[(D + (e >> 5)) * OP_HS + (e & (OP_H - 1))] = 0.f;
  __syncthreads();
  const int r = tid >> 5, j = tid & (OP_H - 1);
  const bool live = r < rows;
  if (live) {
    float acc = vec[j];
    const float* x = X + r * OP_XS;
    for (int q = 0; q < C8; ++q)
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        const int k = 8 * q + u;
        acc = fmaf(W1s[k * OP_HS + j], x[k], acc);
        acc = fmaf(W1s[(k + 4) * OP_HS + j], x[k + 4], acc);
      }
    H1[r * OP_HS + j] = fmaxf(acc, 0.f);
  }
  __syncthreads();
  if (live) {
    float acc = vec[OP_H + j];
    const float* h = H1 + r * OP_HS;
#pragma unroll
    for (int q = 0; q < OP_H / 8; ++q)
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        const int k = 8 * q + u;
        acc = fmaf(W2s[k * OP_HS + j], h[k], acc);
        acc = fmaf(W2s[(k + 4) * OP_HS + j], h[k + 4], acc);
      }
    H2[r * OP_HS + j] = fmaxf(acc, 0.f);
  }
  __syncthreads();
  if (tid < rows) {
    const float* h = H2 + tid * OP_HS;
    const float* w3 = vec + 2 * OP_H;
    float s0 = 0.f, s1 = 0.f;
#pragma unroll
    for (int t = 0; t < 16; ++t) {
      const int f = 8 * (t >> 2) + (t & 3);
      s0 = __fadd_rn(s0, __fmul_rn(h[f], w3[f]));
      s1 = __fadd_rn(s1, __fmul_rn(h[f + 4], w3[f + 4]));
    }
    const float acc = __fadd_rn(vec[3 * OP_H], __fadd_rn(s0, s1));
    const float rew = ia_apply_act(acc, g.out_act);
    g.ring_reward[g.ring_row + i0 + tid] = rew;
    if (g.rewards_host != nullptr) g.rewards_host[i0 + tid] = rew;
  }
}

inline int input_width(int od, int ad, int us, int ua, int un, int ud) {
  return (us ? od : 0) + (ua ? ad : 0) + (un ? od : 0) + (ud ? 1 : 0);
}

}  // namespace

extern "C" int ia_offpolicy_step_rows(void) { return OP_ROWS; }

extern "C" int ia_offpolicy_step_ok(const ia_mlp_desc* d, int obs_dim, int act_dim, int use_state, int use_action,
                                    int use_next_state, int use_done) {
  if (!d || obs_dim < 1 || act_dim < 1) return 0;
  const int D = input_width(obs_dim, act_dim, use_state, use_action, use_next_state, use_done);
  return D >= 1 && D <= OP_DMAX && d->dims[0] == D && ia_disc32_shape_ok(d, (D + 3) / 4 * 4) ? 1 : 0;
}

extern "C" int ia_offpolicy_step(const ia_offpolicy_step_args* a, void* stream) {
  if (!a || a->n <= 0 || a->obs_dim < 1 || a->act_dim < 1 || !a->obs || !a->next_obs || !a->dones || !a->ring_done)
    return IA_ERR_ARG;
  if ((a->act_i64 == nullptr) == (a->act_f32 == nullptr)) return IA_ERR_ARG;   // exactly one kind of action
  if (a->act_i64 && a->ring_act_f32) return IA_ERR_ARG;
  if (!a->ring_obs || !a->ring_next_obs || !a->ring_reward || !a->ring_done_out) return IA_ERR_ARG;
  if (a->act_i64 ? !a->ring_action_i64 : !a->ring_action_f32) return IA_ERR_ARG;
  if (a->ring_row < 0 || a->ring_row + a->n > a->ring_rows) return IA_ERR_ARG;   // the rows stay inside the table
  if (a->tile_obs) {
    if (!a->tile_next_obs || !a->tile_dones || (a->act_i64 ? !a->tile_act_i64 : !a->tile_act_f32)) return IA_ERR_ARG;
    if (a->tile_row < 0 || a->tile_row + a->n > a->tile_rows) return IA_ERR_ARG;
  }
  if (a->desc) {
    if (!a->params) return IA_ERR_ARG;
    if (!ia_offpolicy_step_ok(a->desc, a->obs_dim, a->act_dim, a->use_state, a->use_action, a->use_next_state,
                              a->use_done))
      return IA_ERR_UNSUPPORTED;
    if ((a->norm_mean == nullptr) != (a->norm_var == nullptr)) return IA_ERR_ARG;
  } else if (!a->rewards_in) {
    return IA_ERR_ARG;
  }
  StepArgs g{};
  g.obs = a->obs; g.next_obs = a->next_obs; g.act_i64 = a->act_i64; g.act_f32 = a->act_f32;
  g.ring_act_in = a->ring_act_f32; g.dones = a->dones; g.ring_done_in = a->ring_done;
  g.n = a->n; g.od = a->obs_dim; g.ad = a->act_dim;
  g.us = a->use_state; g.ua = a->use_action; g.un = a->use_next_state; g.ud = a->use_done;
  g.has_net = a->desc != nullptr;
  g.D = g.has_net ? a->desc->dims[0] : 0;
  g.P = a->params; g.mean = a->norm_mean; g.var = a->norm_var; g.eps = a->norm_eps; g.out_act = a->out_act;
  g.rewards_in = a->rewards_in;
  g.ring_obs = a->ring_obs; g.ring_next = a->ring_next_obs; g.ring_act_i64 = a->ring_action_i64;
  g.ring_act_f32 = a->ring_action_f32; g.ring_reward = a->ring_reward; g.ring_done = a->ring_done_out;
  g.ring_row = a->ring_row;
  g.tile_obs = a->tile_obs; g.tile_next = a->tile_next_obs; g.tile_act_i64 = a->tile_act_i64;
  g.tile_act_f32 = a->tile_act_f32; g.tile_dones = a->tile_dones; g.tile_row = a->tile_row;
  g.rewards_host = a->rewards_host;
  hipLaunchKernelGGL(offpolicy_step_kernel, dim3((a->n + OP_ROWS - 1) / OP_ROWS), dim3(OP_THREADS), 0,
                     (hipStream_t)stream, g);
  IA_CHECK_LAUNCH();
  return IA_OK;
}
