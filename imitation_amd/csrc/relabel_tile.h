// The 64-row tile of the one-launch reward forward shared by relabel.hip (`replay_relabel_kernel`) and ensemble.hip
// (`ensemble_forward_kernel`): gather by int64 row index, input norm, D -> H1 -> H2 -> 1 on v_mfma_f32_16x16x4_f32. Both
// kernels run THIS body, so a member's row of the ensemble forward is, bit for bit, the relabel kernel's result with that
// member's parameters: every sum has one fixed k order.
//
// One 256-thread workgroup takes 64 indices, one wave per 16-row tile. The parameters are staged once per workgroup in LDS
// (stride 68 floats: the 16 x 4 lanes of an operand read hit 64 distinct banks); the input tile is assembled in LDS one
// ELEMENT per load, so no read passes the last element of a table row (a table may end where its mapping ends). The layers
// run in the transposed form out^T = W . x^T: A = W[j][k], B = x[row][k], C[j = 4 * lk + reg][row = li]. A lane therefore
// holds, for its row li, the hidden units 16 jt + 4 lk + reg -- exactly a B operand of the next layer when that layer walks
// k in the order (jt, reg) with the matching column of W as A. The hidden activations stay in registers from the first
// layer to the reward.
#pragma once
#include "common.h"

constexpr int RL_ROWS = 64, RL_THREADS = 256, RL_DMAX = 64, RL_LD = 68;

struct RlTileArgs {
  const float *obs, *next_obs, *act_f32; const int64_t* act_i64; const float* done; long long ring_rows;
  const int64_t* idx; long long n;                 // idx null: rows 0 .. n - 1
  int od, ad, us, ua, un, ud, D, act;
  const float *P, *mean, *var; float eps;
};

// Returns the raw reward of tile row r = 16 * wave + (lane & 15) (all four lanes lk = lane >> 4 of a row hold it) and leaves
// that row's table index in `t_row` (-1: masked -- past n, or an index outside the table, which is never followed).
template <int H1, int H2>
__device__ __forceinline__ float rl_tile_forward(const RlTileArgs& g, long long i0, long long& t_row) {
  __shared__ float W1s[H1 * RL_LD];                 // [j][k] = W1[j][k], k < KP (columns D .. KP - 1 zero)
  __shared__ float W2s[H2 * RL_LD];                 // [j][k] = W2[j][k], k < H1
  __shared__ float Xs[RL_ROWS * RL_LD];             // the normalised input rows (masked rows: zeros)
  __shared__ float vec[H1 + 2 * H2 + 1];            // b1, b2, w3, b3
  __shared__ long long sidx[RL_ROWS];               // the table row of each tile row (-1: masked)
  const int tid = threadIdx.x;
  const int od = g.od, ad = g.ad, D = g.D;
  const int KP = (D + 3) & ~3;
  const int off_a = g.us ? od : 0, off_n = off_a + (g.ua ? ad : 0), off_d = off_n + (g.un ? od : 0);

  if (tid < RL_ROWS) {
    long long t = -1;
    if (i0 + tid < g.n) {                           // (no read past idx[n - 1])
      t = g.idx != nullptr ? g.idx[i0 + tid] : i0 + tid;
      if (t < 0 || t >= g.ring_rows) t = -1;        // an index outside the table is skipped, never followed
    }
    sidx[tid] = t;
  }
  // ---- the parameters into LDS
  for (int e = tid; e < H1 * KP; e += RL_THREADS) {
    const int j = e / KP, k = e - j * KP;
    W1s[j * RL_LD + k] = k < D ? g.P[j * D + k] : 0.f;
  }
  const float* P2 = g.P + H1 * D + H1;
  for (int e = tid; e < H2 * H1; e += RL_THREADS) {
    const int j = e / H1, k = e - j * H1;
    W2s[j * RL_LD + k] = P2[e];
  }
  const float* P3 = P2 + H2 * H1 + H2;
  if (tid < H1) vec[tid] = g.P[H1 * D + tid];
  if (tid < H2) {
    vec[H1 + tid] = P2[H2 * H1 + tid];
    vec[H1 + H2 + tid] = P3[tid];
  }
  if (tid == 0) vec[H1 + 2 * H2] = P3[H2];
  __syncthreads();

  // ---- the input tile: one element per load, normalised on the way in
  for (int e = tid; e < RL_ROWS * KP; e += RL_THREADS) {
    const int r = e / KP, k = e - r * KP;
    const long long t = sidx[r];
    float v = 0.f;
    if (t >= 0 && k < D) {
      if (k < off_a) v = g.obs[t * od + k];
      else if (k < off_n) v = g.act_i64 != nullptr ? (g.act_i64[t] == (long long)(k - off_a) ? 1.f : 0.f)
                                                   : g.act_f32[t * ad + (k - off_a)];
      else if (k < off_d) v = g.next_obs[t * od + (k - off_n)];
      else v = g.done[t];
      if (g.mean != nullptr) v = (v - g.mean[k]) / sqrtf(g.var[k] + g.eps);
    }
    Xs[r * RL_LD + k] = v;
  }
  __syncthreads();

  // ---- the layers: wave w owns rows 16 w .. 16 w + 15
  const int lane = tid & 63, li = lane & 15, lk = lane >> 4;
  const int r0 = (tid >> 6) * 16;
  constexpr int T1 = H1 / 16, T2 = H2 / 16;
  f32x4 h1[T1];
#pragma unroll
  for (int jt = 0; jt < T1; ++jt)
#pragma unroll
    for (int q = 0; q < 4; ++q) h1[jt][q] = vec[16 * jt + 4 * lk + q];
  const float* xrow = Xs + (r0 + li) * RL_LD + lk;
  for (int k = 0; k < KP; k += 4) {
    const float b = xrow[k];
#pragma unroll
    for (int jt = 0; jt < T1; ++jt)
      h1[jt] = __builtin_amdgcn_mfma_f32_16x16x4f32(W1s[(16 * jt + li) * RL_LD + k + lk], b, h1[jt], 0, 0, 0);
  }
#pragma unroll
  for (int jt = 0; jt < T1; ++jt)
#pragma unroll
    for (int q = 0; q < 4; ++q) h1[jt][q] = ia_apply_act(h1[jt][q], g.act);

  f32x4 h2[T2];
#pragma unroll
  for (int jt = 0; jt < T2; ++jt)
#pragma unroll
    for (int q = 0; q < 4; ++q) h2[jt][q] = vec[H1 + 16 * jt + 4 * lk + q];
#pragma unroll
  for (int kt = 0; kt < T1; ++kt)
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const float b = h1[kt][q];                    // hidden unit 16 kt + 4 lk + q of row li
#pragma unroll
      for (int jt = 0; jt < T2; ++jt)
        h2[jt] = __builtin_amdgcn_mfma_f32_16x16x4f32(W2s[(16 * jt + li) * RL_LD + 16 * kt + 4 * lk + q], b, h2[jt], 0, 0, 0);
    }
  float part = 0.f;
#pragma unroll
  for (int jt = 0; jt < T2; ++jt)
#pragma unroll
    for (int q = 0; q < 4; ++q)
      part = fmaf(vec[H1 + H2 + 16 * jt + 4 * lk + q], ia_apply_act(h2[jt][q], g.act), part);
  part += __shfl_xor(part, 16);
  part += __shfl_xor(part, 32);
  t_row = sidx[r0 + li];
  return part + vec[H1 + 2 * H2];
}
