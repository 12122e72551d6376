// Sample-time reward relabelling of a replay ring (`ReplayBufferRewardWrapper`), for gfx950, in ONE launch for all the
// minibatches of a `train` call: for each of n int64 ring indices the row is gathered from the ring columns, laid out as
// the reward net's input [state | action (one-hot if Discrete) | next_state | done] by its use_* flags, normalised with the
// frozen input statistics ((x - mean) / sqrt(var + eps)), run through D -> H1 -> H2 -> 1 (D <= 64; H1, H2 in {32, 64};
// ReLU or Tanh), normalised with the frozen scalar output statistics and stored to reward_col[idx]. Duplicate indices
// write equal values (a row's reward depends on nothing but the row and the parameters).
//
// One 256-thread workgroup takes 64 indices, one wave per 16-row tile. The parameters are staged once per workgroup in LDS
// (stride 68 floats: the 16 x 4 lanes of an operand read hit 64 distinct banks); the input tile is assembled in LDS one
// ELEMENT per load, so no read passes the last element of a ring row (a table may end where its mapping ends). The layers
// run on v_mfma_f32_16x16x4_f32 (exact fp32, a k-ordered fmaf chain) in the transposed form out^T = W . x^T: A = W[j][k],
// B = x[row][k], C[j = 4 * lk + reg][row = li]. A lane therefore holds, for its row li, the hidden units 16 jt + 4 lk + reg
// -- exactly a B operand of the next layer when that layer walks k in the order (jt, reg) with the matching column of W as
// A. The hidden activations stay in registers from the first layer to the reward.
#include "common.h"
#include "../../include/imitation_hip.h"

namespace {

constexpr int RL_ROWS = 64, RL_THREADS = 256, RL_DMAX = 64, RL_LD = 68;

struct RelabelArgs {
  const float *obs, *next_obs, *act_f32; const int64_t* act_i64; const float* done; long long ring_rows;
  const int64_t* idx; long long n;
  int od, ad, us, ua, un, ud, D, act;
  const float *P, *mean, *var; float eps;
  const float *omean, *ovar; float oeps;
  float* reward;
};

template <int H1, int H2>
__global__ __launch_bounds__(RL_THREADS) void replay_relabel_kernel(const RelabelArgs g) {
  __shared__ float W1s[H1 * RL_LD];                 // [j][k] = W1[j][k], k < KP (columns D .. KP - 1 zero)
  __shared__ float W2s[H2 * RL_LD];                 // [j][k] = W2[j][k], k < H1
  __shared__ float Xs[RL_ROWS * RL_LD];             // the normalised input rows (masked rows: zeros)
  __shared__ float vec[H1 + 2 * H2 + 1];            // b1, b2, w3, b3
  __shared__ long long sidx[RL_ROWS];               // the ring row of each tile row (-1: masked)
  const int tid = threadIdx.x;
  const long long i0 = (long long)blockIdx.x * RL_ROWS;
  const int od = g.od, ad = g.ad, D = g.D;
  const int KP = (D + 3) & ~3;
  const int off_a = g.us ? od : 0, off_n = off_a + (g.ua ? ad : 0), off_d = off_n + (g.un ? od : 0);

  if (tid < RL_ROWS) {
    long long t = -1;
    if (i0 + tid < g.n) {                           // (no read past idx[n - 1])
      t = g.idx[i0 + tid];
      if (t < 0 || t >= g.ring_rows) t = -1;        // an index outside the ring is skipped, never followed
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
  float rew = part + vec[H1 + 2 * H2];
  if (g.omean != nullptr) rew = (rew - g.omean[0]) / sqrtf(g.ovar[0] + g.oeps);
  const long long t = sidx[r0 + li];
  if (lk == 0 && t >= 0) g.reward[t] = rew;
}

// ---- every other stack: one thread per row, the whole forward in float64 -------------------------------------------------
// Any D -> h1 -> ... -> 1 stack of up to IA_MAX_LAYERS layers. A thread gathers its row (one element per load, as above),
// normalises it and walks the layers with float64 inputs, accumulators and activations, so the stored float32 reward is the
// rounding of the float64 forward: no summation order enters it, and one row alone is as accurate as many. The two
// activation buffers of a thread live in a float64 workspace laid out [buffer][unit][thread] (coalesced); the grid is
// capped at RG_MAX_THREADS threads, which stride over the rows, so the workspace does not grow with n. This is the fall-back
// of shapes the MFMA kernel does not cover and of IA_RELABEL_FUSED=0: a row costs its multiply-adds on one lane.
constexpr int RG_BLOCK = 256, RG_MAX_THREADS = 8192;

struct GeneralArgs {
  const float *obs, *next_obs, *act_f32; const int64_t* act_i64; const float* done; long long ring_rows;
  const int64_t* idx; long long n;
  int od, ad, us, ua, un, ud, act, n_layers;
  int dims[IA_MAX_LAYERS + 1];
  const float *P, *mean, *var; double eps;
  const float *omean, *ovar; double oeps;
  float* reward; double* ws; int maxw; long long threads;
};

__device__ __forceinline__ double rg_act(double x, int act) {
  return act == IA_ACT_RELU ? fmax(x, 0.0) : act == IA_ACT_TANH ? tanh(x) : x;
}

__global__ __launch_bounds__(RG_BLOCK) void replay_relabel_general_kernel(const GeneralArgs g) {
  const long long me = (long long)blockIdx.x * RG_BLOCK + threadIdx.x;
  if (me >= g.threads) return;
  const int od = g.od, ad = g.ad, D = g.dims[0];
  const int off_a = g.us ? od : 0, off_n = off_a + (g.ua ? ad : 0), off_d = off_n + (g.un ? od : 0);
  const long long S = g.threads;                       // stride between a thread's consecutive units
  for (long long i = me; i < g.n; i += S) {
    const long long t = g.idx[i];
    if (t < 0 || t >= g.ring_rows) continue;           // an index outside the ring is skipped, never followed
    double* a = g.ws + me;
    double* b = g.ws + (long long)g.maxw * S + me;
    for (int k = 0; k < D; ++k) {
      float v;
      if (k < off_a) v = g.obs[t * od + k];
      else if (k < off_n) v = g.act_i64 != nullptr ? (g.act_i64[t] == (long long)(k - off_a) ? 1.f : 0.f)
                                                   : g.act_f32[t * ad + (k - off_a)];
      else if (k < off_d) v = g.next_obs[t * od + (k - off_n)];
      else v = g.done[t];
      double x = (double)v;
      if (g.mean != nullptr) x = (x - (double)g.mean[k]) / sqrt((double)g.var[k] + g.eps);
      a[k * S] = x;
    }
    const float* W = g.P;
    for (int l = 0; l < g.n_layers; ++l) {
      const int in = g.dims[l], out = g.dims[l + 1];
      const float* bias = W + (long long)in * out;
      const bool last = l == g.n_layers - 1;
      for (int j = 0; j < out; ++j) {
        double acc = (double)bias[j];
        const float* w = W + (long long)j * in;
        for (int k = 0; k < in; ++k) acc = fma((double)w[k], a[k * S], acc);
        b[j * S] = last ? acc : rg_act(acc, g.act);
      }
      double* s = a; a = b; b = s;
      W = bias + out;
    }
    double r = a[0];
    if (g.omean != nullptr) r = (r - (double)g.omean[0]) / sqrt((double)g.ovar[0] + g.oeps);
    g.reward[t] = (float)r;
  }
}

inline int input_width(int od, int ad, int us, int ua, int un, int ud) {
  return (us ? od : 0) + (ua ? ad : 0) + (un ? od : 0) + (ud ? 1 : 0);
}

inline long long general_threads(long long n) {
  const long long t = (n + RG_BLOCK - 1) / RG_BLOCK * RG_BLOCK;
  return t < RG_MAX_THREADS ? t : RG_MAX_THREADS;
}

inline int general_maxw(const ia_mlp_desc* d) {
  int m = 1;
  for (int l = 0; l <= d->n_layers; ++l) m = d->dims[l] > m ? d->dims[l] : m;
  return m;
}

inline bool general_ok(const ia_mlp_desc* d, int od, int ad, int us, int ua, int un, int ud) {
  if (!d || od < 1 || ad < 1 || d->n_layers < 1 || d->n_layers > IA_MAX_LAYERS) return false;
  for (int l = 0; l <= d->n_layers; ++l)
    if (d->dims[l] < 1) return false;
  return d->dims[0] == input_width(od, ad, us, ua, un, ud) && d->dims[d->n_layers] == 1;
}

}  // namespace

extern "C" int64_t ia_replay_relabel_general_ws_doubles(const ia_mlp_desc* d, int64_t n) {
  if (!d || n < 1 || d->n_layers < 1 || d->n_layers > IA_MAX_LAYERS) return 0;
  return 2LL * general_maxw(d) * general_threads(n);
}

extern "C" int ia_replay_relabel_general(const ia_replay_relabel_args* a, double norm_eps, double out_eps, double* ws,
                                         int64_t ws_doubles, void* stream) {
  if (!a || a->n < 0 || a->ring_rows < 1 || !a->idx || !a->reward || !a->desc || !a->params || !ws) return IA_ERR_ARG;
  if ((a->act_i64 == nullptr) == (a->act_f32 == nullptr)) return IA_ERR_ARG;   // exactly one kind of action
  if (!a->obs || !a->next_obs || !a->done) return IA_ERR_ARG;
  if ((a->norm_mean == nullptr) != (a->norm_var == nullptr) || (a->out_mean == nullptr) != (a->out_var == nullptr))
    return IA_ERR_ARG;
  if (!general_ok(a->desc, a->obs_dim, a->act_dim, a->use_state, a->use_action, a->use_next_state, a->use_done))
    return IA_ERR_UNSUPPORTED;
  if (a->desc->hidden_act != IA_ACT_NONE && a->desc->hidden_act != IA_ACT_RELU && a->desc->hidden_act != IA_ACT_TANH)
    return IA_ERR_UNSUPPORTED;
  if (a->n == 0) return IA_OK;
  if (ws_doubles < ia_replay_relabel_general_ws_doubles(a->desc, a->n)) return IA_ERR_ARG;   // the workspace holds every unit
  GeneralArgs g{};
  g.obs = a->obs; g.next_obs = a->next_obs; g.act_f32 = a->act_f32; g.act_i64 = a->act_i64; g.done = a->done;
  g.ring_rows = a->ring_rows; g.idx = a->idx; g.n = a->n;
  g.od = a->obs_dim; g.ad = a->act_dim;
  g.us = a->use_state; g.ua = a->use_action; g.un = a->use_next_state; g.ud = a->use_done;
  g.act = a->desc->hidden_act; g.n_layers = a->desc->n_layers;
  for (int l = 0; l <= g.n_layers; ++l) g.dims[l] = a->desc->dims[l];
  g.P = a->params; g.mean = a->norm_mean; g.var = a->norm_var; g.eps = norm_eps;
  g.omean = a->out_mean; g.ovar = a->out_var; g.oeps = out_eps;
  g.reward = a->reward; g.ws = ws; g.maxw = general_maxw(a->desc); g.threads = general_threads(a->n);
  hipLaunchKernelGGL(replay_relabel_general_kernel, dim3((unsigned)(g.threads / RG_BLOCK)), dim3(RG_BLOCK), 0,
                     (hipStream_t)stream, g);
  IA_CHECK_LAUNCH();
  return IA_OK;
}

extern "C" int ia_replay_relabel_ok(const ia_mlp_desc* d, int obs_dim, int act_dim, int use_state, int use_action,
                                    int use_next_state, int use_done) {
  if (!d || obs_dim < 1 || act_dim < 1 || d->n_layers != 3) return 0;
  const int D = input_width(obs_dim, act_dim, use_state, use_action, use_next_state, use_done);
  if (D < 1 || D > RL_DMAX || d->dims[0] != D || d->dims[3] != 1) return 0;
  if ((d->dims[1] != 32 && d->dims[1] != 64) || (d->dims[2] != 32 && d->dims[2] != 64)) return 0;
  return d->hidden_act == IA_ACT_RELU || d->hidden_act == IA_ACT_TANH ? 1 : 0;
}

extern "C" int ia_replay_relabel(const ia_replay_relabel_args* a, void* stream) {
  if (!a || a->n < 0 || a->ring_rows < 1 || !a->idx || !a->reward || !a->desc || !a->params) return IA_ERR_ARG;
  if ((a->act_i64 == nullptr) == (a->act_f32 == nullptr)) return IA_ERR_ARG;   // exactly one kind of action
  if (!a->obs || !a->next_obs || !a->done) return IA_ERR_ARG;
  if ((a->norm_mean == nullptr) != (a->norm_var == nullptr) || (a->out_mean == nullptr) != (a->out_var == nullptr))
    return IA_ERR_ARG;
  if (!ia_replay_relabel_ok(a->desc, a->obs_dim, a->act_dim, a->use_state, a->use_action, a->use_next_state, a->use_done))
    return IA_ERR_UNSUPPORTED;
  if (a->n == 0) return IA_OK;
  const long long blocks = (a->n + RL_ROWS - 1) / RL_ROWS;
  if (blocks > 0x7fffffffLL) return IA_ERR_ARG;
  RelabelArgs g{};
  g.obs = a->obs; g.next_obs = a->next_obs; g.act_f32 = a->act_f32; g.act_i64 = a->act_i64; g.done = a->done;
  g.ring_rows = a->ring_rows; g.idx = a->idx; g.n = a->n;
  g.od = a->obs_dim; g.ad = a->act_dim;
  g.us = a->use_state; g.ua = a->use_action; g.un = a->use_next_state; g.ud = a->use_done;
  g.D = a->desc->dims[0]; g.act = a->desc->hidden_act;
  g.P = a->params; g.mean = a->norm_mean; g.var = a->norm_var; g.eps = a->norm_eps;
  g.omean = a->out_mean; g.ovar = a->out_var; g.oeps = a->out_eps;
  g.reward = a->reward;
  const int H1 = a->desc->dims[1], H2 = a->desc->dims[2];
  const dim3 grid((unsigned)blocks), block(RL_THREADS);
  hipStream_t st = (hipStream_t)stream;
  if (H1 == 32 && H2 == 32) hipLaunchKernelGGL((replay_relabel_kernel<32, 32>), grid, block, 0, st, g);
  else if (H1 == 64 && H2 == 32) hipLaunchKernelGGL((replay_relabel_kernel<64, 32>), grid, block, 0, st, g);
  else if (H1 == 32 && H2 == 64) hipLaunchKernelGGL((replay_relabel_kernel<32, 64>), grid, block, 0, st, g);
  else hipLaunchKernelGGL((replay_relabel_kernel<64, 64>), grid, block, 0, st, g);
  IA_CHECK_LAUNCH();
  return IA_OK;
}
