// Sample-time reward relabelling of a replay ring (`ReplayBufferRewardWrapper`), for gfx950, in ONE launch for all the
// minibatches of a `train` call: for each of n int64 ring indices the row is gathered from the ring columns, laid out as
// the reward net's input [state | action (one-hot if Discrete) | next_state | done] by its use_* flags, normalised with the
// frozen input statistics ((x - mean) / sqrt(var + eps)), run through D -> H1 -> H2 -> 1 (D <= 64; H1, H2 in {32, 64};
// ReLU or Tanh), normalised with the frozen scalar output statistics and stored to reward_col[idx]. Duplicate indices
// write equal values (a row's reward depends on nothing but the row and the parameters).
//
// The tile body (staging, gather, the MFMA layers) lives in relabel_tile.h, shared with ensemble.hip.
#include "common.h"
#include "relabel_tile.h"
#include "../../include/imitation_hip.h"

namespace {

struct RelabelArgs {
  RlTileArgs t;
  const float *omean, *ovar; float oeps;
  float* reward;
};

template <int H1, int H2>
__global__ __launch_bounds__(RL_THREADS) void replay_relabel_kernel(const RelabelArgs g) {
  long long t;
  float rew = rl_tile_forward<H1, H2>(g.t, (long long)blockIdx.x * RL_ROWS, t);
  if (g.omean != nullptr) rew = (rew - g.omean[0]) / sqrtf(g.ovar[0] + g.oeps);
  if ((threadIdx.x & 63) >> 4 == 0 && t >= 0) g.reward[t] = rew;
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
  g.t.obs = a->obs; g.t.next_obs = a->next_obs; g.t.act_f32 = a->act_f32; g.t.act_i64 = a->act_i64; g.t.done = a->done;
  g.t.ring_rows = a->ring_rows; g.t.idx = a->idx; g.t.n = a->n;
  g.t.od = a->obs_dim; g.t.ad = a->act_dim;
  g.t.us = a->use_state; g.t.ua = a->use_action; g.t.un = a->use_next_state; g.t.ud = a->use_done;
  g.t.D = a->desc->dims[0]; g.t.act = a->desc->hidden_act;
  g.t.P = a->params; g.t.mean = a->norm_mean; g.t.var = a->norm_var; g.t.eps = a->norm_eps;
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
