// Reward ensembles (`RewardEnsemble` / `AddSTDRewardWrapper`, rewards/reward_nets.py:884-1080) and active selection
// (`ActiveSelectionFragmenter`, algorithms/preference_comparisons.py:668-778) for gfx950: scoring rows with all M members
// in a number of launches that depends on neither M nor the number of steps or fragments.
//
//   A  ensemble_forward          raw[m][i] = member m's forward of row idx[i]            grid (tiles, M)
//   B  ensemble_norm_sequential  per member: `NormalizedRewardNet.predict_processed` step by step   grid (M)
//   C  ensemble_moments          mean / ddof-1 variance / mean + alpha * std over members, NumPy's float32 order
//   D  ensemble_pair_uncertainty `ActiveSelectionFragmenter.variance_estimate` of every candidate pair
//
// A: the members are a grid dimension. A workgroup is the relabel kernel's workgroup (relabel_tile.h: the same body, so
// the same bits) with member blockIdx.y's parameter and input-norm pointers, read from a fixed-size record in the kernel
// arguments. One member's weights fill the tile's static LDS (52 KB at H = 64), so members looping inside a workgroup
// would re-stage the weights behind two more barriers per member to save a gather of at most 64 x 64 floats that L2 serves;
// as a grid dimension the members' workgroups run side by side instead (three 52 KB workgroups fit a CU's 160 KB).
// No atomics; every sum has a fixed order.
#include "common.h"
#include "relabel_tile.h"
#include "rn_common.h"
#include "../../include/imitation_hip.h"

namespace {

struct EnsFwdArgs {
  RlTileArgs t;                                      // (P, mean, var: filled per member in the kernel)
  const float* P[IA_ENSEMBLE_MAX];
  const float* mean[IA_ENSEMBLE_MAX];
  const float* var[IA_ENSEMBLE_MAX];
  float* raw; long long ld;
};

template <int H1, int H2>
__global__ __launch_bounds__(RL_THREADS) void ensemble_forward_kernel(const EnsFwdArgs g) {
  const int m = blockIdx.y;
  RlTileArgs a = g.t;
  a.P = g.P[m]; a.mean = g.mean[m]; a.var = g.var[m];
  const long long i0 = (long long)blockIdx.x * RL_ROWS;
  long long t;
  const float rew = rl_tile_forward<H1, H2>(a, i0, t);
  const int lane = threadIdx.x & 63;
  if ((lane >> 4) == 0 && t >= 0) g.raw[m * g.ld + i0 + (threadIdx.x >> 6) * 16 + (lane & 15)] = rew;
}

struct EnsNormArgs {
  const float* raw; float* out; long long ld; int T, n, update;
  float* mean[IA_ENSEMBLE_MAX];
  float* var[IA_ENSEMBLE_MAX];
  int32_t* count[IA_ENSEMBLE_MAX];
  float eps[IA_ENSEMBLE_MAX];
};

// Block m is `reward_norm_seq_kernel` (mlp.hip) on member m's row: the same loops, the same reduction tree, the same Chan
// update -- the same values and final statistics. A member without an output norm is copied through.
__global__ __launch_bounds__(256) void ensemble_norm_seq_kernel(const EnsNormArgs g) {
  __shared__ float red[256];
  __shared__ float s_mean, s_var;
  __shared__ int s_cnt;
  const int tid = threadIdx.x, m = blockIdx.x;
  const int T = g.T, n = g.n, update = g.update;
  const float* __restrict__ raw = g.raw + m * g.ld;
  float* __restrict__ out = g.out + m * g.ld;
  float* mean = g.mean[m];
  if (mean == nullptr) {
    for (long long i = tid; i < (long long)T * n; i += 256) out[i] = raw[i];
    return;
  }
  float* var = g.var[m];
  int32_t* count = g.count[m];
  const float eps = g.eps[m];
  if (tid == 0) { s_mean = *mean; s_var = *var; s_cnt = *count; }
  __syncthreads();
  for (int t = 0; t < T; ++t) {
    const float mu = s_mean, inv = 1.f / sqrtf(s_var + eps);
    float sum = 0.f;
    for (int i = tid; i < n; i += 256) {
      const float r = raw[(long long)t * n + i];
      out[(long long)t * n + i] = (r - mu) * inv;
      sum += r;
    }
    if (!update) continue;
    red[tid] = sum;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) { if (tid < o) red[tid] += red[tid + o]; __syncthreads(); }
    const float bmean = red[0] / (float)n;
    __syncthreads();
    float q = 0.f;
    for (int i = tid; i < n; i += 256) {
      const float dl = raw[(long long)t * n + i] - bmean;
      q += dl * dl;
    }
    red[tid] = q;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) { if (tid < o) red[tid] += red[tid + o]; __syncthreads(); }
    if (tid == 0) {
      const float bvar = red[0] / (float)n;
      float mc = s_mean, vc = s_var;
      rn_absorb(mc, vc, s_cnt, n, bmean, bvar);
      s_mean = mc;
      s_var = vc;
      s_cnt = rn_count_add(s_cnt, n);
    }
    __syncthreads();
  }
  if (tid == 0 && update) { *mean = s_mean; *var = s_var; *count = s_cnt; }
}

// NumPy's float32 `x.mean(-1)` and `x.var(-1, ddof=1)` of the [R, M] matrix, M < 8 (from 8 members on NumPy's own sum is
// unrolled eight wide; this kernel keeps the index order): members summed in index order, true division by M, deviations
// from that mean, their squares summed in index order, true division by M - 1.
__global__ __launch_bounds__(256) void ensemble_moments_kernel(const float* __restrict__ x, long long ld, int M, long long R,
                                                                float alpha, float* __restrict__ mean,
                                                                float* __restrict__ var, float* __restrict__ bound) {
  const long long r = (long long)blockIdx.x * 256 + threadIdx.x;
  if (r >= R) return;
  float s = 0.f;
  for (int m = 0; m < M; ++m) s += x[m * ld + r];
  const float mu = s / (float)M;
  float q = 0.f;
  for (int m = 0; m < M; ++m) {
    const float d = x[m * ld + r] - mu;
    q += d * d;
  }
  const float v = q / (float)(M - 1);
  if (mean != nullptr) mean[r] = mu;
  if (var != nullptr) var[r] = v;
  if (bound != nullptr) bound[r] = mu + alpha * sqrtf(v);
}

__device__ __forceinline__ float ens_wave_sum(float v) {
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

// One wave per candidate pair, members one after the other: the lanes stride over the fragment's steps, a fixed butterfly
// reduces them (every lane ends with the same sum), and every lane then holds the member's statistic in a register.
//   logit        s_m = sum_t r1 - sum_t r2 (plain sums, no discount: :761-763); est = sum (s_m - mean)^2 / (M - 1)
//   probability  p_m = PreferenceModel.probability (:505-525; the arithmetic of pref.hip); est = sum (p_m - mean)^2 / M
//   label        p = mean of (p_m > 0.5); est = p * (1 - p)
__global__ __launch_bounds__(256) void ensemble_pair_uncertainty_kernel(const float* __restrict__ x, long long ld, int M,
                                                                         int P, int L, int mode, float gamma, float noise,
                                                                         float threshold, float* __restrict__ est) {
  const int lane = threadIdx.x & 63;
  const int p = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (p >= P) return;                                // (wave-uniform; no barrier below)
  const bool plain = (gamma == 1.f);
  float v[IA_ENSEMBLE_MAX];
#pragma unroll
  for (int m = 0; m < IA_ENSEMBLE_MAX; ++m) {
    v[m] = 0.f;
    if (m < M) {
      const float* r1 = x + m * ld + 2LL * p * L;
      const float* r2 = r1 + L;
      if (mode == IA_UNCERTAINTY_LOGIT) {
        float a = 0.f, b = 0.f;
        for (int t = lane; t < L; t += 64) { a += r1[t]; b += r2[t]; }
        v[m] = ens_wave_sum(a) - ens_wave_sum(b);
      } else {
        float d = 0.f;
        for (int t = lane; t < L; t += 64) {
          const float w = plain ? 1.f : powf(gamma, (float)t);
          d += w * (r2[t] - r1[t]);
        }
        d = ens_wave_sum(d);
        const float c = fminf(fmaxf(d, -threshold), threshold);
        const float mp = 1.f / (1.f + expf(c));
        const float pr = (noise * 0.5f) + (1.f - noise) * mp;
        v[m] = mode == IA_UNCERTAINTY_LABEL ? (pr > 0.5f ? 1.f : 0.f) : pr;
      }
    }
  }
  float s = 0.f;
#pragma unroll
  for (int m = 0; m < IA_ENSEMBLE_MAX; ++m)
    if (m < M) s += v[m];
  const float mu = s / (float)M;
  float e;
  if (mode == IA_UNCERTAINTY_LABEL) {
    e = mu * (1.f - mu);
  } else {
    float q = 0.f;
#pragma unroll
    for (int m = 0; m < IA_ENSEMBLE_MAX; ++m)
      if (m < M) {
        const float d = v[m] - mu;
        q += d * d;
      }
    e = q / (float)(mode == IA_UNCERTAINTY_LOGIT ? M - 1 : M);
  }
  if (lane == 0) est[p] = e;
}

inline int ens_width(int od, int ad, int us, int ua, int un, int ud) {
  return (us ? od : 0) + (ua ? ad : 0) + (un ? od : 0) + (ud ? 1 : 0);
}

}  // namespace

extern "C" int ia_ensemble_forward_ok(const ia_mlp_desc* const* descs, int n_members, int obs_dim, int act_dim,
                                      int use_state, int use_action, int use_next_state, int use_done) {
  if (!descs || n_members < 2 || n_members > IA_ENSEMBLE_MAX) return 0;
  for (int m = 0; m < n_members; ++m) {
    const ia_mlp_desc* d = descs[m];
    if (!ia_replay_relabel_ok(d, obs_dim, act_dim, use_state, use_action, use_next_state, use_done)) return 0;
    if (d->n_layers != descs[0]->n_layers || d->hidden_act != descs[0]->hidden_act) return 0;
    for (int l = 0; l <= d->n_layers; ++l)
      if (d->dims[l] != descs[0]->dims[l]) return 0;
  }
  return 1;
}

extern "C" int ia_ensemble_forward(const ia_ensemble_forward_args* a, void* stream) {
  if (!a || a->n < 0 || a->rows < 1 || !a->raw || a->ld < a->n) return IA_ERR_ARG;
  if (a->n_members < 2 || a->n_members > IA_ENSEMBLE_MAX) return IA_ERR_ARG;
  if ((a->act_i64 == nullptr) == (a->act_f32 == nullptr)) return IA_ERR_ARG;   // exactly one kind of action
  if (!a->obs || !a->next_obs || !a->done) return IA_ERR_ARG;
  for (int m = 0; m < a->n_members; ++m) {
    if (!a->desc[m] || !a->params[m]) return IA_ERR_ARG;
    if ((a->norm_mean[m] == nullptr) != (a->norm_var[m] == nullptr)) return IA_ERR_ARG;
  }
  if (!ia_ensemble_forward_ok(a->desc, a->n_members, a->obs_dim, a->act_dim, a->use_state, a->use_action,
                              a->use_next_state, a->use_done))
    return IA_ERR_UNSUPPORTED;
  if (a->idx == nullptr && a->n > a->rows) return IA_ERR_ARG;
  if (a->n == 0) return IA_OK;
  const long long blocks = (a->n + RL_ROWS - 1) / RL_ROWS;
  if (blocks > 0x7fffffffLL) return IA_ERR_ARG;
  EnsFwdArgs g{};
  g.t.obs = a->obs; g.t.next_obs = a->next_obs; g.t.act_f32 = a->act_f32; g.t.act_i64 = a->act_i64; g.t.done = a->done;
  g.t.ring_rows = a->rows; g.t.idx = a->idx; g.t.n = a->n;
  g.t.od = a->obs_dim; g.t.ad = a->act_dim;
  g.t.us = a->use_state; g.t.ua = a->use_action; g.t.un = a->use_next_state; g.t.ud = a->use_done;
  const ia_mlp_desc* d = a->desc[0];
  g.t.D = d->dims[0]; g.t.act = d->hidden_act; g.t.eps = a->norm_eps;
  for (int m = 0; m < a->n_members; ++m) {
    g.P[m] = a->params[m]; g.mean[m] = a->norm_mean[m]; g.var[m] = a->norm_var[m];
  }
  g.raw = a->raw; g.ld = a->ld;
  const int H1 = d->dims[1], H2 = d->dims[2];
  const dim3 grid((unsigned)blocks, (unsigned)a->n_members), block(RL_THREADS);
  hipStream_t st = (hipStream_t)stream;
  if (H1 == 32 && H2 == 32) hipLaunchKernelGGL((ensemble_forward_kernel<32, 32>), grid, block, 0, st, g);
  else if (H1 == 64 && H2 == 32) hipLaunchKernelGGL((ensemble_forward_kernel<64, 32>), grid, block, 0, st, g);
  else if (H1 == 32 && H2 == 64) hipLaunchKernelGGL((ensemble_forward_kernel<32, 64>), grid, block, 0, st, g);
  else hipLaunchKernelGGL((ensemble_forward_kernel<64, 64>), grid, block, 0, st, g);
  IA_CHECK_LAUNCH();
  return IA_OK;
}

extern "C" int ia_ensemble_norm_sequential(const ia_ensemble_norm_args* a, void* stream) {
  if (!a || !a->raw || !a->out || a->T <= 0 || a->n <= 0 || a->ld < (int64_t)a->T * a->n) return IA_ERR_ARG;
  if (a->n_members < 1 || a->n_members > IA_ENSEMBLE_MAX) return IA_ERR_ARG;
  EnsNormArgs g{};
  g.raw = a->raw; g.out = a->out; g.ld = a->ld; g.T = a->T; g.n = a->n; g.update = a->update_stats;
  for (int m = 0; m < a->n_members; ++m) {
    const bool has = a->mean[m] != nullptr;
    if (has != (a->var[m] != nullptr) || has != (a->count[m] != nullptr)) return IA_ERR_ARG;
    g.mean[m] = a->mean[m]; g.var[m] = a->var[m]; g.count[m] = a->count[m]; g.eps[m] = a->eps[m];
  }
  hipLaunchKernelGGL(ensemble_norm_seq_kernel, dim3(a->n_members), dim3(256), 0, (hipStream_t)stream, g);
  IA_CHECK_LAUNCH();
  return IA_OK;
}

extern "C" int ia_ensemble_moments(const float* norm, int64_t ld, int n_members, int64_t R, float alpha, float* mean,
                                   float* var, float* bound, void* stream) {
  if (!norm || R <= 0 || ld < R || n_members < 2 || n_members > IA_ENSEMBLE_MAX) return IA_ERR_ARG;
  const long long blocks = (R + 255) / 256;
  if (blocks > 0x7fffffffLL) return IA_ERR_ARG;
  hipLaunchKernelGGL(ensemble_moments_kernel, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, norm,
                     (long long)ld, n_members, (long long)R, alpha, mean, var, bound);
  IA_CHECK_LAUNCH();
  return IA_OK;
}

extern "C" int ia_ensemble_pair_uncertainty(const float* norm, int64_t ld, int n_members, int P, int L, int mode,
                                            float discount_factor, float noise_prob, float threshold, float* est,
                                            void* stream) {
  if (!norm || !est || P <= 0 || L <= 0 || n_members < 2 || n_members > IA_ENSEMBLE_MAX) return IA_ERR_ARG;
  if (ld < 2LL * P * L) return IA_ERR_ARG;
  if (mode != IA_UNCERTAINTY_LOGIT && mode != IA_UNCERTAINTY_PROBABILITY && mode != IA_UNCERTAINTY_LABEL) return IA_ERR_ARG;
  hipLaunchKernelGGL(ensemble_pair_uncertainty_kernel, dim3((unsigned)((P + 3) / 4)), dim3(256), 0, (hipStream_t)stream,
                     norm, (long long)ld, n_members, P, L, mode, discount_factor, noise_prob, threshold, est);
  IA_CHECK_LAUNCH();
  return IA_OK;
}
