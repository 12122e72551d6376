// The DAgger collection step for gfx950: for one tile of observations, the EXPERT's deterministic action for every
// row (the label that is stored) and the LEARNER's sampled action for the rows a host-drawn mask hands to the
// "robot" (what the environment executes there), in one launch.
//
// Same structure as the rollout step of policy.hip (`policy_act_body`): one 512-thread workgroup per 64 rows, wave
// (tower, q) takes rows q*16 .. q*16+15 of its tower through both tanh layers and the head on the fp32 16x16x4 MFMA
// path without block barriers after the feature staging. There the two towers are the policy and the value tower of
// ONE policy; here tower 0 is the expert's policy tower + action head and tower 1 the learner's -- two parameter
// buffers, two sets of feature-normalisation statistics (either may be absent), no value tower, no log-probability.
// The observation tile is read ONCE (it may live in device-mapped host memory) and normalised into one LDS tile per
// tower. Per row, every expression is the one the act kernel evaluates, in the same order: `expert_act` carries the
// bits of `ia_policy_act` with zero noise (Box) / negative uniform (Discrete), the learner's rows the bits of
// `ia_policy_act` with the same noise; a row's result depends on neither the other rows of the tile nor on n.
// Optionally the step appends (observation, expert action) to a device-resident table at rows base_row + i.
#include "common.h"
#include "../../include/imitation_hip.h"
#include "policy_common.h"

namespace {

template <int H>
struct DLds {   // floats; odd strides as in the act body
  static constexpr int XS = MAXD + 1, HS = H + 1, AS = MAXA + 1;
  static constexpr int x = 0;                          // [2 towers][ROWS][XS]: each tower's normalised features
  static constexpr int a1 = x + 2 * ROWS * XS;         // [2][ROWS][HS]
  static constexpr int a2 = a1 + 2 * ROWS * HS;
  static constexpr int out = a2 + 2 * ROWS * HS;       // [2][ROWS][AS]
  static constexpr int total = out + 2 * ROWS * AS;
};

struct DaggerArgs {
  ia_policy_desc de, dl;                               // expert, learner (same obs_dim / act_dim / hidden / discrete)
  const float *Pe, *Pte, *nme, *nve;
  const float *Pl, *Ptl, *nml, *nvl;
  const float* obs; int n;
  const uint8_t* mask;                                 // [n]: != 0 -> the learner acts
  const float* noise;                                  // [n, A] standard normal (Box) / [n] uniform (Discrete, inverse CDF)
  const float *low, *high;
  float* expert_act; float* actual_act;                // [n, A] (Box) / [n] (Discrete: the index as a float)
  float* logits;                                       // non-null: the learner's head outputs [n, A]; nothing is sampled
  float* tab_obs; float* tab_acts; long long base_row; // non-null: table rows base_row + i <- (obs[i], expert_act[i])
};

template <int H>
__global__ __launch_bounds__(512) void dagger_act_kernel(const DaggerArgs g) {
  extern __shared__ float lds[];
  constexpr int NC = H / 16, KS = H / 4;
  using L = DLds<H>;
  const int tid = threadIdx.x, lane = tid & 63;
  const int wv = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int tw = wv >> 2, q = wv & 3;                  // tower 0: expert, tower 1: learner
  const int li = lane & 15, lk = lane >> 4;
  const int D = g.de.obs_dim, A = g.de.act_dim, discrete = g.de.discrete, n = g.n;
  const PolOff o = pol_offsets(D, A, H, discrete);
  const int i0 = blockIdx.x * ROWS;
  const int S1 = (D + 3) >> 2;
  const float* __restrict__ P = tw ? g.Pl : g.Pe;
  const float* __restrict__ Pt = tw ? g.Ptl : g.Pte;
  // Every load from (possibly host) memory up front: the block's ROWS x D observation elements, the sampling lanes'
  // noise and mask.
  constexpr int NOBS = (ROWS * MAXD + 511) / 512;
  float raw[NOBS];
  const int n_real = ROWS * D;
#pragma unroll
  for (int j = 0; j < NOBS; ++j) {
    const int e = min(tid + 512 * j, n_real - 1);
    const int r = e / D, k = e - r * D;
    raw[j] = g.obs[(long long)min(i0 + r, n - 1) * D + k];
  }
  const int srow = i0 + q * 16 + (lane & 15);          // row this lane finishes (lanes 0..15 of every wave)
  float r_noise[MAXA];
#pragma unroll
  for (int a2 = 0; a2 < MAXA; ++a2) r_noise[a2] = 0.f;
  int r_mask = 0;
  if (lane < 16) {
    r_mask = g.mask[min(srow, n - 1)];
    if (tw == 1 && g.noise != nullptr) {
      const long long nrow = (long long)min(srow, n - 1) * (discrete ? 1 : A);
#pragma unroll
      for (int a2 = 0; a2 < MAXA; ++a2) r_noise[a2] = g.noise[nrow + (discrete ? 0 : min(a2, A - 1))];
    }
  }
  for (int e = tid; e < 2 * ROWS * L::XS; e += 512) lds[L::x + e] = 0.f;   // padding columns / rows of both tiles
  __syncthreads();
#pragma unroll
  for (int j = 0; j < NOBS; ++j) {
    const int e = tid + 512 * j;
    if (e < n_real) {
      const int r = e / D, k = e - r * D;
      const bool live = (i0 + r) < n;
      const float ve = g.de.has_norm ? (raw[j] - g.nme[k]) / sqrtf(g.nve[k] + g.de.norm_eps) : raw[j];
      const float vl = g.dl.has_norm ? (raw[j] - g.nml[k]) / sqrtf(g.nvl[k] + g.dl.norm_eps) : raw[j];
      lds[L::x + r * L::XS + k] = live ? ve : 0.f;
      lds[L::x + ROWS * L::XS + r * L::XS + k] = live ? vl : 0.f;
      if (live && g.tab_obs != nullptr) g.tab_obs[(g.base_row + i0 + r) * D + k] = raw[j];
    }
  }
  // weight fragments straight from global memory: B[k = 4s+lk][j = c*16+li] (the act body's loads, per tower)
  float bW1[16][NC], bW2[KS][NC], bHead[KS], b1v[NC], b2v[NC];
#pragma unroll
  for (int gq = 0; gq < 4; ++gq) {
    if (4 * gq < S1) {
#pragma unroll
      for (int s = 4 * gq; s < 4 * gq + 4; ++s)
#pragma unroll
        for (int c = 0; c < NC; ++c) bW1[s][c] = Pt[o.pW1 + min(4 * s + lk, D - 1) * H + c * 16 + li];
    } else {
#pragma unroll
      for (int s = 4 * gq; s < 4 * gq + 4; ++s)
#pragma unroll
        for (int c = 0; c < NC; ++c) bW1[s][c] = 0.f;
    }
  }
  const int head_base = o.aW + min(li, A - 1) * H;
#pragma unroll
  for (int s = 0; s < KS; ++s) {
    const int kk = 4 * s + lk;
#pragma unroll
    for (int c = 0; c < NC; ++c) bW2[s][c] = Pt[o.pW2 + kk * H + c * 16 + li];
    bHead[s] = P[head_base + kk];
  }
#pragma unroll
  for (int c = 0; c < NC; ++c) {
    b1v[c] = P[o.pb1 + c * 16 + li];
    b2v[c] = P[o.pb2 + c * 16 + li];
  }
  const float head_bias = P[o.ab + min(li, A - 1)];
  __builtin_amdgcn_sched_barrier(0);
#pragma unroll
  for (int s = 0; s < 16; ++s)
#pragma unroll
    for (int c = 0; c < NC; ++c) bW1[s][c] = (4 * s + lk < D) ? bW1[s][c] : 0.f;
#pragma unroll
  for (int s = 0; s < KS; ++s) bHead[s] = li < A ? bHead[s] : 0.f;
  __syncthreads();

  const float* xt = lds + L::x + tw * ROWS * L::XS;
  float* a1t = lds + L::a1 + tw * ROWS * L::HS;
  float* a2t = lds + L::a2 + tw * ROWS * L::HS;
  float* outt = lds + L::out + tw * ROWS * L::AS;
  const int arow = q * 16 + li;
  {
    f32x4 acc[NC];
#pragma unroll
    for (int c = 0; c < NC; ++c) acc[c] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int s = 0; s < 16; ++s)
      if (s < S1) {
        const float a = xt[arow * L::XS + 4 * s + lk];
#pragma unroll
        for (int c = 0; c < NC; ++c) acc[c] = mfma16(a, bW1[s][c], acc[c]);
      }
#pragma unroll
    for (int c = 0; c < NC; ++c)
#pragma unroll
      for (int r = 0; r < 4; ++r) a1t[(q * 16 + lk * 4 + r) * L::HS + c * 16 + li] = fast_tanh(acc[c][r] + b1v[c]);
  }
  wave_sync_lds();
  {
    f32x4 acc[NC];
#pragma unroll
    for (int c = 0; c < NC; ++c) acc[c] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int s = 0; s < KS; ++s) {
      const float a = a1t[arow * L::HS + 4 * s + lk];
#pragma unroll
      for (int c = 0; c < NC; ++c) acc[c] = mfma16(a, bW2[s][c], acc[c]);
    }
#pragma unroll
    for (int c = 0; c < NC; ++c)
#pragma unroll
      for (int r = 0; r < 4; ++r) a2t[(q * 16 + lk * 4 + r) * L::HS + c * 16 + li] = fast_tanh(acc[c][r] + b2v[c]);
  }
  wave_sync_lds();
  {
    f32x4 acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int s = 0; s < KS; ++s) acc = mfma16(a2t[arow * L::HS + 4 * s + lk], bHead[s], acc);
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int rr = q * 16 + lk * 4 + r;
      if (li < A) outt[rr * L::AS + li] = acc[r] + head_bias;
    }
  }
  wave_sync_lds();
  const int row = i0 + q * 16 + lane;
  if (lane >= 16 || row >= n) return;
  const float* outrow = outt + (q * 16 + lane) * L::AS;
  const int aw = discrete ? 1 : A;
  // per-action constants of the finishing lanes (device memory: read here, behind the layer chain, they cost a cache
  // hit; held from the start as the act body holds them, the 64-wide instance spilled registers)
  float r_ls[MAXA], r_low[MAXA], r_high[MAXA];
#pragma unroll
  for (int a2 = 0; a2 < MAXA; ++a2) {
    const int ac = min(a2, A - 1);
    r_ls[a2] = discrete ? 0.f : P[o.log_std + ac];
    r_low[a2] = discrete ? 0.f : g.low[ac];
    r_high[a2] = discrete ? 0.f : g.high[ac];
  }
  if (tw == 0) {
    // the expert's mode: what the act kernel writes to `clipped` for zero noise (Box) / a negative uniform (Discrete).
    // It is the stored label everywhere and the executed action where the mask is clear.
    float lab[MAXA];
    if (!discrete) {
#pragma unroll
      for (int a = 0; a < MAXA; ++a)
        if (a < A) {
          const float act = __fadd_rn(outrow[a], __fmul_rn(0.f, expf(r_ls[a])));
          lab[a] = fminf(fmaxf(act, r_low[a]), r_high[a]);
        }
    } else {
      int pick = 0;
      for (int a = 1; a < A; ++a)
        if (outrow[a] > outrow[pick]) pick = a;
      lab[0] = (float)pick;
    }
    // (a host-sampled Discrete learner: the host overwrites the masked rows of `actual_act` after sampling)
    const bool mine = r_mask == 0 || g.logits != nullptr;
#pragma unroll
    for (int a = 0; a < MAXA; ++a)
      if (a < aw) {
        g.expert_act[(long long)row * aw + a] = lab[a];
        if (mine) g.actual_act[(long long)row * aw + a] = lab[a];
        if (g.tab_acts != nullptr) g.tab_acts[(g.base_row + row) * aw + a] = lab[a];
      }
    return;
  }
  if (g.logits != nullptr) {
    for (int a = 0; a < A; ++a) g.logits[(long long)row * A + a] = outrow[a];
    return;
  }
  if (r_mask == 0) return;
  if (!discrete) {
#pragma unroll
    for (int a = 0; a < MAXA; ++a)
      if (a < A) {
        const float act = __fadd_rn(outrow[a], __fmul_rn(r_noise[a], expf(r_ls[a])));  // Normal.rsample
        g.actual_act[(long long)row * A + a] = fminf(fmaxf(act, r_low[a]), r_high[a]);
      }
  } else {
    float mx = outrow[0];
    for (int a = 1; a < A; ++a) mx = fmaxf(mx, outrow[a]);
    float se = 0.f;
    for (int a = 0; a < A; ++a) se += expf(outrow[a] - mx);
    const float lse = mx + logf(se);
    const float u = r_noise[0];
    float c = 0.f;
    int pick = A - 1;
    if (u < 0.f) {
      pick = 0;
      for (int a = 1; a < A; ++a)
        if (outrow[a] > outrow[pick]) pick = a;
    } else {
      for (int a = 0; a < A; ++a) {
        c += expf(outrow[a] - lse);
        if (u < c) { pick = a; break; }
      }
    }
    g.actual_act[row] = (float)pick;
  }
}

template <int H>
int launch(const DaggerArgs& g, hipStream_t stream) {
  static bool attr = false;
  const size_t bytes = DLds<H>::total * sizeof(float);
  if (!attr) {
    hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(dagger_act_kernel<H>),
                                       hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes);
    if (e != hipSuccess) return (int)e;
    attr = true;
  }
  hipLaunchKernelGGL(dagger_act_kernel<H>, dim3((g.n + ROWS - 1) / ROWS), dim3(512), bytes, stream, g);
  IA_CHECK_LAUNCH();
  return IA_OK;
}

}  // namespace

extern "C" int ia_dagger_act(const ia_policy_desc* expert, const float* e_params, const float* e_params_t,
                             const float* e_norm_mean, const float* e_norm_var, const ia_policy_desc* learner,
                             const float* l_params, const float* l_params_t, const float* l_norm_mean,
                             const float* l_norm_var, const float* obs, int n, const uint8_t* mask, const float* noise,
                             const float* low, const float* high, float* expert_act, float* actual_act,
                             float* learner_logits, float* table_obs, float* table_acts, int64_t base_row,
                             int64_t table_cap, void* stream) {
  if (!expert || !learner || !e_params || !e_params_t || !l_params || !l_params_t || !obs || !mask || !expert_act ||
      !actual_act || n <= 0)
    return IA_ERR_ARG;
  if (expert->obs_dim < 1 || expert->obs_dim > MAXD || expert->act_dim < 1 || expert->act_dim > MAXA) return IA_ERR_ARG;
  if (expert->obs_dim != learner->obs_dim || expert->act_dim != learner->act_dim || expert->hidden != learner->hidden ||
      (expert->discrete != 0) != (learner->discrete != 0) || (expert->hidden != 32 && expert->hidden != 64))
    return IA_ERR_UNSUPPORTED;
  if ((expert->has_norm && (!e_norm_mean || !e_norm_var)) || (learner->has_norm && (!l_norm_mean || !l_norm_var)))
    return IA_ERR_ARG;
  if (!expert->discrete && (!low || !high)) return IA_ERR_ARG;
  if (!learner_logits && !noise) return IA_ERR_ARG;            // the learner samples: it needs its draws
  if ((table_obs == nullptr) != (table_acts == nullptr)) return IA_ERR_ARG;
  if (table_obs && (base_row < 0 || base_row + n > table_cap)) return IA_ERR_ARG;   // the append stays inside the table
  DaggerArgs g{*expert, *learner, e_params, e_params_t, e_norm_mean, e_norm_var, l_params, l_params_t, l_norm_mean,
               l_norm_var, obs, n, mask, noise, low, high, expert_act, actual_act, learner_logits, table_obs, table_acts,
               (long long)base_row};
  return expert->hidden == 32 ? launch<32>(g, (hipStream_t)stream) : launch<64>(g, (hipStream_t)stream);
}
