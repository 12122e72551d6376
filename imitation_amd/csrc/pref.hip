// Reward-model training on preference comparisons (algorithms/preference_comparisons.py):
//   * the preference loss of a minibatch of fragment pairs on per-row rewards (PreferenceModel.probability :491-531,
//     CrossEntropyRewardLoss.forward :1048-1091), forward and backward in one launch;
//   * RunningNorm applied once per fragment, in fragment order (util/networks.py:79-91 inside PreferenceModel.rewards
//     :457-489, one `self.model(...)` call per fragment): per-fragment slab moments for ia_running_norm_merge_seq, and the
//     normalisation of each fragment with the statistics after its own update;
//   * torch.optim.AdamW (decoupled weight decay), element-wise and fused into the split-K slab reduction.
#include "common.h"
#include "rn_common.h"
#include "../../include/imitation_hip.h"

namespace {

constexpr int PREF_THREADS = 512;   // one workgroup, 8 waves: the minibatch's pairs are few and short
constexpr int PREF_WAVES = PREF_THREADS / 64;

__device__ __forceinline__ float wave_sum(float v) {
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

// torch binary_cross_entropy (CPU), one element: (y - 1) * max(log1p(-p), -100) - y * max(log(p), -100)
__device__ __forceinline__ float bce_elem(float p, float y) {
  return (y - 1.f) * fmaxf(log1pf(-p), -100.f) - y * fmaxf(logf(p), -100.f);
}

struct PairProb {
  float p;       // probability that fragment 1 is preferred
  float e;       // exp(clipped returns difference)
  float mp;      // 1 / (1 + e)
  bool inside;   // the clip passes the gradient (torch.clamp: min <= x <= max)
};

// PreferenceModel.probability on the wave's reduced returns difference
__device__ __forceinline__ PairProb pair_probability(float diff, float noise, float threshold) {
  PairProb r;
  r.inside = (diff >= -threshold) && (diff <= threshold);
  const float c = fminf(fmaxf(diff, -threshold), threshold);
  r.e = expf(c);
  r.mp = 1.f / (1.f + r.e);
  r.p = (noise * 0.5f) + (1.f - noise) * r.mp;
  return r;
}

// One workgroup. Wave w takes pairs w, w + 8, ...: its lanes stride over the pair's steps, the wave reduces the
// (discounted) returns difference, lane 0 keeps the running sums of the wave in pair order; the per-row gradient of
// the pair is written right away (it depends on that pair alone and on the batch size). The eight waves' sums are
// combined in wave order: deterministic.
__global__ __launch_bounds__(PREF_THREADS) void pref_loss_kernel(
    const float* __restrict__ rew, const int* __restrict__ pair_off, int n_pairs, const float* __restrict__ prefs,
    const float* __restrict__ gt_rew, float gamma, float noise, float threshold, float loss_scale,
    float* __restrict__ d_rew, float* __restrict__ probs, float* __restrict__ gt_probs, float* __restrict__ stats) {
  __shared__ float red[PREF_WAVES][3];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const bool plain = (gamma == 1.f);
  float s_loss = 0.f, s_acc = 0.f, s_gt = 0.f;
  const float g_mean = loss_scale / (float)n_pairs;   // d(scale * mean(bce)) / d bce_i
  for (int p = wave; p < n_pairs; p += PREF_WAVES) {
    const int o = pair_off[p], L = pair_off[p + 1] - o;
    const float* r1 = rew + 2LL * o;
    const float* r2 = r1 + L;
    float d = 0.f, dg = 0.f;
    for (int t = lane; t < L; t += 64) {
      const float w = plain ? 1.f : powf(gamma, (float)t);
      d += w * (r2[t] - r1[t]);
      if (gt_rew != nullptr) dg += w * (gt_rew[2LL * o + L + t] - gt_rew[2LL * o + t]);
    }
    d = wave_sum(d);
    const float y = prefs[p];
    const PairProb pp = pair_probability(d, noise, threshold);
    const float loss_i = bce_elem(pp.p, y);
    const float acc_i = ((pp.p > 0.5f) == (y > 0.5f)) ? 1.f : 0.f;
    float gt_i = 0.f;
    if (gt_rew != nullptr) {
      dg = wave_sum(dg);
      const PairProb pg = pair_probability(dg, noise, threshold);
      gt_i = bce_elem(pg.p, y);
      if (lane == 0 && gt_probs != nullptr) gt_probs[p] = pg.p;
    }
    if (lane == 0) {
      s_loss += loss_i;
      s_acc += acc_i;
      s_gt += gt_i;
      if (probs != nullptr) probs[p] = pp.p;
    }
    if (d_rew != nullptr) {
      // autograd's chain in the reference's operation order: BCE backward, the noise mix, reciprocal, exp, clamp, sum
      const float g_p = g_mean * (pp.p - y) / fmaxf((1.f - pp.p) * pp.p, 1e-12f);
      const float g_mp = g_p * (1.f - noise);
      const float g_x = -g_mp * (pp.mp * pp.mp);
      const float g_d = pp.inside ? g_x * pp.e : 0.f;
      for (int t = lane; t < L; t += 64) {
        const float w = plain ? g_d : g_d * powf(gamma, (float)t);
        d_rew[2LL * o + t] = -w;
        d_rew[2LL * o + L + t] = w;
      }
    }
  }
  if (lane == 0) {
    red[wave][0] = s_loss;
    red[wave][1] = s_acc;
    red[wave][2] = s_gt;
  }
  __syncthreads();
  if (threadIdx.x == 0 && stats != nullptr) {
    float a = 0.f, b = 0.f, c = 0.f;
    for (int w = 0; w < PREF_WAVES; ++w) {
      a += red[w][0];
      b += red[w][1];
      c += red[w][2];
    }
    const float inv = (float)n_pairs;
    stats[0] = a / inv;
    stats[1] = b / inv;
    stats[2] = gt_rew != nullptr ? c / inv : 0.f;
  }
}

// Slab moments of every fragment in ia_running_norm_partial's layout: fragment f (rows f*L .. f*L+L-1 of X) ->
// ws + f*ws_stride, slab b of RN_ROWS_PER_BLOCK rows -> (mean[D], M2[D]) at (2b, 2b+1) * D. One thread per column.
__global__ __launch_bounds__(256) void pref_frag_moments_kernel(const float* __restrict__ X, int ldx, int L, int D,
                                                                long long ws_stride, float* __restrict__ ws) {
  const int f = blockIdx.y, b = blockIdx.x;
  const int r0 = b * RN_ROWS_PER_BLOCK, rows = min(RN_ROWS_PER_BLOCK, L - r0);
  const float* x = X + ((long long)f * L + r0) * ldx;
  float* w = ws + f * ws_stride + (long long)b * 2 * D;
  for (int c = threadIdx.x; c < D; c += blockDim.x) {
    float s = 0.f;
    for (int r = 0; r < rows; ++r) s += x[(long long)r * ldx + c];
    const float mean = s / (float)rows;
    float q = 0.f;
    for (int r = 0; r < rows; ++r) {
      const float dl = x[(long long)r * ldx + c] - mean;
      q += dl * dl;
    }
    w[c] = mean;
    w[D + c] = q;
  }
}

// rn_apply's arithmetic with fragment f's own statistics snapshot (snap [n][2][D]); columns [D, ldy) zeroed
__global__ void pref_norm_apply_seq_kernel(const float* __restrict__ X, int ldx, int n_frags, int L, int D,
                                           const float* __restrict__ snap, float eps, float* __restrict__ Y, int ldy) {
  const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= (long long)n_frags * L * ldy) return;
  const int c = (int)(i % ldy);
  const long long r = i / ldy;
  const float* s = snap + (r / L) * 2LL * D;
  Y[i] = (c < D) ? (X[r * ldx + c] - s[c]) / sqrtf(s[D + c] + eps) : 0.f;
}

// torch/optim/adam.py _single_tensor_adam with decoupled_weight_decay (AdamW): p *= 1 - lr * wd, then the Adam step
__device__ __forceinline__ void adamw_element(float* __restrict__ p, float grad, float* __restrict__ m,
                                              float* __restrict__ v, long long i, float beta1, float beta2, float eps,
                                              float decay, float step_size, float bc2_sqrt) {
  const float pi = p[i] * decay;
  float mi = m[i];
  mi = mi + (grad - mi) * (1.f - beta1);
  const float vi = v[i] * beta2 + (1.f - beta2) * grad * grad;
  const float denom = sqrtf(vi) / bc2_sqrt + eps;
  p[i] = pi - step_size * (mi / denom);
  m[i] = mi;
  v[i] = vi;
}

__global__ void adamw_kernel(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ m,
                             float* __restrict__ v, long long n, float beta1, float beta2, float eps, float decay,
                             float step_size, float bc2_sqrt) {
  const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  adamw_element(p, g[i], m, v, i, beta1, beta2, eps, decay, step_size, bc2_sqrt);
}

__global__ void reduce_adamw_kernel(const float* __restrict__ partials, int splits, long long n, float scale,
                                    float* __restrict__ grads, float* __restrict__ p, float* __restrict__ m,
                                    float* __restrict__ v, float beta1, float beta2, float eps, float decay,
                                    float step_size, float bc2_sqrt) {
  const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  float s = 0.f;
  for (int k = 0; k < splits; ++k) s += partials[(long long)k * n + i];   // ia_reduce_partials' slab order
  const float grad = s * scale;
  grads[i] = grad;
  adamw_element(p, grad, m, v, i, beta1, beta2, eps, decay, step_size, bc2_sqrt);
}

inline long long cdivl(long long a, long long b) { return (a + b - 1) / b; }

// ---- frame gather: uint8 frame table -> fp32 channel-last CNN input -------------------------------------------------
// One workgroup per tile = (row r, pixels [p0, p0 + tp)). The tile's source bytes are `n_spans` contiguous runs ("spans"):
// table [F, H, W, C]: one per source frame, tp * C bytes; table [F, C, H, W]: one per (source frame, channel), tp bytes.
// Phase 1 copies the spans into LDS, each at the LDS offset congruent to its global address mod 16, so every 16-byte slot
// that lies wholly inside a span moves with one aligned 16-byte load and one 16-byte LDS store; the slots a span only
// partly covers (its unaligned head and tail) move byte by byte. No byte outside a span is read. Phase 2: a lane forms
// four consecutive floats of X from LDS bytes (for the [F, C, H, W] table this is the transpose: a pixel's channels are
// `span_stride` apart in LDS) and stores them as one aligned 16-byte vector; the floats of a tile before the first / after
// the last 16-byte boundary are stored one by one.
constexpr int GF_THREADS = 256;
constexpr int GF_LDS = 16384;         // staged bytes of one tile, the spans' padding included
constexpr int GF_MAX_SPANS = 256;
constexpr int GF_TILE_ELEMS = 8192;   // output floats of one tile, at most

struct GatherFrames {
  const uint8_t* frames;
  long long n_frames;
  const long long* idx;
  const float* lut;     // nullable: 256 floats, the value of every byte
  float* X;
  int HW, C, S, base;   // pixels per frame, channels per frame, source frames per row (1 or 2), first source = idx + base
  int chw;              // table layout [F, C, H, W]
  int TP, tiles_per_row, n_spans, span_stride;
};

__global__ __launch_bounds__(GF_THREADS) void pref_gather_frames_kernel(const GatherFrames g) {
  __shared__ __attribute__((aligned(16))) unsigned char stage[GF_LDS];
  __shared__ int span_off[GF_MAX_SPANS];
  __shared__ float lut[256];
  const int tid = threadIdx.x;
  const int r = blockIdx.x / g.tiles_per_row, tile = blockIdx.x - r * g.tiles_per_row;
  const int p0 = tile * g.TP, tp = min(g.TP, g.HW - p0);
  const int Cin = g.C * g.S;
  const long long N = (long long)g.HW * g.C;
  const long long f0 = g.idx[r] + g.base;
  float* xt = g.X + ((long long)r * g.HW + p0) * Cin;   // the tile's first float
  const int n_out = tp * Cin;
  if (f0 < 0 || f0 + g.S > g.n_frames) {   // a row outside the table reads nothing and is loud downstream
    for (int e = tid; e < n_out; e += GF_THREADS) xt[e] = __builtin_nanf("");
    return;
  }
  const int span_len = g.chw ? tp : tp * g.C;
  auto span_src = [&](int j) -> const uint8_t* {
    if (g.chw) {
      const int s = j / g.C, c = j - s * g.C;
      return g.frames + (f0 + s) * N + (long long)c * g.HW + p0;
    }
    return g.frames + (f0 + j) * N + (long long)p0 * g.C;
  };
  if (g.lut != nullptr) lut[tid] = g.lut[tid];
  for (int j = tid; j < g.n_spans; j += GF_THREADS)
    span_off[j] = j * g.span_stride + (int)((uintptr_t)span_src(j) & 15);
  const int slots = g.span_stride >> 4;
  for (int it = tid; it < g.n_spans * slots; it += GF_THREADS) {
    const int j = it / slots, v = it - j * slots;
    const uintptr_t lo = (uintptr_t)span_src(j), hi = lo + (uintptr_t)span_len;
    const uintptr_t a = (lo & ~(uintptr_t)15) + 16u * (uintptr_t)v;   // the slot's global address (16-byte aligned)
    unsigned char* dst = stage + j * g.span_stride + 16 * v;
    if (a >= lo && a + 16 <= hi) {
      *reinterpret_cast<uint4*>(dst) = *reinterpret_cast<const uint4*>(a);
    } else if (a + 16 > lo && a < hi) {
      for (int b = 0; b < 16; ++b)
        if (a + b >= lo && a + b < hi) dst[b] = *reinterpret_cast<const uint8_t*>(a + b);
    }
  }
  __syncthreads();
  auto value = [&](int p, int ci) -> float {
    const int s = ci >= g.C ? 1 : 0;
    const int at = g.chw ? span_off[ci] + p : span_off[s] + p * g.C + (ci - s * g.C);
    const unsigned b = stage[at];
    return g.lut != nullptr ? lut[b] : (float)b / 255.0f;
  };
  const int mis = (int)(((uintptr_t)xt >> 2) & 3);   // floats between the last 16-byte boundary and the tile's first
  const int nq = (mis + n_out + 3) >> 2;
  const bool quads = (Cin & 3) == 0 && mis == 0;     // every vector lies inside one pixel
  for (int q = tid; q < nq; q += GF_THREADS) {
    const int e0 = 4 * q - mis;
    if (quads) {
      const int p = e0 / Cin, ci = e0 - p * Cin;
      const f32x4 o = {value(p, ci), value(p, ci + 1), value(p, ci + 2), value(p, ci + 3)};
      *reinterpret_cast<f32x4*>(xt + e0) = o;
    } else if (e0 >= 0 && e0 + 4 <= n_out) {
      f32x4 o;
      for (int k = 0; k < 4; ++k) {
        const int p = (e0 + k) / Cin;
        o[k] = value(p, e0 + k - p * Cin);
      }
      *reinterpret_cast<f32x4*>(xt + e0) = o;
    } else {
      for (int k = 0; k < 4; ++k) {
        const int e = e0 + k;
        if (e < 0 || e >= n_out) continue;
        const int p = e / Cin;
        xt[e] = value(p, e - p * Cin);
      }
    }
  }
}

int launch_gather_frames(const uint8_t* frames, long long n_frames, const int64_t* frame_idx, int n_rows, int H, int W,
                         int C, int table_chw, int use_state, int use_next, const float* lut, float* X, void* stream) {
  const int S = (use_state != 0) + (use_next != 0);
  if (frames == nullptr || frame_idx == nullptr || X == nullptr) return IA_ERR_ARG;
  if (S == 0 || n_rows <= 0 || H <= 0 || W <= 0 || C <= 0 || n_frames <= 0) return IA_ERR_ARG;
  const long long HW = (long long)H * W;
  if (HW * C * S > (1LL << 30)) return IA_ERR_UNSUPPORTED;   // a row's float count stays a 32-bit index
  GatherFrames g;
  g.frames = frames;
  g.n_frames = n_frames;
  g.idx = reinterpret_cast<const long long*>(frame_idx);
  g.lut = lut;
  g.X = X;
  g.HW = (int)HW;
  g.C = C;
  g.S = S;
  g.base = use_state ? 0 : 1;
  g.chw = table_chw != 0;
  g.n_spans = g.chw ? S * C : S;
  if (g.n_spans > GF_MAX_SPANS) return IA_ERR_UNSUPPORTED;
  const int unit = g.chw ? 1 : C;                              // bytes of a pixel inside one span
  const int max_len = ((GF_LDS / g.n_spans) & ~15) - 16;       // a span's bytes; 16 more hold its misalignment
  if (max_len < unit) return IA_ERR_UNSUPPORTED;
  long long TP = max_len / unit;
  TP = TP < GF_TILE_ELEMS / (C * S) ? TP : GF_TILE_ELEMS / (C * S);
  TP = TP < 1 ? 1 : (TP > HW ? HW : TP);
  g.TP = (int)TP;
  g.span_stride = (g.TP * unit + 15) / 16 * 16 + 16;
  g.tiles_per_row = (int)cdivl(HW, TP);
  const long long grid = (long long)n_rows * g.tiles_per_row;
  if (grid > 0x7fffffffLL) return IA_ERR_UNSUPPORTED;
  hipLaunchKernelGGL(pref_gather_frames_kernel, dim3((unsigned)grid), dim3(GF_THREADS), 0, (hipStream_t)stream, g);
  IA_CHECK_LAUNCH();
  return IA_OK;
}

}  // namespace

extern "C" {

int ia_pref_loss(const float* rewards, const int* pair_off, int n_pairs, const float* prefs, const float* gt_rewards,
                 float discount_factor, float noise_prob, float threshold, float loss_scale, float* d_rewards,
                 float* probs, float* gt_probs, float* stats, void* stream) {
  if (n_pairs <= 0 || rewards == nullptr || pair_off == nullptr || prefs == nullptr) return IA_ERR_ARG;
  if (!(threshold >= 0.f)) return IA_ERR_ARG;
  hipLaunchKernelGGL(pref_loss_kernel, dim3(1), dim3(PREF_THREADS), 0, (hipStream_t)stream, rewards, pair_off, n_pairs,
                     prefs, gt_rewards, discount_factor, noise_prob, threshold, loss_scale, d_rewards, probs, gt_probs,
                     stats);
  IA_CHECK_LAUNCH();
  return IA_OK;
}

int ia_pref_frag_moments(const float* X, int ldx, int n_frags, int L, int D, int64_t ws_stride, float* ws,
                         void* stream) {
  if (n_frags <= 0 || L <= 0 || D <= 0 || ldx < D) return IA_ERR_ARG;
  if (ws_stride < (int64_t)cdivl(L, RN_ROWS_PER_BLOCK) * 2 * D) return IA_ERR_ARG;
  hipLaunchKernelGGL(pref_frag_moments_kernel, dim3((unsigned)cdivl(L, RN_ROWS_PER_BLOCK), n_frags), dim3(256), 0,
                     (hipStream_t)stream, X, ldx, L, D, (long long)ws_stride, ws);
  IA_CHECK_LAUNCH();
  return IA_OK;
}

int ia_pref_norm_apply_seq(const float* X, int ldx, int n_frags, int L, int D, const float* snapshots, float eps,
                           float* Y, int ldy, void* stream) {
  if (n_frags <= 0 || L <= 0 || D <= 0 || ldx < D || ldy < D) return IA_ERR_ARG;
  const long long n = (long long)n_frags * L * ldy;
  hipLaunchKernelGGL(pref_norm_apply_seq_kernel, dim3((unsigned)cdivl(n, 256)), dim3(256), 0, (hipStream_t)stream, X,
                     ldx, n_frags, L, D, snapshots, eps, Y, ldy);
  IA_CHECK_LAUNCH();
  return IA_OK;
}

int ia_pref_gather_frames(const uint8_t* frames, const int64_t* frame_idx, int n_rows, int H, int W, int C, int table_chw,
                          int use_state, int use_next, float* X, void* stream) {
  return launch_gather_frames(frames, INT64_MAX, frame_idx, n_rows, H, W, C, table_chw, use_state, use_next, nullptr, X,
                              stream);
}

int ia_pref_gather_frames_lut(const uint8_t* frames, int64_t n_frames, const int64_t* frame_idx, int n_rows, int H, int W,
                              int C, int table_chw, int use_state, int use_next, const float* lut, float* X,
                              void* stream) {
  return launch_gather_frames(frames, n_frames, frame_idx, n_rows, H, W, C, table_chw, use_state, use_next, lut, X,
                              stream);
}

int ia_adamw_step(float* params, const float* grads, float* exp_avg, float* exp_avg_sq, int64_t n, float beta1,
                  float beta2, float eps, float decay, float step_size, float bc2_sqrt, void* stream) {
  if (n <= 0) return IA_ERR_ARG;
  hipLaunchKernelGGL(adamw_kernel, dim3((unsigned)cdivl(n, 256)), dim3(256), 0, (hipStream_t)stream, params, grads,
                     exp_avg, exp_avg_sq, (long long)n, beta1, beta2, eps, decay, step_size, bc2_sqrt);
  IA_CHECK_LAUNCH();
  return IA_OK;
}

int ia_reduce_partials_adamw(const float* partials, int splits, int64_t n, float scale, float* grads, float* params,
                             float* exp_avg, float* exp_avg_sq, float beta1, float beta2, float eps, float decay,
                             float step_size, float bc2_sqrt, void* stream) {
  if (n <= 0 || splits <= 0) return IA_ERR_ARG;
  hipLaunchKernelGGL(reduce_adamw_kernel, dim3((unsigned)cdivl(n, 256)), dim3(256), 0, (hipStream_t)stream, partials,
                     splits, (long long)n, scale, grads, params, exp_avg, exp_avg_sq, beta1, beta2, eps, decay,
                     step_size, bc2_sqrt);
  IA_CHECK_LAUNCH();
  return IA_OK;
}

}  // extern "C"
