// SAC kernels ([SB3 sac/sac.py] SAC.train, [SB3 common/distributions.py] SquashedDiagGaussianDistribution): what one
// gradient step needs around the fp32 MFMA stacks beyond csrc/td3.hip (ia_mlp_forward / ia_mlp_backward run the actor, the
// critics and the critic targets; ia_td3_assemble builds the minibatch), each piece ONE launch:
//   * ia_sac_sample: from the actor's head output [mu | log_std] and eps: log_std clamped to [-20, 2], u = mu + exp(log_std) eps,
//     a = tanh(u) into the action columns of a critic input tile (with the observation columns when asked), logp per row, and
//     what the backward needs: a, 1 - a^2, the clamped log_std and which elements the clamp bound. eps == NULL: a = tanh(mu);
//   * ia_sac_alpha_step: alpha = exp(log_ent_coef) as it stands into a device slot and the stats block, ent_coef_loss =
//     -mean(log_ent_coef (logp + target_entropy)), then Adam on the scalar; one workgroup;
//   * ia_sac_critic_loss: y = rew + (1 - done) gamma (min_i Qt_i - alpha logp'), loss = 0.5 sum_i mean((Q_i - y)^2),
//     dQ_i = (Q_i - y) / B, for 1 or 2 critics; alpha from the device slot; which critic attains the minimum per row;
//   * ia_sac_min_seed: the backward seeds of min_i Q_i(s, a_pi): 1 to the critic that attains the row's minimum (ties to the
//     first, as torch.min(dim) does), 0 to the other; the minimum and the int8 argmin record;
//   * ia_sac_actor_seed: actor_loss = mean(alpha logp - min Q) and the gradient of the head output [B, 2A] from the critics'
//     input gradients, through the squash and the reparametrisation.
// 1 - a^2 is formed as 4 t / (1 + t)^2, t = exp(-2 |u|), once |u| >= 1: float32 tanh(u) is 1.0 from |u| = 9.01 on and
// 1 - a * a loses its leading digits long before; below 1 the product form is exact enough and avoids 1 - t near t = 1.
// Loss sums run in float64 in a fixed order (a launch repeats bit for bit); no float atomics; vector stores only.
#include "common.h"
#include "../../include/imitation_hip.h"

namespace {

constexpr int SAC_THREADS = 256;
constexpr float SAC_LOG_STD_MIN = -20.f, SAC_LOG_STD_MAX = 2.f, SAC_EPS = 1e-6f;

// (td3_block_sum's order: lanes by butterfly, then the four wave sums in wave order)
__device__ __forceinline__ double sac_block_sum(double v, double* sm) {
  for (int s = 32; s > 0; s >>= 1) v += __shfl_xor(v, s, 64);
  if ((threadIdx.x & 63) == 0) sm[threadIdx.x >> 6] = v;
  __syncthreads();
  double t = 0.0;
  for (int w = 0; w < SAC_THREADS / 64; ++w) t += sm[w];
  __syncthreads();
  return t;
}

// one thread per row: the row's A elements in order (the log-probability is a sum over them)
__global__ __launch_bounds__(SAC_THREADS) void sac_sample_kernel(const float* __restrict__ head, const float* __restrict__ eps,
                                                                 const float* __restrict__ S, int n, int D, int A, int ld,
                                                                 float* __restrict__ X, float* __restrict__ logp,
                                                                 float* __restrict__ a_out, float* __restrict__ ls_out,
                                                                 float* __restrict__ om_out, int8_t* __restrict__ bound) {
  const long long r = (long long)blockIdx.x * SAC_THREADS + threadIdx.x;
  if (r >= n) return;
  if (S) {
    for (int c = 0; c < D; ++c) X[r * ld + c] = S[r * D + c];
    for (int c = D + A; c < ld; ++c) X[r * ld + c] = 0.f;
  }
  double lp = 0.0;
  for (int j = 0; j < A; ++j) {
    const float mu = head[r * 2 * A + j];
    const float raw = head[r * 2 * A + A + j];
    const float ls = fminf(fmaxf(raw, SAC_LOG_STD_MIN), SAC_LOG_STD_MAX);
    const float e = eps ? eps[r * A + j] : 0.f;
    const float u = eps ? mu + expf(ls) * e : mu;
    const float a = tanhf(u);
    float om = 1.f - a * a;
    if (fabsf(u) >= 1.f) {
      const float t = expf(-2.f * fabsf(u));
      om = (4.f * t) / ((1.f + t) * (1.f + t));
    }
    X[r * ld + D + j] = a;
    const long long o = r * A + j;
    if (a_out) a_out[o] = a;
    if (ls_out) ls_out[o] = ls;
    if (om_out) om_out[o] = om;
    if (bound) bound[o] = raw < SAC_LOG_STD_MIN ? (int8_t)-1 : (raw > SAC_LOG_STD_MAX ? (int8_t)1 : (int8_t)0);
    // Normal(mu, std).log_prob(u) with (u - mu) / std = eps, minus the squash correction
    lp += (-0.5 * (double)e * (double)e - (double)ls - 0.918938533204672742) - (double)logf(om + SAC_EPS);
  }
  if (logp) logp[r] = (float)lp;
}

struct SacAdam {
  float omb1, beta2, omb2, eps;
};

__global__ __launch_bounds__(SAC_THREADS) void sac_alpha_step_kernel(const float* __restrict__ logp, int B, float target_entropy,
                                                                     float* __restrict__ log_ent_coef, float* __restrict__ m,
                                                                     float* __restrict__ v, SacAdam ad, float step_size,
                                                                     float bc2_sqrt, float* __restrict__ alpha_slot,
                                                                     float* __restrict__ stats) {
  __shared__ double sm[SAC_THREADS / 64];
  double s = 0.0;
  for (int b = threadIdx.x; b < B; b += SAC_THREADS) s += (double)(logp[b] + target_entropy);
  const double mean = sac_block_sum(s, sm) / (double)B;
  if (threadIdx.x == 0) {
    const float lec = log_ent_coef[0];
    alpha_slot[0] = expf(lec);
    stats[0] = expf(lec);
    stats[1] = (float)(-(double)lec * mean);
    const float grad = (float)(-mean);
    const float mi = m[0] + (grad - m[0]) * ad.omb1;
    const float vi = v[0] * ad.beta2 + ad.omb2 * grad * grad;
    m[0] = mi;
    v[0] = vi;
    log_ent_coef[0] = lec - step_size * (mi / (sqrtf(vi) / bc2_sqrt + ad.eps));
  }
}

template <int NC>
__global__ __launch_bounds__(SAC_THREADS) void sac_critic_loss_kernel(const float* __restrict__ Q, const float* __restrict__ Qt,
                                                                      const float* __restrict__ logp_next,
                                                                      const float* __restrict__ rew,
                                                                      const float* __restrict__ done,
                                                                      const float* __restrict__ alpha_slot, int B, float gamma,
                                                                      float* __restrict__ dQ, float* __restrict__ y_out,
                                                                      int8_t* __restrict__ argmin, float* __restrict__ loss) {
  __shared__ double sm[SAC_THREADS / 64];
  const float inv_b = 1.f / (float)B;
  const float alpha = alpha_slot[0];
  double s[NC];
#pragma unroll
  for (int i = 0; i < NC; ++i) s[i] = 0.0;
  for (int b = threadIdx.x; b < B; b += SAC_THREADS) {
    float qmin = Qt[b];
    int8_t am = 0;
#pragma unroll
    for (int i = 1; i < NC; ++i) {
      const float qi = Qt[(long long)i * B + b];
      if (qi < qmin) { qmin = qi; am = (int8_t)i; }
    }
    const float next = qmin - alpha * logp_next[b];
    const float y = rew[b] + ((1.f - done[b]) * gamma) * next;
    if (y_out) y_out[b] = y;
    if (argmin) argmin[b] = am;
#pragma unroll
    for (int i = 0; i < NC; ++i) {
      const float d = Q[(long long)i * B + b] - y;
      s[i] += (double)d * (double)d;
      dQ[(long long)i * B + b] = d * inv_b;
    }
  }
  double tot = 0.0;
#pragma unroll
  for (int i = 0; i < NC; ++i) tot += sac_block_sum(s[i], sm) / (double)B;   // sum_i mean_i, critic order
  if (threadIdx.x == 0) loss[0] = (float)(0.5 * tot);
}

__global__ __launch_bounds__(SAC_THREADS) void sac_min_seed_kernel(const float* __restrict__ q, int B, int nc,
                                                                   float* __restrict__ seeds, float* __restrict__ minq,
                                                                   int8_t* __restrict__ argmin) {
  const long long b = (long long)blockIdx.x * SAC_THREADS + threadIdx.x;
  if (b >= B) return;
  float qmin = q[b];
  int8_t am = 0;
  if (nc == 2) {
    const float q1 = q[(long long)B + b];
    if (q1 < qmin) { qmin = q1; am = 1; }
    seeds[(long long)B + b] = am == 1 ? 1.f : 0.f;
  }
  seeds[b] = am == 0 ? 1.f : 0.f;
  minq[b] = qmin;
  argmin[b] = am;
}

// one workgroup: the loss (fixed order) and the B * A elements of the head gradient
__global__ __launch_bounds__(SAC_THREADS) void sac_actor_seed_kernel(const float* __restrict__ dX0, const float* __restrict__ dX1,
                                                                     int ld, int D, const float* __restrict__ a_in,
                                                                     const float* __restrict__ om_in,
                                                                     const float* __restrict__ eps,
                                                                     const float* __restrict__ log_std,
                                                                     const int8_t* __restrict__ bound,
                                                                     const float* __restrict__ alpha_slot,
                                                                     const float* __restrict__ logp,
                                                                     const float* __restrict__ minq, int B, int A,
                                                                     float* __restrict__ dhead, float* __restrict__ loss) {
  __shared__ double sm[SAC_THREADS / 64];
  const float inv_b = 1.f / (float)B;
  const float alpha = alpha_slot[0];
  const float alpha_b = alpha * inv_b;
  double s = 0.0;
  for (int b = threadIdx.x; b < B; b += SAC_THREADS) s += (double)(alpha * logp[b] - minq[b]);
  const double tot = sac_block_sum(s, sm);
  if (threadIdx.x == 0) loss[0] = (float)(tot / (double)B);
  for (long long e = threadIdx.x; e < (long long)B * A; e += SAC_THREADS) {
    const int r = (int)(e / A), j = (int)(e % A);
    float dx = dX0[(long long)r * ld + D + j];
    if (dX1) dx += dX1[(long long)r * ld + D + j];
    const float a = a_in[e], om = om_in[e];
    const float du = om * (dx * -inv_b) + alpha_b * ((2.f * a * om) / (om + SAC_EPS));
    dhead[(long long)r * 2 * A + j] = du;
    dhead[(long long)r * 2 * A + A + j] = bound[e] == 0 ? (du * expf(log_std[e])) * eps[e] - alpha_b : 0.f;
  }
}

inline unsigned sac_blocks(long long n) { return (unsigned)((n + SAC_THREADS - 1) / SAC_THREADS); }

}  // namespace

extern "C" {

int ia_sac_sample(const float* head, const float* eps, const float* S, int n, int D, int A, int ld, float* X, float* logp,
                  float* a, float* log_std, float* one_minus_a2, int8_t* bound, void* stream) {
  if (n < 1 || D < 0 || A < 1 || ld < D + A || !head || !X) return IA_ERR_ARG;
  hipLaunchKernelGGL(sac_sample_kernel, dim3(sac_blocks(n)), dim3(SAC_THREADS), 0, (hipStream_t)stream, head, eps, S, n, D, A,
                     ld, X, logp, a, log_std, one_minus_a2, bound);
  IA_CHECK_LAUNCH();
  return IA_OK;
}

int ia_sac_alpha_step(const float* logp, int B, float target_entropy, float* log_ent_coef, float* exp_avg, float* exp_avg_sq,
                      double beta1, double beta2, float eps, float step_size, float bc2_sqrt, float* alpha_slot, float* stats,
                      void* stream) {
  if (B < 1 || !logp || !log_ent_coef || !exp_avg || !exp_avg_sq || !alpha_slot || !stats) return IA_ERR_ARG;
  SacAdam ad;
  ad.omb1 = (float)(1.0 - beta1); ad.beta2 = (float)beta2; ad.omb2 = (float)(1.0 - beta2); ad.eps = eps;
  hipLaunchKernelGGL(sac_alpha_step_kernel, dim3(1), dim3(SAC_THREADS), 0, (hipStream_t)stream, logp, B, target_entropy,
                     log_ent_coef, exp_avg, exp_avg_sq, ad, step_size, bc2_sqrt, alpha_slot, stats);
  IA_CHECK_LAUNCH();
  return IA_OK;
}

int ia_sac_critic_loss(const float* q, const float* q_target, const float* logp_next, const float* rewards, const float* dones,
                       const float* alpha_slot, int B, int n_critics, float gamma, float* dq, float* y, int8_t* argmin,
                       float* loss, void* stream) {
  if (B < 1 || !q || !q_target || !logp_next || !rewards || !dones || !alpha_slot || !dq || !loss) return IA_ERR_ARG;
  if (n_critics == 1)
    hipLaunchKernelGGL(sac_critic_loss_kernel<1>, dim3(1), dim3(SAC_THREADS), 0, (hipStream_t)stream, q, q_target, logp_next,
                       rewards, dones, alpha_slot, B, gamma, dq, y, argmin, loss);
  else if (n_critics == 2)
    hipLaunchKernelGGL(sac_critic_loss_kernel<2>, dim3(1), dim3(SAC_THREADS), 0, (hipStream_t)stream, q, q_target, logp_next,
                       rewards, dones, alpha_slot, B, gamma, dq, y, argmin, loss);
  else
    return IA_ERR_UNSUPPORTED;
  IA_CHECK_LAUNCH();
  return IA_OK;
}

int ia_sac_min_seed(const float* q, int B, int n_critics, float* seeds, float* min_q, int8_t* argmin, void* stream) {
  if (B < 1 || !q || !seeds || !min_q || !argmin) return IA_ERR_ARG;
  if (n_critics != 1 && n_critics != 2) return IA_ERR_UNSUPPORTED;
  hipLaunchKernelGGL(sac_min_seed_kernel, dim3(sac_blocks(B)), dim3(SAC_THREADS), 0, (hipStream_t)stream, q, B, n_critics, seeds,
                     min_q, argmin);
  IA_CHECK_LAUNCH();
  return IA_OK;
}

int ia_sac_actor_seed(const float* dX0, const float* dX1, int ld, int D, const float* a, const float* one_minus_a2,
                      const float* eps, const float* log_std, const int8_t* bound, const float* alpha_slot, const float* logp,
                      const float* min_q, int B, int A, float* dhead, float* loss, void* stream) {
  if (B < 1 || D < 0 || A < 1 || ld < D + A || !dX0 || !a || !one_minus_a2 || !eps || !log_std || !bound || !alpha_slot ||
      !logp || !min_q || !dhead || !loss)
    return IA_ERR_ARG;
  hipLaunchKernelGGL(sac_actor_seed_kernel, dim3(1), dim3(SAC_THREADS), 0, (hipStream_t)stream, dX0, dX1, ld, D, a, one_minus_a2,
                     eps, log_std, bound, alpha_slot, logp, min_q, B, A, dhead, loss);
  IA_CHECK_LAUNCH();
  return IA_OK;
}

}  // extern "C"
