// TD3 / DDPG kernels ([SB3 td3/td3.py] TD3.train): what one gradient step needs around the fp32 MFMA stacks
// (ia_mlp_forward / ia_mlp_backward run the actor, the critics and their targets), each piece ONE launch:
//   * ia_td3_assemble: the minibatch of a step, from the learner ring and the expert table by ONE index row: the critics'
//     input X = [obs | action], the actor's input S, the next observations S2, rewards and dones (rows < n_new from the
//     ring, the rest from the expert table; a row index outside its table leaves NaN, never a read out of bounds);
//   * ia_td3_target_input: X2 = [next_obs | clamp(mu_target + clamp(noise, +-clip), -1, 1)], the target critics' input;
//   * ia_td3_critic_loss: y = rew + (1 - done) gamma min_i Qt_i, loss = sum_i mean((Q_i - y)^2), dQ_i = 2 (Q_i - y) / B,
//     for 1 or 2 critics, one workgroup, sums in a fixed order (a launch repeats bit for bit);
//   * ia_td3_actor_input: the actor's output into the action columns of X (the first critic's input of the actor loss);
//   * ia_td3_actor_seed: actor_loss = -mean(Q_1) and the seed of the actor's backward from the critic's dX:
//     dmu = dX[:, D:D+A] * (-1/B) * (1 - mu^2) -- ia_mlp_backward does not apply the OUTPUT activation's derivative.
// The twin critics share one input tile: two parameter blocks (two descriptors) over the same X.
#include "common.h"
#include "../../include/imitation_hip.h"

namespace {

constexpr int TD3_THREADS = 256;

// sum over the workgroup in a fixed order: lanes by butterfly, then the four wave sums in wave order. The loss sums run in
// float64 (a mean of signed Q-values cancels: in float32 the last places of the LARGEST term land in the result), so a
// loss leaves its kernel as the rounded float32 of its float64 sum, as in dqn.hip; these are a few hundred adds per launch.
__device__ __forceinline__ double td3_block_sum(double v, double* sm) {
  for (int s = 32; s > 0; s >>= 1) v += __shfl_xor(v, s, 64);
  if ((threadIdx.x & 63) == 0) sm[threadIdx.x >> 6] = v;
  __syncthreads();
  double t = 0.0;
  for (int w = 0; w < TD3_THREADS / 64; ++w) t += sm[w];
  __syncthreads();
  return t;
}

struct Td3Table {
  const float* obs;
  const float* next_obs;
  const float* act;
  const float* rew;
  const float* done;
  long long rows;
};

// one thread per (row, column) of the widened row [obs D | action A | pad ld-D-A | next_obs D | rew | done]
__global__ __launch_bounds__(TD3_THREADS) void td3_assemble_kernel(Td3Table ring, Td3Table expert,
                                                                   const int64_t* __restrict__ idx, int B, int n_new, int D,
                                                                   int A, int ld, float* __restrict__ X, float* __restrict__ S,
                                                                   float* __restrict__ S2, float* __restrict__ rew,
                                                                   float* __restrict__ done) {
  const int W = ld + D + 2;
  const long long e = (long long)blockIdx.x * TD3_THREADS + threadIdx.x;
  if (e >= (long long)B * W) return;
  const int r = (int)(e / W), c = (int)(e % W);
  const Td3Table& t = r < n_new ? ring : expert;
  const long long row = idx[r];
  const bool ok = row >= 0 && row < t.rows;
  const float bad = __builtin_nanf("");
  if (c < D) {
    const float v = ok ? t.obs[row * D + c] : bad;
    X[(long long)r * ld + c] = v;
    S[(long long)r * D + c] = v;
  } else if (c < D + A) {
    X[(long long)r * ld + c] = ok ? t.act[row * A + (c - D)] : bad;
  } else if (c < ld) {
    X[(long long)r * ld + c] = 0.f;
  } else if (c < ld + D) {
    S2[(long long)r * D + (c - ld)] = ok ? t.next_obs[row * D + (c - ld)] : bad;
  } else if (c == ld + D) {
    rew[r] = ok ? t.rew[row] : bad;
  } else {
    done[r] = ok ? t.done[row] : bad;
  }
}

__global__ __launch_bounds__(TD3_THREADS) void td3_target_input_kernel(const float* __restrict__ S2,
                                                                       const float* __restrict__ mu_t,
                                                                       const float* __restrict__ noise, int B, int D, int A,
                                                                       int ld, float clip, float* __restrict__ X2) {
  const long long e = (long long)blockIdx.x * TD3_THREADS + threadIdx.x;
  if (e >= (long long)B * ld) return;
  const int r = (int)(e / ld), c = (int)(e % ld);
  float v = 0.f;
  if (c < D) {
    v = S2[(long long)r * D + c];
  } else if (c < D + A) {
    const long long i = (long long)r * A + (c - D);
    const float nz = fminf(fmaxf(noise[i], -clip), clip);
    v = fminf(fmaxf(mu_t[i] + nz, -1.f), 1.f);
  }
  X2[e] = v;
}

template <int NC>
__global__ __launch_bounds__(TD3_THREADS) void td3_critic_loss_kernel(const float* __restrict__ Q, const float* __restrict__ Qt,
                                                                      const float* __restrict__ rew,
                                                                      const float* __restrict__ done, int B, float gamma,
                                                                      float* __restrict__ dQ, float* __restrict__ y_out,
                                                                      float* __restrict__ loss) {
  __shared__ double sm[TD3_THREADS / 64];
  const float inv_b = 1.f / (float)B;
  double s[NC];
#pragma unroll
  for (int i = 0; i < NC; ++i) s[i] = 0.0;
  for (int b = threadIdx.x; b < B; b += TD3_THREADS) {
    float qmin = Qt[b];
#pragma unroll
    for (int i = 1; i < NC; ++i) qmin = fminf(qmin, Qt[(long long)i * B + b]);
    const float y = rew[b] + ((1.f - done[b]) * gamma) * qmin;
    if (y_out) y_out[b] = y;
#pragma unroll
    for (int i = 0; i < NC; ++i) {
      const float d = Q[(long long)i * B + b] - y;
      s[i] += (double)d * (double)d;
      dQ[(long long)i * B + b] = (2.f * d) * inv_b;
    }
  }
  double tot = 0.0;
#pragma unroll
  for (int i = 0; i < NC; ++i) tot += td3_block_sum(s[i], sm) / (double)B;   // sum_i mean_i, critic order
  if (threadIdx.x == 0) loss[0] = (float)tot;
}

__global__ __launch_bounds__(TD3_THREADS) void td3_actor_input_kernel(const float* __restrict__ mu, int B, int D, int A, int ld,
                                                                      float* __restrict__ X) {
  const long long e = (long long)blockIdx.x * TD3_THREADS + threadIdx.x;
  if (e >= (long long)B * A) return;
  const int r = (int)(e / A), a = (int)(e % A);
  X[(long long)r * ld + D + a] = mu[e];
}

// one workgroup: the loss (fixed order) and the B * A seed elements
__global__ __launch_bounds__(TD3_THREADS) void td3_actor_seed_kernel(const float* __restrict__ q1, const float* __restrict__ dX,
                                                                     const float* __restrict__ mu, int B, int D, int A, int ld,
                                                                     float* __restrict__ dmu, float* __restrict__ loss) {
  __shared__ double sm[TD3_THREADS / 64];
  const float inv_b = 1.f / (float)B;
  double s = 0.0;
  for (int b = threadIdx.x; b < B; b += TD3_THREADS) s += (double)q1[b];
  const double tot = td3_block_sum(s, sm);
  if (threadIdx.x == 0) loss[0] = -(float)(tot / (double)B);
  for (long long e = threadIdx.x; e < (long long)B * A; e += TD3_THREADS) {
    const int r = (int)(e / A), a = (int)(e % A);
    const float m = mu[e];
    dmu[e] = (dX[(long long)r * ld + D + a] * -inv_b) * (1.f - m * m);
  }
}

inline unsigned td3_blocks(long long n) { return (unsigned)((n + TD3_THREADS - 1) / TD3_THREADS); }

}  // namespace

extern "C" {

int ia_td3_assemble(const float* ring_obs, const float* ring_next_obs, const float* ring_act, const float* ring_rew,
                    const float* ring_done, int64_t ring_rows, const float* exp_obs, const float* exp_next_obs,
                    const float* exp_act, const float* exp_rew, const float* exp_done, int64_t exp_rows, const int64_t* idx,
                    int B, int n_new, int D, int A, int ld, float* X, float* S, float* S2, float* rew, float* done,
                    void* stream) {
  if (B < 1 || n_new < 0 || n_new > B || D < 1 || A < 1 || ld < D + A || !idx || !X || !S || !S2 || !rew || !done)
    return IA_ERR_ARG;
  if (n_new > 0 && !(ring_obs && ring_next_obs && ring_act && ring_rew && ring_done && ring_rows > 0)) return IA_ERR_ARG;
  if (n_new < B && !(exp_obs && exp_next_obs && exp_act && exp_rew && exp_done && exp_rows > 0)) return IA_ERR_ARG;
  Td3Table ring{ring_obs, ring_next_obs, ring_act, ring_rew, ring_done, n_new > 0 ? (long long)ring_rows : 0};
  Td3Table expert{exp_obs, exp_next_obs, exp_act, exp_rew, exp_done, n_new < B ? (long long)exp_rows : 0};
  hipLaunchKernelGGL(td3_assemble_kernel, dim3(td3_blocks((long long)B * (ld + D + 2))), dim3(TD3_THREADS), 0,
                     (hipStream_t)stream, ring, expert, idx, B, n_new, D, A, ld, X, S, S2, rew, done);
  IA_CHECK_LAUNCH();
  return IA_OK;
}

int ia_td3_target_input(const float* S2, const float* mu_target, const float* noise, int B, int D, int A, int ld,
                        float noise_clip, float* X2, void* stream) {
  if (B < 1 || D < 1 || A < 1 || ld < D + A || !S2 || !mu_target || !noise || !X2) return IA_ERR_ARG;
  hipLaunchKernelGGL(td3_target_input_kernel, dim3(td3_blocks((long long)B * ld)), dim3(TD3_THREADS), 0, (hipStream_t)stream,
                     S2, mu_target, noise, B, D, A, ld, noise_clip, X2);
  IA_CHECK_LAUNCH();
  return IA_OK;
}

int ia_td3_critic_loss(const float* q, const float* q_target, const float* rewards, const float* dones, int B, int n_critics,
                       float gamma, float* dq, float* y, float* loss, void* stream) {
  if (B < 1 || !q || !q_target || !rewards || !dones || !dq || !loss) return IA_ERR_ARG;
  if (n_critics == 1)
    hipLaunchKernelGGL(td3_critic_loss_kernel<1>, dim3(1), dim3(TD3_THREADS), 0, (hipStream_t)stream, q, q_target, rewards,
                       dones, B, gamma, dq, y, loss);
  else if (n_critics == 2)
    hipLaunchKernelGGL(td3_critic_loss_kernel<2>, dim3(1), dim3(TD3_THREADS), 0, (hipStream_t)stream, q, q_target, rewards,
                       dones, B, gamma, dq, y, loss);
  else
    return IA_ERR_UNSUPPORTED;
  IA_CHECK_LAUNCH();
  return IA_OK;
}

int ia_td3_actor_input(const float* mu, int B, int D, int A, int ld, float* X, void* stream) {
  if (B < 1 || D < 1 || A < 1 || ld < D + A || !mu || !X) return IA_ERR_ARG;
  hipLaunchKernelGGL(td3_actor_input_kernel, dim3(td3_blocks((long long)B * A)), dim3(TD3_THREADS), 0, (hipStream_t)stream, mu,
                     B, D, A, ld, X);
  IA_CHECK_LAUNCH();
  return IA_OK;
}

int ia_td3_actor_seed(const float* q1, const float* dX, const float* mu, int B, int D, int A, int ld, float* dmu, float* loss,
                      void* stream) {
  if (B < 1 || D < 1 || A < 1 || ld < D + A || !q1 || !dX || !mu || !dmu || !loss) return IA_ERR_ARG;
  hipLaunchKernelGGL(td3_actor_seed_kernel, dim3(1), dim3(TD3_THREADS), 0, (hipStream_t)stream, q1, dX, mu, B, D, A, ld, dmu,
                     loss);
  IA_CHECK_LAUNCH();
  return IA_OK;
}

}  // extern "C"
