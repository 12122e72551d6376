// DQN / SQIL kernels ([SB3 dqn.py] DQN.train, the Q-network's act step, the TD loss and the target's polyak update).
//   * ia_dqn_update: n_steps consecutive gradient steps of DQN.train on a D -> H -> H -> A ReLU Q-net in ONE launch of
//     ONE workgroup: per step it gathers the minibatch from the learner ring and the expert table, runs the online
//     forward on s next to the target forward on s', forms the TD target, the Huber loss and dQ, goes back through both
//     ReLU layers, takes the gradient norm, clips and applies torch's Adam; the next step reads the updated weights
//     from LDS. Nothing here waits on another workgroup: every hand-off between waves is a workgroup barrier, every sum
//     has a fixed order, so a launch repeats bit for bit and n launches of one step equal one launch of n.
//   * ia_dqn_q_values: Q and its first arg-max for n observations, 64 rows per workgroup, the same forward code.
//   * ia_dqn_td_loss / ia_polyak_update: the pieces the general path (ia_mlp_forward / _backward) lacks.
// The batch goes through the workgroup in chunks of 16 rows; rows past the batch in the last chunk are zero-filled and
// their dQ is zero, so they add exact zeros to every sum.
#include "policy_common.h"

namespace {

constexpr int DQN_THREADS = 256;   // 4 waves, one per SIMD
constexpr int DQN_RC = 16;         // rows per chunk
constexpr int DQN_MAXB = 256;
constexpr int DQN_QROWS = 64;      // rows per workgroup of the act kernel

// LDS image of the parameters: torch's flat order (W1[H][D], b1, W2[H][H], b2, W3[A][H], b3) with every weight row at an
// ODD stride, so that lanes walking the output index (forward) and lanes walking the input index (backward) both hit
// distinct banks.
struct DqnLay {
  int D, A, ld1, ldh;
  int fW1, fb1, fW2, fb2, fW3, fb3, P;      // flat offsets, parameter count
  int lW1, lb1, lW2, lb2, lW3, lb3, LP;     // offsets in the LDS image, its size
};

template <int H>
__host__ __device__ inline DqnLay dqn_layout(int D, int A) {
  DqnLay l;
  l.D = D; l.A = A; l.ld1 = D | 1; l.ldh = H | 1;
  int p = 0;
  l.fW1 = p; p += H * D; l.fb1 = p; p += H; l.fW2 = p; p += H * H; l.fb2 = p; p += H; l.fW3 = p; p += A * H;
  l.fb3 = p; p += A; l.P = p;
  p = 0;
  l.lW1 = p; p += H * l.ld1; l.lb1 = p; p += H; l.lW2 = p; p += H * l.ldh; l.lb2 = p; p += H; l.lW3 = p; p += A * l.ldh;
  l.lb3 = p; p += A; l.LP = (p + 3) & ~3;
  return l;
}

template <int H>
__device__ __forceinline__ int dqn_flat_to_lds(const DqnLay& l, int e) {
  if (e < l.fb1) return l.lW1 + (e / l.D) * l.ld1 + e % l.D;
  if (e < l.fW2) return l.lb1 + (e - l.fb1);
  if (e < l.fb2) { const int f = e - l.fW2; return l.lW2 + (f / H) * l.ldh + f % H; }
  if (e < l.fW3) return l.lb2 + (e - l.fb2);
  if (e < l.fb3) { const int f = e - l.fW3; return l.lW3 + (f / H) * l.ldh + f % H; }
  return l.lb3 + (e - l.fb3);
}

template <int H>
__device__ __forceinline__ void dqn_load_params(const DqnLay& l, const float* __restrict__ flat, float* __restrict__ img) {
  for (int e = threadIdx.x; e < l.P; e += DQN_THREADS) img[dqn_flat_to_lds<H>(l, e)] = flat[e];
}

// out[r][j] = act(b[j] + sum_k in[r][k] W[j][k]) for the 16 rows of a chunk and N = H outputs, for NP independent
// problems at once (the online and the target net: twice the independent chains per lane). Lane -> j, wave -> rows
// wave, wave + 4, wave + 8, wave + 12.
template <int H, int NP, bool RELU>
__device__ __forceinline__ void dqn_dense_h(const float* const (&W)[NP], int ldw, const float* const (&b)[NP],
                                            const float* const (&in)[NP], int ldi, int K, float* const (&out)[NP]) {
  constexpr int PER = DQN_RC * H / DQN_THREADS;   // rows per thread: 4 (H = 64) or 2 (H = 32)
  constexpr int RSTEP = DQN_THREADS / H;
  const int j = threadIdx.x % H, r0 = threadIdx.x / H;
  // float64 accumulators (half-rate FMAs, but the loop waits on LDS, not on the ALU): h and Q leave this function as the
  // correctly rounded float32 of their float64 sums, so that delta = Q - target of a row in the Huber loss's quadratic zone
  // carries representation error only
  double acc[NP][PER];
#pragma unroll
  for (int p = 0; p < NP; ++p)
#pragma unroll
    for (int i = 0; i < PER; ++i) acc[p][i] = 0.0;
#pragma unroll 4
  for (int k = 0; k < K; ++k) {
#pragma unroll
    for (int p = 0; p < NP; ++p) {
      const double w = (double)W[p][j * ldw + k];
#pragma unroll
      for (int i = 0; i < PER; ++i) acc[p][i] = __builtin_fma((double)in[p][(r0 + RSTEP * i) * ldi + k], w, acc[p][i]);
    }
  }
#pragma unroll
  for (int p = 0; p < NP; ++p)
#pragma unroll
    for (int i = 0; i < PER; ++i) {
      const float v = (float)(acc[p][i] + (double)b[p][j]);
      out[p][(r0 + RSTEP * i) * H + j] = RELU ? fmaxf(v, 0.f) : v;
    }
}

// the head: out[r][a] = b[a] + sum_k in[r][k] W[a][k], 16 * A <= 256 outputs, one per thread
template <int H, int NP>
__device__ __forceinline__ void dqn_head(const float* const (&W)[NP], int ldw, const float* const (&b)[NP],
                                         const float* const (&in)[NP], int A, float* const (&out)[NP]) {
  const int e = threadIdx.x;
  if (e >= DQN_RC * A) return;
  const int r = e / A, a = e % A;
#pragma unroll
  for (int p = 0; p < NP; ++p) {
    double acc = 0.0;
#pragma unroll 8
    for (int k = 0; k < H; ++k) acc = __builtin_fma((double)in[p][r * H + k], (double)W[p][a * ldw + k], acc);
    out[p][r * MAXA + a] = (float)(acc + (double)b[p][a]);
  }
}

// g[j][k] += sum_r dz[r][j] in[r][k] (rows in order) over a flat [N][K] gradient piece; gb[j] += sum_r dz[r][j]
__device__ __forceinline__ void dqn_wgrad(const float* __restrict__ dz, int ldz, int N, const float* __restrict__ in, int ldi,
                                          int K, float* __restrict__ g, float* __restrict__ gb) {
  for (int e = threadIdx.x; e < N * K; e += DQN_THREADS) {
    const int j = e / K, k = e % K;
    float s = 0.f;
#pragma unroll
    for (int r = 0; r < DQN_RC; ++r) s = __builtin_fmaf(dz[r * ldz + j], in[r * ldi + k], s);
    g[e] += s;
  }
  for (int j = threadIdx.x; j < N; j += DQN_THREADS) {
    float s = 0.f;
#pragma unroll
    for (int r = 0; r < DQN_RC; ++r) s += dz[r * ldz + j];
    gb[j] += s;
  }
}

// fixed-order sum over the workgroup: xor butterfly inside each wave, then the four wave sums in wave order
__device__ __forceinline__ float dqn_block_sum(float v, float* sm) {
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) v += __shfl_xor(v, o, 64);
  __syncthreads();
  if ((threadIdx.x & 63) == 0) sm[threadIdx.x >> 6] = v;
  __syncthreads();
  float t = 0.f;
#pragma unroll
  for (int w = 0; w < DQN_THREADS / 64; ++w) t += sm[w];
  return t;
}

// [torch smooth_l1_loss, beta = 1] term and derivative for delta = Q(s, a) - target
__device__ __forceinline__ float dqn_huber(float delta, float* dd) {
  const float ad = fabsf(delta);
  *dd = ad < 1.f ? delta : (delta > 0.f ? 1.f : -1.f);
  return ad < 1.f ? 0.5f * delta * delta : ad - 0.5f;
}

// torch/optim/adam.py _single_tensor_adam for one element with the scalars torch hands its kernels: `1 - beta` formed in
// DOUBLE and then rounded (1.f - 0.999f is 0.99998713e-3: 1.3e-5 off, which a dozen steps carry into the seventh digit of
// the parameters), lerp for the first moment, mul + addcmul for the second, sqrt / bc2_sqrt + eps, addcdiv.
struct DqnAdam {
  float omb1, beta2, omb2, eps;
};
__host__ inline DqnAdam dqn_adam_scalars(double beta1, double beta2, float eps) {
  DqnAdam a;
  a.omb1 = (float)(1.0 - beta1); a.beta2 = (float)beta2; a.omb2 = (float)(1.0 - beta2); a.eps = eps;
  return a;
}
__device__ __forceinline__ float dqn_adam_element(float p, float grad, float* __restrict__ m, float* __restrict__ v,
                                                  const DqnAdam& a, float step_size, float bc2_sqrt) {
  const float mi = *m + (grad - *m) * a.omb1;
  const float vi = *v * a.beta2 + a.omb2 * grad * grad;
  *m = mi;
  *v = vi;
  return p - step_size * (mi / (sqrtf(vi) / bc2_sqrt + a.eps));
}

constexpr int DQN_MAX_STEPS = 32;

struct DqnUpdate {
  int D, A, B, n_new, n_steps;
  float* params; const float* tparams; float* exp_avg; float* exp_avg_sq;
  const float* r_obs; const float* r_next; const int64_t* r_act; const float* r_rew; const float* r_done;
  const float* e_obs; const float* e_next; const int64_t* e_act; const float* e_rew; const float* e_done;
  const int64_t* idx;
  float gamma, max_norm;
  DqnAdam adam;
  float step_size[DQN_MAX_STEPS], bc2_sqrt[DQN_MAX_STEPS];
  float* stats; float* grad_out;
};

template <int H>
__host__ __device__ inline size_t dqn_update_lds_floats(int D, int A) {
  const DqnLay l = dqn_layout<H>(D, A);
  const int Pp = (l.P + 3) & ~3;
  // online image, target image, flat gradient, x, x', four [16][H] tiles, Q, Qt, per-row scalars, loss terms, wave sums
  return (size_t)2 * l.LP + Pp + 2 * DQN_RC * MAXD + 4 * DQN_RC * H + 2 * DQN_RC * MAXA + 4 * DQN_RC + DQN_MAXB + 8;
}

template <int H>
__global__ __launch_bounds__(DQN_THREADS) void dqn_update_kernel(const DqnUpdate u) {
  extern __shared__ __align__(16) float lds[];
  const DqnLay l = dqn_layout<H>(u.D, u.A);
  const int D = u.D, A = u.A, B = u.B, tid = threadIdx.x;
  const int Pp = (l.P + 3) & ~3;
  float* Wo = lds;
  float* Wt = Wo + l.LP;
  float* G = Wt + l.LP;
  float* X = G + Pp;
  float* Xn = X + DQN_RC * MAXD;
  float* H1 = Xn + DQN_RC * MAXD;
  float* H2 = H1 + DQN_RC * H;
  float* T1 = H2 + DQN_RC * H;      // target hidden 1, then dz2
  float* T2 = T1 + DQN_RC * H;      // target hidden 2, then dz1
  float* Q = T2 + DQN_RC * H;
  float* Qt = Q + DQN_RC * MAXA;
  float* dsel = Qt + DQN_RC * MAXA;  // [16] d loss / d Q(s, a) of the taken action
  float* rew = dsel + DQN_RC;
  float* done = rew + DQN_RC;
  int* act = reinterpret_cast<int*>(done + DQN_RC);
  float* rowloss = reinterpret_cast<float*>(act + DQN_RC);   // [256]
  float* sm = rowloss + DQN_MAXB;

  dqn_load_params<H>(l, u.params, Wo);
  dqn_load_params<H>(l, u.tparams, Wt);
  const float inv_b = 1.f / (float)B;

  for (int step = 0; step < u.n_steps; ++step) {
    for (int e = tid; e < l.P; e += DQN_THREADS) G[e] = 0.f;
    if (tid < DQN_MAXB) rowloss[tid] = 0.f;
    const int64_t* idx = u.idx + (long long)step * B;
    for (int c0 = 0; c0 < B; c0 += DQN_RC) {
      __syncthreads();   // the previous chunk's tiles (and, first, the parameter images / cleared sums) are done with
      // ---- gather the chunk: rows < n_new from the learner ring, the rest from the expert table
      for (int e = tid; e < DQN_RC * D; e += DQN_THREADS) {
        const int r = e / D, k = e % D, b = c0 + r;
        float x = 0.f, xn = 0.f;
        if (b < B) {
          const long long g = idx[b];
          const bool ring = b < u.n_new;
          x = (ring ? u.r_obs : u.e_obs)[g * D + k];
          xn = (ring ? u.r_next : u.e_next)[g * D + k];
        }
        X[r * D + k] = x;
        Xn[r * D + k] = xn;
      }
      if (tid < DQN_RC) {
        const int b = c0 + tid;
        int a = 0;
        float rw = 0.f, dn = 0.f;
        if (b < B) {
          const long long g = idx[b];
          const bool ring = b < u.n_new;
          a = (int)(ring ? u.r_act : u.e_act)[g];
          rw = (ring ? u.r_rew : u.e_rew)[g];
          dn = (ring ? u.r_done : u.e_done)[g];
        }
        act[tid] = a; rew[tid] = rw; done[tid] = dn;
      }
      __syncthreads();
      // ---- forward: online on s, target on s'
      {
        const float* const W[2] = {Wo + l.lW1, Wt + l.lW1};
        const float* const bb[2] = {Wo + l.lb1, Wt + l.lb1};
        const float* const in[2] = {X, Xn};
        float* const out[2] = {H1, T1};
        dqn_dense_h<H, 2, true>(W, l.ld1, bb, in, D, D, out);
      }
      __syncthreads();
      {
        const float* const W[2] = {Wo + l.lW2, Wt + l.lW2};
        const float* const bb[2] = {Wo + l.lb2, Wt + l.lb2};
        const float* const in[2] = {H1, T1};
        float* const out[2] = {H2, T2};
        dqn_dense_h<H, 2, true>(W, l.ldh, bb, in, H, H, out);
      }
      __syncthreads();
      {
        const float* const W[2] = {Wo + l.lW3, Wt + l.lW3};
        const float* const bb[2] = {Wo + l.lb3, Wt + l.lb3};
        const float* const in[2] = {H2, T2};
        float* const out[2] = {Q, Qt};
        dqn_head<H, 2>(W, l.ldh, bb, in, A, out);
      }
      __syncthreads();
      // ---- TD target, Huber term, dQ of the taken action (zero on rows past the batch)
      if (tid < DQN_RC) {
        const int b = c0 + tid;
        float d = 0.f;
        if (b < B) {
          float tmax = Qt[tid * MAXA];
          for (int a = 1; a < A; ++a) tmax = fmaxf(tmax, Qt[tid * MAXA + a]);
          const float target = rew[tid] + ((1.f - done[tid]) * u.gamma) * tmax;
          float dd;
          rowloss[b] = dqn_huber(Q[tid * MAXA + act[tid]] - target, &dd);
          d = dd * inv_b;
        }
        dsel[tid] = d;
      }
      __syncthreads();
      // ---- dz2[r][k] = dsel[r] W3[act r][k] (h2 > 0) into T1; head gradient (only the taken action's column is non-zero)
      for (int e = tid; e < DQN_RC * H; e += DQN_THREADS) {
        const int r = e / H, k = e % H;
        T1[e] = H2[e] > 0.f ? dsel[r] * Wo[l.lW3 + act[r] * l.ldh + k] : 0.f;
      }
      for (int e = tid; e < A * H; e += DQN_THREADS) {
        const int a = e / H, k = e % H;
        float s = 0.f;
#pragma unroll
        for (int r = 0; r < DQN_RC; ++r) s = __builtin_fmaf(act[r] == a ? dsel[r] : 0.f, H2[r * H + k], s);
        G[l.fW3 + e] += s;
      }
      if (tid < A) {
        float s = 0.f;
#pragma unroll
        for (int r = 0; r < DQN_RC; ++r) s += act[r] == tid ? dsel[r] : 0.f;
        G[l.fb3 + tid] += s;
      }
      __syncthreads();
      // ---- dz1[r][k] = (sum_j dz2[r][j] W2[j][k]) (h1 > 0) into T2; layer-2 gradient
      {
        constexpr int PER = DQN_RC * H / DQN_THREADS, RSTEP = DQN_THREADS / H;
        const int k = tid % H, r0 = tid / H;
        double acc[PER];
#pragma unroll
        for (int i = 0; i < PER; ++i) acc[i] = 0.0;
#pragma unroll 4
        for (int j = 0; j < H; ++j) {
          const double w = (double)Wo[l.lW2 + j * l.ldh + k];
#pragma unroll
          for (int i = 0; i < PER; ++i) acc[i] = __builtin_fma((double)T1[(r0 + RSTEP * i) * H + j], w, acc[i]);
        }
#pragma unroll
        for (int i = 0; i < PER; ++i) {
          const int o = (r0 + RSTEP * i) * H + k;
          T2[o] = H1[o] > 0.f ? (float)acc[i] : 0.f;
        }
      }
      dqn_wgrad(T1, H, H, H1, H, H, G + l.fW2, G + l.fb2);
      __syncthreads();
      dqn_wgrad(T2, H, H, X, D, D, G + l.fW1, G + l.fb1);
    }
    __syncthreads();
    // ---- loss, gradient norm, clip, Adam
    const float loss = dqn_block_sum(rowloss[tid], sm) * inv_b;
    float q = 0.f;
    for (int e = tid; e < l.P; e += DQN_THREADS) q += G[e] * G[e];
    const float total = sqrtf(dqn_block_sum(q, sm));
    const float coef = fminf(u.max_norm / (total + 1e-6f), 1.0f);   // torch.nn.utils.clip_grad_norm_
    if (tid == 0) {
      u.stats[2 * step] = loss;
      u.stats[2 * step + 1] = total;
    }
    const float step_size = u.step_size[step], bc2 = u.bc2_sqrt[step];
    const bool last = step == u.n_steps - 1;
    for (int e = tid; e < l.P; e += DQN_THREADS) {
      const float grad = G[e] * coef;
      const int li = dqn_flat_to_lds<H>(l, e);
      const float pn = dqn_adam_element(Wo[li], grad, u.exp_avg + e, u.exp_avg_sq + e, u.adam, step_size, bc2);
      Wo[li] = pn;
      u.params[e] = pn;
      if (last && u.grad_out) u.grad_out[e] = grad;
    }
    // (the next step's first barrier stands between these writes and its reads)
  }
}

template <int H>
__global__ __launch_bounds__(DQN_THREADS) void dqn_q_kernel(const float* __restrict__ params, const float* __restrict__ obs,
                                                            int n, int D, int A, float* __restrict__ qout,
                                                            int64_t* __restrict__ amax) {
  extern __shared__ __align__(16) float lds[];
  const DqnLay l = dqn_layout<H>(D, A);
  const int tid = threadIdx.x;
  float* Wo = lds;
  float* X = Wo + l.LP;
  float* H1 = X + DQN_RC * MAXD;
  float* H2 = H1 + DQN_RC * H;
  float* Q = H2 + DQN_RC * H;
  dqn_load_params<H>(l, params, Wo);
  const long long base = (long long)blockIdx.x * DQN_QROWS;
  for (int c0 = 0; c0 < DQN_QROWS && base + c0 < n; c0 += DQN_RC) {
    __syncthreads();
    for (int e = tid; e < DQN_RC * D; e += DQN_THREADS) {
      const long long row = base + c0 + e / D;
      X[e] = row < n ? obs[row * D + e % D] : 0.f;
    }
    __syncthreads();
    {
      const float* const W[1] = {Wo + l.lW1};
      const float* const bb[1] = {Wo + l.lb1};
      const float* const in[1] = {X};
      float* const out[1] = {H1};
      dqn_dense_h<H, 1, true>(W, l.ld1, bb, in, D, D, out);
    }
    __syncthreads();
    {
      const float* const W[1] = {Wo + l.lW2};
      const float* const bb[1] = {Wo + l.lb2};
      const float* const in[1] = {H1};
      float* const out[1] = {H2};
      dqn_dense_h<H, 1, true>(W, l.ldh, bb, in, H, H, out);
    }
    __syncthreads();
    {
      const float* const W[1] = {Wo + l.lW3};
      const float* const bb[1] = {Wo + l.lb3};
      const float* const in[1] = {H2};
      float* const out[1] = {Q};
      dqn_head<H, 1>(W, l.ldh, bb, in, A, out);
    }
    __syncthreads();
    if (tid < DQN_RC) {
      const long long row = base + c0 + tid;
      if (row < n) {
        int best = 0;
        float bq = Q[tid * MAXA];
        qout[row * A] = bq;
        for (int a = 1; a < A; ++a) {
          const float v = Q[tid * MAXA + a];
          qout[row * A + a] = v;
          if (v > bq) { bq = v; best = a; }
        }
        amax[row] = best;
      }
    }
  }
}

// One workgroup: per-row Huber terms, dQ and the mean (per-thread sums over rows t, t + 256, ... then dqn_block_sum).
__global__ __launch_bounds__(DQN_THREADS) void dqn_td_loss_kernel(const float* __restrict__ Q, const float* __restrict__ Qt,
                                                                  const int64_t* __restrict__ act,
                                                                  const float* __restrict__ rew,
                                                                  const float* __restrict__ done, int B, int A, float gamma,
                                                                  float* __restrict__ dQ, float* __restrict__ terms,
                                                                  float* __restrict__ loss) {
  __shared__ float sm[8];
  const float inv_b = 1.f / (float)B;
  float s = 0.f;
  for (int b = threadIdx.x; b < B; b += DQN_THREADS) {
    float tmax = Qt[(long long)b * A];
    for (int a = 1; a < A; ++a) tmax = fmaxf(tmax, Qt[(long long)b * A + a]);
    const float target = rew[b] + ((1.f - done[b]) * gamma) * tmax;
    const int ab = (int)act[b];
    float dd;
    const float t = dqn_huber(Q[(long long)b * A + ab] - target, &dd);
    terms[b] = t;
    s += t;
    for (int a = 0; a < A; ++a) dQ[(long long)b * A + a] = a == ab ? dd * inv_b : 0.f;
  }
  const float tot = dqn_block_sum(s, sm);
  if (threadIdx.x == 0) loss[0] = tot * inv_b;
}

__global__ void dqn_adam_kernel(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ m,
                                float* __restrict__ v, long long n, DqnAdam a, float wd, float step_size, float bc2_sqrt) {
  const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const float pi = p[i];
  p[i] = dqn_adam_element(pi, wd != 0.f ? g[i] + wd * pi : g[i], m + i, v + i, a, step_size, bc2_sqrt);
}

__global__ void dqn_polyak_kernel(const float* __restrict__ online, float* __restrict__ target, long long n, float tau) {
  const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  target[i] = tau == 1.f ? online[i] : tau * online[i] + (1.f - tau) * target[i];
}

template <typename K>
int dqn_raise_lds(K kern, size_t bytes) {
  if (bytes > 160 * 1024) return IA_ERR_UNSUPPORTED;
  if (bytes > 64 * 1024 &&
      hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes) !=
          hipSuccess)
    return IA_ERR_UNSUPPORTED;
  return IA_OK;
}

bool dqn_shape_ok(int D, int H, int A) { return D >= 1 && D <= MAXD && A >= 1 && A <= MAXA && (H == 32 || H == 64); }

}  // namespace

extern "C" {

int ia_dqn_update_ok(int D, int H, int A, int B) { return dqn_shape_ok(D, H, A) && B >= 1 && B <= DQN_MAXB ? 1 : 0; }

int ia_dqn_update(int D, int H, int A, int B, int n_new, int n_steps, float* params, const float* target_params,
                  float* exp_avg, float* exp_avg_sq, const float* ring_obs, const float* ring_next_obs,
                  const int64_t* ring_act, const float* ring_rew, const float* ring_done, const float* exp_obs,
                  const float* exp_next_obs, const int64_t* exp_act, const float* exp_rew, const float* exp_done,
                  const int64_t* idx, float gamma, float max_grad_norm, double beta1, double beta2, float eps,
                  const float* adam_scalars, float* stats, float* grad_out, void* stream) {
  if (!ia_dqn_update_ok(D, H, A, B)) return IA_ERR_UNSUPPORTED;
  if (n_steps < 1 || n_new < 0 || n_new > B || !params || !target_params || !exp_avg || !exp_avg_sq || !idx ||
      !adam_scalars || !stats)
    return IA_ERR_ARG;
  if (n_new > 0 && !(ring_obs && ring_next_obs && ring_act && ring_rew && ring_done)) return IA_ERR_ARG;
  if (n_new < B && !(exp_obs && exp_next_obs && exp_act && exp_rew && exp_done)) return IA_ERR_ARG;
  const size_t lds = (H == 64 ? dqn_update_lds_floats<64>(D, A) : dqn_update_lds_floats<32>(D, A)) * sizeof(float);
  const int rc = H == 64 ? dqn_raise_lds(dqn_update_kernel<64>, lds) : dqn_raise_lds(dqn_update_kernel<32>, lds);
  if (rc != IA_OK) return rc;
  // the steps of one call in launches of at most DQN_MAX_STEPS (their Adam scalars travel as kernel arguments)
  for (int s0 = 0; s0 < n_steps; s0 += DQN_MAX_STEPS) {
    DqnUpdate u;
    u.D = D; u.A = A; u.B = B; u.n_new = n_new;
    u.n_steps = n_steps - s0 < DQN_MAX_STEPS ? n_steps - s0 : DQN_MAX_STEPS;
    u.params = params; u.tparams = target_params; u.exp_avg = exp_avg; u.exp_avg_sq = exp_avg_sq;
    u.r_obs = ring_obs; u.r_next = ring_next_obs; u.r_act = ring_act; u.r_rew = ring_rew; u.r_done = ring_done;
    u.e_obs = exp_obs; u.e_next = exp_next_obs; u.e_act = exp_act; u.e_rew = exp_rew; u.e_done = exp_done;
    u.idx = idx + (long long)s0 * B;
    u.gamma = gamma; u.max_norm = max_grad_norm; u.adam = dqn_adam_scalars(beta1, beta2, eps);
    for (int i = 0; i < DQN_MAX_STEPS; ++i) {
      u.step_size[i] = i < u.n_steps ? adam_scalars[2 * (s0 + i)] : 0.f;
      u.bc2_sqrt[i] = i < u.n_steps ? adam_scalars[2 * (s0 + i) + 1] : 1.f;
    }
    u.stats = stats + 2 * s0;
    u.grad_out = s0 + u.n_steps == n_steps ? grad_out : nullptr;
    if (H == 64)
      hipLaunchKernelGGL(dqn_update_kernel<64>, dim3(1), dim3(DQN_THREADS), lds, (hipStream_t)stream, u);
    else
      hipLaunchKernelGGL(dqn_update_kernel<32>, dim3(1), dim3(DQN_THREADS), lds, (hipStream_t)stream, u);
    IA_CHECK_LAUNCH();
  }
  return IA_OK;
}

int ia_dqn_q_values(int D, int H, int A, const float* params, const float* obs, int n, float* q, int64_t* argmax,
                    void* stream) {
  if (!dqn_shape_ok(D, H, A)) return IA_ERR_UNSUPPORTED;
  if (n < 0 || !params || (n > 0 && (!obs || !q || !argmax))) return IA_ERR_ARG;
  if (n == 0) return IA_OK;
  const DqnLay l = H == 64 ? dqn_layout<64>(D, A) : dqn_layout<32>(D, A);
  const size_t lds = ((size_t)l.LP + DQN_RC * MAXD + 2 * DQN_RC * H + DQN_RC * MAXA) * sizeof(float);
  const int blocks = (n + DQN_QROWS - 1) / DQN_QROWS;
  if (H == 64)
    hipLaunchKernelGGL(dqn_q_kernel<64>, dim3(blocks), dim3(DQN_THREADS), lds, (hipStream_t)stream, params, obs, n, D, A, q,
                       argmax);
  else
    hipLaunchKernelGGL(dqn_q_kernel<32>, dim3(blocks), dim3(DQN_THREADS), lds, (hipStream_t)stream, params, obs, n, D, A, q,
                       argmax);
  IA_CHECK_LAUNCH();
  return IA_OK;
}

int ia_dqn_td_loss(const float* q, const float* q_target, const int64_t* actions, const float* rewards, const float* dones,
                   int B, int A, float gamma, float* dq, float* terms, float* loss, void* stream) {
  if (B < 1 || A < 1 || !q || !q_target || !actions || !rewards || !dones || !dq || !terms || !loss) return IA_ERR_ARG;
  hipLaunchKernelGGL(dqn_td_loss_kernel, dim3(1), dim3(DQN_THREADS), 0, (hipStream_t)stream, q, q_target, actions, rewards,
                     dones, B, A, gamma, dq, terms, loss);
  IA_CHECK_LAUNCH();
  return IA_OK;
}

int ia_dqn_adam_step(float* params, const float* grads, float* exp_avg, float* exp_avg_sq, int64_t n, double beta1,
                     double beta2, float eps, float weight_decay, float step_size, float bc2_sqrt, void* stream) {
  if (n <= 0 || !params || !grads || !exp_avg || !exp_avg_sq) return IA_ERR_ARG;
  hipLaunchKernelGGL(dqn_adam_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, params, grads,
                     exp_avg, exp_avg_sq, (long long)n, dqn_adam_scalars(beta1, beta2, eps), weight_decay, step_size,
                     bc2_sqrt);
  IA_CHECK_LAUNCH();
  return IA_OK;
}

int ia_polyak_update(const float* online, float* target, int64_t n, float tau, void* stream) {
  if (n < 0 || (n > 0 && (!online || !target))) return IA_ERR_ARG;
  if (n == 0) return IA_OK;
  hipLaunchKernelGGL(dqn_polyak_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, online, target,
                     (long long)n, tau);
  IA_CHECK_LAUNCH();
  return IA_OK;
}

}  // extern "C"
