// Finite-horizon tabular maximum-causal-entropy planning (algorithms/mce_irl.py):
//   * the soft Bellman backup (mce_partition_fh :38-93), one launch per timestep, a wave per state;
//   * the forward occupancy pass (mce_occupancy_measures :96-144), per timestep one slab launch over the S*A rows of T and
//     one fixed-order slab sum, then the discounted sum over time;
//   * the reward net's dOut and the termination statistics of MCEIRL.train (:467-544).
// Every table is float64 (NumPy's dtype in the reference); the float32 reward is widened on load. No kernel here waits
// on another workgroup: timesteps depend on each other through launch order on one stream, and sums that cross
// workgroups go through slabs added in a fixed order (no floating-point atomics), so results repeat bit for bit.
#include "common.h"
#include "../../include/imitation_hip.h"

namespace {

constexpr int MCE_THREADS = 256;            // 4 waves
constexpr int MCE_WAVES = MCE_THREADS / 64;
constexpr int MCE_ACHUNK = 8;               // actions whose running sums a wave keeps in registers at once
constexpr int MCE_MAX_A = 1024;             // Q rows wait in LDS for their log-sum-exp: 4 waves * 1024 * 8 B = 32 KiB
constexpr int MCE_SLAB_ROWS = 32;           // least rows of T per forward slab
constexpr int MCE_MAX_SLABS = 128;

__device__ __forceinline__ double wave_sum_f64(double v) {
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}
__device__ __forceinline__ double wave_max_f64(double v) {
  for (int o = 32; o > 0; o >>= 1) v = fmax(v, __shfl_xor(v, o, 64));
  return v;
}

// One timestep of the backup. Wave w of block b owns state s = b * 4 + w. Vnext == nullptr: the base case Q = r.
// Otherwise the wave walks the A contiguous rows T[s, a, :] in chunks of MCE_ACHUNK actions: lane l reads s' = l, l + 64,
// ... (VEC2: pairs 2l, 2l + 1, one 16-byte load; S even keeps every row 16-byte aligned) of each row of the chunk next to
// one read of Vnext, keeps MCE_ACHUNK running sums, and the wave reduces them. The chunk's Q values go to the wave's LDS
// row; once all A are there the wave takes max and sum(exp) over them and writes V, Q and pi -- Q never comes back from
// memory.
template <bool VEC2>
__global__ __launch_bounds__(MCE_THREADS) void mce_backup_kernel(const double* __restrict__ T,
                                                                 const float* __restrict__ reward, int S, int A,
                                                                 double discount, const double* __restrict__ Vnext,
                                                                 double* __restrict__ V, double* __restrict__ Q,
                                                                 double* __restrict__ pi) {
  extern __shared__ double q_lds[];   // [MCE_WAVES][A]
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int s = blockIdx.x * MCE_WAVES + wave;
  if (s >= S) return;   // (whole waves leave; nothing below synchronises the block)
  double* q = q_lds + (long long)wave * A;
  const double r = (double)reward[s];
  if (Vnext == nullptr) {
    for (int a = lane; a < A; a += 64) q[a] = r;
  } else {
    const double* Ts = T + (long long)s * A * S;
    for (int a0 = 0; a0 < A; a0 += MCE_ACHUNK) {
      double acc[MCE_ACHUNK];
#pragma unroll
      for (int j = 0; j < MCE_ACHUNK; ++j) acc[j] = 0.0;
      if (VEC2) {
        for (int sp = 2 * lane; sp < S; sp += 128) {
          const double2 v = *reinterpret_cast<const double2*>(Vnext + sp);
#pragma unroll
          for (int j = 0; j < MCE_ACHUNK; ++j) {
            if (a0 + j < A) {
              const double2 t = *reinterpret_cast<const double2*>(Ts + (long long)(a0 + j) * S + sp);
              acc[j] += t.x * v.x;
              acc[j] += t.y * v.y;
            }
          }
        }
      } else {
        for (int sp = lane; sp < S; sp += 64) {
          const double v = Vnext[sp];
#pragma unroll
          for (int j = 0; j < MCE_ACHUNK; ++j) {
            if (a0 + j < A) acc[j] += Ts[(long long)(a0 + j) * S + sp] * v;
          }
        }
      }
#pragma unroll
      for (int j = 0; j < MCE_ACHUNK; ++j) {
        const double tot = wave_sum_f64(acc[j]);
        if (lane == 0 && a0 + j < A) q[a0 + j] = r + discount * tot;
      }
    }
  }
  // the wave's own LDS row: written and read by this wave only (its lanes run in lockstep; the fence orders the LDS ops)
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
  // scipy.special.logsumexp: m = max, V = log(sum exp(Q - m)) + m
  double m = -INFINITY;
  for (int a = lane; a < A; a += 64) m = fmax(m, q[a]);
  m = wave_max_f64(m);
  if (!isfinite(m)) m = 0.0;
  double e = 0.0;
  for (int a = lane; a < A; a += 64) e += exp(q[a] - m);
  e = wave_sum_f64(e);
  const double v = log(e) + m;
  if (lane == 0) V[s] = v;
  const long long o = (long long)s * A;
  for (int a = lane; a < A; a += 64) {
    const double qa = q[a];
    Q[o + a] = qa;
    pi[o + a] = exp(qa - v);
  }
}

// One timestep of the occupancy pass, slab `blockIdx.y` of the S*A rows of T: thread -> one s' (lanes along s', so each
// row is read in 512-byte runs per wave); the row's weight D[s] * pi[s, a] is the same in every lane. ws[slab, s'] <-
// the slab's sum.
__global__ __launch_bounds__(MCE_THREADS) void mce_forward_slab_kernel(const double* __restrict__ T,
                                                                       const double* __restrict__ pi_t,
                                                                       const double* __restrict__ D_t, int S, int A,
                                                                       int rows_per_slab, double* __restrict__ ws) {
  const int sp = blockIdx.x * MCE_THREADS + threadIdx.x;
  if (sp >= S) return;
  const long long n_rows = (long long)S * A;
  const long long r0 = (long long)blockIdx.y * rows_per_slab;
  const long long r1 = r0 + rows_per_slab < n_rows ? r0 + rows_per_slab : n_rows;
  int s = (int)(r0 / A), a = (int)(r0 % A);
  double acc = 0.0;
#pragma unroll 4
  for (long long row = r0; row < r1; ++row) {
    const double w = D_t[s] * pi_t[row];
    acc += w * T[row * S + sp];
    if (++a == A) {
      a = 0;
      ++s;
    }
  }
  ws[(long long)blockIdx.y * S + sp] = acc;
}

// D_next[s'] = the slabs' sums in slab order
__global__ void mce_forward_sum_kernel(const double* __restrict__ ws, int n_slabs, int S, double* __restrict__ D_next) {
  const int sp = blockIdx.x * blockDim.x + threadIdx.x;
  if (sp >= S) return;
  double acc = 0.0;
  for (int k = 0; k < n_slabs; ++k) acc += ws[(long long)k * S + sp];
  D_next[sp] = acc;
}

__global__ void mce_copy_f64_kernel(const double* __restrict__ src, int n, double* __restrict__ dst) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) dst[i] = src[i];
}

// rollout.discounted_sum over the H + 1 rows of D: a plain sum in time order when discount == 1, else polyval's Horner form
__global__ void mce_discounted_sum_kernel(const double* __restrict__ D, int rows, int S, double discount,
                                          double* __restrict__ Dcum) {
  const int s = blockIdx.x * blockDim.x + threadIdx.x;
  if (s >= S) return;
  double acc;
  if (discount == 1.0) {
    acc = 0.0;
    for (int t = 0; t < rows; ++t) acc += D[(long long)t * S + s];
  } else {
    acc = D[(long long)(rows - 1) * S + s];
    for (int t = rows - 2; t >= 0; --t) acc = D[(long long)t * S + s] + acc * discount;
  }
  Dcum[s] = acc;
}

// One workgroup: w = (float)(Dcum - demo_om), stats[0] = max |demo_om - Dcum|
__global__ __launch_bounds__(MCE_THREADS) void mce_weights_kernel(const double* __restrict__ Dcum,
                                                                  const double* __restrict__ demo_om, int S,
                                                                  float* __restrict__ w, double* __restrict__ stats) {
  __shared__ double red[MCE_WAVES];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  double m = 0.0;
  bool bad = false;
  for (int s = threadIdx.x; s < S; s += MCE_THREADS) {
    const double v = Dcum[s], d = demo_om[s];
    w[s] = (float)(v - d);
    const double ad = fabs(d - v);
    bad = bad || (ad != ad);
    m = fmax(m, ad);
  }
  if (bad) m = NAN;   // np.max propagates NaN; fmax would drop it
  // NaN-propagating reductions
  for (int o = 32; o > 0; o >>= 1) {
    const double x = __shfl_xor(m, o, 64);
    m = (m != m || x != x) ? NAN : fmax(m, x);
  }
  if (lane == 0) red[wave] = m;
  __syncthreads();
  if (threadIdx.x == 0) {
    double a = red[0];
    for (int k = 1; k < MCE_WAVES; ++k) a = (a != a || red[k] != red[k]) ? NAN : fmax(a, red[k]);
    stats[0] = a;
  }
}

// One workgroup: float32 L2 norms of two flat vectors (util.tensor_iter_norm's dtype), widened into stats[1], stats[2]
__global__ __launch_bounds__(MCE_THREADS) void mce_norms_kernel(const float* __restrict__ grads,
                                                                const float* __restrict__ params, long long n,
                                                                double* __restrict__ stats) {
  __shared__ float red[MCE_WAVES][2];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  float g = 0.f, p = 0.f;
  for (long long i = threadIdx.x; i < n; i += MCE_THREADS) {
    g += grads[i] * grads[i];
    p += params[i] * params[i];
  }
  for (int o = 32; o > 0; o >>= 1) {
    g += __shfl_xor(g, o, 64);
    p += __shfl_xor(p, o, 64);
  }
  if (lane == 0) {
    red[wave][0] = g;
    red[wave][1] = p;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    float a = 0.f, b = 0.f;
    for (int k = 0; k < MCE_WAVES; ++k) {
      a += red[k][0];
      b += red[k][1];
    }
    stats[1] = (double)sqrtf(a);
    stats[2] = (double)sqrtf(b);
  }
}

inline int cdiv(long long a, long long b) { return (int)((a + b - 1) / b); }

inline int forward_slabs(int S, int A) {
  const long long rows = (long long)S * A;
  long long n = (rows + MCE_SLAB_ROWS - 1) / MCE_SLAB_ROWS;
  if (n > MCE_MAX_SLABS) n = MCE_MAX_SLABS;
  return (int)(n < 1 ? 1 : n);
}

}  // namespace

extern "C" {

int ia_mce_backup(const double* T, const float* reward, int S, int A, int H, double discount, double* V, double* Q,
                  double* pi, void* stream) {
  if (S <= 0 || A <= 0 || H <= 0 || T == nullptr || reward == nullptr || V == nullptr || Q == nullptr || pi == nullptr)
    return IA_ERR_ARG;
  if (A > MCE_MAX_A) return IA_ERR_UNSUPPORTED;
  const dim3 grid(cdiv(S, MCE_WAVES)), block(MCE_THREADS);
  const size_t lds = sizeof(double) * MCE_WAVES * (size_t)A;
  const bool vec2 = (S % 2 == 0) && (((uintptr_t)T | (uintptr_t)V) % 16 == 0);
  const long long SA = (long long)S * A;
  for (int t = H - 1; t >= 0; --t) {
    const double* vnext = t == H - 1 ? nullptr : V + (long long)(t + 1) * S;
    if (vec2)
      hipLaunchKernelGGL(mce_backup_kernel<true>, grid, block, lds, (hipStream_t)stream, T, reward, S, A, discount, vnext,
                         V + (long long)t * S, Q + t * SA, pi + t * SA);
    else
      hipLaunchKernelGGL(mce_backup_kernel<false>, grid, block, lds, (hipStream_t)stream, T, reward, S, A, discount,
                         vnext, V + (long long)t * S, Q + t * SA, pi + t * SA);
    IA_CHECK_LAUNCH();
  }
  return IA_OK;
}

int64_t ia_mce_forward_ws_doubles(int S, int A) {
  if (S <= 0 || A <= 0) return 0;
  return (int64_t)forward_slabs(S, A) * S;
}

int ia_mce_forward(const double* T, const double* pi, const double* init, int S, int A, int H, double discount,
                   double* D, double* Dcum, double* ws, void* stream) {
  if (S <= 0 || A <= 0 || H <= 0 || T == nullptr || pi == nullptr || init == nullptr || D == nullptr ||
      Dcum == nullptr || ws == nullptr)
    return IA_ERR_ARG;
  const hipStream_t st = (hipStream_t)stream;
  const int n_slabs = forward_slabs(S, A);
  const int rows_per_slab = cdiv((long long)S * A, n_slabs);
  const int sb = cdiv(S, MCE_THREADS);
  hipLaunchKernelGGL(mce_copy_f64_kernel, dim3(sb), dim3(MCE_THREADS), 0, st, init, S, D);
  IA_CHECK_LAUNCH();
  for (int t = 0; t < H; ++t) {
    hipLaunchKernelGGL(mce_forward_slab_kernel, dim3(sb, n_slabs), dim3(MCE_THREADS), 0, st, T,
                       pi + (long long)t * S * A, D + (long long)t * S, S, A, rows_per_slab, ws);
    IA_CHECK_LAUNCH();
    hipLaunchKernelGGL(mce_forward_sum_kernel, dim3(sb), dim3(MCE_THREADS), 0, st, ws, n_slabs, S,
                       D + (long long)(t + 1) * S);
    IA_CHECK_LAUNCH();
  }
  hipLaunchKernelGGL(mce_discounted_sum_kernel, dim3(sb), dim3(MCE_THREADS), 0, st, D, H + 1, S, discount, Dcum);
  IA_CHECK_LAUNCH();
  return IA_OK;
}

int ia_mce_weights(const double* Dcum, const double* demo_om, int S, float* w, double* stats, void* stream) {
  if (S <= 0 || Dcum == nullptr || demo_om == nullptr || w == nullptr || stats == nullptr) return IA_ERR_ARG;
  hipLaunchKernelGGL(mce_weights_kernel, dim3(1), dim3(MCE_THREADS), 0, (hipStream_t)stream, Dcum, demo_om, S, w, stats);
  IA_CHECK_LAUNCH();
  return IA_OK;
}

int ia_mce_norms(const float* grads, const float* params, int64_t n, double* stats, void* stream) {
  if (n <= 0 || grads == nullptr || params == nullptr || stats == nullptr) return IA_ERR_ARG;
  hipLaunchKernelGGL(mce_norms_kernel, dim3(1), dim3(MCE_THREADS), 0, (hipStream_t)stream, grads, params, (long long)n,
                     stats);
  IA_CHECK_LAUNCH();
  return IA_OK;
}

}  // extern "C"
