// Reward regularizers (regularization/regularizers.py, regularization/updaters.py) with lambda resident on the device:
//   A. ia_reg_lp: LpRegularizer._loss_penalty + LossRegularizer.regularize_and_backward -- S = sum |w|^p, the penalty's
//      gradient added to the gradient buffer, regularized_loss into the minibatch's statistics row;
//   B. ia_reg_weight_decay: WeightDecayRegularizer through WeightRegularizer.regularize_and_backward -- w += c w;
//   C. ia_reg_lambda_update: IntervalParamScaler.__call__ on the epoch's summed train / validation losses.
// All three read (C: update) ONE device double, so a training call with a lambda schedule needs no host round trip.
// A and B are one workgroup each: the parameter sets of this path are small (2 k floats for the 32 x 32 BasicRewardNet,
// about 1e5 for CnnRewardNet), one workgroup needs no atomics and has one fixed summation order.
#include <cfloat>
#include <cstdint>

#include "common.h"
#include "../../include/imitation_hip.h"

namespace {

constexpr int REG_THREADS = 512;
constexpr int REG_WAVES = REG_THREADS / 64;

// How a segment (w, g, n) is cut. When w and g are equally aligned modulo 16 bytes: `head` scalar elements up to w's next
// 16-byte boundary (0..3, element i on thread i), `nv` float4s (vector j on thread j % 512, j ascending) and a scalar
// tail (< 4 elements, element k of it on thread k). Otherwise the whole segment is scalar: element i on thread i % 512.
struct SegCut {
  long long head, nv, tail0;   // tail0: index of the first tail element
};

__device__ __forceinline__ SegCut cut_segment(const float* w, const float* g, long long n) {
  SegCut c;
  const uintptr_t aw = reinterpret_cast<uintptr_t>(w), ag = reinterpret_cast<uintptr_t>(g);
  if (g != nullptr && ((aw ^ ag) & 15) != 0) {
    c.head = n;
    c.nv = 0;
    c.tail0 = n;
    return c;
  }
  long long head = (long long)(((16 - (aw & 15)) & 15) >> 2);
  c.head = head < n ? head : n;
  c.nv = (n - c.head) >> 2;
  c.tail0 = c.head + 4 * c.nv;
  return c;
}

// One element of kernel A. a = |w|; q = a^(p-1) as the left-to-right product 1 * a * a ... (p - 2 roundings for p >= 2,
// none for p = 1); the term of S is q * a (one more rounding for p >= 2). The gradient is g + c * (sign(w) * q) with
// c = float(lambda) * p: the sign is exact, the product and the sum round once each (-ffp-contract=off). sign(0) = 0.
__device__ __forceinline__ float lp_elem(float w, float c, int p, float& g) {
  const float a = fabsf(w);
  float q = 1.f;
  for (int k = 1; k < p; ++k) q *= a;
  const float s = (w > 0.f) ? 1.f : ((w < 0.f) ? -1.f : 0.f);
  g = g + c * (s * q);
  return q * a;
}

// Summation order of S: every thread adds its terms into one fp32 accumulator, segment after segment and inside a segment
// head, vectors (components x, y, z, w), tail; the 64 lanes of a wave are combined by a 6-level xor butterfly; thread 0
// adds the 8 waves' sums in wave order. A term passes through at most
//   sum over segments of ((head > 0) + 4 * ceil(nv / 512) + (tail > 0))  [scalar-only segment: ceil(n / 512)]  + 6 + 7
// additions.
__global__ __launch_bounds__(REG_THREADS) void reg_lp_kernel(const ia_reg_segment* __restrict__ segs, int n_segs, int p,
                                                             const double* __restrict__ lambda, float* stats,
                                                             float loss_scale, float* s_out) {
  __shared__ float red[REG_WAVES];
  const int tid = threadIdx.x;
  const float lam = (float)(*lambda);
  const float c = lam * (float)p;
  float acc = 0.f;
  for (int s = 0; s < n_segs; ++s) {
    float* w = segs[s].w;
    float* g = segs[s].g;
    const long long n = segs[s].n;
    const SegCut cut = cut_segment(w, g, n);
    const bool has_g = g != nullptr;   // a null gradient pointer: the segment counts in S only
    for (long long i = tid; i < cut.head; i += REG_THREADS) {
      float b = has_g ? g[i] : 0.f;
      acc += lp_elem(w[i], c, p, b);
      if (has_g) g[i] = b;
    }
    const float4* w4 = reinterpret_cast<const float4*>(w + cut.head);
    float4* g4 = reinterpret_cast<float4*>(g + cut.head);
    for (long long j = tid; j < cut.nv; j += REG_THREADS) {
      const float4 a = w4[j];
      float4 b = has_g ? g4[j] : make_float4(0.f, 0.f, 0.f, 0.f);
      acc += lp_elem(a.x, c, p, b.x);
      acc += lp_elem(a.y, c, p, b.y);
      acc += lp_elem(a.z, c, p, b.z);
      acc += lp_elem(a.w, c, p, b.w);
      if (has_g) g4[j] = b;
    }
    for (long long i = cut.tail0 + tid; i < n; i += REG_THREADS) {
      float b = has_g ? g[i] : 0.f;
      acc += lp_elem(w[i], c, p, b);
      if (has_g) g[i] = b;
    }
  }
  for (int o = 32; o > 0; o >>= 1) acc += __shfl_xor(acc, o, 64);
  if ((tid & 63) == 0) red[tid >> 6] = acc;
  __syncthreads();
  if (tid == 0) {
    float S = 0.f;
    for (int k = 0; k < REG_WAVES; ++k) S += red[k];
    if (s_out != nullptr) *s_out = S;
    // th.add(loss, lambda_ * penalty) on the already scaled loss
    if (stats != nullptr) stats[3] = stats[0] * loss_scale + lam * S;
  }
}

__global__ __launch_bounds__(REG_THREADS) void reg_weight_decay_kernel(const ia_reg_segment* __restrict__ segs, int n_segs,
                                                                       const double* __restrict__ lambda, double lr) {
  const int tid = threadIdx.x;
  const float c = (float)(-(*lambda) * lr);   // formed in double, rounded once
  for (int s = 0; s < n_segs; ++s) {
    float* w = segs[s].w;
    const long long n = segs[s].n;
    const SegCut cut = cut_segment(w, nullptr, n);
    for (long long i = tid; i < cut.head; i += REG_THREADS) w[i] = w[i] + c * w[i];
    float4* w4 = reinterpret_cast<float4*>(w + cut.head);
    for (long long j = tid; j < cut.nv; j += REG_THREADS) {
      float4 a = w4[j];
      a.x = a.x + c * a.x;
      a.y = a.y + c * a.y;
      a.z = a.z + c * a.z;
      a.w = a.w + c * a.w;
      w4[j] = a;
    }
    for (long long i = cut.tail0 + tid; i < n; i += REG_THREADS) w[i] = w[i] + c * w[i];
  }
}

// One thread: the sums are sequential by definition (`train_loss += loss.item()`).
__global__ void reg_lambda_update_kernel(double* lambda, const float* __restrict__ train_stats,
                                         const float* __restrict__ train_scales, int n_train,
                                         const float* __restrict__ val_stats, int n_val, int stride, double scaling,
                                         double lo, double hi, const double* prev_row, double* row) {
  if (threadIdx.x != 0 || blockIdx.x != 0) return;
  double t = 0.0, v = 0.0;
  for (int k = 0; k < n_train; ++k) t += (double)(train_stats[(long long)k * stride] * train_scales[k]);
  for (int k = 0; k < n_val; ++k) v += (double)val_stats[(long long)k * stride];
  double lam = *lambda;
  const double eps = DBL_EPSILON;
  int err = (prev_row != nullptr) ? (int)prev_row[3] : IA_REG_OK;
  if (err == IA_REG_OK) {
    if (eps > fabs(lam)) err = IA_REG_LAMBDA_ZERO;
    else if (lam < 0.0) err = IA_REG_LAMBDA_NEGATIVE;
    else if (t < 0.0 || v < 0.0) err = IA_REG_LOSS_NEGATIVE;
  }
  if (err == IA_REG_OK) {
    if (t < eps && v < eps) {
      // 0 / 0: lambda stays
    } else if (t < eps && eps <= v) {
      lam = lam * (1.0 + scaling);
    } else {
      const double ratio = v / t;
      if (ratio > hi) lam = lam * (1.0 + scaling);
      else if (ratio < lo) lam = lam * (1.0 - scaling);
    }
    *lambda = lam;
  }
  row[0] = lam;
  row[1] = t;
  row[2] = v;
  row[3] = (double)err;
}

int check_segments(const ia_reg_segment* segs, int n_segs, const double* lambda) {
  return (segs == nullptr || n_segs <= 0 || lambda == nullptr) ? IA_ERR_ARG : IA_OK;
}

}  // namespace

extern "C" {

int ia_reg_lp(const ia_reg_segment* segs, int n_segs, int p, const double* lambda, float* stats, float loss_scale,
              float* s_out, void* stream) {
  if (check_segments(segs, n_segs, lambda) != IA_OK || p < 1) return IA_ERR_ARG;
  hipLaunchKernelGGL(reg_lp_kernel, dim3(1), dim3(REG_THREADS), 0, (hipStream_t)stream, segs, n_segs, p, lambda, stats,
                     loss_scale, s_out);
  IA_CHECK_LAUNCH();
  return IA_OK;
}

int ia_reg_weight_decay(const ia_reg_segment* segs, int n_segs, const double* lambda, double lr, void* stream) {
  if (check_segments(segs, n_segs, lambda) != IA_OK) return IA_ERR_ARG;
  hipLaunchKernelGGL(reg_weight_decay_kernel, dim3(1), dim3(REG_THREADS), 0, (hipStream_t)stream, segs, n_segs, lambda,
                     lr);
  IA_CHECK_LAUNCH();
  return IA_OK;
}

int ia_reg_lambda_update(double* lambda, const float* train_stats, const float* train_scales, int n_train,
                         const float* val_stats, int n_val, int stride, double scaling_factor, double lower,
                         double upper, const double* prev_row, double* row, void* stream) {
  if (lambda == nullptr || row == nullptr || n_train < 0 || n_val < 0 || stride < 1) return IA_ERR_ARG;
  if ((n_train > 0 && (train_stats == nullptr || train_scales == nullptr)) || (n_val > 0 && val_stats == nullptr))
    return IA_ERR_ARG;
  hipLaunchKernelGGL(reg_lambda_update_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream, lambda, train_stats,
                     train_scales, n_train, val_stats, n_val, stride, scaling_factor, lower, upper, prev_row, row);
  IA_CHECK_LAUNCH();
  return IA_OK;
}

}  // extern "C"
