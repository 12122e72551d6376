// Definitions shared by the policy kernels (policy.hip) and the DAgger collection step (dagger.hip): the flat
// parameter layout of the fused actor-critic policy, the tanh of the layer chains, the fp32 16x16x4 MFMA wrapper
// and the same-wave LDS hand-off. Everything is internal to the including translation unit (anonymous namespace).
#pragma once
#include "common.h"
#include "../../include/imitation_hip.h"

namespace {

constexpr int MAXD = 64;   // max observation width
constexpr int MAXA = 16;   // max action width / number of discrete actions
constexpr int ROWS = 64;   // rows per block (one wave)
constexpr float LOG_SQRT_2PI = 0.9189385332046727f;  // math.log(math.sqrt(2*math.pi))

struct PolOff {
  int log_std, pW1, pb1, pW2, pb2, vW1, vb1, vW2, vb2, aW, ab, cW, cb, total;
};

__host__ __device__ inline PolOff pol_offsets(int D, int A, int H, int discrete) {
  PolOff o;
  int p = 0;
  o.log_std = discrete ? -1 : 0;
  if (!discrete) p += A;
  o.pW1 = p; p += H * D;
  o.pb1 = p; p += H;
  o.pW2 = p; p += H * H;
  o.pb2 = p; p += H;
  o.vW1 = p; p += H * D;
  o.vb1 = p; p += H;
  o.vW2 = p; p += H * H;
  o.vb2 = p; p += H;
  o.aW = p; p += A * H;
  o.ab = p; p += A;
  o.cW = p; p += H;
  o.cb = p; p += 1;
  o.total = p;
  return o;
}

inline bool pol_ok(const ia_policy_desc* d) {
  return d && d->obs_dim >= 1 && d->obs_dim <= MAXD && d->act_dim >= 1 && d->act_dim <= MAXA &&
         (d->hidden == 32 || d->hidden == 64);
}

// Branch-free tanh: odd polynomial for |x| <= 0.1 (rel. error < 1e-9), 1 - 2/(exp(2|x|)+1) otherwise
// (v_exp_f32 / v_rcp_f32: ~1 ulp each). libm's tanhf costs ~45 instructions and divergent branches.
// Written with explicit fused multiply-adds (the file is built with -ffp-contract=off: as plain expressions the
// polynomial was 3 mul + 3 add, the exponent (|x| + |x|) * log2(e) an add + a mul, 1 - 2 r a mul + a sub -- 16 VALU
// instructions + the two transcendentals per value, 8 values per lane and layer on the PPO chain): 11 + 2. The exponent
// and 1 - 2 r are the same bits as before (scaling by two is exact); the polynomial rounds three times less.
#ifndef IA_TANH_FMA
#define IA_TANH_FMA 1
#endif
__device__ __forceinline__ float fast_tanh(float x) {
  const float ax = fabsf(x);
  const float x2 = x * x;
#if IA_TANH_FMA
  const float poly = x * __builtin_fmaf(x2, __builtin_fmaf(x2, __builtin_fmaf(x2, -0.05396825f, 0.13333334f), -0.33333334f), 1.f);
  const float e = __builtin_amdgcn_exp2f(ax * 2.8853900817779268f);   // = exp2((|x| + |x|) * log2(e)), bit for bit
  const float big = copysignf(__builtin_fmaf(-2.f, __builtin_amdgcn_rcpf(e + 1.f), 1.f), x);
#else
  const float poly = x * (1.f + x2 * (-0.33333334f + x2 * (0.13333334f + x2 * -0.05396825f)));
  const float e = __expf(2.f * ax);
  const float big = copysignf(1.f - 2.f * __builtin_amdgcn_rcpf(e + 1.f), x);
#endif
  return ax <= 0.1f ? poly : big;
}

// fp32 MFMA v_mfma_f32_16x16x4_f32 (lane l: li = l&15, lk = l>>4; A[i=li][k=lk], B[k=lk][j=li], C: col = li,
// rows = 4*lk + reg).
__device__ __forceinline__ f32x4 mfma16(float a, float b, f32x4 c) {
  return __builtin_amdgcn_mfma_f32_16x16x4f32(a, b, c, 0, 0, 0);
}

__device__ __forceinline__ void wave_sync_lds() {
  // same-wave LDS hand-off: DS operations of one wave execute in issue order; this only stops the
  // compiler from moving the reads above the writes
  __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
  __builtin_amdgcn_wave_barrier();
}

}  // namespace
