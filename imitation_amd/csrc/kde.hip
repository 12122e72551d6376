// Kernel density estimate of the density baseline (algorithms/density.py:37-413): for every query row x of group g,
//
//   log p(x) = log sum_{i in group g} K_h(|x - y_i|) - log N_g + c(h, d, kernel)
//
// = sklearn.neighbors.KernelDensity(kernel, bandwidth=h).score_samples with the Euclidean metric, evaluated as one
// all-pairs product X.Y^T (v_mfma_f32_16x16x4_f32: exact fp32, the f32 VALU's rate) with an online log-sum-exp epilogue.
//
// * Standardisation prologue: a workgroup reads its query rows in the caller's order (through `perm`), standardises them
//   as sklearn's StandardScaler.transform does on float32 rows -- (x - mean) and then / scale, each in double and
//   rounded to float32 -- and keeps the tile resident in LDS together with its squared norms.
// * Demo rows (standardised once on the host, fp32, row stride ldy) are streamed in blocks of 64 rows and K chunks of
//   64 columns through LDS, shared by the workgroup's waves; wave w owns query rows 16w .. 16w+15 and computes four
//   16 x 16 (demo x query) tiles per k-step, so each lane holds one query column and 16 demo rows of a block.
// * dist^2 = max(0, |x|^2 + |y|^2 - 2 x.y); the per-pair log kernel is evaluated in log2 units and folded into a per-lane
//   running (max, sum), the max guarded at -inf (a compact kernel with nothing in reach leaves (-inf, 0), never NaN).
//   No deferred-max shortcut: one rescale per lane per 64-row block (16 pairs) is all the online form costs here.
// * Determinism: group g's demo rows are cut into ia_kde_slabs(N_g, d) slabs whose size depends on N_g alone; grid.y is
//   the slab, a workgroup writes one (max, sum) per query row per slab, and the merge kernel combines them in slab
//   order. Nothing a row computes depends on the other rows of its batch or on its position: a row scored alone, in a
//   batch of 16 384 or shuffled gives the same bits.
#include "common.h"

#include <math.h>

namespace {

enum { KDE_GAUSSIAN = 0, KDE_TOPHAT = 1, KDE_EPANECHNIKOV = 2, KDE_EXPONENTIAL = 3, KDE_LINEAR = 4, KDE_COSINE = 5 };

constexpr int KDE_BLOCK = 64;              // demo rows per LDS block (four 16-row MFMA tiles)
constexpr int KDE_KC = 64;                 // K columns per LDS chunk
constexpr int KDE_LDY = KDE_KC + 4;        // LDS row stride (== 4 mod 64 banks: lanes (r, g) read bank 4r + g)
constexpr int KDE_SLAB_TARGET = 1024;      // demo rows per slab aimed at ...
constexpr int KDE_MAX_SLABS = 64;          // ... with at most this many slabs per group
constexpr int KDE_LDS_MAX = 160 * 1024;

__host__ __device__ inline int kde_dp4(int d) { return (d + 3) & ~3; }
__host__ __device__ inline int kde_ldq(int d) { return ((kde_dp4(d) + 63) & ~63) + 4; }

// demo rows per slab of a group of n rows: a function of n only (the determinism rule), a multiple of the block
__host__ __device__ inline int64_t kde_slab_rows(int64_t n) {
  int64_t s = (n + KDE_SLAB_TARGET - 1) / KDE_SLAB_TARGET;
  if (s > KDE_MAX_SLABS) s = KDE_MAX_SLABS;
  if (s < 1) s = 1;
  const int64_t per = (n + s - 1) / s;
  return (per + KDE_BLOCK - 1) / KDE_BLOCK * KDE_BLOCK;
}

inline int kde_tile_rows(int d) {
  const int ldq = kde_ldq(d);
  if (64 * ldq <= 16384) return 64;
  if (32 * ldq <= 16384) return 32;
  return 16;
}

inline size_t kde_lds_bytes(int d, int qt) {
  return sizeof(float) * ((size_t)qt * kde_ldq(d) + (size_t)KDE_BLOCK * KDE_LDY + KDE_BLOCK + qt);
}

struct KdeArgs {
  const float* Y;          // [*, ldy] standardised demo rows, groups contiguous
  const float* ynorm;      // [*] their squared norms
  const int64_t* demo_off; // [G] first row of group g in Y
  const int* demo_n;       // [G] rows of group g
  const float* Q;          // [n_q, d] raw query rows, caller's order
  const double* mean;      // [d]
  const double* scale;     // [d]
  const int* perm;         // [n_q] sorted position -> caller's row (null: identity)
  const int* tiles;        // [n_tiles][3] (first sorted row, rows, group)
  float2* partials;        // [max_slabs][n_q] (max, sum) in log2 units
  int d, ldy, n_q, qt;
  float a, h2, inv_h, c_cos;   // kernel constants (see kde_log2k)
};

// log2 of the unnormalised kernel at squared distance d2 (sklearn's log_*_kernel / ln 2)
template <int KER>
__device__ __forceinline__ float kde_log2k(float d2, const KdeArgs& p) {
  const float NEG_INF = -__builtin_inff();
  if (KER == KDE_GAUSSIAN) return d2 * p.a;                             // a = -log2(e) / (2 h^2)
  if (KER == KDE_EXPONENTIAL) return sqrtf(d2) * p.a;                   // a = -log2(e) / h
  if (!(d2 < p.h2)) return NEG_INF;                                     // compact support: dist < h
  if (KER == KDE_TOPHAT) return 0.0f;
  if (KER == KDE_EPANECHNIKOV) return log2f(1.0f - d2 * p.a);           // a = 1 / h^2
  if (KER == KDE_LINEAR) return log2f(1.0f - sqrtf(d2) * p.inv_h);
  return log2f(cosf(sqrtf(d2) * p.c_cos));                              // cosine: c_cos = pi / (2 h)
}

// (m1, s1) <- (m1, s1) (+) (m2, s2); an all -inf pair keeps the sum at 0
__device__ __forceinline__ void kde_merge(float& m1, float& s1, float m2, float s2) {
  const float m = fmaxf(m1, m2);
  const float base = (m == -__builtin_inff()) ? 0.0f : m;
  s1 = s1 * exp2f(m1 - base) + s2 * exp2f(m2 - base);
  m1 = m;
}

template <int KER>
__global__ void kde_slab_kernel(KdeArgs p) {
  extern __shared__ float lds[];
  const int ldq = kde_ldq(p.d), dp4 = kde_dp4(p.d);
  float* Qs = lds;                                   // [qt][ldq]
  float* Ys = Qs + (size_t)p.qt * ldq;               // [64][KDE_LDY]
  float* yn = Ys + KDE_BLOCK * KDE_LDY;              // [64]
  float* qn = yn + KDE_BLOCK;                        // [qt]

  const int* tile = p.tiles + 3 * blockIdx.x;
  const int q0 = tile[0], qcount = tile[1], g = tile[2];
  const int64_t n_g = p.demo_n[g];
  const int64_t srows = kde_slab_rows(n_g);
  const int64_t lo = (int64_t)blockIdx.y * srows;
  if (lo >= n_g) return;                             // (grid.y covers the group with the most slabs)
  const int64_t hi = lo + srows < n_g ? lo + srows : n_g;
  const float* Yg = p.Y + p.demo_off[g] * (int64_t)p.ldy;
  const float* ynorm_g = p.ynorm + p.demo_off[g];

  const int tid = threadIdx.x, nthr = blockDim.x;
  // ---- prologue: the standardised query tile and its squared norms
  for (int e = tid; e < p.qt * dp4; e += nthr) {
    const int r = e / dp4, k = e - r * dp4;
    float v = 0.0f;
    if (r < qcount && k < p.d) {
      const int row = p.perm ? p.perm[q0 + r] : q0 + r;
      v = (float)((double)p.Q[(int64_t)row * p.d + k] - p.mean[k]);
      v = (float)((double)v / p.scale[k]);
    }
    Qs[r * ldq + k] = v;
  }
  __syncthreads();
  for (int r = tid; r < p.qt; r += nthr) {
    double s = 0.0;
    for (int k = 0; k < p.d; ++k) {
      const double v = Qs[r * ldq + k];
      s += v * v;
    }
    qn[r] = (float)s;
  }

  const int lane = tid & 63, w = tid >> 6;
  const int lr = lane & 15, lg = lane >> 4;
  const bool active = 16 * w < qcount;
  const float* qrow = Qs + (16 * w + lr) * ldq + lg;
  float m = -__builtin_inff(), s = 0.0f;
  float qnorm = 0.0f;

  for (int64_t b0 = lo; b0 < hi; b0 += KDE_BLOCK) {
    // x.y per K chunk of 64 columns, the chunks' sums added in order: the partial sums of one long fp32 chain grow to
    // |x||y| and round at its ulp every step (a 752-wide dot of standardised rows was 2e-3 off in dist^2 as one chain)
    f32x4 acc[4];
#pragma unroll
    for (int t = 0; t < 4; ++t) acc[t] = f32x4{0.0f, 0.0f, 0.0f, 0.0f};
    for (int c0 = 0; c0 < dp4; c0 += KDE_KC) {
      const int kc = dp4 - c0 < KDE_KC ? dp4 - c0 : KDE_KC;
      __syncthreads();   // (every wave is done with the previous chunk and block)
      for (int e = tid; e < KDE_BLOCK * kc; e += nthr) {
        const int r = e / kc, k = e - r * kc;
        const int64_t row = b0 + r;
        Ys[r * KDE_LDY + k] = (row < hi && c0 + k < p.d) ? Yg[row * p.ldy + c0 + k] : 0.0f;
      }
      if (c0 == 0 && tid < KDE_BLOCK) yn[tid] = (b0 + tid < hi) ? ynorm_g[b0 + tid] : __builtin_inff();
      __syncthreads();
      if (active) {
        const float* yrow = Ys + lr * KDE_LDY + lg;
        f32x4 part[4];
#pragma unroll
        for (int t = 0; t < 4; ++t) part[t] = f32x4{0.0f, 0.0f, 0.0f, 0.0f};
        for (int ks = 0; ks < kc; ks += 4) {
          const float bq = qrow[c0 + ks];
#pragma unroll
          for (int t = 0; t < 4; ++t)
            part[t] = __builtin_amdgcn_mfma_f32_16x16x4f32(yrow[16 * t * KDE_LDY + ks], bq, part[t], 0, 0, 0);
        }
#pragma unroll
        for (int t = 0; t < 4; ++t) acc[t] = c0 == 0 ? part[t] : acc[t] + part[t];
      }
    }
    if (!active) continue;
    if (b0 == lo) qnorm = qn[16 * w + lr];
    // lane holds query column lr and demo rows 16t + 4lg + i of the block
    float lk[16];
    float bm = -__builtin_inff();
#pragma unroll
    for (int t = 0; t < 4; ++t) {
      const float4 y4 = *reinterpret_cast<const float4*>(yn + 16 * t + 4 * lg);
      const float yv[4] = {y4.x, y4.y, y4.z, y4.w};
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const float d2 = fmaxf(0.0f, fmaf(-2.0f, acc[t][i], qnorm + yv[i]));
        lk[4 * t + i] = kde_log2k<KER>(d2, p);
        bm = fmaxf(bm, lk[4 * t + i]);
      }
    }
    const float mn = fmaxf(m, bm);
    const float base = (mn == -__builtin_inff()) ? 0.0f : mn;
    float add = 0.0f;
#pragma unroll
    for (int i = 0; i < 16; ++i) add += exp2f(lk[i] - base);
    s = s * exp2f(m - base) + add;
    m = mn;
  }
  if (!active) return;
  // the four lane groups of a query column, in a fixed order (both partners compute the same sum)
  kde_merge(m, s, __shfl_xor(m, 16), __shfl_xor(s, 16));
  kde_merge(m, s, __shfl_xor(m, 32), __shfl_xor(s, 32));
  const int r = 16 * w + lr;
  if (lg == 0 && r < qcount) p.partials[(int64_t)blockIdx.y * p.n_q + q0 + r] = make_float2(m, s);
}

// one workgroup per query tile: the slabs' partials merged in slab order, scattered to the caller's row order
__global__ void kde_merge_kernel(const float2* partials, const int* tiles, const int* demo_n, const double* gconst,
                                 const int* perm, int n_q, float* out) {
  const int* tile = tiles + 3 * blockIdx.x;
  const int q0 = tile[0], qcount = tile[1], g = tile[2];
  const int64_t n_g = demo_n[g];
  const int64_t srows = kde_slab_rows(n_g);
  const int n_slabs = (int)((n_g + srows - 1) / srows);
  for (int r = threadIdx.x; r < qcount; r += blockDim.x) {
    const int q = q0 + r;
    float m = -__builtin_inff(), s = 0.0f;
    for (int k = 0; k < n_slabs; ++k) {
      const float2 v = partials[(int64_t)k * n_q + q];
      kde_merge(m, s, v.x, v.y);
    }
    const double l2 = (s > 0.0f) ? (double)m + log2((double)s) : -__builtin_inf();
    out[perm ? perm[q] : q] = (float)(l2 * 0.69314718055994530942 + gconst[g]);
  }
}

}  // namespace

extern "C" {

int ia_kde_tile_rows(int d) {
  if (d < 1) return IA_ERR_ARG;
  return kde_lds_bytes(d, kde_tile_rows(d)) <= (size_t)KDE_LDS_MAX ? kde_tile_rows(d) : IA_ERR_UNSUPPORTED;
}

int ia_kde_slabs(int64_t n_demo, int d) {
  if (n_demo < 1 || d < 1) return IA_ERR_ARG;
  const int64_t sr = kde_slab_rows(n_demo);
  return (int)((n_demo + sr - 1) / sr);
}

int ia_kde_log_density(int kernel, double h, int d, const float* Y, int ldy, const float* ynorm, const int64_t* demo_off,
                       const int* demo_n, const double* gconst, int max_slabs, const float* Q, int n_q, const double* mean,
                       const double* scale, const int* perm, const int* tiles, int n_tiles, float* partials, float* out,
                       int stages, void* stream) {
  if (kernel < KDE_GAUSSIAN || kernel > KDE_COSINE || !(h > 0.0) || !(h < __builtin_inf()) || d < 1 || ldy < d ||
      n_q < 0 || n_tiles < 0 || max_slabs < 1 || max_slabs > KDE_MAX_SLABS || stages < 1 || stages > 3)
    return IA_ERR_ARG;
  if (n_q == 0 || n_tiles == 0) return IA_OK;
  if (!Y || !ynorm || !demo_off || !demo_n || !gconst || !Q || !mean || !scale || !tiles || !partials || !out)
    return IA_ERR_ARG;
  const int qt = kde_tile_rows(d);
  const size_t lds = kde_lds_bytes(d, qt);
  if (lds > (size_t)KDE_LDS_MAX) return IA_ERR_UNSUPPORTED;
  hipStream_t st = (hipStream_t)stream;
  if (stages & 1) {
    KdeArgs a{};
    a.Y = Y; a.ynorm = ynorm; a.demo_off = demo_off; a.demo_n = demo_n; a.Q = Q; a.mean = mean; a.scale = scale;
    a.perm = perm; a.tiles = tiles; a.partials = reinterpret_cast<float2*>(partials);
    a.d = d; a.ldy = ldy; a.n_q = n_q; a.qt = qt;
    const double log2e = 1.4426950408889634074;
    a.h2 = (float)(h * h);
    a.inv_h = (float)(1.0 / h);
    a.c_cos = (float)(1.5707963267948966192 / h);
    a.a = kernel == KDE_GAUSSIAN ? (float)(-0.5 * log2e / (h * h))
        : kernel == KDE_EXPONENTIAL ? (float)(-log2e / h)
        : kernel == KDE_EPANECHNIKOV ? (float)(1.0 / (h * h)) : 0.0f;
    void (*fn)(KdeArgs) = kernel == KDE_GAUSSIAN ? kde_slab_kernel<KDE_GAUSSIAN>
                        : kernel == KDE_TOPHAT ? kde_slab_kernel<KDE_TOPHAT>
                        : kernel == KDE_EPANECHNIKOV ? kde_slab_kernel<KDE_EPANECHNIKOV>
                        : kernel == KDE_EXPONENTIAL ? kde_slab_kernel<KDE_EXPONENTIAL>
                        : kernel == KDE_LINEAR ? kde_slab_kernel<KDE_LINEAR> : kde_slab_kernel<KDE_COSINE>;
    if (lds > 64 * 1024 &&
        hipFuncSetAttribute(reinterpret_cast<const void*>(fn), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds) !=
            hipSuccess)
      return IA_ERR_UNSUPPORTED;
    hipLaunchKernelGGL(fn, dim3(n_tiles, max_slabs), dim3(4 * qt), lds, st, a);
    IA_CHECK_LAUNCH();
  }
  if (stages & 2) {
    hipLaunchKernelGGL(kde_merge_kernel, dim3(n_tiles), dim3(64), 0, st, reinterpret_cast<const float2*>(partials),
                       tiles, demo_n, gconst, perm, n_q, out);
    IA_CHECK_LAUNCH();
  }
  return IA_OK;
}

}  // extern "C"
