// Adversarial imitation from pixels with an off-policy learner (GAIL over DQN("CnnPolicy")): the frame path. Frames stay
// uint8 from the environment to the reward CNN's input; csrc/offpolicy.hip is the float32-row sibling.
//   * ia_offpolicy_frames_step:   one launch per environment step. The step's n transitions are read ONCE from a pinned host
//     record and written to the learner's uint8 ring, to the uint8 round tile and, through the 256-entry byte table, to the
//     reward CNN's channel-last fp32 input X[n, H, W, C * S] (state channels first).
//   * ia_offpolicy_frames_reward: one launch behind the CNN forward: CnnRewardNet's action / done selection of the CNN's
//     output (or a ready reward vector), optionally softplus, to the ring's reward rows and the pinned host reward tile.
//   * ia_disc_gather_frames:      one launch per discriminator minibatch: rows idx_e of the expert table, then rows idx_g
//     of the generator ring -> X[2 mb, H, W, C * S], actions int64 [2 mb], dones fp32 [2 mb].
//   * ia_gather_frame_rows:       device-to-device copy of uint8 transition rows by an int64 order vector into a ring,
//     wrapping at its capacity (the round tile -> the trainer's generator ring).
// Copies follow csrc/dqn_frames.hip: grid (row, 4 KB chunk), 16-byte words where source and every destination of the row
// are 16-byte aligned, else 4-byte words, else bytes. Plain vector stores only, no atomics, nothing polls host memory.
#include "common.h"
#include "../../include/imitation_hip.h"

namespace {

constexpr int FR_THREADS = 256;
constexpr int FR_CHUNK = FR_THREADS * 16;   // bytes of a row per workgroup

typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));

inline long long cdivl(long long a, long long b) { return (a + b - 1) / b; }

// bytes [0, len) of src to up to two destinations (b may be NULL); returns nothing, every lane of the workgroup takes part
__device__ __forceinline__ void copy_chunk(const uint8_t* __restrict__ src, uint8_t* __restrict__ a, uint8_t* __restrict__ b,
                                           int len) {
  const uintptr_t all = (uintptr_t)src | (uintptr_t)a | (uintptr_t)b;
  int done_bytes = 0;
  if ((all & 15) == 0) {
    const int n16 = len >> 4;
    if ((int)threadIdx.x < n16) {   // (a chunk is at most FR_THREADS words of 16 bytes)
      const u32x4 w = reinterpret_cast<const u32x4*>(src)[threadIdx.x];
      reinterpret_cast<u32x4*>(a)[threadIdx.x] = w;
      if (b != nullptr) reinterpret_cast<u32x4*>(b)[threadIdx.x] = w;
    }
    done_bytes = n16 << 4;
  } else if ((all & 3) == 0) {
    const int n4 = len >> 2;
    for (int i = threadIdx.x; i < n4; i += FR_THREADS) {
      const unsigned int w = reinterpret_cast<const unsigned int*>(src)[i];
      reinterpret_cast<unsigned int*>(a)[i] = w;
      if (b != nullptr) reinterpret_cast<unsigned int*>(b)[i] = w;
    }
    done_bytes = n4 << 2;
  }
  for (int i = done_bytes + threadIdx.x; i < len; i += FR_THREADS) {
    const uint8_t w = src[i];
    a[i] = w;
    if (b != nullptr) b[i] = w;
  }
}

// ---- step store --------------------------------------------------------------------------------------------------------
struct StepFrames {
  const uint8_t *obs, *next_obs; const int64_t* act; const uint8_t* dones; const float* ring_done;
  int n, C, HW, use_state, use_next_state;
  const float* lut; float* X;
  uint8_t *ring_obs, *ring_next; int64_t* ring_act; float* ring_done_out; long long ring_row;
  uint8_t *tile_obs, *tile_next; int64_t* tile_act; uint8_t* tile_dones; long long tile_row;
};

__global__ __launch_bounds__(FR_THREADS) void offpolicy_frames_step_kernel(const StepFrames g) {
  __shared__ __attribute__((aligned(16))) uint8_t stage[FR_CHUNK];
  __shared__ float lut[256];
  const int which = blockIdx.x >= (unsigned)g.n;   // 0: obs, 1: next_obs
  const int r = (int)blockIdx.x - which * g.n;
  const long long FB = (long long)g.C * g.HW;
  if (blockIdx.y == 0 && which == 0 && threadIdx.x == 0) {
    const int64_t a = g.act[r];
    g.ring_act[g.ring_row + r] = a;
    g.ring_done_out[g.ring_row + r] = g.ring_done[r];
    g.tile_act[g.tile_row + r] = a;
    g.tile_dones[g.tile_row + r] = g.dones[r];
  }
  const long long lo = (long long)blockIdx.y * FR_CHUNK;
  const long long left = FB - lo;
  if (left <= 0) return;
  const int len = left < FR_CHUNK ? (int)left : FR_CHUNK;
  const bool to_x = g.X != nullptr && (which ? g.use_next_state : g.use_state);
  if (to_x) lut[threadIdx.x] = g.lut[threadIdx.x];
  // the one read of the host record: into LDS, from there to the ring, the tile and X
  const uint8_t* src = (which ? g.next_obs : g.obs) + (long long)r * FB + lo;
  copy_chunk(src, stage, nullptr, len);   // (`stage` is 16-byte aligned: the width follows the host row's alignment)
  __syncthreads();
  uint8_t* ring = (which ? g.ring_next : g.ring_obs) + (g.ring_row + r) * FB + lo;
  uint8_t* tile = (which ? g.tile_next : g.tile_obs) + (g.tile_row + r) * FB + lo;
  copy_chunk(stage, ring, tile, len);
  if (!to_x) return;
  const int S = (g.use_state != 0) + (g.use_next_state != 0);
  const int Cin = g.C * S;
  const int c0 = (which && g.use_state) ? g.C : 0;   // the next state's channels follow the state's
  float* xr = g.X + (long long)r * g.HW * Cin + c0;
  for (int i = threadIdx.x; i < len; i += FR_THREADS) {
    const long long b = lo + i;            // byte (c, p) of the channel-first frame
    const int c = (int)(b / g.HW), p = (int)(b - (long long)c * g.HW);
    xr[(long long)p * Cin + c] = lut[stage[i]];
  }
}

// ---- reward store ------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void offpolicy_frames_reward_kernel(const float* __restrict__ cnn_out, int n_out,
                                                                      const float* __restrict__ rewards_in,
                                                                      const int64_t* __restrict__ act,
                                                                      const uint8_t* __restrict__ dones, int n, int n_actions,
                                                                      int use_action, int use_done, int softplus,
                                                                      float* __restrict__ ring_reward,
                                                                      float* __restrict__ rewards_host) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  float rew;
  if (rewards_in != nullptr) {
    rew = rewards_in[i];
  } else {
    // CnnRewardNet._select: the output entry the one-hot action (and the done flag) selects
    long long j = 0;
    bool ok = true;
    if (use_action) {
      const long long a = act[i];
      ok = a >= 0 && a < n_actions;
      j = a + (use_done && dones[i] ? n_actions : 0);
    } else if (use_done) {
      j = dones[i] ? 1 : 0;
    }
    rew = ok && j < n_out ? cnn_out[(long long)i * n_out + j] : __builtin_nanf("");
    if (softplus) rew = ia_softplus(rew);
  }
  ring_reward[i] = rew;
  if (rewards_host != nullptr) rewards_host[i] = rew;
}

// ---- discriminator minibatch -------------------------------------------------------------------------------------------
// One workgroup per tile = (row r, pixels [p0, p0 + tp)): the tile's S * C runs of tp bytes (one per source frame and
// channel of the channel-first rows) go to LDS, then X's tile, tp * Cin consecutive floats, is written in order.
constexpr int DG_LDS = 16384;
constexpr int DG_TILE_ELEMS = 8192;

struct DiscGather {
  const uint8_t *e_obs, *e_next; const int64_t* e_act; const uint8_t* e_dones; long long e_rows;
  const uint8_t *g_obs, *g_next; const int64_t* g_act; const uint8_t* g_dones; long long g_rows;
  const long long *idx_e, *idx_g;
  int mb, C, HW, use_state, use_next_state, TP, tiles_per_row;
  const float* lut; float* X; int64_t* acts; float* dones;
};

__global__ __launch_bounds__(FR_THREADS) void disc_gather_frames_kernel(const DiscGather g) {
  __shared__ __attribute__((aligned(16))) uint8_t stage[DG_LDS];
  __shared__ float lut[256];
  const int tid = threadIdx.x;
  const int r = blockIdx.x / g.tiles_per_row, tile = blockIdx.x - r * g.tiles_per_row;
  const bool gen = r >= g.mb;
  const long long row = gen ? g.idx_g[r - g.mb] : g.idx_e[r];
  const long long rows = gen ? g.g_rows : g.e_rows;
  const int S = (g.use_state != 0) + (g.use_next_state != 0);
  const int Cin = g.C * S;
  const int p0 = tile * g.TP, tp = min(g.TP, g.HW - p0);
  float* xt = g.X + ((long long)r * g.HW + p0) * Cin;
  const int n_out = tp * Cin;
  if (row < 0 || row >= rows) {   // a row outside its table reads nothing and is loud downstream
    for (int e = tid; e < n_out; e += FR_THREADS) xt[e] = __builtin_nanf("");
    return;
  }
  if (tile == 0 && tid == 0) {
    g.acts[r] = (gen ? g.g_act : g.e_act)[row];
    g.dones[r] = (gen ? g.g_dones : g.e_dones)[row] ? 1.0f : 0.0f;
  }
  lut[tid] = g.lut[tid];
  const long long FB = (long long)g.C * g.HW;
  const uint8_t* s_obs = (gen ? g.g_obs : g.e_obs) + row * FB;
  const uint8_t* s_next = (gen ? g.g_next : g.e_next) + row * FB;
  for (int j = 0; j < Cin; ++j) {   // run j: source frame j / C (state first), channel j % C
    const int s = j / g.C, c = j - s * g.C;
    const uint8_t* src = ((s == 0 && g.use_state) ? s_obs : s_next) + (long long)c * g.HW + p0;
    uint8_t* dst = stage + j * g.TP;   // (TP is a multiple of 16 whenever a row has more than one tile)
    if ((((uintptr_t)src | (uintptr_t)dst) & 3) == 0) {
      const int n4 = tp >> 2;
      for (int i = tid; i < n4; i += FR_THREADS)
        reinterpret_cast<unsigned int*>(dst)[i] = reinterpret_cast<const unsigned int*>(src)[i];
      for (int i = (n4 << 2) + tid; i < tp; i += FR_THREADS) dst[i] = src[i];
    } else {
      for (int i = tid; i < tp; i += FR_THREADS) dst[i] = src[i];
    }
  }
  __syncthreads();
  for (int e = tid; e < n_out; e += FR_THREADS) {
    const int p = e / Cin, ci = e - p * Cin;
    xt[e] = lut[stage[ci * g.TP + p]];
  }
}

// ---- row gather --------------------------------------------------------------------------------------------------------
struct RowGather {
  const uint8_t *src_obs, *src_next; const int64_t* src_act; const uint8_t* src_dones; long long src_rows;
  const long long* order; long long n, FB;
  uint8_t *dst_obs, *dst_next; int64_t* dst_act; uint8_t* dst_dones; long long dst_row, dst_rows;
};

__global__ __launch_bounds__(FR_THREADS) void gather_frame_rows_kernel(const RowGather g) {
  const int which = blockIdx.x >= (unsigned)g.n;   // 0: obs, 1: next_obs
  const long long i = (long long)blockIdx.x - (which ? g.n : 0);
  const long long from = g.order[i];
  if (from < 0 || from >= g.src_rows) return;      // (uniform over the workgroup; the host validates the order)
  const long long to = (g.dst_row + i) % g.dst_rows;
  if (blockIdx.y == 0 && which == 0 && threadIdx.x == 0) {
    g.dst_act[to] = g.src_act[from];
    g.dst_dones[to] = g.src_dones[from];
  }
  const long long lo = (long long)blockIdx.y * FR_CHUNK;
  const long long left = g.FB - lo;
  if (left <= 0) return;
  const int len = left < FR_CHUNK ? (int)left : FR_CHUNK;
  const uint8_t* src = (which ? g.src_next : g.src_obs) + from * g.FB + lo;
  uint8_t* dst = (which ? g.dst_next : g.dst_obs) + to * g.FB + lo;
  copy_chunk(src, dst, nullptr, len);
}

}  // namespace

extern "C" {

int ia_offpolicy_frames_step(const ia_offpolicy_frames_args* a, void* stream) {
  if (a == nullptr || a->n <= 0 || a->C <= 0 || a->H <= 0 || a->W <= 0) return IA_ERR_ARG;
  if (!a->obs || !a->next_obs || !a->act || !a->dones || !a->ring_done) return IA_ERR_ARG;
  if (!a->ring_obs || !a->ring_next_obs || !a->ring_action || !a->ring_done_out) return IA_ERR_ARG;
  if (!a->tile_obs || !a->tile_next_obs || !a->tile_act || !a->tile_dones) return IA_ERR_ARG;
  if (a->ring_row < 0 || a->ring_row + a->n > a->ring_rows || a->tile_row < 0 || a->tile_row + a->n > a->tile_rows)
    return IA_ERR_ARG;
  const int S = (a->use_state != 0) + (a->use_next_state != 0);
  if (a->X != nullptr && (S == 0 || a->lut == nullptr)) return IA_ERR_ARG;
  const long long HW = (long long)a->H * a->W, FB = HW * a->C;
  if (FB * 2 > (1LL << 30)) return IA_ERR_UNSUPPORTED;   // a row's float count stays a 32-bit index
  const long long chunks = cdivl(FB, FR_CHUNK);
  if (chunks > 65535 || a->n > (1 << 30)) return IA_ERR_UNSUPPORTED;
  StepFrames g;
  g.obs = a->obs; g.next_obs = a->next_obs; g.act = a->act; g.dones = a->dones; g.ring_done = a->ring_done;
  g.n = a->n; g.C = a->C; g.HW = (int)HW; g.use_state = a->use_state; g.use_next_state = a->use_next_state;
  g.lut = a->lut; g.X = a->X;
  g.ring_obs = a->ring_obs; g.ring_next = a->ring_next_obs; g.ring_act = a->ring_action; g.ring_done_out = a->ring_done_out;
  g.ring_row = a->ring_row;
  g.tile_obs = a->tile_obs; g.tile_next = a->tile_next_obs; g.tile_act = a->tile_act; g.tile_dones = a->tile_dones;
  g.tile_row = a->tile_row;
  hipLaunchKernelGGL(offpolicy_frames_step_kernel, dim3(2u * (unsigned)a->n, (unsigned)chunks), dim3(FR_THREADS), 0,
                     (hipStream_t)stream, g);
  IA_CHECK_LAUNCH();
  return IA_OK;
}

int ia_offpolicy_frames_reward(const ia_offpolicy_frames_args* a, const float* cnn_out, int n_out, const float* rewards_in,
                               int n_actions, int use_action, int use_done, int softplus, void* stream) {
  if (a == nullptr || a->n <= 0 || !a->ring_reward || !a->tile_act || !a->tile_dones) return IA_ERR_ARG;
  if ((cnn_out == nullptr) == (rewards_in == nullptr)) return IA_ERR_ARG;   // exactly one source
  if (a->ring_row < 0 || a->ring_row + a->n > a->ring_rows || a->tile_row < 0 || a->tile_row + a->n > a->tile_rows)
    return IA_ERR_ARG;
  if (cnn_out != nullptr) {
    const long long want = (long long)(use_action ? n_actions : 1) * (use_done ? 2 : 1);
    if (n_actions < 1 || n_out != want) return IA_ERR_ARG;
  }
  hipLaunchKernelGGL(offpolicy_frames_reward_kernel, dim3((unsigned)cdivl(a->n, 256)), dim3(256), 0, (hipStream_t)stream,
                     cnn_out, n_out, rewards_in, a->tile_act + a->tile_row, a->tile_dones + a->tile_row, a->n, n_actions,
                     use_action, use_done, softplus, a->ring_reward + a->ring_row, a->rewards_host);
  IA_CHECK_LAUNCH();
  return IA_OK;
}

int ia_disc_gather_frames(const uint8_t* e_obs, const uint8_t* e_next_obs, const int64_t* e_act, const uint8_t* e_dones,
                          int64_t e_rows, const uint8_t* g_obs, const uint8_t* g_next_obs, const int64_t* g_act,
                          const uint8_t* g_dones, int64_t g_rows, const int64_t* idx_e, const int64_t* idx_g, int mb, int H,
                          int W, int C, int use_state, int use_next_state, const float* lut, float* X, int64_t* acts,
                          float* dones, void* stream) {
  const int S = (use_state != 0) + (use_next_state != 0);
  if (mb <= 0 || H <= 0 || W <= 0 || C <= 0 || S == 0 || e_rows <= 0 || g_rows <= 0) return IA_ERR_ARG;
  if (!e_obs || !e_next_obs || !e_act || !e_dones || !g_obs || !g_next_obs || !g_act || !g_dones) return IA_ERR_ARG;
  if (!idx_e || !idx_g || !lut || !X || !acts || !dones) return IA_ERR_ARG;
  const long long HW = (long long)H * W;
  const int Cin = C * S;
  if (HW * Cin > (1LL << 30) || Cin > DG_LDS / 16) return IA_ERR_UNSUPPORTED;
  long long TP = (DG_LDS / Cin) & ~15;
  if (TP > (DG_TILE_ELEMS / Cin)) TP = (DG_TILE_ELEMS / Cin) & ~15;
  if (TP < 16) TP = 16;
  if (TP > HW) TP = HW;   // (one tile per row: the runs need no common alignment)
  if (TP * Cin > DG_LDS) return IA_ERR_UNSUPPORTED;
  DiscGather g;
  g.e_obs = e_obs; g.e_next = e_next_obs; g.e_act = e_act; g.e_dones = e_dones; g.e_rows = e_rows;
  g.g_obs = g_obs; g.g_next = g_next_obs; g.g_act = g_act; g.g_dones = g_dones; g.g_rows = g_rows;
  g.idx_e = reinterpret_cast<const long long*>(idx_e); g.idx_g = reinterpret_cast<const long long*>(idx_g);
  g.mb = mb; g.C = C; g.HW = (int)HW; g.use_state = use_state; g.use_next_state = use_next_state;
  g.TP = (int)TP; g.tiles_per_row = (int)cdivl(HW, TP);
  g.lut = lut; g.X = X; g.acts = acts; g.dones = dones;
  const long long grid = 2LL * mb * g.tiles_per_row;
  if (grid > 0x7fffffffLL) return IA_ERR_UNSUPPORTED;
  hipLaunchKernelGGL(disc_gather_frames_kernel, dim3((unsigned)grid), dim3(FR_THREADS), 0, (hipStream_t)stream, g);
  IA_CHECK_LAUNCH();
  return IA_OK;
}

int ia_gather_frame_rows(const uint8_t* src_obs, const uint8_t* src_next_obs, const int64_t* src_act,
                         const uint8_t* src_dones, int64_t src_rows, const int64_t* order, int64_t n, int64_t frame_bytes,
                         uint8_t* dst_obs, uint8_t* dst_next_obs, int64_t* dst_act, uint8_t* dst_dones, int64_t dst_row,
                         int64_t dst_rows, void* stream) {
  if (n <= 0 || frame_bytes < 1 || src_rows <= 0 || dst_rows <= 0 || dst_row < 0 || dst_row >= dst_rows || n > dst_rows)
    return IA_ERR_ARG;
  if (!src_obs || !src_next_obs || !src_act || !src_dones || !order || !dst_obs || !dst_next_obs || !dst_act || !dst_dones)
    return IA_ERR_ARG;
  const long long chunks = cdivl(frame_bytes, FR_CHUNK);
  if (chunks > 65535 || n > (1 << 30)) return IA_ERR_UNSUPPORTED;
  RowGather g;
  g.src_obs = src_obs; g.src_next = src_next_obs; g.src_act = src_act; g.src_dones = src_dones; g.src_rows = src_rows;
  g.order = reinterpret_cast<const long long*>(order); g.n = n; g.FB = frame_bytes;
  g.dst_obs = dst_obs; g.dst_next = dst_next_obs; g.dst_act = dst_act; g.dst_dones = dst_dones; g.dst_row = dst_row;
  g.dst_rows = dst_rows;
  hipLaunchKernelGGL(gather_frame_rows_kernel, dim3(2u * (unsigned)n, (unsigned)chunks), dim3(FR_THREADS), 0,
                     (hipStream_t)stream, g);
  IA_CHECK_LAUNCH();
  return IA_OK;
}

}  // extern "C"
