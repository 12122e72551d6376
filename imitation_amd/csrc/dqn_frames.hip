// DQN on image observations ([SB3 dqn/dqn.py] DQN.train with a CnnPolicy): the minibatch of one gradient step from the
// two uint8 frame tables (learner ring, expert table) in ONE launch.
//   * ia_dqn_assemble_u8: obs_out / next_out [B, frame_bytes] uint8, act_out int64 [B], rew_out / done_out float [B] of
//     index row idx[B] (rows < n_new index the learner ring, the rest the expert table). Pure data movement, bit-exact.
// Grid: x = 2 B frame rows (obs rows, then next_obs rows), y = the 4 KB chunks of a row -- a batch of 32 frames of
// 4 x 84 x 84 is 64 rows of 28 224 bytes, 448 workgroups of 256 lanes x 16 bytes; a row per workgroup would leave three
// quarters of the 256 compute units idle at that batch. The chunk offset is a multiple of 16, so the widest access a
// workgroup may use follows from the alignment of its source and destination ROW: 16-byte words where both are 16-byte
// aligned, else 4-byte words, else bytes (rows of a table are only frame_bytes-aligned: an odd frame_bytes leaves most
// rows on the byte path); the bytes behind the last whole word go one by one. A row index outside its table writes
// nothing (the host validates the indices; this is the second line).
#include "common.h"
#include "../../include/imitation_hip.h"

namespace {

constexpr int FR_THREADS = 256;
constexpr int FR_CHUNK = FR_THREADS * 16;   // bytes of a row per workgroup

typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));

struct FrameTable {
  const uint8_t* obs;
  const uint8_t* next_obs;
  const int64_t* act;
  const float* rew;
  const float* done;
  long long rows;
};

__global__ __launch_bounds__(FR_THREADS) void dqn_assemble_u8_kernel(FrameTable ring, FrameTable expert,
                                                                      const int64_t* __restrict__ idx, int B, int n_new,
                                                                      long long frame_bytes, uint8_t* __restrict__ obs_out,
                                                                      uint8_t* __restrict__ next_out,
                                                                      int64_t* __restrict__ act_out,
                                                                      float* __restrict__ rew_out,
                                                                      float* __restrict__ done_out) {
  const int which = blockIdx.x >= (unsigned)B;          // 0: obs, 1: next_obs
  const int r = (int)blockIdx.x - which * B;
  const FrameTable& t = r < n_new ? ring : expert;
  const long long row = idx[r];
  if (row < 0 || row >= t.rows) return;                 // (uniform over the workgroup)
  if (blockIdx.y == 0 && which == 0 && threadIdx.x == 0) {
    act_out[r] = t.act[row];
    rew_out[r] = t.rew[row];
    done_out[r] = t.done[row];
  }
  const long long lo = (long long)blockIdx.y * FR_CHUNK;
  const long long left = frame_bytes - lo;
  if (left <= 0) return;
  const int len = left < FR_CHUNK ? (int)left : FR_CHUNK;
  const uint8_t* src = (which ? t.next_obs : t.obs) + row * frame_bytes + lo;
  uint8_t* dst = (which ? next_out : obs_out) + (long long)r * frame_bytes + lo;
  const uintptr_t both = (uintptr_t)src | (uintptr_t)dst;
  int done_bytes = 0;
  if ((both & 15) == 0) {
    const int n16 = len >> 4;
    if ((int)threadIdx.x < n16)   // (a chunk is at most FR_THREADS words of 16 bytes)
      reinterpret_cast<u32x4*>(dst)[threadIdx.x] = reinterpret_cast<const u32x4*>(src)[threadIdx.x];
    done_bytes = n16 << 4;
  } else if ((both & 3) == 0) {
    const int n4 = len >> 2;
    for (int i = threadIdx.x; i < n4; i += FR_THREADS)
      reinterpret_cast<unsigned int*>(dst)[i] = reinterpret_cast<const unsigned int*>(src)[i];
    done_bytes = n4 << 2;
  }
  for (int i = done_bytes + threadIdx.x; i < len; i += FR_THREADS) dst[i] = src[i];
}

}  // namespace

extern "C" {

int ia_dqn_assemble_u8(const uint8_t* ring_obs, const uint8_t* ring_next_obs, const int64_t* ring_act, const float* ring_rew,
                       const float* ring_done, int64_t ring_rows, const uint8_t* exp_obs, const uint8_t* exp_next_obs,
                       const int64_t* exp_act, const float* exp_rew, const float* exp_done, int64_t exp_rows,
                       const int64_t* idx, int B, int n_new, int64_t frame_bytes, uint8_t* obs_out, uint8_t* next_out,
                       int64_t* act_out, float* rew_out, float* done_out, void* stream) {
  if (B <= 0 || n_new < 0 || n_new > B || frame_bytes < 1 || !idx || !obs_out || !next_out || !act_out || !rew_out || !done_out)
    return IA_ERR_ARG;
  if (n_new > 0 && !(ring_obs && ring_next_obs && ring_act && ring_rew && ring_done && ring_rows > 0)) return IA_ERR_ARG;
  if (n_new < B && !(exp_obs && exp_next_obs && exp_act && exp_rew && exp_done && exp_rows > 0)) return IA_ERR_ARG;
  const long long chunks = (frame_bytes + FR_CHUNK - 1) / FR_CHUNK;
  if (chunks > 65535 || B > (1 << 30)) return IA_ERR_UNSUPPORTED;
  FrameTable ring{ring_obs, ring_next_obs, ring_act, ring_rew, ring_done, n_new > 0 ? (long long)ring_rows : 0};
  FrameTable expert{exp_obs, exp_next_obs, exp_act, exp_rew, exp_done, n_new < B ? (long long)exp_rows : 0};
  hipLaunchKernelGGL(dqn_assemble_u8_kernel, dim3(2u * (unsigned)B, (unsigned)chunks), dim3(FR_THREADS), 0,
                     (hipStream_t)stream, ring, expert, idx, B, n_new, (long long)frame_bytes, obs_out, next_out, act_out,
                     rew_out, done_out);
  IA_CHECK_LAUNCH();
  return IA_OK;
}

}  // extern "C"
