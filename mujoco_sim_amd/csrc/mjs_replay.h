// mjs_replay.h — a replay buffer on the device: a [T, N] rollout block to SAC transitions in a ring of caller-owned tensors, and
// batches gathered from it. A restatement of SB3's ReplayBuffer.add / sample (stable_baselines3/common/buffers.py) over the blocks
// mjs_rollout_actor / mjs_rollout_visual_actor write; the rules are in include/mjsim.h next to mjs_replay_add.
//
// The valid rows of a block are appended in (t, n) order, whatever the launch geometry: the flattened rows are cut into chunks of
// CHUNK, and a row's ring position is cursor + (valid rows in the chunks before its own) + (valid rows before it in its chunk).
//   count_kernel    one workgroup per chunk: ballot + popcount per wavefront, summed through LDS -> counts[chunk]
//   scan_kernel     ONE workgroup: exclusive scan of counts in place, tile after tile of its 256 threads with a carry; reads the
//                   cursor, leaves it in the workspace as the block's base and writes cursor + total
//   scatter_kernel  one workgroup per chunk: the row's rank inside the chunk again (ballot + mbcnt, wavefront offsets in LDS),
//                   dest[row] = ring row or -1 to the workspace; then the chunk's obs / next_obs / action elements with
//                   consecutive threads on consecutive floats of the destination rows, and reward / done / timeout per row
//   image_kernel    one workgroup per source row that has a ring row: one H W 3-byte frame per camera to rgb, the next to next_rgb
//   sample_kernel / sample_image_kernel   the gather of B rows, same shapes
// A frame is copied in 16-byte pieces when its size and both addresses allow it, in 4-byte pieces when those allow that, in bytes
// otherwise (37 x 41 x 3 = 4551 bytes: every row after the first is misaligned).
// No atomics, no inline assembly, plain vector stores; nothing is read back to the host.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/mjsim.h"

namespace rpl {

constexpr int THREADS = 256, WAVES = THREADS / 64;
constexpr int CHUNK = THREADS;   // rows per workgroup of count_kernel / scatter_kernel: one per thread
constexpr int MAX_D = MJS_REPLAY_MAX_OBS, MAX_A = 8, MAX_CAM = MJS_REPLAY_MAX_CAMERAS;
constexpr int SAMPLE_ROWS = 16;  // batch rows per workgroup of sample_kernel

// workspace: [0] the block's base (the cursor before the block), then counts / offsets uint32 [nchunks], then dest int32 [T N]
constexpr size_t WS_HEADER = 16;
__host__ __device__ constexpr int64_t n_chunks(int64_t rows) { return (rows + CHUNK - 1) / CHUNK; }
__host__ __device__ constexpr size_t ws_offsets_bytes(int64_t rows) { return ((size_t)n_chunks(rows) * sizeof(uint32_t) + 15) / 16 * 16; }
__host__ __device__ constexpr size_t ws_bytes(int64_t rows) { return WS_HEADER + ws_offsets_bytes(rows) + (size_t)rows * sizeof(int32_t); }

struct ObsIndex {
  int32_t v[MAX_D];
};

struct AddParams {
  int64_t rows;       // T N
  int T, N, src_dim, same_step;
  int D, A, n_cam;
  int64_t capacity;
  uint64_t frame_bytes;  // H W 3
  unsigned long long* cursor;
  unsigned long long* base;  // workspace
  uint32_t* offsets;         // workspace: counts, then their exclusive scan
  int32_t* dest;             // workspace
  const double *obs0, *obs, *terminal_obs, *reward;
  const uint8_t *terminated, *truncated, *step_type;
  const float* squashed;
  const uint8_t *rgb[MAX_CAM], *final_rgb[MAX_CAM];
  float *s_obs, *s_next_obs, *s_actions, *s_rewards, *s_dones;
  uint8_t* s_timeouts;
  uint8_t *s_rgb[MAX_CAM], *s_next_rgb[MAX_CAM];
  ObsIndex index;
};

__device__ __forceinline__ bool row_valid(const AddParams& p, int64_t row) {
  return row < p.rows && (p.same_step || p.step_type[row] != MJS_STEP_FIRST);
}

// the number of `pred` lanes below the calling lane, and in the whole wavefront
__device__ __forceinline__ int wave_rank(bool pred, int& total) {
  const unsigned long long m = __ballot(pred);
  total = __popcll(m);
  return (int)__builtin_amdgcn_mbcnt_hi((uint32_t)(m >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)m, 0u));
}

// grid = n_chunks(rows)
__global__ __launch_bounds__(THREADS) void count_kernel(AddParams p) {
  __shared__ int wave_total[WAVES];
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const int64_t row = (int64_t)blockIdx.x * CHUNK + tid;
  int total;
  (void)wave_rank(row_valid(p, row), total);
  if (lane == 0) wave_total[wave] = total;
  __syncthreads();
  if (tid == 0) {
    int s = 0;
#pragma unroll
    for (int w = 0; w < WAVES; w++) s += wave_total[w];
    p.offsets[blockIdx.x] = (uint32_t)s;
  }
}

// grid = 1
__global__ __launch_bounds__(THREADS) void scan_kernel(AddParams p) {
  __shared__ uint32_t wave_sum[WAVES];
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const int64_t nchunks = n_chunks(p.rows);
  unsigned long long carry = 0;  // valid rows in the tiles before this one (uniform over the workgroup)
  for (int64_t c0 = 0; c0 < nchunks; c0 += THREADS) {
    const int64_t c = c0 + tid;
    const uint32_t v = c < nchunks ? p.offsets[c] : 0u;
    uint32_t incl = v;  // inclusive scan over the wavefront
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
      const uint32_t up = __shfl_up(incl, d, 64);
      if (lane >= d) incl += up;
    }
    if (lane == 63) wave_sum[wave] = incl;
    __syncthreads();
    uint32_t before = 0, tile = 0;
#pragma unroll
    for (int w = 0; w < WAVES; w++) {
      if (w < wave) before += wave_sum[w];
      tile += wave_sum[w];
    }
    if (c < nchunks) p.offsets[c] = (uint32_t)carry + before + incl - v;  // < rows <= capacity < 2^31
    carry += tile;
    __syncthreads();  // wave_sum is rewritten by the next tile
  }
  if (tid == 0) {
    const unsigned long long count = *p.cursor;
    *p.base = count;
    *p.cursor = count + carry;
  }
}

// grid = n_chunks(rows)
__global__ __launch_bounds__(THREADS) void scatter_kernel(AddParams p) {
  __shared__ int wave_total[WAVES];
  __shared__ int32_t dest_s[CHUNK];
  __shared__ uint8_t from_terminal[CHUNK];
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const int64_t row0 = (int64_t)blockIdx.x * CHUNK, row = row0 + tid;
  const bool valid = row_valid(p, row);
  int total;
  int rank = wave_rank(valid, total);
  if (lane == 0) wave_total[wave] = total;
  __syncthreads();
#pragma unroll
  for (int w = 0; w < WAVES; w++)
    if (w < wave) rank += wave_total[w];
  int32_t dest = -1;
  bool done = false;  // the episode ended at this step: terminated | truncated
  if (valid) {
    dest = (int32_t)((*p.base + p.offsets[blockIdx.x] + (unsigned)rank) % (unsigned long long)p.capacity);
    const bool term = p.terminated[row] != 0, trunc = p.truncated[row] != 0;
    done = term || trunc;
    p.s_rewards[dest] = (float)p.reward[row];
    p.s_dones[dest] = term ? 1.0f : 0.0f;
    p.s_timeouts[dest] = trunc ? 1 : 0;
  }
  if (row < p.rows) p.dest[row] = dest;
  dest_s[tid] = dest;
  from_terminal[tid] = (uint8_t)(p.same_step && done);  // next_obs of an episode's last step under same-step auto-reset
  __syncthreads();

  const int D = p.D, A = p.A;
  for (int e = tid; e < CHUNK * D; e += THREADS) {
    const int i = e / D, j = e - i * D;
    const int32_t d = dest_s[i];
    if (d < 0) continue;
    const int64_t r = row0 + i;
    const int col = p.index.v[j];
    const double* prev = r < p.N ? p.obs0 + (size_t)r * p.src_dim : p.obs + (size_t)(r - p.N) * p.src_dim;
    const double* next = (from_terminal[i] ? p.terminal_obs : p.obs) + (size_t)r * p.src_dim;
    p.s_obs[(size_t)d * D + j] = (float)prev[col];
    p.s_next_obs[(size_t)d * D + j] = (float)next[col];
  }
  for (int e = tid; e < CHUNK * A; e += THREADS) {
    const int i = e / A, j = e - i * A;
    const int32_t d = dest_s[i];
    if (d < 0) continue;
    p.s_actions[(size_t)d * A + j] = p.squashed[(size_t)(row0 + i) * A + j];
  }
}

// One frame for the calling workgroup; src NULL: zeros. The path is uniform over the workgroup.
__device__ __forceinline__ void copy_frame(uint8_t* __restrict__ dst, const uint8_t* __restrict__ src, uint64_t bytes, int tid) {
  const uint64_t both = (uint64_t)(uintptr_t)dst | (uint64_t)(uintptr_t)src | bytes;  // (a NULL src is aligned to everything)
  if ((both & 15u) == 0) {
    const uint4* s = reinterpret_cast<const uint4*>(src);
    uint4* d = reinterpret_cast<uint4*>(dst);
    for (uint64_t i = tid; i < bytes / 16; i += THREADS) d[i] = src ? s[i] : uint4{0u, 0u, 0u, 0u};
  } else if ((both & 3u) == 0) {
    const uint32_t* s = reinterpret_cast<const uint32_t*>(src);
    uint32_t* d = reinterpret_cast<uint32_t*>(dst);
    for (uint64_t i = tid; i < bytes / 4; i += THREADS) d[i] = src ? s[i] : 0u;
  } else {
    for (uint64_t i = tid; i < bytes; i += THREADS) dst[i] = src ? src[i] : (uint8_t)0;
  }
}

// grid = rows
__global__ __launch_bounds__(THREADS) void image_kernel(AddParams p) {
  const int64_t row = blockIdx.x;
  const int32_t d = p.dest[row];
  if (d < 0) return;  // (uniform over the workgroup)
  const int64_t n = row % p.N;
  const bool last = row + p.N >= p.rows;  // t == T - 1
  for (int c = 0; c < p.n_cam; c++) {
    const uint8_t* frame = p.rgb[c] + (size_t)row * p.frame_bytes;
    const uint8_t* next = last ? p.final_rgb[c] + (size_t)n * p.frame_bytes : frame + (size_t)p.N * p.frame_bytes;
    copy_frame(p.s_rgb[c] + (size_t)d * p.frame_bytes, frame, p.frame_bytes, threadIdx.x);
    copy_frame(p.s_next_rgb[c] + (size_t)d * p.frame_bytes, next, p.frame_bytes, threadIdx.x);
  }
}

struct SampleParams {
  int B, D, A, n_cam;
  int64_t capacity;
  uint64_t frame_bytes;
  const unsigned long long* cursor;
  const int64_t* draws;
  const float *s_obs, *s_next_obs, *s_actions, *s_rewards, *s_dones;
  const uint8_t* s_timeouts;
  const uint8_t *s_rgb[MAX_CAM], *s_next_rgb[MAX_CAM];
  int64_t* idx_out;
  float *obs, *next_obs, *actions, *rewards, *dones;
  uint8_t* timeouts;
  uint8_t *rgb[MAX_CAM], *next_rgb[MAX_CAM];
};

// the ring row of batch row b, -1 while the buffer is empty (the draw is taken as unsigned: the row is in range whatever it holds)
__device__ __forceinline__ int64_t sampled_row(const SampleParams& p, int b) {
  const unsigned long long count = *p.cursor;
  const unsigned long long size = count < (unsigned long long)p.capacity ? count : (unsigned long long)p.capacity;
  return size ? (int64_t)((unsigned long long)p.draws[b] % size) : -1;
}

// grid = ceil(B / SAMPLE_ROWS)
__global__ __launch_bounds__(THREADS) void sample_kernel(SampleParams p) {
  __shared__ int64_t idx_s[SAMPLE_ROWS];
  const int tid = threadIdx.x, b0 = blockIdx.x * SAMPLE_ROWS;
  if (tid < SAMPLE_ROWS) {
    const int b = b0 + tid;
    int64_t idx = -1;
    if (b < p.B) {
      idx = sampled_row(p, b);
      if (p.idx_out) p.idx_out[b] = idx;
      if (p.rewards) p.rewards[b] = idx >= 0 ? p.s_rewards[idx] : 0.0f;
      if (p.dones) p.dones[b] = idx >= 0 ? p.s_dones[idx] : 0.0f;
      if (p.timeouts) p.timeouts[b] = idx >= 0 ? p.s_timeouts[idx] : (uint8_t)0;
    }
    idx_s[tid] = idx;
  }
  __syncthreads();
  const int D = p.D, A = p.A;
  for (int e = tid; e < SAMPLE_ROWS * D; e += THREADS) {
    const int i = e / D, j = e - i * D;
    if (b0 + i >= p.B) break;
    const int64_t idx = idx_s[i];
    if (p.obs) p.obs[(size_t)(b0 + i) * D + j] = idx >= 0 ? p.s_obs[(size_t)idx * D + j] : 0.0f;
    if (p.next_obs) p.next_obs[(size_t)(b0 + i) * D + j] = idx >= 0 ? p.s_next_obs[(size_t)idx * D + j] : 0.0f;
  }
  if (p.actions) {
    for (int e = tid; e < SAMPLE_ROWS * A; e += THREADS) {
      const int i = e / A, j = e - i * A;
      if (b0 + i >= p.B) break;
      const int64_t idx = idx_s[i];
      p.actions[(size_t)(b0 + i) * A + j] = idx >= 0 ? p.s_actions[(size_t)idx * A + j] : 0.0f;
    }
  }
}

// grid = B
__global__ __launch_bounds__(THREADS) void sample_image_kernel(SampleParams p) {
  const int b = blockIdx.x;
  const int64_t idx = sampled_row(p, b);  // (uniform over the workgroup)
  for (int c = 0; c < p.n_cam; c++) {
    if (p.rgb[c]) copy_frame(p.rgb[c] + (size_t)b * p.frame_bytes, idx >= 0 ? p.s_rgb[c] + (size_t)idx * p.frame_bytes : nullptr, p.frame_bytes, threadIdx.x);
    if (p.next_rgb[c])
      copy_frame(p.next_rgb[c] + (size_t)b * p.frame_bytes, idx >= 0 ? p.s_next_rgb[c] + (size_t)idx * p.frame_bytes : nullptr, p.frame_bytes, threadIdx.x);
  }
}

}  // namespace rpl
