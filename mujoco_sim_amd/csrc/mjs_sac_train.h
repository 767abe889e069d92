// mjs_sac_train.h — everything one SAC gradient step consumes, in ONE launch: the batch's ring rows, the gathered transitions and the
// standard-normal draws of both action samples, from a counter-based generator. It replaces torch.randint + mjs_replay_sample + two
// torch.randn (five launches and seven fresh tensors per step) in front of mjs_sac_td_target / mjs_critic_update / mjs_actor_update,
// which mjs_sac_train (mjsim.hip) strings together on the host with no return to the caller.
//
//   draw_batch_kernel   grid = ceil(B / DRAW_ROWS), 256 threads. For batch row b, gradient-step counter `step` and `seed` (both uint64):
//
// Philox4x32-10 (Salmon et al., SC'11) with the standard constants: multipliers M0 = 0xD2511F53, M1 = 0xCD9E8D57, Weyl constants
// W0 = 0x9E3779B9, W1 = 0xBB67AE85; key (seed & 0xffffffff, seed >> 32); counter (b, block, step & 0xffffffff, step >> 32). A round is
//   hi0:lo0 = M0 * c0;  hi1:lo1 = M1 * c2;  c = (hi1 ^ c1 ^ k0, lo1, hi0 ^ c3 ^ k1, lo0)
// and the key is bumped by (W0, W1) before every round but the first. The blocks of a row:
//   block 0      words w0, w1: draw = (((uint64) w0 << 32) | w1) >> 2, a non-negative int64 below 2^62 (the range mjs_replay_sample's
//                draws have); the ring row is draw % size, size = min(*cursor, capacity) read on the device; size == 0: row -1, zero rows
//   block 1, 2   z_next[b, 0..3], z_next[b, 4..7]
//   block 3, 4   z_pi[b, 0..3],   z_pi[b, 4..7]
// Only components < A are written (A <= 8); a block whose four components all lie at or beyond A is not computed. The normals are
// Box-Muller over the word pairs (w0, w1) -> components 0, 1 and (w2, w3) -> components 2, 3 of the block, in float32, one operation per
// line, no contraction, in this order:
//   u1  = (float)((w >> 8) + 1) * 2^-24          in (0, 1]: the logarithm never sees 0 (both factors exact)
//   u2  = (float)(w' >> 8) * 2^-24               in [0, 1)
//   l   = logf(u1);  m = -2 * l;  r = sqrtf(m)
//   ang = TWO_PI * u2                            TWO_PI = 6.283185307179586 rounded to float32
//   pair = (r * cosf(ang), r * sinf(ang))
//
// Thread roles inside a workgroup of DRAW_ROWS = 16 rows: threads 0..15 (wavefront 0) take one row's block 0 each, write indices, draws,
// rewards and dones and leave the ring row in LDS; threads 64..127 (wavefront 1) take one (row, normal block) each; after the barrier all
// 256 threads gather obs / next_obs / actions with consecutive threads on consecutive floats of a row, the shape of rpl::sample_kernel.
// No atomics, no local arrays, no inline assembly, plain vector stores; nothing is read back to the host.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "mjs_replay.h"

namespace sac {

constexpr int THREADS = 256;
constexpr int DRAW_ROWS = 16;    // batch rows per workgroup
constexpr int NORMAL_BLOCKS = 4;  // Philox blocks 1..4 of a row
constexpr int MAX_A = rpl::MAX_A;
static_assert(DRAW_ROWS <= 64 && DRAW_ROWS * NORMAL_BLOCKS == 64 && THREADS >= 128, "the roles of wavefronts 0 and 1");
static_assert(MAX_A == 2 * 4, "two Philox blocks per action sample");

struct DrawParams {
  int B, D, A;
  int64_t capacity;
  const unsigned long long* cursor;
  uint32_t key0, key1, step_lo, step_hi;
  const float *s_obs, *s_next_obs, *s_actions, *s_rewards, *s_dones;
  int64_t *idx_out, *draws_out;  // draws_out may be NULL
  float *obs, *next_obs, *actions, *rewards, *dones;
  float *z_next, *z_pi;  // [B, A]
};

struct Words {
  uint32_t w0, w1, w2, w3;
};

__host__ __device__ inline Words philox4x32_10(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t k0, uint32_t k1) {
#pragma unroll
  for (int round = 0; round < 10; round++) {
    if (round > 0) {
      k0 += 0x9E3779B9u;
      k1 += 0xBB67AE85u;
    }
    const uint64_t p0 = (uint64_t)0xD2511F53u * c0, p1 = (uint64_t)0xCD9E8D57u * c2;
    const uint32_t n0 = (uint32_t)(p1 >> 32) ^ c1 ^ k0, n2 = (uint32_t)(p0 >> 32) ^ c3 ^ k1;
    c1 = (uint32_t)p1;
    c3 = (uint32_t)p0;
    c0 = n0;
    c2 = n2;
  }
  return Words{c0, c1, c2, c3};
}

#pragma clang fp contract(off)
// one Box-Muller pair from two words, by the lines at the top
__device__ __forceinline__ void box_muller(uint32_t w, uint32_t wp, float& first, float& second) {
  const float u1 = (float)((w >> 8) + 1u) * 0x1p-24f;
  const float u2 = (float)(wp >> 8) * 0x1p-24f;
  const float l = logf(u1);
  const float m = -2.0f * l;
  const float r = sqrtf(m);
  const float ang = 6.283185307179586f * u2;
  first = r * cosf(ang);
  second = r * sinf(ang);
}
#pragma clang fp contract(fast)  // back to hipcc's default

// grid = ceil(B / DRAW_ROWS)
__global__ __launch_bounds__(THREADS) void draw_batch_kernel(DrawParams p) {
  __shared__ int64_t idx_s[DRAW_ROWS];
  const int tid = threadIdx.x, b0 = blockIdx.x * DRAW_ROWS;
  const int A = p.A, D = p.D;
  if (tid < DRAW_ROWS) {
    const int b = b0 + tid;
    int64_t idx = -1;
    if (b < p.B) {
      const Words w = philox4x32_10((uint32_t)b, 0u, p.step_lo, p.step_hi, p.key0, p.key1);
      const unsigned long long draw = (((unsigned long long)w.w0 << 32) | w.w1) >> 2;
      const unsigned long long count = *p.cursor;
      const unsigned long long size = count < (unsigned long long)p.capacity ? count : (unsigned long long)p.capacity;
      idx = size ? (int64_t)(draw % size) : -1;
      p.idx_out[b] = idx;
      if (p.draws_out) p.draws_out[b] = (int64_t)draw;
      p.rewards[b] = idx >= 0 ? p.s_rewards[idx] : 0.0f;
      p.dones[b] = idx >= 0 ? p.s_dones[idx] : 0.0f;
    }
    idx_s[tid] = idx;
  } else if (tid >= 64 && tid < 64 + DRAW_ROWS * NORMAL_BLOCKS) {
    const int item = tid - 64, i = item / NORMAL_BLOCKS, k = item - i * NORMAL_BLOCKS;
    const int b = b0 + i, j0 = (k & 1) * 4;  // the block's first component
    if (b < p.B && j0 < A) {
      const Words w = philox4x32_10((uint32_t)b, (uint32_t)(1 + k), p.step_lo, p.step_hi, p.key0, p.key1);
      float n0, n1, n2 = 0.0f, n3 = 0.0f;
      box_muller(w.w0, w.w1, n0, n1);
      if (j0 + 2 < A) box_muller(w.w2, w.w3, n2, n3);
      float* z = (k < 2 ? p.z_next : p.z_pi) + (size_t)b * A;
      z[j0] = n0;
      if (j0 + 1 < A) z[j0 + 1] = n1;
      if (j0 + 2 < A) z[j0 + 2] = n2;
      if (j0 + 3 < A) z[j0 + 3] = n3;
    }
  }
  __syncthreads();
  for (int e = tid; e < DRAW_ROWS * D; e += THREADS) {
    const int i = e / D, j = e - i * D;
    if (b0 + i >= p.B) break;
    const int64_t idx = idx_s[i];
    p.obs[(size_t)(b0 + i) * D + j] = idx >= 0 ? p.s_obs[(size_t)idx * D + j] : 0.0f;
    p.next_obs[(size_t)(b0 + i) * D + j] = idx >= 0 ? p.s_next_obs[(size_t)idx * D + j] : 0.0f;
  }
  for (int e = tid; e < DRAW_ROWS * A; e += THREADS) {
    const int i = e / A, j = e - i * A;
    if (b0 + i >= p.B) break;
    const int64_t idx = idx_s[i];
    p.actions[(size_t)(b0 + i) * A + j] = idx >= 0 ? p.s_actions[(size_t)idx * A + j] : 0.0f;
  }
}

}  // namespace sac
