// mjs_monitor.h — episode statistics on the device: a [T, N] rollout block reduced to finished episodes in a ring of caller-owned
// tensors, and the ring reduced to the numbers a training log shows. A restatement of SB3's Monitor (stable_baselines3/common/monitor.py)
// + ep_info_buffer (deque(maxlen=100)) and of evaluate_policy's per-env episode targets over the blocks mjs_rollout_actor and its
// siblings write; the rules are in include/mjsim.h next to mjs_monitor_update.
//
// The finished episodes of a block are recorded in (t, n) order, whatever the launch geometry:
//   walk_kernel     one LANE per env, sequential in t (row t of a [T, N] field is contiguous over the lanes: coalesced loads): the
//                   env's carried return / length / count advance row by row; an episode that ends on row (t, n) and is within the
//                   env's quota leaves its return and length in the workspace at that row, every other row length 0
//   count_kernel    one workgroup per chunk of CHUNK flattened rows: ballot + popcount per wavefront, summed through LDS -> counts[chunk]
//   scan_kernel     ONE workgroup: exclusive scan of counts in place (tile after tile of its 256 threads with a carry); leaves the cursor
//                   and the block's episode count E in the workspace and writes cursor + E
//   scatter_kernel  one workgroup per chunk: the row's rank inside the chunk again (rpl::wave_rank, wavefront offsets in LDS); episode
//                   e = offsets[chunk] + rank goes to slot (cursor + e) % W iff e >= E - W, so that no two stores target one slot
// mjs_monitor_update is these FOUR launches on the caller's stream; mjs_monitor_summary is ONE (summary_kernel, one workgroup).
// summary_kernel: thread i adds records i, i + 256, ... in that order, then a fixed tree over the 256 partial sums; the mean; a second
// pass of the same shape for sum((x - mean)^2). The order depends on nothing but the record count: reproducible bit for bit.
// No atomics, no inline assembly, plain vector stores; nothing is read back to the host.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/mjsim.h"
#include "mjs_replay.h"  // rpl::wave_rank

namespace mon {

constexpr int THREADS = 256, WAVES = THREADS / 64;
constexpr int CHUNK = THREADS;  // rows per workgroup of count_kernel / scatter_kernel: one per thread

// workspace: [0] the cursor before the block and [1] the block's episode count E (uint64 each), then counts / offsets uint32 [nchunks],
// then the end records: return float64 [T N] (written at end rows only), length int32 [T N] (0: no episode recorded at this row)
constexpr size_t WS_HEADER = 16;
__host__ __device__ constexpr int64_t n_chunks(int64_t rows) { return (rows + CHUNK - 1) / CHUNK; }
__host__ __device__ constexpr size_t ws_offsets_bytes(int64_t rows) { return ((size_t)n_chunks(rows) * sizeof(uint32_t) + 15) / 16 * 16; }
__host__ __device__ constexpr size_t ws_bytes(int64_t rows) {
  return WS_HEADER + ws_offsets_bytes(rows) + (size_t)rows * sizeof(double) + (size_t)rows * sizeof(int32_t);
}

struct UpdateParams {
  int64_t rows;  // T N
  int T, N, same_step, W;
  double* ep_return;
  int32_t* ep_length;
  int64_t* ep_count;
  const int64_t* quota;  // NULL: unlimited
  unsigned long long* cursor;
  double* r_return;
  int32_t* r_length;
  uint8_t *r_success, *r_terminated;
  int32_t* r_env;
  unsigned long long* base;  // workspace: [0] cursor before the block, [1] E
  uint32_t* offsets;         // workspace: counts, then their exclusive scan
  double* end_return;        // workspace
  int32_t* end_length;       // workspace
  const double* reward;
  const uint8_t *terminated, *truncated, *step_type, *is_success;
};

// grid = ceil(N / THREADS)
__global__ __launch_bounds__(THREADS) void walk_kernel(UpdateParams p) {
  const int n = blockIdx.x * THREADS + threadIdx.x;
  if (n >= p.N) return;
  double ret = p.ep_return[n];
  int32_t len = p.ep_length[n];
  int64_t count = p.ep_count[n];
  const int64_t quota = p.quota ? p.quota[n] : INT64_MAX;
  for (int t = 0; t < p.T; t++) {
    const int64_t row = (int64_t)t * p.N + n;
    int32_t end_len = 0;
    if (p.same_step || p.step_type[row] != MJS_STEP_FIRST) {
      ret += p.reward[row];  // one float64 add per counting row, in t order
      len += 1;
      if ((p.terminated[row] | p.truncated[row]) != 0) {
        if (count < quota) {
          end_len = len;  // >= 1
          p.end_return[row] = ret;
          count += 1;
        }
        ret = 0.0;
        len = 0;
      }
    }
    p.end_length[row] = end_len;
  }
  p.ep_return[n] = ret;
  p.ep_length[n] = len;
  p.ep_count[n] = count;
}

__device__ __forceinline__ bool row_ends(const UpdateParams& p, int64_t row) { return row < p.rows && p.end_length[row] != 0; }

// grid = n_chunks(rows)
__global__ __launch_bounds__(THREADS) void count_kernel(UpdateParams p) {
  __shared__ int wave_total[WAVES];
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const int64_t row = (int64_t)blockIdx.x * CHUNK + tid;
  int total;
  (void)rpl::wave_rank(row_ends(p, row), total);
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
__global__ __launch_bounds__(THREADS) void scan_kernel(UpdateParams p) {
  __shared__ uint32_t wave_sum[WAVES];
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const int64_t nchunks = n_chunks(p.rows);
  unsigned long long carry = 0;  // episodes in the tiles before this one (uniform over the workgroup)
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
    if (c < nchunks) p.offsets[c] = (uint32_t)carry + before + incl - v;  // < rows < 2^31
    carry += tile;
    __syncthreads();  // wave_sum is rewritten by the next tile
  }
  if (tid == 0) {
    const unsigned long long count = *p.cursor;
    p.base[0] = count;
    p.base[1] = carry;
    *p.cursor = count + carry;
  }
}

// grid = n_chunks(rows)
__global__ __launch_bounds__(THREADS) void scatter_kernel(UpdateParams p) {
  __shared__ int wave_total[WAVES];
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const int64_t row = (int64_t)blockIdx.x * CHUNK + tid;
  const bool ends = row_ends(p, row);
  int total;
  int rank = rpl::wave_rank(ends, total);
  if (lane == 0) wave_total[wave] = total;
  __syncthreads();
#pragma unroll
  for (int w = 0; w < WAVES; w++)
    if (w < wave) rank += wave_total[w];
  if (!ends) return;
  const unsigned long long E = p.base[1], e = (unsigned long long)p.offsets[blockIdx.x] + (unsigned)rank;
  if (e + (unsigned long long)p.W < E) return;  // not one of the block's last W episodes: a later one takes the slot
  const int64_t slot = (int64_t)((p.base[0] + e) % (unsigned long long)p.W);
  p.r_return[slot] = p.end_return[row];
  p.r_length[slot] = p.end_length[row];
  p.r_success[slot] = p.is_success[row] != 0 ? 1 : 0;
  p.r_terminated[slot] = p.terminated[row] != 0 ? 1 : 0;
  p.r_env[slot] = (int32_t)(row % p.N);
}

struct SummaryParams {
  int W;
  const unsigned long long* cursor;
  const double* r_return;
  const int32_t* r_length;
  const uint8_t* r_success;
  double* out;  // [MJS_MONITOR_SUMMARY]
};

struct Add {
  template <typename V> __device__ V operator()(V a, V b) const { return a + b; }
};
struct Min {
  __device__ double operator()(double a, double b) const { return b < a ? b : a; }
};
struct Max {
  __device__ double operator()(double a, double b) const { return b > a ? b : a; }
};

// the workgroup's 256 values folded by a fixed tree (slot i takes slot i + s, s = 128, 64, ..., 1); every thread gets the result
template <typename V, typename Op>
__device__ __forceinline__ V block_fold(V v, V* lds, Op op, int tid) {
  __syncthreads();  // lds may still be read by the fold before this one
  lds[tid] = v;
  __syncthreads();
#pragma unroll
  for (int s = THREADS / 2; s > 0; s >>= 1) {
    if (tid < s) lds[tid] = op(lds[tid], lds[tid + s]);
    __syncthreads();
  }
  return lds[0];
}

// grid = 1
__global__ __launch_bounds__(THREADS) void summary_kernel(SummaryParams p) {
  __shared__ double lds_f[THREADS];
  __shared__ long long lds_i[THREADS];
  const int tid = threadIdx.x;
  const unsigned long long count = *p.cursor;
  const int K = count < (unsigned long long)p.W ? (int)count : p.W;  // live records: slots 0..K-1 in either case
  double sum = 0.0, lo = INFINITY, hi = -INFINITY;
  long long len = 0, succ = 0;
  for (int i = tid; i < K; i += THREADS) {
    const double x = p.r_return[i];
    sum += x;
    lo = x < lo ? x : lo;
    hi = x > hi ? x : hi;
    len += p.r_length[i];
    succ += p.r_success[i] != 0 ? 1 : 0;
  }
  sum = block_fold(sum, lds_f, Add(), tid);
  lo = block_fold(lo, lds_f, Min(), tid);
  hi = block_fold(hi, lds_f, Max(), tid);
  len = block_fold(len, lds_i, Add(), tid);
  succ = block_fold(succ, lds_i, Add(), tid);
  const double mean = sum / (double)K;
  double ss = 0.0;
  for (int i = tid; i < K; i += THREADS) {
    const double d = p.r_return[i] - mean;
    ss += d * d;
  }
  ss = block_fold(ss, lds_f, Add(), tid);
  if (tid != 0) return;
  const double nan = __builtin_nan("");
  p.out[MJS_MONITOR_COUNT] = (double)K;
  p.out[MJS_MONITOR_RETURN_MEAN] = K ? mean : nan;
  p.out[MJS_MONITOR_RETURN_STD] = K ? sqrt(ss / (double)K) : nan;
  p.out[MJS_MONITOR_LENGTH_MEAN] = K ? (double)len / (double)K : nan;
  p.out[MJS_MONITOR_SUCCESS_RATE] = K ? (double)succ / (double)K : nan;
  p.out[MJS_MONITOR_RETURN_MIN] = K ? lo : nan;
  p.out[MJS_MONITOR_RETURN_MAX] = K ? hi : nan;
  p.out[MJS_MONITOR_RETURN_SUM] = sum;
  p.out[MJS_MONITOR_LENGTH_SUM] = (double)len;
  p.out[MJS_MONITOR_SUCCESS_COUNT] = (double)succ;
}

}  // namespace mon
