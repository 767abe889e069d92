// mjs_actor.h — SAC's MLP actor (a squashed Gaussian, stable_baselines3/sac/policies.py Actor) as ONE launch: flat float64
// observations in, float64 env actions (and the float32 squashed actions a replay buffer stores) out. What the reference's RL scripts
// evaluate once per control step with torch (scripts/sb3/reach_sac.py, planar_push.py, sb3_sac.py: net_arch pi = [64, 64], [32],
// SB3's default [256, 256]).
//
// float32 with float32 accumulation on the f32-input MFMA of gfx950 (exact f32: the result of an output element is an fmaf chain
// over k that starts at the bias). A workgroup owns TE envs (TE = 16: v_mfma_f32_16x16x4_f32, TE = 32: v_mfma_f32_32x32x2_f32), its
// wavefronts own 32-wide groups of a layer's outputs. Activations ping-pong between two LDS images [env][S], S = the widest layer
// rounded up to 64, + 4 floats: a lane's A operand is one 16-byte read of 4 consecutive k of its env's row, and with S = 4 (mod 64)
// the 16 lanes of a read group (envs r, row stride S) cover the 64 banks once. The weights are the B operand, read from the
// actor's packed copy [k][out] (K-major, the output index contiguous, zero-padded to 16 in k and 32 in out): the lanes of one k read
// one contiguous 128-byte piece. Zero padding is exact (padded weights and biases are 0 and act(0) = 0). mu and log_std are one
// stacked output group. No atomics, no local arrays, no inline assembly.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace act {

constexpr int MAX_IN = 64, MAX_HIDDEN = 256, MAX_LAYERS = 3, MAX_ACT = 8;
constexpr int KPAD = 16, OPAD = 32;   // granularity of the packed copy in k and in the output index
constexpr int WAVES = 4;              // per workgroup: one per SIMD
constexpr float LOG_STD_MIN = -20.0f, LOG_STD_MAX = 2.0f;  // stable_baselines3/sac/policies.py
enum { ACT_RELU = 0, ACT_TANH = 1 };

typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef float f32x16 __attribute__((ext_vector_type(16)));

constexpr int round_up(int x, int m) { return (x + m - 1) / m * m; }
// row stride of the LDS images, in floats, for a widest padded layer of `widest`
constexpr int lds_stride(int widest) { return round_up(widest, 64) + 4; }
constexpr size_t lds_bytes(int te, int widest) { return (size_t)2 * te * lds_stride(widest) * sizeof(float); }

struct ActorParams {
  int N;
  int obs_dim;     // row stride of obs
  int in_dim;      // columns gathered from an obs row
  int n_hidden;    // 1..3
  int A;           // action width
  int activation;  // ACT_*
  int S;           // lds_stride
  int k0;          // in_dim padded to KPAD
  int w0, w1, w2;  // hidden widths padded to OPAD (0 past n_hidden)
  const int* obs_index;                  // [in_dim], device
  const float *W0, *W1, *W2, *WH;        // packed weights [k][out]: hidden layers (unused ones nullptr) and the stacked head [k][32]
  const float *B0, *B1, *B2, *BH;        // padded biases
  const double* obs;                     // [N, obs_dim]
  const float* z;                        // [N, A] standard-normal draws or nullptr (deterministic)
  double* actions;                       // [N, A]
  float* squashed;                       // [N, A] or nullptr
  double low[MAX_ACT], high[MAX_ACT];
};

__device__ __forceinline__ float activate(float x, int activation) { return activation == ACT_RELU ? fmaxf(x, 0.0f) : tanhf(x); }

// 16 k of a 16x16 tile pair (v_mfma_f32_16x16x4_f32), for lane (r, kh) of a wavefront: the k loops of layer<16>, enc::conv and
// enc::fc_kernel. `a` = 4 consecutive k, 4 kh + 0..3 of the 16, of the lane's A row r; `w` = the lane's B column pair at the first of
// them, rows O floats apart; acc0 / acc1 = the tiles of the pair's two columns. Instruction s multiplies the k set {4 kh + s : kh = 0..3}.
struct BColumnPair { float2 k[4]; };  // (only ever indexed by constants: registers)
__device__ __forceinline__ BColumnPair load_b_k16(const float* __restrict__ w, int O) {
  return {{*reinterpret_cast<const float2*>(w), *reinterpret_cast<const float2*>(w + O), *reinterpret_cast<const float2*>(w + 2 * O),
           *reinterpret_cast<const float2*>(w + 3 * O)}};
}
__device__ __forceinline__ void tile_pair_k16(const f32x4 a, const BColumnPair& b, f32x4& acc0, f32x4& acc1) {
#pragma unroll
  for (int s = 0; s < 4; s++) {
    acc0 = __builtin_amdgcn_mfma_f32_16x16x4f32(a[s], b.k[s].x, acc0, 0, 0, 0);
    acc1 = __builtin_amdgcn_mfma_f32_16x16x4f32(a[s], b.k[s].y, acc1, 0, 0, 0);
  }
}
__device__ __forceinline__ void tile_pair_k16(const f32x4 a, const float* __restrict__ w, int O, f32x4& acc0, f32x4& acc1) {
  tile_pair_k16(a, load_b_k16(w, O), acc0, acc1);
}

// One layer for the calling wavefront: Y[env][o] = act(sum_k X[env][k] W[k][o] + b[o]) for the 32-wide output groups
// wave, wave + WAVES, ... below `O`; K a multiple of KPAD, O of OPAD. ACTIVATE false: the head (raw sums).
template <int TE, bool ACTIVATE>
__device__ __forceinline__ void layer(const float* X, float* Y, int S, const float* __restrict__ W, const float* __restrict__ B, int K, int O, int activation,
                                      int wave, int lane) {
  for (int g = wave; g * OPAD < O; g += WAVES) {
    if constexpr (TE == 16) {
      // lane (r, kh): env r, the k quarter kh of every 16; it owns the output columns c and c + 1, c = 32 g + 2 r, as two accumulators
      const int r = lane & 15, kh = lane >> 4, c = g * OPAD + 2 * r;
      const float2 b = *reinterpret_cast<const float2*>(B + c);
      f32x4 acc0 = {b.x, b.x, b.x, b.x}, acc1 = {b.y, b.y, b.y, b.y};
      const float* xrow = X + r * S + 4 * kh;
      const float* wcol = W + (size_t)(4 * kh) * O + c;
      for (int kb = 0; kb < K; kb += 16) tile_pair_k16(*reinterpret_cast<const f32x4*>(xrow + kb), wcol + (size_t)kb * O, O, acc0, acc1);
      // D: column = lane & 15 (here: the lane's column pair), row (env) = 4 (lane >> 4) + register
#pragma unroll
      for (int q = 0; q < 4; q++) {
        float2 y = {acc0[q], acc1[q]};
        if (ACTIVATE) { y.x = activate(y.x, activation); y.y = activate(y.y, activation); }
        *reinterpret_cast<float2*>(Y + (4 * kh + q) * S + c) = y;
      }
    } else {
      // lane (r, kh): env r, the k half kh of every 8; output column c = 32 g + r
      const int r = lane & 31, kh = lane >> 5, c = g * OPAD + r;
      const float b = B[c];
      f32x16 acc;
#pragma unroll
      for (int q = 0; q < 16; q++) acc[q] = b;
      const float* xrow = X + r * S + 4 * kh;
      const float* wcol = W + (size_t)(4 * kh) * O + c;
      for (int kb = 0; kb < K; kb += 8) {
        const f32x4 a = *reinterpret_cast<const f32x4*>(xrow + kb);
        const float* w = wcol + (size_t)kb * O;
        const float b0 = w[0], b1 = w[O], b2 = w[2 * O], b3 = w[3 * O];
        acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a[0], b0, acc, 0, 0, 0);
        acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a[1], b1, acc, 0, 0, 0);
        acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a[2], b2, acc, 0, 0, 0);
        acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a[3], b3, acc, 0, 0, 0);
      }
      // D: column = lane & 31, row (env) = (q & 3) + 8 (q >> 2) + 4 (lane >> 5)
#pragma unroll
      for (int q = 0; q < 16; q++) {
        const float y = ACTIVATE ? activate(acc[q], activation) : acc[q];
        Y[((q & 3) + 8 * (q >> 2) + 4 * kh) * S + c] = y;
      }
    }
  }
}

// The whole forward pass of a workgroup's TE envs: the inputs into LDS, the layers, the head, the squash and the unscale. gather(env, j) is
// input j of an env as float32; it is the one thing the kernels below differ in.
template <int TE, class Gather>
__device__ __forceinline__ void forward(const ActorParams& p, Gather gather) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  const int S = p.S;
  float* buf0 = lds;
  float* buf1 = lds + TE * S;
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const int env0 = blockIdx.x * TE;

  // x: the gathered inputs; rows of envs past N and the k padding are zero
  for (int e = tid; e < TE * p.k0; e += WAVES * 64) {
    const int r = e / p.k0, j = e - r * p.k0;
    float x = 0.0f;
    if (env0 + r < p.N && j < p.in_dim) x = gather(env0 + r, j);
    buf0[r * S + j] = x;
  }
  __syncthreads();

  // hidden layers (the launch's layer count is uniform), then the stacked head: mu in columns 0..A-1, log_std in A..2A-1
  layer<TE, true>(buf0, buf1, S, p.W0, p.B0, p.k0, p.w0, p.activation, wave, lane);
  __syncthreads();
  const float* h = buf1;
  float* other = buf0;
  int K = p.w0;
  if (p.n_hidden > 1) {
    layer<TE, true>(buf1, buf0, S, p.W1, p.B1, p.w0, p.w1, p.activation, wave, lane);
    __syncthreads();
    h = buf0; other = buf1; K = p.w1;
    if (p.n_hidden > 2) {
      layer<TE, true>(buf0, buf1, S, p.W2, p.B2, p.w1, p.w2, p.activation, wave, lane);
      __syncthreads();
      h = buf1; other = buf0; K = p.w2;
    }
  }
  layer<TE, false>(h, other, S, p.WH, p.BH, K, OPAD, p.activation, wave, lane);
  __syncthreads();

  // one thread per (env, action component)
  const int A = p.A;
  if (tid < TE * A) {
    const int r = tid / A, j = tid - r * A, i = env0 + r;
    if (i < p.N) {
      const float mu = other[r * S + j];
      const float ls = fminf(fmaxf(other[r * S + A + j], LOG_STD_MIN), LOG_STD_MAX);
      float u = mu;
      if (p.z) u = mu + expf(ls) * p.z[(size_t)i * A + j];
      const float a = tanhf(u);
      if (p.squashed) p.squashed[(size_t)i * A + j] = a;
      double lo = p.low[0], hi = p.high[0];  // (a select chain: no indexed copy of the argument arrays)
#pragma unroll
      for (int k = 1; k < MAX_ACT; k++) {
        lo = j == k ? p.low[k] : lo;
        hi = j == k ? p.high[k] : hi;
      }
      {
        // SB3's unscale_action, low + (0.5 * (a + 1.0) * (high - low)), operation by operation in float64: no contraction, so that
        // the result is the one numpy / torch give for the stored squashed action
#pragma clang fp contract(off)
        const double t = (double)a + 1.0;
        const double half = 0.5 * t;
        const double span = hi - lo;
        const double scaled = half * span;
        p.actions[(size_t)i * A + j] = lo + scaled;
      }
    }
  }
}

// Feature blocks of a visual actor (mjs_encoder.h): float32 [N, width[s]] per slot (0: scene camera, 1: wrist camera). There, entry j of
// ActorParams::obs_index is an observation column (>= 0) or -(1 + MAX_BLOCK_WIDTH s + f): component f of slot s.
constexpr int MAX_BLOCKS = 2, MAX_BLOCK_WIDTH = 512;
struct FeatureInputs {
  const float* feat[MAX_BLOCKS];
  int width[MAX_BLOCKS];
};

// The kernels: grid = ceil(N / TE) workgroups of WAVES wavefronts; dynamic LDS = lds_bytes(TE, widest layer). The state actor's input j is
// an observation column, float64 -> float32 (round to nearest) ...
template <int TE>
__global__ __launch_bounds__(WAVES * 64) void kernel(ActorParams p) {
  forward<TE>(p, [obs = p.obs, obs_dim = p.obs_dim, index = p.obs_index](int env, int j) { return (float)obs[(size_t)env * obs_dim + index[j]]; });
}
// ... the visual actor's an observation column or a feature component, TE = 16. in_dim and k0 count the feature blocks (k0 up to
// 64 + 2 * 512: the LDS images can pass 64 KB, an opt-in).
__global__ __launch_bounds__(WAVES * 64) void kernel_visual(ActorParams p, FeatureInputs fi) {
  forward<16>(p, [&](int env, int j) {
    const int c = p.obs_index[j];
    if (c >= 0) return (float)p.obs[(size_t)env * p.obs_dim + c];
    const int t = -1 - c, slot = t / MAX_BLOCK_WIDTH, f = t - slot * MAX_BLOCK_WIDTH;
    return slot == 0 ? fi.feat[0][(size_t)env * fi.width[0] + f] : fi.feat[1][(size_t)env * fi.width[1] + f];
  });
}

// torch.nn.Linear parameters (weight [out, in] row-major, bias [out]) -> the packed copy: dst_w [K][O], dst_b [O], K >= in, O >= out0 +
// out1, zero-padded. Two sources stack along the output index (the head: mu, then log_std); src1 nullptr: one source.
struct PackParams {
  const float *w0, *b0, *w1, *b1;
  int out0, out1, in;
  int K, O;
  float *dst_w, *dst_b;
};
__global__ __launch_bounds__(256) void pack_kernel(PackParams p) {
  const int e = blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= p.K * p.O) return;
  const int k = e / p.O, o = e - k * p.O;
  float w = 0.0f, b = 0.0f;
  if (o < p.out0) {
    if (k < p.in) w = p.w0[(size_t)o * p.in + k];
    b = p.b0[o];
  } else if (o < p.out0 + p.out1) {
    if (k < p.in) w = p.w1[(size_t)(o - p.out0) * p.in + k];
    b = p.b1[o - p.out0];
  }
  p.dst_w[e] = w;
  if (k == 0) p.dst_b[o] = b;
}

}  // namespace act
