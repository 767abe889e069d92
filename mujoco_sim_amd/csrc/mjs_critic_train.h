// mjs_critic_train.h — the critic half of a SAC gradient step (stable_baselines3/sac/sac.py SAC.train) on the packed parameter copy of
// mjs_critic.h, which becomes the master copy:
//   grad_kernel      q_c = Q_c(obs, actions); loss_c = mean((q_c - y)^2); the gradient of 0.5 * sum_c loss_c for every layer's weight
//                    and bias, as one partial slab per (split, critic)
//   adam_kernel      g = the slabs summed in order; torch.optim.Adam (amsgrad=False, weight_decay=0, maximize=False) on the packed copy
//   slab_sum_kernel  g alone, for callers that want the gradients
//   blend_kernel     SB3's polyak_update from one packed copy into another
//   unpack_kernel    a packed layer -> torch.nn.Linear layout (act::pack_kernel's inverse for one source)
//
// float32 with float32 accumulation, the contract of mjs_critic.h. The forward pass is fill_input and act::layer<16> with q_kernel's
// arguments, so q is q_kernel's bit for bit; it keeps every layer's activation image. Backward, per layer (head first), from the
// image G of dZ = dLoss/d(pre-activation) [row][o], the layer's input image IN [row][k] and its packed weights W [k][o]:
//   dW[k][o] = sum_r IN[r][k] dZ[r][o]     16x16 tiles of (k, o), the 16 rows as the MFMA's k: 4 x v_mfma_f32_16x16x4_f32 from 0, rows in order
//   db[o]    = sum_r dZ[r][o]              one thread per o, rows in order from 0
//   dIN[r][k] = sum_o dZ[r][o] W[k][o]     16x16 tiles of (r, k), o as the MFMA's k: the A operand is 4 consecutive o of a row of G (one
//                                          16-byte LDS read), the B operand 4 consecutive o of row k of W (one 16-byte global read: the
//                                          packed [k][out] layout serves the transposed product as it is, no second copy)
//   dZ_prev  = dIN * act'(H_prev)          in the same epilogue, from the STORED activation: relu' = H > 0 (so relu'(0) = 0, as torch),
//                                          tanh' = 1 - H^2
// Layer 0 computes no dIN. Zero padding is exact: a padded k has IN = 0 and W's row 0, a padded o has dZ = 0, a row past B has dq = 0.
//
// The sum over the batch is bitwise reproducible, with no atomics: workgroup (split, critic) owns the contiguous 16-row tiles
// [split * tiles_per_split, (split + 1) * tiles_per_split) and one slab in global memory, laid out like the packed copy (Layout). A
// tile's partial gradient (the 16-row sums above, each from 0) is stored for the first tile and ADDED to the slab for every further one, in
// tile order, each element by the lane that owns it in every tile. The running sum lives in the workgroup's own slab, not in registers:
// a [256, 256] critic has 78 368 gradient elements, 306 per lane of a 256-thread workgroup, whose index depends on the (runtime) widths,
// and the LDS holds the activation images. With one tile per workgroup (B <= 16 * splits) nothing is read back. The consumer sums the
// slabs 0, 1, 2, ... in order (slab_sum()). split_rule() is a function of B and the shape alone.
//
// LDS: X, one image per hidden layer, and a gradient ping-pong pair, [16][S] floats each (train_lds_bytes): up to 6 x 16 x 260 x 4 B =
// 99 840 B, above the 64 KB a kernel gets without the opt-in and below the CU's 160 KB. No atomics, no local arrays, no inline assembly.
#pragma once
#include "mjs_critic.h"

namespace crit {

constexpr int MAX_SPLITS = 128;                        // workgroups per critic, at most
constexpr size_t WORKSPACE_CAP = (size_t)128 << 20;    // bytes of slabs, at most (where one slab per critic fits)
constexpr size_t train_lds_bytes(int n_hidden, int widest) { return (size_t)(3 + n_hidden) * ROWS * act::lds_stride(widest) * sizeof(float); }

// Where a critic's parameters sit in a slab (and in the optimiser's m and v): segment 2 l = layer l's weights [K][O], 2 l + 1 = its bias
// [O], l = 3 the head; unused layers are empty. off[8] = the loss partial (one float), total = off[8] + 4 (16-byte multiple).
struct Layout {
  int off[9];
  int total;
};
// One critic's packed copy as the segments' base pointers
struct Packed {
  float* seg[8];
};
// (a select chain: no indexed copy of the argument arrays)
__device__ __forceinline__ float* locate(const Layout& L, const Packed& P, int e) {
  float* p = P.seg[0] + e;
#pragma unroll
  for (int s = 1; s < 8; s++) p = e >= L.off[s] ? P.seg[s] + (e - L.off[s]) : p;
  return p;
}

// tiles = ceil(B / 16); splits_max = min(MAX_SPLITS, max(1, WORKSPACE_CAP / (n_critics * slab bytes)));
// tiles_per_split = ceil(tiles / splits_max); splits = ceil(tiles / tiles_per_split)
struct Split {
  int tiles_per_split, splits;
};
inline int splits_max(int n_critics, int slab_floats) {
  const long long cap = (long long)(WORKSPACE_CAP / ((size_t)n_critics * slab_floats * sizeof(float)));
  return cap < 1 ? 1 : cap > MAX_SPLITS ? MAX_SPLITS : (int)cap;
}
inline Split split_rule(int B, int n_critics, int slab_floats) {
  const long long tiles = ((long long)B + ROWS - 1) / ROWS, cap = splits_max(n_critics, slab_floats);
  const long long tps = tiles < 1 ? 1 : (tiles + cap - 1) / cap;
  return {(int)tps, (int)((tiles + tps - 1) / tps)};
}

struct GradParams {
  CriticParams c;          // S: the stride of the 3 + n_hidden images
  Layout L;
  int tiles_per_split;
  float inv_B;             // 1 / B rounded to float32 on the host
  const float* obs;        // [B, D]
  const float* actions;    // [B, A]
  const float* target;     // [B]
  float* q;                // [n_critics, B] or nullptr
  float* slabs;            // [splits][n_critics][L.total]
};

// tile += or = : the slab's element, by the lane that owns it in every tile
__device__ __forceinline__ void slab_add(float* p, float v, bool first) { *p = first ? v : *p + v; }

// dW and db of one layer into the slab, for the calling workgroup. IN [16][K], G = dZ [16][O]; K a multiple of 16, O of 32.
__device__ __forceinline__ void weight_grad(const float* IN, const float* G, int S, int K, int O, float* dW, float* db, bool first, int tid) {
  const int wave = tid >> 6, lane = tid & 63, c = lane & 15, kh = lane >> 4;
  // A[i][kk] = IN[4 s + kk][kb + i] from lane (i = c, kk = kh), B[kk][j] = G[4 s + kk][ob + j] from lane (kk = kh, j = c):
  // instruction s adds rows 4 s .. 4 s + 3 in order. D register q: dW[kb + 4 kh + q][ob + c]
  for (int ot = wave; ot * 16 < O; ot += act::WAVES) {
    const int ob = ot * 16;
    const float* g = G + kh * S + ob + c;
    const float b0 = g[0], b1 = g[4 * S], b2 = g[8 * S], b3 = g[12 * S];
    for (int kb = 0; kb < K; kb += 16) {
      const float* x = IN + kh * S + kb + c;
      act::f32x4 acc = {0.0f, 0.0f, 0.0f, 0.0f};
      acc = __builtin_amdgcn_mfma_f32_16x16x4f32(x[0], b0, acc, 0, 0, 0);
      acc = __builtin_amdgcn_mfma_f32_16x16x4f32(x[4 * S], b1, acc, 0, 0, 0);
      acc = __builtin_amdgcn_mfma_f32_16x16x4f32(x[8 * S], b2, acc, 0, 0, 0);
      acc = __builtin_amdgcn_mfma_f32_16x16x4f32(x[12 * S], b3, acc, 0, 0, 0);
      float* d = dW + (size_t)(kb + 4 * kh) * O + ob + c;
#pragma unroll
      for (int q = 0; q < 4; q++) slab_add(d + (size_t)q * O, acc[q], first);
    }
  }
  for (int o = tid; o < O; o += act::WAVES * 64) {
    float s = 0.0f;
#pragma unroll
    for (int r = 0; r < ROWS; r++) s += G[r * S + o];
    slab_add(db + o, s, first);
  }
}

// dZ of the layer below into Gout [16][K]: (sum_o G[r][o] W[k][o]) * act'(H[r][k]). K a multiple of 32 (a hidden width), O of 32. As in
// act::layer<16>, a wavefront owns 32-wide groups of the output (here: k) as two 16-wide tiles that share the A operand.
__device__ __forceinline__ void input_grad(const float* G, const float* H, float* Gout, int S, const float* __restrict__ W, int K, int O, int activation,
                                           int wave, int lane) {
  const int c = lane & 15, kh = lane >> 4;
  for (int g = wave; g * 32 < K; g += act::WAVES) {
    const int k0 = g * 32 + c, k1 = k0 + 16;
    const float* grow = G + c * S + 4 * kh;               // A[i = row c][kk = o]: 4 consecutive o
    const float* w0 = W + (size_t)k0 * O + 4 * kh;        // B[kk = o][j = k]: 4 consecutive o of row k
    const float* w1 = W + (size_t)k1 * O + 4 * kh;
    act::f32x4 acc0 = {0.0f, 0.0f, 0.0f, 0.0f}, acc1 = {0.0f, 0.0f, 0.0f, 0.0f};
    for (int ob = 0; ob < O; ob += 16) {
      const act::f32x4 a = *reinterpret_cast<const act::f32x4*>(grow + ob);
      const act::f32x4 b0 = *reinterpret_cast<const act::f32x4*>(w0 + ob);
      const act::f32x4 b1 = *reinterpret_cast<const act::f32x4*>(w1 + ob);
#pragma unroll
      for (int s = 0; s < 4; s++) {
        acc0 = __builtin_amdgcn_mfma_f32_16x16x4f32(a[s], b0[s], acc0, 0, 0, 0);
        acc1 = __builtin_amdgcn_mfma_f32_16x16x4f32(a[s], b1[s], acc1, 0, 0, 0);
      }
    }
    // D register q: row 4 kh + q, column k0 (acc0) / k1 (acc1)
#pragma unroll
    for (int q = 0; q < 4; q++) {
      const int r = 4 * kh + q;
      const float h0 = H[r * S + k0], h1 = H[r * S + k1];
      float d0, d1;
      if (activation == act::ACT_RELU) {
        d0 = h0 > 0.0f ? acc0[q] : 0.0f;
        d1 = h1 > 0.0f ? acc1[q] : 0.0f;
      } else {
        d0 = acc0[q] * (1.0f - h0 * h0);
        d1 = acc1[q] * (1.0f - h1 * h1);
      }
      Gout[r * S + k0] = d0;
      Gout[r * S + k1] = d1;
    }
  }
}

// grid = (splits, n_critics) workgroups of WAVES wavefronts; dynamic LDS = train_lds_bytes(n_hidden, widest)
__global__ __launch_bounds__(act::WAVES * 64) void grad_kernel(GradParams p) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  const int S = p.c.S, B = p.c.B, img = ROWS * S;
  const Mlp& m = blockIdx.y == 0 ? p.c.net[0] : p.c.net[1];
  const int n = m.n_hidden, act_id = m.activation;
  float* X = lds;
  float* H0 = lds + img;
  float* H1 = lds + 2 * img;                 // (images past n_hidden are not there and not touched)
  float* H2 = lds + 3 * img;
  float* GA = lds + (1 + n) * img;
  float* GB = lds + (2 + n) * img;
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  float* slab = p.slabs + ((size_t)blockIdx.x * p.c.n_critics + blockIdx.y) * p.L.total;
  const float* Hlast = n == 1 ? H0 : n == 2 ? H1 : H2;
  const int Klast = n == 1 ? m.w0 : n == 2 ? m.w1 : m.w2;
  const int tile0 = blockIdx.x * p.tiles_per_split, tiles = (B + ROWS - 1) / ROWS;
  float loss = 0.0f;  // thread 0: the workgroup's sum of (q - y)^2, tile sums added in tile order

  for (int t = tile0; t < tile0 + p.tiles_per_split && t < tiles; t++) {
    const int row0 = t * ROWS;
    const bool first = t == tile0;
    // forward: q_kernel's fill and layers, every activation image kept; the head's raw sums land in GA
    fill_input(X, S, m.k0, p.c.D + p.c.A, row0, B, tid,
               [&](int i, int j) { return j < p.c.D ? p.obs[(size_t)i * p.c.D + j] : p.actions[(size_t)i * p.c.A + (j - p.c.D)]; });
    __syncthreads();
    act::layer<ROWS, true>(X, H0, S, m.W0, m.B0, m.k0, m.w0, act_id, wave, lane);
    __syncthreads();
    if (n > 1) {
      act::layer<ROWS, true>(H0, H1, S, m.W1, m.B1, m.w0, m.w1, act_id, wave, lane);
      __syncthreads();
      if (n > 2) {
        act::layer<ROWS, true>(H1, H2, S, m.W2, m.B2, m.w1, m.w2, act_id, wave, lane);
        __syncthreads();
      }
    }
    act::layer<ROWS, false>(Hlast, GA, S, m.WH, m.BH, Klast, act::OPAD, act_id, wave, lane);
    __syncthreads();

    // the head's dZ into GB: dq = (q - y) * (1 / B) in column 0, zero in the other OPAD - 1 and in the rows past B; (q - y)^2 in
    // column OPAD, which no product reads (S > 2 OPAD)
    if (tid < ROWS) {
      const int i = row0 + tid;
      float diff = 0.0f;
      if (i < B) {
        const float qv = GA[tid * S];
        if (p.q) p.q[(size_t)blockIdx.y * B + i] = qv;
        diff = qv - p.target[i];
      }
      float* row = GB + tid * S;
      row[0] = diff * p.inv_B;
#pragma unroll
      for (int o = 1; o < act::OPAD; o++) row[o] = 0.0f;
      row[act::OPAD] = diff * diff;
    }
    __syncthreads();
    if (tid == 0) {
      float s = 0.0f;
#pragma unroll
      for (int r = 0; r < ROWS; r++) s += GB[r * S + act::OPAD];
      loss = first ? s : loss + s;
    }

    // backward, head first; a layer's two products read the same dZ image and write elsewhere (the slab, the other image)
    weight_grad(Hlast, GB, S, Klast, act::OPAD, slab + p.L.off[6], slab + p.L.off[7], first, tid);
    input_grad(GB, Hlast, GA, S, m.WH, Klast, act::OPAD, act_id, wave, lane);
    __syncthreads();
    float* G = GA;      // dZ of the layer at hand
    float* other = GB;
    if (n > 2) {
      weight_grad(H1, G, S, m.w1, m.w2, slab + p.L.off[4], slab + p.L.off[5], first, tid);
      input_grad(G, H1, other, S, m.W2, m.w1, m.w2, act_id, wave, lane);
      __syncthreads();
      float* sw = G; G = other; other = sw;
    }
    if (n > 1) {
      weight_grad(H0, G, S, m.w0, m.w1, slab + p.L.off[2], slab + p.L.off[3], first, tid);
      input_grad(G, H0, other, S, m.W1, m.w0, m.w1, act_id, wave, lane);
      __syncthreads();
      float* sw = G; G = other; other = sw;
    }
    weight_grad(X, G, S, m.k0, m.w0, slab + p.L.off[0], slab + p.L.off[1], first, tid);
    __syncthreads();  // the next tile's fill writes X, its layers the images
  }
  if (tid == 0) slab[p.L.off[8]] = loss;
}

// element e of critic c's gradient: the slabs in order 0, 1, 2, ...
__device__ __forceinline__ float slab_sum(const float* __restrict__ slabs, int splits, int n_critics, int total, int c, int e) {
  const float* s = slabs + (size_t)c * total + e;
  float g = s[0];
  for (int k = 1; k < splits; k++) g += s[(size_t)k * n_critics * total];
  return g;
}

struct SumParams {
  Layout L;
  int n_critics, splits;
  float inv_B;
  const float* slabs;
  float* loss;  // [n_critics] or nullptr: mean((q_c - y)^2) = (the loss partials summed in order) * (1 / B)
};

// grid = (ceil(L.total / 256), n_critics): g into out [n_critics][L.total] (slab layout)
__global__ __launch_bounds__(256) void slab_sum_kernel(SumParams p, float* __restrict__ out) {
  const int e = blockIdx.x * blockDim.x + threadIdx.x, c = blockIdx.y;
  if (e > p.L.off[8]) return;
  const float g = slab_sum(p.slabs, p.splits, p.n_critics, p.L.total, c, e);
  if (e == p.L.off[8]) {
    if (p.loss) p.loss[c] = g * p.inv_B;
    return;
  }
  out[(size_t)c * p.L.total + e] = g;
}

struct AdamParams {
  SumParams s;
  Packed net[MAX_CRITICS];  // the parameters, updated in place
  float* m;                 // [n_critics][L.total], slab layout
  float* v;
  // the host computes these in double from the step count t (after its increment) and rounds each to float32 once:
  float one_minus_beta1;    // 1 - beta1
  float beta2;              // beta2
  float one_minus_beta2;    // 1 - beta2
  float sqrt_bc2;           // sqrt(1 - beta2^t)
  float eps;                // eps
  float step_size;          // lr / (1 - beta1^t)
};

// grid = (ceil(L.total / 256), n_critics). torch.optim.Adam's single-tensor step in float32, one operation per line, no contraction:
//   gm = g - m;  m1 = (1 - beta1) * gm;  m = m + m1                        exp_avg.lerp_(grad, 1 - beta1), as two roundings
//   g2 = g * g;  v1 = beta2 * v;  v2 = (1 - beta2) * g2;  v = v1 + v2      exp_avg_sq.mul_(beta2).addcmul_(grad, grad, value=1 - beta2)
//   sq = sqrtf(v);  d0 = sq / sqrt_bc2;  den = d0 + eps                    (exp_avg_sq.sqrt() / bias_correction2_sqrt).add_(eps)
//   r = m / den;  u = step_size * r;  p = p - u                            param.addcdiv_(exp_avg, denom, value=-step_size)
// sqrtf and the divisions are correctly rounded (no fast-math). The padding has g = m = v = p = 0 and stays 0 (0 / eps = 0).
__global__ __launch_bounds__(256) void adam_kernel(AdamParams p) {
  const int e = blockIdx.x * blockDim.x + threadIdx.x, c = blockIdx.y;
  const Layout& L = p.s.L;
  if (e > L.off[8]) return;
  const float g = slab_sum(p.s.slabs, p.s.splits, p.s.n_critics, L.total, c, e);
  if (e == L.off[8]) {
    if (p.s.loss) p.s.loss[c] = g * p.s.inv_B;
    return;
  }
  float* param = locate(L, c == 0 ? p.net[0] : p.net[1], e);
  const size_t at = (size_t)c * L.total + e;
  const float m0 = p.m[at], v0 = p.v[at], p0 = *param;
  {
#pragma clang fp contract(off)
    const float gm = g - m0;
    const float m1 = p.one_minus_beta1 * gm;
    const float m = m0 + m1;
    const float g2 = g * g;
    const float v1 = p.beta2 * v0;
    const float v2 = p.one_minus_beta2 * g2;
    const float v = v1 + v2;
    const float sq = sqrtf(v);
    const float d0 = sq / p.sqrt_bc2;
    const float den = d0 + p.eps;
    const float r = m / den;
    const float u = p.step_size * r;
    p.m[at] = m;
    p.v[at] = v;
    *param = p0 - u;
  }
}

// grid = (ceil(L.off[8] / 256), n_critics): dst = (1 - tau) * dst + tau * src over the whole packed copies, as pack_lerp_kernel computes
// it: fmaf(tau, src, one_minus_tau * dst). The padding is 0 on both sides and stays 0. COPY (tau == 1): dst = src, dst is not read.
struct BlendParams {
  Layout L;
  Packed dst[MAX_CRITICS], src[MAX_CRITICS];
};
template <bool COPY>
__global__ __launch_bounds__(256) void blend_kernel(BlendParams p, float one_minus_tau, float tau) {
  const int e = blockIdx.x * blockDim.x + threadIdx.x, c = blockIdx.y;
  if (e >= p.L.off[8]) return;
  float* d = locate(p.L, c == 0 ? p.dst[0] : p.dst[1], e);
  const float s = *locate(p.L, c == 0 ? p.src[0] : p.src[1], e);
  *d = COPY ? s : fmaf(tau, s, one_minus_tau * *d);
}

// One packed layer src_w [K][O], src_b [O] -> torch.nn.Linear layout dst_w [out, in], dst_b [out]: act::pack_kernel's inverse for one
// source. grid = ceil(out * in / 256)
struct UnpackParams {
  const float *src_w, *src_b;
  int K, O, in, out;
  float *dst_w, *dst_b;
};
__global__ __launch_bounds__(256) void unpack_kernel(UnpackParams p) {
  const int e = blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= p.out * p.in) return;
  const int o = e / p.in, k = e - o * p.in;
  p.dst_w[e] = p.src_w[(size_t)k * p.O + o];
  if (k == 0) p.dst_b[o] = p.src_b[o];
}

}  // namespace crit
