// mjs_encoder.h — SB3's NatureCNN (stable_baselines3/common/torch_layers.py) on the ray caster's output: uint8 NHWC frames in, float32
// features out. What the reference's RL scripts put between a camera image and SAC's MLP actor (MultiInputPolicy -> CombinedExtractor
// -> NatureCNN per image key; scripts/sb3/reach_sac.py, planar_push.py, sb3_sac.py).
//
//   x[c][y][x] = (float) rgb[y][x][c] / 255.0f         conv1 3->32 8x8 stride 4, conv2 32->64 4x4 stride 2, conv3 64->64 3x3 stride 1, ReLU each,
//   flat = conv3 output in CHW order                    features = ReLU(W_fc flat + b_fc)
//
// float32 with float32 accumulation on the f32-input MFMA (v_mfma_f32_16x16x4_f32), every accumulator starts at the bias. Two kernels:
//   conv_kernel  one workgroup of 4 wavefronts per env, the three convolutions as implicit GEMMs with the activations kept in LDS.
//                Rows of a GEMM are output positions, columns output channels, k runs over (ky, kx, c) with c fastest - the order the
//                image (HWC bytes) and the LDS activations ([position][channel]) are stored in, so that a lane's A operand (4 consecutive
//                k of its position) is ONE 4-byte (image) or 16-byte (activations) LDS read. The image stays uint8 in LDS (27 KB at
//                96x96; as floats it would not fit next to conv1's output) and goes through a 256-entry table of (float) i / 255.0f,
//                the exact quotients. A wavefront owns RT row tiles x 32 channels at a time: the B operand (packed weights [k][out],
//                read from L2) is loaded once for RT tiles. conv3 writes `flat` [N][64 H3 W3] to the caller's workspace.
//   fc_kernel    the linear layer over 16-env tiles, k streamed through LDS in chunks of 256, a wavefront owning up to four 32-wide
//                output groups; act::layer's operand layout.
// LDS strides: 36 floats per conv1 position, 68 per conv2 position (4 mod 32: the 16 lanes of a read group spread over the banks).
// No atomics, no inline assembly, no run-time-indexed local arrays; the grid of conv_kernel is N, fc_kernel masks envs past N.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "mjs_actor.h"

namespace enc {

constexpr int MIN_HW = 36, MAX_HW = 96, MAX_F = 512;
constexpr int C_IN = 3, C1 = 32, C2 = 64, C3 = 64;
constexpr int WAVES = 4;
constexpr int RT = 4;            // row tiles (of 16 output positions) a wavefront carries per pass
constexpr int S1 = C1 + 4, S2 = C2 + 4;  // LDS floats per conv1 / conv2 output position
constexpr int LUT_BYTES = 256 * sizeof(float);
constexpr int FPAD = 32;         // granularity of the packed fc copy in the output index
constexpr int FC_TE = 16, FC_KC = 256, FC_S = FC_KC + 4, FC_GROUPS = MAX_F / 32 / WAVES;

using act::f32x4;
using act::round_up;

constexpr int conv_out(int n, int k, int s) { return (n - k) / s + 1; }

struct Geometry {
  int H, W;
  int H1, W1, H2, W2, H3, W3;
  int RS;         // bytes per image row in LDS (3 W rounded up to 4)
  int n_flatten;  // 64 H3 W3
};
constexpr Geometry geometry(int H, int W) {
  Geometry g{};
  g.H = H; g.W = W;
  g.H1 = conv_out(H, 8, 4); g.W1 = conv_out(W, 8, 4);
  g.H2 = conv_out(g.H1, 4, 2); g.W2 = conv_out(g.W1, 4, 2);
  g.H3 = conv_out(g.H2, 3, 1); g.W3 = conv_out(g.W2, 3, 1);
  g.RS = round_up(3 * W, 4);
  g.n_flatten = C3 * g.H3 * g.W3;
  return g;
}
// dynamic LDS of conv_kernel: table, image, conv1 output, conv2 output (each 16-byte aligned)
constexpr int img_bytes(const Geometry& g) { return round_up(g.H * g.RS, 16); }
constexpr size_t lds_bytes(const Geometry& g) {
  return (size_t)LUT_BYTES + img_bytes(g) + sizeof(float) * ((size_t)g.H1 * g.W1 * S1 + (size_t)g.H2 * g.W2 * S2);
}
static_assert(lds_bytes(geometry(MAX_HW, MAX_HW)) <= 160 * 1024, "one env's activations fit the CU's LDS");

struct ConvParams {
  int N;
  Geometry g;
  const uint8_t* rgb;                          // [N, H, W, 3]
  const float *W1, *B1, *W2, *B2, *W3, *B3;    // packed [k][out], k = (ky KW + kx) CIN + c
  float* flat;                                 // [N, n_flatten]
};

// One convolution for the calling wavefront. IMAGE: the input is the uint8 image (row stride RSb bytes) behind the table `lut`;
// otherwise X [position][XS floats]. GLOBAL_OUT: Y is the env's `flat` row (CHW order, P positions per channel); otherwise LDS
// [position][YS floats].
template <int KH, int KW, int STRIDE, int CIN, int COUT, bool IMAGE, bool GLOBAL_OUT>
__device__ __forceinline__ void conv(const uint8_t* img, const float* lut, int RSb, const float* X, int XS, int Win, int Wout, int P, float* Y, int YS,
                                     const float* __restrict__ Wt, const float* __restrict__ Bs, int wave, int lane) {
  constexpr int K = KH * KW * CIN, NG = COUT / 32;
  static_assert(K % 16 == 0 && COUT % 32 == 0 && (IMAGE ? (KW * CIN) % 4 == 0 : CIN % 16 == 0), "k blocks of 16 and a lane's 4 k stay inside one tap / image row");
  const int r = lane & 15, kh = lane >> 4;
  const int ntiles = (P + 15) >> 4, npass = (ntiles + RT - 1) / RT;
  for (int it = wave; it < npass * NG; it += WAVES) {
    const int pass = it / NG, g = it - pass * NG, tile0 = pass * RT;
    const int c = g * 32 + 2 * r;  // the lane's column pair, as in act::layer
    const float2 bias = *reinterpret_cast<const float2*>(Bs + c);
    f32x4 acc[RT][2];
    int base[RT];
#pragma unroll
    for (int j = 0; j < RT; j++) {
      acc[j][0] = f32x4{bias.x, bias.x, bias.x, bias.x};
      acc[j][1] = f32x4{bias.y, bias.y, bias.y, bias.y};
      int p = (tile0 + j) * 16 + r;  // the lane's A row; rows past P read the last position and are not written
      p = p < P ? p : P - 1;
      const int oy = p / Wout, ox = p - oy * Wout;
      base[j] = IMAGE ? oy * STRIDE * RSb + ox * STRIDE * CIN : (oy * STRIDE * Win + ox * STRIDE) * XS;
    }
    for (int kb = 0; kb < K; kb += 16) {
      const int k4 = kb + 4 * kh;  // the lane's 4 consecutive k
      int off;
      if (IMAGE) {
        const int ky = k4 / (KW * CIN);
        off = ky * RSb + (k4 - ky * KW * CIN);
      } else {
        const int tap = k4 / CIN, c0 = k4 - tap * CIN, ky = tap / KW, kx = tap - ky * KW;
        off = (ky * Win + kx) * XS + c0;
      }
      const act::BColumnPair b = act::load_b_k16(Wt + (size_t)k4 * COUT + c, COUT);  // read once for the RT tiles
#pragma unroll
      for (int j = 0; j < RT; j++) {
        if (tile0 + j < ntiles) {  // (uniform over the wavefront)
          f32x4 a;
          if (IMAGE) {
            const uint32_t u = *reinterpret_cast<const uint32_t*>(img + base[j] + off);
            a = f32x4{lut[u & 255u], lut[(u >> 8) & 255u], lut[(u >> 16) & 255u], lut[u >> 24]};
          } else {
            a = *reinterpret_cast<const f32x4*>(X + base[j] + off);
          }
          act::tile_pair_k16(a, b, acc[j][0], acc[j][1]);
        }
      }
    }
    // D: column = the lane's column pair, row (position) = 4 (lane >> 4) + register
#pragma unroll
    for (int j = 0; j < RT; j++) {
#pragma unroll
      for (int q = 0; q < 4; q++) {
        const int pos = (tile0 + j) * 16 + 4 * kh + q;
        if (pos < P) {
          const float2 y = {fmaxf(acc[j][0][q], 0.0f), fmaxf(acc[j][1][q], 0.0f)};
          if (GLOBAL_OUT) {
            Y[(size_t)c * P + pos] = y.x;
            Y[(size_t)(c + 1) * P + pos] = y.y;
          } else {
            *reinterpret_cast<float2*>(Y + pos * YS + c) = y;
          }
        }
      }
    }
  }
}

// The LDS activations of one env [P][S floats] -> dst [P][C], 16 bytes per thread and step (KEEP below)
template <int C, int S>
__device__ __forceinline__ void store_activations(const float* Y, int P, float* __restrict__ dst, int tid) {
  for (int e = tid; e < P * (C / 4); e += WAVES * 64) {
    const int pos = e / (C / 4), j = e - pos * (C / 4);
    *reinterpret_cast<f32x4*>(dst + (size_t)e * 4) = *reinterpret_cast<const f32x4*>(Y + pos * S + 4 * j);
  }
}

// The three convolutions of one workgroup's env: conv_kernel's body, shared with the training forward (mjs_encoder_train.h), which
// KEEPs the post-ReLU outputs of conv1 in keep1 [N, P1, 32] and of conv2 in keep2 [N, P2, 64] (copies of the LDS images; `flat` is
// conv3's). The arithmetic does not depend on KEEP.
template <bool KEEP>
__device__ __forceinline__ void convs(const ConvParams& p, float* keep1, float* keep2) {
  extern __shared__ __attribute__((aligned(16))) unsigned char enc_lds[];
  const Geometry& g = p.g;
  float* lut = reinterpret_cast<float*>(enc_lds);
  uint8_t* img = enc_lds + LUT_BYTES;
  float* c1 = reinterpret_cast<float*>(img + img_bytes(g));
  float* c2 = c1 + g.H1 * g.W1 * S1;
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const int env = blockIdx.x;
  if (env >= p.N) return;  // (uniform over the workgroup)

  lut[tid] = (float)tid / 255.0f;  // WAVES * 64 = 256 entries; a float32 division, as SB3's preprocess_obs does
  const int row = 3 * g.W;
  const uint8_t* src = p.rgb + (size_t)env * g.H * row;
  for (int e = tid; e < g.H * row; e += WAVES * 64) {
    const int y = e / row, j = e - y * row;
    img[y * g.RS + j] = src[e];
  }
  __syncthreads();
  conv<8, 8, 4, C_IN, C1, true, false>(img, lut, g.RS, nullptr, 0, g.W, g.W1, g.H1 * g.W1, c1, S1, p.W1, p.B1, wave, lane);
  __syncthreads();
  if (KEEP) store_activations<C1, S1>(c1, g.H1 * g.W1, keep1 + (size_t)env * g.H1 * g.W1 * C1, tid);
  conv<4, 4, 2, C1, C2, false, false>(nullptr, nullptr, 0, c1, S1, g.W1, g.W2, g.H2 * g.W2, c2, S2, p.W2, p.B2, wave, lane);
  __syncthreads();
  if (KEEP) store_activations<C2, S2>(c2, g.H2 * g.W2, keep2 + (size_t)env * g.H2 * g.W2 * C2, tid);
  conv<3, 3, 1, C2, C3, false, true>(nullptr, nullptr, 0, c2, S2, g.W2, g.W3, g.H3 * g.W3, p.flat + (size_t)env * g.n_flatten, 0, p.W3, p.B3, wave, lane);
}

// grid = N workgroups of WAVES wavefronts; dynamic LDS = lds_bytes(geometry)
__global__ __launch_bounds__(WAVES * 64) void conv_kernel(ConvParams p) { convs<false>(p, nullptr, nullptr); }
static_assert(WAVES * 64 == 256, "the table of quotients has one entry per thread");

struct FcParams {
  int N, K, F, Fp;     // K = n_flatten (a multiple of 64), Fp = F padded to FPAD
  const float* flat;   // [N, K]
  const float *W, *B;  // packed [K][Fp], [Fp]
  float* out;          // [N, F]
};

// grid = ceil(N / 16) workgroups of WAVES wavefronts. Wavefront w owns the 32-wide output groups w, w + 4, w + 8, w + 12 below Fp.
__global__ __launch_bounds__(WAVES * 64) void fc_kernel(FcParams p) {
  __shared__ __attribute__((aligned(16))) float xs[FC_TE * FC_S];
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const int r = lane & 15, kh = lane >> 4;
  const int env0 = blockIdx.x * FC_TE;
  const int ngroups = p.Fp / 32;
  f32x4 acc[FC_GROUPS][2];
#pragma unroll
  for (int j = 0; j < FC_GROUPS; j++) {
    const int g = wave + WAVES * j;
    float2 b = {0.0f, 0.0f};
    if (g < ngroups) b = *reinterpret_cast<const float2*>(p.B + g * 32 + 2 * r);
    acc[j][0] = f32x4{b.x, b.x, b.x, b.x};
    acc[j][1] = f32x4{b.y, b.y, b.y, b.y};
  }
  for (int k0 = 0; k0 < p.K; k0 += FC_KC) {
    const int kc = p.K - k0 < FC_KC ? p.K - k0 : FC_KC;  // a multiple of 64
    __syncthreads();  // the previous chunk has been read
    for (int e = tid; e < FC_TE * FC_KC; e += WAVES * 64) {
      const int row = e / FC_KC, j = e - row * FC_KC;
      float x = 0.0f;
      if (env0 + row < p.N && j < kc) x = p.flat[(size_t)(env0 + row) * p.K + k0 + j];
      xs[row * FC_S + j] = x;
    }
    __syncthreads();
    for (int kb = 0; kb < kc; kb += 16) {
      const f32x4 a = *reinterpret_cast<const f32x4*>(xs + r * FC_S + kb + 4 * kh);
#pragma unroll
      for (int j = 0; j < FC_GROUPS; j++) {
        const int g = wave + WAVES * j;
        if (g < ngroups)  // (uniform over the wavefront)
          act::tile_pair_k16(a, p.W + (size_t)(k0 + kb + 4 * kh) * p.Fp + g * 32 + 2 * r, p.Fp, acc[j][0], acc[j][1]);
      }
    }
  }
  // D: column = the lane's column pair, row (env) = 4 (lane >> 4) + register
#pragma unroll
  for (int j = 0; j < FC_GROUPS; j++) {
    const int c = (wave + WAVES * j) * 32 + 2 * r;
#pragma unroll
    for (int q = 0; q < 4; q++) {
      const int i = env0 + 4 * kh + q;
      if (i < p.N) {
        if (c < p.F) p.out[(size_t)i * p.F + c] = fmaxf(acc[j][0][q], 0.0f);
        if (c + 1 < p.F) p.out[(size_t)i * p.F + c + 1] = fmaxf(acc[j][1][q], 0.0f);
      }
    }
  }
}

// torch.nn.Conv2d parameters (weight [out, in, kh, kw], bias [out]) -> the packed copy dst_w [k][out], k = (ky KW + kx) CIN + c
struct PackConvParams {
  const float *w, *b;
  int cout, cin, kh, kw;
  float *dst_w, *dst_b;
};
__global__ __launch_bounds__(256) void pack_conv_kernel(PackConvParams p) {
  const int e = blockIdx.x * blockDim.x + threadIdx.x;
  const int K = p.kh * p.kw * p.cin;
  if (e >= K * p.cout) return;
  const int k = e / p.cout, o = e - k * p.cout;
  const int tap = k / p.cin, c = k - tap * p.cin, ky = tap / p.kw, kx = tap - ky * p.kw;
  p.dst_w[e] = p.w[(((size_t)o * p.cin + c) * p.kh + ky) * p.kw + kx];
  if (k == 0) p.dst_b[o] = p.b[o];
}

}  // namespace enc
