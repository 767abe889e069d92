// mjs_encoder_train.h — the backward pass of mjs_encoder.h's NatureCNN on the encoder's packed copy, which becomes the master copy:
// from uint8 frames rgb [n, H, W, 3] and an upstream gradient dfeatures [n, F], the gradient of sum(features * dfeatures) with respect
// to the eight parameter tensors - what features.backward(dfeatures) gives in torch. No gradient with respect to the image.
//
//   forward_kernel   enc::convs<true>: conv_kernel's body with the LDS images of conv1 [n, P1, 32] and conv2 [n, P2, 64] stored next to
//                    `flat`; enc::fc_kernel follows unchanged, so the features are mjs_encoder_features' bit for bit
//   fc_bwd_kernel    Gf = dfeatures * (features > 0), padded to Fp;  dflat = Gf W_fc^T over 16-image tiles (crit::input_grad's operand
//                    layout: 4 consecutive outputs of a row of Gf from LDS, of a row of the packed W from L2);  dZ3 = dflat * (flat > 0)
//                    written position-major [n, P3, 64] (flat is CHW)
//   dgrad_kernel     one workgroup per image. The data gradient of conv3 and of conv2 as a GATHER: rows = 16 input positions, columns =
//                    input channels, the reduction over (ky, kx, out): for every tap the input position's output position, where it
//                    exists ((y - ky) a multiple of the stride and inside), is ONE 16-byte LDS read of dZ [position][68 floats]; a tap
//                    no lane of the tile has is skipped. dZ2 = (.) * (a2 > 0) goes to LDS and to global, dZ1 = (.) * (a1 > 0) to global
//   wgrad_kernel     dW[k][o] = sum over (image, position) patch[k] dZ[o] for one layer: grid (split, k block of 64, o block of 32), a
//                    wavefront owns a 16 x 32 piece of dW as two accumulators and walks its split's images in order, 16 positions per
//                    step (act::tile_pair_k16 with the positions as the MFMA's k). conv1's patches are read from the uint8 image through
//                    the forward's table of exact quotients i / 255.0f. The bias gradient is the same product against a column of ones
//                    (wavefront 0 of k block 0). For the linear layer the "positions" are the split's images.
//   unpack_conv_kernel  packed [k][out] -> torch.nn.Conv2d layout (enc::pack_conv_kernel's inverse)
// Adam, the slab sum, the blend and the linear layer's unpack are crit::adam_kernel, slab_sum_kernel, blend_kernel and unpack_kernel,
// unchanged, over a crit::Layout whose eight segments are conv1..3 and fc (weights, bias).
//
// float32 with float32 accumulation on v_mfma_f32_16x16x4_f32, every accumulator from 0. ReLU's derivative is 1 where the STORED
// activation is > 0 and 0 otherwise (torch's rule). Zero padding is exact: a position past the image's last has dZ = 0 (its patch is read
// from the last position and is finite), the padded outputs of fc have Gf = 0.
//
// The sums over the batch are bitwise reproducible, with no atomics: split s owns the contiguous images [s * images_per_split,
// (s + 1) * images_per_split) and one slab (crit::Layout), every element of which it stores once; the consumer sums the slabs in order.
// split_rule() is a function of n and the shape alone.
//
// LDS: forward_kernel as conv_kernel; dgrad_kernel (P3 + P2) x 68 floats (44.6 KB at 96x96); fc_bwd_kernel 16 x 516 floats;
// wgrad_kernel the 1 KB table. No atomics, no inline assembly, no run-time-indexed local arrays.
#pragma once
#include "mjs_critic_train.h"
#include "mjs_encoder.h"

namespace enct {

using act::BColumnPair;
using act::f32x4;
using enc::WAVES;

constexpr int MAX_SPLITS = 64;                       // slabs, at most
constexpr size_t SLAB_CAP = (size_t)128 << 20;       // bytes of slabs, at most (where one slab fits)
constexpr int ZS = enc::C2 + 4;                      // LDS floats per position of a dZ image (conv3's and conv2's outputs: 64 channels)
static_assert(enc::C2 == enc::C3, "one stride for both dZ images");
constexpr int KBLOCK = 16 * WAVES, OBLOCK = 32;      // a wgrad workgroup's piece of dW
constexpr int FCB_KBLOCK = 32 * WAVES;               // a fc_bwd workgroup's piece of flat's width

// images_per_split = ceil(n / splits_max), splits_max = min(MAX_SPLITS, max(1, SLAB_CAP / slab bytes)); splits = ceil(n / images_per_split)
struct Split {
  int images_per_split, splits;
};
inline int splits_max(int slab_floats) {
  const long long cap = (long long)(SLAB_CAP / ((size_t)slab_floats * sizeof(float)));
  return cap < 1 ? 1 : cap > MAX_SPLITS ? MAX_SPLITS : (int)cap;
}
inline Split split_rule(int n, int slab_floats) {
  const int cap = splits_max(slab_floats);
  const int ips = n < 1 ? 1 : (n + cap - 1) / cap;
  return {ips, n < 1 ? 1 : (n + ips - 1) / ips};
}

// The caller's workspace, in floats from its start (every block a multiple of 4 floats: 16-byte aligned where the workspace is)
struct Workspace {
  size_t a1, a2, flat, feat, gf, dz3, dz2, dz1, slabs, total;
};
inline Workspace workspace(const enc::Geometry& g, int F, int Fp, int n, int splits, int slab_floats) {
  const size_t N = (size_t)n, P1 = (size_t)g.H1 * g.W1, P2 = (size_t)g.H2 * g.W2;
  Workspace w;
  w.a1 = 0;
  w.a2 = w.a1 + N * P1 * enc::C1;
  w.flat = w.a2 + N * P2 * enc::C2;
  w.feat = w.flat + N * g.n_flatten;
  w.gf = w.feat + (N * F + 3) / 4 * 4;
  w.dz3 = w.gf + N * Fp;
  w.dz2 = w.dz3 + N * g.n_flatten;
  w.dz1 = w.dz2 + N * P2 * enc::C2;
  w.slabs = w.dz1 + N * P1 * enc::C1;
  w.total = w.slabs + (size_t)splits * slab_floats;
  return w;
}

struct ForwardParams {
  enc::ConvParams c;
  float *a1, *a2;  // [N, P1, 32], [N, P2, 64]
};
// grid = N workgroups of WAVES wavefronts; dynamic LDS = enc::lds_bytes(geometry)
__global__ __launch_bounds__(WAVES * 64) void forward_kernel(ForwardParams p) { enc::convs<true>(p.c, p.a1, p.a2); }

struct FcBwdParams {
  int N, K, F, Fp, P3;     // K = n_flatten = 64 P3
  const float* dfeatures;  // [N, F]
  const float* features;   // [N, F]
  const float* flat;       // [N, K], CHW
  const float* W;          // packed [K][Fp]
  float* gf;               // [N, Fp]
  float* dz3;              // [N, P3, 64]
};
// grid = (ceil(N / 16), ceil(K / 128)) workgroups of WAVES wavefronts; wavefront w owns the 32 k from 128 blockIdx.y + 32 w
__global__ __launch_bounds__(WAVES * 64) void fc_bwd_kernel(FcBwdParams p) {
  __shared__ __attribute__((aligned(16))) float gs[enc::FC_TE * (enc::MAX_F + 4)];
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const int r = lane & 15, kh = lane >> 4;
  const int env0 = blockIdx.x * enc::FC_TE, S = p.Fp + 4;
  for (int e = tid; e < enc::FC_TE * p.Fp; e += WAVES * 64) {
    const int row = e / p.Fp, o = e - row * p.Fp, i = env0 + row;
    float g = 0.0f;
    if (i < p.N && o < p.F) {
      const size_t at = (size_t)i * p.F + o;
      g = p.features[at] > 0.0f ? p.dfeatures[at] : 0.0f;
    }
    gs[row * S + o] = g;
    if (blockIdx.y == 0 && i < p.N) p.gf[(size_t)i * p.Fp + o] = g;
  }
  __syncthreads();
  const int k0 = blockIdx.y * FCB_KBLOCK + wave * 32 + 2 * r;  // the lane's column pair k0, k0 + 1
  if (k0 - 2 * r >= p.K) return;                                // (uniform over the wavefront; K is a multiple of 64)
  const float* grow = gs + r * S + 4 * kh;
  const float* w0 = p.W + (size_t)k0 * p.Fp + 4 * kh;
  const float* w1 = w0 + p.Fp;
  f32x4 acc0 = {0.0f, 0.0f, 0.0f, 0.0f}, acc1 = {0.0f, 0.0f, 0.0f, 0.0f};
  for (int ob = 0; ob < p.Fp; ob += 16) {
    const f32x4 a = *reinterpret_cast<const f32x4*>(grow + ob);
    const f32x4 b0 = *reinterpret_cast<const f32x4*>(w0 + ob), b1 = *reinterpret_cast<const f32x4*>(w1 + ob);
    const BColumnPair b = {{{b0[0], b1[0]}, {b0[1], b1[1]}, {b0[2], b1[2]}, {b0[3], b1[3]}}};
    act::tile_pair_k16(a, b, acc0, acc1);
  }
  // D: column = the lane's k pair, row (image) = 4 (lane >> 4) + register; k = c P3 + pos
#pragma unroll
  for (int q = 0; q < 4; q++) {
    const int i = env0 + 4 * kh + q;
    if (i < p.N) {
#pragma unroll
      for (int h = 0; h < 2; h++) {
        const int k = k0 + h, c = k / p.P3, pos = k - c * p.P3;
        const float d = h ? acc1[q] : acc0[q];
        p.dz3[((size_t)i * p.P3 + pos) * enc::C3 + c] = p.flat[(size_t)i * p.K + k] > 0.0f ? d : 0.0f;
      }
    }
  }
}

// The data gradient of one convolution for the calling wavefront: dZ [Hout Wout][ZS] (LDS) -> (sum over taps and outputs) * (mask > 0)
// for the Hin x Win input positions, into outL [position][ZS] (LDS_OUT) and outG [position][CIN]. Wt packed [k][COUT], k = (ky KW + kx) CIN + c.
template <int KH, int KW, int STRIDE, int CIN, int COUT, bool LDS_OUT>
__device__ __forceinline__ void dgrad(const float* dZ, int Hout, int Wout, int Hin, int Win, const float* __restrict__ Wt, const float* __restrict__ mask,
                                      float* outL, float* __restrict__ outG, int wave, int lane) {
  static_assert(CIN % 32 == 0 && COUT % 16 == 0 && (STRIDE & (STRIDE - 1)) == 0, "32-wide channel groups, 16 outputs per step");
  constexpr int NG = CIN / 32, SHIFT = STRIDE == 1 ? 0 : STRIDE == 2 ? 1 : 2;
  const int r = lane & 15, kh = lane >> 4;
  const int Pin = Hin * Win, ntiles = (Pin + 15) >> 4;
  for (int it = wave; it < ntiles * NG; it += WAVES) {
    const int tile = it / NG, g = it - tile * NG, c = g * 32 + 2 * r;
    const int prow = tile * 16 + r;  // the lane's A row; rows past Pin take no tap
    const int pc = prow < Pin ? prow : Pin - 1;
    const int y = pc / Win, x = pc - y * Win;
    f32x4 acc0 = {0.0f, 0.0f, 0.0f, 0.0f}, acc1 = {0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll 1
    for (int tap = 0; tap < KH * KW; tap++) {
      const int ky = tap / KW, kx = tap - ky * KW;
      const int ty = y - ky, tx = x - kx;
      const int oy = ty >> SHIFT, ox = tx >> SHIFT;
      const bool valid = prow < Pin && ty >= 0 && tx >= 0 && (ty & (STRIDE - 1)) == 0 && (tx & (STRIDE - 1)) == 0 && oy < Hout && ox < Wout;
      if (__ballot(valid) == 0) continue;  // (uniform over the wavefront)
      const float* zrow = dZ + (valid ? oy * Wout + ox : 0) * ZS + 4 * kh;
      const float* w0 = Wt + ((size_t)tap * CIN + c) * COUT + 4 * kh;
      const float* w1 = w0 + COUT;
#pragma unroll
      for (int ob = 0; ob < COUT; ob += 16) {
        f32x4 a = *reinterpret_cast<const f32x4*>(zrow + ob);
        if (!valid) a = f32x4{0.0f, 0.0f, 0.0f, 0.0f};
        const f32x4 b0 = *reinterpret_cast<const f32x4*>(w0 + ob), b1 = *reinterpret_cast<const f32x4*>(w1 + ob);
        const BColumnPair b = {{{b0[0], b1[0]}, {b0[1], b1[1]}, {b0[2], b1[2]}, {b0[3], b1[3]}}};
        act::tile_pair_k16(a, b, acc0, acc1);
      }
    }
    // D: column = the lane's channel pair, row (position) = 4 (lane >> 4) + register
#pragma unroll
    for (int q = 0; q < 4; q++) {
      const int pos = tile * 16 + 4 * kh + q;
      if (pos < Pin) {
        const float2 m = *reinterpret_cast<const float2*>(mask + (size_t)pos * CIN + c);
        const float2 d = {m.x > 0.0f ? acc0[q] : 0.0f, m.y > 0.0f ? acc1[q] : 0.0f};
        if (LDS_OUT) *reinterpret_cast<float2*>(outL + pos * ZS + c) = d;
        *reinterpret_cast<float2*>(outG + (size_t)pos * CIN + c) = d;
      }
    }
  }
}

struct DgradParams {
  int N;
  enc::Geometry g;
  const float *W2, *W3;  // packed [k][64]
  const float *a1, *a2;  // the stored activations
  const float* dz3;      // [N, P3, 64]
  float* dz2;            // [N, P2, 64]
  float* dz1;            // [N, P1, 32]
};
constexpr size_t dgrad_lds_bytes(const enc::Geometry& g) { return sizeof(float) * ZS * ((size_t)g.H3 * g.W3 + (size_t)g.H2 * g.W2); }
static_assert(dgrad_lds_bytes(enc::geometry(enc::MAX_HW, enc::MAX_HW)) <= 64 * 1024, "the two dZ images need no LDS opt-in");

// grid = N workgroups of WAVES wavefronts; dynamic LDS = dgrad_lds_bytes(geometry)
__global__ __launch_bounds__(WAVES * 64) void dgrad_kernel(DgradParams p) {
  extern __shared__ __attribute__((aligned(16))) unsigned char enc_lds[];
  const enc::Geometry& g = p.g;
  const int P1 = g.H1 * g.W1, P2 = g.H2 * g.W2, P3 = g.H3 * g.W3;
  float* z3 = reinterpret_cast<float*>(enc_lds);
  float* z2 = z3 + P3 * ZS;
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const int img = blockIdx.x;
  if (img >= p.N) return;  // (uniform over the workgroup)
  const float* src = p.dz3 + (size_t)img * P3 * enc::C3;
  for (int e = tid; e < P3 * (enc::C3 / 4); e += WAVES * 64) {
    const int pos = e / (enc::C3 / 4), j = e - pos * (enc::C3 / 4);
    *reinterpret_cast<f32x4*>(z3 + pos * ZS + 4 * j) = *reinterpret_cast<const f32x4*>(src + (size_t)e * 4);
  }
  __syncthreads();
  dgrad<3, 3, 1, enc::C2, enc::C3, true>(z3, g.H3, g.W3, g.H2, g.W2, p.W3, p.a2 + (size_t)img * P2 * enc::C2, z2, p.dz2 + (size_t)img * P2 * enc::C2, wave, lane);
  __syncthreads();
  dgrad<4, 4, 2, enc::C1, enc::C2, false>(z2, g.H2, g.W2, g.H1, g.W1, p.W2, p.a1 + (size_t)img * P1 * enc::C1, nullptr, p.dz1 + (size_t)img * P1 * enc::C1, wave, lane);
}

enum { SRC_IMAGE = 0, SRC_ACT = 1, SRC_FLAT = 2 };
struct WgradParams {
  int n, images_per_split;
  int P, Wout;         // output positions per image and the output's width (SRC_FLAT: unused)
  int Pin, Win;        // input positions per image and the input's width
  int K, O;            // dW is [K][O]; O is also dZ's row stride
  const uint8_t* rgb;  // SRC_IMAGE: [n, H, W, 3]
  const float* X;      // SRC_ACT: [n, Pin, CIN]; SRC_FLAT: [n, K]
  const float* G;      // dZ [n P][O] (SRC_FLAT: Gf [n][O])
  float *dW, *dB;      // split 0's segments; split s at + s * slab_stride
  size_t slab_stride;
};

// grid = (splits, ceil(K / 64), O / 32) workgroups of WAVES wavefronts. Wavefront w owns dW[kb .. kb + 15][ob .. ob + 31], kb = 64 blockIdx.y
// + 16 w, ob = 32 blockIdx.z. MFMA operands: A[i = k][kk = position] = the patch value, B[kk = position][j = o] = dZ; instruction s of a
// step adds positions 4 s .. 4 s + 3 of the step's 16, so an element's sum runs over its split's (image, position) pairs in order.
template <int SRC, int KH, int KW, int STRIDE, int CIN>
__global__ __launch_bounds__(WAVES * 64) void wgrad_kernel(WgradParams p) {
  __shared__ float lut[256];
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  if (SRC == SRC_IMAGE) {
    lut[tid] = (float)tid / 255.0f;  // enc::convs' table
    __syncthreads();
  }
  const int r = lane & 15, kh = lane >> 4;
  const int split = blockIdx.x, kb = (blockIdx.y * WAVES + wave) * 16, ob = blockIdx.z * OBLOCK;
  const int i0 = split * p.images_per_split;
  const int i1 = i0 + p.images_per_split < p.n ? i0 + p.images_per_split : p.n;
  // SRC_FLAT: one unit whose rows are the split's images; otherwise one unit per image, its rows the output positions
  const int units = SRC == SRC_FLAT ? 1 : i1 - i0, rows = SRC == SRC_FLAT ? i1 - i0 : p.P;
  const bool bias_wave = blockIdx.y == 0 && wave == 0;
  if (kb >= p.K && !bias_wave) return;  // (uniform over the wavefront)
  const int k = kb + r;
  int koff = k;
  if (SRC != SRC_FLAT) {
    const int tap = k / CIN, c = k - tap * CIN, ky = tap / KW, kx = tap - ky * KW;
    koff = (ky * p.Win + kx) * CIN + c;
  }
  const size_t unit_stride = SRC == SRC_FLAT ? 0 : (size_t)p.Pin * CIN;
  float* dW = p.dW + (size_t)split * p.slab_stride;
  float* dB = p.dB + (size_t)split * p.slab_stride;
  for (int pass = 0; pass < 2; pass++) {  // 0: the wavefront's piece of dW; 1: the bias gradient (bias_wave)
    if (pass == 0 ? kb >= p.K : !bias_wave) continue;
    f32x4 acc0 = {0.0f, 0.0f, 0.0f, 0.0f}, acc1 = {0.0f, 0.0f, 0.0f, 0.0f};
    for (int u = 0; u < units; u++) {
      const size_t ubase = (size_t)(i0 + u) * unit_stride;
      const float* G = p.G + ((size_t)i0 * (SRC == SRC_FLAT ? 1 : p.P) + (size_t)u * rows) * p.O + ob + 2 * r;
      for (int r0 = 0; r0 < rows; r0 += 16) {
        f32x4 a;
        BColumnPair b;
#pragma unroll
        for (int s = 0; s < 4; s++) {
          const int row = r0 + 4 * s + kh;
          const bool valid = row < rows;
          const int rc = valid ? row : rows - 1;  // a finite operand for the rows past the end; their dZ is 0
          if (pass == 1) {
            a[s] = r == 0 ? 1.0f : 0.0f;
          } else if (SRC == SRC_FLAT) {
            a[s] = p.X[(size_t)(i0 + rc) * p.K + koff];
          } else {
            const int oy = rc / p.Wout, ox = rc - oy * p.Wout;
            const size_t at = ubase + (size_t)((oy * STRIDE * p.Win + ox * STRIDE) * CIN + koff);
            a[s] = SRC == SRC_IMAGE ? lut[p.rgb[at]] : p.X[at];
          }
          const float2 g = *reinterpret_cast<const float2*>(G + (size_t)rc * p.O);
          b.k[s] = valid ? g : float2{0.0f, 0.0f};
        }
        act::tile_pair_k16(a, b, acc0, acc1);
      }
    }
    // D: column = the lane's o pair, row (k) = 4 (lane >> 4) + register
    if (pass == 0) {
#pragma unroll
      for (int q = 0; q < 4; q++) *reinterpret_cast<float2*>(dW + (size_t)(kb + 4 * kh + q) * p.O + ob + 2 * r) = float2{acc0[q], acc1[q]};
    } else if (kh == 0) {
      *reinterpret_cast<float2*>(dB + ob + 2 * r) = float2{acc0[0], acc1[0]};
    }
  }
}

// the packed copy dst_w [k][out], k = (ky KW + kx) CIN + c -> torch.nn.Conv2d layout (weight [out, in, kh, kw], bias [out]);
// grid = ceil(K * cout / 256)
struct UnpackConvParams {
  const float *src_w, *src_b;
  int cout, cin, kh, kw;
  float *dst_w, *dst_b;
};
__global__ __launch_bounds__(256) void unpack_conv_kernel(UnpackConvParams p) {
  const int e = blockIdx.x * blockDim.x + threadIdx.x;
  const int K = p.kh * p.kw * p.cin;
  if (e >= K * p.cout) return;
  const int k = e / p.cout, o = e - k * p.cout;
  const int tap = k / p.cin, c = k - tap * p.cin, ky = tap / p.kw, kx = tap - ky * p.kw;
  p.dst_w[(((size_t)o * p.cin + c) * p.kh + ky) * p.kw + kx] = p.src_w[e];
  if (k == 0) p.dst_b[o] = p.src_b[o];
}

}  // namespace enct
