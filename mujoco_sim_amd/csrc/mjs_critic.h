// mjs_critic.h — SAC's critics (stable_baselines3/common/policies.py ContinuousCritic: n_critics MLPs over [obs | action] with a scalar
// head) and the no-gradient half of SAC.train (stable_baselines3/sac/sac.py) as ONE launch each, on the float32 batch a replay buffer
// hands out (mjs_replay.h):
//   q_kernel           q[c, i] = Q_c(obs[i], action[i])
//   td_target_kernel   a', logp' = actor.action_log_prob(next_obs);  y = r + (1 - done) * gamma * (min_c Q_c(next_obs, a') - ent_coef * logp')
//   pack_lerp_kernel   SB3's polyak_update, straight into a packed parameter copy
//
// float32 with float32 accumulation, the actor's contract (mjs_actor.h): every layer is act::layer<16, ...>, so an output element is an
// fmaf chain over k that starts at the bias, on v_mfma_f32_16x16x4_f32. A workgroup owns 16 batch rows, its WAVES wavefronts the 32-wide
// output groups of a layer. Three LDS images [row][S] of one stride S = act::lds_stride(the widest of the critic's padded input, the
// actor's layers and the critic's layers):
//   X     the input image [obs row | action row], zero in the k padding and in the rows past B. No layer ever writes it, so in
//         td_target_kernel the next_obs columns the actor's first layer read are still there when the critics run: the obs part is
//         KEPT in this third image, not gathered again from global memory (a second gather would cost every critic a global round trip
//         for 16 x D floats that are already in LDS; the image costs 16 S floats of an LDS budget that three images do not fill);
//   P, Q  the activations, ping-pong; a network's head lands in whichever of the two its last hidden layer did not write.
// act::forward is not called: it owns two images and overwrites its input, and its tail is the env-action unscale. mlp() below is the
// layer sequence alone, used for the actor and for every critic. Packed parameters are act::pack_kernel's layout ([k][out], zero-padded
// to KPAD in k and OPAD in out); the critics' head is one output column padded to OPAD. No atomics, no local arrays, no inline assembly.
#pragma once
#include "mjs_actor.h"

namespace crit {

constexpr int MAX_OBS = 64, MAX_ACT = act::MAX_ACT, MAX_CRITICS = 2;
constexpr int MAX_K0 = act::round_up(MAX_OBS + MAX_ACT, act::KPAD);  // 80: above act::MAX_IN
constexpr int ROWS = 16;                                             // batch rows per workgroup
constexpr float LOG_PROB_EPS = 1e-6f;                                // SquashedDiagGaussianDistribution(epsilon=1e-6)
constexpr float HALF_LOG_2PI = 0.918938533204672742f;                // 0.5 * log(2 pi)
constexpr size_t lds_bytes(int widest) { return (size_t)3 * ROWS * act::lds_stride(widest) * sizeof(float); }

// One network's packed copy: hidden layers (unused ones nullptr / 0) and the head [k][OPAD]
struct Mlp {
  const float *W0, *W1, *W2, *WH;
  const float *B0, *B1, *B2, *BH;
  int n_hidden;    // 1..3
  int k0;          // the first layer's fan-in padded to KPAD
  int w0, w1, w2;  // hidden widths padded to OPAD
  int activation;  // act::ACT_*
};

// The layers of `m` over the image X for the calling workgroup; returns the image (P or Q) that holds the head's OPAD raw sums per
// row. Ends behind a barrier. X is only read.
__device__ __forceinline__ const float* mlp(const Mlp& m, const float* X, float* P, float* Q, int S, int wave, int lane) {
  act::layer<ROWS, true>(X, P, S, m.W0, m.B0, m.k0, m.w0, m.activation, wave, lane);
  __syncthreads();
  const float* h = P;
  float* other = Q;
  int K = m.w0;
  if (m.n_hidden > 1) {
    act::layer<ROWS, true>(P, Q, S, m.W1, m.B1, m.w0, m.w1, m.activation, wave, lane);
    __syncthreads();
    h = Q; other = P; K = m.w1;
    if (m.n_hidden > 2) {
      act::layer<ROWS, true>(Q, P, S, m.W2, m.B2, m.w1, m.w2, m.activation, wave, lane);
      __syncthreads();
      h = P; other = Q; K = m.w2;
    }
  }
  act::layer<ROWS, false>(h, other, S, m.WH, m.BH, K, act::OPAD, m.activation, wave, lane);
  __syncthreads();
  return other;
}

struct CriticParams {
  int B;
  int D, A;       // obs and action width; the input image holds D + A columns, zero up to net[].k0
  int n_critics;  // 1..MAX_CRITICS
  int S;          // stride of the three images
  Mlp net[MAX_CRITICS];
};

// Every critic over the image X, in turn: sink(c, r, q) is called by thread r < ROWS with Q_c of the workgroup's row r. The one
// function q_kernel and td_target_kernel share, so that both sum in the same order. (net[] is indexed by constants only.)
template <class Sink>
__device__ __forceinline__ void critics(const CriticParams& p, const float* X, float* P, float* Q, int tid, Sink sink) {
  const int wave = tid >> 6, lane = tid & 63;
#pragma unroll
  for (int c = 0; c < MAX_CRITICS; c++) {
    if (c < p.n_critics) {
      const float* head = mlp(p.net[c], X, P, Q, p.S, wave, lane);
      if (tid < ROWS) sink(c, tid, head[tid * p.S]);
      __syncthreads();  // the next critic's first layer writes P
    }
  }
}

// The input image: gather(i, j) is column j < D + A of batch row i < B; the rest of the k0 columns and of the ROWS rows is zero.
template <class Gather>
__device__ __forceinline__ void fill_input(float* X, int S, int k0, int cols, int row0, int B, int tid, Gather gather) {
  for (int e = tid; e < ROWS * k0; e += act::WAVES * 64) {
    const int r = e / k0, j = e - r * k0;
    float x = 0.0f;
    if (row0 + r < B && j < cols) x = gather(row0 + r, j);
    X[r * S + j] = x;
  }
}

// grid = ceil(B / ROWS) workgroups of WAVES wavefronts; dynamic LDS = lds_bytes(widest)
__global__ __launch_bounds__(act::WAVES * 64) void q_kernel(CriticParams p, const float* __restrict__ obs, const float* __restrict__ actions, float* __restrict__ q) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  float* X = lds;
  float* P = lds + ROWS * p.S;
  float* Q = lds + 2 * ROWS * p.S;
  const int tid = threadIdx.x, row0 = blockIdx.x * ROWS;
  fill_input(X, p.S, p.net[0].k0, p.D + p.A, row0, p.B, tid,
             [&](int i, int j) { return j < p.D ? obs[(size_t)i * p.D + j] : actions[(size_t)i * p.A + (j - p.D)]; });
  __syncthreads();
  critics(p, X, P, Q, tid, [&](int c, int r, float v) {
    if (row0 + r < p.B) q[(size_t)c * p.B + row0 + r] = v;
  });
}

// One component of SB3's actor.action_log_prob for the clamped log_std ls and the draw zj: returns a = tanhf(mu + expf(ls) zj), and the
// component's two log-probability terms. What td_target_kernel and atrain::grad_kernel (mjs_actor_train.h) share, so that both give the
// same bits.
__device__ __forceinline__ float squashed_sample(float mu, float ls, float zj, float& gauss, float& corr) {
  const float a = tanhf(mu + expf(ls) * zj);
  {
    // Normal(mu, exp(ls)).log_prob(u) at u = mu + exp(ls) z, and the squash correction, operation by operation
#pragma clang fp contract(off)
    const float zz = zj * zj;
    const float h = -0.5f * zz;
    const float hl = h - ls;
    gauss = hl - HALF_LOG_2PI;
    const float aa = a * a;
    const float one = 1.0f - aa;
    corr = logf(one + LOG_PROB_EPS);
  }
  return a;
}

struct TdParams {
  CriticParams c;
  Mlp actor;                    // k0 = D padded to KPAD (<= the critics' k0); its head: mu in columns 0..A-1, log_std in A..2A-1
  const float* next_obs;        // [B, D]
  const float* rewards;         // [B]
  const float* dones;           // [B]
  const float* z;               // [B, A]
  float gamma, ent_coef;
  const float* ent_coef_dev;    // one float, read instead of ent_coef where non-null
  float* target;                // [B]
  float* next_actions;          // [B, A] or nullptr
  float* next_log_prob;         // [B] or nullptr
  float* q_next;                // [n_critics, B] or nullptr
};

__global__ __launch_bounds__(act::WAVES * 64) void td_target_kernel(TdParams p) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  const int S = p.c.S, D = p.c.D, A = p.c.A, B = p.c.B;
  float* X = lds;
  float* P = lds + ROWS * S;
  float* Q = lds + 2 * ROWS * S;
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, row0 = blockIdx.x * ROWS;

  // 1. the actor on next_obs: the batch's columns are its inputs, in order. The image is zeroed up to the critics' k0 already.
  fill_input(X, S, p.c.net[0].k0, D, row0, B, tid, [&](int i, int j) { return p.next_obs[(size_t)i * D + j]; });
  __syncthreads();
  // (the head image is written by mlp() and, in its columns past 2 A <= 16, by the threads below: P or Q, not const here)
  float* head = const_cast<float*>(mlp(p.actor, X, P, Q, S, wave, lane));

  // 2. one thread per (row, component): the squashed sample into the critics' input image, and the component's two log-probability
  // terms into the head image's spare columns 16 + j and 24 + j (the head's own 2 A <= 16 columns come first)
  if (tid < ROWS * A) {
    const int r = tid / A, j = tid - r * A, i = row0 + r;
    float a = 0.0f, gauss = 0.0f, corr = 0.0f;  // rows past B stay zero in X
    if (i < B) {
      const float mu = head[r * S + j];
      const float ls = fminf(fmaxf(head[r * S + A + j], act::LOG_STD_MIN), act::LOG_STD_MAX);
      const float zj = p.z[(size_t)i * A + j];
      a = squashed_sample(mu, ls, zj, gauss, corr);
      if (p.next_actions) p.next_actions[(size_t)i * A + j] = a;
    }
    X[r * S + D + j] = a;
    head[r * S + 16 + j] = gauss;
    head[r * S + 24 + j] = corr;
  }
  __syncthreads();

  // 3. one thread per row: both sums run over j = 0..A-1 in order, each from 0.0f; logp = (sum of the Gaussian terms) - (sum of the
  // correction terms), ONE subtraction after both sums are complete (SB3: log_prob = sum(...); log_prob -= sum(log(1 - a^2 + eps)))
  float logp = 0.0f;
  if (tid < ROWS) {
    float sg = 0.0f, sc = 0.0f;
    for (int j = 0; j < A; j++) {
      sg += head[tid * S + 16 + j];
      sc += head[tid * S + 24 + j];
    }
    logp = sg - sc;
    if (row0 + tid < B && p.next_log_prob) p.next_log_prob[row0 + tid] = logp;
  }
  __syncthreads();  // the critics' first layer writes P, which may be the head image

  // 4.-6. the critics over [next_obs | a'], exactly as in q_kernel; qn = min over the critics, in thread r of the workgroup's row r
  float qn = 0.0f;
  critics(p.c, X, P, Q, tid, [&](int c, int r, float v) {
    if (row0 + r < B && p.q_next) p.q_next[(size_t)c * B + row0 + r] = v;
    qn = c == 0 ? v : fminf(qn, v);
  });

  // 7. y = r + (1 - done) * gamma * (qn - ent_coef * logp), operation by operation in this order
  if (tid < ROWS && row0 + tid < B) {
    const int i = row0 + tid;
    const float ent = p.ent_coef_dev ? *p.ent_coef_dev : p.ent_coef;
    const float rew = p.rewards[i], done = p.dones[i];
    {
#pragma clang fp contract(off)
      const float keep = 1.0f - done;
      const float disc = keep * p.gamma;
      const float el = ent * logp;
      const float soft = qn - el;
      const float boot = disc * soft;
      p.target[i] = rew + boot;
    }
  }
}

// act::pack_kernel with a blend, for one source: the real elements of the packed copy become (1 - tau) * dst + tau * src, computed as
// fmaf(tau, src, one_minus_tau * dst) (two roundings; the two coefficients are rounded to float32 on the host); the padding is
// written 0 as act::pack_kernel writes it. tau == 1 never comes here: mjs_critic_load launches act::pack_kernel then, which does not
// read dst (a first load's dst is uninitialised memory).
__global__ __launch_bounds__(256) void pack_lerp_kernel(act::PackParams p, float one_minus_tau, float tau) {
  const int e = blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= p.K * p.O) return;
  const int k = e / p.O, o = e - k * p.O;
  const bool real = o < p.out0;
  float w = 0.0f;
  if (real && k < p.in) w = fmaf(tau, p.w0[(size_t)o * p.in + k], one_minus_tau * p.dst_w[e]);
  p.dst_w[e] = w;
  if (k == 0) p.dst_b[o] = real ? fmaf(tau, p.b0[o], one_minus_tau * p.dst_b[o]) : 0.0f;
}

}  // namespace crit
