// mjs_actor_train.h — the actor half of a SAC gradient step (stable_baselines3/sac/sac.py SAC.train) on the packed parameter copy of
// mjs_actor.h, which becomes the master copy, and the learned entropy coefficient:
//   grad_kernel   a, logp = actor.action_log_prob(obs); q_c = Q_c(obs, a); actor_loss = mean(ent_coef * logp - min_c q_c); the gradient
//                 of actor_loss for every layer's weight and bias of the ACTOR, as one partial slab per split, through the twin critics
//                 (dQ/da; the critics' parameter gradients are not computed)
//   ent_kernel    ent_coef_loss = -(log_ent_coef * (logp + target_entropy)).mean(): one thread, Adam on the scalar, ent_coef = expf(it)
// Adam on the actor is crit::adam_kernel over the actor's slabs (n_critics = 1, the stacked mu / log_std head in slot 3), the summed
// gradient alone crit::slab_sum_kernel, the way back into torch.nn.Linear layout crit::unpack_kernel.
//
// ONE launch for the gradient. A workgroup of act::WAVES wavefronts owns contiguous 16-row tiles (crit::split_rule over the actor's slab
// size). float32 with float32 accumulation on v_mfma_f32_16x16x4_f32; every forward layer is act::layer<16>. Per tile:
//   1. the actor over obs (the batch's columns are its inputs in order, as in td_target_kernel), every hidden activation image kept;
//   2. a and logp as td_target_kernel computes a' and logp (crit::squashed_sample, the same sums); a lands in the critics' input image
//      [obs | a];
//   3. with two critics: critic 0 forward for q_0 alone (crit::mlp on the gradient pair), so that the argmin is known before either
//      backward pass. Ties go to critic 0: critic 1 is the argmin only where q_1 < q_0;
//   4. per critic, 1 first, then 0: forward with every image kept (for critic 0 a second time: the same bits), the head's dZ = 1 in
//      column 0 on the rows (below B) where this critic is the argmin, 0 elsewhere, crit::input_grad down the hidden layers, and the
//      action columns of the first layer's input gradient (action_grad: the one product mjs_critic_train.h never computes),
//        dX[r][D + j] = sum_o dZ0[r][o] W0[D + j][o]   as 16x16 tiles of (r, k) over the at most two 16-k tiles that hold D..D+A-1, o
//                                                     as the MFMA's k from 0 upwards, exactly as input_grad sums;
//      q_c is what crit::critics() gives (q_pi == mjs_critic_q(obs, a) bit for bit);
//   5. the tail, one thread per (row, component j), one operation per line, no contraction, alpha = ent_coef, in this order:
//        dq  = dX_0[D + j] + dX_1[D + j]              critic order 0, 1 (one critic: dX_0 alone)
//        aa  = a * a;  one = 1 - aa;  den = one + 1e-6
//        ta  = 2 * a;  rat = ta / den;  ea = alpha * rat;  da = ea - dq          dL/da
//        du  = da * one                                                          dL/du
//        dmu = du * inv_B
//        ez  = expf(ls) * z;  t0 = du * ez;  t1 = t0 - alpha;  dls = t1 * inv_B  where -20 <= raw log_std <= 2, else 0 (torch's clamp)
//      into the actor head's dZ image: dmu in columns 0..A-1, dls in A..2A-1, zero up to OPAD; rows past B are zero. One thread per row:
//        el = alpha * logp;  l = el - min_c q_c;  e = logp + target_entropy        (0 in the rows past B)
//      and thread 0 sums l and e over the tile's rows in order from 0.0f; a tile's sums are added to the workgroup's in tile order;
//   6. the actor's backward pass: crit::weight_grad and crit::input_grad per layer, head first, into the workgroup's slab. The action
//      columns of X are zeroed first: they lie inside the actor's padded k0 where D is no multiple of 16, and the padding's gradient
//      must stay exactly 0.
// The slab is laid out like the actor's packed copy (crit::Layout); its four trailing floats hold the workgroup's sum of l (off[8]) and of
// e (off[8] + 1). Slabs are summed 0, 1, 2, ... by the consumer: bitwise reproducible, no atomics.
//
// LDS: X, one image per actor hidden layer, one per critic hidden layer (ONE critic's: that is why critic 0 runs twice), the gradient
// pair, [16][S] floats each, and 2 x 16 x 8 floats for the two critics' dX: at most 9 x 16 x 260 x 4 + 1024 = 150 784 B, an opt-in
// below the CU's 160 KB. No atomics, no local arrays, no inline assembly.
#pragma once
#include "mjs_critic_train.h"

namespace atrain {

using crit::ROWS;
constexpr int DQ_FLOATS = crit::MAX_CRITICS * ROWS * act::MAX_ACT;
constexpr size_t lds_bytes(int actor_hidden, int critic_hidden, int widest) {
  return ((size_t)(3 + actor_hidden + critic_hidden) * ROWS * act::lds_stride(widest) + DQ_FLOATS) * sizeof(float);
}

struct GradParams {
  crit::CriticParams c;      // B, D, A, the critics; S: the stride of every image (the widest of the actor's and the critics' layers)
  crit::Mlp actor;
  crit::Layout L;            // the actor's slab
  int tiles_per_split;
  float inv_B;               // 1 / B rounded to float32 on the host
  const float* obs;          // [B, D]
  const float* z;            // [B, A]
  float ent_coef;
  const float* ent_coef_dev; // one float, read instead of ent_coef where non-null
  float target_entropy;
  float* actions;            // [B, A] or nullptr
  float* log_prob;           // [B] or nullptr
  float* q_pi;               // [n_critics, B] or nullptr
  float* dq_da;              // [B, A] or nullptr: d(min_c Q_c)/da
  float* slabs;              // [splits][L.total]
};

// The action columns of a critic's first-layer input gradient into DQ [16][MAX_ACT]: wavefront w < 2 owns the 16-k tile D / 16 + w where
// it still holds a column below D + A (k < k0 always: D + A <= k0, a multiple of 16). G = dZ0 [16][O], W0 [k0][O]; O a multiple of 32.
__device__ __forceinline__ void action_grad(const float* G, int S, const float* __restrict__ W0, int O, int D, int A, float* DQ, int wave, int lane) {
  const int c = lane & 15, kh = lane >> 4;
  const int kb = (D / 16 + wave) * 16;
  if (wave < 2 && kb < D + A) {
    const int k = kb + c;
    const float* grow = G + c * S + 4 * kh;              // A[i = row c][kk = o]: 4 consecutive o
    const float* w = W0 + (size_t)k * O + 4 * kh;        // B[kk = o][j = k]: 4 consecutive o of row k
    act::f32x4 acc = {0.0f, 0.0f, 0.0f, 0.0f};
    for (int ob = 0; ob < O; ob += 16) {
      const act::f32x4 a = *reinterpret_cast<const act::f32x4*>(grow + ob);
      const act::f32x4 b = *reinterpret_cast<const act::f32x4*>(w + ob);
#pragma unroll
      for (int s = 0; s < 4; s++) acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a[s], b[s], acc, 0, 0, 0);
    }
    // D register q: row 4 kh + q, column k
    if (k >= D && k < D + A) {
#pragma unroll
      for (int q = 0; q < 4; q++) DQ[(4 * kh + q) * act::MAX_ACT + (k - D)] = acc[q];
    }
  }
}

// net[0] or net[1], member by member: a select chain over values, not a reference into the argument block (which the compiler would serve
// from a scratch copy of both structures)
__device__ __forceinline__ crit::Mlp pick(const crit::Mlp& a, const crit::Mlp& b, bool first) {
  crit::Mlp m;
  m.W0 = first ? a.W0 : b.W0; m.W1 = first ? a.W1 : b.W1; m.W2 = first ? a.W2 : b.W2; m.WH = first ? a.WH : b.WH;
  m.B0 = first ? a.B0 : b.B0; m.B1 = first ? a.B1 : b.B1; m.B2 = first ? a.B2 : b.B2; m.BH = first ? a.BH : b.BH;
  m.n_hidden = first ? a.n_hidden : b.n_hidden;
  m.k0 = first ? a.k0 : b.k0;
  m.w0 = first ? a.w0 : b.w0; m.w1 = first ? a.w1 : b.w1; m.w2 = first ? a.w2 : b.w2;
  m.activation = first ? a.activation : b.activation;
  return m;
}

// grid = splits workgroups of WAVES wavefronts; dynamic LDS = lds_bytes(actor's n_hidden, critics' n_hidden, widest)
__global__ __launch_bounds__(act::WAVES * 64) void grad_kernel(GradParams p) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  const int S = p.c.S, B = p.c.B, D = p.c.D, A = p.c.A, img = ROWS * S;
  const crit::Mlp& am = p.actor;
  const int na = am.n_hidden, nc = p.c.net[0].n_hidden, ncrit = p.c.n_critics;
  float* X = lds;
  float* AH0 = lds + img;                    // (images past n_hidden are not there and not touched)
  float* AH1 = lds + 2 * img;
  float* AH2 = lds + 3 * img;
  float* CH0 = lds + (1 + na) * img;
  float* CH1 = lds + (2 + na) * img;
  float* CH2 = lds + (3 + na) * img;
  float* GA = lds + (1 + na + nc) * img;
  float* GB = lds + (2 + na + nc) * img;
  float* DQ = lds + (3 + na + nc) * img;     // [critic][16][MAX_ACT]
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  float* slab = p.slabs + (size_t)blockIdx.x * p.L.total;
  const float* AHlast = na == 1 ? AH0 : na == 2 ? AH1 : AH2;
  const int AKlast = na == 1 ? am.w0 : na == 2 ? am.w1 : am.w2;
  const float* CHlast = nc == 1 ? CH0 : nc == 2 ? CH1 : CH2;
  const int tile0 = blockIdx.x * p.tiles_per_split, tiles = (B + ROWS - 1) / ROWS;
  const float alpha = p.ent_coef_dev ? *p.ent_coef_dev : p.ent_coef;
  const bool comp = tid < ROWS * A;          // one thread per (row, component)
  const int r = comp ? tid / A : 0, j = tid - r * A;
  float loss = 0.0f, ent = 0.0f;             // thread 0: the workgroup's sums of l and e, tile sums added in tile order

  for (int t = tile0; t < tile0 + p.tiles_per_split && t < tiles; t++) {
    const int row0 = t * ROWS;
    const bool first = t == tile0;
    // 1. the actor forward; the image is zeroed up to the critics' k0 already. The head's raw sums land in GA
    crit::fill_input(X, S, p.c.net[0].k0, D, row0, B, tid, [&](int i, int jj) { return p.obs[(size_t)i * D + jj]; });
    __syncthreads();
    act::layer<ROWS, true>(X, AH0, S, am.W0, am.B0, am.k0, am.w0, am.activation, wave, lane);
    __syncthreads();
    if (na > 1) {
      act::layer<ROWS, true>(AH0, AH1, S, am.W1, am.B1, am.w0, am.w1, am.activation, wave, lane);
      __syncthreads();
      if (na > 2) {
        act::layer<ROWS, true>(AH1, AH2, S, am.W2, am.B2, am.w1, am.w2, am.activation, wave, lane);
        __syncthreads();
      }
    }
    act::layer<ROWS, false>(AHlast, GA, S, am.WH, am.BH, AKlast, act::OPAD, am.activation, wave, lane);
    __syncthreads();

    // 2. td_target_kernel's steps 2 and 3; the thread keeps its component's a, z, ls and the clamp mask for the tail
    float a = 0.0f, zj = 0.0f, ls = 0.0f;
    bool live = false, inside = false;
    if (comp) {
      const int i = row0 + r;
      float gauss = 0.0f, corr = 0.0f;
      if (i < B) {
        const float mu = GA[r * S + j], raw = GA[r * S + A + j];
        ls = fminf(fmaxf(raw, act::LOG_STD_MIN), act::LOG_STD_MAX);
        zj = p.z[(size_t)i * A + j];
        a = crit::squashed_sample(mu, ls, zj, gauss, corr);
        if (p.actions) p.actions[(size_t)i * A + j] = a;
        live = true;
        inside = raw >= act::LOG_STD_MIN && raw <= act::LOG_STD_MAX;
      }
      X[r * S + D + j] = a;
      GA[r * S + 16 + j] = gauss;
      GA[r * S + 24 + j] = corr;
    }
    __syncthreads();
    float logp = 0.0f;
    if (tid < ROWS) {
      float sg = 0.0f, sc = 0.0f;
      for (int jj = 0; jj < A; jj++) {
        sg += GA[tid * S + 16 + jj];
        sc += GA[tid * S + 24 + jj];
      }
      logp = sg - sc;
      if (row0 + tid < B && p.log_prob) p.log_prob[row0 + tid] = logp;
    }
    __syncthreads();  // the critics' first layer writes GA

    // 3. q_0 alone, where there is a second critic to compare it with
    float q0 = 0.0f, q1 = 0.0f;
    if (ncrit == 2) {
      const float* head = crit::mlp(p.c.net[0], X, GA, GB, S, wave, lane);
      if (tid < ROWS) q0 = head[tid * S];
      __syncthreads();
    }
    // 4. critic 1, then critic 0 (one critic: critic 0)
    for (int pass = 0; pass < ncrit; pass++) {
      const int c = ncrit - 1 - pass;
      const crit::Mlp m = pick(p.c.net[0], p.c.net[1], c == 0);
      act::layer<ROWS, true>(X, CH0, S, m.W0, m.B0, m.k0, m.w0, m.activation, wave, lane);
      __syncthreads();
      if (nc > 1) {
        act::layer<ROWS, true>(CH0, CH1, S, m.W1, m.B1, m.w0, m.w1, m.activation, wave, lane);
        __syncthreads();
        if (nc > 2) {
          act::layer<ROWS, true>(CH1, CH2, S, m.W2, m.B2, m.w1, m.w2, m.activation, wave, lane);
          __syncthreads();
        }
      }
      const int CKlast = nc == 1 ? m.w0 : nc == 2 ? m.w1 : m.w2;
      act::layer<ROWS, false>(CHlast, GA, S, m.WH, m.BH, CKlast, act::OPAD, m.activation, wave, lane);
      __syncthreads();
      if (tid < ROWS) {
        const float qv = GA[tid * S];
        if (c == 0) q0 = qv; else q1 = qv;
        const bool one_is_min = ncrit == 2 && q1 < q0;
        const bool mine = c == 0 ? !one_is_min : one_is_min;
        float* row = GB + tid * S;
        row[0] = row0 + tid < B && mine ? 1.0f : 0.0f;
#pragma unroll
        for (int o = 1; o < act::OPAD; o++) row[o] = 0.0f;
      }
      __syncthreads();
      crit::input_grad(GB, CHlast, GA, S, m.WH, CKlast, act::OPAD, m.activation, wave, lane);
      __syncthreads();
      float* G = GA;
      float* other = GB;
      if (nc > 2) {
        crit::input_grad(G, CH1, other, S, m.W2, m.w1, m.w2, m.activation, wave, lane);
        __syncthreads();
        float* sw = G; G = other; other = sw;
      }
      if (nc > 1) {
        crit::input_grad(G, CH0, other, S, m.W1, m.w0, m.w1, m.activation, wave, lane);
        __syncthreads();
        float* sw = G; G = other; other = sw;
      }
      action_grad(G, S, m.W0, m.w0, D, A, DQ + c * ROWS * act::MAX_ACT, wave, lane);
      __syncthreads();
    }

    // 5. the tail: the actor head's dZ into GB (zero past 2 A), the two loss terms into its spare columns OPAD and OPAD + 1, which no
    // product reads (S > 2 OPAD)
    for (int e = tid; e < ROWS * act::OPAD; e += act::WAVES * 64) {
      const int o = e & (act::OPAD - 1);
      if (o >= 2 * A) GB[(e / act::OPAD) * S + o] = 0.0f;
    }
    if (comp) {
      float dq = DQ[r * act::MAX_ACT + j];
      if (ncrit == 2) dq = dq + DQ[(ROWS + r) * act::MAX_ACT + j];
      float dmu = 0.0f, dls = 0.0f;
      if (live) {
        if (p.dq_da) p.dq_da[(size_t)(row0 + r) * A + j] = dq;
        const float std_ = expf(ls);
        {
#pragma clang fp contract(off)
        const float aa = a * a;
        const float one = 1.0f - aa;
        const float den = one + crit::LOG_PROB_EPS;
        const float ta = 2.0f * a;
        const float rat = ta / den;
        const float ea = alpha * rat;
        const float da = ea - dq;
        const float du = da * one;
        dmu = du * p.inv_B;
        const float ez = std_ * zj;
        const float t0 = du * ez;
        const float t1 = t0 - alpha;
        const float t2 = t1 * p.inv_B;
        dls = inside ? t2 : 0.0f;
        }
      }
      GB[r * S + j] = dmu;
      GB[r * S + A + j] = dls;
      X[r * S + D + j] = 0.0f;  // the actor's first layer never saw these columns; its padding's gradient stays 0
    }
    if (tid < ROWS) {
      const int i = row0 + tid;
      float l = 0.0f, e = 0.0f;
      if (i < B) {
        const float qmin = ncrit == 2 && q1 < q0 ? q1 : q0;
        if (p.q_pi) {
          p.q_pi[i] = q0;
          if (ncrit == 2) p.q_pi[(size_t)B + i] = q1;
        }
        {
#pragma clang fp contract(off)
          const float el = alpha * logp;
          l = el - qmin;
          e = logp + p.target_entropy;
        }
      }
      GB[tid * S + act::OPAD] = l;
      GB[tid * S + act::OPAD + 1] = e;
    }
    __syncthreads();
    if (tid == 0) {
      float sl = 0.0f, se = 0.0f;
#pragma unroll
      for (int rr = 0; rr < ROWS; rr++) {
        sl += GB[rr * S + act::OPAD];
        se += GB[rr * S + act::OPAD + 1];
      }
      loss = first ? sl : loss + sl;
      ent = first ? se : ent + se;
    }

    // 6. the actor backward, head first; a layer's two products read the same dZ image and write elsewhere (the slab, the other image)
    crit::weight_grad(AHlast, GB, S, AKlast, act::OPAD, slab + p.L.off[6], slab + p.L.off[7], first, tid);
    crit::input_grad(GB, AHlast, GA, S, am.WH, AKlast, act::OPAD, am.activation, wave, lane);
    __syncthreads();
    float* G = GA;
    float* other = GB;
    if (na > 2) {
      crit::weight_grad(AH1, G, S, am.w1, am.w2, slab + p.L.off[4], slab + p.L.off[5], first, tid);
      crit::input_grad(G, AH1, other, S, am.W2, am.w1, am.w2, am.activation, wave, lane);
      __syncthreads();
      float* sw = G; G = other; other = sw;
    }
    if (na > 1) {
      crit::weight_grad(AH0, G, S, am.w0, am.w1, slab + p.L.off[2], slab + p.L.off[3], first, tid);
      crit::input_grad(G, AH0, other, S, am.W1, am.w0, am.w1, am.activation, wave, lane);
      __syncthreads();
      float* sw = G; G = other; other = sw;
    }
    crit::weight_grad(X, G, S, am.k0, am.w0, slab + p.L.off[0], slab + p.L.off[1], first, tid);
    __syncthreads();  // the next tile's fill writes X, its layers the images
  }
  if (tid == 0) {
    slab[p.L.off[8]] = loss;
    slab[p.L.off[8] + 1] = ent;
  }
}

// SB3's ent_coef_loss = -(log_ent_coef * (logp + target_entropy).detach()).mean() and its Adam step on the scalar, then ent_coef =
// expf(log_ent_coef): one thread, after the actor's Adam launch in stream order (grad_kernel has read the old ent_coef by then). The
// gradient, one operation per line, no contraction:  s = the slabs' e partials summed in order;  mean = s * inv_B;  g = -mean;  then
// crit::adam_kernel's lines with the coefficients of the scalar's own step count.
struct EntParams {
  const float* slabs;
  int splits, total, at;     // at = L.off[8] + 1
  float inv_B;
  float *log_ent_coef, *ent_coef, *m, *v;  // one float each
  float one_minus_beta1, beta2, one_minus_beta2, sqrt_bc2, eps, step_size;
};
__global__ __launch_bounds__(64) void ent_kernel(EntParams p) {
  if (threadIdx.x != 0 || blockIdx.x != 0) return;
  const float s = crit::slab_sum(p.slabs, p.splits, 1, p.total, 0, p.at);
  const float m0 = *p.m, v0 = *p.v, p0 = *p.log_ent_coef;
  float p1;
  {
#pragma clang fp contract(off)
    const float mean = s * p.inv_B;
    const float g = -mean;
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
    const float rr = m / den;
    const float u = p.step_size * rr;
    p1 = p0 - u;
    *p.m = m;
    *p.v = v;
  }
  *p.log_ent_coef = p1;
  *p.ent_coef = expf(p1);
}

}  // namespace atrain
