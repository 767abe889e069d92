// mjs_stamps_report.h — the report of a diagnostic build (-DMJS_STAMPS): mean phase lengths (shader cycles) of the LAST step launch,
// printed to stderr when a handle is destroyed. Included by mjsim.hip under MJS_STAMPS only (after mjs_push.h); tools/button_stamps_probe.py
// and the profiles/ records parse these lines.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdio>

inline void mjs_stamps_report(const unsigned long long* stamps_dev, int num_envs, int task) {
  const int W = (num_envs + 63) / 64;
  unsigned long long* host = new unsigned long long[16 * (size_t)num_envs];
  (void)hipDeviceSynchronize();
  (void)hipMemcpy(host, stamps_dev, sizeof(unsigned long long) * 16 * (size_t)num_envs, hipMemcpyDeviceToHost);
  double d[5] = {0, 0, 0, 0, 0}, e[5] = {0, 0, 0, 0, 0};
  for (int w = 0; w < W; w++) {
    for (int k = 0; k < 5; k++) d[k] += (double)(host[16 * w + k + 1] - host[16 * w + k]) / W;
    for (int k = 0; k < 5; k++) e[k] += (double)(host[16 * w + 8 + k + 1] - host[16 * w + 8 + k]) / W;
  }
  if (task == MJS_TASK_PLANAR_PUSH) {
    double c[16] = {0}, worst[16] = {0}, worst_total = 0;
    int hist[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
    const int WG = (num_envs + pp::EPW * pp::WAVES - 1) / (pp::EPW * pp::WAVES);
    for (int w = 0; w < WG; w++) {
      double tot = 0;
      for (int k = 0; k < 5; k++) tot += (double)host[16 * w + k];
      for (int k = 0; k < 16; k++) c[k] += (double)host[16 * w + k] / WG;
      if (tot > worst_total) { worst_total = tot; for (int k = 0; k < 16; k++) worst[k] = (double)host[16 * w + k]; }
      const int ns = (int)host[16 * w + 6];
      hist[ns == 0 ? 0 : ns <= 5 ? 1 : ns <= 10 ? 2 : ns <= 20 ? 3 : ns <= 30 ? 4 : ns <= 40 ? 5 : ns <= 60 ? 6 : ns <= 80 ? 7 : 8]++;
    }
    std::fprintf(stderr, "[MJS_STAMPS] planar-push, wave 0 of each workgroup, cycles per control step, MEAN: detect %.0f | arm dynamics %.0f | decoupled solves %.0f | cooperative coupled %.0f (of which the owner lane's publish %.0f) | integrate %.0f\n", c[0], c[1], c[2], c[3], c[5], c[4]);
    std::fprintf(stderr, "[MJS_STAMPS] cooperative solves per wavefront and control step: mean %.2f (%.2f Newton iterations each), slowest wavefront %.0f solves / %.0f iterations; wavefronts with 0 | 1-5 | 6-10 | 11-20 | 21-30 | 31-40 | 41-60 | 61-80 | >80 solves: %d %d %d %d %d %d %d %d %d\n", c[6], c[6] > 0 ? c[7] / c[6] : 0.0, worst[6], worst[7], hist[0], hist[1], hist[2], hist[3], hist[4], hist[5], hist[6], hist[7], hist[8]);
    std::fprintf(stderr, "[MJS_STAMPS] slowest wavefront, inside its cooperative solves: rows %.0f | init (M^-1 f, J a, update) %.0f | gradient+Hessian %.0f | Cholesky+solves %.0f | M v, J v %.0f | line search %.0f | update+gradient norm %.0f | J^T f %.0f\n", worst[15], worst[8], worst[9], worst[10], worst[11], worst[12], worst[13], worst[14]);
    std::fprintf(stderr, "[MJS_STAMPS] SLOWEST workgroup: detect %.0f | arm dynamics %.0f | decoupled solves %.0f | cooperative coupled %.0f (publish %.0f) | integrate %.0f\n", worst[0], worst[1], worst[2], worst[3], worst[5], worst[4]);
  }
  double own = 0;  // Robot-Reach kernel3: stamp 6 = wave 0 has finished its own prologue (load, sincos, substep 0) and reaches the IK barrier
  for (int w = 0; w < W; w++) own += (double)(host[16 * w + 6] - host[16 * w + 0]) / W;
  std::fprintf(stderr, "[MJS_STAMPS] cycles: load+IK %.0f (of which wave 0's own load + sincos + substep 0: %.0f) | substeps %.0f | fk+obs %.0f | contacts %.0f | store %.0f\n", d[0], own, d[1], d[2], d[3], d[4]);
  std::fprintf(stderr, "[MJS_STAMPS] role-0 substep 10: CRBA+factor+invert %.0f | barrier %.0f | apply inverse+publish+barrier %.0f | integrate %.0f\n", e[0], e[1], e[2], e[3]);
  if (task == MJS_TASK_ROBOT_REACH && num_envs >= 64) {  // MJS_ROLE_STAMP (mjs_reach.h): substep 10's tail on both dynamics wavefronts
    for (int role = 0; role < 2; role++) {
      double t[4] = {0, 0, 0, 0};
      for (int w = 0; w < W; w++) {
        const unsigned long long* s = host + 16 * (size_t)(W + w) + 8 * role;
        for (int k = 0; k < 4; k++) t[k] += (double)(s[k + 1] - s[k]) / W;
      }
      std::fprintf(stderr, "[MJS_STAMPS] role-%d substep 10 after barrier 2: qacc read %.0f | v, q, dq2 %.0f | rotate_small %.0f | fallback test + latch, to the top of substep 11 %.0f\n",
                   role, t[0], t[1], t[2], t[3]);
    }
  }
  if (task == MJS_TASK_ROBOT_REACH) {  // MJS_MASK_STATS (mjs_reach.h): counters summed over every launch of the handle
    double n = 0, changed = 0, nonzero = 0, lanes = 0;
    for (int w = 0; w < W; w++) { n += (double)host[16 * w + 13]; changed += (double)host[16 * w + 14]; nonzero += (double)host[16 * w + 15]; lanes += (double)host[16 * w + 7]; }
    if (n > 0)
      std::fprintf(stderr, "[MJS_STAMPS] clamp mask, %.0f wave-substeps of the role loop: some lane's mask differs from one substep earlier %.4f | some lane's mask non-zero %.4f | lane-substeps whose mask differs %.5f\n",
                   n, changed / n, nonzero / n, lanes / (64 * n));
  }
  delete[] host;
}
