// mjsim.hip — libmjsim.so: C ABI (include/mjsim.h) + kernel launches. gfx950 only.
#include <hip/hip_runtime.h>

#include <cstdio>
#include <cstring>
#include <memory>
#include <new>
#include <optional>
#include <string>
#include <vector>

#include "../../include/mjsim.h"
#include "mjs_kernel_common.h"
#include "mjs_pointmass.h"
#include "mjs_reach.h"
#include "mjs_button.h"
#include "mjs_gripper14.h"
#include "mjs_push.h"
#include "mjs_render.h"
#include "mjs_policy.h"
#include "mjs_actor.h"
#include "mjs_encoder.h"
#include "mjs_replay.h"
#include "mjs_critic.h"
#include "mjs_critic_train.h"
#include "mjs_actor_train.h"
#include "mjs_encoder_train.h"
#include "mjs_sac_train.h"
#include "mjs_monitor.h"
#ifdef MJS_STAMPS
#include "mjs_stamps_report.h"
#endif
#include <cmath>

// The six kernel instances. A handle runs one of them, resolved once in mjs_create (resolve_instance); the first four are the
// tasks' default instances, numbered like the tasks.
enum Kind { KIND_POINTMASS = MJS_TASK_POINTMASS_REACH, KIND_REACH = MJS_TASK_ROBOT_REACH, KIND_PUSH2 = MJS_TASK_PLANAR_PUSH, KIND_BUTTON = MJS_TASK_BUTTON_PUSH, KIND_PUSH5, KIND_BUTTON_ARTICULATED };
// The step launch a handle takes (launch<false>), named after what the grid is made of; resolve_instance has the reasons. Every
// reset launch is its kind's one-wavefront kernel.
enum Shape { SHAPE_ONE_WAVE, SHAPE_TWO_ROLES, SHAPE_THREE_WAVES, SHAPE_RESET_GROUPS, SHAPE_ENV_GROUPS, SHAPE_PUSH, SHAPE_PUSH_PREFETCH };

constexpr int alg_bytes(int rows_read, int rows_written, int act_dim, int obs_dim) {
  // state read + state written + flag byte r/w + action + obs + reward + discount + 5 flag bytes + ncon
  return 8 * rows_read + 8 * rows_written + 2 + 8 * act_dim + 8 * obs_dim + (8 + 8 + 5 + 4);
}

struct Instance {
  Kind kind;
  int state_dim, obs_dim, act_dim;  // state rows (without the flag row), flat observation and action widths
  int alg_bytes;                    // algorithmic HBM bytes of one env-step
  int nprim;                        // render primitives per env (0: the scene is drawn without a list)
  int prog_row;                     // Planar-Push: state row with the progress of the prepared next episode; -1 otherwise
  // resolved per handle
  Shape shape = SHAPE_ONE_WAVE;
  int epw = 64;        // envs per workgroup where the kernel takes it as an argument (Button-Push, both grippers)
  size_t lds_pad = 0;  // unused dynamic LDS per workgroup of the default Robot-Reach / Button-Push step launch (A/B builds only)
};

// Every layout constant of an instance, once; indexed by Kind. The per-task queries of the ABI describe the task's default instance.
const Instance INSTANCES[] = {
    {KIND_POINTMASS, pm::STATE_DIM, pm::OBS_DIM, pm::ACT_DIM, alg_bytes(pm::STATE_DIM, pm::STATE_DIM - 2 /*target unchanged*/, pm::ACT_DIM, pm::OBS_DIM), 0, -1},
    // q v time target + carried cos / sin; the qacc_warmstart rows are only touched by the robust path
    {KIND_REACH, rr::STATE_DIM, rr::OBS_DIM, rr::ACT_DIM, alg_bytes(rr::HOT_ROWS_READ, rr::HOT_ROWS_WRITTEN, rr::ACT_DIM, rr::OBS_DIM), rend::RR_NPRIM, -1},
    // Planar-Push: one world's rows (the state also carries the prepared next episode, its progress row, the servo set-point and
    // cos / sin); everything but the target is rewritten
    {KIND_PUSH2, pp::FULL_STATE_DIM, pp::OBS_DIM, pp::ACT_DIM, alg_bytes(pp::STATE_DIM, pp::STATE_DIM - 3, pp::ACT_DIM, pp::OBS_DIM), rend::ARM_NREC + 1 + pp::NB, pp::PROG_ROW},
    {KIND_BUTTON, bp::STATE_DIM, bp::OBS_DIM, bp::ACT_DIM_JOINT, alg_bytes(bp::HOT_ROWS_READ, bp::HOT_ROWS_WRITTEN, bp::ACT_DIM_JOINT, bp::OBS_DIM), rend::BP_NPRIM, -1},
    {KIND_PUSH5, pp5::FULL_STATE_DIM, pp5::OBS_DIM, pp5::ACT_DIM, alg_bytes(pp5::STATE_DIM, pp5::STATE_DIM - 3, pp5::ACT_DIM, pp5::OBS_DIM), rend::ARM_NREC + 1 + pp5::NB, pp5::PROG_ROW},
    {KIND_BUTTON_ARTICULATED, bg::STATE_DIM, bg::OBS_DIM, bp::ACT_DIM_JOINT, alg_bytes(bg::STATE_DIM, bg::STATE_DIM - 3, bp::ACT_DIM_JOINT, bg::OBS_DIM), rend::BP_NPRIM, -1},
};
static_assert(rend::ARM_NREC + 1 + pp5::NB == rend::PP_NPRIM, "the 5-slot instance fills the primitive list's capacity");

#ifdef MJS_AB_KNOBS
#include <cstdlib>
// A/B knobs of diagnostic builds (tools/ab_build.py --flag=-DMJS_AB_KNOBS); the shipped library has none, a stray variable would change
// the workgroup shape behind the bitwise guarantees of include/mjsim.h. Read once per mjs_create (the handle's device is current),
// range-checked, stored in the instance; returns what is wrong with a value, or nullptr. MJS_LDS_PAD: a pad above half of the CU's
// 160 KB leaves room for ONE workgroup per CU, which tells whether the dispatcher packs the few workgroups of a 4096-env launch
// onto shared CUs (profiles/r04_e_workgroup_placement.txt). MJS_BP_EPG, MJS_BG_EPW: envs per workgroup (profiles/r04_d_*, r04_b_*).
static const char* read_ab_knobs(Instance& in) {
  const char* ev;
  if ((in.kind == KIND_REACH || in.kind == KIND_BUTTON) && (ev = std::getenv("MJS_LDS_PAD"))) {
    const void* kernel = in.kind == KIND_REACH ? reinterpret_cast<const void*>(&rr::kernel3<0>) : reinterpret_cast<const void*>(&bp::kernel<false, 2>);
    const long pad = std::atol(ev);
    hipFuncAttributes attr;
    if (hipFuncGetAttributes(&attr, kernel) != hipSuccess || pad < 0 || (size_t)pad > (size_t)160 * 1024 - attr.sharedSizeBytes)
      return "mjs_create: MJS_LDS_PAD is negative or exceeds the CU's 160 KB of LDS minus what the kernel uses";
    if (pad > 0 && hipFuncSetAttribute(kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)pad) != hipSuccess) return "mjs_create: MJS_LDS_PAD opt-in failed";
    in.lds_pad = (size_t)pad;
  }
  if (in.kind == KIND_BUTTON && (ev = std::getenv("MJS_BP_EPG"))) {
    in.epw = std::atoi(ev);
    if (in.epw != 8 && in.epw != 16 && in.epw != 32 && in.epw != 64) return "mjs_create: MJS_BP_EPG must be 8, 16, 32 or 64";
  }
  if (in.kind == KIND_BUTTON_ARTICULATED && (ev = std::getenv("MJS_BG_EPW"))) {
    in.epw = std::atoi(ev);
    if (in.epw < 1 || in.epw > 16) return "mjs_create: MJS_BG_EPW must be 1..16";
  }
  return nullptr;
}
#else
static const char* read_ab_knobs(Instance&) { return nullptr; }
#endif

struct mjs_handle {
  mjs_config cfg;
  Instance inst;
  // render primitive list of the CURRENT state already built on this stream? (the visual configs render two cameras per
  // control step; reset / step / rollout / set_state invalidate)
  bool prims_valid = false;
  void* prims_stream = nullptr;
  double* state = nullptr;     // [state_dim][N]
  uint8_t* flags = nullptr;    // [N]
  uint32_t* rng_mt = nullptr;  // [624][N]
  int32_t* rng_pos = nullptr;  // [N]
  unsigned long long* stamps = nullptr;  // diagnostic builds only
  float* prims = nullptr;      // [N][nprim][PRIM_FLOATS] render primitive list (robot scenes)
  float4* bg_ray = nullptr;    // [bg_H * bg_W] scene-camera ray table (rend::Background), built at the first render of a size and pose
  uint32_t* bg_rgb = nullptr;
  int bg_H = 0, bg_W = 0;
  unsigned bg_serial = 0;      // the cam_serial the table was built for
  mjs_camera_pose cam;         // the scene camera: the task's default, or what mjs_set_scene_camera gave (not part of the state block)
  unsigned cam_serial = 0;     // counts mjs_set_scene_camera calls
  float* cams = nullptr;       // [N][12] wrist-camera poses (Button-Push)
  double* ws = nullptr;        // [rr::WS_ROWS][N] contact workspace of the general constraint stage (Robot-Reach, Button-Push)
  int epoch = 0;               // parity of the next step launch (FLAG_EPOCH)
  double* ws14 = nullptr;      // [bg::WS_DOUBLES][N] constraint rows of the articulated-gripper kernel (mjs_gripper14.h)
  std::string err;
};

// A learned policy (mjs_actor.h): the shape, and the library's packed copy of the parameters. No per-handle state.
struct mjs_actor {
  mjs_actor_desc desc;             // validated; obs_index points at `index`
  std::vector<int32_t> index;      // host copy of obs_index
  int max_index = 0;               // the largest obs_index entry: a handle's observation row must be wider
  int k0 = 0, width[3] = {0, 0, 0};  // in_dim padded to act::KPAD, hidden widths padded to act::OPAD
  int widest = 0;                  // of k0, width[], act::OPAD: sizes the LDS images
  int* index_dev = nullptr;
  float* w[4] = {nullptr, nullptr, nullptr, nullptr};  // packed [k][out]: hidden layers, then (slot 3) the stacked mu / log_std head
  float* b[4] = {nullptr, nullptr, nullptr, nullptr};
  bool loaded = false;             // mjs_actor_load has run
  // a visual actor (mjs_actor_create_visual): feature blocks among the first layer's inputs. `index` then has in_total entries in
  // act::FeatureInputs' encoding
  bool visual = false;
  int in_total = 0;                // desc.in_dim + the blocks' widths: the first layer's fan-in
  int block_width[act::MAX_BLOCKS] = {0, 0};
};

// SAC's critics (mjs_critic.h): the shape, and the library's packed copy of every network's parameters.
struct mjs_critic {
  mjs_critic_desc desc;
  int k0 = 0, width[3] = {0, 0, 0};  // obs_dim + action_dim padded to act::KPAD, hidden widths padded to act::OPAD
  int widest = 0;                    // of k0, width[], act::OPAD
  float* w[crit::MAX_CRITICS][4] = {};  // packed [k][out] per critic: hidden layers, then (slot 3) the scalar head padded to act::OPAD
  float* b[crit::MAX_CRITICS][4] = {};
  bool loaded = false;               // mjs_critic_load has run
};

// Adam on one critic's packed copy (mjs_critic_train.h): the moments, the slab workspace and the step count.
struct mjs_critic_opt {
  mjs_critic* critic = nullptr;  // the critic it was created for; must outlive the optimiser
  mjs_critic_opt_desc desc;
  crit::Layout L;
  int max_splits = 0;            // slabs the workspace holds per critic
  float* m = nullptr;            // [n_critics][L.total], slab layout
  float* v = nullptr;
  float* slabs = nullptr;        // [max_splits][n_critics][L.total]
  float* gsum = nullptr;         // [n_critics][L.total]: the summed gradient on its way to nn.Linear layout
  int64_t t = 0;                 // optimiser steps taken
};

// Adam on an actor's packed copy (mjs_actor_train.h): the moments, the slab workspace and the step count.
struct mjs_actor_opt {
  mjs_actor* actor = nullptr;    // the actor it was created for; must outlive the optimiser
  mjs_actor_opt_desc desc;
  crit::Layout L;
  int max_splits = 0;            // slabs the workspace holds
  float* m = nullptr;            // [L.total], slab layout
  float* v = nullptr;
  float* slabs = nullptr;        // [max_splits][L.total]
  float* gsum = nullptr;         // [L.total]: the summed gradient on its way to nn.Linear layout
  int64_t t = 0;                 // optimiser steps taken
};

// An image encoder (mjs_encoder.h): the geometry, and the library's packed copy of the parameters. No per-handle state.
struct mjs_encoder {
  mjs_encoder_desc desc;
  enc::Geometry g;
  int Fp = 0;                      // features_dim padded to enc::FPAD
  float* w[4] = {nullptr, nullptr, nullptr, nullptr};  // packed [k][out]: conv1..3, fc
  float* b[4] = {nullptr, nullptr, nullptr, nullptr};
  bool loaded = false;
};

// Adam on an encoder's packed copy (mjs_encoder_train.h): the moments and the step count. The slabs live in the caller's workspace.
struct mjs_encoder_opt {
  mjs_encoder* encoder = nullptr;  // the encoder it was created for; must outlive the optimiser
  mjs_encoder_opt_desc desc;
  crit::Layout L;
  float* m = nullptr;              // [L.total], slab layout
  float* v = nullptr;
  float* gsum = nullptr;           // [L.total]: the summed gradient on its way to torch layout
  int64_t t = 0;                   // optimiser steps taken
};

namespace {

thread_local std::string g_err;

int fail(mjs_handle* h, int code, const std::string& msg) {
  if (h) h->err = msg;
  g_err = msg;
  return code;
}
int hip_fail(mjs_handle* h, hipError_t e, const char* what) {
  return fail(h, MJS_ERR_HIP, std::string(what) + ": " + hipGetErrorString(e));
}
#define HIP_TRY(h, expr)                                   \
  do {                                                     \
    hipError_t e_ = (expr);                                \
    if (e_ != hipSuccess) return hip_fail(h, e_, #expr);   \
  } while (0)

// a failing HIP call of a create function `fn` (the scope guard there frees what the object holds so far); `what` replaces the call's text
#define CREATE_TRY(fn, expr, ...)                                                                                       \
  do {                                                                                                                  \
    hipError_t e_ = (expr);                                                                                             \
    const char* what_ = "" __VA_ARGS__;                                                                                 \
    if (e_ != hipSuccess) return hip_fail(nullptr, e_, (std::string(fn) + ": " + (*what_ ? what_ : #expr)).c_str());    \
  } while (0)
// what the create functions refuse about a device ordinal; MJS_OK = fine
int device_refusal(const std::string& name, int device) {
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) return fail(nullptr, MJS_ERR_NO_DEVICE, name + ": no HIP device visible (this library has no CPU path)");
  if (device < 0 || device >= ndev) return fail(nullptr, MJS_ERR_INVALID_ARG, name + ": device ordinal out of range");
  return MJS_OK;
}
// the device buffers of an object that is being destroyed
void free_all(std::initializer_list<void*> buffers) {
  for (void* p : buffers)
    if (p) (void)hipFree(p);
}

// Select the handle's device for the duration of one ABI call and restore the caller's current device afterwards
// (torch's notion of the current device must not change behind its back). Same device: one hipGetDevice, no switch.
struct DeviceGuard {
  int prev = -1;
  hipError_t err;
  explicit DeviceGuard(int dev) {
    err = hipGetDevice(&prev);
    if (err == hipSuccess && prev != dev) err = hipSetDevice(dev);
    else prev = -1;
  }
  ~DeviceGuard() {
    if (prev >= 0) (void)hipSetDevice(prev);
  }
  DeviceGuard(const DeviceGuard&) = delete;
  DeviceGuard& operator=(const DeviceGuard&) = delete;
};

double default_time_limit(int task) {
  if (task == MJS_TASK_POINTMASS_REACH) return MJS_PM_MAX_CONTROL_STEPS * MJS_PM_CONTROL_DT;  // mujoco_sim/__init__.py:21,28
  if (task == MJS_TASK_BUTTON_PUSH) return MJS_BP_MAX_CONTROL_STEPS * MJS_RR_CONTROL_DT;      // mujoco_sim/__init__.py:45-49
  if (task == MJS_TASK_PLANAR_PUSH) return 1e300;  // scripts/sb3/planar_push.py:72: no Environment time limit, the task counts steps
  return MJS_RR_MAX_CONTROL_STEPS * MJS_RR_CONTROL_DT;                                       // BASELINE config 3
}
int default_reward(int task) { return task == MJS_TASK_POINTMASS_REACH ? MJS_REW_DENSE_BIASED_NEG_DISTANCE : MJS_REW_DENSE_NEG_DISTANCE; }

__global__ __launch_bounds__(64) void seed_kernel(DevRng rng, uint32_t base_seed, int offset) {
  int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= rng.N) return;
  rng_seed_lane(rng, i, base_seed + (uint32_t)(offset + i));
}

// Pointmass bookkeeping starts at 1.0 at construction (point_reach.py:112-113); flags = reset pending
// host_pending: the byte of an env that waits for its next-step reset, as the host writes it (reset-groups handles: with the
// parity OPPOSITE to the next step launch's, i.e. "ended in an earlier launch", mjs_kernel_common.h)
__global__ void fill_row_kernel(double* row, int N, double value) {
  int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < N) row[i] = value;
}
__global__ void init_kernel(double* state, uint8_t* flags, int N, int task, uint8_t host_pending) {
  int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= N) return;
  flags[i] = host_pending;
  if (task == MJS_TASK_POINTMASS_REACH) {
    state[(size_t)pm::S_DIST * N + i] = 1.0;
    state[(size_t)pm::S_PREV * N + i] = 1.0;
  }
}

__global__ void get_state_kernel(const double* state, const uint8_t* flags, double* out, int N, int S) {
  int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= N) return;
  for (int k = 0; k < S; k++) out[(size_t)k * N + i] = state[(size_t)k * N + i];
  // the launch-parity protocol of the reset-groups variant is not part of a checkpoint: a restored env is neither "reset in
  // this launch" nor marked with a parity of the handle it came from
  out[(size_t)S * N + i] = (double)(uint8_t)(flags[i] & ~(FLAG_FRESH | FLAG_EPOCH));
}
__global__ void set_state_kernel(double* state, uint8_t* flags, const double* in, int N, int S, int task, uint8_t host_pending) {
  int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= N) return;
  for (int k = 0; k < S; k++) state[(size_t)k * N + i] = in[(size_t)k * N + i];
  uint8_t f = (uint8_t)((uint8_t)in[(size_t)S * N + i] & ~(FLAG_FRESH | FLAG_EPOCH));
  if (f & FLAG_RESET_PENDING) f = (uint8_t)(f | host_pending);
  if (task == MJS_TASK_ROBOT_REACH || task == MJS_TASK_BUTTON_PUSH) {
    // the caller may have edited the joints: the carried cos / sin rows are kept when they belong to the given q (a checkpoint
    // resumes bit for bit) and rewritten with exact values when they do not
    const int first = task == MJS_TASK_ROBOT_REACH ? rr::S_CS : bp::S_CS;
    double q[rr::NJ];
    for (int j = 0; j < rr::NJ; j++) {
      q[j] = in[(size_t)(rr::S_Q + j) * N + i];
      double sn, cs;
      sincos(q[j], &sn, &cs);
      const double c_in = in[(size_t)(first + j) * N + i], s_in = in[(size_t)(first + rr::NJ + j) * N + i];
      if (!(fabs(c_in - cs) < 1e-11 && fabs(s_in - sn) < 1e-11)) {
        state[(size_t)(first + j) * N + i] = cs;
        state[(size_t)(first + rr::NJ + j) * N + i] = sn;
      }
    }
    if (task == MJS_TASK_ROBOT_REACH)  // FLAG_CLEAR is a function of the joints
      f = (uint8_t)((f & ~FLAG_CLEAR) | (rr::config_is_clear(q) ? FLAG_CLEAR : 0));
  }
  flags[i] = f;
}

__global__ void debug_ik_kernel(const double* T, const double* guess, double* q, uint8_t* ok, int n) {
  int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  rr::Aff A;
  for (int k = 0; k < 9; k++) A.r[k] = T[(size_t)i * 12 + k];
  for (int k = 0; k < 3; k++) A.t[k] = T[(size_t)i * 12 + 9 + k];
  double g[6], out[6] = {0, 0, 0, 0, 0, 0};
  for (int k = 0; k < 6; k++) g[k] = guess[(size_t)i * 6 + k];
  bool found = rr::ik_closest(A, g, out);
  for (int k = 0; k < 6; k++) q[(size_t)i * 6 + k] = out[k];
  ok[i] = found;
}

__global__ void tcp_to_joints_kernel(const double* pos, const double* guess, double* q, uint8_t* ok, int n) {
  int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  double p3[3], g[6], out[6];
  for (int k = 0; k < 3; k++) p3[k] = pos[(size_t)i * 3 + k];
  for (int k = 0; k < 6; k++) { g[k] = guess[(size_t)i * 6 + k]; out[k] = g[k]; }
  bool found = rr::tcp_pose_to_joints(p3, g, out);
  for (int k = 0; k < 6; k++) q[(size_t)i * 6 + k] = found ? out[k] : g[k];
  ok[i] = found;
}

// The instance a task's per-task queries describe, and the one its handles run unless the config widens it; nullptr: no such task
const Instance* task_defaults(int task) { return task >= KIND_POINTMASS && task <= KIND_BUTTON ? &INSTANCES[task] : nullptr; }

// What a handle runs, from its validated config (defaults filled in). Everything here is constant for the life of the handle.
Instance resolve_instance(const mjs_config& cfg) {
  Kind kind = task_defaults(cfg.task)->kind;
  if (kind == KIND_BUTTON && cfg.gripper_model == MJS_GRIPPER_ARTICULATED) kind = KIND_BUTTON_ARTICULATED;
  if (kind == KIND_PUSH2 && cfg.n_objects > MJS_PP_FAST_OBJECTS) kind = KIND_PUSH5;  // 3..5 blocks: the 5-slot instance
  Instance in = INSTANCES[kind];
  in.act_dim = mjs_action_dim_for(cfg.task, cfg.action_type);
  const bool next_step = cfg.autoreset == MJS_AUTORESET_NEXT_STEP;
  switch (kind) {
    case KIND_POINTMASS: break;  // SHAPE_ONE_WAVE
    case KIND_PUSH2:
    case KIND_PUSH5:
      // next episodes are prepared ahead of time by prefetch workgroups (mjs_push_impl.h NEXT_ROW0); variant 1 keeps round 3's
      // behaviour (the settle steps of a reset run inside the step launch) for A/B measurements
      in.shape = next_step && cfg.kernel_variant != MJS_VARIANT_SINGLE_WAVE ? SHAPE_PUSH_PREFETCH : SHAPE_PUSH;
      break;
    case KIND_BUTTON_ARTICULATED:
      // One kernel shape (a workgroup resets its own envs, never reset groups). The kernel is bound by instruction DELIVERY (its
      // substep streams ~150 KB of code through the instruction cache), so fewer, fuller wavefronts win as soon as every CU has one:
      // 16 envs per workgroup (what the LDS holds: 16 x 9.8 KB) from 4096 envs on - 11.7 ms per launch against 14.9 with 4
      // (profiles/r04_b_*)
      in.shape = SHAPE_ENV_GROUPS;
      in.epw = cfg.num_envs < 1024 ? 4 : cfg.num_envs < 4096 ? 8 : 16;
      in.alg_bytes += 8 * (in.act_dim - INSTANCES[kind].act_dim);  // this instance counts the handle's action width
      break;
    case KIND_REACH:
    case KIND_BUTTON:
      // Button-Push: envs per workgroup = 64 (in.epw). Smaller groups were measured (profiles/r04_d_button_group_size.txt) and LOSE:
      // with 16 envs per group the steady state goes 53 -> 84 us per launch and the desynchronised case stays at 260 us - four times
      // the wavefronts share SIMDs (the dispatcher packs workgroups onto CUs), which costs more than the smaller groups save.
      if (cfg.kernel_variant == MJS_VARIANT_SINGLE_WAVE) in.shape = SHAPE_ONE_WAVE;
      // Robot-Reach, two shapes of the same step (results equal to rounding): an IK wave + two role-specialised dynamics waves per
      // 64 envs is the faster one while every workgroup has a CU to itself (the launch is one workgroup's latency: -10 % at 4096
      // envs); past 16384 envs per GPU the chip is full and the third, mostly idle wave costs a SIMD: the two-role kernel of round 1
      // then has twice the throughput (profiles/r02_j_batch_size_scaling.txt: 65536 envs 435 vs 822 M env-steps/s).
      else if (kind == KIND_REACH && (cfg.kernel_variant == MJS_VARIANT_TWO_ROLES || (cfg.kernel_variant == MJS_VARIANT_DEFAULT && cfg.num_envs > 16384)))
        in.shape = SHAPE_TWO_ROLES;
      // MJS_VARIANT_RESET_GROUPS, for episodes that end at different times: the second half of the grid are reset workgroups (one
      // per 64 envs, on other CUs: an env whose episode ended is reset there while the first half steps the others: 54 -> 38 us per
      // launch with 1 % of the envs ending in every step); the launch parity tells a freshly reset env from one that waits. Not the
      // default for synchronous episodes: the 64 extra workgroups cost 0.9 us per launch at 4096 envs.
      else if (cfg.kernel_variant == MJS_VARIANT_RESET_GROUPS && next_step) in.shape = SHAPE_RESET_GROUPS;
      else in.shape = kind == KIND_REACH ? SHAPE_THREE_WAVES : SHAPE_TWO_ROLES;
      break;
  }
  return in;
}

uint8_t host_pending_byte(const mjs_handle* h) {
  return (uint8_t)(FLAG_RESET_PENDING | ((h->inst.shape == SHAPE_RESET_GROUPS && !h->epoch) ? FLAG_EPOCH : 0));
}

KernelParams make_params(const mjs_handle* h, const double* actions, const uint8_t* mask, const mjs_outputs* out) {
  KernelParams p;
  p.N = h->cfg.num_envs;
  p.reward_type = h->cfg.reward_type;
  p.autoreset = h->cfg.autoreset;
  p.terminate_on_success = h->cfg.terminate_on_success;
  p.action_type = h->cfg.action_type;
  p.button_disturbances = h->cfg.button_disturbances;
  p.n_objects = h->cfg.n_objects;
  p.max_episode_steps = h->cfg.max_episode_steps;
  p.block_shape = h->cfg.block_shape;
  p.epoch = h->epoch;
  p.reset_groups = h->inst.shape == SHAPE_RESET_GROUPS;
  p.epg = h->inst.kind == KIND_BUTTON ? h->inst.epw : 64;
  p.prefetch = h->inst.shape == SHAPE_PUSH_PREFETCH;
  p.time_limit = h->cfg.time_limit;
  p.state = h->state;
  p.flags = h->flags;
  p.ws = h->ws;
  p.rng = DevRng{h->rng_mt, h->rng_pos, h->cfg.num_envs};
  p.actions = actions;
  p.reset_mask = mask;
  if (out) p.out = *out; else std::memset(&p.out, 0, sizeof p.out);
  p.stamps = h->stamps;
  return p;
}

constexpr int BLOCK = 64;  // one wavefront per workgroup: N/64 workgroups spread over the CUs
inline dim3 grid_for(int n) { return dim3((unsigned)((n + BLOCK - 1) / BLOCK)); }

template <bool IS_RESET>
int launch(mjs_handle* h, const KernelParams& p, hipStream_t s) {
  const Instance& in = h->inst;
  const Shape shape = IS_RESET ? SHAPE_ONE_WAVE : in.shape;  // Robot-Reach / Button-Push reset on their one-wavefront kernel
  const dim3 bgrid((unsigned)((p.N + p.epg - 1) / p.epg));   // Button-Push
  switch (in.kind) {
    case KIND_POINTMASS: pm::kernel<IS_RESET><<<grid_for(p.N), BLOCK, 0, s>>>(p); break;
    case KIND_PUSH2: pp::kernel<IS_RESET><<<dim3((unsigned)(((!IS_RESET && p.prefetch) ? 2 : 1) * ((p.N + pp::EPW * pp::WAVES - 1) / (pp::EPW * pp::WAVES)))), BLOCK * pp::WAVES, pp::LDS_BYTES, s>>>(p); break;
    case KIND_PUSH5: pp5::kernel<IS_RESET><<<dim3((unsigned)(((!IS_RESET && p.prefetch) ? 2 : 1) * ((p.N + pp5::EPW * pp5::WAVES - 1) / (pp5::EPW * pp5::WAVES)))), BLOCK * pp5::WAVES, pp5::LDS_BYTES, s>>>(p); break;
    case KIND_BUTTON_ARTICULATED:  // stepping: bg::ROLES wavefronts share the envs
      bg::kernel<IS_RESET><<<dim3((unsigned)((p.N + in.epw - 1) / in.epw)), IS_RESET ? BLOCK : bg::ROLES * BLOCK, (size_t)in.epw * sizeof(bg::Env), s>>>(p, h->ws14, in.epw); break;
    case KIND_BUTTON:
      switch (shape) {
        case SHAPE_ONE_WAVE: bp::kernel<IS_RESET, 1><<<bgrid, BLOCK, 0, s>>>(p); break;
        case SHAPE_RESET_GROUPS: bp::kernel<false, 2><<<dim3(2 * bgrid.x), 2 * BLOCK, 0, s>>>(p); break;
        default: bp::kernel<false, 2><<<bgrid, 2 * BLOCK, in.lds_pad, s>>>(p); break;  // SHAPE_TWO_ROLES
      }
      break;
    case KIND_REACH:
      switch (shape) {
        case SHAPE_ONE_WAVE: rr::kernel<IS_RESET, 1><<<grid_for(p.N), BLOCK, 0, s>>>(p); break;
        case SHAPE_TWO_ROLES: rr::kernel<false, 2><<<grid_for(p.N), 2 * BLOCK, 0, s>>>(p); break;
        case SHAPE_RESET_GROUPS: rr::kernel3<0><<<dim3(2 * grid_for(p.N).x), 3 * BLOCK, 0, s>>>(p); break;
        default: rr::kernel3<0><<<grid_for(p.N), 3 * BLOCK, in.lds_pad, s>>>(p); break;  // SHAPE_THREE_WAVES
      }
      break;
  }
  HIP_TRY(h, hipGetLastError());
  if (shape == SHAPE_RESET_GROUPS) h->epoch ^= 1;  // only a launch that was accepted consumed its parity
  return MJS_OK;
}

void default_scene_camera(int task, mjs_camera_pose& c) {
  const double* q = task == MJS_TASK_POINTMASS_REACH ? MJS_PM_CAM_QUAT : task == MJS_TASK_BUTTON_PUSH ? MJS_BP_CAM_QUAT : MJS_RR_CAM_QUAT;
  const double* cpos = task == MJS_TASK_POINTMASS_REACH ? MJS_PM_CAM_POS : task == MJS_TASK_BUTTON_PUSH ? MJS_BP_CAM_POS : MJS_RR_CAM_POS;
  c.struct_size = (uint32_t)sizeof(mjs_camera_pose);
  c.reserved0 = 0;
  for (int k = 0; k < 3; k++) c.pos[k] = cpos[k];
  for (int k = 0; k < 4; k++) c.quat[k] = q[k];
  c.fovy = task == MJS_TASK_POINTMASS_REACH ? MJS_PM_CAM_FOVY : task == MJS_TASK_BUTTON_PUSH ? MJS_BP_CAM_FOVY : MJS_RR_CAM_FOVY;
}

// The launches of one render, for what it writes (OUT: rend::OUT_RGB | rend::OUT_DEPTH). The OUT_RGB instantiations are the
// kernels mjs_render has always launched.
template <int OUT>
int render_launch(mjs_handle* h, rend::RenderParams& p, float* depth, bool wrist, bool rect_walk, int band_rows, unsigned nbands, hipStream_t stream) {
  const int task = h->cfg.task, height = p.H, width = p.W;
  dim3 grid((unsigned)((height * width + 255) / 256), (unsigned)p.N);
  const int tiles = ((height + 7) / 8) * ((width + 7) / 8);  // robot scenes: one wavefront per 8x8 tile
  dim3 tile_grid((unsigned)((tiles + 3) / 4), (unsigned)p.N);
  auto robot_scene = [&]() {
    const dim3 rw_grid((unsigned)p.N, nbands);
    if (rect_walk && p.env_cams) rend::robot_scene_rect_walk_kernel<false, OUT><<<rw_grid, 256, 0, stream>>>(p, h->prims, rend::Background{nullptr, nullptr}, band_rows, depth);
    else if (rect_walk) rend::robot_scene_rect_walk_kernel<true, OUT><<<rw_grid, 256, 0, stream>>>(p, h->prims, rend::Background{h->bg_ray, h->bg_rgb}, band_rows, depth);
    else rend::robot_scene_kernel<OUT><<<tile_grid, 256, 0, stream>>>(p, h->prims, depth);
  };
  const bool fresh = h->prims_valid && h->prims_stream == stream;  // same state, same stream: the list is still good
  h->prims_valid = true;
  h->prims_stream = stream;
  p.nprim = h->inst.nprim;
  if (task == MJS_TASK_POINTMASS_REACH) {
    rend::pointmass_kernel<OUT><<<grid, 256, 0, stream>>>(p, depth);
  } else if (task == MJS_TASK_BUTTON_PUSH) {
    if (!fresh) {
      rend::ScenePose sp;
      for (int k = 0; k < 3; k++) sp.pos[k] = h->cam.pos[k];
      for (int k = 0; k < 4; k++) sp.quat[k] = h->cam.quat[k];
      rend::button_prims_kernel<<<grid_for(p.N), BLOCK, 0, stream>>>(h->state, h->flags, h->prims, h->cams, p.N, sp);
    }
    if (wrist) p.env_cams = h->cams;
    robot_scene();
  } else if (task == MJS_TASK_PLANAR_PUSH) {  // robot_planar_push.py:45,66: the FRONT_TILTED camera of Robot-Reach unless the handle's was set
    if (!fresh) rend::push_prims_kernel<<<grid_for(p.N), BLOCK, 0, stream>>>(h->state, h->prims, p.N, h->cfg.n_objects, p.nprim - (rend::ARM_NREC + 1));
    robot_scene();
  } else {
    if (!fresh) rend::reach_prims_kernel<<<grid_for(p.N), BLOCK, 0, stream>>>(h->state, h->prims, p.N);
    robot_scene();
  }
  HIP_TRY(h, hipGetLastError());
  return MJS_OK;
}

// slice t of rollout outputs (every field carries a leading time axis [T, N, ...])
mjs_outputs slice_outputs(const mjs_handle* h, const mjs_outputs* out, int32_t t) {
  mjs_outputs o;
  std::memset(&o, 0, sizeof o);
  if (!out) return o;
  const size_t N = (size_t)h->cfg.num_envs;
  o = *out;
  if (o.obs) o.obs += (size_t)t * N * h->inst.obs_dim;
  if (o.terminal_obs) o.terminal_obs += (size_t)t * N * h->inst.obs_dim;
  if (o.reward) o.reward += t * N;
  if (o.discount) o.discount += t * N;
  if (o.terminated) o.terminated += t * N;
  if (o.truncated) o.truncated += t * N;
  if (o.is_success) o.is_success += t * N;
  if (o.step_type) o.step_type += t * N;
  if (o.fault) o.fault += t * N;
  if (o.ncon) o.ncon += t * N;
  return o;
}

// one launch of the demonstration-policy kernel (mjs_policy.h) for the handle's task and action type; arguments validated by the callers
int launch_policy(mjs_handle* h, const double* obs, const double* z, double noise, double* actions, uint8_t* ik_ok, hipStream_t s) {
  pol::PolicyParams p;
  p.N = h->cfg.num_envs;
  p.task = h->cfg.task;
  p.action_type = h->cfg.action_type;
  p.obs_dim = h->inst.obs_dim;
  p.act_dim = h->inst.act_dim;
  p.noise = noise;
  p.obs = obs;
  p.z = noise != 0 ? z : nullptr;
  p.actions = actions;
  p.ik_ok = ik_ok;
  pol::kernel<<<grid_for(p.N), BLOCK, 0, s>>>(p);
  HIP_TRY(h, hipGetLastError());
  return MJS_OK;
}
// what both policy entry points refuse; nullptr = fine
const char* policy_refusal(const mjs_handle* h, double noise, int& code) {
  code = MJS_ERR_UNSUPPORTED;
  if (h->cfg.task == MJS_TASK_PLANAR_PUSH)
    return "Planar-Push has no scripted demonstration policy (the reference's is a keyboard teleop, robot_planar_push.py:288-308)";
  code = MJS_ERR_INVALID_ARG;
  if (!(noise >= 0) || !std::isfinite(noise)) return "noise must be finite and >= 0";
  return nullptr;
}


// The closed loop both policy rollouts run (mjs_rollout_demonstration, mjs_rollout_actor): what it writes besides mjs_outputs ...
struct ClosedLoop {
  double* actions_out;  // [T, N, action_dim]
  uint8_t *scene_rgb, *wrist_rgb;
  int32_t height, width;
};
// ... what it refuses (empty = fine; `arg` names the caller's struct in the text) ...
std::string closed_loop_refusal(const mjs_handle* h, const char* arg, int32_t T, const ClosedLoop& loop, const mjs_outputs* out) {
  if (T < 0) return "T is negative";
  if (!out || !out->obs) return "out->obs is required (the policy of step t reads slice t-1)";
  if (!loop.actions_out) return std::string(arg) + "->actions_out_dev is required";
  if (loop.wrist_rgb && h->cfg.task != MJS_TASK_BUTTON_PUSH) return "a wrist image buffer on a task without a wrist camera";
  if ((loop.scene_rgb || loop.wrist_rgb) && (loop.height <= 0 || loop.width <= 0)) return "image buffers need a positive height and width";
  return "";
}
// ... and the loop: policy(t, obs of step t-1, slice t of actions_out) launches the policy of step t; the frames of the state it has
// just looked at; the ordinary step launch. Arguments validated, the handle's device selected by the caller.
template <class Policy>
int closed_loop(mjs_handle* h, const double* obs0, int32_t T, const ClosedLoop& loop, const mjs_outputs* out, hipStream_t stream, Policy policy) {
  const size_t N = (size_t)h->cfg.num_envs, A = (size_t)h->inst.act_dim, O = (size_t)h->inst.obs_dim;
  const bool images = loop.scene_rgb || loop.wrist_rgb;
  const size_t frame = images ? N * (size_t)loop.height * (size_t)loop.width * 3 : 0;
  for (int32_t t = 0; t < T; t++) {
    const double* obs = t == 0 ? obs0 : out->obs + (size_t)(t - 1) * N * O;
    double* actions = loop.actions_out + (size_t)t * N * A;
    int rc = policy(t, obs, actions);
    if (rc != MJS_OK) return rc;
    if (loop.scene_rgb && (rc = mjs_render(h, MJS_CAMERA_SCENE, loop.height, loop.width, loop.scene_rgb + (size_t)t * frame, stream)) != MJS_OK) return rc;
    if (loop.wrist_rgb && (rc = mjs_render(h, MJS_CAMERA_WRIST, loop.height, loop.width, loop.wrist_rgb + (size_t)t * frame, stream)) != MJS_OK) return rc;
    const mjs_outputs o = slice_outputs(h, out, t);
    h->prims_valid = false;
    rc = launch<false>(h, make_params(h, actions, nullptr, &o), stream);
    if (rc != MJS_OK) return rc;
  }
  return MJS_OK;
}


// what the actor entry points refuse about the pair (handle, actor), `visual` for the two that take feature blocks; empty = fine
std::string actor_refusal(const mjs_handle* h, const mjs_actor* a, const double* low, const double* high, bool visual) {
  if (!a) return "actor is null";
  if (a->visual != visual)
    return visual ? "the actor has no feature blocks (mjs_actor_create): use mjs_actor_actions / mjs_rollout_actor"
                  : "the actor reads feature blocks (mjs_actor_create_visual): use mjs_actor_actions_visual / mjs_rollout_visual_actor";
  if (a->desc.device != h->cfg.device) return "the actor lives on another device than the handle";
  if (!a->loaded) return "the actor has no parameters yet (mjs_actor_load)";
  if (a->desc.action_dim != h->inst.act_dim) return "the actor's action_dim is not the handle's action width";
  if (a->max_index >= h->inst.obs_dim) return "an obs_index entry lies outside the handle's observation row (mjs_env_obs_dim)";
  if (!low || !high) return "low or high is null";
  return "";
}
// what the visual entry points refuse about the feature buffers; empty = fine
std::string features_refusal(const mjs_actor* a, const float* const* features) {
  if (!features) return "features_dev is null";
  for (int b = 0; b < act::MAX_BLOCKS; b++)
    if (a->block_width[b] && !features[b]) return "a feature buffer of a block the actor has is null";
  return "";
}
// one launch of the actor kernel for every env of the handle (features: a visual actor's blocks, nullptr otherwise); arguments
// validated by the callers
int launch_actor(mjs_handle* h, const mjs_actor* a, const double* obs, const float* const* features, const float* z, const double* low, const double* high,
                 double* actions, float* squashed, hipStream_t s) {
  act::ActorParams p;
  std::memset(&p, 0, sizeof p);
  p.N = h->cfg.num_envs;
  p.obs_dim = h->inst.obs_dim;
  p.in_dim = a->in_total;
  p.n_hidden = a->desc.n_hidden;
  p.A = a->desc.action_dim;
  p.activation = a->desc.activation == MJS_ACTIVATION_TANH ? act::ACT_TANH : act::ACT_RELU;
  p.S = act::lds_stride(a->widest);
  p.k0 = a->k0;
  p.w0 = a->width[0]; p.w1 = a->width[1]; p.w2 = a->width[2];
  p.obs_index = a->index_dev;
  p.W0 = a->w[0]; p.W1 = a->w[1]; p.W2 = a->w[2]; p.WH = a->w[3];
  p.B0 = a->b[0]; p.B1 = a->b[1]; p.B2 = a->b[2]; p.BH = a->b[3];
  p.obs = obs;
  p.z = z;
  p.actions = actions;
  p.squashed = squashed;
  for (int k = 0; k < p.A; k++) { p.low[k] = low[k]; p.high[k] = high[k]; }
  // 16 envs per workgroup on the 16x16x4 instruction: at 4096 envs that is one workgroup for each of the 256 CUs, where 32-env
  // tiles leave half of them idle (numbers: DESIGN.md 4, profiles/actor_rollout_timing.txt)
  if (a->visual) {
    act::FeatureInputs fi;
    for (int b = 0; b < act::MAX_BLOCKS; b++) { fi.feat[b] = a->block_width[b] ? features[b] : nullptr; fi.width[b] = a->block_width[b]; }
    act::kernel_visual<<<dim3((unsigned)((p.N + 15) / 16)), act::WAVES * 64, act::lds_bytes(16, a->widest), s>>>(p, fi);
  } else if (a->desc.variant == MJS_ACTOR_VARIANT_TILE32)
    act::kernel<32><<<dim3((unsigned)((p.N + 31) / 32)), act::WAVES * 64, act::lds_bytes(32, a->widest), s>>>(p);
  else
    act::kernel<16><<<dim3((unsigned)((p.N + 15) / 16)), act::WAVES * 64, act::lds_bytes(16, a->widest), s>>>(p);
  HIP_TRY(h, hipGetLastError());
  return MJS_OK;
}
// mjs_actor_actions and (visual: with the feature blocks) mjs_actor_actions_visual
int actor_actions(const char* fn, bool visual, mjs_handle* h, const mjs_actor* actor, const double* obs, const float* const* features, const float* z,
                  const double* low, const double* high, double* actions, float* squashed, void* stream) {
  const std::string name = fn;
  if (!h) return fail(nullptr, MJS_ERR_INVALID_ARG, name + ": null handle");
  std::string why = actor_refusal(h, actor, low, high, visual);
  if (why.empty() && visual) why = features_refusal(actor, features);
  if (!why.empty()) return fail(h, MJS_ERR_INVALID_ARG, name + ": " + why);
  if (!obs || !actions) return fail(h, MJS_ERR_INVALID_ARG, name + ": obs_dev or actions_dev is null");
  DeviceGuard dev_(h->cfg.device);
  HIP_TRY(h, dev_.err);
  return launch_actor(h, actor, obs, features, z, low, high, actions, squashed, (hipStream_t)stream);
}

// the loop of each rollout struct
ClosedLoop loop_of(const mjs_demo_rollout& r) { return {r.actions_out_dev, r.scene_rgb_dev, r.wrist_rgb_dev, r.height, r.width}; }
ClosedLoop loop_of(const mjs_actor_rollout& r) { return {r.actions_out_dev, r.scene_rgb_dev, r.wrist_rgb_dev, r.height, r.width}; }
// (renders nothing itself: the frames are the policy's input, taken in its own launches)
ClosedLoop loop_of(const mjs_visual_rollout& r) { return {r.actions_out_dev, nullptr, nullptr, 0, 0}; }
std::string no_refusal() { return ""; }
// The prologue of the three closed-loop rollouts, in the order they report it: the null handle, the null struct and its struct_size
// (`arg` and `type` name it in the texts), the entry's own refusals, the loop's, the entry's late ones (the visual entry reports its
// buffers after the loop's arguments), T == 0, obs0_dev, the handle's device. own(code) and late() run once `roll` may be read and
// return a text, empty = fine; own may replace the code, MJS_ERR_INVALID_ARG. True: run the loop, `dev` holds the device; false:
// return rc.
template <class Roll, class Own, class Late>
bool rollout_prologue(mjs_handle* h, const std::string& name, const char* arg, const char* type, const Roll* roll, const double* obs0, int32_t T,
                      const mjs_outputs* out, Own own, Late late, ClosedLoop& loop, std::optional<DeviceGuard>& dev, int& rc) {
  const auto refuse = [&](mjs_handle* hh, int code, const std::string& why) { rc = fail(hh, code, name + ": " + why); return false; };
  if (!h) return refuse(nullptr, MJS_ERR_INVALID_ARG, "null handle");
  if (!roll) return refuse(h, MJS_ERR_INVALID_ARG, std::string(arg) + " is null");
  if (roll->struct_size != sizeof(Roll)) return refuse(h, MJS_ERR_INVALID_ARG, std::string(type) + ".struct_size does not match this library's header");
  int code = MJS_ERR_INVALID_ARG;
  std::string why = own(code);
  if (!why.empty()) return refuse(h, code, why);
  loop = loop_of(*roll);
  why = closed_loop_refusal(h, arg, T, loop, out);
  if (why.empty()) why = late();
  if (!why.empty()) return refuse(h, MJS_ERR_INVALID_ARG, why);
  rc = MJS_OK;
  if (T == 0) return false;
  if (!obs0) return refuse(h, MJS_ERR_INVALID_ARG, "obs0_dev is null");
  dev.emplace(h->cfg.device);
  if (dev->err != hipSuccess) { rc = hip_fail(h, dev->err, "dev_.err"); return false; }
  return true;
}
}  // namespace

extern "C" {

#ifndef MJS_SOURCE_HASH
#define MJS_SOURCE_HASH "unhashed"  // the in-tree build (mujoco_sim_amd/_native.py) passes -DMJS_SOURCE_HASH=<sha256 of csrc/ + include/>
#endif
#define MJS_STR2(x) #x
#define MJS_STR(x) MJS_STR2(x)
const char* mjs_version(void) { return "mjsim-hip 0.3 (gfx950, abi " MJS_STR(MJS_ABI_VERSION) ") src=" MJS_SOURCE_HASH; }

int mjs_obs_dim(int task) { const Instance* d = task_defaults(task); return d ? d->obs_dim : -1; }
int mjs_action_dim_for(int task, int action_type) {
  if (task == MJS_TASK_BUTTON_PUSH) return action_type == MJS_ACTION_ABS_EEF ? bp::ACT_DIM_EEF : action_type == MJS_ACTION_ABS_JOINT ? bp::ACT_DIM_JOINT : -1;
  const Instance* d = task_defaults(task);
  return d ? d->act_dim : -1;
}
int mjs_action_dim(int task) { return mjs_action_dim_for(task, MJS_ACTION_ABS_JOINT); }
int mjs_state_dim(int task) { const Instance* d = task_defaults(task); return d ? d->state_dim + 1 : -1; }
int mjs_algorithmic_bytes_per_env_step(int task) { const Instance* d = task_defaults(task); return d ? d->alg_bytes : -1; }
int mjs_env_obs_dim(const mjs_handle* h) { return h ? h->inst.obs_dim : -1; }
int mjs_env_state_dim(const mjs_handle* h) { return h ? h->inst.state_dim + 1 : -1; }
int mjs_env_algorithmic_bytes_per_env_step(const mjs_handle* h) { return h ? h->inst.alg_bytes : -1; }
int mjs_substeps(int task) { return task == MJS_TASK_POINTMASS_REACH ? MJS_PM_NSUB : task_defaults(task) ? MJS_RR_NSUB : -1; }

const char* mjs_last_error(const mjs_handle* h) { return h ? h->err.c_str() : g_err.c_str(); }

#define LDS_OPT_IN(what, kernel, bytes) \
  CREATE_TRY("mjs_create", hipFuncSetAttribute(reinterpret_cast<const void*>(&kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)(bytes)), what)

int mjs_create(const mjs_config* cfg, mjs_handle** out) {
  if (!cfg || !out) return fail(nullptr, MJS_ERR_INVALID_ARG, "mjs_create: null argument");
  *out = nullptr;
  if (cfg->struct_size != sizeof(mjs_config))
    return fail(nullptr, MJS_ERR_INVALID_ARG, "mjs_create: mjs_config.struct_size does not match this library's header (abi " MJS_STR(MJS_ABI_VERSION) "): the caller was built against another include/mjsim.h");
  if (!task_defaults(cfg->task)) return fail(nullptr, MJS_ERR_UNSUPPORTED, "mjs_create: unknown task id");
  if (mjs_action_dim_for(cfg->task, cfg->action_type) < 0) return fail(nullptr, MJS_ERR_INVALID_ARG, "mjs_create: bad action_type");
  if (cfg->gripper_model != MJS_GRIPPER_REDUCED && cfg->gripper_model != MJS_GRIPPER_ARTICULATED) return fail(nullptr, MJS_ERR_INVALID_ARG, "mjs_create: bad gripper_model");
  if (cfg->gripper_model == MJS_GRIPPER_ARTICULATED && cfg->task != MJS_TASK_BUTTON_PUSH)
    return fail(nullptr, MJS_ERR_UNSUPPORTED, "mjs_create: the articulated 2F-85 is built for Button-Push only (Robot-Reach keeps the rigid payload, BASELINE config 3 \"UR5e 6-DoF\")");
  if (cfg->task == MJS_TASK_PLANAR_PUSH && cfg->n_objects > MJS_PP_MAX_OBJECTS) return fail(nullptr, MJS_ERR_INVALID_ARG, "mjs_create: n_objects exceeds MJS_PP_MAX_OBJECTS");
  if (cfg->task == MJS_TASK_PLANAR_PUSH && cfg->block_shape != MJS_BLOCKS_MESH && cfg->block_shape != MJS_BLOCKS_BOX)
    return fail(nullptr, MJS_ERR_INVALID_ARG, "mjs_create: bad block_shape");
  if (cfg->num_envs <= 0) return fail(nullptr, MJS_ERR_INVALID_ARG, "mjs_create: num_envs must be positive");
  if (cfg->autoreset < MJS_AUTORESET_NEXT_STEP || cfg->autoreset > MJS_AUTORESET_DISABLED)
    return fail(nullptr, MJS_ERR_INVALID_ARG, "mjs_create: bad autoreset mode");
  if (int rc = device_refusal("mjs_create", cfg->device)) return rc;
  DeviceGuard dev_(cfg->device);  // ahead of the handle's guard: a failed create frees the handle while its device is still selected
  std::unique_ptr<mjs_handle, void (*)(mjs_handle*)> guard(new (std::nothrow) mjs_handle(), mjs_destroy);  // every early return cleans up
  mjs_handle* h = guard.get();
  if (!h) return fail(nullptr, MJS_ERR_ALLOC, "mjs_create: out of host memory");
  h->cfg = *cfg;
  if (h->cfg.reward_type < 0) h->cfg.reward_type = default_reward(cfg->task);
  if (h->cfg.n_objects <= 0) h->cfg.n_objects = MJS_PP_FAST_OBJECTS;
  if (h->cfg.max_episode_steps <= 0) h->cfg.max_episode_steps = MJS_PP_MAX_CONTROL_STEPS;
  if (!(h->cfg.time_limit > 0)) h->cfg.time_limit = default_time_limit(cfg->task);
  h->inst = resolve_instance(h->cfg);
  default_scene_camera(cfg->task, h->cam);
  const Instance& in = h->inst;
  const size_t N = (size_t)cfg->num_envs;
  CREATE_TRY("mjs_create", dev_.err, "device allocation");
  if (const char* bad_knob = read_ab_knobs(h->inst)) return fail(nullptr, MJS_ERR_INVALID_ARG, bad_knob);
  // > 64 KB of dynamic LDS per workgroup is an opt-in (gfx950 has 160 KB per CU): Planar-Push's cooperative workspaces + hull tables,
  // 16 envs per workgroup of the articulated-gripper kernel at large batches
#ifndef MJS_STAMPS  // the diagnostic build's phase counters live in the env slots: its 5-slot instance does not fit and is not used
  static_assert(pp5::LDS_BYTES <= 160 * 1024, "cooperative workspace exceeds the CU's LDS");
#endif
  static_assert(pp::LDS_BYTES <= 160 * 1024, "cooperative workspace exceeds the CU's LDS");
  static_assert(16 * sizeof(bg::Env) <= 160 * 1024, "16 envs per workgroup fit the CU's LDS");
  if (in.kind == KIND_PUSH2) { LDS_OPT_IN("device allocation", pp::kernel<false>, pp::LDS_BYTES); LDS_OPT_IN("device allocation", pp::kernel<true>, pp::LDS_BYTES); }
  if (in.kind == KIND_PUSH5) { LDS_OPT_IN("device allocation", pp5::kernel<false>, pp5::LDS_BYTES); LDS_OPT_IN("device allocation", pp5::kernel<true>, pp5::LDS_BYTES); }
  CREATE_TRY("mjs_create", hipMalloc(&h->state, sizeof(double) * in.state_dim * N), "device allocation");
  CREATE_TRY("mjs_create", hipMalloc(&h->flags, N), "device allocation");
  CREATE_TRY("mjs_create", hipMalloc(&h->rng_mt, sizeof(uint32_t) * 624 * N), "device allocation");
  CREATE_TRY("mjs_create", hipMalloc(&h->rng_pos, sizeof(int32_t) * N), "device allocation");
  CREATE_TRY("mjs_create", hipMemset(h->state, 0, sizeof(double) * in.state_dim * N), "device allocation");
  if (in.nprim) CREATE_TRY("mjs_create", hipMalloc(&h->prims, sizeof(float) * rend::PRIM_FLOATS * in.nprim * N), "device allocation");  // no allocation in launch paths
  if (cfg->task == MJS_TASK_BUTTON_PUSH) CREATE_TRY("mjs_create", hipMalloc(&h->cams, sizeof(float) * 12 * N), "device allocation");
  if (in.kind == KIND_BUTTON_ARTICULATED) CREATE_TRY("mjs_create", hipMalloc(&h->ws14, sizeof(double) * (size_t)bg::WS_DOUBLES * N), "device allocation");  // 15 KB per env: every row of every env
  if (in.kind != KIND_POINTMASS)  // 3.4 KB per env, touched only by lanes with an arm geom in the floor
    CREATE_TRY("mjs_create", hipMalloc(&h->ws, sizeof(double) * rr::WS_ROWS * N), "device allocation");
#ifdef MJS_STAMPS
  CREATE_TRY("mjs_create", hipMalloc(&h->stamps, sizeof(unsigned long long) * 16 * N), "device allocation");  // one slot block per workgroup, at most N workgroups
  CREATE_TRY("mjs_create", hipMemset(h->stamps, 0, sizeof(unsigned long long) * 16 * N), "device allocation");
#endif
  if (in.kind == KIND_BUTTON_ARTICULATED) {
    LDS_OPT_IN("LDS opt-in", bg::kernel<false>, 16 * sizeof(bg::Env));
    LDS_OPT_IN("LDS opt-in", bg::kernel<true>, 16 * sizeof(bg::Env));
    // the compiled 14-body model: a __device__ global of this device, the same constants for every handle
    static const bg::Model host_model = [] { bg::Model m; std::memset(&m, 0, sizeof m); bg::build_model(m); return m; }();
    CREATE_TRY("mjs_create", hipMemcpyToSymbol(HIP_SYMBOL(bg::g_model), &host_model, sizeof host_model), "model upload");
  }
  init_kernel<<<grid_for((int)N), BLOCK>>>(h->state, h->flags, (int)N, cfg->task, host_pending_byte(h));
  if (in.prog_row >= 0) fill_row_kernel<<<grid_for((int)N), BLOCK>>>(h->state + (size_t)in.prog_row * N, (int)N, -1.0);  // no next episode prepared
  seed_kernel<<<grid_for((int)N), BLOCK>>>(DevRng{h->rng_mt, h->rng_pos, (int)N}, 0u, cfg->env_index_offset);
  CREATE_TRY("mjs_create", hipDeviceSynchronize(), "init kernels");
  *out = guard.release();
  return MJS_OK;
}

void mjs_destroy(mjs_handle* h) {  // the one place that frees what a handle owns
  if (!h) return;
#ifdef MJS_STAMPS
  if (h->stamps) mjs_stamps_report(h->stamps, h->cfg.num_envs, h->cfg.task);
#endif
  free_all({h->state, h->flags, h->rng_mt, h->rng_pos, h->stamps, h->prims, h->bg_ray, h->bg_rgb, h->cams, h->ws, h->ws14});
  delete h;
}

int mjs_seed(mjs_handle* h, uint32_t base_seed, void* stream) {
  if (!h) return fail(nullptr, MJS_ERR_INVALID_ARG, "mjs_seed: null handle");
  DeviceGuard dev_(h->cfg.device);
  HIP_TRY(h, dev_.err);
  seed_kernel<<<grid_for(h->cfg.num_envs), BLOCK, 0, (hipStream_t)stream>>>(DevRng{h->rng_mt, h->rng_pos, h->cfg.num_envs}, base_seed,
                                                                           h->cfg.env_index_offset);
  if (h->inst.prog_row >= 0)  // Planar-Push: episodes prepared from the old streams are void
    fill_row_kernel<<<grid_for(h->cfg.num_envs), BLOCK, 0, (hipStream_t)stream>>>(h->state + (size_t)h->inst.prog_row * h->cfg.num_envs, h->cfg.num_envs, -1.0);
  HIP_TRY(h, hipGetLastError());
  return MJS_OK;
}

int mjs_reset(mjs_handle* h, const uint8_t* mask_dev, const mjs_outputs* out, void* stream) {
  if (!h) return fail(nullptr, MJS_ERR_INVALID_ARG, "mjs_reset: null handle");
  DeviceGuard dev_(h->cfg.device);
  HIP_TRY(h, dev_.err);
  h->prims_valid = false;
  return launch<true>(h, make_params(h, nullptr, mask_dev, out), (hipStream_t)stream);
}

int mjs_step(mjs_handle* h, const double* actions_dev, const mjs_outputs* out, void* stream) {
  if (!h) return fail(nullptr, MJS_ERR_INVALID_ARG, "mjs_step: null handle");
  if (!actions_dev) return fail(h, MJS_ERR_INVALID_ARG, "mjs_step: actions_dev is null");
  DeviceGuard dev_(h->cfg.device);
  HIP_TRY(h, dev_.err);
  h->prims_valid = false;
  return launch<false>(h, make_params(h, actions_dev, nullptr, out), (hipStream_t)stream);
}

int mjs_rollout(mjs_handle* h, const double* actions_dev, int32_t T, const mjs_outputs* out, void* stream) {
  if (!h) return fail(nullptr, MJS_ERR_INVALID_ARG, "mjs_rollout: null handle");
  if (!actions_dev || T < 0) return fail(h, MJS_ERR_INVALID_ARG, "mjs_rollout: bad arguments");
  DeviceGuard dev_(h->cfg.device);
  HIP_TRY(h, dev_.err);
  h->prims_valid = false;
  const size_t N = (size_t)h->cfg.num_envs;
  for (int32_t t = 0; t < T; t++) {
    const mjs_outputs o = slice_outputs(h, out, t);
    int rc = launch<false>(h, make_params(h, actions_dev + (size_t)t * N * h->inst.act_dim, nullptr, &o), (hipStream_t)stream);
    if (rc != MJS_OK) return rc;
  }
  return MJS_OK;
}

// ---- demonstration policies ----------------------------------------------------------------------------------------------
int mjs_demonstration_actions(mjs_handle* h, const double* obs_dev, const double* noise_z_dev, double noise, double* actions_dev, uint8_t* ik_ok_dev,
                              void* stream) {
  if (!h) return fail(nullptr, MJS_ERR_INVALID_ARG, "mjs_demonstration_actions: null handle");
  int code;
  if (const char* why = policy_refusal(h, noise, code)) return fail(h, code, std::string("mjs_demonstration_actions: ") + why);
  if (!obs_dev || !actions_dev) return fail(h, MJS_ERR_INVALID_ARG, "mjs_demonstration_actions: obs_dev or actions_dev is null");
  DeviceGuard dev_(h->cfg.device);
  HIP_TRY(h, dev_.err);
  return launch_policy(h, obs_dev, noise_z_dev, noise, actions_dev, ik_ok_dev, (hipStream_t)stream);
}

int mjs_rollout_demonstration(mjs_handle* h, const double* obs0_dev, int32_t T, const mjs_demo_rollout* demo, const mjs_outputs* out, void* stream) {
  ClosedLoop loop;
  std::optional<DeviceGuard> dev_;
  int rc;
  const auto own = [&](int& code) -> std::string { const char* why = policy_refusal(h, demo->noise, code); return why ? why : ""; };
  if (!rollout_prologue(h, "mjs_rollout_demonstration", "demo", "mjs_demo_rollout", demo, obs0_dev, T, out, own, no_refusal, loop, dev_, rc)) return rc;
  const size_t N = (size_t)h->cfg.num_envs;
  const size_t k = h->cfg.task == MJS_TASK_POINTMASS_REACH ? 2 : 3;  // noise draws per env
  return closed_loop(h, obs0_dev, T, loop, out, (hipStream_t)stream, [&](int32_t t, const double* obs, double* actions) {
    return launch_policy(h, obs, demo->noise_z_dev ? demo->noise_z_dev + (size_t)t * N * k : nullptr, demo->noise, actions,
                         demo->ik_ok_dev ? demo->ik_ok_dev + (size_t)t * N : nullptr, (hipStream_t)stream);
  });
}

// ---- learned policies: the MLP actor ------------------------------------------------------------------------------------------
// mjs_actor_create (blocks nullptr) and mjs_actor_create_visual
static int actor_create(const char* fn, const mjs_actor_desc* desc, const mjs_actor_feature_inputs* blocks, mjs_actor** out) {
  const std::string name = fn;
  const bool visual = blocks != nullptr;
  if (!desc || !out) return fail(nullptr, MJS_ERR_INVALID_ARG, name + ": null argument");
  *out = nullptr;
  if (desc->struct_size != sizeof(mjs_actor_desc))
    return fail(nullptr, MJS_ERR_INVALID_ARG, name + ": mjs_actor_desc.struct_size does not match this library's header");
  if (desc->in_dim < (visual ? 0 : 1) || desc->in_dim > act::MAX_IN) return fail(nullptr, MJS_ERR_INVALID_ARG, name + (visual ? ": in_dim must be 0..64" : ": in_dim must be 1..64"));
  if (desc->n_hidden < 1 || desc->n_hidden > act::MAX_LAYERS) return fail(nullptr, MJS_ERR_INVALID_ARG, name + ": n_hidden must be 1..3");
  for (int l = 0; l < desc->n_hidden; l++)
    if (desc->hidden[l] < 1 || desc->hidden[l] > act::MAX_HIDDEN) return fail(nullptr, MJS_ERR_INVALID_ARG, name + ": every hidden width must be 1..256");
  if (desc->action_dim < 1 || desc->action_dim > act::MAX_ACT) return fail(nullptr, MJS_ERR_INVALID_ARG, name + ": action_dim must be 1..8");
  if (desc->activation != MJS_ACTIVATION_RELU && desc->activation != MJS_ACTIVATION_TANH) return fail(nullptr, MJS_ERR_INVALID_ARG, name + ": bad activation");
  if (desc->variant != MJS_ACTOR_VARIANT_DEFAULT && (visual || desc->variant != MJS_ACTOR_VARIANT_TILE32)) return fail(nullptr, MJS_ERR_INVALID_ARG, name + ": bad variant");
  if (desc->in_dim > 0 && !desc->obs_index) return fail(nullptr, MJS_ERR_INVALID_ARG, name + ": obs_index is null");
  for (int j = 0; j < desc->in_dim; j++)
    if (desc->obs_index[j] < 0) return fail(nullptr, MJS_ERR_INVALID_ARG, name + ": an obs_index entry is negative");
  int in_total = desc->in_dim;
  if (visual) {
    if (blocks->struct_size != sizeof(mjs_actor_feature_inputs))
      return fail(nullptr, MJS_ERR_INVALID_ARG, name + ": mjs_actor_feature_inputs.struct_size does not match this library's header");
    int used = 0;
    for (int b = 0; b < act::MAX_BLOCKS; b++) {
      if (blocks->width[b] < 0 || blocks->width[b] > act::MAX_BLOCK_WIDTH) return fail(nullptr, MJS_ERR_INVALID_ARG, name + ": a block width must be 0 (absent) or 1..512");
      used += blocks->width[b] > 0;
      in_total += blocks->width[b];
    }
    if (used < 1 || used != blocks->n_blocks) return fail(nullptr, MJS_ERR_INVALID_ARG, name + ": n_blocks must be 1..2 and count the slots with a positive width");
    for (int b = 0; b < act::MAX_BLOCKS; b++)
      if (blocks->width[b] && (blocks->start[b] < 0 || blocks->start[b] + blocks->width[b] > in_total))
        return fail(nullptr, MJS_ERR_INVALID_ARG, name + ": a block does not lie inside the input vector");
    if (used == 2 && blocks->start[0] < blocks->start[1] + blocks->width[1] && blocks->start[1] < blocks->start[0] + blocks->width[0])
      return fail(nullptr, MJS_ERR_INVALID_ARG, name + ": the blocks overlap");
  }
  if (int rc = device_refusal(name, desc->device)) return rc;
  DeviceGuard dev_(desc->device);
  std::unique_ptr<mjs_actor, void (*)(mjs_actor*)> guard(new (std::nothrow) mjs_actor(), mjs_actor_destroy);
  mjs_actor* a = guard.get();
  if (!a) return fail(nullptr, MJS_ERR_ALLOC, name + ": out of host memory");
  CREATE_TRY(name, dev_.err);
  a->desc = *desc;
  a->visual = visual;
  a->in_total = in_total;
  for (int j = 0; j < desc->in_dim; j++) a->max_index = desc->obs_index[j] > a->max_index ? desc->obs_index[j] : a->max_index;
  if (!visual) {
    a->index.assign(desc->obs_index, desc->obs_index + desc->in_dim);
  } else {
    // the input vector, position by position: a block's component (act::FeatureInputs' encoding) or the next observation column
    a->index.assign((size_t)in_total, 0);
    std::vector<bool> taken((size_t)in_total, false);
    for (int b = 0; b < act::MAX_BLOCKS; b++) {
      a->block_width[b] = blocks->width[b];
      for (int f = 0; f < blocks->width[b]; f++) {
        a->index[(size_t)(blocks->start[b] + f)] = -(1 + act::MAX_BLOCK_WIDTH * b + f);
        taken[(size_t)(blocks->start[b] + f)] = true;
      }
    }
    for (int j = 0, col = 0; j < in_total; j++)
      if (!taken[(size_t)j]) a->index[(size_t)j] = desc->obs_index[col++];
  }
  a->desc.obs_index = visual ? nullptr : a->index.data();
  a->k0 = act::round_up(in_total, act::KPAD);
  a->widest = a->k0 > act::OPAD ? a->k0 : act::OPAD;
  for (int l = 0; l < desc->n_hidden; l++) {
    a->width[l] = act::round_up(desc->hidden[l], act::OPAD);
    a->widest = a->width[l] > a->widest ? a->width[l] : a->widest;
  }
  CREATE_TRY(name, hipMalloc(&a->index_dev, sizeof(int32_t) * a->index.size()));
  CREATE_TRY(name, hipMemcpy(a->index_dev, a->index.data(), sizeof(int32_t) * a->index.size(), hipMemcpyHostToDevice));
  int K = a->k0;
  for (int l = 0; l < desc->n_hidden; l++) {
    CREATE_TRY(name, hipMalloc(&a->w[l], sizeof(float) * (size_t)K * a->width[l]));
    CREATE_TRY(name, hipMalloc(&a->b[l], sizeof(float) * a->width[l]));
    K = a->width[l];
  }
  CREATE_TRY(name, hipMalloc(&a->w[3], sizeof(float) * (size_t)K * act::OPAD));
  CREATE_TRY(name, hipMalloc(&a->b[3], sizeof(float) * act::OPAD));
  // the two LDS images of the 32-env kernel pass 64 KB from a widest layer of 256 on: an opt-in (gfx950 has 160 KB per CU); so do
  // those of the visual kernel from a first layer of 512 inputs on
  constexpr int VISUAL_WIDEST = act::round_up(act::MAX_IN + act::MAX_BLOCKS * act::MAX_BLOCK_WIDTH, act::KPAD);
  static_assert(act::lds_bytes(32, act::MAX_HIDDEN) <= 160 * 1024 && act::lds_bytes(16, act::MAX_HIDDEN) <= 64 * 1024 && act::lds_bytes(16, VISUAL_WIDEST) <= 160 * 1024,
                "LDS images of the actor kernels");
  if (desc->variant == MJS_ACTOR_VARIANT_TILE32)
    CREATE_TRY(name, hipFuncSetAttribute(reinterpret_cast<const void*>(&act::kernel<32>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)act::lds_bytes(32, act::MAX_HIDDEN)));
  if (visual)
    CREATE_TRY(name, hipFuncSetAttribute(reinterpret_cast<const void*>(&act::kernel_visual), hipFuncAttributeMaxDynamicSharedMemorySize, (int)act::lds_bytes(16, VISUAL_WIDEST)));
  *out = guard.release();
  return MJS_OK;
}
int mjs_actor_create(const mjs_actor_desc* desc, mjs_actor** out) { return actor_create("mjs_actor_create", desc, nullptr, out); }
int mjs_actor_create_visual(const mjs_actor_desc* desc, const mjs_actor_feature_inputs* blocks, mjs_actor** out) {
  if (!blocks) return fail(nullptr, MJS_ERR_INVALID_ARG, "mjs_actor_create_visual: blocks is null");
  return actor_create("mjs_actor_create_visual", desc, blocks, out);
}

void mjs_actor_destroy(mjs_actor* a) {
  if (!a) return;
  free_all({a->index_dev, a->w[0], a->w[1], a->w[2], a->w[3], a->b[0], a->b[1], a->b[2], a->b[3]});
  delete a;
}

int mjs_actor_load(mjs_actor* a, const mjs_actor_weights* wts, void* stream) {
  if (!a || !wts) return fail(nullptr, MJS_ERR_INVALID_ARG, "mjs_actor_load: null argument");
  if (wts->struct_size != sizeof(mjs_actor_weights))
    return fail(nullptr, MJS_ERR_INVALID_ARG, "mjs_actor_load: mjs_actor_weights.struct_size does not match this library's header");
  for (int l = 0; l < a->desc.n_hidden; l++)
    if (!wts->hidden_w[l] || !wts->hidden_b[l]) return fail(nullptr, MJS_ERR_INVALID_ARG, "mjs_actor_load: a hidden layer's weight or bias is null");
  if (!wts->mu_w || !wts->mu_b || !wts->log_std_w || !wts->log_std_b) return fail(nullptr, MJS_ERR_INVALID_ARG, "mjs_actor_load: a head's weight or bias is null");
  DeviceGuard dev_(a->desc.device);
  HIP_TRY(nullptr, dev_.err);
  int in = a->in_total, K = a->k0;
  for (int l = 0; l <= a->desc.n_hidden; l++) {
    const bool head = l == a->desc.n_hidden;
    act::PackParams p;
    p.w0 = head ? wts->mu_w : wts->hidden_w[l];
    p.b0 = head ? wts->mu_b : wts->hidden_b[l];
    p.w1 = head ? wts->log_std_w : nullptr;
    p.b1 = head ? wts->log_std_b : nullptr;
    p.out0 = head ? a->desc.action_dim : a->desc.hidden[l];
    p.out1 = head ? a->desc.action_dim : 0;
    p.in = in;
    p.K = K;
    p.O = head ? act::OPAD : a->width[l];
    p.dst_w = a->w[head ? 3 : l];
    p.dst_b = a->b[head ? 3 : l];
    act::pack_kernel<<<dim3((unsigned)((p.K * p.O + 255) / 256)), 256, 0, (hipStream_t)stream>>>(p);
    if (!head) { in = a->desc.hidden[l]; K = a->width[l]; }
  }
  HIP_TRY(nullptr, hipGetLastError());
  a->loaded = true;
  return MJS_OK;
}

int mjs_actor_actions(mjs_handle* h, const mjs_actor* actor, const double* obs_dev, const float* z_dev, const double* low, const double* high,
                      double* actions_dev, float* squashed_out_dev, void* stream) {
  return actor_actions("mjs_actor_actions", false, h, actor, obs_dev, nullptr, z_dev, low, high, actions_dev, squashed_out_dev, stream);
}

int mjs_rollout_actor(mjs_handle* h, const mjs_actor* actor, const double* obs0_dev, int32_t T, const mjs_actor_rollout* roll, const mjs_outputs* out,
                      void* stream) {
  ClosedLoop loop;
  std::optional<DeviceGuard> dev_;
  int rc;
  const auto own = [&](int&) { return actor_refusal(h, actor, roll->low, roll->high, false); };
  if (!rollout_prologue(h, "mjs_rollout_actor", "roll", "mjs_actor_rollout", roll, obs0_dev, T, out, own, no_refusal, loop, dev_, rc)) return rc;
  const size_t NA = (size_t)h->cfg.num_envs * (size_t)h->inst.act_dim;
  return closed_loop(h, obs0_dev, T, loop, out, (hipStream_t)stream, [&](int32_t t, const double* obs, double* actions) {
    return launch_actor(h, actor, obs, nullptr, roll->z_dev ? roll->z_dev + (size_t)t * NA : nullptr, roll->low, roll->high, actions,
                        roll->squashed_out_dev ? roll->squashed_out_dev + (size_t)t * NA : nullptr, (hipStream_t)stream);
  });
}

// ---- visual policies: the NatureCNN encoder, feature blocks in the actor ----------------------------------------------------
int mjs_encoder_create(const mjs_encoder_desc* desc, mjs_encoder** out) {
  if (!desc || !out) return fail(nullptr, MJS_ERR_INVALID_ARG, "mjs_encoder_create: null argument");
  *out = nullptr;
  if (desc->struct_size != sizeof(mjs_encoder_desc))
    return fail(nullptr, MJS_ERR_INVALID_ARG, "mjs_encoder_create: mjs_encoder_desc.struct_size does not match this library's header");
  if (desc->height < enc::MIN_HW || desc->height > enc::MAX_HW || desc->width < enc::MIN_HW || desc->width > enc::MAX_HW)
    return fail(nullptr, MJS_ERR_INVALID_ARG, "mjs_encoder_create: height and width must each be 36..96");
  if (desc->channels != enc::C_IN) return fail(nullptr, MJS_ERR_INVALID_ARG, "mjs_encoder_create: channels must be 3");
  if (desc->features_dim < 1 || desc->features_dim > enc::MAX_F) return fail(nullptr, MJS_ERR_INVALID_ARG, "mjs_encoder_create: features_dim must be 1..512");
  if (int rc = device_refusal("mjs_encoder_create", desc->device)) return rc;
  DeviceGuard dev_(desc->device);
  std::unique_ptr<mjs_encoder, void (*)(mjs_encoder*)> guard(new (std::nothrow) mjs_encoder(), mjs_encoder_destroy);
  mjs_encoder* e = guard.get();
  if (!e) return fail(nullptr, MJS_ERR_ALLOC, "mjs_encoder_create: out of host memory");
  CREATE_TRY("mjs_encoder_create", dev_.err);
  e->desc = *desc;
  e->g = enc::geometry(desc->height, desc->width);
  e->Fp = act::round_up(desc->features_dim, enc::FPAD);
  const size_t wsize[4] = {(size_t)8 * 8 * enc::C_IN * enc::C1, (size_t)4 * 4 * enc::C1 * enc::C2, (size_t)3 * 3 * enc::C2 * enc::C3, (size_t)e->g.n_flatten * e->Fp};
  const size_t bsize[4] = {(size_t)enc::C1, (size_t)enc::C2, (size_t)enc::C3, (size_t)e->Fp};
  for (int l = 0; l < 4; l++) {
    CREATE_TRY("mjs_encoder_create", hipMalloc(&e->w[l], sizeof(float) * wsize[l]));
    CREATE_TRY("mjs_encoder_create", hipMalloc(&e->b[l], sizeof(float) * bsize[l]));
  }
  // one env's image and activations pass 64 KB of LDS from about 72x72 on: an opt-in (gfx950 has 160 KB per CU)
  CREATE_TRY("mjs_encoder_create", hipFuncSetAttribute(reinterpret_cast<const void*>(&enc::conv_kernel), hipFuncAttributeMaxDynamicSharedMemorySize,
                              (int)enc::lds_bytes(enc::geometry(enc::MAX_HW, enc::MAX_HW))));
  *out = guard.release();
  return MJS_OK;
}

void mjs_encoder_destroy(mjs_encoder* e) {
  if (!e) return;
  free_all({e->w[0], e->w[1], e->w[2], e->w[3], e->b[0], e->b[1], e->b[2], e->b[3]});
  delete e;
}

int mjs_encoder_load(mjs_encoder* e, const mjs_encoder_weights* wts, void* stream) {
  if (!e || !wts) return fail(nullptr, MJS_ERR_INVALID_ARG, "mjs_encoder_load: null argument");
  if (wts->struct_size != sizeof(mjs_encoder_weights))
    return fail(nullptr, MJS_ERR_INVALID_ARG, "mjs_encoder_load: mjs_encoder_weights.struct_size does not match this library's header");
  if (!wts->conv1_w || !wts->conv1_b || !wts->conv2_w || !wts->conv2_b || !wts->conv3_w || !wts->conv3_b || !wts->fc_w || !wts->fc_b)
    return fail(nullptr, MJS_ERR_INVALID_ARG, "mjs_encoder_load: a weight or bias is null");
  DeviceGuard dev_(e->desc.device);
  HIP_TRY(nullptr, dev_.err);
  const enc::PackConvParams conv[3] = {{wts->conv1_w, wts->conv1_b, enc::C1, enc::C_IN, 8, 8, e->w[0], e->b[0]},
                                       {wts->conv2_w, wts->conv2_b, enc::C2, enc::C1, 4, 4, e->w[1], e->b[1]},
                                       {wts->conv3_w, wts->conv3_b, enc::C3, enc::C2, 3, 3, e->w[2], e->b[2]}};
  for (const enc::PackConvParams& p : conv)
    enc::pack_conv_kernel<<<dim3((unsigned)((p.kh * p.kw * p.cin * p.cout + 255) / 256)), 256, 0, (hipStream_t)stream>>>(p);
  act::PackParams p;  // the linear layer: the actor's packing, one source
  p.w0 = wts->fc_w; p.b0 = wts->fc_b; p.w1 = nullptr; p.b1 = nullptr;
  p.out0 = e->desc.features_dim; p.out1 = 0;
  p.in = e->g.n_flatten; p.K = e->g.n_flatten; p.O = e->Fp;
  p.dst_w = e->w[3]; p.dst_b = e->b[3];
  act::pack_kernel<<<dim3((unsigned)((p.K * p.O + 255) / 256)), 256, 0, (hipStream_t)stream>>>(p);
  HIP_TRY(nullptr, hipGetLastError());
  e->loaded = true;
  return MJS_OK;
}

int mjs_encoder_flat_dim(const mjs_encoder* e) { return e ? e->g.n_flatten : -1; }
uint64_t mjs_encoder_workspace_bytes(const mjs_encoder* e, int32_t n) { return e && n > 0 ? (uint64_t)n * (uint64_t)e->g.n_flatten * sizeof(float) : 0; }

// the two launches of an encoder on the current device; arguments validated by the callers
static int launch_encoder(mjs_handle* h, const mjs_encoder* e, const uint8_t* rgb, int n, void* workspace, float* features, hipStream_t s) {
  enc::ConvParams c;
  c.N = n; c.g = e->g; c.rgb = rgb;
  c.W1 = e->w[0]; c.B1 = e->b[0]; c.W2 = e->w[1]; c.B2 = e->b[1]; c.W3 = e->w[2]; c.B3 = e->b[2];
  c.flat = static_cast<float*>(workspace);
  enc::conv_kernel<<<dim3((unsigned)n), enc::WAVES * 64, enc::lds_bytes(e->g), s>>>(c);
  enc::FcParams f;
  f.N = n; f.K = e->g.n_flatten; f.F = e->desc.features_dim; f.Fp = e->Fp;
  f.flat = c.flat; f.W = e->w[3]; f.B = e->b[3]; f.out = features;
  enc::fc_kernel<<<dim3((unsigned)((n + enc::FC_TE - 1) / enc::FC_TE)), enc::WAVES * 64, 0, s>>>(f);
  HIP_TRY(h, hipGetLastError());
  return MJS_OK;
}

int mjs_encoder_features(const mjs_encoder* e, const uint8_t* rgb_dev, int32_t n, void* workspace_dev, float* features_dev, void* stream) {
  if (!e) return fail(nullptr, MJS_ERR_INVALID_ARG, "mjs_encoder_features: encoder is null");
  if (n < 0) return fail(nullptr, MJS_ERR_INVALID_ARG, "mjs_encoder_features: n is negative");
  if (!e->loaded) return fail(nullptr, MJS_ERR_INVALID_ARG, "mjs_encoder_features: the encoder has no parameters yet (mjs_encoder_load)");
  if (n == 0) return MJS_OK;
  if (!rgb_dev || !workspace_dev || !features_dev) return fail(nullptr, MJS_ERR_INVALID_ARG, "mjs_encoder_features: rgb_dev, workspace_dev or features_dev is null");
  DeviceGuard dev_(e->desc.device);
  HIP_TRY(nullptr, dev_.err);
  return launch_encoder(nullptr, e, rgb_dev, n, workspace_dev, features_dev, (hipStream_t)stream);
}

int mjs_actor_actions_visual(mjs_handle* h, const mjs_actor* actor, const double* obs_dev, const float* const features_dev[2], const float* z_dev,
                             const double* low, const double* high, double* actions_dev, float* squashed_out_dev, void* stream) {
  return actor_actions("mjs_actor_actions_visual", true, h, actor, obs_dev, features_dev, z_dev, low, high, actions_dev, squashed_out_dev, stream);
}

int mjs_rollout_visual_actor(mjs_handle* h, const mjs_actor* actor, mjs_encoder* const encs[2], const double* obs0_dev, int32_t T,
                             const mjs_visual_rollout* roll, const mjs_outputs* out, void* stream) {
  ClosedLoop loop;
  std::optional<DeviceGuard> dev_;
  int rc;
  int32_t H = 0, W = 0;
  const auto own = [&](int&) -> std::string {
    std::string why = actor_refusal(h, actor, roll->low, roll->high, true);
    if (why.empty()) why = features_refusal(actor, roll->features_dev);
    if (!why.empty()) return why;
    if (!encs) return "enc is null";
    for (int b = 0; b < act::MAX_BLOCKS; b++) {
      const mjs_encoder* e = encs[b];
      if (!e && actor->block_width[b]) return "the actor has a feature block without an encoder";
      if (!e) continue;
      if (b == 1 && h->cfg.task != MJS_TASK_BUTTON_PUSH) return "a wrist encoder on a task without a wrist camera";
      if (!actor->block_width[b]) return "an encoder for a feature block the actor does not have";
      if (e->desc.device != h->cfg.device) return "an encoder lives on another device than the handle";
      if (!e->loaded) return "an encoder has no parameters yet (mjs_encoder_load)";
      if (e->desc.features_dim != actor->block_width[b]) return "an encoder's features_dim is not the actor's block width";
      if (H && (H != e->desc.height || W != e->desc.width)) return "the two encoders have different image sizes";
      H = e->desc.height; W = e->desc.width;
    }
    return "";
  };
  const auto late = [&]() -> std::string {
    if (roll->wrist_rgb_dev && h->cfg.task != MJS_TASK_BUTTON_PUSH) return "a wrist image buffer on a task without a wrist camera";
    if (!roll->workspace_dev) return "roll->workspace_dev is null";
    for (int b = 0; b < act::MAX_BLOCKS; b++)
      if (encs[b] && !(b == 0 ? roll->scene_rgb_dev : roll->wrist_rgb_dev) && !(b == 0 ? roll->scene_scratch_dev : roll->wrist_scratch_dev))
        return "a camera the actor uses has neither a [T, ...] buffer nor a one-step scratch";
    return "";
  };
  if (!rollout_prologue(h, "mjs_rollout_visual_actor", "roll", "mjs_visual_rollout", roll, obs0_dev, T, out, own, late, loop, dev_, rc)) return rc;
  uint8_t* const block_frames[2] = {roll->scene_rgb_dev, roll->wrist_rgb_dev};
  uint8_t* const scratch[2] = {roll->scene_scratch_dev, roll->wrist_scratch_dev};
  const size_t N = (size_t)h->cfg.num_envs, NA = N * (size_t)h->inst.act_dim, frame = N * (size_t)H * (size_t)W * 3;
  const hipStream_t s = (hipStream_t)stream;
  return closed_loop(h, obs0_dev, T, loop, out, s, [&](int32_t t, const double* obs, double* actions) {
    for (int b = 0; b < act::MAX_BLOCKS; b++) {
      if (!encs[b] && !block_frames[b]) continue;
      uint8_t* rgb = block_frames[b] ? block_frames[b] + (size_t)t * frame : scratch[b];
      int rc = mjs_render(h, b == 0 ? MJS_CAMERA_SCENE : MJS_CAMERA_WRIST, H, W, rgb, stream);
      if (rc == MJS_OK && encs[b]) rc = launch_encoder(h, encs[b], rgb, (int)N, roll->workspace_dev, roll->features_dev[b], s);
      if (rc != MJS_OK) return rc;
    }
    return launch_actor(h, actor, obs, roll->features_dev, roll->z_dev ? roll->z_dev + (size_t)t * NA : nullptr, roll->low, roll->high, actions,
                        roll->squashed_out_dev ? roll->squashed_out_dev + (size_t)t * NA : nullptr, s);
  });
}

// ---- replay buffer (mjs_replay.h) ---------------------------------------------------------------------------------------
// what mjs_replay_add / mjs_replay_sample refuse about a storage descriptor; empty = fine
static std::string replay_storage_refusal(const mjs_replay_storage* st) {
  if (!st) return "storage is null";
  if (st->struct_size != sizeof(mjs_replay_storage)) return "mjs_replay_storage.struct_size does not match this library's header";
  if (st->capacity < 1) return "capacity must be at least 1";
  if (st->obs_dim < 0 || st->obs_dim > rpl::MAX_D) return "obs_dim must be 0..64";
  if (st->action_dim < 1 || st->action_dim > rpl::MAX_A) return "action_dim must be 1..8";
  if (st->n_cameras < 0 || st->n_cameras > rpl::MAX_CAM) return "n_cameras must be 0..2";
  if (st->n_cameras > 0 && (st->height < 1 || st->width < 1)) return "cameras need a positive height and width";
  if (!st->cursor_dev) return "cursor_dev is null";
  if (st->obs_dim > 0 && (!st->obs || !st->next_obs)) return "the storage's obs or next_obs is null";
  if (!st->actions || !st->rewards || !st->dones || !st->timeouts) return "the storage's actions, rewards, dones or timeouts is null";
  for (int c = 0; c < st->n_cameras; c++)
    if (!st->rgb[c] || !st->next_rgb[c]) return "the storage's rgb or next_rgb of a camera is null";
  return "";
}

uint64_t mjs_replay_workspace_bytes(int32_t T, int32_t N) { return T > 0 && N > 0 ? (uint64_t)rpl::ws_bytes((int64_t)T * N) : 0; }

int mjs_replay_add(const mjs_replay_storage* st, const mjs_replay_block* blk, void* workspace_dev, void* stream) {
  const auto refuse = [](const std::string& why) { return fail(nullptr, MJS_ERR_INVALID_ARG, "mjs_replay_add: " + why); };
  if (std::string why = replay_storage_refusal(st); !why.empty()) return refuse(why);
  if (!blk) return refuse("block is null");
  if (blk->struct_size != sizeof(mjs_replay_block)) return refuse("mjs_replay_block.struct_size does not match this library's header");
  if (blk->T < 0) return refuse("T is negative");
  if (blk->N < 1) return refuse("N must be positive");
  if (blk->autoreset != MJS_AUTORESET_NEXT_STEP && blk->autoreset != MJS_AUTORESET_SAME_STEP)
    return refuse("the block's autoreset must be next-step or same-step (with auto-reset disabled a finished env stops producing transitions)");
  const bool same_step = blk->autoreset == MJS_AUTORESET_SAME_STEP;
  if (same_step && st->n_cameras > 0) return refuse("images under same-step auto-reset: the frame of the terminal state does not exist");
  if (blk->src_dim < 1) return refuse("src_dim must be positive");
  if (st->obs_dim > 0 && !blk->obs_index) return refuse("obs_index is null");
  for (int j = 0; j < st->obs_dim; j++)
    if (blk->obs_index[j] < 0 || blk->obs_index[j] >= blk->src_dim) return refuse("an obs_index entry lies outside the source row");
  const int64_t rows = (int64_t)blk->T * blk->N;
  if (rows > st->capacity) return refuse("T * N exceeds the capacity");
  if (blk->T == 0) return MJS_OK;
  if (!blk->obs0 || !blk->obs || !blk->reward || !blk->terminated || !blk->truncated || !blk->squashed_actions)
    return refuse("obs0, obs, reward, terminated, truncated or squashed_actions is null");
  if (same_step && !blk->terminal_obs) return refuse("same-step auto-reset needs terminal_obs");
  if (!same_step && !blk->step_type) return refuse("next-step auto-reset needs step_type");
  for (int c = 0; c < st->n_cameras; c++)
    if (!blk->rgb[c] || !blk->final_rgb[c]) return refuse("the block's rgb or final_rgb of a camera is null");
  if (st->n_cameras > 0 && rows * rpl::THREADS >= ((int64_t)1 << 32)) return refuse("a block with images holds at most 2^24 - 1 rows");
  if (!workspace_dev) return refuse("workspace_dev is null");
  if (int rc = device_refusal("mjs_replay_add", st->device)) return rc;
  DeviceGuard dev_(st->device);
  HIP_TRY(nullptr, dev_.err);

  rpl::AddParams p{};
  p.rows = rows; p.T = blk->T; p.N = blk->N; p.src_dim = blk->src_dim; p.same_step = same_step;
  p.D = st->obs_dim; p.A = st->action_dim; p.n_cam = st->n_cameras; p.capacity = st->capacity;
  p.frame_bytes = (uint64_t)st->height * (uint64_t)st->width * 3;
  p.cursor = reinterpret_cast<unsigned long long*>(st->cursor_dev);
  unsigned char* ws = static_cast<unsigned char*>(workspace_dev);
  p.base = reinterpret_cast<unsigned long long*>(ws);
  p.offsets = reinterpret_cast<uint32_t*>(ws + rpl::WS_HEADER);
  p.dest = reinterpret_cast<int32_t*>(ws + rpl::WS_HEADER + rpl::ws_offsets_bytes(rows));
  p.obs0 = blk->obs0; p.obs = blk->obs; p.terminal_obs = blk->terminal_obs; p.reward = blk->reward;
  p.terminated = blk->terminated; p.truncated = blk->truncated; p.step_type = blk->step_type; p.squashed = blk->squashed_actions;
  p.s_obs = st->obs; p.s_next_obs = st->next_obs; p.s_actions = st->actions; p.s_rewards = st->rewards; p.s_dones = st->dones; p.s_timeouts = st->timeouts;
  for (int c = 0; c < st->n_cameras; c++) {
    p.rgb[c] = blk->rgb[c]; p.final_rgb[c] = blk->final_rgb[c]; p.s_rgb[c] = st->rgb[c]; p.s_next_rgb[c] = st->next_rgb[c];
  }
  for (int j = 0; j < st->obs_dim; j++) p.index.v[j] = blk->obs_index[j];
  const hipStream_t s = (hipStream_t)stream;
  const dim3 chunks((unsigned)rpl::n_chunks(rows));
  rpl::count_kernel<<<chunks, rpl::THREADS, 0, s>>>(p);
  rpl::scan_kernel<<<dim3(1), rpl::THREADS, 0, s>>>(p);
  rpl::scatter_kernel<<<chunks, rpl::THREADS, 0, s>>>(p);
  if (p.n_cam > 0) rpl::image_kernel<<<dim3((unsigned)rows), rpl::THREADS, 0, s>>>(p);
  HIP_TRY(nullptr, hipGetLastError());
  return MJS_OK;
}

int mjs_replay_sample(const mjs_replay_storage* st, const int64_t* draws_dev, int32_t B, const mjs_replay_batch* out, void* stream) {
  const auto refuse = [](const std::string& why) { return fail(nullptr, MJS_ERR_INVALID_ARG, "mjs_replay_sample: " + why); };
  if (std::string why = replay_storage_refusal(st); !why.empty()) return refuse(why);
  if (!out) return refuse("out is null");
  if (out->struct_size != sizeof(mjs_replay_batch)) return refuse("mjs_replay_batch.struct_size does not match this library's header");
  if (B < 0) return refuse("B is negative");
  if (B == 0) return MJS_OK;
  if (!draws_dev) return refuse("draws_dev is null");
  if (int rc = device_refusal("mjs_replay_sample", st->device)) return rc;
  DeviceGuard dev_(st->device);
  HIP_TRY(nullptr, dev_.err);

  rpl::SampleParams p{};
  p.B = B; p.D = st->obs_dim; p.A = st->action_dim; p.n_cam = st->n_cameras; p.capacity = st->capacity;
  p.frame_bytes = (uint64_t)st->height * (uint64_t)st->width * 3;
  p.cursor = reinterpret_cast<const unsigned long long*>(st->cursor_dev);
  p.draws = draws_dev;
  p.s_obs = st->obs; p.s_next_obs = st->next_obs; p.s_actions = st->actions; p.s_rewards = st->rewards; p.s_dones = st->dones; p.s_timeouts = st->timeouts;
  p.idx_out = out->idx_out;
  p.obs = st->obs_dim > 0 ? out->obs : nullptr; p.next_obs = st->obs_dim > 0 ? out->next_obs : nullptr;
  p.actions = out->actions; p.rewards = out->rewards; p.dones = out->dones; p.timeouts = out->timeouts;
  bool images = false;
  for (int c = 0; c < st->n_cameras; c++) {
    p.s_rgb[c] = st->rgb[c]; p.s_next_rgb[c] = st->next_rgb[c]; p.rgb[c] = out->rgb[c]; p.next_rgb[c] = out->next_rgb[c];
    images = images || out->rgb[c] || out->next_rgb[c];
  }
  if (images && (int64_t)B * rpl::THREADS >= ((int64_t)1 << 32)) return refuse("a batch with images holds at most 2^24 - 1 rows");
  const hipStream_t s = (hipStream_t)stream;
  rpl::sample_kernel<<<dim3((unsigned)(((int64_t)B + rpl::SAMPLE_ROWS - 1) / rpl::SAMPLE_ROWS)), rpl::THREADS, 0, s>>>(p);
  if (images) rpl::sample_image_kernel<<<dim3((unsigned)B), rpl::THREADS, 0, s>>>(p);
  HIP_TRY(nullptr, hipGetLastError());
  return MJS_OK;
}

// ---- SAC's critics and the fused TD target (mjs_critic.h) ---------------------------------------------------------------------
int mjs_critic_create(const mjs_critic_desc* desc, mjs_critic** out) {
  const std::string name = "mjs_critic_create";
  if (!desc || !out) return fail(nullptr, MJS_ERR_INVALID_ARG, name + ": null argument");
  *out = nullptr;
  if (desc->struct_size != sizeof(mjs_critic_desc))
    return fail(nullptr, MJS_ERR_INVALID_ARG, name + ": mjs_critic_desc.struct_size does not match this library's header");
  if (desc->obs_dim < 1 || desc->obs_dim > crit::MAX_OBS) return fail(nullptr, MJS_ERR_INVALID_ARG, name + ": obs_dim must be 1..64");
  if (desc->action_dim < 1 || desc->action_dim > crit::MAX_ACT) return fail(nullptr, MJS_ERR_INVALID_ARG, name + ": action_dim must be 1..8");
  if (desc->n_critics < 1 || desc->n_critics > crit::MAX_CRITICS) return fail(nullptr, MJS_ERR_INVALID_ARG, name + ": n_critics must be 1..2");
  if (desc->n_hidden < 1 || desc->n_hidden > act::MAX_LAYERS) return fail(nullptr, MJS_ERR_INVALID_ARG, name + ": n_hidden must be 1..3");
  for (int l = 0; l < desc->n_hidden; l++)
    if (desc->hidden[l] < 1 || desc->hidden[l] > act::MAX_HIDDEN) return fail(nullptr, MJS_ERR_INVALID_ARG, name + ": every hidden width must be 1..256");
  if (desc->activation != MJS_ACTIVATION_RELU && desc->activation != MJS_ACTIVATION_TANH) return fail(nullptr, MJS_ERR_INVALID_ARG, name + ": bad activation");
  if (int rc = device_refusal(name, desc->device)) return rc;
  DeviceGuard dev_(desc->device);
  std::unique_ptr<mjs_critic, void (*)(mjs_critic*)> guard(new (std::nothrow) mjs_critic(), mjs_critic_destroy);
  mjs_critic* q = guard.get();
  if (!q) return fail(nullptr, MJS_ERR_ALLOC, name + ": out of host memory");
  CREATE_TRY(name, dev_.err);
  q->desc = *desc;
  q->k0 = act::round_up(desc->obs_dim + desc->action_dim, act::KPAD);
  q->widest = q->k0 > act::OPAD ? q->k0 : act::OPAD;
  for (int l = 0; l < desc->n_hidden; l++) {
    q->width[l] = act::round_up(desc->hidden[l], act::OPAD);
    q->widest = q->width[l] > q->widest ? q->width[l] : q->widest;
  }
  for (int c = 0; c < desc->n_critics; c++) {
    int K = q->k0;
    for (int l = 0; l < desc->n_hidden; l++) {
      CREATE_TRY(name, hipMalloc(&q->w[c][l], sizeof(float) * (size_t)K * q->width[l]));
      CREATE_TRY(name, hipMalloc(&q->b[c][l], sizeof(float) * q->width[l]));
      K = q->width[l];
    }
    CREATE_TRY(name, hipMalloc(&q->w[c][3], sizeof(float) * (size_t)K * act::OPAD));
    CREATE_TRY(name, hipMalloc(&q->b[c][3], sizeof(float) * act::OPAD));
  }
  // three images of the widest stride any actor / critic pair can ask for stay below the 64 KB no kernel needs an opt-in for
  static_assert(crit::MAX_K0 <= act::MAX_HIDDEN && crit::lds_bytes(act::MAX_HIDDEN) <= 64 * 1024, "LDS images of the critic kernels");
  *out = guard.release();
  return MJS_OK;
}

void mjs_critic_destroy(mjs_critic* q) {
  if (!q) return;
  for (int c = 0; c < crit::MAX_CRITICS; c++) free_all({q->w[c][0], q->w[c][1], q->w[c][2], q->w[c][3], q->b[c][0], q->b[c][1], q->b[c][2], q->b[c][3]});
  delete q;
}

int mjs_critic_load(mjs_critic* q, const mjs_critic_weights* wts, double tau, void* stream) {
  const auto refuse = [](const std::string& why) { return fail(nullptr, MJS_ERR_INVALID_ARG, "mjs_critic_load: " + why); };
  if (!q || !wts) return refuse("null argument");
  if (wts->struct_size != sizeof(mjs_critic_weights)) return refuse("mjs_critic_weights.struct_size does not match this library's header");
  if (!(tau > 0.0 && tau <= 1.0)) return refuse("tau must lie in (0, 1]");
  if (!q->loaded && tau != 1.0) return refuse("a first load must have tau == 1 (there is nothing to blend with yet)");
  for (int c = 0; c < q->desc.n_critics; c++) {
    for (int l = 0; l < q->desc.n_hidden; l++)
      if (!wts->hidden_w[c][l] || !wts->hidden_b[c][l]) return refuse("a hidden layer's weight or bias is null");
    if (!wts->out_w[c] || !wts->out_b[c]) return refuse("a head's weight or bias is null");
  }
  DeviceGuard dev_(q->desc.device);
  HIP_TRY(nullptr, dev_.err);
  for (int c = 0; c < q->desc.n_critics; c++) {
    int in = q->desc.obs_dim + q->desc.action_dim, K = q->k0;
    for (int l = 0; l <= q->desc.n_hidden; l++) {
      const bool head = l == q->desc.n_hidden;
      act::PackParams p;
      p.w0 = head ? wts->out_w[c] : wts->hidden_w[c][l];
      p.b0 = head ? wts->out_b[c] : wts->hidden_b[c][l];
      p.w1 = p.b1 = nullptr;
      p.out0 = head ? 1 : q->desc.hidden[l];
      p.out1 = 0;
      p.in = in;
      p.K = K;
      p.O = head ? act::OPAD : q->width[l];
      p.dst_w = q->w[c][head ? 3 : l];
      p.dst_b = q->b[c][head ? 3 : l];
      const dim3 grid((unsigned)((p.K * p.O + 255) / 256));
      if (tau == 1.0) act::pack_kernel<<<grid, 256, 0, (hipStream_t)stream>>>(p);  // the plain copy: never reads the destination
      else crit::pack_lerp_kernel<<<grid, 256, 0, (hipStream_t)stream>>>(p, (float)(1.0 - tau), (float)tau);
      if (!head) { in = q->desc.hidden[l]; K = q->width[l]; }
    }
  }
  HIP_TRY(nullptr, hipGetLastError());
  q->loaded = true;
  return MJS_OK;
}

// the kernels' view of one packed network: a critic's copy c, or (critic nullptr) the actor's
static crit::Mlp mlp_of(const mjs_critic* q, int c, const mjs_actor* a) {
  crit::Mlp m;
  float* const* w = q ? q->w[c] : a->w;
  float* const* b = q ? q->b[c] : a->b;
  const int* width = q ? q->width : a->width;
  m.W0 = w[0]; m.W1 = w[1]; m.W2 = w[2]; m.WH = w[3];
  m.B0 = b[0]; m.B1 = b[1]; m.B2 = b[2]; m.BH = b[3];
  m.n_hidden = q ? q->desc.n_hidden : a->desc.n_hidden;
  m.k0 = q ? q->k0 : a->k0;
  m.w0 = width[0]; m.w1 = width[1]; m.w2 = width[2];
  m.activation = (q ? q->desc.activation : a->desc.activation) == MJS_ACTIVATION_TANH ? act::ACT_TANH : act::ACT_RELU;
  return m;
}
static crit::CriticParams critic_params(const mjs_critic* q, int32_t B, int widest) {
  crit::CriticParams p{};
  p.B = B; p.D = q->desc.obs_dim; p.A = q->desc.action_dim; p.n_critics = q->desc.n_critics;
  p.S = act::lds_stride(widest);
  for (int c = 0; c < q->desc.n_critics; c++) p.net[c] = mlp_of(q, c, nullptr);
  return p;
}

int mjs_critic_q(const mjs_critic* q, const float* obs_dev, const float* actions_dev, int32_t B, float* q_out_dev, void* stream) {
  const auto refuse = [](const std::string& why) { return fail(nullptr, MJS_ERR_INVALID_ARG, "mjs_critic_q: " + why); };
  if (!q) return refuse("critic is null");
  if (!q->loaded) return refuse("the critic has no parameters yet (mjs_critic_load)");
  if (B < 0) return refuse("B is negative");
  if (B == 0) return MJS_OK;
  if (!obs_dev || !actions_dev || !q_out_dev) return refuse("obs_dev, actions_dev or q_out_dev is null");
  DeviceGuard dev_(q->desc.device);
  HIP_TRY(nullptr, dev_.err);
  const crit::CriticParams p = critic_params(q, B, q->widest);
  crit::q_kernel<<<dim3((unsigned)(((int64_t)B + crit::ROWS - 1) / crit::ROWS)), act::WAVES * 64, crit::lds_bytes(q->widest), (hipStream_t)stream>>>(p, obs_dev, actions_dev, q_out_dev);
  HIP_TRY(nullptr, hipGetLastError());
  return MJS_OK;
}

// what mjs_sac_td_target refuses; "" = fine
static std::string td_refusal(const mjs_actor* actor, const mjs_critic* q, const mjs_td_target_args* args) {
  if (!actor || !q || !args) return "actor, critic or args is null";
  if (args->struct_size != sizeof(mjs_td_target_args)) return "mjs_td_target_args.struct_size does not match this library's header";
  if (actor->visual) return "the actor reads feature blocks (mjs_actor_create_visual): visual critics are not built";
  if (actor->desc.device != q->desc.device) return "the actor lives on another device than the critic";
  if (!actor->loaded) return "the actor has no parameters yet (mjs_actor_load)";
  if (!q->loaded) return "the critic has no parameters yet (mjs_critic_load)";
  if (actor->desc.in_dim != q->desc.obs_dim) return "the actor's in_dim is not the critic's obs_dim";
  if (actor->desc.action_dim != q->desc.action_dim) return "the actor's action_dim is not the critic's";
  if (args->B < 0) return "B is negative";
  if (!(args->gamma >= 0.0 && args->gamma <= 1.0)) return "gamma must lie in [0, 1]";
  if (args->B > 0 && (!args->next_obs_dev || !args->rewards_dev || !args->dones_dev || !args->z_dev || !args->target_out_dev))
    return "next_obs_dev, rewards_dev, dones_dev, z_dev or target_out_dev is null";
  return "";
}

int mjs_sac_td_target(const mjs_actor* actor, const mjs_critic* q, const mjs_td_target_args* args, void* stream) {
  if (std::string why = td_refusal(actor, q, args); !why.empty()) return fail(nullptr, MJS_ERR_INVALID_ARG, "mjs_sac_td_target: " + why);
  if (args->B == 0) return MJS_OK;
  DeviceGuard dev_(q->desc.device);
  HIP_TRY(nullptr, dev_.err);
  const int widest = actor->widest > q->widest ? actor->widest : q->widest;  // one stride for the actor's and the critics' layers
  crit::TdParams p{};
  p.c = critic_params(q, args->B, widest);
  p.actor = mlp_of(nullptr, 0, actor);
  p.next_obs = args->next_obs_dev; p.rewards = args->rewards_dev; p.dones = args->dones_dev; p.z = args->z_dev;
  p.gamma = (float)args->gamma; p.ent_coef = (float)args->ent_coef; p.ent_coef_dev = args->ent_coef_dev;
  p.target = args->target_out_dev; p.next_actions = args->next_actions_out_dev; p.next_log_prob = args->next_log_prob_out_dev; p.q_next = args->q_next_out_dev;
  crit::td_target_kernel<<<dim3((unsigned)(((int64_t)args->B + crit::ROWS - 1) / crit::ROWS)), act::WAVES * 64, crit::lds_bytes(widest), (hipStream_t)stream>>>(p);
  HIP_TRY(nullptr, hipGetLastError());
  return MJS_OK;
}

// ---- the critic update (mjs_critic_train.h) -----------------------------------------------------------------------------------
// where a critic's layers sit in a slab, and its packed copy as the segments' pointers
static crit::Layout layout_of(const mjs_critic* q) {
  crit::Layout L{};
  int at = 0, K = q->k0;
  for (int l = 0; l < 4; l++) {
    const bool used = l < q->desc.n_hidden || l == 3;
    const int O = l == 3 ? act::OPAD : q->width[l];
    L.off[2 * l] = at;
    if (used) at += K * O;
    L.off[2 * l + 1] = at;
    if (used) at += O;
    if (used && l < 3) K = O;
  }
  L.off[8] = at;
  L.total = at + 4;
  return L;
}
static crit::Packed packed_of(const mjs_critic* q, int c) {
  crit::Packed P;
  for (int l = 0; l < 4; l++) { P.seg[2 * l] = q->w[c][l]; P.seg[2 * l + 1] = q->b[c][l]; }
  return P;
}
static bool same_shape(const mjs_critic* a, const mjs_critic* b) {
  bool same = a->desc.obs_dim == b->desc.obs_dim && a->desc.action_dim == b->desc.action_dim && a->desc.n_critics == b->desc.n_critics &&
              a->desc.n_hidden == b->desc.n_hidden && a->desc.activation == b->desc.activation;
  for (int l = 0; same && l < a->desc.n_hidden; l++) same = a->desc.hidden[l] == b->desc.hidden[l];
  return same;
}
// every layer of every critic given? (mjs_critic_weights as inputs or as outputs)
static bool all_layers_given(const mjs_critic* q, const mjs_critic_weights* w) {
  for (int c = 0; c < q->desc.n_critics; c++) {
    for (int l = 0; l < q->desc.n_hidden; l++)
      if (!w->hidden_w[c][l] || !w->hidden_b[c][l]) return false;
    if (!w->out_w[c] || !w->out_b[c]) return false;
  }
  return true;
}
// packed layers (w[c][slot], b[c][slot] of one critic's segments) -> nn.Linear layout, one launch per layer
static void launch_unpack(const mjs_critic* q, const float* const* seg, int c, const mjs_critic_weights* out, hipStream_t s) {
  int in = q->desc.obs_dim + q->desc.action_dim, K = q->k0;
  for (int l = 0; l <= q->desc.n_hidden; l++) {
    const bool head = l == q->desc.n_hidden;
    const int slot = head ? 3 : l;
    crit::UnpackParams p;
    p.src_w = seg[2 * slot]; p.src_b = seg[2 * slot + 1];
    p.K = K; p.O = head ? act::OPAD : q->width[l];
    p.in = in; p.out = head ? 1 : q->desc.hidden[l];
    p.dst_w = const_cast<float*>(head ? out->out_w[c] : out->hidden_w[c][l]);
    p.dst_b = const_cast<float*>(head ? out->out_b[c] : out->hidden_b[c][l]);
    crit::unpack_kernel<<<dim3((unsigned)((p.out * p.in + 255) / 256)), 256, 0, s>>>(p);
    if (!head) { in = q->desc.hidden[l]; K = q->width[l]; }
  }
}

int mjs_critic_opt_create(mjs_critic* q, const mjs_critic_opt_desc* desc, mjs_critic_opt** out) {
  const std::string name = "mjs_critic_opt_create";
  const auto refuse = [&](const std::string& why) { return fail(nullptr, MJS_ERR_INVALID_ARG, name + ": " + why); };
  if (out) *out = nullptr;
  if (!q || !desc || !out) return refuse("null argument");
  if (desc->struct_size != sizeof(mjs_critic_opt_desc)) return refuse("mjs_critic_opt_desc.struct_size does not match this library's header");
  if (!q->loaded) return refuse("the critic has no parameters yet (mjs_critic_load)");
  if (!(desc->lr >= 0.0) || !std::isfinite(desc->lr)) return refuse("lr must be finite and >= 0");
  if (!(desc->beta1 >= 0.0 && desc->beta1 < 1.0) || !(desc->beta2 >= 0.0 && desc->beta2 < 1.0)) return refuse("beta1 and beta2 must lie in [0, 1)");
  if (!(desc->eps > 0.0) || !std::isfinite(desc->eps)) return refuse("eps must be finite and > 0");
  DeviceGuard dev_(q->desc.device);
  std::unique_ptr<mjs_critic_opt, void (*)(mjs_critic_opt*)> guard(new (std::nothrow) mjs_critic_opt(), mjs_critic_opt_destroy);
  mjs_critic_opt* o = guard.get();
  if (!o) return fail(nullptr, MJS_ERR_ALLOC, name + ": out of host memory");
  CREATE_TRY(name, dev_.err);
  o->critic = q;
  o->desc = *desc;
  o->L = layout_of(q);
  const int nc = q->desc.n_critics;
  o->max_splits = crit::splits_max(nc, o->L.total);
  const size_t per = sizeof(float) * (size_t)nc * o->L.total;
  CREATE_TRY(name, hipMalloc(&o->m, per));
  CREATE_TRY(name, hipMalloc(&o->v, per));
  CREATE_TRY(name, hipMalloc(&o->gsum, per));
  CREATE_TRY(name, hipMalloc(&o->slabs, per * o->max_splits));
  CREATE_TRY(name, hipMemset(o->m, 0, per));
  CREATE_TRY(name, hipMemset(o->v, 0, per));
  CREATE_TRY(name, hipDeviceSynchronize());  // the moments are zero before any stream's first step
  // X, three hidden images and the gradient pair of the widest critic pass 64 KB: an opt-in, below the CU's 160 KB
  static_assert(crit::train_lds_bytes(act::MAX_LAYERS, act::MAX_HIDDEN) <= 160 * 1024, "LDS images of grad_kernel");
  CREATE_TRY(name, hipFuncSetAttribute(reinterpret_cast<const void*>(&crit::grad_kernel), hipFuncAttributeMaxDynamicSharedMemorySize,
                                       (int)crit::train_lds_bytes(act::MAX_LAYERS, act::MAX_HIDDEN)));
  *out = guard.release();
  return MJS_OK;
}

void mjs_critic_opt_destroy(mjs_critic_opt* o) {
  if (!o) return;
  free_all({o->m, o->v, o->slabs, o->gsum});
  delete o;
}

uint64_t mjs_critic_train_workspace_bytes(const mjs_critic* q, int32_t B) {
  if (!q || B <= 0) return 0;
  const crit::Layout L = layout_of(q);
  return (uint64_t)crit::split_rule(B, q->desc.n_critics, L.total).splits * q->desc.n_critics * L.total * sizeof(float);
}

// what mjs_critic_grad and mjs_critic_update refuse alike; "" = fine
static std::string grad_refusal(const mjs_critic* q, const mjs_critic_opt* o, const mjs_critic_grad_args* args) {
  if (!q || !o || !args) return "critic, optimiser or args is null";
  if (args->struct_size != sizeof(mjs_critic_grad_args)) return "mjs_critic_grad_args.struct_size does not match this library's header";
  if (o->critic != q) return "the optimiser was created for another critic";
  if (!q->loaded) return "the critic has no parameters yet (mjs_critic_load)";
  if (args->B < 0) return "B is negative";
  if (args->B > 0 && (!args->obs_dev || !args->actions_dev || !args->target_dev)) return "obs_dev, actions_dev or target_dev is null";
  return "";
}
// the gradient launch into the optimiser's slabs; returns the splits it wrote
static int launch_grad(const mjs_critic* q, mjs_critic_opt* o, const mjs_critic_grad_args* args, hipStream_t s) {
  const crit::Split sp = crit::split_rule(args->B, q->desc.n_critics, o->L.total);
  crit::GradParams p{};
  p.c = critic_params(q, args->B, q->widest);
  p.L = o->L;
  p.tiles_per_split = sp.tiles_per_split;
  p.inv_B = (float)(1.0 / (double)args->B);
  p.obs = args->obs_dev; p.actions = args->actions_dev; p.target = args->target_dev;
  p.q = args->q_out_dev;
  p.slabs = o->slabs;
  crit::grad_kernel<<<dim3((unsigned)sp.splits, (unsigned)q->desc.n_critics), act::WAVES * 64, crit::train_lds_bytes(q->desc.n_hidden, q->widest), s>>>(p);
  return sp.splits;
}
static crit::SumParams sum_params(const mjs_critic* q, const mjs_critic_opt* o, const mjs_critic_grad_args* args, int splits) {
  crit::SumParams p{};
  p.L = o->L; p.n_critics = q->desc.n_critics; p.splits = splits;
  p.inv_B = (float)(1.0 / (double)args->B);
  p.slabs = o->slabs; p.loss = args->loss_out_dev;
  return p;
}

int mjs_critic_grad(const mjs_critic* q, mjs_critic_opt* o, const mjs_critic_grad_args* args, void* stream) {
  const auto refuse = [](const std::string& why) { return fail(nullptr, MJS_ERR_INVALID_ARG, "mjs_critic_grad: " + why); };
  const std::string why = grad_refusal(q, o, args);
  if (!why.empty()) return refuse(why);
  if (args->grads_out) {
    if (args->grads_out->struct_size != sizeof(mjs_critic_weights)) return refuse("mjs_critic_weights.struct_size does not match this library's header");
    if (!all_layers_given(q, args->grads_out)) return refuse("grads_out: a layer's weight or bias pointer is null");
  }
  if (args->B == 0) return MJS_OK;
  DeviceGuard dev_(q->desc.device);
  HIP_TRY(nullptr, dev_.err);
  const hipStream_t s = (hipStream_t)stream;
  const int splits = launch_grad(q, o, args, s);
  if (args->loss_out_dev || args->grads_out) {
    const dim3 grid((unsigned)((o->L.off[8] + 1 + 255) / 256), (unsigned)q->desc.n_critics);
    crit::slab_sum_kernel<<<grid, 256, 0, s>>>(sum_params(q, o, args, splits), o->gsum);
  }
  if (args->grads_out)
    for (int c = 0; c < q->desc.n_critics; c++) {
      const float* seg[8];
      for (int k = 0; k < 8; k++) seg[k] = o->gsum + (size_t)c * o->L.total + o->L.off[k];
      launch_unpack(q, seg, c, args->grads_out, s);
    }
  HIP_TRY(nullptr, hipGetLastError());
  return MJS_OK;
}

int mjs_critic_update(mjs_critic_opt* o, const mjs_critic_grad_args* args, double lr, void* stream) {
  const auto refuse = [](const std::string& why) { return fail(nullptr, MJS_ERR_INVALID_ARG, "mjs_critic_update: " + why); };
  const std::string why = grad_refusal(o ? o->critic : nullptr, o, args);
  if (!why.empty()) return refuse(why);
  if (!(lr >= 0.0) || !std::isfinite(lr)) return refuse("lr must be finite and >= 0");
  if (args->grads_out) return refuse("grads_out must be null (mjs_critic_grad returns gradients)");
  if (args->B == 0) return MJS_OK;
  mjs_critic* q = o->critic;
  DeviceGuard dev_(q->desc.device);
  HIP_TRY(nullptr, dev_.err);
  const hipStream_t s = (hipStream_t)stream;
  const int splits = launch_grad(q, o, args, s);
  const double t = (double)(o->t + 1);
  crit::AdamParams p{};
  p.s = sum_params(q, o, args, splits);
  for (int c = 0; c < q->desc.n_critics; c++) p.net[c] = packed_of(q, c);
  p.m = o->m; p.v = o->v;
  p.one_minus_beta1 = (float)(1.0 - o->desc.beta1);
  p.beta2 = (float)o->desc.beta2;
  p.one_minus_beta2 = (float)(1.0 - o->desc.beta2);
  p.sqrt_bc2 = (float)std::sqrt(1.0 - std::pow(o->desc.beta2, t));
  p.eps = (float)o->desc.eps;
  p.step_size = (float)(lr / (1.0 - std::pow(o->desc.beta1, t)));
  crit::adam_kernel<<<dim3((unsigned)((o->L.off[8] + 1 + 255) / 256), (unsigned)q->desc.n_critics), 256, 0, s>>>(p);
  HIP_TRY(nullptr, hipGetLastError());
  o->t += 1;
  return MJS_OK;
}

// what mjs_critic_blend refuses; "" = fine
static std::string blend_refusal(const mjs_critic* dst, const mjs_critic* src, double tau) {
  if (!dst || !src) return "null critic";
  if (!same_shape(dst, src)) return "the two critics differ in shape";
  if (dst->desc.device != src->desc.device) return "the two critics live on different devices";
  if (!src->loaded) return "the source critic has no parameters yet (mjs_critic_load)";
  if (!(tau > 0.0 && tau <= 1.0)) return "tau must lie in (0, 1]";
  if (!dst->loaded && tau != 1.0) return "a critic that was never loaded takes tau == 1 only (there is nothing to blend with yet)";
  return "";
}

int mjs_critic_blend(mjs_critic* dst, const mjs_critic* src, double tau, void* stream) {
  if (std::string why = blend_refusal(dst, src, tau); !why.empty()) return fail(nullptr, MJS_ERR_INVALID_ARG, "mjs_critic_blend: " + why);
  if (dst == src) return MJS_OK;  // a blend of a copy with itself
  DeviceGuard dev_(dst->desc.device);
  HIP_TRY(nullptr, dev_.err);
  crit::BlendParams p{};
  p.L = layout_of(dst);
  for (int c = 0; c < dst->desc.n_critics; c++) { p.dst[c] = packed_of(dst, c); p.src[c] = packed_of(src, c); }
  const dim3 grid((unsigned)((p.L.off[8] + 255) / 256), (unsigned)dst->desc.n_critics);
  if (tau == 1.0) crit::blend_kernel<true><<<grid, 256, 0, (hipStream_t)stream>>>(p, 0.0f, 1.0f);
  else crit::blend_kernel<false><<<grid, 256, 0, (hipStream_t)stream>>>(p, (float)(1.0 - tau), (float)tau);
  HIP_TRY(nullptr, hipGetLastError());
  dst->loaded = true;
  return MJS_OK;
}

int mjs_critic_export(const mjs_critic* q, const mjs_critic_weights* out, void* stream) {
  const auto refuse = [](const std::string& why) { return fail(nullptr, MJS_ERR_INVALID_ARG, "mjs_critic_export: " + why); };
  if (!q || !out) return refuse("null argument");
  if (out->struct_size != sizeof(mjs_critic_weights)) return refuse("mjs_critic_weights.struct_size does not match this library's header");
  if (!q->loaded) return refuse("the critic has no parameters yet (mjs_critic_load)");
  if (!all_layers_given(q, out)) return refuse("a layer's weight or bias pointer is null");
  DeviceGuard dev_(q->desc.device);
  HIP_TRY(nullptr, dev_.err);
  for (int c = 0; c < q->desc.n_critics; c++) {
    const crit::Packed P = packed_of(q, c);
    launch_unpack(q, P.seg, c, out, (hipStream_t)stream);
  }
  HIP_TRY(nullptr, hipGetLastError());
  return MJS_OK;
}

// ---- the actor and entropy-coefficient update (mjs_actor_train.h) -------------------------------------------------------------
// where an actor's layers sit in a slab (the stacked head in slot 3), and its packed copy as the segments' pointers
static crit::Layout actor_layout_of(const mjs_actor* a) {
  crit::Layout L{};
  int at = 0, K = a->k0;
  for (int l = 0; l < 4; l++) {
    const bool used = l < a->desc.n_hidden || l == 3;
    const int O = l == 3 ? act::OPAD : a->width[l];
    L.off[2 * l] = at;
    if (used) at += K * O;
    L.off[2 * l + 1] = at;
    if (used) at += O;
    if (used && l < 3) K = O;
  }
  L.off[8] = at;
  L.total = at + 4;
  return L;
}
static crit::Packed actor_packed_of(const mjs_actor* a) {
  crit::Packed P;
  for (int l = 0; l < 4; l++) { P.seg[2 * l] = a->w[l]; P.seg[2 * l + 1] = a->b[l]; }
  return P;
}
static bool actor_layers_given(const mjs_actor* a, const mjs_actor_weights* w) {
  for (int l = 0; l < a->desc.n_hidden; l++)
    if (!w->hidden_w[l] || !w->hidden_b[l]) return false;
  return w->mu_w && w->mu_b && w->log_std_w && w->log_std_b;
}
// packed layers (the segments of the actor's copy or of a summed slab) -> nn.Linear layout: one launch per hidden layer, two for the head
// (mu = the head's columns 0..A-1, log_std = A..2A-1)
static void launch_actor_unpack(const mjs_actor* a, const float* const* seg, const mjs_actor_weights* out, hipStream_t s) {
  int in = a->desc.in_dim, K = a->k0;
  const int A = a->desc.action_dim;
  for (int l = 0; l < a->desc.n_hidden; l++) {
    crit::UnpackParams p;
    p.src_w = seg[2 * l]; p.src_b = seg[2 * l + 1];
    p.K = K; p.O = a->width[l];
    p.in = in; p.out = a->desc.hidden[l];
    p.dst_w = const_cast<float*>(out->hidden_w[l]);
    p.dst_b = const_cast<float*>(out->hidden_b[l]);
    crit::unpack_kernel<<<dim3((unsigned)((p.out * p.in + 255) / 256)), 256, 0, s>>>(p);
    in = a->desc.hidden[l]; K = a->width[l];
  }
  for (int half = 0; half < 2; half++) {
    crit::UnpackParams p;
    p.src_w = seg[6] + half * A; p.src_b = seg[7] + half * A;
    p.K = K; p.O = act::OPAD;
    p.in = in; p.out = A;
    p.dst_w = const_cast<float*>(half ? out->log_std_w : out->mu_w);
    p.dst_b = const_cast<float*>(half ? out->log_std_b : out->mu_b);
    crit::unpack_kernel<<<dim3((unsigned)((p.out * p.in + 255) / 256)), 256, 0, s>>>(p);
  }
}

int mjs_actor_opt_create(mjs_actor* a, const mjs_actor_opt_desc* desc, mjs_actor_opt** out) {
  const std::string name = "mjs_actor_opt_create";
  const auto refuse = [&](const std::string& why) { return fail(nullptr, MJS_ERR_INVALID_ARG, name + ": " + why); };
  if (out) *out = nullptr;
  if (!a || !desc || !out) return refuse("null argument");
  if (desc->struct_size != sizeof(mjs_actor_opt_desc)) return refuse("mjs_actor_opt_desc.struct_size does not match this library's header");
  if (a->visual) return refuse("the actor reads feature blocks (mjs_actor_create_visual): the visual actor's update is not built");
  if (!a->loaded) return refuse("the actor has no parameters yet (mjs_actor_load)");
  if (!(desc->lr >= 0.0) || !std::isfinite(desc->lr)) return refuse("lr must be finite and >= 0");
  if (!(desc->beta1 >= 0.0 && desc->beta1 < 1.0) || !(desc->beta2 >= 0.0 && desc->beta2 < 1.0)) return refuse("beta1 and beta2 must lie in [0, 1)");
  if (!(desc->eps > 0.0) || !std::isfinite(desc->eps)) return refuse("eps must be finite and > 0");
  DeviceGuard dev_(a->desc.device);
  std::unique_ptr<mjs_actor_opt, void (*)(mjs_actor_opt*)> guard(new (std::nothrow) mjs_actor_opt(), mjs_actor_opt_destroy);
  mjs_actor_opt* o = guard.get();
  if (!o) return fail(nullptr, MJS_ERR_ALLOC, name + ": out of host memory");
  CREATE_TRY(name, dev_.err);
  o->actor = a;
  o->desc = *desc;
  o->L = actor_layout_of(a);
  o->max_splits = crit::splits_max(1, o->L.total);
  const size_t per = sizeof(float) * (size_t)o->L.total;
  CREATE_TRY(name, hipMalloc(&o->m, per));
  CREATE_TRY(name, hipMalloc(&o->v, per));
  CREATE_TRY(name, hipMalloc(&o->gsum, per));
  CREATE_TRY(name, hipMalloc(&o->slabs, per * o->max_splits));
  CREATE_TRY(name, hipMemset(o->m, 0, per));
  CREATE_TRY(name, hipMemset(o->v, 0, per));
  CREATE_TRY(name, hipDeviceSynchronize());  // the moments are zero before any stream's first step
  // X, three actor images, three critic images and the gradient pair at the widest stride, and the two critics' action gradients:
  // an opt-in, below the CU's 160 KB
  static_assert(atrain::lds_bytes(act::MAX_LAYERS, act::MAX_LAYERS, act::MAX_HIDDEN) <= 160 * 1024, "LDS images of atrain::grad_kernel");
  CREATE_TRY(name, hipFuncSetAttribute(reinterpret_cast<const void*>(&atrain::grad_kernel), hipFuncAttributeMaxDynamicSharedMemorySize,
                                       (int)atrain::lds_bytes(act::MAX_LAYERS, act::MAX_LAYERS, act::MAX_HIDDEN)));
  *out = guard.release();
  return MJS_OK;
}

void mjs_actor_opt_destroy(mjs_actor_opt* o) {
  if (!o) return;
  free_all({o->m, o->v, o->slabs, o->gsum});
  delete o;
}

uint64_t mjs_actor_train_workspace_bytes(const mjs_actor* a, int32_t B) {
  if (!a || a->visual || B <= 0) return 0;
  const crit::Layout L = actor_layout_of(a);
  return (uint64_t)crit::split_rule(B, 1, L.total).splits * L.total * sizeof(float);
}

// what mjs_actor_grad and mjs_actor_update refuse alike; "" = fine
static std::string actor_grad_refusal(const mjs_actor* a, const mjs_actor_opt* o, const mjs_actor_grad_args* args) {
  if (!a || !o || !args) return "actor, optimiser or args is null";
  if (args->struct_size != sizeof(mjs_actor_grad_args)) return "mjs_actor_grad_args.struct_size does not match this library's header";
  if (o->actor != a) return "the optimiser was created for another actor";
  if (a->visual) return "the actor reads feature blocks (mjs_actor_create_visual): the visual actor's update is not built";
  const mjs_critic* q = args->critic;
  if (!q) return "critic is null";
  if (a->desc.device != q->desc.device) return "the actor lives on another device than the critic";
  if (!a->loaded) return "the actor has no parameters yet (mjs_actor_load)";
  if (!q->loaded) return "the critic has no parameters yet (mjs_critic_load)";
  if (a->desc.in_dim != q->desc.obs_dim) return "the actor's in_dim is not the critic's obs_dim";
  if (a->desc.action_dim != q->desc.action_dim) return "the actor's action_dim is not the critic's";
  if (args->B < 0) return "B is negative";
  if (args->B > 0 && (!args->obs_dev || !args->z_dev)) return "obs_dev or z_dev is null";
  if (const mjs_entropy_step* e = args->entropy) {
    if (e->struct_size != sizeof(mjs_entropy_step)) return "mjs_entropy_step.struct_size does not match this library's header";
    if (!e->log_ent_coef_dev || !e->ent_coef_dev || !e->m_dev || !e->v_dev) return "entropy: log_ent_coef_dev, ent_coef_dev, m_dev or v_dev is null";
    if (!(e->lr >= 0.0) || !std::isfinite(e->lr)) return "entropy: lr must be finite and >= 0";
    if (e->t < 1) return "entropy: t must be >= 1 (the step count after this step)";
    if (!(e->beta1 >= 0.0 && e->beta1 < 1.0) || !(e->beta2 >= 0.0 && e->beta2 < 1.0)) return "entropy: beta1 and beta2 must lie in [0, 1)";
    if (!(e->eps > 0.0) || !std::isfinite(e->eps)) return "entropy: eps must be finite and > 0";
    if (!std::isfinite(e->target_entropy)) return "entropy: target_entropy must be finite";
  }
  return "";
}
// the gradient launch into the optimiser's slabs; returns the splits it wrote
static int launch_actor_grad(const mjs_actor* a, mjs_actor_opt* o, const mjs_actor_grad_args* args, hipStream_t s) {
  const mjs_critic* q = args->critic;
  const crit::Split sp = crit::split_rule(args->B, 1, o->L.total);
  const int widest = a->widest > q->widest ? a->widest : q->widest;  // one stride for the actor's and the critics' layers
  atrain::GradParams p{};
  p.c = critic_params(q, args->B, widest);
  p.actor = mlp_of(nullptr, 0, a);
  p.L = o->L;
  p.tiles_per_split = sp.tiles_per_split;
  p.inv_B = (float)(1.0 / (double)args->B);
  p.obs = args->obs_dev; p.z = args->z_dev;
  p.ent_coef = (float)args->ent_coef; p.ent_coef_dev = args->ent_coef_dev;
  p.target_entropy = args->entropy ? (float)args->entropy->target_entropy : 0.0f;
  p.actions = args->actions_out_dev; p.log_prob = args->log_prob_out_dev; p.q_pi = args->q_pi_out_dev; p.dq_da = args->min_q_action_grad_out_dev;
  p.slabs = o->slabs;
  atrain::grad_kernel<<<dim3((unsigned)sp.splits), act::WAVES * 64, atrain::lds_bytes(a->desc.n_hidden, q->desc.n_hidden, widest), s>>>(p);
  return sp.splits;
}
static crit::SumParams actor_sum_params(const mjs_actor_opt* o, const mjs_actor_grad_args* args, int splits) {
  crit::SumParams p{};
  p.L = o->L; p.n_critics = 1; p.splits = splits;
  p.inv_B = (float)(1.0 / (double)args->B);
  p.slabs = o->slabs; p.loss = args->loss_out_dev;
  return p;
}

int mjs_actor_grad(const mjs_actor* a, mjs_actor_opt* o, const mjs_actor_grad_args* args, void* stream) {
  const auto refuse = [](const std::string& why) { return fail(nullptr, MJS_ERR_INVALID_ARG, "mjs_actor_grad: " + why); };
  const std::string why = actor_grad_refusal(a, o, args);
  if (!why.empty()) return refuse(why);
  if (args->grads_out) {
    if (args->grads_out->struct_size != sizeof(mjs_actor_weights)) return refuse("mjs_actor_weights.struct_size does not match this library's header");
    if (!actor_layers_given(a, args->grads_out)) return refuse("grads_out: a layer's weight or bias pointer is null");
  }
  if (args->B == 0) return MJS_OK;
  DeviceGuard dev_(a->desc.device);
  HIP_TRY(nullptr, dev_.err);
  const hipStream_t s = (hipStream_t)stream;
  const int splits = launch_actor_grad(a, o, args, s);
  if (args->loss_out_dev || args->grads_out)
    crit::slab_sum_kernel<<<dim3((unsigned)((o->L.off[8] + 1 + 255) / 256), 1), 256, 0, s>>>(actor_sum_params(o, args, splits), o->gsum);
  if (args->grads_out) {
    const float* seg[8];
    for (int k = 0; k < 8; k++) seg[k] = o->gsum + o->L.off[k];
    launch_actor_unpack(a, seg, args->grads_out, s);
  }
  HIP_TRY(nullptr, hipGetLastError());
  return MJS_OK;
}

int mjs_actor_update(mjs_actor_opt* o, const mjs_actor_grad_args* args, double lr, void* stream) {
  const auto refuse = [](const std::string& why) { return fail(nullptr, MJS_ERR_INVALID_ARG, "mjs_actor_update: " + why); };
  const std::string why = actor_grad_refusal(o ? o->actor : nullptr, o, args);
  if (!why.empty()) return refuse(why);
  if (!(lr >= 0.0) || !std::isfinite(lr)) return refuse("lr must be finite and >= 0");
  if (args->grads_out) return refuse("grads_out must be null (mjs_actor_grad returns gradients)");
  if (args->B == 0) return MJS_OK;
  mjs_actor* a = o->actor;
  DeviceGuard dev_(a->desc.device);
  HIP_TRY(nullptr, dev_.err);
  const hipStream_t s = (hipStream_t)stream;
  const int splits = launch_actor_grad(a, o, args, s);
  const double t = (double)(o->t + 1);
  crit::AdamParams p{};
  p.s = actor_sum_params(o, args, splits);
  p.net[0] = actor_packed_of(a);
  p.m = o->m; p.v = o->v;
  p.one_minus_beta1 = (float)(1.0 - o->desc.beta1);
  p.beta2 = (float)o->desc.beta2;
  p.one_minus_beta2 = (float)(1.0 - o->desc.beta2);
  p.sqrt_bc2 = (float)std::sqrt(1.0 - std::pow(o->desc.beta2, t));
  p.eps = (float)o->desc.eps;
  p.step_size = (float)(lr / (1.0 - std::pow(o->desc.beta1, t)));
  crit::adam_kernel<<<dim3((unsigned)((o->L.off[8] + 1 + 255) / 256), 1), 256, 0, s>>>(p);
  if (const mjs_entropy_step* e = args->entropy) {
    const double te = (double)e->t;
    atrain::EntParams ep{};
    ep.slabs = o->slabs; ep.splits = splits; ep.total = o->L.total; ep.at = o->L.off[8] + 1;
    ep.inv_B = (float)(1.0 / (double)args->B);
    ep.log_ent_coef = e->log_ent_coef_dev; ep.ent_coef = e->ent_coef_dev; ep.m = e->m_dev; ep.v = e->v_dev;
    ep.one_minus_beta1 = (float)(1.0 - e->beta1);
    ep.beta2 = (float)e->beta2;
    ep.one_minus_beta2 = (float)(1.0 - e->beta2);
    ep.sqrt_bc2 = (float)std::sqrt(1.0 - std::pow(e->beta2, te));
    ep.eps = (float)e->eps;
    ep.step_size = (float)(e->lr / (1.0 - std::pow(e->beta1, te)));
    atrain::ent_kernel<<<dim3(1), 64, 0, s>>>(ep);
  }
  HIP_TRY(nullptr, hipGetLastError());
  o->t += 1;
  return MJS_OK;
}

int mjs_actor_export(const mjs_actor* a, const mjs_actor_weights* out, void* stream) {
  const auto refuse = [](const std::string& why) { return fail(nullptr, MJS_ERR_INVALID_ARG, "mjs_actor_export: " + why); };
  if (!a || !out) return refuse("null argument");
  if (out->struct_size != sizeof(mjs_actor_weights)) return refuse("mjs_actor_weights.struct_size does not match this library's header");
  if (a->visual) return refuse("the actor reads feature blocks (mjs_actor_create_visual): its first layer has no nn.Linear counterpart here");
  if (!a->loaded) return refuse("the actor has no parameters yet (mjs_actor_load)");
  if (!actor_layers_given(a, out)) return refuse("a layer's weight or bias pointer is null");
  DeviceGuard dev_(a->desc.device);
  HIP_TRY(nullptr, dev_.err);
  const crit::Packed P = actor_packed_of(a);
  launch_actor_unpack(a, P.seg, out, (hipStream_t)stream);
  HIP_TRY(nullptr, hipGetLastError());
  return MJS_OK;
}

// ---- the encoder's backward pass, Adam step, blend and export (mjs_encoder_train.h) ----------------------------------------------
// where an encoder's layers sit in a slab: conv1..3 and fc, weights then bias each
static crit::Layout encoder_layout_of(const mjs_encoder* e) {
  const int K[4] = {8 * 8 * enc::C_IN, 4 * 4 * enc::C1, 3 * 3 * enc::C2, e->g.n_flatten};
  const int O[4] = {enc::C1, enc::C2, enc::C3, e->Fp};
  crit::Layout L{};
  int at = 0;
  for (int l = 0; l < 4; l++) {
    L.off[2 * l] = at;
    at += K[l] * O[l];
    L.off[2 * l + 1] = at;
    at += O[l];
  }
  L.off[8] = at;
  L.total = at + 4;
  return L;
}
static crit::Packed encoder_packed_of(const mjs_encoder* e) {
  crit::Packed P;
  for (int l = 0; l < 4; l++) { P.seg[2 * l] = e->w[l]; P.seg[2 * l + 1] = e->b[l]; }
  return P;
}
static bool encoder_tensors_given(const mjs_encoder_weights* w) {
  return w->conv1_w && w->conv1_b && w->conv2_w && w->conv2_b && w->conv3_w && w->conv3_b && w->fc_w && w->fc_b;
}
// packed layers (the segments of the encoder's copy or of a summed slab) -> torch layout: one small launch per layer
static void launch_encoder_unpack(const mjs_encoder* e, const float* const* seg, const mjs_encoder_weights* out, hipStream_t s) {
  const enct::UnpackConvParams conv[3] = {{seg[0], seg[1], enc::C1, enc::C_IN, 8, 8, const_cast<float*>(out->conv1_w), const_cast<float*>(out->conv1_b)},
                                          {seg[2], seg[3], enc::C2, enc::C1, 4, 4, const_cast<float*>(out->conv2_w), const_cast<float*>(out->conv2_b)},
                                          {seg[4], seg[5], enc::C3, enc::C2, 3, 3, const_cast<float*>(out->conv3_w), const_cast<float*>(out->conv3_b)}};
  for (const enct::UnpackConvParams& p : conv)
    enct::unpack_conv_kernel<<<dim3((unsigned)((p.kh * p.kw * p.cin * p.cout + 255) / 256)), 256, 0, s>>>(p);
  crit::UnpackParams p;
  p.src_w = seg[6]; p.src_b = seg[7];
  p.K = e->g.n_flatten; p.O = e->Fp;
  p.in = e->g.n_flatten; p.out = e->desc.features_dim;
  p.dst_w = const_cast<float*>(out->fc_w); p.dst_b = const_cast<float*>(out->fc_b);
  crit::unpack_kernel<<<dim3((unsigned)((p.out * p.in + 255) / 256)), 256, 0, s>>>(p);
}

int mjs_encoder_opt_create(mjs_encoder* e, const mjs_encoder_opt_desc* desc, mjs_encoder_opt** out) {
  const std::string name = "mjs_encoder_opt_create";
  const auto refuse = [&](const std::string& why) { return fail(nullptr, MJS_ERR_INVALID_ARG, name + ": " + why); };
  if (out) *out = nullptr;
  if (!e || !desc || !out) return refuse("null argument");
  if (desc->struct_size != sizeof(mjs_encoder_opt_desc)) return refuse("mjs_encoder_opt_desc.struct_size does not match this library's header");
  if (!e->loaded) return refuse("the encoder has no parameters yet (mjs_encoder_load)");
  if (!(desc->lr >= 0.0) || !std::isfinite(desc->lr)) return refuse("lr must be finite and >= 0");
  if (!(desc->beta1 >= 0.0 && desc->beta1 < 1.0) || !(desc->beta2 >= 0.0 && desc->beta2 < 1.0)) return refuse("beta1 and beta2 must lie in [0, 1)");
  if (!(desc->eps > 0.0) || !std::isfinite(desc->eps)) return refuse("eps must be finite and > 0");
  DeviceGuard dev_(e->desc.device);
  std::unique_ptr<mjs_encoder_opt, void (*)(mjs_encoder_opt*)> guard(new (std::nothrow) mjs_encoder_opt(), mjs_encoder_opt_destroy);
  mjs_encoder_opt* o = guard.get();
  if (!o) return fail(nullptr, MJS_ERR_ALLOC, name + ": out of host memory");
  CREATE_TRY(name, dev_.err);
  o->encoder = e;
  o->desc = *desc;
  o->L = encoder_layout_of(e);
  const size_t per = sizeof(float) * (size_t)o->L.total;
  CREATE_TRY(name, hipMalloc(&o->m, per));
  CREATE_TRY(name, hipMalloc(&o->v, per));
  CREATE_TRY(name, hipMalloc(&o->gsum, per));
  CREATE_TRY(name, hipMemset(o->m, 0, per));
  CREATE_TRY(name, hipMemset(o->v, 0, per));
  CREATE_TRY(name, hipDeviceSynchronize());  // the moments are zero before any stream's first step
  CREATE_TRY(name, hipFuncSetAttribute(reinterpret_cast<const void*>(&enct::forward_kernel), hipFuncAttributeMaxDynamicSharedMemorySize,
                                       (int)enc::lds_bytes(enc::geometry(enc::MAX_HW, enc::MAX_HW))));
  *out = guard.release();
  return MJS_OK;
}

void mjs_encoder_opt_destroy(mjs_encoder_opt* o) {
  if (!o) return;
  free_all({o->m, o->v, o->gsum});
  delete o;
}

uint64_t mjs_encoder_train_workspace_bytes(const mjs_encoder* e, int32_t n) {
  if (!e || n <= 0) return 0;
  const crit::Layout L = encoder_layout_of(e);
  return (uint64_t)enct::workspace(e->g, e->desc.features_dim, e->Fp, n, enct::split_rule(n, L.total).splits, L.total).total * sizeof(float);
}

// what mjs_encoder_grad and mjs_encoder_update refuse alike; "" = fine
static std::string encoder_grad_refusal(const mjs_encoder* e, const mjs_encoder_opt* o, const mjs_encoder_grad_args* args) {
  if (!e || !o || !args) return "encoder, optimiser or args is null";
  if (args->struct_size != sizeof(mjs_encoder_grad_args)) return "mjs_encoder_grad_args.struct_size does not match this library's header";
  if (o->encoder != e) return "the optimiser was created for another encoder";
  if (!e->loaded) return "the encoder has no parameters yet (mjs_encoder_load)";
  if (args->n < 0) return "n is negative";
  if (args->n > 0 && (!args->rgb_dev || !args->dfeatures_dev || !args->workspace_dev)) return "rgb_dev, dfeatures_dev or workspace_dev is null";
  return "";
}
// the forward and the backward into the workspace's slabs; returns the splits written
static int launch_encoder_grad(const mjs_encoder* e, const mjs_encoder_opt* o, const mjs_encoder_grad_args* args, hipStream_t s) {
  const enc::Geometry& g = e->g;
  const int n = args->n, F = e->desc.features_dim, Fp = e->Fp, NF = g.n_flatten;
  const int P1 = g.H1 * g.W1, P2 = g.H2 * g.W2, P3 = g.H3 * g.W3;
  const enct::Split sp = enct::split_rule(n, o->L.total);
  const enct::Workspace w = enct::workspace(g, F, Fp, n, sp.splits, o->L.total);
  float* ws = static_cast<float*>(args->workspace_dev);
  enct::ForwardParams fw;
  fw.c.N = n; fw.c.g = g; fw.c.rgb = args->rgb_dev;
  fw.c.W1 = e->w[0]; fw.c.B1 = e->b[0]; fw.c.W2 = e->w[1]; fw.c.B2 = e->b[1]; fw.c.W3 = e->w[2]; fw.c.B3 = e->b[2];
  fw.c.flat = ws + w.flat; fw.a1 = ws + w.a1; fw.a2 = ws + w.a2;
  enct::forward_kernel<<<dim3((unsigned)n), enc::WAVES * 64, enc::lds_bytes(g), s>>>(fw);
  enc::FcParams f;
  f.N = n; f.K = NF; f.F = F; f.Fp = Fp;
  f.flat = ws + w.flat; f.W = e->w[3]; f.B = e->b[3]; f.out = ws + w.feat;
  enc::fc_kernel<<<dim3((unsigned)((n + enc::FC_TE - 1) / enc::FC_TE)), enc::WAVES * 64, 0, s>>>(f);
  enct::FcBwdParams fb;
  fb.N = n; fb.K = NF; fb.F = F; fb.Fp = Fp; fb.P3 = P3;
  fb.dfeatures = args->dfeatures_dev; fb.features = ws + w.feat; fb.flat = ws + w.flat; fb.W = e->w[3];
  fb.gf = ws + w.gf; fb.dz3 = ws + w.dz3;
  enct::fc_bwd_kernel<<<dim3((unsigned)((n + enc::FC_TE - 1) / enc::FC_TE), (unsigned)((NF + enct::FCB_KBLOCK - 1) / enct::FCB_KBLOCK)), enc::WAVES * 64, 0, s>>>(fb);
  enct::DgradParams dg;
  dg.N = n; dg.g = g; dg.W2 = e->w[1]; dg.W3 = e->w[2]; dg.a1 = ws + w.a1; dg.a2 = ws + w.a2;
  dg.dz3 = ws + w.dz3; dg.dz2 = ws + w.dz2; dg.dz1 = ws + w.dz1;
  enct::dgrad_kernel<<<dim3((unsigned)n), enc::WAVES * 64, enct::dgrad_lds_bytes(g), s>>>(dg);
  float* slab = ws + w.slabs;
  enct::WgradParams wp{};
  wp.n = n; wp.images_per_split = sp.images_per_split; wp.slab_stride = (size_t)o->L.total;
  const auto grid = [&](int K, int O) { return dim3((unsigned)sp.splits, (unsigned)((K + enct::KBLOCK - 1) / enct::KBLOCK), (unsigned)(O / enct::OBLOCK)); };
  wp.P = 1; wp.Wout = 1; wp.Pin = 1; wp.Win = 1; wp.K = NF; wp.O = Fp;
  wp.rgb = nullptr; wp.X = ws + w.flat; wp.G = ws + w.gf; wp.dW = slab + o->L.off[6]; wp.dB = slab + o->L.off[7];
  enct::wgrad_kernel<enct::SRC_FLAT, 1, 1, 1, 1><<<grid(wp.K, wp.O), enc::WAVES * 64, 0, s>>>(wp);
  wp.P = P3; wp.Wout = g.W3; wp.Pin = P2; wp.Win = g.W2; wp.K = 3 * 3 * enc::C2; wp.O = enc::C3;
  wp.X = ws + w.a2; wp.G = ws + w.dz3; wp.dW = slab + o->L.off[4]; wp.dB = slab + o->L.off[5];
  enct::wgrad_kernel<enct::SRC_ACT, 3, 3, 1, enc::C2><<<grid(wp.K, wp.O), enc::WAVES * 64, 0, s>>>(wp);
  wp.P = P2; wp.Wout = g.W2; wp.Pin = P1; wp.Win = g.W1; wp.K = 4 * 4 * enc::C1; wp.O = enc::C2;
  wp.X = ws + w.a1; wp.G = ws + w.dz2; wp.dW = slab + o->L.off[2]; wp.dB = slab + o->L.off[3];
  enct::wgrad_kernel<enct::SRC_ACT, 4, 4, 2, enc::C1><<<grid(wp.K, wp.O), enc::WAVES * 64, 0, s>>>(wp);
  wp.P = P1; wp.Wout = g.W1; wp.Pin = g.H * g.W; wp.Win = g.W; wp.K = 8 * 8 * enc::C_IN; wp.O = enc::C1;
  wp.rgb = args->rgb_dev; wp.X = nullptr; wp.G = ws + w.dz1; wp.dW = slab + o->L.off[0]; wp.dB = slab + o->L.off[1];
  enct::wgrad_kernel<enct::SRC_IMAGE, 8, 8, 4, enc::C_IN><<<grid(wp.K, wp.O), enc::WAVES * 64, 0, s>>>(wp);
  // the optional copies out of the workspace (device to device, on the stream)
  const struct { float* dst; size_t at, count; } copies[4] = {{args->features_out_dev, w.feat, (size_t)n * F},
                                                              {args->activations_out_dev[0], w.a1, (size_t)n * P1 * enc::C1},
                                                              {args->activations_out_dev[1], w.a2, (size_t)n * P2 * enc::C2},
                                                              {args->activations_out_dev[2], w.flat, (size_t)n * NF}};
  for (const auto& c : copies)
    if (c.dst) (void)hipMemcpyAsync(c.dst, ws + c.at, c.count * sizeof(float), hipMemcpyDeviceToDevice, s);
  return sp.splits;
}
static crit::SumParams encoder_sum_params(const mjs_encoder_opt* o, const mjs_encoder_grad_args* args, int splits, const enct::Workspace& w) {
  crit::SumParams p{};
  p.L = o->L; p.n_critics = 1; p.splits = splits;
  p.inv_B = 1.0f;
  p.slabs = static_cast<const float*>(args->workspace_dev) + w.slabs; p.loss = nullptr;
  return p;
}
static enct::Workspace encoder_workspace_of(const mjs_encoder* e, const mjs_encoder_opt* o, int n) {
  return enct::workspace(e->g, e->desc.features_dim, e->Fp, n, enct::split_rule(n, o->L.total).splits, o->L.total);
}

int mjs_encoder_grad(const mjs_encoder* e, mjs_encoder_opt* o, const mjs_encoder_grad_args* args, void* stream) {
  const auto refuse = [](const std::string& why) { return fail(nullptr, MJS_ERR_INVALID_ARG, "mjs_encoder_grad: " + why); };
  const std::string why = encoder_grad_refusal(e, o, args);
  if (!why.empty()) return refuse(why);
  if (args->grads_out) {
    if (args->grads_out->struct_size != sizeof(mjs_encoder_weights)) return refuse("mjs_encoder_weights.struct_size does not match this library's header");
    if (!encoder_tensors_given(args->grads_out)) return refuse("grads_out: a weight or bias pointer is null");
  }
  if (args->n == 0) return MJS_OK;
  DeviceGuard dev_(e->desc.device);
  HIP_TRY(nullptr, dev_.err);
  const hipStream_t s = (hipStream_t)stream;
  const int splits = launch_encoder_grad(e, o, args, s);
  if (args->grads_out) {
    crit::slab_sum_kernel<<<dim3((unsigned)((o->L.off[8] + 1 + 255) / 256), 1), 256, 0, s>>>(encoder_sum_params(o, args, splits, encoder_workspace_of(e, o, args->n)), o->gsum);
    const float* seg[8];
    for (int k = 0; k < 8; k++) seg[k] = o->gsum + o->L.off[k];
    launch_encoder_unpack(e, seg, args->grads_out, s);
  }
  HIP_TRY(nullptr, hipGetLastError());
  return MJS_OK;
}

int mjs_encoder_update(mjs_encoder_opt* o, const mjs_encoder_grad_args* args, double lr, void* stream) {
  const auto refuse = [](const std::string& why) { return fail(nullptr, MJS_ERR_INVALID_ARG, "mjs_encoder_update: " + why); };
  const std::string why = encoder_grad_refusal(o ? o->encoder : nullptr, o, args);
  if (!why.empty()) return refuse(why);
  if (!(lr >= 0.0) || !std::isfinite(lr)) return refuse("lr must be finite and >= 0");
  if (args->grads_out) return refuse("grads_out must be null (mjs_encoder_grad returns gradients)");
  if (args->n == 0) return MJS_OK;
  mjs_encoder* e = o->encoder;
  DeviceGuard dev_(e->desc.device);
  HIP_TRY(nullptr, dev_.err);
  const hipStream_t s = (hipStream_t)stream;
  const int splits = launch_encoder_grad(e, o, args, s);
  const double t = (double)(o->t + 1);
  crit::AdamParams p{};
  p.s = encoder_sum_params(o, args, splits, encoder_workspace_of(e, o, args->n));
  p.net[0] = encoder_packed_of(e);
  p.m = o->m; p.v = o->v;
  p.one_minus_beta1 = (float)(1.0 - o->desc.beta1);
  p.beta2 = (float)o->desc.beta2;
  p.one_minus_beta2 = (float)(1.0 - o->desc.beta2);
  p.sqrt_bc2 = (float)std::sqrt(1.0 - std::pow(o->desc.beta2, t));
  p.eps = (float)o->desc.eps;
  p.step_size = (float)(lr / (1.0 - std::pow(o->desc.beta1, t)));
  crit::adam_kernel<<<dim3((unsigned)((o->L.off[8] + 1 + 255) / 256), 1), 256, 0, s>>>(p);
  HIP_TRY(nullptr, hipGetLastError());
  o->t += 1;
  return MJS_OK;
}

int mjs_encoder_blend(mjs_encoder* dst, const mjs_encoder* src, double tau, void* stream) {
  const auto refuse = [](const std::string& why) { return fail(nullptr, MJS_ERR_INVALID_ARG, "mjs_encoder_blend: " + why); };
  if (!dst || !src) return refuse("an encoder is null");
  if (dst->desc.device != src->desc.device) return refuse("the encoders live on different devices");
  if (dst->desc.height != src->desc.height || dst->desc.width != src->desc.width || dst->desc.features_dim != src->desc.features_dim)
    return refuse("the encoders differ in shape");
  if (!src->loaded) return refuse("the source encoder has no parameters yet (mjs_encoder_load)");
  if (!(tau > 0.0 && tau <= 1.0)) return refuse("tau must lie in (0, 1]");
  if (tau != 1.0 && !dst->loaded) return refuse("tau != 1 into an encoder that has no parameters yet (tau == 1 copies)");
  if (dst == src) return MJS_OK;  // a blend of a copy with itself
  DeviceGuard dev_(dst->desc.device);
  HIP_TRY(nullptr, dev_.err);
  crit::BlendParams p{};
  p.L = encoder_layout_of(dst);
  p.dst[0] = encoder_packed_of(dst);
  p.src[0] = encoder_packed_of(src);
  const dim3 grid((unsigned)((p.L.off[8] + 255) / 256), 1);
  if (tau == 1.0) crit::blend_kernel<true><<<grid, 256, 0, (hipStream_t)stream>>>(p, 0.0f, 1.0f);
  else crit::blend_kernel<false><<<grid, 256, 0, (hipStream_t)stream>>>(p, (float)(1.0 - tau), (float)tau);
  HIP_TRY(nullptr, hipGetLastError());
  dst->loaded = true;
  return MJS_OK;
}

int mjs_encoder_export(const mjs_encoder* e, const mjs_encoder_weights* out, void* stream) {
  const auto refuse = [](const std::string& why) { return fail(nullptr, MJS_ERR_INVALID_ARG, "mjs_encoder_export: " + why); };
  if (!e || !out) return refuse("null argument");
  if (out->struct_size != sizeof(mjs_encoder_weights)) return refuse("mjs_encoder_weights.struct_size does not match this library's header");
  if (!e->loaded) return refuse("the encoder has no parameters yet (mjs_encoder_load)");
  if (!encoder_tensors_given(out)) return refuse("a weight or bias pointer is null");
  DeviceGuard dev_(e->desc.device);
  HIP_TRY(nullptr, dev_.err);
  const crit::Packed P = encoder_packed_of(e);
  launch_encoder_unpack(e, P.seg, out, (hipStream_t)stream);
  HIP_TRY(nullptr, hipGetLastError());
  return MJS_OK;
}

// ---- the gradient loop (mjs_sac_train.h) ----------------------------------------------------------------------------------------
// what mjs_sac_draw_batch and mjs_sac_train refuse about the storage and the batch buffers alike; "" = fine
static std::string draw_refusal(const mjs_replay_storage* st, const mjs_sac_batch* out, int32_t B) {
  if (std::string why = replay_storage_refusal(st); !why.empty()) return why;
  if (st->n_cameras > 0) return "the storage holds cameras: the SAC update is state-only (visual critics are not built)";
  if (!out) return "the batch (mjs_sac_batch) is null";
  if (out->struct_size != sizeof(mjs_sac_batch)) return "mjs_sac_batch.struct_size does not match this library's header";
  if (B < 0) return "B is negative";
  if (B > 0) {
    if (!out->idx_out || !out->actions || !out->rewards || !out->dones) return "the batch's idx_out, actions, rewards or dones is null";
    if (st->obs_dim > 0 && (!out->obs || !out->next_obs)) return "the batch's obs or next_obs is null";
    if (!out->z_next || !out->z_pi) return "the batch's z_next or z_pi is null";
  }
  return "";
}
static void launch_draw(const mjs_replay_storage* st, const mjs_sac_batch* out, int32_t B, uint64_t seed, uint64_t step, hipStream_t s) {
  sac::DrawParams p{};
  p.B = B; p.D = st->obs_dim; p.A = st->action_dim; p.capacity = st->capacity;
  p.cursor = reinterpret_cast<const unsigned long long*>(st->cursor_dev);
  p.key0 = (uint32_t)(seed & 0xffffffffu); p.key1 = (uint32_t)(seed >> 32);
  p.step_lo = (uint32_t)(step & 0xffffffffu); p.step_hi = (uint32_t)(step >> 32);
  p.s_obs = st->obs; p.s_next_obs = st->next_obs; p.s_actions = st->actions; p.s_rewards = st->rewards; p.s_dones = st->dones;
  p.idx_out = out->idx_out; p.draws_out = out->draws_out;
  p.obs = out->obs; p.next_obs = out->next_obs; p.actions = out->actions; p.rewards = out->rewards; p.dones = out->dones;
  p.z_next = out->z_next; p.z_pi = out->z_pi;
  sac::draw_batch_kernel<<<dim3((unsigned)(((int64_t)B + sac::DRAW_ROWS - 1) / sac::DRAW_ROWS)), sac::THREADS, 0, s>>>(p);
}

int mjs_sac_draw_batch(const mjs_replay_storage* st, const mjs_sac_batch* out, int32_t B, uint64_t seed, uint64_t step, void* stream) {
  if (std::string why = draw_refusal(st, out, B); !why.empty()) return fail(nullptr, MJS_ERR_INVALID_ARG, "mjs_sac_draw_batch: " + why);
  if (B == 0) return MJS_OK;
  if (int rc = device_refusal("mjs_sac_draw_batch", st->device)) return rc;
  DeviceGuard dev_(st->device);
  HIP_TRY(nullptr, dev_.err);
  launch_draw(st, out, B, seed, step, (hipStream_t)stream);
  HIP_TRY(nullptr, hipGetLastError());
  return MJS_OK;
}

int mjs_sac_train(const mjs_sac_train_args* a, void* stream) {
  const auto refuse = [](const std::string& why) { return fail(nullptr, MJS_ERR_INVALID_ARG, "mjs_sac_train: " + why); };
  if (!a) return refuse("args is null");
  if (a->struct_size != sizeof(mjs_sac_train_args)) return refuse("mjs_sac_train_args.struct_size does not match this library's header");
  if (!a->storage || !a->actor || !a->critic || !a->target_critic || !a->critic_opt || !a->actor_opt || !a->batch || !a->target_dev)
    return refuse("storage, actor, critic, target_critic, critic_opt, actor_opt, batch or target_dev is null");
  if (a->B < 1) return refuse("B must be at least 1");
  if (a->G < 0) return refuse("G is negative");
  if (a->target_update_interval < 1) return refuse("target_update_interval must be at least 1");
  if (std::string why = draw_refusal(a->storage, a->batch, a->B); !why.empty()) return refuse(why);
  const mjs_replay_storage* st = a->storage;
  if (st->obs_dim != a->actor->desc.in_dim || st->obs_dim != a->critic->desc.obs_dim) return refuse("the storage's obs_dim is not the networks'");
  if (st->action_dim != a->actor->desc.action_dim || st->action_dim != a->critic->desc.action_dim) return refuse("the storage's action_dim is not the networks'");
  if (st->device != a->actor->desc.device || st->device != a->critic->desc.device || st->device != a->target_critic->desc.device)
    return refuse("the storage, the actor and the critics live on different devices");
  if (a->critic_opt->critic != a->critic) return refuse("critic_opt was created for another critic");
  if (a->actor_opt->actor != a->actor) return refuse("actor_opt was created for another actor");
  if (a->target_critic == a->critic) return refuse("target_critic and critic are one object");
  if (!(a->tau > 0.0 && a->tau <= 1.0)) return refuse("tau must lie in (0, 1]");
  if (!(a->gamma >= 0.0 && a->gamma <= 1.0)) return refuse("gamma must lie in [0, 1]");
  if (!(a->critic_lr >= 0.0) || !std::isfinite(a->critic_lr) || !(a->actor_lr >= 0.0) || !std::isfinite(a->actor_lr))
    return refuse("critic_lr and actor_lr must be finite and >= 0");
  // the three steps' arguments over the scratch batch, and what their entry points and the blend refuse, before the first launch
  const mjs_sac_batch* bt = a->batch;
  const float* ent_dev = a->ent_coef_dev ? a->ent_coef_dev : a->entropy ? a->entropy->ent_coef_dev : nullptr;
  mjs_td_target_args td{};
  td.struct_size = sizeof(td); td.B = a->B;
  td.next_obs_dev = bt->next_obs; td.rewards_dev = bt->rewards; td.dones_dev = bt->dones; td.z_dev = bt->z_next;
  td.gamma = a->gamma; td.ent_coef = a->ent_coef; td.ent_coef_dev = ent_dev; td.target_out_dev = a->target_dev;
  mjs_critic_grad_args cg{};
  cg.struct_size = sizeof(cg); cg.B = a->B;
  cg.obs_dev = bt->obs; cg.actions_dev = bt->actions; cg.target_dev = a->target_dev;
  mjs_entropy_step ent{};
  if (a->entropy) ent = *a->entropy;
  mjs_actor_grad_args ag{};
  ag.struct_size = sizeof(ag); ag.B = a->B;
  ag.obs_dev = bt->obs; ag.z_dev = bt->z_pi; ag.critic = a->critic; ag.ent_coef = a->ent_coef; ag.ent_coef_dev = ent_dev;
  ag.entropy = a->entropy ? &ent : nullptr;
  if (std::string why = td_refusal(a->actor, a->target_critic, &td); !why.empty()) return refuse("mjs_sac_td_target: " + why);
  if (std::string why = grad_refusal(a->critic, a->critic_opt, &cg); !why.empty()) return refuse("mjs_critic_update: " + why);
  if (std::string why = actor_grad_refusal(a->actor, a->actor_opt, &ag); !why.empty()) return refuse("mjs_actor_update: " + why);
  if (std::string why = blend_refusal(a->target_critic, a->critic, a->tau); !why.empty()) return refuse("mjs_critic_blend: " + why);
  if (a->G == 0) return MJS_OK;
  if (int rc = device_refusal("mjs_sac_train", st->device)) return rc;
  DeviceGuard dev_(st->device);
  HIP_TRY(nullptr, dev_.err);
  const int64_t t0 = ent.t;
  for (int32_t g = 0; g < a->G; g++) {
    const uint64_t step = a->step0 + (uint64_t)g;
    launch_draw(st, bt, a->B, a->seed, step, (hipStream_t)stream);
    if (int rc = mjs_sac_td_target(a->actor, a->target_critic, &td, stream)) return rc;
    if (int rc = mjs_critic_update(a->critic_opt, &cg, a->critic_lr, stream)) return rc;
    ent.t = t0 + g;
    if (int rc = mjs_actor_update(a->actor_opt, &ag, a->actor_lr, stream)) return rc;
    if ((step + 1) % (uint64_t)a->target_update_interval == 0)
      if (int rc = mjs_critic_blend(a->target_critic, a->critic, a->tau, stream)) return rc;
  }
  HIP_TRY(nullptr, hipGetLastError());
  return MJS_OK;
}

// ---- episode statistics (mjs_monitor.h) -----------------------------------------------------------------------------------------
// what mjs_monitor_update / mjs_monitor_summary refuse about a state descriptor; empty = fine
static std::string monitor_state_refusal(const mjs_monitor_state* st) {
  if (!st) return "state is null";
  if (st->struct_size != sizeof(mjs_monitor_state)) return "mjs_monitor_state.struct_size does not match this library's header";
  if (st->num_envs < 1) return "num_envs must be at least 1";
  if (st->window < 1) return "window must be at least 1";
  if (!st->ep_return || !st->ep_length || !st->ep_count) return "the state's ep_return, ep_length or ep_count is null";
  if (!st->cursor_dev) return "cursor_dev is null";
  if (!st->ring_return || !st->ring_length || !st->ring_success || !st->ring_terminated || !st->ring_env)
    return "the ring's return, length, success, terminated or env is null";
  return "";
}

uint64_t mjs_monitor_workspace_bytes(int32_t T, int32_t N) {
  return T > 0 && N > 0 && (int64_t)T * N < ((int64_t)1 << 31) ? (uint64_t)mon::ws_bytes((int64_t)T * N) : 0;
}

int mjs_monitor_update(const mjs_monitor_state* st, const mjs_monitor_block* blk, void* workspace_dev, void* stream) {
  const auto refuse = [](const std::string& why) { return fail(nullptr, MJS_ERR_INVALID_ARG, "mjs_monitor_update: " + why); };
  if (std::string why = monitor_state_refusal(st); !why.empty()) return refuse(why);
  if (!blk) return refuse("block is null");
  if (blk->struct_size != sizeof(mjs_monitor_block)) return refuse("mjs_monitor_block.struct_size does not match this library's header");
  if (blk->T < 0) return refuse("T is negative");
  if (blk->N < 1) return refuse("N must be positive");
  if (blk->N != st->num_envs) return refuse("the block's N is not the state's num_envs");
  if (blk->autoreset != MJS_AUTORESET_NEXT_STEP && blk->autoreset != MJS_AUTORESET_SAME_STEP)
    return refuse("the block's autoreset must be next-step or same-step (with auto-reset disabled a finished env starts no new episode)");
  const bool same_step = blk->autoreset == MJS_AUTORESET_SAME_STEP;
  const int64_t rows = (int64_t)blk->T * blk->N;
  if (rows >= ((int64_t)1 << 31)) return refuse("T * N must stay below 2^31");
  if (blk->T == 0) return MJS_OK;
  if (!blk->reward || !blk->terminated || !blk->truncated || !blk->is_success) return refuse("reward, terminated, truncated or is_success is null");
  if (!same_step && !blk->step_type) return refuse("next-step auto-reset needs step_type");
  if (!workspace_dev) return refuse("workspace_dev is null");
  if (int rc = device_refusal("mjs_monitor_update", st->device)) return rc;
  DeviceGuard dev_(st->device);
  HIP_TRY(nullptr, dev_.err);

  mon::UpdateParams p{};
  p.rows = rows; p.T = blk->T; p.N = blk->N; p.same_step = same_step; p.W = st->window;
  p.ep_return = st->ep_return; p.ep_length = st->ep_length; p.ep_count = st->ep_count; p.quota = st->quota;
  p.cursor = reinterpret_cast<unsigned long long*>(st->cursor_dev);
  p.r_return = st->ring_return; p.r_length = st->ring_length; p.r_success = st->ring_success; p.r_terminated = st->ring_terminated; p.r_env = st->ring_env;
  unsigned char* ws = static_cast<unsigned char*>(workspace_dev);
  p.base = reinterpret_cast<unsigned long long*>(ws);
  p.offsets = reinterpret_cast<uint32_t*>(ws + mon::WS_HEADER);
  p.end_return = reinterpret_cast<double*>(ws + mon::WS_HEADER + mon::ws_offsets_bytes(rows));
  p.end_length = reinterpret_cast<int32_t*>(ws + mon::WS_HEADER + mon::ws_offsets_bytes(rows) + (size_t)rows * sizeof(double));
  p.reward = blk->reward; p.terminated = blk->terminated; p.truncated = blk->truncated; p.step_type = blk->step_type; p.is_success = blk->is_success;
  const hipStream_t s = (hipStream_t)stream;
  const dim3 chunks((unsigned)mon::n_chunks(rows));
  mon::walk_kernel<<<dim3((unsigned)((blk->N + mon::THREADS - 1) / mon::THREADS)), mon::THREADS, 0, s>>>(p);
  mon::count_kernel<<<chunks, mon::THREADS, 0, s>>>(p);
  mon::scan_kernel<<<dim3(1), mon::THREADS, 0, s>>>(p);
  mon::scatter_kernel<<<chunks, mon::THREADS, 0, s>>>(p);
  HIP_TRY(nullptr, hipGetLastError());
  return MJS_OK;
}

int mjs_monitor_summary(const mjs_monitor_state* st, double* out_dev, void* stream) {
  const auto refuse = [](const std::string& why) { return fail(nullptr, MJS_ERR_INVALID_ARG, "mjs_monitor_summary: " + why); };
  if (std::string why = monitor_state_refusal(st); !why.empty()) return refuse(why);
  if (!out_dev) return refuse("out_dev is null");
  if (int rc = device_refusal("mjs_monitor_summary", st->device)) return rc;
  DeviceGuard dev_(st->device);
  HIP_TRY(nullptr, dev_.err);
  mon::SummaryParams p{};
  p.W = st->window;
  p.cursor = reinterpret_cast<const unsigned long long*>(st->cursor_dev);
  p.r_return = st->ring_return; p.r_length = st->ring_length; p.r_success = st->ring_success;
  p.out = out_dev;
  mon::summary_kernel<<<dim3(1), mon::THREADS, 0, (hipStream_t)stream>>>(p);
  HIP_TRY(nullptr, hipGetLastError());
  return MJS_OK;
}

// ---- cameras ------------------------------------------------------------------------------------------------------------
int mjs_set_scene_camera(mjs_handle* h, const mjs_camera_pose* pose) {
  if (!h) return fail(nullptr, MJS_ERR_INVALID_ARG, "mjs_set_scene_camera: null handle");
  mjs_camera_pose c;
  if (!pose) default_scene_camera(h->cfg.task, c);
  else {
    if (pose->struct_size != sizeof(mjs_camera_pose))
      return fail(h, MJS_ERR_INVALID_ARG, "mjs_set_scene_camera: mjs_camera_pose.struct_size does not match this library's header");
    c = *pose;
    bool finite = std::isfinite(c.fovy);
    double n2 = 0;
    for (int k = 0; k < 3; k++) finite = finite && std::isfinite(c.pos[k]);
    for (int k = 0; k < 4; k++) { finite = finite && std::isfinite(c.quat[k]); n2 += c.quat[k] * c.quat[k]; }
    if (!finite) return fail(h, MJS_ERR_INVALID_ARG, "mjs_set_scene_camera: position, quaternion and fovy must be finite");
    if (!(std::sqrt(n2) >= 1e-9)) return fail(h, MJS_ERR_INVALID_ARG, "mjs_set_scene_camera: the quaternion's norm is below 1e-9");
    if (!(c.fovy > 0 && c.fovy < 180)) return fail(h, MJS_ERR_INVALID_ARG, "mjs_set_scene_camera: fovy must lie in (0, 180) degrees");
  }
  // kept as given: the frame is derived from these numbers exactly as from the compiled-in defaults (a pose equal to the default
  // gives the default's images byte for byte); mjs_get_scene_camera normalises the quaternion
  h->cam = c;
  h->cam_serial++;         // the ray / floor table of the old pose is void ...
  h->prims_valid = false;  // ... and so is the primitive list: the camera's own body moves with the pose
  return MJS_OK;
}

int mjs_get_scene_camera(const mjs_handle* h, mjs_camera_pose* out) {
  if (!h || !out) return fail(nullptr, MJS_ERR_INVALID_ARG, "mjs_get_scene_camera: null argument");
  *out = h->cam;
  const double* q = h->cam.quat;
  const double n = std::sqrt(q[0] * q[0] + q[1] * q[1] + q[2] * q[2] + q[3] * q[3]);
  for (int k = 0; k < 4; k++) out->quat[k] = q[k] / n;
  return MJS_OK;
}

int mjs_render_rgbd(mjs_handle* h, int32_t camera, int32_t height, int32_t width, uint8_t* rgb_dev, float* depth_dev, void* stream) {
  if (!h || (!rgb_dev && !depth_dev)) return fail(h, MJS_ERR_INVALID_ARG, "mjs_render_rgbd: null handle, or neither an rgb nor a depth buffer");
  const int task = h->cfg.task;
  const bool wrist = camera == MJS_CAMERA_WRIST;
  if ((camera != MJS_CAMERA_SCENE && !(wrist && task == MJS_TASK_BUTTON_PUSH)) || height <= 0 || width <= 0)
    return fail(h, MJS_ERR_INVALID_ARG, "mjs_render: bad camera or size");
  DeviceGuard dev_(h->cfg.device);
  HIP_TRY(h, dev_.err);
  rend::RenderParams p;
  p.N = h->cfg.num_envs; p.H = height; p.W = width; p.state = h->state; p.out = rgb_dev;
  p.env_cams = nullptr; p.nprim = 0;
  // camera frame from the MuJoCo quaternion (w,x,y,z): columns of R are the local x (right), y (up), z (back) axes
  const double* q = h->cam.quat;
  const double* cpos = h->cam.pos;
  const double fovy = wrist ? MJS_WCAM_FOVY : h->cam.fovy;
  const double n = std::sqrt(q[0] * q[0] + q[1] * q[1] + q[2] * q[2] + q[3] * q[3]);
  const double w = q[0] / n, x = q[1] / n, y = q[2] / n, z = q[3] / n;
  const double R[9] = {1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w), 2 * (x * y + z * w), 1 - 2 * (x * x + z * z),
                       2 * (y * z - x * w), 2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)};
  for (int k = 0; k < 3; k++) {
    p.cam.pos[k] = (float)cpos[k];
    p.cam.right[k] = (float)R[3 * k + 0];
    p.cam.up[k] = (float)R[3 * k + 1];
    p.cam.back[k] = (float)R[3 * k + 2];
  }
  p.cam.tan_half = (float)std::tan(fovy * 3.14159265358979323846 / 360.0);
  // robot scenes: the rectangle walk (per-primitive pixel rectangles, colours staged in 16 KB of LDS) with one workgroup per
  // env image, or per band of rows when the image has more than 4096 pixels; the fixed scene cameras add the table of
  // env-independent rays and floor colours, computed once per size and pose. Sizes that are not multiples of 8 (and
  // kernel_variant 1) keep the 8x8-tile walk. Ladder: profiles/r02_g_render_ladder.txt.
  int band_rows = height;
  if (height * width > rend::RECT_WALK_MAX_PIXELS) band_rows = (rend::RECT_WALK_MAX_PIXELS / width) & ~7;
  const bool rect_walk = height % 8 == 0 && width % 8 == 0 && band_rows >= 8 && h->cfg.kernel_variant != MJS_VARIANT_SINGLE_WAVE;
  const unsigned nbands = rect_walk ? (unsigned)((height + band_rows - 1) / band_rows) : 1u;
  // the table is keyed by the image size and by the pose it was built for (cam_serial counts mjs_set_scene_camera calls)
  if (rect_walk && !wrist && (h->bg_H != height || h->bg_W != width || h->bg_serial != h->cam_serial)) {
    if (h->bg_ray) (void)hipFree(h->bg_ray);
    if (h->bg_rgb) (void)hipFree(h->bg_rgb);
    h->bg_ray = nullptr; h->bg_rgb = nullptr; h->bg_H = h->bg_W = 0;
    HIP_TRY(h, hipMalloc(&h->bg_ray, sizeof(float4) * height * width));
    HIP_TRY(h, hipMalloc(&h->bg_rgb, sizeof(uint32_t) * height * width));
    rend::scene_background_kernel<<<(unsigned)((height * width + 255) / 256), 256, 0, (hipStream_t)stream>>>(p, h->bg_ray, h->bg_rgb);
    HIP_TRY(h, hipGetLastError());
    HIP_TRY(h, hipStreamSynchronize((hipStream_t)stream));  // once per size and pose: later renders may come on another stream
    h->bg_H = height; h->bg_W = width; h->bg_serial = h->cam_serial;
  }
  if (rgb_dev && depth_dev) return render_launch<rend::OUT_RGB | rend::OUT_DEPTH>(h, p, depth_dev, wrist, rect_walk, band_rows, nbands, (hipStream_t)stream);
  if (depth_dev) return render_launch<rend::OUT_DEPTH>(h, p, depth_dev, wrist, rect_walk, band_rows, nbands, (hipStream_t)stream);
  return render_launch<rend::OUT_RGB>(h, p, nullptr, wrist, rect_walk, band_rows, nbands, (hipStream_t)stream);
}

int mjs_render(mjs_handle* h, int32_t camera, int32_t height, int32_t width, uint8_t* rgb_dev, void* stream) {
  if (!h || !rgb_dev) return fail(h, MJS_ERR_INVALID_ARG, "mjs_render: null argument");
  return mjs_render_rgbd(h, camera, height, width, rgb_dev, nullptr, stream);
}

int mjs_debug_ur5e_ik(const double* T_dev, const double* guess_dev, double* q_dev, uint8_t* ok_dev, int32_t n, void* stream) {
  if (!T_dev || !guess_dev || !q_dev || !ok_dev || n < 0) return fail(nullptr, MJS_ERR_INVALID_ARG, "mjs_debug_ur5e_ik: bad argument");
  debug_ik_kernel<<<grid_for(n), BLOCK, 0, (hipStream_t)stream>>>(T_dev, guess_dev, q_dev, ok_dev, n);
  HIP_TRY(nullptr, hipGetLastError());
  return MJS_OK;
}

int mjs_ur5e_tcp_to_joints(const double* tcp_pos_dev, const double* guess_dev, double* q_dev, uint8_t* ok_dev, int32_t n, void* stream) {
  if (!tcp_pos_dev || !guess_dev || !q_dev || !ok_dev || n < 0) return fail(nullptr, MJS_ERR_INVALID_ARG, "mjs_ur5e_tcp_to_joints: bad argument");
  tcp_to_joints_kernel<<<grid_for(n), BLOCK, 0, (hipStream_t)stream>>>(tcp_pos_dev, guess_dev, q_dev, ok_dev, n);
  HIP_TRY(nullptr, hipGetLastError());
  return MJS_OK;
}

int mjs_ur5e_robot_run(double* state_dev, const double* target_dev, int32_t command, double param, int32_t n_substeps, int32_t eef, double dt,
                       double* tcp_pose_out_dev, uint8_t* status_dev, int32_t n, void* stream) {
  if (!state_dev || n < 0 || n_substeps < 0 || command < MJS_UR_CMD_NONE || command > MJS_UR_CMD_SERVOJ || (command != MJS_UR_CMD_NONE && !target_dev) ||
      (eef != MJS_UR_EEF_NONE && eef != MJS_UR_EEF_GRIPPER) || !(dt > 0) || (command != MJS_UR_CMD_NONE && !(param > 0)))
    return fail(nullptr, MJS_ERR_INVALID_ARG, "mjs_ur5e_robot_run: bad argument");
  static_assert(rr::UR_STATE == MJS_UR_STATE, "state block layout");
  rr::ur_robot_kernel<<<grid_for(n), BLOCK, 0, (hipStream_t)stream>>>(state_dev, target_dev, command, param, n_substeps, eef, dt, tcp_pose_out_dev, status_dev, n);
  HIP_TRY(nullptr, hipGetLastError());
  return MJS_OK;
}

int mjs_get_state(mjs_handle* h, double* state_dev, void* stream) {
  if (!h || !state_dev) return fail(h, MJS_ERR_INVALID_ARG, "mjs_get_state: null argument");
  DeviceGuard dev_(h->cfg.device);
  HIP_TRY(h, dev_.err);
  get_state_kernel<<<grid_for(h->cfg.num_envs), BLOCK, 0, (hipStream_t)stream>>>(h->state, h->flags, state_dev, h->cfg.num_envs, h->inst.state_dim);
  HIP_TRY(h, hipGetLastError());
  return MJS_OK;
}

int mjs_set_state(mjs_handle* h, const double* state_dev, void* stream) {
  if (!h || !state_dev) return fail(h, MJS_ERR_INVALID_ARG, "mjs_set_state: null argument");
  DeviceGuard dev_(h->cfg.device);
  HIP_TRY(h, dev_.err);
  h->prims_valid = false;
  set_state_kernel<<<grid_for(h->cfg.num_envs), BLOCK, 0, (hipStream_t)stream>>>(h->state, h->flags, state_dev, h->cfg.num_envs, h->inst.state_dim, h->cfg.task, host_pending_byte(h));
  HIP_TRY(h, hipGetLastError());
  return MJS_OK;
}

int mjs_get_rng_state(mjs_handle* h, uint32_t* mt_dev, int32_t* pos_dev, void* stream) {
  if (!h || !mt_dev || !pos_dev) return fail(h, MJS_ERR_INVALID_ARG, "mjs_get_rng_state: null argument");
  DeviceGuard dev_(h->cfg.device);
  HIP_TRY(h, dev_.err);
  const size_t N = (size_t)h->cfg.num_envs;
  HIP_TRY(h, hipMemcpyAsync(mt_dev, h->rng_mt, sizeof(uint32_t) * 624 * N, hipMemcpyDeviceToDevice, (hipStream_t)stream));
  HIP_TRY(h, hipMemcpyAsync(pos_dev, h->rng_pos, sizeof(int32_t) * N, hipMemcpyDeviceToDevice, (hipStream_t)stream));
  return MJS_OK;
}

int mjs_set_rng_state(mjs_handle* h, const uint32_t* mt_dev, const int32_t* pos_dev, void* stream) {
  if (!h || !mt_dev || !pos_dev) return fail(h, MJS_ERR_INVALID_ARG, "mjs_set_rng_state: null argument");
  DeviceGuard dev_(h->cfg.device);
  HIP_TRY(h, dev_.err);
  const size_t N = (size_t)h->cfg.num_envs;
  HIP_TRY(h, hipMemcpyAsync(h->rng_mt, mt_dev, sizeof(uint32_t) * 624 * N, hipMemcpyDeviceToDevice, (hipStream_t)stream));
  HIP_TRY(h, hipMemcpyAsync(h->rng_pos, pos_dev, sizeof(int32_t) * N, hipMemcpyDeviceToDevice, (hipStream_t)stream));
  return MJS_OK;
}

}  // extern "C"
