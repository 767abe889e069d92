/* mjsim.h — C ABI of libmjsim.so: the MI355X-native batched replacement for the
 * reference's per-step hot path.
 *
 * The reference has no native boundary (it is Python over the third-party
 * `mujoco`/`dm_control` wheels), so each entry point below cites the Python
 * interface it replaces (paths relative to /root/reference/mujoco_sim/). A
 * handle steps N independent environments of ONE task on ONE GPU; all pointers
 * named *_dev are DEVICE pointers owned by the caller (PyTorch-ROCm tensors);
 * the engine owns only its persistent struct-of-arrays state. Every call
 * enqueues work on the caller's HIP stream (`stream` = hipStream_t, NULL = the
 * default stream) and never synchronises. Return value: 0 = ok, negative =
 * MJS_ERR_*; nothing throws across the ABI; per-env faults are data
 * (`mjs_outputs.fault`), not errors. A handle is not thread-safe.
 * Binding stubs for the reference side: INTEGRATION.md.
 */
#ifndef MJSIM_H
#define MJSIM_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* 2 (round 3): mjs_config starts with struct_size (validated by mjs_create: a caller built against another header is refused
 * instead of being read past its end); Robot-Reach / Button-Push state blocks grew 18 rows (qacc_warmstart, carried cos / sin):
 * checkpoints of abi 1 do not fit mjs_set_state any more (mjs_state_dim reports the new widths).
 * 3 (round 4): mjs_config ends with gripper_model and reserved0 (80 bytes; a 72-byte abi 2 config is refused by the struct_size
 * check). Entry points added since (mjs_env_algorithmic_bytes_per_env_step) leave mjs_config, and so the number, alone. */
#define MJS_ABI_VERSION 3

/* tasks (environments/tasks/*.py) */
enum {
  MJS_TASK_POINTMASS_REACH = 0, /* tasks/point_reach.py */
  MJS_TASK_ROBOT_REACH = 1,     /* tasks/robot_reach.py */
  MJS_TASK_PLANAR_PUSH = 2,     /* tasks/robot_planar_push.py (intended semantics; the reference's mesh blocks by default, DESIGN D-9) */
  MJS_TASK_BUTTON_PUSH = 3      /* tasks/robot_push_button.py */
};
/* Button-Push action spaces (robot_push_button.py:35-36,143-157): absolute joints + gripper (7-D, the
 * registered default) or absolute TCP position + gripper (4-D). The last component is the commanded finger opening in
 * metres, [0, 0.085] (Robotiq2f85.move, gripper.py:77-84): it drives the handle's 2F-85, either the reduced one (the default;
 * driver angle and velocity = rows 16, 17 of the Button-Push state) or the articulated one
 * (mjs_config.gripper_model). Other tasks ignore the field. */
enum { MJS_ACTION_ABS_JOINT = 0, MJS_ACTION_ABS_EEF = 1 };
/* reward types: point_reach.py:11-14, robot_reach.py:37-38 */
enum { MJS_REW_SPARSE = 0, MJS_REW_DENSE_POTENTIAL = 1, MJS_REW_DENSE_NEG_DISTANCE = 2, MJS_REW_DENSE_BIASED_NEG_DISTANCE = 3 };
/* dm_env StepType as produced by composer.Environment (dmc2gym.py:144-145 reads .last()) */
enum { MJS_STEP_FIRST = 0, MJS_STEP_MID = 1, MJS_STEP_LAST = 2 };
/* auto-reset: NEXT_STEP is composer.Environment's behaviour (the step after LAST ignores the
 * action and returns the reset observation); SAME_STEP is what SB3 VecEnv expects
 * (scripts/sb3/reach_sac.py:93-96): reset immediately, expose `terminal_obs`. */
enum { MJS_AUTORESET_NEXT_STEP = 0, MJS_AUTORESET_SAME_STEP = 1, MJS_AUTORESET_DISABLED = 2 };
/* kernel variants (results identical up to rounding; used for A/B profiles). Variant 1 = the first-generation kernels:
 * the single-wavefront step kernels of Robot-Reach / Button-Push (default: two role-specialised wavefronts) and the
 * 8x8-tile camera kernel for every image (default: the rectangle walk for images up to 64x64) */
enum { MJS_VARIANT_DEFAULT = 0, MJS_VARIANT_SINGLE_WAVE = 1, MJS_VARIANT_TWO_ROLES = 2 /* Robot-Reach: round 1's two-wavefront kernel */,
       MJS_VARIANT_RESET_GROUPS = 3 /* Robot-Reach (Button-Push accepts it too): the default kernel with the next-step auto-resets on workgroups
                                       of their own (other CUs, same launch). For episodes that END AT DIFFERENT TIMES
                                       (terminate_on_success): 38 instead of 54 us per launch at 4096 envs with 1 % of the envs ending
                                       in every step; with synchronous episodes it costs 0.9 us per launch. Bitwise the default's
                                       results. (The Python host picks it when terminate_on_success is set.) */ };
/* Shard invariance (env i of a sharded job == env i of the whole job, global seeds via env_index_offset) is BITWISE as long as
 * every handle of the comparison launches the same kernel. Robot-Reach with MJS_VARIANT_DEFAULT switches kernels at 16384 envs
 * per handle (three-wavefront kernel up to there, the two-role kernel above: same results to rounding only), so shards of at
 * most 16384 envs are bit-identical to each other and to any whole job of at most 16384; pin kernel_variant to compare across
 * that size. All other tasks use one kernel at every size. */
/* mjs_outputs.fault bits */
enum {
  MJS_FAULT_BAD_STATE = 1,            /* NaN / huge qpos, qvel or qacc: dm_control's PhysicsError path (episode ends, reward 0, discount 0) */
  MJS_FAULT_IK_FAILED = 2,            /* servoL found no IK solution (the reference raises ValueError): the env holds its joints */
  MJS_FAULT_LIMIT_COLDSTART = 4,      /* constraint rows (joint limits / contacts) were active in some substep (informational; the solver is
                                         warm-started like mj_fwdConstraint: qacc_warmstart = the previous Physics.step()'s solution) */
  MJS_FAULT_UNSUPPORTED_CONTACT = 8,  /* a lane had more simultaneously ACTIVE contacts than the constraint stage holds (24 on the robot
                                         scenes' robust path: arm links on the floor are solved since abi 2; Planar-Push with the arm on
                                         the floor WHILE it is coupled to a block: 5 arm-floor contacts; articulated gripper: 16 contacts);
                                         the surplus made no rows */
  MJS_FAULT_FASTPATH_VIOLATED = 16    /* the row-free fast path's a-posteriori check failed (a joint left its range, or an arm geom / the
                                         gripper stand-in touches something, at the end of a step taken without constraint rows): this env's
                                         step is unreliable */
};

enum {
  MJS_OK = 0,
  MJS_ERR_INVALID_ARG = -1,
  MJS_ERR_NO_DEVICE = -2,
  MJS_ERR_HIP = -3,
  MJS_ERR_ALLOC = -4,
  MJS_ERR_UNSUPPORTED = -5
};

typedef struct mjs_handle mjs_handle;

typedef struct {
  uint32_t struct_size;         /* sizeof(mjs_config) of the caller's header: mjs_create refuses any other value */
  int32_t task;                 /* MJS_TASK_* */
  int32_t num_envs;             /* N on this GPU */
  int32_t device;               /* HIP device ordinal */
  int32_t reward_type;          /* MJS_REW_*; <0 = task default */
  int32_t autoreset;            /* MJS_AUTORESET_* */
  int32_t terminate_on_success; /* Robot-Reach opt-in; ignored by Pointmass */
  int32_t env_index_offset;     /* global index of local env 0 (multi-GPU shards keep global seeds) */
  int32_t kernel_variant;       /* MJS_VARIANT_*: 0 = default (tuned); others for A/B profiling */
  double time_limit;            /* composer.Environment(time_limit=...) (__init__.py:21); <=0 = task default */
  int32_t action_type;          /* MJS_ACTION_* (Button-Push only) */
  int32_t button_disturbances;  /* Button-Push only: after each control step an active, released switch is
                                 * deactivated with probability 0.01 from the env's stream (robot_push_button.py:159-165) */
  int32_t n_objects;            /* Planar-Push only: number of blocks, 1..5 (robot_planar_push.py:61; <= 0: 2 = the registered env, :315,
                                 * and BASELINE config 4). 1..2 run the 2-slot kernel, 3..5 the 5-slot kernel */
  int32_t max_episode_steps;    /* Planar-Push only: RobotTask step limit (tasks/base.py:47-51); <= 0: 500 */
  int32_t block_shape;          /* Planar-Push only: MJS_BLOCKS_MESH (0, the reference: GoogleBlockProp.sample_random_object per episode,
                                 * google_block.py:55-68, category / colour / scale from the env's seeded stream) or MJS_BLOCKS_BOX (round 1's box
                                 * stand-in of the cube mesh's bounding box, scale 1: a documented fast variant) */
  int32_t gripper_model;        /* Button-Push only (abi 3): MJS_GRIPPER_REDUCED (0: the one-coordinate 2F-85 of DESIGN.md D-1b on the 6-dof arm, the
                                 * fast default) or MJS_GRIPPER_ARTICULATED (1: the Robotiq 2F-85 as entities/eef/gripper.py:36-98 attaches it -
                                 * eight hinges, two connect equalities, the driver coupling, the fixed-tendon fingers_actuator, pad boxes,
                                 * elliptic cones with impratio 10: nv = 14; mjs_env_state_dim() reports its wider state) */
  int32_t reserved0;            /* 0 */
} mjs_config;
enum { MJS_BLOCKS_MESH = 0, MJS_BLOCKS_BOX = 1 };
enum { MJS_GRIPPER_REDUCED = 0, MJS_GRIPPER_ARTICULATED = 1 };

/* Per-step outputs. Device pointers, caller-owned, any may be NULL.
 * Replaces the (obs, reward, terminated, truncated, info) tuple of
 * DMCEnvironmentAdapter.step (environments/dmc2gym.py:133-155). */
typedef struct {
  double* obs;           /* [N, obs_dim] row-major, layout: mjs_obs_dim() */
  double* terminal_obs;  /* [N, obs_dim]; written only under SAME_STEP for envs that ended */
  double* reward;        /* [N]; 0 on FIRST (dm_env: None) */
  double* discount;      /* [N]; info["discount"] (dmc2gym.py:153); 1 on FIRST (dm_env: None) */
  uint8_t* terminated;   /* [N]; last && discount == 0 (dmc2gym.py:145) */
  uint8_t* truncated;    /* [N]; last && discount > 0  (dmc2gym.py:144) */
  uint8_t* is_success;   /* [N]; info["is_success"] (dmc2gym.py:149-150) */
  uint8_t* step_type;    /* [N]; MJS_STEP_* */
  uint8_t* fault;        /* [N]; MJS_FAULT_* bits */
  int32_t* ncon;         /* [N]; detected contacts after the step (MuJoCo's d->ncon) */
} mjs_outputs;

/* Rollout outputs: same fields with a leading time axis [T, N, ...]. */

const char* mjs_version(void);
/* flat observation width: Pointmass {pointmass/position(2), goal_position(2)} (point_reach.py:115-118);
 * Robot-Reach {ur5e/tcp_position(3), ur5e/joint_configuration(6), target_position(3)}
 * (robot_reach.py:134-137, robot.py:292-298); Button-Push {ur5e/joint_configuration(6),
 * ur5e/tcp_position(3), switch/position(3), switch/active(1)} (robot_push_button.py:113-119, switch.py:99-108);
 * Planar-Push {ur5e/tcp_position(3), target_position(2), block_positions(2 per block slot; 2 slots here,
 * 5 for handles with n_objects 3..5: mjs_env_obs_dim)}
 * (robot_planar_push.py:120-126,134-138,178-179) */
int mjs_obs_dim(int task);
/* action width: 2 (point_reach.py:204-209) / 3 (robot_reach.py:187-201) / Button-Push default 7
 * (robot_push_button.py:181-203) / Planar-Push 2 (absolute TCP xy, robot_planar_push.py:197-201,222-228) */
int mjs_action_dim(int task);
/* action width for a task + MJS_ACTION_* pair (Button-Push: 7 or 4); equals mjs_action_dim otherwise */
int mjs_action_dim_for(int task, int action_type);
/* number of float64 per env in mjs_get_state / mjs_set_state: the task's state rows + 1 (the flag byte as a double, last row).
 * Robot-Reach: q6, v6, time, target3, qacc_warmstart6, cos6, sin6; Button-Push: q6, v6, time, switch position3, gripper driver
 * angle and velocity, qacc_warmstart6, cos6, sin6. cos / sin are the kernels' carried cache of the joint angles: mjs_set_state
 * keeps rows that belong to the given q (a checkpoint resumes bit for bit) and rewrites them with exact values otherwise (a
 * caller that edits q need not touch them); it also recomputes the flags that are functions of the configuration. */
int mjs_state_dim(int task);
/* the same two widths for a created handle. The per-task queries above describe each task's default instance: Planar-Push with
 * 2 block slots (obs 5 + 2*2 = 9; state 114 = two worlds of 17 + 15*2 = 47 rows, the current one and the prepared next episode,
 * + its progress row + the servo set-point 6 + cos / sin 12 + the flag row), Button-Push with the reduced gripper. Planar-Push
 * with n_objects 3..5 uses 5 block slots (obs 5 + 2*5 = 15, state 2 * (17 + 15*5) + 1 + 6 + 12 + 1 = 204), Button-Push with
 * MJS_GRIPPER_ARTICULATED 61 rows. */
int mjs_env_obs_dim(const mjs_handle* h);
int mjs_env_state_dim(const mjs_handle* h);
/* algorithmic HBM bytes one env-step moves (state R+W, action, outputs), from the real layout: of the task's default instance,
 * and of the instance a created handle runs (what a roofline figure for that handle uses) */
int mjs_algorithmic_bytes_per_env_step(int task);
int mjs_env_algorithmic_bytes_per_env_step(const mjs_handle* h);
/* physics substeps per control step: 5 (point_reach.py:24-25) / 20 (robot_reach.py:62-63, robot_planar_push.py:51-52,
 * robot_push_button.py:38-39) */
int mjs_substeps(int task);

/* Replaces task + composer.Environment + DMCEnvironmentAdapter construction
 * (mujoco_sim/__init__.py:19-23). Allocates the SoA state for N envs. */
int mjs_create(const mjs_config* cfg, mjs_handle** out);
void mjs_destroy(mjs_handle* h);
const char* mjs_last_error(const mjs_handle* h);

/* Replaces DMCEnvironmentAdapter.seed (dmc2gym.py:126-131): env i gets the numpy-legacy
 * MT19937 stream RandomState(base_seed + env_index_offset + i) (reach_sac.py:84 seeds
 * sub-env `rank` with seed+rank). The stream lives on the device. */
int mjs_seed(mjs_handle* h, uint32_t base_seed, void* stream);

/* Replaces DMCEnvironmentAdapter.reset -> composer.Environment.reset (dmc2gym.py:157-163):
 * starts a new episode for every env whose mask byte is non-zero (mask_dev NULL = all). */
int mjs_reset(mjs_handle* h, const uint8_t* mask_dev, const mjs_outputs* out, void* stream);

/* Replaces DMCEnvironmentAdapter.step -> composer.Environment.step -> n_sub x Physics.step
 * (dmc2gym.py:133-155): one control step of all N envs, one kernel launch.
 * actions_dev: float64 [N, action_dim]. */
int mjs_step(mjs_handle* h, const double* actions_dev, const mjs_outputs* out, void* stream);

/* T consecutive mjs_step calls with precomputed actions [T, N, action_dim]; outputs carry a
 * leading T axis. Open-loop rollouts (random / scripted policies, point_reach.py:218-240). */
int mjs_rollout(mjs_handle* h, const double* actions_dev, int32_t T, const mjs_outputs* out, void* stream);

/* Replaces Camera.get_rgb_image -> physics.render(height, width, camera_id) (entities/camera.py:94-103)
 * and DMCEnvironmentAdapter.render (dmc2gym.py:165-168) for the task's scene camera
 * (camera = MJS_CAMERA_SCENE) and, for Button-Push, the camera mounted on the flange
 * (MJS_CAMERA_WRIST, robot_push_button.py:90-96): rgb_dev uint8 [N, height, width, 3]. Own ray caster,
 * cannot match OpenGL pixels. */
enum { MJS_CAMERA_SCENE = 0, MJS_CAMERA_WRIST = 1 };
int mjs_render(mjs_handle* h, int32_t camera, int32_t height, int32_t width, uint8_t* rgb_dev, void* stream);

/* The scene camera of a handle (entry points added after abi 3; mjs_config and the number stay as they are). Replaces the
 * `cameraconfig` field of RobotReachConfig / RobotPushConfig (tasks/robot_reach.py:70, robot_planar_push.py:63: any
 * CameraConfig(position, orientation, fov), entities/camera.py:55-64) for MJS_CAMERA_SCENE of all four tasks; the Button-Push
 * wrist camera stays mounted on the flange. The pose belongs to the handle, not to the state block: checkpoints
 * (get / set state) neither carry nor touch it, and it plays no part in shard invariance. The camera's own body (box and lens,
 * camera.py:78-88) moves with the pose. Collision is unchanged: neither side collides the camera's geoms,
 * wherever the camera stands. */
typedef struct {
  uint32_t struct_size; /* sizeof(mjs_camera_pose), validated like mjs_config's */
  int32_t reserved0;    /* 0 */
  double pos[3];        /* world */
  double quat[4];       /* MuJoCo order w,x,y,z; normalised by the library; the camera looks along its local -z, +y is up (camera.py:58) */
  double fovy;          /* degrees, 0 < fovy < 180 */
} mjs_camera_pose;      /* 72 bytes */
/* pose NULL: back to the task's default. MJS_ERR_INVALID_ARG (text in mjs_last_error) for non-finite numbers, a quaternion of
 * norm below 1e-9, fovy out of range or a wrong struct_size; the handle's camera is then unchanged. */
int mjs_set_scene_camera(mjs_handle* h, const mjs_camera_pose* pose);
/* the pose in use, with the quaternion normalised */
int mjs_get_scene_camera(const mjs_handle* h, mjs_camera_pose* out);
/* The render entry point with an optional depth map (Camera.get_depth_map, camera.py:105-114): rgb_dev uint8 [N, height, width, 3]
 * or NULL, depth_dev float32 [N, height, width] or NULL (both NULL: MJS_ERR_INVALID_ARG). Depth is z-depth in metres, the
 * nearest hit's distance along the optical axis as physics.render(depth=True) defines it, +inf where the ray hits nothing; the
 * translucent Pointmass sphere counts as a surface. The rgb image is the one the rgb-only entry point above writes. */
int mjs_render_rgbd(mjs_handle* h, int32_t camera, int32_t height, int32_t width, uint8_t* rgb_dev, float* depth_dev, void* stream);

/* Test hook: the device implementation of ur5e.inverse_kinematics_closest (entities/robots/robot.py:33-37)
 * on n independent inputs: flange poses T_dev [n, 12] (row-major 3x3 rotation then translation),
 * guesses [n, 6] -> q_dev [n, 6], ok_dev [n]. No handle needed; device = current HIP device. */
int mjs_debug_ur5e_ik(const double* T_dev, const double* guess_dev, double* q_dev, uint8_t* ok_dev, int32_t n, void* stream);

/* Replaces Robot.get_joint_positions_from_tcp_pose (entities/robots/robot.py:33-37,140-151) for the top-down
 * TCP orientation every task uses: n TCP positions [n, 3] + current joints [n, 6] -> closest IK solution
 * q_dev [n, 6] (the guess itself where none exists), ok_dev [n]. What a host policy needs to turn a
 * Cartesian target into a Button-Push joint action (robot_push_button.py:287-291). */
int mjs_ur5e_tcp_to_joints(const double* tcp_pos_dev, const double* guess_dev, double* q_dev, uint8_t* ok_dev, int32_t n, void* stream);

/* The tasks' scripted demonstration policies on the device (entry points added after abi 3; mjs_config and the number stay as they
 * are). Replaces the policy closures the reference's collector drives (scripts/demonstration_collection.py:303-345):
 * PointMassReachTask.create_demonstation_policy (point_reach.py:227-240), create_demonstration_policy of robot_reach.py:222-253 and
 * RobotPushButtonTask.create_demonstration_policy (robot_push_button.py:231-300). One launch for the handle's task and action type:
 * obs_dev float64 [N, obs_dim] (layout: mjs_obs_dim; what the last reset / step wrote) -> actions_dev float64 [N, action_dim],
 * ik_ok_dev uint8 [N] or NULL. Button-Push with MJS_ACTION_ABS_JOINT runs the IK of mjs_ur5e_tcp_to_joints inside the same launch
 * (guess = the joints in obs); where no solution exists the action holds the current joints and ik_ok is 0 (the reference
 * raises); ik_ok is 1 wherever no IK was needed. Noise: the reference draws it from the global np.random (no env stream, so
 * nothing to reproduce); the caller passes standard-normal draws noise_z_dev, float64 [N, 2] for Pointmass (a *= 1 + noise * z) or
 * [N, 3] for Robot-Reach (d += noise * z); NULL or noise == 0: none; Button-Push ignores both. MJS_ERR_INVALID_ARG for a negative or
 * non-finite noise; MJS_ERR_UNSUPPORTED for Planar-Push, whose "demonstration policy" is a keyboard teleop
 * (robot_planar_push.py:288-308). */
int mjs_demonstration_actions(mjs_handle* h, const double* obs_dev, const double* noise_z_dev, double noise, double* actions_dev, uint8_t* ik_ok_dev,
                              void* stream);

/* What a closed-loop demonstration rollout writes besides mjs_outputs, and its noise. */
typedef struct {
  uint32_t struct_size;        /* sizeof(mjs_demo_rollout), validated like mjs_config's */
  int32_t height, width;       /* of the image buffers; ignored when both are NULL */
  int32_t reserved0;           /* 0 */
  double noise;                /* as in mjs_demonstration_actions */
  const double* noise_z_dev;   /* [T, N, k] (k = 2 Pointmass, 3 Robot-Reach) or NULL */
  double* actions_out_dev;     /* [T, N, action_dim], required: the action the policy chose at every step */
  uint8_t* ik_ok_dev;          /* [T, N] or NULL */
  uint8_t* scene_rgb_dev;      /* [T, N, height, width, 3] or NULL: MJS_CAMERA_SCENE before every step */
  uint8_t* wrist_rgb_dev;      /* the same for MJS_CAMERA_WRIST (Button-Push only) */
} mjs_demo_rollout;            /* 64 bytes */
/* The collector's loop (demonstration_collection.py:303-345) for T control steps without returning to the host: before step t the
 * policy reads the observation of step t-1 (slice t-1 of out->obs; obs0_dev, the observation the caller's last reset or step
 * wrote, for t = 0) and writes slice t of demo->actions_out_dev (and of ik_ok_dev); the cameras, where buffers are given, are
 * rendered next (slice t = the frame BEFORE the action, which is what the recorder stores; the launches of mjs_render); then the
 * ordinary step launch writes slice t of out, sliced as mjs_rollout slices it. 2 launches per step without images. out->obs and
 * demo->actions_out_dev are required (MJS_ERR_INVALID_ARG otherwise, as for T < 0, a wrong struct_size, a wrist buffer on a task
 * without a wrist camera, image buffers without a positive size, or obs0_dev NULL with T > 0); T == 0 does nothing and returns 0.
 * MJS_ERR_UNSUPPORTED for Planar-Push. */
int mjs_rollout_demonstration(mjs_handle* h, const double* obs0_dev, int32_t T, const mjs_demo_rollout* demo, const mjs_outputs* out, void* stream);

/* A learned policy on the device (entry points added after abi 3; mjs_config and the number stay as they are): the MLP actor of SAC
 * as the reference's RL scripts configure it (scripts/sb3/reach_sac.py, planar_push.py, sb3_sac.py: net_arch pi = [64, 64] / [32],
 * SB3's default [256, 256]; stable_baselines3/sac/policies.py Actor), evaluated for every env of a handle in ONE launch
 * (csrc/mjs_actor.h), in float32 with float32 accumulation, as SB3 evaluates it:
 *   x_j = (float) obs[i, obs_index[j]]   j < in_dim            h_l = act(W_l h_{l-1} + b_l)   l = 1..n_hidden
 *   mu = W_mu h + b_mu    ls = clamp(W_ls h + b_ls, -20, 2)     u = mu (z NULL) or mu + expf(ls) * z[i]
 *   a = tanhf(u) -> squashed_out (what a replay buffer stores)  actions = low + 0.5 * ((double) a + 1.0) * (high - low)  in float64
 * An actor belongs to a device, not to a handle: any handle of that device whose action width is action_dim and whose observation
 * row holds every obs_index entry may use it. */
typedef struct mjs_actor mjs_actor;
enum { MJS_ACTIVATION_RELU = 0, MJS_ACTIVATION_TANH = 1 };
enum { MJS_ACTOR_VARIANT_DEFAULT = 0 /* 16 envs per workgroup on v_mfma_f32_16x16x4_f32 */,
       MJS_ACTOR_VARIANT_TILE32 = 1 /* 32 envs per workgroup on v_mfma_f32_32x32x2_f32: results equal to rounding (another summation
                                       order over k); for A/B measurements */ };
typedef struct {
  uint32_t struct_size;      /* sizeof(mjs_actor_desc), validated like mjs_config's */
  int32_t device;            /* HIP device ordinal */
  int32_t in_dim;            /* 1..64 */
  int32_t n_hidden;          /* 1..3 */
  int32_t hidden[3];         /* widths, each 1..256; entries past n_hidden are ignored */
  int32_t action_dim;        /* 1..8; must equal the action width of every handle the actor is used with */
  int32_t activation;        /* MJS_ACTIVATION_* */
  int32_t variant;           /* MJS_ACTOR_VARIANT_* */
  const int32_t* obs_index;  /* HOST int32 [in_dim], copied: the column of a flat observation row that feeds input j; each >= 0 */
} mjs_actor_desc;            /* 48 bytes */
/* Allocates the packed weight buffers and nothing else. MJS_ERR_INVALID_ARG (text in mjs_last_error(NULL)) for a wrong struct_size,
 * a null pointer, or in_dim, n_hidden, a width, action_dim, activation, variant or an obs_index entry out of range. */
int mjs_actor_create(const mjs_actor_desc* desc, mjs_actor** out);
void mjs_actor_destroy(mjs_actor* actor);
/* DEVICE pointers to float32 parameters in torch.nn.Linear layout: weight [out, in] row-major, bias [out]. */
typedef struct {
  uint32_t struct_size;        /* sizeof(mjs_actor_weights) */
  int32_t reserved0;           /* 0 */
  const float* hidden_w[3];    /* layer l: [hidden[l], l == 0 ? in_dim : hidden[l-1]]; entries past n_hidden are ignored */
  const float* hidden_b[3];
  const float *mu_w, *mu_b;    /* [action_dim, hidden[n_hidden-1]], [action_dim] */
  const float *log_std_w, *log_std_b;
} mjs_actor_weights;           /* 88 bytes */
/* Packs the parameters into the actor's own K-major copy with small kernels on the caller's stream; never synchronises (a training
 * loop calls it after every policy update; launches that use the actor are ordered after it by the stream). */
int mjs_actor_load(mjs_actor* actor, const mjs_actor_weights* weights, void* stream);
/* One launch: obs_dev float64 [N, obs_dim] (what the last reset / step wrote) -> actions_dev float64 [N, action_dim] and, unless
 * NULL, squashed_out_dev float32 [N, action_dim]. z_dev: float32 [N, action_dim] standard-normal draws, or NULL for the
 * deterministic action. low / high: HOST float64 [action_dim], the action space's bounds. MJS_ERR_INVALID_ARG (nothing launched)
 * for a null required pointer, an obs_index entry outside the handle's mjs_env_obs_dim, an action_dim other than the handle's, an
 * actor of another device, or an actor that was never loaded. All four tasks. */
int mjs_actor_actions(mjs_handle* h, const mjs_actor* actor, const double* obs_dev, const float* z_dev, const double* low, const double* high,
                      double* actions_dev, float* squashed_out_dev, void* stream);
typedef struct {
  uint32_t struct_size;        /* sizeof(mjs_actor_rollout) */
  int32_t height, width;       /* of the image buffers; ignored when both are NULL */
  int32_t reserved0;           /* 0 */
  const float* z_dev;          /* [T, N, action_dim] or NULL (deterministic) */
  const double* low;           /* HOST [action_dim] */
  const double* high;          /* HOST [action_dim] */
  double* actions_out_dev;     /* [T, N, action_dim], required */
  float* squashed_out_dev;     /* [T, N, action_dim] or NULL */
  uint8_t* scene_rgb_dev;      /* [T, N, height, width, 3] or NULL: MJS_CAMERA_SCENE before every step */
  uint8_t* wrist_rgb_dev;      /* the same for MJS_CAMERA_WRIST (Button-Push only) */
} mjs_actor_rollout;           /* 72 bytes */
/* mjs_rollout_demonstration with the actor as the policy, clause for clause (the same loop): before step t the actor reads the
 * observation of step t-1 (slice t-1 of out->obs; obs0_dev for t = 0) and writes slice t of actions_out_dev (and of
 * squashed_out_dev); the cameras, where buffers are given, are rendered next; then the ordinary step launch writes slice t of
 * out. 2 launches per step without images. The refusals of mjs_rollout_demonstration and of mjs_actor_actions; T == 0 does nothing
 * and returns 0. All four tasks (Planar-Push too). */
int mjs_rollout_actor(mjs_handle* h, const mjs_actor* actor, const double* obs0_dev, int32_t T, const mjs_actor_rollout* roll, const mjs_outputs* out,
                      void* stream);

/* The image encoder of a visual policy on the device (entry points added after abi 3; mjs_config and the number stay as they are):
 * SB3's NatureCNN (stable_baselines3/common/torch_layers.py), what MultiInputPolicy's CombinedExtractor puts between every camera
 * image and the actor above in the reference's RL scripts (scripts/sb3/reach_sac.py, planar_push.py, sb3_sac.py: observation_type
 * VISUAL_OBS), evaluated on the frames mjs_render writes (csrc/mjs_encoder.h), in float32 with float32 accumulation:
 *   x[c][y][x] = (float) rgb[n][y][x][c] / 255.0f      conv1 3->32 8x8 stride 4, conv2 32->64 4x4 stride 2, conv3 64->64 3x3 stride 1,
 *   no padding, ReLU after each; flat = conv3's output in CHW order; features = ReLU(W_fc flat + b_fc).
 * An encoder belongs to a device and an image size, not to a handle. */
typedef struct mjs_encoder mjs_encoder;
typedef struct {
  uint32_t struct_size;      /* sizeof(mjs_encoder_desc), validated like mjs_config's */
  int32_t device;            /* HIP device ordinal */
  int32_t height, width;     /* of the frames: each 36..96 (36 is NatureCNN's own minimum), need not be equal */
  int32_t channels;          /* 3 */
  int32_t features_dim;      /* F: 1..512 */
} mjs_encoder_desc;          /* 24 bytes */
/* Allocates the packed weight buffers and nothing else. MJS_ERR_INVALID_ARG (text in mjs_last_error(NULL)) for a wrong struct_size, a
 * null pointer or any field out of range. */
int mjs_encoder_create(const mjs_encoder_desc* desc, mjs_encoder** out);
void mjs_encoder_destroy(mjs_encoder* enc);
/* DEVICE pointers to float32 parameters in torch layout: Conv2d weight [out, in, kh, kw], Linear weight [F, n_flatten], biases [out]. */
typedef struct {
  uint32_t struct_size;      /* sizeof(mjs_encoder_weights) */
  int32_t reserved0;         /* 0 */
  const float *conv1_w, *conv1_b;  /* [32, 3, 8, 8], [32] */
  const float *conv2_w, *conv2_b;  /* [64, 32, 4, 4], [64] */
  const float *conv3_w, *conv3_b;  /* [64, 64, 3, 3], [64] */
  const float *fc_w, *fc_b;        /* [F, mjs_encoder_flat_dim], [F] */
} mjs_encoder_weights;       /* 72 bytes */
/* Packs the parameters into the encoder's own K-major copy with small kernels on the caller's stream; never synchronises
 * (mjs_actor_load's contract). */
int mjs_encoder_load(mjs_encoder* enc, const mjs_encoder_weights* weights, void* stream);
/* n_flatten = 64 * H3 * W3, the width of the linear layer's input (negative: enc is NULL) */
int mjs_encoder_flat_dim(const mjs_encoder* enc);
/* bytes of the workspace mjs_encoder_features needs for n images (conv3's output, float32 [n, n_flatten]); 0 for a bad argument */
uint64_t mjs_encoder_workspace_bytes(const mjs_encoder* enc, int32_t n);
/* Two launches: rgb_dev uint8 [n, height, width, 3] -> features_dev float32 [n, F]. workspace_dev: mjs_encoder_workspace_bytes(enc, n)
 * bytes, 16-byte aligned, overwritten. No handle; the launches go to the encoder's device. MJS_ERR_INVALID_ARG (nothing launched) for
 * a null pointer, n < 0 or an encoder that was never loaded; n == 0 does nothing and returns 0. */
int mjs_encoder_features(const mjs_encoder* enc, const uint8_t* rgb_dev, int32_t n, void* workspace_dev, float* features_dev, void* stream);

/* A visual actor: the MLP actor above whose input vector is a concatenation of observation columns (desc->in_dim of them, 0..64, in
 * obs_index order) and up to two float32 feature blocks [N, width] from encoders. Slot 0 is the scene camera's block, slot 1 the
 * wrist camera's (Button-Push); a slot of width 0 is absent. start[s] is the position of the block's first component in the input
 * vector; the observation columns fill the positions the blocks leave, in order. The first layer's weight is
 * [hidden[0], in_dim + width[0] + width[1]]. */
typedef struct {
  uint32_t struct_size;      /* sizeof(mjs_actor_feature_inputs) */
  int32_t n_blocks;          /* 1..2: the number of slots with a positive width */
  int32_t width[2];          /* 0 (absent) or 1..512 */
  int32_t start[2];          /* 0..in_dim + the other block's width; blocks must not overlap */
} mjs_actor_feature_inputs;  /* 24 bytes */
/* mjs_actor_create for a visual actor. desc as there, except that in_dim may be 0 (obs_index is then ignored) and variant must be
 * MJS_ACTOR_VARIANT_DEFAULT. Such an actor is refused by mjs_actor_actions / mjs_rollout_actor, and an actor of mjs_actor_create by
 * the two entry points below; mjs_actor_load and mjs_actor_destroy serve both. */
int mjs_actor_create_visual(const mjs_actor_desc* desc, const mjs_actor_feature_inputs* blocks, mjs_actor** out);
/* mjs_actor_actions with the feature blocks: features_dev[s] float32 [N, width[s]] for every slot the actor has (others ignored). */
int mjs_actor_actions_visual(mjs_handle* h, const mjs_actor* actor, const double* obs_dev, const float* const features_dev[2], const float* z_dev,
                             const double* low, const double* high, double* actions_dev, float* squashed_out_dev, void* stream);
typedef struct {
  uint32_t struct_size;        /* sizeof(mjs_visual_rollout) */
  int32_t reserved0;           /* 0 */
  const float* z_dev;          /* [T, N, action_dim] or NULL (deterministic) */
  const double* low;           /* HOST [action_dim] */
  const double* high;          /* HOST [action_dim] */
  double* actions_out_dev;     /* [T, N, action_dim], required */
  float* squashed_out_dev;     /* [T, N, action_dim] or NULL */
  uint8_t* scene_rgb_dev;      /* [T, N, H, W, 3] or NULL; H x W are the encoders' */
  uint8_t* wrist_rgb_dev;      /* the same for MJS_CAMERA_WRIST (Button-Push only) */
  uint8_t* scene_scratch_dev;  /* [N, H, W, 3]: one step's frame of a camera the actor uses; required where its [T, ...] buffer is NULL */
  uint8_t* wrist_scratch_dev;
  float* features_dev[2];      /* [N, width[s]]: required for every slot the actor has; overwritten at every step */
  void* workspace_dev;         /* required: the largest mjs_encoder_workspace_bytes(enc[s], N) of the encoders given */
} mjs_visual_rollout;          /* 104 bytes */
/* mjs_rollout_actor for a visual actor: enc[0] encodes the scene camera, enc[1] the wrist camera, given exactly for the slots the
 * actor has; both of one image size. Per control step t, in order: the cameras the actor uses (and those with a [T, ...] buffer) are
 * rendered at the encoders' H x W (the launches of mjs_render; slice t = the frame BEFORE the action); the encoders run
 * (mjs_encoder_features); the actor launch reads slice t-1 of out->obs (obs0_dev for t = 0) and the feature blocks; the ordinary step
 * launch writes slice t of out. Refusals (nothing launched, text in mjs_last_error): those of mjs_rollout_actor; an encoder of another
 * device; an encoder never loaded; an encoder whose F is not the actor's block width, or missing or surplus for a slot; encoders of
 * two image sizes; a wrist encoder or buffer on a task without a wrist camera; a null workspace, feature buffer or required
 * scratch. T == 0 does nothing and returns 0. All four tasks, whatever the handle's observation settings. */
int mjs_rollout_visual_actor(mjs_handle* h, const mjs_actor* actor, mjs_encoder* const enc[2], const double* obs0_dev, int32_t T,
                             const mjs_visual_rollout* roll, const mjs_outputs* out, void* stream);

/* A replay buffer on the device (entry points added after abi 3; mjs_config and the number stay as they are): the blocks the two
 * rollouts above write, turned into the transitions SAC learns from, and batches drawn from them. A restatement of SB3's
 * ReplayBuffer.add / sample (stable_baselines3/common/buffers.py; buffer_size=200_000 in scripts/sb3/reach_sac.py:108-124) over a
 * [T, N] block. The entry points are stateless: the storage is a descriptor of caller-owned device memory (csrc/mjs_replay.h).
 *
 * Row (t, n) of a block is a transition iff step_type[t, n] != MJS_STEP_FIRST under MJS_AUTORESET_NEXT_STEP (the step after a LAST
 * returns FIRST with the action ignored, composer.Environment's auto-reset) and always under MJS_AUTORESET_SAME_STEP. It stores
 *   obs      = (float) prev[n, obs_index[j]], prev = obs[t-1], obs0 for t = 0 (the rounding of the actor's own input)
 *   next_obs = the same columns of obs[t]; under same-step auto-reset, where terminated | truncated, of terminal_obs[t]
 *   action   = squashed_actions[t, n]        reward = (float) reward[t, n]
 *   done     = terminated ? 1.0f : 0.0f      (SB3's dones * (1 - timeouts); dmc2gym.py:144-145)      timeout = truncated
 *   rgb[c]   = frame t of camera c, next_rgb[c] = frame t + 1, final_rgb[c] for t = T - 1 (frames are taken BEFORE the action)
 * The r-th transition of a block in (t, n) order goes to ring row (count + r) % capacity, count = *cursor_dev = the number of
 * transitions ever added; afterwards count += the block's transitions. Neither entry point reads anything back to the host or
 * synchronises. */
#define MJS_REPLAY_MAX_OBS 64
#define MJS_REPLAY_MAX_CAMERAS 2
typedef struct {
  uint32_t struct_size;      /* sizeof(mjs_replay_storage), validated like mjs_config's */
  int32_t device;            /* HIP device ordinal */
  int32_t capacity;          /* ring rows: >= 1 */
  int32_t obs_dim;           /* D, stored observation columns: 0..64 */
  int32_t action_dim;        /* 1..8 */
  int32_t n_cameras;         /* 0..2 */
  int32_t height, width;     /* of the frames; positive where n_cameras > 0 */
  uint64_t* cursor_dev;      /* one uint64: transitions ever added */
  float* obs;                /* [capacity, D] (may be NULL where D == 0, like next_obs) */
  float* next_obs;           /* [capacity, D] */
  float* actions;            /* [capacity, action_dim] */
  float* rewards;            /* [capacity] */
  float* dones;              /* [capacity] */
  uint8_t* timeouts;         /* [capacity] */
  uint8_t* rgb[2];           /* [capacity, height, width, 3] for every camera c < n_cameras */
  uint8_t* next_rgb[2];
} mjs_replay_storage;        /* 120 bytes */
typedef struct {
  uint32_t struct_size;            /* sizeof(mjs_replay_block) */
  int32_t T, N;                    /* control steps and envs of the block */
  int32_t src_dim;                 /* width of a row of obs0 / obs / terminal_obs */
  int32_t autoreset;               /* MJS_AUTORESET_NEXT_STEP or MJS_AUTORESET_SAME_STEP, the mode the block was made under */
  int32_t reserved0;               /* 0 */
  const int32_t* obs_index;        /* HOST [D]: the source column of stored column j, each 0..src_dim-1; copied during the call */
  const double* obs0;              /* [N, src_dim]: the observation the first actor launch read */
  const double* obs;               /* [T, N, src_dim] */
  const double* terminal_obs;      /* [T, N, src_dim]: required under same-step auto-reset, ignored otherwise */
  const double* reward;            /* [T, N] */
  const uint8_t* terminated;       /* [T, N] */
  const uint8_t* truncated;        /* [T, N] */
  const uint8_t* step_type;        /* [T, N]: required under next-step auto-reset */
  const float* squashed_actions;   /* [T, N, action_dim] */
  const uint8_t* rgb[2];           /* [T, N, height, width, 3] for every camera of the storage */
  const uint8_t* final_rgb[2];     /* [N, height, width, 3]: the frame after the block's last step */
} mjs_replay_block;                /* 128 bytes */
typedef struct {
  uint32_t struct_size;      /* sizeof(mjs_replay_batch) */
  int32_t reserved0;         /* 0 */
  int64_t* idx_out;          /* [B]: the ring rows gathered; like every pointer below it may be NULL (that output is skipped) */
  float* obs;                /* [B, D] */
  float* next_obs;           /* [B, D] */
  float* actions;            /* [B, action_dim] */
  float* rewards;            /* [B] */
  float* dones;              /* [B] */
  uint8_t* timeouts;         /* [B] */
  uint8_t* rgb[2];           /* [B, height, width, 3] */
  uint8_t* next_rgb[2];
} mjs_replay_batch;          /* 96 bytes */
/* bytes of the workspace mjs_replay_add needs for a block of T x N rows (chunk counts and every row's ring row); 0 for a bad argument */
uint64_t mjs_replay_workspace_bytes(int32_t T, int32_t N);
/* Appends a block's transitions: three launches on the caller's stream, a fourth with cameras. workspace_dev:
 * mjs_replay_workspace_bytes(T, N) bytes, 16-byte aligned, overwritten. MJS_ERR_INVALID_ARG (nothing launched, text in
 * mjs_last_error(NULL)) for a null argument or required pointer, a wrong struct_size, capacity < 1, T * N > capacity, obs_dim,
 * action_dim or n_cameras out of range, cameras without a positive size, src_dim < 1, an obs_index entry outside the source row,
 * MJS_AUTORESET_DISABLED (or no mode at all), cameras under same-step auto-reset (the terminal frame does not exist there), same-step
 * auto-reset without terminal_obs, T < 0 or N < 1. T == 0 does nothing and returns 0. */
int mjs_replay_add(const mjs_replay_storage* storage, const mjs_replay_block* block, void* workspace_dev, void* stream);
/* Gathers ring rows draws_dev[b] % min(count, capacity) into the outputs given, and the rows used into idx_out: two launches at most.
 * draws_dev: non-negative int64 [B] on the device. While the buffer is empty idx_out is -1 and every output row zero.
 * MJS_ERR_INVALID_ARG (nothing launched) for a null argument, a wrong struct_size, a storage mjs_replay_add would refuse or B < 0;
 * B == 0 does nothing and returns 0. */
int mjs_replay_sample(const mjs_replay_storage* storage, const int64_t* draws_dev, int32_t B, const mjs_replay_batch* out, void* stream);

/* SAC's critics and the no-gradient half of its update on the device (entry points added after abi 3; mjs_config and the number stay as
 * they are): what stable_baselines3/sac/sac.py SAC.train computes first from a batch of mjs_replay_sample, under torch.no_grad(),
 * with the twin Q networks of stable_baselines3/common/policies.py ContinuousCritic (csrc/mjs_critic.h), in float32 with float32
 * accumulation like the actor above:
 *   Q_c(o, a)   = W_head act(... act(W_0 [o | a] + b_0) ...) + b_head                       c < n_critics, one scalar per row
 *   ls = clamp(log_std(next_obs), -20, 2)    u = mu(next_obs) + expf(ls) * z    a' = tanhf(u)
 *   logp = sum_j (-0.5 z_j^2 - ls_j - 0.5 log(2 pi)) - sum_j logf(1 - a'_j^2 + 1e-6)         j = 0..action_dim-1 in order, then one subtraction
 *   target = r + (1 - done) * gamma * (min_c Q_c(next_obs, a') - ent_coef * logp)            operation by operation, no contraction
 * Nothing here takes a gradient. A critic belongs to a device, like an actor. */
#define MJS_CRITIC_MAX 2
typedef struct mjs_critic mjs_critic;
typedef struct {
  uint32_t struct_size;      /* sizeof(mjs_critic_desc), validated like mjs_config's */
  int32_t device;            /* HIP device ordinal */
  int32_t obs_dim;           /* D: 1..64 (MJS_REPLAY_MAX_OBS) */
  int32_t action_dim;        /* A: 1..8; the first layer reads D + A columns */
  int32_t n_critics;         /* 1..2 networks of one architecture */
  int32_t n_hidden;          /* 1..3 */
  int32_t hidden[3];         /* widths, each 1..256; entries past n_hidden are ignored */
  int32_t activation;        /* MJS_ACTIVATION_* */
} mjs_critic_desc;           /* 40 bytes */
/* Allocates the packed weight buffers and nothing else. MJS_ERR_INVALID_ARG (text in mjs_last_error(NULL)) for a wrong struct_size,
 * a null pointer or any field out of range. */
int mjs_critic_create(const mjs_critic_desc* desc, mjs_critic** out);
void mjs_critic_destroy(mjs_critic* critic);
/* DEVICE pointers to float32 parameters in torch.nn.Linear layout, per critic c < n_critics (entries past it are ignored). */
typedef struct {
  uint32_t struct_size;          /* sizeof(mjs_critic_weights) */
  int32_t reserved0;             /* 0 */
  const float* hidden_w[2][3];   /* [c][l]: [hidden[l], l == 0 ? obs_dim + action_dim : hidden[l-1]]; layers past n_hidden are ignored */
  const float* hidden_b[2][3];
  const float* out_w[2];         /* [1, hidden[n_hidden-1]] */
  const float* out_b[2];         /* [1] */
} mjs_critic_weights;            /* 136 bytes */
/* Blends the parameters into the critic's own K-major copy with small kernels on the caller's stream: copy = (1 - tau) * copy + tau *
 * given, SB3's polyak_update done on the packed copy (its padding stays 0), so that a target critic needs no torch module. tau in
 * (0, 1]; tau == 1 copies, and a first load must have tau == 1 (the copy is uninitialised before it): MJS_ERR_INVALID_ARG otherwise,
 * as for a null pointer or a wrong struct_size. Never synchronises (the contract of mjs_actor_load). */
int mjs_critic_load(mjs_critic* critic, const mjs_critic_weights* weights, double tau, void* stream);
/* One launch: obs_dev float32 [B, obs_dim], actions_dev float32 [B, action_dim] -> q_out_dev float32 [n_critics, B]. No handle; the
 * launch goes to the critic's device. MJS_ERR_INVALID_ARG (nothing launched) for a null pointer, B < 0 or a critic that was never
 * loaded; B == 0 does nothing and returns 0. */
int mjs_critic_q(const mjs_critic* critic, const float* obs_dev, const float* actions_dev, int32_t B, float* q_out_dev, void* stream);
typedef struct {
  uint32_t struct_size;          /* sizeof(mjs_td_target_args) */
  int32_t B;                     /* batch rows: >= 0 */
  const float* next_obs_dev;     /* [B, obs_dim], required: the actor's input columns in order (its obs_index plays no role) */
  const float* rewards_dev;      /* [B], required */
  const float* dones_dev;        /* [B], required: 1.0f where the episode terminated (mjs_replay_sample's dones) */
  const float* z_dev;            /* [B, action_dim], required: standard-normal draws */
  double gamma;                  /* 0..1, rounded to float32 */
  double ent_coef;               /* rounded to float32; ignored where ent_coef_dev is given */
  const float* ent_coef_dev;     /* one float32 on the device (SB3's learned coefficient), read by the kernel, or NULL */
  float* target_out_dev;         /* [B], required */
  float* next_actions_out_dev;   /* [B, action_dim] or NULL: a' */
  float* next_log_prob_out_dev;  /* [B] or NULL: logp */
  float* q_next_out_dev;         /* [n_critics, B] or NULL: Q_c(next_obs, a') before the min */
} mjs_td_target_args;            /* 96 bytes */
/* One launch for the whole block above (the actor's variant is ignored: 16 rows per workgroup). q_next_out_dev equals, bit for bit,
 * what mjs_critic_q gives on (next_obs, next_actions_out_dev). MJS_ERR_INVALID_ARG (nothing launched, text in mjs_last_error(NULL)) for
 * a null argument or required pointer, a wrong struct_size, B < 0, gamma outside [0, 1], an actor or critic that was never loaded,
 * actor and critic of different devices, an actor of mjs_actor_create_visual, or an actor whose in_dim or action_dim is not the
 * critic's obs_dim or action_dim. B == 0 does nothing and returns 0. */
int mjs_sac_td_target(const mjs_actor* actor, const mjs_critic* critic, const mjs_td_target_args* args, void* stream);

/* The critic update of SAC.train on the device (csrc/mjs_critic_train.h; entry points added after abi 3 as well): for a batch and the
 * target y of mjs_sac_td_target,
 *   critic_loss = 0.5 * sum_c mean((Q_c(obs, actions) - y)^2);  zero_grad, backward, torch.optim.Adam.step  (amsgrad, weight decay: off)
 * on the critic's PACKED copy, which becomes the master copy of the parameters: mjs_critic_q and mjs_sac_td_target see every step at
 * once, a target critic blends from the online critic's packed copy (mjs_critic_blend), and mjs_critic_export writes torch.nn.Linear
 * tensors when somebody wants them. float32 with float32 accumulation. The sum over the batch is bitwise reproducible: workgroups own
 * contiguous 16-row tiles, store one partial slab each, and the slabs are summed in order (no atomics). */
typedef struct mjs_critic_opt mjs_critic_opt;
typedef struct {
  uint32_t struct_size;      /* sizeof(mjs_critic_opt_desc) */
  int32_t reserved0;         /* 0 */
  double lr;                 /* >= 0: the default of mjs_critic_update's lr argument is the caller's business; kept for reference */
  double beta1;              /* [0, 1) */
  double beta2;              /* [0, 1) */
  double eps;                /* > 0 */
} mjs_critic_opt_desc;       /* 40 bytes */
/* An optimiser is bound to ONE loaded critic, which must outlive it. It owns zeroed first and second moments, the slab workspace (the
 * largest mjs_critic_train_workspace_bytes of any B) and the step count t = 0. MJS_ERR_INVALID_ARG for a null pointer, a wrong
 * struct_size, a critic that was never loaded, lr < 0, a beta outside [0, 1) or eps <= 0. */
int mjs_critic_opt_create(mjs_critic* critic, const mjs_critic_opt_desc* desc, mjs_critic_opt** out);
void mjs_critic_opt_destroy(mjs_critic_opt* opt);
/* Bytes of partial slabs a batch of B rows uses: splits(B) * n_critics * slab bytes, with tiles = ceil(B / 16), splits_max = min(128,
 * max(1, 128 MiB / (n_critics * slab bytes))), tiles_per_split = ceil(tiles / splits_max), splits = ceil(tiles / tiles_per_split):
 * a function of B and the shape alone. 0 for a null critic or B <= 0. */
uint64_t mjs_critic_train_workspace_bytes(const mjs_critic* critic, int32_t B);
typedef struct {
  uint32_t struct_size;                  /* sizeof(mjs_critic_grad_args) */
  int32_t B;                             /* batch rows: >= 0 */
  const float* obs_dev;                  /* [B, obs_dim], required */
  const float* actions_dev;              /* [B, action_dim], required */
  const float* target_dev;               /* [B], required: y */
  float* q_out_dev;                      /* [n_critics, B] or NULL: Q_c(obs, actions), mjs_critic_q's values bit for bit */
  float* loss_out_dev;                   /* [n_critics] or NULL: mean((Q_c - y)^2) */
  const mjs_critic_weights* grads_out;   /* HOST struct of DEVICE pointers the gradients are WRITTEN to, torch.nn.Linear layout, or NULL
                                          * (mjs_critic_grad only; every layer of every critic < n_critics must be given) */
} mjs_critic_grad_args;                  /* 56 bytes */
/* The gradient of critic_loss with respect to every weight and bias, and no update: t and the parameters stay. One launch, and two small
 * ones per layer where grads_out is given. MJS_ERR_INVALID_ARG (nothing launched, text in mjs_last_error(NULL)) for a null argument or
 * required pointer, a wrong struct_size, B < 0, a critic that was never loaded, or an optimiser of another critic. B == 0 does nothing. */
int mjs_critic_grad(const mjs_critic* critic, mjs_critic_opt* opt, const mjs_critic_grad_args* args, void* stream);
/* One gradient step of the optimiser's critic: the gradient launch, then Adam over the packed copy (two launches), t += 1. lr >= 0 is
 * given per call (SB3 evaluates its schedule per train()). With g the gradient, in float32, one rounding per operation:
 *   m = m + (1 - beta1) * (g - m);  v = beta2 * v + (1 - beta2) * (g * g);  p = p - step_size * (m / (sqrtf(v) / sqrt_bc2 + eps))
 * with (1 - beta1), beta2, (1 - beta2), sqrt_bc2 = sqrt(1 - beta2^t), eps and step_size = lr / (1 - beta1^t) computed in double on the
 * host from the new t and rounded to float32 once each. Nothing is read back. Refusals as mjs_critic_grad's, and lr < 0 or a non-NULL
 * grads_out. B == 0 does nothing (t stays). */
int mjs_critic_update(mjs_critic_opt* opt, const mjs_critic_grad_args* args, double lr, void* stream);
/* dst = (1 - tau) * dst + tau * src between the packed copies of two critics (polyak_update without torch modules), one launch, as
 * fmaf(tau, src, (1 - tau) * dst) with both coefficients rounded to float32 on the host; tau == 1 copies and does not read dst.
 * MJS_ERR_INVALID_ARG for a null critic, critics of different shapes or devices, a src that was never loaded, tau outside (0, 1], or
 * tau != 1 into a dst that was never loaded. */
int mjs_critic_blend(mjs_critic* dst_critic, const mjs_critic* src_critic, double tau, void* stream);
/* The packed copy back into torch.nn.Linear layout: weights_out holds DEVICE pointers that are WRITTEN (every layer of every critic <
 * n_critics). One small launch per layer. MJS_ERR_INVALID_ARG for a null pointer, a wrong struct_size or a critic never loaded. */
int mjs_critic_export(const mjs_critic* critic, const mjs_critic_weights* weights_out, void* stream);

/* The encoder's backward pass, Adam step, blend and export on the device (csrc/mjs_encoder_train.h; entry points added after abi 3 as
 * well). From frames rgb [n, H, W, 3] and an upstream gradient dfeatures [n, F] (float32, read as it is: the 1/B of a mean loss is the
 * caller's business, as with autograd), the gradient of sum(features * dfeatures) with respect to the eight parameter tensors of the
 * NatureCNN that mjs_encoder_features evaluates - torch's features.backward(dfeatures). float32 with float32 accumulation; ReLU's
 * derivative is 1 where the stored activation is > 0 and 0 otherwise; no gradient with respect to the image. The encoder's PACKED copy
 * becomes the master copy of the parameters: mjs_encoder_features and the visual rollout see every step at once, a target encoder blends
 * from it (mjs_encoder_blend), mjs_encoder_export writes torch tensors, and mjs_encoder_load would overwrite the trained parameters.
 *
 * The sums over the batch are bitwise reproducible (no atomics): split s owns the contiguous images [s * images_per_split,
 * (s + 1) * images_per_split) and stores one partial slab; the slabs are summed in order. With
 *   slab = 192*32 + 32 + 512*64 + 64 + 576*64 + 64 + n_flatten*Fp + Fp + 4 floats  (Fp = F rounded up to 32),
 *   splits_max = min(64, max(1, 128 MiB / (4 * slab))),  images_per_split = ceil(n / splits_max),  splits = ceil(n / images_per_split),
 * a function of n and the shape alone.
 *
 * The workspace, float32, in this order (P1, P2, P3 = output positions H1*W1, H2*W2, H3*W3 of the three convolutions; every block
 * starts on a multiple of 4 floats):
 *   conv1 [n, P1, 32] | conv2 [n, P2, 64] | flat [n, n_flatten]            the post-ReLU activations (flat in CHW order)
 *   features [n, F] (n*F rounded up to 4) | Gf [n, Fp]                     Gf = dfeatures where features > 0, else 0
 *   dZ3 [n, P3, 64] | dZ2 [n, P2, 64] | dZ1 [n, P1, 32]                    gradients at the convolutions' pre-activations
 *   slabs [splits][slab]
 * so mjs_encoder_train_workspace_bytes = 4 * (2*n*P1*32 + 2*n*P2*64 + 2*n*n_flatten + roundup4(n*F) + n*Fp + splits*slab). */
typedef struct mjs_encoder_opt mjs_encoder_opt;
typedef struct {
  uint32_t struct_size;      /* sizeof(mjs_encoder_opt_desc) */
  int32_t reserved0;         /* 0 */
  double lr;                 /* >= 0; kept for reference, mjs_encoder_update takes lr per call */
  double beta1;              /* [0, 1) */
  double beta2;              /* [0, 1) */
  double eps;                /* > 0 */
} mjs_encoder_opt_desc;      /* 40 bytes */
/* An optimiser is bound to ONE loaded encoder, which must outlive it. It owns zeroed first and second moments and the step count t = 0.
 * MJS_ERR_INVALID_ARG for a null pointer, a wrong struct_size, an encoder that was never loaded, lr < 0, a beta outside [0, 1) or eps <= 0. */
int mjs_encoder_opt_create(mjs_encoder* enc, const mjs_encoder_opt_desc* desc, mjs_encoder_opt** out);
void mjs_encoder_opt_destroy(mjs_encoder_opt* opt);
/* Bytes of the workspace above for n images; 0 for a null encoder or n <= 0. */
uint64_t mjs_encoder_train_workspace_bytes(const mjs_encoder* enc, int32_t n);
typedef struct {
  uint32_t struct_size;                  /* sizeof(mjs_encoder_grad_args) */
  int32_t n;                             /* images: >= 0 */
  const uint8_t* rgb_dev;                /* [n, height, width, 3], required */
  const float* dfeatures_dev;            /* [n, F], required */
  void* workspace_dev;                   /* mjs_encoder_train_workspace_bytes(enc, n) bytes, 16-byte aligned, overwritten; required */
  float* features_out_dev;               /* [n, F] or NULL: mjs_encoder_features' values bit for bit */
  const mjs_encoder_weights* grads_out;  /* HOST struct of DEVICE pointers the gradients are WRITTEN to, torch layout, or NULL
                                          * (mjs_encoder_grad only; all eight must be given) */
  float* activations_out_dev[3];         /* each NULL or WRITTEN: conv1 [n, P1, 32], conv2 [n, P2, 64], flat [n, n_flatten], post-ReLU */
} mjs_encoder_grad_args;                 /* 72 bytes */
/* The forward (which keeps the activations) and the backward, and no update: t and the parameters stay. Eight launches, five small ones
 * more where grads_out is given, one device-to-device copy per optional output. MJS_ERR_INVALID_ARG (nothing launched, text in
 * mjs_last_error(NULL)) for a null argument or required pointer, a wrong struct_size, n < 0, an encoder that was never loaded or an
 * optimiser of another encoder. n == 0 does nothing and returns 0. Nothing is read back, nothing synchronises. */
int mjs_encoder_grad(const mjs_encoder* enc, mjs_encoder_opt* opt, const mjs_encoder_grad_args* args, void* stream);
/* One gradient step of the optimiser's encoder: mjs_encoder_grad's launches, then Adam over the packed copy by the lines and the
 * coefficient rule of mjs_critic_update (one launch), t += 1. The padding of the packed copy has zero gradient and stays zero. Refusals
 * as mjs_encoder_grad's, and lr < 0 or a non-NULL grads_out. n == 0 does nothing (t stays). */
int mjs_encoder_update(mjs_encoder_opt* opt, const mjs_encoder_grad_args* args, double lr, void* stream);
/* dst = (1 - tau) * dst + tau * src between the packed copies of two encoders (polyak_update for a target critic's own extractor), one
 * launch, mjs_critic_blend's formula and rounding; tau == 1 copies and does not read dst. MJS_ERR_INVALID_ARG for a null encoder,
 * encoders of different shapes or devices, a src that was never loaded, tau outside (0, 1], or tau != 1 into a dst never loaded. */
int mjs_encoder_blend(mjs_encoder* dst_enc, const mjs_encoder* src_enc, double tau, void* stream);
/* The packed copy back into torch layout (Conv2d [out, in, kh, kw], Linear [F, n_flatten]): weights_out holds DEVICE pointers that are
 * WRITTEN. Four small launches. MJS_ERR_INVALID_ARG for a null pointer, a wrong struct_size or an encoder never loaded. */
int mjs_encoder_export(const mjs_encoder* enc, const mjs_encoder_weights* weights_out, void* stream);

/* The actor and entropy-coefficient update of SAC.train on the device (csrc/mjs_actor_train.h; entry points added after abi 3 as well):
 *   a, logp = actor.action_log_prob(obs)  on the caller's draws z, as mjs_sac_td_target computes a' and logp
 *   actor_loss = mean(ent_coef * logp - min_c Q_c(obs, a));  zero_grad, backward, torch.optim.Adam.step on the ACTOR alone
 *   ent_coef_loss = -mean(log_ent_coef * (logp + target_entropy));  Adam on log_ent_coef;  ent_coef = expf(log_ent_coef)   (optional)
 * on the actor's PACKED copy, which becomes the master copy of the parameters: mjs_actor_actions, mjs_rollout_actor and
 * mjs_sac_td_target see every step at once, and mjs_actor_export writes torch.nn.Linear tensors when somebody wants them. Both losses
 * use the ent_coef from BEFORE this call's entropy step. The critics are read, never written; their parameter gradients are not computed.
 * float32 with float32 accumulation; the sum over the batch is bitwise reproducible, by the scheme of mjs_critic_update. */
typedef struct mjs_actor_opt mjs_actor_opt;
typedef struct {
  uint32_t struct_size;      /* sizeof(mjs_actor_opt_desc) */
  int32_t reserved0;         /* 0 */
  double lr;                 /* >= 0; kept for reference, mjs_actor_update takes lr per call */
  double beta1;              /* [0, 1) */
  double beta2;              /* [0, 1) */
  double eps;                /* > 0 */
} mjs_actor_opt_desc;        /* 40 bytes */
/* An optimiser is bound to ONE loaded actor of mjs_actor_create, which must outlive it. It owns zeroed first and second moments, the slab
 * workspace (the largest mjs_actor_train_workspace_bytes of any B) and the step count t = 0. MJS_ERR_INVALID_ARG for a null pointer, a
 * wrong struct_size, an actor that was never loaded or reads feature blocks, lr < 0, a beta outside [0, 1) or eps <= 0. */
int mjs_actor_opt_create(mjs_actor* actor, const mjs_actor_opt_desc* desc, mjs_actor_opt** out);
void mjs_actor_opt_destroy(mjs_actor_opt* opt);
/* Bytes of partial slabs a batch of B rows uses: mjs_critic_train_workspace_bytes' rule with n_critics = 1 over the actor's slab (every
 * layer's packed weights and bias, the stacked head last, and 4 floats). 0 for a null or visual actor or B <= 0. */
uint64_t mjs_actor_train_workspace_bytes(const mjs_actor* actor, int32_t B);
/* SB3's learned entropy coefficient (ent_coef = "auto"): four DEVICE floats of the caller's and the HOST values of one Adam step. */
typedef struct {
  uint32_t struct_size;        /* sizeof(mjs_entropy_step) */
  int32_t reserved0;           /* 0 */
  float* log_ent_coef_dev;     /* one float, required: updated */
  float* ent_coef_dev;         /* one float, required: WRITTEN expf(log_ent_coef) after the step */
  float* m_dev;                /* one float, required: Adam's first moment */
  float* v_dev;                /* one float, required: Adam's second moment */
  int64_t t;                   /* >= 1: the scalar's step count AFTER this step */
  double lr;                   /* >= 0 */
  double beta1;                /* [0, 1) */
  double beta2;                /* [0, 1) */
  double eps;                  /* > 0 */
  double target_entropy;       /* rounded to float32 */
} mjs_entropy_step;            /* 88 bytes */
typedef struct {
  uint32_t struct_size;                  /* sizeof(mjs_actor_grad_args) */
  int32_t B;                             /* batch rows: >= 0 */
  const float* obs_dev;                  /* [B, obs_dim], required: the actor's input columns in order (its obs_index plays no role) */
  const float* z_dev;                    /* [B, action_dim], required: standard-normal draws */
  const mjs_critic* critic;              /* required: loaded, on the actor's device, obs_dim == in_dim, the same action_dim */
  double ent_coef;                       /* rounded to float32; ignored where ent_coef_dev is given */
  const float* ent_coef_dev;             /* one float32 on the device, read by the gradient launch, or NULL */
  float* actions_out_dev;                /* [B, action_dim] or NULL: a */
  float* log_prob_out_dev;               /* [B] or NULL: logp */
  float* q_pi_out_dev;                   /* [n_critics, B] or NULL: Q_c(obs, a), mjs_critic_q's values bit for bit */
  float* min_q_action_grad_out_dev;      /* [B, action_dim] or NULL: d(min_c Q_c)/da */
  float* loss_out_dev;                   /* [1] or NULL: actor_loss */
  const mjs_actor_weights* grads_out;    /* HOST struct of DEVICE pointers the gradients are WRITTEN to, torch.nn.Linear layout, or NULL
                                          * (mjs_actor_grad only; every layer must be given) */
  const mjs_entropy_step* entropy;       /* NULL, or the entropy step mjs_actor_update takes after the actor's (mjs_actor_grad checks it
                                          * and uses its target_entropy only) */
} mjs_actor_grad_args;                   /* 104 bytes */
/* The gradient of actor_loss with respect to every weight and bias of the actor, and no update: t, the parameters and the entropy
 * scalars stay. One launch, and two small ones per layer where grads_out is given. MJS_ERR_INVALID_ARG (nothing launched, text in
 * mjs_last_error(NULL)) for a null argument or required pointer, a wrong struct_size, B < 0, an actor or critic that was never loaded,
 * an actor of mjs_actor_create_visual, actor and critic of different devices, an actor whose in_dim or action_dim is not the critic's
 * obs_dim or action_dim, an optimiser of another actor, or an entropy block with a null pointer, lr < 0, t < 1, a beta outside [0, 1)
 * or eps <= 0. B == 0 does nothing. */
int mjs_actor_grad(const mjs_actor* actor, mjs_actor_opt* opt, const mjs_actor_grad_args* args, void* stream);
/* One gradient step of the optimiser's actor: the gradient launch, then Adam over the packed copy by the lines and the coefficient rule
 * of mjs_critic_update (two launches), t += 1; with an entropy block a third, one-thread launch:
 *   g = -(sum of (logp + target_entropy) in row order) * (1 / B);  the same Adam lines on log_ent_coef;  ent_coef = expf(log_ent_coef)
 * with the block's own t, lr, betas and eps. The gradient launch has read ent_coef before that write, in stream order. Nothing is read
 * back. Refusals as mjs_actor_grad's, and lr < 0 or a non-NULL grads_out. B == 0 does nothing (t stays). */
int mjs_actor_update(mjs_actor_opt* opt, const mjs_actor_grad_args* args, double lr, void* stream);
/* The packed copy back into torch.nn.Linear layout, the head unstacked into mu and log_std: weights_out holds DEVICE pointers that are
 * WRITTEN (every layer). One small launch per layer and two for the head. MJS_ERR_INVALID_ARG for a null pointer, a wrong struct_size, a
 * visual actor or an actor never loaded. */
int mjs_actor_export(const mjs_actor* actor, const mjs_actor_weights* weights_out, void* stream);

/* SAC's gradient loop on the device (csrc/mjs_sac_train.h; entry points added after abi 3 as well): the batch and both action samples'
 * draws of one gradient step from ONE launch, and G whole gradient steps of SAC.train from one call. The generator is counter based:
 * Philox4x32-10 with key (seed & 0xffffffff, seed >> 32) and counter (b, block, step & 0xffffffff, step >> 32) for batch row b and
 * gradient-step counter step. Block 0's words w0, w1 give draw = (((uint64) w0 << 32) | w1) >> 2, the int64 below 2^62 that
 * mjs_replay_sample takes, and the ring row draw % min(count, capacity); blocks 1, 2 give z_next[b, 0..3] and [b, 4..7], blocks 3, 4
 * z_pi likewise, by Box-Muller in float32 over the word pairs (w0, w1) and (w2, w3):
 *   u1 = ((w >> 8) + 1) * 2^-24;  u2 = (w' >> 8) * 2^-24;  r = sqrtf(-2 * logf(u1));  pair = (r * cosf(2 pi u2), r * sinf(2 pi u2))
 * Only components below action_dim are written. Nothing is read back and no other generator is involved: a (seed, step) pair names
 * its batch. */
typedef struct {
  uint32_t struct_size;      /* sizeof(mjs_sac_batch) */
  int32_t reserved0;         /* 0 */
  int64_t* idx_out;          /* [B], required: the ring rows gathered, -1 while the buffer is empty (every gathered row is zero then) */
  int64_t* draws_out;        /* [B] or NULL: the raw draws; mjs_replay_sample on them gathers the same rows */
  float* obs;                /* [B, D], required where D > 0, like next_obs */
  float* next_obs;           /* [B, D] */
  float* actions;            /* [B, action_dim], required */
  float* rewards;            /* [B], required */
  float* dones;              /* [B], required */
  float* z_next;             /* [B, action_dim], required: the draws of the target's action sample */
  float* z_pi;               /* [B, action_dim], required: the draws of the actor loss's action sample */
} mjs_sac_batch;             /* 80 bytes */
/* One launch on the caller's stream. MJS_ERR_INVALID_ARG (nothing launched, text in mjs_last_error(NULL)) for a null argument or
 * required pointer, a wrong struct_size, a storage mjs_replay_sample would refuse, a storage with cameras (the SAC update is state-only)
 * or B < 0; B == 0 does nothing and returns 0. */
int mjs_sac_draw_batch(const mjs_replay_storage* storage, const mjs_sac_batch* out, int32_t B, uint64_t seed, uint64_t step, void* stream);
typedef struct {
  uint32_t struct_size;                  /* sizeof(mjs_sac_train_args) */
  int32_t B;                             /* batch rows: >= 1 */
  int32_t G;                             /* gradient steps: >= 0 */
  int32_t target_update_interval;        /* >= 1 */
  const mjs_replay_storage* storage;     /* required: no cameras, obs_dim and action_dim the networks' */
  mjs_actor* actor;                      /* required: loaded, of mjs_actor_create */
  mjs_critic* critic;                    /* required: the online critic */
  mjs_critic* target_critic;             /* required: another object of the same shape */
  mjs_critic_opt* critic_opt;            /* required: created for critic */
  mjs_actor_opt* actor_opt;              /* required: created for actor */
  const mjs_sac_batch* batch;            /* required: the caller's scratch for B rows, overwritten by every step; draws_out may be NULL */
  float* target_dev;                     /* [B], required: scratch for the TD target */
  uint64_t seed;                         /* the generator's key */
  uint64_t step0;                        /* the gradient-step counter of the first step; step g uses step0 + g */
  double gamma;                          /* [0, 1] */
  double tau;                            /* (0, 1] */
  double critic_lr;                      /* >= 0 */
  double actor_lr;                       /* >= 0 */
  double ent_coef;                       /* the fixed coefficient; ignored where ent_coef_dev is given */
  const float* ent_coef_dev;             /* one float32 on the device or NULL; with an entropy block, its ent_coef_dev */
  const mjs_entropy_step* entropy;       /* NULL, or the learned coefficient's step; t is the count after the FIRST step, step g uses t + g */
} mjs_sac_train_args;                    /* 152 bytes */
/* G gradient steps with no return to the caller, as plain launches on the caller's stream (eight per step with a learned coefficient and a
 * blending target: 1 + 1 + 2 + 3 + 1; no graph capture): for g = 0..G-1, through the entry points above and their unchanged kernels,
 *   1. mjs_sac_draw_batch(seed, step0 + g) into batch
 *   2. mjs_sac_td_target on target_critic with the coefficient from before the step, into target_dev
 *   3. mjs_critic_update(critic_opt, critic_lr)
 *   4. mjs_actor_update(actor_opt, actor_lr), with an entropy block the coefficient's step as well
 *   5. mjs_critic_blend(target_critic, critic, tau) where (step0 + g + 1) % target_update_interval == 0
 * Both optimisers' step counts advance by G. MJS_ERR_INVALID_ARG (nothing launched, text in mjs_last_error(NULL)) for a null argument
 * or required pointer, a wrong struct_size, B < 1, G < 0, target_update_interval < 1, cameras in the storage, a storage whose obs_dim or
 * action_dim is not the networks', objects on different devices, an optimiser of another network, target_critic == critic, tau outside
 * (0, 1], gamma outside [0, 1], a negative lr, and anything one of the five entry points refuses: all of it is checked before the first
 * launch. G == 0 does nothing and returns 0. */
int mjs_sac_train(const mjs_sac_train_args* args, void* stream);

/* Episode statistics on the device (csrc/mjs_monitor.h; entry points added after abi 3 as well): the [T, N] blocks the rollouts above
 * write, reduced to finished episodes. A restatement of SB3's Monitor + ep_info_buffer (stable_baselines3/common/monitor.py, a
 * deque(maxlen=100); scripts/sb3/reach_sac.py:83) and of evaluate_policy's per-env episode targets. The entry points are stateless: the
 * state is a descriptor of caller-owned device memory.
 *
 * Row (t, n) of a block counts iff step_type[t, n] != MJS_STEP_FIRST under MJS_AUTORESET_NEXT_STEP and always under
 * MJS_AUTORESET_SAME_STEP (mjs_replay_add's rule for a transition). A counting row does ep_return[n] += reward[t, n] in float64, one add
 * per row in t order, and ep_length[n] += 1. Where terminated | truncated on a counting row the episode ends: if quota == NULL or
 * ep_count[n] < quota[n] it is RECORDED (return, length, success = is_success[t, n], terminated = terminated[t, n], env = n) and
 * ep_count[n] += 1; in every case both accumulators return to 0. The recorded episodes of a block are ordered by (t, n); the e-th goes
 * to ring slot (count + e) % window, count = *cursor_dev = the number of episodes ever recorded, and afterwards count += E. Of a block
 * with E > window episodes only the last `window` are written. A negative quota entry cannot be checked without reading the device: its
 * effect is undefined. Returns are kept in full float64 (Monitor rounds them to 6 digits; this does not). Neither entry point reads
 * anything back to the host or synchronises, and two runs from equal state give equal bits. */
typedef struct {
  uint32_t struct_size;      /* sizeof(mjs_monitor_state), validated like mjs_config's */
  int32_t device;            /* HIP device ordinal */
  int32_t num_envs;          /* N >= 1 */
  int32_t window;            /* W, ring slots: >= 1 */
  double* ep_return;         /* [N]: the running episode's return */
  int32_t* ep_length;        /* [N]: the running episode's counting rows */
  int64_t* ep_count;         /* [N]: episodes recorded for the env */
  const int64_t* quota;      /* [N] non-negative, or NULL (unlimited): episodes of an env beyond it are not recorded */
  uint64_t* cursor_dev;      /* one uint64: episodes ever recorded */
  double* ring_return;       /* [W] */
  int32_t* ring_length;      /* [W] */
  uint8_t* ring_success;     /* [W] */
  uint8_t* ring_terminated;  /* [W]: 1 = terminated, 0 = truncated */
  int32_t* ring_env;         /* [W] */
} mjs_monitor_state;         /* 96 bytes */
typedef struct {
  uint32_t struct_size;        /* sizeof(mjs_monitor_block) */
  int32_t T;                   /* control steps of the block: >= 0 */
  int32_t N;                   /* envs of the block: the state's num_envs */
  int32_t autoreset;           /* MJS_AUTORESET_NEXT_STEP or MJS_AUTORESET_SAME_STEP, the mode the block was made under */
  const double* reward;        /* [T, N] */
  const uint8_t* terminated;   /* [T, N] */
  const uint8_t* truncated;    /* [T, N] */
  const uint8_t* is_success;   /* [T, N] */
  const uint8_t* step_type;    /* [T, N]: required under next-step auto-reset, ignored otherwise */
} mjs_monitor_block;           /* 56 bytes */
/* what mjs_monitor_summary writes: MJS_MONITOR_SUMMARY float64 values over the K = min(count, window) live records. With K == 0 the
 * count and the three sums are 0 and every other value NaN (SB3's safe_mean of an empty buffer). */
enum {
  MJS_MONITOR_COUNT = 0,          /* K */
  MJS_MONITOR_RETURN_MEAN = 1,    /* RETURN_SUM / K, one rounding */
  MJS_MONITOR_RETURN_STD = 2,     /* sqrt(sum((x - mean)^2) / K): the population value, numpy.std's definition */
  MJS_MONITOR_LENGTH_MEAN = 3,    /* LENGTH_SUM / K */
  MJS_MONITOR_SUCCESS_RATE = 4,   /* SUCCESS_COUNT / K */
  MJS_MONITOR_RETURN_MIN = 5,
  MJS_MONITOR_RETURN_MAX = 6,
  MJS_MONITOR_RETURN_SUM = 7,     /* float64 adds in a fixed order (csrc/mjs_monitor.h) */
  MJS_MONITOR_LENGTH_SUM = 8,     /* exact (an int64 sum) */
  MJS_MONITOR_SUCCESS_COUNT = 9,  /* exact */
  MJS_MONITOR_SUMMARY = 10
};
/* bytes of the workspace mjs_monitor_update needs for a block of T x N rows (chunk counts and every row's end record); 0 for a bad
 * argument */
uint64_t mjs_monitor_workspace_bytes(int32_t T, int32_t N);
/* Advances the state over a block: FOUR launches on the caller's stream (walk, count, scan, scatter). workspace_dev:
 * mjs_monitor_workspace_bytes(T, N) bytes, 16-byte aligned, overwritten. MJS_ERR_INVALID_ARG (nothing launched, text in
 * mjs_last_error(NULL)) for a null argument or required pointer (every pointer of the state but quota; reward, terminated, truncated and
 * is_success of the block), a wrong struct_size, num_envs < 1, window < 1, a block whose N is not the state's num_envs, T < 0, T * N >=
 * 2^31, MJS_AUTORESET_DISABLED (or no mode at all), or next-step auto-reset without step_type. T == 0 does nothing and returns 0. */
int mjs_monitor_update(const mjs_monitor_state* state, const mjs_monitor_block* block, void* workspace_dev, void* stream);
/* The ring's live records reduced into out_dev, float64 [MJS_MONITOR_SUMMARY] on the device: ONE launch of one workgroup, sums in a
 * fixed order. MJS_ERR_INVALID_ARG (nothing launched) for a null argument or a state mjs_monitor_update would refuse. */
int mjs_monitor_summary(const mjs_monitor_state* state, double* out_dev, void* stream);

/* Replaces the Robot entity's control API on a stand-alone UR5e (entities/robots/robot.py:198-272): Robot.moveJ :211-216,
 * Robot.movej_IK :198-209, Robot.servoL :218-225, Robot.servoJ :227-259, then n_substeps x (Robot.before_substep :261-272 +
 * JointTrajectory.get_target_joint_positions joint_trajectory.py:41-47; Physics.step), then Robot.get_tcp_pose :153-168.
 * This is the component the reference's own tests drive (test/test_ur_control_api.py:7-82: UR5e() + raw mjcf.Physics at
 * the XML's timestep); n independent robots, one lane each.
 *   state_dev   float64 [n, MJS_UR_STATE], in/out: q[6], v[6], ctrl[6], time, trajectory active, q0[6], q1[6], t0, t1
 *   target_dev  float64 [n, 7]: 6 joint angles (MOVEJ / SERVOJ) or a TCP pose xyz + scalar-LAST quaternion
 *               (MOVEJ_IK / SERVOL, type_aliases.py:6-10); unused for MJS_UR_CMD_NONE
 *   param       speed [rad/s] for MOVEJ / MOVEJ_IK, duration [s] for SERVOL / SERVOJ
 *   eef         MJS_UR_EEF_NONE (bare flange, TCP = flange) or MJS_UR_EEF_GRIPPER (lumped 2F-85, TCP offset 0.174)
 *   dt          physics timestep (the menagerie XML sets none: MuJoCo's default 0.002)
 *   tcp_pose_out_dev float64 [n, 7] or NULL; status_dev uint8 [n] or NULL: bit 0 = the command's IK found a solution
 *               (movej_IK prints and returns, servoL raises), bit 1 = a joint left its range (limit rows are not modelled by
 *               this entry point), bit 2 = non-finite acceleration. No handle; device = current HIP device. */
#define MJS_UR_STATE 34
enum { MJS_UR_CMD_NONE = 0, MJS_UR_CMD_MOVEJ = 1, MJS_UR_CMD_MOVEJ_IK = 2, MJS_UR_CMD_SERVOL = 3, MJS_UR_CMD_SERVOJ = 4 };
enum { MJS_UR_EEF_NONE = 0, MJS_UR_EEF_GRIPPER = 1 };
int mjs_ur5e_robot_run(double* state_dev, const double* target_dev, int32_t command, double param, int32_t n_substeps, int32_t eef, double dt,
                       double* tcp_pose_out_dev, uint8_t* status_dev, int32_t n, void* stream);

/* checkpoint / resume of the physics+task state: float64 [state_dim, N] ... */
int mjs_get_state(mjs_handle* h, double* state_dev, void* stream);
int mjs_set_state(mjs_handle* h, const double* state_dev, void* stream);
/* ... and of the per-env MT19937 streams: mt_dev uint32 [624, N], pos_dev int32 [N]
 * (what pickling env._random_state would capture in the reference, dmc2gym.py:129) */
int mjs_get_rng_state(mjs_handle* h, uint32_t* mt_dev, int32_t* pos_dev, void* stream);
int mjs_set_rng_state(mjs_handle* h, const uint32_t* mt_dev, const int32_t* pos_dev, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* MJSIM_H */
