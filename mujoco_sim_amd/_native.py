"""ctypes binding of libmjsim.so (C ABI in include/mjsim.h) and its in-tree hipcc build.

There is NO CPU fallback: if the shared library is missing or no HIP device is visible the
product path raises. The oracle under ``oracle/`` is test infrastructure and is never imported
from here.
"""
from __future__ import annotations

import ctypes as C
import hashlib
import os
import re
import subprocess
from pathlib import Path

_PKG = Path(__file__).resolve().parent
_ROOT = _PKG.parent
LIB_PATH = Path(os.environ["MJS_LIB"]) if os.environ.get("MJS_LIB") else _PKG / "lib" / "libmjsim.so"  # MJS_LIB: diagnostic builds


def _sources() -> list[Path]:
    """Every file the library is compiled from: csrc/*.{h,hip} and include/*.h."""
    return [*sorted(p for p in (_PKG / "csrc").glob("*") if p.suffix in (".h", ".hip")), *sorted((_ROOT / "include").glob("*.h"))]


TASK_POINTMASS_REACH, TASK_ROBOT_REACH, TASK_PLANAR_PUSH, TASK_BUTTON_PUSH = 0, 1, 2, 3
ACTION_ABS_JOINT, ACTION_ABS_EEF = 0, 1
REW_SPARSE, REW_DENSE_POTENTIAL, REW_DENSE_NEG_DISTANCE, REW_DENSE_BIASED_NEG_DISTANCE = 0, 1, 2, 3
STEP_FIRST, STEP_MID, STEP_LAST = 0, 1, 2
AUTORESET_NEXT_STEP, AUTORESET_SAME_STEP, AUTORESET_DISABLED = 0, 1, 2
FAULT_BAD_STATE, FAULT_IK_FAILED, FAULT_LIMIT_COLDSTART, FAULT_UNSUPPORTED_CONTACT, FAULT_FASTPATH_VIOLATED = 1, 2, 4, 8, 16
BLOCKS_MESH, BLOCKS_BOX = 0, 1
GRIPPER_REDUCED, GRIPPER_ARTICULATED = 0, 1
VARIANT_DEFAULT, VARIANT_SINGLE_WAVE, VARIANT_TWO_ROLES, VARIANT_RESET_GROUPS = 0, 1, 2, 3
UR_STATE = 34
UR_CMD_NONE, UR_CMD_MOVEJ, UR_CMD_MOVEJ_IK, UR_CMD_SERVOL, UR_CMD_SERVOJ = 0, 1, 2, 3, 4
UR_EEF_NONE, UR_EEF_GRIPPER = 0, 1
ACTIVATION_RELU, ACTIVATION_TANH = 0, 1
ACTOR_VARIANT_DEFAULT, ACTOR_VARIANT_TILE32 = 0, 1
ACTOR_MAX_IN, ACTOR_MAX_HIDDEN, ACTOR_MAX_LAYERS, ACTOR_MAX_ACTIONS = 64, 256, 3, 8  # the limits mjs_actor_create checks
ENCODER_MIN_SIZE, ENCODER_MAX_SIZE, ENCODER_MAX_FEATURES, ACTOR_MAX_BLOCKS = 36, 96, 512, 2  # the limits mjs_encoder_create / mjs_actor_create_visual check
REPLAY_MAX_OBS, REPLAY_MAX_CAMERAS = 64, 2  # the limits mjs_replay_add checks (with ACTOR_MAX_ACTIONS)
CRITIC_MAX_OBS, CRITIC_MAX_CRITICS = REPLAY_MAX_OBS, 2  # the limits mjs_critic_create checks (with ACTOR_MAX_HIDDEN / _LAYERS / _ACTIONS)

EXPORTED_SYMBOLS = [
    "mjs_version", "mjs_obs_dim", "mjs_action_dim", "mjs_action_dim_for", "mjs_state_dim", "mjs_env_obs_dim", "mjs_env_state_dim", "mjs_algorithmic_bytes_per_env_step", "mjs_env_algorithmic_bytes_per_env_step", "mjs_substeps",
    "mjs_create", "mjs_destroy", "mjs_last_error", "mjs_seed", "mjs_reset", "mjs_step", "mjs_rollout",
    "mjs_get_state", "mjs_set_state", "mjs_get_rng_state", "mjs_set_rng_state", "mjs_render", "mjs_set_scene_camera", "mjs_get_scene_camera", "mjs_render_rgbd", "mjs_debug_ur5e_ik", "mjs_ur5e_tcp_to_joints", "mjs_ur5e_robot_run",
    "mjs_demonstration_actions", "mjs_rollout_demonstration",
    "mjs_actor_create", "mjs_actor_destroy", "mjs_actor_load", "mjs_actor_actions", "mjs_rollout_actor",
    "mjs_encoder_create", "mjs_encoder_destroy", "mjs_encoder_load", "mjs_encoder_flat_dim", "mjs_encoder_workspace_bytes", "mjs_encoder_features",
    "mjs_actor_create_visual", "mjs_actor_actions_visual", "mjs_rollout_visual_actor",
    "mjs_replay_workspace_bytes", "mjs_replay_add", "mjs_replay_sample",
    "mjs_critic_create", "mjs_critic_destroy", "mjs_critic_load", "mjs_critic_q", "mjs_sac_td_target",
    "mjs_critic_opt_create", "mjs_critic_opt_destroy", "mjs_critic_train_workspace_bytes", "mjs_critic_grad", "mjs_critic_update", "mjs_critic_blend",
    "mjs_critic_export",
    "mjs_actor_opt_create", "mjs_actor_opt_destroy", "mjs_actor_train_workspace_bytes", "mjs_actor_grad", "mjs_actor_update", "mjs_actor_export",
    "mjs_sac_draw_batch", "mjs_sac_train",
    "mjs_encoder_opt_create", "mjs_encoder_opt_destroy", "mjs_encoder_train_workspace_bytes", "mjs_encoder_grad", "mjs_encoder_update", "mjs_encoder_blend",
    "mjs_encoder_export",
    "mjs_monitor_workspace_bytes", "mjs_monitor_update", "mjs_monitor_summary",
]


class MjsConfig(C.Structure):
    _fields_ = [
        ("struct_size", C.c_uint32), ("task", C.c_int32), ("num_envs", C.c_int32), ("device", C.c_int32), ("reward_type", C.c_int32),
        ("autoreset", C.c_int32), ("terminate_on_success", C.c_int32), ("env_index_offset", C.c_int32),
        ("kernel_variant", C.c_int32), ("time_limit", C.c_double), ("action_type", C.c_int32), ("button_disturbances", C.c_int32), ("n_objects", C.c_int32), ("max_episode_steps", C.c_int32), ("block_shape", C.c_int32),
        ("gripper_model", C.c_int32), ("reserved0", C.c_int32),
    ]

    def __init__(self, *args, **kw):  # struct_size = sizeof(mjs_config) of THIS binding: mjs_create refuses a mismatch (abi 2+)
        super().__init__(*args, **kw)
        if "struct_size" not in kw:
            self.struct_size = C.sizeof(MjsConfig)


class MjsOutputs(C.Structure):
    _fields_ = [
        ("obs", C.c_void_p), ("terminal_obs", C.c_void_p), ("reward", C.c_void_p), ("discount", C.c_void_p),
        ("terminated", C.c_void_p), ("truncated", C.c_void_p), ("is_success", C.c_void_p), ("step_type", C.c_void_p),
        ("fault", C.c_void_p), ("ncon", C.c_void_p),
    ]


class MjsCameraPose(C.Structure):
    """mjs_camera_pose: the scene camera of a handle (world position, MuJoCo quaternion w,x,y,z, vertical field of view in degrees)."""
    _fields_ = [("struct_size", C.c_uint32), ("reserved0", C.c_int32), ("pos", C.c_double * 3), ("quat", C.c_double * 4), ("fovy", C.c_double)]

    def __init__(self, *args, **kw):
        super().__init__(*args, **kw)
        if "struct_size" not in kw:
            self.struct_size = C.sizeof(MjsCameraPose)


class MjsDemoRollout(C.Structure):
    """mjs_demo_rollout: what a closed-loop demonstration rollout writes besides MjsOutputs (actions, ik_ok, camera frames), and its noise."""
    _fields_ = [("struct_size", C.c_uint32), ("height", C.c_int32), ("width", C.c_int32), ("reserved0", C.c_int32), ("noise", C.c_double),
                ("noise_z_dev", C.c_void_p), ("actions_out_dev", C.c_void_p), ("ik_ok_dev", C.c_void_p), ("scene_rgb_dev", C.c_void_p),
                ("wrist_rgb_dev", C.c_void_p)]

    def __init__(self, *args, **kw):
        super().__init__(*args, **kw)
        if "struct_size" not in kw:
            self.struct_size = C.sizeof(MjsDemoRollout)


class _Sized(C.Structure):
    """A structure whose first field is the struct_size the library validates."""

    def __init__(self, *args, **kw):
        super().__init__(*args, **kw)
        if "struct_size" not in kw:
            self.struct_size = C.sizeof(type(self))


class MjsActorDesc(_Sized):
    """mjs_actor_desc: the shape of an MLP actor; obs_index is a HOST int32 array (the library copies it)."""
    _fields_ = [("struct_size", C.c_uint32), ("device", C.c_int32), ("in_dim", C.c_int32), ("n_hidden", C.c_int32), ("hidden", C.c_int32 * 3),
                ("action_dim", C.c_int32), ("activation", C.c_int32), ("variant", C.c_int32), ("obs_index", C.POINTER(C.c_int32))]


class MjsActorWeights(_Sized):
    """mjs_actor_weights: DEVICE pointers to float32 parameters in torch.nn.Linear layout."""
    _fields_ = [("struct_size", C.c_uint32), ("reserved0", C.c_int32), ("hidden_w", C.c_void_p * 3), ("hidden_b", C.c_void_p * 3),
                ("mu_w", C.c_void_p), ("mu_b", C.c_void_p), ("log_std_w", C.c_void_p), ("log_std_b", C.c_void_p)]


class MjsActorRollout(_Sized):
    """mjs_actor_rollout: what a closed-loop actor rollout writes besides MjsOutputs, its noise draws and the action bounds (HOST)."""
    _fields_ = [("struct_size", C.c_uint32), ("height", C.c_int32), ("width", C.c_int32), ("reserved0", C.c_int32), ("z_dev", C.c_void_p),
                ("low", C.POINTER(C.c_double)), ("high", C.POINTER(C.c_double)), ("actions_out_dev", C.c_void_p), ("squashed_out_dev", C.c_void_p),
                ("scene_rgb_dev", C.c_void_p), ("wrist_rgb_dev", C.c_void_p)]


class MjsEncoderDesc(_Sized):
    """mjs_encoder_desc: the image size and feature width of a NatureCNN encoder."""
    _fields_ = [("struct_size", C.c_uint32), ("device", C.c_int32), ("height", C.c_int32), ("width", C.c_int32), ("channels", C.c_int32),
                ("features_dim", C.c_int32)]


class MjsEncoderWeights(_Sized):
    """mjs_encoder_weights: DEVICE pointers to float32 parameters in torch layout (Conv2d [out, in, kh, kw], Linear [F, n_flatten])."""
    _fields_ = [("struct_size", C.c_uint32), ("reserved0", C.c_int32), ("conv1_w", C.c_void_p), ("conv1_b", C.c_void_p), ("conv2_w", C.c_void_p),
                ("conv2_b", C.c_void_p), ("conv3_w", C.c_void_p), ("conv3_b", C.c_void_p), ("fc_w", C.c_void_p), ("fc_b", C.c_void_p)]


class MjsActorFeatureInputs(_Sized):
    """mjs_actor_feature_inputs: the feature blocks of a visual actor (slot 0: scene camera, slot 1: wrist camera; width 0: absent)."""
    _fields_ = [("struct_size", C.c_uint32), ("n_blocks", C.c_int32), ("width", C.c_int32 * 2), ("start", C.c_int32 * 2)]


class MjsVisualRollout(_Sized):
    """mjs_visual_rollout: what a closed-loop visual-actor rollout writes besides MjsOutputs, its draws, bounds (HOST) and scratch."""
    _fields_ = [("struct_size", C.c_uint32), ("reserved0", C.c_int32), ("z_dev", C.c_void_p), ("low", C.POINTER(C.c_double)), ("high", C.POINTER(C.c_double)),
                ("actions_out_dev", C.c_void_p), ("squashed_out_dev", C.c_void_p), ("scene_rgb_dev", C.c_void_p), ("wrist_rgb_dev", C.c_void_p),
                ("scene_scratch_dev", C.c_void_p), ("wrist_scratch_dev", C.c_void_p), ("features_dev", C.c_void_p * 2), ("workspace_dev", C.c_void_p)]


class MjsReplayStorage(_Sized):
    """mjs_replay_storage: a replay ring as DEVICE pointers to caller-owned tensors, and its device cursor."""
    _fields_ = [("struct_size", C.c_uint32), ("device", C.c_int32), ("capacity", C.c_int32), ("obs_dim", C.c_int32), ("action_dim", C.c_int32),
                ("n_cameras", C.c_int32), ("height", C.c_int32), ("width", C.c_int32), ("cursor_dev", C.c_void_p), ("obs", C.c_void_p),
                ("next_obs", C.c_void_p), ("actions", C.c_void_p), ("rewards", C.c_void_p), ("dones", C.c_void_p), ("timeouts", C.c_void_p),
                ("rgb", C.c_void_p * 2), ("next_rgb", C.c_void_p * 2)]


class MjsReplayBlock(_Sized):
    """mjs_replay_block: a [T, N] rollout block as DEVICE pointers; obs_index is a HOST int32 array (copied during the call)."""
    _fields_ = [("struct_size", C.c_uint32), ("T", C.c_int32), ("N", C.c_int32), ("src_dim", C.c_int32), ("autoreset", C.c_int32), ("reserved0", C.c_int32),
                ("obs_index", C.POINTER(C.c_int32)), ("obs0", C.c_void_p), ("obs", C.c_void_p), ("terminal_obs", C.c_void_p), ("reward", C.c_void_p),
                ("terminated", C.c_void_p), ("truncated", C.c_void_p), ("step_type", C.c_void_p), ("squashed_actions", C.c_void_p),
                ("rgb", C.c_void_p * 2), ("final_rgb", C.c_void_p * 2)]


class MjsReplayBatch(_Sized):
    """mjs_replay_batch: where mjs_replay_sample writes; a NULL output is skipped."""
    _fields_ = [("struct_size", C.c_uint32), ("reserved0", C.c_int32), ("idx_out", C.c_void_p), ("obs", C.c_void_p), ("next_obs", C.c_void_p),
                ("actions", C.c_void_p), ("rewards", C.c_void_p), ("dones", C.c_void_p), ("timeouts", C.c_void_p), ("rgb", C.c_void_p * 2),
                ("next_rgb", C.c_void_p * 2)]


class MjsCriticDesc(_Sized):
    """mjs_critic_desc: the shape of SAC's critics (n_critics networks of one architecture over [obs | action])."""
    _fields_ = [("struct_size", C.c_uint32), ("device", C.c_int32), ("obs_dim", C.c_int32), ("action_dim", C.c_int32), ("n_critics", C.c_int32),
                ("n_hidden", C.c_int32), ("hidden", C.c_int32 * 3), ("activation", C.c_int32)]


class MjsCriticWeights(_Sized):
    """mjs_critic_weights: DEVICE pointers to float32 parameters in torch.nn.Linear layout, [critic][layer]."""
    _fields_ = [("struct_size", C.c_uint32), ("reserved0", C.c_int32), ("hidden_w", C.c_void_p * 3 * 2), ("hidden_b", C.c_void_p * 3 * 2),
                ("out_w", C.c_void_p * 2), ("out_b", C.c_void_p * 2)]


class MjsTdTargetArgs(_Sized):
    """mjs_td_target_args: a batch's DEVICE tensors, the discount and entropy coefficient, and where mjs_sac_td_target writes."""
    _fields_ = [("struct_size", C.c_uint32), ("B", C.c_int32), ("next_obs_dev", C.c_void_p), ("rewards_dev", C.c_void_p), ("dones_dev", C.c_void_p),
                ("z_dev", C.c_void_p), ("gamma", C.c_double), ("ent_coef", C.c_double), ("ent_coef_dev", C.c_void_p), ("target_out_dev", C.c_void_p),
                ("next_actions_out_dev", C.c_void_p), ("next_log_prob_out_dev", C.c_void_p), ("q_next_out_dev", C.c_void_p)]


class MjsCriticOptDesc(_Sized):
    """mjs_critic_opt_desc: Adam's settings for a critic's packed copy."""
    _fields_ = [("struct_size", C.c_uint32), ("reserved0", C.c_int32), ("lr", C.c_double), ("beta1", C.c_double), ("beta2", C.c_double), ("eps", C.c_double)]


class MjsCriticGradArgs(_Sized):
    """mjs_critic_grad_args: a batch's DEVICE tensors, the target, and where mjs_critic_grad / mjs_critic_update write."""
    _fields_ = [("struct_size", C.c_uint32), ("B", C.c_int32), ("obs_dev", C.c_void_p), ("actions_dev", C.c_void_p), ("target_dev", C.c_void_p),
                ("q_out_dev", C.c_void_p), ("loss_out_dev", C.c_void_p), ("grads_out", C.POINTER(MjsCriticWeights))]


class MjsActorOptDesc(_Sized):
    """mjs_actor_opt_desc: Adam's settings for an actor's packed copy."""
    _fields_ = [("struct_size", C.c_uint32), ("reserved0", C.c_int32), ("lr", C.c_double), ("beta1", C.c_double), ("beta2", C.c_double), ("eps", C.c_double)]


class MjsEncoderOptDesc(_Sized):
    """mjs_encoder_opt_desc: Adam's settings for an encoder's packed copy."""
    _fields_ = [("struct_size", C.c_uint32), ("reserved0", C.c_int32), ("lr", C.c_double), ("beta1", C.c_double), ("beta2", C.c_double), ("eps", C.c_double)]


class MjsEncoderGradArgs(_Sized):
    """mjs_encoder_grad_args: the frames, the upstream gradient, the workspace, and where mjs_encoder_grad / mjs_encoder_update write."""
    _fields_ = [("struct_size", C.c_uint32), ("n", C.c_int32), ("rgb_dev", C.c_void_p), ("dfeatures_dev", C.c_void_p), ("workspace_dev", C.c_void_p),
                ("features_out_dev", C.c_void_p), ("grads_out", C.POINTER(MjsEncoderWeights)), ("activations_out_dev", C.c_void_p * 3)]


class MjsEntropyStep(_Sized):
    """mjs_entropy_step: SB3's learned entropy coefficient as DEVICE scalars, and the HOST values of its Adam step."""
    _fields_ = [("struct_size", C.c_uint32), ("reserved0", C.c_int32), ("log_ent_coef_dev", C.c_void_p), ("ent_coef_dev", C.c_void_p), ("m_dev", C.c_void_p),
                ("v_dev", C.c_void_p), ("t", C.c_int64), ("lr", C.c_double), ("beta1", C.c_double), ("beta2", C.c_double), ("eps", C.c_double),
                ("target_entropy", C.c_double)]


class MjsActorGradArgs(_Sized):
    """mjs_actor_grad_args: a batch's DEVICE tensors, the critic, the entropy coefficient, and where mjs_actor_grad / mjs_actor_update write."""
    _fields_ = [("struct_size", C.c_uint32), ("B", C.c_int32), ("obs_dev", C.c_void_p), ("z_dev", C.c_void_p), ("critic", C.c_void_p),
                ("ent_coef", C.c_double), ("ent_coef_dev", C.c_void_p), ("actions_out_dev", C.c_void_p), ("log_prob_out_dev", C.c_void_p),
                ("q_pi_out_dev", C.c_void_p), ("min_q_action_grad_out_dev", C.c_void_p), ("loss_out_dev", C.c_void_p),
                ("grads_out", C.POINTER(MjsActorWeights)), ("entropy", C.POINTER(MjsEntropyStep))]


class MjsSacBatch(_Sized):
    """mjs_sac_batch: where mjs_sac_draw_batch writes a gradient step's batch and draws (caller-owned scratch); draws_out may be NULL."""
    _fields_ = [("struct_size", C.c_uint32), ("reserved0", C.c_int32), ("idx_out", C.c_void_p), ("draws_out", C.c_void_p), ("obs", C.c_void_p),
                ("next_obs", C.c_void_p), ("actions", C.c_void_p), ("rewards", C.c_void_p), ("dones", C.c_void_p), ("z_next", C.c_void_p),
                ("z_pi", C.c_void_p)]


class MjsSacTrainArgs(_Sized):
    """mjs_sac_train_args: the objects, scratch buffers and hyperparameters of G gradient steps in one native call."""
    _fields_ = [("struct_size", C.c_uint32), ("B", C.c_int32), ("G", C.c_int32), ("target_update_interval", C.c_int32),
                ("storage", C.POINTER(MjsReplayStorage)), ("actor", C.c_void_p), ("critic", C.c_void_p), ("target_critic", C.c_void_p),
                ("critic_opt", C.c_void_p), ("actor_opt", C.c_void_p), ("batch", C.POINTER(MjsSacBatch)), ("target_dev", C.c_void_p),
                ("seed", C.c_uint64), ("step0", C.c_uint64), ("gamma", C.c_double), ("tau", C.c_double), ("critic_lr", C.c_double),
                ("actor_lr", C.c_double), ("ent_coef", C.c_double), ("ent_coef_dev", C.c_void_p), ("entropy", C.POINTER(MjsEntropyStep))]


class MjsMonitorState(_Sized):
    """mjs_monitor_state: per-env episode accumulators, the optional quota, and the ring of finished episodes with its device cursor."""
    _fields_ = [("struct_size", C.c_uint32), ("device", C.c_int32), ("num_envs", C.c_int32), ("window", C.c_int32), ("ep_return", C.c_void_p),
                ("ep_length", C.c_void_p), ("ep_count", C.c_void_p), ("quota", C.c_void_p), ("cursor_dev", C.c_void_p), ("ring_return", C.c_void_p),
                ("ring_length", C.c_void_p), ("ring_success", C.c_void_p), ("ring_terminated", C.c_void_p), ("ring_env", C.c_void_p)]


class MjsMonitorBlock(_Sized):
    """mjs_monitor_block: the [T, N] fields of a rollout block the episode statistics read, as DEVICE pointers."""
    _fields_ = [("struct_size", C.c_uint32), ("T", C.c_int32), ("N", C.c_int32), ("autoreset", C.c_int32), ("reward", C.c_void_p),
                ("terminated", C.c_void_p), ("truncated", C.c_void_p), ("is_success", C.c_void_p), ("step_type", C.c_void_p)]


# the slots of mjs_monitor_summary's output (the MJS_MONITOR_* enum)
MONITOR_SUMMARY_FIELDS = ("count", "return_mean", "return_std", "length_mean", "success_rate", "return_min", "return_max", "return_sum", "length_sum",
                          "success_count")


class MjsError(RuntimeError):
    pass


def source_hash() -> str:
    """sha256 over the names and bytes of every file the library is compiled from (csrc/ + the two headers). The build
    embeds it (``-DMJS_SOURCE_HASH``) and ``mjs_version()`` reports it, so a binary that does not belong to the sources
    next to it is detected whatever the file times say (a copied tree, a git checkout, the gpurun snapshot)."""
    h = hashlib.sha256()
    for s in _sources():
        h.update(s.name.encode() + b"\0" + s.read_bytes() + b"\0")
    return h.hexdigest()[:16]


def built_hash(path: Path | None = None) -> str | None:
    """The source hash embedded in an existing library (None if the file is absent or carries none)."""
    path = Path(path or LIB_PATH)
    if not path.exists():
        return None
    m = re.search(rb"mjsim-hip [^\0]* src=([0-9a-f]{16}|unhashed)", path.read_bytes())
    return m.group(1).decode() if m else None


def build(force: bool = False, verbose: bool = False) -> Path:
    """Compile mujoco_sim_amd/csrc/mjsim.hip for gfx950 into mujoco_sim_amd/lib/libmjsim.so (skipped when the existing
    library already embeds the hash of the current sources)."""
    want = source_hash()
    if not force and built_hash() == want:
        return LIB_PATH
    LIB_PATH.parent.mkdir(parents=True, exist_ok=True)
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    # max-ilp: the kernels run one wavefront per SIMD, so schedule for ILP, not occupancy (+2% measured).
    # enable-ipra=0: with inter-procedural register allocation the call to the (rare, register-hungry) robust path clobbers every
    # AGPR in the step kernels' eyes, and their hot loops then spill to scratch instead of to AGPRs: Robot-Reach 39.7 -> 36.8 us,
    # Button-Push 110.9 -> 93.9 us per launch (profiles/r03_c_ipra_ab.txt); Planar-Push / Pointmass unchanged.
    flags = ["--offload-arch=gfx950", "-O3", "-std=c++17", "-Wno-comment", "-mllvm", "-amdgpu-sched-strategy=max-ilp", "-mllvm", "-enable-ipra=0",
             f'-DMJS_SOURCE_HASH="{want}"']
    src = str(_PKG / "csrc" / "mjsim.hip")
    # the same compilation once more, to device assembly, for the ISA lint (_isa_lint.py: a code-generation fault of this
    # compiler that the flags above provoke around out-of-line calls); both run side by side
    asm_path = LIB_PATH.with_suffix(".gfx950.s")
    asm = subprocess.Popen([hipcc, *flags, "-S", "--cuda-device-only", "-Wno-unused-command-line-argument", "-o", str(asm_path), src],
                           stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
    res = subprocess.run([hipcc, *flags, "-fPIC", "-shared", "-o", str(LIB_PATH), src], capture_output=True, text=True)
    asm_err = asm.communicate()[1]
    if res.returncode != 0 or asm.returncode != 0:
        LIB_PATH.unlink(missing_ok=True)
        raise MjsError(f"hipcc failed:\n{res.stderr}\n{asm_err}")
    from ._isa_lint import lint
    findings = lint(asm_path.read_text().split("\n"))
    asm_path.unlink(missing_ok=True)
    if findings:
        LIB_PATH.unlink(missing_ok=True)
        raise MjsError("ISA lint: register copies ahead of an exec-mask restore (see mujoco_sim_amd/_isa_lint.py): "
                       + "; ".join(f"{fn} {label}: {copies[:2]}" for fn, label, copies, _ in findings))
    if verbose:
        print(res.stderr)
    return LIB_PATH


_lib = None


def lib() -> C.CDLL:
    """Load libmjsim.so. On the first load the hash embedded in the binary is compared with the hash of the sources
    next to it: a missing or stale library is rebuilt, and if that is impossible the load FAILS (no stale binary is
    ever used silently, and there is no CPU fallback). MJS_LIB (diagnostic builds) bypasses the check."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.environ.get("MJS_LIB") and built_hash() != source_hash():
        try:
            build()
        except Exception as e:  # noqa: BLE001
            raise MjsError(f"libmjsim.so is missing or older than its sources (embedded {built_hash()}, sources "
                           f"{source_hash()}) and could not be rebuilt ({e}); there is no CPU fallback") from e
    L = C.CDLL(str(LIB_PATH))
    L.mjs_version.restype = C.c_char_p
    if not os.environ.get("MJS_LIB") and f"src={source_hash()}".encode() not in L.mjs_version():
        raise MjsError(f"loaded {LIB_PATH} reports {L.mjs_version()!r}, sources hash to {source_hash()}")
    for name in ("mjs_obs_dim", "mjs_action_dim", "mjs_state_dim", "mjs_algorithmic_bytes_per_env_step", "mjs_substeps"):
        getattr(L, name).argtypes = [C.c_int]
        getattr(L, name).restype = C.c_int
    for name in ("mjs_env_obs_dim", "mjs_env_state_dim", "mjs_env_algorithmic_bytes_per_env_step"):
        getattr(L, name).argtypes = [C.c_void_p]
        getattr(L, name).restype = C.c_int
    L.mjs_action_dim_for.argtypes = [C.c_int, C.c_int]
    L.mjs_action_dim_for.restype = C.c_int
    L.mjs_create.argtypes = [C.POINTER(MjsConfig), C.POINTER(C.c_void_p)]
    L.mjs_destroy.argtypes = [C.c_void_p]
    L.mjs_destroy.restype = None
    L.mjs_last_error.argtypes = [C.c_void_p]
    L.mjs_last_error.restype = C.c_char_p
    L.mjs_seed.argtypes = [C.c_void_p, C.c_uint32, C.c_void_p]
    L.mjs_reset.argtypes = [C.c_void_p, C.c_void_p, C.POINTER(MjsOutputs), C.c_void_p]
    L.mjs_step.argtypes = [C.c_void_p, C.c_void_p, C.POINTER(MjsOutputs), C.c_void_p]
    L.mjs_rollout.argtypes = [C.c_void_p, C.c_void_p, C.c_int32, C.POINTER(MjsOutputs), C.c_void_p]
    L.mjs_get_state.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p]
    L.mjs_set_state.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p]
    L.mjs_debug_ur5e_ik.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p]
    L.mjs_ur5e_tcp_to_joints.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p]
    L.mjs_ur5e_robot_run.argtypes = [C.c_void_p, C.c_void_p, C.c_int32, C.c_double, C.c_int32, C.c_int32, C.c_double, C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p]
    L.mjs_render.argtypes = [C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p]
    L.mjs_set_scene_camera.argtypes = [C.c_void_p, C.POINTER(MjsCameraPose)]
    L.mjs_get_scene_camera.argtypes = [C.c_void_p, C.POINTER(MjsCameraPose)]
    L.mjs_render_rgbd.argtypes = [C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p]
    L.mjs_demonstration_actions.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_double, C.c_void_p, C.c_void_p, C.c_void_p]
    L.mjs_rollout_demonstration.argtypes = [C.c_void_p, C.c_void_p, C.c_int32, C.POINTER(MjsDemoRollout), C.POINTER(MjsOutputs), C.c_void_p]
    L.mjs_actor_create.argtypes = [C.POINTER(MjsActorDesc), C.POINTER(C.c_void_p)]
    L.mjs_actor_destroy.argtypes = [C.c_void_p]
    L.mjs_actor_destroy.restype = None
    L.mjs_actor_load.argtypes = [C.c_void_p, C.POINTER(MjsActorWeights), C.c_void_p]
    L.mjs_actor_actions.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(C.c_double), C.POINTER(C.c_double), C.c_void_p, C.c_void_p, C.c_void_p]
    L.mjs_rollout_actor.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.POINTER(MjsActorRollout), C.POINTER(MjsOutputs), C.c_void_p]
    L.mjs_encoder_create.argtypes = [C.POINTER(MjsEncoderDesc), C.POINTER(C.c_void_p)]
    L.mjs_encoder_destroy.argtypes = [C.c_void_p]
    L.mjs_encoder_destroy.restype = None
    L.mjs_encoder_load.argtypes = [C.c_void_p, C.POINTER(MjsEncoderWeights), C.c_void_p]
    L.mjs_encoder_flat_dim.argtypes = [C.c_void_p]
    L.mjs_encoder_workspace_bytes.argtypes = [C.c_void_p, C.c_int32]
    L.mjs_encoder_workspace_bytes.restype = C.c_uint64
    L.mjs_encoder_features.argtypes = [C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p]
    L.mjs_actor_create_visual.argtypes = [C.POINTER(MjsActorDesc), C.POINTER(MjsActorFeatureInputs), C.POINTER(C.c_void_p)]
    L.mjs_actor_actions_visual.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(C.c_void_p * 2), C.c_void_p, C.POINTER(C.c_double), C.POINTER(C.c_double),
                                           C.c_void_p, C.c_void_p, C.c_void_p]
    L.mjs_rollout_visual_actor.argtypes = [C.c_void_p, C.c_void_p, C.POINTER(C.c_void_p * 2), C.c_void_p, C.c_int32, C.POINTER(MjsVisualRollout), C.POINTER(MjsOutputs),
                                           C.c_void_p]
    L.mjs_replay_workspace_bytes.argtypes = [C.c_int32, C.c_int32]
    L.mjs_replay_workspace_bytes.restype = C.c_uint64
    L.mjs_replay_add.argtypes = [C.POINTER(MjsReplayStorage), C.POINTER(MjsReplayBlock), C.c_void_p, C.c_void_p]
    L.mjs_replay_sample.argtypes = [C.POINTER(MjsReplayStorage), C.c_void_p, C.c_int32, C.POINTER(MjsReplayBatch), C.c_void_p]
    L.mjs_critic_create.argtypes = [C.POINTER(MjsCriticDesc), C.POINTER(C.c_void_p)]
    L.mjs_critic_destroy.argtypes = [C.c_void_p]
    L.mjs_critic_destroy.restype = None
    L.mjs_critic_load.argtypes = [C.c_void_p, C.POINTER(MjsCriticWeights), C.c_double, C.c_void_p]
    L.mjs_critic_q.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p]
    L.mjs_sac_td_target.argtypes = [C.c_void_p, C.c_void_p, C.POINTER(MjsTdTargetArgs), C.c_void_p]
    L.mjs_critic_opt_create.argtypes = [C.c_void_p, C.POINTER(MjsCriticOptDesc), C.POINTER(C.c_void_p)]
    L.mjs_critic_opt_destroy.argtypes = [C.c_void_p]
    L.mjs_critic_opt_destroy.restype = None
    L.mjs_critic_train_workspace_bytes.argtypes = [C.c_void_p, C.c_int32]
    L.mjs_critic_train_workspace_bytes.restype = C.c_uint64
    L.mjs_critic_grad.argtypes = [C.c_void_p, C.c_void_p, C.POINTER(MjsCriticGradArgs), C.c_void_p]
    L.mjs_critic_update.argtypes = [C.c_void_p, C.POINTER(MjsCriticGradArgs), C.c_double, C.c_void_p]
    L.mjs_critic_blend.argtypes = [C.c_void_p, C.c_void_p, C.c_double, C.c_void_p]
    L.mjs_critic_export.argtypes = [C.c_void_p, C.POINTER(MjsCriticWeights), C.c_void_p]
    L.mjs_actor_opt_create.argtypes = [C.c_void_p, C.POINTER(MjsActorOptDesc), C.POINTER(C.c_void_p)]
    L.mjs_actor_opt_destroy.argtypes = [C.c_void_p]
    L.mjs_actor_opt_destroy.restype = None
    L.mjs_actor_train_workspace_bytes.argtypes = [C.c_void_p, C.c_int32]
    L.mjs_actor_train_workspace_bytes.restype = C.c_uint64
    L.mjs_actor_grad.argtypes = [C.c_void_p, C.c_void_p, C.POINTER(MjsActorGradArgs), C.c_void_p]
    L.mjs_actor_update.argtypes = [C.c_void_p, C.POINTER(MjsActorGradArgs), C.c_double, C.c_void_p]
    L.mjs_actor_export.argtypes = [C.c_void_p, C.POINTER(MjsActorWeights), C.c_void_p]
    L.mjs_encoder_opt_create.argtypes = [C.c_void_p, C.POINTER(MjsEncoderOptDesc), C.POINTER(C.c_void_p)]
    L.mjs_encoder_opt_destroy.argtypes = [C.c_void_p]
    L.mjs_encoder_opt_destroy.restype = None
    L.mjs_encoder_train_workspace_bytes.argtypes = [C.c_void_p, C.c_int32]
    L.mjs_encoder_train_workspace_bytes.restype = C.c_uint64
    L.mjs_encoder_grad.argtypes = [C.c_void_p, C.c_void_p, C.POINTER(MjsEncoderGradArgs), C.c_void_p]
    L.mjs_encoder_update.argtypes = [C.c_void_p, C.POINTER(MjsEncoderGradArgs), C.c_double, C.c_void_p]
    L.mjs_encoder_blend.argtypes = [C.c_void_p, C.c_void_p, C.c_double, C.c_void_p]
    L.mjs_encoder_export.argtypes = [C.c_void_p, C.POINTER(MjsEncoderWeights), C.c_void_p]
    L.mjs_sac_draw_batch.argtypes = [C.POINTER(MjsReplayStorage), C.POINTER(MjsSacBatch), C.c_int32, C.c_uint64, C.c_uint64, C.c_void_p]
    L.mjs_sac_train.argtypes = [C.POINTER(MjsSacTrainArgs), C.c_void_p]
    L.mjs_monitor_workspace_bytes.argtypes = [C.c_int32, C.c_int32]
    L.mjs_monitor_workspace_bytes.restype = C.c_uint64
    L.mjs_monitor_update.argtypes = [C.POINTER(MjsMonitorState), C.POINTER(MjsMonitorBlock), C.c_void_p, C.c_void_p]
    L.mjs_monitor_summary.argtypes = [C.POINTER(MjsMonitorState), C.c_void_p, C.c_void_p]
    L.mjs_get_rng_state.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    L.mjs_set_rng_state.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    _lib = L
    return L


def check(rc: int, handle=None):
    if rc != 0:
        msg = lib().mjs_last_error(handle)
        raise MjsError(f"libmjsim error {rc}: {msg.decode() if msg else '?'}")
