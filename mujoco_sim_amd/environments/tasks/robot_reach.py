"""Robot-Reach task description (host side).

Mirrors ``mujoco_sim/environments/tasks/robot_reach.py:33-83`` (RobotReachConfig dataclass:
same fields and defaults), the task constructor at :85-132 and the module-level demonstration policy at
:222-253. Physics and task logic run in csrc/mjs_reach.h, the policy in csrc/mjs_policy.h.
"""
from __future__ import annotations

import dataclasses

import numpy as np

from ...entities.camera import CameraConfig
from .point_reach import BoundedArraySpec


@dataclasses.dataclass
class RobotReachConfig:
    SPARSE_REWARD = "sparse_reward"
    DENSE_NEG_DISTANCE_REWARD = "dense_negative_distance_reward"
    STATE_OBS = "state_observations"
    VISUAL_OBS = "visual_observations"
    REL_EEF_ACTION = "relative_eef_action"
    ABS_EEF_ACTION = "absolute_eef_action"
    REL_JOIN_ACTION = "relative_joint_action"
    ABS_JOIN_ACTION = "absolute_joint_action"
    REWARD_TYPES = (SPARSE_REWARD, DENSE_NEG_DISTANCE_REWARD)
    OBSERVATION_TYPES = (STATE_OBS, VISUAL_OBS)
    ACTION_TYPES = (REL_EEF_ACTION, ABS_EEF_ACTION, REL_JOIN_ACTION, ABS_JOIN_ACTION)
    FRONT_TILTED_CAMERA_CONFIG = CameraConfig(np.array([0.0, -1.1, 0.5]), np.array([-0.7, -0.35, 0, 0.0]), 70)  # robot_reach.py:52

    reward_type: str = None
    observation_type: str = None
    action_type: str = None
    max_step_size: float = 0.05
    physics_timestep: float = 0.005
    control_timestep: float = 0.1
    max_control_steps_per_episode: int = 100
    image_resolution: int = 96
    goal_distance_threshold: float = 0.02
    target_radius = 0.03
    # opt-in: the reference task never terminates on success
    terminate_on_success: bool = False
    cameraconfig: CameraConfig = None  # the scene camera (robot_reach.py:70,78): None = FRONT_TILTED_CAMERA_CONFIG

    def __post_init__(self):
        self.reward_type = self.reward_type or RobotReachConfig.DENSE_NEG_DISTANCE_REWARD
        self.observation_type = self.observation_type or RobotReachConfig.STATE_OBS
        self.action_type = self.action_type or RobotReachConfig.ABS_EEF_ACTION
        self.cameraconfig = self.cameraconfig or RobotReachConfig.FRONT_TILTED_CAMERA_CONFIG
        assert self.observation_type in RobotReachConfig.OBSERVATION_TYPES
        assert self.reward_type in RobotReachConfig.REWARD_TYPES
        assert self.action_type in RobotReachConfig.ACTION_TYPES


class RobotReachTask:
    task_name = "robot_reach"

    def __init__(self, config: RobotReachConfig | None = None) -> None:
        self.config = config or RobotReachConfig()
        self.physics_timestep = self.config.physics_timestep
        self.control_timestep = self.config.control_timestep
        self.reward_type = self.config.reward_type
        self.observation_type = self.config.observation_type
        self.image_resolution = self.config.image_resolution
        # robot_reach.py:116-117: the task overwrites the camera config's image size with its image_resolution
        self.cameraconfig = self.config.cameraconfig
        self.cameraconfig.image_width = self.cameraconfig.image_height = self.config.image_resolution
        if self.config.action_type != RobotReachConfig.ABS_EEF_ACTION:
            # the reference's before_step only implements the absolute-EEF path (robot_reach.py:159-169)
            raise NotImplementedError("only ABS_EEF_ACTION is implemented (as in the reference)")

    @property
    def CONTROL_TIMESTEP(self):
        return self.config.control_timestep

    def action_spec(self, physics=None):
        return BoundedArraySpec((3,), np.float64, [-0.1, -0.6, 0.02], [0.1, -0.4, 0.2])

    def create_random_policy(self):
        spec = self.action_spec()

        def random_policy(time_step):
            return np.random.uniform(spec.minimum, spec.maximum, spec.shape)

        return random_policy

    def demonstration_actions(self, venv, noise_level: float = 0.0, generator=None):
        """One batched step of the reference's demonstration policy (robot_reach.py:240-249) for every env of ``venv`` (a
        HipVectorEnv of this task), computed on the device (csrc/mjs_policy.h): the TCP position plus the difference to the target,
        with ``noise_level`` times a standard-normal draw added to the difference and the reference's speed clamp."""
        return venv.demonstration_actions(noise=noise_level, generator=generator)[0]


def create_demonstration_policy(environment, noise_level=0.0):
    """robot_reach.py:222-253, module-level as there: policy(time_step) -> absolute TCP target (numpy) for a single-env
    ``HipEnvironment`` of this task (or a ``HipVectorEnv``, whose env 0 it then drives)."""
    venv = environment._venv if hasattr(environment, "_venv") else environment
    task = getattr(environment, "task", None)
    assert task is None or isinstance(task, RobotReachTask)  # robot_reach.py:225

    def demonstration_policy(time_step=None):
        return venv.demonstration_actions(noise=noise_level)[0][0].cpu().numpy()

    return demonstration_policy
