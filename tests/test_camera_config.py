"""Scene-camera configuration, host side (no GPU): the C struct of the pose, the CameraConfig schema and presets of the
reference (entities/camera.py:55-64, robot_reach.py:52,70,78,116-117, robot_planar_push.py:42-43,63,70,110-111) and the
visual observation layout with and without depth maps."""
import ctypes as C
import re
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parents[1]


def test_camera_pose_struct_matches_the_header():
    from mujoco_sim_amd import _native as nat

    assert C.sizeof(nat.MjsCameraPose) == 72
    header = (ROOT / "include" / "mjsim.h").read_text()
    body = re.search(r"typedef struct \{([^}]*)\} mjs_camera_pose;", header).group(1)
    declared = re.findall(r"^\s*(uint32_t|int32_t|double)\s+(\w+)(?:\[(\d)\])?;", body, re.M)
    assert [(n, int(k or 1)) for _, n, k in declared] == [("struct_size", 1), ("reserved0", 1), ("pos", 3), ("quat", 4), ("fovy", 1)]
    sizes = {"uint32_t": 4, "int32_t": 4, "double": 8}
    off = 0
    for ctype, name, count in declared:  # natural alignment, no padding: the header's order gives the offsets
        field = getattr(nat.MjsCameraPose, name)
        assert (field.offset, field.size) == (off, sizes[ctype] * int(count or 1)), name
        off += field.size
    assert off == 72
    assert nat.MjsCameraPose().struct_size == 72  # filled in like MjsConfig's
    assert {"mjs_set_scene_camera", "mjs_get_scene_camera", "mjs_render_rgbd"} <= set(nat.EXPORTED_SYMBOLS)


def test_camera_config_schema_and_presets():
    from mujoco_sim_amd.entities.camera import CameraConfig
    from mujoco_sim_amd.environments.tasks.robot_planar_push import RobotPushConfig
    from mujoco_sim_amd.environments.tasks.robot_reach import RobotReachConfig

    c = CameraConfig()
    assert (c.position, c.orientation, c.fov, c.image_height, c.image_width, c.name) == (None, None, None, 96, 96, "Camera")
    c = CameraConfig(np.array([1.0, 2.0, 3.0]), np.array([1.0, 0, 0, 0]), 45)
    assert c.fov == 45 and c.position.tolist() == [1.0, 2.0, 3.0]
    for preset in (RobotReachConfig.FRONT_TILTED_CAMERA_CONFIG, RobotPushConfig.FRONT_TILTED_CAMERA_CONFIG):
        assert isinstance(preset, CameraConfig)
        assert (list(preset.position), list(preset.orientation), preset.fov) == ([0.0, -1.1, 0.5], [-0.7, -0.35, 0.0, 0.0], 70)
    top = RobotPushConfig.TOP_DOWN_CAMERA_CONFIG
    assert (list(top.position), list(top.orientation), top.fov) == ([0.0, -0.5, 2.4], [1.0, 0.0, 0.0, 0.0], 30)
    assert not hasattr(RobotReachConfig, "TOP_DOWN_CAMERA_CONFIG")  # robot_reach.py has the front-tilted preset only


def test_cameraconfig_plumbing_of_the_task_configs():
    from mujoco_sim_amd.entities.camera import CameraConfig
    from mujoco_sim_amd.environments.tasks.robot_planar_push import RobotPushConfig, RobotPushTask
    from mujoco_sim_amd.environments.tasks.robot_reach import RobotReachConfig, RobotReachTask

    assert RobotReachConfig().cameraconfig is RobotReachConfig.FRONT_TILTED_CAMERA_CONFIG  # None resolves to front-tilted
    assert RobotPushConfig().cameraconfig is RobotPushConfig.FRONT_TILTED_CAMERA_CONFIG
    assert RobotPushConfig(cameraconfig=RobotPushConfig.TOP_DOWN_CAMERA_CONFIG).cameraconfig is RobotPushConfig.TOP_DOWN_CAMERA_CONFIG
    for config_cls, task_cls, res in ((RobotReachConfig, RobotReachTask, 48), (RobotPushConfig, RobotPushTask, 32)):
        mine = CameraConfig(np.array([0.3, -1.0, 0.8]), np.array([0.9, 0.4, 0.0, 0.1]), 55, image_height=7, image_width=9)
        task = task_cls(config_cls(cameraconfig=mine, image_resolution=res))
        assert task.cameraconfig is mine and task.config.cameraconfig is mine
        assert (mine.image_height, mine.image_width) == (res, res)  # overwritten by image_resolution, as in the reference
        assert (mine.fov, list(mine.position)) == (55, [0.3, -1.0, 0.8])
        default_task = task_cls(config_cls(image_resolution=res))
        assert default_task.cameraconfig is config_cls.FRONT_TILTED_CAMERA_CONFIG and default_task.cameraconfig.image_height == res


def test_visual_observation_layout_with_and_without_depth():
    from mujoco_sim_amd.vector_env import visual_observation_layout as layout

    r = 32
    rgb, depth = ((r, r, 3), np.uint8), ((r, r), np.float32)
    for task, state_key in (("point_mass_reach", "pointmass/position"), ("robot_reach", "ur5e/tcp_position"), ("robot_planar_push", "ur5e/tcp_position")):
        plain = layout(task, None, r)
        assert [k for k, _, _ in plain] == [state_key, "Camera/rgb_image"]
        assert plain == layout(task, None, r, depth_observations=False)  # off by default: existing layouts unchanged
        deep = layout(task, None, r, depth_observations=True)
        assert [k for k, _, _ in deep] == [state_key, "Camera/rgb_image", "Camera/depth_map"]
        assert deep[1][1:] == rgb and deep[2][1:] == depth
        assert deep[:2] == plain
    plain = layout("robot_push_button", "absolute_joint_action", r)
    assert [k for k, _, _ in plain] == ["ur5e/joint_configuration", "ur5e/Camera/rgb_image", "Camera/rgb_image"]
    deep = layout("robot_push_button", "absolute_joint_action", r, depth_observations=True)
    assert [k for k, _, _ in deep] == ["ur5e/joint_configuration", "ur5e/Camera/rgb_image", "ur5e/Camera/depth_map", "Camera/rgb_image", "Camera/depth_map"]
    assert [e[1:] for e in deep[1:]] == [rgb, depth, rgb, depth]
    no_wrist = layout("robot_push_button", "absolute_eef_action", r, use_wrist_camera=False, depth_observations=True)
    assert [k for k, _, _ in no_wrist] == ["ur5e/tcp_position", "Camera/rgb_image", "Camera/depth_map"]
