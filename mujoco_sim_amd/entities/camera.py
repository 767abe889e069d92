"""Camera description (host side).

Mirrors the schema of ``mujoco_sim/entities/camera.py:55-64`` (``CameraConfig``: same fields and defaults). The camera
itself - pose, body geoms, RGB image and depth map (camera.py:76-114) - lives in the engine: ``mjs_set_scene_camera`` /
``mjs_render_rgbd`` (include/mjsim.h), ``HipVectorEnv.set_scene_camera`` / ``render_rgbd``.
"""
from __future__ import annotations

import dataclasses

import numpy as np


@dataclasses.dataclass
class CameraConfig:
    # orientation is a MuJoCo quaternion (w, x, y, z) in MuJoCo's camera frame: the camera looks along its local -z, +y is up
    position: np.ndarray = None
    orientation: np.ndarray = None
    fov: float = None  # vertical field of view in degrees
    image_height: int = 96
    image_width: int = 96
    name: str = "Camera"
