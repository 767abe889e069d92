"""Configurable scene camera and depth output of the ray caster, on the GPU (include/mjsim.h: mjs_set_scene_camera,
mjs_get_scene_camera, mjs_render_rgbd). The default views are pinned byte for byte by the oracle image tests of
test_gpu_parity.py; everything here is checked from geometry alone: symmetries of the pinhole model (a rolled camera, a
wider lens) against those pinned views, and unprojection of the depth map in numpy float64. Moved poses (translated, re-aimed,
close to the arm) and the depth maps of both cameras are pinned pixel by pixel against the oracle in test_camera_oracle.py.

Bars. Images of two poses that see the same rays agree only to float32 rounding of the rays, so they are held to the bar the
robot-scene images have against the oracle: differing bytes below 2e-4 of all bytes, none off by more than 2. Depth: float32
at a range of at most 5 m rounds to about 1e-6 m per operation, the bar is 1e-4 m. A point rebuilt in float64 from a float32
depth inherits that 1e-4 m."""
import ctypes as C
import re
from pathlib import Path

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

ROOT = Path(__file__).resolve().parents[1]
N = 12
ROBOT_TASKS = ("robot_reach", "robot_planar_push", "robot_push_button")
ALL_TASKS = ("point_mass_reach",) + ROBOT_TASKS
# the tasks' own scene cameras (point_reach.py:22, robot_reach.py:52, robot_planar_push.py:43, robot_push_button.py:51-52,87)
DEFAULTS = {
    "point_mass_reach": ([0.0, 0.0, 2.4], [1.0, 0.0, 0.0, 0.0], 30.0),
    "robot_reach": ([0.0, -1.1, 0.5], [-0.7, -0.35, 0.0, 0.0], 70.0),
    "robot_planar_push": ([0.0, -1.1, 0.5], [-0.7, -0.35, 0.0, 0.0], 70.0),
    "robot_push_button": ([0.0, -1.7, 0.7], [-0.7, -0.35, 0.0, 0.0], 70.0),
}
ARENA_HALF = 1.5  # EmptyRobotArena(3)
DEPTH_TOL = 1e-4


def _spec_constant(name):
    text = (ROOT / "include" / "mjs_scene_spec.h").read_text()
    return float(re.search(rf"\b{name}\s*=\s*([-0-9.eE]+)f?;", text).group(1))


@pytest.fixture(scope="module")
def envs():
    """One handle per task, a few random steps in (the arms differ); every test leaves the default camera behind."""
    import mujoco_sim_amd as m

    made = {}

    def get(task):
        if task not in made:
            venv = m.HipVectorEnv(task, N, seed=41)
            venv.reset()
            rng = np.random.RandomState(9)
            lo, hi = np.asarray(venv.action_low, dtype=np.float64), np.asarray(venv.action_high, dtype=np.float64)
            for _ in range(4):
                venv.step(torch.as_tensor(lo + rng.uniform(0, 1, (N, venv.action_dim)) * (hi - lo), device="cuda"))
            made[task] = venv
        made[task].set_scene_camera(None)
        return made[task]

    yield get
    for venv in made.values():
        venv.close()


def _quat_mul(a, b):
    aw, ax, ay, az = a
    bw, bx, by, bz = b
    return np.array([aw * bw - ax * bx - ay * by - az * bz, aw * bx + ax * bw + ay * bz - az * by,
                     aw * by - ax * bz + ay * bw + az * bx, aw * bz + ax * by - ay * bx + az * bw])


def _frame(quat):
    """Columns of the rotation matrix of a MuJoCo quaternion: the camera's right (+x), up (+y) and back (+z) axes in the world."""
    w, x, y, z = np.asarray(quat, dtype=np.float64) / np.linalg.norm(quat)
    R = np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)],
                  [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
                  [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]])
    return R[:, 0], R[:, 1], R[:, 2]


def _rays(pose, H, W):
    """Pinhole rays through the pixel centres, float64: unit directions [H, W, 3] and -(d . back) [H, W]."""
    pos, quat, fov = pose
    right, up, back = _frame(quat)
    th = np.tan(np.radians(fov) / 2)
    px = (2 * (np.arange(W) + 0.5) / W - 1) * th * (W / H)
    py = (1 - 2 * (np.arange(H) + 0.5) / H) * th
    d = px[None, :, None] * right + py[:, None, None] * up - back
    d = d / np.linalg.norm(d, axis=2, keepdims=True)
    return d, -(d @ back)


def _unproject(pose, depth):
    """P = eye + depth / (-(d . back)) * d for every pixel of depth [N, H, W] (non-finite depths give non-finite points)."""
    d, zs = _rays(pose, depth.shape[1], depth.shape[2])
    with np.errstate(invalid="ignore"):
        return np.asarray(pose[0], dtype=np.float64) + (depth.astype(np.float64) / zs)[..., None] * d


def _pixel_of(pose, points, H, W):
    """(row, col) of the pixel onto which world points [n, 3] project."""
    pos, quat, fov = pose
    right, up, back = _frame(quat)
    v = np.asarray(points, dtype=np.float64) - np.asarray(pos, dtype=np.float64)
    z = -(v @ back)
    th = np.tan(np.radians(fov) / 2)
    col = np.floor(((v @ right) / z / (th * W / H) + 1) / 2 * W).astype(int)
    row = np.floor((1 - (v @ up) / z / th) / 2 * H).astype(int)
    assert (z > 0).all() and (col >= 0).all() and (col < W).all() and (row >= 0).all() and (row < H).all()
    return row, col


def _assert_same_view(rgb_a, depth_a, rgb_b, depth_b, what):
    diff = np.abs(rgb_a.astype(np.int16) - rgb_b.astype(np.int16))
    print(what, "bytes differing", float((diff > 0).mean()), "max", int(diff.max()))
    both = np.isfinite(depth_a) & np.isfinite(depth_b)
    dd = np.abs(depth_a[both] - depth_b[both])
    print(what, "depth max |delta|", float(dd.max()), "finite in both", float(both.mean()))
    assert (diff > 0).mean() < 2e-4 and diff.max() <= 2, (what, float((diff > 0).mean()), int(diff.max()))
    assert both.any() and dd.max() <= DEPTH_TOL, (what, float(dd.max()))


def _cpu(*tensors):
    return [t.cpu().numpy() for t in tensors]


# ---------------------------------------------------------------------------------------------------------- 1. nothing moved
@pytest.mark.parametrize("task", ALL_TASKS)
def test_rgbd_and_default_pose_leave_every_image_as_it_was(envs, task):
    """64x64: one workgroup per image; 96x96: bands of rows; 40x24: a non-square single workgroup; 30x22: no multiple of 8, the
    8x8-tile walk. render_rgbd's image is render's; setting the task's own default numbers, and None, changes no byte."""
    venv = envs(task)
    cams = (0, 1) if task == "robot_push_button" else (0,)
    for h, w in ((64, 64), (96, 96), (40, 24), (30, 22)):
        for cam in cams:
            base = venv.render(h, w, camera=cam).clone()
            assert base.float().std() > 10
            rgb, depth = venv.render_rgbd(h, w, camera=cam)
            assert torch.equal(rgb, base), (task, h, w, cam)
            assert torch.equal(venv.render_depth(h, w, camera=cam), depth), (task, h, w, cam)  # the depth-only launch: same map
            assert torch.isfinite(depth).any() and not torch.isnan(depth).any() and (depth > 0).all()
            venv.set_scene_camera(*DEFAULTS[task])
            assert torch.equal(venv.render(h, w, camera=cam), base), (task, h, w, cam, "default numbers")
            venv.set_scene_camera(None)
            assert torch.equal(venv.render(h, w, camera=cam), base), (task, h, w, cam, "None")


# ---------------------------------------------------------------------------------------------------------- 2. rolled camera
@pytest.mark.parametrize("task", ROBOT_TASKS)
def test_camera_rolled_half_a_turn_sees_the_image_upside_down(envs, task):
    """default (x) 180 degrees about the optical axis: right and up change sign, so pixel (r, c) sees what (H-1-r, W-1-c) saw. A
    genuinely different frame through the rectangles, the culling and the table, against a view the oracle pins."""
    venv = envs(task)
    pos, quat, fov = DEFAULTS[task]
    rolled = _quat_mul(quat, [0.0, 0.0, 0.0, 1.0])
    for h, w in ((64, 64), (40, 24)):
        rgb0, depth0 = _cpu(*venv.render_rgbd(h, w))
        venv.set_scene_camera(pos, rolled, fov)
        rgb1, depth1 = _cpu(*venv.render_rgbd(h, w))
        venv.set_scene_camera(None)
        _assert_same_view(rgb1, depth1, rgb0[:, ::-1, ::-1], depth0[:, ::-1, ::-1], (task, h, w, "rolled"))


@pytest.mark.parametrize("task", ROBOT_TASKS)
def test_tile_walk_and_rectangle_walk_agree_under_a_moved_camera(envs, task):
    """The 8x8-tile walk (what sizes that are no multiple of 8 take, and every size of kernel_variant 1) and the rectangle walk
    with its table only differ in WHICH exact ray tests they run: from a moved, rolled camera with another lens their images
    and their depth maps are equal bit for bit, as test_scene_camera_kernels_agree_byte_for_byte holds for the default view.
    (The mirror symmetry above is no bar for the tile walk's own sizes: at 30x22 the mirrored pixel coordinates are not each
    other's negatives in float32, and 6e-4 of 23760 bytes came out one level apart - three times the 2e-4 that larger images meet.)"""
    import mujoco_sim_amd as m

    venv = envs(task)
    tile = m.HipVectorEnv(task, N, seed=41, kernel_variant=1)
    tile.set_state(venv.get_state())
    pos, quat, fov = DEFAULTS[task]
    moved = (np.asarray(pos) + [0.2, -0.1, 0.3], _quat_mul(quat, [0.0, 0.0, 0.0, 1.0]), 55.0)
    venv.set_scene_camera(*moved)
    tile.set_scene_camera(*moved)
    for h, w in ((64, 64), (96, 96), (40, 24)):
        (rgb_a, depth_a), (rgb_b, depth_b) = venv.render_rgbd(h, w), tile.render_rgbd(h, w)
        assert torch.equal(rgb_a, rgb_b), (task, h, w, int((rgb_a != rgb_b).sum()))
        assert torch.equal(depth_a, depth_b), (task, h, w, int((depth_a != depth_b).sum()))
        assert rgb_a.float().std() > 10 and torch.isfinite(depth_a).any()
    venv.set_scene_camera(None)
    tile.close()


# ---------------------------------------------------------------------------------------------------------- 3. wider lens
@pytest.mark.parametrize("task", ALL_TASKS)
def test_centre_crop_of_a_wider_lens_is_the_default_view(envs, task):
    """tan(fovy'/2) = 2 tan(fovy/2) at 2H x 2W: the centre H x W pixels look along the default image's rays. H = 32: the wide
    image is one workgroup's; H = 48: it is cut into bands."""
    venv = envs(task)
    pos, quat, fov = DEFAULTS[task]
    wide = float(np.degrees(2 * np.arctan(2 * np.tan(np.radians(fov) / 2))))
    for h in (32, 48):
        rgb0, depth0 = _cpu(*venv.render_rgbd(h, h))
        venv.set_scene_camera(pos, quat, wide)
        rgb1, depth1 = _cpu(*venv.render_rgbd(2 * h, 2 * h))
        venv.set_scene_camera(None)
        crop = slice(h // 2, h // 2 + h)
        _assert_same_view(rgb1[:, crop, crop], depth1[:, crop, crop], rgb0, depth0, (task, h, "wide"))


# ---------------------------------------------------------------------------------------------------------- 4. unprojection
@pytest.mark.parametrize("task", ROBOT_TASKS)
def test_depth_unprojects_onto_the_robot_scene(envs, task):
    venv = envs(task)
    pose = DEFAULTS[task]
    eye = np.asarray(pose[0])
    for h, w in ((64, 64), (96, 96), (30, 22)):
        rgb, depth = _cpu(*venv.render_rgbd(h, w))
        P = _unproject(pose, depth)
        finite = np.isfinite(depth)
        assert (P[finite][:, 2] >= -DEPTH_TOL).all(), (task, h, w, float(P[finite][:, 2].min()))
        floor = finite & (P[..., 2] <= DEPTH_TOL)
        above = finite & (P[..., 2] > 0.02)
        assert floor.any() and above.any()
        assert (np.abs(P[floor][:, :2]) <= ARENA_HALF + DEPTH_TOL).all(), (task, h, w, float(np.abs(P[floor][:, :2]).max()))
        # +inf exactly where the pixel is the background's (0, 0, 0) and its ray misses the arena rectangle
        d, _ = _rays(pose, h, w)
        with np.errstate(divide="ignore", invalid="ignore"):
            t = -eye[2] / d[..., 2]
            x, y = eye[0] + t * d[..., 0], eye[1] + t * d[..., 1]
        misses = ~((t > 0) & (np.abs(x) <= ARENA_HALF) & (np.abs(y) <= ARENA_HALF))
        black = (rgb == 0).all(axis=3)
        inf = np.isposinf(depth)
        # A black BODY in front of the sky is the one exception: the gripper stand-in and the camera bodies are black
        # (rgb 0 0 0 with a specular term below half a grey level), and with the arm raised they show above the arena's far
        # edge - finite depth, black pixel, a ray that misses the floor. Such a pixel must then unproject onto the robot:
        # above the floor and within the arm's reach of its base (0.85 m + the 0.17 m gripper + the base's height).
        body = black & misses[None] & ~inf
        print(task, h, w, "inf", int(inf.sum()), "inf off the rule", int((inf & ~(black & misses[None])).sum()), "black bodies before the sky", int(body.sum()))
        assert not (inf & ~(black & misses[None])).any(), (task, h, w)
        assert body.mean() < 0.02 and (P[body][:, 2] > 0.02).all() and (np.linalg.norm(P[body], axis=1) < 1.3).all(), (task, h, w, int(body.sum()))
        assert not np.isnan(depth).any() and not np.isneginf(depth).any()


def test_depth_unprojects_onto_the_pointmass_sphere(envs):
    """All envs, no exemptions: the pixel onto which the sphere's centre projects shows the sphere (the translucent sphere is a
    surface), so the rebuilt point lies one radius from the centre."""
    venv = envs("point_mass_reach")
    pose = DEFAULTS["point_mass_reach"]
    radius = _spec_constant("MJS_PM_RADIUS")
    centre = np.concatenate([venv.flat_obs[:, 0:2].cpu().numpy(), np.full((N, 1), radius)], axis=1)  # pointmass/position, z = radius
    for h, w in ((64, 64), (96, 96), (30, 44)):  # the last one wider than high: the whole arena stays in view
        depth = venv.render_depth(h, w).cpu().numpy()
        P = _unproject(pose, depth)
        row, col = _pixel_of(pose, centre, h, w)
        err = np.abs(np.linalg.norm(P[np.arange(N), row, col] - centre, axis=1) - radius)
        print("pointmass", h, w, "max | |P - centre| - radius |", float(err.max()))
        assert (err <= 1e-3).all(), (h, w, err)


# ---------------------------------------------------------------------------------------------------------- 5. top-down preset
def test_top_down_preset_on_planar_push():
    """TOP_DOWN_CAMERA_CONFIG at 128x128 (half a pixel is about 5 mm on the floor): the z-depth of a horizontal plane under a
    camera that looks straight down is constant."""
    import mujoco_sim_amd as m

    top = m.RobotPushConfig.TOP_DOWN_CAMERA_CONFIG
    pose = (list(top.position), list(top.orientation), float(top.fov))
    height = pose[0][2]
    # the config route: a visual-observation env built with the preset shows what a state handle of the same seed renders
    vis = m.HipVectorEnv("robot_planar_push", N, seed=5, observation_type="visual_observations", image_resolution=64, cameraconfig=top,
                         depth_observations=True)
    venv = m.HipVectorEnv("robot_planar_push", N, seed=5)
    obs, _ = vis.reset()
    venv.reset()
    assert list(obs) == ["ur5e/tcp_position", "Camera/rgb_image", "Camera/depth_map"]
    assert obs["Camera/depth_map"].shape == (N, 64, 64) and obs["Camera/depth_map"].dtype == torch.float32
    default_image = venv.render(64, 64).clone()
    venv.set_scene_camera(top.position, top.orientation, top.fov)
    assert torch.equal(obs["Camera/rgb_image"], venv.render(64, 64))
    assert torch.equal(obs["Camera/depth_map"], venv.render_depth(64, 64))
    assert not torch.equal(obs["Camera/rgb_image"], default_image)
    for got, want in zip(vis.get_scene_camera(), pose):
        assert np.allclose(got, want, rtol=0, atol=1e-15)
    vis.close()
    # a few steps to TCP targets drawn from the task's own workspace (robot_planar_push.py:102: |x| <= 0.2, y in [-0.6, -0.3])
    rng = np.random.RandomState(9)
    for _ in range(3):
        venv.step(torch.as_tensor(rng.uniform([-0.2, -0.6], [0.2, -0.3], (N, 2)), device="cuda"))
    rgb, depth = _cpu(*venv.render_rgbd(128, 128))
    tcp = venv.flat_obs[:, 0:3].cpu().numpy()  # ur5e/tcp_position
    venv.close()
    assert np.isfinite(depth).all()  # 1.29 m of floor around (0, -0.5): all inside the arena
    assert (depth <= height + DEPTH_TOL).all(), float(depth.max())
    # Floor pixels, told from where things ARE and not from their depth: the arm stands at x = 0 and works within |x| <= 0.2 (its
    # links at most 0.13 m beside the plane through base and tool), blocks and target spawn within |x| <= 0.15, and what stands
    # 0.5 m high is drawn at most a quarter further from the axis; the view's two outer strips, whose rays meet the floor at
    # |x| > 0.5, show nothing but floor.
    d, _ = _rays(pose, 128, 128)
    x_on_floor = pose[0][0] - height / d[..., 2] * d[..., 0]
    strips = np.broadcast_to(np.abs(x_on_floor) > 0.5, depth.shape)
    assert strips.mean() > 0.15
    print("top-down floor strips: max |depth - height|", float(np.abs(depth[strips] - height).max()), "share of the image at the floor's depth",
          float((np.abs(depth - height) <= DEPTH_TOL).mean()))
    assert (np.abs(depth[strips] - height) <= DEPTH_TOL).all(), float(np.abs(depth[strips] - height).max())
    assert (np.abs(depth - height) <= DEPTH_TOL).mean() > 0.5  # and the floor is most of the image
    # the CylinderEEF (radius 0.02) stands on the TCP: the ray of the pixel nearest the TCP's projection hits it or the arm above
    row, col = _pixel_of(pose, tcp, 128, 128)
    at_tcp = depth[np.arange(N), row, col]
    print("top-down depth at the TCP", at_tcp, "tcp z", tcp[:, 2])
    assert (at_tcp <= height - tcp[:, 2] + 2e-3).all(), (at_tcp, tcp[:, 2])


def test_button_push_depth_observations(envs):
    """depth_observations adds each camera's depth map right after its image; off by default."""
    import mujoco_sim_amd as m
    from mujoco_sim_amd.vector_env import visual_observation_layout

    kw = dict(seed=3, observation_type="visual_observations", image_resolution=32)
    deep = m.HipVectorEnv("robot_push_button", 4, depth_observations=True, **kw)
    plain = m.HipVectorEnv("robot_push_button", 4, **kw)
    obs, _ = deep.reset()
    ref, _ = plain.reset()
    layout = visual_observation_layout("robot_push_button", "absolute_joint_action", 32, True, depth_observations=True)
    assert list(obs) == [k for k, _, _ in layout] == list(deep.single_observation_space.spaces)
    assert list(ref) == ["ur5e/joint_configuration", "ur5e/Camera/rgb_image", "Camera/rgb_image"]
    for k, shape, dt in layout:
        assert tuple(obs[k].shape) == (4,) + shape and obs[k].cpu().numpy().dtype == dt, k
    for k in ref:
        assert torch.equal(obs[k], ref[k]), k
    assert torch.equal(obs["Camera/depth_map"], plain.render_depth(32, 32))
    assert torch.equal(obs["ur5e/Camera/depth_map"], plain.render_depth(32, 32, camera=1))
    deep.close()
    plain.close()


# ---------------------------------------------------------------------------------------------------------- 6. the body moves
def test_the_cameras_body_moves_with_the_pose(envs):
    """Button-Push draws the scene camera's box and lens. Pulled back 0.3 m along its own optical axis, the camera must not find
    its body at the old place (a box left there would fill the centre pixel at about 0.29 m); and from any pose its own body,
    which contains the eye, is never hit."""
    venv = envs("robot_push_button")
    pos, quat, fov = DEFAULTS["robot_push_button"]
    centre = venv.render_depth(64, 64)[:, 32, 32].cpu().numpy()
    assert np.isfinite(centre).all() and (centre > 0.5).all(), centre  # not its own box from inside
    back = _frame(quat)[2]
    venv.set_scene_camera(np.asarray(pos) + 0.3 * back, quat, fov)
    pulled = venv.render_depth(64, 64)[:, 32, 32].cpu().numpy()
    venv.set_scene_camera(None)
    print("centre depth", centre, "pulled back", pulled)
    assert (pulled > 0.5).all(), pulled


# ---------------------------------------------------------------------------------------------------------- 7. refusals, round trip
def test_invalid_camera_arguments_are_refused(envs):
    from mujoco_sim_amd import _native as nat

    venv = envs("robot_reach")
    L, h = venv._lib, venv._h
    pos, quat, fov = DEFAULTS["robot_reach"]
    before = venv.get_scene_camera()

    def pose(pos=pos, quat=quat, fov=fov, **kw):
        return nat.MjsCameraPose(pos=(C.c_double * 3)(*pos), quat=(C.c_double * 4)(*quat), fovy=fov, **kw)

    bad = {
        "nan position": pose(pos=[0.0, float("nan"), 1.0]), "inf position": pose(pos=[float("inf"), 0.0, 1.0]),
        "nan quaternion": pose(quat=[1.0, 0.0, float("nan"), 0.0]), "inf fovy": pose(fov=float("inf")), "nan fovy": pose(fov=float("nan")),
        "zero quaternion": pose(quat=[0.0, 0.0, 0.0, 0.0]), "tiny quaternion": pose(quat=[1e-10, 0.0, 0.0, 0.0]),
        "fovy 0": pose(fov=0.0), "fovy 180": pose(fov=180.0), "fovy negative": pose(fov=-30.0),
        "struct_size": pose(struct_size=64),
    }
    for name, p in bad.items():
        assert L.mjs_set_scene_camera(h, C.byref(p)) == -1, name  # MJS_ERR_INVALID_ARG
        assert b"mjs_set_scene_camera" in L.mjs_last_error(h), name
        with pytest.raises(nat.MjsError):
            nat.check(L.mjs_set_scene_camera(h, C.byref(p)), h)
    assert b"struct_size" in L.mjs_last_error(h)
    with pytest.raises(nat.MjsError):
        venv.set_scene_camera([0.0, 0.0, 1.0], [0.0, 0.0, 0.0, 0.0], 45.0)
    after = venv.get_scene_camera()
    assert all(np.array_equal(a, b) for a, b in zip(before, after))  # a refused pose changes nothing
    assert L.mjs_render_rgbd(h, 0, 32, 32, None, None, None) == -1 and b"mjs_render_rgbd" in L.mjs_last_error(h)
    img = torch.empty(N, 32, 32, 3, dtype=torch.uint8, device="cuda")
    assert L.mjs_render_rgbd(h, 1, 32, 32, img.data_ptr(), None, None) == -1  # no wrist camera on Robot-Reach
    assert L.mjs_set_scene_camera(None, None) == -1 and L.mjs_get_scene_camera(h, None) == -1


def test_camera_round_trip_and_state_independence(envs):
    import mujoco_sim_amd as m

    venv = envs("robot_reach")
    for got, want in zip(venv.get_scene_camera(), DEFAULTS["robot_reach"]):  # the default, quaternion normalised
        want = np.asarray(want) / np.linalg.norm(want) if np.ndim(want) and len(want) == 4 else want
        assert np.allclose(got, want, rtol=0, atol=1e-15)
    pos, quat, fov = [0.4, -1.3, 0.9], [2.0, 1.0, 0.2, -0.4], 55.0
    venv.set_scene_camera(pos, quat, fov)
    gp, gq, gf = venv.get_scene_camera()
    assert np.array_equal(gp, pos) and gf == fov
    assert np.allclose(gq, np.asarray(quat) / np.linalg.norm(quat), rtol=0, atol=1e-15) and abs(np.linalg.norm(gq) - 1) < 1e-15
    moved = venv.render(32, 32).clone()
    # the pose is the handle's, not the state block's
    state = venv.get_state()
    venv.set_state(state)
    assert all(np.array_equal(a, b) for a, b in zip(venv.get_scene_camera(), (gp, gq, gf)))
    assert torch.equal(venv.render(32, 32), moved)
    other = m.HipVectorEnv("robot_reach", N, seed=41, env_index_offset=N)  # a second handle (a shard) has its own, default camera
    for got, want in zip(other.get_scene_camera(), DEFAULTS["robot_reach"]):
        want = np.asarray(want) / np.linalg.norm(want) if np.ndim(want) and len(want) == 4 else want
        assert np.allclose(got, want, rtol=0, atol=1e-15)
    other.set_state(state)  # a checkpoint carries no camera: same state, the other handle's default view
    assert all(np.array_equal(a, b) for a, b in zip(venv.get_scene_camera(), (gp, gq, gf)))
    venv.set_scene_camera(None)
    assert torch.equal(other.render(32, 32), venv.render(32, 32)) and not torch.equal(venv.render(32, 32), moved)
    other.close()
