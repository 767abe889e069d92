"""Moved scene cameras and depth maps of the HIP ray caster against the CPU oracle (oracle/om_render.c: om_render_view tests every
primitive against every ray, no culling, no table, no tiles, in the same float32 operations). test_gpu_parity.py pins the default
views' RGB this way; this file pins what depends on the pose - the tan-space rectangles and their near-plane clipping, the
"eye within 5 mm of the box" rule, the per-pose ray / floor table and its cache, the Button-Push camera body placed at the pose -
and the depth output of both cameras. The oracle's own new part is checked on the CPU first (test_oracle_known_answers.py).

Poses, states and bars: tests/_camera_poses.py. Both sides reach the same state by the same seed and the same few actions as the
existing image tests. RGB: Point-Mass bit for bit; Robot-Reach and Button-Push below 1e-4 differing bytes, Planar-Push below 2e-4,
none off by more than 2 grey levels. Depth: Point-Mass bit for bit; robot scenes the same +inf mask and at most 1e-4 m apart
where both are finite - the image bar of 2 grey levels means no silhouette pixel flips between primitives, so none may here.
Every comparison prints its figures (a "PARITY" line); profiles/camera_oracle_parity.txt keeps those of one run."""
import numpy as np
import pytest
import torch

import _camera_poses as cp

pytestmark = pytest.mark.gpu
N = cp.N


@pytest.fixture(scope="module")
def pairs(oracle_mod):
    """task -> (GPU handle, the same state in a kernel_variant=1 handle (8x8-tile walk at every size), oracle batch, mask of the
    envs whose observations agree to 1e-8). Built once; every test leaves the default camera behind."""
    import mujoco_sim_amd as m

    made = {}

    def get(task):
        if task not in made:
            ob, acts, obs = cp.make_oracle(oracle_mod, task)
            venv = m.HipVectorEnv(task, N, seed=cp.SEEDS[task])
            venv.reset()
            for a in acts:
                venv.step(torch.from_numpy(a))
            same = np.abs(venv.flat_obs.cpu().numpy() - obs).max(axis=1) < 1e-8
            assert same.sum() >= N - 2 if task == "robot_planar_push" else same.all(), (task, same)
            tile = m.HipVectorEnv(task, N, seed=cp.SEEDS[task], kernel_variant=1)
            tile.set_state(venv.get_state())
            made[task] = (venv, tile, ob, same)
        for handle in made[task][:2]:
            handle.set_scene_camera(None)
        return made[task]

    yield get
    for venv, tile, ob, _ in made.values():
        venv.close()
        tile.close()


def _set(venv, pose):
    if pose is None:
        venv.set_scene_camera(None)
    else:
        venv.set_scene_camera(*pose)


def _locate(ob, pose, camera, same, bad, gpu_depth, cpu_depth):
    """The first few offending pixels, for the report: (env, row, col, the surface the oracle's brute force gives the pixel
    (-1 nothing, 0 floor, k + 1 primitive k), oracle depth, GPU depth)."""
    h, w = bad.shape[1:]
    win = ob.render_winner(h, w, camera, pose)[same]
    envs = np.flatnonzero(same)
    return [(int(envs[i]), int(r), int(c), int(win[i, r, c]), float(cpu_depth[i, r, c]), float(gpu_depth[i, r, c])) for i, r, c in np.argwhere(bad)[:6]]


def _compare(task, what, ob, same, pose, camera, h, w, rgb=None, depth=None):
    """One GPU image and / or depth map against the oracle's, to the task's bars; prints the figures before it asserts."""
    cpu_rgb, cpu_depth = ob.render_rgbd(h, w, camera, pose)
    cpu_rgb, cpu_depth = cpu_rgb[same], cpu_depth[same]
    exact = task == "point_mass_reach"
    line = f"PARITY {task} {what} {h}x{w} camera {camera}:"
    errors = []
    if rgb is not None:
        rgb = rgb.cpu().numpy()[same]
        share, level = cp.image_shares(rgb, cpu_rgb)
        line += f" bytes differing {share:.2e} max level {level}"
        if not (share == 0 if exact else (share < cp.BYTE_BAR[task] and level <= 2)):
            errors.append(("rgb", share, level))
    if depth is not None:
        depth = depth.cpu().numpy()[same]
        assert depth.dtype == np.float32 and not np.isnan(depth).any() and not np.isneginf(depth).any()
        dmax, dinf, _ = cp.depth_shares(depth, cpu_depth)
        line += f" depth max |delta| {dmax:.2e} inf-mask mismatches {dinf}"
        if exact:
            if not np.array_equal(depth, cpu_depth):
                errors.append(("depth bits", int((depth != cpu_depth).sum())))
        elif dinf or dmax > cp.DEPTH_TOL:
            with np.errstate(invalid="ignore"):
                bad = (np.isfinite(depth) != np.isfinite(cpu_depth)) | (np.abs(depth - cpu_depth) > cp.DEPTH_TOL)
            errors.append(("depth", dmax, dinf, _locate(ob, pose, camera, same, bad, depth, cpu_depth)))
    print(line)
    assert not errors, (task, what, h, w, camera, errors)
    return cpu_rgb, cpu_depth


def _cases():
    return [(task, name) for task in cp.TASK_IDS for name in cp.poses(task)]


# ------------------------------------------------------------------------------------------------------ 1. the pose table
@pytest.mark.parametrize("task,name", _cases())
def test_moved_scene_camera_matches_oracle(pairs, task, name):
    """Every pose of the table at 64x64 (one workgroup per image), 96x96 (bands of rows), 40x24 (non-square) and 30x22 (no
    multiple of 8: the 8x8-tile walk), image and depth from one launch; and the kernel_variant=1 handle, which walks tiles at
    every size, at 64x64 and 40x24."""
    venv, tile, ob, same = pairs(task)
    pose = cp.poses(task)[name]
    _set(venv, pose)
    _set(tile, pose)
    for h, w in cp.SIZES:
        rgb, depth = venv.render_rgbd(h, w)
        cpu_rgb, cpu_depth = _compare(task, name, ob, same, pose, 0, h, w, rgb, depth)
        if name == "sky":
            assert not cpu_rgb.any() and np.isposinf(cpu_depth).all()
        else:
            assert cpu_rgb.std() > 10 and np.isfinite(cpu_depth).mean() > 0.05
    for h, w in ((64, 64), (40, 24)):
        rgb, depth = tile.render_rgbd(h, w)
        _compare(task, name + "/variant1", ob, same, pose, 0, h, w, rgb, depth)
    _set(venv, None)
    _set(tile, None)


# ------------------------------------------------------------------------------------------------------ 2. default-pose depth
@pytest.mark.parametrize("task", list(cp.TASK_IDS))
def test_default_pose_depth_matches_oracle(pairs, task):
    """The default views' RGB is pinned by test_gpu_parity.py; their depth maps (and the images that come with them) here."""
    venv, tile, ob, same = pairs(task)
    for h, w in cp.SIZES:
        rgb, depth = venv.render_rgbd(h, w)
        _compare(task, "default", ob, same, None, 0, h, w, rgb, depth)
    rgb, depth = tile.render_rgbd(64, 64)
    _compare(task, "default/variant1", ob, same, None, 0, 64, 64, rgb, depth)


# ------------------------------------------------------------------------------------------------------ 3. wrist camera
@pytest.mark.parametrize("name", ["default", "moved", "in_wrist_view"])
def test_wrist_camera_rgb_and_depth_match_oracle(pairs, name):
    """The wrist camera keeps its own view, but the scene camera's body stands at the scene pose. At the default pose and at 'moved'
    (the pose of the issue) no wrist camera sees that body: those two pin the wrist's image and depth and that a moved scene
    camera does not disturb them. 'in_wrist_view' puts the body where the wrist cameras look, along axes of its own: that case
    is the witness of where and how button_prims_kernel places it (the oracle-only test
    test_wrist_camera_sees_the_scene_cameras_body_at_the_in_wrist_view_pose shows the body wins pixels there and nowhere else)."""
    task = "robot_push_button"
    venv, tile, ob, same = pairs(task)
    pose = None if name == "default" else cp.robot_poses(task)[name]
    _set(venv, pose)
    _set(tile, pose)
    for h, w in cp.SIZES:
        rgb, depth = venv.render_rgbd(h, w, camera=1)
        cpu_rgb, cpu_depth = _compare(task, "wrist/" + name, ob, same, pose, 1, h, w, rgb, depth)
        assert cpu_rgb.std() > 10 and np.isfinite(cpu_depth).mean() > 0.05
        if name == "in_wrist_view":
            body = np.isin(ob.render_winner(h, w, 1, pose)[same], [k + 1 for k in cp.WRIST_BODY_PRIMS])
            assert body.any(axis=(1, 2)).sum() >= N // 2, (h, w, int(body.sum()))
    rgb, depth = tile.render_rgbd(64, 64, camera=1)
    _compare(task, "wrist/" + name + "/variant1", ob, same, pose, 1, 64, 64, rgb, depth)
    _set(venv, None)
    _set(tile, None)


# ------------------------------------------------------------------------------------------------------ 4. output modes
@pytest.mark.parametrize("task", cp.ROBOT_TASKS)
def test_output_modes_under_the_close_in_pose(pairs, task):
    """The three instantiations of every image kernel (rgb only, depth only, both) under pose 'close_in', rectangle walk and tile
    walk; Button-Push also through its wrist camera, with the scene camera at 'in_wrist_view', where the wrist sees its body."""
    venv, _, ob, same = pairs(task)
    for camera, name in (((0, "close_in"), (1, "in_wrist_view")) if task == "robot_push_button" else ((0, "close_in"),)):
        pose = cp.robot_poses(task)[name]
        _set(venv, pose)
        for h, w in ((64, 64), (30, 22)):
            _compare(task, name + "/rgb-only", ob, same, pose, camera, h, w, rgb=venv.render(h, w, camera=camera))
            _compare(task, name + "/depth-only", ob, same, pose, camera, h, w, depth=venv.render_depth(h, w, camera=camera))
            rgb, depth = venv.render_rgbd(h, w, camera=camera)
            _compare(task, name + "/both", ob, same, pose, camera, h, w, rgb, depth)
    _set(venv, None)


# ------------------------------------------------------------------------------------------------------ 5. the table cache
@pytest.mark.parametrize("task", cp.ROBOT_TASKS)
def test_ray_table_follows_the_pose_at_one_size(pairs, task):
    """One handle, one size: 'moved', 'behind', 'moved' again, then the default. The ray / floor table is keyed by the size and
    the pose's serial: a table kept from the previous pose of the same size would show that pose's floor."""
    venv, _, ob, same = pairs(task)
    table = cp.robot_poses(task)
    for step, name in enumerate(("moved", "behind", "moved", None)):
        pose = table[name] if name else None
        _set(venv, pose)
        rgb, depth = venv.render_rgbd(64, 64)
        _compare(task, f"cache-step-{step}/{name or 'default'}", ob, same, pose, 0, 64, 64, rgb, depth)
    _set(venv, None)


# ------------------------------------------------------------------------------------------------------ 6. observation route
def _reset_pair(oracle_mod, task, seed, **kw):
    import mujoco_sim_amd as m

    okw = {"action_type": 0} if task == "robot_push_button" else {"block_shape": 0}
    ob = oracle_mod.OracleBatch(cp.TASK_IDS[task], N, seed, nthreads=4, **okw)
    o = ob.reset()
    vis = m.HipVectorEnv(task, N, seed=seed, observation_type="visual_observations", image_resolution=64, depth_observations=True, **kw)
    obs, _ = vis.reset()
    same = np.abs(vis.flat_obs.cpu().numpy() - o["obs"]).max(axis=1) < 1e-8
    assert same.sum() >= N - 2 if task == "robot_planar_push" else same.all(), (task, same)
    return vis, obs, ob, same


def test_top_down_depth_observations_match_oracle(oracle_mod):
    """visual_observations with cameraconfig=TOP_DOWN_CAMERA_CONFIG and depth_observations: the image and the depth map of the
    observation dict after reset, against the oracle's render of the oracle's reset state."""
    import mujoco_sim_amd as m

    top = m.RobotPushConfig.TOP_DOWN_CAMERA_CONFIG
    pose = (list(top.position), list(top.orientation), float(top.fov))
    assert pose == tuple(cp.robot_poses("robot_planar_push")["top_down"])
    vis, obs, ob, same = _reset_pair(oracle_mod, "robot_planar_push", 5, cameraconfig=top)
    assert list(obs) == ["ur5e/tcp_position", "Camera/rgb_image", "Camera/depth_map"]
    _compare("robot_planar_push", "observations/top_down", ob, same, pose, 0, 64, 64, obs["Camera/rgb_image"], obs["Camera/depth_map"])
    vis.close()


def test_button_push_depth_observations_match_oracle(oracle_mod):
    task = "robot_push_button"
    vis, obs, ob, same = _reset_pair(oracle_mod, task, 3)
    assert list(obs) == ["ur5e/joint_configuration", "ur5e/Camera/rgb_image", "ur5e/Camera/depth_map", "Camera/rgb_image", "Camera/depth_map"]
    _compare(task, "observations/scene", ob, same, None, 0, 64, 64, obs["Camera/rgb_image"], obs["Camera/depth_map"])
    _compare(task, "observations/wrist", ob, same, None, 1, 64, 64, obs["ur5e/Camera/rgb_image"], obs["ur5e/Camera/depth_map"])
    vis.close()
