"""Shared by test_oracle_known_answers.py (CPU) and test_camera_oracle.py (GPU): the table of moved scene-camera poses, the
states both sides are brought to, and the bars. Host logic only: numpy and the oracle, no device.

Bars (the oracle image tests' own, test_gpu_parity.py): Point-Mass bit for bit; Robot-Reach and Button-Push below 1e-4 differing
bytes, Planar-Push below 2e-4, none off by more than 2 grey levels. Depth: Point-Mass bit for bit; robot scenes the same +inf mask
and at most DEPTH_TOL (1e-4 m, test_camera_views.py's bar) apart where both are finite."""
import numpy as np

N = 12
DEPTH_TOL = 1e-4
TASK_IDS = {"point_mass_reach": 0, "robot_reach": 1, "robot_planar_push": 2, "robot_push_button": 3}
ROBOT_TASKS = ("robot_reach", "robot_planar_push", "robot_push_button")
BYTE_BAR = {"point_mass_reach": 0.0, "robot_reach": 1e-4, "robot_push_button": 1e-4, "robot_planar_push": 2e-4}
SEEDS = {"point_mass_reach": 2025, "robot_reach": 2025, "robot_planar_push": 2032, "robot_push_button": 3}
SIZES = ((64, 64), (96, 96), (40, 24), (30, 22))  # one workgroup, bands of rows, non-square, the 8x8-tile walk
# the tasks' own scene cameras (point_reach.py:22, robot_reach.py:52, robot_planar_push.py:43, robot_push_button.py:51-52,87)
DEFAULTS = {
    "point_mass_reach": ([0.0, 0.0, 2.4], [1.0, 0.0, 0.0, 0.0], 30.0),
    "robot_reach": ([0.0, -1.1, 0.5], [-0.7, -0.35, 0.0, 0.0], 70.0),
    "robot_planar_push": ([0.0, -1.1, 0.5], [-0.7, -0.35, 0.0, 0.0], 70.0),
    "robot_push_button": ([0.0, -1.7, 0.7], [-0.7, -0.35, 0.0, 0.0], 70.0),
}


def quat_mul(a, b):
    aw, ax, ay, az = a
    bw, bx, by, bz = b
    return [aw * bw - ax * bx - ay * by - az * bz, aw * bx + ax * bw + ay * bz - az * by,
            aw * by - ax * bz + ay * bw + az * bx, aw * bz + ax * by - ay * bx + az * bw]


def frame(quat):
    """Columns of the rotation matrix of a MuJoCo quaternion: the camera's right (+x), up (+y) and back (+z) axes in the world."""
    w, x, y, z = np.asarray(quat, dtype=np.float64) / np.linalg.norm(quat)
    R = np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)],
                  [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
                  [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]])
    return R[:, 0], R[:, 1], R[:, 2]


def rays(pose, H, W):
    """Pinhole rays through the pixel centres, float64: unit directions [H, W, 3] and the axis cosine -(d . back) [H, W]."""
    pos, quat, fov = pose
    right, up, back = frame(quat)
    th = np.tan(np.radians(fov) / 2)
    px = (2 * (np.arange(W) + 0.5) / W - 1) * th * (W / H)
    py = (1 - 2 * (np.arange(H) + 0.5) / H) * th
    d = px[None, :, None] * right + py[:, None, None] * up - back
    d = d / np.linalg.norm(d, axis=2, keepdims=True)
    return d, -(d @ back)


def look_at(eye, target, roll_deg=0.0):
    """Quaternion (w, x, y, z) of a camera at eye that looks at target with the world's +z up, rolled about its optical axis."""
    eye, target = np.asarray(eye, dtype=np.float64), np.asarray(target, dtype=np.float64)
    back = (eye - target) / np.linalg.norm(eye - target)
    right = np.cross([0.0, 0.0, 1.0], back)
    right = right / np.linalg.norm(right)
    up = np.cross(back, right)
    a = np.radians(roll_deg)
    right, up = np.cos(a) * right + np.sin(a) * up, -np.sin(a) * right + np.cos(a) * up
    R = np.stack([right, up, back], axis=1)
    w = np.sqrt(max(0.0, 1 + R[0, 0] + R[1, 1] + R[2, 2])) / 2
    x = np.sqrt(max(0.0, 1 + R[0, 0] - R[1, 1] - R[2, 2])) / 2
    y = np.sqrt(max(0.0, 1 - R[0, 0] + R[1, 1] - R[2, 2])) / 2
    z = np.sqrt(max(0.0, 1 - R[0, 0] - R[1, 1] + R[2, 2])) / 2
    return [w, np.copysign(x, R[2, 1] - R[1, 2]), np.copysign(y, R[0, 2] - R[2, 0]), np.copysign(z, R[1, 0] - R[0, 1])]


def robot_poses(task):
    """The moved poses of a robot task, name -> (position, quaternion as given, fovy). 'moved' is the pose of
    test_tile_walk_and_rectangle_walk_agree_under_a_moved_camera; quaternions are deliberately left unnormalised."""
    pos, quat, fov = DEFAULTS[task]
    table = {
        "moved": ((np.asarray(pos) + [0.2, -0.1, 0.3]).tolist(), quat_mul(quat, [0.0, 0.0, 0.0, 1.0]), 55.0),
        "top_down": ([0.0, -0.5, 2.4], [1.0, 0.0, 0.0, 0.0], 30.0),  # RobotPushConfig.TOP_DOWN_CAMERA_CONFIG
        "behind": BEHIND,
        "close_in": CLOSE_IN,
        "wide": WIDE,
        "narrow": NARROW,
        "sky": (pos, [0.0, 2.0, 0.0, 0.0], fov),  # half a turn about the camera's x from straight down: straight up
    }
    if task == "robot_push_button":  # the only scene that draws the scene camera's body
        table["in_wrist_view"] = IN_WRIST_VIEW
    return table


# from behind the robot (y > 0), looking back over the arm at its workspace
BEHIND = ([0.35, 0.9, 0.95], [0.1188, 0.0663, 0.483, 0.865], 60.0)  # look_at((0, -0.35, 0.15)), four decimals
# close in: 0.25 m from the base's axis at z = 0.4, inside the arm's reach, aimed at the shoulder (look_at((0, 0, 0.16))): links
# of the 12 arms lie behind and across the camera plane, the nearest surface is 3 to 15 cm from the eye
CLOSE_IN = ([-0.18, -0.17, 0.40], [0.8457, 0.358, -0.1543, -0.3645], 75.0)
WIDE = ([0.1, -0.8, 0.45], [-0.7, -0.35, 0.05, 0.02], 120.0)
NARROW = ([-0.3, -1.2, 0.6], [0.8045, 0.5729, -0.1451, -0.0593], 20.0)  # look_at((0, -0.3, 0.3)) rolled 10 degrees
# Button-Push: the scene camera 0.2 m above the floor in front of the grippers, where the wrist cameras of most of the 12 envs
# look, turned against the world's axes (look_at((0, -0.1, 0.5)) rolled 20 degrees): its 9 x 2.5 x 2.5 cm box and its lens win
# pixels of the wrist images, so these show where button_prims_kernel put the body and along which axes. From every other pose
# of the table no wrist camera sees the body at all.
IN_WRIST_VIEW = ([-0.55, -0.5, 0.2], [0.5223, 0.6692, -0.504, -0.1595], 60.0)
WRIST_BODY_PRIMS = (14, 15)  # the scene camera's box and lens in the Button-Push primitive list (render_winner gives k + 1)
POINTMASS_POSES = {
    "tilted": ([0.2, -0.15, 2.2], [0.99, 0.07, -0.05, 0.06], 45.0),
    "sky": ([0.0, 0.0, 2.4], [0.0, 2.0, 0.0, 0.0], 30.0),
}


def poses(task):
    return POINTMASS_POSES if task == "point_mass_reach" else robot_poses(task)


def shifted(pose, mm=2.0):
    """The pose moved by `mm` millimetres along its own right + up diagonal (across the image, not along the view)."""
    right, up, _ = frame(pose[1])
    return ((np.asarray(pose[0], dtype=np.float64) + mm * 1e-3 * (right + up) / np.sqrt(2.0)).tolist(), pose[1], pose[2])


def make_oracle(oracle_mod, task, n=N):
    """The oracle batch of a task after reset and the few steps of the existing image tests (test_gpu_parity.py), with the
    actions it took ([T, n, A]) so that the GPU side can take the same ones, and its last observations."""
    seed = SEEDS[task]
    rs = np.random.RandomState(12345)
    if task == "point_mass_reach":
        ob = oracle_mod.OracleBatch(0, n, seed)
        acts = rs.uniform(-0.05, 0.05, (7, n, 2)).astype(np.float32).astype(np.float64)
    elif task == "robot_reach":
        ob = oracle_mod.OracleBatch(1, n, seed)
        acts = rs.uniform([-0.1, -0.6, 0.02], [0.1, -0.4, 0.2], (5, n, 3))
    elif task == "robot_push_button":  # joint actions around the nominal configuration: the arms differ widely
        ob = oracle_mod.OracleBatch(3, n, seed, nthreads=4, action_type=0)
        nominal = np.array([-1.57, -1.57, 1.57, -1.57, -1.57, 0.0, 0.04])
        acts = nominal + rs.uniform(-1, 1, (4, n, 7)) * np.array([0.6, 0.4, 0.4, 0.4, 0.4, 0.6, 0.04])
    else:
        ob = oracle_mod.OracleBatch(2, n, seed, nthreads=4, block_shape=0)  # mesh blocks, the default of both sides
        acts = None
    o = ob.reset()
    if acts is None:  # Planar-Push: a few steps towards the first block (test_planar_push_camera_matches_oracle)
        acts = []
        for _ in range(4):
            a = o["obs"][:, :2] + np.clip(o["obs"][:, 5:7] - o["obs"][:, :2], -0.02, 0.02)
            acts.append(a)
            o = ob.step(a)
        acts = np.stack(acts)
    else:
        for a in acts:
            o = ob.step(a)
    return ob, acts, o["obs"]


def clearance(prims, eye):
    """Distance (float64, metres) from eye to the nearest of the oracle's primitive records [n, 17] (scene_primitives); negative
    inside one. Capped cylinders are measured as the capsules that enclose them: never more than the true distance."""
    eye = np.asarray(eye, dtype=np.float64)
    best = np.inf
    for rec in np.asarray(prims, dtype=np.float64):
        kind, a, b, c, half, r = int(rec[0]), rec[1:4], rec[4:7], rec[7:10], rec[10:13], rec[13]
        if kind == 1:
            dist = np.linalg.norm(eye - a) - r
        elif kind in (2, 3):
            ab = b - a
            s = np.clip(np.dot(eye - a, ab) / np.dot(ab, ab), 0.0, 1.0)
            dist = np.linalg.norm(eye - (a + s * ab)) - r
        else:
            local = np.array([np.dot(eye - a, b), np.dot(eye - a, c), np.dot(eye - a, np.cross(b, c))])
            q = np.abs(local) - half
            dist = np.linalg.norm(np.maximum(q, 0.0)) + min(q.max(), 0.0)
        best = min(best, dist)
    return best


def image_shares(rgb_a, rgb_b):
    """(share of differing bytes, largest difference in grey levels)"""
    diff = np.abs(rgb_a.astype(np.int16) - rgb_b.astype(np.int16))
    return float((diff > 0).mean()), int(diff.max())


def depth_shares(depth_a, depth_b):
    """(largest |delta| where both are finite, number of pixels whose +inf masks differ, share of pixels that moved by more than
    DEPTH_TOL or changed mask)"""
    fa, fb = np.isfinite(depth_a), np.isfinite(depth_b)
    both = fa & fb
    dd = np.abs(depth_a[both].astype(np.float64) - depth_b[both].astype(np.float64))
    moved = (fa != fb).sum() + (dd > DEPTH_TOL).sum()
    return float(dd.max()) if dd.size else 0.0, int((fa != fb).sum()), float(moved / depth_a.size)
