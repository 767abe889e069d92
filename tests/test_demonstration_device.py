"""The scripted demonstration policies on the device (csrc/mjs_policy.h), the closed-loop demonstration rollout
(mjs_rollout_demonstration) and the recorder's block path (LeRobotDatasetRecorder.record_rollout).

Bars: Cartesian actions 1e-12 absolute against a float64 numpy restatement / the host torch policies (a handful of float64
operations on numbers below 1: 1 ulp is 1e-16, a fused multiply-add moves a result by an ulp or two). Joint actions: bit for bit
against ``tcp_to_joints`` on the SAME inputs (the same device function); 1e-7, the bar of
``test_device_ik_matches_oracle_on_random_inputs``, where the IK's inputs themselves agree only to 1e-12 (device against host policy).
The rollout against the step-by-step loop: bit for bit (the same launches on the same data).
"""
import ctypes as C

import numpy as np
import pytest
import torch

gpu = pytest.mark.gpu
N_SYN = 70  # one full wavefront and a partial one: the tail guard
FIELDS = ("obs", "reward", "terminated", "truncated", "is_success", "step_type", "fault", "ncon", "discount")
END_POS = np.array([-0.3, -0.2, 0.3])  # robot_push_button.py:88 robot_end_position
DT = 0.1


# ---------------------------------------------------------------------------------------------- numpy restatements
def _margin(value, threshold):
    assert abs(value - threshold) >= 1e-3, (value, threshold)  # no decision on a rounding edge


def button_policy_np(obs):
    """robot_push_button.py:236-288 row by row (Cartesian target + closed gripper). The rising branch is speed-limited like the
    others, as the host mirror RobotPushButtonTask.demonstration_actions has it."""
    out, phases = np.zeros((len(obs), 4)), []
    for i, o in enumerate(obs):
        tcp, sw, active = o[6:9].copy(), o[9:12].copy(), o[12] > 0.5
        planar = np.linalg.norm(tcp[:2] - sw[:2])
        if active:
            _margin(planar, 0.05)
            goal = END_POS.copy()
            if planar < 0.05:
                goal[2] = sw[2] + 0.1
            phase = "3near" if planar < 0.05 else "3far"
        else:
            if tcp[2] > sw[2]:
                _margin(planar, 0.01)
            if planar < 0.01:
                _margin(tcp[2], sw[2])
            if tcp[2] > sw[2] and planar < 0.01:
                goal, phase = sw.copy(), "2"
            else:
                _margin(tcp[2], sw[2] + 0.02)
                if tcp[2] < sw[2] + 0.02:
                    goal, phase = np.array([tcp[0], tcp[1], sw[2] + 0.05]), "1rise"
                else:
                    goal, phase = np.array([sw[0], sw[1], sw[2] + 0.05]), "1hover"
        diff = goal - tcp
        m = np.max(np.abs(diff))
        _margin(m, 0.5 * DT)
        if m > 0.5 * DT:
            diff = diff * 0.5 / m * DT
        out[i, :3] = tcp + diff
        phases.append((phase, bool(m > 0.5 * DT)))
    return out, phases


def reach_policy_np(obs, z=None, noise=0.0):
    out, clamped = np.zeros((len(obs), 3)), []
    for i, o in enumerate(obs):
        d = o[9:12] - o[0:3]
        if z is not None:
            d = d + noise * z[i]
        m = np.max(np.abs(d))
        _margin(m, 0.5)
        if m > 0.5:
            d = d * 0.5 / m * DT
        out[i] = o[0:3] + d
        clamped.append(bool(m > 0.5))
    return out, clamped


def pointmass_policy_np(obs, z=None, noise=0.0):
    a = obs[:, 2:4] - obs[:, 0:2]
    if z is not None and noise > 0:
        a = a * (1 + noise * z)
    return a * (0.05 / np.maximum(np.abs(a).max(axis=1, keepdims=True), 1e-300))


# ---------------------------------------------------------------------------------------------- synthetic observations
Q_HOME = np.array([0.3, -1.8, -1.6, -1.3, 1.5, 0.2])


def button_obs():
    """[70, 13]: the ten decision cases (phase x clamp), each seven times with offsets of at most 5e-4 per coordinate."""
    sw = np.array([0.05, -0.45, 0.03])
    sw_end = np.array([-0.29, -0.21, 0.03])  # a switch next to the end pose: phase 3 "near" without the clamp
    cases = [  # (tcp, switch, active)
        (sw + [0.10, 0.05, 0.015], sw, 0),    # 1 rising, 0.035 to go
        (sw + [0.10, 0.05, -0.020], sw, 0),   # 1 rising, clamped
        (sw + [0.03, -0.02, 0.060], sw, 0),   # 1 hover
        (sw + [0.15, 0.08, 0.060], sw, 0),    # 1 hover, clamped
        (sw + [0.003, 0.002, 0.040], sw, 0),  # 2
        (sw + [0.003, -0.002, 0.080], sw, 0),  # 2, clamped
        (END_POS + [0.02, -0.01, -0.20], sw_end, 1),  # 3 near the switch: lift to switch + 0.1
        (sw + [0.01, 0.02, 0.005], sw, 1),    # 3 near, clamped
        (END_POS + [0.02, -0.03, 0.01], sw, 1),  # 3 far
        (sw + [0.10, 0.0, 0.05], sw, 1),      # 3 far, clamped
    ]
    rs = np.random.RandomState(5)
    obs = np.zeros((N_SYN, 13))
    for i in range(N_SYN):
        tcp, s, active = cases[i % 10]
        obs[i, 0:6] = Q_HOME + rs.uniform(-0.05, 0.05, 6)
        obs[i, 6:9] = np.asarray(tcp) + rs.uniform(-5e-4, 5e-4, 3)
        obs[i, 9:12] = np.asarray(s) + rs.uniform(-5e-4, 5e-4, 3)
        obs[i, 12] = active
    return obs


def _call_policy(venv, obs, z=None, noise=0.0, want_ok=True):
    from mujoco_sim_amd import _native as nat

    o = torch.as_tensor(obs, dtype=torch.float64, device=venv.device).contiguous()
    zt = None if z is None else torch.as_tensor(z, dtype=torch.float64, device=venv.device).contiguous()
    a = torch.full((venv.num_envs, venv.action_dim), np.nan, dtype=torch.float64, device=venv.device)
    ok = torch.full((venv.num_envs,), 7, dtype=torch.uint8, device=venv.device)
    nat.check(venv._lib.mjs_demonstration_actions(venv._h, o.data_ptr(), None if zt is None else zt.data_ptr(), float(noise), a.data_ptr(),
                                                  ok.data_ptr() if want_ok else None, venv._stream()), venv._h)
    return a.cpu().numpy(), ok.cpu().numpy()


# ---------------------------------------------------------------------------------------------- 1. every branch
@gpu
def test_button_policy_every_branch_from_synthetic_observations():
    import mujoco_sim_amd as m

    obs = button_obs()
    want, phases = button_policy_np(obs)
    assert set(phases) == {(p, c) for p in ("1rise", "1hover", "2", "3near", "3far") for c in (False, True)}
    venv = m.HipVectorEnv("robot_push_button", N_SYN, action_type="absolute_eef_action")
    got, ok = _call_policy(venv, obs)
    print("button eef max |diff|", np.abs(got - want).max())
    np.testing.assert_allclose(got, want, rtol=0, atol=1e-12)
    assert (got[:, 3] == 0).all() and (ok == 1).all()
    got2, ok2 = _call_policy(venv, obs, want_ok=False)  # ik_ok is optional
    assert np.array_equal(got, got2) and (ok2 == 7).all()
    venv.close()


@gpu
def test_reach_policy_both_sides_of_the_clamp_and_noise():
    import mujoco_sim_amd as m

    rs = np.random.RandomState(6)
    obs = np.zeros((N_SYN, 12))
    obs[:, 0:3] = rs.uniform([-0.1, -0.6, 0.02], [0.1, -0.4, 0.2], (N_SYN, 3))
    obs[:, 3:9] = Q_HOME
    obs[:, 9:12] = rs.uniform([-0.1, -0.6, 0.02], [0.1, -0.4, 0.2], (N_SYN, 3))
    obs[::3, 9] += 0.7    # a target more than 0.5 away: the clamp
    obs[1::6, 11] -= 0.9
    venv = m.HipVectorEnv("robot_reach", N_SYN)
    want, clamped = reach_policy_np(obs)
    assert 10 < sum(clamped) < N_SYN - 10
    got, ok = _call_policy(venv, obs)
    print("reach max |diff|", np.abs(got - want).max())
    np.testing.assert_allclose(got, want, rtol=0, atol=1e-12)
    assert (ok == 1).all()
    z = rs.standard_normal((N_SYN, 3))
    want_n, clamped_n = reach_policy_np(obs, z, 0.05)
    got_n, _ = _call_policy(venv, obs, z, 0.05)
    np.testing.assert_allclose(got_n, want_n, rtol=0, atol=1e-12)
    assert np.abs(got_n - got).max() > 1e-3
    assert np.array_equal(_call_policy(venv, obs, None, 0.05)[0], got) and np.array_equal(_call_policy(venv, obs, z, 0.0)[0], got)  # no z / no noise
    venv.close()


@gpu
def test_pointmass_policy_with_the_zero_difference_row_and_noise():
    import mujoco_sim_amd as m

    rs = np.random.RandomState(7)
    obs = rs.uniform(-0.8, 0.8, (N_SYN, 4))
    obs[3, 2:4] = obs[3, 0:2]    # the mass sits on the goal: the reference divides by zero here
    obs[68, 2:4] = obs[68, 0:2]  # ... and in the partial wavefront
    venv = m.HipVectorEnv("point_mass_reach", N_SYN)
    got, ok = _call_policy(venv, obs)
    want = pointmass_policy_np(obs)
    print("pointmass max |diff|", np.abs(got - want).max())
    np.testing.assert_allclose(got, want, rtol=0, atol=1e-12)
    assert (got[[3, 68]] == 0).all() and np.isfinite(got).all() and (ok == 1).all()
    live = np.ones(N_SYN, bool)
    live[[3, 68]] = False
    np.testing.assert_allclose(np.abs(got[live]).max(axis=1), 0.05, rtol=0, atol=1e-12)
    z = rs.standard_normal((N_SYN, 2))
    got_n, _ = _call_policy(venv, obs, z, 0.3)
    np.testing.assert_allclose(got_n, pointmass_policy_np(obs, z, 0.3), rtol=0, atol=1e-12)
    assert (got_n[[3, 68]] == 0).all() and np.abs(got_n - got).max() > 1e-3
    venv.close()


# ---------------------------------------------------------------------------------------------- 2. joint actions
@gpu
def test_button_joint_actions_are_the_device_ik_of_the_cartesian_actions():
    import mujoco_sim_amd as m

    obs = button_obs()
    obs[13, 6:9] *= 3.0  # a TCP far outside the arm's reach: the clamped target stays there
    eef = m.HipVectorEnv("robot_push_button", N_SYN, action_type="absolute_eef_action")
    joint = m.HipVectorEnv("robot_push_button", N_SYN, action_type="absolute_joint_action")
    a_eef, _ = _call_policy(eef, obs)
    a_joint, ok = _call_policy(joint, obs)
    q, found = joint.tcp_to_joints(torch.from_numpy(a_eef[:, :3].copy()), torch.from_numpy(obs[:, 0:6].copy()))
    q, found = q.cpu().numpy(), found.cpu().numpy()
    print("joint actions against tcp_to_joints: max |diff|", np.abs(a_joint[:, :6] - q).max())
    assert np.array_equal(a_joint[:, :6], q)  # the same device function on the same inputs
    assert np.array_equal(ok.astype(bool), found) and (a_joint[:, 6] == 0).all()
    assert ok[13] == 0 and np.array_equal(a_joint[13, :6], obs[13, 0:6])  # held joints
    assert ok.sum() == N_SYN - 1
    assert np.abs(a_joint[ok == 1, :6] - obs[ok == 1, 0:6]).max() > 1e-3  # ... and real solutions elsewhere
    eef.close()
    joint.close()


# ---------------------------------------------------------------------------------------------- 3. device against host policy
@gpu
@pytest.mark.parametrize("action_type", ["absolute_eef_action", "absolute_joint_action"])
def test_button_device_policy_matches_host_policy_in_closed_loop(action_type):
    import mujoco_sim_amd as m

    N = 64
    task = m.RobotPushButtonTask(observation_type="state_observations", action_type=action_type)
    venv = m.HipVectorEnv("robot_push_button", N, seed=77, autoreset="disabled", action_type=action_type)
    venv.reset()
    done = torch.zeros(N, dtype=torch.bool, device=venv.device)
    success = torch.zeros_like(done)
    worst = 0.0
    for t in range(100):
        host = task.demonstration_actions(venv)
        dev, ok = venv.demonstration_actions()
        err = (dev - host).abs().amax().item()
        worst = max(worst, err)
        # joint actions: the IK's inputs (the Cartesian targets) agree to 1e-12 only, so its outputs are held to the IK's own bar
        assert err <= (1e-7 if action_type == "absolute_joint_action" else 1e-12), (t, err)
        assert bool(ok.all())
        venv.step(dev)
        b = venv._buf
        success |= ~done & b["is_success"].bool()
        done |= b["step_type"] == 2
    print(action_type, "device against host policy, worst |diff|", worst)
    assert int(success.sum()) >= N // 2, int(success.sum())
    venv.close()


@gpu
def test_pointmass_device_policy_matches_host_policy_in_closed_loop():
    import mujoco_sim_amd as m

    N = 64
    task = m.PointMassReachTask(observation_type="state_observations")
    venv = m.HipVectorEnv("point_mass_reach", N, seed=3, autoreset="disabled")
    venv.reset()
    done = torch.zeros(N, dtype=torch.bool, device=venv.device)
    for t in range(50):
        host = task.demonstration_actions(venv)
        dev, _ = venv.demonstration_actions()
        assert (dev - host).abs().amax().item() <= 1e-12, t
        *_, term, trunc, info = venv.step(dev)
        done |= term
    assert done.float().mean().item() > 0.7, done.float().mean().item()
    venv.close()


# ---------------------------------------------------------------------------------------------- 4. the rollout is the loop
def _equal_blocks(a, b, keys):
    for k in keys:
        assert torch.equal(a[k], b[k]), k


@gpu
@pytest.mark.parametrize("task,kw,noise", [("robot_push_button", {"action_type": "absolute_eef_action"}, 0.0), ("robot_reach", {}, 0.0),
                                           ("point_mass_reach", {}, 0.0), ("robot_reach", {}, 0.01)])
def test_demonstration_rollout_is_the_step_by_step_loop(task, kw, noise):
    import mujoco_sim_amd as m

    N, T = 70, 60
    A, B, Cc = (m.HipVectorEnv(task, N, autoreset="next_step", **kw) for _ in range(3))
    for v in (A, B, Cc):
        v.reset(seed=11)
    gen = torch.Generator(device=A.device)
    gen.manual_seed(5)
    blk = A.demonstration_rollout(T, noise=noise, generator=gen)
    assert blk["actions"].shape == (T, N, A.action_dim) and blk["ik_ok"].shape == (T, N) and blk["ik_ok"].dtype == torch.bool
    assert torch.equal(A.flat_obs, blk["obs"][-1])
    if noise == 0.0:
        loop = {k: [] for k in FIELDS + ("actions",)}
        for t in range(T):
            a, ok = B.demonstration_actions()
            loop["actions"].append(a.clone())
            B.step(a)
            for k in FIELDS:
                loop[k].append(B._buf[k].clone())
        _equal_blocks(blk, {k: torch.stack(v) for k, v in loop.items()}, FIELDS + ("actions",))
        assert int((blk["step_type"] == 2).sum()) > 0 or task == "robot_reach"  # episodes end (and restart) inside the block
    else:  # seeded noise: repeatable bit for bit, and another seed gives other actions
        gen.manual_seed(5)
        again = B.demonstration_rollout(T, noise=noise, generator=gen)
        _equal_blocks(blk, again, FIELDS + ("actions",))
        gen.manual_seed(6)
        B.reset(seed=11)
        other = B.demonstration_rollout(T, noise=noise, generator=gen)
        assert not torch.equal(other["actions"], blk["actions"])
    replay = Cc.rollout(blk["actions"])  # the open-loop rollout of the recorded actions
    _equal_blocks(blk, replay, FIELDS)
    for v in (A, B, Cc):
        v.close()


# ---------------------------------------------------------------------------------------------- 5. Robot-Reach policy
@gpu
def test_reach_demonstration_policy_reaches_the_target():
    import mujoco_sim_amd as m

    N = 64
    venv = m.HipVectorEnv("robot_reach", N, seed=21, terminate_on_success=True)
    venv.reset()
    task = m.RobotReachTask()
    a = task.demonstration_actions(venv)
    np.testing.assert_allclose(a.cpu().numpy(), venv.flat_obs[:, 9:12].cpu().numpy(), rtol=0, atol=1e-12)  # inside the workspace the action is the target
    blk = venv.demonstration_rollout(40)
    share = blk["is_success"].bool().any(dim=0).float().mean().item()
    print("Robot-Reach success share within 40 steps:", share)
    assert share >= 0.9, share
    venv.close()
    # the single-env closure, module-level as in the reference
    from mujoco_sim_amd.environments.tasks.robot_reach import create_demonstration_policy

    env = m.make("mujoco_sim/robot_reach_state-v0")
    env.seed(1)
    env.reset()
    policy = create_demonstration_policy(env.dmc_env)
    n, ended, best = 0, False, -np.inf
    while not ended and n < 110:  # the registered task ends at its 100-step limit
        _, reward, term, trunc, _ = env.step(policy(None))
        ended, n, best = term or trunc, n + 1, max(best, reward)
    assert ended and best > -0.02, (n, best)  # dense reward = -distance: inside the 2 cm goal threshold
    env.close()


# ---------------------------------------------------------------------------------------------- 6. images
@gpu
def test_demonstration_rollout_frames_are_the_renders_before_each_step():
    import mujoco_sim_amd as m

    N, R, T = 8, 16, 12
    kw = dict(seed=3, action_type="absolute_eef_action", observation_type="visual_observations", image_resolution=R)
    A = m.HipVectorEnv("robot_push_button", N, **kw)
    B = m.HipVectorEnv("robot_push_button", N, **kw)
    A.reset()
    B.reset()
    blk = A.demonstration_rollout(T, render=True)
    assert blk["Camera/rgb_image"].shape == (T, N, R, R, 3) and blk["ur5e/Camera/rgb_image"].shape == (T, N, R, R, 3)
    for t in range(T):
        a, _ = B.demonstration_actions()
        assert torch.equal(blk["Camera/rgb_image"][t], B.render(R, R)), t
        assert torch.equal(blk["ur5e/Camera/rgb_image"][t], B.render(R, R, camera=1)), t
        B.step_flat(a)
    assert torch.equal(blk["obs"][-1], B.flat_obs)
    assert not torch.equal(blk["ur5e/Camera/rgb_image"][0], blk["ur5e/Camera/rgb_image"][-1]) and blk["Camera/rgb_image"].float().std() > 10
    A.close()
    B.close()


# ---------------------------------------------------------------------------------------------- 7. arguments
@gpu
def test_demonstration_entry_points_refuse_bad_arguments():
    import mujoco_sim_amd as m
    from mujoco_sim_amd import _native as nat

    L = nat.lib()
    INVALID, UNSUPPORTED = -1, -5

    def err(v):
        return L.mjs_last_error(v._h)

    N, T = 4, 2
    push = m.HipVectorEnv("robot_planar_push", N)
    a = torch.zeros(T, N, 8, dtype=torch.float64, device=push.device)
    obs = torch.zeros(T, N, 16, dtype=torch.float64, device=push.device)
    img = torch.zeros(T, N, 8, 8, 3, dtype=torch.uint8, device=push.device)
    s = push._stream()
    assert L.mjs_demonstration_actions(push._h, obs.data_ptr(), None, 0.0, a.data_ptr(), None, s) == UNSUPPORTED and b"teleop" in err(push)
    demo = nat.MjsDemoRollout(actions_out_dev=a.data_ptr())
    out = nat.MjsOutputs(obs=obs.data_ptr())
    assert L.mjs_rollout_demonstration(push._h, obs.data_ptr(), T, C.byref(demo), C.byref(out), s) == UNSUPPORTED and b"teleop" in err(push)
    push.close()

    reach = m.HipVectorEnv("robot_reach", N, seed=1)
    reach.reset()
    obs0, s = reach.flat_obs.clone(), reach._stream()
    call = lambda T_, demo_, out_: L.mjs_rollout_demonstration(reach._h, obs0.data_ptr(), T_, C.byref(demo_), None if out_ is None else C.byref(out_), s)  # noqa: E731
    assert call(T, demo, nat.MjsOutputs()) == INVALID and b"out->obs" in err(reach)
    assert call(T, demo, None) == INVALID and b"out->obs" in err(reach)
    assert call(T, nat.MjsDemoRollout(), out) == INVALID and b"actions_out_dev" in err(reach)
    assert call(T, nat.MjsDemoRollout(actions_out_dev=a.data_ptr(), struct_size=C.sizeof(nat.MjsDemoRollout) - 8), out) == INVALID and b"struct_size" in err(reach)
    assert call(T, nat.MjsDemoRollout(actions_out_dev=a.data_ptr(), wrist_rgb_dev=img.data_ptr(), height=8, width=8), out) == INVALID and b"wrist" in err(reach)
    assert call(T, nat.MjsDemoRollout(actions_out_dev=a.data_ptr(), scene_rgb_dev=img.data_ptr()), out) == INVALID and b"height" in err(reach)
    assert call(-1, demo, out) == INVALID and b"negative" in err(reach)
    assert call(T, nat.MjsDemoRollout(actions_out_dev=a.data_ptr(), noise=-0.1), out) == INVALID and b"noise" in err(reach)
    assert L.mjs_demonstration_actions(reach._h, None, None, 0.0, a.data_ptr(), None, s) == INVALID and b"null" in err(reach)
    # none of the refused calls stepped anything; T == 0 does nothing either
    state = reach.get_state()
    a.fill_(7.0)
    assert call(0, demo, out) == 0
    assert torch.equal(reach.get_state(), state) and bool((a == 7.0).all())
    assert reach.demonstration_rollout(0)["actions"].shape == (0, N, 3)
    assert call(T, demo, out) == 0
    torch.cuda.synchronize()
    assert not torch.equal(reach.get_state(), state) and bool((a.reshape(-1)[:T * N * 3] != 7.0).all())
    reach.close()


# ---------------------------------------------------------------------------------------------- 8. recorder (no GPU)
def test_record_rollout_writes_what_a_record_batch_loop_writes(tmp_path):
    from collections import OrderedDict

    import pyarrow.parquet as pq

    from mujoco_sim_amd.recording import LeRobotDatasetRecorder
    from mujoco_sim_amd.spaces import Box, Dict

    N, T, R = 5, 20, 4
    layout = (("ur5e/joint_configuration", 0, 6), ("unnamed_model/position", 9, 3), ("unnamed_model/active", 12, 1))  # Button-Push, joint actions

    class FakeEnv:
        single_observation_space = Dict(OrderedDict([(k, Box(-np.inf, np.inf, shape=(n,), dtype=np.float64)) for k, _, n in layout]
                                                    + [("ur5e/Camera/rgb_image", Box(0, 255, shape=(R, R, 3), dtype=np.uint8)),
                                                       ("Camera/rgb_image", Box(0, 255, shape=(R, R, 3), dtype=np.uint8))]))
        single_action_space = Box(-3.14, 3.14, shape=(7,), dtype=np.float32)
        flat_observation_layout = layout
        autoreset = "next_step"

    FIRST, MID, LAST = 0, 1, 2
    st = np.full((T, N), MID, np.uint8)
    st[4, 0] = LAST; st[5, 0] = FIRST; st[12, 0] = LAST; st[13, 0] = FIRST        # two episodes (5 and 7 frames) and an unfinished tail
    st[19, 1] = LAST                                                               # one episode filling the block
    st[0, 2] = FIRST; st[9, 2] = LAST; st[10, 2] = FIRST; st[11, 2] = LAST         # a FIRST row at the start, then a one-frame episode
    st[4, 3] = LAST; st[5, 3] = FIRST                                              # closes in the same row as env 0: the order of writing
    # env 4 never finishes: nothing is written for it
    rs = np.random.RandomState(0)
    block = {"obs": rs.standard_normal((T, N, 13)), "actions": rs.standard_normal((T, N, 7)), "reward": rs.standard_normal((T, N)),
             "is_success": (st == LAST) & (rs.uniform(size=(T, N)) < 0.7), "step_type": st,
             "Camera/rgb_image": rs.randint(0, 256, (T, N, R, R, 3)).astype(np.uint8), "ur5e/Camera/rgb_image": rs.randint(0, 256, (T, N, R, R, 3)).astype(np.uint8)}
    obs0 = rs.standard_normal((N, 13))
    seeds = [40 + i for i in range(N)]

    def as_dict(flat, t):
        d = {k: flat[:, s:s + n] for k, s, n in layout}
        d.update({k: block[k][t] for k in ("Camera/rgb_image", "ur5e/Camera/rgb_image")})
        return d

    def run(autoreset, name):
        env = FakeEnv()
        env.autoreset = autoreset
        loop = LeRobotDatasetRecorder(env, tmp_path / (name + "_loop"), "test/" + name, fps=10, task="push the button")
        done = np.zeros(N, bool)
        for t in range(T):
            active = (st[t] != FIRST) & (~done if autoreset == "disabled" else True)
            loop.record_batch(as_dict(obs0 if t == 0 else block["obs"][t - 1], t), block["actions"][t], block["reward"][t], block["is_success"][t],
                              st[t] == LAST, seeds=seeds, active=active)
            done |= (st[t] == LAST) & active
        loop.finish_recording()
        fast = LeRobotDatasetRecorder(env, tmp_path / (name + "_fast"), "test/" + name, fps=10, task="push the button")
        fast.record_rollout(block, obs0, seeds=seeds)
        fast.finish_recording()
        assert fast.n_recorded_episodes == loop.n_recorded_episodes
        for rel in ("meta/info.json", "meta/episodes.jsonl", "meta/tasks.jsonl"):
            assert (tmp_path / (name + "_fast") / rel).read_text() == (tmp_path / (name + "_loop") / rel).read_text(), rel
        for ep in range(loop.n_recorded_episodes):
            rel = f"data/chunk-000/episode_{ep:06d}.parquet"
            f, l = pq.read_table(tmp_path / (name + "_fast") / rel), pq.read_table(tmp_path / (name + "_loop") / rel)
            assert f.schema.equals(l.schema) and f.column_names == l.column_names
            for col in l.column_names:
                assert f[col].equals(l[col]), (ep, col)
        return loop.n_recorded_episodes

    assert run("next_step", "auto") == 6   # env 0: 2, env 1: 1, env 2: 2, env 3: 1
    assert run("disabled", "first") == 4   # each env's first episode only
    lengths = [len(pq.read_table(tmp_path / "auto_fast" / f"data/chunk-000/episode_{ep:06d}.parquet")) for ep in range(6)]
    assert lengths == [5, 5, 9, 1, 7, 20]  # in the order of closing: (row 4: envs 0, 3), (9: env 2), (11: env 2), (12: env 0), (19: env 1)
    tab = pq.read_table(tmp_path / "auto_fast" / "data/chunk-000/episode_000002.parquet").to_pydict()  # env 2: rows 1..9, observations of rows 0..8
    np.testing.assert_array_equal(np.asarray(tab["ur5e_joint_configuration"][0], np.float32), block["obs"][0, 2, 0:6].astype(np.float32))
    assert tab["seed"][0] == [42] and tab["observation.images.Camera_rgb_image"][0] == block["Camera/rgb_image"][1, 2].ravel().tolist()
