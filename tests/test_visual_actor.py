"""The visual actor on the device: NatureCNN feature blocks as first-layer inputs of the MLP actor (act::kernel_visual), one launch
against torch on the CPU, the closed loop render -> encoder -> actor -> step (mjs_rollout_visual_actor) against the step-by-step loop,
reloads, and the refusals of the C ABI.

Bars: test_actor_device.py's. The squashed action against the CPU float64 forward of CNN -> concatenation in input_order -> MLP on the
same frames, observations and draws: max(4 e32, 8 * 2^-24), e32 = max |float32 forward - float64 forward| measured in the test.
``actions`` against the float64 unscale of the kernel's own ``squashed``, and the rollout against the step-by-step loop: bit for bit.
"""
import ctypes as C

import pytest
import torch

from _visual_nets import SCENE, ULP, WRIST, cnn_forward, make_cnn, make_mlp, mlp_forward

gpu = pytest.mark.gpu
FIELDS = ("obs", "reward", "terminated", "truncated", "is_success", "step_type", "fault", "ncon", "discount")
R = 36  # image size of every test here: conv3's output is 1x1, n_flatten = 64
TASKS = {
    "robot_reach": ({}, (SCENE,)),
    "robot_push_button": ({"action_type": "absolute_joint_action"}, (SCENE, WRIST)),
    "point_mass_reach": ({}, (SCENE,)),
}
F_OF = {SCENE: 24, WRIST: 40}  # feature widths: neither a multiple of the packing granularities


def unscale(venv, squashed):
    low = torch.tensor(venv.action_low, dtype=torch.float64, device=squashed.device)
    high = torch.tensor(venv.action_high, dtype=torch.float64, device=squashed.device)
    return low + (0.5 * (squashed.double() + 1.0) * (high - low))  # SB3's unscale_action, in float64


def state_keys(venv):
    return [k for k, _, _ in venv.flat_observation_layout]


def make_policy(venv, cameras, widths, seed, order=None, state=True):
    """(actor, encoders by key, cnns by key, mlp, input_order): one NatureCNN per camera, an MLP over the concatenation."""
    import mujoco_sim_amd as m

    cnns = {k: make_cnn(R, R, F_OF[k], seed=seed + 10 * i, device=venv.device) for i, k in enumerate(cameras)}
    encs = {k: m.DeviceEncoder.from_sb3(venv, c, R, R) for k, c in cnns.items()}
    if order is None:
        order = (state_keys(venv) if state else []) + [k for k in venv.camera_keys if k in cameras]
    width = {k: n for k, _, n in venv.flat_observation_layout}
    in_total = sum(F_OF[k] if k in cnns else width[k] for k in order)
    net = make_mlp(in_total, widths, venv.action_dim, seed=seed + 1, device=venv.device)
    actor = m.DeviceActor.from_linears(venv, *net, encoders=encs, input_order=order)
    assert actor.in_total == in_total
    return actor, encs, cnns, net, order


def close_policy(actor, encs):
    actor.close()
    for e in encs.values():
        e.close()


def reference(venv, cnns, net, order, z, dtype):
    """The CPU forward in ``dtype`` on this handle's current frames and observations."""
    where = {k: (s, n) for k, s, n in venv.flat_observation_layout}
    parts = []
    for k in order:
        if k in cnns:
            parts.append(cnn_forward(cnns[k], venv.render(R, R, camera=0 if k == SCENE else 1), dtype))
        else:
            parts.append(venv.flat_obs[:, where[k][0]:where[k][0] + where[k][1]].cpu().to(dtype))
    return mlp_forward(net, torch.cat(parts, dim=1), z, dtype)


def check_against_torch(venv, actor, cnns, net, order, z, what):
    actions, squashed = venv.actor_actions(actor, deterministic=z is None, z=z)
    ref64, ref32 = reference(venv, cnns, net, order, z, torch.float64), reference(venv, cnns, net, order, z, torch.float32)
    e32 = (ref32.double() - ref64).abs().max().item()
    err = (squashed.cpu().double() - ref64).abs().max().item()
    bar = max(4 * e32, 8 * ULP)
    print(f"{what}: kernel vs float64 {err:.3e}, torch float32 vs float64 {e32:.3e}, bar {bar:.3e}, ratio to e32 {err / max(e32, 1e-300):.2f}")
    assert squashed.dtype == torch.float32 and actions.dtype == torch.float64
    assert err <= bar, (what, err, e32)
    assert torch.equal(actions, unscale(venv, squashed)), what
    return squashed


@pytest.fixture(scope="module")
def envs():
    """One seeded, reset handle per (task, N); the tests only read their observations and frames."""
    import mujoco_sim_amd as m

    made = {}

    def get(task, N):
        if (task, N) not in made:
            v = m.HipVectorEnv(task, N, seed=7, **TASKS[task][0])
            v.reset()
            made[task, N] = v
        return made[task, N]

    yield get
    for v in made.values():
        v.close()


# ---------------------------------------------------------------------------------------------- 4. against torch
@gpu
@pytest.mark.parametrize("widths", [[32], [64, 64]], ids=lambda w: "x".join(map(str, w)))
@pytest.mark.parametrize("N", [5, 19])
@pytest.mark.parametrize("task", ["robot_reach", "robot_push_button"])
def test_visual_actor_matches_torch(envs, task, N, widths):
    import mujoco_sim_amd as m

    venv = envs(task, N)
    cameras = TASKS[task][1]
    actor, encs, cnns, net, order = make_policy(venv, cameras, widths, seed=len(widths) * 100 + N)
    assert actor.visual and actor.in_dim == {"robot_reach": 12, "robot_push_button": 10}[task]
    check_against_torch(venv, actor, cnns, net, order, None, f"{task} N={N} {widths} deterministic")
    z = torch.randn(N, venv.action_dim, dtype=torch.float32, device=venv.device, generator=torch.Generator(device=venv.device).manual_seed(3))
    s_a = check_against_torch(venv, actor, cnns, net, order, z, f"{task} N={N} {widths} sampled")
    # the cameras first, the first layer's input columns permuted the same way: the same products in another order over k
    other = [k for k in order if k in cnns][::-1] + [k for k in order if k not in cnns]
    width = {k: n for k, _, n in venv.flat_observation_layout}
    size = lambda k: F_OF[k] if k in cnns else width[k]  # noqa: E731
    begin, pos = {}, 0
    for k in order:
        begin[k], pos = pos, pos + size(k)
    perm = [c for k in other for c in range(begin[k], begin[k] + size(k))]
    swapped = make_mlp(pos, widths, venv.action_dim, seed=len(widths) * 100 + N + 1, device=venv.device)
    with torch.no_grad():
        swapped[0][0].weight.copy_(net[0][0].weight[:, perm])
    reordered = m.DeviceActor.from_linears(venv, *swapped, encoders=encs, input_order=other)
    s_b = check_against_torch(venv, reordered, cnns, net, order, z, f"{task} N={N} {widths} cameras first")
    assert reordered.block_start != actor.block_start and (s_a - s_b).abs().max().item() < 1e-3
    reordered.close()
    close_policy(actor, encs)


@gpu
@pytest.mark.parametrize("N", [5, 19])
def test_images_only_actor_matches_torch(envs, N):
    venv = envs("robot_push_button", N)
    actor, encs, cnns, net, order = make_policy(venv, (SCENE, WRIST), [64, 64], seed=77, state=False)
    assert actor.in_dim == 0 and actor.obs_index == [] and order == [WRIST, SCENE]
    check_against_torch(venv, actor, cnns, net, order, None, f"images only N={N}")
    single, encs1, cnns1, net1, order1 = make_policy(venv, (WRIST,), [32], seed=78, state=False)  # the wrist camera alone: slot 1 without slot 0
    z = torch.randn(N, venv.action_dim, dtype=torch.float32, device=venv.device, generator=torch.Generator(device=venv.device).manual_seed(5))
    check_against_torch(venv, single, cnns1, net1, order1, z, f"wrist only N={N}")
    close_policy(actor, encs)
    close_policy(single, encs1)


# ---------------------------------------------------------------------------------------------- 5. the closed loop
def _equal_blocks(a, b, keys):
    for k in keys:
        assert torch.equal(a[k], b[k]), k


@gpu
@pytest.mark.parametrize("task,kw,N,T", [
    ("robot_reach", {}, 19, 3),
    ("robot_push_button", {"action_type": "absolute_joint_action"}, 5, 2),
    ("point_mass_reach", {"time_limit": 0.3, "autoreset": "next_step"}, 5, 8),
    ("point_mass_reach", {"time_limit": 0.3, "autoreset": "same_step"}, 5, 8),
])
def test_visual_actor_rollout_is_the_step_by_step_loop(task, kw, N, T):
    import mujoco_sim_amd as m

    handles = [m.HipVectorEnv(task, N, **kw) for _ in range(5)]
    A, B, Cc, D, E = handles
    for v in handles:
        v.reset(seed=11)
    cameras = TASKS[task][1]
    actor, encs, _, _, _ = make_policy(A, cameras, [64, 64], seed=8)  # one actor and its encoders, five handles
    image_keys = tuple(k for k in A.camera_keys if k in cameras)
    z = torch.randn(T, N, A.action_dim, dtype=torch.float32, device=A.device, generator=torch.Generator(device=A.device).manual_seed(5))
    blk = A.actor_rollout(actor, T, z=z, render=True)
    for k in image_keys:
        assert blk[k].shape == (T, N, R, R, 3) and blk[k].dtype == torch.uint8 and blk[k].float().std() > 1
    assert blk["actions"].shape == (T, N, A.action_dim) and blk["squashed_actions"].dtype == torch.float32 and "ik_ok" not in blk
    assert torch.equal(A.flat_obs, blk["obs"][-1])
    keys = FIELDS + ("actions", "squashed_actions") + image_keys
    loop = {k: [] for k in keys}
    for t in range(T):
        feats = {}
        for k in image_keys:
            frame = B.render(R, R, camera=0 if k == SCENE else 1)
            loop[k].append(frame.clone())
            feats[k] = encs[k].features(frame)  # mjs_encoder_features
        a, s = B.actor_actions(actor, z=z[t], features=feats)
        loop["actions"].append(a.clone())
        loop["squashed_actions"].append(s.clone())
        B.step(a)
        for k in FIELDS:
            loop[k].append(B._buf[k].clone())
    _equal_blocks(blk, {k: torch.stack(v) for k, v in loop.items()}, keys)
    if task == "point_mass_reach":  # 0.3 s = 3 control steps: episodes end and restart inside the block
        assert int((blk["step_type"] == 2).sum()) >= N
        assert int((blk["step_type"] == 0).sum()) >= N or kw["autoreset"] == "same_step"
    _equal_blocks(blk, Cc.rollout(blk["actions"]), FIELDS)  # the open-loop rollout of the recorded actions
    T1 = T // 2
    first, second = D.actor_rollout(actor, T1, z=z[:T1].contiguous(), render=True), D.actor_rollout(actor, T - T1, z=z[T1:].contiguous(), render=True)
    _equal_blocks(blk, {k: torch.cat([first[k], second[k]]) for k in keys}, keys)
    plain = E.actor_rollout(actor, T, z=z)  # without frames: the one-step scratch
    assert not any(k in plain for k in (SCENE, WRIST))
    _equal_blocks(blk, plain, FIELDS + ("actions", "squashed_actions"))
    a_e, s_e = E.actor_actions(actor, deterministic=True)  # renders and encodes by itself
    a_a, s_a = A.actor_actions(actor, deterministic=True)
    assert torch.equal(a_e, a_a) and torch.equal(s_e, s_a)
    assert E.actor_rollout(actor, 0)["actions"].shape == (0, N, A.action_dim)
    close_policy(actor, encs)
    for v in handles:
        v.close()


@gpu
def test_recorder_takes_a_visual_actor_rollout_block(tmp_path):
    import pyarrow.parquet as pq

    import mujoco_sim_amd as m

    N, T = 6, 8
    kw = dict(seed=2, time_limit=0.3)
    A, B = m.HipVectorEnv("point_mass_reach", N, **kw), m.HipVectorEnv("point_mass_reach", N, **kw)
    A.reset()
    B.reset()
    actor, encs, _, _, _ = make_policy(A, (SCENE,), [32], seed=12)
    fast = m.LeRobotDatasetRecorder(A, tmp_path / "fast", "test/visual_actor", fps=10, task="reach")
    obs0 = A.flat_obs.clone()
    fast.record_rollout(A.actor_rollout(actor, T, deterministic=True, render=True), obs0)
    fast.finish_recording()
    loop = m.LeRobotDatasetRecorder(B, tmp_path / "loop", "test/visual_actor", fps=10, task="reach")
    for t in range(T):
        obs = {k: v.clone() for k, v in B._obs_dict(B.flat_obs).items()}
        a, _ = B.actor_actions(actor, deterministic=True)
        b = B.step_flat(a)
        loop.record_batch(obs, a, b["reward"], b["is_success"].bool(), b["step_type"] == 2, active=b["step_type"] != 0)
    loop.finish_recording()
    assert fast.n_recorded_episodes == loop.n_recorded_episodes >= N
    for rel in ("meta/info.json", "meta/episodes.jsonl", "meta/tasks.jsonl"):
        assert (tmp_path / "fast" / rel).read_text() == (tmp_path / "loop" / rel).read_text(), rel
    for ep in range(loop.n_recorded_episodes):
        rel = f"data/chunk-000/episode_{ep:06d}.parquet"
        f, l = pq.read_table(tmp_path / "fast" / rel), pq.read_table(tmp_path / "loop" / rel)
        assert f.column_names == l.column_names
        for col in l.column_names:
            assert f[col].equals(l[col]), (ep, col)
    close_policy(actor, encs)
    A.close()
    B.close()


# ---------------------------------------------------------------------------------------------- 6. reload, sharing
@gpu
def test_load_follows_the_modules_and_handles_share_a_visual_actor():
    import mujoco_sim_amd as m

    N = 5
    one, two = m.HipVectorEnv("robot_reach", N, seed=1), m.HipVectorEnv("robot_reach", N, seed=500)
    one.reset()
    two.reset()
    actor, encs, cnns, net, order = make_policy(one, (SCENE,), [64, 64], seed=6)
    before = check_against_torch(one, actor, cnns, net, order, None, "before the update").clone()
    torch.manual_seed(60)
    with torch.no_grad():
        for p in [*cnns[SCENE].parameters(), *(q for mod in (*net[0], net[1], net[2]) for q in mod.parameters())]:
            p.add_(0.1 * torch.randn_like(p))
    _, stale = one.actor_actions(actor, deterministic=True)
    assert torch.equal(stale, before)  # the library's copies, until load()
    encs[SCENE].load()
    _, half = one.actor_actions(actor, deterministic=True)
    assert not torch.equal(half, before)  # the encoder's copy alone already moves the features
    actor.load()
    after = check_against_torch(one, actor, cnns, net, order, None, "after load()").clone()
    assert (after - before).abs().max().item() > 1e-3
    s_two = check_against_torch(two, actor, cnns, net, order, None, "the second handle")
    assert not torch.equal(s_two, after)
    _, again = one.actor_actions(actor, deterministic=True)
    assert torch.equal(again, after)
    close_policy(actor, encs)
    one.close()
    two.close()


# ---------------------------------------------------------------------------------------------- 7. refusals
@gpu
def test_visual_entry_points_refuse_bad_arguments():
    import mujoco_sim_amd as m
    from mujoco_sim_amd import _native as nat

    L = nat.lib()
    INVALID = -1
    N, T = 4, 2
    reach = m.HipVectorEnv("robot_reach", N, seed=1)
    reach.reset()
    dev = reach.device
    s = reach._stream()
    err = lambda: L.mjs_last_error(reach._h)  # noqa: E731
    index = (C.c_int32 * 12)(*range(12))

    def create(blocks_kw=None, **kw):
        base = dict(device=reach._dev_index, in_dim=12, n_hidden=1, hidden=(C.c_int32 * 3)(32, 0, 0), action_dim=3, activation=0, variant=0, obs_index=index)
        base.update(kw)
        blocks = dict(n_blocks=1, width=(C.c_int32 * 2)(24, 0), start=(C.c_int32 * 2)(12, 0))
        blocks.update(blocks_kw or {})
        a = C.c_void_p()
        rc = L.mjs_actor_create_visual(C.byref(nat.MjsActorDesc(**base)), C.byref(nat.MjsActorFeatureInputs(**blocks)), C.byref(a))
        assert (rc == 0) == bool(a.value)
        return rc, a

    pair = lambda a, b: (C.c_int32 * 2)(a, b)  # noqa: E731
    for blocks_kw, kw in ((dict(struct_size=8), {}), (dict(n_blocks=2), {}), (dict(n_blocks=0, width=pair(0, 0)), {}), (dict(width=pair(513, 0)), {}),
                          (dict(width=pair(-1, 0)), {}), (dict(start=pair(13, 0)), {}), (dict(start=pair(-1, 0)), {}),
                          (dict(n_blocks=2, width=pair(24, 40), start=pair(12, 30)), {}),  # overlapping blocks
                          ({}, dict(in_dim=65)), ({}, dict(in_dim=-1)), ({}, dict(variant=1)), ({}, dict(obs_index=None)), ({}, dict(struct_size=40)), ({}, dict(device=999))):
        rc, _ = create(blocks_kw, **kw)
        assert rc == INVALID and len(L.mjs_last_error(None)) > 0, (blocks_kw, kw)
    a0 = C.c_void_p()
    assert L.mjs_actor_create_visual(C.byref(nat.MjsActorDesc(device=0, in_dim=12, n_hidden=1, hidden=(C.c_int32 * 3)(32, 0, 0), action_dim=3, obs_index=index)), None, C.byref(a0)) == INVALID
    rc, images_only = create(dict(start=pair(0, 0)), in_dim=0, obs_index=None)  # in_dim 0 is a visual actor's right
    assert rc == 0
    L.mjs_actor_destroy(images_only)

    # a loaded visual actor (12 columns + 24 scene features), a loaded state actor, encoders
    actor, encs, _, net, _ = make_policy(reach, (SCENE,), [32], seed=1)
    enc = encs[SCENE]
    state_net = make_mlp(12, [32], 3, seed=2, device=dev)
    state_actor = m.DeviceActor.from_linears(reach, *state_net)
    wide = m.DeviceEncoder.from_sb3(reach, make_cnn(R, R, 40, seed=3, device=dev), R, R)  # F = 40, not the actor's 24
    rc, unloaded = L.mjs_encoder_create(C.byref(nat.MjsEncoderDesc(device=reach._dev_index, height=R, width=R, channels=3, features_dim=24)), C.byref(e0 := C.c_void_p())), e0
    assert rc == 0
    rc, fresh = create()  # a visual actor that was never loaded
    assert rc == 0

    low, high = reach._action_bounds()
    actions = torch.full((T, N, 3), 7.0, dtype=torch.float64, device=dev)
    obs = torch.zeros(T, N, 12, dtype=torch.float64, device=dev)
    frames = torch.zeros(T, N, R, R, 3, dtype=torch.uint8, device=dev)
    scratch = torch.zeros(N, R, R, 3, dtype=torch.uint8, device=dev)
    feats = torch.full((N, 40), 7.0, dtype=torch.float32, device=dev)
    ws = torch.zeros(N, 64, dtype=torch.float32, device=dev)
    out = nat.MjsOutputs(obs=obs.data_ptr())
    obs0 = reach.flat_obs.clone()
    fptr = lambda t: (C.c_void_p * 2)(t.data_ptr() if t is not None else None, None)  # noqa: E731

    def roll(**kw):
        base = dict(low=low, high=high, actions_out_dev=actions.data_ptr(), scene_scratch_dev=scratch.data_ptr(), features_dev=fptr(feats), workspace_dev=ws.data_ptr())
        base.update(kw)
        return nat.MjsVisualRollout(**base)

    def act_call(a, obs_=obs0, feats_=feats, low_=low, act_=actions):
        return L.mjs_actor_actions_visual(reach._h, a, obs_.data_ptr() if obs_ is not None else None, C.byref(fptr(feats_)), None, low_, high,
                                          act_.data_ptr() if act_ is not None else None, None, s)

    def roll_call(a, T_, roll_, out_=out, enc_=enc._e, wrist_=None, obs0_=obs0):
        encs_ = (C.c_void_p * 2)(enc_, wrist_)
        return L.mjs_rollout_visual_actor(reach._h, a, C.byref(encs_), obs0_.data_ptr() if obs0_ is not None else None, T_,
                                          None if roll_ is None else C.byref(roll_), None if out_ is None else C.byref(out_), s)

    va = actor._a
    # the refusals of mjs_rollout_actor / mjs_actor_actions
    assert act_call(fresh) == INVALID and b"mjs_actor_load" in err()
    assert roll_call(fresh, T, roll()) == INVALID and b"mjs_actor_load" in err()
    assert act_call(None) == INVALID and b"actor" in err()
    assert roll_call(None, T, roll()) == INVALID and b"actor" in err()
    assert act_call(va, obs_=None) == INVALID and b"null" in err()
    assert act_call(va, act_=None) == INVALID and b"null" in err()
    assert act_call(va, low_=None) == INVALID and b"low" in err()
    assert act_call(va, feats_=None) == INVALID and b"feature" in err()
    assert L.mjs_actor_actions_visual(reach._h, va, obs0.data_ptr(), None, None, low, high, actions.data_ptr(), None, s) == INVALID and b"features_dev" in err()
    assert roll_call(va, T, None) == INVALID and b"roll" in err()
    assert roll_call(va, T, roll(struct_size=C.sizeof(nat.MjsVisualRollout) - 8)) == INVALID and b"struct_size" in err()
    assert roll_call(va, -1, roll()) == INVALID and b"negative" in err()
    assert roll_call(va, T, roll(), nat.MjsOutputs()) == INVALID and b"out->obs" in err()
    assert roll_call(va, T, roll(), None) == INVALID and b"out->obs" in err()
    assert roll_call(va, T, roll(actions_out_dev=None)) == INVALID and b"actions_out_dev" in err()
    assert roll_call(va, T, roll(low=None)) == INVALID and b"low" in err()
    assert roll_call(va, T, roll(), obs0_=None) == INVALID and b"obs0_dev" in err()
    button = m.HipVectorEnv("robot_push_button", N, seed=1)  # 7 action components: not this actor's 3
    assert L.mjs_actor_actions_visual(button._h, va, obs0.data_ptr(), C.byref(fptr(feats)), None, low, high, actions.data_ptr(), None, s) == INVALID
    assert b"action" in L.mjs_last_error(button._h)
    button.close()
    # the encoders
    assert roll_call(va, T, roll(), enc_=unloaded) == INVALID and b"mjs_encoder_load" in err()
    assert roll_call(va, T, roll(), enc_=wide._e) == INVALID and b"features_dim" in err()
    assert roll_call(va, T, roll(), enc_=None) == INVALID and b"without an encoder" in err()
    assert roll_call(va, T, roll(), wrist_=enc._e) == INVALID and b"wrist" in err()
    assert roll_call(va, T, roll(wrist_rgb_dev=frames.data_ptr())) == INVALID and b"wrist" in err()
    assert L.mjs_rollout_visual_actor(reach._h, va, None, obs0.data_ptr(), T, C.byref(roll()), C.byref(out), s) == INVALID and b"enc" in err()
    if torch.cuda.device_count() > 1:  # an encoder of another device
        far = C.c_void_p()
        assert L.mjs_encoder_create(C.byref(nat.MjsEncoderDesc(device=1, height=R, width=R, channels=3, features_dim=24)), C.byref(far)) == 0
        assert roll_call(va, T, roll(), enc_=far) == INVALID and b"device" in err()
        L.mjs_encoder_destroy(far)
    # the workspaces
    assert roll_call(va, T, roll(workspace_dev=None)) == INVALID and b"workspace" in err()
    assert roll_call(va, T, roll(features_dev=fptr(None))) == INVALID and b"feature" in err()
    assert roll_call(va, T, roll(scene_scratch_dev=None)) == INVALID and b"scratch" in err()
    # a state actor at the visual entry points, a visual actor at the state actor's
    assert act_call(state_actor._a) == INVALID and b"mjs_actor_create" in err()
    assert roll_call(state_actor._a, T, roll()) == INVALID and b"mjs_actor_create" in err()
    assert L.mjs_actor_actions(reach._h, va, obs0.data_ptr(), None, low, high, actions.data_ptr(), None, s) == INVALID and b"mjs_actor_create_visual" in err()
    state_roll = nat.MjsActorRollout(low=low, high=high, actions_out_dev=actions.data_ptr())
    assert L.mjs_rollout_actor(reach._h, va, obs0.data_ptr(), T, C.byref(state_roll), C.byref(out), s) == INVALID and b"mjs_actor_create_visual" in err()
    # none of the refused calls launched anything, T == 0 does nothing, and the handle is still usable
    state = reach.get_state()
    torch.cuda.synchronize()
    assert bool((actions == 7.0).all()) and bool((feats == 7.0).all()) and bool((obs == 0).all()) and bool((scratch == 0).all())
    assert roll_call(va, 0, roll()) == 0
    assert torch.equal(reach.get_state(), state) and bool((actions == 7.0).all())
    assert roll_call(va, T, roll(scene_scratch_dev=None, scene_rgb_dev=frames.data_ptr())) == 0  # frames kept: no scratch needed
    assert act_call(va) == 0
    torch.cuda.synchronize()
    assert not torch.equal(reach.get_state(), state) and bool((actions != 7.0).all()) and frames.float().std() > 1
    L.mjs_actor_destroy(fresh)
    L.mjs_encoder_destroy(unloaded)
    wide.close()
    state_actor.close()
    close_policy(actor, encs)
    reach.close()
