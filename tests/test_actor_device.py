"""The MLP actor on the device (csrc/mjs_actor.h, mujoco_sim_amd/policies.py): one launch against torch, the closed-loop rollout
(mjs_rollout_actor) against the step-by-step loop, and the argument checks.

Bars. The kernel is float32 with float32 accumulation (an fmaf chain over k on the f32-input MFMA), torch's own float32 forward is
another float32 accumulation of the same length in another order, so both sit at the same order of distance from the float64
forward of the same module on the same observations and draws. The yardstick e32 = max |torch float32 - torch float64| is measured
in the test; the bar is max(4 e32, 8 * 2^-24) (the floor covers an accidentally tiny e32; 2^-24 is half a float32 ulp below 1, the
largest magnitude a squashed action has). ``actions`` against the float64 unscale of the kernel's own ``squashed``: bit for bit. The
rollout against the step-by-step loop: bit for bit (the same launches on the same data).
"""
import ctypes as C
import math
import re
from pathlib import Path

import numpy as np
import pytest
import torch

gpu = pytest.mark.gpu
ROOT = Path(__file__).resolve().parents[1]
FIELDS = ("obs", "reward", "terminated", "truncated", "is_success", "step_type", "fault", "ncon", "discount")
ULP = 2.0 ** -24
WIDTHS = ([32], [48], [64, 64], [256, 256], [64, 32, 96])
# task name -> (constructor arguments, obs_index or None for the env's own keys): in_dim 4 / 12 / 13, A 2 / 3 / 7
TASK_CASES = {
    "point_mass_reach": ({}, None),
    "robot_reach": ({}, None),
    "robot_push_button": ({"action_type": "absolute_joint_action"}, list(range(13))),
}


# ---------------------------------------------------------------------------------------------- torch side
def make_net(in_dim, widths, A, seed, device="cpu", dtype=torch.float32):
    """(hidden, mu, log_std): default Linear init from torch.manual_seed(seed)."""
    torch.manual_seed(seed)
    hidden, d = [], in_dim
    for w in widths:
        hidden.append(torch.nn.Linear(d, w))
        d = w
    mu, log_std = torch.nn.Linear(d, A), torch.nn.Linear(d, A)
    for m in (*hidden, mu, log_std):
        m.to(device=device, dtype=dtype)
    return hidden, mu, log_std


def torch_forward(net, x, z, activation, dtype):
    """SAC's actor in ``dtype``: the squashed action of the module's parameters cast to dtype."""
    hidden, mu, log_std = net
    f = torch.relu if activation == "relu" else torch.tanh
    lin = lambda m, h: torch.nn.functional.linear(h, m.weight.detach().to(dtype), m.bias.detach().to(dtype))  # noqa: E731
    h = x.to(dtype)
    for m in hidden:
        h = f(lin(m, h))
    u, ls = lin(mu, h), lin(log_std, h).clamp(-20.0, 2.0)
    if z is not None:
        u = u + ls.exp() * z.to(dtype)
    return torch.tanh(u)


def unscale(venv, squashed):
    low = torch.tensor(venv.action_low, dtype=torch.float64, device=squashed.device)
    high = torch.tensor(venv.action_high, dtype=torch.float64, device=squashed.device)
    return low + (0.5 * (squashed.double() + 1.0) * (high - low))  # SB3's unscale_action, in float64


def check_against_torch(venv, actor, net, activation, cols, z, what=""):
    """Test 1's comparison for the env's current observations; returns (error, e32)."""
    actions, squashed = venv.actor_actions(actor, deterministic=z is None, z=z)
    x = venv.flat_obs[:, cols]
    ref64 = torch_forward(net, x, z, activation, torch.float64)
    ref32 = torch_forward(net, x, z, activation, torch.float32)
    e32 = (ref32.double() - ref64).abs().max().item()
    err = (squashed.double() - ref64).abs().max().item()
    bar = max(4 * e32, 8 * ULP)
    print(f"{what}: kernel vs float64 {err:.3e}, torch float32 vs float64 {e32:.3e}, bar {bar:.3e}, ratio to e32 {err / max(e32, 1e-300):.2f}")
    assert squashed.dtype == torch.float32 and actions.dtype == torch.float64
    assert err <= bar, (what, err, e32)
    assert torch.equal(actions, unscale(venv, squashed)), what
    return err, e32


def columns(venv, obs_index):
    if obs_index is not None:
        return list(obs_index)
    return [c for _, s, n in venv.flat_observation_layout for c in range(s, s + n)]


@pytest.fixture(scope="module")
def envs():
    """One seeded, reset handle per (task, N); the tests only read their observations (or restore what they overwrite)."""
    import mujoco_sim_amd as m

    made = {}

    def get(task, N):
        if (task, N) not in made:
            v = m.HipVectorEnv(task, N, seed=7, **TASK_CASES.get(task, ({}, None))[0])
            v.reset()
            made[task, N] = v
        return made[task, N]

    yield get
    for v in made.values():
        v.close()


# ---------------------------------------------------------------------------------------------- 1. against torch
@gpu
@pytest.mark.parametrize("activation", ["relu", "tanh"])
@pytest.mark.parametrize("widths", WIDTHS, ids=lambda w: "x".join(map(str, w)))
@pytest.mark.parametrize("N", [33, 96])
@pytest.mark.parametrize("task", list(TASK_CASES))
def test_actor_matches_torch(envs, task, N, widths, activation):
    from mujoco_sim_amd import DeviceActor

    venv = envs(task, N)
    obs_index = TASK_CASES[task][1]
    cols = columns(venv, obs_index)
    net = make_net(len(cols), widths, venv.action_dim, seed=len(widths) * 1000 + widths[0], device=venv.device)
    actor = DeviceActor.from_linears(venv, *net, activation=activation, obs_index=obs_index)
    assert actor.in_dim == {"point_mass_reach": 4, "robot_reach": 12, "robot_push_button": 13}[task]
    check_against_torch(venv, actor, net, activation, cols, None, f"{task} N={N} {widths} {activation} deterministic")
    z = torch.randn(N, venv.action_dim, dtype=torch.float32, device=venv.device, generator=torch.Generator(device=venv.device).manual_seed(3))
    check_against_torch(venv, actor, net, activation, cols, z, f"{task} N={N} {widths} {activation} sampled")
    actor.close()


@gpu
@pytest.mark.parametrize("widths", [[48], [256, 256]], ids=lambda w: "x".join(map(str, w)))
def test_the_32_env_tile_variant_matches_torch_too(envs, widths):
    """The A/B variant (32 envs per workgroup on the 32x32x2 instruction; 256-wide layers take its LDS past 64 KB)."""
    from mujoco_sim_amd import DeviceActor
    from mujoco_sim_amd import _native as nat

    venv = envs("robot_reach", 96)
    cols = columns(venv, None)
    net = make_net(12, widths, 3, seed=5, device=venv.device)
    actor = DeviceActor.from_linears(venv, *net, activation="tanh", variant=nat.ACTOR_VARIANT_TILE32)
    z = torch.randn(96, 3, dtype=torch.float32, device=venv.device, generator=torch.Generator(device=venv.device).manual_seed(4))
    check_against_torch(venv, actor, net, "tanh", cols, z, f"tile32 {widths}")
    small = envs("robot_reach", 33)
    check_against_torch(small, actor, net, "tanh", cols, None, f"tile32 {widths} N=33")
    actor.close()


# ---------------------------------------------------------------------------------------------- 2. known answers
@gpu
@pytest.mark.parametrize("task", ["point_mass_reach", "robot_push_button"])
def test_known_answers_and_the_log_std_clamp(envs, task):
    from mujoco_sim_amd import DeviceActor

    venv = envs(task, 33)
    N, A = 33, venv.action_dim
    net = make_net(len(columns(venv, None)), [48], A, seed=1, device=venv.device)
    hidden, mu, log_std = net
    b_mu = math.atanh(0.5)
    with torch.no_grad():
        for m in (*hidden, mu, log_std):
            m.weight.zero_()
            m.bias.zero_()
        mu.bias.fill_(b_mu)
    actor = DeviceActor.from_linears(venv, *net)
    actions, squashed = venv.actor_actions(actor, deterministic=True)
    assert (squashed.double() - 0.5).abs().max().item() <= 2 * ULP
    low, high = (torch.tensor(b, dtype=torch.float64, device=venv.device) for b in (venv.action_low, venv.action_high))
    want = (low + 0.75 * (high - low)).expand(N, A)
    assert ((actions - want).abs() <= 2 * ULP * 0.5 * (high - low) + 1e-15).all()  # the squashed action's 2 ulp through the affine map
    assert torch.equal(actions, unscale(venv, squashed))
    # the clamp: log_std = +10 acts as 2, -30 as -20 (z = 1); b_mu as float32, the number the kernel adds to
    ones = torch.ones(N, A, dtype=torch.float32, device=venv.device)
    mu32 = float(np.float32(b_mu))
    for b_ls, clamped in ((10.0, 2.0), (-30.0, -20.0)):
        with torch.no_grad():
            log_std.bias.fill_(b_ls)
        actor.load()
        _, squashed = venv.actor_actions(actor, z=ones)
        want = math.tanh(mu32 + math.exp(clamped))
        assert (squashed.double() - want).abs().max().item() <= 2 * ULP, (b_ls, squashed[0], want)
    # (an unclamped +10 would be seen: tanh would be exactly 1, more than 4 ulp away; e^-20 and e^-30 both vanish next to mu in float32)
    assert abs(math.tanh(mu32 + math.exp(10.0)) - math.tanh(mu32 + math.exp(2.0))) > 4 * ULP
    actor.close()


# ---------------------------------------------------------------------------------------------- 3. tile independence
@gpu
@pytest.mark.parametrize("widths", [[48], [256, 256]], ids=lambda w: "x".join(map(str, w)))
def test_rows_are_independent_of_their_tile(envs, widths):
    from mujoco_sim_amd import DeviceActor

    big, small = envs("robot_reach", 96), envs("robot_reach", 33)
    assert torch.equal(big.flat_obs[:33], small.flat_obs)  # env i is seeded with seed + i
    net = make_net(12, widths, 3, seed=2, device=big.device)
    actor = DeviceActor.from_linears(big, *net, activation="tanh")
    z = torch.randn(96, 3, dtype=torch.float32, device=big.device, generator=torch.Generator(device=big.device).manual_seed(9))
    a96, s96 = big.actor_actions(actor, z=z)
    a33, s33 = small.actor_actions(actor, z=z[:33].contiguous())
    assert torch.equal(a33, a96[:33]) and torch.equal(s33, s96[:33])
    perm = torch.randperm(96, device=big.device, generator=torch.Generator(device=big.device).manual_seed(1))
    keep = big.flat_obs.clone()
    big.flat_obs.copy_(keep[perm])
    ap, sp = big.actor_actions(actor, z=z[perm].contiguous())
    big.flat_obs.copy_(keep)
    assert torch.equal(ap, a96[perm]) and torch.equal(sp, s96[perm])
    actor.close()


# ---------------------------------------------------------------------------------------------- 4. obs_keys
@gpu
@pytest.mark.parametrize("N", [33, 96])
def test_obs_keys_select_and_order_the_columns(envs, N):
    from mujoco_sim_amd import DeviceActor

    venv = envs("robot_reach", N)
    keys = ("ur5e/tcp_position", "target_position")  # the reference's STATE observation of Robot-Reach
    cols = [0, 1, 2, 9, 10, 11]
    net = make_net(6, [64, 64], 3, seed=4, device=venv.device)
    actor = DeviceActor.from_linears(venv, *net, obs_keys=keys)
    assert actor.obs_index == cols and actor.in_dim == 6
    check_against_torch(venv, actor, net, "relu", cols, None, f"obs_keys N={N}")
    _, s_a = venv.actor_actions(actor, deterministic=True)
    # the other key order with the first layer's input columns permuted the same way: the same products. The kernel sums them over
    # k in another order, so the two agree to the bar of test 1, not bit for bit
    swapped = make_net(6, [64, 64], 3, seed=4, device=venv.device)
    with torch.no_grad():
        swapped[0][0].weight.copy_(net[0][0].weight[:, [3, 4, 5, 0, 1, 2]])
    other = DeviceActor.from_linears(venv, *swapped, obs_keys=keys[::-1])
    assert other.obs_index == [9, 10, 11, 0, 1, 2]
    check_against_torch(venv, other, net, "relu", cols, None, f"obs_keys reordered N={N}")
    _, s_b = venv.actor_actions(other, deterministic=True)
    ref64 = torch_forward(net, venv.flat_obs[:, cols], None, "relu", torch.float64)
    e32 = (torch_forward(net, venv.flat_obs[:, cols], None, "relu", torch.float32).double() - ref64).abs().max().item()
    assert (s_a.double() - s_b.double()).abs().max().item() <= 2 * max(4 * e32, 8 * ULP)  # each within the bar of the same reference
    actor.close()
    other.close()


# ---------------------------------------------------------------------------------------------- 5. the closed loop
def _equal_blocks(a, b, keys):
    for k in keys:
        assert torch.equal(a[k], b[k]), k


@gpu
@pytest.mark.parametrize("task,kw,N,T,widths", [
    ("robot_reach", {}, 96, 5, [64, 64]),
    ("robot_push_button", {"action_type": "absolute_joint_action"}, 33, 4, [64, 32, 96]),
    ("robot_planar_push", {}, 33, 2, [32]),
    ("point_mass_reach", {"time_limit": 0.3, "autoreset": "next_step"}, 33, 8, [48]),
    ("point_mass_reach", {"time_limit": 0.3, "autoreset": "same_step"}, 33, 8, [48]),
])
def test_actor_rollout_is_the_step_by_step_loop(task, kw, N, T, widths):
    import mujoco_sim_amd as m

    envs_ = [m.HipVectorEnv(task, N, **kw) for _ in range(4)]
    A, B, Cc, D = envs_
    for v in envs_:
        v.reset(seed=11)
    net = make_net(A.obs_dim, widths, A.action_dim, seed=8, device=A.device)
    actor = m.DeviceActor.from_linears(A, *net, activation="tanh", obs_index=list(range(A.obs_dim)))  # one actor, four handles
    z = torch.randn(T, N, A.action_dim, dtype=torch.float32, device=A.device, generator=torch.Generator(device=A.device).manual_seed(5))
    blk = A.actor_rollout(actor, T, z=z)
    assert blk["actions"].shape == (T, N, A.action_dim) and blk["squashed_actions"].shape == (T, N, A.action_dim)
    assert blk["squashed_actions"].dtype == torch.float32 and "ik_ok" not in blk
    assert torch.equal(A.flat_obs, blk["obs"][-1])
    keys = FIELDS + ("actions", "squashed_actions")
    loop = {k: [] for k in keys}
    for t in range(T):
        a, s = B.actor_actions(actor, z=z[t])
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
    first, second = D.actor_rollout(actor, T1, z=z[:T1].contiguous()), D.actor_rollout(actor, T - T1, z=z[T1:].contiguous())
    _equal_blocks(blk, {k: torch.cat([first[k], second[k]]) for k in keys}, keys)
    det = D.actor_rollout(actor, 1, deterministic=True)
    assert det["actions"].shape == (1, N, A.action_dim) and D.actor_rollout(actor, 0)["actions"].shape == (0, N, A.action_dim)
    actor.close()
    for v in envs_:
        v.close()


# ---------------------------------------------------------------------------------------------- 6. reload, sharing
@gpu
def test_load_follows_the_modules_and_handles_share_an_actor():
    import mujoco_sim_amd as m

    N = 33
    one, two = m.HipVectorEnv("robot_reach", N, seed=1), m.HipVectorEnv("robot_reach", N, seed=500)
    one.reset()
    two.reset()
    cols = list(range(12))
    net = make_net(12, [64, 64], 3, seed=6, device=one.device)
    actor = m.DeviceActor.from_linears(one, *net)
    check_against_torch(one, actor, net, "relu", cols, None, "before the update")
    _, before = one.actor_actions(actor, deterministic=True)
    torch.manual_seed(60)
    with torch.no_grad():
        for mod in (*net[0], net[1], net[2]):
            mod.weight.add_(0.2 * torch.randn_like(mod.weight))
            mod.bias.add_(0.2 * torch.randn_like(mod.bias))
    _, stale = one.actor_actions(actor, deterministic=True)
    assert torch.equal(stale, before)  # the library's copy, until load()
    actor.load()
    check_against_torch(one, actor, net, "relu", cols, None, "after load()")
    _, after = one.actor_actions(actor, deterministic=True)
    assert (after - before).abs().max().item() > 1e-3
    check_against_torch(two, actor, net, "relu", cols, None, "the second handle")
    _, s_two = two.actor_actions(actor, deterministic=True)
    assert not torch.equal(s_two, after)
    _, again = one.actor_actions(actor, deterministic=True)
    assert torch.equal(again, after)
    actor.close()
    one.close()
    two.close()


# ---------------------------------------------------------------------------------------------- 7. frames, recorder
@gpu
def test_actor_rollout_frames_are_the_renders_before_each_step():
    import mujoco_sim_amd as m

    N, R, T = 8, 16, 2
    kw = dict(seed=3, action_type="absolute_joint_action", observation_type="visual_observations", image_resolution=R)
    A, B = m.HipVectorEnv("robot_push_button", N, **kw), m.HipVectorEnv("robot_push_button", N, **kw)
    A.reset()
    B.reset()
    net = make_net(10, [32], 7, seed=3, device=A.device)
    actor = m.DeviceActor.from_linears(A, *net, obs_index=[0, 1, 2, 3, 4, 5, 9, 10, 11, 12])
    blk = A.actor_rollout(actor, T, deterministic=True, render=True)
    assert blk["Camera/rgb_image"].shape == (T, N, R, R, 3) and blk["ur5e/Camera/rgb_image"].shape == (T, N, R, R, 3)
    for t in range(T):
        a, _ = B.actor_actions(actor, deterministic=True)
        assert torch.equal(blk["Camera/rgb_image"][t], B.render(R, R)), t
        assert torch.equal(blk["ur5e/Camera/rgb_image"][t], B.render(R, R, camera=1)), t
        B.step_flat(a)
    assert torch.equal(blk["obs"][-1], B.flat_obs) and blk["Camera/rgb_image"].float().std() > 10
    actor.close()
    A.close()
    B.close()


@gpu
def test_recorder_takes_an_actor_rollout_block(tmp_path):
    import pyarrow.parquet as pq

    import mujoco_sim_amd as m

    N, T = 6, 8
    kw = dict(seed=2, time_limit=0.3)
    A, B = m.HipVectorEnv("point_mass_reach", N, **kw), m.HipVectorEnv("point_mass_reach", N, **kw)
    A.reset()
    B.reset()
    net = make_net(4, [32], 2, seed=12, device=A.device)
    actor = m.DeviceActor.from_linears(A, *net)
    fast = m.LeRobotDatasetRecorder(A, tmp_path / "fast", "test/actor", fps=10, task="reach")
    obs0 = A.flat_obs.clone()
    fast.record_rollout(A.actor_rollout(actor, T, deterministic=True), obs0)
    fast.finish_recording()
    loop = m.LeRobotDatasetRecorder(B, tmp_path / "loop", "test/actor", fps=10, task="reach")
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
    actor.close()
    A.close()
    B.close()


# ---------------------------------------------------------------------------------------------- 8. refusals
@gpu
def test_actor_entry_points_refuse_bad_arguments():
    import mujoco_sim_amd as m
    from mujoco_sim_amd import _native as nat

    L = nat.lib()
    INVALID = -1
    N, T = 4, 2
    reach = m.HipVectorEnv("robot_reach", N, seed=1)
    reach.reset()
    dev = reach.device
    index = (C.c_int32 * 12)(*range(12))

    def desc(**kw):
        base = dict(device=reach._dev_index, in_dim=12, n_hidden=2, hidden=(C.c_int32 * 3)(64, 64, 0), action_dim=3, activation=0, variant=0, obs_index=index)
        base.update(kw)
        return nat.MjsActorDesc(**base)

    def create(**kw):
        a = C.c_void_p()
        rc = L.mjs_actor_create(C.byref(desc(**kw)), C.byref(a))
        assert (rc == 0) == bool(a.value)
        return rc, a

    bad_index = (C.c_int32 * 12)(*([0] * 11 + [-1]))
    for kw in (dict(struct_size=C.sizeof(nat.MjsActorDesc) - 8), dict(in_dim=0), dict(in_dim=65), dict(n_hidden=0), dict(n_hidden=4),
               dict(hidden=(C.c_int32 * 3)(64, 257, 0)), dict(hidden=(C.c_int32 * 3)(0, 64, 0)), dict(action_dim=0), dict(action_dim=9),
               dict(activation=2), dict(variant=5), dict(obs_index=None), dict(obs_index=bad_index), dict(device=999)):
        rc, _ = create(**kw)
        assert rc == INVALID and len(L.mjs_last_error(None)) > 0, kw
    assert L.mjs_actor_create(None, None) == INVALID

    err = lambda: L.mjs_last_error(reach._h)  # noqa: E731
    s = reach._stream()
    low, high = reach._action_bounds()
    actions = torch.full((T, N, 3), 7.0, dtype=torch.float64, device=dev)
    obs = torch.zeros(T, N, 12, dtype=torch.float64, device=dev)
    img = torch.zeros(T, N, 8, 8, 3, dtype=torch.uint8, device=dev)
    out = nat.MjsOutputs(obs=obs.data_ptr())
    obs0 = reach.flat_obs.clone()
    roll = lambda **kw: nat.MjsActorRollout(**{**dict(low=low, high=high, actions_out_dev=actions.data_ptr()), **kw})  # noqa: E731

    def act_call(actor, obs_=obs0, low_=low, act_=actions):
        return L.mjs_actor_actions(reach._h, actor, obs_.data_ptr() if obs_ is not None else None, None, low_, high, act_.data_ptr() if act_ is not None else None, None, s)

    def roll_call(actor, T_, roll_, out_=out):
        return L.mjs_rollout_actor(reach._h, actor, obs0.data_ptr(), T_, None if roll_ is None else C.byref(roll_), None if out_ is None else C.byref(out_), s)

    # before the first load
    rc, fresh = create()
    assert rc == 0
    assert act_call(fresh) == INVALID and b"mjs_actor_load" in err()
    assert roll_call(fresh, T, roll()) == INVALID and b"mjs_actor_load" in err()
    net = make_net(12, [64, 64], 3, seed=1, device=dev)
    w = nat.MjsActorWeights(hidden_w=(C.c_void_p * 3)(net[0][0].weight.data_ptr(), net[0][1].weight.data_ptr()),
                            hidden_b=(C.c_void_p * 3)(net[0][0].bias.data_ptr(), net[0][1].bias.data_ptr()),
                            mu_w=net[1].weight.data_ptr(), mu_b=net[1].bias.data_ptr(), log_std_w=net[2].weight.data_ptr(), log_std_b=net[2].bias.data_ptr())
    assert L.mjs_actor_load(fresh, C.byref(nat.MjsActorWeights(struct_size=8)), s) == INVALID and b"struct_size" in L.mjs_last_error(None)
    assert L.mjs_actor_load(fresh, C.byref(nat.MjsActorWeights()), s) == INVALID and b"null" in L.mjs_last_error(None)
    assert L.mjs_actor_load(fresh, None, s) == INVALID and L.mjs_actor_load(None, C.byref(w), s) == INVALID
    assert act_call(fresh) == INVALID  # the refused loads loaded nothing
    assert L.mjs_actor_load(fresh, C.byref(w), s) == 0
    # an actor that does not fit this handle: action width, observation columns
    for kw, text in ((dict(action_dim=2), b"action"), (dict(obs_index=(C.c_int32 * 12)(*([0] * 11 + [12]))), b"obs_index")):
        rc, other = create(**kw)
        assert rc == 0 and L.mjs_actor_load(other, C.byref(w), s) == 0  # (shapes of w do not matter: nothing is launched with it)
        torch.cuda.synchronize()
        assert act_call(other) == INVALID and text in err()
        assert roll_call(other, T, roll()) == INVALID and text in err()
        L.mjs_actor_destroy(other)
    if torch.cuda.device_count() > 1:  # an actor of another device
        rc, far = create(device=1)
        assert rc == 0
        assert act_call(far) == INVALID and b"device" in err()
        L.mjs_actor_destroy(far)
    # null pointers, T, struct sizes, image buffers
    assert act_call(None) == INVALID and b"actor" in err()
    assert act_call(fresh, obs_=None) == INVALID and b"null" in err()
    assert act_call(fresh, act_=None) == INVALID and b"null" in err()
    assert act_call(fresh, low_=None) == INVALID and b"low" in err()
    assert L.mjs_actor_actions(None, fresh, obs0.data_ptr(), None, low, high, actions.data_ptr(), None, s) == INVALID
    assert roll_call(None, T, roll()) == INVALID and b"actor" in err()
    assert roll_call(fresh, T, None) == INVALID and b"roll" in err()
    assert roll_call(fresh, T, roll(struct_size=C.sizeof(nat.MjsActorRollout) - 8)) == INVALID and b"struct_size" in err()
    assert roll_call(fresh, -1, roll()) == INVALID and b"negative" in err()
    assert roll_call(fresh, T, roll(), nat.MjsOutputs()) == INVALID and b"out->obs" in err()
    assert roll_call(fresh, T, roll(), None) == INVALID and b"out->obs" in err()
    assert roll_call(fresh, T, roll(actions_out_dev=None)) == INVALID and b"actions_out_dev" in err()
    assert roll_call(fresh, T, roll(low=None)) == INVALID and b"low" in err()
    assert roll_call(fresh, T, roll(wrist_rgb_dev=img.data_ptr(), height=8, width=8)) == INVALID and b"wrist" in err()
    assert roll_call(fresh, T, roll(scene_rgb_dev=img.data_ptr())) == INVALID and b"height" in err()
    assert L.mjs_rollout_actor(reach._h, fresh, None, T, C.byref(roll()), C.byref(out), s) == INVALID and b"obs0_dev" in err()
    # none of the refused calls launched anything, T == 0 does nothing, and the handle is still usable
    state = reach.get_state()
    torch.cuda.synchronize()
    assert bool((actions == 7.0).all())
    assert roll_call(fresh, 0, roll()) == 0
    assert torch.equal(reach.get_state(), state) and bool((actions == 7.0).all())
    assert act_call(fresh) == 0 and roll_call(fresh, T, roll()) == 0
    torch.cuda.synchronize()
    assert not torch.equal(reach.get_state(), state) and bool((actions != 7.0).all())
    L.mjs_actor_destroy(fresh)
    L.mjs_actor_destroy(None)
    reach.close()


# ---------------------------------------------------------------------------------------------- CPU: header, binding, argument checks
def test_header_declares_and_library_exports_the_actor_entry_points():
    from mujoco_sim_amd import _native as nat

    nat.build()
    header = (ROOT / "include" / "mjsim.h").read_text()
    names = ("mjs_actor_create", "mjs_actor_destroy", "mjs_actor_load", "mjs_actor_actions", "mjs_rollout_actor")
    L = C.CDLL(str(nat.LIB_PATH))
    for name in names:
        assert re.search(rf"\b{name}\s*\(", header), name
        assert name in nat.EXPORTED_SYMBOLS and hasattr(L, name), name
    assert "#define MJS_ABI_VERSION 3" in header  # entry points added after abi 3 leave the number alone


def test_binding_struct_sizes_are_the_header_s():
    from mujoco_sim_amd import _native as nat

    header = (ROOT / "include" / "mjsim.h").read_text()
    for c_name, binding in (("mjs_actor_desc", nat.MjsActorDesc), ("mjs_actor_weights", nat.MjsActorWeights), ("mjs_actor_rollout", nat.MjsActorRollout)):
        stated = re.search(rf"\}}\s*{c_name};\s*/\*\s*(\d+) bytes\s*\*/", header)
        assert stated, c_name
        assert int(stated.group(1)) == C.sizeof(binding), c_name
        assert binding().struct_size == C.sizeof(binding)
    assert [n for n, _ in nat.MjsActorDesc._fields_] == ["struct_size", "device", "in_dim", "n_hidden", "hidden", "action_dim", "activation", "variant", "obs_index"]
    assert nat.MjsActorDesc.obs_index.offset == 40 and nat.MjsActorWeights.mu_w.offset == 56 and nat.MjsActorRollout.actions_out_dev.offset == 40


class _StubEnv:
    """What DeviceActor reads of a HipVectorEnv before it touches the native layer (Robot-Reach's layout, on the CPU)."""
    device = torch.device("cpu")
    _dev_index = 0
    action_dim = 3
    obs_dim = 12
    flat_observation_layout = (("ur5e/tcp_position", 0, 3), ("ur5e/joint_configuration", 3, 6), ("target_position", 9, 3))


@pytest.fixture
def no_native(monkeypatch):
    from mujoco_sim_amd import _native as nat

    def touched(*a, **k):
        raise AssertionError("the native layer was touched")

    monkeypatch.setattr(nat, "lib", touched)
    monkeypatch.setattr(nat, "check", touched)


def test_device_actor_checks_its_arguments_before_any_native_call(no_native):
    from mujoco_sim_amd import DeviceActor

    venv = _StubEnv()
    good = lambda: make_net(12, [64, 64], 3, seed=0)  # noqa: E731
    with pytest.raises(AssertionError, match="native layer"):  # valid arguments reach the (patched) native layer: the checks below stop earlier
        DeviceActor.from_linears(venv, *good())
    with pytest.raises(ValueError, match="float32"):
        DeviceActor.from_linears(venv, *make_net(12, [64, 64], 3, seed=0, dtype=torch.float64))
    with pytest.raises(ValueError, match="live on"):
        DeviceActor.from_linears(venv, *make_net(12, [64], 3, seed=0, device="meta"))
    with pytest.raises(ValueError, match="unknown observation key"):
        DeviceActor.from_linears(venv, *good(), obs_keys=("ur5e/tcp_position", "goal"))
    with pytest.raises(ValueError, match="expected"):  # first layer reads 12 columns, the keys give 6
        DeviceActor.from_linears(venv, *good(), obs_keys=("ur5e/tcp_position", "target_position"))
    hidden, mu, log_std = good()
    with pytest.raises(ValueError, match="expected"):
        DeviceActor.from_linears(venv, hidden, torch.nn.Linear(64, 2), log_std)  # action width
    with pytest.raises(ValueError, match="expected"):
        DeviceActor.from_linears(venv, [hidden[0], torch.nn.Linear(32, 64)], mu, log_std)  # chain
    with pytest.raises(ValueError, match="outside"):
        DeviceActor.from_linears(venv, *make_net(12, [257], 3, seed=0))
    with pytest.raises(ValueError, match="hidden layers"):
        DeviceActor.from_linears(venv, [], mu, log_std)
    with pytest.raises(ValueError, match="hidden layers"):
        DeviceActor.from_linears(venv, *make_net(12, [8, 8, 8, 8], 3, seed=0))
    with pytest.raises(ValueError, match="activation"):
        DeviceActor.from_linears(venv, *good(), activation="gelu")
    with pytest.raises(ValueError, match="not a Linear"):
        DeviceActor.from_linears(venv, [torch.nn.ReLU()], mu, log_std)
    with pytest.raises(ValueError, match="without bias"):
        DeviceActor.from_linears(venv, [torch.nn.Linear(12, 64, bias=False), hidden[1]], mu, log_std)
    with pytest.raises(ValueError, match="obs_index"):
        DeviceActor.from_linears(venv, *good(), obs_index=list(range(1, 13)))
    with pytest.raises(ValueError, match="not both"):
        DeviceActor.from_linears(venv, *good(), obs_keys=("target_position",), obs_index=[0])
    with pytest.raises(ValueError, match="observation columns"):
        DeviceActor.from_linears(venv, *make_net(72, [8], 3, seed=0), obs_index=list(range(12)) * 6)


class _SacActorStandIn(torch.nn.Module):
    """The attributes of stable_baselines3.sac.policies.Actor that from_sb3 reads (SB3 itself is not installed here)."""

    def __init__(self, in_dim, net_arch, A, activation_fn=torch.nn.ReLU):
        super().__init__()
        layers, d = [], in_dim
        for w in net_arch:
            layers += [torch.nn.Linear(d, w), activation_fn()]
            d = w
        self.latent_pi = torch.nn.Sequential(*layers)
        self.mu = torch.nn.Linear(d, A)
        self.log_std = torch.nn.Linear(d, A)


def test_from_sb3_reads_a_sac_shaped_actor(no_native, monkeypatch):
    from mujoco_sim_amd import DeviceActor

    venv = _StubEnv()
    seen = {}

    def init(self, venv_, hidden, mu, log_std, activation="relu", obs_keys=None, **kw):
        seen.update(hidden=hidden, mu=mu, log_std=log_std, activation=activation, obs_keys=obs_keys)

    sac = _SacActorStandIn(12, [64, 32], 3, torch.nn.Tanh)
    with monkeypatch.context() as mp:
        mp.setattr(DeviceActor, "__init__", init)
        DeviceActor.from_sb3(venv, sac, obs_keys=("target_position",))
    assert seen["hidden"] == [sac.latent_pi[0], sac.latent_pi[2]] and seen["mu"] is sac.mu and seen["log_std"] is sac.log_std
    assert seen["activation"] == "tanh" and seen["obs_keys"] == ("target_position",)
    with pytest.raises(AssertionError, match="native layer"):  # the real constructor accepts it and goes on to the native layer
        DeviceActor.from_sb3(venv, _SacActorStandIn(12, [64, 64], 3))

    class NoLatent(torch.nn.Module):
        def __init__(self):
            super().__init__()
            self.mu, self.log_std = torch.nn.Linear(4, 3), torch.nn.Linear(4, 3)

    with pytest.raises(ValueError, match="latent_pi"):
        DeviceActor.from_sb3(venv, NoLatent())
    gelu = _SacActorStandIn(12, [64], 3, torch.nn.GELU)
    with pytest.raises(ValueError, match="GELU"):
        DeviceActor.from_sb3(venv, gelu)


@gpu
def test_from_sb3_on_the_device(envs):
    from mujoco_sim_amd import DeviceActor

    venv = envs("robot_reach", 33)
    torch.manual_seed(21)
    sac = _SacActorStandIn(12, [64, 64], 3).to(venv.device)
    keys = sorted(k for k, _, _ in venv.flat_observation_layout)  # what SB3's CombinedExtractor concatenates
    actor = DeviceActor.from_sb3(venv, sac, obs_keys=keys)
    where = {k: (s, n) for k, s, n in venv.flat_observation_layout}
    cols = [c for k in keys for c in range(where[k][0], where[k][0] + where[k][1])]
    assert actor.obs_index == cols and actor.activation == "relu"
    check_against_torch(venv, actor, ([sac.latent_pi[0], sac.latent_pi[2]], sac.mu, sac.log_std), "relu", cols, None, "from_sb3")
    actor.close()
