"""The replay buffer on the device (csrc/mjs_replay.h, mujoco_sim_amd/replay.py) against a restatement of its rules in this file.

Every comparison is bitwise (``torch.equal``): the float64 -> float32 casts are single exact operations and the order of the
transitions is specified, so there is no tolerance to choose. The reference (``RefRing``) walks a block row by row in (t, n) order,
decides with the rules of include/mjsim.h which rows are transitions and where in the ring they go, and never calls the code under
test; rows are then copied with numpy indexing (a block holds at most ``capacity`` rows, so no ring row is written twice).
"""
import ctypes as C

import numpy as np
import pytest
import torch

from _visual_nets import SCENE, WRIST, make_cnn, make_mlp

gpu = pytest.mark.gpu
FIRST, MID, LAST = 0, 1, 2
SCALARS = ("obs", "next_obs", "actions", "rewards", "dones", "timeouts")


# ---------------------------------------------------------------------------------------------- the restatement
def to_np(block):
    return {k: v.cpu().numpy() for k, v in block.items() if isinstance(v, torch.Tensor)}


class RefRing:
    def __init__(self, capacity, cols, A, cameras=(), hw=(0, 0)):
        self.capacity, self.cols, self.count, self.cameras = capacity, list(cols), 0, tuple(cameras)
        D = len(self.cols)
        self.obs, self.next_obs = np.zeros((capacity, D), np.float32), np.zeros((capacity, D), np.float32)
        self.actions = np.zeros((capacity, A), np.float32)
        self.rewards, self.dones, self.timeouts = np.zeros(capacity, np.float32), np.zeros(capacity, np.float32), np.zeros(capacity, np.uint8)
        self.rgb = {k: np.zeros((capacity, *hw, 3), np.uint8) for k in self.cameras}
        self.next_rgb = {k: np.zeros((capacity, *hw, 3), np.uint8) for k in self.cameras}

    def add(self, obs0, blk, mode, final=None):
        """blk: numpy arrays. Returns the number of transitions."""
        T, N = blk["obs"].shape[:2]
        assert T * N <= self.capacity
        step_type, ended = blk["step_type"].tolist(), ((blk["terminated"] != 0) | (blk["truncated"] != 0)).tolist()
        ts, ns, ring, from_terminal = [], [], [], []
        for t in range(T):  # the rules, row by row in (t, n) order
            for n in range(N):
                if mode == "next_step" and step_type[t][n] == FIRST:
                    continue  # the step after a LAST: a reset, the action was ignored
                ts.append(t)
                ns.append(n)
                ring.append(self.count % self.capacity)
                from_terminal.append(mode == "same_step" and ended[t][n])
                self.count += 1
        if not ring:
            return 0
        ts, ns, ring, from_terminal = np.array(ts), np.array(ns), np.array(ring), np.array(from_terminal)
        prev = np.concatenate([obs0[None], blk["obs"][:-1]])  # prev[t] = obs[t - 1], obs0 for t = 0
        cols = np.array(self.cols, dtype=np.int64)
        self.obs[ring] = prev[ts, ns][:, cols].astype(np.float32)
        nxt = blk["obs"][ts, ns]
        if mode == "same_step":
            nxt = np.where(from_terminal[:, None], blk["terminal_obs"][ts, ns], nxt)
        self.next_obs[ring] = nxt[:, cols].astype(np.float32)
        self.actions[ring] = blk["squashed_actions"][ts, ns]
        self.rewards[ring] = blk["reward"][ts, ns].astype(np.float32)
        self.dones[ring] = np.where(blk["terminated"][ts, ns] != 0, np.float32(1), np.float32(0))
        self.timeouts[ring] = (blk["truncated"][ts, ns] != 0).astype(np.uint8)
        for k in self.cameras:
            frames = np.concatenate([blk[k], final[k][None]])  # frame T = the render after the block
            self.rgb[k][ring] = frames[ts, ns]
            self.next_rgb[k][ring] = frames[ts + 1, ns]
        return len(ring)


def assert_ring(buf, ref, what=""):
    for name in SCALARS:
        got, want = getattr(buf, name).cpu(), torch.from_numpy(getattr(ref, name))
        assert got.dtype == want.dtype and torch.equal(got, want), (what, name)
    for k in ref.cameras:
        assert torch.equal(buf.rgb[k].cpu(), torch.from_numpy(ref.rgb[k])), (what, k, "rgb")
        assert torch.equal(buf.next_rgb[k].cpu(), torch.from_numpy(ref.next_rgb[k])), (what, k, "next_rgb")
    assert buf.count == ref.count and buf.size == min(ref.count, ref.capacity), (what, buf.count, ref.count)


def snapshot(buf):
    return {**{n: getattr(buf, n).clone() for n in SCALARS}, **{f"rgb/{k}": v.clone() for k, v in buf.rgb.items()},
            **{f"next_rgb/{k}": v.clone() for k, v in buf.next_rgb.items()}, "cursor": buf._cursor.clone()}


def assert_untouched(buf, snap):
    now = snapshot(buf)
    for k, v in snap.items():
        assert torch.equal(now[k], v), k


# ---------------------------------------------------------------------------------------------- 1, 2. blocks from real envs
ENV_CASES = {
    "point_mass_reach": ({}, None),
    "robot_reach": ({}, ("ur5e/tcp_position", "target_position")),
    "robot_push_button": ({"action_type": "absolute_eef_action"}, None),
}


def columns(venv, keys):
    layout = {k: (s, n) for k, s, n in venv.flat_observation_layout}
    return [c for k in (keys if keys is not None else layout) for c in range(layout[k][0], layout[k][0] + layout[k][1])]


def staggered_env(task, N, autoreset, seed=3):
    """(env, actor, stored columns): three steps in, a masked third of the envs reset, so that episodes end at different steps."""
    import mujoco_sim_amd as m

    kw, keys = ENV_CASES[task]
    venv = m.HipVectorEnv(task, N, seed=seed, time_limit=0.5, autoreset=autoreset, **kw)
    venv.reset()
    cols = columns(venv, keys)
    actor = m.DeviceActor.from_linears(venv, *make_mlp(len(cols), [64, 64], venv.action_dim, seed=seed + 1, device=venv.device), obs_keys=keys)
    venv.actor_rollout(actor, 3, generator=torch.Generator(device=venv.device).manual_seed(seed))
    venv.reset(mask=torch.arange(N) % 3 == 0)
    return venv, actor, cols, keys


def collect_and_restate(buf, ref, venv, actor, T, gen):
    obs0 = venv.flat_obs.clone().cpu().numpy()
    blk = buf.collect(venv, actor, T, generator=gen)
    ref.add(obs0, to_np(blk), venv.autoreset)
    return blk


@gpu
@pytest.mark.parametrize("N", [33, 96])
@pytest.mark.parametrize("autoreset", ["next_step", "same_step"])
@pytest.mark.parametrize("task", list(ENV_CASES))
def test_blocks_from_real_envs_equal_the_restatement(task, autoreset, N):
    import mujoco_sim_amd as m

    T = 16
    venv, actor, cols, keys = staggered_env(task, N, autoreset)
    buf = m.DeviceReplayBuffer(venv, 2 * T * N, obs_keys=keys)
    ref = RefRing(buf.capacity, cols, venv.action_dim)
    assert buf.obs_index == cols and buf.obs.shape == (buf.capacity, len(cols))
    blk = collect_and_restate(buf, ref, venv, actor, T, torch.Generator(device=venv.device).manual_seed(1))
    st = blk["step_type"]
    n_first, n_last = int((st == FIRST).sum()), int((st == LAST).sum())
    print(f"{task} {autoreset} N={N}: {ref.count} transitions of {T * N} rows, {n_last} LAST, {n_first} FIRST")
    assert n_last >= 1
    if autoreset == "next_step":
        assert n_first >= 1 and 0 < ref.count < T * N and ref.count == T * N - n_first
    else:
        assert "terminal_obs" in blk and ref.count == T * N
        stored_next = buf.next_obs[:T * N].view(T, N, -1)
        assert not torch.equal(stored_next, blk["obs"][:, :, cols].float())  # a terminal observation was stored somewhere
    assert_ring(buf, ref, f"{task} {autoreset} {N}")
    assert bool((buf.dones[:ref.count] == 0).all()) or bool(blk["terminated"].any())  # a time limit alone never sets done
    assert int(buf.timeouts.sum()) == int((blk["truncated"] != 0)[st != FIRST].sum() if autoreset == "next_step" else (blk["truncated"] != 0).sum())
    buf.close()
    actor.close()
    venv.close()


@gpu
@pytest.mark.parametrize("task,autoreset", [("point_mass_reach", "next_step"), ("robot_reach", "same_step")])
def test_ring_wraps(task, autoreset):
    import mujoco_sim_amd as m

    venv, actor, cols, keys = staggered_env(task, 33, autoreset)
    buf = m.DeviceReplayBuffer(venv, 1000, obs_keys=keys)
    ref = RefRing(1000, cols, venv.action_dim)
    gen = torch.Generator(device=venv.device).manual_seed(2)
    for call in range(4):
        collect_and_restate(buf, ref, venv, actor, 16, gen)
        assert_ring(buf, ref, f"call {call}")
    assert ref.count > 1000  # the ring did wrap
    buf.close()
    actor.close()
    venv.close()


# ---------------------------------------------------------------------------------------------- 3. scan and rank edges
@pytest.fixture(scope="module")
def pointmass():
    import mujoco_sim_amd as m

    venv = m.HipVectorEnv("point_mass_reach", 4, seed=1)
    venv.reset()
    yield venv
    venv.close()


def synthetic_block(T, N, src_dim, A, pattern, device, seed=0):
    """A block whose observations encode (t, n) (integers below 2^24 and halves: exact in float32), with a step_type pattern."""
    rs = np.random.RandomState(seed)
    rows = T * N
    t, n = np.divmod(np.arange(rows), N)
    obs = np.zeros((rows, src_dim))
    obs[:, 0], obs[:, 1], obs[:, 2] = t, n, np.arange(rows) + 0.5
    obs0 = np.zeros((N, src_dim))
    obs0[:, 0], obs0[:, 1], obs0[:, 2] = -1, np.arange(N), -np.arange(N) - 0.5
    valid = {"all": np.ones(rows, bool), "none": np.zeros(rows, bool), "last": np.arange(rows) == rows - 1, "alternating": np.arange(rows) % 2 == 1,
             "random": rs.rand(rows) < 0.7}[pattern]
    step_type = np.where(valid, np.where(rs.rand(rows) < 0.2, LAST, MID), FIRST).astype(np.uint8)
    blk = {"obs": obs.reshape(T, N, src_dim), "reward": (np.arange(rows) * 0.25 - 3).reshape(T, N), "step_type": step_type.reshape(T, N),
           "terminated": (rs.rand(T, N) < 0.3).astype(np.uint8), "truncated": (rs.rand(T, N) < 0.3).astype(np.uint8),
           "squashed_actions": rs.uniform(-1, 1, (T, N, A)).astype(np.float32)}
    return obs0, blk, torch.from_numpy(obs0).to(device), {k: torch.from_numpy(v).to(device) for k, v in blk.items()}


# T x N = 1, 63, 64, 65, 1023, 1025 (around a wavefront and a chunk), 20 001 (more chunks than a wavefront has lanes), 300 001 (more
# than the scan's workgroup has threads)
SHAPES = [(1, 1), (7, 9), (2, 32), (5, 13), (3, 341), (25, 41), (3, 6667), (13, 23077)]


@gpu
@pytest.mark.parametrize("pattern", ["all", "none", "last", "alternating", "random"])
@pytest.mark.parametrize("T,N", SHAPES)
def test_scan_and_rank_edges(pointmass, T, N, pattern):
    import mujoco_sim_amd as m

    rows, cols = T * N, [2, 0]
    buf = m.DeviceReplayBuffer(pointmass, rows + 7, obs_index=cols)  # src_dim 4, A 2
    ref = RefRing(rows + 7, cols, 2)
    obs0, blk, obs0_d, blk_d = synthetic_block(T, N, 4, 2, pattern, buf.device, seed=rows)
    for call in range(2):  # the second block wraps around the ring's end (where the pattern has enough rows)
        before = snapshot(buf)
        buf.add_block(obs0_d, blk_d)
        added = ref.add(obs0, blk, "next_step")
        if pattern == "none":
            assert added == 0
            assert_untouched(buf, before)
        assert_ring(buf, ref, f"{T}x{N} {pattern} call {call}")
    assert ref.count == 2 * int((blk["step_type"] != FIRST).sum())
    buf.close()


# ---------------------------------------------------------------------------------------------- 4. images
@pytest.fixture(scope="module")
def button():
    import mujoco_sim_amd as m

    venv = m.HipVectorEnv("robot_push_button", 33, seed=1)  # two cameras
    venv.reset()
    yield venv
    venv.close()


def synthetic_frames(T, N, H, W, cam):
    """uint8 [T + 1, N, H, W, 3] with (t, n) and the byte's position in every byte."""
    t, n = np.arange(T + 1)[:, None, None], np.arange(N)[None, :, None]
    return ((np.arange(H * W * 3)[None, None, :] * 7 + t * 37 + n * 5 + cam * 11) % 251).astype(np.uint8).reshape(T + 1, N, H, W, 3)


def image_buffer(button, H, W, capacity, calls=2):
    """A two-camera buffer filled from synthetic blocks (FIRST rows present), and its restatement."""
    import mujoco_sim_amd as m

    T, N, cams = 5, 33, (WRIST, SCENE)
    buf = m.DeviceReplayBuffer(button, capacity, obs_index=[12, 0, 5], cameras=cams, image_size=(H, W))
    ref = RefRing(capacity, [12, 0, 5], 7, cams, (H, W))
    for call in range(calls):
        obs0, blk, obs0_d, blk_d = synthetic_block(T, N, 13, 7, "random", buf.device, seed=call)
        assert (blk["step_type"] == FIRST).any() and (blk["step_type"][-1] != FIRST).any()
        final, final_d = {}, {}
        for c, k in enumerate(cams):
            frames = synthetic_frames(T, N, H, W, c + 2 * call)
            blk[k], final[k] = frames[:T], frames[T]
            blk_d[k], final_d[k] = torch.from_numpy(frames[:T].copy()).to(buf.device), torch.from_numpy(frames[T].copy()).to(buf.device)
        buf.add_block(obs0_d, blk_d, final_d)
        ref.add(obs0, blk, "next_step", final)
    return buf, ref


@gpu
@pytest.mark.parametrize("H,W", [(36, 36), (37, 41)])  # 3888 bytes: the 16-byte path; 4551 bytes: odd, every row after the first misaligned
def test_images(button, H, W):
    import mujoco_sim_amd as m

    buf, ref = image_buffer(button, H, W, 200)
    assert ref.count > 200  # the second block wrapped
    assert_ring(buf, ref, f"{H}x{W}")
    buf.close()
    same = m.HipVectorEnv("point_mass_reach", 4, seed=1, autoreset="same_step")
    with pytest.raises(ValueError, match="next_step"):
        m.DeviceReplayBuffer(same, 100, cameras=(SCENE,), image_size=36)
    same.close()


# ---------------------------------------------------------------------------------------------- 5. collect with a visual actor
def visual_policy(venv, R=36, F=24, seed=5):
    import mujoco_sim_amd as m

    enc = m.DeviceEncoder.from_sb3(venv, make_cnn(R, R, F, seed=seed, device=venv.device), R, R)
    width = sum(n for _, _, n in venv.flat_observation_layout)
    actor = m.DeviceActor.from_linears(venv, *make_mlp(width + F, [64, 64], venv.action_dim, seed=seed + 1, device=venv.device), encoders={SCENE: enc})
    return actor, enc


@gpu
def test_collect_with_a_visual_actor():
    import mujoco_sim_amd as m

    N, T, R = 33, 8, 36
    one, two, loop = (m.HipVectorEnv("point_mass_reach", N, seed=9, time_limit=0.5) for _ in range(3))
    for v in (one, two, loop):
        v.reset()
    actor, enc = visual_policy(one)
    z = torch.randn(2 * T, N, 2, dtype=torch.float32, device=one.device, generator=torch.Generator(device=one.device).manual_seed(4))
    cols = columns(one, None)
    b_one, b_two = (m.DeviceReplayBuffer(v, 3 * T * N, cameras=(SCENE,), image_size=R) for v in (one, two))
    obs0 = one.flat_obs.clone().cpu().numpy()
    blk = b_one.collect(one, actor, 2 * T, z=z)
    assert blk[SCENE].shape == (2 * T, N, R, R, 3) and int((blk["step_type"] == FIRST).sum()) >= 1
    # the frames, from a second handle stepped by hand with the recorded actions: render before every step, and after the last
    frames = []
    for t in range(2 * T):
        frames.append(loop.render(R, R).cpu().numpy())
        loop.step_flat(blk["actions"][t].contiguous())
    final = loop.render(R, R).cpu().numpy()
    assert float(np.stack(frames).std()) > 1  # the frames show something
    ref = RefRing(b_one.capacity, cols, 2, (SCENE,), (R, R))
    ref.add(obs0, {**{k: v for k, v in to_np(blk).items() if k != SCENE}, SCENE: np.stack(frames)}, "next_step", {SCENE: final})
    assert_ring(b_one, ref, "one collect(2T)")
    b_two.collect(two, actor, T, z=z[:T].contiguous())
    b_two.collect(two, actor, T, z=z[T:].contiguous())
    assert_ring(b_two, ref, "two collect(T)")
    for o in (b_one, b_two, actor, enc, one, two, loop):
        o.close()


# ---------------------------------------------------------------------------------------------- 6. sample
def check_sample(buf, draws, what):
    out = buf.sample(len(draws), draws=draws)
    size, d = buf.size, draws.cpu().numpy()
    idx = np.array([int(x) % size for x in d], dtype=np.int64)  # the rule, row by row
    assert out["indices"].dtype == torch.int64 and torch.equal(out["indices"].cpu(), torch.from_numpy(idx)), what
    for name in SCALARS:
        assert torch.equal(out[name].cpu(), getattr(buf, name).cpu()[idx]), (what, name)
    for k in buf.cameras:
        assert torch.equal(out["rgb"][k].cpu(), buf.rgb[k].cpu()[idx]) and torch.equal(out["next_rgb"][k].cpu(), buf.next_rgb[k].cpu()[idx]), (what, k)
    return out


@gpu
@pytest.mark.parametrize("B", [1, 65, 1000])
def test_sample(pointmass, button, B):
    import mujoco_sim_amd as m
    from mujoco_sim_amd import _native as nat

    dev = pointmass.device
    gen = torch.Generator(device=dev).manual_seed(B)
    draws = torch.randint(0, 2**62, (B,), dtype=torch.int64, device=dev, generator=gen)
    buf = m.DeviceReplayBuffer(pointmass, 500, obs_index=[3, 1, 0])
    # empty: indices -1, zero rows
    out = buf.sample(B, draws=draws)
    assert bool((out["indices"] == -1).all()) and all(not bool(out[k].any()) for k in SCALARS)
    obs0, blk, obs0_d, blk_d = synthetic_block(7, 41, 4, 2, "random", dev, seed=3)
    buf.add_block(obs0_d, blk_d)
    assert 0 < buf.size < 500
    check_sample(buf, draws, "part-full")
    check_sample(buf, torch.arange(B, dtype=torch.int64, device=dev), "part-full, consecutive draws")
    for _ in range(2):
        buf.add_block(obs0_d, blk_d)
    assert buf.size == 500 and buf.count > 500
    check_sample(buf, draws, "full")
    # the default draws come from the generator
    a, b = buf.sample(B, generator=torch.Generator(device=dev).manual_seed(7)), buf.sample(B, generator=torch.Generator(device=dev).manual_seed(7))
    want = torch.randint(0, 2**62, (B,), dtype=torch.int64, device=dev, generator=torch.Generator(device=dev).manual_seed(7)) % 500
    assert torch.equal(a["indices"], want) and all(torch.equal(a[k], b[k]) for k in a)
    # NULL outputs are skipped: only rewards and the indices asked for
    rewards, idx = torch.full((B,), -7.0, dtype=torch.float32, device=dev), torch.full((B,), -7, dtype=torch.int64, device=dev)
    batch = nat.MjsReplayBatch(idx_out=idx.data_ptr(), rewards=rewards.data_ptr())
    assert nat.lib().mjs_replay_sample(C.byref(buf._storage), draws.data_ptr(), B, C.byref(batch), buf._stream()) == 0
    assert torch.equal(idx, draws % 500) and torch.equal(rewards, buf.rewards[idx])
    assert nat.lib().mjs_replay_sample(C.byref(buf._storage), draws.data_ptr(), B, C.byref(nat.MjsReplayBatch()), buf._stream()) == 0  # nothing asked for
    assert buf.sample(0)["obs"].shape == (0, 3)
    buf.close()
    # with images, both copy paths
    for H, W in ((36, 36), (37, 41)):
        ibuf, _ = image_buffer(button, H, W, 400, calls=1)
        check_sample(ibuf, draws, f"images {H}x{W}")
        ibuf.close()


# ---------------------------------------------------------------------------------------------- 7. refusals at the ABI
def copy_of(s, **changes):
    c = type(s).from_buffer_copy(s)
    for k, v in changes.items():
        setattr(c, k, v)
    return c


@gpu
def test_refusals_at_the_abi(pointmass, button):
    import mujoco_sim_amd as m
    from mujoco_sim_amd import _native as nat

    L = nat.lib()
    dev = pointmass.device
    T, N = 6, 10
    buf = m.DeviceReplayBuffer(pointmass, 100, obs_index=[0, 3])
    obs0, blk, obs0_d, blk_d = synthetic_block(T, N, 4, 2, "random", dev)
    blk_d["terminal_obs"] = blk_d["obs"].clone()
    buf.add_block(obs0_d, blk_d)  # something to leave unchanged
    ws = torch.empty(int(L.mjs_replay_workspace_bytes(T, N)), dtype=torch.uint8, device=dev)
    index = (C.c_int32 * 2)(0, 3)
    good = nat.MjsReplayBlock(T=T, N=N, src_dim=4, autoreset=nat.AUTORESET_NEXT_STEP, obs_index=index, obs0=obs0_d.data_ptr(), obs=blk_d["obs"].data_ptr(),
                              terminal_obs=blk_d["terminal_obs"].data_ptr(), reward=blk_d["reward"].data_ptr(), terminated=blk_d["terminated"].data_ptr(),
                              truncated=blk_d["truncated"].data_ptr(), step_type=blk_d["step_type"].data_ptr(), squashed_actions=blk_d["squashed_actions"].data_ptr())
    st = buf._storage
    before = snapshot(buf)
    stream = buf._stream()
    assert L.mjs_replay_workspace_bytes(0, 5) == 0 and L.mjs_replay_workspace_bytes(5, -1) == 0

    def refused_add(storage, block, workspace=ws.data_ptr(), what=""):
        rc = L.mjs_replay_add(C.byref(storage) if storage is not None else None, C.byref(block) if block is not None else None, workspace, stream)
        assert rc == -1 and L.mjs_last_error(None), what  # MJS_ERR_INVALID_ARG, with a text
        assert L.mjs_last_error(None).startswith(b"mjs_replay_add: "), what
        assert_untouched(buf, before)

    refused_add(copy_of(st, struct_size=C.sizeof(st) - 8), good, what="storage struct_size")
    refused_add(st, copy_of(good, struct_size=C.sizeof(good) + 8), what="block struct_size")
    refused_add(None, good, what="null storage")
    refused_add(st, None, what="null block")
    refused_add(st, good, workspace=None, what="null workspace")
    for field in ("cursor_dev", "obs", "next_obs", "actions", "rewards", "dones", "timeouts"):
        refused_add(copy_of(st, **{field: None}), good, what=f"storage.{field}")
    for field in ("obs0", "obs", "reward", "terminated", "truncated", "step_type", "squashed_actions", "obs_index"):
        refused_add(st, copy_of(good, **{field: None}), what=f"block.{field}")
    refused_add(copy_of(st, capacity=0), good, what="capacity 0")
    refused_add(copy_of(st, capacity=T * N - 1), good, what="T N > capacity")
    for D in (-1, 65):
        refused_add(copy_of(st, obs_dim=D), good, what=f"obs_dim {D}")
    for A in (0, 9):
        refused_add(copy_of(st, action_dim=A), good, what=f"action_dim {A}")
    for bad in ((0, 4), (-1, 3)):
        refused_add(st, copy_of(good, obs_index=(C.c_int32 * 2)(*bad)), what=f"obs_index {bad}")
    refused_add(st, copy_of(good, autoreset=nat.AUTORESET_DISABLED), what="autoreset disabled")
    refused_add(st, copy_of(good, autoreset=nat.AUTORESET_SAME_STEP, terminal_obs=None), what="same-step without terminal_obs")
    refused_add(st, copy_of(good, T=-1), what="negative T")
    refused_add(st, copy_of(good, N=0), what="N 0")
    refused_add(st, copy_of(good, src_dim=0), what="src_dim 0")
    refused_add(copy_of(st, n_cameras=3), good, what="three cameras")
    # cameras: a two-camera storage of its own
    ibuf = m.DeviceReplayBuffer(button, 100, obs_index=[0, 3], cameras=(WRIST, SCENE), image_size=(37, 41))
    frames = torch.zeros(T + 1, N, 37, 41, 3, dtype=torch.uint8, device=dev)
    pair = lambda t: (C.c_void_p * 2)(t.data_ptr(), t.data_ptr())  # noqa: E731
    igood = copy_of(good, rgb=pair(frames), final_rgb=pair(frames[T]))
    ist, ibefore = copy_of(ibuf._storage, action_dim=2), snapshot(ibuf)

    def refused_images(storage, block, what):
        assert L.mjs_replay_add(C.byref(storage), C.byref(block), ws.data_ptr(), stream) == -1 and L.mjs_last_error(None), what
        assert_untouched(ibuf, ibefore)

    refused_images(copy_of(ist, height=0), igood, "cameras without a height")
    refused_images(copy_of(ist, width=-3), igood, "cameras without a width")
    refused_images(ist, copy_of(igood, autoreset=nat.AUTORESET_SAME_STEP), "cameras under same-step auto-reset")
    refused_images(ist, good, "a camera's frames are null")
    refused_images(ist, copy_of(igood, final_rgb=(C.c_void_p * 2)(frames.data_ptr(), None)), "a camera's final frame is null")
    refused_images(copy_of(ist, next_rgb=(C.c_void_p * 2)(None, None)), igood, "the storage's next_rgb is null")
    # ... and the descriptor as it stands is fine: T == 0 returns 0 and does nothing, T rows are taken
    assert L.mjs_replay_add(C.byref(ist), C.byref(copy_of(igood, T=0)), ws.data_ptr(), stream) == 0
    assert_untouched(ibuf, ibefore)
    assert L.mjs_replay_add(C.byref(ist), C.byref(igood), ws.data_ptr(), stream) == 0
    assert ibuf.count == int((blk["step_type"] != FIRST).sum())
    ibuf.close()

    # sample
    draws = torch.arange(8, dtype=torch.int64, device=dev)
    rewards = torch.full((8,), -7.0, dtype=torch.float32, device=dev)
    batch = nat.MjsReplayBatch(rewards=rewards.data_ptr())

    def refused_sample(storage, d, B, out, what):
        rc = L.mjs_replay_sample(C.byref(storage) if storage is not None else None, d, B, C.byref(out) if out is not None else None, stream)
        assert rc == -1 and L.mjs_last_error(None).startswith(b"mjs_replay_sample: "), what
        assert_untouched(buf, before)
        assert bool((rewards == -7).all()), what

    refused_sample(st, draws.data_ptr(), -1, batch, "negative B")
    refused_sample(st, None, 8, batch, "null draws")
    refused_sample(st, draws.data_ptr(), 8, None, "null batch")
    refused_sample(None, draws.data_ptr(), 8, batch, "null storage")
    refused_sample(st, draws.data_ptr(), 8, copy_of(batch, struct_size=4), "batch struct_size")
    refused_sample(copy_of(st, struct_size=0), draws.data_ptr(), 8, batch, "storage struct_size")
    refused_sample(copy_of(st, capacity=-5), draws.data_ptr(), 8, batch, "capacity")
    assert L.mjs_replay_sample(C.byref(st), None, 0, C.byref(batch), stream) == 0 and bool((rewards == -7).all())  # B == 0
    assert L.mjs_replay_add(C.byref(st), C.byref(copy_of(good, T=0)), ws.data_ptr(), stream) == 0  # T == 0
    assert_untouched(buf, before)
    # the same-step descriptor with terminal_obs is taken
    assert L.mjs_replay_add(C.byref(st), C.byref(copy_of(good, autoreset=nat.AUTORESET_SAME_STEP, step_type=None)), ws.data_ptr(), stream) == 0
    assert buf.count == int(before["cursor"].item()) + T * N
    buf.close()
