"""Episode statistics on the device (csrc/mjs_monitor.h, mujoco_sim_amd/monitor.py) against the numpy restatement of its rules in
_monitor_reference.py, against step-by-step host loops over real envs, and inside DeviceSAC.learn.

Every comparison of the state is bitwise (float64 fields through their int64 view): one float64 add per counting row in t order and a
specified record order leave no tolerance to choose. The summary's bounds are derived in its test's docstring.
"""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import _critic_reference as cref
import _monitor_reference as mref
from _monitor_reference import FIRST, LAST, MID, BlockMaker, to_dev
from _visual_nets import make_mlp

gpu = pytest.mark.gpu
DEV = "cuda:0"
MODES = ("next_step", "same_step")
BLOCK_KEYS = ("reward", "terminated", "truncated", "is_success", "step_type")


def bits(t):
    t = t.detach().cpu()
    return t.view(torch.int64) if t.dtype == torch.float64 else t


def assert_state(mon, ref, what=""):
    for name in mref.RING_FIELDS + ("ep_return", "ep_length", "ep_count"):
        got, want = getattr(mon, name).cpu(), torch.from_numpy(getattr(ref, name))
        assert got.dtype == want.dtype and torch.equal(bits(got), bits(want)), (what, name, got, want)
    assert mon.count == ref.cursor, (what, mon.count, ref.cursor)
    ep, live = mon.episodes(), ref.live()
    for key, want in zip(("return", "length", "success", "terminated", "env"), live):
        assert torch.equal(bits(ep[key]), bits(torch.from_numpy(want))), (what, key)


def snapshot(mon):
    return [bits(getattr(mon, n)).clone() for n in mref.RING_FIELDS + ("ep_return", "ep_length", "ep_count", "_cursor")]


def both(N, window=100, quota=None):
    import mujoco_sim_amd as m

    return m.DeviceEpisodeMonitor(N, device=DEV, window=window, quota=quota), mref.RefMonitor(N, window, quota)


# ---------------------------------------------------------------------------------------------- 1. the rules, bit for bit
@gpu
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("T", [1, 2, 7])
@pytest.mark.parametrize("N", [1, 63, 64, 65, 257])
def test_synthetic_blocks_equal_the_restatement(N, T, mode):
    mon, ref = both(N, window=100)
    maker = BlockMaker(N, mode, seed=1000 * N + T)
    for i in range(3):  # the second and third block start from carried accumulators (and, next-step, from FIRST rows at t = 0)
        blk = maker.block(T)
        mon.update(to_dev(blk), mode)
        ref.update(blk, mode)
        assert_state(mon, ref, f"block {i}")
    assert ref.cursor > 0 or N * T < 8
    mon.close()


@gpu
@pytest.mark.parametrize("mode", MODES)
def test_no_end_and_every_row_an_end(mode):
    N, T = 65, 7
    mon, ref = both(N, window=1000)
    maker = BlockMaker(N, mode, seed=5)
    quiet = maker.block(T, p_end=0.0)
    mon.update(to_dev(quiet), mode)
    assert ref.update(quiet, mode) == 0
    assert_state(mon, ref, "no end")
    assert mon.count == 0 and int(mon.ep_length.min()) == T and mon.summary()["count"] == 0
    every = maker.block(T, p_end=0.0)
    every["terminated"][:] = 1
    every["step_type"][:] = LAST  # (a synthetic block: the rule reads only step_type != FIRST)
    mon.update(to_dev(every), mode)
    assert ref.update(every, mode) == T * N
    assert_state(mon, ref, "every row")
    assert int(mon.ep_length.max()) == 0 and mon.count == T * N
    mon.close()


@gpu
def test_first_rows_are_ignored_whatever_they_carry():
    """Next-step auto-reset: block 1 ends on LAST for every env, so block 2 starts with FIRST at t = 0; those rows carry a reward of 1e6
    and both flags and change nothing; under same-step auto-reset the same rows count."""
    N = 65
    one = {"reward": np.full((2, N), 1.5), "terminated": np.zeros((2, N), np.uint8), "truncated": np.zeros((2, N), np.uint8),
           "is_success": np.zeros((2, N), np.uint8), "step_type": np.full((2, N), MID, np.uint8)}
    one["truncated"][1], one["step_type"][1] = 1, LAST
    two = {"reward": np.full((2, N), 0.25), "terminated": np.zeros((2, N), np.uint8), "truncated": np.zeros((2, N), np.uint8),
           "is_success": np.ones((2, N), np.uint8), "step_type": np.full((2, N), MID, np.uint8)}
    two["reward"][0], two["terminated"][0], two["truncated"][0], two["step_type"][0] = 1e6, 1, 1, FIRST
    mon, ref = both(N, window=4 * N)
    for blk in (one, two):
        mon.update(to_dev(blk), "next_step")
        ref.update(blk, "next_step")
    assert_state(mon, ref, "next-step")
    assert mon.count == N and bool((mon.ep_return == 0.25).all()) and bool((mon.ep_length == 1).all()) and bool((mon.ring_return[:N] == 3.0).all())
    mon.reset()
    assert mon.count == 0 and not bool(mon.ring_return.any()) and not bool(mon.ep_count.any())
    ref = mref.RefMonitor(N, 4 * N)
    for blk in (one, two):
        mon.update(to_dev(blk), "same_step")
        ref.update(blk, "same_step")
    assert_state(mon, ref, "same-step")
    assert mon.count == 2 * N and bool((mon.ring_return[N:2 * N] == 1e6).all())
    mon.close()


@gpu
@pytest.mark.parametrize("mode", MODES)
def test_two_updates_of_T_leave_what_one_of_2T_leaves(mode):
    N, T = 257, 7
    blk = BlockMaker(N, mode, seed=9).block(2 * T)
    halves = [{k: v[:T] for k, v in blk.items()}, {k: v[T:] for k, v in blk.items()}]
    a, ref = both(N, window=50)
    b, _ = both(N, window=50)
    for h in halves:
        a.update(to_dev(h), mode)
    b.update(to_dev(blk), mode)
    ref.update(blk, mode)
    assert ref.cursor > 50  # the window wrapped on the way
    assert_state(a, ref, "two halves")
    assert_state(b, ref, "one block")
    assert all(torch.equal(x, y) for x, y in zip(snapshot(a), snapshot(b)))
    a.close()
    b.close()


@gpu
@pytest.mark.parametrize("mode", MODES)
def test_ring_wraps_over_several_blocks(mode):
    N, W = 3, 5
    mon, ref = both(N, window=W)
    maker = BlockMaker(N, mode, seed=2, p_end=0.4)
    for i in range(6):
        blk = maker.block(4)
        mon.update(to_dev(blk), mode)
        ref.update(blk, mode)
        assert_state(mon, ref, f"block {i}")
    assert ref.cursor > 2 * W
    mon.close()


@gpu
def test_a_block_with_more_episodes_than_the_window():
    """E = 7 > W = 4 in ONE block (7 ends among 2 x 5 rows), after 2 earlier records: the last four survive, in order, at slots
    (2 + 3..6) % 4 = 1, 2, 3, 0."""
    N, W = 5, 4
    mon, ref = both(N, window=W)
    head = {"reward": np.array([[1.0, 2.0, 3.0, 4.0, 5.0]]), "terminated": np.array([[1, 0, 0, 1, 0]], np.uint8), "truncated": np.zeros((1, N), np.uint8),
            "is_success": np.zeros((1, N), np.uint8), "step_type": np.full((1, N), MID, np.uint8)}
    blk = {"reward": np.arange(10, 20, dtype=np.float64).reshape(2, N), "terminated": np.array([[1, 1, 0, 1, 0], [1, 1, 1, 0, 1]], np.uint8),
           "truncated": np.zeros((2, N), np.uint8), "is_success": np.array([[1, 0, 0, 1, 0], [0, 1, 0, 0, 1]], np.uint8), "step_type": np.full((2, N), MID, np.uint8)}
    for b in (head, blk):
        mon.update(to_dev(b), "same_step")
        ref.update(b, "same_step")
    assert ref.cursor == 9
    assert_state(mon, ref)
    ep = mon.episodes()
    # (t 0: envs 0, 1, 3 are dropped) t 1: env 0 (15), env 1 (16), env 2 (3 + 12 + 17), env 4 (5 + 14 + 19)
    assert ep["return"].tolist() == [15.0, 16.0, 32.0, 38.0] and ep["env"].tolist() == [0, 1, 2, 4] and ep["length"].tolist() == [1, 1, 3, 3]
    assert mon.ring_env.tolist() == [4, 0, 1, 2]
    mon.close()


@gpu
@pytest.mark.parametrize("mode", MODES)
def test_quota(mode):
    N = 65
    quota = [(i % 4) for i in range(N)]  # zero for every fourth env; 1..3 are reached mid-block
    mon, ref = both(N, window=200, quota=quota)
    maker = BlockMaker(N, mode, seed=4, p_end=0.5)
    assert int(mon.remaining()) == sum(quota)
    for i in range(5):
        blk = maker.block(7)
        mon.update(to_dev(blk), mode)
        ref.update(blk, mode)
        assert_state(mon, ref, f"block {i}")
        rem = mon.remaining()
        assert rem.device.type == "cuda" and rem.dim() == 0 and int(rem) == ref.remaining()
    assert ref.remaining() == 0 and mon.count == sum(quota) and mon.ep_count.tolist() == quota
    assert not bool((mon.ring_env[:mon.count] % 4 == 0).any())  # a zero quota records nothing ...
    last = maker.block(1, p_end=0.0)
    mon.update(to_dev(last), mode)
    ref.update(last, mode)
    assert_state(mon, ref, "after the quota")  # ... yet the accumulators of such an env reset at every end, as the restatement's do
    mon.close()


@gpu
def test_two_runs_give_equal_bits():
    N, T = 257, 7
    blocks = [BlockMaker(N, "next_step", seed=8).block(T) for _ in range(3)]
    runs = []
    for _ in range(2):
        mon, _ = both(N, window=64, quota=[3] * N)
        for blk in blocks:
            mon.update(to_dev(blk), "next_step")
        mon.summary()
        runs.append(snapshot(mon) + [bits(mon._summary).clone()])
        mon.close()
    assert all(torch.equal(x, y) for x, y in zip(*runs))


# ---------------------------------------------------------------------------------------------- 2. the summary
@gpu
@pytest.mark.parametrize("W,blocks", [(100, 1), (100, 4), (700, 6), (1, 2)])
def test_summary_against_numpy(W, blocks):
    """count, min, max and the success rate are exact. A float64 sum of K terms in ANY order is within K * 2^-52 * sum|x_i| of the exact
    one (each of the K - 1 adds rounds by at most 2^-53 relative to a partial sum bounded by sum|x_i|; both sides of the comparison do,
    hence 2^-52): the bound on the returns' sum against numpy's. The lengths' sum is exact. The mean is that sum divided by K in one
    rounding. For the std, numpy.std's own error on the same records is measured against an exact recomputation (rational arithmetic),
    and the kernel is allowed 4 x that (_monitor_reference.std_bar). The exact value is itself a float64, so the measurement resolves whole
    ulps of it only; where numpy's error reads 0 the measurement is taken as its resolution, one ulp, so the bar is never below 4 ulp.
    A single record has std 0 on both sides, exactly."""
    N, mode = 65, "same_step"
    mon, ref = both(N, window=W)
    maker = BlockMaker(N, mode, seed=W + blocks, p_end=0.3)
    for _ in range(blocks):
        blk = maker.block(7)
        mon.update(to_dev(blk), mode)
        ref.update(blk, mode)
    ret, length, success, _, _ = ref.live()
    K = len(ret)
    assert K == min(ref.cursor, W) and K > 0
    s = mon.summary()
    assert s["count"] == K and s["return_min"] == ret.min() and s["return_max"] == ret.max()
    assert s["success_count"] == int(success.sum()) and s["success_rate"] == np.mean(success.astype(np.float64))
    assert s["length_sum"] == int(length.sum()) and s["length_mean"] == float(length.sum()) / K
    bound = K * 2.0 ** -52 * float(np.abs(ret).sum())
    print(f"W={W} K={K}: return sum {s['return_sum']!r} against numpy's {float(ret.sum())!r}, |difference| {abs(s['return_sum'] - float(ret.sum())):.3e}, bound {bound:.3e}")
    assert abs(s["return_sum"] - float(ret.sum())) <= bound
    assert s["return_mean"] == s["return_sum"] / K
    exact, numpy_err, bar = mref.std_bar(ret)
    kernel_err = abs(s["return_std"] - exact)
    print(f"W={W} K={K}: std {s['return_std']!r}, exact {exact!r} (one ulp {float(np.spacing(exact)):.3e}): numpy's error {numpy_err:.3e}, the kernel's {kernel_err:.3e}, bar {bar:.3e}")
    assert kernel_err <= bar
    mon.close()


# ---------------------------------------------------------------------------------------------- 3. refusals at the ABI
def copy_of(s, **changes):
    c = type(s).from_buffer_copy(s)
    for k, v in changes.items():
        setattr(c, k, v)
    return c


@gpu
def test_refusals_at_the_abi():
    from mujoco_sim_amd import _native as nat

    N, T = 5, 3
    mon, _ = both(N, window=4, quota=[1] * N)
    L, st, stream = mon._lib, mon._state, mon._stream()
    blk = to_dev(BlockMaker(N, "next_step", seed=1).block(T))
    mon.update(blk, "next_step")
    good = nat.MjsMonitorBlock(T=T, N=N, autoreset=nat.AUTORESET_NEXT_STEP, **{k: blk[k].data_ptr() for k in BLOCK_KEYS})
    ws = torch.empty(int(L.mjs_monitor_workspace_bytes(T, N)), dtype=torch.uint8, device=DEV)
    out = torch.full((10,), -7.0, dtype=torch.float64, device=DEV)
    before = snapshot(mon)
    assert L.mjs_monitor_workspace_bytes(0, 5) == 0 and L.mjs_monitor_workspace_bytes(5, -1) == 0 and L.mjs_monitor_workspace_bytes(2**16, 2**15) == 0
    assert L.mjs_monitor_workspace_bytes(T, N) >= 16 + 16 + T * N * 12

    def refused(state, block, text, workspace=ws.data_ptr()):
        rc = L.mjs_monitor_update(C.byref(state) if state is not None else None, C.byref(block) if block is not None else None, workspace, stream)
        err = L.mjs_last_error(None)
        assert rc == -1 and err.startswith(b"mjs_monitor_update: ") and text.encode() in err, (text, rc, err)  # MJS_ERR_INVALID_ARG
        assert all(torch.equal(x, y) for x, y in zip(snapshot(mon), before)), text

    refused(None, good, "state is null")
    refused(st, None, "block is null")
    refused(st, good, "workspace_dev is null", workspace=None)
    refused(copy_of(st, struct_size=C.sizeof(st) - 8), good, "mjs_monitor_state.struct_size")
    refused(st, copy_of(good, struct_size=C.sizeof(good) + 8), "mjs_monitor_block.struct_size")
    for field in ("ep_return", "ep_length", "ep_count"):
        refused(copy_of(st, **{field: None}), good, "ep_return, ep_length or ep_count is null")
    refused(copy_of(st, cursor_dev=None), good, "cursor_dev is null")
    for field in ("ring_return", "ring_length", "ring_success", "ring_terminated", "ring_env"):
        refused(copy_of(st, **{field: None}), good, "the ring's")
    for field in ("reward", "terminated", "truncated", "is_success"):
        refused(st, copy_of(good, **{field: None}), "reward, terminated, truncated or is_success is null")
    refused(st, copy_of(good, step_type=None), "next-step auto-reset needs step_type")
    refused(copy_of(st, num_envs=0), copy_of(good, N=0), "num_envs must be at least 1")
    refused(st, copy_of(good, N=0), "N must be positive")
    refused(st, copy_of(good, N=N + 1), "not the state's num_envs")
    refused(st, copy_of(good, T=-1), "T is negative")
    refused(copy_of(st, window=0), good, "window must be at least 1")
    refused(st, copy_of(good, autoreset=nat.AUTORESET_DISABLED), "autoreset must be next-step or same-step")
    refused(st, copy_of(good, autoreset=7), "autoreset must be next-step or same-step")
    refused(copy_of(st, num_envs=2**16), copy_of(good, N=2**16, T=2**15), "below 2^31")

    def refused_summary(state, dst, text):
        rc = L.mjs_monitor_summary(C.byref(state) if state is not None else None, dst, stream)
        err = L.mjs_last_error(None)
        assert rc == -1 and err.startswith(b"mjs_monitor_summary: ") and text.encode() in err, (text, rc, err)
        assert bool((out == -7).all()), text

    refused_summary(None, out.data_ptr(), "state is null")
    refused_summary(st, None, "out_dev is null")
    refused_summary(copy_of(st, struct_size=4), out.data_ptr(), "struct_size")
    refused_summary(copy_of(st, window=-1), out.data_ptr(), "window")
    refused_summary(copy_of(st, ring_length=None), out.data_ptr(), "the ring's")
    # ... and the descriptors as they stand are fine: T == 0 returns 0 and does nothing (without pointers), same-step needs no step_type
    assert L.mjs_monitor_update(C.byref(st), C.byref(nat.MjsMonitorBlock(T=0, N=N, autoreset=nat.AUTORESET_NEXT_STEP)), None, stream) == 0
    assert all(torch.equal(x, y) for x, y in zip(snapshot(mon), before))
    assert L.mjs_monitor_update(C.byref(copy_of(st, quota=None)), C.byref(copy_of(good, autoreset=nat.AUTORESET_SAME_STEP, step_type=None)), ws.data_ptr(), stream) == 0
    assert L.mjs_monitor_summary(C.byref(st), out.data_ptr(), stream) == 0
    assert float(out[0]) == min(mon.count, 4)
    mon.close()


# ---------------------------------------------------------------------------------------------- 4. a real env
N_ENV, T_ENV = 64, 120


def pointmass(N, mode, seed=5):
    import mujoco_sim_amd as m

    venv = m.HipVectorEnv("point_mass_reach", N, seed=seed, autoreset=mode)
    venv.reset()
    return venv


def small_actor(venv, seed=17):
    import mujoco_sim_amd as m

    return m.DeviceActor.from_linears(venv, *make_mlp(int(venv.obs_dim), [32], int(venv.action_dim), seed=seed, device=DEV))


def host_loop(venv, actor, z, mode):
    """T x (actor_actions; step_flat) with host accumulators written like HipSB3VecEnv.step_wait's, in float64: the records in (t, n) order."""
    N = venv.num_envs
    ep_return, ep_length, records = np.zeros(N, np.float64), np.zeros(N, np.int64), []
    for t in range(z.shape[0]):
        actions, _ = venv.actor_actions(actor, z=z[t])
        b = venv.step_flat(actions)
        h = {k: b[k].cpu().numpy() for k in BLOCK_KEYS}
        counting = np.ones(N, bool) if mode == "same_step" else h["step_type"] != FIRST
        ep_return[counting] += h["reward"][counting]
        ep_length[counting] += 1
        dones = (h["terminated"].astype(bool) | h["truncated"].astype(bool)) & counting
        for i in np.nonzero(dones)[0]:
            records.append((ep_return[i], int(ep_length[i]), int(h["is_success"][i]), int(i)))
            ep_return[i] = 0
            ep_length[i] = 0
    return records, ep_return, ep_length


@gpu
@pytest.mark.parametrize("mode", MODES)
def test_a_pointmass_block_equals_the_restatement_and_a_host_loop(mode):
    import mujoco_sim_amd as m

    venv, twin = pointmass(N_ENV, mode), pointmass(N_ENV, mode)
    actor = small_actor(venv)
    z = torch.randn(T_ENV, N_ENV, int(venv.action_dim), dtype=torch.float32, device=DEV, generator=torch.Generator(device=DEV).manual_seed(3))
    keep = BLOCK_KEYS + (("terminal_obs",) if mode == "same_step" else ())
    blk = venv.actor_rollout(actor, T_ENV, z=z, keep=keep)
    mon = m.DeviceEpisodeMonitor(venv, window=1000)
    mon.update(blk)
    ref = mref.RefMonitor(N_ENV, 1000)
    ref.update({k: blk[k].cpu().numpy() for k in BLOCK_KEYS}, mode)
    assert ref.cursor >= 2 * N_ENV  # episodes of at most 51 control steps: every env finishes two in 120
    assert_state(mon, ref, "restatement")
    records, ep_return, ep_length = host_loop(twin, actor, z, mode)
    ep = {k: v.cpu().numpy() for k, v in mon.episodes().items()}
    assert len(records) == len(ep["return"])
    assert np.array_equal(np.array([r[0] for r in records]).view(np.int64), ep["return"].view(np.int64))  # bit for bit
    assert [r[1] for r in records] == ep["length"].tolist() and [r[2] for r in records] == ep["success"].tolist() and [r[3] for r in records] == ep["env"].tolist()
    assert np.array_equal(ep_return.view(np.int64), mon.ep_return.cpu().numpy().view(np.int64)) and ep_length.tolist() == mon.ep_length.tolist()
    assert int(ep["length"].max()) <= 51
    print(f"{mode}: {len(records)} episodes, {int(ep['success'].sum())} of them successes, longest {int(ep['length'].max())}")
    # is_success on an end row describes the TERMINAL state in both modes: Pointmass terminates exactly on success, and under same-step
    # auto-reset the terminal observation (position, target) is within the goal threshold exactly where is_success is set
    ended = (blk["terminated"] | blk["truncated"]).bool() & ((blk["step_type"] != FIRST) | (mode == "same_step"))
    assert torch.equal(blk["is_success"][ended], blk["terminated"][ended]) and torch.equal(torch.from_numpy(ep["success"]), torch.from_numpy(ep["terminated"]))
    if mode == "same_step":
        term = blk["terminal_obs"][ended]
        dist = ((term[:, 0] - term[:, 2]) ** 2 + (term[:, 1] - term[:, 3]) ** 2).sqrt()
        near, far = dist[blk["is_success"][ended].bool()], dist[~blk["is_success"][ended].bool()]
        assert far.numel() and (not near.numel() or float(near.max()) < float(far.min()))
    mon.close()
    actor.close()
    venv.close()
    twin.close()


def sb3_evaluate(venv, actor, n_eval_episodes, mode):
    """stable_baselines3/common/evaluation.py evaluate_policy's loop over step_flat: per-env targets, the counters advance only for
    envs below their target, episodes append in env order within a step. (Next-step auto-reset: a FIRST row is the reset SB3's VecEnv
    never shows, so it is skipped.)"""
    N = venv.num_envs
    targets = mref.sb3_targets(n_eval_episodes, N)
    counts, cur_r, cur_l = np.zeros(N, dtype="int"), np.zeros(N), np.zeros(N, dtype="int")
    returns, lengths = [], []
    venv.reset()
    while (counts < targets).any():
        actions, _ = venv.actor_actions(actor, deterministic=True)
        b = venv.step_flat(actions)
        h = {k: b[k].cpu().numpy() for k in BLOCK_KEYS}
        for i in range(N):
            if counts[i] < targets[i] and (mode == "same_step" or h["step_type"][i] != FIRST):
                cur_r[i] += h["reward"][i]
                cur_l[i] += 1
                if h["terminated"][i] or h["truncated"][i]:
                    returns.append(float(cur_r[i]))
                    lengths.append(int(cur_l[i]))
                    counts[i] += 1
                    cur_r[i] = 0
                    cur_l[i] = 0
    return returns, lengths


@gpu
@pytest.mark.parametrize("mode", MODES)
def test_evaluate_policy_equals_sb3s_loop(mode):
    import mujoco_sim_amd as m

    venv, twin = pointmass(8, mode, seed=11), pointmass(8, mode, seed=11)
    actor = small_actor(venv)
    returns, lengths = m.evaluate_policy(venv, actor, n_eval_episodes=11, block_steps=16, return_episode_rewards=True)
    want_r, want_l = sb3_evaluate(twin, actor, 11, mode)
    assert len(returns) == 11 and np.array_equal(np.array(returns).view(np.int64), np.array(want_r).view(np.int64)) and lengths == want_l
    third = pointmass(8, mode, seed=11)  # (a second call on venv would go on in its generators' streams: other episodes)
    mean, std = m.evaluate_policy(third, actor, n_eval_episodes=11, block_steps=16)
    third.close()
    bound = 11 * 2.0 ** -52 * float(np.abs(want_r).sum())  # test_summary_against_numpy's bound on the sum; the mean is a smaller number still
    assert abs(mean - np.mean(want_r)) <= bound
    exact, numpy_err, bar = mref.std_bar(want_r)
    print(f"{mode}: std {std!r}, exact {exact!r}: numpy's error {numpy_err:.3e}, the kernel's {abs(std - exact):.3e}, bar {bar:.3e}")
    assert abs(std - exact) <= bar
    with pytest.raises(m.MjsError, match=r"\d+ of 11 episodes are missing after 4 control steps"):
        m.evaluate_policy(venv, actor, n_eval_episodes=11, block_steps=4, max_steps=4)
    actor.close()
    venv.close()
    twin.close()


# ---------------------------------------------------------------------------------------------- 5. DeviceSAC.learn
def trainer(mode="next_step"):
    import mujoco_sim_amd as m

    venv = m.HipVectorEnv("point_mass_reach", 64, seed=7, autoreset=mode)
    venv.reset(seed=3)
    D, A = int(venv.obs_dim), int(venv.action_dim)
    net = cref.make_actor(D, [64, 64], A, seed=81, device=DEV)
    q_nets = cref.make_q_nets(D, A, [64, 64], 2, seed=82, device=DEV)
    t = m.DeviceSAC(venv, m.DeviceActor.from_linears(venv, *net), m.DeviceCritic.from_linears(DEV, D, A, q_nets), buffer_size=8192, learning_starts=256, train_freq=8,
                    gradient_steps=2, batch_size=32, seed=11)
    return t, venv, net, q_nets


def learned(t, net, q_nets):
    t.actor.export(net)
    t.critic.export(q_nets)
    out = [p.detach().clone() for m_ in (*net[0], *net[1:]) for p in (m_.weight, m_.bias)] + [p.detach().clone() for q in q_nets for m_ in q for p in (m_.weight, m_.bias)]
    t.target_critic.export(q_nets)
    return out + [p.detach().clone() for q in q_nets for m_ in q for p in (m_.weight, m_.bias)] + [t.coef.log_ent_coef.clone(), t.coef.ent_coef.clone()]


def shut(t, venv, *more):
    actor, critic = t.actor, t.critic
    t.close()
    critic.close()
    actor.close()
    for obj in (venv, *more):
        obj.close()


KEYS = {"num_timesteps", "num_gradient_steps", "rollout/ep_rew_mean", "rollout/ep_len_mean", "rollout/success_rate", "eval/mean_reward", "eval/std_reward",
        "eval/success_rate", "eval/mean_ep_length"}
STEPS = 8 * 512  # 8 blocks of 8 steps x 64 envs: one warm-up block, then seven followed by two gradient steps each


@functools.lru_cache(maxsize=None)
def plain_run():
    """learn with every new argument at its default: the parameters afterwards (computed once, shared, left unchanged)."""
    t, venv, net, q_nets = trainer()
    t.learn(STEPS, generator=torch.Generator(device=DEV).manual_seed(21))
    out = learned(t, net, q_nets)
    assert t.log == []
    shut(t, venv)
    return out


@gpu
def test_learn_with_a_monitor_and_a_log_leaves_the_same_parameters():
    import mujoco_sim_amd as m

    t, venv, net, q_nets = trainer()
    mon = m.DeviceEpisodeMonitor(venv)
    ref, blocks, seen = mref.RefMonitor(64, 100), [], []
    collect, uniform = t.buffer.collect, t._collect_uniform

    def keep_block(blk):
        blocks.append({k: blk[k].cpu().numpy() for k in BLOCK_KEYS})
        return blk

    t.buffer.collect = lambda *a, **kw: keep_block(collect(*a, **kw))
    t._collect_uniform = lambda *a, **kw: keep_block(uniform(*a, **kw))
    t.learn(STEPS, generator=torch.Generator(device=DEV).manual_seed(21), monitor=mon, log_interval=2, callback=seen.append)
    assert all(torch.equal(a, b) for a, b in zip(learned(t, net, q_nets), plain_run()))  # bit for bit the run without them
    assert len(blocks) == 8 and t.num_timesteps == STEPS
    # a training phase follows every block (512 > learning_starts after the first); a record after every second one
    assert [r["num_timesteps"] for r in t.log] == [2 * 512, 4 * 512, 6 * 512, 8 * 512] and [r["num_gradient_steps"] for r in t.log] == [4, 8, 12, 16] and seen == t.log
    fed = 0
    for record in t.log:
        assert set(record) == KEYS
        while fed * 512 < record["num_timesteps"]:
            ref.update(blocks[fed], "next_step")
            fed += 1
        ret, length, success, _, _ = ref.live()
        assert len(ret) > 0
        bound = len(ret) * 2.0 ** -52 * float(np.abs(ret).sum())  # test_summary_against_numpy's bound on the sum, here on sum = mean * K
        assert abs(record["rollout/ep_rew_mean"] * len(ret) - float(ret.sum())) <= 2 * bound
        assert record["rollout/ep_len_mean"] == float(length.sum()) / len(length) and record["rollout/success_rate"] == float(success.sum()) / len(success)
        assert all(np.isnan(record[k]) for k in KEYS if k.startswith("eval/"))
    while fed < 8:
        ref.update(blocks[fed], "next_step")
        fed += 1
    assert_state(mon, ref, "every block was fed, the warm-up's included")
    shut(t, venv, mon)


@gpu
def test_learn_evaluates_on_a_second_env_and_on_its_own():
    import mujoco_sim_amd as m

    # a second env: the training env's trajectory, hence the learned parameters, are those of the plain run
    t, venv, net, q_nets = trainer()
    eval_env = m.HipVectorEnv("point_mass_reach", 16, seed=99)
    t.learn(STEPS, generator=torch.Generator(device=DEV).manual_seed(21), eval_env=eval_env, eval_freq=1024, n_eval_episodes=5)
    assert all(torch.equal(a, b) for a, b in zip(learned(t, net, q_nets), plain_run()))
    assert [r["num_timesteps"] for r in t.log] == [1024, 2048, 3072, 4096]
    for record in t.log:
        assert set(record) == KEYS and np.isnan(record["rollout/ep_rew_mean"])
        assert np.isfinite([record[k] for k in KEYS if k.startswith("eval/")]).all() and 1 <= record["eval/mean_ep_length"] <= 51 and record["eval/std_reward"] >= 0
    first_record = t.log[0]
    shut(t, venv, eval_env)
    # the first record is evaluate_policy of the actor after 1024 steps on a fresh env of the eval env's seed
    t, venv, net, q_nets = trainer()
    twin = m.HipVectorEnv("point_mass_reach", 16, seed=99)
    t.learn(1024, generator=torch.Generator(device=DEV).manual_seed(21))
    assert m.evaluate_policy(twin, t.actor, n_eval_episodes=5) == (first_record["eval/mean_reward"], first_record["eval/std_reward"])
    shut(t, venv, twin)
    # eval_env is the training env: it runs, the record holds both halves, and the in-flight accumulators are cleared after the evaluation
    t, venv, net, q_nets = trainer()
    mon = m.DeviceEpisodeMonitor(venv)
    t.learn(1024, generator=torch.Generator(device=DEV).manual_seed(21), monitor=mon, eval_env=venv, eval_freq=1024, n_eval_episodes=5)
    assert len(t.log) == 1 and t.log[0]["num_timesteps"] == 1024 and set(t.log[0]) == KEYS
    assert np.isfinite(t.log[0]["eval/mean_reward"]) and 1 <= t.log[0]["eval/mean_ep_length"] <= 51
    assert not bool(mon.ep_return.any()) and not bool(mon.ep_length.any())
    t.learn(512, generator=torch.Generator(device=DEV).manual_seed(22), monitor=mon)  # collection continues from the reset state: 8 steps in
    assert 0 < int(mon.ep_length.max()) <= 8  # (16 and more without the reset)
    shut(t, venv, mon)
