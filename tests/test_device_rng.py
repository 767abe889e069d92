"""The per-env MT19937 streams on the device (csrc/mjs_dev_rng.h) against numpy's legacy RandomState itself and against the CPU
oracle, on a real MI355X: seeding, streams long enough to regenerate state that was already regenerated in place, a regeneration
at every position inside a reset (between its uniforms and between the two words of one uniform), draws inside the step kernel,
resets that consume a variable number of words, masked resets, and a checkpoint taken just before a regeneration.

Streams, cursors and drawn numbers are compared BITWISE. Observations that pass through IK or physics keep the tolerances of
test_gpu_parity.py. N = 70: one full wavefront and a partial one, so lanes 63 / 64 and the tail are all present. Injected
cursors lie in [0, 624], the range numpy's set_state accepts."""
import numpy as np
import pytest
import torch
from test_gpu_parity import ATOL, _compare, _gpu_result

pytestmark = pytest.mark.gpu
N = 70
POS = [0, 1, 311, 312, 615, 616, 617, 618, 619, 620, 621, 622, 623, 624]


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def _streams(venv):
    """(key uint32 [624, N], pos int32 [N]) of the device"""
    mt, pos = venv.get_rng_state()
    assert mt.dtype == torch.int32 and tuple(mt.shape) == (624, venv.num_envs) and pos.dtype == torch.int32
    return mt.cpu().numpy().view(np.uint32), pos.cpu().numpy()


def _inject(venv, key, pos):
    key, pos = np.ascontiguousarray(key, dtype=np.uint32), np.ascontiguousarray(pos, dtype=np.int32)
    assert ((pos >= 0) & (pos <= 624)).all()
    venv.set_rng_state((torch.from_numpy(key.view(np.int32)), torch.from_numpy(pos)))


def _numpy_streams(rss):
    st = [rs.get_state() for rs in rss]
    return np.stack([s[1] for s in st], axis=1), np.array([s[2] for s in st], dtype=np.int32)


def _assert_streams_equal(got, want, what):
    assert got[0].dtype == np.uint32 and want[0].dtype == np.uint32
    bad = np.nonzero(got[1] != want[1])[0]
    assert bad.size == 0, (what, "cursor", bad[:8], got[1][bad[:8]], want[1][bad[:8]])
    bad = np.nonzero((got[0] != want[0]).any(axis=0))[0]
    assert bad.size == 0, (what, "key words differ in envs", bad[:8])
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])


def _injected(cursors):
    """numpy streams RandomState(100 + i) advanced by 50 + i uniforms, cursor of env i overridden with cursors[i]"""
    rss = []
    for i in range(N):
        rs = np.random.RandomState(100 + i)
        rs.uniform(size=50 + i)
        rs.set_state(("MT19937", rs.get_state()[1], int(cursors[i])))
        rss.append(rs)
    key, pos = _numpy_streams(rss)
    assert np.array_equal(pos, np.asarray(cursors))  # numpy took the cursors as given
    return rss, key, pos


def _numpy_pointmass_resets(rss, n_resets):
    """[n_resets, N, 4] observations (px, py, gx, gy) of resets that draw gx, gy, px, py = uniform(-0.45, 0.45) in that order"""
    draws = np.stack([rs.uniform(-0.45, 0.45, size=(n_resets, 4)) for rs in rss], axis=1)
    return draws[:, :, [2, 3, 0, 1]]


# ------------------------------------------------------------------------------------------ a. seeding
@pytest.mark.parametrize("seed,offset", [(0, 0), (2025, 0), (2025, 1000), (2**32 - 3, 0), (2**32 - 40, 37)])
def test_seeding_equals_numpy(seed, offset):
    """env i <- RandomState((seed + env_index_offset + i) mod 2^32); the last two cases wrap inside the batch"""
    import mujoco_sim_amd as m

    venv = m.HipVectorEnv("point_mass_reach", N, seed=seed, env_index_offset=offset)
    want = _numpy_streams([np.random.RandomState((seed + offset + i) & 0xFFFFFFFF) for i in range(N)])
    assert (want[1] == 624).all()
    _assert_streams_equal(_streams(venv), want, (seed, offset))
    venv.close()


def test_reseeding_a_used_handle_equals_a_fresh_one():
    import mujoco_sim_amd as m

    s, offset = 2**32 - 40, 37
    venv = m.HipVectorEnv("point_mass_reach", N, seed=5, env_index_offset=offset)
    for _ in range(3):
        venv.reset()
    assert (_streams(venv)[1] == 24).all()
    venv.seed(s)
    fresh = m.HipVectorEnv("point_mass_reach", N, seed=s, env_index_offset=offset)
    want = _numpy_streams([np.random.RandomState((s + offset + i) & 0xFFFFFFFF) for i in range(N)])
    _assert_streams_equal(_streams(venv), want, "reseeded")
    _assert_streams_equal(_streams(fresh), want, "fresh")
    venv.reset()
    fresh.reset()
    assert np.array_equal(_bits(venv.flat_obs.cpu().numpy()), _bits(fresh.flat_obs.cpu().numpy()))
    venv.close()
    fresh.close()


# ------------------------------------------------------------------------------------------ b. a long stream
def test_pointmass_long_stream_equals_numpy():
    """170 resets = 1360 words per env: the regeneration of the seeded state and two more, of state that was regenerated in place"""
    import mujoco_sim_amd as m

    R = 170
    rss = [np.random.RandomState(2025 + i) for i in range(N)]
    want = _bits(_numpy_pointmass_resets(rss, R))
    venv = m.HipVectorEnv("point_mass_reach", N, seed=2025)
    for r in range(R):
        venv.reset()
        got = _bits(venv.flat_obs.cpu().numpy())
        assert np.array_equal(got, want[r]), (r, np.nonzero((got != want[r]).any(axis=1))[0][:8])
    want_streams = _numpy_streams(rss)
    assert (want_streams[1] == 8 * R - 2 * 624).all()
    _assert_streams_equal(_streams(venv), want_streams, "after the last reset")
    venv.close()


# ------------------------------------------------------------------------------------------ c. every alignment, injected
def test_pointmass_reset_across_every_alignment_of_the_block_boundary():
    """odd cursors split a uniform's two words across the regeneration; 617..623 put it after each of the reset's eight words"""
    import mujoco_sim_amd as m

    rss, key, pos = _injected([POS[i % len(POS)] for i in range(N)])
    venv = m.HipVectorEnv("point_mass_reach", N, seed=3)
    _inject(venv, key, pos)
    _assert_streams_equal(_streams(venv), (key, pos), "what was set is what is read")
    venv.reset()
    want = _bits(_numpy_pointmass_resets(rss, 1)[0])
    got = _bits(venv.flat_obs.cpu().numpy())
    assert np.array_equal(got, want), np.nonzero((got != want).any(axis=1))[0][:8]
    _assert_streams_equal(_streams(venv), _numpy_streams(rss), "after the reset")
    venv.close()


def test_robot_reach_reset_across_every_alignment_of_the_block_boundary(oracle_mod):
    """12 words per reset; the same injected states go into the oracle through its accessor"""
    import mujoco_sim_amd as m

    rss, key, pos = _injected([POS[i % len(POS)] for i in range(N)])
    venv = m.HipVectorEnv("robot_reach", N, seed=3)
    ob = oracle_mod.OracleBatch(oracle_mod.TASK_ROBOT_REACH, N, 4, nthreads=8)
    _inject(venv, key, pos)
    ob.set_rng_state((key, pos))
    venv.reset()
    o = ob.reset()
    g = _gpu_result(venv)
    assert np.array_equal(_bits(g["obs"][:, 9:12]), _bits(o["obs"][:, 9:12]))  # the target is drawn, not computed
    np.testing.assert_allclose(g["obs"][:, :9], o["obs"][:, :9], rtol=0, atol=ATOL)
    assert np.array_equal(g["ncon"], o["ncon"]) and (g["step_type"] == 0).all()
    after = _streams(venv)
    _assert_streams_equal(after, ob.rng_state(), "device against oracle")
    for rs in rss:  # numpy itself: robot xyz, then target xyz; the bounds do not matter to the stream
        rs.uniform(size=6)
    _assert_streams_equal(after, _numpy_streams(rss), "device against numpy")
    venv.close()


# ------------------------------------------------------------------------------------------ d. a boundary inside an episode
@pytest.mark.parametrize("autoreset", ["next_step", "same_step"])
def test_button_disturbance_draws_cross_the_block_boundary_mid_episode(oracle_mod, autoreset):
    """bp::disturb draws one uniform(0, 1) at the end of a step, but only while the switch is active and not pressed
    (robot_push_button.py:159-165), so each env starts drawing at its own time. The demonstration policy's 0.5 m/s limit does not
    reach a switch within 16 steps; the scripted action here aims straight into the switch and, once it is active, hovers 0.1 m
    above it, computed from the oracle's observations and fed to both sides. Cursors 600..623 are injected after the first reset,
    so the draws of the steps cross the regeneration."""
    import mujoco_sim_amd as m

    T = 16
    venv = m.HipVectorEnv("robot_push_button", N, seed=2025, autoreset=autoreset, action_type="absolute_eef_action", button_disturbances=True)
    ob = oracle_mod.OracleBatch(oracle_mod.TASK_BUTTON_PUSH, N, 2025, autoreset={"next_step": 0, "same_step": 1}[autoreset], nthreads=8,
                                action_type=1, button_disturbances=True)
    venv.reset()
    o = ob.reset()
    key, pos = _streams(venv)
    _assert_streams_equal((key, pos), ob.rng_state(), "after the first reset")
    injected = (600 + np.arange(N) % 24).astype(np.int32)
    _inject(venv, key, injected)
    ob.set_rng_state((key, injected))
    prev = injected
    uneven = False
    for t in range(T):
        sw, active = o["obs"][:, 9:12], o["obs"][:, 12] > 0.5
        a = np.zeros((N, 4))
        a[:, :3] = sw
        a[:, 2] = np.where(active, sw[:, 2] + 0.1, sw[:, 2] - 0.005)
        venv.step(torch.from_numpy(a))
        o = ob.step(a)
        g = _gpu_result(venv)
        _compare(t, g, o)
        assert np.array_equal((g["fault"] & 1).astype(bool), o["fault"]) and np.array_equal((g["fault"] & 2).astype(bool), o["ik_failed"])
        cur = venv.get_rng_state()[1].cpu().numpy()
        assert np.array_equal(cur, ob.rng_state()[1]), ("cursor", t)
        used = (cur - prev) % 624
        assert np.isin(used, (0, 2)).all(), (t, used)  # no reset within these steps: at most the one uniform of the disturbance
        uneven |= bool((used == 2).any() and (used == 0).any())
        prev = cur
    _assert_streams_equal(_streams(venv), ob.rng_state(), "after the last step")
    assert (prev < injected).any()  # some env's cursor wrapped: its draws crossed the regeneration
    assert uneven                   # some env drew in a step in which another did not: the cursors are per env
    venv.close()


# ------------------------------------------------------------------------------------------ e. variable consumption
@pytest.mark.parametrize("block_shape,n_objects", [("box", 2), ("mesh", 5)])
def test_planar_push_rejection_sampling_consumes_what_the_oracle_consumes(oracle_mod, block_shape, n_objects):
    """Inline resets (kernel_variant 1; the default variant is pinned to it bit for bit by
    test_planar_push_prepared_episodes_equal_inline_resets). Block positions are redrawn until nothing touches, so a contact count
    that differs from the oracle's in one attempt shifts every later draw: the streams must be equal after every reset. Seed 21
    gives rejection rounds in both configurations (oracle alone: 10+ of 70 envs per reset with two boxes, 29+ with five meshes).
    Observations as in test_planar_push_parity_with_oracle: 1e-8 on the envs whose 150 settle steps the oracle itself reproduces
    under a 1e-13 perturbation."""
    import ctypes as C

    import mujoco_sim_amd as m

    mesh = block_shape == "mesh"
    minimum = 2 * (3 * n_objects * mesh + 3 + 3 + 3 * n_objects)  # words of a reset without a rejection round
    knob = C.c_double.in_dll(oracle_mod.lib(), "om_dbg_perturb")
    venv = m.HipVectorEnv("robot_planar_push", N, seed=21, kernel_variant=1, n_objects=n_objects, block_shape=block_shape)
    okw = dict(nthreads=8, n_objects=n_objects, block_shape=0 if mesh else 1)
    ob = oracle_mod.OracleBatch(oracle_mod.TASK_PLANAR_PUSH, N, 21, **okw)
    ob2 = oracle_mod.OracleBatch(oracle_mod.TASK_PLANAR_PUSH, N, 21, **okw)
    key, pos = _streams(venv)
    _assert_streams_equal((key, pos), ob.rng_state(), "as seeded")
    injected = (560 + np.arange(N) % 64).astype(np.int32)
    _inject(venv, key, injected)
    ob.set_rng_state((key, injected))
    ob2.set_rng_state((key, injected))
    prev = injected
    n_rejected = n_wrapped = 0
    for r in range(3):
        venv.reset()
        o = ob.reset()
        try:
            knob.value = 1e-13
            o2 = ob2.reset()
        finally:
            knob.value = 0.0
        after = _streams(venv)
        _assert_streams_equal(after, ob.rng_state(), f"reset {r}")
        g = _gpu_result(venv)
        for k in ("step_type", "terminated", "truncated", "is_success"):
            assert np.array_equal(np.asarray(g[k]).astype(int), np.asarray(o[k]).astype(int)), (k, r)
        assert np.array_equal(_bits(g["obs"][:, 3:5]), _bits(o["obs"][:, 3:5])), r  # the target is drawn, not computed
        ok = np.abs(o["obs"] - o2["obs"]).max(axis=1) <= 1e-10
        assert ok.mean() > 0.5, (r, ok.mean())
        np.testing.assert_allclose(g["obs"][ok], o["obs"][ok], rtol=0, atol=1e-8, err_msg=f"obs reset {r}")
        assert np.array_equal(np.asarray(g["ncon"])[ok], o["ncon"][ok]), r
        used = (after[1] - prev) % 624  # (a reset of more than 624 words would need 18+ rounds)
        assert (used >= minimum).all() and ((used - minimum) % (6 * n_objects) == 0).all(), (r, used)
        n_rejected += int((used > minimum).sum())
        n_wrapped += int((after[1] < prev).sum())
        prev = after[1]
    assert n_rejected > 0  # a rejection round happened
    assert n_wrapped > 0   # and a reset crossed the regeneration
    venv.close()


# ------------------------------------------------------------------------------------------ f. masked resets
MASKED = [("point_mass_reach", {}, 8), ("robot_reach", {}, 12), ("robot_push_button", {}, 12),
          ("robot_push_button", {"gripper_model": "articulated"}, 12), ("robot_planar_push", {"kernel_variant": 1}, None)]


@pytest.mark.parametrize("task,kw,words", MASKED, ids=[t + "".join(f"-{v}" for v in kw.values()) for t, kw, _ in MASKED])
def test_masked_reset_consumes_nothing_for_masked_out_envs(oracle_mod, task, kw, words):
    import mujoco_sim_amd as m

    venv = m.HipVectorEnv(task, N, seed=21, **kw)
    venv.reset()
    before, out_before, state_before = _streams(venv), _gpu_result(venv), venv.get_state().cpu().numpy()
    # an all-zero mask changes nothing at all
    venv.reset(mask=torch.zeros(N, dtype=torch.bool))
    _assert_streams_equal(_streams(venv), before, "all-zero mask")
    out = _gpu_result(venv)
    for k, v in out_before.items():
        assert np.array_equal(out[k].view(np.uint8), v.view(np.uint8)), ("all-zero mask", k)
    assert np.array_equal(_bits(venv.get_state().cpu().numpy()), _bits(state_before))
    # every third env starts a new episode
    mask = np.arange(N) % 3 == 0
    venv.reset(mask=torch.from_numpy(mask))
    after, out = _streams(venv), _gpu_result(venv)
    assert np.array_equal(after[0][:, ~mask], before[0][:, ~mask]) and np.array_equal(after[1][~mask], before[1][~mask])
    for k, v in out_before.items():
        assert np.array_equal(out[k][~mask].view(np.uint8), v[~mask].view(np.uint8)), ("masked-out outputs", k)
    assert (out["obs"][mask] != out_before["obs"][mask]).any(axis=1).all()  # the others did get a new episode
    if words is not None:
        assert np.array_equal(after[1][mask], before[1][mask] + words)  # (the second reset of a stream: no regeneration yet)
        assert np.array_equal(after[0], before[0])
    else:  # Planar-Push: as many words as the oracle's rejection sampling takes
        ob = oracle_mod.OracleBatch(oracle_mod.TASK_PLANAR_PUSH, N, 21, nthreads=8)
        ob.reset()
        _assert_streams_equal(before, ob.rng_state(), "after the full reset")
        ob.reset_envs(np.nonzero(mask)[0])
        _assert_streams_equal(after, ob.rng_state(), "after the masked reset")
        assert (after[1][mask] != before[1][mask]).all()
    venv.close()


# ------------------------------------------------------------------------------------------ g. checkpoint across a boundary
def test_pointmass_checkpoint_taken_just_before_a_regeneration():
    import mujoco_sim_amd as m

    rss, key, pos = _injected([616 + i % 8 for i in range(N)])
    a_env = m.HipVectorEnv("point_mass_reach", N, seed=11)
    a_env.reset()
    a_env.step(torch.from_numpy(np.random.RandomState(1).uniform(-0.05, 0.05, (N, 2))))
    _inject(a_env, key, pos)
    saved = (a_env.get_state().clone(), tuple(t.clone() for t in a_env.get_rng_state()))
    b_env = m.HipVectorEnv("point_mass_reach", N, seed=999)
    b_env.set_state(saved[0])
    b_env.set_rng_state(saved[1])
    _assert_streams_equal(_streams(b_env), (key, pos), "loaded")
    want = _bits(_numpy_pointmass_resets(rss, 1)[0])
    for env in (a_env, b_env):
        env.reset()
        assert np.array_equal(_bits(env.flat_obs.cpu().numpy()), want)
        _assert_streams_equal(_streams(env), _numpy_streams(rss), "after the reset")
    assert torch.equal(a_env.get_state(), b_env.get_state())
    act = torch.from_numpy(np.random.RandomState(2).uniform(-0.05, 0.05, (N, 2)))
    for env in (a_env, b_env):
        env.step(act)
    assert np.array_equal(_bits(a_env.flat_obs.cpu().numpy()), _bits(b_env.flat_obs.cpu().numpy()))
    a_env.close()
    b_env.close()
