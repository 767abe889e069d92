"""Robot-Reach role loop: the integration of a substep runs at the top of the next iteration, the fallback leaves by a side door.

In the role-specialised substep loop (rr::kernel3 and rr::kernel<false, 2>, mjs_reach.h role_loop) each role's iteration is
the integration of the previous substep's qacc followed by the role's own block, one scheduling region; the first block is
peeled, one integration follows the loop, and the dq2 > 0.01 fallback (exact sincos) leaves the region by a wave-uniform
test behind the block: a cold copy redoes the block for the lanes that need it. What can go wrong: a carried cos / sin pair
(state rows 22-33) that misses or doubles a rotation (off by |dq| ~ 1e-3), a fallback whose block still belongs to the
rotated pair, a fallback taken by one lane only, the pairs after an episode's reset, and the hand-over to the
single-wavefront tail (which happens between the peeled block's inputs and the loop).

Everything is compared with the CPU oracle at the tolerances of test_gpu_parity.py (observations and rewards 1e-9, flags and
ncon bit-exact). The cases are checked on the CPU from the oracle alone (its q and v of every substep, the predicates of
mjs_reach.h restated in numpy as in test_reach_clamp_mask.py), so a case cannot pass by leaving the fast path.

Case 5: corner-to-corner actions alone never make travel_is_long true (their travel^2 stays below 1.8 of the 2.5 allowed); the
driven lane also gets a wrist velocity of 15 rad/s on joints 3-5, which adds 3 x (0.05 x 15)^2 to the sum.
"""
import numpy as np
import pytest
import torch

from test_reach_clamp_mask import BOX_HI, BOX_LO, CONTROL_DT, JNT_RANGE, TRAVEL2_MAX, _servo_target

pytestmark = pytest.mark.gpu
ATOL = 1e-9
CS_ATOL = 1e-13   # carried pair against cos / sin of the stored angle (rotate_small drifts ~1e-15 over a control step)
EXACT_ATOL = 2.0 ** -52  # a reset writes sincos itself: one ulp of a value below 1 between the device's and numpy's functions
NSUB, PHYSICS_DT, DRIVEN_LANE = 20, CONTROL_DT / 20, 17
S_WARM, S_CS, S_SN = 16, 22, 28
SPIN = 25.0  # rad/s on the base joint: dq = 0.125 rad per substep, dq^2 = 0.0156 > 0.01 until the servo has braked it below 20
_FLAG_KEYS = ("step_type", "terminated", "truncated", "is_success", "ncon")


def _in_box(rs, n):
    return rs.uniform(BOX_LO, BOX_HI, (n, 3))


def _guard_ok(oracle_mod, ob, a):
    """Per env: the fast path's predicates (action_in_box, joint_near_range, travel_is_long) and travel^2, from the oracle's state."""
    q0, v0, _ = ob.get_state()
    q0, v0 = q0[:, :6], v0[:, :6]
    q1 = np.array([_servo_target(oracle_mod, a[i], q0[i]) for i in range(len(a))])
    in_box = ((a >= BOX_LO) & (a <= BOX_HI)).all(axis=1)
    margin = 0.6 + CONTROL_DT * np.abs(v0)
    near = ((q0 - JNT_RANGE[:, 0] < margin) | (JNT_RANGE[:, 1] - q0 < margin)).any(axis=1)
    travel2 = ((np.abs(q1 - q0) + 0.05 * np.abs(v0)) ** 2).sum(axis=1)
    return in_box & ~near, travel2, q0, q1


def _substep_dq2(replay, q0, q1):
    """sum(dq^2) of each of the 20 substeps of one control step, [NSUB, N], from a second oracle stepped substep by substep."""
    t0 = replay.get_state()[2].copy()
    out = []
    for _ in range(NSUB):
        qa, _, ts = replay.get_state()
        frac = (np.clip(ts, t0, t0 + CONTROL_DT) - t0) / CONTROL_DT
        ctrl = q0 + (q1 - q0) * frac[:, None]
        for u in range(6):
            replay.set_ctrl(u, ctrl[:, u])
        replay.substeps(1)
        qb = replay.get_state()[0]
        out.append(((qb[:, :6] - qa[:, :6]) ** 2).sum(axis=1))
    return np.array(out)


def _inject(venv, ob, q, v, replay=None):
    """the same joints into the device (mjs_set_state) and the oracle (its debug setter zeroes qacc_warmstart)"""
    gs = venv.get_state().clone()
    gs[0:6] = torch.from_numpy(np.ascontiguousarray(q.T))
    gs[6:12] = torch.from_numpy(np.ascontiguousarray(v.T))
    gs[S_WARM:S_WARM + 6] = 0.0
    gs[-1] = torch.from_numpy((gs[-1].cpu().numpy().astype(np.uint8) | 16).astype(np.float64))
    venv.set_state(gs)
    ob.set_robot_state(q, v)
    if replay is not None:
        replay.set_robot_state(q, v)


def _check_step(venv, o, tag, allow_robust=False):
    b = venv._buf
    g = {k: b[k].cpu().numpy() for k in ("obs", "reward", "discount", "fault") + _FLAG_KEYS}
    print(f"{tag}: max |obs - oracle| {np.abs(g['obs'] - o['obs']).max():.3e}, max |reward - oracle| {np.abs(g['reward'] - o['reward']).max():.3e}")
    np.testing.assert_allclose(g["obs"], o["obs"], rtol=0, atol=ATOL, err_msg=f"obs {tag}")
    np.testing.assert_allclose(g["reward"], o["reward"], rtol=0, atol=ATOL, err_msg=f"reward {tag}")
    np.testing.assert_allclose(g["discount"], o["discount"], rtol=0, atol=0, err_msg=f"discount {tag}")
    for k in _FLAG_KEYS:
        assert np.array_equal(np.asarray(g[k]).astype(np.int64), np.asarray(o[k]).astype(np.int64)), (k, tag)
    assert np.array_equal((g["fault"] & 1).astype(bool), o["fault"]) and np.array_equal((g["fault"] & 2).astype(bool), o["ik_failed"]), tag
    if not allow_robust:
        assert not (g["fault"] & (4 | 8 | 16)).any(), (tag, g["fault"])


def _check_cache(venv, tag, atol=CS_ATOL):
    s = venv.get_state().cpu().numpy()
    q = s[0:6]
    dc, ds = np.abs(s[S_CS:S_CS + 6] - np.cos(q)).max(axis=1), np.abs(s[S_SN:S_SN + 6] - np.sin(q)).max(axis=1)
    print(f"{tag}: max |row - cos q| per joint {dc}, max |row - sin q| {ds}")
    assert (dc <= atol).all() and (ds <= atol).all(), (tag, dc, ds)


def _pair(oracle_mod, m, N, seed, kernel_variant, **kw):
    venv = m.HipVectorEnv("robot_reach", N, seed=seed, kernel_variant=kernel_variant, **kw)
    ob = oracle_mod.OracleBatch(oracle_mod.TASK_ROBOT_REACH, N, seed, nthreads=8, **kw)
    venv.reset()
    o = ob.reset()
    np.testing.assert_allclose(venv._buf["obs"].cpu().numpy(), o["obs"], rtol=0, atol=ATOL)
    return venv, ob, o


@pytest.mark.parametrize("N", [1, 64, 70])
@pytest.mark.parametrize("kernel_variant", [0, 2])
def test_carried_pair_stays_consistent(oracle_mod, N, kernel_variant):
    """Case 1: ten control steps of in-box actions; after every step the carried pairs of all six joints belong to the stored angles."""
    import mujoco_sim_amd as m

    venv, ob, _ = _pair(oracle_mod, m, N, 23, kernel_variant, time_limit=1e9)
    rs = np.random.RandomState(5)
    fast = 0
    for t in range(10):
        a = _in_box(rs, N)
        ok, travel2, _, _ = _guard_ok(oracle_mod, ob, a)
        fast += int((ok & (travel2 <= TRAVEL2_MAX)).all())
        venv.step(torch.from_numpy(a))
        _check_step(venv, ob.step(a), f"N {N} variant {kernel_variant} step {t}")
        _check_cache(venv, f"N {N} variant {kernel_variant} step {t}")
    assert fast == 10, fast  # every step met the fast path's conditions for all its envs
    venv.close()


def _spin_case(oracle_mod, m, N, kernel_variant, single):
    venv, ob, o = _pair(oracle_mod, m, N, 11, kernel_variant, time_limit=1e9)
    replay = oracle_mod.OracleBatch(oracle_mod.TASK_ROBOT_REACH, N, 11, nthreads=8, time_limit=1e9)
    replay.reset()
    driven = (np.arange(N) % 64 == DRIVEN_LANE) if single else np.ones(N, bool)
    q, v = o["obs"][:, 3:9].copy(), np.zeros((N, 6))
    v[driven, 0] = SPIN
    _inject(venv, ob, q, v, replay)
    a = np.clip(o["obs"][:, 0:3], BOX_LO, BOX_HI)  # the current TCP position (a reset may leave it a hair outside the box)
    # the case, from the oracle alone: the whole group is on the fast path, and the fallback stops holding inside the loop
    ok, travel2, q0, q1 = _guard_ok(oracle_mod, ob, a)
    assert ok.all() and (travel2 <= TRAVEL2_MAX).all(), (ok, travel2)
    exact = _substep_dq2(replay, q0, q1) > 0.01  # [NSUB, N]
    first_fast = np.array([int(np.argmin(exact[:, i])) for i in range(N)])
    print(f"first substep without the fallback, driven lanes: {first_fast[driven]}")
    assert exact[0:2, driven].all(), "the fallback must hold in substep 0 and in the loop's first substep"
    assert ((first_fast[driven] >= 2) & (first_fast[driven] <= 18)).all() and not exact[19, driven].any(), "the crossing must lie inside substeps 1..19"
    assert not exact[:, ~driven].any()
    if single:
        assert (exact[:, :64].sum(axis=1) == 1).any(), "no substep in which exactly one lane of the wavefront takes the fallback"
    venv.step(torch.from_numpy(a))
    tag = f"spin N {N} variant {kernel_variant} single {single}"
    _check_step(venv, ob.step(a), tag)
    _check_cache(venv, tag)
    # one more step from where the spin left the arm (the driven lanes' TCP is outside the box now: clipped target, any path)
    a = np.clip(venv._buf["obs"].cpu().numpy()[:, 0:3], BOX_LO, BOX_HI)
    venv.step(torch.from_numpy(a))
    _check_step(venv, ob.step(a), tag + " step 1", allow_robust=True)
    _check_cache(venv, tag + " step 1")
    venv.close()


@pytest.mark.parametrize("N", [64, 70])
@pytest.mark.parametrize("kernel_variant", [0, 2])
def test_fallback_stops_inside_the_loop(oracle_mod, N, kernel_variant):
    """Case 2: every lane spins its base joint at 25 rad/s; dq2 > 0.01 holds for the first substeps and stops holding inside 1..19."""
    import mujoco_sim_amd as m

    _spin_case(oracle_mod, m, N, kernel_variant, single=False)


@pytest.mark.parametrize("kernel_variant", [0, 2])
def test_fallback_of_a_single_lane(oracle_mod, kernel_variant):
    """Case 3: one lane of 64 spins, the other 63 hold still: the wave-uniform exit is taken for one lane's sake."""
    import mujoco_sim_amd as m

    _spin_case(oracle_mod, m, 64, kernel_variant, single=True)


@pytest.mark.parametrize("kernel_variant", [0, 2])
def test_episode_end_and_reset(oracle_mod, kernel_variant):
    """Case 4: N = 70, default time limit, 101 control steps with the next-step auto-reset: parity across the reset, exact rows after it."""
    import mujoco_sim_amd as m

    N = 70
    venv, ob, _ = _pair(oracle_mod, m, N, 31, kernel_variant)
    rs = np.random.RandomState(9)
    for t in range(101):
        a = _in_box(rs, N)
        venv.step(torch.from_numpy(a))
        o = ob.step(a)
        _check_step(venv, o, f"variant {kernel_variant} step {t}")
        if t == 99:
            assert (np.asarray(o["step_type"]) == 2).all() and o["truncated"].all()  # the time limit ends every episode here
            _check_cache(venv, f"variant {kernel_variant} last step")
    assert (np.asarray(o["step_type"]) == 0).all()  # step 100 is the reset step
    _check_cache(venv, f"variant {kernel_variant} reset step", atol=EXACT_ATOL)
    venv.close()


@pytest.mark.parametrize("kernel_variant", [0, 2])
def test_long_travel_hand_over(oracle_mod, kernel_variant):
    """Case 5: one lane's joint-space travel is long (known after the IK, i.e. after substep 0 in rr::kernel3): the group goes to the solo tail."""
    import mujoco_sim_amd as m

    N = 64
    venv, ob, o = _pair(oracle_mod, m, N, 11, kernel_variant, time_limit=1e9)
    signs = np.array([[1, 1, 1], [1, 1, -1], [1, -1, 1], [1, -1, -1]])[np.arange(N) % 4]
    far, back = np.where(signs > 0, BOX_HI, BOX_LO), np.where(signs > 0, BOX_LO, BOX_HI)
    for t in range(4):
        a = far if t % 2 == 0 else back
        if t == 2:  # the driven lane's wrist spins: its travel is long, everything known at kernel entry is still fine
            q, v, _ = ob.get_state()
            q, v = q[:, :6].copy(), v[:, :6].copy()
            v[DRIVEN_LANE, 3:6] = 15.0
            _inject(venv, ob, q, v)
        if t <= 2:  # the case, from the oracle alone (step 3 only follows the solo tail's result, on whatever path)
            ok, travel2, _, _ = _guard_ok(oracle_mod, ob, a)
            long_lanes = np.where(travel2 > TRAVEL2_MAX)[0]
            print(f"step {t}: travel^2 max {travel2.max():.3f}, long lanes {long_lanes}")
            assert ok.all(), (t, ok)
            assert list(long_lanes) == ([DRIVEN_LANE] if t == 2 else []), (t, long_lanes)
        venv.step(torch.from_numpy(a))
        _check_step(venv, ob.step(a), f"variant {kernel_variant} step {t}", allow_robust=(t >= 2))
        _check_cache(venv, f"variant {kernel_variant} step {t}")
    venv.close()
