"""Robot-Reach fast path with actuators that saturate and release inside a control step.

In the role-specialised substep loop (rr::kernel3 and rr::kernel<false, 2>) the wavefront that factorises the implicitfast
matrix works out only WHICH servos are force-clamped (actuator_clamp_mask, mjs_reach.h); the other one evaluates the forces.
The two must agree in every substep, or the matrix belongs to another set of clamped servos than the right-hand side. The
actions here jump between opposite corners of the task's action box every control step, so every control step starts
saturated and releases on the way; in one case a single lane of the wavefront does that while the other 63 hold still.

Everything is compared with the CPU oracle at the tolerances of test_gpu_parity.py (observations and rewards 1e-9, flags
bit-exact). The case itself is checked on the CPU, from the oracle alone, so the test cannot pass by leaving the fast path
or by never clamping: at least 90 % of the env-steps meet the fast path's conditions for their whole 64-env group (action in
the box, joints away from their ranges, short joint-space travel: the predicates of mjs_reach.h restated in numpy), and the
clamp masks, recomputed in numpy from the oracle's q and v of every substep and the constants of include/mjs_scene_spec.h,
contain clamped substeps, free substeps and changes between them inside the loop's substeps (1..19).
"""
import re
from pathlib import Path

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
ATOL = 1e-9
T_STEPS, NSUB, DRIVEN_LANE = 30, 20, 17
CASES = {"all_lanes_n64": (64, False), "all_lanes_n130": (130, False), "single_lane_n64": (64, True)}
_SPEC = (Path(__file__).resolve().parents[1] / "include" / "mjs_scene_spec.h").read_text()


def _spec(name):
    body = re.search(r"\b" + name + r"(?:\[[^\]]*\])*\s*=\s*\{?([^;]*?)\}?;", _SPEC, re.S).group(1)
    return np.array([float(x) for x in re.findall(r"-?\d+\.?\d*(?:[eE][-+]?\d+)?", body)])


KP, KD, FRC = _spec("MJS_UR_ACT_KP"), _spec("MJS_UR_ACT_KD"), _spec("MJS_UR_ACT_FRC")
JNT_RANGE, CTRL_RANGE = _spec("MJS_UR_JNT_RANGE").reshape(6, 2), _spec("MJS_UR_ACT_CTRLRANGE").reshape(6, 2)
BOX_LO, BOX_HI = _spec("MJS_RR_SPACE_LO"), _spec("MJS_RR_SPACE_HI")
CONTROL_DT, TCP_Z = float(_spec("MJS_RR_CONTROL_DT")[0]), float(_spec("MJS_G2F85_TCP_Z")[0])
TRAVEL2_MAX = 2.5  # mjs_reach.h
_cache = {}


def _servo_target(oracle_mod, tcp, guess):
    R = np.array([[1.0, 0, 0], [0, -1, 0], [0, 0, -1]])  # top-down TCP orientation
    T = np.eye(4)
    T[:3, :3] = R
    T[:3, 3] = np.asarray(tcp) - R[:, 2] * TCP_Z
    q = oracle_mod.ur5e_ik_closest(T, guess)
    return guess.copy() if q is None else q


def _case(oracle_mod, name):
    """The oracle's run of a case, computed once: actions, per-step results, the fast-path share and the clamp-mask history."""
    if name in _cache:
        return _cache[name]
    N, single = CASES[name]
    ob = oracle_mod.OracleBatch(oracle_mod.TASK_ROBOT_REACH, N, 11, time_limit=1e9, nthreads=8)
    replay = oracle_mod.OracleBatch(oracle_mod.TASK_ROBOT_REACH, N, 11, time_limit=1e9, nthreads=8)  # the same run, substep by substep
    o = ob.reset()
    replay.reset()
    reset_obs = o["obs"].copy()
    signs = np.array([[1, 1, 1], [1, 1, -1], [1, -1, 1], [1, -1, -1]])[np.arange(N) % 4]  # the box's four body diagonals
    far, back = np.where(signs > 0, BOX_HI, BOX_LO), np.where(signs > 0, BOX_LO, BOX_HI)
    driven = (np.arange(N) % 64 == DRIVEN_LANE) if single else np.ones(N, bool)
    actions, results, masks = [], [], []
    fast_env_steps = 0
    for t in range(T_STEPS):
        a = far if t % 2 == 0 else back
        a = np.where(driven[:, None], a, np.clip(o["obs"][:, 0:3], BOX_LO, BOX_HI))  # the others: their current TCP position
        q0, v0, _ = ob.get_state()
        q0, v0 = q0[:, :6], v0[:, :6]
        q1 = np.array([_servo_target(oracle_mod, a[i], q0[i]) for i in range(N)])
        # the fast path's guard (action_in_box, joint_near_range, travel_is_long), decided per 64-env group
        in_box = ((a >= BOX_LO) & (a <= BOX_HI)).all(axis=1)
        margin = 0.6 + CONTROL_DT * np.abs(v0)
        near = ((q0 - JNT_RANGE[:, 0] < margin) | (JNT_RANGE[:, 1] - q0 < margin)).any(axis=1)
        travel2 = ((np.abs(q1 - q0) + 0.05 * np.abs(v0)) ** 2).sum(axis=1)
        ok = in_box & ~near & (travel2 <= TRAVEL2_MAX)
        for g in range(0, N, 64):
            fast_env_steps += int(ok[g:g + 64].all()) * len(ok[g:g + 64])
        # the clamp mask of every substep: servo set-point lerp, ctrl clamp, force against the force limit
        t0 = replay.get_state()[2].copy()
        step_masks = []
        for s in range(NSUB):
            qs, vs, ts = replay.get_state()
            frac = np.clip(ts, t0, t0 + CONTROL_DT) - t0
            ctrl = np.clip(q0 + (q1 - q0) * (frac / CONTROL_DT)[:, None], CTRL_RANGE[:, 0], CTRL_RANGE[:, 1])
            f = KP * ctrl - KP * qs[:, :6] - KD * vs[:, :6]
            step_masks.append(~(np.abs(f) < FRC))
            for u in range(6):
                replay.set_ctrl(u, ctrl[:, u])
            replay.substeps(1)
        masks.append(step_masks)
        o = ob.step(a)
        qe, ve, _ = ob.get_state()
        qr, vr, _ = replay.get_state()
        assert np.abs(qe[:, :6] - qr[:, :6]).max() < 1e-9 and np.abs(ve[:, :6] - vr[:, :6]).max() < 1e-9, f"the substep replay left the oracle's trajectory at step {t}"
        actions.append(a)
        results.append(o)
    masks = np.array(masks)  # [T, NSUB, N, 6]
    _cache[name] = dict(N=N, driven=driven, reset_obs=reset_obs, actions=np.array(actions), results=results, masks=masks,
                        fast_share=fast_env_steps / (T_STEPS * N))
    return _cache[name]


@pytest.mark.parametrize("name", list(CASES))
@pytest.mark.parametrize("kernel_variant", [0, 2])
def test_saturating_servos_match_oracle(oracle_mod, name, kernel_variant):
    import mujoco_sim_amd as m

    c = _case(oracle_mod, name)
    N, masks = c["N"], c["masks"]
    # the case, from the oracle alone
    loop = masks[:, 1:]  # the role loop's substeps
    any_clamped = loop.any(axis=3)  # [T, 19, N]
    changed = (masks[:, 1:] != masks[:, :-1]).any(axis=3)  # against one substep earlier
    print(f"{name}: fast-path share {c['fast_share']:.3f}, clamped lane-substeps {int(any_clamped.sum())}, free {int((~any_clamped).sum())}, mask changes {int(changed.sum())}")
    assert c["fast_share"] >= 0.9, c["fast_share"]
    assert any_clamped.sum() > 0 and (~any_clamped).sum() > 0 and changed.sum() > 0
    assert (any_clamped.any(axis=1) & (~any_clamped).any(axis=1))[:, c["driven"]].any(), "no servo saturates and releases within one control step"
    if name.startswith("single_lane"):
        assert changed[:, :, c["driven"]].sum() > 0
        assert (changed[:, :, :64].sum(axis=2) == 1).any(), "no substep in which exactly one lane of the wavefront changes its mask"
    # the device against the oracle
    venv = m.HipVectorEnv("robot_reach", N, seed=11, time_limit=1e9, kernel_variant=kernel_variant)
    venv.reset()
    b = venv._buf
    np.testing.assert_allclose(b["obs"].cpu().numpy(), c["reset_obs"], rtol=0, atol=ATOL)
    for t in range(T_STEPS):
        venv.step(torch.from_numpy(c["actions"][t]))
        o = c["results"][t]
        g = {k: b[k].cpu().numpy() for k in ("obs", "reward", "discount", "step_type", "terminated", "truncated", "is_success", "ncon", "fault")}
        np.testing.assert_allclose(g["obs"], o["obs"], rtol=0, atol=ATOL, err_msg=f"obs step {t}")
        np.testing.assert_allclose(g["reward"], o["reward"], rtol=0, atol=ATOL, err_msg=f"reward step {t}")
        np.testing.assert_allclose(g["discount"], o["discount"], rtol=0, atol=0, err_msg=f"discount step {t}")
        for k in ("step_type", "terminated", "truncated", "is_success", "ncon"):
            assert np.array_equal(np.asarray(g[k]).astype(np.int64), np.asarray(o[k]).astype(np.int64)), (k, t)
        assert np.array_equal((g["fault"] & 1).astype(bool), o["fault"]) and np.array_equal((g["fault"] & 2).astype(bool), o["ik_failed"]), t
        assert not (g["fault"] & (4 | 8 | 16)).any(), (t, g["fault"])  # no constraint rows, no a-posteriori report
    venv.close()
