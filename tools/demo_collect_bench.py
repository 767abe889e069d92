#!/usr/bin/env python3
"""Demonstration-collection rate, two ways, in one process (Button-Push, joint actions, no images):
  (a) the host loop: the torch policy ``RobotPushButtonTask.demonstration_actions`` (about 25 elementwise launches + the IK launch)
      followed by ``HipVectorEnv.step``, once per control step from Python (also printed with ``step_flat``, the leanest
      loop Python can run);
  (b) ``HipVectorEnv.demonstration_rollout``: the policy kernel (csrc/mjs_policy.h, IK fused) + the step kernel per control
      step, enqueued by one native call.
Both are timed with HIP events after a warm-up, on the same handle settings and seed; prints the env-steps/s of each and their
ratio, and next to them the step launches alone (the open-loop rollout of the actions (b) chose). The MI355X output is kept in profiles/demo_rollout_timing.txt.

  python tools/demo_collect_bench.py [--envs 4096] [--steps 100] [--repeats 5]"""
import argparse
import sys
from pathlib import Path

import torch

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))
import mujoco_sim_amd as m  # noqa: E402


def timed(fn, repeats):
    """Median milliseconds of fn() between two HIP events; one untimed call first."""
    fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(repeats):
        start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        start.record()
        fn()
        end.record()
        end.synchronize()
        ms.append(start.elapsed_time(end))
    return sorted(ms)[len(ms) // 2], ms


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=4096)
    ap.add_argument("--steps", type=int, default=100)
    ap.add_argument("--repeats", type=int, default=5)
    args = ap.parse_args()
    N, T = args.envs, args.steps
    action_type = "absolute_joint_action"
    task = m.RobotPushButtonTask(observation_type="state_observations", action_type=action_type)
    venv = m.HipVectorEnv("robot_push_button", N, seed=1, action_type=action_type)

    def host_loop():
        venv.reset(seed=1)
        for _ in range(T):
            venv.step(task.demonstration_actions(venv))

    def host_loop_flat():  # the same with the zero-copy step: the leanest loop Python can run
        venv.reset(seed=1)
        for _ in range(T):
            venv.step_flat(task.demonstration_actions(venv))

    keep = ("obs", "reward", "is_success", "step_type")

    def device_rollout():
        venv.reset(seed=1)
        return venv.demonstration_rollout(T, keep=keep)

    actions = device_rollout()["actions"]

    def open_loop():  # the step launches alone, on the actions (b) chose: what the physics costs under this policy
        venv.reset(seed=1)
        venv.rollout(actions, keep=keep)

    a_ms, a_all = timed(host_loop, args.repeats)
    f_ms, f_all = timed(host_loop_flat, args.repeats)
    b_ms, b_all = timed(device_rollout, args.repeats)
    c_ms, c_all = timed(open_loop, args.repeats)
    a_rate, f_rate, b_rate, c_rate = (N * T / (ms * 1e-3) for ms in (a_ms, f_ms, b_ms, c_ms))
    print(f"device: {torch.cuda.get_device_name(0)}; Button-Push, {action_type}, {N} envs x {T} control steps, no images; median of {args.repeats} "
          f"(each: seeded reset + {T} steps), HIP events")
    print(f"(a) host loop   torch policy + step      : {a_ms:9.3f} ms  {a_rate / 1e6:8.3f} M env-steps/s   runs {[round(x, 2) for x in a_all]}")
    print(f"    host loop   torch policy + step_flat : {f_ms:9.3f} ms  {f_rate / 1e6:8.3f} M env-steps/s   runs {[round(x, 2) for x in f_all]}")
    print(f"(b) device loop demonstration_rollout    : {b_ms:9.3f} ms  {b_rate / 1e6:8.3f} M env-steps/s   runs {[round(x, 2) for x in b_all]}")
    print(f"    steps alone rollout of (b)'s actions : {c_ms:9.3f} ms  {c_rate / 1e6:8.3f} M env-steps/s   runs {[round(x, 2) for x in c_all]}")
    print(f"ratio (b) / (a): {b_rate / a_rate:.2f}x; against the step_flat loop: {b_rate / f_rate:.2f}x" + ("" if b_rate >= max(a_rate, f_rate) else "   ** (b) IS SLOWER **"))
    venv.close()


if __name__ == "__main__":
    main()
