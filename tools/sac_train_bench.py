#!/usr/bin/env python3
"""The native gradient loop (``DeviceSAC.train``, one ``mjs_sac_train`` call for G steps; csrc/mjs_sac_train.h) against the route a user had
to write before it: a Python loop of ``buffer.sample(B)`` + ``sac_gradient_step(...)`` with torch's default draws, on the same filled buffer,
in one process.

Part 1, per widths ([64, 64], [256, 256]) and B (32, 256, 4096), D = 12, A = 3, two critics, ReLU, learned coefficient: G = ``--steps``
gradient steps between two HIP events, host side included in both, the two routes alternating, ``--repeats`` times after an untimed run of
each; medians with every run. Then ``draw_batch`` alone (one launch, fresh output tensors) against ``torch.randint`` + ``sample`` + two
``torch.randn``. Part 2: one ``learn`` run on Robot-Reach with 4096 envs at ``train_freq=1, gradient_steps=1`` and at ``gradient_steps=64``:
env-steps/s and gradient steps/s, wall clock around a synchronised run. No ratio is set beforehand: every one is printed, and a slower
native loop is marked. The MI355X output is kept in profiles/sac_train_timing.txt.

  python tools/sac_train_bench.py [--repeats 7] [--steps 200] [--learn-blocks 64]"""
import argparse
import sys
import time
from pathlib import Path

import torch

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tools"))
import mujoco_sim_amd as m  # noqa: E402
from td_target_bench import GAMMA, A, D, alternate, mlp  # noqa: E402

TAU = 0.005


def networks(venv, widths):
    dev = venv.device
    latent = mlp(D, widths, 0).to(dev)
    mu, log_std = torch.nn.Linear(widths[-1], A).to(dev), torch.nn.Linear(widths[-1], A).to(dev)
    q_nets = [[l for l in mlp(D + A, widths, 1).to(dev) if isinstance(l, torch.nn.Linear)] for _ in range(2)]
    actor = m.DeviceActor.from_linears(venv, [l for l in latent if isinstance(l, torch.nn.Linear)], mu, log_std)
    return actor, m.DeviceCritic.from_linears(dev, D, A, q_nets)


def case(venv, buffer, widths, B, args):
    torch.manual_seed(0)
    actor, critic = networks(venv, widths)
    trainer = m.DeviceSAC(venv, actor, critic, buffer=buffer, batch_size=B, gamma=GAMMA, tau=TAU)
    # the parent route's objects: networks of their own from the same seed, the same buffer
    torch.manual_seed(0)
    p_actor, p_critic = networks(venv, widths)
    p_target = m.DeviceCritic.from_linears(venv.device, D, A, p_critic.q_nets)
    c_opt, a_opt, coef = m.DeviceCriticOptimizer(p_critic), m.DeviceActorOptimizer(p_actor), m.DeviceEntropyCoef(venv.device, A)
    G = args.steps

    def python_loop():
        for _ in range(G):
            batch = buffer.sample(B)
            m.sac_gradient_step(batch, p_actor, p_critic, p_target, c_opt, a_opt, coef, GAMMA, TAU)

    def python_draws():
        for _ in range(G):
            buffer.sample(B, draws=torch.randint(0, 2**62, (B,), dtype=torch.int64, device=venv.device))
            torch.randn(B, A, dtype=torch.float32, device=venv.device)
            torch.randn(B, A, dtype=torch.float32, device=venv.device)

    per = lambda runs: [round(x * 1e3 / G, 2) for x in runs]  # noqa: E731
    us = lambda ms: ms * 1e3 / G  # noqa: E731
    (n, p), (nr, pr) = alternate([lambda: trainer.train(G), python_loop], args.repeats)
    print(f"\nwidths {widths}, B = {B}")
    print(f"  DeviceSAC.train({G}): one native call          : {us(n):10.2f} us per gradient step   runs {per(nr)}")
    print(f"  Python loop of sample + sac_gradient_step     : {us(p):10.2f} us per gradient step   runs {per(pr)}")
    print(f"  Python loop / native loop: {p / n:.2f}x" + ("" if n <= p else "   ** THE NATIVE LOOP IS SLOWER **"))
    (n, p), (nr, pr) = alternate([lambda: [trainer.draw_batch() for _ in range(G)], python_draws], args.repeats)
    print(f"  draw_batch alone (one launch, fresh tensors)  : {us(n):10.2f} us per batch   runs {per(nr)}")
    print(f"  torch.randint + sample + 2 x torch.randn      : {us(p):10.2f} us per batch   runs {per(pr)}")
    print(f"  five launches / one launch: {p / n:.2f}x" + ("" if n <= p else "   ** THE FUSED DRAW IS SLOWER **"))
    trainer.close()
    for o in (c_opt, a_opt, p_target, p_critic, p_actor, critic, actor):
        o.close()


def learn_run(gradient_steps, args):
    venv = m.HipVectorEnv("robot_reach", 4096, seed=1)
    venv.reset(seed=2)
    torch.manual_seed(0)
    actor, critic = networks(venv, [64, 64])
    trainer = m.DeviceSAC(venv, actor, critic, buffer_size=1_000_000, batch_size=256, train_freq=1, gradient_steps=gradient_steps, learning_starts=4096 * 4)
    g = torch.Generator(device=venv.device).manual_seed(3)
    trainer.learn(4096 * 8, generator=g)  # the warm-up, the one read of the size and the first training phases: untimed
    torch.cuda.synchronize()
    steps0, grads0, t0 = trainer.num_timesteps, trainer.num_gradient_steps, time.perf_counter()
    trainer.learn(4096 * args.learn_blocks, generator=g)
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    env_steps, grad_steps = trainer.num_timesteps - steps0, trainer.num_gradient_steps - grads0
    print(f"  train_freq=1, gradient_steps={gradient_steps:3d}: {env_steps} env steps and {grad_steps} gradient steps in {dt:.3f} s: "
          f"{env_steps / dt:12.0f} env-steps/s, {grad_steps / dt:9.0f} gradient steps/s")
    trainer.close()
    critic.close()
    actor.close()
    venv.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--learn-blocks", type=int, default=64)
    args = ap.parse_args()
    print(f"device: {torch.cuda.get_device_name(0)}; part 1: median of {args.repeats} alternating runs, each {args.steps} gradient steps between two HIP "
          f"events; host-side overhead (Python, ctypes, torch's dispatcher and allocator) is inside every number")
    venv = m.HipVectorEnv("robot_reach", 1024, seed=1)
    venv.reset(seed=2)
    torch.manual_seed(0)
    filler, filler_critic = networks(venv, [64, 64])
    buffer = m.DeviceReplayBuffer(venv, 200_000)
    g = torch.Generator(device=venv.device).manual_seed(1)
    for _ in range(8):
        buffer.collect(venv, filler, 16, generator=g)
    print(f"buffer: {buffer.size} of {buffer.capacity} rows filled from Robot-Reach")
    for widths in ([64, 64], [256, 256]):
        for B in (32, 256, 4096):
            case(venv, buffer, widths, B, args)
    filler_critic.close()
    filler.close()
    buffer.close()
    venv.close()
    print(f"\npart 2: learn on Robot-Reach, 4096 envs, [64, 64] networks, batch 256, {args.learn_blocks} timed blocks of one control step (wall clock, synchronised)")
    for gradient_steps in (1, 64):
        learn_run(gradient_steps, args)


if __name__ == "__main__":
    main()
