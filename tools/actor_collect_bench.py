#!/usr/bin/env python3
"""Closed-loop rollout under a learned MLP actor (SAC's squashed Gaussian), two ways, in one process (Robot-Reach, state observations):
  (a) the host loop: the torch module in float32 (forward, sample, tanh, unscale: a dozen launches) followed by
      ``HipVectorEnv.step_flat``, once per control step from Python;
  (b) ``HipVectorEnv.actor_rollout``: the actor kernel (csrc/mjs_actor.h) + the step kernel per control step, enqueued by one
      native call;
and the actor launch alone against torch's forward alone (HIP events around a batch of launches), for the default kernel
(16 envs per workgroup, 16x16x4 MFMA) and the 32-env variant (32x32x2). (a) and (b) alternate, repeat by repeat, on the same
handle settings and seed; medians are printed with every run next to them. The MI355X output is kept in
profiles/actor_rollout_timing.txt.

  python tools/actor_collect_bench.py [--envs 4096] [--steps 200] [--repeats 5]"""
import argparse
import sys
from pathlib import Path

import torch

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))
import mujoco_sim_amd as m  # noqa: E402
from mujoco_sim_amd import _native as nat  # noqa: E402


def event_ms(fn):
    start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    fn()
    end.record()
    end.synchronize()
    return start.elapsed_time(end)


def alternate(fns, repeats):
    """Milliseconds of each fn, interleaved (a, b, a, b, ...) after one untimed call of each: ([median...], [[runs]...])."""
    for fn in fns:
        fn()
    torch.cuda.synchronize()
    runs = [[] for _ in fns]
    for _ in range(repeats):
        for k, fn in enumerate(fns):
            runs[k].append(event_ms(fn))
    return [sorted(r)[len(r) // 2] for r in runs], runs


class TorchActor(torch.nn.Module):
    """The module SB3 builds for SAC (latent_pi, mu, log_std) and its action for an env: sample, squash, unscale."""

    def __init__(self, in_dim, net_arch, A):
        super().__init__()
        layers, d = [], in_dim
        for w in net_arch:
            layers += [torch.nn.Linear(d, w), torch.nn.ReLU()]
            d = w
        self.latent_pi = torch.nn.Sequential(*layers)
        self.mu, self.log_std = torch.nn.Linear(d, A), torch.nn.Linear(d, A)

    @torch.no_grad()
    def forward(self, obs32, z):
        h = self.latent_pi(obs32)
        return torch.tanh(self.mu(h) + self.log_std(h).clamp(-20.0, 2.0).exp() * z)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=4096)
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--repeats", type=int, default=5)
    args = ap.parse_args()
    N, T = args.envs, args.steps
    venv = m.HipVectorEnv("robot_reach", N, seed=1)
    dev = venv.device
    low = torch.tensor(venv.action_low, dtype=torch.float64, device=dev)
    span = torch.tensor(venv.action_high, dtype=torch.float64, device=dev) - low
    keep = ("obs", "reward", "is_success", "step_type")
    print(f"device: {torch.cuda.get_device_name(0)}; Robot-Reach, {N} envs x {T} control steps, state observations (12 inputs, 3 actions); "
          f"median of {args.repeats} alternating runs (each: seeded reset + {T} steps), HIP events")
    for arch in ([64, 64], [256, 256]):
        torch.manual_seed(0)
        net = TorchActor(venv.obs_dim, arch, venv.action_dim).to(dev)
        actors = {"16-env tiles, 16x16x4 (default)": m.DeviceActor.from_sb3(venv, net),
                  "32-env tiles, 32x32x2": m.DeviceActor.from_sb3(venv, net, variant=nat.ACTOR_VARIANT_TILE32)}
        actor = actors["16-env tiles, 16x16x4 (default)"]
        z = torch.randn(T, N, venv.action_dim, dtype=torch.float32, device=dev)

        def host_loop():
            venv.reset(seed=1)
            for t in range(T):
                a = net(venv.flat_obs.float(), z[t])
                venv.step_flat(low + 0.5 * (a.double() + 1.0) * span)

        def device_loop():
            venv.reset(seed=1)
            return venv.actor_rollout(actor, T, z=z, keep=keep)

        actions = device_loop()["actions"]

        def open_loop():  # the step launches alone, on the actions (b) chose
            venv.reset(seed=1)
            venv.rollout(actions, keep=keep)

        (a_ms, b_ms, c_ms), (a_all, b_all, c_all) = alternate((host_loop, device_loop, open_loop), args.repeats)
        us = lambda ms: ms * 1e3 / T  # noqa: E731
        print(f"\nactor {arch}:")
        print(f"(a) host loop   torch actor + step_flat : {a_ms:9.3f} ms  {us(a_ms):8.2f} us/control step  {N * T / a_ms / 1e3:8.3f} M env-steps/s   runs {[round(x, 2) for x in a_all]}")
        print(f"(b) device loop actor_rollout           : {b_ms:9.3f} ms  {us(b_ms):8.2f} us/control step  {N * T / b_ms / 1e3:8.3f} M env-steps/s   runs {[round(x, 2) for x in b_all]}")
        print(f"    steps alone rollout of (b)'s actions: {c_ms:9.3f} ms  {us(c_ms):8.2f} us/control step  {N * T / c_ms / 1e3:8.3f} M env-steps/s   runs {[round(x, 2) for x in c_all]}")
        print(f"ratio (b) / (a): {a_ms / b_ms:.2f}x" + ("" if b_ms <= a_ms else "   ** (b) IS SLOWER **")
              + f"; the actor inside the device loop, (b) - steps alone: {us(b_ms) - us(c_ms):.2f} us/control step")
        # the policy alone: `reps` calls back to back between two events (the larger of the host's enqueue time and the device's)
        venv.reset(seed=1)
        reps = 200
        obs32 = venv.flat_obs.float()
        out = torch.empty(N, venv.action_dim, dtype=torch.float64, device=dev)
        fns = [lambda: [net(obs32, z[0]) for _ in range(reps)],
               lambda: [low + 0.5 * (net(venv.flat_obs.float(), z[0]).double() + 1.0) * span for _ in range(reps)]]
        names = ["torch forward alone (float32 in, squashed out)", "torch forward + cast + unscale (what (a) runs)"]
        L, (lo_c, hi_c), stream = nat.lib(), venv._action_bounds(), venv._stream()
        sq = torch.empty(N, venv.action_dim, dtype=torch.float32, device=dev)
        for name, act_ in actors.items():  # the bare native call: Python adds about 2 us per enqueue, less than the kernel takes
            fns.append(lambda act_=act_: [L.mjs_actor_actions(venv._h, act_._a, venv.flat_obs.data_ptr(), z[0].data_ptr(), lo_c, hi_c, out.data_ptr(),
                                                              sq.data_ptr(), stream) for _ in range(reps)])
            names.append(f"actor launch, {name}")
        med, runs = alternate(fns, args.repeats)
        for name, ms, r in zip(names, med, runs):
            print(f"    {name:48s}: {ms * 1e3 / reps:8.2f} us per call   runs {[round(x * 1e3 / reps, 2) for x in r]}")
        for act_ in actors.values():
            act_.close()
    venv.close()


if __name__ == "__main__":
    main()
