#!/usr/bin/env python3
"""The fused TD target (``sac_td_target``, csrc/mjs_critic.h: ONE launch) against the same computation as torch modules on the same
device tensors, in one process: the no-gradient half of SB3's ``SAC.train``,

    a', logp = actor.action_log_prob(next_obs);  y = r + (1 - done) * gamma * (min_c Q_c(next_obs, a') - ent_coef * logp)

for Robot-Reach's widths (D = 12, A = 3), two critics, ReLU, at B = 32 (the reference's batch_size), 256 (SB3's default) and 4096, with
actor / critic widths [64, 64] (the reference's net_arch) and [256, 256]. The torch side is what SB3 runs: ``nn.Sequential`` modules
under ``torch.no_grad()``, the squashed-Gaussian log-probability with epsilon 1e-6, ``torch.cat`` for the critics' input, ``torch.min``
over the stacked critics. Both sides get the same draws ``z`` and the entropy coefficient as a device tensor, and allocate their
outputs. Every timing is ``--calls`` calls back to back between two HIP events, the two paths alternating, ``--repeats`` times after
an untimed call of each; medians with every run. The results are compared first. The MI355X output is kept in
profiles/td_target_timing.txt.

  python tools/td_target_bench.py [--repeats 7] [--calls 200]"""
import argparse
import math
import sys
from pathlib import Path

import torch

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))
import mujoco_sim_amd as m  # noqa: E402

D, A, GAMMA = 12, 3, 0.99


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


def mlp(fan_in, widths, out):
    layers, d = [], fan_in
    for w in widths:
        layers += [torch.nn.Linear(d, w), torch.nn.ReLU()]
        d = w
    return torch.nn.Sequential(*layers, torch.nn.Linear(d, out)) if out else torch.nn.Sequential(*layers)


class TorchTarget:
    """SB3's modules and its train() lines, forward only."""

    def __init__(self, widths, dev):
        self.latent_pi = mlp(D, widths, 0).to(dev)
        self.mu, self.log_std = torch.nn.Linear(widths[-1], A).to(dev), torch.nn.Linear(widths[-1], A).to(dev)
        self.q_networks = [mlp(D + A, widths, 1).to(dev) for _ in range(2)]

    @torch.no_grad()
    def __call__(self, batch, ent_coef, z):
        next_obs = batch["next_obs"]
        latent = self.latent_pi(next_obs)
        mean, log_std = self.mu(latent), torch.clamp(self.log_std(latent), -20.0, 2.0)
        std = log_std.exp()
        gaussian = mean + std * z  # Normal(mean, std).rsample() with the draws given
        actions = torch.tanh(gaussian)
        log_prob = (-((gaussian - mean) ** 2) / (2 * std ** 2) - log_std - math.log(math.sqrt(2 * math.pi))).sum(dim=1)
        log_prob = log_prob - torch.sum(torch.log(1 - actions ** 2 + 1e-6), dim=1)
        q_in = torch.cat([next_obs, actions], dim=1)
        next_q = torch.cat([q(q_in) for q in self.q_networks], dim=1)
        next_q, _ = torch.min(next_q, dim=1, keepdim=True)
        next_q = next_q - ent_coef * log_prob.reshape(-1, 1)
        return (batch["rewards"].reshape(-1, 1) + (1 - batch["dones"].reshape(-1, 1)) * GAMMA * next_q).reshape(-1)


def flops(B, widths):
    """Multiply-adds x 2 of the three networks on B rows (the useful ones: no padding)."""
    def net(fan_in, out):
        total, d = 0, fan_in
        for w in (*widths, out):
            total += d * w
            d = w
        return total
    return 2 * B * (net(D, 2 * A) + 2 * net(D + A, 1))


def case(venv, widths, B, args):
    dev = venv.device
    torch.manual_seed(0)
    t = TorchTarget(widths, dev)
    hidden = [l for l in t.latent_pi if isinstance(l, torch.nn.Linear)]
    actor = m.DeviceActor.from_linears(venv, hidden, t.mu, t.log_std)
    critic = m.DeviceCritic.from_linears(dev, D, A, [[l for l in q if isinstance(l, torch.nn.Linear)] for q in t.q_networks])
    g = torch.Generator(device=dev).manual_seed(B)
    rn = lambda *s: torch.randn(*s, dtype=torch.float32, device=dev, generator=g)  # noqa: E731
    batch = {"next_obs": rn(B, D), "rewards": rn(B), "dones": (torch.arange(B, device=dev) % 7 == 0).float()}
    z = rn(B, A).clamp(-2.0, 2.0)
    ent = torch.tensor([0.005], dtype=torch.float32, device=dev)
    ours, theirs = m.sac_td_target(batch, actor, critic, GAMMA, ent, z=z), t(batch, ent, z)
    diff = (ours - theirs).abs().max().item()
    calls = args.calls
    (k_ms, t_ms), (k_runs, t_runs) = alternate([lambda: [m.sac_td_target(batch, actor, critic, GAMMA, ent, z=z) for _ in range(calls)],
                                                lambda: [t(batch, ent, z) for _ in range(calls)]], args.repeats)
    k_us, t_us = k_ms * 1e3 / calls, t_ms * 1e3 / calls
    per = lambda runs: [round(x * 1e3 / calls, 2) for x in runs]  # noqa: E731
    print(f"\nwidths {widths}, B = {B}: max |kernel - torch float32| of the target {diff:.3e}; {flops(B, widths) / 1e6:.3f} MFLOP per call")
    print(f"    sac_td_target (one launch)               : {k_us:10.2f} us per call  {flops(B, widths) / k_us / 1e6:9.4f} TFLOP/s   runs {per(k_runs)}")
    print(f"    torch modules (SB3's lines, no_grad)     : {t_us:10.2f} us per call  {flops(B, widths) / t_us / 1e6:9.4f} TFLOP/s   runs {per(t_runs)}")
    print(f"    torch / kernel: {t_us / k_us:.2f}x" + ("" if k_us <= t_us else "   ** THE KERNEL IS SLOWER **"))
    if not diff < 1e-3:
        raise SystemExit("the two paths disagree")
    actor.close()
    critic.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--calls", type=int, default=200)
    args = ap.parse_args()
    print(f"device: {torch.cuda.get_device_name(0)}; median of {args.repeats} alternating runs, each {args.calls} calls back to back between two HIP events; "
          f"host-side call overhead (Python, ctypes, torch's dispatcher) is inside both numbers")
    venv = m.HipVectorEnv("robot_reach", 16, seed=1)  # DeviceActor takes its device and action width from an env
    for widths in ([64, 64], [256, 256]):
        for B in (32, 256, 4096):
            case(venv, widths, B, args)
    venv.close()


if __name__ == "__main__":
    main()
