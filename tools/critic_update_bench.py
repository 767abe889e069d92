#!/usr/bin/env python3
"""The critic update on the device (``DeviceCriticOptimizer.step``, csrc/mjs_critic_train.h: two launches) against the same lines of
SB3's ``SAC.train`` in torch on the same device tensors, in one process:

    current_q = critic(obs, actions);  critic_loss = 0.5 * sum(F.mse_loss(q, y) for q in current_q)
    critic.optimizer.zero_grad();  critic_loss.backward();  critic.optimizer.step()                  # torch.optim.Adam, default settings

for Robot-Reach's widths (D = 12, A = 3), two critics, ReLU, at B = 32, 256 and 4096 with widths [64, 64] and [256, 256]. Three tables
per case: (1) ``step`` against torch's lines; (2) the HIP-event time of the two launches separately (``gradients`` without outputs is
the first launch plus the small ordered-sum launch; step minus that is Adam's share), and the forward ``q_values`` launch as the floor: a
backward pass is two more products per layer, so about 3x the floor plus the Adam pass over the parameter bytes; (3) the full gradient
step ``sac_td_target`` + ``step`` + ``blend_from`` against its torch equivalent (the target under no_grad, the lines above, polyak).
Every timing is ``--calls`` calls back to back between two HIP events, the paths alternating, ``--repeats`` times after an untimed call of
each; medians with every run. The MI355X output is kept in profiles/critic_update_timing.txt.

  python tools/critic_update_bench.py [--repeats 7] [--calls 200]"""
import argparse
import sys
from pathlib import Path

import torch
import torch.nn.functional as F

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tools"))
import mujoco_sim_amd as m  # noqa: E402
from td_target_bench import GAMMA, A, D, TorchTarget, alternate  # noqa: E402

TAU = 0.005


class TorchUpdate:
    """SB3's critic lines on TorchTarget's q networks, its Adam, and a target copy for polyak_update."""

    def __init__(self, t, dev):
        self.t = t
        self.params = [p for q in t.q_networks for p in q.parameters()]
        self.opt = torch.optim.Adam(self.params, lr=3e-4)
        self.target_params = [p.detach().clone() for p in self.params]

    def step(self, batch, y):
        q_in = torch.cat([batch["obs"], batch["actions"]], dim=1)
        current_q = [q(q_in) for q in self.t.q_networks]
        loss = 0.5 * sum(F.mse_loss(q, y.reshape(-1, 1)) for q in current_q)
        self.opt.zero_grad()
        loss.backward()
        self.opt.step()

    def polyak(self):
        with torch.no_grad():  # stable_baselines3.common.utils.polyak_update
            torch._foreach_mul_(self.target_params, 1 - TAU)
            torch._foreach_add_(self.target_params, self.params, alpha=TAU)

    def full(self, batch, ent, z):
        self.step(batch, self.t(batch, ent, z))
        self.polyak()


def case(venv, widths, B, args):
    dev = venv.device
    torch.manual_seed(0)
    t = TorchTarget(widths, dev)
    hidden = [l for l in t.latent_pi if isinstance(l, torch.nn.Linear)]
    linears = [[l for l in q if isinstance(l, torch.nn.Linear)] for q in t.q_networks]
    actor = m.DeviceActor.from_linears(venv, hidden, t.mu, t.log_std)
    critic, target = m.DeviceCritic.from_linears(dev, D, A, linears), m.DeviceCritic.from_linears(dev, D, A, linears)
    opt = m.DeviceCriticOptimizer(critic)
    upd = TorchUpdate(t, dev)
    g = torch.Generator(device=dev).manual_seed(B)
    rn = lambda *s: torch.randn(*s, dtype=torch.float32, device=dev, generator=g)  # noqa: E731
    batch = {"obs": rn(B, D), "actions": torch.tanh(rn(B, A)), "next_obs": rn(B, D), "rewards": rn(B), "dones": (torch.arange(B, device=dev) % 7 == 0).float()}
    z, y = rn(B, A).clamp(-2.0, 2.0), rn(B)
    ent = torch.tensor([0.005], dtype=torch.float32, device=dev)

    # the two paths agree on one step from the same parameters (compared before anything is timed)
    opt.step(batch, y)
    upd.step(batch, y)
    ours = [p for net in critic.export([[torch.nn.Linear(l.in_features, l.out_features).to(dev) for l in net] for net in linears]) for l in net for p in (l.weight, l.bias)]
    theirs = [p for net in linears for l in net for p in (l.weight, l.bias)]
    diff = max((a - b).abs().max().item() for a, b in zip(ours, theirs))

    calls = args.calls
    per = lambda runs: [round(x * 1e3 / calls, 2) for x in runs]  # noqa: E731
    us = lambda ms: ms * 1e3 / calls  # noqa: E731
    n_par = sum(p.numel() for p in theirs)
    print(f"\nwidths {widths}, B = {B}: {n_par} parameters; max |kernel - torch float32| of a parameter after one step {diff:.3e}")

    (k, tt), (kr, tr) = alternate([lambda: [opt.step(batch, y) for _ in range(calls)], lambda: [upd.step(batch, y) for _ in range(calls)]], args.repeats)
    print(f"  1. the critic update\n    DeviceCriticOptimizer.step (two launches): {us(k):10.2f} us per call   runs {per(kr)}")
    print(f"    torch (modules, mse_loss, backward, Adam): {us(tt):10.2f} us per call   runs {per(tr)}")
    print(f"    torch / kernel: {tt / k:.2f}x" + ("" if k <= tt else "   ** THE KERNEL IS SLOWER **"))

    L, stream = critic._lib, torch.cuda.current_stream(dev).cuda_stream
    import ctypes as C
    a = opt._args(batch["obs"], batch["actions"], y, B, None, None)
    grad_only = lambda: [L.mjs_critic_grad(critic._q, opt._o, C.byref(a), C.c_void_p(stream)) for _ in range(calls)]  # noqa: E731  (one launch: no outputs asked)
    both = lambda: [L.mjs_critic_update(opt._o, C.byref(a), 3e-4, C.c_void_p(stream)) for _ in range(calls)]  # noqa: E731
    fwd = lambda: [critic.q_values(batch["obs"], batch["actions"]) for _ in range(calls)]  # noqa: E731
    (gk, bk, fk), (gr, br, fr) = alternate([grad_only, both, fwd], args.repeats)
    print(f"  2. the launches, through ctypes (no tensor allocated)\n    grad_kernel alone                        : {us(gk):10.2f} us per call   runs {per(gr)}")
    print(f"    grad_kernel + adam_kernel                : {us(bk):10.2f} us per call   runs {per(br)}   (adam_kernel: {us(bk - gk):.2f} us)")
    print(f"    q_values (forward q_kernel, the floor)   : {us(fk):10.2f} us per call   runs {per(fr)}")
    print(f"    grad_kernel / floor: {gk / fk:.2f}x   update / floor: {bk / fk:.2f}x")

    def ours_full():
        for _ in range(calls):
            opt.step(batch, m.sac_td_target(batch, actor, target, GAMMA, ent, z=z))
            target.blend_from(critic, TAU)

    (k, tt), (kr, tr) = alternate([ours_full, lambda: [upd.full(batch, ent, z) for _ in range(calls)]], args.repeats)
    print(f"  3. the full gradient step of the critic\n    sac_td_target + step + blend_from        : {us(k):10.2f} us per call   runs {per(kr)}")
    print(f"    torch (target, update, polyak_update)    : {us(tt):10.2f} us per call   runs {per(tr)}")
    print(f"    torch / kernel: {tt / k:.2f}x" + ("" if k <= tt else "   ** THE KERNEL IS SLOWER **"))
    if not diff < 1e-4:
        raise SystemExit("the two paths disagree")
    for o in (opt, target, critic, actor):
        o.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--calls", type=int, default=200)
    args = ap.parse_args()
    print(f"device: {torch.cuda.get_device_name(0)}; median of {args.repeats} alternating runs, each {args.calls} calls back to back between two HIP events; "
          f"host-side call overhead (Python, ctypes, torch's dispatcher) is inside every number")
    venv = m.HipVectorEnv("robot_reach", 16, seed=1)  # DeviceActor takes its device and action width from an env
    for widths in ([64, 64], [256, 256]):
        for B in (32, 256, 4096):
            case(venv, widths, B, args)
    venv.close()


if __name__ == "__main__":
    main()
