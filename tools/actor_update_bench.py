#!/usr/bin/env python3
"""The actor update on the device (``DeviceActorOptimizer.step``, csrc/mjs_actor_train.h: two launches, three with a learned entropy
coefficient) against the same lines of SB3's ``SAC.train`` in torch on the same device tensors, in one process:

    actions_pi, log_prob = actor.action_log_prob(obs);  min_qf_pi = min_c Q_c(obs, actions_pi)
    actor_loss = (ent_coef * log_prob - min_qf_pi).mean();  actor.optimizer.zero_grad();  actor_loss.backward();  actor.optimizer.step()

for Robot-Reach's widths (D = 12, A = 3), two critics, ReLU, at B = 32, 256 and 4096 with widths [64, 64] and [256, 256]. Four tables
per case: (1) ``step`` with a fixed coefficient against torch's lines, and what the torch route needs on top of them today, listed
separately: ``critic.export()`` before and ``actor.load()`` after; (2) ``step`` with a learned coefficient against torch's lines with the
ent_coef optimiser; (3) the HIP-event time of the launches through ctypes, with ``sac_td_target`` on the same shape next to the gradient
launch (one actor and two critic forward chains there; one actor forward, three critic forwards and three backward chains here);
(4) ``sac_gradient_step`` against the whole of SB3's lines in torch. Every timing is ``--calls`` calls back to back between two HIP events,
the paths alternating, ``--repeats`` times after an untimed call of each; medians with every run. No ratio is set beforehand: every one
is printed, and a slower kernel path is marked. The MI355X output is kept in profiles/actor_update_timing.txt.

  python tools/actor_update_bench.py [--repeats 7] [--calls 200]"""
import argparse
import ctypes as C
import math
import sys
from pathlib import Path

import torch

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tools"))
import mujoco_sim_amd as m  # noqa: E402
from critic_update_bench import TAU, TorchUpdate  # noqa: E402
from td_target_bench import GAMMA, A, D, TorchTarget, alternate  # noqa: E402


class TorchActorUpdate:
    """SB3's actor and ent_coef lines on TorchTarget's modules, with their Adam optimisers."""

    def __init__(self, t, dev):
        self.t = t
        self.params = [p for mod in (t.latent_pi, t.mu, t.log_std) for p in mod.parameters()]
        self.opt = torch.optim.Adam(self.params, lr=3e-4)
        self.log_ent_coef = torch.log(torch.ones(1, device=dev)).requires_grad_(True)
        self.ent_opt = torch.optim.Adam([self.log_ent_coef], lr=3e-4)
        self.target_entropy = -float(A)

    def sample(self, obs, z):
        t = self.t
        latent = t.latent_pi(obs)
        mean, log_std = t.mu(latent), torch.clamp(t.log_std(latent), -20.0, 2.0)
        std = log_std.exp()
        gaussian = mean + std * z
        actions = torch.tanh(gaussian)
        log_prob = (-((gaussian - mean) ** 2) / (2 * std ** 2) - log_std - math.log(math.sqrt(2 * math.pi))).sum(dim=1)
        return actions, log_prob - torch.sum(torch.log(1 - actions ** 2 + 1e-6), dim=1)

    def actor_step(self, obs, actions_pi, log_prob, ent_coef):
        q_in = torch.cat([obs, actions_pi], dim=1)
        min_qf_pi, _ = torch.min(torch.cat([q(q_in) for q in self.t.q_networks], dim=1), dim=1, keepdim=True)
        actor_loss = (ent_coef * log_prob.reshape(-1, 1) - min_qf_pi).mean()
        self.opt.zero_grad()
        actor_loss.backward()
        self.opt.step()

    def fixed(self, batch, ent, z):
        actions_pi, log_prob = self.sample(batch["obs"], z)
        self.actor_step(batch["obs"], actions_pi, log_prob, ent)

    def ent_step(self, log_prob):
        ent_coef = torch.exp(self.log_ent_coef.detach())
        ent_coef_loss = -(self.log_ent_coef * (log_prob + self.target_entropy).detach()).mean()
        self.ent_opt.zero_grad()
        ent_coef_loss.backward()
        self.ent_opt.step()
        return ent_coef

    def learned(self, batch, z):
        actions_pi, log_prob = self.sample(batch["obs"], z)
        self.actor_step(batch["obs"], actions_pi, log_prob, self.ent_step(log_prob))

    def train(self, upd, batch, z_next, z_pi):
        """SAC.train's lines for one gradient step, in SB3's order (upd: the critic side, TorchUpdate)."""
        actions_pi, log_prob = self.sample(batch["obs"], z_pi)
        ent_coef = self.ent_step(log_prob)
        upd.step(batch, self.t(batch, ent_coef, z_next))
        self.actor_step(batch["obs"], actions_pi, log_prob, ent_coef)
        upd.polyak()


def case(venv, widths, B, args):
    dev = venv.device
    torch.manual_seed(0)
    t = TorchTarget(widths, dev)
    hidden = [l for l in t.latent_pi if isinstance(l, torch.nn.Linear)]
    linears = [[l for l in q if isinstance(l, torch.nn.Linear)] for q in t.q_networks]
    actor = m.DeviceActor.from_linears(venv, hidden, t.mu, t.log_std)
    critic, target = m.DeviceCritic.from_linears(dev, D, A, linears), m.DeviceCritic.from_linears(dev, D, A, linears)
    a_opt, c_opt = m.DeviceActorOptimizer(actor), m.DeviceCriticOptimizer(critic)
    coef = m.DeviceEntropyCoef(dev, A)
    tor, upd = TorchActorUpdate(t, dev), TorchUpdate(t, dev)
    g = torch.Generator(device=dev).manual_seed(B)
    rn = lambda *s: torch.randn(*s, dtype=torch.float32, device=dev, generator=g)  # noqa: E731
    batch = {"obs": rn(B, D), "actions": torch.tanh(rn(B, A)), "next_obs": rn(B, D), "rewards": rn(B), "dones": (torch.arange(B, device=dev) % 7 == 0).float()}
    z, z_next = rn(B, A).clamp(-2.0, 2.0), rn(B, A).clamp(-2.0, 2.0)
    ent = torch.tensor([0.005], dtype=torch.float32, device=dev)

    # the two paths agree on one step from the same parameters (compared before anything is timed)
    a_opt.step(batch, critic, ent, z=z)
    tor.fixed(batch, ent, z)
    fresh = ([torch.nn.Linear(l.in_features, l.out_features).to(dev) for l in hidden], torch.nn.Linear(widths[-1], A).to(dev), torch.nn.Linear(widths[-1], A).to(dev))
    actor.export(fresh)
    ours = [p for l in (*fresh[0], fresh[1], fresh[2]) for p in (l.weight, l.bias)]
    theirs = [p for l in (*hidden, t.mu, t.log_std) for p in (l.weight, l.bias)]
    diff = max((a - b).abs().max().item() for a, b in zip(ours, theirs))

    calls = args.calls
    per = lambda runs: [round(x * 1e3 / calls, 2) for x in runs]  # noqa: E731
    us = lambda ms: ms * 1e3 / calls  # noqa: E731
    slower = lambda k, tt: "" if k <= tt else "   ** THE KERNEL IS SLOWER **"  # noqa: E731
    print(f"\nwidths {widths}, B = {B}: {sum(p.numel() for p in theirs)} actor parameters; max |kernel - torch float32| of a parameter after one step {diff:.3e}")

    fns = [lambda: [a_opt.step(batch, critic, ent, z=z) for _ in range(calls)], lambda: [tor.fixed(batch, ent, z) for _ in range(calls)],
           lambda: [critic.export() for _ in range(calls)], lambda: [actor.load() for _ in range(calls)]]
    (k, tt, ex, ld), (kr, tr, er, lr) = alternate(fns, args.repeats)
    print(f"  1. the actor update, fixed ent_coef\n    DeviceActorOptimizer.step (two launches)  : {us(k):10.2f} us per call   runs {per(kr)}")
    print(f"    torch (modules, backward, Adam)           : {us(tt):10.2f} us per call   runs {per(tr)}")
    print(f"    what the torch route needs besides: critic.export() {us(ex):.2f} us   runs {per(er)};   actor.load() {us(ld):.2f} us   runs {per(lr)}")
    print(f"    torch / kernel: {tt / k:.2f}x;   with export and load: {(tt + ex + ld) / k:.2f}x" + slower(k, tt))
    # (the load() calls above packed torch's parameters: both paths continue from torch's)

    (k, tt), (kr, tr) = alternate([lambda: [a_opt.step(batch, critic, coef, z=z) for _ in range(calls)], lambda: [tor.learned(batch, z) for _ in range(calls)]], args.repeats)
    print(f"  2. the actor update, learned ent_coef\n    DeviceActorOptimizer.step (three launches): {us(k):10.2f} us per call   runs {per(kr)}")
    print(f"    torch (as above, and the ent_coef lines)  : {us(tt):10.2f} us per call   runs {per(tr)}")
    print(f"    torch / kernel: {tt / k:.2f}x" + slower(k, tt))

    L, stream = actor._lib, torch.cuda.current_stream(dev).cuda_stream
    a = a_opt._args(batch["obs"], z, critic, B, 0.0, ent, None)
    grad_only = lambda: [L.mjs_actor_grad(actor._a, a_opt._o, C.byref(a), C.c_void_p(stream)) for _ in range(calls)]  # noqa: E731  (one launch: no outputs asked)
    both = lambda: [L.mjs_actor_update(a_opt._o, C.byref(a), 3e-4, C.c_void_p(stream)) for _ in range(calls)]  # noqa: E731
    td = lambda: [m.sac_td_target(batch, actor, target, GAMMA, ent, z=z_next) for _ in range(calls)]  # noqa: E731
    (gk, bk, fk), (gr, br, fr) = alternate([grad_only, both, td], args.repeats)
    print(f"  3. the launches, through ctypes (no tensor allocated)\n    grad_kernel alone                         : {us(gk):10.2f} us per call   runs {per(gr)}")
    print(f"    grad_kernel + adam_kernel                 : {us(bk):10.2f} us per call   runs {per(br)}   (adam_kernel: {us(bk - gk):.2f} us)")
    print(f"    sac_td_target (1 actor + 2 critic forward chains, allocates its output): {us(fk):10.2f} us per call   runs {per(fr)}")
    print(f"    grad_kernel / sac_td_target: {gk / fk:.2f}x   (1 actor forward, 3 critic forwards, 3 backward chains against 3 forward chains)")

    fns = [lambda: [m.sac_gradient_step(batch, actor, critic, target, c_opt, a_opt, coef, GAMMA, TAU, z_next=z_next, z_pi=z) for _ in range(calls)],
           lambda: [tor.train(upd, batch, z_next, z) for _ in range(calls)]]
    (k, tt), (kr, tr) = alternate(fns, args.repeats)
    print(f"  4. one whole gradient step, learned ent_coef\n    sac_gradient_step (seven launches)        : {us(k):10.2f} us per call   runs {per(kr)}")
    print(f"    torch (SAC.train's lines)                 : {us(tt):10.2f} us per call   runs {per(tr)}")
    print(f"    torch / kernel: {tt / k:.2f}x" + slower(k, tt))
    if not diff < 1e-4:
        raise SystemExit("the two paths disagree")
    for o in (a_opt, c_opt, target, critic, actor):
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
