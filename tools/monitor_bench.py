#!/usr/bin/env python3
"""Episode statistics on the device (``DeviceEpisodeMonitor``, ``evaluate_policy``; csrc/mjs_monitor.h) against the routes a user had before
them, in one process.

Part 1, ``update`` on one block of Robot-Reach (4096 envs x 200 steps) and of Pointmass (4096 x 51), both auto-reset modes' rule on the
next-step block: four launches against a torch restatement with no Python loop over N - a loop over T with masked ``torch.where``
accumulators and a boolean-mask append of the finished episodes (each of which reads a count back). HIP events around the calls, and wall
time around a synchronised call; the two routes alternate, ``--repeats`` times after an untimed run of each; medians with every run.
Part 2, ``evaluate_policy`` with 4096 episodes on 4096 Pointmass envs against a step-by-step host loop (``actor_actions`` + ``step_flat``, one
device-to-host copy per control step, numpy accumulators like ``HipSB3VecEnv.step_wait``'s; the exported-model route adds SB3's own policy
forward and Python on top of this). Part 3, ``learn`` on Robot-Reach, 4096 envs, one gradient step per control step, with the monitor fed
and no records, against the same ``learn`` with every new argument at its default (the parent's launches), alternating. Part 4, the
summary's standard deviation against an exact recomputation, next to numpy's own error (tests/test_monitor_device.py). No ratio is set
beforehand: every one is printed, and a slower device route is marked. The MI355X output is kept in profiles/monitor_timing.txt.

  python tools/monitor_bench.py [--repeats 7] [--learn-blocks 64]"""
import argparse
import sys
import time
from pathlib import Path

import numpy as np
import torch

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tools"))
sys.path.insert(0, str(ROOT / "tests"))
import mujoco_sim_amd as m  # noqa: E402
from sac_train_bench import networks  # noqa: E402
from td_target_bench import alternate  # noqa: E402

FIRST = 0


def wall_ms(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3


def small_actor(venv, seed=0):
    torch.manual_seed(seed)
    D, A, dev = int(venv.obs_dim), int(venv.action_dim), venv.device
    hidden = [torch.nn.Linear(D, 32).to(dev)]
    return m.DeviceActor.from_linears(venv, hidden, torch.nn.Linear(32, A).to(dev), torch.nn.Linear(32, A).to(dev))


class TorchMonitor:
    """The rules in torch, vectorised over N: a Python loop over T, masked accumulators, boolean-mask append."""

    def __init__(self, N, dev):
        self.ep_return, self.ep_length = torch.zeros(N, dtype=torch.float64, device=dev), torch.zeros(N, dtype=torch.int32, device=dev)
        self.env = torch.arange(N, dtype=torch.int32, device=dev)
        self.records = []

    def update(self, blk, same_step):
        reward, ended, success = blk["reward"], (blk["terminated"] | blk["truncated"]) != 0, blk["is_success"]
        for t in range(reward.shape[0]):
            counting = torch.ones_like(ended[t]) if same_step else blk["step_type"][t] != FIRST
            self.ep_return = torch.where(counting, self.ep_return + reward[t], self.ep_return)
            self.ep_length = torch.where(counting, self.ep_length + 1, self.ep_length)
            end = counting & ended[t]
            self.records.append((self.ep_return[end], self.ep_length[end], success[t][end], self.env[end]))
            self.ep_return = torch.where(end, 0.0, self.ep_return)
            self.ep_length = torch.where(end, 0, self.ep_length)

    def returns(self):
        return torch.cat([r[0] for r in self.records])


def update_case(task, T, args):
    N = 4096
    venv = m.HipVectorEnv(task, N, seed=1)
    venv.reset(seed=2)
    actor = small_actor(venv)
    blk = venv.actor_rollout(actor, T, generator=torch.Generator(device=venv.device).manual_seed(3))
    mon = m.DeviceEpisodeMonitor(venv, window=100)
    ref = TorchMonitor(N, venv.device)
    mon.update(blk)
    ref.update(blk, False)
    episodes = mon.count
    check = m.DeviceEpisodeMonitor(venv, window=max(episodes, 1))
    check.update(blk)
    same = episodes == len(ref.returns()) and torch.equal(check.episodes()["return"], ref.returns())
    print(f"\n{task}, one block of {N} envs x {T} steps: {episodes} finished episodes; the two routes' returns are " + ("equal bit for bit" if same else "** DIFFERENT **"))

    def device():
        mon.update(blk)

    def restated():
        ref.records.clear()
        ref.update(blk, False)

    (d, r), (dr, rr) = alternate([device, restated], args.repeats)
    rnd = lambda runs: [round(x * 1e3, 1) for x in runs]  # noqa: E731
    print(f"  DeviceEpisodeMonitor.update (four launches)      : {d * 1e3:10.1f} us   runs {rnd(dr)}")
    print(f"  torch: loop over T, torch.where, mask append     : {r * 1e3:10.1f} us   runs {rnd(rr)}")
    print(f"  torch / device (HIP events, host side included): {r / d:.1f}x" + ("" if d <= r else "   ** THE DEVICE ROUTE IS SLOWER **"))
    dw, rw = sorted(wall_ms(device) for _ in range(args.repeats)), sorted(wall_ms(restated) for _ in range(args.repeats))
    print(f"  wall, synchronised: device {dw[len(dw) // 2] * 1e3:.1f} us (min {dw[0] * 1e3:.1f}, max {dw[-1] * 1e3:.1f}), torch {rw[len(rw) // 2] * 1e3:.1f} us "
          f"(min {rw[0] * 1e3:.1f}, max {rw[-1] * 1e3:.1f})")
    for o in (check, mon, actor, venv):
        o.close()


def host_evaluate(venv, actor, n_eval_episodes):
    N = venv.num_envs
    targets = np.array([(n_eval_episodes + i) // N for i in range(N)])
    counts, ep_return, ep_length, returns = np.zeros(N, np.int64), np.zeros(N), np.zeros(N, np.int64), []
    venv.reset()
    while (counts < targets).any():
        actions, _ = venv.actor_actions(actor, deterministic=True)
        b = venv.step_flat(actions)
        reward, step_type = b["reward"].cpu().numpy(), b["step_type"].cpu().numpy()
        dones = (b["terminated"] | b["truncated"]).cpu().numpy().astype(bool)
        counting = (step_type != FIRST) & (counts < targets)
        ep_return[counting] += reward[counting]
        ep_length[counting] += 1
        for i in np.nonzero(dones & counting)[0]:
            returns.append(ep_return[i])
            counts[i] += 1
            ep_return[i] = ep_length[i] = 0
    return float(np.mean(returns)), float(np.std(returns))


def evaluate_case(args):
    N = 4096
    venv = m.HipVectorEnv("point_mass_reach", N, seed=1)
    actor = small_actor(venv)
    got, want = m.evaluate_policy(venv, actor, n_eval_episodes=N), host_evaluate(venv, actor, N)
    print(f"\nevaluate_policy, Pointmass, {N} episodes on {N} envs: device (mean, std) {got}, host loop {want}")
    dev = sorted(wall_ms(lambda: m.evaluate_policy(venv, actor, n_eval_episodes=N)) for _ in range(args.repeats))
    host = sorted(wall_ms(lambda: host_evaluate(venv, actor, N)) for _ in range(args.repeats))
    print(f"  evaluate_policy (blocks of 32 steps, one scalar read per block): {dev[len(dev) // 2]:9.2f} ms wall   (min {dev[0]:.2f}, max {dev[-1]:.2f})")
    print(f"  host loop (one copy per control step, numpy accumulators)      : {host[len(host) // 2]:9.2f} ms wall   (min {host[0]:.2f}, max {host[-1]:.2f})")
    print(f"  host / device: {host[len(host) // 2] / dev[len(dev) // 2]:.1f}x" + ("" if dev[len(dev) // 2] <= host[len(host) // 2] else "   ** THE DEVICE ROUTE IS SLOWER **"))
    actor.close()
    venv.close()


def learn_case(args):
    print(f"\nlearn on Robot-Reach, 4096 envs, [64, 64] networks, batch 256, train_freq=1, gradient_steps=1: {args.learn_blocks} timed blocks of one control step "
          f"(wall clock, synchronised), the two settings alternating")
    runs = {False: [], True: []}
    trainers = {}
    for fed in (False, True):
        venv = m.HipVectorEnv("robot_reach", 4096, seed=1)
        venv.reset(seed=2)
        torch.manual_seed(0)
        actor, critic = networks(venv, [64, 64])
        trainer = m.DeviceSAC(venv, actor, critic, buffer_size=1_000_000, batch_size=256, train_freq=1, gradient_steps=1, learning_starts=4096 * 4)
        mon = m.DeviceEpisodeMonitor(venv) if fed else None
        g = torch.Generator(device=venv.device).manual_seed(3)
        trainer.learn(4096 * 8, generator=g, monitor=mon)  # the warm-up, the one read of the size and the first training phases: untimed
        trainers[fed] = (trainer, mon, g, actor, critic, venv)
    for _ in range(args.repeats):
        for fed in (False, True):
            trainer, mon, g = trainers[fed][:3]
            steps0 = trainer.num_timesteps
            ms = wall_ms(lambda: trainer.learn(4096 * args.learn_blocks, generator=g, monitor=mon))
            runs[fed].append((trainer.num_timesteps - steps0) / (ms * 1e-3))
    for fed, name in ((False, "every new argument at its default"), (True, "monitor fed, no records         ")):
        r = sorted(runs[fed])
        print(f"  {name}: {r[len(r) // 2]:12.0f} env-steps/s   (min {r[0]:.0f}, max {r[-1]:.0f})   runs {[round(x / 1e6, 2) for x in runs[fed]]} M")
    plain, fed = sorted(runs[False])[args.repeats // 2], sorted(runs[True])[args.repeats // 2]
    per_block = (4096 / fed - 4096 / plain) * 1e6
    print(f"  the monitor costs {per_block:.1f} us per block of one control step ({(1 - fed / plain) * 100:.1f} % of the rate): four launches of a [1, 4096] block")
    for trainer, mon, g, actor, critic, venv in trainers.values():
        for o in (trainer, mon, critic, actor, venv):
            if o is not None:
                o.close()


def std_case():
    import _monitor_reference as mref
    from _monitor_reference import BlockMaker, to_dev

    print("\nthe summary's std against an exact recomputation (rational arithmetic), next to numpy.std's own error on the same records; allowed: 4 x "
          "numpy's, a measured 0 counting as the measurement's resolution, one ulp of the exact value (tests/_monitor_reference.py std_bar)")
    for W, blocks in ((100, 1), (100, 4), (700, 6), (1, 2)):
        mon, ref = m.DeviceEpisodeMonitor(65, device="cuda:0", window=W), mref.RefMonitor(65, W)
        maker = BlockMaker(65, "same_step", seed=W + blocks, p_end=0.3)
        for _ in range(blocks):
            blk = maker.block(7)
            mon.update(to_dev(blk), "same_step")
            ref.update(blk, "same_step")
        ret = ref.live()[0]
        (exact, numpy_err, bar), s = mref.std_bar(ret), mon.summary()
        print(f"  K = {len(ret):3d}: std {exact!r} (one ulp {float(np.spacing(exact)):.3e}): numpy's error {numpy_err:.3e}, the kernel's "
              f"{abs(s['return_std'] - exact):.3e}, allowed {bar:.3e}; return sum against numpy's {abs(s['return_sum'] - float(ret.sum())):.3e} "
              f"(bound {len(ret) * 2.0 ** -52 * float(np.abs(ret).sum()):.3e})")
        mon.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--learn-blocks", type=int, default=64)
    args = ap.parse_args()
    print(f"device: {torch.cuda.get_device_name(0)}; medians of {args.repeats} runs; host-side overhead (Python, ctypes, torch's dispatcher and allocator) is inside "
          f"every number")
    update_case("robot_reach", 200, args)
    update_case("point_mass_reach", 51, args)
    evaluate_case(args)
    learn_case(args)
    std_case()


if __name__ == "__main__":
    main()
