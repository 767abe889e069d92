#!/usr/bin/env python3
"""The device replay buffer against the torch-ops path a user writes without it, in one process:
  add     ``DeviceReplayBuffer.add_block`` (csrc/mjs_replay.h: count, scan, scatter, image scatter) against boolean-mask indexing of the
          block + ``index_copy_`` into the same storage layout (the mask's count comes back to the host on every block);
  sample  ``DeviceReplayBuffer.sample`` against ``index_select`` per stream, B = 256 and 4096;
for Robot-Reach at 4096 envs x 200 steps (state only) and Pointmass at 4096 x 16 with one 64 x 64 camera. The blocks come from
``actor_rollout`` once; every timing is ``--calls`` calls back to back between two HIP events, the two paths alternating,
``--repeats`` times after an untimed call of each; medians with every run. GB/s are the bytes a path must move (``add_bytes`` /
``sample_bytes`` below) over the time. Both paths are checked to leave the same storage first. The MI355X output is kept in
profiles/replay_timing.txt.

  python tools/replay_bench.py [--envs 4096] [--repeats 5] [--calls 50]"""
import argparse
import sys
from pathlib import Path

import torch

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))
import mujoco_sim_amd as m  # noqa: E402

SCENE = "Camera/rgb_image"
STREAMS = ("obs", "next_obs", "actions", "rewards", "dones", "timeouts")


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


class TorchRing:
    """The same storage filled with torch ops: what a user of actor_rollout writes today. The write position lives on the host."""

    def __init__(self, buf):
        self.capacity, self.cols, self.count = buf.capacity, torch.tensor(buf.obs_index, device=buf.device), 0
        for name in STREAMS:
            setattr(self, name, torch.zeros_like(getattr(buf, name)))
        self.rgb, self.next_rgb = {k: torch.zeros_like(v) for k, v in buf.rgb.items()}, {k: torch.zeros_like(v) for k, v in buf.next_rgb.items()}

    def add_block(self, obs0, blk, final=None):
        T, N = blk["obs"].shape[:2]
        valid = (blk["step_type"] != 0).reshape(-1)
        flat = lambda t: t.reshape(T * N, *t.shape[2:])  # noqa: E731
        prev = torch.cat([obs0[None], blk["obs"][:-1]])
        obs = flat(prev)[valid][:, self.cols].float()  # the boolean mask: its count is read back by the host here
        k = obs.shape[0]
        idx = (self.count + torch.arange(k, device=obs.device)) % self.capacity
        self.obs.index_copy_(0, idx, obs)
        self.next_obs.index_copy_(0, idx, flat(blk["obs"])[valid][:, self.cols].float())
        self.actions.index_copy_(0, idx, flat(blk["squashed_actions"])[valid])
        self.rewards.index_copy_(0, idx, flat(blk["reward"])[valid].float())
        self.dones.index_copy_(0, idx, flat(blk["terminated"])[valid].float())
        self.timeouts.index_copy_(0, idx, flat(blk["truncated"])[valid])
        for key in self.rgb:
            self.rgb[key].index_copy_(0, idx, flat(blk[key])[valid])
            self.next_rgb[key].index_copy_(0, idx, flat(torch.cat([blk[key][1:], final[key][None]]))[valid])
        self.count += k

    def sample(self, draws):
        idx = draws % min(self.count, self.capacity)
        out = {name: getattr(self, name).index_select(0, idx) for name in STREAMS}
        out["indices"] = idx
        out["rgb"] = {k: v.index_select(0, idx) for k, v in self.rgb.items()}
        out["next_rgb"] = {k: v.index_select(0, idx) for k, v in self.next_rgb.items()}
        return out


def add_bytes(buf, rows, valid):
    """Bytes an add must move: the mask byte of every row; per transition the float64 columns of obs and next_obs, the action, the
    reward and two flags read, the float32 row written; per camera two frames read and two written."""
    D, A, frame = buf.obs_dim, buf.action_dim, buf.height * buf.width * 3
    return rows + valid * (2 * D * 8 + A * 4 + 8 + 2 + 2 * D * 4 + A * 4 + 4 + 4 + 1 + len(buf.cameras) * 4 * frame)


def sample_bytes(buf, B):
    """Bytes a sample must move: the draw read and the index written, every stream's row read and written."""
    D, A, frame = buf.obs_dim, buf.action_dim, buf.height * buf.width * 3
    return B * (16 + 2 * (2 * D * 4 + A * 4 + 4 + 4 + 1 + len(buf.cameras) * 2 * frame))


def same_storage(buf, ring):
    return all(torch.equal(getattr(buf, n), getattr(ring, n)) for n in STREAMS) and all(
        torch.equal(buf.rgb[k], ring.rgb[k]) and torch.equal(buf.next_rgb[k], ring.next_rgb[k]) for k in buf.cameras)


def line(name, ms, runs, calls, nbytes):
    us = ms * 1e3 / calls
    print(f"    {name:44s}: {us:10.2f} us per call  {nbytes / us / 1e3:9.2f} GB/s   runs {[round(x * 1e3 / calls, 2) for x in runs]}")
    return us


def case(title, venv, T, capacity, cameras, args):
    dev, N = venv.device, venv.num_envs
    torch.manual_seed(0)
    width = sum(n for _, _, n in venv.flat_observation_layout)
    hidden = [torch.nn.Linear(width, 64), torch.nn.Linear(64, 64)]
    net = [m_.to(dev) for m_ in (*hidden, torch.nn.Linear(64, venv.action_dim), torch.nn.Linear(64, venv.action_dim))]
    actor = m.DeviceActor.from_linears(venv, net[:2], net[2], net[3])
    buf = m.DeviceReplayBuffer(venv, capacity, cameras=cameras, image_size=venv.image_resolution if cameras else None)
    ring = TorchRing(buf)
    venv.reset(seed=1)
    obs0 = venv.flat_obs.clone()
    blk = venv.actor_rollout(actor, T, render=bool(cameras), generator=torch.Generator(device=dev).manual_seed(2))
    final = {k: venv.render(buf.height, buf.width) for k in cameras}
    rows, valid = T * N, int((blk["step_type"] != 0).sum())
    for _ in range(2):  # the second block wraps around the ring's end
        buf.add_block(obs0, blk, final)
        ring.add_block(obs0, blk, final)
    same = same_storage(buf, ring) and buf.count == ring.count
    frame = f", one {buf.height} x {buf.width} camera" if cameras else ", state only"
    print(f"\n{title}: {N} envs x {T} steps = {rows} rows, {valid} transitions{frame}; D = {buf.obs_dim}, A = {buf.action_dim}, capacity {capacity}; "
          f"both paths leave the same storage: {same}")
    if not same:
        raise SystemExit("the two paths disagree")
    calls = args.calls
    nbytes = add_bytes(buf, rows, valid)
    (k_ms, t_ms), (k_runs, t_runs) = alternate(([lambda: [buf.add_block(obs0, blk, final) for _ in range(calls)],
                                                 lambda: [ring.add_block(obs0, blk, final) for _ in range(calls)]]), args.repeats)
    print(f"  add ({nbytes / 1e6:.1f} MB to move per block)")
    k_us = line("add_block (count, scan, scatter kernels)", k_ms, k_runs, calls, nbytes)
    t_us = line("torch ops (boolean mask + index_copy_)", t_ms, t_runs, calls, nbytes)
    print(f"    torch ops / kernels: {t_us / k_us:.2f}x" + ("" if k_us <= t_us else "   ** THE KERNELS ARE SLOWER **"))
    for B in (256, 4096):
        draws = torch.randint(0, 2**62, (B,), dtype=torch.int64, device=dev, generator=torch.Generator(device=dev).manual_seed(B))
        a, b = buf.sample(B, draws=draws), ring.sample(draws)
        assert all(torch.equal(a[n], b[n]) for n in (*STREAMS, "indices")) and all(torch.equal(a["rgb"][k], b["rgb"][k]) for k in cameras)
        nbytes = sample_bytes(buf, B)
        (k_ms, t_ms), (k_runs, t_runs) = alternate(([lambda: [buf.sample(B, draws=draws) for _ in range(calls)],
                                                     lambda: [ring.sample(draws) for _ in range(calls)]]), args.repeats)
        print(f"  sample B = {B} ({nbytes / 1e6:.3f} MB to move per batch; both paths allocate their outputs)")
        k_us = line("sample (gather kernels)", k_ms, k_runs, calls, nbytes)
        t_us = line("torch ops (index_select per stream)", t_ms, t_runs, calls, nbytes)
        print(f"    torch ops / kernels: {t_us / k_us:.2f}x" + ("" if k_us <= t_us else "   ** THE KERNELS ARE SLOWER **"))
    buf.close()
    actor.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=4096)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--calls", type=int, default=50)
    args = ap.parse_args()
    N = args.envs
    print(f"device: {torch.cuda.get_device_name(0)}; median of {args.repeats} alternating runs, each {args.calls} calls back to back between two HIP events")
    venv = m.HipVectorEnv("robot_reach", N, seed=1)
    case("Robot-Reach", venv, 200, 300 * N, (), args)
    venv.close()
    venv = m.HipVectorEnv("point_mass_reach", N, seed=1, image_resolution=64, time_limit=1.0)  # episodes of 10 steps: the block holds FIRST rows
    case("Pointmass", venv, 16, 24 * N, (SCENE,), args)
    venv.close()


if __name__ == "__main__":
    main()
