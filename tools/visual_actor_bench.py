#!/usr/bin/env python3
"""Closed-loop rollout under a visual policy (SB3's MultiInputPolicy: NatureCNN on the scene camera + state columns -> SAC's MLP
actor), two ways, in one process (Robot-Reach, 64x64 frames):
  (a) the host loop: ``render`` -> the torch modules in float32 (uint8 NHWC -> float NCHW / 255, three Conv2d, Linear, the MLP,
      sample, tanh, unscale) -> ``HipVectorEnv.step_flat``, once per control step from Python;
  (b) ``HipVectorEnv.actor_rollout`` with a visual ``DeviceActor``: render, encoder (csrc/mjs_encoder.h), actor and step kernels per
      control step, enqueued by one native call;
and the encoder's two launches alone (HIP events around a batch of calls) against their arithmetic floor: 6.83 MFLOP per env at 64x64
with 256 features (conv1 2.76, conv2 2.36, conv3 1.18, fc 0.52), at the 157 TFLOP/s peak of the f32-input MFMA. (a) and (b) alternate,
repeat by repeat, on the same handle settings and seed; medians are printed with every run next to them. If torch's GPU convolution
cannot run (MIOpen without kernels for this device), the tool says so and times the device loop alone. The MI355X output is kept in
profiles/visual_actor_timing.txt.

  python tools/visual_actor_bench.py [--envs 4096] [--steps 50] [--repeats 5] [--size 64]"""
import argparse
import sys
from pathlib import Path

import torch

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))
import mujoco_sim_amd as m  # noqa: E402
from mujoco_sim_amd import _native as nat  # noqa: E402

sys.path.insert(0, str(ROOT / "tools"))
from actor_collect_bench import TorchActor, alternate  # noqa: E402

SCENE = "Camera/rgb_image"
PEAK_F32_MFMA = 157e12


class NatureCNN(torch.nn.Module):
    """stable_baselines3.common.torch_layers.NatureCNN, features_dim 256."""

    def __init__(self, size, features_dim=256):
        super().__init__()
        nn = torch.nn
        self.cnn = nn.Sequential(nn.Conv2d(3, 32, 8, 4), nn.ReLU(), nn.Conv2d(32, 64, 4, 2), nn.ReLU(), nn.Conv2d(64, 64, 3, 1), nn.ReLU(), nn.Flatten())
        with torch.no_grad():
            n_flatten = self.cnn(torch.zeros(1, 3, size, size)).shape[1]
        self.linear = nn.Sequential(nn.Linear(n_flatten, features_dim), nn.ReLU())

    @torch.no_grad()
    def forward(self, rgb):  # uint8 NHWC, as the ray caster writes it
        return self.linear(self.cnn(rgb.permute(0, 3, 1, 2).float() / 255.0))


def encoder_flop(size, F):
    s1 = (size - 8) // 4 + 1
    s2 = (s1 - 4) // 2 + 1
    s3 = s2 - 2
    return 2 * (s1 * s1 * 32 * 192 + s2 * s2 * 64 * 512 + s3 * s3 * 64 * 576 + 64 * s3 * s3 * F)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=4096)
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--size", type=int, default=64)
    args = ap.parse_args()
    N, T, R = args.envs, args.steps, args.size
    venv = m.HipVectorEnv("robot_reach", N, seed=1)
    dev = venv.device
    low = torch.tensor(venv.action_low, dtype=torch.float64, device=dev)
    span = torch.tensor(venv.action_high, dtype=torch.float64, device=dev) - low
    keep = ("obs", "reward", "is_success", "step_type")
    torch.manual_seed(0)
    cnn = NatureCNN(R).to(dev)
    F = cnn.linear[0].out_features
    net = TorchActor(venv.obs_dim + F, [64, 64], venv.action_dim).to(dev)
    enc = m.DeviceEncoder.from_sb3(venv, cnn, R, R)
    actor = m.DeviceActor.from_sb3(venv, net, encoders={SCENE: enc})  # state columns, then the scene camera's features
    z = torch.randn(T, N, venv.action_dim, dtype=torch.float32, device=dev)
    print(f"device: {torch.cuda.get_device_name(0)}; Robot-Reach, {N} envs x {T} control steps, {R}x{R} scene camera -> NatureCNN ({F} features) + 12 state "
          f"columns -> [64, 64] actor; median of {args.repeats} alternating runs (each: seeded reset + {T} steps), HIP events")
    frame = torch.empty(N, R, R, 3, dtype=torch.uint8, device=dev)

    def host_loop():
        venv.reset(seed=1)
        for t in range(T):
            x = torch.cat([venv.flat_obs.float(), cnn(venv.render(R, R, out=frame))], dim=1)
            venv.step_flat(low + 0.5 * (net(x, z[t]).double() + 1.0) * span)

    def device_loop():
        venv.reset(seed=1)
        return venv.actor_rollout(actor, T, z=z, keep=keep)

    torch_conv = True
    try:
        venv.reset(seed=1)
        cnn(venv.render(R, R, out=frame))
        torch.cuda.synchronize()
    except RuntimeError as e:  # MIOpen without a kernel for this device / shape
        torch_conv = False
        print(f"torch's GPU convolution cannot run here ({str(e).splitlines()[0][:160]}): the device loop is timed alone")
    us = lambda ms: ms * 1e3 / T  # noqa: E731
    fns = (host_loop, device_loop) if torch_conv else (device_loop,)
    med, runs = alternate(fns, args.repeats)
    b_ms, b_all = med[-1], runs[-1]
    if torch_conv:
        print(f"(a) host loop   render + torch CNN + MLP + step_flat : {med[0]:9.3f} ms  {us(med[0]):8.2f} us/control step  {N * T / med[0] / 1e3:8.3f} M env-steps/s   runs {[round(x, 2) for x in runs[0]]}")
    print(f"(b) device loop actor_rollout (visual actor)         : {b_ms:9.3f} ms  {us(b_ms):8.2f} us/control step  {N * T / b_ms / 1e3:8.3f} M env-steps/s   runs {[round(x, 2) for x in b_all]}")
    if torch_conv:
        print(f"ratio (b) / (a): {med[0] / b_ms:.2f}x" + ("" if b_ms <= med[0] else "   ** (b) IS SLOWER **"))
    # the pieces alone: `reps` calls back to back between two events
    venv.reset(seed=1)
    venv.render(R, R, out=frame)
    reps = 20
    L, stream = nat.lib(), venv._stream()
    ws, feats = enc.workspace(N), torch.empty(N, F, dtype=torch.float32, device=dev)
    fns = [lambda: [L.mjs_encoder_features(enc._e, frame.data_ptr(), N, ws.data_ptr(), feats.data_ptr(), stream) for _ in range(reps)],
           lambda: [venv.render(R, R, out=frame) for _ in range(reps)]]
    names = ["encoder launches (conv + fc kernels)", "render launch"]
    if torch_conv:
        fns.append(lambda: [cnn(frame) for _ in range(reps)])
        names.append("torch NatureCNN forward (permute, float, / 255, MIOpen)")
    med, runs = alternate(fns, args.repeats)
    for name, ms, r in zip(names, med, runs):
        print(f"    {name:56s}: {ms * 1e3 / reps:9.2f} us per call   runs {[round(x * 1e3 / reps, 2) for x in r]}")
    flop = encoder_flop(R, F) * N
    floor_us = flop / PEAK_F32_MFMA * 1e6
    enc_us = med[0] * 1e3 / reps
    print(f"encoder arithmetic: {encoder_flop(R, F) / 1e6:.2f} MFLOP per env x {N} = {flop / 1e9:.1f} GFLOP; floor at 157 TFLOP/s {floor_us:.0f} us; "
          f"measured {enc_us:.0f} us = {enc_us / floor_us:.1f}x the floor ({flop / enc_us / 1e6:.1f} TFLOP/s)")
    actor.close()
    enc.close()
    venv.close()


if __name__ == "__main__":
    main()
