#!/usr/bin/env python3
"""One encoder update on the device (``DeviceEncoderOptimizer.step``: forward that keeps the activations, backward, Adam;
csrc/mjs_encoder_train.h) against the same update in torch on the same device: permute + float + ``/255``, the NatureCNN's forward,
``features.backward(dfeatures)`` and ``torch.optim.Adam.step``.

64x64 images, F = 256, n = 32 and 256 (the reference's batch sizes). ``--steps`` updates between two HIP events, host side included
in both, the two routes alternating, ``--repeats`` times after an untimed run of each; medians with every run, and the run-to-run
spread (max - min) of each route. No ratio is set beforehand: a slower device route is marked. Achieved TFLOP/s are the update's
arithmetic (3 x the forward's multiply-adds: forward, data gradient, weight gradient; no data gradient for conv1) over the
device route's time per update - an end-to-end rate, not a kernel's. The MI355X output is kept in profiles/encoder_train_timing.txt.

  python tools/encoder_train_bench.py [--repeats 7] [--steps 50]"""
import argparse
import statistics
import sys
from pathlib import Path

import torch

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))
import mujoco_sim_amd as m  # noqa: E402

H = W = 64
F = 256


class NatureCNN(torch.nn.Module):
    def __init__(self, flat):
        super().__init__()
        nn = torch.nn
        self.cnn = nn.Sequential(nn.Conv2d(3, 32, 8, 4), nn.ReLU(), nn.Conv2d(32, 64, 4, 2), nn.ReLU(), nn.Conv2d(64, 64, 3, 1), nn.ReLU(), nn.Flatten())
        self.linear = nn.Sequential(nn.Linear(flat, F), nn.ReLU())

    def forward(self, x):
        return self.linear(self.cnn(x))


def update_flops(n):
    """Floating-point operations of one update of n images: (forward, backward), 2 per multiply-add."""
    out = lambda v, k, s: (v - k) // s + 1  # noqa: E731
    p1 = out(H, 8, 4) * out(W, 8, 4)
    h2, w2 = out(out(H, 8, 4), 4, 2), out(out(W, 8, 4), 4, 2)
    p2, p3 = h2 * w2, out(h2, 3, 1) * out(w2, 3, 1)
    layers = [p1 * 192 * 32, p2 * 512 * 64, p3 * 576 * 64, 64 * p3 * F]  # multiply-adds per image
    forward = 2 * sum(layers)
    return n * forward, n * (2 * forward - 2 * layers[0])


def timed(fn, steps):
    start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    for _ in range(steps):
        fn()
    end.record()
    end.synchronize()
    return start.elapsed_time(end) * 1e3 / steps  # microseconds per update


def case(venv, n, args):
    dev = venv.device
    torch.manual_seed(0)
    cnn = NatureCNN(64 * 4 * 4).to(dev)
    torch.manual_seed(0)
    ref = NatureCNN(64 * 4 * 4).to(dev)
    enc = m.DeviceEncoder.from_sb3(venv, cnn, H, W)
    opt = m.DeviceEncoderOptimizer(enc)
    adam = torch.optim.Adam(ref.parameters(), lr=3e-4)
    g = torch.Generator(device="cpu").manual_seed(n)
    images = torch.randint(0, 256, (n, H, W, 3), dtype=torch.uint8, generator=g).to(dev)
    dfeat = (torch.randn(n, F, generator=g) / n).to(dev)

    def device_route():
        opt.step(images, dfeat)

    def torch_route():
        x = images.permute(0, 3, 1, 2).float() / 255.0
        adam.zero_grad()
        ref(x).backward(dfeat)
        adam.step()

    for fn in (device_route, torch_route):  # untimed: code objects, MIOpen's algorithm search, the workspace
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    runs = {"device": [], "torch": []}
    for _ in range(args.repeats):
        runs["device"].append(timed(device_route, args.steps))
        runs["torch"].append(timed(torch_route, args.steps))
    med = {k: statistics.median(v) for k, v in runs.items()}
    spread = {k: max(v) - min(v) for k, v in runs.items()}
    fwd, bwd = update_flops(n)
    print(f"n = {n}: {args.steps} updates per run, microseconds per update")
    for k in ("device", "torch"):
        print(f"  {k:6s} median {med[k]:9.1f}  spread {spread[k]:8.1f}  runs " + " ".join(f"{v:.1f}" for v in runs[k]))
    slower = med["device"] > med["torch"] + spread["device"] + spread["torch"]
    print(f"  torch / device = {med['torch'] / med['device']:.2f}" + ("   DEVICE ROUTE SLOWER than torch by more than the spread" if slower else ""))
    print(f"  arithmetic per update: forward {fwd / 1e9:.3f} GFLOP, backward {bwd / 1e9:.3f} GFLOP; device route end to end "
          f"{(fwd + bwd) / med['device'] / 1e6:.2f} TFLOP/s")
    print("  launches per update: forward 2, backward 6 (fc_bwd, dgrad, 4 x wgrad), Adam 1")
    opt.close()
    enc.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--steps", type=int, default=50)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("encoder_train_bench.py measures on the GPU; none is visible")
    venv = m.HipVectorEnv("robot_reach", 4, seed=0)
    venv.reset()
    print(f"{torch.cuda.get_device_name(0)}; {H}x{W} images, F = {F}; torch {torch.__version__}")
    for n in (32, 256):
        case(venv, n, args)
    venv.close()


if __name__ == "__main__":
    main()
