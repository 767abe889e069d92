"""The torch and numpy side of the encoder-training tests (test_encoder_train_host.py, test_encoder_train_device.py): the split and
workspace rule of include/mjsim.h restated, the cases, the NatureCNN restated with CONSTANT masks (each layer ``conv(x) * mask``,
differentiated by autograd) in a chosen dtype, the plain forward's pre-activations, the mask condition, a float32 evaluation with the
kernel's summation shape (one gradient per split's images, the slabs added in order), and the small regression loop.

Why masks. A unit whose pre-activation is within rounding of 0 can be on in one float32 evaluation and off in another, and its gradient
contribution is not small; with about 1e5 units per case no seed avoids all of them. So gradients are compared under ONE set of masks
(the kernel's own on the device, torch float32's on the CPU), and the masks themselves are held to the plain float64 forward: they may
differ only in units with |pre64| <= 64 e_layer, e_layer = max |pre32 - pre64| of that layer, and in at most 0.1 % of a layer's units."""
import copy
import functools

import numpy as np
import torch

import _critic_reference as ref
from _visual_nets import conv_out, final_size, make_cnn

F32 = torch.float32
MAX_SPLITS, SLAB_CAP, FPAD = 64, 128 << 20, 32   # csrc/mjs_encoder_train.h, csrc/mjs_encoder.h
MASK_BAND, MASK_SHARE = 64.0, 1e-3
LAYERS = ("conv1", "conv2", "conv3", "fc")
STRIDES = (4, 2, 1)

SHAPES = [(36, 36, 256), (36, 52, 40), (44, 44, 33), (64, 64, 256)]  # conv3 output 1x1, 1x3, 2x2, 4x4; F no multiple of 32; H != W
CASES = [(H, W, F, n) for H, W, F in SHAPES for n in (1, 17, 33)] + [(44, 44, 33, "multi")]


def geometry(H, W):
    """((H1, W1), (H2, W2), (H3, W3))"""
    out = []
    for k, s in ((8, 4), (4, 2), (3, 1)):
        H, W = conv_out(H, k, s), conv_out(W, k, s)
        out.append((H, W))
    return out


def slab_floats(H, W, F):
    """Floats of one split's slab: the packed weights [K][O] and bias [O] of conv1..3 and fc (F padded to 32), and 4."""
    h3, w3 = final_size(H, W)
    Fp = ref.round_up(F, FPAD)
    return 192 * 32 + 32 + 512 * 64 + 64 + 576 * 64 + 64 + 64 * h3 * w3 * Fp + Fp + 4


def splits_max(H, W, F):
    return min(MAX_SPLITS, max(1, SLAB_CAP // (4 * slab_floats(H, W, F))))


def split_rule(n, H, W, F):
    """(images_per_split, splits) of n images: a function of n and the shape alone."""
    ips = max(1, -(-n // splits_max(H, W, F)))
    return ips, -(-n // ips)


def workspace_bytes(n, H, W, F):
    (h1, w1), (h2, w2), (h3, w3) = geometry(H, W)
    nf, Fp = 64 * h3 * w3, ref.round_up(F, FPAD)
    return 4 * (2 * n * h1 * w1 * 32 + 2 * n * h2 * w2 * 64 + 2 * n * nf + ref.round_up(n * F, 4) + n * Fp + split_rule(n, H, W, F)[1] * slab_floats(H, W, F))


def multi_n(H, W, F):
    """The smallest n at which a split owns more than one image; it then also has more than one split (asserted by the tests)."""
    return splits_max(H, W, F) + 1


def resolve_n(case):
    H, W, F, n = case
    return multi_n(H, W, F) if n == "multi" else n


def case_id(case):
    return "{}x{}-F{}-n{}".format(*case)


def case_seed(case):
    return 300 + 17 * CASES.index(case)


def random_images(n, H, W, seed):
    g = torch.Generator(device="cpu").manual_seed(seed)
    return torch.randint(0, 256, (n, H, W, 3), dtype=torch.uint8, generator=g)


def synthetic_renders(n, H, W, seed):
    """What stands in for venv.render where there is no device: flat regions, a shaded floor and a bright box per image, like a frame
    of the ray caster (large areas of equal bytes, a few edges)."""
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:H, 0:W]
    out = np.zeros((n, H, W, 3), np.uint8)
    for i in range(n):
        horizon = rng.integers(H // 4, H // 2)
        img = np.where((yy < horizon)[..., None], np.array([135, 170, 200]), (60 + 120 * (yy - horizon) / max(1, H - horizon))[..., None] * np.array([1.0, 0.9, 0.8]))
        y0, x0, s = rng.integers(0, H - 8), rng.integers(0, W - 8), rng.integers(4, 9)
        img = np.where(((yy >= y0) & (yy < y0 + s) & (xx >= x0) & (xx < x0 + s))[..., None], rng.integers(0, 256, 3), img)
        out[i] = img.astype(np.uint8)
    return torch.from_numpy(out)


def make_dfeatures(case):
    g = torch.Generator(device="cpu").manual_seed(case_seed(case) + 1)
    return torch.randn(resolve_n(case), case[2], generator=g)


def case_cnn(case, device="cpu"):
    return make_cnn(case[0], case[1], case[2], seed=case_seed(case), device=device)


def host_images(case):
    """Half synthetic renders and half random bytes (the CPU tests; the device tests render the first half)."""
    H, W, _, _ = case
    n = resolve_n(case)
    return torch.cat([synthetic_renders(n - n // 2, H, W, case_seed(case)), random_images(n // 2, H, W, case_seed(case) + 2)])


def params_of(cnn, dtype):
    """[(W, b)] of conv1, conv2, conv3, fc as fresh leaves in ``dtype``."""
    mods = [cnn.cnn[0], cnn.cnn[2], cnn.cnn[4], cnn.linear[0]]
    return [(m.weight.detach().cpu().to(dtype).clone().requires_grad_(True), m.bias.detach().cpu().to(dtype).clone().requires_grad_(True)) for m in mods]


def to_input(images, dtype):
    """uint8 NHWC -> NCHW float32 / 255 (a float32 division, SB3's preprocess_obs), then ``dtype``."""
    return (images.detach().cpu().permute(0, 3, 1, 2).float() / 255.0).to(dtype)


def plain_forward(cnn, images, dtype):
    """The pre-activations [conv1, conv2, conv3 (NCHW), fc] of the ordinary ReLU forward in ``dtype``."""
    params = params_of(cnn, dtype)
    h, pre = to_input(images, dtype), []
    with torch.no_grad():
        for (w, b), s in zip(params[:3], STRIDES):
            pre.append(torch.nn.functional.conv2d(h, w, b, stride=s))
            h = torch.relu(pre[-1])
        pre.append(torch.nn.functional.linear(h.flatten(1), *params[3]))
    return pre


def masks_of_pre(pre):
    return [p > 0 for p in pre]


def masks_of_activations(activations, features, H, W):
    """The kernel's masks in NCHW: conv1 [n, P1, 32] and conv2 [n, P2, 64] are position-major, flat is CHW."""
    (h1, w1), (h2, w2), (h3, w3) = geometry(H, W)
    n = features.shape[0]
    a1 = activations["conv1"].cpu().reshape(n, h1, w1, 32).permute(0, 3, 1, 2)
    a2 = activations["conv2"].cpu().reshape(n, h2, w2, 64).permute(0, 3, 1, 2)
    a3 = activations["flat"].cpu().reshape(n, 64, h3, w3)
    return [a1 > 0, a2 > 0, a3 > 0, features.cpu() > 0]


def masked_backward(cnn, images, dfeatures, masks, dtype):
    """The network with constant masks, differentiated by autograd in ``dtype``: ([(dW, db)] x 4, features)."""
    params = params_of(cnn, dtype)
    h = to_input(images, dtype)
    for (w, b), s, m in zip(params[:3], STRIDES, masks[:3]):
        h = torch.nn.functional.conv2d(h, w, b, stride=s) * m.to(dtype)
    f = torch.nn.functional.linear(h.flatten(1), *params[3]) * masks[3].to(dtype)
    f.backward(dfeatures.cpu().to(dtype))
    return [(w.grad, b.grad) for w, b in params], f.detach()


def masked_backward_slabs32(cnn, images, dfeatures, masks, images_per_split):
    """float32 with the kernel's summation shape: one gradient per split's images, the slabs added in order."""
    total = None
    for i0 in range(0, images.shape[0], images_per_split):
        sl = slice(i0, i0 + images_per_split)
        part, _ = masked_backward(cnn, images[sl], dfeatures[sl], [m[sl] for m in masks], F32)
        if total is None:
            total = [(w.clone(), b.clone()) for w, b in part]
        else:
            for (w, b), (pw, pb) in zip(total, part):
                w += pw
                b += pb
    return total


def check_masks(what, masks, pre64, pre32):
    """The condition on a set of masks against the plain float64 forward; prints and asserts per layer."""
    for name, m, p64, p32 in zip(LAYERS, masks, pre64, pre32):
        e_layer = (p32.double() - p64).abs().max().item()
        differ = m != (p64 > 0)
        count, worst = int(differ.sum()), (p64.abs()[differ].max().item() if differ.any() else 0.0)
        print(f"{what} {name}: {count} of {m.numel()} units differ from float64's mask, largest |pre64| among them {worst:.3e}, e_layer {e_layer:.3e}")
        assert tuple(m.shape) == tuple(p64.shape), (what, name, m.shape, p64.shape)
        assert worst <= MASK_BAND * e_layer, (what, name, worst, e_layer)
        assert count <= MASK_SHARE * m.numel(), (what, name, count, m.numel())


def check_grads(what, got, ref64, ref32):
    for name, (gw, gb), (w64, b64), (w32, b32) in zip(LAYERS, got, ref64, ref32):
        ref.within_bar(f"{what} dW {name}", gw.cpu(), w64, w32)
        ref.within_bar(f"{what} db {name}", gb.cpu(), b64, b32)


@functools.lru_cache(maxsize=None)
def forward_references(index, images_key=None):
    """(cnn, pre64, pre32) of CASES[index] on host_images, computed once and shared; nobody writes to them."""
    case = CASES[index]
    cnn, images = case_cnn(case), host_images(case)
    return cnn, images, plain_forward(cnn, images, torch.float64), plain_forward(cnn, images, F32)


# ---------------------------------------------------------------------------------------------- the small regression
REG = dict(H=36, W=36, F=32, n=16, steps=30, lr=3e-3, seed=4242)


def regression_setup():
    """(cnn, head, images, targets) on the CPU from REG's seed."""
    cnn = make_cnn(REG["H"], REG["W"], REG["F"], seed=REG["seed"])
    torch.manual_seed(REG["seed"] + 1)
    head = torch.nn.Linear(REG["F"], 3)
    n = REG["n"]
    images = torch.cat([synthetic_renders(n // 2, REG["H"], REG["W"], REG["seed"]), random_images(n - n // 2, REG["H"], REG["W"], REG["seed"] + 2)])
    targets = torch.randn(n, 3, generator=torch.Generator().manual_seed(REG["seed"] + 3))
    return cnn, head, images, targets


def regression_torch(dtype):
    """The loop in torch on the CPU in ``dtype``: Adam (SB3's defaults, REG's lr) on the CNN and on the head; the losses before each step."""
    cnn, head, images, targets = regression_setup()
    cnn, head = copy.deepcopy(cnn).to(dtype), copy.deepcopy(head).to(dtype)
    x, y = to_input(images, dtype), targets.to(dtype)
    opts = [torch.optim.Adam(cnn.parameters(), lr=REG["lr"]), torch.optim.Adam(head.parameters(), lr=REG["lr"])]
    losses = []
    for _ in range(REG["steps"]):
        loss = torch.nn.functional.mse_loss(head(cnn(x)), y)
        for o in opts:
            o.zero_grad()
        loss.backward()
        for o in opts:
            o.step()
        losses.append(loss.item())
    return np.array(losses)


@functools.lru_cache(maxsize=None)
def regression_references():
    """(losses64, d32): the float64 curve and the largest relative difference of the float32 curve from it."""
    l64, l32 = regression_torch(torch.float64), regression_torch(F32)
    return l64, float(np.max(np.abs(l32 - l64) / np.abs(l64)))
