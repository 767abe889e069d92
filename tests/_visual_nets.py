"""Torch stand-ins and CPU reference forwards shared by test_encoder_device.py and test_visual_actor.py (SB3 is not installed where the
tests run): modules with the attributes of SB3's NatureCNN, CombinedExtractor and SAC actor that the package reads, default torch.nn
init from a fixed torch.manual_seed. Every reference forward runs on the CPU (no test depends on MIOpen)."""
import copy

import torch

ULP = 2.0 ** -24
SCENE, WRIST = "Camera/rgb_image", "ur5e/Camera/rgb_image"


def conv_out(n, k, s):
    return (n - k) // s + 1


def final_size(H, W):
    for k, s in ((8, 4), (4, 2), (3, 1)):
        H, W = conv_out(H, k, s), conv_out(W, k, s)
    return H, W


class NatureCNNStandIn(torch.nn.Module):
    """stable_baselines3.common.torch_layers.NatureCNN's attributes: .cnn (Conv2d / ReLU / Flatten), .linear (Linear, ReLU)."""

    def __init__(self, H, W, F):
        super().__init__()
        nn = torch.nn
        self.cnn = nn.Sequential(nn.Conv2d(3, 32, kernel_size=8, stride=4, padding=0), nn.ReLU(), nn.Conv2d(32, 64, kernel_size=4, stride=2, padding=0), nn.ReLU(),
                                 nn.Conv2d(64, 64, kernel_size=3, stride=1, padding=0), nn.ReLU(), nn.Flatten())
        h3, w3 = final_size(H, W)
        self.linear = nn.Sequential(nn.Linear(64 * h3 * w3, F), nn.ReLU())

    def forward(self, x):
        return self.linear(self.cnn(x))


def make_cnn(H, W, F, seed, device="cpu"):
    torch.manual_seed(seed)
    return NatureCNNStandIn(H, W, F).to(device)


def cnn_forward(cnn, images, dtype):
    """The module's forward on the CPU in ``dtype``: uint8 NHWC -> NCHW float32 / 255 (a float32 division, SB3's preprocess_obs)."""
    x = images.detach().cpu().permute(0, 3, 1, 2).float() / 255.0
    with torch.no_grad():
        return copy.deepcopy(cnn).cpu().to(dtype)(x.to(dtype))


def encoder_bar(ref64, ref32):
    """(e32, bar) of the encoder tests: 4 x the float32 reference's own distance from the float64 one, floored at 8 half-ulps of the
    largest feature (features are not bounded by 1)."""
    e32 = (ref32.double() - ref64).abs().max().item()
    return e32, max(4 * e32, 8 * ULP * max(1.0, ref64.abs().max().item()))


class SacActorStandIn(torch.nn.Module):
    """stable_baselines3.sac.policies.Actor's attributes: latent_pi, mu, log_std (+ features_extractor for MultiInputPolicy)."""

    def __init__(self, in_dim, net_arch, A, activation_fn=torch.nn.ReLU, features_extractor=None):
        super().__init__()
        layers, d = [], in_dim
        for w in net_arch:
            layers += [torch.nn.Linear(d, w), activation_fn()]
            d = w
        self.latent_pi = torch.nn.Sequential(*layers)
        self.mu = torch.nn.Linear(d, A)
        self.log_std = torch.nn.Linear(d, A)
        if features_extractor is not None:
            self.features_extractor = features_extractor


class CombinedExtractorStandIn(torch.nn.Module):
    """stable_baselines3.common.torch_layers.CombinedExtractor's attribute: .extractors, a ModuleDict of NatureCNN / Flatten."""

    def __init__(self, extractors):
        super().__init__()
        self.extractors = torch.nn.ModuleDict(extractors)


def make_mlp(in_dim, widths, A, seed, device="cpu"):
    """(hidden, mu, log_std): default Linear init from torch.manual_seed(seed)."""
    torch.manual_seed(seed)
    hidden, d = [], in_dim
    for w in widths:
        hidden.append(torch.nn.Linear(d, w))
        d = w
    mu, log_std = torch.nn.Linear(d, A), torch.nn.Linear(d, A)
    for m in (*hidden, mu, log_std):
        m.to(device)
    return hidden, mu, log_std


def mlp_forward(net, x, z, dtype):
    """SAC's ReLU actor on the CPU in ``dtype``: the squashed action."""
    hidden, mu, log_std = net
    lin = lambda m, h: torch.nn.functional.linear(h, m.weight.detach().cpu().to(dtype), m.bias.detach().cpu().to(dtype))  # noqa: E731
    h = x.cpu().to(dtype)
    for m in hidden:
        h = torch.relu(lin(m, h))
    u, ls = lin(mu, h), lin(log_std, h).clamp(-20.0, 2.0)
    if z is not None:
        u = u + ls.exp() * z.cpu().to(dtype)
    return torch.tanh(u)
