"""The torch and numpy side of the critic tests (test_critic_host.py, test_critic_device.py): plain ``nn.Linear`` modules with the
default init from a fixed seed, SB3's formulas evaluated in a chosen dtype, the project's bar, and the packed-lerp layout restated."""
import math

import numpy as np
import torch

ULP = 2.0 ** -24
KPAD, OPAD = 16, 32  # granularity of the packed copy in k and in the output index (csrc/mjs_actor.h)


def make_actor(D, widths, A, seed, device="cpu"):
    """(hidden, mu, log_std): default Linear init from torch.manual_seed(seed)."""
    torch.manual_seed(seed)
    hidden, d = [], D
    for w in widths:
        hidden.append(torch.nn.Linear(d, w))
        d = w
    mu, log_std = torch.nn.Linear(d, A), torch.nn.Linear(d, A)
    for m in (*hidden, mu, log_std):
        m.to(device=device, dtype=torch.float32)
    return hidden, mu, log_std


def make_q_nets(D, A, widths, n_critics, seed, device="cpu"):
    """n_critics lists (hidden..., out), every critic from a seed of its own."""
    nets = []
    for c in range(n_critics):
        torch.manual_seed(seed + 7919 * c)
        net, d = [], D + A
        for w in widths:
            net.append(torch.nn.Linear(d, w))
            d = w
        net.append(torch.nn.Linear(d, 1))
        nets.append([m.to(device=device, dtype=torch.float32) for m in net])
    return nets


def _lin(m, h, dtype):
    return torch.nn.functional.linear(h, m.weight.detach().to(dtype), m.bias.detach().to(dtype))


def q_ref(q_nets, obs, actions, activation, dtype):
    """[n_critics, B]: the modules' parameters cast to ``dtype``."""
    f = torch.relu if activation == "relu" else torch.tanh
    out = []
    for net in q_nets:
        h = torch.cat([obs.to(dtype), actions.to(dtype)], dim=1)
        for m in net[:-1]:
            h = f(_lin(m, h, dtype))
        out.append(_lin(net[-1], h, dtype)[:, 0])
    return torch.stack(out)


def action_log_prob_ref(actor_net, x, z, activation, dtype):
    """SB3's actor.action_log_prob on the draws z: (a', logp) with SquashedDiagGaussianDistribution.log_prob, epsilon = 1e-6."""
    hidden, mu, log_std = actor_net
    f = torch.relu if activation == "relu" else torch.tanh
    h = x.to(dtype)
    for m in hidden:
        h = f(_lin(m, h, dtype))
    z = z.to(dtype)
    ls = _lin(log_std, h, dtype).clamp(-20.0, 2.0)
    a = torch.tanh(_lin(mu, h, dtype) + ls.exp() * z)
    gauss = (-0.5 * z * z - ls - 0.5 * math.log(2.0 * math.pi)).sum(dim=1)
    return a, gauss - torch.log(1.0 - a * a + 1e-6).sum(dim=1)


def td_ref(actor_net, q_nets, batch, z, gamma, ent_coef, actor_activation, critic_activation, dtype):
    """The whole block in ``dtype``: next_actions, next_log_prob, q_next, target."""
    a, logp = action_log_prob_ref(actor_net, batch["next_obs"], z, actor_activation, dtype)
    q = q_ref(q_nets, batch["next_obs"], a, critic_activation, dtype)
    r, d = batch["rewards"].to(dtype), batch["dones"].to(dtype)
    target = r + (1.0 - d) * gamma * (q.min(dim=0).values - ent_coef * logp)
    return {"next_actions": a, "next_log_prob": logp, "q_next": q, "target": target}


def within_bar(what, got, ref64, ref32):
    """The project's bar: e32 = max |torch float32 - torch float64|; max |kernel - float64| <= max(4 e32, 8 * 2^-24 * max(1, max |ref64|))."""
    e32 = (ref32.double() - ref64).abs().max().item()
    err = (got.double() - ref64).abs().max().item()
    bar = max(4 * e32, 8 * ULP * max(1.0, ref64.abs().max().item()))
    print(f"{what}: kernel vs float64 {err:.3e}, torch float32 vs float64 {e32:.3e}, bar {bar:.3e}, ratio to e32 {err / max(e32, 1e-300):.2f}")
    assert got.dtype == torch.float32 and got.shape == ref64.shape, (what, got.dtype, got.shape)
    assert err <= bar, (what, err, e32, bar)


def round_up(x, m):
    return (x + m - 1) // m * m


def pack_lerp_np(dst_w, dst_b, weight, bias, K, O, tau):
    """mjs_critic_load for one layer, restated: ``weight`` [out, in], ``bias`` [out] (nn.Linear layout) into the packed copy dst_w [K, O]
    (K-major: row k holds input k's weights, the output index contiguous), dst_b [O]. tau == 1 copies and never reads dst (None is
    fine); otherwise real elements become fmaf(tau32, src, (1 - tau)32 * dst) in float32 (here: the product rounded, the sum in float64
    rounded once, which is the fmaf's result up to double rounding) and the padding is written 0."""
    out, fan_in = weight.shape
    assert K % KPAD == 0 and O % OPAD == 0 and K >= fan_in and O >= out
    w, b = np.zeros((K, O), np.float32), np.zeros(O, np.float32)
    if tau == 1.0:
        w[:fan_in, :out], b[:out] = weight.T, bias
        return w, b
    t, omt = np.float32(tau), np.float32(1.0 - tau)
    blend = lambda d, s: (np.float64(t) * s.astype(np.float64) + (omt * d).astype(np.float64)).astype(np.float32)  # noqa: E731
    w[:fan_in, :out] = blend(dst_w[:fan_in, :out], weight.T.astype(np.float32))
    b[:out] = blend(dst_b[:out], bias.astype(np.float32))
    return w, b
