"""The torch and numpy side of the critic-update tests (test_critic_train_host.py, test_critic_train_device.py): the split rule and the
slab size restated, the cases, torch autograd and torch.optim.Adam in a chosen dtype, a float32 evaluation with the kernel's summation
shape (per-16-row-tile gradients added in order), and Adam restated operation by operation as csrc/mjs_critic_train.h states it."""
import functools
import math

import numpy as np
import torch

import _critic_reference as ref

D, A = 12, 3
ROWS, MAX_SPLITS, WORKSPACE_CAP = 16, 128, 128 << 20  # csrc/mjs_critic_train.h
LR, BETAS, EPS = 3e-4, (0.9, 0.999), 1e-8             # SB3's Adam


def slab_floats(widths, obs_dim=D, action_dim=A):
    """Floats of one (split, critic) slab: every layer's packed weights [K][O] and bias [O], the loss partial, padded to 4."""
    total, K = 0, ref.round_up(obs_dim + action_dim, ref.KPAD)
    for w in widths:
        O = ref.round_up(w, ref.OPAD)
        total += K * O + O
        K = O
    return total + K * ref.OPAD + ref.OPAD + 4


def splits_max(widths, n_critics):
    return min(MAX_SPLITS, max(1, WORKSPACE_CAP // (n_critics * slab_floats(widths) * 4)))


def split_rule(B, widths, n_critics):
    """(tiles_per_split, splits) of a batch of B rows: a function of B and the shape alone."""
    tiles = -(-B // ROWS)
    tps = max(1, -(-tiles // splits_max(widths, n_critics)))
    return tps, -(-tiles // tps)


def multi_B(widths, n_critics):
    """The smallest B at which a workgroup owns more than one tile; it then also has more than one split (asserted by the tests)."""
    return ROWS * splits_max(widths, n_critics) + 1


# (widths, activation, n_critics, B or "multi"): every width list, both activations, one and two critics, every B of the issue
CASES = [
    ([64, 64], "relu", 2, 256), ([64, 64], "tanh", 2, 33), ([64, 64], "relu", 1, 1),
    ([32], "relu", 1, 17), ([32], "tanh", 2, 16), ([32], "tanh", 1, 256),
    ([256, 256], "relu", 2, 256), ([256, 256], "tanh", 1, 33), ([256, 256], "relu", 2, 17),
    ([40, 24, 33], "tanh", 2, 17), ([40, 24, 33], "relu", 2, 256), ([40, 24, 33], "relu", 1, 1), ([40, 24, 33], "tanh", 1, 16),
    ([64, 64], "relu", 2, "multi"), ([40, 24, 33], "tanh", 2, "multi"), ([256, 256], "relu", 2, "multi"),
]
ADAM_CASES = [([64, 64], "relu", 2, 256), ([40, 24, 33], "tanh", 2, 33), ([32], "tanh", 1, 17)]


def case_id(case):
    widths, activation, n_critics, B = case
    return f"{'x'.join(map(str, widths))}-{activation}-{n_critics}c-B{B}"


def case_seed(case):
    listed = CASES + ADAM_CASES
    if case in listed:
        return 100 + 13 * listed.index(case)
    return 5000 + sum(case[0]) + 31 * case[2] + (0 if case[3] == "multi" else case[3])


def resolve_B(case):
    widths, _, n_critics, B = case
    return multi_B(widths, n_critics) if B == "multi" else B


def make_batch(case, n_batches=1):
    """CPU float32 (obs, actions, target) per batch, from the case's seed."""
    g = torch.Generator().manual_seed(case_seed(case))
    B = resolve_B(case)
    return [(torch.randn(B, D, generator=g), torch.tanh(torch.randn(B, A, generator=g)), torch.randn(B, generator=g)) for _ in range(n_batches)]


def make_nets(case, device="cpu"):
    widths, _, n_critics, _ = case
    return ref.make_q_nets(D, A, widths, n_critics, seed=case_seed(case), device=device)


def _params(q_nets, dtype):
    return [[(m.weight.detach().to(dtype).clone().requires_grad_(True), m.bias.detach().to(dtype).clone().requires_grad_(True)) for m in net] for net in q_nets]


def _forward(params, obs, actions, activation):
    f = torch.relu if activation == "relu" else torch.tanh
    out = []
    for net in params:
        h = torch.cat([obs, actions], dim=1)
        for w, b in net[:-1]:
            h = f(torch.nn.functional.linear(h, w, b))
        out.append(torch.nn.functional.linear(h, *net[-1])[:, 0])
    return torch.stack(out)


def grad_ref(q_nets, batch, activation, dtype):
    """torch autograd of SB3's critic_loss = 0.5 * sum_c mse_loss(q_c, y) in ``dtype``: (grads[c][l] = (dW, db), loss [n_critics], q)."""
    obs, actions, target = (t.to(dtype) for t in batch)
    params = _params(q_nets, dtype)
    q = _forward(params, obs, actions, activation)
    losses = torch.stack([torch.nn.functional.mse_loss(qc, target) for qc in q])
    (0.5 * losses.sum()).backward()
    return [[(w.grad, b.grad) for w, b in net] for net in params], losses.detach(), q.detach()


def grad_tiled32(q_nets, batch, activation, tiles_per_split):
    """float32 with the kernel's summation shape: the gradient of every 16-row tile (its rows' share of the loss, scaled by 1 / B),
    tiles added in order inside a split, the splits' slabs added in order. (grads, loss)."""
    obs, actions, target = batch
    B = obs.shape[0]
    inv_B = torch.tensor(1.0 / B, dtype=torch.float32)
    slabs, slab = [], None
    for t, row0 in enumerate(range(0, B, ROWS)):
        params = _params(q_nets, torch.float32)
        rows = slice(row0, row0 + ROWS)
        diff = _forward(params, obs[rows], actions[rows], activation) - target[rows]
        (0.5 * (diff * diff * inv_B).sum()).backward()
        part = [[(w.grad, b.grad) for w, b in net] for net in params], (diff.detach() ** 2).sum(dim=1)
        if t % tiles_per_split == 0:
            slab = part
            slabs.append(slab)
        else:
            for net, pnet in zip(slab[0], part[0]):
                for (w, b), (pw, pb) in zip(net, pnet):
                    w += pw
                    b += pb
            slab[1].add_(part[1])
    grads, loss = slabs[0]
    for g2, l2 in slabs[1:]:
        for net, pnet in zip(grads, g2):
            for (w, b), (pw, pb) in zip(net, pnet):
                w += pw
                b += pb
        loss = loss + l2
    return grads, loss * inv_B


def adam_coefficients(t, lr=LR, betas=BETAS, eps=EPS):
    """What the host computes in double from the step count t and rounds to float32 once each (csrc/mjsim.hip mjs_critic_update)."""
    f = np.float32
    return {"one_minus_beta1": f(1.0 - betas[0]), "beta2": f(betas[1]), "one_minus_beta2": f(1.0 - betas[1]),
            "sqrt_bc2": f(math.sqrt(1.0 - betas[1] ** float(t))), "eps": f(eps), "step_size": f(lr / (1.0 - betas[0] ** float(t)))}


def adam_step32(p, g, m, v, t, lr=LR, betas=BETAS, eps=EPS):
    """adam_kernel's float32 operation order on numpy float32 arrays, one rounding per line; returns (p, m, v)."""
    k = adam_coefficients(t, lr, betas, eps)
    assert all(a.dtype == np.float32 for a in (p, g, m, v))
    gm = g - m
    m1 = k["one_minus_beta1"] * gm
    m = m + m1
    g2 = g * g
    v1 = k["beta2"] * v
    v2 = k["one_minus_beta2"] * g2
    v = v1 + v2
    sq = np.sqrt(v)
    d0 = sq / k["sqrt_bc2"]
    den = d0 + k["eps"]
    r = m / den
    u = k["step_size"] * r
    p = p - u
    assert all(a.dtype == np.float32 for a in (p, m, v))
    return p, m, v


def adam_torch(q_nets, batches, activation, dtype, lr=LR):
    """SB3's lines with torch.optim.Adam (default betas / eps) in ``dtype``, one step per batch: the parameters [c][l] = (W, b)."""
    params = _params(q_nets, dtype)
    flat = [t for net in params for pair in net for t in pair]
    opt = torch.optim.Adam(flat, lr=lr)
    for batch in batches:
        obs, actions, target = (t.to(dtype) for t in batch)
        loss = 0.5 * sum(torch.nn.functional.mse_loss(qc, target) for qc in _forward(params, obs, actions, activation))
        opt.zero_grad()
        loss.backward()
        opt.step()
    return [[(w.detach(), b.detach()) for w, b in net] for net in params]


def adam_tiled32(q_nets, batches, activation, tiles_per_split, lr=LR):
    """float32 with the kernel's summation shape and the header's Adam: what the device is expected to give, up to the order inside a tile."""
    nets = [[torch.nn.Linear(m.in_features, m.out_features) for m in net] for net in q_nets]
    for net, src in zip(nets, q_nets):
        for m, s in zip(net, src):
            m.load_state_dict(s.state_dict())
    state = [[[np.zeros(tuple(t.shape), np.float32) for t in (m.weight, m.bias) for _ in (0, 1)] for m in net] for net in nets]
    for t, batch in enumerate(batches, start=1):
        grads, _ = grad_tiled32(nets, batch, activation, tiles_per_split)
        for net, gnet, snet in zip(nets, grads, state):
            for m, (gw, gb), s in zip(net, gnet, snet):
                for k, (param, g) in enumerate(((m.weight, gw), (m.bias, gb))):
                    p, s[2 * k], s[2 * k + 1] = adam_step32(param.detach().numpy().copy(), g.numpy(), s[2 * k], s[2 * k + 1], t, lr)
                    with torch.no_grad():
                        param.copy_(torch.from_numpy(p))
    return [[(m.weight.detach(), m.bias.detach()) for m in net] for net in nets]


@functools.lru_cache(maxsize=None)
def grad_references(index):
    """(nets, batch, ref64, ref32) of CASES[index], computed once on the CPU and shared; nobody writes to them."""
    case = CASES[index]
    nets, batch = make_nets(case), make_batch(case)[0]
    return nets, batch, grad_ref(nets, batch, case[1], torch.float64), grad_ref(nets, batch, case[1], torch.float32)


@functools.lru_cache(maxsize=None)
def adam_references(index, steps=5):
    case = ADAM_CASES[index]
    nets, batches = make_nets(case), make_batch(case, steps)
    return nets, batches, adam_torch(nets, batches, case[1], torch.float64), adam_torch(nets, batches, case[1], torch.float32)


def check_grads(what, got, ref64, ref32):
    """within_bar per parameter tensor and for the loss; ``got`` / ``ref`` = (grads, loss[, q])."""
    for c, (gnet, net64, net32) in enumerate(zip(got[0], ref64[0], ref32[0])):
        for l, ((gw, gb), (w64, b64), (w32, b32)) in enumerate(zip(gnet, net64, net32)):
            ref.within_bar(f"{what} dW[{c}][{l}]", gw.cpu(), w64, w32)
            ref.within_bar(f"{what} db[{c}][{l}]", gb.cpu(), b64, b32)
    ref.within_bar(f"{what} loss", got[1].cpu(), ref64[1], ref32[1])


def check_params(what, got, ref64, ref32):
    for c, (gnet, net64, net32) in enumerate(zip(got, ref64, ref32)):
        for l, ((gw, gb), (w64, b64), (w32, b32)) in enumerate(zip(gnet, net64, net32)):
            ref.within_bar(f"{what} W[{c}][{l}]", gw.cpu(), w64, w32)
            ref.within_bar(f"{what} b[{c}][{l}]", gb.cpu(), b64, b32)
