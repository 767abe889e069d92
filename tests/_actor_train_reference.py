"""The torch and numpy side of the actor-update tests (test_actor_train_host.py, test_actor_train_device.py): the cases and their seeds,
SB3's actor loss under torch autograd and torch.optim.Adam in a chosen dtype, a float32 evaluation with the kernel's summation shape
(per-16-row-tile gradients added in order, csrc/mjs_actor_train.h), the entropy-coefficient step restated in numpy float32, and SB3's
whole ``SAC.train`` restated for ``sac_gradient_step``."""
import functools
import math

import numpy as np
import torch

import _critic_reference as ref
import _critic_train_reference as tref

ROWS = tref.ROWS
LR, BETAS, EPS = tref.LR, tref.BETAS, tref.EPS
ENT = 0.005  # the reference scripts' fixed ent_coef

# (actor widths, critic widths, actor activation, critic activation, n_critics, B or "multi", D, A, flag)
CASES = [
    ([64, 64], [64, 64], "relu", "relu", 2, 256, 12, 3, ""),
    ([64, 64], [64, 64], "tanh", "tanh", 2, 33, 12, 3, ""),
    ([32], [64], "relu", "tanh", 1, 17, 12, 3, ""),
    ([32], [64], "tanh", "relu", 2, 1, 12, 3, ""),
    ([256, 256], [256, 256], "relu", "relu", 2, 33, 12, 3, ""),
    ([256, 256], [256, 256], "tanh", "relu", 1, 16, 12, 3, ""),
    ([40, 24, 33], [40, 24, 33], "tanh", "tanh", 2, 17, 12, 3, ""),
    ([40, 24, 33], [40, 24, 33], "relu", "relu", 2, 256, 12, 3, ""),
    ([32], [256, 256], "relu", "relu", 2, 33, 12, 3, ""),            # the critic sets the stride
    ([64, 64], [64, 64], "relu", "relu", 2, "multi", 12, 3, ""),     # two tiles per workgroup, more than one split
    ([64, 64], [64, 64], "relu", "tanh", 2, 33, 12, 8, ""),          # the head's 16 columns full; action columns 12..19 straddle a k tile
    ([64, 64], [64, 64], "relu", "relu", 2, 17, 64, 8, ""),          # critic k0 = 80 above the actor's 64
    ([32], [64], "tanh", "relu", 2, 33, 5, 3, ""),                   # k padding
    ([64, 64], [64, 64], "relu", "relu", 2, 33, 12, 3, "clamp"),     # log_std above 2 (component 0) and below -20 (component 1)
]
ADAM_CASES = [1, 6, 2]  # indices into CASES: five steps against torch.optim.Adam
SEED_BUMP = {}          # case index -> added to its seed where the first seed misses a condition of test_actor_train_host.py


def case_id(case):
    aw, cw, aa, ca, n, B, D, A, flag = case
    return f"pi{'x'.join(map(str, aw))}-{aa}-qf{'x'.join(map(str, cw))}-{ca}-{n}c-B{B}-D{D}A{A}" + (f"-{flag}" if flag else "")


def case_seed(case):
    index = CASES.index(case)
    return 300 + 17 * index + SEED_BUMP.get(index, 0)


def actor_slab_floats(widths, D):
    """Floats of one actor slab: every layer's packed weights [K][O] and bias [O], the stacked head, and 4."""
    total, K = 0, ref.round_up(D, ref.KPAD)
    for w in widths:
        O = ref.round_up(w, ref.OPAD)
        total += K * O + O
        K = O
    return total + K * ref.OPAD + ref.OPAD + 4


def splits_max(widths, D):
    return min(tref.MAX_SPLITS, max(1, tref.WORKSPACE_CAP // (actor_slab_floats(widths, D) * 4)))


def split_rule(B, widths, D):
    """(tiles_per_split, splits): crit::split_rule with n_critics = 1 over the actor's slab."""
    tiles = -(-B // ROWS)
    tps = max(1, -(-tiles // splits_max(widths, D)))
    return tps, -(-tiles // tps)


def resolve_B(case):
    return ROWS * splits_max(case[0], case[6]) + 1 if case[5] == "multi" else case[5]


def make_nets(case, device="cpu"):
    """(actor modules (hidden, mu, log_std), q_nets) from the case's seed."""
    aw, cw, _, _, n, _, D, A, flag = case
    seed = case_seed(case)
    actor = ref.make_actor(D, aw, A, seed=seed, device=device)
    if flag == "clamp":
        with torch.no_grad():
            actor[2].bias[0] += 30.0
            actor[2].bias[1] -= 40.0
    return actor, ref.make_q_nets(D, A, cw, n, seed=seed + 1, device=device)


def make_batch(case, n_batches=1):
    """CPU float32 (obs, z) per batch; z = randn.clamp(-2, 2) (test_critic_device.py's reason), and in the clamp case the component whose
    log_std sits at 2 draws 0.05 z, so that tanh does not saturate."""
    g = torch.Generator().manual_seed(case_seed(case) + 5)
    B, D, A = resolve_B(case), case[6], case[7]
    out = []
    for _ in range(n_batches):
        obs, z = torch.randn(B, D, generator=g), torch.randn(B, A, generator=g).clamp(-2.0, 2.0)
        if case[8] == "clamp":
            z[:, 0] *= 0.05
        out.append((obs, z))
    return out


def actor_params(actor, dtype):
    hidden, mu, log_std = actor
    return [(m.weight.detach().to(dtype).clone().requires_grad_(True), m.bias.detach().to(dtype).clone().requires_grad_(True)) for m in (*hidden, mu, log_std)]


def critic_params(q_nets, dtype, grad=False):
    return [[(m.weight.detach().to(dtype).clone().requires_grad_(grad), m.bias.detach().to(dtype).clone().requires_grad_(grad)) for m in net] for net in q_nets]


def sample(params, obs, z, activation):
    """SB3's actor.action_log_prob on the draws z from the parameter list: (a, logp, raw log_std)."""
    f = torch.relu if activation == "relu" else torch.tanh
    h = obs
    for w, b in params[:-2]:
        h = f(torch.nn.functional.linear(h, w, b))
    mu, raw = torch.nn.functional.linear(h, *params[-2]), torch.nn.functional.linear(h, *params[-1])
    ls = raw.clamp(-20.0, 2.0)
    a = torch.tanh(mu + ls.exp() * z)
    gauss = (-0.5 * z * z - ls - 0.5 * math.log(2.0 * math.pi)).sum(dim=1)
    return a, gauss - torch.log(1.0 - a * a + 1e-6).sum(dim=1), raw


def grad_ref(actor, q_nets, batch, alpha, case, dtype):
    """torch autograd of SB3's actor_loss = (alpha * logp - min_c Q_c(obs, a)).mean() in ``dtype``: a dict with grads [(dW, db)] (hidden
    layers, mu, log_std), actions, log_prob, q_pi, min_q_action_grad, loss [1] and raw_log_std."""
    obs, z = (t.to(dtype) for t in batch)
    params, cp = actor_params(actor, dtype), critic_params(q_nets, dtype)
    a, logp, raw = sample(params, obs, z, case[2])
    q = tref._forward(cp, obs, a, case[3])
    min_q = q.min(dim=0).values
    loss = (alpha * logp - min_q).mean()
    dq = torch.autograd.grad(min_q.sum(), a, retain_graph=True)[0]
    loss.backward()
    return {"grads": [(w.grad, b.grad) for w, b in params], "actions": a.detach(), "log_prob": logp.detach(), "q_pi": q.detach(),
            "min_q_action_grad": dq, "loss": loss.detach().reshape(1), "raw_log_std": raw.detach()}


def grad_tiled32(actor, q_nets, batch, alpha, case, tiles_per_split):
    """float32 with the kernel's summation shape: the gradient of every 16-row tile (its rows' share of the loss, scaled by 1 / B), tiles
    added in order inside a split, the splits' slabs added in order. (grads, loss [1])."""
    obs, z = batch
    B = obs.shape[0]
    inv_B = torch.tensor(1.0 / B, dtype=torch.float32)
    cp = critic_params(q_nets, torch.float32)
    slabs, slab = [], None
    for t, row0 in enumerate(range(0, B, ROWS)):
        params = actor_params(actor, torch.float32)
        rows = slice(row0, row0 + ROWS)
        a, logp, _ = sample(params, obs[rows], z[rows], case[2])
        terms = alpha * logp - tref._forward(cp, obs[rows], a, case[3]).min(dim=0).values
        (terms * inv_B).sum().backward()
        part = [[w.grad, b.grad] for w, b in params], terms.detach().sum().reshape(1)
        if t % tiles_per_split == 0:
            slab = part
            slabs.append(slab)
        else:
            for (w, b), (pw, pb) in zip(slab[0], part[0]):
                w += pw
                b += pb
            slab[1].add_(part[1])
    grads, loss = slabs[0]
    for g2, l2 in slabs[1:]:
        for (w, b), (pw, pb) in zip(grads, g2):
            w += pw
            b += pb
        loss = loss + l2
    return [tuple(p) for p in grads], loss * inv_B


def adam_torch(actor, q_nets, batches, alpha, case, dtype, lr=LR):
    """SB3's actor lines with torch.optim.Adam (default betas / eps) in ``dtype``, one step per batch: the parameters [(W, b)]."""
    params, cp = actor_params(actor, dtype), critic_params(q_nets, dtype)
    opt = torch.optim.Adam([t for pair in params for t in pair], lr=lr)
    for batch in batches:
        obs, z = (t.to(dtype) for t in batch)
        a, logp, _ = sample(params, obs, z, case[2])
        loss = (alpha * logp - tref._forward(cp, obs, a, case[3]).min(dim=0).values).mean()
        opt.zero_grad()
        loss.backward()
        opt.step()
    return [(w.detach(), b.detach()) for w, b in params]


def adam_tiled32(actor, q_nets, batches, alpha, case, tiles_per_split, lr=LR):
    """float32 with the kernel's summation shape and the header's Adam: what the device is expected to give, up to the order inside a tile."""
    hidden, mu, log_std = actor
    mods = [torch.nn.Linear(m.in_features, m.out_features) for m in (*hidden, mu, log_std)]
    for m, s in zip(mods, (*hidden, mu, log_std)):
        m.load_state_dict(s.state_dict())
    net = (mods[:-2], mods[-2], mods[-1])
    state = [[np.zeros(tuple(t.shape), np.float32) for t in (m.weight, m.bias) for _ in (0, 1)] for m in mods]
    for t, batch in enumerate(batches, start=1):
        grads, _ = grad_tiled32(net, q_nets, batch, alpha, case, tiles_per_split)
        for m, (gw, gb), s in zip(mods, grads, state):
            for k, (param, g) in enumerate(((m.weight, gw), (m.bias, gb))):
                p, s[2 * k], s[2 * k + 1] = tref.adam_step32(param.detach().numpy().copy(), g.numpy(), s[2 * k], s[2 * k + 1], t, lr)
                with torch.no_grad():
                    param.copy_(torch.from_numpy(p))
    return [(m.weight.detach(), m.bias.detach()) for m in mods]


@functools.lru_cache(maxsize=None)
def grad_references(index):
    """(actor, q_nets, batch, ref64, ref32) of CASES[index] with the fixed ent_coef, computed once on the CPU and shared; nobody writes to them."""
    case = CASES[index]
    actor, q_nets = make_nets(case)
    batch = make_batch(case)[0]
    return actor, q_nets, batch, grad_ref(actor, q_nets, batch, ENT, case, torch.float64), grad_ref(actor, q_nets, batch, ENT, case, torch.float32)


@functools.lru_cache(maxsize=None)
def adam_references(index, steps=5):
    case = CASES[index]
    actor, q_nets = make_nets(case)
    batches = make_batch(case, steps)
    return actor, q_nets, batches, adam_torch(actor, q_nets, batches, ENT, case, torch.float64), adam_torch(actor, q_nets, batches, ENT, case, torch.float32)


PARTS = ("actions", "log_prob", "q_pi", "min_q_action_grad", "loss")


def check_grads(what, grads, ref64, ref32):
    for l, ((gw, gb), (w64, b64), (w32, b32)) in enumerate(zip(grads, ref64["grads"], ref32["grads"])):
        ref.within_bar(f"{what} dW[{l}]", gw.cpu(), w64, w32)
        ref.within_bar(f"{what} db[{l}]", gb.cpu(), b64, b32)


def check_params(what, got, ref64, ref32):
    for l, ((gw, gb), (w64, b64), (w32, b32)) in enumerate(zip(got, ref64, ref32)):
        ref.within_bar(f"{what} W[{l}]", gw.cpu(), w64, w32)
        ref.within_bar(f"{what} b[{l}]", gb.cpu(), b64, b32)


# ---------------------------------------------------------------------------------------------- the entropy coefficient
def entropy_partial32(log_prob, target_entropy, tiles_per_split):
    """The kernel's sum of (logp + target_entropy) over the batch, in numpy float32 and in its stated order: rows in order from 0.0f inside a
    16-row tile, a workgroup's tiles added in tile order, the workgroups' partials added in order."""
    lp, te = np.asarray(log_prob, np.float32), np.float32(target_entropy)
    slabs = []
    for t, row0 in enumerate(range(0, len(lp), ROWS)):
        s = np.float32(0.0)
        for v in lp[row0:row0 + ROWS]:
            s = np.float32(s + np.float32(v + te))
        if t % tiles_per_split == 0:
            slabs.append(s)
        else:
            slabs[-1] = np.float32(slabs[-1] + s)
    total = slabs[0]
    for s in slabs[1:]:
        total = np.float32(total + s)
    return total


def entropy_step32(log_ent_coef, m, v, log_prob, target_entropy, tiles_per_split, t, lr=LR):
    """ent_kernel restated: g = -(partial * (1 / B)), then adam_kernel's lines on the scalar. One-element float32 arrays in and out."""
    inv_B = np.float32(1.0 / len(log_prob))
    mean = np.float32(entropy_partial32(log_prob, target_entropy, tiles_per_split) * inv_B)
    g = np.array([-mean], np.float32)
    return tref.adam_step32(log_ent_coef, g, m, v, t, lr)


# ---------------------------------------------------------------------------------------------- SB3's SAC.train, restated
def sac_train_torch(actor, q_nets, target_nets, batches, draws, case, gamma, tau, dtype, lr=LR, init_ent=1.0):
    """stable_baselines3/sac/sac.py SAC.train with ent_coef = "auto", one gradient step per batch, in ``dtype`` with the given draws
    (z_next, z_pi) per step. ``batches``: dicts of CPU float32 tensors. Returns (actor params, critic params, target params, log_ent_coef)."""
    A = case[7]
    ap, cp, tp = actor_params(actor, dtype), critic_params(q_nets, dtype, grad=True), critic_params(target_nets, dtype)
    log_ent = torch.log(torch.ones(1, dtype=torch.float32) * init_ent).to(dtype).requires_grad_(True)
    a_opt = torch.optim.Adam([t for pair in ap for t in pair], lr=lr)
    c_opt = torch.optim.Adam([t for net in cp for pair in net for t in pair], lr=lr)
    e_opt = torch.optim.Adam([log_ent], lr=lr)
    target_entropy = -float(A)
    for batch, (z_next, z_pi) in zip(batches, draws):
        b = {k: v.to(dtype) for k, v in batch.items()}
        actions_pi, log_prob, _ = sample(ap, b["obs"], z_pi.to(dtype), case[2])
        ent_coef = torch.exp(log_ent.detach())
        ent_loss = -(log_ent * (log_prob + target_entropy).detach()).mean()
        e_opt.zero_grad()
        ent_loss.backward()
        e_opt.step()
        with torch.no_grad():
            next_a, next_logp, _ = sample(ap, b["next_obs"], z_next.to(dtype), case[2])
            next_q = tref._forward(tp, b["next_obs"], next_a, case[3]).min(dim=0).values - ent_coef * next_logp
            target = b["rewards"] + (1.0 - b["dones"]) * gamma * next_q
        critic_loss = 0.5 * sum(torch.nn.functional.mse_loss(qc, target) for qc in tref._forward(cp, b["obs"], b["actions"], case[3]))
        c_opt.zero_grad()
        critic_loss.backward()
        c_opt.step()
        min_q = tref._forward(cp, b["obs"], actions_pi, case[3]).min(dim=0).values
        actor_loss = (ent_coef * log_prob - min_q).mean()
        a_opt.zero_grad()
        actor_loss.backward()
        a_opt.step()
        with torch.no_grad():
            for tn, cn in zip(tp, cp):
                for (tw, tb), (cw, cb) in zip(tn, cn):
                    tw.mul_(1.0 - tau).add_(cw, alpha=tau)
                    tb.mul_(1.0 - tau).add_(cb, alpha=tau)
    return ([(w.detach(), b.detach()) for w, b in ap], [[(w.detach(), b.detach()) for w, b in net] for net in cp],
            [[(w.detach(), b.detach()) for w, b in net] for net in tp], log_ent.detach())
