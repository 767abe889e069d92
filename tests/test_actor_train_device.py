"""The actor and entropy-coefficient update on the device (csrc/mjs_actor_train.h, DeviceActorOptimizer, DeviceEntropyCoef,
sac_gradient_step) against torch autograd and torch.optim.Adam.

Bars: the project's (tests/_critic_reference.py within_bar), per parameter tensor and per part; the seeds are the ones
test_actor_train_host.py checks on the CPU (argmin margin, distance from the clamp's edges, a float32 evaluation of the kernel's summation
shape). Compositions are bit for bit: the sample against sac_td_target, q_pi against q_values, two runs against each other, Adam and the
entropy step against their float32 restatements on the kernel's own parts, the master copy against a fresh actor, sac_gradient_step against
its four calls.
"""
import ctypes as C
import types

import numpy as np
import pytest
import torch

import _actor_train_reference as aref
import _critic_reference as ref
import _critic_train_reference as tref

gpu = pytest.mark.gpu
DEV = "cuda:0"
CASE_IDS = [aref.case_id(c) for c in aref.CASES]


def shape_env(D, A):
    """What DeviceActor reads of an env: the device, the action width and the observation row. The update needs no handle."""
    return types.SimpleNamespace(device=DEV, action_dim=A, obs_dim=D, _dev_index=0, flat_observation_layout=[("obs", 0, D)])


def on_device(case, nets_cpu=None):
    """(DeviceActor, DeviceCritic, actor modules, q_nets) over device copies of the case's CPU modules."""
    from mujoco_sim_amd import DeviceActor, DeviceCritic

    actor_net, q_nets = aref.make_nets(case, device=DEV)
    if nets_cpu is not None:
        for m, s in zip((*actor_net[0], *actor_net[1:], *[m for net in q_nets for m in net]), (*nets_cpu[0][0], *nets_cpu[0][1:], *[m for net in nets_cpu[1] for m in net])):
            assert torch.equal(m.weight.cpu(), s.weight) and torch.equal(m.bias.cpu(), s.bias)  # the same seed, the same parameters
    D, A = case[6], case[7]
    actor = DeviceActor.from_linears(shape_env(D, A), *actor_net, activation=case[2], obs_index=list(range(D)))
    critic = DeviceCritic.from_linears(DEV, D, A, q_nets, activation=case[3])
    return actor, critic, actor_net, q_nets


def to_dev(batch):
    obs, z = (t.to(DEV) for t in batch)
    return {"obs": obs}, z


def exported(actor, case):
    """The packed parameters as fresh modules' tensors [(W, b)]; the actor's own modules stay as they are."""
    hidden, mu, log_std = aref.make_nets(case, device=DEV)[0]
    actor.export((hidden, mu, log_std))
    return [(m.weight.detach().clone(), m.bias.detach().clone()) for m in (*hidden, mu, log_std)]


def flat(pairs):
    return [t for pair in pairs for t in pair]


def close(*objects):
    for o in objects:
        o.close()


# ------------------------------------------------------------------------- 1. + 2. gradients and compositions
@gpu
@pytest.mark.parametrize("index", range(len(aref.CASES)), ids=CASE_IDS)
def test_gradients_match_autograd(index):
    from mujoco_sim_amd import DeviceActorOptimizer, _native as nat, sac_td_target

    case = aref.CASES[index]
    B, D, A = aref.resolve_B(case), case[6], case[7]
    tps, splits = aref.split_rule(B, case[0], D)
    if case[5] == "multi":
        assert B == 16 * aref.splits_max(case[0], D) + 1 == 2049 and tps == 2 and splits > 1
    actor_cpu, q_cpu, batch_cpu, ref64, ref32 = aref.grad_references(index)
    actor, critic, _, _ = on_device(case, (actor_cpu, q_cpu))
    assert nat.lib().mjs_actor_train_workspace_bytes(actor._a, B) == splits * aref.actor_slab_floats(case[0], D) * 4
    opt = DeviceActorOptimizer(actor)
    batch, z = to_dev(batch_cpu)
    got = opt.gradients(batch, critic, aref.ENT, z)
    assert opt.step_count == 0
    # 1. against autograd: every dW / db and every part
    assert [(tuple(w.shape), tuple(b.shape)) for w, b in got["grads"]] == [(tuple(m.weight.shape), tuple(m.bias.shape)) for m in (*actor_cpu[0], *actor_cpu[1:])]
    aref.check_grads(aref.case_id(case), got["grads"], ref64, ref32)
    for name in aref.PARTS:
        ref.within_bar(f"{aref.case_id(case)} {name}", got[name].cpu(), ref64[name], ref32[name])
    if case[8] == "clamp":  # no gradient through a clamped log_std: exactly 0
        assert not bool(got["grads"][-1][0][:2].any()) and not bool(got["grads"][-1][1][:2].any()) and bool(got["grads"][-1][1][2:].any())
    # the same bits again
    again = opt.gradients(batch, critic, aref.ENT, z)
    assert all(torch.equal(a, b) for a, b in zip(flat(got["grads"]), flat(again["grads"]))) and all(torch.equal(got[k], again[k]) for k in aref.PARTS)
    # ... and with the coefficient read from device memory
    dev = opt.gradients(batch, critic, torch.tensor([aref.ENT], dtype=torch.float32, device=DEV), z)
    assert all(torch.equal(a, b) for a, b in zip(flat(got["grads"]), flat(dev["grads"]))) and torch.equal(got["loss"], dev["loss"])
    # 2. composition, bit for bit
    td = {"next_obs": batch["obs"], "rewards": torch.zeros(B, device=DEV), "dones": torch.zeros(B, device=DEV)}
    parts = sac_td_target(td, actor, critic, 0.99, aref.ENT, z=z, return_parts=True)
    assert torch.equal(got["actions"], parts["next_actions"]) and torch.equal(got["log_prob"], parts["next_log_prob"])
    assert torch.equal(got["q_pi"], critic.q_values(batch["obs"], got["actions"]))
    close(opt, critic, actor)


# ------------------------------------------------------------------------- 3. Adam, operation by operation
@gpu
@pytest.mark.parametrize("index", [1, 7, 12], ids=[CASE_IDS[i] for i in (1, 7, 12)])
def test_adam_matches_its_float32_restatement(index):
    """Three steps with a learning rate that changes per step, on the kernel's OWN gradients: the exported parameters equal the header's
    operation order restated in numpy float32, bit for bit."""
    from mujoco_sim_amd import DeviceActorOptimizer

    case = aref.CASES[index]
    actor, critic, _, _ = on_device(case)
    opt = DeviceActorOptimizer(actor)
    want = [t.cpu().numpy() for t in flat(exported(actor, case))]
    m = [np.zeros_like(p) for p in want]
    v = [np.zeros_like(p) for p in want]
    for t, (b, lr) in enumerate(zip(aref.make_batch(case, 3), (None, 1e-3, 3e-4)), start=1):
        batch, z = to_dev(b)
        before = opt.gradients(batch, critic, aref.ENT, z)
        parts = opt.step(batch, critic, aref.ENT, z=z, lr=lr, return_parts=True)
        assert opt.step_count == t and all(torch.equal(parts[k], before[k]) for k in aref.PARTS)  # the parts are the values BEFORE the step
        for k, g in enumerate(g.cpu().numpy() for g in flat(before["grads"])):
            want[k], m[k], v[k] = tref.adam_step32(want[k], g, m[k], v[k], t, lr=aref.LR if lr is None else lr)
        got = [p.cpu().numpy() for p in flat(exported(actor, case))]
        for k, (a, b_) in enumerate(zip(got, want)):
            assert np.array_equal(a, b_), (t, k, np.abs(a - b_).max())
    close(opt, critic, actor)


# ------------------------------------------------------------------------- 4. against torch.optim.Adam
@gpu
@pytest.mark.parametrize("index", aref.ADAM_CASES, ids=[CASE_IDS[i] for i in aref.ADAM_CASES])
def test_five_steps_match_torch_adam(index):
    from mujoco_sim_amd import DeviceActorOptimizer

    case = aref.CASES[index]
    actor_cpu, q_cpu, batches, ref64, ref32 = aref.adam_references(index)
    actor, critic, _, _ = on_device(case, (actor_cpu, q_cpu))
    opt = DeviceActorOptimizer(actor)
    for b in batches:
        batch, z = to_dev(b)
        opt.step(batch, critic, aref.ENT, z=z)
    assert opt.step_count == 5
    aref.check_params(aref.case_id(case), exported(actor, case), ref64, ref32)
    close(opt, critic, actor)


# ------------------------------------------------------------------------- 5. the entropy coefficient
def ulps(a, b):
    return abs(int(np.float32(a).view(np.int32)) - int(np.float32(b).view(np.int32)))


@gpu
@pytest.mark.parametrize("index", [1, 9], ids=[CASE_IDS[i] for i in (1, 9)])
def test_entropy_coefficient_step(index):
    from mujoco_sim_amd import DeviceActorOptimizer, DeviceEntropyCoef

    case = aref.CASES[index]
    B, A = aref.resolve_B(case), case[7]
    tps, _ = aref.split_rule(B, case[0], case[6])
    actor, critic, _, _ = on_device(case)
    fixed_actor, fixed_critic, _, _ = on_device(case)
    opt, fixed_opt = DeviceActorOptimizer(actor), DeviceActorOptimizer(fixed_actor)
    coef = DeviceEntropyCoef(DEV, A, init=0.2, lr=1e-2)
    assert coef.target_entropy == -float(A)
    p, m, v = coef.log_ent_coef.cpu().numpy().copy(), np.zeros(1, np.float32), np.zeros(1, np.float32)
    # torch, float64 / float32: SB3's lines for the actor and the coefficient, the same draws
    tor = {}
    for dtype in (torch.float64, torch.float32):
        ap = aref.actor_params(aref.make_nets(case)[0], dtype)
        log_ent = torch.log(torch.ones(1) * 0.2).to(dtype).requires_grad_(True)
        tor[dtype] = (ap, aref.critic_params(aref.make_nets(case)[1], dtype), log_ent, torch.optim.Adam(flat(ap), lr=aref.LR), torch.optim.Adam([log_ent], lr=1e-2), [])
    for t, b in enumerate(aref.make_batch(case, 3), start=1):
        batch, z = to_dev(b)
        alpha = float(coef.ent_coef.cpu())  # the value BEFORE this step (a read-back of the test's, not of the library's)
        old_grads = flat(opt.gradients(batch, critic, coef, z)["grads"])
        fixed_grads = flat(fixed_opt.gradients(batch, fixed_critic, alpha, z)["grads"])
        assert all(torch.equal(a, b_) for a, b_ in zip(old_grads, fixed_grads))  # the gradient uses the old coefficient
        parts = opt.step(batch, critic, coef, z=z, return_parts=True)
        fixed_opt.step(batch, fixed_critic, alpha, z=z)
        assert coef.step_count == t == opt.step_count
        assert all(torch.equal(a, b_) for a, b_ in zip(flat(exported(actor, case)), flat(exported(fixed_actor, case))))  # ... and so does the step
        # the float32 restatement on the kernel's own log_prob, bit for bit; expf within 2 ulp
        p, m, v = aref.entropy_step32(p, m, v, parts["log_prob"].cpu().numpy(), coef.target_entropy, tps, t, lr=1e-2)
        got_log, got_ent = coef.log_ent_coef.cpu().numpy(), coef.ent_coef.cpu().numpy()
        assert np.array_equal(got_log, p), (t, got_log, p)
        assert ulps(got_ent[0], np.exp(p.astype(np.float32))[0]) <= 2, (t, got_ent, np.exp(p))
        for dtype, (ap, cp, log_ent, a_opt, e_opt, trace) in tor.items():
            obs, zz = (x.to(dtype) for x in b)
            a, logp, _ = aref.sample(ap, obs, zz, case[2])
            ent = torch.exp(log_ent.detach())
            e_opt.zero_grad()
            (-(log_ent * (logp + coef.target_entropy).detach()).mean()).backward()
            e_opt.step()
            a_opt.zero_grad()
            (ent * logp - tref._forward(cp, obs, a, case[3]).min(dim=0).values).mean().backward()
            a_opt.step()
            trace.append(log_ent.detach().clone())
        ref.within_bar(f"log_ent_coef after step {t}", coef.log_ent_coef.cpu(), tor[torch.float64][5][-1], tor[torch.float32][5][-1])
    aref.check_params("actor with a learned coefficient", exported(actor, case), [(w.detach(), b_.detach()) for w, b_ in tor[torch.float64][0]],
                      [(w.detach(), b_.detach()) for w, b_ in tor[torch.float32][0]])
    close(opt, fixed_opt, critic, fixed_critic, actor, fixed_actor)


# ------------------------------------------------------------------------- 6. the packed copy is the master copy
@gpu
def test_stepped_actor_drives_the_env_and_keeps_its_padding_zero():
    """[40, 24, 33] with tanh: every layer has padded columns, the first layer padded rows next to the action columns of the critics' input
    image, and tanh'(0) = 1 would carry a non-zero padding forward. After steps, actor_actions equals that of a fresh actor made from the
    exported modules (its padding is written 0 by the pack kernels) bit for bit, and differs from before."""
    import mujoco_sim_amd as m

    venv = m.HipVectorEnv("point_mass_reach", 16, seed=7)
    obs = venv.reset(seed=3)
    D, A = int(venv.obs_dim), int(venv.action_dim)
    widths = [40, 24, 33]
    net = ref.make_actor(D, widths, A, seed=61, device=DEV)
    q_nets = ref.make_q_nets(D, A, widths, 2, seed=62, device=DEV)
    actor = m.DeviceActor.from_linears(venv, *net, activation="tanh")
    critic = m.DeviceCritic.from_linears(DEV, D, A, q_nets, activation="tanh")
    opt = m.DeviceActorOptimizer(actor, lr=1e-2)
    g = torch.Generator(device=DEV).manual_seed(5)
    z_act = torch.randn(16, A, dtype=torch.float32, device=DEV, generator=g)
    acts = lambda a: torch.cat([t.double() for t in venv.actor_actions(a, z=z_act)], dim=1).clone()  # noqa: E731  (env actions | squashed)
    before = acts(actor)
    for _ in range(4):
        batch = {"obs": torch.randn(33, D, dtype=torch.float32, device=DEV, generator=g)}
        opt.step(batch, critic, 0.2, generator=g)
    after = acts(actor)
    assert actor.export() == (actor.hidden, actor.mu, actor.log_std)  # into the modules the object was made from
    fresh = m.DeviceActor.from_linears(venv, *net, activation="tanh")
    assert torch.equal(acts(fresh), after) and not torch.equal(before, after)
    del obs
    close(opt, fresh, critic, actor)
    venv.close()


# ------------------------------------------------------------------------- 7. zero gradients
@gpu
@pytest.mark.parametrize("index", [0, 6], ids=[CASE_IDS[i] for i in (0, 6)])
def test_no_entropy_term_and_a_critic_blind_to_the_action_move_nothing(index):
    from mujoco_sim_amd import DeviceActorOptimizer, DeviceCritic

    case = aref.CASES[index]
    D, A = case[6], case[7]
    actor, critic, _, q_nets = on_device(case)
    critic.close()
    with torch.no_grad():
        for net in q_nets:
            net[0].weight[:, D:] = 0.0  # the first layer's action rows
    critic = DeviceCritic.from_linears(DEV, D, A, q_nets, activation=case[3])
    opt = DeviceActorOptimizer(actor)
    batch, z = to_dev(aref.make_batch(case)[0])
    got = opt.gradients(batch, critic, 0.0, z)
    assert all(not bool(t.any()) for t in flat(got["grads"])) and not bool(got["min_q_action_grad"].any())
    before = exported(actor, case)
    opt.step(batch, critic, 0.0, z=z)
    assert opt.step_count == 1 and all(torch.equal(a, b) for a, b in zip(flat(before), flat(exported(actor, case))))
    close(opt, critic, actor)


# ------------------------------------------------------------------------- 8. the whole gradient step
def full_batches(case, n):
    g = torch.Generator().manual_seed(977)
    B, D, A = 33, case[6], case[7]
    batches = [{"obs": torch.randn(B, D, generator=g), "actions": torch.tanh(torch.randn(B, A, generator=g)), "next_obs": torch.randn(B, D, generator=g),
                "rewards": torch.randn(B, generator=g), "dones": (torch.arange(B) % 3 == 1).float()} for _ in range(n)]
    draws = [(torch.randn(B, A, generator=g).clamp(-2.0, 2.0), torch.randn(B, A, generator=g).clamp(-2.0, 2.0)) for _ in range(n)]
    return batches, draws


def critic_tensors(critic, case):
    nets = ref.make_q_nets(case[6], case[7], case[1], case[4], seed=1, device=DEV)
    critic.export(nets)
    return [[(m.weight.detach().clone(), m.bias.detach().clone()) for m in net] for net in nets]


@gpu
def test_sac_gradient_step_matches_sac_train_and_its_four_calls():
    import mujoco_sim_amd as m

    case = aref.CASES[0][:5] + (33,) + aref.CASES[0][6:]  # [64, 64] / [64, 64], two critics, B = 33
    A = case[7]
    gamma, tau = 0.99, 0.005
    batches, draws = full_batches(case, 3)
    actor_cpu, q_cpu = aref.make_nets(aref.CASES[0])
    runs = []
    for by_hand in (False, True):
        actor, critic, _, q_nets = on_device(aref.CASES[0])
        target = m.DeviceCritic.from_linears(DEV, case[6], A, q_nets, activation=case[3])
        c_opt, a_opt, coef = m.DeviceCriticOptimizer(critic), m.DeviceActorOptimizer(actor), m.DeviceEntropyCoef(DEV, A)
        for b, (z_next, z_pi) in zip(batches, draws):
            batch = {k: v.to(DEV) for k, v in b.items()}
            z_next, z_pi = z_next.to(DEV), z_pi.to(DEV)
            if by_hand:
                y = m.sac_td_target(batch, actor, target, gamma, coef.ent_coef, z=z_next)
                c_opt.step(batch, y)
                a_opt.step(batch, critic, coef, z=z_pi)
                target.blend_from(critic, tau)
            else:
                assert m.sac_gradient_step(batch, actor, critic, target, c_opt, a_opt, coef, gamma, tau, z_next=z_next, z_pi=z_pi) is None
        assert (c_opt.step_count, a_opt.step_count, coef.step_count) == (3, 3, 3)
        runs.append((exported(actor, aref.CASES[0]), critic_tensors(critic, case), critic_tensors(target, case), coef.log_ent_coef.clone(), coef.ent_coef.clone()))
        close(c_opt, a_opt, target, critic, actor)
    (pa, pc, pt, le, ec), (ha, hc, ht, hle, hec) = runs
    tensors = lambda a, c, t: flat(a) + [x for net in c + t for x in flat(net)]  # noqa: E731
    assert all(torch.equal(x, y) for x, y in zip(tensors(pa, pc, pt), tensors(ha, hc, ht))) and torch.equal(le, hle) and torch.equal(ec, hec)
    ref64 = aref.sac_train_torch(actor_cpu, q_cpu, q_cpu, batches, draws, case, gamma, tau, torch.float64)
    ref32 = aref.sac_train_torch(actor_cpu, q_cpu, q_cpu, batches, draws, case, gamma, tau, torch.float32)
    aref.check_params("actor", pa, ref64[0], ref32[0])
    tref.check_params("critic", pc, ref64[1], ref32[1])
    tref.check_params("target critic", pt, ref64[2], ref32[2])
    ref.within_bar("log_ent_coef", le.cpu(), ref64[3], ref32[3])


# ------------------------------------------------------------------------- 9. native refusals
def copy_of(struct, **changes):
    c = type(struct)()
    C.memmove(C.byref(c), C.byref(struct), C.sizeof(struct))
    for k, v in changes.items():
        setattr(c, k, v)
    return c


@gpu
def test_native_refusals():
    """Every MJS_ERR_INVALID_ARG of the new entry points through ctypes: the return code, a text in mjs_last_error, nothing launched (the
    outputs keep their fill; the parameters, the moments' effect and t are unchanged: a later good step equals that of an untouched twin).
    Every case names a piece of the text it expects, so that no refusal can stand in for another one that is checked earlier."""
    from mujoco_sim_amd import DeviceActorOptimizer, DeviceCritic, DeviceEntropyCoef, _native as nat

    L = nat.lib()
    case = aref.CASES[2]
    B, D, A = 8, case[6], case[7]
    actor, critic, actor_net, _ = on_device(aref.CASES[2])
    twin, twin_critic, _, _ = on_device(aref.CASES[2])
    other, other_critic, _, _ = on_device(aref.CASES[2])
    opt, twin_opt, other_opt = DeviceActorOptimizer(actor), DeviceActorOptimizer(twin), DeviceActorOptimizer(other)
    coef = DeviceEntropyCoef(DEV, A)
    stream = C.c_void_p(torch.cuda.current_stream(torch.device(DEV)).cuda_stream)
    g = torch.Generator(device=DEV).manual_seed(3)
    obs, z = torch.randn(B, D, device=DEV, generator=g), torch.randn(B, A, device=DEV, generator=g).clamp(-2.0, 2.0)
    fill = -7.0
    outs = {k: torch.full(s, fill, device=DEV) for k, s in (("actions", (B, A)), ("log_prob", (B,)), ("q_pi", (1, B)), ("dq", (B, A)), ("loss", (1,)))}
    params = flat(exported(actor, case))
    state0 = coef._state.clone()

    def untouched():
        return all(bool((t == fill).all()) for t in outs.values()) and all(torch.equal(a, b) for a, b in zip(params, flat(exported(actor, case)))) \
            and torch.equal(coef._state, state0)

    def refused(rc, name, what, text):
        err = L.mjs_last_error(None)
        assert rc == -1 and err.startswith(name.encode() + b": ") and text.encode() in err[len(name) + 2:], (what, text, rc, err)
        assert untouched(), what

    index = (C.c_int32 * D)(*range(D))
    desc = nat.MjsActorDesc(device=0, in_dim=D, n_hidden=1, hidden=(C.c_int32 * 3)(32, 0, 0), action_dim=A, activation=nat.ACTIVATION_RELU, variant=0, obs_index=index)
    unloaded, visual = C.c_void_p(), C.c_void_p()
    assert L.mjs_actor_create(C.byref(desc), C.byref(unloaded)) == 0
    blocks = nat.MjsActorFeatureInputs(n_blocks=1, width=(C.c_int32 * 2)(16, 0), start=(C.c_int32 * 2)(D, 0))
    assert L.mjs_actor_create_visual(C.byref(desc), C.byref(blocks), C.byref(visual)) == 0
    cdesc = nat.MjsCriticDesc(device=0, obs_dim=D, action_dim=A, n_critics=1, n_hidden=1, hidden=(C.c_int32 * 3)(64, 0, 0), activation=nat.ACTIVATION_TANH)
    q_unloaded = C.c_void_p()
    assert L.mjs_critic_create(C.byref(cdesc), C.byref(q_unloaded)) == 0
    # LOADED critics of another obs_dim / action_dim: only the dimension checks stand between them and the launch
    q_wide = DeviceCritic.from_linears(DEV, D + 1, A, ref.make_q_nets(D + 1, A, [64], 1, seed=5, device=DEV), activation="tanh")
    q_more = DeviceCritic.from_linears(DEV, D, A + 1, ref.make_q_nets(D, A + 1, [64], 1, seed=6, device=DEV), activation="tanh")

    # mjs_actor_opt_create
    good = nat.MjsActorOptDesc(lr=3e-4, beta1=0.9, beta2=0.999, eps=1e-8)
    h = C.c_void_p()
    for what, a, d, text in [("null actor", None, good, "null argument"), ("null desc", actor._a, None, "null argument"),
                             ("struct_size", actor._a, copy_of(good, struct_size=32), "mjs_actor_opt_desc.struct_size"),
                             ("never loaded", unloaded, good, "no parameters yet"), ("visual", visual, good, "feature blocks"),
                             ("lr < 0", actor._a, copy_of(good, lr=-1e-3), "lr must"), ("lr nan", actor._a, copy_of(good, lr=float("nan")), "lr must"),
                             ("beta1 = 1", actor._a, copy_of(good, beta1=1.0), "beta1 and beta2"), ("beta2 < 0", actor._a, copy_of(good, beta2=-0.1), "beta1 and beta2"),
                             ("eps = 0", actor._a, copy_of(good, eps=0.0), "eps must")]:
        refused(L.mjs_actor_opt_create(a, C.byref(d) if d is not None else None, C.byref(h)), "mjs_actor_opt_create", what, text)
        assert not h.value, what
    refused(L.mjs_actor_opt_create(actor._a, C.byref(good), None), "mjs_actor_opt_create", "null out", "null argument")
    assert L.mjs_actor_train_workspace_bytes(None, B) == 0 and L.mjs_actor_train_workspace_bytes(actor._a, 0) == 0
    assert L.mjs_actor_train_workspace_bytes(actor._a, -3) == 0 and L.mjs_actor_train_workspace_bytes(visual, B) == 0

    # mjs_actor_grad and mjs_actor_update
    block = coef._block()
    args = nat.MjsActorGradArgs(B=B, obs_dev=obs.data_ptr(), z_dev=z.data_ptr(), critic=critic._q, ent_coef=0.2, actions_out_dev=outs["actions"].data_ptr(),
                                log_prob_out_dev=outs["log_prob"].data_ptr(), q_pi_out_dev=outs["q_pi"].data_ptr(),
                                min_q_action_grad_out_dev=outs["dq"].data_ptr(), loss_out_dev=outs["loss"].data_ptr())
    grads = actor._empty_like_parameters()
    gw = actor._weights_struct(grads)
    missing = copy_of(gw, log_std_b=None)
    ent = lambda **kw: C.pointer(copy_of(block, **kw))  # noqa: E731
    common = [("null args", None, "args is null"), ("struct_size", copy_of(args, struct_size=96), "mjs_actor_grad_args.struct_size"),
              ("B < 0", copy_of(args, B=-1), "B is negative"), ("null obs", copy_of(args, obs_dev=None), "obs_dev or z_dev is null"),
              ("null z", copy_of(args, z_dev=None), "obs_dev or z_dev is null"), ("null critic", copy_of(args, critic=None), "critic is null"),
              ("critic never loaded", copy_of(args, critic=q_unloaded), "the critic has no parameters yet"),
              ("obs_dim mismatch", copy_of(args, critic=q_wide._q), "in_dim is not the critic's obs_dim"),
              ("action_dim mismatch", copy_of(args, critic=q_more._q), "action_dim is not the critic's"),
              ("entropy struct_size", copy_of(args, entropy=ent(struct_size=80)), "mjs_entropy_step.struct_size"),
              ("entropy null log_ent_coef", copy_of(args, entropy=ent(log_ent_coef_dev=None)), "entropy: log_ent_coef_dev"),
              ("entropy null ent_coef", copy_of(args, entropy=ent(ent_coef_dev=None)), "entropy: log_ent_coef_dev"),
              ("entropy null m", copy_of(args, entropy=ent(m_dev=None)), "entropy: log_ent_coef_dev"),
              ("entropy null v", copy_of(args, entropy=ent(v_dev=None)), "entropy: log_ent_coef_dev"),
              ("entropy lr < 0", copy_of(args, entropy=ent(lr=-1e-3)), "entropy: lr"), ("entropy lr nan", copy_of(args, entropy=ent(lr=float("nan"))), "entropy: lr"),
              ("entropy t = 0", copy_of(args, entropy=ent(t=0)), "entropy: t"), ("entropy beta1 = 1", copy_of(args, entropy=ent(beta1=1.0)), "entropy: beta1"),
              ("entropy eps = 0", copy_of(args, entropy=ent(eps=0.0)), "entropy: eps"),
              ("entropy target nan", copy_of(args, entropy=ent(target_entropy=float("nan"))), "entropy: target_entropy")]
    for what, a, text in common:
        ref_a = C.byref(a) if a is not None else None
        refused(L.mjs_actor_grad(actor._a, opt._o, ref_a, stream), "mjs_actor_grad", what, text)
        refused(L.mjs_actor_update(opt._o, ref_a, 3e-4, stream), "mjs_actor_update", what, text)
    refused(L.mjs_actor_grad(None, opt._o, C.byref(args), stream), "mjs_actor_grad", "null actor", "actor, optimiser or args is null")
    refused(L.mjs_actor_grad(actor._a, None, C.byref(args), stream), "mjs_actor_grad", "null optimiser", "actor, optimiser or args is null")
    # An optimiser cannot be created for an actor that was never loaded or that reads feature blocks (mjs_actor_opt_create refuses both,
    # above), and the gradient entry points take the optimiser's own actor: with any other actor, such a one included, the refusal is this
    # one. Their never-loaded and visual refusals guard against a later change of that order and cannot be reached through the ABI today.
    for what, a in (("an optimiser of another actor", other._a), ("a never-loaded actor", unloaded), ("a visual actor", visual)):
        refused(L.mjs_actor_grad(a, opt._o, C.byref(args), stream), "mjs_actor_grad", what, "created for another actor")
    refused(L.mjs_actor_grad(actor._a, other_opt._o, C.byref(args), stream), "mjs_actor_grad", "another actor's optimiser", "created for another actor")
    refused(L.mjs_actor_grad(actor._a, opt._o, C.byref(copy_of(args, grads_out=C.pointer(copy_of(gw, struct_size=80)))), stream), "mjs_actor_grad", "grads struct_size",
            "mjs_actor_weights.struct_size")
    refused(L.mjs_actor_grad(actor._a, opt._o, C.byref(copy_of(args, grads_out=C.pointer(missing))), stream), "mjs_actor_grad", "a null gradient pointer", "grads_out: a layer")
    refused(L.mjs_actor_update(None, C.byref(args), 3e-4, stream), "mjs_actor_update", "null optimiser", "actor, optimiser or args is null")
    for lr in (-1e-3, float("nan"), float("inf")):
        refused(L.mjs_actor_update(opt._o, C.byref(args), lr, stream), "mjs_actor_update", f"lr {lr}", "lr must be finite")
    refused(L.mjs_actor_update(opt._o, C.byref(copy_of(args, grads_out=C.pointer(gw))), 3e-4, stream), "mjs_actor_update", "grads_out in update", "grads_out must be null")
    if torch.cuda.device_count() > 1:
        far = C.c_void_p()
        assert L.mjs_critic_create(C.byref(copy_of(cdesc, device=1)), C.byref(far)) == 0
        refused(L.mjs_actor_grad(actor._a, opt._o, C.byref(copy_of(args, critic=far)), stream), "mjs_actor_grad", "another device", "another device")
        L.mjs_critic_destroy(far)
    # B == 0 does nothing, with null pointers too, and counts no step
    assert L.mjs_actor_grad(actor._a, opt._o, C.byref(copy_of(args, B=0, obs_dev=None)), stream) == 0 and untouched()
    assert L.mjs_actor_update(opt._o, C.byref(copy_of(args, B=0, z_dev=None)), 3e-4, stream) == 0 and untouched()

    # mjs_actor_export
    refused(L.mjs_actor_export(None, C.byref(gw), stream), "mjs_actor_export", "null actor", "null argument")
    refused(L.mjs_actor_export(actor._a, None, stream), "mjs_actor_export", "null weights", "null argument")
    refused(L.mjs_actor_export(actor._a, C.byref(copy_of(gw, struct_size=80)), stream), "mjs_actor_export", "struct_size", "mjs_actor_weights.struct_size")
    refused(L.mjs_actor_export(unloaded, C.byref(gw), stream), "mjs_actor_export", "never loaded", "no parameters yet")
    refused(L.mjs_actor_export(visual, C.byref(gw), stream), "mjs_actor_export", "visual", "feature blocks")
    refused(L.mjs_actor_export(actor._a, C.byref(missing), stream), "mjs_actor_export", "a null pointer", "weight or bias pointer is null")

    # the moments and t are unchanged: the first good step equals the first step of a twin that saw no refusal, bit for bit
    batch = {"obs": obs}
    opt.step(batch, critic, 0.2, z=z)
    twin_opt.step(batch, twin_critic, 0.2, z=z)
    assert opt.step_count == 1 and all(torch.equal(a, b) for a, b in zip(flat(exported(actor, case)), flat(exported(twin, case))))
    assert not all(torch.equal(a, b) for a, b in zip(params, flat(exported(actor, case))))
    # and the good native call goes through
    assert L.mjs_actor_grad(actor._a, opt._o, C.byref(args), stream) == 0
    torch.cuda.synchronize()
    assert not any(bool((t == fill).any()) for t in outs.values())
    for a in (unloaded, visual):
        L.mjs_actor_destroy(a)
    L.mjs_critic_destroy(q_unloaded)
    close(opt, twin_opt, other_opt, q_wide, q_more, critic, twin_critic, other_critic, actor, twin, other)
