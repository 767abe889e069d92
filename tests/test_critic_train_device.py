"""The critic update on the device (csrc/mjs_critic_train.h, DeviceCriticOptimizer) against torch autograd and torch.optim.Adam.

Bars: the project's (tests/_critic_reference.py within_bar), per parameter tensor and for the loss; the seeds are the ones
test_critic_train_host.py checks on the CPU with a float32 evaluation of the kernel's summation shape. Compositions are bit for bit:
the forward pass against q_values, two runs against each other, Adam against its float32 restatement on the kernel's own gradients,
the export / from_linears round trip, the zero-gradient step and the packed-to-packed blend.
"""
import ctypes as C

import numpy as np
import pytest
import torch

import _critic_reference as ref
import _critic_train_reference as tref

gpu = pytest.mark.gpu
DEV = "cuda:0"
D, A = tref.D, tref.A
CASE_IDS = [tref.case_id(c) for c in tref.CASES]


def on_device(case, nets_cpu):
    """A DeviceCritic over device copies of the CPU modules, and those copies."""
    from mujoco_sim_amd import DeviceCritic

    nets = tref.make_nets(case, device=DEV)
    for net, src in zip(nets, nets_cpu):
        for m, s in zip(net, src):
            assert torch.equal(m.weight.cpu(), s.weight) and torch.equal(m.bias.cpu(), s.bias)  # the same seed, the same parameters
    return DeviceCritic.from_linears(DEV, D, A, nets, activation=case[1]), nets


def to_dev(batch):
    obs, actions, target = (t.to(DEV) for t in batch)
    return {"obs": obs, "actions": actions}, target


def exported(critic, case):
    """The packed parameters as fresh modules' tensors [c][l] = (W, b); the critic's own modules stay as they are."""
    nets = tref.make_nets(case, device=DEV)
    critic.export(nets)
    return [[(m.weight.detach().clone(), m.bias.detach().clone()) for m in net] for net in nets]


def flat(tensors):
    return [t for net in tensors for pair in net for t in pair]


# ------------------------------------------------------------------------- 1. - 3. forward, gradients, reproducibility
@gpu
@pytest.mark.parametrize("index", range(len(tref.CASES)), ids=CASE_IDS)
def test_gradients_match_autograd(index):
    from mujoco_sim_amd import DeviceCriticOptimizer, _native as nat

    case = tref.CASES[index]
    widths, activation, n_critics, _ = case
    B = tref.resolve_B(case)
    tps, splits = tref.split_rule(B, widths, n_critics)
    if case[3] == "multi":
        # B = 16 * splits_max + 1: one tile more than there may be splits, so a workgroup owns two tiles, and more than one split
        assert B == 16 * tref.splits_max(widths, n_critics) + 1 and tps == 2 and splits > 1
    nets_cpu, batch_cpu, ref64, ref32 = tref.grad_references(index)
    critic, _ = on_device(case, nets_cpu)
    assert nat.lib().mjs_critic_train_workspace_bytes(critic._q, B) == splits * n_critics * tref.slab_floats(widths) * 4
    opt = DeviceCriticOptimizer(critic)
    batch, target = to_dev(batch_cpu)
    got = opt.gradients(batch, target)
    assert opt.step_count == 0
    # 1. the forward pass is q_kernel's, bit for bit
    assert torch.equal(got["q"], critic.q_values(batch["obs"], batch["actions"]))
    # 2. against autograd
    shapes = [[(tuple(w.shape), tuple(b.shape)) for w, b in net] for net in got["grads"]]
    assert shapes == [[(tuple(m.weight.shape), tuple(m.bias.shape)) for m in net] for net in nets_cpu]
    tref.check_grads(tref.case_id(case), (got["grads"], got["loss"]), ref64, ref32)
    # 3. the same bits again
    again = opt.gradients(batch, target)
    assert all(torch.equal(a, b) for a, b in zip(flat(got["grads"]), flat(again["grads"]))) and torch.equal(got["loss"], again["loss"])
    opt.close()
    critic.close()


@gpu
@pytest.mark.parametrize("case", [tref.CASES[0], tref.CASES[14]], ids=tref.case_id)
def test_two_optimisers_leave_equal_bits(case):
    from mujoco_sim_amd import DeviceCriticOptimizer

    batches = tref.make_batch(case, 3)
    qs = []
    for _ in range(2):
        critic, _ = on_device(case, tref.make_nets(case))
        opt = DeviceCriticOptimizer(critic)
        for b in batches:
            opt.step(*to_dev(b))
        assert opt.step_count == 3
        probe, _ = to_dev(batches[0])
        qs.append(critic.q_values(probe["obs"], probe["actions"]))
        opt.close()
        critic.close()
    assert torch.equal(qs[0], qs[1])
    fresh, _ = on_device(case, tref.make_nets(case))
    assert not torch.equal(qs[0], fresh.q_values(probe["obs"], probe["actions"]))  # and the steps did move the critic
    fresh.close()


# ------------------------------------------------------------------------- 4. Adam, operation by operation
@gpu
@pytest.mark.parametrize("case", [tref.CASES[1], tref.CASES[10], tref.CASES[13]], ids=tref.case_id)
def test_adam_matches_its_float32_restatement(case):
    """Three steps (step 1: both bias corrections at their largest) on the kernel's OWN gradients: the exported parameters equal the
    header's operation order restated in numpy float32, bit for bit. The learning rate changes per step, as SB3's schedule may."""
    from mujoco_sim_amd import DeviceCriticOptimizer

    critic, _ = on_device(case, tref.make_nets(case))
    opt = DeviceCriticOptimizer(critic)
    want = [t.cpu().numpy() for t in flat(exported(critic, case))]
    m = [np.zeros_like(p) for p in want]
    v = [np.zeros_like(p) for p in want]
    for t, (b, lr) in enumerate(zip(tref.make_batch(case, 3), (None, 1e-3, 3e-4)), start=1):
        batch, target = to_dev(b)
        grads = [g.cpu().numpy() for g in flat(opt.gradients(batch, target)["grads"])]
        q_before = critic.q_values(batch["obs"], batch["actions"])
        parts = opt.step(batch, target, lr=lr, return_parts=True)
        assert opt.step_count == t and torch.equal(parts["q"], q_before)  # q and loss are the values BEFORE the step
        for k, g in enumerate(grads):
            want[k], m[k], v[k] = tref.adam_step32(want[k], g, m[k], v[k], t, lr=tref.LR if lr is None else lr)
        got = [p.cpu().numpy() for p in flat(exported(critic, case))]
        for k, (a, b_) in enumerate(zip(got, want)):
            assert np.array_equal(a, b_), (t, k, np.abs(a - b_).max())
    opt.close()
    critic.close()


# ------------------------------------------------------------------------- 5. against torch.optim.Adam
@gpu
@pytest.mark.parametrize("index", range(len(tref.ADAM_CASES)), ids=[tref.case_id(c) for c in tref.ADAM_CASES])
def test_five_steps_match_torch_adam(index):
    from mujoco_sim_amd import DeviceCriticOptimizer

    case = tref.ADAM_CASES[index]
    nets_cpu, batches, ref64, ref32 = tref.adam_references(index)
    critic, _ = on_device(case, nets_cpu)
    opt = DeviceCriticOptimizer(critic)
    for b in batches:
        opt.step(*to_dev(b))
    assert opt.step_count == 5
    tref.check_params(tref.case_id(case), exported(critic, case), ref64, ref32)
    opt.close()
    critic.close()


# ------------------------------------------------------------------------- 6. padding and the round trip
@gpu
def test_round_trip_after_training_keeps_the_padding_zero():
    """[40, 24, 33] with tanh: every layer has padded columns, and tanh'(0) = 1 would carry a non-zero padding forward. A fresh critic made
    from the exported modules (its padding is written 0 by the pack kernels) gives the trained object's q bit for bit."""
    from mujoco_sim_amd import DeviceCritic, DeviceCriticOptimizer

    case = ([40, 24, 33], "tanh", 2, 33)
    critic, nets = on_device(case, tref.make_nets(case))
    opt = DeviceCriticOptimizer(critic)
    batches = tref.make_batch(case, 5)
    before = [t.clone() for t in flat([[(m.weight.detach(), m.bias.detach()) for m in net] for net in nets])]
    for b in batches:
        opt.step(*to_dev(b))
    assert critic.export() is critic.q_nets  # into the modules the object was made from
    after = flat([[(m.weight.detach(), m.bias.detach()) for m in net] for net in nets])
    assert all(not torch.equal(a, b) for a, b in zip(before, after))
    fresh = DeviceCritic.from_linears(DEV, D, A, nets, activation="tanh")
    probe, _ = to_dev(batches[0])
    assert torch.equal(fresh.q_values(probe["obs"], probe["actions"]), critic.q_values(probe["obs"], probe["actions"]))
    for o in (opt, fresh, critic):
        o.close()


# ------------------------------------------------------------------------- 7. zero-gradient rows
@gpu
@pytest.mark.parametrize("case", [tref.CASES[0], tref.CASES[9]], ids=tref.case_id)
def test_a_target_equal_to_q_moves_nothing(case):
    from mujoco_sim_amd import DeviceCritic, DeviceCriticOptimizer

    one = (case[0], case[1], 1, case[3])  # target == q for EVERY critic: one critic, its own q
    critic, _ = on_device(one, tref.make_nets(one))
    opt = DeviceCriticOptimizer(critic)
    batch, _ = to_dev(tref.make_batch(one)[0])
    target = critic.q_values(batch["obs"], batch["actions"])[0].contiguous()
    got = opt.gradients(batch, target)
    assert all(not bool(t.any()) for t in flat(got["grads"])) and not bool(got["loss"].any())
    before = exported(critic, one)
    opt.step(batch, target)
    assert opt.step_count == 1
    assert all(torch.equal(a, b) for a, b in zip(flat(before), flat(exported(critic, one))))
    opt.close()
    critic.close()


# ------------------------------------------------------------------------- 8. blend_from
@gpu
def test_blend_from_a_packed_copy():
    from mujoco_sim_amd import DeviceCritic, DeviceCriticOptimizer

    case = ([40, 24, 33], "relu", 2, 33)
    online, _ = on_device(case, tref.make_nets(case))
    other_nets = ref.make_q_nets(D, A, case[0], 2, seed=977, device=DEV)
    target = DeviceCritic.from_linears(DEV, D, A, other_nets, activation="relu")
    opt = DeviceCriticOptimizer(online)
    batches = tref.make_batch(case, 2)
    for b in batches:
        opt.step(*to_dev(b))
    probe, _ = to_dev(batches[0])
    src, dst = exported(online, case), exported(target, case)
    tau = 0.005
    target.blend_from(online, tau)
    got = exported(target, case)
    for (gw, gb), (sw, sb), (dw, db) in zip((p for net in got for p in net), (p for net in src for p in net), (p for net in dst for p in net)):
        out, fan_in = gw.shape
        K, O = ref.round_up(fan_in, ref.KPAD), ref.round_up(out, ref.OPAD)
        packed_w, packed_b = ref.pack_lerp_np(None, None, dw.cpu().numpy(), db.cpu().numpy(), K, O, 1.0)
        want_w, want_b = ref.pack_lerp_np(packed_w, packed_b, sw.cpu().numpy(), sb.cpu().numpy(), K, O, tau)
        assert np.array_equal(gw.cpu().numpy(), want_w[:fan_in, :out].T) and np.array_equal(gb.cpu().numpy(), want_b[:out])
    assert not torch.equal(target.q_values(probe["obs"], probe["actions"]), online.q_values(probe["obs"], probe["actions"]))
    target.blend_from(online, 1.0)
    assert torch.equal(target.q_values(probe["obs"], probe["actions"]), online.q_values(probe["obs"], probe["actions"]))
    for o in (opt, target, online):
        o.close()


# ------------------------------------------------------------------------- 9. a full gradient step on a sampled batch
@gpu
def test_full_gradient_steps_on_a_sampled_batch():
    import mujoco_sim_amd as m

    venv = m.HipVectorEnv("robot_reach", 16, seed=7)
    venv.reset(seed=3)
    assert sum(n for _, _, n in venv.flat_observation_layout) == D and venv.action_dim == A
    actor = m.DeviceActor.from_linears(venv, *ref.make_actor(D, [64, 64], A, seed=41, device=DEV))
    nets = ref.make_q_nets(D, A, [64, 64], 2, seed=42, device=DEV)
    critic, target_critic = m.DeviceCritic.from_linears(DEV, D, A, nets), m.DeviceCritic.from_linears(DEV, D, A, nets)
    opt = m.DeviceCriticOptimizer(critic, lr=1e-3)
    buf = m.DeviceReplayBuffer(venv, 1000)
    buf.collect(venv, actor, 8, generator=torch.Generator(device=DEV).manual_seed(1))
    batch = buf.sample(64, generator=torch.Generator(device=DEV).manual_seed(2))
    z = torch.randn(64, A, dtype=torch.float32, device=DEV, generator=torch.Generator(device=DEV).manual_seed(3)).clamp(-2.0, 2.0)
    y0 = m.sac_td_target(batch, actor, target_critic, 0.99, 0.005, z=z)  # the regression target the losses below are measured against
    first = opt.gradients(batch, y0)["loss"]
    for _ in range(20):
        y = m.sac_td_target(batch, actor, target_critic, 0.99, 0.005, z=z)
        parts = opt.step(batch, y, return_parts=True)
        target_critic.blend_from(critic, 0.005)
        assert bool(torch.isfinite(parts["loss"]).all())
    last = opt.gradients(batch, y0)["loss"]
    print(f"critic losses on the batch: {first.tolist()} -> {last.tolist()} after 20 steps")
    assert opt.step_count == 20 and bool(torch.isfinite(last).all()) and bool((last < first).all())
    for o in (opt, target_critic, critic, actor, buf):
        o.close()
    venv.close()


# ------------------------------------------------------------------------- 10. native refusals
def copy_of(struct, **changes):
    c = type(struct)()
    C.memmove(C.byref(c), C.byref(struct), C.sizeof(struct))
    for k, v in changes.items():
        setattr(c, k, v)
    return c


@gpu
def test_native_refusals():
    """Every MJS_ERR_INVALID_ARG of the new entry points through ctypes: the return code, text in mjs_last_error, nothing launched (the
    outputs keep their fill, the parameters their bits)."""
    from mujoco_sim_amd import DeviceCritic, DeviceCriticOptimizer, _native as nat

    L = nat.lib()
    case = ([32], "relu", 2, 8)
    B = 8
    critic, nets = on_device(case, tref.make_nets(case))
    other, _ = on_device(case, tref.make_nets(case))
    opt, other_opt = DeviceCriticOptimizer(critic), DeviceCriticOptimizer(other)
    stream = C.c_void_p(torch.cuda.current_stream(torch.device(DEV)).cuda_stream)
    batch, target = to_dev(tref.make_batch(case)[0])
    fill = -7.0
    q_out, loss_out = torch.full((2, B), fill, device=DEV), torch.full((2,), fill, device=DEV)
    probe = critic.q_values(batch["obs"], batch["actions"])

    def untouched():
        return bool((q_out == fill).all()) and bool((loss_out == fill).all()) and torch.equal(probe, critic.q_values(batch["obs"], batch["actions"]))

    def refused(rc, name, what):
        err = L.mjs_last_error(None)
        assert rc == -1 and err.startswith(name.encode() + b": ") and len(err) > len(name) + 2, (what, rc, err)
        assert untouched(), what

    # an unloaded critic of the same shape
    desc = nat.MjsCriticDesc(device=0, obs_dim=D, action_dim=A, n_critics=2, n_hidden=1, hidden=(C.c_int32 * 3)(32, 0, 0), activation=nat.ACTIVATION_RELU)
    unloaded, narrow = C.c_void_p(), C.c_void_p()
    assert L.mjs_critic_create(C.byref(desc), C.byref(unloaded)) == 0
    assert L.mjs_critic_create(C.byref(copy_of(desc, hidden=(C.c_int32 * 3)(33, 0, 0))), C.byref(narrow)) == 0

    # mjs_critic_opt_create
    good = nat.MjsCriticOptDesc(lr=3e-4, beta1=0.9, beta2=0.999, eps=1e-8)
    h = C.c_void_p()
    for what, q, d in [("null critic", None, good), ("null desc", critic._q, None), ("struct_size", critic._q, copy_of(good, struct_size=32)),
                       ("never loaded", unloaded, good), ("lr < 0", critic._q, copy_of(good, lr=-1e-3)), ("lr nan", critic._q, copy_of(good, lr=float("nan"))),
                       ("beta1 = 1", critic._q, copy_of(good, beta1=1.0)), ("beta1 < 0", critic._q, copy_of(good, beta1=-0.1)),
                       ("beta2 = 1", critic._q, copy_of(good, beta2=1.0)), ("beta2 nan", critic._q, copy_of(good, beta2=float("nan"))),
                       ("eps = 0", critic._q, copy_of(good, eps=0.0)), ("eps < 0", critic._q, copy_of(good, eps=-1e-8))]:
        refused(L.mjs_critic_opt_create(q, C.byref(d) if d is not None else None, C.byref(h)), "mjs_critic_opt_create", what)
        assert not h.value, what
    refused(L.mjs_critic_opt_create(critic._q, C.byref(good), None), "mjs_critic_opt_create", "null out")
    assert L.mjs_critic_train_workspace_bytes(None, B) == 0 and L.mjs_critic_train_workspace_bytes(critic._q, 0) == 0
    assert L.mjs_critic_train_workspace_bytes(critic._q, -3) == 0

    # mjs_critic_grad and mjs_critic_update
    args = nat.MjsCriticGradArgs(B=B, obs_dev=batch["obs"].data_ptr(), actions_dev=batch["actions"].data_ptr(), target_dev=target.data_ptr(),
                                 q_out_dev=q_out.data_ptr(), loss_out_dev=loss_out.data_ptr())
    grads = critic._empty_like_parameters()
    gw = critic._weights_struct(grads)
    missing = copy_of(gw)
    missing.hidden_b[1][0] = None
    common = [("null args", None), ("struct_size", copy_of(args, struct_size=48)), ("B < 0", copy_of(args, B=-1)), ("null obs", copy_of(args, obs_dev=None)),
              ("null actions", copy_of(args, actions_dev=None)), ("null target", copy_of(args, target_dev=None))]
    for what, a in common:
        ref_a = C.byref(a) if a is not None else None
        refused(L.mjs_critic_grad(critic._q, opt._o, ref_a, stream), "mjs_critic_grad", what)
        refused(L.mjs_critic_update(opt._o, ref_a, 3e-4, stream), "mjs_critic_update", what)
    refused(L.mjs_critic_grad(None, opt._o, C.byref(args), stream), "mjs_critic_grad", "null critic")
    refused(L.mjs_critic_grad(critic._q, None, C.byref(args), stream), "mjs_critic_grad", "null optimiser")
    refused(L.mjs_critic_grad(critic._q, other_opt._o, C.byref(args), stream), "mjs_critic_grad", "an optimiser of another critic")
    refused(L.mjs_critic_grad(critic._q, opt._o, C.byref(copy_of(args, grads_out=C.pointer(copy_of(gw, struct_size=128)))), stream), "mjs_critic_grad", "grads struct_size")
    refused(L.mjs_critic_grad(critic._q, opt._o, C.byref(copy_of(args, grads_out=C.pointer(missing))), stream), "mjs_critic_grad", "a null gradient pointer")
    refused(L.mjs_critic_update(None, C.byref(args), 3e-4, stream), "mjs_critic_update", "null optimiser")
    for lr in (-1e-3, float("nan"), float("inf")):
        refused(L.mjs_critic_update(opt._o, C.byref(args), lr, stream), "mjs_critic_update", f"lr {lr}")
    refused(L.mjs_critic_update(opt._o, C.byref(copy_of(args, grads_out=C.pointer(gw))), 3e-4, stream), "mjs_critic_update", "grads_out in update")
    # B == 0 does nothing, with null pointers too
    assert L.mjs_critic_grad(critic._q, opt._o, C.byref(copy_of(args, B=0, obs_dev=None)), stream) == 0 and untouched()
    assert L.mjs_critic_update(opt._o, C.byref(copy_of(args, B=0, target_dev=None)), 3e-4, stream) == 0 and untouched()

    # mjs_critic_blend
    for what, dst, src, tau in [("null dst", None, critic._q, 0.5), ("null src", critic._q, None, 0.5), ("another shape", critic._q, narrow, 0.5),
                                ("src never loaded", critic._q, unloaded, 0.5), ("dst never loaded, tau < 1", unloaded, critic._q, 0.5),
                                ("tau 0", critic._q, other._q, 0.0), ("tau < 0", critic._q, other._q, -0.5), ("tau > 1", critic._q, other._q, 1.5),
                                ("tau nan", critic._q, other._q, float("nan"))]:
        refused(L.mjs_critic_blend(dst, src, tau, stream), "mjs_critic_blend", what)
    if torch.cuda.device_count() > 1:
        far = C.c_void_p()
        assert L.mjs_critic_create(C.byref(copy_of(desc, device=1)), C.byref(far)) == 0
        refused(L.mjs_critic_blend(far, critic._q, 1.0, stream), "mjs_critic_blend", "another device")
        L.mjs_critic_destroy(far)

    # mjs_critic_export
    refused(L.mjs_critic_export(None, C.byref(gw), stream), "mjs_critic_export", "null critic")
    refused(L.mjs_critic_export(critic._q, None, stream), "mjs_critic_export", "null weights")
    refused(L.mjs_critic_export(critic._q, C.byref(copy_of(gw, struct_size=128)), stream), "mjs_critic_export", "struct_size")
    refused(L.mjs_critic_export(unloaded, C.byref(gw), stream), "mjs_critic_export", "never loaded")
    refused(L.mjs_critic_export(critic._q, C.byref(missing), stream), "mjs_critic_export", "a null pointer")

    # and the good calls go through: a never-loaded dst takes tau = 1
    assert L.mjs_critic_blend(unloaded, critic._q, 1.0, stream) == 0
    unl_q = torch.empty(2, B, device=DEV)
    assert L.mjs_critic_q(unloaded, batch["obs"].data_ptr(), batch["actions"].data_ptr(), B, unl_q.data_ptr(), stream) == 0
    assert torch.equal(unl_q, probe)
    assert L.mjs_critic_grad(critic._q, opt._o, C.byref(args), stream) == 0 and torch.equal(q_out, probe) and bool((loss_out > 0).all())
    torch.cuda.synchronize()
    L.mjs_critic_destroy(unloaded)
    L.mjs_critic_destroy(narrow)
    for o in (opt, other_opt, other, critic):
        o.close()
