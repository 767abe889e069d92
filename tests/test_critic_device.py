"""SAC's critics and the fused TD target on the device (csrc/mjs_critic.h, mujoco_sim_amd/policies.py) against torch.

Bars. The kernels are float32 with float32 accumulation; torch's own float32 evaluation of the same modules is another float32
evaluation in another summation order, so both sit at the same order of distance from the float64 evaluation. The yardstick e32 =
max |torch float32 - torch float64| is measured per quantity in the test, and a quantity passes if max |kernel - torch float64| <=
max(4 e32, 8 * 2^-24 * max(1, max |float64|)) (tests/_critic_reference.py within_bar). The draws z are clamped to [-2, 2]: log(1 - a^2 +
1e-6) amplifies a one-ulp difference in a without bound as |a| -> 1, and the comparison is to test the kernel, not conditioning.
Compositions (q_next against q_values, target against its formula on the kernel's own parts) and the done mask: bit for bit.
"""
import ctypes as C

import numpy as np
import pytest
import torch

import _critic_reference as ref

gpu = pytest.mark.gpu
DEV = "cuda:0"
BATCHES = (1, 15, 16, 17, 33)  # the edges of the 16-row tile
WIDTHS = ([32], [48], [64, 64], [256, 256], [64, 32, 96])
SHAPES = ((4, 2), (12, 3), (60, 8))  # (D, A); the last crosses 64 input columns
GAMMA, ENT = 0.99, 0.005


def make_batch(B, D, A, seed):
    """obs / next_obs randn, stored actions tanh(randn), rewards randn, dones with both values present (B > 1), z = randn.clamp(-2, 2)."""
    g = torch.Generator(device=DEV).manual_seed(seed)
    rn = lambda *s: torch.randn(*s, dtype=torch.float32, device=DEV, generator=g)  # noqa: E731
    dones = (torch.arange(B, device=DEV) % 3 == 1).float()
    return {"obs": rn(B, D), "next_obs": rn(B, D), "actions": torch.tanh(rn(B, A)), "rewards": rn(B), "dones": dones}, rn(B, A).clamp(-2.0, 2.0)


def float32_formula(parts, batch, gamma, ent_coef):
    """r + (1 - d) * gamma * (q_next.min(0) - ent_coef * logp) in torch float32, one operation per line, on the kernel's own parts."""
    f32 = lambda v: torch.tensor(v, dtype=torch.float32, device=DEV)  # noqa: E731
    keep = 1.0 - batch["dones"]
    disc = keep * f32(gamma)
    el = f32(ent_coef) * parts["next_log_prob"]
    soft = parts["q_next"].min(dim=0).values - el
    boot = disc * soft
    return batch["rewards"] + boot


# ---------------------------------------------------------------------------------------------- 1. q_values against torch
@gpu
@pytest.mark.parametrize("activation", ["relu", "tanh"])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: f"D{s[0]}A{s[1]}")
@pytest.mark.parametrize("widths", WIDTHS, ids=lambda w: "x".join(map(str, w)))
def test_q_values_match_torch(widths, shape, activation):
    from mujoco_sim_amd import DeviceCritic

    D, A = shape
    for n_critics in (1, 2):
        nets = ref.make_q_nets(D, A, widths, n_critics, seed=1000 * len(widths) + widths[0], device=DEV)
        critic = DeviceCritic.from_linears(DEV, D, A, nets, activation=activation)
        assert (critic.n_critics, critic.obs_dim, critic.action_dim, critic.widths) == (n_critics, D, A, list(widths))
        for B in BATCHES:
            batch, _ = make_batch(B, D, A, seed=B)
            q = critic.q_values(batch["obs"], batch["actions"])
            ref64 = ref.q_ref(nets, batch["obs"], batch["actions"], activation, torch.float64)
            ref32 = ref.q_ref(nets, batch["obs"], batch["actions"], activation, torch.float32)
            ref.within_bar(f"q {widths} {activation} D={D} A={A} n={n_critics} B={B}", q, ref64, ref32)
            if n_critics == 2:
                assert not torch.equal(q[0], q[1])  # two critics from two seeds
        assert critic.q_values(batch["obs"][:0], batch["actions"][:0]).shape == (n_critics, 0)
        critic.close()


# ---------------------------------------------------------------------------------------------- 2. + 3. the fused target
ACTOR_CRITIC = (([32], [256, 256]), ([256, 256], [48]))  # different shapes in both directions: the LDS stride must serve the wider one


@pytest.fixture(scope="module")
def reach():
    """A Robot-Reach handle: DeviceActor takes its device and action width (3) from an env; tests 2-5 pick its columns by obs_index."""
    import mujoco_sim_amd as m

    venv = m.HipVectorEnv("robot_reach", 33, seed=7)
    venv.reset()
    yield venv
    venv.close()


def make_pair(venv, D, actor_widths, critic_widths, n_critics=2, actor_activation="relu", critic_activation="tanh", seed=11):
    from mujoco_sim_amd import DeviceActor, DeviceCritic

    A = venv.action_dim
    actor_net = ref.make_actor(D, actor_widths, A, seed=seed, device=DEV)
    nets = ref.make_q_nets(D, A, critic_widths, n_critics, seed=seed + 1, device=DEV)
    actor = DeviceActor.from_linears(venv, *actor_net, activation=actor_activation, obs_index=list(range(D)))
    critic = DeviceCritic.from_linears(DEV, D, A, nets, activation=critic_activation)
    return actor, critic, actor_net, nets


@gpu
@pytest.mark.parametrize("D", [5, 12])
@pytest.mark.parametrize("widths", ACTOR_CRITIC, ids=lambda w: "x".join(map(str, w)))
def test_td_target_parts_match_torch_and_compose_bit_for_bit(reach, widths, D):
    from mujoco_sim_amd import sac_td_target

    actor, critic, actor_net, nets = make_pair(reach, D, *widths)
    A = reach.action_dim
    ent_dev = torch.tensor([ENT], dtype=torch.float32, device=DEV)
    for B in BATCHES:
        batch, z = make_batch(B, D, A, seed=100 + B)
        parts = sac_td_target(batch, actor, critic, GAMMA, ENT, z=z, return_parts=True)
        ref64 = ref.td_ref(actor_net, nets, batch, z, GAMMA, ENT, "relu", "tanh", torch.float64)
        ref32 = ref.td_ref(actor_net, nets, batch, z, GAMMA, ENT, "relu", "tanh", torch.float32)
        for name in ("next_actions", "next_log_prob", "q_next", "target"):
            ref.within_bar(f"{name} actor {widths[0]} critic {widths[1]} D={D} B={B}", parts[name], ref64[name], ref32[name])
        # the entropy coefficient from device memory: the same float32, the same results
        parts_dev = sac_td_target(batch, actor, critic, GAMMA, ent_dev, z=z, return_parts=True)
        for name in parts:
            assert torch.equal(parts[name], parts_dev[name]), (name, B)
        assert torch.equal(sac_td_target(batch, actor, critic, GAMMA, ENT, z=z), parts["target"])  # without the optional outputs
        # 3. composition, bit for bit: the critics run as in q_values, and the tail is the formula operation by operation
        assert torch.equal(parts["q_next"], critic.q_values(batch["next_obs"], parts["next_actions"])), B
        assert torch.equal(parts["target"], float32_formula(parts, batch, GAMMA, ENT)), B
    actor.close()
    critic.close()


@gpu
def test_one_critic_and_default_draws(reach):
    """n_critics = 1 (the min over one), and z drawn by the call: the generator's torch.randn(B, A)."""
    from mujoco_sim_amd import sac_td_target

    D, A, B = 12, reach.action_dim, 17
    actor, critic, actor_net, nets = make_pair(reach, D, [64, 64], [64, 64], n_critics=1, critic_activation="relu")
    batch, _ = make_batch(B, D, A, seed=5)
    parts = sac_td_target(batch, actor, critic, GAMMA, ENT, generator=torch.Generator(device=DEV).manual_seed(9), return_parts=True)
    z = torch.randn(B, A, dtype=torch.float32, device=DEV, generator=torch.Generator(device=DEV).manual_seed(9))
    same = sac_td_target(batch, actor, critic, GAMMA, ENT, z=z, return_parts=True)
    for name in parts:
        assert torch.equal(parts[name], same[name]), name
    assert parts["q_next"].shape == (1, B) and torch.equal(parts["target"], float32_formula(parts, batch, GAMMA, ENT))
    actor.close()
    critic.close()


# ---------------------------------------------------------------------------------------------- 4. masks matter
@gpu
def test_done_rows_do_not_bootstrap(reach):
    from mujoco_sim_amd import sac_td_target

    D, A, B = 12, reach.action_dim, 33
    actor, critic, _, _ = make_pair(reach, D, [64, 64], [64, 64])
    batch, z = make_batch(B, D, A, seed=6)
    target = sac_td_target(batch, actor, critic, GAMMA, ENT, z=z)
    done = batch["dones"] == 1
    assert bool(done.any()) and bool((~done).any())
    assert torch.equal(target[done], batch["rewards"][done])       # bit for bit the reward
    assert not bool((target[~done] == batch["rewards"][~done]).any())
    for row in (0, 16, 32):  # flipping one row's done changes that row only
        flipped = {**batch, "dones": batch["dones"].clone()}
        flipped["dones"][row] = 1.0 - flipped["dones"][row]
        other = sac_td_target(flipped, actor, critic, GAMMA, ENT, z=z)
        changed = other != target
        assert bool(changed[row]) and int(changed.sum()) == 1, row
    actor.close()
    critic.close()


# ---------------------------------------------------------------------------------------------- 5. lerp load
@gpu
def test_lerp_load_matches_a_float64_blend():
    from mujoco_sim_amd import DeviceCritic

    D, A, B, tau, widths = 12, 3, 33, 0.005, [64, 48]
    q0 = ref.make_q_nets(D, A, widths, 2, seed=21, device=DEV)
    q1 = ref.make_q_nets(D, A, widths, 2, seed=22, device=DEV)
    critic = DeviceCritic.from_linears(DEV, D, A, q0)
    critic.load(q1, tau=tau)
    blend = ref.make_q_nets(D, A, widths, 2, seed=23, device=DEV)
    for nb, n0, n1 in zip(blend, q0, q1):
        for mb, m0, m1 in zip(nb, n0, n1):
            mb.double()
            with torch.no_grad():
                mb.weight.copy_((1.0 - tau) * m0.weight.double() + tau * m1.weight.double())
                mb.bias.copy_((1.0 - tau) * m0.bias.double() + tau * m1.bias.double())
    batch, _ = make_batch(B, D, A, seed=8)
    q = critic.q_values(batch["obs"], batch["actions"])
    ref64 = ref.q_ref(blend, batch["obs"], batch["actions"], "relu", torch.float64)
    ref32 = ref.q_ref(blend, batch["obs"], batch["actions"], "relu", torch.float32)  # (the float64 blend rounded to float32)
    ref.within_bar("q after load(q0); load(q1, tau=0.005)", q, ref64, ref32)
    assert not torch.equal(q, DeviceCritic.from_linears(DEV, D, A, q0).q_values(batch["obs"], batch["actions"]))  # the blend moved it
    # tau = 1 after a lerp reproduces a fresh load bit for bit
    critic.load(q1, tau=1.0)
    fresh = DeviceCritic.from_linears(DEV, D, A, q1)
    assert torch.equal(critic.q_values(batch["obs"], batch["actions"]), fresh.q_values(batch["obs"], batch["actions"]))
    critic.close()
    fresh.close()


def probe_nets(D, A, seed):
    """One critic whose hidden layer is the identity on D + A inputs with zero biases: on the one-hot input e_k (relu) the hidden
    activations are e_k and q = out_w[k], exactly. Blending two of them leaves the identity alone where fl32(tau) + fl32(1 - tau)
    rounds to 1 (checked by the caller), so q reads the blended out_w[k]."""
    n = D + A
    hidden, out = torch.nn.Linear(n, n), torch.nn.Linear(n, 1)
    with torch.no_grad():
        hidden.weight.copy_(torch.eye(n))
        hidden.bias.zero_()
        out.weight.copy_(torch.randn(1, n, generator=torch.Generator().manual_seed(seed)))
        out.bias.zero_()
    return [[hidden.to(DEV), out.to(DEV)]]


@gpu
def test_lerp_load_blends_each_parameter_within_four_half_ulps():
    from mujoco_sim_amd import DeviceCritic

    D, A, tau = 5, 3, 0.005
    assert np.float32(np.float64(np.float32(tau)) + np.float64(np.float32(1.0 - tau))) == np.float32(1.0)  # the identity's diagonal stays 1
    q0, q1 = probe_nets(D, A, seed=31), probe_nets(D, A, seed=32)
    critic = DeviceCritic.from_linears(DEV, D, A, q0)
    eye = torch.eye(D + A, dtype=torch.float32, device=DEV)
    obs, actions = eye[:, :D].contiguous(), eye[:, D:].contiguous()
    assert torch.equal(critic.q_values(obs, actions)[0], q0[0][1].weight.detach()[0])  # the probe reads a parameter exactly
    critic.load(q1, tau=tau)  # (a FIRST load with tau < 1 is refused: test_native_refusals, and tests/test_critic_host.py for the Python check)
    got = critic.q_values(obs, actions)[0].double().cpu()
    t, p = q0[0][1].weight.detach()[0].double().cpu(), q1[0][1].weight.detach()[0].double().cpu()
    want = (1.0 - tau) * t + tau * p
    bound = 4 * ref.ULP * torch.maximum(t.abs(), p.abs())
    print(f"blended parameters: max |kernel - float64 blend| / bound = {((got - want).abs() / bound).max().item():.3f}")
    assert bool(((got - want).abs() <= bound).all())
    critic.close()


# ---------------------------------------------------------------------------------------------- 6. from the buffer
@gpu
def test_td_target_on_a_sampled_batch(reach):
    from mujoco_sim_amd import DeviceActor, DeviceCritic, DeviceReplayBuffer, sac_td_target

    venv = reach
    D, A = 12, venv.action_dim
    assert sum(n for _, _, n in venv.flat_observation_layout) == D
    actor_net = ref.make_actor(D, [64, 64], A, seed=41, device=DEV)
    nets = ref.make_q_nets(D, A, [64, 64], 2, seed=42, device=DEV)
    actor = DeviceActor.from_linears(venv, *actor_net)
    critic = DeviceCritic.from_linears(DEV, D, A, nets)
    buf = DeviceReplayBuffer(venv, 1000)
    venv.reset(seed=3)
    buf.collect(venv, actor, 8, generator=torch.Generator(device=DEV).manual_seed(1))
    batch = buf.sample(17, generator=torch.Generator(device=DEV).manual_seed(2))
    z = torch.randn(17, A, dtype=torch.float32, device=DEV, generator=torch.Generator(device=DEV).manual_seed(3)).clamp(-2.0, 2.0)
    parts = sac_td_target(batch, actor, critic, GAMMA, ENT, z=z, return_parts=True)
    ref64 = ref.td_ref(actor_net, nets, batch, z, GAMMA, ENT, "relu", "relu", torch.float64)
    ref32 = ref.td_ref(actor_net, nets, batch, z, GAMMA, ENT, "relu", "relu", torch.float32)
    for name in ("next_actions", "next_log_prob", "q_next", "target"):
        ref.within_bar(f"{name} on a batch of the buffer", parts[name], ref64[name], ref32[name])
    ref.within_bar("q_values on the batch", critic.q_values(batch["obs"], batch["actions"]), ref.q_ref(nets, batch["obs"], batch["actions"], "relu", torch.float64),
                   ref.q_ref(nets, batch["obs"], batch["actions"], "relu", torch.float32))
    # an actor that reads other columns than the buffer stores
    narrow_net = ref.make_actor(6, [32], A, seed=43, device=DEV)
    narrow = DeviceActor.from_linears(venv, *narrow_net, obs_index=list(range(6)))
    with pytest.raises(ValueError, match="observation columns"):
        sac_td_target(batch, narrow, critic, GAMMA, ENT, z=z)
    for o in (narrow, actor, critic, buf):
        o.close()


# ---------------------------------------------------------------------------------------------- 7. native refusals
def copy_of(struct, **changes):
    c = type(struct)()
    C.memmove(C.byref(c), C.byref(struct), C.sizeof(struct))
    for k, v in changes.items():
        setattr(c, k, v)
    return c


@gpu
def test_native_refusals(reach):
    """Every MJS_ERR_INVALID_ARG of include/mjsim.h through ctypes: nothing launched (the outputs keep their fill), text set."""
    from mujoco_sim_amd import _native as nat

    L = nat.lib()
    D, A, B = 12, reach.action_dim, 8
    actor, critic, _, _ = make_pair(reach, D, [32], [32])
    stream = C.c_void_p(torch.cuda.current_stream(torch.device(DEV)).cuda_stream)
    batch, z = make_batch(B, D, A, seed=1)
    fill = -7.0
    target, q_out = torch.full((B,), fill, device=DEV), torch.full((2, B), fill, device=DEV)

    def untouched():
        return bool((target == fill).all()) and bool((q_out == fill).all())

    # mjs_critic_create
    good_desc = nat.MjsCriticDesc(device=0, obs_dim=D, action_dim=A, n_critics=2, n_hidden=1, hidden=(C.c_int32 * 3)(32, 0, 0), activation=nat.ACTIVATION_RELU)
    h = C.c_void_p()
    for what, desc in [("struct_size", copy_of(good_desc, struct_size=36)), ("obs_dim 0", copy_of(good_desc, obs_dim=0)), ("obs_dim 65", copy_of(good_desc, obs_dim=65)),
                       ("action_dim 0", copy_of(good_desc, action_dim=0)), ("action_dim 9", copy_of(good_desc, action_dim=9)), ("n_critics 0", copy_of(good_desc, n_critics=0)),
                       ("n_critics 3", copy_of(good_desc, n_critics=3)), ("n_hidden 0", copy_of(good_desc, n_hidden=0)), ("n_hidden 4", copy_of(good_desc, n_hidden=4)),
                       ("width 0", copy_of(good_desc, n_hidden=2)), ("width 257", copy_of(good_desc, hidden=(C.c_int32 * 3)(257, 0, 0))),
                       ("activation", copy_of(good_desc, activation=2)), ("device", copy_of(good_desc, device=-1))]:
        assert L.mjs_critic_create(C.byref(desc), C.byref(h)) == -1 and L.mjs_last_error(None).startswith(b"mjs_critic_create: ") and not h.value, what
    assert L.mjs_critic_create(None, C.byref(h)) == -1 and L.mjs_critic_create(C.byref(good_desc), None) == -1
    # mjs_critic_load, on a critic that was never loaded
    assert L.mjs_critic_create(C.byref(good_desc), C.byref(h)) == 0 and h.value
    w = nat.MjsCriticWeights()
    for c, net in enumerate(critic._staged):
        for l, (wt, bs) in enumerate(net[:-1]):
            w.hidden_w[c][l], w.hidden_b[c][l] = wt.data_ptr(), bs.data_ptr()
        w.out_w[c], w.out_b[c] = net[-1][0].data_ptr(), net[-1][1].data_ptr()

    def refused_load(weights, tau, what, text):
        rc = L.mjs_critic_load(h, C.byref(weights) if weights is not None else None, tau, stream)
        assert rc == -1 and L.mjs_last_error(None).startswith(b"mjs_critic_load: ") and text in L.mjs_last_error(None), (what, L.mjs_last_error(None))

    refused_load(w, 0.5, "a first load with tau < 1", b"first load")
    for tau in (0.0, -1.0, 1.5, float("nan")):
        refused_load(w, tau, f"tau {tau}", b"tau must lie")
    refused_load(None, 1.0, "null weights", b"null argument")
    refused_load(copy_of(w, struct_size=128), 1.0, "weights struct_size", b"struct_size")
    missing = copy_of(w)
    missing.hidden_b[1][0] = None
    refused_load(missing, 1.0, "a null bias", b"hidden layer")
    missing = copy_of(w)
    missing.out_w[0] = None
    refused_load(missing, 1.0, "a null head", b"head")
    assert L.mjs_critic_load(None, C.byref(w), 1.0, stream) == -1
    # ... which mjs_critic_q and mjs_sac_td_target refuse
    obs_p, act_p = batch["obs"].data_ptr(), batch["actions"].data_ptr()

    def refused_q(crit_h, o, a, n, out, what):
        assert L.mjs_critic_q(crit_h, o, a, n, out, stream) == -1 and L.mjs_last_error(None).startswith(b"mjs_critic_q: "), what
        assert untouched(), what

    refused_q(h, obs_p, act_p, B, q_out.data_ptr(), "a critic that was never loaded")
    refused_q(None, obs_p, act_p, B, q_out.data_ptr(), "null critic")
    refused_q(critic._q, None, act_p, B, q_out.data_ptr(), "null obs")
    refused_q(critic._q, obs_p, None, B, q_out.data_ptr(), "null actions")
    refused_q(critic._q, obs_p, act_p, B, None, "null output")
    refused_q(critic._q, obs_p, act_p, -1, q_out.data_ptr(), "negative B")
    assert L.mjs_critic_q(critic._q, None, None, 0, None, stream) == 0 and untouched()  # B == 0

    good = nat.MjsTdTargetArgs(B=B, next_obs_dev=batch["next_obs"].data_ptr(), rewards_dev=batch["rewards"].data_ptr(), dones_dev=batch["dones"].data_ptr(),
                               z_dev=z.data_ptr(), gamma=GAMMA, ent_coef=ENT, target_out_dev=target.data_ptr(), q_next_out_dev=q_out.data_ptr())

    def refused_td(a, q, args, what, text):
        rc = L.mjs_sac_td_target(a, q, C.byref(args) if args is not None else None, stream)
        assert rc == -1 and L.mjs_last_error(None).startswith(b"mjs_sac_td_target: ") and text in L.mjs_last_error(None), (what, L.mjs_last_error(None))
        assert untouched(), what

    refused_td(actor._a, h, good, "a critic that was never loaded", b"mjs_critic_load")
    refused_td(None, critic._q, good, "null actor", b"is null")
    refused_td(actor._a, None, good, "null critic", b"is null")
    refused_td(actor._a, critic._q, None, "null args", b"is null")
    refused_td(actor._a, critic._q, copy_of(good, struct_size=88), "args struct_size", b"struct_size")
    for field in ("next_obs_dev", "rewards_dev", "dones_dev", "z_dev", "target_out_dev"):
        refused_td(actor._a, critic._q, copy_of(good, **{field: None}), field, b"is null")
    refused_td(actor._a, critic._q, copy_of(good, B=-1), "negative B", b"B is negative")
    for gamma in (-0.01, 1.01, float("nan")):
        refused_td(actor._a, critic._q, copy_of(good, gamma=gamma), f"gamma {gamma}", b"gamma")
    # actors that do not fit: never loaded, other widths, feature blocks
    index = (C.c_int32 * 12)(*range(12))
    adesc = nat.MjsActorDesc(device=0, in_dim=D, n_hidden=1, hidden=(C.c_int32 * 3)(32, 0, 0), action_dim=A, activation=nat.ACTIVATION_RELU, obs_index=index)
    made = []

    def native_actor(desc, blocks=None):
        a = C.c_void_p()
        rc = L.mjs_actor_create_visual(C.byref(desc), C.byref(blocks), C.byref(a)) if blocks is not None else L.mjs_actor_create(C.byref(desc), C.byref(a))
        assert rc == 0 and a.value
        made.append(a)
        return a

    def loaded(a, in_dim, n_out):
        """mjs_actor_load with zero parameters of the right shapes."""
        hw, hb = torch.zeros(32, in_dim, device=DEV), torch.zeros(32, device=DEV)
        ow, ob = torch.zeros(n_out, 32, device=DEV), torch.zeros(n_out, device=DEV)
        wts = nat.MjsActorWeights(hidden_w=(C.c_void_p * 3)(hw.data_ptr()), hidden_b=(C.c_void_p * 3)(hb.data_ptr()), mu_w=ow.data_ptr(), mu_b=ob.data_ptr(),
                                  log_std_w=ow.data_ptr(), log_std_b=ob.data_ptr())
        assert L.mjs_actor_load(a, C.byref(wts), stream) == 0
        torch.cuda.synchronize()  # the pack kernels read the temporaries
        return a

    refused_td(native_actor(adesc), critic._q, good, "an actor that was never loaded", b"mjs_actor_load")
    refused_td(loaded(native_actor(copy_of(adesc, in_dim=D - 1)), D - 1, A), critic._q, good, "in_dim != obs_dim", b"in_dim")
    refused_td(loaded(native_actor(copy_of(adesc, action_dim=A + 1)), D, A + 1), critic._q, good, "action_dim differs", b"action_dim")
    blocks = nat.MjsActorFeatureInputs(n_blocks=1, width=(C.c_int32 * 2)(4, 0), start=(C.c_int32 * 2)(D - 4, 0))
    refused_td(loaded(native_actor(copy_of(adesc, in_dim=D - 4), blocks), D, A), critic._q, good, "a visual actor", b"feature blocks")
    if torch.cuda.device_count() > 1:  # (a second device is needed to make an object there)
        other = C.c_void_p()
        assert L.mjs_critic_create(C.byref(copy_of(good_desc, device=1)), C.byref(other)) == 0
        refused_td(actor._a, other, good, "another device", b"another device")
        L.mjs_critic_destroy(other)
    # ... and the arguments as they stand are fine: B == 0 launches nothing, B rows are written
    assert L.mjs_sac_td_target(actor._a, critic._q, C.byref(copy_of(good, B=0)), stream) == 0 and untouched()
    assert L.mjs_sac_td_target(actor._a, critic._q, C.byref(good), stream) == 0
    torch.cuda.synchronize()
    assert not bool((target == fill).any()) and not bool((q_out == fill).any())
    assert L.mjs_critic_load(h, C.byref(w), 1.0, stream) == 0 and L.mjs_critic_load(h, C.byref(w), 0.5, stream) == 0  # after a first load tau < 1 is taken
    torch.cuda.synchronize()
    for a in made:
        L.mjs_actor_destroy(a)
    L.mjs_critic_destroy(h)
    actor.close()
    critic.close()
