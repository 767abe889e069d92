"""The gradient loop on the device (csrc/mjs_sac_train.h, mjs_sac_draw_batch, mjs_sac_train, DeviceSAC): the fused batch draw against the
numpy restatement of its counter layout (bit for bit) and of its Box-Muller lines (4 x the float32 restatement's own error), the native
loop against the same steps written by hand in Python (bit for bit), one step against SB3's SAC.train in torch (the project's bar), a
regression it must learn, every native refusal, and learn end to end on an env.
"""
import ctypes as C
import functools
import types

import numpy as np
import pytest
import torch

import _actor_train_reference as aref
import _critic_reference as ref
import _critic_train_reference as tref
import _sac_train_reference as sref

gpu = pytest.mark.gpu
DEV = "cuda:0"
CAPACITY = 128
BIG_SEED, BIG_STEP = 2**63 + 12345, 2**32 + 3
# (widths, activation, n_critics, D, A) in aref's case layout, for make_nets / sac_train_torch
CASE_64 = ([64, 64], [64, 64], "relu", "relu", 2, 17, 12, 3, "")
CASE_TANH = ([40, 24], [40, 24], "tanh", "tanh", 1, 300, 12, 3, "")


def make_nets(case, device="cpu"):
    """(actor modules (hidden, mu, log_std), q_nets) of a case from fixed seeds: the same parameters on every call."""
    aw, cw, _, _, n, _, D, A, _ = case
    return ref.make_actor(D, aw, A, seed=501 + len(aw) * 7 + aw[0], device=device), ref.make_q_nets(D, A, cw, n, seed=502 + cw[0], device=device)


def shape_env(D, A, N=4):
    """What DeviceActor, DeviceReplayBuffer and DeviceSAC read of an env when no step is taken."""
    return types.SimpleNamespace(device=DEV, action_dim=A, obs_dim=D, num_envs=N, _dev_index=0, autoreset="next_step", flat_observation_layout=[("obs", 0, D)])


def block_of(rows, D, A, seed):
    """CPU tensors of a [1, rows] block and its first observation: what add_block takes, every row a transition (step_type MID)."""
    g = torch.Generator().manual_seed(seed)
    obs0 = torch.randn(rows, D, generator=g, dtype=torch.float64)
    return obs0, {"obs": torch.randn(1, rows, D, generator=g, dtype=torch.float64), "reward": torch.randn(1, rows, generator=g, dtype=torch.float64),
                  "terminated": (torch.arange(rows) % 3 == 1).to(torch.uint8)[None], "truncated": torch.zeros(1, rows, dtype=torch.uint8),
                  "step_type": torch.ones(1, rows, dtype=torch.uint8), "squashed_actions": torch.tanh(torch.randn(1, rows, A, generator=g))}


FILLS = {"empty": (), "five": (5,), "full": (CAPACITY,), "wrapped": (CAPACITY, 40)}


def filled_buffer(D, A, fill, seed=0, blocks=None):
    from mujoco_sim_amd import DeviceReplayBuffer

    buf = DeviceReplayBuffer(shape_env(D, A), CAPACITY, obs_index=list(range(D)))
    for k, rows in enumerate(FILLS[fill]):
        obs0, block = blocks[k] if blocks is not None else block_of(rows, D, A, seed + k)
        buf.add_block(obs0.to(DEV), {key: v.to(DEV) for key, v in block.items()})
    return buf


def native_draw(buf, B, seed, step, pad=0, fill=-7.0):
    """mjs_sac_draw_batch through ctypes into buffers of the test's own: z_next / z_pi with ``pad`` extra floats behind their B A."""
    from mujoco_sim_amd import _native as nat

    D, A = buf.obs_dim, buf.action_dim
    f32 = lambda *s: torch.full(s, fill, dtype=torch.float32, device=DEV)  # noqa: E731
    out = {"obs": f32(B, D), "next_obs": f32(B, D), "actions": f32(B, A), "rewards": f32(B), "dones": f32(B),
           "indices": torch.full((B,), -9, dtype=torch.int64, device=DEV), "draws": torch.full((B,), -9, dtype=torch.int64, device=DEV),
           "z_next_flat": f32(B * A + pad), "z_pi_flat": f32(B * A + pad)}
    batch = nat.MjsSacBatch(idx_out=out["indices"].data_ptr(), draws_out=out["draws"].data_ptr(), obs=out["obs"].data_ptr(), next_obs=out["next_obs"].data_ptr(),
                            actions=out["actions"].data_ptr(), rewards=out["rewards"].data_ptr(), dones=out["dones"].data_ptr(),
                            z_next=out["z_next_flat"].data_ptr(), z_pi=out["z_pi_flat"].data_ptr())
    stream = C.c_void_p(torch.cuda.current_stream(torch.device(DEV)).cuda_stream)
    nat.check(nat.lib().mjs_sac_draw_batch(C.byref(buf._storage), C.byref(batch), B, seed, step, stream))
    out["z_next"], out["z_pi"] = out["z_next_flat"][:B * A].view(B, A), out["z_pi_flat"][:B * A].view(B, A)
    return out


# every B, A, D, fill, seed and step the issue names, each at least once; the ragged and the multi-workgroup B with every fill
DRAW_CASES = [(1, 1, 1, "five", 0, 0), (17, 3, 12, "full", BIG_SEED, 7), (64, 8, 33, "wrapped", 0, BIG_STEP), (300, 3, 12, "wrapped", BIG_SEED, BIG_STEP),
              (300, 8, 1, "five", 0, 7), (17, 1, 33, "empty", BIG_SEED, 0), (64, 3, 12, "empty", 0, BIG_STEP), (300, 1, 12, "full", 0, 0), (1, 8, 12, "wrapped", BIG_SEED, 7)]


# ------------------------------------------------------------------------- 1. draws, bit for bit
@gpu
@pytest.mark.parametrize("B,A,D,fill,seed,step", DRAW_CASES, ids=[f"B{c[0]}-A{c[1]}-D{c[2]}-{c[3]}-seed{c[4] % 1000}-step{c[5] % 1000}" for c in DRAW_CASES])
def test_draws_and_gather_bit_for_bit(B, A, D, fill, seed, step):
    buf = filled_buffer(D, A, fill, seed=40)
    size = min(sum(FILLS[fill]), CAPACITY)
    got = native_draw(buf, B, seed, step)
    want = sref.draws(B, step, seed)
    assert np.array_equal(got["draws"].cpu().numpy(), want)
    assert np.array_equal(got["indices"].cpu().numpy(), sref.indices(want, size))
    sampled = buf.sample(B, draws=got["draws"])
    for key in ("obs", "next_obs", "actions", "rewards", "dones", "indices"):
        assert torch.equal(got[key], sampled[key]), key
    if size == 0:
        assert bool((got["indices"] == -1).all()) and not any(bool(got[k].any()) for k in ("obs", "next_obs", "actions", "rewards", "dones"))
    else:
        assert bool(got["obs"].any()) or D * B < 4
    again = native_draw(buf, B, seed, step)
    assert all(torch.equal(got[k], again[k]) for k in got)
    if B >= 17:
        assert not torch.equal(got["draws"], native_draw(buf, B, seed, step + 1)["draws"]) and not torch.equal(got["draws"], native_draw(buf, B, seed ^ 1, step)["draws"])
        assert not torch.equal(got["z_pi"], native_draw(buf, B, seed, step + 1)["z_pi"]) and not torch.equal(got["z_next"], got["z_pi"])
    buf.close()


# ------------------------------------------------------------------------- 2. normals
@gpu
@pytest.mark.parametrize("B,A,D,fill,seed,step", DRAW_CASES[:5] + DRAW_CASES[7:], ids=[f"B{c[0]}-A{c[1]}-seed{c[4] % 1000}-step{c[5] % 1000}" for c in DRAW_CASES[:5] + DRAW_CASES[7:]])
def test_normals_follow_the_box_muller_lines(B, A, D, fill, seed, step):
    """Allowed max |device - float64| = 4 x max |numpy float32 restatement - float64 restatement| on the same bits (the yardstick is the
    reference's own error; the 4 covers device logf / sinf / cosf at a few ulp where numpy's are about one)."""
    buf = filled_buffer(D, A, fill, seed=40)
    PAD = 37
    got = native_draw(buf, B, seed, step, pad=PAD)
    for which in ("z_next", "z_pi"):
        z = got[which].cpu().numpy()
        a, b = sref.normal_words(B, A, step, seed, which)
        z64, z32 = sref.box_muller(a, b, np.float64), sref.box_muller(a, b, np.float32)
        e32 = np.abs(z32.astype(np.float64) - z64).max()
        err = np.abs(z.astype(np.float64) - z64).max()
        print(f"{which} B{B} A{A}: device vs float64 {err:.3e}, numpy float32 vs float64 {e32:.3e}, ratio {err / max(e32, 1e-300):.2f} (allowed 4)")
        assert z.dtype == np.float32 and np.isfinite(z).all()
        assert err <= 4 * e32, (which, err, e32)
        assert bool((got[which + "_flat"][B * A:] == -7.0).all())  # nothing behind the B A components is written
    buf.close()


@gpu
def test_normals_over_many_rows_report_their_error():
    """4096 rows x 8 components, both samples: the same bar on 65 536 values, and the figure profiles/sac_train_timing.txt records."""
    buf = filled_buffer(12, 8, "full", seed=40)
    got = native_draw(buf, 4096, 2025, 11)
    for which in ("z_next", "z_pi"):
        a, b = sref.normal_words(4096, 8, 11, 2025, which)
        z64, z32 = sref.box_muller(a, b, np.float64), sref.box_muller(a, b, np.float32)
        e32, err = np.abs(z32.astype(np.float64) - z64).max(), np.abs(got[which].cpu().numpy().astype(np.float64) - z64).max()
        print(f"{which} 4096 x 8: device vs float64 {err:.3e}, numpy float32 vs float64 {e32:.3e}, ratio {err / e32:.2f} (allowed 4)")
        assert err <= 4 * e32, (which, err, e32)
    buf.close()


# ------------------------------------------------------------------------- 3. the native loop, bit for bit
def make_trainer(case, fill="full", blocks=None, **kw):
    """(trainer, actor, critic): fresh modules from the case's seed, a buffer with the given blocks, everything on the device."""
    import mujoco_sim_amd as m

    D, A = case[6], case[7]
    actor_net, q_nets = make_nets(case, device=DEV)
    actor = m.DeviceActor.from_linears(shape_env(D, A), *actor_net, activation=case[2], obs_index=list(range(D)))
    critic = m.DeviceCritic.from_linears(DEV, D, A, q_nets, activation=case[3])
    buf = filled_buffer(D, A, fill, seed=70, blocks=blocks)
    return m.DeviceSAC(shape_env(D, A), actor, critic, buffer=buf, **kw), actor, critic


def parameters(trainer, case):
    """Every exported tensor of the actor, the critic and the target critic, and the coefficient's scalars, as clones."""
    actor_net, q_nets = make_nets(case, device=DEV)
    trainer.actor.export(actor_net)
    out = [t.detach().clone() for m_ in (*actor_net[0], *actor_net[1:]) for t in (m_.weight, m_.bias)]
    for critic in (trainer.critic, trainer.target_critic):
        critic.export(q_nets)
        out += [t.detach().clone() for net in q_nets for m_ in net for t in (m_.weight, m_.bias)]
    if trainer.coef is not None:
        out += [trainer.coef.log_ent_coef.clone(), trainer.coef.ent_coef.clone()]
    return out


def target_parameters(trainer, case):
    q_nets = make_nets(case, device=DEV)[1]
    trainer.target_critic.export(q_nets)
    return [t.detach().clone() for net in q_nets for m_ in net for t in (m_.weight, m_.bias)]


def same(a, b):
    return len(a) == len(b) and all(torch.equal(x, y) for x, y in zip(a, b))


def close_trainer(t):
    buf, actor, critic = t.buffer, t.actor, t.critic
    t.close()
    critic.close()
    actor.close()
    buf.close()


@gpu
@pytest.mark.parametrize("case,kw", [(CASE_64, dict(batch_size=17, ent_coef="auto")), (CASE_TANH, dict(batch_size=300, ent_coef=0.2, target_update_interval=2))],
                         ids=["64x64-relu-2c-auto-B17", "40x24-tanh-1c-fixed-B300-interval2"])
def test_native_loop_equals_the_steps_written_by_hand(case, kw):
    import mujoco_sim_amd as m

    kw = dict(kw, seed=BIG_SEED, gamma=0.99, tau=0.05, learning_rate=1e-3)
    interval = kw.get("target_update_interval", 1)
    native, _, _ = make_trainer(case, "wrapped", **kw)
    hand, actor, critic = make_trainer(case, "wrapped", **kw)
    assert same(parameters(native, case), parameters(hand, case))
    start = parameters(native, case)
    native.train(3)
    assert (native.num_gradient_steps, native.critic_opt.step_count, native.actor_opt.step_count) == (3, 3, 3)
    assert native.coef is None or native.coef.step_count == 3

    def by_hand(t, step):
        b = t.draw_batch(step)
        if interval == 1:
            m.sac_gradient_step(b, t.actor, t.critic, t.target_critic, t.critic_opt, t.actor_opt, t.ent_coef, t.gamma, t.tau, z_next=b["z_next"], z_pi=b["z_pi"])
        else:
            alpha = t.coef.ent_coef if t.coef is not None else t.ent_coef_fixed
            y = m.sac_td_target(b, t.actor, t.target_critic, t.gamma, alpha, z=b["z_next"])
            t.critic_opt.step(b, y)
            t.actor_opt.step(b, t.critic, t.ent_coef, z=b["z_pi"])
            if (step + 1) % interval == 0:
                t.target_critic.blend_from(t.critic, t.tau)

    targets = [target_parameters(hand, case)]
    for step in range(3):
        by_hand(hand, step)
        targets.append(target_parameters(hand, case))
    if interval == 2:  # the target moved after step 2 only
        assert same(targets[0], targets[1]) and not same(targets[1], targets[2]) and same(targets[2], targets[3])
    else:
        assert not same(targets[0], targets[1]) and not same(targets[1], targets[2]) and not same(targets[2], targets[3])
    got, want = parameters(native, case), parameters(hand, case)
    assert same(got, want), [i for i, (x, y) in enumerate(zip(got, want)) if not torch.equal(x, y)]
    assert not any(torch.equal(x, y) for x, y in zip(got[:4], start[:4]))  # and they did move
    # the step counts were carried: one more hand-written step on both sides still agrees (the native side draws its own counter's batch)
    assert torch.equal(native.draw_batch()["draws"], hand.draw_batch(3)["draws"])
    by_hand(native, native.num_gradient_steps)
    by_hand(hand, 3)
    assert same(parameters(native, case), parameters(hand, case))
    # ... and so does a native step after the hand-written one, once the trainers' own counters say 4
    native.num_gradient_steps = hand.num_gradient_steps = 4
    native.train(1)
    hand.train(1)
    assert same(parameters(native, case), parameters(hand, case))
    close_trainer(native)
    close_trainer(hand)
    del actor, critic


# ------------------------------------------------------------------------- 4. against torch
@gpu
def test_one_native_step_matches_sac_train_in_torch():
    """train(1) at [64, 64], B = 64 against tests/_actor_train_reference.py's SAC.train restatement, fed the kernel's own batch and draws;
    the bar is the one test_actor_train_device.py holds sac_gradient_step to (ref.within_bar through check_params)."""
    case = CASE_64
    gamma, tau = 0.99, 0.005
    t, _, _ = make_trainer(case, "full", batch_size=64, seed=5, gamma=gamma, tau=tau)
    b = {k: v.cpu() for k, v in t.draw_batch(0).items()}
    t.train(1)
    actor_cpu, q_cpu = make_nets(case)
    A = case[7]
    n_actor = 2 * (len(case[0]) + 2)
    got = parameters(t, case)
    n_q = (len(got) - 2 - n_actor) // 2
    pairs = lambda ts: [(ts[i], ts[i + 1]) for i in range(0, len(ts), 2)]  # noqa: E731
    per_net = lambda ts: [pairs(ts)[i:i + len(case[1]) + 1] for i in range(0, len(ts) // 2, len(case[1]) + 1)]  # noqa: E731
    refs = [aref.sac_train_torch(actor_cpu, q_cpu, q_cpu, [b], [(b["z_next"], b["z_pi"])], case, gamma, tau, dtype) for dtype in (torch.float64, torch.float32)]
    aref.check_params("actor", pairs(got[:n_actor]), refs[0][0], refs[1][0])
    tref.check_params("critic", per_net(got[n_actor:n_actor + n_q]), refs[0][1], refs[1][1])
    tref.check_params("target critic", per_net(got[n_actor + n_q:n_actor + 2 * n_q]), refs[0][2], refs[1][2])
    ref.within_bar("log_ent_coef", got[-2].cpu(), refs[0][3], refs[1][3])
    assert A == 3
    close_trainer(t)


# ------------------------------------------------------------------------- 5. it learns something
LEARN_SEED, LEARN_STEPS, LEARN_B, LEARN_LR = 9, 200, 64, 3e-4  # SB3's default learning rate


@functools.lru_cache(maxsize=None)
def learn_blocks():
    """128 rows whose reward is a linear function of the observation and the action: with gamma = 0 the critic update is a regression on it."""
    D, A = CASE_64[6], CASE_64[7]
    obs0, block = block_of(CAPACITY, D, A, seed=123)
    g = torch.Generator().manual_seed(124)
    w, v = torch.randn(D, generator=g, dtype=torch.float64) * 0.3, torch.randn(A, generator=g, dtype=torch.float64) * 0.5
    block["reward"] = (obs0 @ w + block["squashed_actions"][0].double() @ v)[None]
    block["terminated"] = torch.zeros(1, CAPACITY, dtype=torch.uint8)
    return obs0, block


def learn_rows():
    """The ring's content as CPU float32 tensors (add_block's rounding): obs, next_obs, actions, rewards, dones."""
    obs0, block = learn_blocks()
    return {"obs": obs0.float(), "next_obs": block["obs"][0].float(), "actions": block["squashed_actions"][0], "rewards": block["reward"][0].float(),
            "dones": torch.zeros(CAPACITY)}


def regression_loss(q_params, rows, activation):
    q = tref._forward(q_params, rows["obs"].to(q_params[0][0][0].dtype), rows["actions"].to(q_params[0][0][0].dtype), activation)
    return ((q - rows["rewards"].to(q.dtype)) ** 2).mean(dim=1)


@functools.lru_cache(maxsize=None)
def learn_reference(lr=LEARN_LR):
    """(loss before, loss after) per critic of the torch float32 restatement of SAC.train on the same rows, with the batches and draws the
    numpy restatement of the generator names: the CPU side of the condition the device test asserts."""
    case, rows = CASE_64, learn_rows()
    A = case[7]
    actor_cpu, q_cpu = make_nets(case)
    batches, draws = [], []
    for g in range(LEARN_STEPS):
        idx = torch.from_numpy(sref.indices(sref.draws(LEARN_B, g, LEARN_SEED), CAPACITY))
        batches.append({k: v[idx] for k, v in rows.items()})
        draws.append(tuple(torch.from_numpy(sref.normals(LEARN_B, A, g, LEARN_SEED, which)) for which in ("z_next", "z_pi")))
    before = regression_loss(aref.critic_params(q_cpu, torch.float32), rows, case[3])
    trained = aref.sac_train_torch(actor_cpu, q_cpu, q_cpu, batches, draws, case, 0.0, 0.005, torch.float32, lr=lr)
    return before, regression_loss(trained[1], rows, case[3])


@gpu
def test_the_loop_learns_a_regression():
    from mujoco_sim_amd import DeviceCriticOptimizer

    before_ref, after_ref = learn_reference()
    print(f"torch float32 restatement: critic loss {before_ref.tolist()} -> {after_ref.tolist()}")
    assert bool((after_ref < 0.25 * before_ref).all())  # the restatement meets the condition with room to spare
    t, _, critic = make_trainer(CASE_64, "full", blocks=[learn_blocks()], batch_size=LEARN_B, seed=LEARN_SEED, gamma=0.0, learning_rate=LEARN_LR)
    rows = {k: v.to(DEV) for k, v in learn_rows().items()}
    probe = DeviceCriticOptimizer(critic)  # reads the loss on the fixed batch of all 128 rows; it never steps
    before = probe.gradients(rows, rows["rewards"])["loss"].cpu()
    assert torch.allclose(before, before_ref, rtol=1e-4, atol=1e-6)
    t.train(LEARN_STEPS)
    after = probe.gradients(rows, rows["rewards"])["loss"].cpu()
    print(f"device: critic loss {before.tolist()} -> {after.tolist()}")
    assert bool((after < 0.5 * before).all()), (before, after)
    probe.close()
    close_trainer(t)


# ------------------------------------------------------------------------- 6. native refusals
def copy_of(struct, **changes):
    c = type(struct)()
    C.memmove(C.byref(c), C.byref(struct), C.sizeof(struct))
    for k, v in changes.items():
        setattr(c, k, v)
    return c


@gpu
def test_native_refusals():
    """Every MJS_ERR_INVALID_ARG of mjs_sac_train and mjs_sac_draw_batch through ctypes: the return code, the entry point's name and a piece
    of the text that no earlier refusal shares, nothing launched (the scratch keeps its fill, the parameters and the coefficient their bits)."""
    import mujoco_sim_amd as m
    from mujoco_sim_amd import _native as nat

    L = nat.lib()
    case = CASE_64
    D, A, B = case[6], case[7], 17
    t, actor, critic = make_trainer(case, "full", batch_size=B, seed=3)
    other, other_actor, other_critic = make_trainer(case, "five", batch_size=B, seed=3)
    stream = C.c_void_p(torch.cuda.current_stream(torch.device(DEV)).cuda_stream)
    args = t._train_args(2, B)
    scratch = t._scratch[1]
    for v in scratch.values():
        v.fill_(-7)
    params = parameters(t, case)

    def untouched():
        return all(bool((v == -7).all()) for v in scratch.values()) and same(params, parameters(t, case))

    def refused(rc, name, what, text):
        err = L.mjs_last_error(None)
        assert rc == -1 and err.startswith(name.encode() + b": ") and text.encode() in err[len(name) + 2:], (what, text, rc, err)
        assert untouched(), what

    ptr = lambda s: C.pointer(s)  # noqa: E731
    cams = copy_of(t.buffer._storage, n_cameras=1, height=8, width=8)
    cams.rgb[0] = cams.next_rgb[0] = scratch["obs"].data_ptr()
    wide = m.DeviceCritic.from_linears(DEV, D + 1, A, ref.make_q_nets(D + 1, A, [64, 64], 2, seed=5, device=DEV))
    more = m.DeviceCritic.from_linears(DEV, D, A + 1, ref.make_q_nets(D, A + 1, [64, 64], 2, seed=5, device=DEV))
    slim = m.DeviceCritic.from_linears(DEV, D, A, ref.make_q_nets(D, A, [64], 2, seed=5, device=DEV))
    batch, block = args.batch.contents, args.entropy.contents
    cases = [
        ("struct_size", copy_of(args, struct_size=144), "mjs_sac_train_args.struct_size"),
        *[(f"null {f}", copy_of(args, **{f: None}), "batch or target_dev is null") for f in ("storage", "actor", "critic", "target_critic", "critic_opt", "actor_opt", "batch", "target_dev")],
        ("B = 0", copy_of(args, B=0), "B must be at least 1"), ("G < 0", copy_of(args, G=-1), "G is negative"),
        ("interval = 0", copy_of(args, target_update_interval=0), "target_update_interval"),
        ("storage struct_size", copy_of(args, storage=ptr(copy_of(t.buffer._storage, struct_size=112))), "mjs_replay_storage.struct_size"),
        ("storage without cursor", copy_of(args, storage=ptr(copy_of(t.buffer._storage, cursor_dev=None))), "cursor_dev is null"),
        ("cameras", copy_of(args, storage=ptr(cams)), "state-only"),
        ("batch struct_size", copy_of(args, batch=ptr(copy_of(batch, struct_size=72))), "mjs_sac_batch.struct_size"),
        ("batch without idx", copy_of(args, batch=ptr(copy_of(batch, idx_out=None))), "idx_out, actions, rewards or dones"),
        ("batch without obs", copy_of(args, batch=ptr(copy_of(batch, next_obs=None))), "obs or next_obs is null"),
        ("batch without z", copy_of(args, batch=ptr(copy_of(batch, z_pi=None))), "z_next or z_pi is null"),
        ("storage obs_dim", copy_of(args, storage=ptr(copy_of(t.buffer._storage, obs_dim=D - 1))), "obs_dim is not the networks'"),
        ("critic obs_dim", copy_of(args, critic=wide._q), "obs_dim is not the networks'"),
        ("storage action_dim", copy_of(args, storage=ptr(copy_of(t.buffer._storage, action_dim=A - 1))), "action_dim is not the networks'"),
        ("critic action_dim", copy_of(args, critic=more._q), "action_dim is not the networks'"),
        ("another critic's optimiser", copy_of(args, critic_opt=other.critic_opt._o), "critic_opt was created for another critic"),
        ("another actor's optimiser", copy_of(args, actor_opt=other.actor_opt._o), "actor_opt was created for another actor"),
        ("target is the critic", copy_of(args, target_critic=critic._q), "one object"),
        ("tau = 0", copy_of(args, tau=0.0), "tau must lie"), ("tau > 1", copy_of(args, tau=1.5), "tau must lie"), ("tau nan", copy_of(args, tau=float("nan")), "tau must lie"),
        ("gamma < 0", copy_of(args, gamma=-0.1), "gamma must lie"), ("gamma > 1", copy_of(args, gamma=1.1), "gamma must lie"),
        ("critic_lr < 0", copy_of(args, critic_lr=-1e-3), "critic_lr and actor_lr"), ("actor_lr nan", copy_of(args, actor_lr=float("nan")), "critic_lr and actor_lr"),
        # what the underlying entry points refuse, named by them
        ("target of another shape", copy_of(args, target_critic=slim._q), "mjs_critic_blend: the two critics differ in shape"),
        ("entropy struct_size", copy_of(args, entropy=ptr(copy_of(block, struct_size=80))), "mjs_actor_update: mjs_entropy_step.struct_size"),
        ("entropy null m", copy_of(args, entropy=ptr(copy_of(block, m_dev=None))), "mjs_actor_update: entropy: log_ent_coef_dev"),
        ("entropy t = 0", copy_of(args, entropy=ptr(copy_of(block, t=0))), "mjs_actor_update: entropy: t"),
        ("entropy lr < 0", copy_of(args, entropy=ptr(copy_of(block, lr=-1.0))), "mjs_actor_update: entropy: lr"),
        ("entropy eps = 0", copy_of(args, entropy=ptr(copy_of(block, eps=0.0))), "mjs_actor_update: entropy: eps"),
    ]
    for what, a, text in cases:
        refused(L.mjs_sac_train(C.byref(a), stream), "mjs_sac_train", what, text)
    refused(L.mjs_sac_train(None, stream), "mjs_sac_train", "null args", "args is null")
    # never-loaded networks: only their entry points' own checks stand between them and the launch
    desc = nat.MjsCriticDesc(device=0, obs_dim=D, action_dim=A, n_critics=2, n_hidden=2, hidden=(C.c_int32 * 3)(64, 64, 0), activation=nat.ACTIVATION_RELU)
    unloaded = C.c_void_p()
    assert L.mjs_critic_create(C.byref(desc), C.byref(unloaded)) == 0
    refused(L.mjs_sac_train(C.byref(copy_of(args, target_critic=unloaded)), stream), "mjs_sac_train", "target never loaded", "mjs_sac_td_target: the critic has no parameters yet")
    L.mjs_critic_destroy(unloaded)
    if torch.cuda.device_count() > 1:
        far = copy_of(t.buffer._storage, device=1)
        refused(L.mjs_sac_train(C.byref(copy_of(args, storage=ptr(far))), stream), "mjs_sac_train", "another device", "different devices")
    # G == 0 does nothing
    assert L.mjs_sac_train(C.byref(copy_of(args, G=0)), stream) == 0 and untouched()

    # mjs_sac_draw_batch
    st = t.buffer._storage
    for what, s, b, n, text in [("null storage", None, batch, B, "storage is null"), ("null batch", st, None, B, "mjs_sac_batch) is null"),
                                ("storage struct_size", copy_of(st, struct_size=112), batch, B, "mjs_replay_storage.struct_size"),
                                ("cameras", cams, batch, B, "state-only"), ("batch struct_size", st, copy_of(batch, struct_size=72), B, "mjs_sac_batch.struct_size"),
                                ("B < 0", st, batch, -1, "B is negative"), ("null actions", st, copy_of(batch, actions=None), B, "idx_out, actions, rewards or dones"),
                                ("null z_next", st, copy_of(batch, z_next=None), B, "z_next or z_pi is null")]:
        rc = L.mjs_sac_draw_batch(C.byref(s) if s is not None else None, C.byref(b) if b is not None else None, n, 0, 0, stream)
        refused(rc, "mjs_sac_draw_batch", what, text)
    assert L.mjs_sac_draw_batch(C.byref(st), C.byref(copy_of(batch, z_pi=None)), 0, 0, 0, stream) == 0 and untouched()  # B == 0 does nothing
    # draws_out is optional, and the good calls go through
    assert L.mjs_sac_draw_batch(C.byref(st), C.byref(copy_of(batch, draws_out=None)), B, 3, 0, stream) == 0
    torch.cuda.synchronize()
    assert bool((scratch["draws"] == -7).all()) and not bool((scratch["indices"] == -7).any())
    assert L.mjs_sac_train(C.byref(args), stream) == 0
    torch.cuda.synchronize()
    assert not same(params, parameters(t, case)) and t.critic_opt.step_count == 0  # (the native counts moved; the test bypassed train's bookkeeping)
    for q in (wide, more, slim):
        q.close()
    close_trainer(t)
    close_trainer(other)
    del actor, other_actor, other_critic


# ------------------------------------------------------------------------- 7. learn, end to end
def point_mass_trainer():
    import mujoco_sim_amd as m

    venv = m.HipVectorEnv("point_mass_reach", 64, seed=7)
    venv.reset(seed=3)
    D, A = int(venv.obs_dim), int(venv.action_dim)
    net = ref.make_actor(D, [64, 64], A, seed=81, device=DEV)
    q_nets = ref.make_q_nets(D, A, [64, 64], 2, seed=82, device=DEV)
    actor = m.DeviceActor.from_linears(venv, *net)
    critic = m.DeviceCritic.from_linears(DEV, D, A, q_nets)
    t = m.DeviceSAC(venv, actor, critic, buffer_size=4096, learning_starts=256, train_freq=4, gradient_steps=2, batch_size=32, seed=11)
    return t, venv, net, q_nets


def learned_tensors(t, net, q_nets):
    t.actor.export(net)
    t.critic.export(q_nets)
    out = [p.detach().clone() for m_ in (*net[0], *net[1:]) for p in (m_.weight, m_.bias)] + [p.detach().clone() for q in q_nets for m_ in q for p in (m_.weight, m_.bias)]
    t.target_critic.export(q_nets)
    return out + [p.detach().clone() for q in q_nets for m_ in q for p in (m_.weight, m_.bias)] + [t.coef.log_ent_coef.clone()]


@gpu
def test_learn_end_to_end():
    runs = []
    for _ in range(2):
        t, venv, net, q_nets = point_mass_trainer()
        start = learned_tensors(t, net, q_nets)
        g = torch.Generator(device=DEV).manual_seed(21)
        assert t.learn(1024, generator=g) is t
        # 4 steps x 64 envs = 256 env steps per block: one uniform block, then three of the actor's, each followed by 2 gradient steps
        assert t.num_timesteps == 1024 and t.num_gradient_steps == 6 and (t.critic_opt.step_count, t.actor_opt.step_count, t.coef.step_count) == (6, 6, 6)
        size = t.buffer.size
        assert 0 < size <= 1024
        end = learned_tensors(t, net, q_nets)
        assert all(bool(torch.isfinite(x).all()) for x in end) and not any(torch.equal(a, b) for a, b in zip(start, end))
        runs.append(end)
        actor, critic = t.actor, t.critic
        t.close()
        critic.close()
        actor.close()
        venv.close()
    assert same(*runs)
