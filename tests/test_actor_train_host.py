"""The actor update's host side, without a GPU: the C ABI (declared, exported, struct sizes as stated), the argument checks of
DeviceActorOptimizer, DeviceActor.export, DeviceEntropyCoef and sac_gradient_step, which raise ValueError before the native layer is
touched, the workspace-size rule, and the checks of the device tests' seeds: the argmin margin, the distance of log_std from the clamp's
edges, and a float32 evaluation with the kernel's summation shape inside the bar."""
import ctypes as C
import re
from pathlib import Path

import numpy as np
import pytest
import torch

import _actor_train_reference as aref
import _critic_reference as ref
import _critic_train_reference as tref

ROOT = Path(__file__).resolve().parents[1]
CASE_IDS = [aref.case_id(c) for c in aref.CASES]


class _TouchedLib:
    def __getattr__(self, name):
        raise AssertionError("the native layer was touched")


def _stub(cls, **attrs):
    """An object of a native-backed class without its constructor: what the argument checks read, and a library that raises."""
    obj = cls.__new__(cls)
    obj.__dict__.update(_lib=_TouchedLib(), device=torch.device("cpu"), **attrs)
    return obj


ENTRY_POINTS = (("mjs_actor_opt_create", "int"), ("mjs_actor_opt_destroy", "void"), ("mjs_actor_train_workspace_bytes", "uint64_t"),
                ("mjs_actor_grad", "int"), ("mjs_actor_update", "int"), ("mjs_actor_export", "int"))


def test_header_declares_and_library_exports_the_entry_points():
    from mujoco_sim_amd import _native

    header = (ROOT / "include" / "mjsim.h").read_text()
    for name, ret in ENTRY_POINTS:
        assert re.search(rf"^{ret} {name}\(", header, re.M), name
        assert name in _native.EXPORTED_SYMBOLS
    assert re.search(r"^#define MJS_ABI_VERSION 3$", header, re.M)  # entry points added after abi 3: the number stays
    assert "typedef struct mjs_actor_opt mjs_actor_opt;" in header
    _native.build()
    L = C.CDLL(str(_native.LIB_PATH))
    for name, _ in ENTRY_POINTS:
        assert hasattr(L, name), f"libmjsim.so does not export {name}"


def test_struct_sizes_stated_in_the_header_are_the_bindings():
    from mujoco_sim_amd import _native as nat

    header = (ROOT / "include" / "mjsim.h").read_text()
    for name, binding, size in (("mjs_actor_opt_desc", nat.MjsActorOptDesc, 40), ("mjs_entropy_step", nat.MjsEntropyStep, 88),
                                ("mjs_actor_grad_args", nat.MjsActorGradArgs, 104)):
        stated = re.search(rf"\}} {name};\s*/\* (\d+) bytes \*/", header)
        assert stated, name
        assert int(stated.group(1)) == C.sizeof(binding) == size, name
        assert binding().struct_size == C.sizeof(binding)
        body = header[header.rindex("typedef struct {", 0, stated.start()):stated.start()]
        declared = re.findall(r"^\s+(?:const )?\w+\s*\**\s*(\w+)(?:\[\d+\])*;", body, re.M)
        assert declared == [n for n, _ in binding._fields_], name  # the same fields in the same order


def test_kernel_header_states_its_plan():
    text = (ROOT / "mujoco_sim_amd" / "csrc" / "mjs_actor_train.h").read_text()
    assert '#include "mjs_critic_train.h"' in text and "crit::squashed_sample" in text
    for reused in ("crit::weight_grad", "crit::input_grad", "crit::fill_input", "crit::slab_sum"):
        assert reused in text, reused
    assert "atomic" not in text.replace("no atomics", "").replace("No atomics", "") and "asm" not in text.replace("inline assembly", "")
    # td_target_kernel and the new kernel share the per-component sample
    assert "squashed_sample(mu, ls, zj, gauss, corr)" in (ROOT / "mujoco_sim_amd" / "csrc" / "mjs_critic.h").read_text()


def test_workspace_rule_is_the_critics_with_one_network_over_the_actor_slab():
    assert aref.actor_slab_floats([64, 64], 12) == 16 * 64 + 64 + 64 * 64 + 64 + 64 * 32 + 32 + 4
    assert aref.actor_slab_floats([32], 5) == 16 * 32 + 32 + 32 * 32 + 32 + 4
    assert aref.actor_slab_floats([40, 24, 33], 64) == 64 * 64 + 64 + 64 * 32 + 32 + 32 * 64 + 64 + 64 * 32 + 32 + 4
    for case in aref.CASES:
        assert aref.splits_max(case[0], case[6]) == 128
    assert aref.split_rule(1, [64, 64], 12) == (1, 1) and aref.split_rule(17, [64, 64], 12) == (1, 2) and aref.split_rule(4096, [256, 256], 12) == (2, 128)
    multi = [c for c in aref.CASES if c[5] == "multi"]
    assert multi
    for case in multi:
        B = aref.resolve_B(case)
        assert B == 2049 and aref.split_rule(B, case[0], case[6]) == (2, 65) and aref.split_rule(B - 1, case[0], case[6]) == (1, 128)


def test_cases_cover_what_the_kernel_can_get_wrong():
    pairs = {(tuple(c[0]), tuple(c[1])) for c in aref.CASES}
    assert {((64, 64), (64, 64)), ((32,), (64,)), ((256, 256), (256, 256)), ((40, 24, 33), (40, 24, 33)), ((32,), (256, 256))} <= pairs
    assert {c[2] for c in aref.CASES} == {c[3] for c in aref.CASES} == {"relu", "tanh"} and {c[4] for c in aref.CASES} == {1, 2}
    assert {1, 16, 17, 33, 256, "multi"} <= {c[5] for c in aref.CASES}
    assert {(12, 8), (64, 8), (5, 3)} <= {(c[6], c[7]) for c in aref.CASES} and any(c[8] == "clamp" for c in aref.CASES)


def test_entropy_restatement_follows_torch():
    """ent_kernel restated in numpy float32 against SB3's lines under torch.optim.Adam in float64, three steps on given log-probabilities."""
    rng = np.random.default_rng(5)
    log_ent64 = torch.zeros(1, dtype=torch.float64, requires_grad=True)
    opt = torch.optim.Adam([log_ent64], lr=aref.LR)
    p, m, v = np.zeros(1, np.float32), np.zeros(1, np.float32), np.zeros(1, np.float32)
    for t in range(1, 4):
        logp = rng.standard_normal(33).astype(np.float32) * 2.0
        p, m, v = aref.entropy_step32(p, m, v, logp, -3.0, 1, t)
        loss = -(log_ent64 * (torch.tensor(logp, dtype=torch.float64) - 3.0)).mean()
        opt.zero_grad()
        loss.backward()
        opt.step()
        assert abs(float(p[0]) - float(log_ent64.detach())) <= 8 * t * ref.ULP
    # the order of the sum: a workgroup's tiles are added before the workgroups are
    logp = rng.standard_normal(100).astype(np.float32)
    assert aref.entropy_partial32(logp, -3.0, 1).dtype == np.float32
    assert abs(float(aref.entropy_partial32(logp, -3.0, 2)) - float((logp.astype(np.float64) - 3.0).sum())) < 1e-3


@pytest.mark.parametrize("index", range(len(aref.CASES)), ids=CASE_IDS)
def test_seeds_meet_the_conditions_of_the_device_tests(index):
    """(1) With two critics every row's |q0 - q1| in float64 is at least 64 x max |q32 - q64|: the float32 argmin is the float64 one in
    every row. (2) No raw log_std lies within 1e-3 of -20 or 2. (3) A float32 evaluation with the kernel's summation shape stays inside
    the bar the device test holds the kernel to. The clamp case has components on both sides of the clamp."""
    case = aref.CASES[index]
    actor, q_nets, batch, ref64, ref32 = aref.grad_references(index)
    if case[4] == 2:
        gap = (ref64["q_pi"][0] - ref64["q_pi"][1]).abs().min().item()
        err = (ref32["q_pi"].double() - ref64["q_pi"]).abs().max().item()
        print(f"{aref.case_id(case)}: min |q0 - q1| {gap:.3e}, max |q32 - q64| {err:.3e}")
        assert gap >= 64 * err, (gap, err)
        assert torch.equal(ref64["q_pi"].argmin(dim=0), ref32["q_pi"].argmin(dim=0))
    raw = ref64["raw_log_std"]
    assert ((raw + 20.0).abs().min().item() > 1e-3) and ((raw - 2.0).abs().min().item() > 1e-3)
    if case[8] == "clamp":
        assert bool((raw[:, 0] > 2.0).all()) and bool((raw[:, 1] < -20.0).all()) and bool(((raw[:, 2] > -20.0) & (raw[:, 2] < 2.0)).all())
        A = case[7]
        for r in (ref64, ref32):  # torch's clamp backward: no gradient through the clamped components' log_std
            assert not bool(r["grads"][-1][0][:2].any()) and not bool(r["grads"][-1][1][:2].any()) and bool(r["grads"][-1][1][2:A].any())
    else:
        assert bool(((raw > -20.0) & (raw < 2.0)).all())
    tps, _ = aref.split_rule(aref.resolve_B(case), case[0], case[6])
    grads, loss = aref.grad_tiled32(actor, q_nets, batch, aref.ENT, case, tps)
    aref.check_grads(aref.case_id(case), grads, ref64, ref32)
    ref.within_bar("loss", loss, ref64["loss"], ref32["loss"])


@pytest.mark.parametrize("index", aref.ADAM_CASES, ids=[aref.case_id(aref.CASES[i]) for i in aref.ADAM_CASES])
def test_seeds_keep_a_tiled_float32_adam_run_inside_the_bar(index):
    case = aref.CASES[index]
    actor, q_nets, batches, ref64, ref32 = aref.adam_references(index)
    tps, _ = aref.split_rule(aref.resolve_B(case), case[0], case[6])
    aref.check_params(aref.case_id(case), aref.adam_tiled32(actor, q_nets, batches, aref.ENT, case, tps), ref64, ref32)


# ---------------------------------------------------------------------------------------------- argument checks
D, A = 5, 2


@pytest.fixture
def stubs():
    from mujoco_sim_amd import DeviceActor, DeviceActorOptimizer, DeviceCritic, DeviceCriticOptimizer

    hidden, mu, log_std = ref.make_actor(D, [16, 8], A, seed=1)
    actor = _stub(DeviceActor, _a=1, hidden=hidden, mu=mu, log_std=log_std, widths=[16, 8], in_dim=D, in_total=D, action_dim=A, visual=False,
                  activation="relu", _owned_encoders=(), _staged=())
    shape = dict(obs_dim=D, action_dim=A, n_critics=2, widths=[16, 8], activation="relu", _loaded=True, _staged=())
    critic = _stub(DeviceCritic, _q=1, q_nets=ref.make_q_nets(D, A, [16, 8], 2, seed=1), **shape)
    target = _stub(DeviceCritic, _q=2, q_nets=ref.make_q_nets(D, A, [16, 8], 2, seed=2), **shape)
    actor_opt = _stub(DeviceActorOptimizer, _o=1, actor=actor, lr=3e-4, betas=(0.9, 0.999), eps=1e-8, step_count=0)
    critic_opt = _stub(DeviceCriticOptimizer, _o=1, critic=critic, lr=3e-4, betas=(0.9, 0.999), eps=1e-8, step_count=0)
    yield actor, critic, target, actor_opt, critic_opt
    actor._a = critic._q = target._q = actor_opt._o = critic_opt._o = None  # nothing native to destroy


def _batch(B=6):
    return {"obs": torch.zeros(B, D), "actions": torch.zeros(B, A), "next_obs": torch.zeros(B, D), "rewards": torch.zeros(B), "dones": torch.zeros(B)}


def test_optimizer_checks_its_arguments_before_any_native_call(stubs):
    from mujoco_sim_amd import DeviceActorOptimizer, DeviceEntropyCoef, MjsError

    actor, critic, _, opt, _ = stubs
    with pytest.raises(AssertionError, match="native layer"):  # valid arguments reach the (stubbed) native layer
        DeviceActorOptimizer(actor)
    for kw, match in ((dict(lr=-1e-3), "lr"), (dict(lr=float("nan")), "lr"), (dict(lr="fast"), "lr"), (dict(betas=(1.0, 0.999)), "betas"),
                      (dict(betas=0.9), "betas"), (dict(eps=0.0), "eps"), (dict(eps=float("inf")), "eps")):
        with pytest.raises(ValueError, match=match):
            DeviceActorOptimizer(actor, **kw)
    with pytest.raises(ValueError, match="must be a DeviceActor"):
        DeviceActorOptimizer(object())
    actor.visual = True
    with pytest.raises(ValueError, match="visual"):
        DeviceActorOptimizer(actor)
    actor.visual = False

    B = 6
    batch, z = _batch(B), torch.zeros(B, A)
    coef = DeviceEntropyCoef("cpu", A)
    calls = (lambda **kw: opt.step(**{"z": z, **kw}), lambda **kw: opt.gradients(**{"z": z, **kw}))
    for call in calls:
        for ent in (0.005, torch.tensor([0.005]), torch.tensor(0.005), coef):
            with pytest.raises(AssertionError, match="native layer"):
                call(batch=batch, critic=critic, ent_coef=ent)
        bad = [
            (dict(batch=[1, 2]), "dict"), (dict(batch={"actions": batch["actions"]}), "dict"), (dict(batch={**batch, "obs": batch["obs"][0]}), r"\[B, obs_dim\]"),
            (dict(batch={**batch, "obs": torch.zeros(B, D + 1)}), "shape"), (dict(batch={**batch, "obs": batch["obs"].double()}), "torch.float32"),
            (dict(batch={**batch, "obs": torch.zeros(D, B).t()}), "contiguous"), (dict(batch={**batch, "obs": torch.zeros(B, D, device="meta")}), "lives on"),
            (dict(critic=object()), "must be a DeviceCritic"), (dict(ent_coef="auto"), "ent_coef"), (dict(ent_coef=torch.zeros(2)), "shape"),
            (dict(ent_coef=torch.zeros(1, dtype=torch.float64)), "torch.float32"), (dict(ent_coef=DeviceEntropyCoef("cpu", A + 1)), "action components"),
            (dict(ent_coef=DeviceEntropyCoef("meta", A)), "lives on"), (dict(z=torch.zeros(B, A + 1)), "shape"), (dict(z=z.double()), "torch.float32"),
            (dict(z=torch.zeros(B - 1, A)), "shape"),
        ]
        for kw, match in bad:
            args = dict(batch=batch, critic=critic, ent_coef=0.005)
            args.update(kw)
            with pytest.raises(ValueError, match=match):
                call(**args)
                pytest.fail(match)
        for attr, value, match in (("obs_dim", D + 1, "observation columns"), ("action_dim", A + 1, "action components"), ("device", torch.device("meta"), "lives on")):
            keep = getattr(critic, attr)
            setattr(critic, attr, value)
            with pytest.raises(ValueError, match=match):
                call(batch=batch, critic=critic, ent_coef=0.005)
            setattr(critic, attr, keep)
    with pytest.raises(ValueError, match="z must be given"):
        opt.gradients(batch, critic, 0.005, None)
    for lr in (-1.0, float("inf"), "slow"):
        with pytest.raises(ValueError, match="lr"):
            opt.step(batch, critic, 0.005, z=z, lr=lr)
    # an empty batch: nothing to launch, and not a step, for the optimiser and for a learned coefficient
    empty = {k: v[:0] for k, v in batch.items()}
    assert opt.step(empty, critic, coef, z=z[:0]) is None and opt.step_count == 0 and coef.step_count == 0
    parts = opt.step(empty, critic, 0.005, return_parts=True)
    assert {k: tuple(v.shape) for k, v in parts.items()} == {"actions": (0, A), "log_prob": (0,), "q_pi": (2, 0), "min_q_action_grad": (0, A), "loss": (1,)}
    g = opt.gradients(empty, critic, 0.005, z[:0])
    assert [(tuple(w.shape), tuple(b.shape)) for w, b in g["grads"]] == [((16, D), (16,)), ((8, 16), (8,)), ((A, 8), (A,)), ((A, 8), (A,))]
    assert not any(t.any() for pair in g["grads"] for t in pair) and g["q_pi"].shape == (2, 0)
    opt._o = None
    with pytest.raises(MjsError, match="closed"):
        opt.step(batch, critic, 0.005, z=z)
    opt._o, critic._q = 1, None
    with pytest.raises(MjsError, match="closed"):
        opt.gradients(batch, critic, 0.005, z)
    critic._q, actor._a = 1, None
    with pytest.raises(MjsError, match="closed"):
        opt.step(batch, critic, 0.005, z=z)


def test_export_checks_its_arguments_before_any_native_call(stubs):
    from mujoco_sim_amd import DeviceActor, MjsError

    actor = stubs[0]
    with pytest.raises(AssertionError, match="native layer"):
        actor.export()
    with pytest.raises(AssertionError, match="native layer"):
        actor.export(ref.make_actor(D, [16, 8], A, seed=9))
    for modules, match in ((3, "hidden layers, mu, log_std"), (ref.make_actor(D, [16], A, seed=9), "hidden layers"), (ref.make_actor(D, [16, 12], A, seed=9), "expected"),
                           (ref.make_actor(D + 1, [16, 8], A, seed=9), "expected"), (ref.make_actor(D, [16, 8], A + 1, seed=9), "expected"),
                           (tuple(m if i else [x.double() for x in m] for i, m in enumerate(ref.make_actor(D, [16, 8], A, seed=9))), "float32 by contract"),
                           (([torch.nn.ReLU(), torch.nn.ReLU()], *ref.make_actor(D, [16, 8], A, seed=9)[1:]), "not a Linear")):
        with pytest.raises(ValueError, match=match):
            actor.export(modules)
    actor.visual = True
    with pytest.raises(ValueError, match="visual"):
        actor.export()
    actor.visual, actor._a = False, None
    with pytest.raises(MjsError, match="closed"):
        actor.export()
    assert "export" in DeviceActor.load.__doc__ and "stale" in DeviceActor.load.__doc__  # load() after a step overwrites: the docstring says so


def test_entropy_coefficient_object():
    from mujoco_sim_amd import DeviceEntropyCoef

    c = DeviceEntropyCoef("cpu", 3)
    assert c.target_entropy == -3.0 and c.step_count == 0 and c.lr == 3e-4
    assert c.ent_coef.shape == (1,) and c.log_ent_coef.shape == (1,) and c.ent_coef.dtype == torch.float32
    assert float(c.ent_coef) == 1.0 and float(c.log_ent_coef) == 0.0
    assert c.ent_coef.data_ptr() == c.log_ent_coef.data_ptr() + 4  # views of ONE small tensor
    c = DeviceEntropyCoef("cpu", 2, init=0.1, lr=1e-3, target_entropy=-1.5)
    assert c.target_entropy == -1.5 and torch.equal(c.log_ent_coef, torch.log(torch.ones(1) * 0.1)) and torch.equal(c.ent_coef, c.log_ent_coef.exp())
    block = c._block()
    assert (block.t, block.lr, block.target_entropy, block.m_dev - block.log_ent_coef_dev) == (1, 1e-3, -1.5, 8)
    for kw, match in ((dict(action_dim=0), "action_dim"), (dict(action_dim=9), "action_dim"), (dict(init=0.0), "init"), (dict(init=-1.0), "init"),
                      (dict(lr=-1.0), "lr"), (dict(target_entropy=float("nan")), "target_entropy"), (dict(target_entropy="low"), "target_entropy"),
                      (dict(betas=(1.0, 0.5)), "betas"), (dict(eps=0.0), "eps")):
        args = dict(device="cpu", action_dim=3)
        args.update(kw)
        with pytest.raises(ValueError, match=match):
            DeviceEntropyCoef(**args)


def test_sac_gradient_step_checks_its_arguments_before_any_native_call(stubs):
    from mujoco_sim_amd import DeviceEntropyCoef, MjsError, sac_gradient_step

    actor, critic, target, actor_opt, critic_opt = stubs
    B = 6
    batch = _batch(B)
    good = dict(batch=batch, actor=actor, critic=critic, target_critic=target, critic_opt=critic_opt, actor_opt=actor_opt, ent_coef=DeviceEntropyCoef("cpu", A),
                gamma=0.99, tau=0.005, z_next=torch.zeros(B, A), z_pi=torch.zeros(B, A))
    with pytest.raises(AssertionError, match="native layer"):
        sac_gradient_step(**good)
    bad = [
        (dict(critic_opt=actor_opt), "DeviceCriticOptimizer"), (dict(actor_opt=critic_opt), "DeviceActorOptimizer"), (dict(target_critic=critic), "one object"),
        (dict(target_critic=object()), "must be a DeviceCritic"), (dict(critic=target), "another critic"), (dict(tau=0.0), "tau"), (dict(tau=1.5), "tau"),
        (dict(gamma=1.5), "gamma"), (dict(batch={k: v for k, v in batch.items() if k != "actions"}), "dict"), (dict(batch={**batch, "actions": torch.zeros(B, A + 1)}), "shape"),
        (dict(batch={**batch, "rewards": torch.zeros(B + 1)}), "rows"), (dict(batch={**batch, "dones": torch.zeros(B).double()}), "torch.float32"),
        (dict(batch={**batch, "next_obs": torch.zeros(B, D + 1)}), "columns"), (dict(z_pi=torch.zeros(B, A + 1)), "shape"), (dict(z_next=torch.zeros(B + 1, A)), "shape"),
        (dict(ent_coef="auto"), "ent_coef"),
    ]
    for kw, match in bad:
        args = dict(good)
        args.update(kw)
        with pytest.raises(ValueError, match=match):
            sac_gradient_step(**args)
            pytest.fail(match)
    other = _stub(type(actor), **{k: v for k, v in actor.__dict__.items() if k not in ("_lib", "device")})
    with pytest.raises(ValueError, match="another actor"):
        sac_gradient_step(**{**good, "actor": other})
    other._a = None
    for obj, attr in ((critic_opt, "_o"), (actor_opt, "_o"), (target, "_q")):  # a closed object: MjsError, and still nothing native
        setattr(obj, attr, None)
        with pytest.raises(MjsError, match="closed"):
            sac_gradient_step(**good)
        setattr(obj, attr, 1 if obj is not target else 2)
    target.widths = [16, 12]
    with pytest.raises(ValueError, match="differs from the critic"):
        sac_gradient_step(**good)
