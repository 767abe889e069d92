"""The critic update's host side, without a GPU: the C ABI (declared, exported, struct sizes as stated), the argument checks of
DeviceCriticOptimizer, DeviceCritic.export and DeviceCritic.blend_from, which raise ValueError before the native layer is touched, the
split rule, and the check of the device tests' seeds: a float32 evaluation with the kernel's summation shape stays inside the bar."""
import ctypes as C
import re
from pathlib import Path

import numpy as np
import pytest
import torch

import _critic_reference as ref
import _critic_train_reference as tref

ROOT = Path(__file__).resolve().parents[1]


class _TouchedLib:
    def __getattr__(self, name):
        raise AssertionError("the native layer was touched")


def _stub(cls, **attrs):
    """An object of a native-backed class without its constructor: what the argument checks read, and a library that raises."""
    obj = cls.__new__(cls)
    obj.__dict__.update(_lib=_TouchedLib(), device=torch.device("cpu"), **attrs)
    return obj


ENTRY_POINTS = (("mjs_critic_opt_create", "int"), ("mjs_critic_opt_destroy", "void"), ("mjs_critic_train_workspace_bytes", "uint64_t"),
                ("mjs_critic_grad", "int"), ("mjs_critic_update", "int"), ("mjs_critic_blend", "int"), ("mjs_critic_export", "int"))


def test_header_declares_and_library_exports_the_entry_points():
    from mujoco_sim_amd import _native

    header = (ROOT / "include" / "mjsim.h").read_text()
    for name, ret in ENTRY_POINTS:
        assert re.search(rf"^{ret} {name}\(", header, re.M), name
        assert name in _native.EXPORTED_SYMBOLS
    assert re.search(r"^#define MJS_ABI_VERSION 3$", header, re.M)  # entry points added after abi 3: the number stays
    assert "typedef struct mjs_critic_opt mjs_critic_opt;" in header
    _native.build()
    L = C.CDLL(str(_native.LIB_PATH))
    for name, _ in ENTRY_POINTS:
        assert hasattr(L, name), f"libmjsim.so does not export {name}"


def test_struct_sizes_stated_in_the_header_are_the_bindings():
    from mujoco_sim_amd import _native as nat

    header = (ROOT / "include" / "mjsim.h").read_text()
    for name, binding, size in (("mjs_critic_opt_desc", nat.MjsCriticOptDesc, 40), ("mjs_critic_grad_args", nat.MjsCriticGradArgs, 56)):
        stated = re.search(rf"\}} {name};\s*/\* (\d+) bytes \*/", header)
        assert stated, name
        assert int(stated.group(1)) == C.sizeof(binding) == size, name
        assert binding().struct_size == C.sizeof(binding)
        body = header[header.rindex("typedef struct {", 0, stated.start()):stated.start()]
        declared = re.findall(r"^\s+(?:const )?\w+\s*\**\s*(\w+)(?:\[\d+\])*;", body, re.M)
        assert declared == [n for n, _ in binding._fields_], name  # the same fields in the same order


def test_split_rule_is_a_function_of_the_batch_and_the_shape():
    assert tref.slab_floats([64, 64]) == 16 * 64 + 64 + 64 * 64 + 64 + 64 * 32 + 32 + 4
    assert tref.slab_floats([40, 24, 33]) == 16 * 64 + 64 + 64 * 32 + 32 + 32 * 64 + 64 + 64 * 32 + 32 + 4
    assert tref.splits_max([64, 64], 2) == 128 == tref.splits_max([256, 256], 2)
    assert tref.splits_max([256, 256, 256], 2) == (128 << 20) // (2 * 4 * tref.slab_floats([256, 256, 256])) == 116  # the widest shape: the byte cap binds
    assert tref.split_rule(1, [64, 64], 2) == (1, 1) and tref.split_rule(17, [64, 64], 2) == (1, 2) and tref.split_rule(256, [64, 64], 2) == (1, 16)
    assert tref.split_rule(4096, [64, 64], 2) == (2, 128) and tref.split_rule(4096, [256, 256], 2) == (2, 128) and tref.split_rule(4096, [256, 256, 256], 2) == (3, 86)
    for widths, n_critics in (([64, 64], 2), ([256, 256], 2), ([40, 24, 33], 2), ([32], 1)):
        B = tref.multi_B(widths, n_critics)
        tps, splits = tref.split_rule(B, widths, n_critics)
        assert tps == 2 and splits > 1, (widths, B, tps, splits)  # more than one tile per workgroup AND more than one split
        assert tref.split_rule(B - 1, widths, n_critics)[0] == 1
        assert splits * n_critics * tref.slab_floats(widths) * 4 <= 128 << 20  # the workspace stays bounded


def test_adam_restatement_follows_torch():
    """The header's float32 operation order, restated in numpy, against torch.optim.Adam in float64 on the same gradients: three steps,
    each element within a few float32 roundings of the step's size."""
    rng = np.random.default_rng(3)
    p0 = rng.standard_normal(500).astype(np.float32)
    grads = [(rng.standard_normal(500) * s).astype(np.float32) for s in (1.0, 1e-3, 10.0)]
    p, m, v = p0.copy(), np.zeros(500, np.float32), np.zeros(500, np.float32)
    t64 = torch.tensor(p0, dtype=torch.float64, requires_grad=True)
    opt = torch.optim.Adam([t64], lr=tref.LR)
    for t, g in enumerate(grads, start=1):
        p, m, v = tref.adam_step32(p, g, m, v, t)
        t64.grad = torch.tensor(g, dtype=torch.float64)
        opt.step()
        assert np.abs(p.astype(np.float64) - t64.detach().numpy()).max() <= 4 * t * ref.ULP * max(1.0, np.abs(p0).max())
    assert tref.adam_coefficients(1)["step_size"] == np.float32(tref.LR / (1.0 - 0.9)) and tref.adam_coefficients(1)["sqrt_bc2"] == np.float32((1.0 - 0.999) ** 0.5)


@pytest.mark.parametrize("index", range(len(tref.CASES)), ids=[tref.case_id(c) for c in tref.CASES])
def test_seeds_keep_a_tiled_float32_gradient_inside_the_bar(index):
    """The device test holds the kernel's gradients to within_bar against torch autograd. For the seeds it uses, a second float32
    evaluation with the kernel's summation shape (per-16-row-tile gradients, added in order) must stay inside that bar on the CPU."""
    case = tref.CASES[index]
    nets, batch, ref64, ref32 = tref.grad_references(index)
    tps, _ = tref.split_rule(tref.resolve_B(case), case[0], case[2])
    tref.check_grads(tref.case_id(case), tref.grad_tiled32(nets, batch, case[1], tps), ref64, ref32)


@pytest.mark.parametrize("index", range(len(tref.ADAM_CASES)), ids=[tref.case_id(c) for c in tref.ADAM_CASES])
def test_seeds_keep_a_tiled_float32_adam_run_inside_the_bar(index):
    """The same for five Adam steps: tiled float32 gradients and the header's Adam against torch.optim.Adam in float64 and float32."""
    case = tref.ADAM_CASES[index]
    nets, batches, ref64, ref32 = tref.adam_references(index)
    tps, _ = tref.split_rule(tref.resolve_B(case), case[0], case[2])
    tref.check_params(tref.case_id(case), tref.adam_tiled32(nets, batches, case[1], tps), ref64, ref32)


@pytest.fixture
def stubs():
    from mujoco_sim_amd import DeviceCritic, DeviceCriticOptimizer

    D, A = 5, 2
    nets = ref.make_q_nets(D, A, [16, 8], 2, seed=1)
    shape = dict(obs_dim=D, action_dim=A, n_critics=2, widths=[16, 8], activation="relu", _loaded=True, _staged=())
    critic = _stub(DeviceCritic, _q=1, q_nets=nets, **shape)
    other = _stub(DeviceCritic, _q=2, q_nets=ref.make_q_nets(D, A, [16, 8], 2, seed=2), **shape)
    opt = _stub(DeviceCriticOptimizer, _o=1, critic=critic, lr=3e-4, betas=(0.9, 0.999), eps=1e-8, step_count=0)
    yield critic, other, opt, nets
    critic._q = other._q = opt._o = None  # nothing native to destroy


def test_optimizer_checks_its_arguments_before_any_native_call(stubs):
    from mujoco_sim_amd import DeviceCriticOptimizer, MjsError

    critic, _, opt, _ = stubs
    with pytest.raises(AssertionError, match="native layer"):  # valid arguments reach the (stubbed) native layer
        DeviceCriticOptimizer(critic)
    for kw, match in ((dict(lr=-1e-3), "lr"), (dict(lr=float("nan")), "lr"), (dict(lr="fast"), "lr"), (dict(betas=(1.0, 0.999)), "betas"),
                      (dict(betas=(0.9, -0.1)), "betas"), (dict(betas=0.9), "betas"), (dict(betas=(0.9, 0.99, 0.999)), "betas"),
                      (dict(eps=0.0), "eps"), (dict(eps=-1e-8), "eps"), (dict(eps=float("inf")), "eps")):
        with pytest.raises(ValueError, match=match):
            DeviceCriticOptimizer(critic, **kw)
    with pytest.raises(ValueError, match="must be a DeviceCritic"):
        DeviceCriticOptimizer(object())

    B, D, A = 6, 5, 2
    batch = {"obs": torch.zeros(B, D), "actions": torch.zeros(B, A), "rewards": torch.zeros(B)}
    target = torch.zeros(B)
    for call in (opt.step, opt.gradients):
        with pytest.raises(AssertionError, match="native layer"):
            call(batch, target)
        bad = [
            (dict(batch=[1, 2]), "dict"), (dict(batch={"obs": batch["obs"]}), "dict"),
            (dict(batch={**batch, "obs": batch["obs"][0]}), r"\[B, obs_dim\]"), (dict(batch={**batch, "obs": torch.zeros(B, D + 1)}), "shape"),
            (dict(batch={**batch, "obs": batch["obs"].double()}), "torch.float32"), (dict(batch={**batch, "actions": torch.zeros(B, A + 1)}), "shape"),
            (dict(batch={**batch, "actions": torch.zeros(B - 1, A)}), "shape"), (dict(batch={**batch, "actions": torch.zeros(A, B).t()}), "contiguous"),
            (dict(batch={**batch, "obs": torch.zeros(B, D, device="meta")}), "lives on"), (dict(target=torch.zeros(B, 1)), "shape"),
            (dict(target=target.double()), "torch.float32"), (dict(target=[0.0] * B), "tensor"), (dict(target=torch.zeros(B + 1)), "shape"),
        ]
        for kw, match in bad:
            args = dict(batch=batch, target=target)
            args.update(kw)
            with pytest.raises(ValueError, match=match):
                call(**args)
                pytest.fail(match)
    for lr in (-1.0, float("inf"), "slow"):
        with pytest.raises(ValueError, match="lr"):
            opt.step(batch, target, lr=lr)
    # an empty batch: nothing to launch, and not a step
    empty = {k: v[:0] for k, v in batch.items()}
    assert opt.step(empty, target[:0]) is None and opt.step_count == 0
    parts = opt.step(empty, target[:0], return_parts=True)
    assert {k: tuple(v.shape) for k, v in parts.items()} == {"loss": (2,), "q": (2, 0)}
    g = opt.gradients(empty, target[:0])
    assert [[(tuple(w.shape), tuple(b.shape)) for w, b in net] for net in g["grads"]] == [[((16, 7), (16,)), ((8, 16), (8,)), ((1, 8), (1,))]] * 2
    assert not any(t.any() for net in g["grads"] for pair in net for t in pair) and g["q"].shape == (2, 0)
    opt._o = None
    with pytest.raises(MjsError, match="closed"):
        opt.step(batch, target)
    opt._o, critic._q = 1, None
    with pytest.raises(MjsError, match="closed"):
        opt.gradients(batch, target)


def test_export_and_blend_from_check_their_arguments_before_any_native_call(stubs):
    from mujoco_sim_amd import DeviceCritic, MjsError

    critic, other, _, nets = stubs
    with pytest.raises(AssertionError, match="native layer"):
        critic.export()
    with pytest.raises(AssertionError, match="native layer"):
        critic.export(ref.make_q_nets(5, 2, [16, 8], 2, seed=9))
    with pytest.raises(ValueError, match="holds 2 critics"):
        critic.export(nets[:1])
    with pytest.raises(ValueError, match="expected"):
        critic.export(ref.make_q_nets(5, 2, [16, 12], 2, seed=9))
    with pytest.raises(ValueError, match="float32 by contract"):
        critic.export([[m.double() for m in net] for net in ref.make_q_nets(5, 2, [16, 8], 2, seed=9)])
    with pytest.raises(ValueError, match="list of 1..2 sequences"):
        critic.export(3)

    with pytest.raises(AssertionError, match="native layer"):
        critic.blend_from(other, 0.005)
    with pytest.raises(AssertionError, match="native layer"):
        critic.blend_from(other, 1.0)
    for tau in (0.0, -0.1, 1.5, float("nan")):
        with pytest.raises(ValueError, match="tau"):
            critic.blend_from(other, tau)
    with pytest.raises(ValueError, match="must be a DeviceCritic"):
        critic.blend_from(nets, 0.5)
    for attr, value in (("obs_dim", 6), ("action_dim", 3), ("n_critics", 1), ("widths", [16, 12]), ("widths", [16]), ("activation", "tanh")):
        keep = getattr(other, attr)
        setattr(other, attr, value)
        with pytest.raises(ValueError, match="differ in shape"):
            critic.blend_from(other, 0.5)
        setattr(other, attr, keep)
    other.device = torch.device("meta")
    with pytest.raises(ValueError, match="lives on"):
        critic.blend_from(other, 0.5)
    other.device = torch.device("cpu")
    critic._loaded = False
    with pytest.raises(ValueError, match="tau == 1 only"):
        critic.blend_from(other, 0.5)
    critic._loaded = True
    other._q = None
    with pytest.raises(MjsError, match="closed"):
        critic.blend_from(other, 0.5)
    assert "export" in DeviceCritic.load.__doc__ and "stale" in DeviceCritic.load.__doc__  # load() after a step overwrites: the docstring says so
