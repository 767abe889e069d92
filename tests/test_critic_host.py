"""The critics' host side, without a GPU: the C ABI (declared, exported, struct sizes as stated), the argument checks of DeviceCritic
and sac_td_target, which raise ValueError before the native layer is touched, and the packed-lerp layout restated in numpy."""
import ctypes as C
import re
from pathlib import Path
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import _critic_reference as ref

ROOT = Path(__file__).resolve().parents[1]
ENTRY_POINTS = (("mjs_critic_create", "int"), ("mjs_critic_destroy", "void"), ("mjs_critic_load", "int"), ("mjs_critic_q", "int"), ("mjs_sac_td_target", "int"))


def test_header_declares_and_library_exports_the_entry_points():
    from mujoco_sim_amd import _native

    header = (ROOT / "include" / "mjsim.h").read_text()
    for name, ret in ENTRY_POINTS:
        assert re.search(rf"^{ret} {name}\(", header, re.M), name
        assert name in _native.EXPORTED_SYMBOLS
    assert re.search(r"^#define MJS_ABI_VERSION 3$", header, re.M)  # entry points added after abi 3: the number stays
    _native.build()
    L = C.CDLL(str(_native.LIB_PATH))
    for name, _ in ENTRY_POINTS:
        assert hasattr(L, name), f"libmjsim.so does not export {name}"


def test_struct_sizes_stated_in_the_header_are_the_bindings():
    from mujoco_sim_amd import _native as nat

    header = (ROOT / "include" / "mjsim.h").read_text()
    for name, binding, size in (("mjs_critic_desc", nat.MjsCriticDesc, 40), ("mjs_critic_weights", nat.MjsCriticWeights, 136),
                                ("mjs_td_target_args", nat.MjsTdTargetArgs, 96)):
        stated = re.search(rf"\}} {name};\s*/\* (\d+) bytes \*/", header)
        assert stated, name
        assert int(stated.group(1)) == C.sizeof(binding) == size, name
        assert binding().struct_size == C.sizeof(binding)
        body = header[header.rindex("typedef struct {", 0, stated.start()):stated.start()]
        declared = re.findall(r"^\s+(?:const )?\w+\s*\**\s*(\w+)(?:\[\d+\])*;", body, re.M)
        assert declared == [n for n, _ in binding._fields_], name  # the same fields in the same order
    assert nat.MjsCriticWeights.hidden_w.size == 6 * C.sizeof(C.c_void_p)  # [2][3] pointers
    assert (nat.CRITIC_MAX_OBS, nat.CRITIC_MAX_CRITICS) == (64, 2) == (nat.REPLAY_MAX_OBS, 2)
    assert re.search(r"^#define MJS_CRITIC_MAX 2$", header, re.M)


@pytest.fixture
def no_native(monkeypatch):
    from mujoco_sim_amd import _native as nat

    def touched(*a, **k):
        raise AssertionError("the native layer was touched")

    monkeypatch.setattr(nat, "lib", touched)
    monkeypatch.setattr(nat, "check", touched)


def test_device_critic_checks_its_arguments_before_any_native_call(no_native):
    from mujoco_sim_amd import DeviceCritic

    D, A = 5, 2
    nets = ref.make_q_nets(D, A, [16, 8], 2, seed=1)
    with pytest.raises(AssertionError, match="native layer"):  # valid arguments reach the (patched) native layer: the checks below stop earlier
        DeviceCritic.from_linears("cpu", D, A, nets)
    with pytest.raises(AssertionError, match="native layer"):
        DeviceCritic.from_linears("cpu", D, A, nets[:1], activation="tanh")
    with pytest.raises(ValueError, match="activation"):
        DeviceCritic.from_linears("cpu", D, A, nets, activation="gelu")
    for bad in (0, 65):
        with pytest.raises(ValueError, match="observation columns"):
            DeviceCritic.from_linears("cpu", bad, A, nets)
    for bad in (0, 9):
        with pytest.raises(ValueError, match="action components"):
            DeviceCritic.from_linears("cpu", D, bad, nets)
    with pytest.raises(ValueError, match="1..2 critics"):
        DeviceCritic.from_linears("cpu", D, A, nets + nets[:1])
    with pytest.raises(ValueError, match="1..2 critics"):
        DeviceCritic.from_linears("cpu", D, A, [])
    with pytest.raises(ValueError, match="list of 1..2 sequences"):
        DeviceCritic.from_linears("cpu", D, A, 3)
    with pytest.raises(ValueError, match="at least one hidden layer"):
        DeviceCritic.from_linears("cpu", D, A, [nets[0][-1:]])
    with pytest.raises(ValueError, match="not a Linear"):
        DeviceCritic.from_linears("cpu", D, A, [[nets[0][0], torch.nn.ReLU(), nets[0][2]]])
    with pytest.raises(ValueError, match="hidden layers"):
        DeviceCritic.from_linears("cpu", D, A, ref.make_q_nets(D, A, [8, 8, 8, 8], 1, seed=1))
    with pytest.raises(ValueError, match="share an architecture"):
        DeviceCritic.from_linears("cpu", D, A, [nets[0], ref.make_q_nets(D, A, [16], 1, seed=2)[0]])
    with pytest.raises(ValueError, match="width 257"):
        DeviceCritic.from_linears("cpu", D, A, ref.make_q_nets(D, A, [257], 1, seed=1))
    with pytest.raises(ValueError, match="expected"):  # the first layer reads D + A columns
        DeviceCritic.from_linears("cpu", D + 1, A, nets)
    with pytest.raises(ValueError, match="expected"):  # the two critics' widths differ
        DeviceCritic.from_linears("cpu", D, A, [nets[0], ref.make_q_nets(D, A, [16, 12], 1, seed=2)[0]])
    with pytest.raises(ValueError, match="expected"):  # the head is Linear(., 1)
        DeviceCritic.from_linears("cpu", D, A, [[*nets[0][:-1], torch.nn.Linear(8, 2)]])
    with pytest.raises(ValueError, match="float32 by contract"):
        DeviceCritic.from_linears("cpu", D, A, [[m.double() for m in ref.make_q_nets(D, A, [16, 8], 1, seed=1)[0]]])
    with pytest.raises(ValueError, match="live on meta"):
        DeviceCritic.from_linears("cpu", D, A, [[m.to("meta") for m in ref.make_q_nets(D, A, [16, 8], 1, seed=1)[0]]])
    with pytest.raises(ValueError, match="without bias"):
        DeviceCritic.from_linears("cpu", D, A, [[torch.nn.Linear(D + A, 16, bias=False), *nets[0][1:]]])
    # from_sb3: duck-typed on q_networks
    act = torch.nn.Tanh
    sb3 = SimpleNamespace(q_networks=[torch.nn.Sequential(n[0], act(), n[1], act(), n[2]) for n in nets], action_space=SimpleNamespace(shape=(A,)))
    with pytest.raises(AssertionError, match="native layer"):
        DeviceCritic.from_sb3(sb3)
    with pytest.raises(ValueError, match="q_networks"):
        DeviceCritic.from_sb3(SimpleNamespace())
    with pytest.raises(ValueError, match="give action_dim"):
        DeviceCritic.from_sb3(SimpleNamespace(q_networks=sb3.q_networks))
    with pytest.raises(ValueError, match="mix ReLU and Tanh"):
        DeviceCritic.from_sb3(SimpleNamespace(q_networks=[torch.nn.Sequential(nets[0][0], act(), nets[0][1], torch.nn.ReLU(), nets[0][2])]), action_dim=A)
    with pytest.raises(ValueError, match="only Linear, ReLU and Tanh"):
        DeviceCritic.from_sb3(SimpleNamespace(q_networks=[torch.nn.Sequential(nets[0][0], torch.nn.GELU(), nets[0][1], nets[0][2])]), action_dim=A)


class _TouchedLib:
    def __getattr__(self, name):
        raise AssertionError("the native layer was touched")


def _stub(cls, **attrs):
    """An object of a native-backed class without its constructor: what the argument checks read, and a library that raises."""
    obj = cls.__new__(cls)
    obj.__dict__.update(_lib=_TouchedLib(), device=torch.device("cpu"), **attrs)
    return obj


@pytest.fixture
def stubs():
    from mujoco_sim_amd import DeviceActor, DeviceCritic

    D, A = 5, 2
    nets = ref.make_q_nets(D, A, [16, 8], 2, seed=1)
    critic = _stub(DeviceCritic, _q=1, obs_dim=D, action_dim=A, n_critics=2, widths=[16, 8], q_nets=nets, _loaded=True, _staged=())
    actor = _stub(DeviceActor, _a=1, in_dim=D, action_dim=A, visual=False, _owned_encoders=())
    yield actor, critic, nets
    actor._a = critic._q = None  # nothing native to destroy


def test_load_and_q_values_check_their_arguments_before_any_native_call(stubs):
    from mujoco_sim_amd import MjsError

    _, critic, nets = stubs
    with pytest.raises(AssertionError, match="native layer"):
        critic.load()
    with pytest.raises(AssertionError, match="native layer"):
        critic.load(ref.make_q_nets(5, 2, [16, 8], 2, seed=9), tau=0.005)
    for tau in (0.0, -0.1, 1.5, float("nan")):
        with pytest.raises(ValueError, match="tau"):
            critic.load(tau=tau)
    with pytest.raises(ValueError, match="holds 2 critics"):
        critic.load(nets[:1])
    with pytest.raises(ValueError, match="expected"):
        critic.load(ref.make_q_nets(5, 2, [16, 12], 2, seed=9))
    critic._loaded = False
    with pytest.raises(ValueError, match="first load"):
        critic.load(tau=0.5)
    critic._loaded = True
    obs, actions = torch.zeros(7, 5), torch.zeros(7, 2)
    with pytest.raises(AssertionError, match="native layer"):
        critic.q_values(obs, actions)
    assert critic.q_values(obs[:0], actions[:0]).shape == (2, 0)  # an empty batch: nothing to launch
    for o, a, match in ((obs.double(), actions, "torch.float32"), (obs, actions[:, :1].contiguous(), "shape"), (obs[:, :4].contiguous(), actions, "shape"),
                        (obs, actions[:6], "shape"), (obs.to("meta"), actions, "lives on"), (torch.zeros(5, 7).t(), actions, "contiguous"),
                        (obs.numpy(), actions, "tensor"), (obs[0], actions, r"\[B, obs_dim\]")):
        with pytest.raises(ValueError, match=match):
            critic.q_values(o, a)
    critic._q = None
    with pytest.raises(MjsError, match="closed"):
        critic.q_values(obs, actions)
    with pytest.raises(MjsError, match="closed"):
        critic.load()


def test_sac_td_target_checks_its_arguments_before_any_native_call(stubs):
    from mujoco_sim_amd import DeviceActor, MjsError, sac_td_target

    actor, critic, _ = stubs
    B, D, A = 6, 5, 2
    batch = {"next_obs": torch.zeros(B, D), "rewards": torch.zeros(B), "dones": torch.zeros(B), "obs": torch.zeros(B, D)}
    z = torch.zeros(B, A)
    with pytest.raises(AssertionError, match="native layer"):
        sac_td_target(batch, actor, critic, 0.99, 0.005, z=z)
    with pytest.raises(AssertionError, match="native layer"):
        sac_td_target(batch, actor, critic, 0.99, torch.tensor([0.005]), z=z, return_parts=True)
    empty = {k: v[:0] for k, v in batch.items()}
    assert sac_td_target(empty, actor, critic, 0.99, 0.005).shape == (0,)  # an empty batch: nothing to launch
    parts = sac_td_target(empty, actor, critic, 0.99, 0.005, return_parts=True)
    assert {k: tuple(v.shape) for k, v in parts.items()} == {"target": (0,), "next_actions": (0, A), "next_log_prob": (0,), "q_next": (2, 0)}
    bad = [
        (dict(actor=object()), "must be a DeviceActor"),
        (dict(critic=object()), "must be a DeviceCritic"),
        (dict(actor=_stub(DeviceActor, _a=None, in_dim=D, action_dim=A, visual=True, _owned_encoders=())), "visual"),
        (dict(actor=_stub(DeviceActor, _a=None, in_dim=D - 1, action_dim=A, visual=False, _owned_encoders=())), "observation columns"),
        (dict(actor=_stub(DeviceActor, _a=None, in_dim=D, action_dim=A + 1, visual=False, _owned_encoders=())), "action components"),
        (dict(gamma=1.01), "gamma"), (dict(gamma=-0.1), "gamma"), (dict(gamma=float("nan")), "gamma"),
        (dict(batch=[1, 2]), "dict"), (dict(batch={k: v for k, v in batch.items() if k != "dones"}), "dict"),
        (dict(batch={**batch, "next_obs": batch["next_obs"][0]}), r"\[B, obs_dim\]"),
        (dict(batch={**batch, "next_obs": torch.zeros(B, D + 1)}), "columns"),
        (dict(batch={**batch, "next_obs": batch["next_obs"].double()}), "torch.float32"),
        (dict(batch={**batch, "rewards": torch.zeros(B, 1)}), "shape"),
        (dict(batch={**batch, "dones": torch.zeros(B, dtype=torch.uint8)}), "torch.float32"),
        (dict(batch={**batch, "rewards": torch.zeros(B, device="meta")}), "lives on"),
        (dict(ent_coef="high"), "ent_coef"), (dict(ent_coef=torch.zeros(2)), "shape"), (dict(ent_coef=torch.zeros(1, dtype=torch.float64)), "torch.float32"),
        (dict(ent_coef=torch.zeros(1, device="meta")), "lives on"),
        (dict(z=torch.zeros(B, A + 1)), "shape"), (dict(z=z.double()), "torch.float32"), (dict(z=torch.zeros(A, B).t()), "contiguous"),
    ]
    for kw, match in bad:
        args = dict(batch=batch, actor=actor, critic=critic, gamma=0.99, ent_coef=0.005, z=z)
        args.update(kw)
        with pytest.raises(ValueError, match=match):
            sac_td_target(**args)
            pytest.fail(match)
    other = _stub(DeviceActor, _a=None, in_dim=D, action_dim=A, visual=False, _owned_encoders=())
    other.device = torch.device("meta")
    with pytest.raises(ValueError, match="the critic on"):
        sac_td_target(batch, other, critic, 0.99, 0.005, z=z)
    critic._q = None
    with pytest.raises(MjsError, match="closed"):
        sac_td_target(batch, actor, critic, 0.99, 0.005, z=z)


def test_packed_lerp_layout_restated_in_numpy():
    """What mjs_critic_load leaves in a layer's packed copy (csrc/mjs_critic.h pack_lerp_kernel, csrc/mjs_actor.h pack_kernel): K-major,
    zero padding that a blend keeps zero, tau = 1 a copy that never reads the destination, and each blended element within
    4 * 2^-24 * max(|dst|, |src|) of the float64 blend."""
    rng = np.random.default_rng(0)
    for out, fan_in in ((1, 64), (48, 7), (256, 72), (33, 17)):
        K, O = ref.round_up(fan_in, ref.KPAD), ref.round_up(out, ref.OPAD)
        w0, b0 = rng.standard_normal((out, fan_in)).astype(np.float32), rng.standard_normal(out).astype(np.float32)
        w1, b1 = rng.standard_normal((out, fan_in)).astype(np.float32), rng.standard_normal(out).astype(np.float32)
        pw, pb = ref.pack_lerp_np(None, None, w0, b0, K, O, 1.0)  # a first load: dst is not read
        assert pw.shape == (K, O) and pb.shape == (O,) and pw.dtype == np.float32
        assert np.array_equal(pw[:fan_in, :out], w0.T) and np.array_equal(pb[:out], b0)  # packed[k][o] = weight[o][k]
        assert not pw[fan_in:].any() and not pw[:, out:].any() and not pb[out:].any()
        tau = 0.005
        lw, lb = ref.pack_lerp_np(pw, pb, w1, b1, K, O, tau)
        assert not lw[fan_in:].any() and not lw[:, out:].any() and not lb[out:].any()  # the padding stays 0
        want = (1.0 - tau) * w0.T.astype(np.float64) + tau * w1.T.astype(np.float64)
        bound = 4 * ref.ULP * np.maximum(np.abs(w0.T), np.abs(w1.T))
        assert (np.abs(lw[:fan_in, :out] - want) <= bound).all()
        want_b = (1.0 - tau) * b0.astype(np.float64) + tau * b1.astype(np.float64)
        assert (np.abs(lb[:out] - want_b) <= 4 * ref.ULP * np.maximum(np.abs(b0), np.abs(b1))).all()
        again_w, again_b = ref.pack_lerp_np(lw, lb, w1, b1, K, O, 1.0)  # tau = 1 after a lerp: a fresh load
        fresh_w, fresh_b = ref.pack_lerp_np(None, None, w1, b1, K, O, 1.0)
        assert np.array_equal(again_w, fresh_w) and np.array_equal(again_b, fresh_b)
