"""The gradient loop's host side, without a GPU: Philox4x32-10 restated against its known answers, the restated normals' first two moments,
the C ABI (declared, exported, struct sizes as stated), every ValueError of DeviceSAC and from_sb3 before the native layer is touched, and the
bookkeeping of learn with a buffer and an env that count calls."""
import ctypes as C
import re
import types
from pathlib import Path

import numpy as np
import pytest
import torch

import _critic_reference as ref
import _sac_train_reference as sref

ROOT = Path(__file__).resolve().parents[1]
D, A = 5, 2


# ---------------------------------------------------------------------------------------------- the generator
def test_philox_known_answers():
    kat = [((0, 0, 0, 0), (0, 0), "6627e8d5 e169c58d bc57ac4c 9b00dbd8"),
           ((0xFFFFFFFF,) * 4, (0xFFFFFFFF, 0xFFFFFFFF), "408f276d 41c83b0e a20bc7c6 6d5451fd"),
           ((0x243F6A88, 0x85A308D3, 0x13198A2E, 0x03707344), (0xA4093822, 0x299F31D0), "d16cfe09 94fdcceb 5001e420 24126ea1")]
    for counter, key, want in kat:
        got = sref.philox4x32_10(np.array(counter, np.uint32), key)
        assert " ".join(f"{int(w):08x}" for w in got) == want, (counter, key)
    # vectorised over rows as over single counters, and the counter layout: (b, block, step lo, step hi), key (seed lo, seed hi)
    step, seed = 2**32 + 3, 2**63 + 12345
    rows = sref.row_words(5, 2, step, seed)
    for b in range(5):
        assert np.array_equal(rows[b], sref.philox4x32_10(np.array([b, 2, 3, 1], np.uint32), (12345, 2**31)))


def test_draws_lie_in_the_range_sample_documents():
    d = sref.draws(4096, 7, 0)
    assert d.dtype == np.int64 and d.min() >= 0 and d.max() < 2**62 and len(np.unique(d)) == 4096
    assert not np.array_equal(d, sref.draws(4096, 8, 0)) and not np.array_equal(d, sref.draws(4096, 7, 1))
    assert np.array_equal(sref.indices(d, 0), np.full(4096, -1)) and sref.indices(d, 5).max() == 4 and sref.indices(d, 5).min() == 0


def test_restated_normals_have_the_moments_of_a_standard_normal():
    """2^16 rows x 8 components: |mean| < 5 / sqrt(n) and |variance - 1| < 5 sqrt(2 / n) (five standard errors of the mean and of the
    variance of n standard normals), for both samples, in float64 and float32; the float32 lines stay within 1e-5 of the float64 ones."""
    B, n = 2**16, 2**16 * 8
    for which in ("z_next", "z_pi"):
        z64 = sref.normals(B, 8, 11, 2025, which, np.float64)
        z32 = sref.normals(B, 8, 11, 2025, which, np.float32)
        assert z32.dtype == np.float32 and np.isfinite(z64).all() and np.isfinite(z32).all()
        for z in (z64, z32.astype(np.float64)):
            mean, var = z.mean(), z.var()
            print(f"{which}: mean {mean:.3e} (bound {5 / np.sqrt(n):.3e}), variance - 1 {var - 1:.3e} (bound {5 * np.sqrt(2 / n):.3e})")
            assert abs(mean) < 5 / np.sqrt(n) and abs(var - 1.0) < 5 * np.sqrt(2.0 / n)
        assert np.abs(z32 - z64).max() < 1e-5
    assert not np.array_equal(sref.normals(64, 8, 11, 2025, "z_next"), sref.normals(64, 8, 11, 2025, "z_pi"))
    # a narrower action space takes a prefix of the same components
    assert np.array_equal(sref.normals(64, 3, 11, 2025, "z_pi"), sref.normals(64, 8, 11, 2025, "z_pi")[:, :3])


# ---------------------------------------------------------------------------------------------- the C ABI
ENTRY_POINTS = (("mjs_sac_draw_batch", "int"), ("mjs_sac_train", "int"))


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
    for name, binding, size in (("mjs_sac_batch", nat.MjsSacBatch, 80), ("mjs_sac_train_args", nat.MjsSacTrainArgs, 152)):
        stated = re.search(rf"\}} {name};\s*/\* (\d+) bytes \*/", header)
        assert stated, name
        assert int(stated.group(1)) == C.sizeof(binding) == size, name
        assert binding().struct_size == C.sizeof(binding)
        body = header[header.rindex("typedef struct {", 0, stated.start()):stated.start()]
        declared = re.findall(r"^\s+(?:const )?\w+\s*\**\s*(\w+)(?:\[\d+\])*;", body, re.M)
        assert declared == [n for n, _ in binding._fields_], name  # the same fields in the same order


def test_kernel_header_states_its_lines():
    text = (ROOT / "mujoco_sim_amd" / "csrc" / "mjs_sac_train.h").read_text()
    for piece in ("0xD2511F53", "0xCD9E8D57", "0x9E3779B9", "0xBB67AE85", "u1  = (float)((w >> 8) + 1) * 2^-24", "r = sqrtf(m)", "ang = TWO_PI * u2",
                  "(b, block, step & 0xffffffff, step >> 32)"):
        assert piece in text, piece
    assert "atomic" not in text.replace("No atomics", "") and "asm" not in text.replace("inline assembly", "")


# ---------------------------------------------------------------------------------------------- argument checks
def test_the_trainer_is_new():
    """The test that fails without the feature: the module and the package's export."""
    from mujoco_sim_amd.sac import DeviceSAC
    import mujoco_sim_amd as m

    assert m.DeviceSAC is DeviceSAC


class _TouchedLib:
    def __getattr__(self, name):
        raise AssertionError("the native layer was touched")


def _stub(cls, **attrs):
    obj = cls.__new__(cls)
    obj.__dict__.update(_lib=_TouchedLib(), device=torch.device("cpu"), **attrs)
    return obj


@pytest.fixture
def stubs():
    from mujoco_sim_amd import DeviceActor, DeviceCritic, DeviceReplayBuffer

    hidden, mu, log_std = ref.make_actor(D, [16, 8], A, seed=1)
    actor = _stub(DeviceActor, _a=1, hidden=hidden, mu=mu, log_std=log_std, widths=[16, 8], in_dim=D, in_total=D, action_dim=A, visual=False,
                  activation="relu", _owned_encoders=(), _staged=(), obs_index=list(range(D)))
    shape = dict(obs_dim=D, action_dim=A, n_critics=2, widths=[16, 8], activation="relu", _loaded=True, _staged=())
    critic = _stub(DeviceCritic, _q=1, q_nets=ref.make_q_nets(D, A, [16, 8], 2, seed=1), **shape)
    target = _stub(DeviceCritic, _q=2, q_nets=ref.make_q_nets(D, A, [16, 8], 2, seed=2), **shape)
    buffer = _stub(DeviceReplayBuffer, capacity=64, obs_dim=D, action_dim=A, cameras=(), obs_index=list(range(D)), autoreset="next_step", _storage=None)
    venv = types.SimpleNamespace(device="cpu", action_dim=A, obs_dim=D, num_envs=4, autoreset="next_step")
    yield venv, actor, critic, target, buffer
    actor._a = critic._q = target._q = None  # nothing native to destroy
    buffer._lib = None


def test_constructor_checks_its_arguments_before_any_native_call(stubs):
    from mujoco_sim_amd import DeviceSAC, MjsError

    venv, actor, critic, target, buffer = stubs
    with pytest.raises(AssertionError, match="native layer"):  # valid arguments reach the (stubbed) native layer
        DeviceSAC(venv, actor, critic, target, buffer)
    bad = [
        (dict(tau=0.0), "tau"), (dict(tau=1.5), "tau"), (dict(tau="slow"), "tau"), (dict(gamma=-0.1), "gamma"), (dict(gamma=1.01), "gamma"),
        (dict(batch_size=0), "batch_size"), (dict(batch_size=2.5), "batch_size"), (dict(gradient_steps=-2), "gradient_steps"), (dict(gradient_steps="many"), "gradient_steps"),
        (dict(train_freq=0), "train_freq"), (dict(train_freq=(1, "episode")), "episodes"), (dict(train_freq=(4, "lap")), "unit"), (dict(train_freq=(1, 2, 3)), "train_freq"),
        (dict(learning_starts=-1), "learning_starts"), (dict(target_update_interval=0), "target_update_interval"), (dict(learning_rate=-1e-3), "learning_rate"),
        (dict(learning_rate=float("nan")), "learning_rate"), (dict(ent_coef="manual"), "ent_coef"), (dict(ent_coef="auto_x"), "ent_coef"), (dict(ent_coef="auto_-1"), "ent_coef"),
        (dict(ent_coef=-0.1), "ent_coef"), (dict(target_entropy="low"), "target_entropy"), (dict(target_entropy=float("inf")), "target_entropy"),
        (dict(buffer_size=0), "buffer_size"), (dict(seed=-1), "seed"), (dict(seed=2**64), "seed"), (dict(seed=0.5), "seed"),
    ]
    for kw, match in bad:
        with pytest.raises(ValueError, match=match):
            DeviceSAC(venv, actor, critic, target, buffer, **kw)
            pytest.fail(match)
    with pytest.raises(ValueError, match="must be a DeviceActor"):
        DeviceSAC(venv, object(), critic, target, buffer)
    with pytest.raises(ValueError, match="must be a DeviceCritic"):
        DeviceSAC(venv, actor, object(), target, buffer)
    with pytest.raises(ValueError, match="target_critic must be a DeviceCritic"):
        DeviceSAC(venv, actor, critic, object(), buffer)
    with pytest.raises(ValueError, match="one object"):
        DeviceSAC(venv, actor, critic, critic, buffer)
    with pytest.raises(ValueError, match="must be a DeviceReplayBuffer"):
        DeviceSAC(venv, actor, critic, target, object())
    actor.visual = True
    with pytest.raises(ValueError, match="visual critics are not built"):  # sac_td_target's sentence
        DeviceSAC(venv, actor, critic, target, buffer)
    actor.visual = False
    for obj, attr, value, match in ((critic, "obs_dim", D + 1, "observation columns"), (critic, "action_dim", A + 1, "action components"),
                                    (critic, "device", torch.device("meta"), "lives on"), (target, "widths", [16, 12], "differs from the critic"),
                                    (target, "n_critics", 1, "differs from the critic"), (buffer, "cameras", ("Camera/rgb_image",), "state-only"),
                                    (buffer, "obs_dim", D + 1, "observation and"), (buffer, "action_dim", A + 1, "observation and"),
                                    (buffer, "device", torch.device("meta"), "lives on"), (buffer, "obs_index", list(range(D))[::-1], "in order"),
                                    (venv, "action_dim", A + 1, "the env has"), (venv, "device", "meta", "the env lives on")):
        keep = getattr(obj, attr)
        setattr(obj, attr, value)
        with pytest.raises(ValueError, match=match):
            DeviceSAC(venv, actor, critic, target, buffer)
        setattr(obj, attr, keep)
    # closed objects: MjsError, and still nothing native
    for obj, attr in ((actor, "_a"), (critic, "_q"), (target, "_q")):
        keep = getattr(obj, attr)
        setattr(obj, attr, None)
        with pytest.raises(MjsError, match="closed"):
            DeviceSAC(venv, actor, critic, target, buffer)
        setattr(obj, attr, keep)


def test_ent_coef_and_train_freq_forms():
    from mujoco_sim_amd.sac import DeviceSAC, _parse_ent_coef, _parse_train_freq

    assert _parse_ent_coef("auto") == (True, 1.0) and _parse_ent_coef("auto_0.1") == (True, 0.1) and _parse_ent_coef(0.005) == (False, 0.005)
    assert _parse_train_freq(4) == 4 and _parse_train_freq((8, "step")) == 8
    unit = types.SimpleNamespace(value="step")  # SB3's TrainFrequencyUnit.STEP
    assert _parse_train_freq(types.SimpleNamespace(frequency=2, unit=unit)) == 2
    with pytest.raises(ValueError, match="episodes"):
        _parse_train_freq(types.SimpleNamespace(frequency=1, unit=types.SimpleNamespace(value="episode")))
    hp = DeviceSAC._hyperparameters(buffer_size=10, batch_size=4, learning_rate=1e-3, gamma=0.9, tau=1.0, ent_coef="auto_0.5", target_entropy="auto", train_freq=2,
                                    gradient_steps=-1, learning_starts=0, target_update_interval=3, seed=2**64 - 1)
    assert (hp["ent_coef_learned"], hp["ent_coef_init"], hp["target_entropy"], hp["gradient_steps"], hp["seed"]) == (True, 0.5, None, -1, 2**64 - 1)


def _sb3_model(**over):
    """A stand-in with the attributes of stable_baselines3.SAC after _setup_model."""
    hidden, mu, log_std = ref.make_actor(D, [16, 8], A, seed=3)
    latent = torch.nn.Sequential(hidden[0], torch.nn.ReLU(), hidden[1], torch.nn.ReLU())
    nets = lambda seed: torch.nn.ModuleList([torch.nn.Sequential(n[0], torch.nn.ReLU(), n[1], torch.nn.ReLU(), n[2]) for n in ref.make_q_nets(D, A, [16, 8], 2, seed=seed)])  # noqa: E731
    space = types.SimpleNamespace(shape=(A,))
    model = types.SimpleNamespace(actor=types.SimpleNamespace(latent_pi=latent, mu=mu, log_std=log_std),
                                  critic=types.SimpleNamespace(q_networks=nets(4), action_space=space),
                                  critic_target=types.SimpleNamespace(q_networks=nets(5), action_space=space),
                                  gamma=0.98, tau=0.02, batch_size=32, buffer_size=1000, learning_starts=64, gradient_steps=-1, target_update_interval=2, ent_coef="auto_0.2",
                                  target_entropy=-2.0, train_freq=types.SimpleNamespace(frequency=4, unit=types.SimpleNamespace(value="step")), lr_schedule=lambda p: 7e-4 * p,
                                  learning_rate=3e-4, log_ent_coef=torch.zeros(1))
    model.__dict__.update(over)
    return model


def test_from_sb3_checks_before_any_native_call(monkeypatch):
    from mujoco_sim_amd import DeviceActor, DeviceSAC

    venv = types.SimpleNamespace(device="cpu", action_dim=A, obs_dim=D, num_envs=4, _dev_index=0, flat_observation_layout=[("obs", 0, D)])
    seen = {}

    def reached(cls, venv_, actor, obs_keys=None, **kw):
        seen["actor"] = actor
        raise AssertionError("the native layer was touched")

    monkeypatch.setattr(DeviceActor, "from_sb3", classmethod(reached))
    with pytest.raises(AssertionError, match="native layer"):  # a good model's hyperparameters pass, and the first native object is the actor
        DeviceSAC.from_sb3(venv, _sb3_model())
    assert "actor" in seen
    bad = [(dict(train_freq=types.SimpleNamespace(frequency=1, unit=types.SimpleNamespace(value="episode"))), "episodes"), (dict(train_freq=(1, "episode")), "episodes"),
           (dict(tau=0.0), "tau"), (dict(gamma=2.0), "gamma"), (dict(batch_size=0), "batch_size"), (dict(gradient_steps=-3), "gradient_steps"),
           (dict(ent_coef="fixed"), "ent_coef"), (dict(lr_schedule=lambda p: -1.0), "learning_rate"), (dict(actor=None), "no attribute 'actor'"),
           (dict(critic_target=None), "no attribute 'critic_target'")]
    for over, match in bad:
        seen.clear()
        with pytest.raises(ValueError, match=match):
            DeviceSAC.from_sb3(venv, _sb3_model(**over))
        assert not seen, match
    with pytest.raises(ValueError, match="unknown arguments"):
        DeviceSAC.from_sb3(venv, _sb3_model(), momentum=0.9)
    with pytest.raises(ValueError, match="tau"):  # a keyword overrides the model, and is checked like it
        DeviceSAC.from_sb3(venv, _sb3_model(), tau=-1.0)


def test_from_sb3_reads_the_models_hyperparameters(monkeypatch):
    from mujoco_sim_amd import DeviceSAC

    got = {}
    monkeypatch.setattr(DeviceSAC, "_hyperparameters", staticmethod(lambda **kw: got.update(kw) or (_ for _ in ()).throw(ValueError("stop here"))))
    venv = types.SimpleNamespace(device="cpu", action_dim=A, obs_dim=D, num_envs=4)
    with pytest.raises(ValueError, match="stop here"):
        DeviceSAC.from_sb3(venv, _sb3_model(), learning_starts=8)
    assert (got["gamma"], got["tau"], got["batch_size"], got["buffer_size"], got["learning_starts"], got["gradient_steps"], got["target_update_interval"]) == \
        (0.98, 0.02, 32, 1000, 8, -1, 2)
    assert (got["ent_coef"], got["target_entropy"], got["learning_rate"], got["seed"]) == ("auto_0.2", -2.0, 7e-4, 0) and got["train_freq"].frequency == 4
    got.clear()
    with pytest.raises(ValueError, match="stop here"):
        DeviceSAC.from_sb3(venv, _sb3_model(lr_schedule=None, learning_rate=1e-3, target_entropy="auto"))
    assert got["learning_rate"] == 1e-3 and got["target_entropy"] == "auto"


# ---------------------------------------------------------------------------------------------- learn's bookkeeping
class _CountingBuffer:
    autoreset = "next_step"

    def __init__(self, rows=1):
        self.calls, self.rows, self.size_reads = [], rows, 0

    def _open(self):
        pass

    def collect(self, venv, actor, T, generator=None):
        self.calls.append(("collect", T))

    def add_block(self, obs0, block, final_frames=None):
        assert block["squashed_actions"].dtype == torch.float32 and float(block["squashed_actions"].abs().max()) <= 1.0
        self.calls.append(("uniform", int(block["obs"].shape[0])))

    @property
    def size(self):
        self.size_reads += 1
        return self.rows


class _CountingEnv:
    device, num_envs, action_dim, obs_dim, autoreset = "cpu", 8, A, D, "next_step"
    action_low, action_high = (-2.0, 0.0), (2.0, 1.0)

    def __init__(self):
        self.flat_obs = torch.zeros(self.num_envs, D, dtype=torch.float64)
        self.actions = []

    def rollout(self, actions, keep=()):
        T = actions.shape[0]
        assert actions.dtype == torch.float64 and tuple(actions.shape) == (T, self.num_envs, A)
        self.actions.append(actions)
        return {"obs": torch.full((T, self.num_envs, D), float(len(self.actions)), dtype=torch.float64)}


def _bare_trainer(**hp):
    from mujoco_sim_amd import DeviceSAC

    t = DeviceSAC.__new__(DeviceSAC)
    t.__dict__.update(_closed=False, venv=_CountingEnv(), buffer=_CountingBuffer(), actor=None, device=torch.device("cpu"), num_timesteps=0, num_gradient_steps=0,
                      _size_checked=False, trained=[], **hp)
    t._open = lambda: None
    t.train = lambda G, batch_size=None: (t.trained.append(G), setattr(t, "num_gradient_steps", t.num_gradient_steps + G))
    return t


def test_learn_bookkeeping():
    t = _bare_trainer(train_freq=4, gradient_steps=2, learning_starts=64)
    g = torch.Generator().manual_seed(3)
    assert t.learn(128, generator=g) is t
    # 8 envs x 4 steps = 32 env steps per block: uniform while num_timesteps < 64, training once num_timesteps > 64
    assert t.buffer.calls == [("uniform", 4), ("uniform", 4), ("collect", 4), ("collect", 4)]
    assert t.num_timesteps == 128 and t.trained == [2, 2] and t.num_gradient_steps == 4 and t.buffer.size_reads == 1
    a = torch.cat(t.venv.actions)
    assert float(a[..., 0].min()) >= -2.0 and float(a[..., 0].max()) <= 2.0 and float(a[..., 1].min()) >= 0.0 and float(a[..., 1].max()) <= 1.0
    assert float(a[..., 0].std()) > 0.5  # spread over the action space, not a constant
    assert float(t.venv.flat_obs[0, 0]) == 2.0  # the next block starts from the last observation of the warm-up's
    # a second call continues: no warm-up, no second read of the size, whole blocks only
    t.learn(40)
    assert t.num_timesteps == 128 + 64 and t.buffer.calls[4:] == [("collect", 4), ("collect", 4)] and t.trained == [2, 2, 2, 2] and t.buffer.size_reads == 1
    t.learn(0)
    assert t.num_timesteps == 192
    with pytest.raises(ValueError, match="total_timesteps"):
        t.learn(-1)


def test_gradient_steps_minus_one_and_an_empty_buffer():
    from mujoco_sim_amd import MjsError

    t = _bare_trainer(train_freq=3, gradient_steps=-1, learning_starts=0)
    assert t._gradient_steps_per_phase() == 3 * 8
    t.learn(48)
    assert t.buffer.calls == [("collect", 3), ("collect", 3)] and t.trained == [24, 24] and t.num_timesteps == 48
    t = _bare_trainer(train_freq=1, gradient_steps=0, learning_starts=0)
    t.learn(8)
    assert t.trained == [0]
    t = _bare_trainer(train_freq=1, gradient_steps=1, learning_starts=0)
    t.buffer.rows = 0
    with pytest.raises(MjsError, match="empty"):
        t.learn(8)
    assert t.trained == []


def test_same_step_warm_up_needs_terminal_obs():
    t = _bare_trainer(train_freq=1, gradient_steps=1, learning_starts=100)
    t.buffer.autoreset = "same_step"
    with pytest.raises(ValueError, match="terminal_obs"):
        t.learn(8)


def test_train_and_draw_batch_check_their_arguments(stubs):
    from mujoco_sim_amd import DeviceSAC, MjsError

    t = DeviceSAC.__new__(DeviceSAC)
    t.__dict__.update(_closed=True, batch_size=8, num_gradient_steps=0)
    for call, kw, match in ((t.train, dict(gradient_steps=-1), "gradient_steps"), (t.train, dict(gradient_steps=1.5), "gradient_steps"),
                            (t.train, dict(gradient_steps=1, batch_size=0), "batch_size"), (t.draw_batch, dict(step=-1), "step"), (t.draw_batch, dict(step=2**64), "step"),
                            (t.draw_batch, dict(batch_size=0), "batch_size")):
        with pytest.raises(ValueError, match=match):
            call(**kw)
    for call in (lambda: t.train(1), t.draw_batch, lambda: t.learn(8), lambda: t.export_to(_sb3_model())):
        with pytest.raises(MjsError, match="closed"):
            call()
    with pytest.raises(ValueError, match="no attribute 'critic'"):
        t.export_to(types.SimpleNamespace(actor=1, critic=None, critic_target=1))
    t.close()  # closing twice is fine
