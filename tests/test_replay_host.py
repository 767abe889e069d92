"""The replay buffer's host side, without a GPU: the C ABI (declared, exported, struct sizes as stated) and DeviceReplayBuffer's
argument checks, which raise ValueError before the native layer is touched."""
import ctypes as C
import re
from pathlib import Path

import pytest
import torch

ROOT = Path(__file__).resolve().parents[1]
ENTRY_POINTS = ("mjs_replay_workspace_bytes", "mjs_replay_add", "mjs_replay_sample")
SCENE, WRIST = "Camera/rgb_image", "ur5e/Camera/rgb_image"


def test_header_declares_and_library_exports_the_entry_points():
    from mujoco_sim_amd import _native

    header = (ROOT / "include" / "mjsim.h").read_text()
    for name, ret in zip(ENTRY_POINTS, ("uint64_t", "int", "int")):
        assert re.search(rf"^{ret} {name}\(", header, re.M), name
        assert name in _native.EXPORTED_SYMBOLS
    assert re.search(r"^#define MJS_ABI_VERSION 3$", header, re.M)
    _native.build()
    L = C.CDLL(str(_native.LIB_PATH))
    for name in ENTRY_POINTS:
        assert hasattr(L, name), f"libmjsim.so does not export {name}"
    L.mjs_replay_workspace_bytes.restype = C.c_uint64
    L.mjs_replay_workspace_bytes.argtypes = [C.c_int32, C.c_int32]
    assert L.mjs_replay_workspace_bytes(0, 4) == 0 and L.mjs_replay_workspace_bytes(4, 0) == 0
    small, large = L.mjs_replay_workspace_bytes(1, 1), L.mjs_replay_workspace_bytes(200, 4096)
    assert small >= 8 + 4 + 4 and large >= 4 * 200 * 4096 and large % 4 == 0  # the base, a chunk count and every row's ring row


def test_struct_sizes_stated_in_the_header_are_the_bindings():
    from mujoco_sim_amd import _native as nat

    header = (ROOT / "include" / "mjsim.h").read_text()
    for name, binding in (("mjs_replay_storage", nat.MjsReplayStorage), ("mjs_replay_block", nat.MjsReplayBlock), ("mjs_replay_batch", nat.MjsReplayBatch)):
        stated = re.search(rf"\}} {name};\s*/\* (\d+) bytes \*/", header)
        assert stated, name
        assert int(stated.group(1)) == C.sizeof(binding), name
        assert binding().struct_size == C.sizeof(binding)
        body = header[header.rindex("typedef struct {", 0, stated.start()):stated.start()]
        declared = [n for decl in re.findall(r"^\s+(?:const )?\w+\s*\**\s*([^;/]+);", body, re.M) for n in re.findall(r"\b([A-Za-z_]\w*)\b(?:\[\d+\])?", decl)]
        assert declared == [n for n, _ in binding._fields_], name  # the same fields in the same order


class _StubEnv:
    """What DeviceReplayBuffer reads of a HipVectorEnv before it touches the native layer (Button-Push's layout, on the CPU)."""
    device = torch.device("cpu")
    _dev_index = 0
    action_dim = 7
    obs_dim = 13
    autoreset = "next_step"
    camera_keys = (WRIST, SCENE)
    flat_observation_layout = (("ur5e/joint_configuration", 0, 6), ("unnamed_model/position", 9, 3), ("unnamed_model/active", 12, 1))


@pytest.fixture
def no_native(monkeypatch):
    from mujoco_sim_amd import _native as nat

    def touched(*a, **k):
        raise AssertionError("the native layer was touched")

    monkeypatch.setattr(nat, "lib", touched)
    monkeypatch.setattr(nat, "check", touched)


def test_constructor_checks_its_arguments_before_any_native_call(no_native):
    from mujoco_sim_amd import DeviceReplayBuffer

    venv = _StubEnv()
    with pytest.raises(AssertionError, match="native layer"):  # valid arguments reach the (patched) native layer: the checks below stop earlier
        DeviceReplayBuffer(venv, 1000)
    with pytest.raises(AssertionError, match="native layer"):
        DeviceReplayBuffer(venv, 1000, obs_keys=("unnamed_model/position",), cameras=(SCENE, WRIST), image_size=(37, 41))
    with pytest.raises(ValueError, match="unknown observation key"):
        DeviceReplayBuffer(venv, 1000, obs_keys=("ur5e/tcp_position",))
    with pytest.raises(ValueError, match="not both"):
        DeviceReplayBuffer(venv, 1000, obs_keys=("unnamed_model/active",), obs_index=[0])
    with pytest.raises(ValueError, match="obs_index entries"):
        DeviceReplayBuffer(venv, 1000, obs_index=[0, 13])
    with pytest.raises(ValueError, match="at most 64"):
        DeviceReplayBuffer(venv, 1000, obs_index=[0] * 65)
    for capacity in (0, -3, 2**31):
        with pytest.raises(ValueError, match="capacity"):
            DeviceReplayBuffer(venv, capacity)
    with pytest.raises(ValueError, match="unknown camera key"):
        DeviceReplayBuffer(venv, 1000, cameras=("wrist",), image_size=64)
    with pytest.raises(ValueError, match="twice"):
        DeviceReplayBuffer(venv, 1000, cameras=(SCENE, SCENE), image_size=64)
    with pytest.raises(ValueError, match="need an image_size"):
        DeviceReplayBuffer(venv, 1000, cameras=(SCENE,))
    for size in (0, (64, -1), (64, 64, 3), "big"):
        with pytest.raises(ValueError, match="image_size"):
            DeviceReplayBuffer(venv, 1000, cameras=(SCENE,), image_size=size)
    with pytest.raises(ValueError, match="with cameras"):
        DeviceReplayBuffer(venv, 1000, image_size=64)
    venv.autoreset = "disabled"
    with pytest.raises(ValueError, match="disabled"):
        DeviceReplayBuffer(venv, 1000)
    venv.autoreset = "same_step"
    with pytest.raises(ValueError, match="next_step"):
        DeviceReplayBuffer(venv, 1000, cameras=(SCENE,), image_size=64)
    venv.autoreset, venv.action_dim = "next_step", 9
    with pytest.raises(ValueError, match="action components"):
        DeviceReplayBuffer(venv, 1000)


class _TouchedLib:
    def __getattr__(self, name):
        raise AssertionError("the native layer was touched")


@pytest.fixture
def stub_buffers(monkeypatch):
    """Buffers on the CPU stub env whose library raises at the first call: construction allocates, every entry point is native."""
    from mujoco_sim_amd import DeviceReplayBuffer
    from mujoco_sim_amd import _native as nat

    monkeypatch.setattr(nat, "lib", lambda: _TouchedLib())
    monkeypatch.setattr(nat, "check", lambda *a, **k: (_ for _ in ()).throw(AssertionError("the native layer was touched")))

    def make(autoreset="next_step", **kw):
        venv = _StubEnv()
        venv.autoreset = autoreset
        return DeviceReplayBuffer(venv, 1000, **kw)

    return make


def _block(T, N, A=7, src=13, cameras=(), hw=(36, 36), terminal=False):
    blk = {"obs": torch.zeros(T, N, src, dtype=torch.float64), "reward": torch.zeros(T, N, dtype=torch.float64),
           "terminated": torch.zeros(T, N, dtype=torch.uint8), "truncated": torch.zeros(T, N, dtype=torch.uint8),
           "step_type": torch.ones(T, N, dtype=torch.uint8), "squashed_actions": torch.zeros(T, N, A, dtype=torch.float32)}
    if terminal:
        blk["terminal_obs"] = torch.zeros(T, N, src, dtype=torch.float64)
    for k in cameras:
        blk[k] = torch.zeros(T, N, *hw, 3, dtype=torch.uint8)
    return torch.zeros(N, src, dtype=torch.float64), blk, {k: torch.zeros(N, *hw, 3, dtype=torch.uint8) for k in cameras}


def test_add_block_and_sample_check_their_arguments_before_any_native_call(stub_buffers):
    buf = stub_buffers(obs_keys=("unnamed_model/position",))
    assert buf.obs_index == [9, 10, 11] and buf.obs.shape == (1000, 3) and buf.actions.shape == (1000, 7) and buf.timeouts.dtype == torch.uint8
    T, N = 4, 5
    obs0, blk, _ = _block(T, N)
    with pytest.raises(AssertionError, match="native layer"):  # a well-formed block reaches the native layer
        buf.add_block(obs0, blk)
    buf.add_block(*_block(0, N)[:2])  # an empty block: nothing to launch
    bad = [
        ("dtype", obs0.float(), blk, "torch.float64"),
        ("shape", obs0[:, :12].contiguous(), blk, "shape"),
        ("device", obs0.to("meta"), blk, "lives on"),
        ("contiguity", torch.zeros(13, N, dtype=torch.float64).t(), blk, "contiguous"),
        ("not a tensor", obs0.numpy(), blk, "tensor"),
        ("no dict", obs0, blk["obs"], "dict"),
        ("obs rank", obs0, {**blk, "obs": blk["obs"][0]}, r"\[T, N, obs_dim\]"),
        ("reward dtype", obs0, {**blk, "reward": blk["reward"].float()}, "torch.float64"),
        ("flags dtype", obs0, {**blk, "terminated": blk["terminated"].bool()}, "torch.uint8"),
        ("step_type shape", obs0, {**blk, "step_type": blk["step_type"][:, :4].contiguous()}, "shape"),
        ("step_type missing", obs0, {k: v for k, v in blk.items() if k != "step_type"}, "no 'step_type'"),
        ("actions dtype", obs0, {**blk, "squashed_actions": blk["squashed_actions"].double()}, "torch.float32"),
        ("actions width", obs0, {**blk, "squashed_actions": blk["squashed_actions"][..., :3].contiguous()}, "shape"),
        ("too many rows", *_block(201, N)[:2], "capacity"),
    ]
    for what, o, b, match in bad:
        with pytest.raises(ValueError, match=match):
            buf.add_block(o, b)
            pytest.fail(what)
    # same-step auto-reset needs the terminal observations
    same = stub_buffers(autoreset="same_step")
    with pytest.raises(ValueError, match="terminal_obs"):
        same.add_block(obs0, blk)
    with pytest.raises(AssertionError, match="native layer"):
        same.add_block(*_block(T, N, terminal=True)[:2])
    # cameras: the frames of every camera, and the frames after the block
    cams = stub_buffers(cameras=(SCENE, WRIST), image_size=(37, 41))
    assert cams.rgb[WRIST].shape == (1000, 37, 41, 3) and cams.next_rgb[SCENE].dtype == torch.uint8
    o, b, final = _block(T, N, cameras=(SCENE, WRIST), hw=(37, 41))
    with pytest.raises(AssertionError, match="native layer"):
        cams.add_block(o, b, final)
    with pytest.raises(ValueError, match="final_frames has no"):
        cams.add_block(o, b, {SCENE: final[SCENE]})
    with pytest.raises(ValueError, match="block has no"):
        cams.add_block(o, {k: v for k, v in b.items() if k != WRIST}, final)
    with pytest.raises(ValueError, match="shape"):
        cams.add_block(o, {**b, SCENE: torch.zeros(T, N, 41, 37, 3, dtype=torch.uint8)}, final)
    with pytest.raises(ValueError, match="torch.uint8"):
        cams.add_block(o, b, {**final, WRIST: final[WRIST].float()})
    # sample
    with pytest.raises(AssertionError, match="native layer"):
        buf.sample(8, draws=torch.zeros(8, dtype=torch.int64))
    assert buf.sample(0)["actions"].shape == (0, 7)
    with pytest.raises(ValueError, match="negative"):
        buf.sample(-1)
    with pytest.raises(ValueError, match="torch.int64"):
        buf.sample(8, draws=torch.zeros(8, dtype=torch.int32))
    with pytest.raises(ValueError, match="shape"):
        buf.sample(8, draws=torch.zeros(9, dtype=torch.int64))
    # collect refuses an env the buffer was not made for before it runs anything
    other = _StubEnv()
    other.autoreset = "same_step"
    with pytest.raises(ValueError, match="autoreset"):
        buf.collect(other, None, 4)
    other.autoreset, other.obs_dim = "next_step", 12
    with pytest.raises(ValueError, match="observation and"):
        buf.collect(other, None, 4)
    buf.close()
    from mujoco_sim_amd import MjsError

    with pytest.raises(MjsError, match="closed"):
        buf.sample(1)
