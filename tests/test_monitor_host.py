"""Episode statistics and evaluation, without a GPU: the C ABI (declared, exported, struct sizes as stated), the numpy restatement of the
rules against a hand-worked block, SB3's per-env episode targets, and every ValueError of DeviceEpisodeMonitor, evaluate_policy and
DeviceSAC.learn's reporting arguments before the native layer is touched."""
import ctypes as C
import inspect
import re
import types
from pathlib import Path

import numpy as np
import pytest
import torch

import _monitor_reference as mref
from _monitor_reference import FIRST, LAST, MID

ROOT = Path(__file__).resolve().parents[1]
ENTRY_POINTS = (("mjs_monitor_workspace_bytes", "uint64_t"), ("mjs_monitor_update", "int"), ("mjs_monitor_summary", "int"))


def test_the_monitor_is_new():
    """The test that fails without the feature: the module and the package's exports."""
    import mujoco_sim_amd as m
    from mujoco_sim_amd.monitor import DeviceEpisodeMonitor, evaluate_policy

    assert m.DeviceEpisodeMonitor is DeviceEpisodeMonitor and m.evaluate_policy is evaluate_policy


# ---------------------------------------------------------------------------------------------- the C ABI
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
    for name, binding, size in (("mjs_monitor_state", nat.MjsMonitorState, 96), ("mjs_monitor_block", nat.MjsMonitorBlock, 56)):
        stated = re.search(rf"\}} {name};\s*/\* (\d+) bytes \*/", header)
        assert stated, name
        assert int(stated.group(1)) == C.sizeof(binding) == size, name
        assert binding().struct_size == C.sizeof(binding)
        body = header[header.rindex("typedef struct {", 0, stated.start()):stated.start()]
        declared = re.findall(r"^\s+(?:const )?\w+\s*\**\s*(\w+)(?:\[\d+\])*;", body, re.M)
        assert declared == [n for n, _ in binding._fields_], name  # the same fields in the same order
    # the summary's slots: the enum in the header is the binding's tuple, in order
    slots = re.findall(r"^\s+MJS_MONITOR_(\w+) = (\d+),?", header, re.M)
    assert [s.lower() for s, _ in slots[:-1]] == list(nat.MONITOR_SUMMARY_FIELDS) and [int(i) for _, i in slots] == list(range(len(slots)))
    assert slots[-1] == ("SUMMARY", str(len(nat.MONITOR_SUMMARY_FIELDS)))


# ---------------------------------------------------------------------------------------------- the restatement
def _worked_block():
    return {"reward": np.array([[1.0, 0.5], [2.0, -1.0], [4.0, 8.0]]),
            "step_type": np.array([[MID, FIRST], [LAST, MID], [FIRST, LAST]], np.uint8),
            "terminated": np.array([[0, 0], [1, 0], [0, 0]], np.uint8),
            "truncated": np.array([[0, 0], [0, 0], [0, 1]], np.uint8),
            "is_success": np.array([[0, 0], [1, 0], [0, 0]], np.uint8)}


def test_reference_reproduces_a_hand_worked_block():
    """3 steps x 2 envs. Env 0 carries an episode of return 10 over 3 steps into the block.

    next-step: env 0 adds 1 and 2 (return 13, length 5), terminates with success on t = 1, and its FIRST row on t = 2 (reward 4) is ignored;
    env 1's FIRST row on t = 0 (reward 0.5) is ignored, it adds -1 and 8 (return 7, length 2) and is truncated on t = 2.
    The records enter in (t, n) order: (t 1, env 0) before (t 2, env 1).
    same-step (step_type plays no role): env 0 as before, then a new episode holds the 4 of t = 2; env 1 adds 0.5 - 1 + 8 = 7.5 over 3."""
    ref = mref.RefMonitor(2, window=4)
    ref.ep_return[0], ref.ep_length[0] = 10.0, 3
    assert ref.update(_worked_block(), "next_step") == 2 and ref.cursor == 2
    assert ref.ring_return.tolist() == [13.0, 7.0, 0.0, 0.0] and ref.ring_length.tolist() == [5, 2, 0, 0]
    assert ref.ring_success.tolist() == [1, 0, 0, 0] and ref.ring_terminated.tolist() == [1, 0, 0, 0] and ref.ring_env.tolist() == [0, 1, 0, 0]
    assert ref.ep_return.tolist() == [0.0, 0.0] and ref.ep_length.tolist() == [0, 0] and ref.ep_count.tolist() == [1, 1]
    ref = mref.RefMonitor(2, window=4)
    ref.ep_return[0], ref.ep_length[0] = 10.0, 3
    assert ref.update(_worked_block(), "same_step") == 2
    assert ref.ring_return.tolist() == [13.0, 7.5, 0.0, 0.0] and ref.ring_length.tolist() == [5, 3, 0, 0] and ref.ring_env.tolist() == [0, 1, 0, 0]
    assert ref.ep_return.tolist() == [4.0, 0.0] and ref.ep_length.tolist() == [1, 0]
    # a quota of 0 for env 0: its episode is not recorded, its accumulators reset all the same; the ring wraps at the window
    ref = mref.RefMonitor(2, window=1, quota=[0, 5])
    ref.ep_return[0], ref.ep_length[0] = 10.0, 3
    assert ref.update(_worked_block(), "same_step") == 1 and ref.cursor == 1 and ref.ring_return.tolist() == [7.5] and ref.ring_env.tolist() == [1]
    assert ref.ep_return.tolist() == [4.0, 0.0] and ref.ep_count.tolist() == [0, 1] and ref.remaining() == 4
    ret, length, success, terminated, env = ref.live()
    assert ret.tolist() == [7.5] and length.tolist() == [3] and success.tolist() == [0] and terminated.tolist() == [0] and env.tolist() == [1]


def test_std_exact_is_the_population_value():
    x = [1.0, 2.0, 4.0, 7.0]
    assert mref.std_exact(x) == pytest.approx(np.std(x), rel=1e-15) and mref.std_exact([3.5]) == 0.0


@pytest.mark.parametrize("n_eval,N", [(1, 1), (5, 8), (11, 8), (8, 8)])
def test_episode_targets_are_sb3s(n_eval, N):
    from mujoco_sim_amd.monitor import episode_targets

    got = episode_targets(n_eval, N)
    assert got == mref.sb3_targets(n_eval, N).tolist() and sum(got) == n_eval and all(isinstance(q, int) for q in got)


# ---------------------------------------------------------------------------------------------- argument checks
class _TouchedLib:
    def __getattr__(self, name):
        raise AssertionError("the native layer was touched")


def test_constructor_checks_its_arguments_before_any_native_call(monkeypatch):
    from mujoco_sim_amd import DeviceEpisodeMonitor
    from mujoco_sim_amd import _native as nat

    monkeypatch.setattr(nat, "lib", lambda: (_ for _ in ()).throw(AssertionError("the native layer was touched")))
    venv = types.SimpleNamespace(num_envs=4, device="cuda:0", autoreset="same_step")
    with pytest.raises(AssertionError, match="native layer"):  # valid arguments reach the (stubbed) native layer
        DeviceEpisodeMonitor(venv, window=7, quota=[1, 0, 2, 3])
    with pytest.raises(AssertionError, match="native layer"):
        DeviceEpisodeMonitor(4, device="cuda:0")
    for args, kw, match in (((0,), {}, "num_envs"), ((-3,), {}, "num_envs"), ((2.5,), {}, "venv_or_num_envs"), ((True,), {}, "venv_or_num_envs"),
                            ((venv,), dict(window=0), "window"), ((venv,), dict(window=1.5), "window"), ((venv,), dict(window=2**31), "window"),
                            ((venv,), dict(quota=[1, 2, 3]), "quota"), ((venv,), dict(quota=[1, 2, 3, -1]), "quota"), ((venv,), dict(quota=5), "quota"),
                            ((venv,), dict(quota=["a"] * 4), "quota"), ((venv,), dict(device="cuda:1"), "device"), ((4,), dict(device="cpu"), "device"),
                            ((types.SimpleNamespace(num_envs=0, device="cuda:0"),), {}, "num_envs")):
        with pytest.raises(ValueError, match=match):
            DeviceEpisodeMonitor(*args, **kw)


def _stub_monitor(**attrs):
    from mujoco_sim_amd import DeviceEpisodeMonitor

    mon = DeviceEpisodeMonitor.__new__(DeviceEpisodeMonitor)
    mon.__dict__.update(_lib=_TouchedLib(), device=torch.device("cpu"), num_envs=2, window=4, autoreset="next_step", quota=None, _workspace=None, **attrs)
    return mon


def _torch_block(T=3, N=2):
    return {"reward": torch.zeros(T, N, dtype=torch.float64), **{k: torch.zeros(T, N, dtype=torch.uint8) for k in ("terminated", "truncated", "is_success", "step_type")}}


def test_update_checks_its_block_before_any_native_call():
    from mujoco_sim_amd import MjsError

    mon = _stub_monitor()
    with pytest.raises(AssertionError, match="native layer"):  # a good block reaches the (stubbed) native layer
        mon.update(_torch_block())
    mon.update(_torch_block(T=0))  # an empty block needs nothing native
    bad = [("reward", lambda t: t.float(), r"block\['reward'\] must be torch.float64"), ("reward", lambda t: t[:, :1], r"block\['reward'\] must have shape"),
           ("reward", lambda t: t.to("meta"), r"block\['reward'\] lives on"), ("reward", lambda t: t.t().contiguous().t(), r"block\['reward'\] must be contiguous"),
           ("reward", lambda t: None, "block must be a dict"), ("reward", lambda t: t[0], "block must be a dict"),
           ("terminated", lambda t: t.bool(), r"block\['terminated'\] must be torch.uint8"), ("truncated", lambda t: t[:2], r"block\['truncated'\] must have shape"),
           ("is_success", lambda t: None, "block has no 'is_success'"), ("is_success", lambda t: t.double(), r"block\['is_success'\]"),
           ("step_type", lambda t: None, "block has no 'step_type'"), ("step_type", lambda t: t.to("meta"), r"block\['step_type'\] lives on"),
           ("terminated", lambda t: t.numpy(), r"block\['terminated'\] must be a tensor")]
    for key, change, match in bad:
        blk = _torch_block()
        blk[key] = change(blk[key])
        with pytest.raises(ValueError, match=match):
            mon.update(blk)
    with pytest.raises(ValueError, match="block must be a dict"):
        mon.update([torch.zeros(3, 2)])
    with pytest.raises(ValueError, match="autoreset"):
        mon.update(_torch_block(), autoreset="disabled")
    with pytest.raises(ValueError, match="autoreset"):
        mon.update(_torch_block(), autoreset="sometimes")
    blk = _torch_block()
    del blk["step_type"]  # same-step auto-reset needs no step_type
    with pytest.raises(AssertionError, match="native layer"):
        mon.update(blk, autoreset="same_step")
    with pytest.raises(ValueError, match="autoreset must be given"):
        _with(_stub_monitor(), autoreset=None).update(_torch_block())  # a monitor made from an env count
    with pytest.raises(ValueError, match="quota"):
        mon.remaining()
    mon._lib = None
    for call in (lambda: mon.update(_torch_block()), mon.summary, mon.episodes, mon.remaining, mon.reset, mon.reset_in_flight):
        with pytest.raises(MjsError, match="closed"):
            call()
    mon.close()  # closing twice is fine


def _with(obj, **attrs):
    obj.__dict__.update(attrs)
    return obj


def test_evaluate_policy_checks_its_arguments_before_any_native_call():
    from mujoco_sim_amd import evaluate_policy

    def touched(*a, **kw):
        raise AssertionError("the native layer was touched")

    venv = types.SimpleNamespace(num_envs=8, device="cuda:0", autoreset="next_step", reset=touched, actor_rollout=touched)
    with pytest.raises(AssertionError, match="native layer"):  # valid arguments reach the env
        evaluate_policy(venv, object(), n_eval_episodes=11, block_steps=16)
    for kw, match in ((dict(n_eval_episodes=0), "n_eval_episodes"), (dict(n_eval_episodes=2.5), "n_eval_episodes"), (dict(block_steps=0), "block_steps"),
                      (dict(block_steps="many"), "block_steps"), (dict(max_steps=0), "max_steps"), (dict(max_steps=1.5), "max_steps")):
        with pytest.raises(ValueError, match=match):
            evaluate_policy(venv, object(), **kw)
    venv.autoreset = "disabled"
    with pytest.raises(ValueError, match="autoreset"):
        evaluate_policy(venv, object())


def test_learns_new_keywords_default_to_off_and_are_checked_before_anything_native():
    from mujoco_sim_amd import DeviceEpisodeMonitor, DeviceSAC, MjsError

    params = inspect.signature(DeviceSAC.learn).parameters
    assert list(params) == ["self", "total_timesteps", "generator", "monitor", "log_interval", "eval_env", "eval_freq", "n_eval_episodes", "callback"]
    for name in ("monitor", "log_interval", "eval_env", "eval_freq", "callback"):
        assert params[name].default is None and params[name].kind is inspect.Parameter.KEYWORD_ONLY, name
    assert params["n_eval_episodes"].default == 5

    t = DeviceSAC.__new__(DeviceSAC)
    venv = types.SimpleNamespace(num_envs=2, device="cpu", autoreset="next_step", reset=None, actor_rollout=None)
    t.__dict__.update(_closed=True, venv=venv, device=torch.device("cpu"))
    mon = _stub_monitor()
    good = dict(monitor=mon, log_interval=2, eval_env=venv, eval_freq=100, n_eval_episodes=3, callback=print)
    with pytest.raises(MjsError, match="closed"):  # valid arguments pass the checks (and the closed trainer stops before anything native)
        t.learn(8, **good)
    other = types.SimpleNamespace(num_envs=2, device="meta", autoreset="next_step", reset=None, actor_rollout=None)
    disabled = types.SimpleNamespace(num_envs=2, device="cpu", autoreset="disabled", reset=None, actor_rollout=None)
    for change, match in ((dict(monitor=object()), "monitor must be a DeviceEpisodeMonitor"), (dict(monitor=_with(_stub_monitor(), num_envs=3)), "monitor was made for"),
                          (dict(monitor=_with(_stub_monitor(), device=torch.device("meta"))), "monitor lives on"), (dict(log_interval=0), "log_interval"),
                          (dict(log_interval=1.5), "log_interval"), (dict(monitor=None), "log_interval needs a monitor"), (dict(eval_env=None), "eval_env and eval_freq"),
                          (dict(eval_freq=None), "eval_env and eval_freq"), (dict(eval_freq=0), "eval_freq"), (dict(eval_freq="often"), "eval_freq"),
                          (dict(n_eval_episodes=0), "n_eval_episodes"), (dict(eval_env=object()), "eval_env must be a HipVectorEnv"),
                          (dict(eval_env=other), "eval_env lives on"), (dict(eval_env=disabled), "eval_env runs autoreset"), (dict(callback=3), "callback must be callable")):
        with pytest.raises(ValueError, match=match):
            t.learn(8, **{**good, **change})
    with pytest.raises(ValueError, match="callback"):
        t.learn(8, callback=print)
    with pytest.raises(MjsError, match="closed"):  # a monitor alone (no records) is fine
        t.learn(8, monitor=mon)
    assert isinstance(mon, DeviceEpisodeMonitor)
