"""What the encoder-training work promises without a device: the entry points are declared and bound, the Python classes check their
arguments before anything native, the split / workspace rule restated in _encoder_train_reference.py is self-consistent, torch
float32's own masks stay inside the mask condition for every case, and a float32 evaluation with the kernel's summation shape meets
the gradient bar (so the bar is known to be reachable before the device sees it)."""
import ctypes as C
import re
from pathlib import Path

import numpy as np
import pytest
import torch

import _encoder_train_reference as R
from _visual_nets import NatureCNNStandIn

ROOT = Path(__file__).resolve().parents[1]
NEW_SYMBOLS = ("mjs_encoder_opt_create", "mjs_encoder_opt_destroy", "mjs_encoder_train_workspace_bytes", "mjs_encoder_grad", "mjs_encoder_update",
               "mjs_encoder_blend", "mjs_encoder_export")


def test_header_declares_and_library_exports_the_new_entry_points():
    from mujoco_sim_amd import _native as nat

    nat.build()
    header = (ROOT / "include" / "mjsim.h").read_text()
    L = C.CDLL(str(nat.LIB_PATH))
    for name in NEW_SYMBOLS:
        assert re.search(rf"\b{name}\s*\(", header), name
        assert name in nat.EXPORTED_SYMBOLS and hasattr(L, name), name
    assert "#define MJS_ABI_VERSION 3" in header  # entry points added after abi 3 leave the number alone


def test_binding_struct_sizes_are_the_header_s():
    import mujoco_sim_amd as m
    from mujoco_sim_amd import _native as nat

    header = (ROOT / "include" / "mjsim.h").read_text()
    for c_name, binding in (("mjs_encoder_opt_desc", nat.MjsEncoderOptDesc), ("mjs_encoder_grad_args", nat.MjsEncoderGradArgs)):
        stated = re.search(rf"\}}\s*{c_name};\s*/\*\s*(\d+) bytes\s*\*/", header)
        assert stated, c_name
        assert int(stated.group(1)) == C.sizeof(binding), c_name
        assert binding().struct_size == C.sizeof(binding)
    assert C.sizeof(nat.MjsEncoderOptDesc) == C.sizeof(nat.MjsCriticOptDesc)  # the critic optimiser's fields
    assert nat.MjsEncoderGradArgs.grads_out.offset == 40 and nat.MjsEncoderGradArgs.activations_out_dev.offset == 48
    assert hasattr(m, "DeviceEncoderOptimizer")


class _StubEnv:
    device = torch.device("cpu")
    _dev_index = 0


def _fake_encoder(H=36, W=36, F=16):
    """A DeviceEncoder as the optimiser's argument checks see it, made without the native layer (its handle is a stand-in)."""
    from mujoco_sim_amd import DeviceEncoder

    cnn = NatureCNNStandIn(H, W, F)
    e = object.__new__(DeviceEncoder)
    e._e, e.features_dim, e.height, e.width, e.device = None, F, H, W, torch.device("cpu")
    e.convs, e.fc, e.flat_dim = [cnn.cnn[0], cnn.cnn[2], cnn.cnn[4]], cnn.linear[0], int(cnn.linear[0].in_features)
    return e


def _fake_optimizer(enc):
    from mujoco_sim_amd import DeviceEncoderOptimizer

    o = object.__new__(DeviceEncoderOptimizer)
    o._o, o.encoder, o.device, o.lr, o.step_count = None, enc, enc.device, 3e-4, 0
    return o


@pytest.fixture
def no_native(monkeypatch):
    from mujoco_sim_amd import _native as nat

    def touched(*a, **k):
        raise AssertionError("the native layer was touched")

    monkeypatch.setattr(nat, "lib", touched)
    monkeypatch.setattr(nat, "check", touched)


def test_optimizer_checks_its_arguments_before_any_native_call(no_native):
    from mujoco_sim_amd import DeviceEncoderOptimizer
    from mujoco_sim_amd import _native as nat

    enc = _fake_encoder()
    with pytest.raises(ValueError, match="DeviceEncoder"):
        DeviceEncoderOptimizer(torch.nn.Linear(3, 3))
    for kw, what in ((dict(lr=-1.0), "lr"), (dict(lr="fast"), "lr"), (dict(betas=(0.9, 1.0)), "betas"), (dict(betas=0.9), "betas"), (dict(eps=0.0), "eps")):
        with pytest.raises(ValueError, match=what):
            DeviceEncoderOptimizer(enc, **kw)
    with pytest.raises(nat.MjsError, match="closed"):  # valid settings reach the encoder's (absent) handle
        DeviceEncoderOptimizer(enc)
    opt = _fake_optimizer(enc)
    images, dfeat = torch.zeros(4, 36, 36, 3, dtype=torch.uint8), torch.zeros(4, 16)
    for call in (opt.step, opt.gradients):
        with pytest.raises(nat.MjsError, match="closed"):  # valid tensors pass the checks
            call(images, dfeat)
        for bad in (images.float(), images[:, :35], images.permute(0, 2, 1, 3)[:, :, :, :], images[:, :, :, :2], torch.zeros(4, 36, 36, 6, dtype=torch.uint8)[..., ::2],
                    images.to("meta"), "images"):
            with pytest.raises(ValueError, match="images"):
                call(bad, dfeat)
        for bad in (dfeat.double(), dfeat[:3], torch.zeros(4, 17), torch.zeros(4, 32)[:, ::2], dfeat.to("meta"), None):
            with pytest.raises(ValueError, match="dfeatures"):
                call(images, bad)
    with pytest.raises(ValueError, match="lr"):
        opt.step(images, dfeat, lr=-1e-3)


def test_export_and_blend_check_their_arguments_before_any_native_call(no_native):
    from mujoco_sim_amd import _native as nat

    enc = _fake_encoder()
    nn = torch.nn
    good = NatureCNNStandIn(36, 36, 16)
    mods = lambda **swap: tuple({**dict(conv1=good.cnn[0], conv2=good.cnn[2], conv3=good.cnn[4], fc=good.linear[0]), **swap}.values())  # noqa: E731
    with pytest.raises(nat.MjsError, match="closed"):  # valid modules (its own, or given) pass the checks
        enc.export()
    with pytest.raises(nat.MjsError, match="closed"):
        enc.export(mods())
    with pytest.raises(ValueError, match="modules must be"):
        enc.export(good)
    with pytest.raises(ValueError, match="not a Conv2d"):
        enc.export(mods(conv2=nn.ReLU()))
    with pytest.raises(ValueError, match="conv1: weight"):
        enc.export(mods(conv1=nn.Conv2d(3, 32, 7, 4)))
    with pytest.raises(ValueError, match="float32"):
        enc.export(mods(conv3=nn.Conv2d(64, 64, 3, 1).double()))
    with pytest.raises(ValueError, match="live on"):
        enc.export(mods(fc=nn.Linear(64, 16, device="meta")))
    with pytest.raises(ValueError, match="fc: weight"):
        enc.export(mods(fc=nn.Linear(64, 17)))
    with pytest.raises(ValueError, match="not a Linear"):
        enc.export(mods(fc=nn.ReLU()))
    with pytest.raises(ValueError, match="DeviceEncoder"):
        enc.blend_from(good, 0.5)
    for tau in (0.0, 1.5, -1.0):
        with pytest.raises(ValueError, match="tau"):
            enc.blend_from(_fake_encoder(), tau)
    with pytest.raises(ValueError, match="shape"):
        enc.blend_from(_fake_encoder(44, 44, 16), 0.5)
    with pytest.raises(ValueError, match="shape"):
        enc.blend_from(_fake_encoder(36, 36, 17), 0.5)
    other = _fake_encoder()
    other.device = torch.device("meta")
    with pytest.raises(ValueError, match="lives on"):
        enc.blend_from(other, 0.5)
    with pytest.raises(nat.MjsError, match="closed"):
        enc.blend_from(_fake_encoder(), 0.5)


def test_existing_refusals_of_visual_actors_stay():
    src = (ROOT / "mujoco_sim_amd" / "policies.py").read_text() + (ROOT / "mujoco_sim_amd" / "sac.py").read_text()
    assert src.count("a visual actor: its update is not built") >= 2


def test_split_and_workspace_rule_is_self_consistent():
    header = (ROOT / "include" / "mjsim.h").read_text()
    assert "splits_max = min(64, max(1, 128 MiB / (4 * slab)))" in header and "images_per_split = ceil(n / splits_max)" in header
    assert R.slab_floats(64, 64, 256) == 6144 + 32 + 32768 + 64 + 36864 + 64 + 1024 * 256 + 256 + 4
    assert R.slab_floats(36, 52, 40) == 6144 + 32 + 32768 + 64 + 36864 + 64 + 192 * 64 + 64 + 4  # F = 40 is padded to 64
    assert R.splits_max(96, 96, 512) == 15 and R.splits_max(64, 64, 256) == 64  # the byte cap binds for the largest encoder only
    for H, W, F in R.SHAPES + [(96, 96, 512)]:
        cap = R.splits_max(H, W, F)
        assert 1 <= cap <= R.MAX_SPLITS and cap * 4 * R.slab_floats(H, W, F) <= R.SLAB_CAP
        for n in (1, 2, 16, 17, 33, cap, cap + 1, 2 * cap, 2 * cap + 1, 256, 1000):
            ips, splits = R.split_rule(n, H, W, F)
            assert 1 <= splits <= cap and ips * (splits - 1) < n <= ips * splits  # every split owns at least one image, together all
            assert (ips == 1) == (n <= cap)
            assert R.workspace_bytes(n, H, W, F) % 16 == 0 and R.workspace_bytes(n, H, W, F) > 4 * splits * R.slab_floats(H, W, F)
        assert R.split_rule(R.multi_n(H, W, F), H, W, F) == (2, (cap + 2) // 2) and (cap + 2) // 2 > 1
    case = R.CASES[-1]
    assert case[3] == "multi" and R.resolve_n(case) == 65 and R.split_rule(65, *case[:3]) == (2, 33)
    assert len(R.CASES) == 13 and len({R.case_seed(c) for c in R.CASES}) == 13


@pytest.mark.parametrize("index", range(len(R.CASES)), ids=[R.case_id(c) for c in R.CASES])
def test_float32_masks_and_slab_sums_meet_the_conditions_on_the_cpu(index):
    case = R.CASES[index]
    H, W, F, _ = case
    n = R.resolve_n(case)
    cnn, images, pre64, pre32 = R.forward_references(index)
    masks32 = R.masks_of_pre(pre32)
    R.check_masks(R.case_id(case), masks32, pre64, pre32)  # torch float32's own masks stay inside the condition
    dfeat = R.make_dfeatures(case)
    ref64, f64 = R.masked_backward(cnn, images, dfeat, masks32, torch.float64)
    ref32, f32 = R.masked_backward(cnn, images, dfeat, masks32, torch.float32)
    assert torch.equal(f32, torch.relu(pre32[3]))  # the masked network IS the ReLU network under its own masks
    slabs = R.masked_backward_slabs32(cnn, images, dfeat, masks32, R.split_rule(n, H, W, F)[0])
    R.check_grads(R.case_id(case) + " slabs in order", slabs, ref64, ref32)
    assert max(w.abs().max().item() for w, _ in ref64) > 1e-3


def test_regression_reference_learns():
    l64, d32 = R.regression_references()
    print(f"regression reference: loss {l64[0]:.4f} -> {l64[-1]:.4f}, d32 {d32:.3e}")
    assert len(l64) == R.REG["steps"] and l64[-1] < 0.5 * l64[0] and 0 < d32 < 1e-2
    assert np.isfinite(l64).all()
