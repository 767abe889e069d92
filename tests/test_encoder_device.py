"""The NatureCNN encoder on the device (csrc/mjs_encoder.h, mujoco_sim_amd.policies.DeviceEncoder) against torch on the CPU, its
index map by a known answer, and the argument checks of the encoder and of the visual DeviceActor.

Bar. The kernels are float32 with float32 accumulation (fmaf chains on the f32-input MFMA, starting at the bias); torch's float32
forward is another float32 accumulation of the same lengths (k = 192, 512, 576, n_flatten) in another order. Both are compared with the
float64 forward of the same modules on the same float32 input x = uint8 / 255: e32 = max |ref32 - ref64| is measured, the bar is
max(4 e32, 8 * 2^-24 * max(1, max |ref64|)) - test_actor_device.py's, the floor scaled because features are not bounded by 1.
"""
import ctypes as C
import re
from pathlib import Path

import numpy as np
import pytest
import torch

from _visual_nets import SCENE, WRIST, CombinedExtractorStandIn, NatureCNNStandIn, SacActorStandIn, cnn_forward, encoder_bar, final_size, make_cnn, make_mlp

gpu = pytest.mark.gpu
ROOT = Path(__file__).resolve().parents[1]
SHAPES = [(36, 36, 256), (44, 44, 40), (36, 52, 256), (64, 64, 256)]  # conv3 output 1x1, 2x2, 1x3, 4x4
NEW_SYMBOLS = ("mjs_encoder_create", "mjs_encoder_destroy", "mjs_encoder_load", "mjs_encoder_flat_dim", "mjs_encoder_workspace_bytes", "mjs_encoder_features",
               "mjs_actor_create_visual", "mjs_actor_actions_visual", "mjs_rollout_visual_actor")


@pytest.fixture(scope="module")
def venv():
    """One seeded, reset Robot-Reach handle of 19 envs: the source of real frames, and the device the encoders live on."""
    import mujoco_sim_amd as m

    v = m.HipVectorEnv("robot_reach", 19, seed=7)
    v.reset()
    yield v
    v.close()


def frames(venv, H, W, n):
    """n real renders and n random images, uint8 [2, n, H, W, 3]."""
    g = torch.Generator(device="cpu").manual_seed(H * 100 + W)
    noise = torch.randint(0, 256, (n, H, W, 3), dtype=torch.uint8, generator=g).to(venv.device)
    return torch.stack([venv.render(H, W)[:n].contiguous(), noise])


# ---------------------------------------------------------------------------------------------- 1. against torch
@gpu
@pytest.mark.parametrize("N", [5, 19])
@pytest.mark.parametrize("H,W,F", SHAPES, ids=lambda v: str(v))
def test_encoder_matches_torch(venv, H, W, F, N):
    from mujoco_sim_amd import DeviceEncoder

    cnn = make_cnn(H, W, F, seed=H + W + F, device=venv.device)
    enc = DeviceEncoder.from_sb3(venv, cnn, H, W)
    h3, w3 = final_size(H, W)
    assert enc.flat_dim == 64 * h3 * w3 and enc.features_dim == F
    for what, images in zip(("render", "random"), frames(venv, H, W, N)):
        out = enc.features(images)
        assert out.shape == (N, F) and out.dtype == torch.float32
        ref64, ref32 = cnn_forward(cnn, images, torch.float64), cnn_forward(cnn, images, torch.float32)
        e32, bar = encoder_bar(ref64, ref32)
        err = (out.cpu().double() - ref64).abs().max().item()
        print(f"{H}x{W} F={F} N={N} {what}: kernel vs float64 {err:.3e}, torch float32 vs float64 {e32:.3e}, bar {bar:.3e}, ratio to e32 {err / max(e32, 1e-300):.2f}")
        assert err <= bar, (what, err, e32)
        assert ref64.abs().max().item() > 1e-3  # the features are not all cut off by the ReLUs
    enc.close()


# ---------------------------------------------------------------------------------------------- 2. the index map
@gpu
def test_index_map_known_answer(venv):
    from mujoco_sim_amd import DeviceEncoder

    H = W = 44
    N, F = 5, 4
    cnn = make_cnn(H, W, F, seed=1, device=venv.device)
    c1, c2, c3, fc = cnn.cnn[0], cnn.cnn[2], cnn.cnn[4], cnn.linear[0]
    tap1, tap2, tap3 = (1, 2, 5), (1, 3), (2, 0)  # conv1 (c, ky, kx), conv2 (ky, kx), conv3 (ky, kx)
    with torch.no_grad():
        for m in (c1, c2, c3, fc):
            m.weight.zero_()
            m.bias.zero_()
        c1.weight[0, tap1[0], tap1[1], tap1[2]] = 1.0
        c2.weight[0, 0, tap2[0], tap2[1]] = 1.0
        c3.weight[0, 0, tap3[0], tap3[1]] = 1.0
        for f in range(F):
            fc.weight[f, f] = 1.0
    enc = DeviceEncoder.from_sb3(venv, cnn, H, W)
    images = frames(venv, H, W, N)[1]  # random bytes: neighbouring pixels differ
    out = enc.features(images).cpu().numpy()
    h3, w3 = final_size(H, W)
    assert (h3, w3) == (2, 2)
    rgb = images.cpu().numpy()
    for y3 in range(h3):
        for x3 in range(w3):
            y2, x2 = y3 * c3.stride[0] + tap3[0], x3 * c3.stride[1] + tap3[1]
            y1, x1 = y2 * c2.stride[0] + tap2[0], x2 * c2.stride[1] + tap2[1]
            y, x = y1 * c1.stride[0] + tap1[1], x1 * c1.stride[1] + tap1[2]
            assert (y, x) == (4 * (2 * (y3 + 2) + 1) + 2, 4 * (2 * (x3 + 0) + 3) + 5)
            want = rgb[:, y, x, tap1[0]].astype(np.float32) / np.float32(255.0)
            got = out[:, y3 * w3 + x3]  # channel 0 of the CHW flatten
            assert (np.abs(got - want) <= np.spacing(np.maximum(want, np.float32(2.0 ** -126)))).all(), (y3, x3, got, want)
    assert len(np.unique(out)) > 4
    enc.close()


# ---------------------------------------------------------------------------------------------- 3. tile independence
@gpu
@pytest.mark.parametrize("H,W,F", [(44, 44, 40), (64, 64, 256)], ids=lambda v: str(v))
def test_rows_are_independent_of_their_tile(venv, H, W, F):
    from mujoco_sim_amd import DeviceEncoder

    cnn = make_cnn(H, W, F, seed=3, device=venv.device)
    enc = DeviceEncoder.from_sb3(venv, cnn, H, W)
    images = frames(venv, H, W, 19)[0]
    f19 = enc.features(images).clone()
    f5 = enc.features(images[:5].contiguous())
    assert torch.equal(f5, f19[:5])
    perm = torch.randperm(19, generator=torch.Generator().manual_seed(1)).to(venv.device)
    assert torch.equal(enc.features(images[perm].contiguous()), f19[perm])
    enc.close()


# ---------------------------------------------------------------------------------------------- 6. reload, sharing
@gpu
def test_load_follows_the_modules():
    import mujoco_sim_amd as m

    one, two = m.HipVectorEnv("robot_reach", 5, seed=1), m.HipVectorEnv("point_mass_reach", 5, seed=2)
    one.reset()
    two.reset()
    cnn = make_cnn(36, 36, 64, seed=6, device=one.device)
    enc = m.DeviceEncoder.from_sb3(one, cnn, 36, 36)
    images = one.render(36, 36)
    before = enc.features(images).clone()
    torch.manual_seed(60)
    with torch.no_grad():
        for p in cnn.parameters():
            p.add_(0.05 * torch.randn_like(p))
    assert torch.equal(enc.features(images), before)  # the library's copy, until load()
    enc.load()
    after = enc.features(images).clone()
    ref64, ref32 = cnn_forward(cnn, images, torch.float64), cnn_forward(cnn, images, torch.float32)
    e32, bar = encoder_bar(ref64, ref32)
    assert (after.cpu().double() - ref64).abs().max().item() <= bar
    assert (after - before).abs().max().item() > 1e-3
    other = two.render(36, 36)  # the same encoder on another handle's frames
    ref64 = cnn_forward(cnn, other, torch.float64)
    e32, bar = encoder_bar(ref64, cnn_forward(cnn, other, torch.float32))
    assert (enc.features(other).cpu().double() - ref64).abs().max().item() <= bar
    assert torch.equal(enc.features(images), after)
    enc.close()
    one.close()
    two.close()


# ---------------------------------------------------------------------------------------------- 7. refusals
@gpu
def test_encoder_entry_points_refuse_bad_arguments(venv):
    from mujoco_sim_amd import _native as nat

    L = nat.lib()
    INVALID = -1
    dev = venv.device
    s = venv._stream()

    def create(**kw):
        base = dict(device=venv._dev_index, height=36, width=36, channels=3, features_dim=8)
        base.update(kw)
        e = C.c_void_p()
        rc = L.mjs_encoder_create(C.byref(nat.MjsEncoderDesc(**base)), C.byref(e))
        assert (rc == 0) == bool(e.value)
        return rc, e

    for kw in (dict(struct_size=C.sizeof(nat.MjsEncoderDesc) - 4), dict(height=35), dict(height=97), dict(width=35), dict(width=97), dict(channels=1), dict(channels=4),
               dict(features_dim=0), dict(features_dim=513), dict(device=999)):
        rc, _ = create(**kw)
        assert rc == INVALID and len(L.mjs_last_error(None)) > 0, kw
    assert L.mjs_encoder_create(None, None) == INVALID
    rc, enc = create(height=36, width=96, features_dim=512)  # the corners of the supported range are accepted
    assert rc == 0 and L.mjs_encoder_flat_dim(enc) == 64 * 1 * 8
    L.mjs_encoder_destroy(enc)
    rc, enc = create()
    assert rc == 0 and L.mjs_encoder_flat_dim(enc) == 64 and L.mjs_encoder_flat_dim(None) < 0
    assert L.mjs_encoder_workspace_bytes(enc, 5) == 5 * 64 * 4 and L.mjs_encoder_workspace_bytes(enc, -1) == 0 and L.mjs_encoder_workspace_bytes(None, 5) == 0
    n = 5
    images = torch.zeros(n, 36, 36, 3, dtype=torch.uint8, device=dev)
    ws = torch.full((n, 64), 7.0, dtype=torch.float32, device=dev)
    out = torch.full((n, 8), 7.0, dtype=torch.float32, device=dev)

    def run(e=enc, img=images, n_=n, ws_=ws, out_=out):
        ptr = lambda t: t.data_ptr() if t is not None else None  # noqa: E731
        return L.mjs_encoder_features(e, ptr(img), n_, ptr(ws_), ptr(out_), s)

    err = lambda: L.mjs_last_error(None)  # noqa: E731
    assert run() == INVALID and b"mjs_encoder_load" in err()  # never loaded
    cnn = make_cnn(36, 36, 8, seed=2, device=dev)
    t = [cnn.cnn[0], cnn.cnn[2], cnn.cnn[4], cnn.linear[0]]
    w = nat.MjsEncoderWeights(conv1_w=t[0].weight.data_ptr(), conv1_b=t[0].bias.data_ptr(), conv2_w=t[1].weight.data_ptr(), conv2_b=t[1].bias.data_ptr(),
                              conv3_w=t[2].weight.data_ptr(), conv3_b=t[2].bias.data_ptr(), fc_w=t[3].weight.data_ptr(), fc_b=t[3].bias.data_ptr())
    assert L.mjs_encoder_load(enc, C.byref(nat.MjsEncoderWeights(struct_size=8)), s) == INVALID and b"struct_size" in err()
    assert L.mjs_encoder_load(enc, C.byref(nat.MjsEncoderWeights()), s) == INVALID and b"null" in err()
    assert L.mjs_encoder_load(enc, None, s) == INVALID and L.mjs_encoder_load(None, C.byref(w), s) == INVALID
    assert run() == INVALID  # the refused loads loaded nothing
    assert L.mjs_encoder_load(enc, C.byref(w), s) == 0
    assert run(e=None) == INVALID and b"null" in err()
    assert run(img=None) == INVALID and b"null" in err()
    assert run(ws_=None) == INVALID and b"null" in err()
    assert run(out_=None) == INVALID and b"null" in err()
    assert run(n_=-1) == INVALID and b"negative" in err()
    assert run(n_=0) == 0
    torch.cuda.synchronize()
    assert bool((out == 7.0).all()) and bool((ws == 7.0).all())  # none of these launched anything
    assert run() == 0
    torch.cuda.synchronize()
    assert bool((out != 7.0).any()) and bool((ws != 7.0).all())
    L.mjs_encoder_destroy(enc)
    L.mjs_encoder_destroy(None)


# ---------------------------------------------------------------------------------------------- CPU: header, binding, argument checks
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
    from mujoco_sim_amd import _native as nat

    header = (ROOT / "include" / "mjsim.h").read_text()
    for c_name, binding in (("mjs_encoder_desc", nat.MjsEncoderDesc), ("mjs_encoder_weights", nat.MjsEncoderWeights),
                            ("mjs_actor_feature_inputs", nat.MjsActorFeatureInputs), ("mjs_visual_rollout", nat.MjsVisualRollout)):
        stated = re.search(rf"\}}\s*{c_name};\s*/\*\s*(\d+) bytes\s*\*/", header)
        assert stated, c_name
        assert int(stated.group(1)) == C.sizeof(binding), c_name
        assert binding().struct_size == C.sizeof(binding)
    assert C.sizeof(nat.MjsActorDesc) == 48  # the visual actor reuses the state actor's descriptor as it is
    assert nat.MjsVisualRollout.features_dev.offset == 80 and nat.MjsVisualRollout.workspace_dev.offset == 96


class _StubEnv:
    """What DeviceEncoder / DeviceActor read of a HipVectorEnv before they touch the native layer (Button-Push's layout, on the CPU)."""
    device = torch.device("cpu")
    _dev_index = 0
    action_dim = 7
    obs_dim = 13
    image_resolution = 36
    flat_observation_layout = (("ur5e/joint_configuration", 0, 6), ("unnamed_model/position", 9, 3), ("unnamed_model/active", 12, 1))
    camera_keys = (WRIST, SCENE)


@pytest.fixture
def no_native(monkeypatch):
    from mujoco_sim_amd import _native as nat

    def touched(*a, **k):
        raise AssertionError("the native layer was touched")

    monkeypatch.setattr(nat, "lib", touched)
    monkeypatch.setattr(nat, "check", touched)


def test_device_encoder_checks_its_arguments_before_any_native_call(no_native):
    from mujoco_sim_amd import DeviceEncoder

    venv = _StubEnv()
    nn = torch.nn

    def parts(H=36, W=36, F=16, **swap):
        cnn = NatureCNNStandIn(H, W, F)
        p = dict(conv1=cnn.cnn[0], conv2=cnn.cnn[2], conv3=cnn.cnn[4], fc=cnn.linear[0])
        p.update(swap)
        return p["conv1"], p["conv2"], p["conv3"], p["fc"]

    with pytest.raises(AssertionError, match="native layer"):  # valid arguments reach the (patched) native layer
        DeviceEncoder(venv, *parts(), 36, 36)
    with pytest.raises(AssertionError, match="native layer"):
        DeviceEncoder.from_sb3(venv, NatureCNNStandIn(96, 40, 512), 96, 40)
    with pytest.raises(ValueError, match="kernel size"):
        DeviceEncoder(venv, *parts(conv1=nn.Conv2d(3, 32, 7, 4)), 36, 36)
    with pytest.raises(ValueError, match="stride"):
        DeviceEncoder(venv, *parts(conv2=nn.Conv2d(32, 64, 4, 1)), 36, 36)
    with pytest.raises(ValueError, match="padding"):
        DeviceEncoder(venv, *parts(conv3=nn.Conv2d(64, 64, 3, 1, padding=1)), 36, 36)
    with pytest.raises(ValueError, match="channels"):
        DeviceEncoder(venv, *parts(conv1=nn.Conv2d(4, 32, 8, 4)), 36, 36)
    with pytest.raises(ValueError, match="channels"):
        DeviceEncoder(venv, *parts(conv2=nn.Conv2d(32, 32, 4, 2)), 36, 36)
    with pytest.raises(ValueError, match="in_features"):
        DeviceEncoder(venv, *parts(), 44, 44)  # a 36x36 net on 44x44 frames
    with pytest.raises(ValueError, match="in_features"):
        DeviceEncoder(venv, *parts(fc=nn.Linear(65, 16)), 36, 36)
    with pytest.raises(ValueError, match="float32"):
        DeviceEncoder(venv, *parts(conv3=nn.Conv2d(64, 64, 3, 1).double()), 36, 36)
    with pytest.raises(ValueError, match="float32"):
        DeviceEncoder.from_sb3(venv, NatureCNNStandIn(36, 36, 16).double(), 36, 36)
    with pytest.raises(ValueError, match="live on"):
        DeviceEncoder(venv, *parts(fc=nn.Linear(64, 16, device="meta")), 36, 36)
    with pytest.raises(ValueError, match="features_dim"):
        DeviceEncoder(venv, *parts(fc=nn.Linear(64, 513)), 36, 36)
    for H, W in ((35, 36), (36, 35), (97, 64), (64, 97)):
        with pytest.raises(ValueError, match="outside"):
            DeviceEncoder(venv, *parts(), H, W)
    with pytest.raises(ValueError, match="not a Conv2d"):
        DeviceEncoder(venv, *parts(conv2=nn.ReLU()), 36, 36)
    bad = NatureCNNStandIn(36, 36, 16)
    bad.cnn[1] = nn.Tanh()
    with pytest.raises(ValueError, match="Tanh"):
        DeviceEncoder.from_sb3(venv, bad, 36, 36)
    with pytest.raises(ValueError, match="cnn"):
        DeviceEncoder.from_sb3(venv, nn.Linear(3, 3), 36, 36)


def _fake_encoder(F, H=36, W=36):
    """A DeviceEncoder as the actor's argument checks see it, made without the native layer."""
    from mujoco_sim_amd import DeviceEncoder

    e = object.__new__(DeviceEncoder)
    e._e, e.features_dim, e.height, e.width = None, F, H, W
    return e


def test_visual_device_actor_checks_its_arguments_before_any_native_call(no_native):
    from mujoco_sim_amd import DeviceActor

    venv = _StubEnv()
    scene, wrist = _fake_encoder(16), _fake_encoder(24)
    both = {SCENE: scene, WRIST: wrist}
    net = lambda d: make_mlp(d, [32], 7, seed=0)  # noqa: E731
    with pytest.raises(AssertionError, match="native layer"):  # 10 columns + wrist 24 + scene 16, the default order
        DeviceActor.from_linears(venv, *net(50), encoders=both)
    cols, encs, starts = DeviceActor._segments(venv, None, None, both, None)
    assert cols == [0, 1, 2, 3, 4, 5, 9, 10, 11, 12] and encs == (scene, wrist) and starts == (34, 10)  # state keys, wrist, scene
    cols, encs, starts = DeviceActor._segments(venv, None, None, both, [SCENE, "unnamed_model/active", WRIST])
    assert cols == [12] and encs == (scene, wrist) and starts == (0, 17)
    cols, encs, starts = DeviceActor._segments(venv, None, None, {WRIST: wrist}, [WRIST])
    assert cols == [] and encs == (None, wrist) and starts == (0, 0)
    with pytest.raises(AssertionError, match="native layer"):  # images only: no observation columns
        DeviceActor.from_linears(venv, *net(16), encoders={SCENE: scene}, input_order=[SCENE])
    with pytest.raises(ValueError, match="expected"):  # the first layer must read columns + features
        DeviceActor.from_linears(venv, *net(10), encoders=both)
    with pytest.raises(ValueError, match="unknown camera key"):
        DeviceActor.from_linears(venv, *net(26), encoders={"TopCamera/rgb_image": scene})
    with pytest.raises(ValueError, match="twice"):
        DeviceActor.from_linears(venv, *net(32), encoders={SCENE: scene}, input_order=[SCENE, "ur5e/joint_configuration", SCENE])
    with pytest.raises(ValueError, match="misses"):
        DeviceActor.from_linears(venv, *net(46), encoders=both, input_order=["ur5e/joint_configuration", SCENE])
    with pytest.raises(ValueError, match="unknown observation key"):
        DeviceActor.from_linears(venv, *net(26), encoders={SCENE: scene}, input_order=["goal", SCENE])
    with pytest.raises(ValueError, match="no encoder"):
        DeviceActor.from_linears(venv, *net(26), encoders={SCENE: scene}, input_order=[WRIST, SCENE])
    with pytest.raises(ValueError, match="at most 2"):
        DeviceActor.from_linears(venv, *net(26), encoders={SCENE: scene, WRIST: wrist, "Third/rgb_image": scene})
    with pytest.raises(ValueError, match="not a DeviceEncoder"):
        DeviceActor.from_linears(venv, *net(26), encoders={SCENE: torch.nn.Linear(3, 3)})
    with pytest.raises(ValueError, match="image size"):
        DeviceActor.from_linears(venv, *net(50), encoders={SCENE: scene, WRIST: _fake_encoder(24, 44, 44)})
    with pytest.raises(ValueError, match="input_order names"):
        DeviceActor.from_linears(venv, *net(26), encoders={SCENE: scene}, input_order=[SCENE], obs_keys=("unnamed_model/active",))
    with pytest.raises(ValueError, match="give encoders"):
        DeviceActor.from_linears(venv, *net(10), input_order=["ur5e/joint_configuration"])
    with pytest.raises(ValueError, match="float32"):
        hidden, mu, log_std = net(26)
        DeviceActor.from_linears(venv, [hidden[0].double()], mu, log_std, encoders={SCENE: scene})


def test_from_sb3_multi_input_reads_a_combined_extractor(no_native, monkeypatch):
    from mujoco_sim_amd import DeviceActor, DeviceEncoder

    venv = _StubEnv()
    # SB3's CombinedExtractor walks the observation space's (sorted) keys: scene camera, joints, wrist camera
    extractors = {"scene": NatureCNNStandIn(36, 36, 16), "ur5e/joint_configuration": torch.nn.Flatten(), WRIST: NatureCNNStandIn(36, 36, 24)}
    sac = SacActorStandIn(16 + 6 + 24, [64, 64], 7, features_extractor=CombinedExtractorStandIn(extractors))
    made, seen = [], {}

    def from_sb3(venv_, cnn, H, W):
        made.append((cnn, H, W))
        return _fake_encoder(int(cnn.linear[0].out_features), H, W)

    def init(self, venv_, hidden, mu, log_std, activation="relu", obs_keys=None, **kw):
        seen.update(hidden=hidden, mu=mu, log_std=log_std, activation=activation, obs_keys=obs_keys, **kw)
        self._a, self._owned_encoders = None, ()

    with monkeypatch.context() as mp:
        mp.setattr(DeviceEncoder, "from_sb3", staticmethod(from_sb3))
        mp.setattr(DeviceActor, "__init__", init)
        actor = DeviceActor.from_sb3_multi_input(venv, sac, key_map={"scene": SCENE})
    assert [(c, H, W) for c, H, W in made] == [(extractors["scene"], 36, 36), (extractors[WRIST], 36, 36)]
    assert seen["input_order"] == [SCENE, "ur5e/joint_configuration", WRIST]
    assert [e.features_dim for e in (seen["encoders"][SCENE], seen["encoders"][WRIST])] == [16, 24]
    assert seen["hidden"] == [sac.latent_pi[0], sac.latent_pi[2]] and seen["mu"] is sac.mu and seen["activation"] == "relu"
    assert len(actor._owned_encoders) == 2
    with pytest.raises(AssertionError, match="native layer"):  # the real constructors accept it and go on to the native layer
        DeviceActor.from_sb3_multi_input(venv, sac, key_map={"scene": SCENE})
    with pytest.raises(ValueError, match="unknown camera key"):
        DeviceActor.from_sb3_multi_input(venv, sac)  # "scene" is not one of this env's camera keys
    with pytest.raises(ValueError, match="features_extractor"):
        DeviceActor.from_sb3_multi_input(venv, SacActorStandIn(6, [32], 7))
    odd = SacActorStandIn(6, [32], 7, features_extractor=CombinedExtractorStandIn({"ur5e/joint_configuration": torch.nn.Linear(6, 6)}))
    with pytest.raises(ValueError, match="Linear"):
        DeviceActor.from_sb3_multi_input(venv, odd)
