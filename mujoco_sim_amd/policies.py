"""Learned policies on the device: the MLP actor of SAC as ONE launch per control step (csrc/mjs_actor.h).

The reference's RL scripts (scripts/sb3/reach_sac.py, planar_push.py, sb3_sac.py) train SAC with an MLP actor
(``net_arch pi=[64, 64]`` / ``[32]``, SB3's default ``[256, 256]``): hidden ``Linear`` + activation layers, a ``mu`` and a
``log_std`` head, ``tanh`` squashing and the affine map onto the action space. :class:`DeviceActor` takes such modules, keeps a
packed copy of their parameters inside the library, and :meth:`HipVectorEnv.actor_actions` / :meth:`HipVectorEnv.actor_rollout`
evaluate it for every env without returning to Python. The numerics are float32 with float32 accumulation by contract, as SB3's
are; the float64 observations are rounded to float32 on the way in, the action is unscaled in float64.
"""
from __future__ import annotations

import ctypes as C

import torch

from . import _native as nat

_ACTIVATION_IDS = {"relu": nat.ACTIVATION_RELU, "tanh": nat.ACTIVATION_TANH}


SCENE_CAMERA_KEY, WRIST_CAMERA_KEY = "Camera/rgb_image", "ur5e/Camera/rgb_image"  # visual_observation_layout's camera keys
_CAMERA_SLOTS = {SCENE_CAMERA_KEY: 0, WRIST_CAMERA_KEY: 1}  # the feature block (and mjs_rollout_visual_actor's enc[]) a camera feeds
_NATURE_CNN = ((3, 32, 8, 4), (32, 64, 4, 2), (64, 64, 3, 1))  # (in, out, kernel, stride) of SB3's NatureCNN


def _is_linear(m) -> bool:
    return hasattr(m, "weight") and hasattr(m, "bias") and hasattr(m, "in_features") and hasattr(m, "out_features")


def _is_conv(m) -> bool:
    return all(hasattr(m, a) for a in ("weight", "bias", "kernel_size", "stride", "padding", "in_channels", "out_channels"))


def _pair(v):
    return (int(v), int(v)) if isinstance(v, int) else tuple(int(x) for x in v)


def _camera_keys(venv) -> tuple:
    """The env's camera keys in visual_observation_layout's order (wrist camera first where the task has one)."""
    keys = getattr(venv, "camera_keys", None)
    return tuple(keys) if keys is not None else (SCENE_CAMERA_KEY,)


def _check_parameters(name, m, layer, owner, device):
    """A layer's bias is there, and its parameters are float32 on ``device``; ValueError with the layer's ``name`` otherwise."""
    if m.bias is None:
        raise ValueError(f"{name}: a {layer} without bias")
    for t in (m.weight, m.bias):
        if t.dtype != torch.float32:
            raise ValueError(f"{name}: parameters are {t.dtype}; the device {owner} is float32 by contract (module.float())")
        if t.device != device:
            raise ValueError(f"{name}: parameters live on {t.device}, the env on {device}")


class _NativeObject:
    """An object of libmjsim.so behind a Python one: the handle's attribute, and the call that destroys it."""
    _handle, _destroy = "", ""

    def close(self):
        if getattr(self, self._handle, None):
            torch.cuda.synchronize(self.device)
            getattr(self._lib, self._destroy)(getattr(self, self._handle))
            setattr(self, self._handle, None)

    def __del__(self):
        try:
            self.close()
        except Exception:  # noqa: BLE001
            pass


class DeviceEncoder(_NativeObject):
    """SB3's ``NatureCNN`` (three ``Conv2d`` + ReLU, ``Flatten``, ``Linear`` + ReLU) held by libmjsim.so for the device of ``venv`` and
    one image size (csrc/mjs_encoder.h): uint8 [n, H, W, 3] frames, as :meth:`HipVectorEnv.render` writes them, to float32 features
    [n, F]. float32 with float32 accumulation; the division by 255 and the NHWC -> CHW reading are part of the kernel.

    Like :class:`DeviceActor` it keeps references to the torch modules and :meth:`load` packs their CURRENT parameters."""
    _handle, _destroy = "_e", "mjs_encoder_destroy"

    def __init__(self, venv, conv1, conv2, conv3, fc, height, width):
        self._e = None
        self.height, self.width = int(height), int(width)
        for name, v in (("height", self.height), ("width", self.width)):
            if not nat.ENCODER_MIN_SIZE <= v <= nat.ENCODER_MAX_SIZE:
                raise ValueError(f"{name} {v} outside {nat.ENCODER_MIN_SIZE}..{nat.ENCODER_MAX_SIZE}")
        self.convs, self.fc = [conv1, conv2, conv3], fc
        self.device = torch.device(venv.device)
        out = lambda n, k, s: (n - k) // s + 1  # noqa: E731
        h, w = self.height, self.width
        for _, _, k, st in _NATURE_CNN:
            h, w = out(h, k, st), out(w, k, st)
        self.flat_dim = 64 * h * w
        self._check_modules()
        self.features_dim = int(fc.out_features)
        # ---- native from here on
        self._lib = nat.lib()
        desc = nat.MjsEncoderDesc(device=int(venv._dev_index), height=self.height, width=self.width, channels=3, features_dim=self.features_dim)
        e = C.c_void_p()
        nat.check(self._lib.mjs_encoder_create(C.byref(desc), C.byref(e)))
        self._e = e
        self._staged = ()
        self._workspace = None
        self.load()

    @classmethod
    def from_sb3(cls, venv, nature_cnn, height, width):
        """From an object shaped like ``stable_baselines3.common.torch_layers.NatureCNN``: ``.cnn`` an ``nn.Sequential`` of ``Conv2d`` /
        ``ReLU`` / ``Flatten`` and ``.linear`` an ``nn.Sequential`` of ``Linear``, ``ReLU``. Duck-typed (SB3 is not a dependency)."""
        for name in ("cnn", "linear"):
            if not hasattr(nature_cnn, name):
                raise ValueError(f"not a NatureCNN-shaped module: no attribute {name!r}")
        convs = []
        for m in nature_cnn.cnn:
            if _is_conv(m):
                convs.append(m)
            elif not isinstance(m, (torch.nn.ReLU, torch.nn.Flatten)):
                raise ValueError(f"cnn holds a {type(m).__name__}: only Conv2d, ReLU and Flatten are built")
        linears = [m for m in nature_cnn.linear if _is_linear(m)]
        for m in nature_cnn.linear:
            if not _is_linear(m) and not isinstance(m, torch.nn.ReLU):
                raise ValueError(f"linear holds a {type(m).__name__}: only Linear and ReLU are built")
        if len(convs) != 3 or len(linears) != 1:
            raise ValueError(f"NatureCNN has three Conv2d and one Linear, got {len(convs)} and {len(linears)}")
        return cls(venv, *convs, linears[0], height, width)

    def _check_modules(self):
        """Shapes, dtype and device of the modules' current parameters; ValueError before anything native sees them."""
        for i, (m, (cin, cout, k, st)) in enumerate(zip(self.convs, _NATURE_CNN)):
            name = f"conv{i + 1}"
            if not _is_conv(m):
                raise ValueError(f"{name}: {type(m).__name__} is not a Conv2d")
            if _pair(m.kernel_size) != (k, k):
                raise ValueError(f"{name}: kernel size {tuple(m.kernel_size)}, NatureCNN's is {(k, k)}")
            if _pair(m.stride) != (st, st):
                raise ValueError(f"{name}: stride {tuple(m.stride)}, NatureCNN's is {(st, st)}")
            if isinstance(m.padding, str) or _pair(m.padding) != (0, 0):
                raise ValueError(f"{name}: padding {m.padding!r}, NatureCNN's is 0")
            if (int(m.in_channels), int(m.out_channels)) != (cin, cout):
                raise ValueError(f"{name}: channels {m.in_channels} -> {m.out_channels}, expected {cin} -> {cout}")
            _check_parameters(name, m, "Conv2d", "encoder", self.device)
            if tuple(m.weight.shape) != (cout, cin, k, k) or tuple(m.bias.shape) != (cout,):
                raise ValueError(f"{name}: weight {tuple(m.weight.shape)} (dilation, groups?), expected {(cout, cin, k, k)}")
        fc = self.fc
        if not _is_linear(fc):
            raise ValueError(f"fc: {type(fc).__name__} is not a Linear layer")
        _check_parameters("fc", fc, "Linear", "encoder", self.device)
        if int(fc.in_features) != self.flat_dim:
            raise ValueError(f"fc.in_features is {fc.in_features}; a {self.height}x{self.width} image flattens to {self.flat_dim}")
        F = int(fc.out_features)
        if not 1 <= F <= nat.ENCODER_MAX_FEATURES:
            raise ValueError(f"fc: features_dim {F} outside 1..{nat.ENCODER_MAX_FEATURES}")
        if tuple(fc.weight.shape) != (F, self.flat_dim) or tuple(fc.bias.shape) != (F,):
            raise ValueError(f"fc: weight {tuple(fc.weight.shape)} / bias {tuple(fc.bias.shape)}, expected {(F, self.flat_dim)} / {(F,)}")

    def load(self):
        """Pack the modules' current parameters into the library's copy (small kernels on the current stream, no synchronisation)."""
        if self._e is None:
            raise nat.MjsError("the encoder is closed")
        self._check_modules()
        if int(self.fc.out_features) != self.features_dim:
            raise ValueError("fc.out_features changed since the encoder was made")
        staged = [t.detach().contiguous() for m in (*self.convs, self.fc) for t in (m.weight, m.bias)]
        w = nat.MjsEncoderWeights(**{f: t.data_ptr() for f, t in zip(("conv1_w", "conv1_b", "conv2_w", "conv2_b", "conv3_w", "conv3_b", "fc_w", "fc_b"), staged)})
        stream = torch.cuda.current_stream(self.device).cuda_stream
        nat.check(self._lib.mjs_encoder_load(self._e, C.byref(w), C.c_void_p(stream)))
        self._staged = staged  # alive until the next load: the pack kernels read them asynchronously

    def workspace(self, n):
        """A float32 [n, flat_dim] device tensor for mjs_encoder_features (kept and reused while n does not grow)."""
        if self._workspace is None or self._workspace.shape[0] < n:
            assert self._lib.mjs_encoder_workspace_bytes(self._e, int(n)) == 4 * int(n) * self.flat_dim
            self._workspace = torch.empty(int(n), self.flat_dim, dtype=torch.float32, device=self.device)
        return self._workspace

    def features(self, images, out=None):
        """uint8 [n, H, W, 3] on the device -> float32 [n, F] (two launches on the current stream)."""
        if self._e is None:
            raise nat.MjsError("the encoder is closed")
        n = int(images.shape[0])
        if tuple(images.shape) != (n, self.height, self.width, 3) or images.dtype != torch.uint8 or images.device != self.device or not images.is_contiguous():
            raise ValueError(f"images must be a contiguous uint8 tensor [n, {self.height}, {self.width}, 3] on {self.device}")
        if out is None:
            out = torch.empty(n, self.features_dim, dtype=torch.float32, device=self.device)
        assert out.shape == (n, self.features_dim) and out.dtype == torch.float32 and out.is_contiguous()
        if n:
            stream = torch.cuda.current_stream(self.device).cuda_stream
            nat.check(self._lib.mjs_encoder_features(self._e, images.data_ptr(), n, self.workspace(n).data_ptr(), out.data_ptr(), C.c_void_p(stream)))
        return out


class DeviceActor(_NativeObject):
    """An MLP actor (SAC's squashed Gaussian) held by libmjsim.so for the device of ``venv``.

    The object keeps references to the torch modules; :meth:`load` packs their CURRENT parameters (a training loop calls it after
    every policy update; it enqueues small kernels on the current stream and never synchronises). An actor belongs to a device and
    a shape, not to a handle: any ``HipVectorEnv`` of the same task settings on that device may use it."""
    _handle, _destroy = "_a", "mjs_actor_destroy"

    def __init__(self, venv, hidden, mu, log_std, activation="relu", obs_keys=None, obs_index=None, variant=nat.ACTOR_VARIANT_DEFAULT,
                 encoders=None, input_order=None):
        self._a = None
        self._owned_encoders = ()
        hidden = list(hidden)
        if activation not in _ACTIVATION_IDS:
            raise ValueError(f"activation must be one of {sorted(_ACTIVATION_IDS)}, got {activation!r}")
        if variant not in (nat.ACTOR_VARIANT_DEFAULT, nat.ACTOR_VARIANT_TILE32):
            raise ValueError("variant must be ACTOR_VARIANT_DEFAULT (16 envs per workgroup) or ACTOR_VARIANT_TILE32")
        if not 1 <= len(hidden) <= nat.ACTOR_MAX_LAYERS:
            raise ValueError(f"an actor has 1..{nat.ACTOR_MAX_LAYERS} hidden layers, got {len(hidden)}")
        for m in (*hidden, mu, log_std):
            if not _is_linear(m):
                raise ValueError(f"{type(m).__name__} is not a Linear layer (weight, bias, in_features, out_features)")
        self.visual = bool(encoders) or input_order is not None
        if self.visual:
            self.obs_index, self.encoders, self.block_start = self._segments(venv, obs_keys, obs_index, encoders or {}, input_order)
            if variant != nat.ACTOR_VARIANT_DEFAULT:
                raise ValueError("a visual actor runs the default variant (16 envs per workgroup)")
        else:
            self.obs_index, self.encoders, self.block_start = self._columns(venv, obs_keys, obs_index), (None, None), (0, 0)
        self.in_dim = len(self.obs_index)
        if not (0 if self.visual else 1) <= self.in_dim <= nat.ACTOR_MAX_IN:
            raise ValueError(f"an actor reads 1..{nat.ACTOR_MAX_IN} observation columns, got {self.in_dim}")
        self.block_width = tuple(e.features_dim if e is not None else 0 for e in self.encoders)
        self.in_total = self.in_dim + sum(self.block_width)  # the first layer's fan-in
        self.device = torch.device(venv.device)
        self.action_dim = int(venv.action_dim)
        if self.action_dim > nat.ACTOR_MAX_ACTIONS:
            raise ValueError(f"an actor has at most {nat.ACTOR_MAX_ACTIONS} action components")
        self.hidden, self.mu, self.log_std = hidden, mu, log_std
        self.activation = activation
        self.widths = [int(m.out_features) for m in hidden]
        self._check_modules()
        # ---- native from here on
        self._lib = nat.lib()
        index = (C.c_int32 * max(self.in_dim, 1))(*self.obs_index)
        desc = nat.MjsActorDesc(device=int(venv._dev_index), in_dim=self.in_dim, n_hidden=len(hidden), hidden=(C.c_int32 * 3)(*self.widths),
                                action_dim=self.action_dim, activation=_ACTIVATION_IDS[activation], variant=int(variant), obs_index=index)
        a = C.c_void_p()
        if self.visual:
            blocks = nat.MjsActorFeatureInputs(n_blocks=sum(w > 0 for w in self.block_width), width=(C.c_int32 * 2)(*self.block_width),
                                               start=(C.c_int32 * 2)(*self.block_start))
            nat.check(self._lib.mjs_actor_create_visual(C.byref(desc), C.byref(blocks), C.byref(a)))
        else:
            nat.check(self._lib.mjs_actor_create(C.byref(desc), C.byref(a)))
        self._a = a
        self._staged = ()
        self.load()

    # ------------------------------------------------------------------ construction
    @classmethod
    def from_linears(cls, venv, hidden, mu, log_std, activation="relu", obs_keys=None, **kw):
        """``hidden``: 1..3 ``torch.nn.Linear`` (widths 1..256), ``mu`` / ``log_std``: ``Linear`` onto the env's action width, all
        float32 on the env's device. ``obs_keys`` selects and orders the input columns through ``venv.flat_observation_layout``
        (``None``: every state key in the env's order), e.g. ``("ur5e/tcp_position", "target_position")``, the reference's STATE
        observation of Robot-Reach, or ``sorted(keys)``, the order SB3's ``CombinedExtractor`` concatenates a gymnasium ``Dict`` in.
        ``obs_index=[...]`` gives the columns of a ``flat_obs`` row directly instead. Raises ``ValueError`` for a float64 module, a
        parameter on another device, mismatched shapes or an unknown key, before any native call.

        A visual actor: ``encoders={"Camera/rgb_image": DeviceEncoder, ...}`` (at most two, keyed by the env's camera keys, those of
        ``visual_observation_layout``) makes every encoder's features a block of the first layer's input. ``input_order`` lists
        observation keys and camera keys in concatenation order (default: the state keys - ``obs_keys`` or the env's - then the
        cameras in the env's order); ``hidden[0]`` then reads ``columns + sum of features_dim`` inputs, and the columns may be none."""
        return cls(venv, hidden, mu, log_std, activation=activation, obs_keys=obs_keys, **kw)

    @classmethod
    def from_sb3_multi_input(cls, venv, actor, key_map=None, **kw):
        """From an object shaped like SAC's actor of a ``MultiInputPolicy``: ``actor.features_extractor.extractors`` a ``ModuleDict`` of
        per-key extractors (NatureCNN-shaped, with ``.cnn`` and ``.linear`` -> a :class:`DeviceEncoder` at the env's
        ``image_resolution``; anything else is ``Flatten`` -> that key's observation columns), concatenated in the ModuleDict's
        order as SB3's ``CombinedExtractor`` does, plus ``latent_pi`` / ``mu`` / ``log_std`` as in :meth:`from_sb3`. ``key_map`` maps
        the ModuleDict's keys to this env's observation / camera keys where they differ. The actor owns the encoders it makes
        (``actor.encoders``; :meth:`close` closes them, :meth:`load` reloads them too). Duck-typed, like :meth:`from_sb3`."""
        extractor = getattr(actor, "features_extractor", None)
        if extractor is None or not hasattr(extractor, "extractors"):
            raise ValueError("not an SB3-shaped MultiInputPolicy actor: no features_extractor.extractors")
        key_map = dict(key_map or {})
        order, cnn = [], {}
        for key, ext in extractor.extractors.items():
            ours = key_map.get(key, key)
            order.append(ours)
            if hasattr(ext, "cnn") and hasattr(ext, "linear"):
                cnn[ours] = ext
            elif not isinstance(ext, torch.nn.Flatten):
                raise ValueError(f"extractor {key!r} is a {type(ext).__name__}: only NatureCNN-shaped modules and Flatten are built")
        known = set(_camera_keys(venv))
        for k in cnn:
            if k not in known:
                raise ValueError(f"unknown camera key {k!r}; this env has {sorted(known)}")
        if len(cnn) > nat.ACTOR_MAX_BLOCKS:
            raise ValueError(f"at most {nat.ACTOR_MAX_BLOCKS} encoders, got {len(cnn)}")
        r = int(venv.image_resolution)
        made = {}
        try:
            for k, ext in cnn.items():
                made[k] = DeviceEncoder.from_sb3(venv, ext, r, r)
            self = cls.from_sb3(venv, actor, encoders=made, input_order=order, **kw)
        except Exception:
            for e in made.values():
                e.close()
            raise
        self._owned_encoders = tuple(made.values())
        return self

    @classmethod
    def _segments(cls, venv, obs_keys, obs_index, encoders, input_order):
        """(observation columns, encoders by slot, block starts) of a visual actor's input vector; ValueError for what does not fit."""
        encoders = dict(encoders)
        if len(encoders) > nat.ACTOR_MAX_BLOCKS:
            raise ValueError(f"at most {nat.ACTOR_MAX_BLOCKS} encoders, got {len(encoders)}")
        cameras = _camera_keys(venv)
        for k, e in encoders.items():
            if k not in cameras:
                raise ValueError(f"unknown camera key {k!r}; this env has {list(cameras)}")
            if not isinstance(e, DeviceEncoder):
                raise ValueError(f"encoders[{k!r}] is a {type(e).__name__}, not a DeviceEncoder")
        if not encoders:
            raise ValueError("input_order is for visual actors: give encoders")
        sizes = {(e.height, e.width) for e in encoders.values()}
        if len(sizes) > 1:
            raise ValueError(f"the encoders of one actor share an image size, got {sorted(sizes)}")
        if input_order is None:
            if obs_index is not None:
                cols = cls._columns(venv, obs_keys, obs_index)
                by_slot, pos = [None, None], len(cols)
                starts = [0, 0]
                for k in cameras:
                    if k in encoders:
                        by_slot[_CAMERA_SLOTS[k]], starts[_CAMERA_SLOTS[k]] = encoders[k], pos
                        pos += encoders[k].features_dim
                return cols, tuple(by_slot), tuple(starts)
            state = [k for k, _, _ in venv.flat_observation_layout] if obs_keys is None else list(obs_keys)
            input_order = state + [k for k in cameras if k in encoders]
        elif obs_keys is not None or obs_index is not None:
            raise ValueError("input_order names the observation keys itself: give no obs_keys / obs_index with it")
        input_order = list(input_order)
        if len(set(input_order)) != len(input_order):
            raise ValueError(f"input_order lists a key twice: {input_order}")
        for k in encoders:
            if k not in input_order:
                raise ValueError(f"input_order misses the camera key {k!r} of an encoder")
        layout = {k: (s, n) for k, s, n in venv.flat_observation_layout}
        cols, by_slot, starts, pos = [], [None, None], [0, 0], 0
        for k in input_order:
            if k in encoders:
                by_slot[_CAMERA_SLOTS[k]], starts[_CAMERA_SLOTS[k]] = encoders[k], pos
                pos += encoders[k].features_dim
            elif k in layout:
                cols.extend(range(layout[k][0], layout[k][0] + layout[k][1]))
                pos += layout[k][1]
            elif k in cameras:
                raise ValueError(f"input_order names the camera {k!r}, which has no encoder")
            else:
                raise ValueError(f"unknown observation key {k!r}; this env has {list(layout)} and the cameras {list(cameras)}")
        return cols, tuple(by_slot), tuple(starts)

    @classmethod
    def from_sb3(cls, venv, actor, obs_keys=None, **kw):
        """From an object shaped like ``stable_baselines3.sac.policies.Actor``: ``actor.latent_pi`` an ``nn.Sequential`` of
        ``Linear`` / activation (``ReLU`` or ``Tanh``, one kind) modules, ``actor.mu`` and ``actor.log_std`` ``Linear``. Duck-typed:
        stable_baselines3 itself is not a dependency of this package and is not installed where its tests run, so this path is
        tested against a stand-in module with those attributes, not against SB3. The actor's features extractor is not evaluated:
        ``obs_keys`` must name the columns in the order it concatenates them (``Flatten`` of a flat Box: the env's order;
        ``CombinedExtractor`` of a Dict: sorted keys). gSDE actors (``use_sde``) have no ``log_std`` layer and are refused."""
        for name in ("latent_pi", "mu", "log_std"):
            if not hasattr(actor, name):
                raise ValueError(f"not an SB3-shaped SAC actor: no attribute {name!r}")
        hidden, kinds = [], set()
        for m in actor.latent_pi:
            if _is_linear(m):
                hidden.append(m)
            elif isinstance(m, torch.nn.ReLU):
                kinds.add("relu")
            elif isinstance(m, torch.nn.Tanh):
                kinds.add("tanh")
            else:
                raise ValueError(f"latent_pi holds a {type(m).__name__}: only Linear, ReLU and Tanh are built")
        if len(kinds) > 1:
            raise ValueError("latent_pi mixes ReLU and Tanh")
        return cls(venv, hidden, actor.mu, actor.log_std, activation=kinds.pop() if kinds else "relu", obs_keys=obs_keys, **kw)

    @staticmethod
    def _columns(venv, obs_keys, obs_index):
        if obs_index is not None:
            if obs_keys is not None:
                raise ValueError("give obs_keys or obs_index, not both")
            cols = [int(c) for c in obs_index]
            if any(c < 0 or c >= int(venv.obs_dim) for c in cols):
                raise ValueError(f"obs_index entries must lie in 0..{int(venv.obs_dim) - 1}")
            return cols
        layout = {k: (s, n) for k, s, n in venv.flat_observation_layout}
        keys = list(layout) if obs_keys is None else list(obs_keys)
        cols = []
        for k in keys:
            if k not in layout:
                raise ValueError(f"unknown observation key {k!r}; this env has {list(layout)}")
            cols.extend(range(layout[k][0], layout[k][0] + layout[k][1]))
        return cols

    def _check_modules(self):
        """Shapes, dtype and device of the modules' current parameters; ValueError before anything native sees them."""
        fan_in = self.in_total
        layers = [(f"hidden[{i}]", m, w) for i, (m, w) in enumerate(zip(self.hidden, self.widths))] + [("mu", self.mu, self.action_dim), ("log_std", self.log_std, self.action_dim)]
        for name, m, width in layers:
            if not 1 <= width <= nat.ACTOR_MAX_HIDDEN:
                raise ValueError(f"{name}: width {width} outside 1..{nat.ACTOR_MAX_HIDDEN}")
            _check_parameters(name, m, "Linear", "actor", self.device)
            if name in ("mu", "log_std"):
                fan_in = self.widths[-1]
            if tuple(m.weight.shape) != (width, fan_in) or tuple(m.bias.shape) != (width,):
                raise ValueError(f"{name}: weight {tuple(m.weight.shape)} / bias {tuple(m.bias.shape)}, expected {(width, fan_in)} / {(width,)}")
            fan_in = width

    # ------------------------------------------------------------------ use
    def load(self):
        """Pack the modules' current parameters into the library's copy (small kernels on the current stream, no synchronisation)."""
        if self._a is None:
            raise nat.MjsError("the actor is closed")
        self._check_modules()
        staged = [t.detach().contiguous() for m in (*self.hidden, self.mu, self.log_std) for t in (m.weight, m.bias)]
        n = len(self.hidden)
        w = nat.MjsActorWeights(hidden_w=(C.c_void_p * 3)(*[staged[2 * i].data_ptr() for i in range(n)]),
                                hidden_b=(C.c_void_p * 3)(*[staged[2 * i + 1].data_ptr() for i in range(n)]),
                                mu_w=staged[2 * n].data_ptr(), mu_b=staged[2 * n + 1].data_ptr(),
                                log_std_w=staged[2 * n + 2].data_ptr(), log_std_b=staged[2 * n + 3].data_ptr())
        stream = torch.cuda.current_stream(self.device).cuda_stream
        nat.check(self._lib.mjs_actor_load(self._a, C.byref(w), C.c_void_p(stream)))
        self._staged = staged  # alive until the next load: the pack kernels read them asynchronously
        for e in self._owned_encoders:
            e.load()

    def close(self):
        super().close()
        for e in getattr(self, "_owned_encoders", ()):
            e.close()
