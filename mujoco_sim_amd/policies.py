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

    Like :class:`DeviceActor` it keeps references to the torch modules and :meth:`load` packs their CURRENT parameters. Once a
    :class:`DeviceEncoderOptimizer` exists the packed copy is the master copy: :meth:`load` would overwrite the trained parameters
    with the stale modules, :meth:`export` writes them back into torch, :meth:`blend_from` follows another encoder's copy."""
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

    def _weights_struct(self, tensors):
        """mjs_encoder_weights over the flat list (weight, bias) of conv1, conv2, conv3, fc."""
        return nat.MjsEncoderWeights(**{f: t.data_ptr() for f, t in zip(("conv1_w", "conv1_b", "conv2_w", "conv2_b", "conv3_w", "conv3_b", "fc_w", "fc_b"), tensors)})

    def _empty_like_parameters(self):
        """Fresh contiguous float32 tensors in torch layout: the flat list (weight, bias) of conv1, conv2, conv3, fc."""
        out = []
        for cin, cout, k, _ in _NATURE_CNN:
            out += [torch.empty(cout, cin, k, k, dtype=torch.float32, device=self.device), torch.empty(cout, dtype=torch.float32, device=self.device)]
        return out + [torch.empty(self.features_dim, self.flat_dim, dtype=torch.float32, device=self.device),
                      torch.empty(self.features_dim, dtype=torch.float32, device=self.device)]

    def _check_export_modules(self, modules):
        """(conv1, conv2, conv3, fc) with this encoder's shapes, float32 on its device; ValueError otherwise."""
        try:
            conv1, conv2, conv3, fc = modules
        except (TypeError, ValueError):
            raise ValueError("modules must be (conv1, conv2, conv3, fc), as DeviceEncoder takes them") from None
        for name, m, (cin, cout, k, _) in zip(("conv1", "conv2", "conv3"), (conv1, conv2, conv3), _NATURE_CNN):
            if not _is_conv(m):
                raise ValueError(f"{name}: {type(m).__name__} is not a Conv2d")
            _check_parameters(name, m, "Conv2d", "encoder", self.device)
            if tuple(m.weight.shape) != (cout, cin, k, k) or tuple(m.bias.shape) != (cout,):
                raise ValueError(f"{name}: weight {tuple(m.weight.shape)} / bias {tuple(m.bias.shape)}, expected {(cout, cin, k, k)} / {(cout,)}")
        if not _is_linear(fc):
            raise ValueError(f"fc: {type(fc).__name__} is not a Linear layer (weight, bias, in_features, out_features)")
        _check_parameters("fc", fc, "Linear", "encoder", self.device)
        if tuple(fc.weight.shape) != (self.features_dim, self.flat_dim) or tuple(fc.bias.shape) != (self.features_dim,):
            raise ValueError(f"fc: weight {tuple(fc.weight.shape)} / bias {tuple(fc.bias.shape)}, expected {(self.features_dim, self.flat_dim)} / {(self.features_dim,)}")
        return conv1, conv2, conv3, fc

    def export(self, modules=None):
        """The packed parameters into ``modules = (conv1, conv2, conv3, fc)`` (default: the modules this object was made from), with
        ``copy_`` under ``no_grad``: the way back into torch after steps of a :class:`DeviceEncoderOptimizer`. Small kernels on the
        current stream, no synchronisation. Returns ``(conv1, conv2, conv3, fc)``."""
        mods = self._check_export_modules((*self.convs, self.fc) if modules is None else modules)
        if self._e is None:
            raise nat.MjsError("the encoder is closed")
        staged = self._empty_like_parameters()
        w = self._weights_struct(staged)
        launch = self._lib.mjs_encoder_export
        stream = torch.cuda.current_stream(self.device).cuda_stream
        nat.check(launch(self._e, C.byref(w), C.c_void_p(stream)))
        with torch.no_grad():
            for k, m in enumerate(mods):
                m.weight.copy_(staged[2 * k])
                m.bias.copy_(staged[2 * k + 1])
        return mods

    def blend_from(self, other, tau):
        """``packed = (1 - tau) * packed + tau * other's packed`` (SB3's ``polyak_update`` between two packed copies, one launch): what
        a target critic's own extractor does after every step of the online one. ``other``: a :class:`DeviceEncoder` of the same
        image size and ``features_dim`` on the same device; ``tau`` in (0, 1], ``tau = 1`` copies."""
        if not isinstance(other, DeviceEncoder):
            raise ValueError(f"other must be a DeviceEncoder, got {type(other).__name__}")
        tau = float(tau)
        if not 0.0 < tau <= 1.0:
            raise ValueError(f"tau must lie in (0, 1], got {tau}")
        if other.device != self.device:
            raise ValueError(f"the other encoder lives on {other.device}, this one on {self.device}")
        mine, theirs = (self.height, self.width, self.features_dim), (other.height, other.width, other.features_dim)
        if mine != theirs:
            raise ValueError(f"the encoders differ in shape: (height, width, features_dim) {mine} against {theirs}")
        if self._e is None or other._e is None:
            raise nat.MjsError("the encoder is closed")
        blend = self._lib.mjs_encoder_blend
        stream = torch.cuda.current_stream(self.device).cuda_stream
        nat.check(blend(self._e, other._e, tau, C.c_void_p(stream)))


class DeviceEncoderOptimizer(_NativeObject):
    """The backward pass of a :class:`DeviceEncoder` and ``torch.optim.Adam`` on its packed parameters (csrc/mjs_encoder_train.h)::

        features = cnn(images); features.backward(dfeatures); optimizer.step()              # torch.optim.Adam, SB3's defaults

    ``dfeatures`` is read as it is (the ``1/B`` of a mean loss is the caller's, as with autograd). With a head of any kind in torch -
    ``f = enc.features(images).requires_grad_(); loss(head(f)).backward(); opt.step(images, f.grad)`` - the CNN trains on the device.
    The sums over the batch are bitwise reproducible. The packed copy is the master copy from the first step on:
    ``encoder.features`` and the visual rollout see every step at once, a target encoder follows with
    ``target.blend_from(encoder, tau)``, ``encoder.export()`` refreshes the torch modules, and ``encoder.load()`` would overwrite the
    trained parameters with the stale modules. The optimiser keeps the encoder alive."""
    _handle, _destroy = "_o", "mjs_encoder_opt_destroy"

    def __init__(self, encoder, lr=3e-4, betas=(0.9, 0.999), eps=1e-8):
        self._o = None
        if not isinstance(encoder, DeviceEncoder):
            raise ValueError(f"encoder must be a DeviceEncoder, got {type(encoder).__name__}")
        self.lr = DeviceCriticOptimizer._checked_lr(lr)
        try:
            beta1, beta2 = (float(b) for b in betas)
        except (TypeError, ValueError):
            raise ValueError("betas must be two floats in [0, 1)") from None
        if not (0.0 <= beta1 < 1.0 and 0.0 <= beta2 < 1.0):
            raise ValueError(f"betas must lie in [0, 1), got {(beta1, beta2)}")
        eps = float(eps)
        if not 0.0 < eps < float("inf"):
            raise ValueError(f"eps must be positive and finite, got {eps}")
        self.betas, self.eps = (beta1, beta2), eps
        self.encoder, self.device = encoder, encoder.device
        self.step_count = 0
        self._workspace = None
        if encoder._e is None:
            raise nat.MjsError("the encoder is closed")
        # ---- native from here on
        self._lib = encoder._lib
        desc = nat.MjsEncoderOptDesc(lr=self.lr, beta1=beta1, beta2=beta2, eps=eps)
        o = C.c_void_p()
        nat.check(self._lib.mjs_encoder_opt_create(encoder._e, C.byref(desc), C.byref(o)))
        self._o = o

    def _checked(self, images, dfeatures):
        """n, with both tensors checked; ValueError before anything native."""
        e = self.encoder
        if not isinstance(images, torch.Tensor) or images.dim() != 4:
            raise ValueError(f"images must be a contiguous uint8 tensor [n, {e.height}, {e.width}, 3] on {self.device}")
        n = int(images.shape[0])
        if tuple(images.shape) != (n, e.height, e.width, 3) or images.dtype != torch.uint8 or images.device != self.device or not images.is_contiguous():
            raise ValueError(f"images must be a contiguous uint8 tensor [n, {e.height}, {e.width}, 3] on {self.device}")
        if (not isinstance(dfeatures, torch.Tensor) or tuple(dfeatures.shape) != (n, e.features_dim) or dfeatures.dtype != torch.float32
                or dfeatures.device != self.device or not dfeatures.is_contiguous()):
            raise ValueError(f"dfeatures must be a contiguous float32 tensor [{n}, {e.features_dim}] on {self.device}")
        return n

    def _open(self):
        if self.encoder._e is None:
            raise nat.MjsError("the encoder is closed")
        if self._o is None:
            raise nat.MjsError("the optimiser is closed")

    def workspace(self, n):
        """A float32 device tensor of mjs_encoder_train_workspace_bytes(n) (kept and reused while it is large enough)."""
        floats = int(self._lib.mjs_encoder_train_workspace_bytes(self.encoder._e, int(n))) // 4
        if self._workspace is None or self._workspace.numel() < floats:
            self._workspace = torch.empty(floats, dtype=torch.float32, device=self.device)
        return self._workspace

    def _args(self, images, dfeatures, n, features=None, grads=None, activations=None):
        acts = (C.c_void_p * 3)(*[t.data_ptr() for t in activations]) if activations is not None else (C.c_void_p * 3)()
        return nat.MjsEncoderGradArgs(n=n, rgb_dev=images.data_ptr(), dfeatures_dev=dfeatures.data_ptr(), workspace_dev=self.workspace(n).data_ptr(),
                                      features_out_dev=features.data_ptr() if features is not None else None,
                                      grads_out=C.pointer(grads) if grads is not None else None, activations_out_dev=acts)

    def step(self, images, dfeatures, lr=None, return_parts=False):
        """One Adam step on the gradient of ``sum(features * dfeatures)`` with the learning rate ``lr`` (default: the constructor's).
        Nine launches on the current stream; nothing is read back. Returns ``None``, or with ``return_parts`` a dict with ``features``
        [n, F] (BEFORE the step). An empty batch does nothing and is not counted."""
        n = self._checked(images, dfeatures)
        lr = self.lr if lr is None else DeviceCriticOptimizer._checked_lr(lr)
        self._open()
        features = torch.empty(n, self.encoder.features_dim, dtype=torch.float32, device=self.device) if return_parts else None
        if n:
            args = self._args(images, dfeatures, n, features)
            update = self._lib.mjs_encoder_update
            stream = torch.cuda.current_stream(self.device).cuda_stream
            nat.check(update(self._o, C.byref(args), lr, C.c_void_p(stream)))
            self.step_count += 1
        return {"features": features} if return_parts else None

    def gradients(self, images, dfeatures):
        """The gradients :meth:`step` would apply, and no update: a dict with ``features`` [n, F], ``grads`` (a list of ``(weight_grad,
        bias_grad)`` in torch layout for conv1, conv2, conv3, fc) and ``activations`` (``conv1`` [n, P1, 32], ``conv2`` [n, P2, 64],
        ``flat`` [n, flat_dim], post-ReLU: the masks the backward pass used)."""
        n = self._checked(images, dfeatures)
        self._open()
        e = self.encoder
        h1, w1 = (e.height - 8) // 4 + 1, (e.width - 8) // 4 + 1
        h2, w2 = (h1 - 4) // 2 + 1, (w1 - 4) // 2 + 1
        new = lambda *shape: torch.zeros(*shape, dtype=torch.float32, device=self.device)  # noqa: E731
        features = new(n, e.features_dim)
        acts = {"conv1": new(n, h1 * w1, 32), "conv2": new(n, h2 * w2, 64), "flat": new(n, e.flat_dim)}
        flat = e._empty_like_parameters()
        if n:
            args = self._args(images, dfeatures, n, features, e._weights_struct(flat), (acts["conv1"], acts["conv2"], acts["flat"]))
            grad = self._lib.mjs_encoder_grad
            stream = torch.cuda.current_stream(self.device).cuda_stream
            nat.check(grad(e._e, self._o, C.byref(args), C.c_void_p(stream)))
        else:
            for t in flat:
                t.zero_()
        return {"features": features, "grads": [(flat[2 * k], flat[2 * k + 1]) for k in range(4)], "activations": acts}


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
        """Pack the modules' current parameters into the library's copy (small kernels on the current stream, no synchronisation).

        Once a :class:`DeviceActorOptimizer` has stepped this actor, the packed copy is the master copy and the modules are stale:
        ``load()`` would overwrite the trained parameters with them. :meth:`export` is the way back into torch."""
        if self._a is None:
            raise nat.MjsError("the actor is closed")
        self._check_modules()
        staged = [t.detach().contiguous() for m in (*self.hidden, self.mu, self.log_std) for t in (m.weight, m.bias)]
        w = self._weights_struct(staged)
        stream = torch.cuda.current_stream(self.device).cuda_stream
        nat.check(self._lib.mjs_actor_load(self._a, C.byref(w), C.c_void_p(stream)))
        self._staged = staged  # alive until the next load: the pack kernels read them asynchronously
        for e in self._owned_encoders:
            e.load()

    def _weights_struct(self, tensors):
        """mjs_actor_weights over the flat list (weight, bias) per hidden layer, then mu's and log_std's."""
        n = len(self.hidden)
        return nat.MjsActorWeights(hidden_w=(C.c_void_p * 3)(*[tensors[2 * i].data_ptr() for i in range(n)]),
                                   hidden_b=(C.c_void_p * 3)(*[tensors[2 * i + 1].data_ptr() for i in range(n)]),
                                   mu_w=tensors[2 * n].data_ptr(), mu_b=tensors[2 * n + 1].data_ptr(),
                                   log_std_w=tensors[2 * n + 2].data_ptr(), log_std_b=tensors[2 * n + 3].data_ptr())

    def _empty_like_parameters(self):
        """Fresh contiguous float32 tensors in ``nn.Linear`` shapes: the flat list (weight, bias) per hidden layer, then mu's and log_std's."""
        out, fan_in = [], self.in_total
        for width in self.widths:
            out += [torch.empty(width, fan_in, dtype=torch.float32, device=self.device), torch.empty(width, dtype=torch.float32, device=self.device)]
            fan_in = width
        for _ in range(2):
            out += [torch.empty(self.action_dim, fan_in, dtype=torch.float32, device=self.device), torch.empty(self.action_dim, dtype=torch.float32, device=self.device)]
        return out

    def _check_export_modules(self, modules):
        """(hidden, mu, log_std) with this actor's shapes, float32 on its device; ValueError otherwise."""
        try:
            hidden, mu, log_std = modules
            hidden = list(hidden)
        except (TypeError, ValueError):
            raise ValueError("modules must be (hidden layers, mu, log_std), as DeviceActor.from_linears takes them") from None
        if len(hidden) != len(self.widths):
            raise ValueError(f"modules hold {len(hidden)} hidden layers, this actor {len(self.widths)}")
        fan_in = self.in_total
        for name, m, width in [(f"hidden[{i}]", m, w) for i, (m, w) in enumerate(zip(hidden, self.widths))] + [("mu", mu, self.action_dim), ("log_std", log_std, self.action_dim)]:
            if not _is_linear(m):
                raise ValueError(f"{name}: {type(m).__name__} is not a Linear layer (weight, bias, in_features, out_features)")
            _check_parameters(name, m, "Linear", "actor", self.device)
            if name in ("mu", "log_std"):
                fan_in = self.widths[-1]
            if tuple(m.weight.shape) != (width, fan_in) or tuple(m.bias.shape) != (width,):
                raise ValueError(f"{name}: weight {tuple(m.weight.shape)} / bias {tuple(m.bias.shape)}, expected {(width, fan_in)} / {(width,)}")
            fan_in = width
        return hidden, mu, log_std

    def export(self, modules=None):
        """The packed parameters into ``modules = (hidden, mu, log_std)`` of ``torch.nn.Linear`` (default: the modules this object was
        made from), with ``copy_`` under ``no_grad``: the way back into torch after steps of a :class:`DeviceActorOptimizer`. Small
        kernels on the current stream, no synchronisation. Returns ``(hidden, mu, log_std)``. State actors only."""
        if self.visual:
            raise ValueError("a visual actor: its update is not built, and its first layer has no single nn.Linear input here")
        hidden, mu, log_std = self._check_export_modules((self.hidden, self.mu, self.log_std) if modules is None else modules)
        if self._a is None:
            raise nat.MjsError("the actor is closed")
        staged = self._empty_like_parameters()
        w = self._weights_struct(staged)
        launch = self._lib.mjs_actor_export
        stream = torch.cuda.current_stream(self.device).cuda_stream
        nat.check(launch(self._a, C.byref(w), C.c_void_p(stream)))
        with torch.no_grad():
            for k, m in enumerate((*hidden, mu, log_std)):
                m.weight.copy_(staged[2 * k])
                m.bias.copy_(staged[2 * k + 1])
        return hidden, mu, log_std

    def close(self):
        super().close()
        for e in getattr(self, "_owned_encoders", ()):
            e.close()


class DeviceCritic(_NativeObject):
    """SAC's critics (SB3's ``ContinuousCritic``: ``n_critics`` MLPs over ``[obs | action]`` with a scalar head) held by libmjsim.so
    for one device (csrc/mjs_critic.h). :meth:`q_values` and :func:`sac_td_target` take no gradient; the critic loss, its gradients
    and the Adam step run on the packed copy through :class:`DeviceCriticOptimizer` (csrc/mjs_critic_train.h), a target critic follows
    with :meth:`blend_from`, the actor loss reads the packed copy through :class:`DeviceActorOptimizer` (csrc/mjs_actor_train.h), and
    :meth:`export` writes the trained parameters back into torch modules. float32 with float32 accumulation, like :class:`DeviceActor`.

    The object keeps references to the torch modules it was made from; :meth:`load` packs their CURRENT parameters, or blends those
    of other modules of the same shapes into the packed copy (``tau < 1``: SB3's ``polyak_update``), so that a TARGET critic can
    live in the library alone: ``target = DeviceCritic.from_sb3(critic)`` once, ``target.load(critic_q_nets, tau=0.005)`` per
    gradient step."""
    _handle, _destroy = "_q", "mjs_critic_destroy"

    def __init__(self, device, obs_dim, action_dim, q_nets, activation="relu"):
        self._q = None
        if activation not in _ACTIVATION_IDS:
            raise ValueError(f"activation must be one of {sorted(_ACTIVATION_IDS)}, got {activation!r}")
        self.activation = activation
        self.obs_dim, self.action_dim = int(obs_dim), int(action_dim)
        if not 1 <= self.obs_dim <= nat.CRITIC_MAX_OBS:
            raise ValueError(f"a critic reads 1..{nat.CRITIC_MAX_OBS} observation columns, got {self.obs_dim}")
        if not 1 <= self.action_dim <= nat.ACTOR_MAX_ACTIONS:
            raise ValueError(f"a critic reads 1..{nat.ACTOR_MAX_ACTIONS} action components, got {self.action_dim}")
        self.device = torch.device(device if not isinstance(device, int) else f"cuda:{device}")
        self.q_nets = self._as_nets(q_nets)
        self.n_critics = len(self.q_nets)
        self.widths = [int(m.out_features) for m in self.q_nets[0][:-1]]
        if not 1 <= len(self.widths) <= nat.ACTOR_MAX_LAYERS:
            raise ValueError(f"a critic has 1..{nat.ACTOR_MAX_LAYERS} hidden layers, got {len(self.widths)}")
        self._check_modules(self.q_nets)
        if self.device.type == "cuda" and self.device.index is None:
            self.device = torch.device("cuda", torch.cuda.current_device())
        self._dev_index = self.device.index or 0
        # ---- native from here on
        self._lib = nat.lib()
        desc = nat.MjsCriticDesc(device=self._dev_index, obs_dim=self.obs_dim, action_dim=self.action_dim, n_critics=self.n_critics,
                                 n_hidden=len(self.widths), hidden=(C.c_int32 * 3)(*self.widths), activation=_ACTIVATION_IDS[activation])
        q = C.c_void_p()
        nat.check(self._lib.mjs_critic_create(C.byref(desc), C.byref(q)))
        self._q = q
        self._staged = ()
        self._loaded = False
        self.load()

    @classmethod
    def from_linears(cls, device, obs_dim, action_dim, q_nets, activation="relu"):
        """``q_nets``: 1..2 sequences of ``torch.nn.Linear``, each ``(hidden..., out)`` with 1..3 hidden layers of width 1..256, the
        first reading ``obs_dim + action_dim`` columns (``obs_dim`` 1..64, ``action_dim`` 1..8), ``out`` a ``Linear(., 1)``; all
        critics of one architecture, float32 on ``device``. ``ValueError`` for anything else, before any native call."""
        return cls(device, obs_dim, action_dim, q_nets, activation=activation)

    @classmethod
    def from_sb3(cls, critic, action_dim=None):
        """From an object shaped like ``stable_baselines3.common.policies.ContinuousCritic``: ``critic.q_networks`` a list of
        ``nn.Sequential`` of ``Linear`` / activation (``ReLU`` or ``Tanh``, one kind) ... ``Linear(., 1)``. ``action_dim`` defaults to
        ``critic.action_space.shape[0]``; the rest of the first layer's inputs are observation columns (the features extractor is not
        evaluated: state observations only). The device is the parameters'. Duck-typed, like :meth:`DeviceActor.from_sb3`."""
        if not hasattr(critic, "q_networks"):
            raise ValueError("not an SB3-shaped critic: no attribute 'q_networks'")
        q_nets, kinds = [], set()
        for net in critic.q_networks:
            layers = []
            for m in net:
                if _is_linear(m):
                    layers.append(m)
                elif isinstance(m, torch.nn.ReLU):
                    kinds.add("relu")
                elif isinstance(m, torch.nn.Tanh):
                    kinds.add("tanh")
                else:
                    raise ValueError(f"a q network holds a {type(m).__name__}: only Linear, ReLU and Tanh are built")
            q_nets.append(layers)
        if len(kinds) > 1:
            raise ValueError("the q networks mix ReLU and Tanh")
        if not q_nets or not q_nets[0]:
            raise ValueError("q_networks holds no Linear layer")
        if action_dim is None:
            space = getattr(critic, "action_space", None)
            if space is None or not getattr(space, "shape", None):
                raise ValueError("the critic has no action_space.shape: give action_dim")
            action_dim = int(space.shape[0])
        first = q_nets[0][0]
        return cls(first.weight.device, int(first.in_features) - int(action_dim), action_dim, q_nets, activation=kinds.pop() if kinds else "relu")

    @staticmethod
    def _as_nets(q_nets):
        try:
            nets = [list(net) for net in q_nets]
        except TypeError:
            raise ValueError("q_nets must be a list of 1..2 sequences of Linear layers (hidden..., out)") from None
        if not 1 <= len(nets) <= nat.CRITIC_MAX_CRITICS:
            raise ValueError(f"1..{nat.CRITIC_MAX_CRITICS} critics, got {len(nets)}")
        for c, net in enumerate(nets):
            if len(net) < 2:
                raise ValueError(f"q_nets[{c}] needs at least one hidden layer and the output layer")
            for m in net:
                if not _is_linear(m):
                    raise ValueError(f"{type(m).__name__} is not a Linear layer (weight, bias, in_features, out_features)")
        return nets

    def _check_modules(self, nets):
        """Shapes, dtype and device of the modules' current parameters; ValueError before anything native sees them."""
        if len(nets) != self.n_critics:
            raise ValueError(f"this object holds {self.n_critics} critics, got {len(nets)}")
        for c, net in enumerate(nets):
            if len(net) != len(self.widths) + 1:
                raise ValueError(f"q_nets[{c}] has {len(net) - 1} hidden layers, the critics of one object share an architecture ({len(self.widths)})")
            fan_in = self.obs_dim + self.action_dim
            for l, (m, width) in enumerate(zip(net, [*self.widths, 1])):
                name = f"q_nets[{c}][{l}]"
                if not 1 <= width <= nat.ACTOR_MAX_HIDDEN:
                    raise ValueError(f"{name}: width {width} outside 1..{nat.ACTOR_MAX_HIDDEN}")
                _check_parameters(name, m, "Linear", "critic", self.device)
                if tuple(m.weight.shape) != (width, fan_in) or tuple(m.bias.shape) != (width,):
                    raise ValueError(f"{name}: weight {tuple(m.weight.shape)} / bias {tuple(m.bias.shape)}, expected {(width, fan_in)} / {(width,)}")
                fan_in = width

    def _open(self):
        if self._q is None:
            raise nat.MjsError("the critic is closed")

    def load(self, q_nets=None, tau=1.0):
        """``packed = (1 - tau) * packed + tau * parameters`` for the CURRENT parameters of ``q_nets`` (default: the modules this object
        was made from), ``tau`` in (0, 1]; ``tau = 1`` copies. Small kernels on the current stream, no synchronisation.

        Once a :class:`DeviceCriticOptimizer` has stepped this critic, the packed copy is the master copy and the modules are stale:
        ``load()`` with no argument would overwrite the trained parameters with them. :meth:`export` is the way back into torch."""
        self._open()
        tau = float(tau)
        if not 0.0 < tau <= 1.0:
            raise ValueError(f"tau must lie in (0, 1], got {tau}")
        if not self._loaded and tau != 1.0:
            raise ValueError("a first load must have tau == 1: there is nothing to blend with yet")
        nets = self.q_nets if q_nets is None else self._as_nets(q_nets)
        self._check_modules(nets)
        staged = [[(m.weight.detach().contiguous(), m.bias.detach().contiguous()) for m in net] for net in nets]
        w = nat.MjsCriticWeights()
        for c, net in enumerate(staged):
            for l, (wt, bs) in enumerate(net[:-1]):
                w.hidden_w[c][l], w.hidden_b[c][l] = wt.data_ptr(), bs.data_ptr()
            w.out_w[c], w.out_b[c] = net[-1][0].data_ptr(), net[-1][1].data_ptr()
        load = self._lib.mjs_critic_load
        stream = torch.cuda.current_stream(self.device).cuda_stream
        nat.check(load(self._q, C.byref(w), tau, C.c_void_p(stream)))
        self._staged = staged  # alive until the next load: the pack kernels read them asynchronously
        self._loaded = True

    def q_values(self, obs, actions):
        """float32 ``obs`` [B, obs_dim] and ``actions`` [B, action_dim] on the device -> float32 [n_critics, B], one launch on the current
        stream; nothing is read back."""
        from .replay import _want

        self._open()
        if not isinstance(obs, torch.Tensor) or obs.dim() != 2:
            raise ValueError("obs must be a float32 tensor [B, obs_dim]")
        B = int(obs.shape[0])
        _want("obs", obs, (B, self.obs_dim), torch.float32, self.device)
        _want("actions", actions, (B, self.action_dim), torch.float32, self.device)
        q = torch.empty(self.n_critics, B, dtype=torch.float32, device=self.device)
        if B:
            launch = self._lib.mjs_critic_q
            stream = torch.cuda.current_stream(self.device).cuda_stream
            nat.check(launch(self._q, obs.data_ptr(), actions.data_ptr(), B, q.data_ptr(), C.c_void_p(stream)))
        return q

    def _weights_struct(self, tensors):
        """mjs_critic_weights over ``tensors[c][l] = (weight, bias)``."""
        w = nat.MjsCriticWeights()
        for c, net in enumerate(tensors):
            for l, (wt, bs) in enumerate(net[:-1]):
                w.hidden_w[c][l], w.hidden_b[c][l] = wt.data_ptr(), bs.data_ptr()
            w.out_w[c], w.out_b[c] = net[-1][0].data_ptr(), net[-1][1].data_ptr()
        return w

    def _empty_like_parameters(self):
        """Fresh contiguous float32 tensors in ``nn.Linear`` shapes: ``[c][l] = (weight, bias)``."""
        out = []
        for _ in range(self.n_critics):
            net, fan_in = [], self.obs_dim + self.action_dim
            for width in [*self.widths, 1]:
                net.append((torch.empty(width, fan_in, dtype=torch.float32, device=self.device), torch.empty(width, dtype=torch.float32, device=self.device)))
                fan_in = width
            out.append(net)
        return out

    def export(self, q_nets=None):
        """The packed parameters into the ``torch.nn.Linear`` modules ``q_nets`` (default: the modules this object was made from), with
        ``copy_`` under ``no_grad``: after steps of a :class:`DeviceCriticOptimizer`, an actor loss that stays in torch sees the trained
        critic. Small kernels on the current stream, no synchronisation. Returns the modules."""
        self._open()
        nets = self.q_nets if q_nets is None else self._as_nets(q_nets)
        self._check_modules(nets)
        staged = self._empty_like_parameters()
        w = self._weights_struct(staged)
        launch = self._lib.mjs_critic_export
        stream = torch.cuda.current_stream(self.device).cuda_stream
        nat.check(launch(self._q, C.byref(w), C.c_void_p(stream)))
        with torch.no_grad():
            for net, tensors in zip(nets, staged):
                for m, (wt, bs) in zip(net, tensors):
                    m.weight.copy_(wt)
                    m.bias.copy_(bs)
        return nets

    def blend_from(self, other, tau):
        """``packed = (1 - tau) * packed + tau * other's packed`` (SB3's ``polyak_update`` between two packed copies, one launch): what a
        target critic does after every step of the online critic's optimiser. ``other``: a :class:`DeviceCritic` of the same shape on
        the same device; ``tau`` in (0, 1], ``tau = 1`` copies."""
        if not isinstance(other, DeviceCritic):
            raise ValueError(f"other must be a DeviceCritic, got {type(other).__name__}")
        tau = float(tau)
        if not 0.0 < tau <= 1.0:
            raise ValueError(f"tau must lie in (0, 1], got {tau}")
        if other.device != self.device:
            raise ValueError(f"the other critic lives on {other.device}, this one on {self.device}")
        mine, theirs = (self.obs_dim, self.action_dim, self.n_critics, self.widths, self.activation), \
                       (other.obs_dim, other.action_dim, other.n_critics, other.widths, other.activation)
        if mine != theirs:
            raise ValueError(f"the critics differ in shape: (obs_dim, action_dim, n_critics, widths, activation) {mine} against {theirs}")
        if not self._loaded and tau != 1.0:
            raise ValueError("a critic without parameters takes tau == 1 only: there is nothing to blend with yet")
        self._open()
        other._open()
        blend = self._lib.mjs_critic_blend
        stream = torch.cuda.current_stream(self.device).cuda_stream
        nat.check(blend(self._q, other._q, tau, C.c_void_p(stream)))
        self._loaded = True


class DeviceCriticOptimizer(_NativeObject):
    """The critic update of SB3's ``SAC.train`` on a :class:`DeviceCritic`'s packed parameters (csrc/mjs_critic_train.h)::

        critic_loss = 0.5 * sum(F.mse_loss(q, target) for q in critic(obs, actions))
        critic.optimizer.zero_grad(); critic_loss.backward(); critic.optimizer.step()        # torch.optim.Adam, SB3's defaults

    as two launches per :meth:`step`: the forward and backward pass with a bitwise reproducible sum over the batch, then Adam. The
    packed copy is the master copy from the first step on: ``critic.q_values`` and :func:`sac_td_target` see every step at once, a
    target critic follows with ``target.blend_from(critic, tau)``, ``critic.export()`` refreshes the torch modules, and
    ``critic.load()`` would overwrite the trained parameters with the stale modules. The optimiser keeps the critic alive."""
    _handle, _destroy = "_o", "mjs_critic_opt_destroy"

    def __init__(self, critic, lr=3e-4, betas=(0.9, 0.999), eps=1e-8):
        self._o = None
        if not isinstance(critic, DeviceCritic):
            raise ValueError(f"critic must be a DeviceCritic, got {type(critic).__name__}")
        self.lr = self._checked_lr(lr)
        try:
            beta1, beta2 = (float(b) for b in betas)
        except (TypeError, ValueError):
            raise ValueError("betas must be two floats in [0, 1)") from None
        if not (0.0 <= beta1 < 1.0 and 0.0 <= beta2 < 1.0):
            raise ValueError(f"betas must lie in [0, 1), got {(beta1, beta2)}")
        eps = float(eps)
        if not 0.0 < eps < float("inf"):
            raise ValueError(f"eps must be positive and finite, got {eps}")
        self.betas, self.eps = (beta1, beta2), eps
        self.critic, self.device = critic, critic.device
        self.step_count = 0
        critic._open()
        # ---- native from here on
        self._lib = critic._lib
        desc = nat.MjsCriticOptDesc(lr=self.lr, beta1=beta1, beta2=beta2, eps=eps)
        o = C.c_void_p()
        nat.check(self._lib.mjs_critic_opt_create(critic._q, C.byref(desc), C.byref(o)))
        self._o = o

    @staticmethod
    def _checked_lr(lr):
        try:
            lr = float(lr)
        except (TypeError, ValueError):
            raise ValueError(f"lr must be a float, got {type(lr).__name__}") from None
        if not 0.0 <= lr < float("inf"):
            raise ValueError(f"lr must be finite and >= 0, got {lr}")
        return lr

    def _batch(self, batch, target):
        """(obs, actions, target, B) checked; ValueError before anything native."""
        from .replay import _want

        c = self.critic
        if not isinstance(batch, dict) or any(k not in batch for k in ("obs", "actions")):
            raise ValueError("batch must be a dict with 'obs' and 'actions' (DeviceReplayBuffer.sample's result)")
        obs = batch["obs"]
        if not isinstance(obs, torch.Tensor) or obs.dim() != 2:
            raise ValueError("batch['obs'] must be a float32 tensor [B, obs_dim]")
        B = int(obs.shape[0])
        _want("batch['obs']", obs, (B, c.obs_dim), torch.float32, self.device)
        _want("batch['actions']", batch["actions"], (B, c.action_dim), torch.float32, self.device)
        _want("target", target, (B,), torch.float32, self.device)
        return obs, batch["actions"], target, B

    def _open(self):
        self.critic._open()
        if self._o is None:
            raise nat.MjsError("the optimiser is closed")

    def _args(self, obs, actions, target, B, q, loss, grads=None):
        return nat.MjsCriticGradArgs(B=B, obs_dev=obs.data_ptr(), actions_dev=actions.data_ptr(), target_dev=target.data_ptr(),
                                     q_out_dev=q.data_ptr() if q is not None else None, loss_out_dev=loss.data_ptr() if loss is not None else None,
                                     grads_out=C.pointer(grads) if grads is not None else None)

    def step(self, batch, target, lr=None, return_parts=False):
        """One gradient step on ``batch`` (:meth:`DeviceReplayBuffer.sample`'s dict: float32 ``obs`` [B, obs_dim] and ``actions``
        [B, action_dim]) towards ``target`` float32 [B] (:func:`sac_td_target`), with the learning rate ``lr`` (default: the
        constructor's; SB3 evaluates its schedule per ``train``). Two launches on the current stream; nothing is read back. Returns
        ``None``, or with ``return_parts`` a dict with ``loss`` [n_critics] (``mean((q_c - target)^2)`` BEFORE the step) and ``q``
        [n_critics, B]. An empty batch does nothing and is not counted."""
        obs, actions, target, B = self._batch(batch, target)
        lr = self.lr if lr is None else self._checked_lr(lr)
        self._open()
        c = self.critic
        q = loss = None
        if return_parts:
            q = torch.empty(c.n_critics, B, dtype=torch.float32, device=self.device)
            loss = torch.zeros(c.n_critics, dtype=torch.float32, device=self.device)
        if B:
            args = self._args(obs, actions, target, B, q, loss)
            update = self._lib.mjs_critic_update
            stream = torch.cuda.current_stream(self.device).cuda_stream
            nat.check(update(self._o, C.byref(args), lr, C.c_void_p(stream)))
            self.step_count += 1
        return {"loss": loss, "q": q} if return_parts else None

    def gradients(self, batch, target):
        """The gradients :meth:`step` would apply, and no update: a dict with ``grads`` (per critic a list of ``(weight_grad,
        bias_grad)`` in ``nn.Linear`` shapes, hidden layers then the head), ``q`` [n_critics, B] and ``loss`` [n_critics]."""
        obs, actions, target, B = self._batch(batch, target)
        self._open()
        c = self.critic
        q = torch.empty(c.n_critics, B, dtype=torch.float32, device=self.device)
        loss = torch.zeros(c.n_critics, dtype=torch.float32, device=self.device)
        grads = c._empty_like_parameters()
        if B:
            args = self._args(obs, actions, target, B, q, loss, c._weights_struct(grads))
            grad = self._lib.mjs_critic_grad
            stream = torch.cuda.current_stream(self.device).cuda_stream
            nat.check(grad(c._q, self._o, C.byref(args), C.c_void_p(stream)))
        else:
            for net in grads:
                for wt, bs in net:
                    wt.zero_()
                    bs.zero_()
        return {"grads": grads, "q": q, "loss": loss}


def sac_td_target(batch, actor, critic, gamma, ent_coef, z=None, generator=None, return_parts=False):
    """The no-gradient half of SB3's ``SAC.train`` in ONE launch (csrc/mjs_critic.h)::

        a', logp = actor.action_log_prob(next_obs);  target = r + (1 - done) * gamma * (min_c Q_c(next_obs, a') - ent_coef * logp)

    ``batch``: what :meth:`DeviceReplayBuffer.sample` returns, or any dict with float32 ``next_obs`` [B, D], ``rewards`` [B] and ``dones``
    [B] on the device; the batch's columns are the actor's inputs, in order. ``actor``: a state :class:`DeviceActor`, ``critic``: the
    (target) :class:`DeviceCritic`, of the same widths D and A. ``ent_coef``: a float, or a one-element float32 device tensor (SB3's
    learned coefficient, read by the kernel: no synchronisation). ``z``: float32 [B, A] standard-normal draws (default
    ``torch.randn(B, A, generator=generator)`` on the device). Returns ``target`` float32 [B]; with ``return_parts`` a dict with
    ``target``, ``next_actions`` [B, A], ``next_log_prob`` [B] and ``q_next`` [n_critics, B] (before the min). All argument checks raise
    ``ValueError`` before any native call; nothing is read back."""
    from .replay import _want

    if not isinstance(actor, DeviceActor):
        raise ValueError(f"actor must be a DeviceActor, got {type(actor).__name__}")
    if not isinstance(critic, DeviceCritic):
        raise ValueError(f"critic must be a DeviceCritic, got {type(critic).__name__}")
    if actor.visual:
        raise ValueError("a visual actor: visual critics are not built (state observations only)")
    if actor.device != critic.device:
        raise ValueError(f"the actor lives on {actor.device}, the critic on {critic.device}")
    if actor.in_dim != critic.obs_dim:
        raise ValueError(f"the actor reads {actor.in_dim} observation columns, the critic {critic.obs_dim}")
    if actor.action_dim != critic.action_dim:
        raise ValueError(f"the actor has {actor.action_dim} action components, the critic {critic.action_dim}")
    gamma = float(gamma)
    if not 0.0 <= gamma <= 1.0:
        raise ValueError(f"gamma must lie in [0, 1], got {gamma}")
    dev, D, A = critic.device, critic.obs_dim, critic.action_dim
    if not isinstance(batch, dict) or any(k not in batch for k in ("next_obs", "rewards", "dones")):
        raise ValueError("batch must be a dict with 'next_obs', 'rewards' and 'dones' (DeviceReplayBuffer.sample's result)")
    next_obs = batch["next_obs"]
    if not isinstance(next_obs, torch.Tensor) or next_obs.dim() != 2:
        raise ValueError("batch['next_obs'] must be a float32 tensor [B, obs_dim]")
    B = int(next_obs.shape[0])
    if int(next_obs.shape[1]) != D:
        raise ValueError(f"batch['next_obs'] has {int(next_obs.shape[1])} columns, the actor and the critic read {D}")
    _want("batch['next_obs']", next_obs, (B, D), torch.float32, dev)
    _want("batch['rewards']", batch["rewards"], (B,), torch.float32, dev)
    _want("batch['dones']", batch["dones"], (B,), torch.float32, dev)
    ent_dev = None
    if isinstance(ent_coef, torch.Tensor):
        ent_dev = _want("ent_coef", ent_coef, tuple(ent_coef.shape) if ent_coef.numel() == 1 and ent_coef.dim() <= 1 else (1,), torch.float32, dev)
        ent_coef = 0.0
    else:
        try:
            ent_coef = float(ent_coef)
        except (TypeError, ValueError):
            raise ValueError(f"ent_coef must be a float or a one-element float32 tensor, got {type(ent_coef).__name__}") from None
    if z is not None:
        _want("z", z, (B, A), torch.float32, dev)
    if actor._a is None:
        raise nat.MjsError("the actor is closed")
    critic._open()
    if z is None:
        z = torch.randn(B, A, dtype=torch.float32, device=dev, generator=generator)
    out = {"target": torch.empty(B, dtype=torch.float32, device=dev)}
    if return_parts:
        out.update(next_actions=torch.empty(B, A, dtype=torch.float32, device=dev), next_log_prob=torch.empty(B, dtype=torch.float32, device=dev),
                   q_next=torch.empty(critic.n_critics, B, dtype=torch.float32, device=dev))
    if B:
        args = nat.MjsTdTargetArgs(B=B, next_obs_dev=next_obs.data_ptr(), rewards_dev=batch["rewards"].data_ptr(), dones_dev=batch["dones"].data_ptr(),
                                   z_dev=z.data_ptr(), gamma=gamma, ent_coef=ent_coef, ent_coef_dev=ent_dev.data_ptr() if ent_dev is not None else None,
                                   target_out_dev=out["target"].data_ptr(),
                                   next_actions_out_dev=out["next_actions"].data_ptr() if return_parts else None,
                                   next_log_prob_out_dev=out["next_log_prob"].data_ptr() if return_parts else None,
                                   q_next_out_dev=out["q_next"].data_ptr() if return_parts else None)
        launch = critic._lib.mjs_sac_td_target
        stream = torch.cuda.current_stream(dev).cuda_stream
        nat.check(launch(actor._a, critic._q, C.byref(args), C.c_void_p(stream)))
    return out if return_parts else out["target"]


class DeviceEntropyCoef:
    """SB3's learned entropy coefficient (``ent_coef="auto"``) as one small device tensor: ``log_ent_coef``, ``ent_coef = exp(log_ent_coef)``
    and Adam's two moments, plus the step count on the host. :meth:`DeviceActorOptimizer.step` updates it in the same call, after its old
    value was used (csrc/mjs_actor_train.h ent_kernel)::

        ent_coef_loss = -(log_ent_coef * (log_prob + target_entropy).detach()).mean();  Adam step on log_ent_coef

    ``.ent_coef`` is the one-element device view :func:`sac_td_target` accepts; nothing is ever read back. ``init`` is SB3's
    ``ent_coef="auto_<init>"`` (default 1.0), ``target_entropy`` defaults to ``-action_dim``."""

    def __init__(self, device, action_dim, init=1.0, lr=3e-4, target_entropy=None, betas=(0.9, 0.999), eps=1e-8):
        try:
            action_dim, init = int(action_dim), float(init)
        except (TypeError, ValueError):
            raise ValueError("action_dim must be an int and init a float") from None
        if not 1 <= action_dim <= nat.ACTOR_MAX_ACTIONS:
            raise ValueError(f"action_dim must lie in 1..{nat.ACTOR_MAX_ACTIONS}, got {action_dim}")
        if not 0.0 < init < float("inf"):
            raise ValueError(f"init must be positive and finite, got {init}")
        self.lr = DeviceCriticOptimizer._checked_lr(lr)
        try:
            beta1, beta2 = (float(b) for b in betas)
        except (TypeError, ValueError):
            raise ValueError("betas must be two floats in [0, 1)") from None
        if not (0.0 <= beta1 < 1.0 and 0.0 <= beta2 < 1.0):
            raise ValueError(f"betas must lie in [0, 1), got {(beta1, beta2)}")
        eps = float(eps)
        if not 0.0 < eps < float("inf"):
            raise ValueError(f"eps must be positive and finite, got {eps}")
        self.betas, self.eps = (beta1, beta2), eps
        try:
            self.target_entropy = float(-action_dim if target_entropy is None else target_entropy)
        except (TypeError, ValueError):
            raise ValueError("target_entropy must be a float") from None
        if self.target_entropy != self.target_entropy or abs(self.target_entropy) == float("inf"):
            raise ValueError(f"target_entropy must be finite, got {self.target_entropy}")
        self.action_dim = action_dim
        self.device = torch.device(device if not isinstance(device, int) else f"cuda:{device}")
        if self.device.type == "cuda" and self.device.index is None:
            self.device = torch.device("cuda", torch.cuda.current_device())
        log_init = torch.log(torch.ones(1, dtype=torch.float32) * init)  # SB3: th.log(th.ones(1) * init_value)
        self._state = torch.cat([log_init, log_init.exp(), torch.zeros(2)]).to(self.device)  # log_ent_coef, ent_coef, m, v
        self.step_count = 0

    @property
    def log_ent_coef(self):
        return self._state[0:1]

    @property
    def ent_coef(self):
        return self._state[1:2]

    def _block(self, lr=None):
        """mjs_entropy_step for the NEXT step (t = step_count + 1)."""
        base = self._state.data_ptr()
        return nat.MjsEntropyStep(log_ent_coef_dev=base, ent_coef_dev=base + 4, m_dev=base + 8, v_dev=base + 12, t=self.step_count + 1,
                                  lr=self.lr if lr is None else lr, beta1=self.betas[0], beta2=self.betas[1], eps=self.eps, target_entropy=self.target_entropy)


class DeviceActorOptimizer(_NativeObject):
    """The actor update of SB3's ``SAC.train`` on a :class:`DeviceActor`'s packed parameters (csrc/mjs_actor_train.h)::

        a, log_prob = actor.action_log_prob(obs)
        actor_loss = (ent_coef * log_prob - min_c Q_c(obs, a)).mean()
        actor.optimizer.zero_grad(); actor_loss.backward(); actor.optimizer.step()            # torch.optim.Adam, SB3's defaults

    as two launches per :meth:`step` (three with a learned entropy coefficient): the forward pass of the actor and the critics, the backward
    pass through the critics' inputs and the actor with a bitwise reproducible sum over the batch, then Adam. The critics are only read.
    The packed copy is the master copy from the first step on: ``venv.actor_actions``, ``venv.actor_rollout`` and :func:`sac_td_target`
    see every step at once, ``actor.export()`` refreshes the torch modules, and ``actor.load()`` would overwrite the trained parameters
    with the stale modules. The optimiser keeps the actor alive."""
    _handle, _destroy = "_o", "mjs_actor_opt_destroy"

    def __init__(self, actor, lr=3e-4, betas=(0.9, 0.999), eps=1e-8):
        self._o = None
        if not isinstance(actor, DeviceActor):
            raise ValueError(f"actor must be a DeviceActor, got {type(actor).__name__}")
        if actor.visual:
            raise ValueError("a visual actor: its update is not built (state observations only)")
        self.lr = DeviceCriticOptimizer._checked_lr(lr)
        try:
            beta1, beta2 = (float(b) for b in betas)
        except (TypeError, ValueError):
            raise ValueError("betas must be two floats in [0, 1)") from None
        if not (0.0 <= beta1 < 1.0 and 0.0 <= beta2 < 1.0):
            raise ValueError(f"betas must lie in [0, 1), got {(beta1, beta2)}")
        eps = float(eps)
        if not 0.0 < eps < float("inf"):
            raise ValueError(f"eps must be positive and finite, got {eps}")
        self.betas, self.eps = (beta1, beta2), eps
        self.actor, self.device = actor, actor.device
        self.step_count = 0
        if actor._a is None:
            raise nat.MjsError("the actor is closed")
        # ---- native from here on
        self._lib = actor._lib
        desc = nat.MjsActorOptDesc(lr=self.lr, beta1=beta1, beta2=beta2, eps=eps)
        o = C.c_void_p()
        nat.check(self._lib.mjs_actor_opt_create(actor._a, C.byref(desc), C.byref(o)))
        self._o = o

    def _checked(self, batch, critic, ent_coef, z):
        """(obs, B, ent_coef float, ent_coef tensor or None, DeviceEntropyCoef or None) checked; ValueError before anything native."""
        from .replay import _want

        a = self.actor
        if not isinstance(critic, DeviceCritic):
            raise ValueError(f"critic must be a DeviceCritic, got {type(critic).__name__}")
        if a.device != critic.device:
            raise ValueError(f"the actor lives on {a.device}, the critic on {critic.device}")
        if a.in_dim != critic.obs_dim:
            raise ValueError(f"the actor reads {a.in_dim} observation columns, the critic {critic.obs_dim}")
        if a.action_dim != critic.action_dim:
            raise ValueError(f"the actor has {a.action_dim} action components, the critic {critic.action_dim}")
        if not isinstance(batch, dict) or "obs" not in batch:
            raise ValueError("batch must be a dict with 'obs' (DeviceReplayBuffer.sample's result)")
        obs = batch["obs"]
        if not isinstance(obs, torch.Tensor) or obs.dim() != 2:
            raise ValueError("batch['obs'] must be a float32 tensor [B, obs_dim]")
        B = int(obs.shape[0])
        _want("batch['obs']", obs, (B, a.in_dim), torch.float32, self.device)
        learned = ent_dev = None
        if isinstance(ent_coef, DeviceEntropyCoef):
            if ent_coef.device != self.device:
                raise ValueError(f"the entropy coefficient lives on {ent_coef.device}, the actor on {self.device}")
            if ent_coef.action_dim != a.action_dim:
                raise ValueError(f"the entropy coefficient was made for {ent_coef.action_dim} action components, the actor has {a.action_dim}")
            learned, ent_dev, ent = ent_coef, ent_coef.ent_coef, 0.0
        elif isinstance(ent_coef, torch.Tensor):
            ent_dev = _want("ent_coef", ent_coef, tuple(ent_coef.shape) if ent_coef.numel() == 1 and ent_coef.dim() <= 1 else (1,), torch.float32, self.device)
            ent = 0.0
        else:
            try:
                ent = float(ent_coef)
            except (TypeError, ValueError):
                raise ValueError(f"ent_coef must be a float, a one-element float32 tensor or a DeviceEntropyCoef, got {type(ent_coef).__name__}") from None
        if z is not None:
            _want("z", z, (B, a.action_dim), torch.float32, self.device)
        return obs, B, ent, ent_dev, learned

    def _open(self, critic):
        if self.actor._a is None:
            raise nat.MjsError("the actor is closed")
        critic._open()
        if self._o is None:
            raise nat.MjsError("the optimiser is closed")

    def _parts(self, critic, B):
        dev, A = self.device, self.actor.action_dim
        return {"actions": torch.empty(B, A, dtype=torch.float32, device=dev), "log_prob": torch.empty(B, dtype=torch.float32, device=dev),
                "q_pi": torch.empty(critic.n_critics, B, dtype=torch.float32, device=dev),
                "min_q_action_grad": torch.empty(B, A, dtype=torch.float32, device=dev), "loss": torch.zeros(1, dtype=torch.float32, device=dev)}

    @staticmethod
    def _args(obs, z, critic, B, ent, ent_dev, parts, grads=None, entropy=None):
        ptr = lambda k: parts[k].data_ptr() if parts is not None else None  # noqa: E731
        return nat.MjsActorGradArgs(B=B, obs_dev=obs.data_ptr(), z_dev=z.data_ptr(), critic=critic._q, ent_coef=ent,
                                    ent_coef_dev=ent_dev.data_ptr() if ent_dev is not None else None, actions_out_dev=ptr("actions"),
                                    log_prob_out_dev=ptr("log_prob"), q_pi_out_dev=ptr("q_pi"), min_q_action_grad_out_dev=ptr("min_q_action_grad"),
                                    loss_out_dev=ptr("loss"), grads_out=C.pointer(grads) if grads is not None else None,
                                    entropy=C.pointer(entropy) if entropy is not None else None)

    def step(self, batch, critic, ent_coef, z=None, generator=None, lr=None, return_parts=False):
        """One gradient step of the actor on ``batch['obs']`` (float32 [B, obs_dim]; the batch's columns are the actor's inputs, in order)
        through ``critic`` (the ONLINE :class:`DeviceCritic`, after its own step). ``ent_coef``: a float, a one-element float32 device tensor, or
        a :class:`DeviceEntropyCoef`, which is updated by the same call AFTER its old value was used for both losses, as SB3 does.
        ``z``: float32 [B, A] standard-normal draws (default ``torch.randn(B, A, generator=generator)`` on the device). ``lr``: this step's
        learning rate for the actor (default: the constructor's). Two or three launches on the current stream; nothing is read back.
        Returns ``None``, or with ``return_parts`` a dict with ``actions`` [B, A], ``log_prob`` [B], ``q_pi`` [n_critics, B],
        ``min_q_action_grad`` [B, A] and ``loss`` [1] (the actor loss BEFORE the step). An empty batch does nothing and is not counted."""
        obs, B, ent, ent_dev, learned = self._checked(batch, critic, ent_coef, z)
        lr = self.lr if lr is None else DeviceCriticOptimizer._checked_lr(lr)
        self._open(critic)
        parts = self._parts(critic, B) if return_parts else None
        if B:
            if z is None:
                z = torch.randn(B, self.actor.action_dim, dtype=torch.float32, device=self.device, generator=generator)
            block = learned._block() if learned is not None else None
            args = self._args(obs, z, critic, B, ent, ent_dev, parts, entropy=block)
            update = self._lib.mjs_actor_update
            stream = torch.cuda.current_stream(self.device).cuda_stream
            nat.check(update(self._o, C.byref(args), lr, C.c_void_p(stream)))
            self.step_count += 1
            if learned is not None:
                learned.step_count += 1
        return parts

    def gradients(self, batch, critic, ent_coef, z):
        """The gradients :meth:`step` would apply, and no update (a :class:`DeviceEntropyCoef` is read, not stepped): a dict with ``grads``
        (a list of ``(weight_grad, bias_grad)`` in ``nn.Linear`` shapes: the hidden layers, then mu, then log_std) and the parts of
        :meth:`step`."""
        if z is None:
            raise ValueError("z must be given: float32 [B, action_dim] standard-normal draws")
        obs, B, ent, ent_dev, _ = self._checked(batch, critic, ent_coef, z)
        self._open(critic)
        parts = self._parts(critic, B)
        flat = self.actor._empty_like_parameters()
        if B:
            args = self._args(obs, z, critic, B, ent, ent_dev, parts, grads=self.actor._weights_struct(flat))
            grad = self._lib.mjs_actor_grad
            stream = torch.cuda.current_stream(self.device).cuda_stream
            nat.check(grad(self.actor._a, self._o, C.byref(args), C.c_void_p(stream)))
        else:
            for t in flat:
                t.zero_()
        return {"grads": [(flat[2 * k], flat[2 * k + 1]) for k in range(len(flat) // 2)], **parts}


def sac_gradient_step(batch, actor, critic, target_critic, critic_opt, actor_opt, ent_coef, gamma, tau, z_next=None, z_pi=None, generator=None):
    """One whole gradient step of SB3's ``SAC.train`` on the device, in SB3's order, with no native code of its own:

    1. :func:`sac_td_target` on ``target_critic`` with the entropy coefficient from BEFORE this step;
    2. ``critic_opt.step(batch, target)``;
    3. ``actor_opt.step(batch, critic, ent_coef)``, which also moves a :class:`DeviceEntropyCoef`;
    4. ``target_critic.blend_from(critic, tau)``.

    ``batch``: :meth:`DeviceReplayBuffer.sample`'s dict. ``z_next`` / ``z_pi``: the standard-normal draws of the target's and the actor
    loss's action samples (default: fresh ones from ``generator``, which both share: ``z_next`` is drawn first, in step 1, then ``z_pi``,
    in step 3). Every argument check raises ``ValueError``, and a closed object ``MjsError``, before any native call; nothing is read back.
    Returns ``None``."""
    if not isinstance(critic_opt, DeviceCriticOptimizer):
        raise ValueError(f"critic_opt must be a DeviceCriticOptimizer, got {type(critic_opt).__name__}")
    if not isinstance(actor_opt, DeviceActorOptimizer):
        raise ValueError(f"actor_opt must be a DeviceActorOptimizer, got {type(actor_opt).__name__}")
    if critic_opt.critic is not critic:
        raise ValueError("critic_opt was made for another critic")
    if actor_opt.actor is not actor:
        raise ValueError("actor_opt was made for another actor")
    if not isinstance(target_critic, DeviceCritic):
        raise ValueError(f"target_critic must be a DeviceCritic, got {type(target_critic).__name__}")
    if target_critic is critic:
        raise ValueError("target_critic and critic are one object")
    if not isinstance(batch, dict) or any(k not in batch for k in ("obs", "actions", "next_obs", "rewards", "dones")):
        raise ValueError("batch must be a dict with 'obs', 'actions', 'next_obs', 'rewards' and 'dones' (DeviceReplayBuffer.sample's result)")
    tau = float(tau)
    if not 0.0 < tau <= 1.0:
        raise ValueError(f"tau must lie in (0, 1], got {tau}")
    mine, theirs = (target_critic.obs_dim, target_critic.action_dim, target_critic.n_critics, target_critic.widths, target_critic.activation), \
                   (critic.obs_dim, critic.action_dim, critic.n_critics, critic.widths, critic.activation)
    if mine != theirs or target_critic.device != critic.device:
        raise ValueError(f"the target critic differs from the critic: (obs_dim, action_dim, n_critics, widths, activation) {mine} against {theirs}")
    # the remaining checks of the later calls, before the first launch
    from .replay import _want

    _, B, _, _, _ = actor_opt._checked(batch, critic, ent_coef, z_pi)
    _want("batch['actions']", batch["actions"], (B, critic.action_dim), torch.float32, critic.device)
    for name in ("next_obs", "rewards", "dones"):
        if not isinstance(batch[name], torch.Tensor) or int(batch[name].shape[0] if batch[name].dim() else -1) != B:
            raise ValueError(f"batch[{name!r}] must be a float32 tensor of {B} rows, as batch['obs']")
    alpha = ent_coef.ent_coef if isinstance(ent_coef, DeviceEntropyCoef) else ent_coef
    target_critic._open()
    critic_opt._open()
    actor_opt._open(critic)
    target = sac_td_target(batch, actor, target_critic, gamma, alpha, z=z_next, generator=generator)  # (its own checks precede its launch)
    critic_opt.step(batch, target)
    actor_opt.step(batch, critic, ent_coef, z=z_pi, generator=generator)
    target_critic.blend_from(critic, tau)
