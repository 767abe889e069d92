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


def _is_linear(m) -> bool:
    return hasattr(m, "weight") and hasattr(m, "bias") and hasattr(m, "in_features") and hasattr(m, "out_features")


class DeviceActor:
    """An MLP actor (SAC's squashed Gaussian) held by libmjsim.so for the device of ``venv``.

    The object keeps references to the torch modules; :meth:`load` packs their CURRENT parameters (a training loop calls it after
    every policy update; it enqueues small kernels on the current stream and never synchronises). An actor belongs to a device and
    a shape, not to a handle: any ``HipVectorEnv`` of the same task settings on that device may use it."""

    def __init__(self, venv, hidden, mu, log_std, activation="relu", obs_keys=None, obs_index=None, variant=nat.ACTOR_VARIANT_DEFAULT):
        self._a = None
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
        self.obs_index = self._columns(venv, obs_keys, obs_index)
        self.in_dim = len(self.obs_index)
        if not 1 <= self.in_dim <= nat.ACTOR_MAX_IN:
            raise ValueError(f"an actor reads 1..{nat.ACTOR_MAX_IN} observation columns, got {self.in_dim}")
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
        index = (C.c_int32 * self.in_dim)(*self.obs_index)
        desc = nat.MjsActorDesc(device=int(venv._dev_index), in_dim=self.in_dim, n_hidden=len(hidden), hidden=(C.c_int32 * 3)(*self.widths),
                                action_dim=self.action_dim, activation=_ACTIVATION_IDS[activation], variant=int(variant), obs_index=index)
        a = C.c_void_p()
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
        parameter on another device, mismatched shapes or an unknown key, before any native call."""
        return cls(venv, hidden, mu, log_std, activation=activation, obs_keys=obs_keys, **kw)

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
        fan_in = self.in_dim
        layers = [(f"hidden[{i}]", m, w) for i, (m, w) in enumerate(zip(self.hidden, self.widths))] + [("mu", self.mu, self.action_dim), ("log_std", self.log_std, self.action_dim)]
        for name, m, width in layers:
            if not 1 <= width <= nat.ACTOR_MAX_HIDDEN:
                raise ValueError(f"{name}: width {width} outside 1..{nat.ACTOR_MAX_HIDDEN}")
            if m.bias is None:
                raise ValueError(f"{name}: a Linear without bias")
            if name in ("mu", "log_std"):
                fan_in = self.widths[-1]
            if tuple(m.weight.shape) != (width, fan_in) or tuple(m.bias.shape) != (width,):
                raise ValueError(f"{name}: weight {tuple(m.weight.shape)} / bias {tuple(m.bias.shape)}, expected {(width, fan_in)} / {(width,)}")
            for t in (m.weight, m.bias):
                if t.dtype != torch.float32:
                    raise ValueError(f"{name}: parameters are {t.dtype}; the device actor is float32 by contract (module.float())")
                if t.device != self.device:
                    raise ValueError(f"{name}: parameters live on {t.device}, the env on {self.device}")
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

    def close(self):
        if getattr(self, "_a", None):
            torch.cuda.synchronize(self.device)
            self._lib.mjs_actor_destroy(self._a)
            self._a = None

    def __del__(self):
        try:
            self.close()
        except Exception:  # noqa: BLE001
            pass
