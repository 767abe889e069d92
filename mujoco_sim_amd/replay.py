"""A replay buffer on the device: rollout blocks to SAC transitions, and batches for a learner (csrc/mjs_replay.h).

The reference trains SAC over SB3's ``ReplayBuffer`` (scripts/sb3/reach_sac.py:108-124, planar_push.py, sb3_sac.py). :class:`DeviceReplayBuffer`
restates its ``add`` / ``sample`` over the ``[T, N, ...]`` blocks :meth:`HipVectorEnv.actor_rollout` returns: which rows are transitions
under the env's auto-reset mode, what their next observation is, and how ``terminated`` / ``truncated`` become ``done`` / ``timeout``
(include/mjsim.h, next to ``mjs_replay_add``). The storage is plain torch tensors, so a learner indexes it directly; the write cursor
lives on the device, and neither :meth:`add_block` nor :meth:`sample` synchronises or reads anything back.
"""
from __future__ import annotations

import ctypes as C

import torch

from . import _native as nat
from .policies import _CAMERA_SLOTS, DeviceActor, _camera_keys

_AUTORESET_IDS = {"next_step": nat.AUTORESET_NEXT_STEP, "same_step": nat.AUTORESET_SAME_STEP}
_ROLLOUT_KEEP = ("obs", "reward", "terminated", "truncated", "is_success", "step_type", "fault", "ncon", "discount")  # actor_rollout's default


def _want(name, t, shape, dtype, device):
    """``t`` is a contiguous tensor of that shape and dtype on ``device``; ValueError with its ``name`` otherwise."""
    if not isinstance(t, torch.Tensor):
        raise ValueError(f"{name} must be a tensor, got {type(t).__name__}")
    if t.dtype != dtype:
        raise ValueError(f"{name} must be {dtype}, got {t.dtype}")
    if t.device != device:
        raise ValueError(f"{name} lives on {t.device}, the buffer on {device}")
    if tuple(t.shape) != tuple(shape):
        raise ValueError(f"{name} must have shape {tuple(shape)}, got {tuple(t.shape)}")
    if not t.is_contiguous():
        raise ValueError(f"{name} must be contiguous")
    return t


class DeviceReplayBuffer:
    """A ring of ``capacity`` SAC transitions on the device of ``venv``, filled from rollout blocks.

    ``obs_keys`` / ``obs_index`` select and order the stored observation columns exactly as :class:`DeviceActor` selects its input
    (``None``: every state key in the env's order). ``cameras``: keys of ``venv.camera_keys`` whose frames are stored with every
    transition, at ``image_size`` (an int or ``(height, width)``); images need next-step auto-reset, where the frame after an
    episode's last step still shows the terminal state. An env with ``autoreset="disabled"`` is refused.

    Storage (torch tensors, rows in ring order): ``obs`` / ``next_obs`` float32 [capacity, D], ``actions`` float32 [capacity, A] (the
    squashed actions in [-1, 1], what SB3 stores), ``rewards`` / ``dones`` float32 [capacity] (``done`` = terminated: a truncated
    episode bootstraps), ``timeouts`` uint8 [capacity], ``rgb[key]`` / ``next_rgb[key]`` uint8 [capacity, H, W, 3].
    All argument checks raise ``ValueError`` before any native call."""

    def __init__(self, venv, capacity, obs_keys=None, obs_index=None, cameras=(), image_size=None):
        self._lib = None
        self.capacity = int(capacity)
        if not 1 <= self.capacity < 2**31:
            raise ValueError(f"capacity must lie in 1..2^31 - 1, got {capacity}")
        mode = getattr(venv, "autoreset", "next_step")
        if mode not in _AUTORESET_IDS:
            raise ValueError(f"autoreset={mode!r}: a finished env stops producing transitions; use 'next_step' or 'same_step'")
        self.autoreset = mode
        self.obs_index = DeviceActor._columns(venv, obs_keys, obs_index)
        self.obs_dim = len(self.obs_index)
        if self.obs_dim > nat.REPLAY_MAX_OBS:
            raise ValueError(f"a buffer stores at most {nat.REPLAY_MAX_OBS} observation columns, got {self.obs_dim}")
        self.src_dim = int(venv.obs_dim)
        self.action_dim = int(venv.action_dim)
        if not 1 <= self.action_dim <= nat.ACTOR_MAX_ACTIONS:
            raise ValueError(f"a buffer stores 1..{nat.ACTOR_MAX_ACTIONS} action components, got {self.action_dim}")
        self.cameras = (cameras,) if isinstance(cameras, str) else tuple(cameras)
        known = _camera_keys(venv)
        for k in self.cameras:
            if k not in known:
                raise ValueError(f"unknown camera key {k!r}; this env has {list(known)}")
        if len(set(self.cameras)) != len(self.cameras):
            raise ValueError(f"cameras lists a key twice: {list(self.cameras)}")
        if len(self.cameras) > nat.REPLAY_MAX_CAMERAS:
            raise ValueError(f"at most {nat.REPLAY_MAX_CAMERAS} cameras, got {len(self.cameras)}")
        self.height = self.width = 0
        if self.cameras:
            if mode != "next_step":
                raise ValueError("images need autoreset='next_step': under same-step auto-reset the frame of the terminal state does not exist")
            if image_size is None:
                raise ValueError("cameras need an image_size")
            try:
                hw = (int(image_size),) * 2 if isinstance(image_size, int) else tuple(int(x) for x in image_size)
            except (TypeError, ValueError):
                raise ValueError(f"image_size must be an int or (height, width), got {image_size!r}") from None
            if len(hw) != 2 or hw[0] < 1 or hw[1] < 1:
                raise ValueError(f"image_size must be a positive int or (height, width), got {image_size!r}")
            self.height, self.width = hw
        elif image_size is not None:
            raise ValueError("image_size is for a buffer with cameras")
        self.device = torch.device(venv.device)
        self._dev_index = int(venv._dev_index)
        # ---- native from here on
        self._lib = nat.lib()
        cap, dev = self.capacity, self.device
        self.obs = torch.zeros(cap, self.obs_dim, dtype=torch.float32, device=dev)
        self.next_obs = torch.zeros(cap, self.obs_dim, dtype=torch.float32, device=dev)
        self.actions = torch.zeros(cap, self.action_dim, dtype=torch.float32, device=dev)
        self.rewards = torch.zeros(cap, dtype=torch.float32, device=dev)
        self.dones = torch.zeros(cap, dtype=torch.float32, device=dev)
        self.timeouts = torch.zeros(cap, dtype=torch.uint8, device=dev)
        self.rgb = {k: torch.zeros(cap, self.height, self.width, 3, dtype=torch.uint8, device=dev) for k in self.cameras}
        self.next_rgb = {k: torch.zeros(cap, self.height, self.width, 3, dtype=torch.uint8, device=dev) for k in self.cameras}
        self._cursor = torch.zeros(1, dtype=torch.int64, device=dev)  # the library's uint64: transitions ever added
        self._workspace = None
        self._index = (C.c_int32 * max(self.obs_dim, 1))(*self.obs_index)
        per_camera = lambda d: (C.c_void_p * 2)(*[d[k].data_ptr() for k in self.cameras])  # noqa: E731
        self._storage = nat.MjsReplayStorage(
            device=self._dev_index, capacity=cap, obs_dim=self.obs_dim, action_dim=self.action_dim, n_cameras=len(self.cameras), height=self.height,
            width=self.width, cursor_dev=self._cursor.data_ptr(), obs=self.obs.data_ptr() if self.obs_dim else None,
            next_obs=self.next_obs.data_ptr() if self.obs_dim else None, actions=self.actions.data_ptr(), rewards=self.rewards.data_ptr(),
            dones=self.dones.data_ptr(), timeouts=self.timeouts.data_ptr(), rgb=per_camera(self.rgb), next_rgb=per_camera(self.next_rgb))

    # ------------------------------------------------------------------ plumbing
    def _open(self):
        if self._lib is None:
            raise nat.MjsError("the buffer is closed")

    def _stream(self):
        return C.c_void_p(torch.cuda.current_stream(self.device).cuda_stream)

    def _workspace_for(self, T, N):
        need = int(self._lib.mjs_replay_workspace_bytes(T, N))
        if self._workspace is None or self._workspace.numel() < need:
            self._workspace = torch.empty(need, dtype=torch.uint8, device=self.device)
        return self._workspace

    # ------------------------------------------------------------------ filling
    def add_block(self, obs0, block, final_frames=None):
        """Append the transitions of one rollout block (plain tensors; it need not come from an env). ``obs0``: float64 [N, obs_dim],
        the observation the block's first action was computed from. ``block``: the dict :meth:`HipVectorEnv.actor_rollout` returns -
        ``obs`` float64 [T, N, obs_dim], ``reward`` float64 [T, N], ``terminated`` / ``truncated`` / ``step_type`` uint8 [T, N],
        ``squashed_actions`` float32 [T, N, A], ``terminal_obs`` like ``obs`` under same-step auto-reset, and uint8 [T, N, H, W, 3]
        frames under every camera key of the buffer (frame t taken BEFORE action t). ``final_frames``: {camera key: uint8
        [N, H, W, 3]}, rendered after the block. Four launches at most on the current stream; nothing is read back."""
        self._open()
        dev = self.device
        if not isinstance(block, dict) or "obs" not in block:
            raise ValueError("block must be a dict with the keys of actor_rollout's result ('obs', ...)")
        obs = block["obs"]
        if not isinstance(obs, torch.Tensor) or obs.dim() != 3:
            raise ValueError("block['obs'] must be a float64 tensor [T, N, obs_dim]")
        T, N = int(obs.shape[0]), int(obs.shape[1])
        if N < 1:
            raise ValueError("a block has at least one env")
        if T * N > self.capacity:
            raise ValueError(f"a block of {T} x {N} rows does not fit the capacity {self.capacity}")
        same_step = self.autoreset == "same_step"
        names = ["reward", "terminated", "truncated", "squashed_actions", "terminal_obs" if same_step else "step_type", *self.cameras]
        for k in names:
            if block.get(k) is None:
                raise ValueError(f"block has no {k!r}" + (" (actor_rollout(..., keep=(..., 'terminal_obs')))" if k == "terminal_obs" else ""))
        _want("obs0", obs0, (N, self.src_dim), torch.float64, dev)
        _want("block['obs']", obs, (T, N, self.src_dim), torch.float64, dev)
        _want("block['reward']", block["reward"], (T, N), torch.float64, dev)
        for k in ("terminated", "truncated") + (() if same_step else ("step_type",)):
            _want(f"block[{k!r}]", block[k], (T, N), torch.uint8, dev)
        if same_step:
            _want("block['terminal_obs']", block["terminal_obs"], (T, N, self.src_dim), torch.float64, dev)
        _want("block['squashed_actions']", block["squashed_actions"], (T, N, self.action_dim), torch.float32, dev)
        final_frames = dict(final_frames or {})
        for k in self.cameras:
            _want(f"block[{k!r}]", block[k], (T, N, self.height, self.width, 3), torch.uint8, dev)
            if final_frames.get(k) is None:
                raise ValueError(f"final_frames has no {k!r}: the frame after the block's last step")
            _want(f"final_frames[{k!r}]", final_frames[k], (N, self.height, self.width, 3), torch.uint8, dev)
        if T == 0:  # (an empty block needs no launch, and empty tensors have no address to pass)
            return
        blk = nat.MjsReplayBlock(T=T, N=N, src_dim=self.src_dim, autoreset=_AUTORESET_IDS[self.autoreset], obs_index=self._index, obs0=obs0.data_ptr(),
                                 obs=obs.data_ptr(), terminal_obs=block["terminal_obs"].data_ptr() if same_step else None, reward=block["reward"].data_ptr(),
                                 terminated=block["terminated"].data_ptr(), truncated=block["truncated"].data_ptr(), step_type=None if same_step else block["step_type"].data_ptr(),
                                 squashed_actions=block["squashed_actions"].data_ptr(),
                                 rgb=(C.c_void_p * 2)(*[block[k].data_ptr() for k in self.cameras]),
                                 final_rgb=(C.c_void_p * 2)(*[final_frames[k].data_ptr() for k in self.cameras]))
        nat.check(self._lib.mjs_replay_add(C.byref(self._storage), C.byref(blk), self._workspace_for(T, N).data_ptr(), self._stream()))

    def collect(self, venv, actor, T, deterministic=False, generator=None, z=None):
        """``T`` closed-loop control steps of ``actor`` on ``venv`` (:meth:`HipVectorEnv.actor_rollout`, unchanged), ingested: the
        block's first observation is a clone of ``venv.flat_obs``, the frames after its last step are rendered at the buffer's image
        size. Returns the block. Calls chain: two ``collect(T)`` leave the ring one ``collect(2 T)`` with the same draws leaves."""
        self._open()
        if torch.device(venv.device) != self.device:
            raise ValueError(f"the env lives on {venv.device}, the buffer on {self.device}")
        if int(venv.obs_dim) != self.src_dim or int(venv.action_dim) != self.action_dim:
            raise ValueError(f"the env has {venv.obs_dim} observation and {venv.action_dim} action columns, the buffer was made for {self.src_dim} and {self.action_dim}")
        if venv.autoreset != self.autoreset:
            raise ValueError(f"the env runs autoreset={venv.autoreset!r}, the buffer was made for {self.autoreset!r}")
        for k in self.cameras:
            if k not in venv.camera_keys:
                raise ValueError(f"unknown camera key {k!r}; this env has {list(venv.camera_keys)}")
        obs0 = venv.flat_obs.clone()
        keep = _ROLLOUT_KEEP + (("terminal_obs",) if self.autoreset == "same_step" else ())
        block = venv.actor_rollout(actor, T, deterministic=deterministic, generator=generator, render=bool(self.cameras), keep=keep, z=z)
        final = {k: venv.render(self.height, self.width, camera=_CAMERA_SLOTS[k]) for k in self.cameras}
        self.add_block(obs0, block, final)
        return block

    # ------------------------------------------------------------------ drawing
    def sample(self, batch_size, generator=None, draws=None):
        """A batch of ``batch_size`` transitions: rows ``draws % size`` of the ring, ``draws`` non-negative int64 [B] on the device
        (default ``torch.randint(0, 2**62, (B,), generator=generator)`` there). Returns ``obs`` / ``next_obs`` / ``actions`` /
        ``rewards`` / ``dones`` / ``timeouts`` as in the storage, ``indices`` int64 [B] (the rows used) and, with cameras, ``rgb`` /
        ``next_rgb`` {camera key: uint8 [B, H, W, 3]}. An empty buffer gives indices -1 and zero rows. Two launches at most on
        the current stream; nothing is read back (the size is read on the device)."""
        self._open()
        B = int(batch_size)
        if B < 0:
            raise ValueError("batch_size must not be negative")
        dev = self.device
        if draws is None:
            draws = torch.randint(0, 2**62, (B,), dtype=torch.int64, device=dev, generator=generator)
        _want("draws", draws, (B,), torch.int64, dev)
        out = {"obs": torch.empty(B, self.obs_dim, dtype=torch.float32, device=dev), "next_obs": torch.empty(B, self.obs_dim, dtype=torch.float32, device=dev),
               "actions": torch.empty(B, self.action_dim, dtype=torch.float32, device=dev), "rewards": torch.empty(B, dtype=torch.float32, device=dev),
               "dones": torch.empty(B, dtype=torch.float32, device=dev), "timeouts": torch.empty(B, dtype=torch.uint8, device=dev),
               "indices": torch.empty(B, dtype=torch.int64, device=dev)}
        if self.cameras:
            out["rgb"] = {k: torch.empty(B, self.height, self.width, 3, dtype=torch.uint8, device=dev) for k in self.cameras}
            out["next_rgb"] = {k: torch.empty(B, self.height, self.width, 3, dtype=torch.uint8, device=dev) for k in self.cameras}
        if B:
            per_camera = lambda name: (C.c_void_p * 2)(*[out[name][k].data_ptr() for k in self.cameras])  # noqa: E731
            batch = nat.MjsReplayBatch(idx_out=out["indices"].data_ptr(), obs=out["obs"].data_ptr() if self.obs_dim else None,
                                       next_obs=out["next_obs"].data_ptr() if self.obs_dim else None, actions=out["actions"].data_ptr(),
                                       rewards=out["rewards"].data_ptr(), dones=out["dones"].data_ptr(), timeouts=out["timeouts"].data_ptr(),
                                       rgb=per_camera("rgb"), next_rgb=per_camera("next_rgb"))
            nat.check(self._lib.mjs_replay_sample(C.byref(self._storage), draws.data_ptr(), B, C.byref(batch), self._stream()))
        return out

    # ------------------------------------------------------------------ state
    @property
    def count(self) -> int:
        """Transitions ever added. Reads the device cursor: this SYNCHRONISES with the stream (like :attr:`size`; nothing else here does)."""
        self._open()
        return int(self._cursor.item())

    @property
    def size(self) -> int:
        """Transitions held, ``min(count, capacity)``. Reads the device cursor: this SYNCHRONISES with the stream."""
        return min(self.count, self.capacity)

    def close(self):
        """Release the storage (after the work queued on it has finished)."""
        if self._lib is not None:
            if self.device.type == "cuda":
                torch.cuda.synchronize(self.device)
            self._lib = None
            self._storage = self._workspace = self._cursor = None
            self.obs = self.next_obs = self.actions = self.rewards = self.dones = self.timeouts = None
            self.rgb, self.next_rgb = {}, {}
