"""Episode statistics and policy evaluation on the device (csrc/mjs_monitor.h).

The reference's training scripts wrap the env in SB3's ``Monitor`` and run an ``EvalCallback`` next to ``SAC(...).learn``
(scripts/sb3/reach_sac.py:83,126-131, planar_push.py). :class:`DeviceEpisodeMonitor` restates ``Monitor`` + ``ep_info_buffer`` over the
``[T, N]`` blocks :meth:`HipVectorEnv.actor_rollout` / ``rollout`` / ``demonstration_rollout`` return: which rows count, where an episode
ends and in which order finished episodes enter the window (include/mjsim.h, next to ``mjs_monitor_update``). :func:`evaluate_policy`
is SB3's function of that name for a vectorised env, over the same kernels. The state is plain torch tensors; :meth:`update` neither
synchronises nor reads anything back. Deviation from ``Monitor``: returns keep full float64, they are not rounded to 6 digits.
"""
from __future__ import annotations

import ctypes as C

import torch

from . import _native as nat
from .replay import _AUTORESET_IDS, _want

_EVAL_KEEP = ("reward", "terminated", "truncated", "is_success", "step_type")


def _positive_int(name, value, low=1):
    try:
        ok = not isinstance(value, bool) and int(value) == value
    except (TypeError, ValueError):
        ok = False
    if not ok or int(value) < low:
        raise ValueError(f"{name} must be an int >= {low}, got {value!r}")
    return int(value)


def episode_targets(n_eval_episodes, num_envs):
    """SB3's ``evaluate_policy`` targets: env i runs ``(n_eval_episodes + i) // num_envs`` episodes (they sum to ``n_eval_episodes``)."""
    n, N = _positive_int("n_eval_episodes", n_eval_episodes), _positive_int("num_envs", num_envs)
    return [(n + i) // N for i in range(N)]


class DeviceEpisodeMonitor:
    """Per-env episode return / length accumulators and a window of the last ``window`` finished episodes, on the device.

    ``venv_or_num_envs``: a :class:`HipVectorEnv` (its env count, device and auto-reset mode are taken) or an env count, then with
    ``device`` (default ``cuda``'s current device). ``window``: SB3's ``stats_window_size``. ``quota``: ``None``, or one non-negative int
    per env - episodes of an env beyond its quota are ignored (its accumulators still reset), which is how ``evaluate_policy`` counts.

    State (torch tensors): ``ep_return`` float64 [N], ``ep_length`` int32 [N], ``ep_count`` int64 [N], and the ring ``ring_return`` float64
    / ``ring_length`` int32 / ``ring_success`` uint8 / ``ring_terminated`` uint8 (1 = terminated, 0 = truncated) / ``ring_env`` int32 [W]
    with its device cursor (episodes ever recorded). All argument checks raise ``ValueError`` before any native call."""

    def __init__(self, venv_or_num_envs, device=None, window=100, quota=None):
        self._lib = None
        venv = None if isinstance(venv_or_num_envs, int) and not isinstance(venv_or_num_envs, bool) else venv_or_num_envs
        if venv is not None and not hasattr(venv, "num_envs"):
            raise ValueError(f"venv_or_num_envs must be an env or an env count, got {type(venv_or_num_envs).__name__}")
        self.num_envs = _positive_int("num_envs", venv_or_num_envs if venv is None else venv.num_envs)
        if self.num_envs >= 2**31:
            raise ValueError(f"num_envs must stay below 2^31, got {self.num_envs}")
        self.window = _positive_int("window", window)
        if self.window >= 2**31:
            raise ValueError(f"window must stay below 2^31, got {self.window}")
        self.autoreset = None if venv is None else getattr(venv, "autoreset", "next_step")
        if venv is not None:
            if device is not None and torch.device(device) != torch.device(venv.device):
                raise ValueError(f"device {device} is not the env's, {venv.device}")
            self.device = torch.device(venv.device)
        else:
            self.device = torch.device("cuda" if device is None else (f"cuda:{device}" if isinstance(device, int) else device))
        if self.device.type != "cuda":
            raise ValueError(f"device must be a HIP device (torch device 'cuda:N'), got {self.device}; there is no CPU path")
        if quota is not None:
            try:
                quota = [int(q) for q in (quota.tolist() if isinstance(quota, torch.Tensor) else quota)]
            except (TypeError, ValueError):
                raise ValueError(f"quota must be None or {self.num_envs} non-negative ints, got {type(quota).__name__}") from None
            if len(quota) != self.num_envs or any(q < 0 for q in quota):
                raise ValueError(f"quota must be None or {self.num_envs} non-negative ints, got {len(quota)} entries, smallest {min(quota, default=0)}")
        # ---- native from here on
        self._lib = nat.lib()
        if self.device.index is None:
            self.device = torch.device("cuda", torch.cuda.current_device())
        dev, N, W = self.device, self.num_envs, self.window
        self.ep_return = torch.zeros(N, dtype=torch.float64, device=dev)
        self.ep_length = torch.zeros(N, dtype=torch.int32, device=dev)
        self.ep_count = torch.zeros(N, dtype=torch.int64, device=dev)
        self.quota = torch.tensor(quota, dtype=torch.int64, device=dev) if quota is not None else None
        self.ring_return = torch.zeros(W, dtype=torch.float64, device=dev)
        self.ring_length = torch.zeros(W, dtype=torch.int32, device=dev)
        self.ring_success = torch.zeros(W, dtype=torch.uint8, device=dev)
        self.ring_terminated = torch.zeros(W, dtype=torch.uint8, device=dev)
        self.ring_env = torch.zeros(W, dtype=torch.int32, device=dev)
        self._cursor = torch.zeros(1, dtype=torch.int64, device=dev)  # the library's uint64: episodes ever recorded
        self._summary = torch.zeros(len(nat.MONITOR_SUMMARY_FIELDS), dtype=torch.float64, device=dev)
        self._workspace = None
        self._state = nat.MjsMonitorState(
            device=dev.index, num_envs=N, window=W, ep_return=self.ep_return.data_ptr(), ep_length=self.ep_length.data_ptr(),
            ep_count=self.ep_count.data_ptr(), quota=self.quota.data_ptr() if self.quota is not None else None, cursor_dev=self._cursor.data_ptr(),
            ring_return=self.ring_return.data_ptr(), ring_length=self.ring_length.data_ptr(), ring_success=self.ring_success.data_ptr(),
            ring_terminated=self.ring_terminated.data_ptr(), ring_env=self.ring_env.data_ptr())

    # ------------------------------------------------------------------ plumbing
    def _open(self):
        if self._lib is None:
            raise nat.MjsError("the monitor is closed")

    def _stream(self):
        return C.c_void_p(torch.cuda.current_stream(self.device).cuda_stream)

    def _workspace_for(self, T, N):
        need = int(self._lib.mjs_monitor_workspace_bytes(T, N))
        if self._workspace is None or self._workspace.numel() < need:
            self._workspace = torch.empty(need, dtype=torch.uint8, device=self.device)
        return self._workspace

    # ------------------------------------------------------------------ filling
    def update(self, block, autoreset=None):
        """Advance over one rollout block (plain tensors; it need not come from an env): a dict with ``reward`` float64 [T, N] and
        ``terminated`` / ``truncated`` / ``is_success`` uint8 [T, N], and ``step_type`` uint8 [T, N] under next-step auto-reset - what
        ``actor_rollout`` / ``rollout`` / ``demonstration_rollout`` return. ``autoreset``: ``"next_step"`` or ``"same_step"``, the mode
        the block was made under (default: the env's the monitor was made for). Four launches on the current stream; does not
        synchronise, nothing is read back."""
        self._open()
        mode = self.autoreset if autoreset is None else autoreset
        if mode is None:
            raise ValueError("autoreset must be given ('next_step' or 'same_step'): the monitor was made from an env count, not an env")
        if mode not in _AUTORESET_IDS:
            raise ValueError(f"autoreset={mode!r}: a finished env starts no new episode; use 'next_step' or 'same_step'")
        if not isinstance(block, dict) or not isinstance(block.get("reward"), torch.Tensor) or block["reward"].dim() != 2:
            raise ValueError("block must be a dict with the keys of a rollout's result; block['reward'] a float64 tensor [T, N]")
        T, N, dev = int(block["reward"].shape[0]), self.num_envs, self.device
        if T * N >= 2**31:
            raise ValueError(f"a block of {T} x {N} rows: T * N must stay below 2^31")
        names = ("terminated", "truncated", "is_success") + (("step_type",) if mode == "next_step" else ())
        for k in names:
            if block.get(k) is None:
                raise ValueError(f"block has no {k!r}")
        _want("block['reward']", block["reward"], (T, N), torch.float64, dev)
        for k in names:
            _want(f"block[{k!r}]", block[k], (T, N), torch.uint8, dev)
        if T == 0:  # (an empty block needs no launch, and empty tensors have no address to pass)
            return
        blk = nat.MjsMonitorBlock(T=T, N=N, autoreset=_AUTORESET_IDS[mode], reward=block["reward"].data_ptr(), terminated=block["terminated"].data_ptr(),
                                  truncated=block["truncated"].data_ptr(), is_success=block["is_success"].data_ptr(),
                                  step_type=block["step_type"].data_ptr() if mode == "next_step" else None)
        nat.check(self._lib.mjs_monitor_update(C.byref(self._state), C.byref(blk), self._workspace_for(T, N).data_ptr(), self._stream()))

    # ------------------------------------------------------------------ reading
    def summary(self):
        """The window reduced on the device (one launch) and copied to the host: a dict of Python numbers - ``count`` (int),
        ``return_mean`` / ``return_std`` (population) / ``return_min`` / ``return_max`` / ``return_sum``, ``length_mean`` / ``length_sum``
        (int), ``success_rate`` / ``success_count`` (int). An empty window gives count 0 and NaN means. The one small device-to-host copy
        SYNCHRONISES with the stream: this is the monitor's synchronising call."""
        self._open()
        nat.check(self._lib.mjs_monitor_summary(C.byref(self._state), self._summary.data_ptr(), self._stream()))
        out = dict(zip(nat.MONITOR_SUMMARY_FIELDS, self._summary.cpu().tolist()))
        for k in ("count", "length_sum", "success_count"):
            out[k] = int(out[k])
        return out

    def episodes(self):
        """The live records in chronological order (oldest first) as fresh tensors: ``return`` float64, ``length`` int32, ``success`` /
        ``terminated`` uint8, ``env`` int32, each [min(count, window)]. Reads the device cursor: this SYNCHRONISES with the stream."""
        self._open()
        count, W = self.count, self.window
        K, start = min(count, W), (count % W if count > W else 0)
        idx = (torch.arange(K, device=self.device) + start) % W
        return {"return": self.ring_return[idx], "length": self.ring_length[idx], "success": self.ring_success[idx],
                "terminated": self.ring_terminated[idx], "env": self.ring_env[idx]}

    def remaining(self):
        """``sum(max(quota - ep_count, 0))`` as a device scalar (int64): the episodes still to record. Needs a quota."""
        self._open()
        if self.quota is None:
            raise ValueError("remaining() is for a monitor with a quota")
        return (self.quota - self.ep_count).clamp_min(0).sum()

    @property
    def count(self) -> int:
        """Episodes ever recorded. Reads the device cursor: this SYNCHRONISES with the stream."""
        self._open()
        return int(self._cursor.item())

    # ------------------------------------------------------------------ state
    def reset_in_flight(self):
        """Zero the per-env accumulators only (the running episodes are forgotten; the window, the counts and the cursor stay): for an
        env that was reset by hand."""
        self._open()
        self.ep_return.zero_()
        self.ep_length.zero_()

    def reset(self):
        """Zero everything: accumulators, counts, window and cursor."""
        self.reset_in_flight()
        for t in (self.ep_count, self.ring_return, self.ring_length, self.ring_success, self.ring_terminated, self.ring_env, self._cursor):
            t.zero_()

    def close(self):
        """Release the state (after the work queued on it has finished)."""
        if self._lib is not None:
            if self.device.type == "cuda":
                torch.cuda.synchronize(self.device)
            self._lib = None
            self._state = self._workspace = self._cursor = self._summary = self.quota = None
            self.ep_return = self.ep_length = self.ep_count = None
            self.ring_return = self.ring_length = self.ring_success = self.ring_terminated = self.ring_env = None


def _run_evaluation(venv, actor, n_eval_episodes, deterministic, block_steps, max_steps, generator):
    """The loop of :func:`evaluate_policy`: the monitor holding exactly ``n_eval_episodes`` records (the caller closes it)."""
    n = _positive_int("n_eval_episodes", n_eval_episodes)
    T = _positive_int("block_steps", block_steps)
    if max_steps is not None:
        max_steps = _positive_int("max_steps", max_steps)
    if n >= 2**31:
        raise ValueError(f"n_eval_episodes must stay below 2^31, got {n}")
    if getattr(venv, "autoreset", "next_step") not in _AUTORESET_IDS:
        raise ValueError(f"autoreset={venv.autoreset!r}: a finished env starts no new episode; evaluate on an env with 'next_step' or 'same_step'")
    targets = episode_targets(n, venv.num_envs)
    venv.reset()
    monitor = DeviceEpisodeMonitor(venv, window=n, quota=targets)
    try:
        steps = 0
        while True:
            monitor.update(venv.actor_rollout(actor, T, deterministic=deterministic, generator=generator, keep=_EVAL_KEEP))
            steps += T
            missing = int(monitor.remaining().item())  # one scalar per block: the loop's only synchronisation
            if missing == 0:
                return monitor
            if max_steps is not None and steps >= max_steps:
                raise nat.MjsError(f"evaluate_policy: {missing} of {n} episodes are missing after {steps} control steps per env (max_steps={max_steps})")
    except Exception:
        monitor.close()
        raise


def evaluate_policy(venv, actor, n_eval_episodes=10, deterministic=True, return_episode_rewards=False, block_steps=32, max_steps=None, generator=None):
    """SB3's ``evaluate_policy`` (stable_baselines3/common/evaluation.py) for a :class:`HipVectorEnv` and a :class:`DeviceActor`, state or
    visual: ``venv.reset()``, then blocks of ``block_steps`` control steps of ``actor_rollout`` reduced by a :class:`DeviceEpisodeMonitor`
    whose window is ``n_eval_episodes`` and whose per-env quota is SB3's target ``(n_eval_episodes + i) // num_envs``; episodes of an env
    beyond its target are ignored. After every block ONE scalar is read back, the episodes still missing (the only synchronisation); once
    ``max_steps`` control steps per env have run with episodes missing, ``MjsError`` names their number. ``generator`` gives the draws
    of a stochastic policy (``deterministic=False``). Returns ``(mean_reward, std_reward)``, computed on the device, or with
    ``return_episode_rewards`` the lists ``(returns, lengths)`` in the order SB3 appends them: by step, then by env.
    Argument checks raise ``ValueError`` before any native call."""
    monitor = _run_evaluation(venv, actor, n_eval_episodes, deterministic, block_steps, max_steps, generator)
    try:
        if return_episode_rewards:
            ep = monitor.episodes()
            return ep["return"].cpu().tolist(), ep["length"].cpu().tolist()
        s = monitor.summary()
        return s["return_mean"], s["return_std"]
    finally:
        monitor.close()
