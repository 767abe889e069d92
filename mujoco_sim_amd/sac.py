"""SAC's training loop on the device: ``SAC(...).learn(timesteps)`` of the reference's scripts/sb3/*.py over the pieces of policies.py and
replay.py, with the gradient steps of one training phase in ONE native call (csrc/mjs_sac_train.h, ``mjs_sac_train``).

:class:`DeviceSAC` restates stable_baselines3's ``SAC`` / ``OffPolicyAlgorithm.learn`` over a :class:`HipVectorEnv`: blocks of
``train_freq`` control steps collected by the device actor into a :class:`DeviceReplayBuffer`, then ``gradient_steps`` gradient steps,
each on a batch drawn by ``sac::draw_batch_kernel`` from a counter-based generator: a (seed, gradient-step counter) pair names its batch
and both action samples' draws, so a training run is reproducible bit for bit and any step of it can be redrawn (:meth:`draw_batch`).
No torch generator is involved after the warm-up, and nothing is read back except ``buffer.size`` once, when training starts.
"""
from __future__ import annotations

import ctypes as C
import math

import torch

from . import _native as nat
from .monitor import DeviceEpisodeMonitor, _run_evaluation
from .policies import DeviceActor, DeviceActorOptimizer, DeviceCritic, DeviceCriticOptimizer, DeviceEntropyCoef, _is_linear
from .replay import _ROLLOUT_KEEP, DeviceReplayBuffer

_BATCH_KEYS = ("obs", "next_obs", "actions", "rewards", "dones", "indices", "draws", "z_next", "z_pi")


def _int_in(name, value, low, what):
    try:
        ok = not isinstance(value, bool) and int(value) == value
    except (TypeError, ValueError):
        ok = False
    if not ok or int(value) < low:
        raise ValueError(f"{name} must be an int {what}, got {value!r}")
    return int(value)


def _counter(name, value):
    """A uint64: the generator's key or its gradient-step counter."""
    value = _int_in(name, value, 0, "in 0 .. 2^64 - 1")
    if value >= 2**64:
        raise ValueError(f"{name} must be an int in 0 .. 2^64 - 1, got {value}")
    return value


def _float_in(name, value, ok, what):
    try:
        value = float(value)
    except (TypeError, ValueError):
        raise ValueError(f"{name} must be a float {what}, got {type(value).__name__}") from None
    if not ok(value):
        raise ValueError(f"{name} must lie {what}, got {value}")
    return value


def _parse_ent_coef(ent_coef):
    """SB3's ``ent_coef``: (learned, value) - a fixed float, or ``"auto"`` / ``"auto_<init>"`` with the initial value."""
    if isinstance(ent_coef, str):
        if not ent_coef.startswith("auto"):
            raise ValueError(f"ent_coef must be a float, 'auto' or 'auto_<init>', got {ent_coef!r}")
        init = 1.0
        if ent_coef != "auto":
            try:
                init = float(ent_coef.split("_", 1)[1]) if "_" in ent_coef else float("nan")
            except ValueError:
                init = float("nan")
            if not 0.0 < init < float("inf"):
                raise ValueError(f"ent_coef={ent_coef!r}: the initial value after 'auto_' must be a positive float")
        return True, init
    return False, _float_in("ent_coef", ent_coef, lambda v: 0.0 <= v < float("inf"), "in [0, inf) (or be 'auto' / 'auto_<init>')")


def _parse_train_freq(train_freq):
    """An int, or SB3's ``TrainFreq(frequency, unit)`` / ``(frequency, unit)`` with unit ``"step"``."""
    freq, unit = train_freq, "step"
    if hasattr(train_freq, "frequency") and hasattr(train_freq, "unit"):
        freq, unit = train_freq.frequency, train_freq.unit
    elif isinstance(train_freq, (tuple, list)):
        if len(train_freq) != 2:
            raise ValueError(f"train_freq must be an int or (frequency, unit), got {train_freq!r}")
        freq, unit = train_freq
    unit = getattr(unit, "value", unit)
    if unit == "episode":
        raise ValueError("train_freq in episodes: the envs of a HipVectorEnv finish at different steps and a block is a fixed number of control "
                         "steps; give train_freq in steps")
    if unit != "step":
        raise ValueError(f"train_freq's unit must be 'step', got {unit!r}")
    return _int_in("train_freq", freq, 1, ">= 1 (control steps per env between training phases)")


class DeviceSAC:
    """SAC on the device of ``venv``: ``DeviceSAC(venv, actor, critic).learn(total_timesteps)``.

    ``actor``: a state :class:`DeviceActor`, ``critic``: the online :class:`DeviceCritic`; ``target_critic`` defaults to a copy of it
    (a ``tau = 1`` blend) and ``buffer`` to a :class:`DeviceReplayBuffer` of ``buffer_size`` rows over the actor's input columns. The
    keyword arguments have SB3's names, defaults and meanings: ``ent_coef`` a float, ``"auto"`` or ``"auto_<init>"``; ``train_freq`` control
    steps per env between training phases; ``gradient_steps = -1``: as many gradient steps as env steps were collected, ``train_freq *
    num_envs``; ``learning_starts`` in env steps summed over the envs; ``learning_rate`` one constant for the three optimisers.
    ``seed`` (0 .. 2^64 - 1) keys the batch generator. Every argument check raises ``ValueError`` before any native call; the trainer owns
    what it made itself (optimisers, target critic, buffer) and :meth:`close` releases that."""

    def __init__(self, venv, actor, critic, target_critic=None, buffer=None, *, buffer_size=1_000_000, batch_size=256, learning_rate=3e-4,
                 gamma=0.99, tau=0.005, ent_coef="auto", target_entropy=None, train_freq=1, gradient_steps=1, learning_starts=100,
                 target_update_interval=1, seed=0):
        self._closed = True
        hp = self._hyperparameters(buffer_size=buffer_size, batch_size=batch_size, learning_rate=learning_rate, gamma=gamma, tau=tau, ent_coef=ent_coef,
                                   target_entropy=target_entropy, train_freq=train_freq, gradient_steps=gradient_steps, learning_starts=learning_starts,
                                   target_update_interval=target_update_interval, seed=seed)
        self._check_objects(venv, actor, critic, target_critic, buffer)
        self.__dict__.update(hp)
        self.venv, self.actor, self.critic, self.device = venv, actor, critic, actor.device
        self.num_timesteps = 0       # env steps taken by learn, summed over the envs
        self.num_gradient_steps = 0  # the gradient-step counter: the next step's batch is draw_batch(num_gradient_steps)
        self.log = []                # learn's records (with log_interval or eval_freq)
        self.eval_block_steps = 32   # evaluate_policy's block_steps and max_steps for learn's evaluations: with max_steps set, an eval_env whose
        self.eval_max_steps = None   # episodes do not end raises MjsError after that many control steps per env instead of looping for ever
        self._size_checked = False
        self._scratch = None
        if actor._a is None:
            raise nat.MjsError("the actor is closed")
        critic._open()
        if target_critic is not None:
            target_critic._open()
        if buffer is not None:
            buffer._open()
        # ---- native from here on
        self._lib = critic._lib
        self._owned = []
        try:
            self.critic_opt = self._own(DeviceCriticOptimizer(critic, lr=self.learning_rate))
            self.actor_opt = self._own(DeviceActorOptimizer(actor, lr=self.learning_rate))
            if target_critic is None:
                target_critic = self._own(DeviceCritic(critic.device, critic.obs_dim, critic.action_dim, critic.q_nets, activation=critic.activation))
                target_critic.blend_from(critic, 1.0)  # the online critic's packed copy, whatever its modules hold by now
            self.target_critic = target_critic
            if buffer is None:
                buffer = self._own(DeviceReplayBuffer(venv, self.buffer_size, obs_index=actor.obs_index))
            self.buffer = buffer
            self.coef = DeviceEntropyCoef(self.device, actor.action_dim, init=self.ent_coef_init, lr=self.learning_rate,
                                          target_entropy=self.target_entropy) if self.ent_coef_learned else None
            self._scratch_for(self.batch_size)
        except Exception:
            self._release()
            raise
        self._closed = False

    # ------------------------------------------------------------------ checks (no native call)
    @staticmethod
    def _hyperparameters(*, buffer_size, batch_size, learning_rate, gamma, tau, ent_coef, target_entropy, train_freq, gradient_steps, learning_starts,
                         target_update_interval, seed):
        """The keyword arguments checked and normalised; ValueError with the argument's name otherwise."""
        learned, value = _parse_ent_coef(ent_coef)
        if target_entropy is not None and not (isinstance(target_entropy, str) and target_entropy == "auto"):
            target_entropy = _float_in("target_entropy", target_entropy, math.isfinite, "in the finite floats")
        else:
            target_entropy = None
        return dict(
            buffer_size=_int_in("buffer_size", buffer_size, 1, ">= 1"),
            batch_size=_int_in("batch_size", batch_size, 1, ">= 1"),
            learning_rate=_float_in("learning_rate", learning_rate, lambda v: 0.0 <= v < float("inf"), "in [0, inf)"),
            gamma=_float_in("gamma", gamma, lambda v: 0.0 <= v <= 1.0, "in [0, 1]"),
            tau=_float_in("tau", tau, lambda v: 0.0 < v <= 1.0, "in (0, 1]"),
            ent_coef_learned=learned, ent_coef_init=value if learned else 1.0, ent_coef_fixed=0.0 if learned else value,
            target_entropy=target_entropy,
            train_freq=_parse_train_freq(train_freq),
            gradient_steps=_int_in("gradient_steps", gradient_steps, -1, ">= 0, or -1 for as many as env steps were collected"),
            learning_starts=_int_in("learning_starts", learning_starts, 0, ">= 0 (env steps summed over the envs)"),
            target_update_interval=_int_in("target_update_interval", target_update_interval, 1, ">= 1"),
            seed=_counter("seed", seed),
        )

    @staticmethod
    def _check_objects(venv, actor, critic, target_critic, buffer):
        if not isinstance(actor, DeviceActor):
            raise ValueError(f"actor must be a DeviceActor, got {type(actor).__name__}")
        if not isinstance(critic, DeviceCritic):
            raise ValueError(f"critic must be a DeviceCritic, got {type(critic).__name__}")
        if actor.visual:
            raise ValueError("a visual actor: visual critics are not built (state observations only)")
        if actor.device != critic.device:
            raise ValueError(f"the actor lives on {actor.device}, the critic on {critic.device}")
        if torch.device(venv.device) != actor.device:
            raise ValueError(f"the env lives on {venv.device}, the actor on {actor.device}")
        if actor.in_dim != critic.obs_dim:
            raise ValueError(f"the actor reads {actor.in_dim} observation columns, the critic {critic.obs_dim}")
        if actor.action_dim != critic.action_dim:
            raise ValueError(f"the actor has {actor.action_dim} action components, the critic {critic.action_dim}")
        if int(venv.action_dim) != actor.action_dim:
            raise ValueError(f"the env has {venv.action_dim} action components, the actor {actor.action_dim}")
        if target_critic is not None:
            if not isinstance(target_critic, DeviceCritic):
                raise ValueError(f"target_critic must be a DeviceCritic, got {type(target_critic).__name__}")
            if target_critic is critic:
                raise ValueError("target_critic and critic are one object")
            mine, theirs = (target_critic.obs_dim, target_critic.action_dim, target_critic.n_critics, target_critic.widths, target_critic.activation), \
                           (critic.obs_dim, critic.action_dim, critic.n_critics, critic.widths, critic.activation)
            if mine != theirs or target_critic.device != critic.device:
                raise ValueError(f"the target critic differs from the critic: (obs_dim, action_dim, n_critics, widths, activation) {mine} against {theirs}")
        if buffer is not None:
            if not isinstance(buffer, DeviceReplayBuffer):
                raise ValueError(f"buffer must be a DeviceReplayBuffer, got {type(buffer).__name__}")
            if buffer.cameras:
                raise ValueError("the buffer stores cameras: the SAC update is state-only (visual critics are not built)")
            if buffer.device != actor.device:
                raise ValueError(f"the buffer lives on {buffer.device}, the actor on {actor.device}")
            if buffer.obs_dim != actor.in_dim or buffer.action_dim != actor.action_dim:
                raise ValueError(f"the buffer stores {buffer.obs_dim} observation and {buffer.action_dim} action columns, the networks read "
                                 f"{actor.in_dim} and {actor.action_dim}")
            if list(buffer.obs_index) != list(actor.obs_index):
                raise ValueError("the buffer's observation columns are not the actor's input columns, in order")

    # ------------------------------------------------------------------ plumbing
    def _own(self, obj):
        self._owned.append(obj)
        return obj

    def _release(self):
        for obj in reversed(getattr(self, "_owned", [])):
            obj.close()
        self._owned = []

    def _open(self):
        if self._closed:
            raise nat.MjsError("the trainer is closed")
        if self.actor._a is None:
            raise nat.MjsError("the actor is closed")
        self.critic._open()
        self.target_critic._open()
        self.critic_opt._open()
        self.actor_opt._open(self.critic)
        self.buffer._open()

    def _stream(self):
        return C.c_void_p(torch.cuda.current_stream(self.device).cuda_stream)

    def _new_batch(self, B):
        dev, D, A = self.device, self.buffer.obs_dim, self.buffer.action_dim
        f32 = lambda *shape: torch.empty(*shape, dtype=torch.float32, device=dev)  # noqa: E731
        i64 = lambda: torch.empty(B, dtype=torch.int64, device=dev)  # noqa: E731
        return {"obs": f32(B, D), "next_obs": f32(B, D), "actions": f32(B, A), "rewards": f32(B), "dones": f32(B), "indices": i64(), "draws": i64(),
                "z_next": f32(B, A), "z_pi": f32(B, A)}

    @staticmethod
    def _batch_struct(out):
        return nat.MjsSacBatch(idx_out=out["indices"].data_ptr(), draws_out=out["draws"].data_ptr(), obs=out["obs"].data_ptr(),
                               next_obs=out["next_obs"].data_ptr(), actions=out["actions"].data_ptr(), rewards=out["rewards"].data_ptr(),
                               dones=out["dones"].data_ptr(), z_next=out["z_next"].data_ptr(), z_pi=out["z_pi"].data_ptr())

    def _scratch_for(self, B):
        """The batch and target scratch of ``train`` for B rows: allocated once per batch size, overwritten by every gradient step."""
        if self._scratch is None or self._scratch[0] != B:
            out = self._new_batch(B)
            self._scratch = (B, out, self._batch_struct(out), torch.empty(B, dtype=torch.float32, device=self.device))
        return self._scratch

    def _checked_batch_size(self, batch_size):
        return self.batch_size if batch_size is None else _int_in("batch_size", batch_size, 1, ">= 1")

    @property
    def ent_coef(self):
        """What :func:`sac_gradient_step` takes as ``ent_coef``: the :class:`DeviceEntropyCoef`, or the fixed float."""
        return self.coef if self.coef is not None else self.ent_coef_fixed

    # ------------------------------------------------------------------ the gradient loop
    def draw_batch(self, step=None, batch_size=None):
        """The batch of gradient-step counter ``step`` (default: the trainer's own, the next step's) as fresh tensors: the dict
        :meth:`DeviceReplayBuffer.sample` returns, without ``timeouts``, plus ``draws`` int64 [B] (``buffer.sample(B, draws=draws)`` gathers
        the same rows), ``z_next`` and ``z_pi`` float32 [B, A], the standard-normal draws of the target's and the actor loss's action
        samples. ONE launch on the current stream (``sac::draw_batch_kernel`` alone); nothing is read back and the counter stays."""
        step = self.num_gradient_steps if step is None else _counter("step", step)
        B = self._checked_batch_size(batch_size)
        self._open()
        out = self._new_batch(B)
        batch = self._batch_struct(out)
        nat.check(self._lib.mjs_sac_draw_batch(C.byref(self.buffer._storage), C.byref(batch), B, self.seed, step, self._stream()))
        return out

    def _train_args(self, G, B):
        """mjs_sac_train_args for the next ``G`` steps at ``B`` rows over the trainer's scratch (which the struct's pointers keep alive)."""
        _, _, batch, target = self._scratch_for(B)
        coef = self.coef
        block = coef._block() if coef is not None else None
        return nat.MjsSacTrainArgs(B=B, G=G, target_update_interval=self.target_update_interval, storage=C.pointer(self.buffer._storage),
                                   actor=self.actor._a, critic=self.critic._q, target_critic=self.target_critic._q, critic_opt=self.critic_opt._o,
                                   actor_opt=self.actor_opt._o, batch=C.pointer(batch), target_dev=target.data_ptr(), seed=self.seed,
                                   step0=self.num_gradient_steps, gamma=self.gamma, tau=self.tau, critic_lr=self.learning_rate,
                                   actor_lr=self.learning_rate, ent_coef=self.ent_coef_fixed,
                                   ent_coef_dev=coef.ent_coef.data_ptr() if coef is not None else None,
                                   entropy=C.pointer(block) if block is not None else None)

    def train(self, gradient_steps, batch_size=None):
        """``gradient_steps`` gradient steps of SB3's ``SAC.train`` in ONE native call (``mjs_sac_train``): per step the batch of the trainer's
        counter, the TD target on the target critic with the coefficient from before the step, the critic update, the actor update (and
        the learned coefficient's), and the target's blend where ``target_update_interval`` says so. Plain launches on the current stream;
        nothing is read back. The step counts of both optimisers, of the coefficient and of the trainer advance, so that a hand-written
        :func:`sac_gradient_step` on ``draw_batch()`` continues the run bit for bit."""
        G = _int_in("gradient_steps", gradient_steps, 0, ">= 0")
        B = self._checked_batch_size(batch_size)
        self._open()
        if G == 0:
            return
        coef = self.coef
        args = self._train_args(G, B)
        nat.check(self._lib.mjs_sac_train(C.byref(args), self._stream()))
        self.num_gradient_steps += G
        self.critic_opt.step_count += G
        self.actor_opt.step_count += G
        if coef is not None:
            coef.step_count += G

    # ------------------------------------------------------------------ the outer loop
    def _gradient_steps_per_phase(self):
        return self.gradient_steps if self.gradient_steps >= 0 else self.train_freq * int(self.venv.num_envs)

    def _collect_uniform(self, T, generator):
        """``T`` control steps of actions uniform in the action space (SB3's warm-up) through ``venv.rollout``, ingested: u ~ U(-1, 1)
        float32 is what the buffer stores, scaled to the env's bounds by the rule ``actor_actions`` uses, in float64."""
        venv, dev = self.venv, self.device
        u = torch.rand(T, int(venv.num_envs), int(venv.action_dim), dtype=torch.float32, device=dev, generator=generator) * 2.0 - 1.0
        low = torch.as_tensor([float(x) for x in venv.action_low], dtype=torch.float64, device=dev)
        high = torch.as_tensor([float(x) for x in venv.action_high], dtype=torch.float64, device=dev)
        actions = low + (0.5 * (u.double() + 1.0) * (high - low))
        obs0 = venv.flat_obs.clone()
        same_step = self.buffer.autoreset == "same_step"
        block = dict(venv.rollout(actions, keep=_ROLLOUT_KEEP + (("terminal_obs",) if same_step else ())))
        if same_step and block.get("terminal_obs") is None:
            raise ValueError("learning_starts > 0 under autoreset='same_step': rollout does not supply 'terminal_obs', which add_block needs there")
        block["squashed_actions"] = u
        if T:
            venv.flat_obs.copy_(block["obs"][-1])  # so that the next block starts from this one's last observation
        self.buffer.add_block(obs0, block)
        return block

    def _check_reporting(self, monitor, log_interval, eval_env, eval_freq, n_eval_episodes, callback):
        """learn's reporting arguments checked (ValueError with the argument's name); True where records are to be made."""
        if monitor is not None:
            if not isinstance(monitor, DeviceEpisodeMonitor):
                raise ValueError(f"monitor must be a DeviceEpisodeMonitor, got {type(monitor).__name__}")
            if monitor.num_envs != int(self.venv.num_envs):
                raise ValueError(f"monitor was made for {monitor.num_envs} envs, the env has {self.venv.num_envs}")
            if monitor.device != torch.device(self.venv.device):
                raise ValueError(f"monitor lives on {monitor.device}, the env on {self.venv.device}")
        if log_interval is not None:
            _int_in("log_interval", log_interval, 1, ">= 1 (training phases between records)")
            if monitor is None:
                raise ValueError("log_interval needs a monitor: the records hold its statistics")
        if (eval_env is None) != (eval_freq is None):
            raise ValueError("eval_env and eval_freq go together: give both or neither")
        if eval_freq is not None:
            _int_in("eval_freq", eval_freq, 1, ">= 1 (env steps summed over the envs between evaluations)")
            _int_in("n_eval_episodes", n_eval_episodes, 1, ">= 1")
            for attr in ("num_envs", "device", "reset", "actor_rollout"):
                if not hasattr(eval_env, attr):
                    raise ValueError(f"eval_env must be a HipVectorEnv, got {type(eval_env).__name__}")
            if torch.device(eval_env.device) != self.device:
                raise ValueError(f"eval_env lives on {eval_env.device}, the actor on {self.device}")
            if getattr(eval_env, "autoreset", "next_step") not in ("next_step", "same_step"):
                raise ValueError(f"eval_env runs autoreset={eval_env.autoreset!r}: a finished env starts no new episode")
        reporting = log_interval is not None or eval_freq is not None
        if callback is not None and not callable(callback):
            raise ValueError(f"callback must be callable, got {type(callback).__name__}")
        if callback is not None and not reporting:
            raise ValueError("callback is called with every record: it needs log_interval or eval_freq")
        return reporting

    def _record(self, monitor):
        """A log record with every documented key; the statistics not taken at this point are NaN."""
        nan = float("nan")
        record = {"num_timesteps": self.num_timesteps, "num_gradient_steps": self.num_gradient_steps, "rollout/ep_rew_mean": nan, "rollout/ep_len_mean": nan,
                  "rollout/success_rate": nan, "eval/mean_reward": nan, "eval/std_reward": nan, "eval/success_rate": nan, "eval/mean_ep_length": nan}
        if monitor is not None:
            s = monitor.summary()
            record.update({"rollout/ep_rew_mean": s["return_mean"], "rollout/ep_len_mean": s["length_mean"], "rollout/success_rate": s["success_rate"]})
        return record

    def _evaluate_into(self, record, eval_env, n_eval_episodes, monitor):
        """SB3's EvalCallback step: ``n_eval_episodes`` deterministic episodes of the actor on ``eval_env``, into ``record``."""
        ev = _run_evaluation(eval_env, self.actor, n_eval_episodes, True, self.eval_block_steps, self.eval_max_steps, None)
        try:
            s = ev.summary()
        finally:
            ev.close()
        record.update({"eval/mean_reward": s["return_mean"], "eval/std_reward": s["return_std"], "eval/success_rate": s["success_rate"],
                       "eval/mean_ep_length": s["length_mean"]})
        if eval_env is self.venv:  # the training env ran the evaluation's episodes: collection continues from a reset state
            self.venv.reset()
            if monitor is not None:
                monitor.reset_in_flight()

    def learn(self, total_timesteps, generator=None, *, monitor=None, log_interval=None, eval_env=None, eval_freq=None, n_eval_episodes=5, callback=None):
        """Alternates ``buffer.collect(venv, actor, train_freq)`` with :meth:`train` until ``total_timesteps`` more env steps, summed over
        the envs, have been taken (whole blocks: ``train_freq * num_envs`` at a time). While ``num_timesteps < learning_starts`` the actions
        are uniform in the action space, drawn from ``generator``, which also gives the actor's draws afterwards; training starts once
        ``num_timesteps > learning_starts``, as in SB3. The env must have been reset. ``buffer.size`` is read ONCE, before the first
        training phase (the one synchronisation here); an empty buffer raises. Returns ``self``.

        Reporting (all off by default: the launches and the one read-back are then exactly the above). ``monitor``: a
        :class:`DeviceEpisodeMonitor`, fed every collected block, warm-up blocks included (four launches per block, no synchronisation).
        Every ``log_interval`` training phases, and every ``eval_freq`` env steps summed over the envs (SB3's count), a record is appended
        to ``self.log`` and passed to ``callback(record)``: a dict with ``num_timesteps``, ``num_gradient_steps``, ``rollout/ep_rew_mean``,
        ``rollout/ep_len_mean``, ``rollout/success_rate`` (the monitor's window; one small read-back per record) and ``eval/mean_reward``,
        ``eval/std_reward``, ``eval/success_rate``, ``eval/mean_ep_length`` (:func:`evaluate_policy`'s loop on ``eval_env``: ``n_eval_episodes``
        deterministic episodes, SB3's ``EvalCallback``); what a record did not take is NaN. ``eval_env`` may be ``self.venv``, as in the
        reference's script: the env is then reset after the evaluation, the monitor's in-flight accumulators are zeroed and collection
        continues from the reset state. The attributes ``eval_block_steps`` (32) and ``eval_max_steps`` (``None``: unbounded) are
        :func:`evaluate_policy`'s ``block_steps`` and ``max_steps`` for these evaluations. Argument checks raise ``ValueError`` before anything native."""
        total = _int_in("total_timesteps", total_timesteps, 0, ">= 0")
        reporting = self._check_reporting(monitor, log_interval, eval_env, eval_freq, n_eval_episodes, callback)
        self._open()
        N, T = int(self.venv.num_envs), self.train_freq
        end = self.num_timesteps + total
        phases, next_eval = 0, self.num_timesteps + (eval_freq or 0)
        while self.num_timesteps < end:
            if self.num_timesteps < self.learning_starts:
                block = self._collect_uniform(T, generator)
            else:
                block = self.buffer.collect(self.venv, self.actor, T, generator=generator)
            if monitor is not None:
                monitor.update(block, self.buffer.autoreset)
            self.num_timesteps += T * N
            trained = self.num_timesteps > self.learning_starts
            if trained:
                if not self._size_checked:
                    if self.buffer.size == 0:
                        raise nat.MjsError("the replay buffer is empty after the collected blocks: nothing to train on")
                    self._size_checked = True
                self.train(self._gradient_steps_per_phase())
            if reporting:
                phases += trained
                record = None
                if log_interval is not None and trained and phases % log_interval == 0:
                    record = self._record(monitor)
                if eval_freq is not None and self.num_timesteps >= next_eval:
                    record = record or self._record(monitor)
                    self._evaluate_into(record, eval_env, n_eval_episodes, monitor)
                    next_eval += -(-(self.num_timesteps - next_eval + 1) // eval_freq) * eval_freq  # the first multiple past num_timesteps
                if record is not None:
                    self.log.append(record)
                    if callback is not None:
                        callback(record)
        return self

    # ------------------------------------------------------------------ SB3
    @classmethod
    def from_sb3(cls, venv, model, obs_keys=None, **kw):
        """From an object shaped like ``stable_baselines3.SAC`` after ``_setup_model``: ``model.actor``, ``model.critic`` and
        ``model.critic_target`` (:meth:`DeviceActor.from_sb3`, :meth:`DeviceCritic.from_sb3`), and ``gamma``, ``tau``, ``batch_size``,
        ``buffer_size``, ``learning_starts``, ``gradient_steps``, ``target_update_interval``, ``ent_coef``, ``target_entropy``, ``train_freq``
        (an int or ``TrainFreq(frequency, unit)`` with unit ``"step"``) and ``lr_schedule(1.0)`` or ``learning_rate``. Duck-typed:
        stable_baselines3 is not a dependency. ``kw`` overrides what the model says; ``obs_keys`` as in :meth:`DeviceActor.from_sb3`."""
        for name in ("actor", "critic", "critic_target"):
            if getattr(model, name, None) is None:
                raise ValueError(f"not an SB3-shaped SAC model: no attribute {name!r}")
        hp = {}
        for name in ("gamma", "tau", "batch_size", "buffer_size", "learning_starts", "gradient_steps", "target_update_interval", "ent_coef", "target_entropy",
                     "train_freq", "seed"):
            if getattr(model, name, None) is not None:
                hp[name] = getattr(model, name)
        schedule = getattr(model, "lr_schedule", None)
        lr = schedule(1.0) if callable(schedule) else getattr(model, "learning_rate", None)
        if callable(lr):
            lr = lr(1.0)
        if lr is not None:
            hp["learning_rate"] = lr
        hp.update(kw)
        given = {k: hp.pop(k) for k in ("buffer", "target_critic") if k in hp}
        defaults = dict(buffer_size=1_000_000, batch_size=256, learning_rate=3e-4, gamma=0.99, tau=0.005, ent_coef="auto", target_entropy=None, train_freq=1,
                        gradient_steps=1, learning_starts=100, target_update_interval=1, seed=0)
        unknown = sorted(set(hp) - set(defaults))
        if unknown:
            raise ValueError(f"unknown arguments {unknown}")
        cls._hyperparameters(**{**defaults, **hp})  # every refusal before anything native
        actor = DeviceActor.from_sb3(venv, model.actor, obs_keys=obs_keys)
        made = [actor]
        try:
            critic = DeviceCritic.from_sb3(model.critic, action_dim=actor.action_dim)
            made.append(critic)
            target = given.pop("target_critic", None)
            if target is None:
                target = DeviceCritic.from_sb3(model.critic_target, action_dim=actor.action_dim)
                made.append(target)
            self = cls(venv, actor, critic, target, given.pop("buffer", None), **hp)
        except Exception:
            for obj in reversed(made):
                obj.close()
            raise
        self._owned = made + self._owned
        return self

    @staticmethod
    def _sb3_modules(model):
        a = model.actor
        return ([m for m in a.latent_pi if _is_linear(m)], a.mu, a.log_std), [[m for m in net if _is_linear(m)] for net in model.critic.q_networks], \
            [[m for m in net if _is_linear(m)] for net in model.critic_target.q_networks]

    def export_to(self, model):
        """The trained parameters back into an SB3-shaped ``model``: the actor into ``model.actor``, the critics into ``model.critic`` and
        ``model.critic_target`` (the ``export`` methods), and the learned ``log_ent_coef`` into ``model.log_ent_coef`` where the model has
        one. Returns ``model``."""
        for name in ("actor", "critic", "critic_target"):
            if getattr(model, name, None) is None:
                raise ValueError(f"not an SB3-shaped SAC model: no attribute {name!r}")
        actor_modules, q_nets, target_nets = self._sb3_modules(model)
        self._open()
        self.actor.export(actor_modules)
        self.critic.export(q_nets)
        self.target_critic.export(target_nets)
        log_ent = getattr(model, "log_ent_coef", None)
        if self.coef is not None and isinstance(log_ent, torch.Tensor):
            with torch.no_grad():
                log_ent.copy_(self.coef.log_ent_coef.reshape(log_ent.shape))
        return model

    def close(self):
        """Release what the trainer made itself (after the work queued on it has finished); objects handed in stay open."""
        if not self._closed:
            self._closed = True
            self._release()
            self._scratch = None

    def __del__(self):
        try:
            self.close()
        except Exception:  # noqa: BLE001
            pass
