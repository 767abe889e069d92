"""The rules of mjs_monitor_update (include/mjsim.h) restated in numpy: a plain double loop over t and n, float64 adds in t order. It never
calls the code under test."""
import math
from fractions import Fraction

import numpy as np

FIRST, MID, LAST = 0, 1, 2
RING_FIELDS = ("ring_return", "ring_length", "ring_success", "ring_terminated", "ring_env")


class BlockMaker:
    """[T, N] blocks as numpy arrays, chained: under next-step auto-reset the row after a LAST is FIRST, and a FIRST row carries a non-zero
    reward and random flags, which must be ignored. Rewards have mixed signs and magnitudes 1e-3 .. 1e3, so float64 add order shows."""

    def __init__(self, N, mode, seed, p_end=0.25):
        self.N, self.mode, self.p_end = N, mode, p_end
        self.rng = np.random.default_rng(seed)
        self.after_last = np.zeros(N, bool)

    def block(self, T, p_end=None):
        rng, N, p = self.rng, self.N, self.p_end if p_end is None else p_end
        reward = rng.standard_normal((T, N)) * 10.0 ** rng.integers(-3, 4, (T, N))
        is_success = rng.integers(0, 2, (T, N)).astype(np.uint8)
        terminated, truncated, step_type = np.zeros((T, N), np.uint8), np.zeros((T, N), np.uint8), np.full((T, N), MID, np.uint8)
        for t in range(T):
            end = rng.random(N) < p
            kind = rng.integers(0, 3, N)  # terminated, truncated, both
            first = self.after_last & (self.mode == "next_step")
            flagged = end | (first & (rng.random(N) < 0.5))  # flags on a FIRST row: noise
            terminated[t] = flagged & (kind != 1)
            truncated[t] = flagged & (kind != 0)
            step_type[t] = np.where(first, FIRST, np.where(end, LAST, MID))
            self.after_last = end & ~first
        return {"reward": reward, "terminated": terminated, "truncated": truncated, "is_success": is_success, "step_type": step_type}


def to_dev(blk, device="cuda:0"):
    """A numpy block as contiguous torch tensors on the device."""
    import torch

    return {k: torch.from_numpy(np.ascontiguousarray(v)).to(device) for k, v in blk.items()}


class RefMonitor:
    def __init__(self, num_envs, window=100, quota=None):
        self.N, self.W = num_envs, window
        self.ep_return = np.zeros(num_envs, np.float64)
        self.ep_length = np.zeros(num_envs, np.int32)
        self.ep_count = np.zeros(num_envs, np.int64)
        self.quota = None if quota is None else np.asarray(quota, np.int64)
        self.ring_return = np.zeros(window, np.float64)
        self.ring_length = np.zeros(window, np.int32)
        self.ring_success = np.zeros(window, np.uint8)
        self.ring_terminated = np.zeros(window, np.uint8)
        self.ring_env = np.zeros(window, np.int32)
        self.cursor = 0
        self.records = []  # every episode ever recorded: (return, length, success, terminated, env)

    def update(self, blk, mode):
        """blk: numpy arrays [T, N]. Returns the number of episodes recorded."""
        reward = blk["reward"]
        T, N = reward.shape
        assert N == self.N
        recorded = 0
        for t in range(T):
            for n in range(N):
                if mode == "next_step" and blk["step_type"][t, n] == FIRST:
                    continue  # the step after a LAST: a reset, the action was ignored
                self.ep_return[n] = self.ep_return[n] + reward[t, n]
                self.ep_length[n] += 1
                if blk["terminated"][t, n] or blk["truncated"][t, n]:
                    if self.quota is None or self.ep_count[n] < self.quota[n]:
                        slot = self.cursor % self.W
                        rec = (self.ep_return[n], self.ep_length[n], np.uint8(blk["is_success"][t, n] != 0), np.uint8(blk["terminated"][t, n] != 0), np.int32(n))
                        self.ring_return[slot], self.ring_length[slot], self.ring_success[slot], self.ring_terminated[slot], self.ring_env[slot] = rec
                        self.records.append(rec)
                        self.cursor += 1
                        self.ep_count[n] += 1
                        recorded += 1
                    self.ep_return[n] = 0.0
                    self.ep_length[n] = 0
        return recorded

    def remaining(self):
        return int(np.maximum(self.quota - self.ep_count, 0).sum())

    def live(self):
        """The live records in chronological order: arrays (return, length, success, terminated, env)."""
        recs = self.records[-min(self.cursor, self.W):] if self.cursor else []
        cols = list(zip(*recs)) if recs else [[]] * 5
        return (np.array(cols[0], np.float64), np.array(cols[1], np.int32), np.array(cols[2], np.uint8), np.array(cols[3], np.uint8), np.array(cols[4], np.int32))


def std_exact(x):
    """The population standard deviation from an exact variance (rational arithmetic), rounded once and rooted once: the higher-precision
    recomputation. math.fsum gives the same mean; the squares need more than it offers."""
    x = [Fraction(float(v)) for v in x]
    mean = sum(x) / len(x)
    return math.sqrt(float(sum((v - mean) ** 2 for v in x) / len(x)))


def std_bar(x):
    """(exact, numpy's error, bar) for a standard deviation computed from x: numpy.std's own distance from std_exact on these values, and
    what the code under test is allowed, 4 x that. std_exact is itself a float64, so a distance from it is a whole number of its ulps
    and a measured 0 says only "below one ulp": the measurement is floored at its resolution, one ulp of the exact value, before the factor 4 (no floor for
    a single value, whose std is exactly 0 on every side)."""
    exact = std_exact(x)
    numpy_err = abs(float(np.std(np.asarray(x, np.float64))) - exact)
    return exact, numpy_err, 4.0 * max(numpy_err, float(np.spacing(exact)) if exact > 0.0 else 0.0)


def sb3_targets(n_eval_episodes, n_envs):
    """stable_baselines3/common/evaluation.py: np.array([(n_eval_episodes + i) // n_envs for i in range(n_envs)], dtype="int")."""
    return np.array([(n_eval_episodes + i) // n_envs for i in range(n_envs)], dtype="int")
