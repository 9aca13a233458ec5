"""Plain-numpy restatement of the baseline policies (marlsc/baselines.py, csrc/policy.hip), written to
check the kernel against: it works on the observations of oracle.OracleEnv and states the rules the
way the reference's action functions do (src/experiments/run_baselines.py:193-205, :255-292), calling
np.mean / np.var themselves on the stacked float32 window.

The oracle env runs with obs_normalization off and the features inventory, pipeline and
incoming_demand_home only, so a local observation is [inventory K | pipeline Lmax x K |
home demand K] (EnvSpec.n_features' block order), every entry an exact integer in float32. The
pending total of a (warehouse, SKU) is the sum of its Lmax pipeline buckets: bucket 0 collects every
order due next step or overdue, so the buckets partition the pending orders.
"""
from __future__ import annotations

import numpy as np

EMU_FEATURES = {"inventory": True, "pipeline": True, "incoming_demand_home": True}


def emu_features(all_keys) -> dict:
    return {k: bool(EMU_FEATURES.get(k, False)) for k in all_keys}


def split_obs(spec, obs: np.ndarray):
    """(inventory, pending total, home demand), each [E, W, K]: the first two float64, the demand float32
    as the reference env keeps it."""
    K, Lm = spec.K, spec.max_expected_lead_time
    assert obs.shape[-1] == K + Lm * K + K, (obs.shape, K, Lm)
    inv = obs[..., :K].astype(np.float64)
    pipe = obs[..., K:K + Lm * K].reshape(obs.shape[:-1] + (Lm, K))
    pend = pipe.astype(np.float64).sum(axis=-2)
    dem = np.ascontiguousarray(obs[..., K + Lm * K:], dtype=np.float32)
    return inv, pend, dem


def order_up_to_actions(S, inv, pend, maxq) -> np.ndarray:
    """float32 of 2 clip(S - inv - pend, 0, maxq) / maxq - 1, all float64 before the cast."""
    qty = np.clip(S - inv - pend, 0.0, maxq)
    return (2.0 * qty / maxq - 1.0).astype(np.float32)


def window_stats(window):
    """(mean, var) of a list of float32 [W, K] demand arrays, as the reference's adaptive rule takes
    them: numpy's axis-0 mean and (ddof = 0) var of the float32 stack; the mean for a single entry."""
    stack = np.array(window)
    assert stack.dtype == np.float32
    mean = stack.mean(axis=0)
    var = stack.var(axis=0, ddof=0) if len(window) > 1 else mean.copy()
    return mean, var


def window_stats_loop(window):
    """The same statistics as literal float32 loops, oldest entry first (what the kernel does)."""
    n = len(window)
    shape = np.shape(window[0])
    mean = np.zeros(shape, np.float32)
    var = np.zeros(shape, np.float32)
    for idx in np.ndindex(*shape):
        s = np.float32(0.0)
        for x in window:
            s = np.float32(s + np.float32(x[idx]))
        m = np.float32(s / np.float32(n))
        if n == 1:
            v = m
        else:
            q = np.float32(0.0)
            for x in window:
                d = np.float32(np.float32(x[idx]) - m)
                q = np.float32(q + np.float32(d * d))
            v = np.float32(q / np.float32(n))
        mean[idx], var[idx] = m, v
    return mean, var


class BaseStockEmulation:
    """Fixed levels S [C, W, K] with the env -> candidate map."""

    def __init__(self, spec, levels, candidates):
        self.maxq = np.asarray(spec.action_param, np.float64)
        S = np.asarray(levels, np.float64)
        self.S = (S[None] if S.ndim == 2 else S)[np.asarray(candidates)]  # [E, W, K]

    def act(self, t: int, inv, pend, dem) -> np.ndarray:
        return order_up_to_actions(self.S, inv, pend, self.maxq)


class AdaptiveEmulation:
    """Rolling mean / variance base-stock with per-env (z, H); one demand list per env, cleared at t == 0."""

    def __init__(self, spec, z, H, candidates):
        self.maxq = np.asarray(spec.action_param, np.float64)
        self.lead = np.asarray(spec.expected_lead_times, np.float64).reshape(spec.W, spec.K)
        cand = np.asarray(candidates)
        self.z = np.atleast_1d(np.asarray(z, np.float64))[cand]
        self.H = np.atleast_1d(np.asarray(H, np.int64))[cand]
        self.buf = [[] for _ in range(len(cand))]

    def act(self, t: int, inv, pend, dem) -> np.ndarray:
        out = np.empty(inv.shape, np.float32)
        for e in range(inv.shape[0]):
            if t == 0:
                self.buf[e].clear()
                out[e] = -1.0
                continue
            self.buf[e].append(dem[e].copy())
            mean, var = window_stats(self.buf[e][-int(self.H[e]):])
            S = self.lead * mean + self.z[e] * np.sqrt(self.lead * var)
            out[e] = order_up_to_actions(S, inv[e], pend[e], self.maxq)
        return out


class RandomEmulation:
    """Env k draws W * K doubles per step from default_rng(seed)'s stream starting at draw
    k * draws_per_env, as one long uniform(-1, 1) stream cast to float32."""

    def __init__(self, spec, seed: int, n_envs: int, n_steps: int):
        self.wk = spec.W * spec.K
        self.shape = (spec.W, spec.K)
        per_env = spec.episode_length * self.wk
        total = (n_envs - 1) * per_env + n_steps * self.wk
        self.stream = np.random.default_rng(seed).uniform(-1.0, 1.0, size=total).astype(np.float32)
        self.start = np.arange(n_envs) * per_env
        self.step = 0

    def act(self, t: int, inv, pend, dem) -> np.ndarray:
        o = self.start + self.step * self.wk
        self.step += 1
        return np.stack([self.stream[a:a + self.wk].reshape(self.shape) for a in o])


def oracle_episode_totals(ref, spec, emu, n_episodes: int):
    """Run n_episodes episodes of a one-env oracle under `emu`: per-episode return (all agents, all
    steps) and the four cost sums, accumulated in float64."""
    obs = ref.reset()
    info = ref.alloc_info()
    rets, costs = np.zeros(n_episodes), np.zeros((n_episodes, 4))
    for ep in range(n_episodes):
        for t in range(spec.episode_length):
            a = emu.act(t, *split_obs(spec, obs))
            obs, rew, tr, _ = ref.step(a, info=info)
            rets[ep] += rew[0].sum()
            costs[ep] += info["costs"][0].sum(axis=-1)
        assert tr[0]
    return rets, costs
