"""Heuristic baseline policies on the vectorised env: random, constant order, BS-Newsvendor,
BS-Adaptive and BS-Optimized, under the RL evaluation's seed protocol.

The counterpart of the reference's src/experiments/run_baselines.py. There a baseline is an action
function that reads one CPU env object between two steps, and a hyper-parameter sweep runs its
thousands of episodes one after another. Here the policy step is a HIP kernel on the env's own device
state (csrc/policy.hip, msc_policy_act) and every (candidate, episode) pair of a sweep is its own env
of one handle: env c * n + i plays episode i of the sweep's seed with candidate c's parameters.

Episodes side by side follow PPOTrainer.evaluate: n envs with one root seed whose episode counters
start at 0..n-1 replay the episodes the reference's single env runs one after another
(msc_env_set_episode_counters). Returns and the four cost components are accumulated in float64 on
the device.

bs_optimized: the reference searches the base-stock levels with a Gaussian-process optimiser
(skopt.gp_minimize). The objective is the same here (`evaluate_levels`: mean train-mode return over
n_obj_episodes episodes with root seeds optimization_seed + i); the search on top of it is a seeded
cross-entropy method with elitism (`optimize_levels`), see DESIGN.md section 7. bs_independent is
not built.
"""
from __future__ import annotations

import argparse
import ctypes as C
import sys
from pathlib import Path
from typing import Any, Callable, Dict, List, Optional, Sequence, Tuple

import numpy as np

from .seeding import EXPERIMENT_SEEDS, SeedManager

BASELINE_NAMES: Tuple[str, ...] = ("random", "constant", "bs_newsvendor", "bs_adaptive", "bs_optimized")
BASELINE_DISPLAY_NAMES: Dict[str, str] = {
    "random": "Random", "constant": "ConstantOrder", "bs_newsvendor": "BSNewsvendor", "bs_adaptive": "BSAdaptive",
    "bs_optimized": "BSOptimized",
}
DEFAULT_EVAL_SEED = 123       # src/experiments/utils/args.py:5
DEFAULT_EVAL_EPISODES = 100   # src/experiments/utils/args.py:7
DEFAULT_ALPHA_VALUES: List[float] = [round(0.05 * i, 2) for i in range(1, 41)]  # run_baselines.py:940
DEFAULT_Z_VALUES: List[float] = [round(0.25 * i, 2) for i in range(25)]         # run_baselines.py:1019
DEFAULT_H_VALUES: List[int] = [5, 10, 20, 30, 40, 50, 100]                      # run_baselines.py:1085


def _g(node: Any, key: str) -> Any:
    return node[key] if isinstance(node, dict) else getattr(node, key)


def _require_direct(env_config: Any) -> np.ndarray:
    """max_order_quantities [K] of a `direct` action space; the baselines refuse any other
    (run_baselines.py:1347-1351)."""
    act = _g(env_config, "action_space")
    atype = _g(act, "type")
    if atype != "direct":
        raise ValueError(f"Baselines require action_space.type='direct', got '{atype}'.")
    return np.asarray(_g(act, "params")["max_order_quantities"], dtype=np.float64)


# ---- host-side parameter helpers ---------------------------------------------------------------
def newsvendor_levels(env_config: Any, z: float) -> np.ndarray:
    """BS-Newsvendor base-stock levels [W, K] (run_baselines.py:159-190): with h the warehouse's home
    region (argmin of its distance row), D = lambda_orders[h] * probability_skus[h] *
    lambda_quantity[h, k] and L the expected lead time, S = L D + z sqrt(L D)."""
    ds = _g(_g(env_config, "components"), "demand_sampler")
    if _g(ds, "type") != "poisson":
        raise ValueError(f"newsvendor_levels needs the true demand parameters of the 'poisson' sampler, "
                         f"got '{_g(ds, 'type')}'")
    W, K, R = int(_g(env_config, "n_warehouses")), int(_g(env_config, "n_skus")), int(_g(env_config, "n_regions"))
    p = _g(ds, "params")
    lo, ps, lq = p["lambda_orders"], p["probability_skus"], p["lambda_quantity"]
    if np.isscalar(lo):
        lo, ps, lq = np.full(R, float(lo)), np.full(R, float(ps)), np.full((R, K), float(lq))
    lo, ps, lq = np.asarray(lo, np.float64), np.asarray(ps, np.float64), np.asarray(lq, np.float64)
    lead = np.asarray(_g(_g(_g(env_config, "components"), "lead_time_sampler"), "params")["expected_lead_times"])
    home = np.argmin(np.asarray(_g(_g(env_config, "cost_structure"), "distances"), np.float64), axis=1)
    S = np.zeros((W, K))
    for w in range(W):
        h = home[w]
        for k in range(K):
            L = lead[w, k]
            d = lo[h] * ps[h] * lq[h, k]
            S[w, k] = L * d + z * np.sqrt(L * d)
    return S


def constant_actions(quantities: np.ndarray, max_order_quantities: np.ndarray) -> np.ndarray:
    """The constant-order policy's actions (run_baselines.py:117-121): f32 of 2 clip(q, 0, max) / max - 1."""
    q = np.clip(np.asarray(quantities, np.float64), 0.0, max_order_quantities)
    return (2.0 * q / max_order_quantities - 1.0).astype(np.float32)


def first_strict_argmax(values: Sequence[float]) -> int:
    """The reference sweep's tie rule (run_baselines.py:589-607): a later equal value does not replace
    the incumbent; index 0 when nothing exceeds -inf."""
    best, best_v = 0, -np.inf
    for i, v in enumerate(values):
        if v > best_v:
            best, best_v = i, v
    return best


def baseline_train_seeds(baseline: str, root_seed: int) -> List[int]:
    """SeedManager(root_seed).spawn_child_seeds("train", n): n = 2 for `constant` (calibration,
    validation), 1 for the swept / optimised baselines, none for `random` (its generator is seeded with
    root_seed itself)."""
    n = {"random": 0, "constant": 2, "bs_newsvendor": 1, "bs_adaptive": 1, "bs_optimized": 1}[baseline]
    return SeedManager(root_seed, EXPERIMENT_SEEDS).spawn_child_seeds("train", n) if n else []


def random_stream_states(seed: int, n_envs: int, draws_per_env: int) -> np.ndarray:
    """PCG64 states [n_envs, 4] u64 {state_hi, state_lo, inc_hi, inc_lo}: env k starts at draw
    k * draws_per_env of default_rng(seed). The reference draws one stream across the episodes of its
    single eval env, T * W * K doubles per episode."""
    out = np.zeros((n_envs, 4), np.uint64)
    m = (1 << 64) - 1
    for k in range(n_envs):
        bg = np.random.PCG64(seed)
        bg.advance(k * int(draws_per_env))
        st = bg.state["state"]
        out[k] = [st["state"] >> 64, st["state"] & m, st["inc"] >> 64, st["inc"] & m]
    return out


def aggregate_results(returns: np.ndarray, costs: Optional[np.ndarray]) -> Dict[str, Any]:
    """The reference's result dict (run_baselines.py:479-506, :853-867) from per-episode returns [n]
    and cost sums [n, 4] (holding, penalty, outbound, inbound); std with ddof = 1, 0 for one episode."""
    r = np.asarray(returns, np.float64)
    n = int(r.shape[0])
    out: Dict[str, Any] = {
        "episode_return_mean": float(np.mean(r)),
        "episode_return_std": float(np.std(r, ddof=1) if n > 1 else 0.0),
        "episode_return_min": float(np.min(r)),
        "episode_return_max": float(np.max(r)),
        "num_episodes": n,
    }
    if costs is not None:
        c = np.asarray(costs, np.float64)
        total = c[:, 0] + c[:, 1] + c[:, 2] + c[:, 3]
        out["cost_components"] = {
            "holding_mean": float(np.mean(c[:, 0])), "penalty_mean": float(np.mean(c[:, 1])),
            "outbound_mean": float(np.mean(c[:, 2])), "inbound_mean": float(np.mean(c[:, 3])),
            "total_cost_mean": float(np.mean(total)),
            "total_cost_std": float(np.std(total, ddof=1) if n > 1 else 0.0),
        }
    return out


# ---- policies ----------------------------------------------------------------------------------
def _cand_array(candidates, n_envs: int, n_cand: int) -> np.ndarray:
    if candidates is None:
        if n_cand != 1:
            raise ValueError(f"{n_cand} candidates need the env -> candidate map")
        return np.zeros(n_envs, np.int32)
    c = np.ascontiguousarray(candidates, dtype=np.int32)
    if c.shape != (n_envs,):
        raise ValueError(f"candidates must have shape ({n_envs},), got {c.shape}")
    return c


def _hp(a: Optional[np.ndarray]):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


class _DevicePolicy:
    """A msc_policy handle bound to one VecInventoryEnv; `act` is one kernel launch on the current stream."""
    KIND = -1

    def _create(self, env, n_cand: int, h_max: int = 0, S=None, z=None, H=None, cand=None, rng=None) -> None:
        import torch
        from . import abi
        self.env, self.n_candidates = env, int(n_cand)
        self.actions = torch.zeros((env.n_envs, env.W, env.K), dtype=torch.float32, device=env.device)
        h = C.c_void_p()
        with torch.cuda.device(env.device):
            abi.check(abi.lib().msc_policy_create(env._h, self.KIND, int(n_cand), int(h_max), _hp(S), _hp(z), _hp(H),
                                                  _hp(cand), _hp(rng), C.byref(h)))
        self._h = h

    def _set(self, S=None, z=None, H=None, cand=None) -> None:
        from . import abi
        abi.check(abi.lib().msc_policy_set_tables(self._h, self.n_candidates, _hp(S), _hp(z), _hp(H), _hp(cand)))

    def act(self, env=None):
        """Actions [E, W, K] f32 of every env from its device state (a resident buffer, rewritten by each call)."""
        import torch
        from . import abi
        env = self.env if env is None else env
        abi.check(abi.lib().msc_policy_act(self._h, env._h, C.c_void_p(self.actions.data_ptr()),
                                           C.c_void_p(torch.cuda.current_stream().cuda_stream)))
        return self.actions

    def close(self) -> None:
        if getattr(self, "_h", None):
            from . import abi
            abi.lib().msc_policy_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class BaseStockPolicy(_DevicePolicy):
    """Fixed base-stock levels (BS-Newsvendor / BS-Optimized): `levels` [W, K] or, per candidate,
    [C, W, K] with `candidates` [E] mapping each env to its row."""
    KIND = 0

    def __init__(self, env, levels, candidates=None):
        S = self._levels(env, levels)
        self._create(env, S.shape[0], S=S, cand=_cand_array(candidates, env.n_envs, S.shape[0]))

    @staticmethod
    def _levels(env, levels) -> np.ndarray:
        S = np.asarray(levels, dtype=np.float64)
        if S.ndim == 2:
            S = S[None]
        if S.ndim != 3 or S.shape[1:] != (env.W, env.K):
            raise ValueError(f"levels must have shape [C, {env.W}, {env.K}] or [{env.W}, {env.K}], got {S.shape}")
        return np.ascontiguousarray(S)

    def set_levels(self, levels, candidates=None) -> None:
        """Replace the levels (same candidate count) and optionally the env -> candidate map."""
        S = self._levels(self.env, levels)
        cand = None if candidates is None else _cand_array(candidates, self.env.n_envs, S.shape[0])
        if S.shape[0] != self.n_candidates:
            raise ValueError(f"{S.shape[0]} candidates given, the policy holds {self.n_candidates}")
        self._set(S=S, cand=cand)


class AdaptiveBaseStockPolicy(_DevicePolicy):
    """Rolling mean / variance base-stock (BS-Adaptive): safety factor(s) `z` and window(s) `H`, one
    value or one per candidate; the demand window lives in the policy (h_max slots per env)."""
    KIND = 1

    def __init__(self, env, z, H, candidates=None, h_max: Optional[int] = None):
        za = np.ascontiguousarray(np.atleast_1d(np.asarray(z, np.float64)))
        Ha = np.ascontiguousarray(np.atleast_1d(np.asarray(H)).astype(np.int32))
        if za.shape != Ha.shape or za.ndim != 1:
            raise ValueError("z and H must be scalars or 1-d arrays of one length")
        self._create(env, za.shape[0], h_max=int(h_max or 0), z=za, H=Ha,
                     cand=_cand_array(candidates, env.n_envs, za.shape[0]))


class RandomPolicy(_DevicePolicy):
    """Uniform actions in [-1, 1) from one PCG64 stream per env: `states` [E, 4] u64
    (random_stream_states), or `seed` with env k starting at draw k * episode_length * W * K."""
    KIND = 2

    def __init__(self, env, seed: Optional[int] = None, states: Optional[np.ndarray] = None):
        if states is None:
            if seed is None:
                raise ValueError("RandomPolicy needs a seed or the per-env generator states")
            states = random_stream_states(seed, env.n_envs, env.spec.episode_length * env.W * env.K)
        st = np.ascontiguousarray(states, dtype=np.uint64)
        if st.shape != (env.n_envs, 4):
            raise ValueError(f"states must have shape ({env.n_envs}, 4), got {st.shape}")
        _require_direct_env(env)
        self._create(env, 1, rng=st)


class ConstantPolicy:
    """Constant order quantities [W, K] (or [C, W, K] with the env -> candidate map): a resident action
    tensor, no kernel."""

    def __init__(self, env, quantities, candidates=None):
        import torch
        _require_direct_env(env)
        q = np.asarray(quantities, np.float64)
        if q.ndim == 2:
            q = q[None]
        if q.ndim != 3 or q.shape[1:] != (env.W, env.K):
            raise ValueError(f"quantities must have shape [C, {env.W}, {env.K}] or [{env.W}, {env.K}], got {q.shape}")
        a = constant_actions(q, env.spec.action_param)
        cand = _cand_array(candidates, env.n_envs, q.shape[0])
        self.actions = torch.from_numpy(np.ascontiguousarray(a[cand])).to(env.device)

    def act(self, env=None):
        return self.actions

    def close(self) -> None:
        pass


def _require_direct_env(env) -> None:
    if env.spec.action_type != "direct":
        raise ValueError(f"Baselines require action_space.type='direct', got '{env.spec.action_type}'.")


# ---- rollouts ----------------------------------------------------------------------------------
def run_episodes(env_config: Any, policy_factory: Callable, env_seeds, counters, *, data_mode: str,
                 num_eval_episodes: int = 0, device: int = 0, env_meta: Optional[Dict[str, Any]] = None,
                 want_costs: bool = True, want_demand: bool = False) -> Dict[str, np.ndarray]:
    """One episode in each of len(env_seeds) envs side by side: env j has root seed env_seeds[j] and
    plays episode counters[j] of it under policy_factory(env). Returns per-env float64 `returns` [E]
    (summed over agents and steps), `costs` [E, 4] (holding, penalty, outbound, inbound) and, with
    want_demand, `demand_sum` [W, K]: last-step home demand summed over envs and steps."""
    import torch
    from . import abi
    from .spec import EnvSpec
    from .vec_env import VecInventoryEnv
    _require_direct(env_config)
    seeds = np.ascontiguousarray(np.asarray(env_seeds, dtype=np.int64) & 0xFFFFFFFF, dtype=np.uint32)
    E = int(seeds.shape[0])
    meta = dict(env_meta or {})
    meta["data_mode"] = data_mode
    meta["num_eval_episodes"] = int(num_eval_episodes)
    spec = EnvSpec.from_config(env_config, meta)
    env = VecInventoryEnv(None, E, spec=spec, device=device, env_seeds=seeds, episode_ahead=0)
    policy = None
    try:
        env.set_episode_counters(np.ascontiguousarray(counters, dtype=np.int32))
        env.reset()
        policy = policy_factory(env)
        dev, W = env.device, env.W
        ret = torch.zeros(E, dtype=torch.float64, device=dev)
        team = torch.zeros(E, dtype=torch.float64, device=dev)
        info: Dict[str, Any] = {}
        if want_costs:
            info["costs"] = torch.zeros((E, 4, W), dtype=torch.float64, device=dev)
            csum = torch.zeros((E, 4), dtype=torch.float64, device=dev)
            cstep = torch.zeros((E, 4), dtype=torch.float64, device=dev)
        if want_demand:
            info["demand_per_region"] = torch.zeros((E, env.R, env.K), dtype=torch.int32, device=dev)
            home = torch.from_numpy(np.asarray(spec.home_regions, np.int64)).to(dev)
            dsum = torch.zeros((W, env.K), dtype=torch.float64, device=dev)
        L = abi.lib()
        for _ in range(spec.episode_length):
            env.step(policy.act(env), want_final_obs=False, want_f64=True, info=info or None)
            st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
            # agent-order f64 sums, one launch each: an env's sums do not depend on its neighbours
            abi.check(L.msc_reward_team_sum(C.c_void_p(env.rewards_f64.data_ptr()), E, W, None,
                                            C.c_void_p(team.data_ptr()), st))
            ret += team
            if want_costs:
                abi.check(L.msc_reward_team_sum(C.c_void_p(info["costs"].data_ptr()), 4 * E, W, None,
                                                C.c_void_p(cstep.data_ptr()), st))
                csum += cstep
            if want_demand:
                dsum += info["demand_per_region"][:, home, :].sum(0, dtype=torch.float64)
        env.check()
        out = {"returns": ret.cpu().numpy()}
        if want_costs:
            out["costs"] = csum.cpu().numpy()
        if want_demand:
            out["demand_sum"] = dsum.cpu().numpy()
        return out
    finally:
        if policy is not None:
            policy.close()
        env.close()


def rollout_episodes(env_config: Any, policy_factory: Callable, root_seed: int, n_episodes: int, *,
                     data_mode: str = "val", counters=None, device: int = 0,
                     env_meta: Optional[Dict[str, Any]] = None, return_episodes: bool = False) -> Dict[str, Any]:
    """n episodes of one root seed side by side (episode counters 0..n-1 unless given), as the reference's
    _eval_action_fn_on_eval_seed runs them one after another (run_baselines.py:826-867); the reference's
    result keys. return_episodes adds the per-episode arrays under `episode_returns` / `episode_costs`."""
    n = int(n_episodes)
    cnt = np.arange(n, dtype=np.int32) if counters is None else np.asarray(counters, np.int32)
    raw = run_episodes(env_config, policy_factory, np.full(n, int(root_seed), np.int64), cnt, data_mode=data_mode,
                       num_eval_episodes=n if data_mode == "val" else 0, device=device, env_meta=env_meta)
    out = aggregate_results(raw["returns"], raw["costs"])
    if return_episodes:
        out["episode_returns"], out["episode_costs"] = raw["returns"], raw["costs"]
    return out


def calibrate_demand(env_config: Any, calibration_seed: int, num_calibration_episodes: int = 50, *,
                     device: int = 0, env_meta: Optional[Dict[str, Any]] = None) -> np.ndarray:
    """Mean home demand per (warehouse, SKU) over zero-order pilot episodes in train mode
    (run_baselines.py:513-553): the mean over all episodes x steps of last-step home demand."""
    n = int(num_calibration_episodes)
    W, K = int(_g(env_config, "n_warehouses")), int(_g(env_config, "n_skus"))
    raw = run_episodes(env_config, lambda env: ConstantPolicy(env, np.zeros((W, K))), np.full(n, int(calibration_seed)),
                       np.arange(n), data_mode="train", device=device, env_meta=env_meta, want_costs=False,
                       want_demand=True)
    return raw["demand_sum"] / float(n * int(_g(env_config, "episode_length")))


def validation_sweep(env_config: Any, validation_seed: int, n_episodes: int, n_candidates: int,
                     policy_factory: Callable, *, device: int = 0, env_meta: Optional[Dict[str, Any]] = None,
                     return_episodes: bool = False):
    """All candidates x episodes in one handle (train mode, run_baselines.py:556-609): env c * n + i plays
    episode i of validation_seed with candidate c; policy_factory(env, candidates) builds the policy from
    the env -> candidate map. Returns (mean return per candidate, first strict argmax[, returns [C, n]])."""
    n, Cn = int(n_episodes), int(n_candidates)
    cand = np.repeat(np.arange(Cn, dtype=np.int32), n)
    raw = run_episodes(env_config, lambda env: policy_factory(env, cand), np.full(Cn * n, int(validation_seed)),
                       np.tile(np.arange(n, dtype=np.int32), Cn), data_mode="train", device=device, env_meta=env_meta,
                       want_costs=False)
    per = raw["returns"].reshape(Cn, n)
    means = [float(np.mean(per[c])) for c in range(Cn)]
    best = first_strict_argmax(means)
    return (means, best, per) if return_episodes else (means, best)


def evaluate_levels(env_config: Any, S_batch, optimization_seed: int, n_obj_episodes: int, *, device: int = 0,
                    env_meta: Optional[Dict[str, Any]] = None) -> np.ndarray:
    """The objective the reference's bs_optimized maximises (run_baselines.py:655-680), for a batch of
    level sets [C, W, K] in one run: candidate c x episode i is an env with root seed
    optimization_seed + i in train mode playing its first episode. Mean return per candidate [C]."""
    S = np.asarray(S_batch, np.float64)
    Cn, n = int(S.shape[0]), int(n_obj_episodes)
    cand = np.repeat(np.arange(Cn, dtype=np.int32), n)
    raw = run_episodes(env_config, lambda env: BaseStockPolicy(env, S, cand),
                       np.tile(int(optimization_seed) + np.arange(n, dtype=np.int64), Cn), np.zeros(Cn * n, np.int32),
                       data_mode="train", device=device, env_meta=env_meta, want_costs=False)
    return raw["returns"].reshape(Cn, n).mean(axis=1)


def optimize_levels(env_config: Any, optimization_seed: int, *, n_generations: int = 12, population: int = 64,
                    n_obj_episodes: int = 50, upper_bound: float = 200.0, elite_fraction: float = 0.25,
                    z_values: Optional[Sequence[float]] = None, device: int = 0,
                    env_meta: Optional[Dict[str, Any]] = None) -> Tuple[np.ndarray, List[float], float]:
    """Seeded cross-entropy search over base-stock levels in [0, upper_bound]^(W K), maximising
    evaluate_levels. Generation 0 is the newsvendor levels of the z grid; each later generation keeps the
    incumbent and draws the rest from a normal fitted to the elite, clipped to the bounds. The incumbent
    is re-scored on the same seeds every generation, so the best objective never decreases. Returns
    (levels [W, K], best objective per generation, the newsvendor start's best objective)."""
    W, K = int(_g(env_config, "n_warehouses")), int(_g(env_config, "n_skus"))
    zs = list(DEFAULT_Z_VALUES if z_values is None else z_values)
    rng = np.random.default_rng(int(optimization_seed))
    pop = np.clip(np.stack([newsvendor_levels(env_config, z) for z in zs]), 0.0, upper_bound).reshape(len(zs), W * K)
    n_elite = max(2, int(round(elite_fraction * population)))
    history: List[float] = []
    start_best = None
    best_S, best_v = pop[0].copy(), -np.inf
    for gen in range(int(n_generations) + 1):
        scores = evaluate_levels(env_config, pop.reshape(-1, W, K), optimization_seed, n_obj_episodes, device=device,
                                 env_meta=env_meta)
        i = first_strict_argmax(scores)
        if scores[i] > best_v:
            best_S, best_v = pop[i].copy(), float(scores[i])
        if gen == 0:
            start_best = best_v
        else:
            history.append(best_v)
        if gen == n_generations:
            break
        elite = pop[np.argsort(-scores, kind="stable")[:min(n_elite, len(pop))]]
        mean = elite.mean(axis=0)
        std = np.maximum(elite.std(axis=0), 0.02 * upper_bound)
        draws = np.clip(mean + std * rng.standard_normal((population - 1, W * K)), 0.0, upper_bound)
        pop = np.concatenate([best_S[None], draws], axis=0)
    return best_S.reshape(W, K), history, float(start_best)


# ---- runners (run_baselines.py:870-1190) -------------------------------------------------------
def _final_eval(env_config, policy_factory, eval_seed, eval_episodes, device, env_meta) -> Dict[str, Any]:
    return rollout_episodes(env_config, policy_factory, eval_seed, eval_episodes, data_mode="val", device=device,
                            env_meta=env_meta)


def run_random_baseline(env_config, root_seed, eval_seed, eval_episodes, *, device=0, env_meta=None) -> Dict[str, Any]:
    res = _final_eval(env_config, lambda env: RandomPolicy(env, seed=int(root_seed)), eval_seed, eval_episodes, device,
                      env_meta)
    return {"baseline": "random", "selected_hparams": {}, **res}


def run_constant_baseline(env_config, root_seed, eval_seed, eval_episodes, *, alpha_values=None,
                          num_calibration_episodes: int = 50, num_validation_episodes=None, device=0,
                          env_meta=None) -> Dict[str, Any]:
    calibration_seed, validation_seed = baseline_train_seeds("constant", root_seed)
    alphas = list(DEFAULT_ALPHA_VALUES if alpha_values is None else alpha_values)
    val_episodes = int(num_validation_episodes or eval_episodes)
    mean_demand = calibrate_demand(env_config, calibration_seed, num_calibration_episodes, device=device, env_meta=env_meta)
    q = np.stack([np.round(a * mean_demand) for a in alphas])
    val, best = validation_sweep(env_config, validation_seed, val_episodes, len(alphas),
                                 lambda env, cand: ConstantPolicy(env, q, cand), device=device, env_meta=env_meta)
    res = _final_eval(env_config, lambda env: ConstantPolicy(env, q[best]), eval_seed, eval_episodes, device, env_meta)
    return {
        "baseline": "constant",
        "selected_hparams": {"best_alpha": float(alphas[best]), "calibrated_mean_demand": mean_demand.tolist(),
                             "best_quantities": q[best].tolist()},
        "validation": {"validation_seed": int(validation_seed), "validation_episodes": val_episodes,
                       "alpha_values": [float(a) for a in alphas], "validation_rewards": [float(r) for r in val],
                       "best_idx": int(best)},
        "calibration": {"calibration_seed": int(calibration_seed),
                        "num_calibration_episodes": int(num_calibration_episodes)},
        **res,
    }


def run_bs_newsvendor_baseline(env_config, root_seed, eval_seed, eval_episodes, *, z_values=None,
                               num_validation_episodes=None, device=0, env_meta=None) -> Dict[str, Any]:
    (validation_seed,) = baseline_train_seeds("bs_newsvendor", root_seed)
    zs = list(DEFAULT_Z_VALUES if z_values is None else z_values)
    val_episodes = int(num_validation_episodes or eval_episodes)
    S = np.stack([newsvendor_levels(env_config, z) for z in zs])
    val, best = validation_sweep(env_config, validation_seed, val_episodes, len(zs),
                                 lambda env, cand: BaseStockPolicy(env, S, cand), device=device, env_meta=env_meta)
    res = _final_eval(env_config, lambda env: BaseStockPolicy(env, S[best]), eval_seed, eval_episodes, device, env_meta)
    return {
        "baseline": "bs_newsvendor",
        "selected_hparams": {"best_z": float(zs[best])},
        "validation": {"validation_seed": int(validation_seed), "validation_episodes": val_episodes,
                       "z_values": [float(z) for z in zs], "validation_rewards": [float(r) for r in val],
                       "best_idx": int(best)},
        **res,
    }


def run_bs_adaptive_baseline(env_config, root_seed, eval_seed, eval_episodes, *, z_values=None, H_values=None,
                             num_validation_episodes=None, device=0, env_meta=None) -> Dict[str, Any]:
    (validation_seed,) = baseline_train_seeds("bs_adaptive", root_seed)
    zs = list(DEFAULT_Z_VALUES if z_values is None else z_values)
    Hs = list(DEFAULT_H_VALUES if H_values is None else H_values)
    val_episodes = int(num_validation_episodes or eval_episodes)
    sweep = [(z, H) for H in Hs for z in zs]  # the reference's order: H outer, z inner
    za, Ha = np.array([p[0] for p in sweep], np.float64), np.array([p[1] for p in sweep], np.int32)
    val, best = validation_sweep(env_config, validation_seed, val_episodes, len(sweep),
                                 lambda env, cand: AdaptiveBaseStockPolicy(env, za, Ha, cand), device=device,
                                 env_meta=env_meta)
    bz, bH = sweep[best]
    res = _final_eval(env_config, lambda env: AdaptiveBaseStockPolicy(env, bz, bH), eval_seed, eval_episodes, device,
                      env_meta)
    return {
        "baseline": "bs_adaptive",
        "selected_hparams": {"best_z": float(bz), "best_H": int(bH)},
        "validation": {"validation_seed": int(validation_seed), "validation_episodes": val_episodes,
                       "z_values": [float(z) for z in zs], "H_values": [int(h) for h in Hs],
                       "sweep_params": [[float(z), int(h)] for z, h in sweep],
                       "validation_rewards": [float(r) for r in val], "best_idx": int(best)},
        **res,
    }


def run_bs_optimized_baseline(env_config, root_seed, eval_seed, eval_episodes, *, n_generations: int = 12,
                              population: int = 64, n_obj_episodes: int = 50, upper_bound: float = 200.0, device=0,
                              env_meta=None) -> Dict[str, Any]:
    (optimization_seed,) = baseline_train_seeds("bs_optimized", root_seed)
    S, history, start = optimize_levels(env_config, optimization_seed, n_generations=n_generations, population=population,
                                        n_obj_episodes=n_obj_episodes, upper_bound=upper_bound, device=device,
                                        env_meta=env_meta)
    res = _final_eval(env_config, lambda env: BaseStockPolicy(env, S), eval_seed, eval_episodes, device, env_meta)
    return {
        "baseline": "bs_optimized",
        "selected_hparams": {"best_base_stock_levels": S.tolist()},
        "optimization": {"optimization_seed": int(optimization_seed), "method": "cross_entropy",
                         "n_generations": int(n_generations), "population": int(population),
                         "n_obj_episodes": int(n_obj_episodes), "upper_bound": float(upper_bound),
                         "newsvendor_start_objective": float(start), "convergence": [float(v) for v in history]},
        **res,
    }


BASELINE_REGISTRY: Dict[str, Callable] = {
    "random": run_random_baseline, "constant": run_constant_baseline, "bs_newsvendor": run_bs_newsvendor_baseline,
    "bs_adaptive": run_bs_adaptive_baseline, "bs_optimized": run_bs_optimized_baseline,
}


# ---- output and command line (run_baselines.py:1296-1449, :1532-1713) --------------------------
def existing_result(eval_file: Path) -> Optional[Dict[str, Any]]:
    """The dict of a finished eval_results_best.yaml (numeric episode_return_mean), else None."""
    import yaml
    if not Path(eval_file).exists():
        return None
    try:
        with open(eval_file, encoding="utf-8") as fh:
            d = yaml.safe_load(fh) or {}
    except (OSError, yaml.YAMLError):
        return None
    v = d.get("episode_return_mean") if isinstance(d, dict) else None
    return d if isinstance(v, (int, float)) and not isinstance(v, bool) else None


def run_single_baseline_seed_eval(baseline: str, env_config: Any, root_seed: int, eval_seed: int, eval_episodes: int,
                                  output_dir, *, skip_if_done: bool = True, device: int = 0,
                                  runner_kwargs: Optional[Dict[str, Any]] = None) -> Dict[str, Any]:
    """One (baseline, root_seed) pair -> <output_dir>/eval_results_best.yaml."""
    import yaml
    if baseline not in BASELINE_REGISTRY:
        raise ValueError(f"Unknown baseline {baseline!r}. Choose from: {sorted(BASELINE_REGISTRY)}")
    out = Path(output_dir)
    out.mkdir(parents=True, exist_ok=True)
    eval_file = out / "eval_results_best.yaml"
    if skip_if_done:
        done = existing_result(eval_file)
        if done is not None:
            print(f"[SKIP] {out.name}: eval_results_best.yaml already complete "
                  f"(episode_return_mean={done['episode_return_mean']:.4f})")
            return done
    _require_direct(env_config)
    res = BASELINE_REGISTRY[baseline](env_config, int(root_seed), int(eval_seed), int(eval_episodes), device=device,
                                      **(runner_kwargs or {}))
    res["root_seed"], res["eval_seed"] = int(root_seed), int(eval_seed)
    res["display_name"] = BASELINE_DISPLAY_NAMES[baseline]
    with open(eval_file, "w", encoding="utf-8") as fh:
        yaml.safe_dump(res, fh, default_flow_style=False, sort_keys=False)
    print(f"[INFO] {res['display_name']} (root_seed={root_seed}): episode_return_mean = "
          f"{res['episode_return_mean']:.4f}\n[INFO] Saved: {eval_file}")
    return res


def run_baselines_across_seeds(env_config: Any, n_seeds: int, eval_seed: int, eval_episodes: int, seed_eval_dir,
                               baselines: Optional[Sequence[str]] = None, *, skip_if_done: bool = True,
                               device: int = 0) -> None:
    """Every (baseline, root seed 100, 200, ...) pair, one after another."""
    for b in (list(BASELINE_NAMES) if baselines is None else list(baselines)):
        if b not in BASELINE_REGISTRY:
            raise ValueError(f"Unknown baseline {b!r}. Choose from: {sorted(BASELINE_REGISTRY)}")
        for i in range(1, int(n_seeds) + 1):
            run_single_baseline_seed_eval(b, env_config, 100 * i, eval_seed, eval_episodes,
                                          Path(seed_eval_dir) / f"{BASELINE_DISPLAY_NAMES[b]}_Seed{100 * i}",
                                          skip_if_done=skip_if_done, device=device)


def parse_args(argv: Optional[List[str]] = None) -> argparse.Namespace:
    ap = argparse.ArgumentParser(description="Run baseline policies as seed-comparable evaluations.")
    ap.add_argument("--mode", choices=["single", "all-seeds"], default="all-seeds")
    ap.add_argument("--env-config", type=str, required=True)
    ap.add_argument("--storage-dir", type=str, default="./experiment_outputs/Runs")
    ap.add_argument("--experiment-name", type=str, default=None)
    ap.add_argument("--n-seeds", type=int, default=5, help="seeds per baseline (--mode all-seeds only)")
    ap.add_argument("--eval-episodes", type=int, default=DEFAULT_EVAL_EPISODES)
    ap.add_argument("--eval-seed", type=int, default=DEFAULT_EVAL_SEED)
    ap.add_argument("--baselines", type=str, nargs="+", choices=list(BASELINE_NAMES), default=None,
                    help="subset of baselines (--mode all-seeds only)")
    ap.add_argument("--baseline", type=str, choices=list(BASELINE_NAMES), default=None, help="--mode single only")
    ap.add_argument("--root-seed", type=int, default=None, help="per-run root seed (--mode single only)")
    ap.add_argument("--device", type=int, default=0)
    args = ap.parse_args(argv)
    if args.mode == "single":
        if args.baseline is None or args.root_seed is None:
            ap.error("--mode single requires --baseline and --root-seed")
        if args.baselines is not None:
            ap.error("--baselines (plural) is incompatible with --mode single; use --baseline (singular) instead.")
    elif args.baseline is not None or args.root_seed is not None:
        ap.error("--baseline / --root-seed are only valid for --mode single; use --baselines (plural) and "
                 "--n-seeds for --mode all-seeds.")
    return args


def main(argv: Optional[List[str]] = None) -> int:
    from datetime import datetime
    from .config import load_environment_config
    args = parse_args(argv)
    env_config = load_environment_config(args.env_config, allow_nr_ne_nw=True)
    name = args.experiment_name or (f"BASELINE_{env_config.n_warehouses}WH_{env_config.n_skus}SKU_"
                                    f"{datetime.now().strftime('%Y%m%d_%H%M')}")
    seed_eval_dir = Path(args.storage_dir) / name / "seed_evaluation"
    seed_eval_dir.mkdir(parents=True, exist_ok=True)
    if args.mode == "single":
        run_single_baseline_seed_eval(args.baseline, env_config, args.root_seed, args.eval_seed, args.eval_episodes,
                                      seed_eval_dir / f"{BASELINE_DISPLAY_NAMES[args.baseline]}_Seed{args.root_seed}",
                                      device=args.device)
    else:
        run_baselines_across_seeds(env_config, args.n_seeds, args.eval_seed, args.eval_episodes, seed_eval_dir,
                                   args.baselines, device=args.device)
        print(f"[INFO] All baseline outputs in: {seed_eval_dir.resolve()}")
    return 0


if __name__ == "__main__":
    sys.exit(main())
