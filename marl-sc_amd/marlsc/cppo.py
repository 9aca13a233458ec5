"""Centralised PPO (CPPO): the reference's single-agent upper-bound baseline (src/algorithms/cppo.py
over src/environment/envs/single_env.py) on this build's training path.

One policy sees the global observation concat(local_0 .. local_{W-1}) (W L floats, no warehouse
one-hot: cppo.py:86-87) and emits the joint action (W K floats, split per warehouse in agent order);
the reward is the team sum. Here that is the IPPO / MAPPO trainer over another view of the same env:

* `CentralizedRolloutEnv` presents a `VecInventoryEnv` to `RolloutCollector` as W' = 1 agent with
  K' = W K actions and a local observation of W L: the inner env writes the collector's observation
  row through an [E, W, L] view of the same memory (no copy), the team reward is one launch of
  msc_reward_team_sum over the inner env's f64 per-agent rewards, and the rollout noise stays keyed
  by global env id with W K values per env row;
* `CPPOTrainer` is `PPOTrainer` with that view, the module `MultiAgentActorCritic(1, W L, 0, W K)`
  and one advantage group; evaluation, checkpoints, resume and module_weights.pt are the parent's;
* the actor's W K outputs (40 at C3, 80 at C5) take the wide fused kernel at rollout with
  MSC_WIDE_MLP=1 (marlsc/mlp.py:wide_forward; opt-in), else the torch layers and
  msc_gaussian_sample; up to 8 outputs they take the narrow kernels as any actor does.

Parity with RLlib's PPO on the reference's CentralizedEnvWrapper is unpinned, as for the other
learners (RLlib is not importable here); the tests pin the view against `VecCentralizedEnv`, which
is pinned against the oracle, and the collector against its own kernels.
"""
from __future__ import annotations

import ctypes as C
from dataclasses import dataclass
from typing import Any, Dict, Optional

import torch

from . import abi
from .ppo import MultiAgentActorCritic, PPOConfig, PPOTrainer
from .rollout import RolloutConfig, fused_actor_sample


@dataclass
class CPPOConfig(PPOConfig):
    """PPOConfig's fields and validation for `name: cppo`: both observation types "local" (the
    centralised view's local observation IS the global vector) and no parameter sharing."""
    name: str = "cppo"

    _NAMES = ("cppo",)

    @classmethod
    def from_algorithm_config(cls, cfg: Dict[str, Any]) -> "CPPOConfig":
        c = super().from_algorithm_config(cfg)
        c.actor_obs_type = c.critic_obs_type = "local"
        c.parameter_sharing = False
        return c


def algorithm_name(cfg: Dict[str, Any]) -> str:
    return str(cfg.get("algorithm", cfg).get("name", "ippo")).lower()


def config_from_algorithm_config(cfg: Dict[str, Any]) -> PPOConfig:
    """The config class the algorithm's name selects: CPPOConfig for cppo, PPOConfig otherwise."""
    return (CPPOConfig if algorithm_name(cfg) == "cppo" else PPOConfig).from_algorithm_config(cfg)


def trainer_class(cfg: PPOConfig):
    return CPPOTrainer if cfg.name == "cppo" else PPOTrainer


def reward_team_sum(rewards_f64: torch.Tensor, out32: Optional[torch.Tensor] = None,
                    out64: Optional[torch.Tensor] = None):
    """msc_reward_team_sum: per env the agent-order f64 sum ((r0 + r1) + r2) ... of rewards_f64
    [E, W] into out64 [E] and, rounded once to f32, into out32 (any shape of E elements)."""
    E, W = rewards_f64.shape
    if not (rewards_f64.is_cuda and rewards_f64.dtype == torch.float64 and rewards_f64.is_contiguous()):
        raise ValueError("rewards must be a contiguous float64 CUDA tensor [E, W]")
    if out32 is None:
        out32 = torch.empty(E, dtype=torch.float32, device=rewards_f64.device)
    if out64 is None:
        out64 = torch.empty(E, dtype=torch.float64, device=rewards_f64.device)
    for t, dt in ((out32, torch.float32), (out64, torch.float64)):
        if not (t.is_cuda and t.dtype == dt and t.is_contiguous() and t.numel() == E):
            raise ValueError("out32 / out64 must be contiguous CUDA tensors of E elements (float32 / float64)")
    abi.check(abi.lib().msc_reward_team_sum(C.c_void_p(rewards_f64.data_ptr()), E, W, C.c_void_p(out32.data_ptr()),
                                            C.c_void_p(out64.data_ptr()),
                                            C.c_void_p(torch.cuda.current_stream(rewards_f64.device).cuda_stream)))
    return out32, out64


class CentralizedRolloutEnv:
    """A `VecInventoryEnv` as the rollout collector's env with one agent: obs [E, 1, W L] (a view of
    the inner env's [E, W, L] buffer), actions [E, 1, W K], rewards [E, 1] (f32 of the f64 team sum,
    which `rewards_f64` [E] keeps), truncated [E]."""

    STEP_C_FORM, ALLOC_PRIO_SPLIT = 1, 2  # VecInventoryEnv's option keys

    def __init__(self, env):
        self.venv = env
        self.n_envs, self.device, self.spec = env.n_envs, env.device, env.spec
        self.env_index_offset, self.ea_slots = env.env_index_offset, env.ea_slots
        self.n_warehouses, self.n_skus = env.W, env.K
        self.W, self.K, self.L = 1, env.W * env.K, env.W * env.L
        E = self.n_envs
        self.obs = env.obs.view(E, 1, self.L)
        self.final_obs = env.final_obs.view(E, 1, self.L)
        self.rewards = torch.zeros((E, 1), dtype=torch.float32, device=self.device)
        self.rewards_f64 = torch.zeros(E, dtype=torch.float64, device=self.device)

    @property
    def n_agents(self) -> int:
        return 1

    @property
    def local_obs_dim(self) -> int:
        return self.L

    @property
    def global_obs_dim(self) -> int:
        return self.L

    @property
    def _t_sync(self) -> int:  # (the trainer checkpoints the inner env's lockstep tracker)
        return getattr(self.venv, "_t_sync", -1)

    @_t_sync.setter
    def _t_sync(self, v: int) -> None:
        self.venv._t_sync = int(v)

    def reset(self, **kw) -> torch.Tensor:
        self.venv.reset(**kw)
        return self.obs

    def step(self, actions: torch.Tensor, *, obs_out: Optional[torch.Tensor] = None,
             rewards_out: Optional[torch.Tensor] = None, truncated_out: Optional[torch.Tensor] = None,
             want_final_obs: bool = True):
        """actions [E, 1, W K] (or [E, W K]); obs_out [E, 1, W L] / rewards_out [E, 1] / truncated_out [E]
        as VecInventoryEnv.step's: the inner env writes obs_out through an [E, W, L] view."""
        E, v = self.n_envs, self.venv
        if actions.dtype != torch.float32 or not actions.is_contiguous() or actions.device != self.device:
            actions = actions.to(device=self.device, dtype=torch.float32).contiguous()
        if actions.numel() != E * self.K:
            raise ValueError(f"actions must hold {E} x {self.K} values, got {tuple(actions.shape)}")
        if obs_out is not None and (obs_out.dtype != torch.float32 or not obs_out.is_contiguous()
                                    or obs_out.device != self.device or obs_out.numel() != E * self.L):
            raise ValueError(f"obs_out must be a contiguous float32 ({E}, 1, {self.L}) tensor on {self.device}")
        rew = self.rewards if rewards_out is None else rewards_out
        if rew.dtype != torch.float32 or not rew.is_contiguous() or rew.device != self.device or rew.numel() != E:
            raise ValueError(f"rewards_out must be a contiguous float32 ({E}, 1) tensor on {self.device}")
        _, _, trunc, final = v.step(actions.view(E, v.W, v.K), want_final_obs=want_final_obs, want_f64=True,
                                    obs_out=None if obs_out is None else obs_out.view(E, v.W, v.L),
                                    truncated_out=truncated_out)
        reward_team_sum(v.rewards_f64, rew, self.rewards_f64)
        return (self.obs if obs_out is None else obs_out), rew, trunc, (None if final is None else self.final_obs)

    def obs_flat(self, obs: Optional[torch.Tensor] = None, out: Optional[torch.Tensor] = None) -> torch.Tensor:
        raise ValueError("the centralised view has no local || global observation (both obs types are 'local')")

    # the rest is the inner env's
    def may_truncate(self) -> bool:
        return self.venv.may_truncate()

    def set_option(self, key: int, value: int) -> None:
        self.venv.set_option(key, value)

    def set_episode_ahead(self, enabled: bool) -> None:
        self.venv.set_episode_ahead(enabled)

    def set_chain_priority(self, enabled: bool) -> None:
        self.venv.set_chain_priority(enabled)

    def set_episode_counters(self, counters) -> None:
        self.venv.set_episode_counters(counters)

    def read_state(self):
        return self.venv.read_state()

    def save_state(self) -> bytes:
        return self.venv.save_state()

    def load_state(self, blob: bytes) -> None:
        self.venv.load_state(blob)

    def check(self) -> None:
        self.venv.check()

    def close(self) -> None:
        self.venv.close()


class CentralizedActorCritic(MultiAgentActorCritic):
    """MultiAgentActorCritic(1, W L, 0, W K, rc, shared=False): one policy for the one centralised agent
    (state-dict keys policies.0.*). The parent fuses the sampling into the actor kernel for a shared
    policy only; a single policy is the same case (every row is its row), so it is taken here too."""

    def __init__(self, obs_dim: int, action_dim: int, rc: RolloutConfig):
        super().__init__(1, obs_dim, 0, action_dim, rc, False, multi_mlp=False)  # one policy: nothing to batch

    def actor_sample_x(self, x: torch.Tensor, sample) -> bool:
        return fused_actor_sample(self.policies[0].actor, x, sample)


class CPPOTrainer(PPOTrainer):
    """PPOTrainer on the centralised view: one module over (W L) -> (W K), one advantage group, the
    meanstd filter over W L columns; evaluate() plays the mean action, clipped, on the same view with
    the reference's eval seeding."""

    def __init__(self, env_config: Any, cfg: PPOConfig, **kw):
        if cfg.name != "cppo":
            raise ValueError(f"CPPOTrainer needs a CPPOConfig (name 'cppo'), not '{cfg.name}'")
        super().__init__(env_config, cfg, **kw)

    def _include_warehouse_id(self) -> bool:
        return False  # cppo.py:86-87

    def _wrap_env(self, env):
        return CentralizedRolloutEnv(env)

    def _build_module(self, rc: RolloutConfig) -> MultiAgentActorCritic:
        return CentralizedActorCritic(self.env.L, self.env.K, rc)
