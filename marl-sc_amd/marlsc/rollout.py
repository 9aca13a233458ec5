"""On-device rollout for IPPO / MAPPO: the actor/critic forward of the reference's RLModule in
PyTorch-ROCm over the HIP env, and GAE + advantage normalisation in HIP.

Reference structure restated (RLlib itself is not importable here, so this row is parity
unpinned against the reference and checked against the numpy GAE in oracle/gae_ref.py):
* `MLP`: `MLPArchitecture.build` (src/algorithms/models/architectures/mlp.py:14-60) -- Linear +
  activation per hidden size, output Linear, optional output activation;
* `ActorCritic`: `BaseRLModule._forward_inference/_forward_train/compute_values`
  (src/algorithms/models/rlmodules/base.py:480-715) for MLP networks without shared layers --
  actor on the local slice (or the full flat obs when actor_obs_type == "global"), free `log_std`
  clamped at `logstd_floor` (`_append_log_std`), critic on local (IPPO) or full flat obs (MAPPO);
  with `use_mu_sigma_head` the actor is a backbone under `MuSigmaHead` (base.py:213-252, :434-435;
  architectures/mu_sigma_head.py) and log_std depends on the observation (`head_sample`);
* `GRUNet` / `PolicyNets`: the `gru` architecture (architectures/gru.py:14-85) as actor, critic or shared
  trunk, its states threaded through step / sequence forwards (base.py:99-141, 351-388, 480-715); one
  fused launch per network and rollout step (marlsc/gru.py, csrc/gru.hip);
* GAE(gamma, lambda) with truncation bootstrap V(final_obs) and RLlib's per-batch standardisation
  `(A - mean) / max(1e-4, std)`, statistics all-reduced across ranks (marlsc/dist.py).

Memory plan (288 GB HBM): the rollout stores the LOCAL observations only ([T, E, W, L] f32, 3.6 GB
at C3); the MAPPO critic's flat input (local || global of the same env) is rebuilt on the device by
`msc_env_obs_flat` when needed instead of storing [T, E, W, L(1+W)] (32 GB at C3).
"""
from __future__ import annotations

import contextlib
import ctypes as C
import os
from dataclasses import dataclass
from typing import Any, Dict, Optional

import torch
import torch.nn as nn

from . import abi
from . import mlp as mlp3
from .dist import allreduce_adv_stats
from .mlp import mlp3_forward
from .vec_env import VecInventoryEnv

_ACT = {"relu": nn.ReLU, "tanh": nn.Tanh, "elu": nn.ELU, "gelu": nn.GELU, "sigmoid": nn.Sigmoid}


def _act(name: str) -> nn.Module:
    return _ACT.get(str(name).lower(), nn.ReLU)()


class MLP(nn.Sequential):
    def __init__(self, in_dim: int, out_dim: int, config: Dict[str, Any]):
        layers, d = [], in_dim
        for h in config.get("hidden_sizes", [128, 128]):
            layers += [nn.Linear(d, h), _act(config.get("activation", "relu"))]
            d = h
        layers.append(nn.Linear(d, out_dim))
        if config.get("output_activation"):
            layers.append(_act(config["output_activation"]))
        super().__init__(*layers)

    def forward(self, x: torch.Tensor) -> torch.Tensor:
        return mlp_forward(self, x)


class GRUNet(nn.ModuleDict):
    """The reference's `gru` architecture (architectures/gru.py:14-85): {"gru": nn.GRU(batch_first),
    "output_proj": Linear, or Sequential([act,] Linear [, out_act]) when `activation` /
    `output_activation` are set}, stepped as BaseRLModule._forward_gru does (rlmodules/base.py:99-141)
    with the state laid out [rows, num_layers, hidden]. Unidirectional, no dropout."""

    def __init__(self, in_dim: int, out_dim: int, config: Dict[str, Any]):
        cfg = config or {}
        if cfg.get("bidirectional", False):
            raise ValueError("gru: bidirectional GRUs are not supported")
        if float(cfg.get("dropout", 0.0) or 0.0) > 0.0:
            raise ValueError("gru: dropout > 0 is not supported")
        hidden, layers = int(cfg.get("hidden_size", 128)), int(cfg.get("num_layers", 2))
        gru = nn.GRU(input_size=in_dim, hidden_size=hidden, num_layers=layers, batch_first=True)
        proj = []
        if cfg.get("activation"):
            proj.append(_act(cfg["activation"]))
        proj.append(nn.Linear(hidden, out_dim))
        if cfg.get("output_activation"):
            proj.append(_act(cfg["output_activation"]))
        super().__init__({"gru": gru, "output_proj": nn.Sequential(*proj) if len(proj) > 1 else proj[0]})
        self.in_dim, self.out_dim, self.hidden, self.layers = int(in_dim), int(out_dim), hidden, layers
        self.max_seq_len = int(cfg["max_seq_len"]) if cfg.get("max_seq_len") is not None else None

    def zero_state(self, *lead: int, device=None) -> torch.Tensor:
        dev = device if device is not None else next(self.parameters()).device
        return torch.zeros(*lead, self.layers, self.hidden, device=dev)

    def step(self, x: torch.Tensor, h: torch.Tensor, reset: Optional[torch.Tensor] = None, group: int = 1, *,
             store_state: bool = True, h_out: Optional[torch.Tensor] = None):
        """One time step: x [..., in], h [..., layers, hidden] -> (y [..., out], h' or None); rows whose
        group's reset flag is non-zero start from zero. One fused launch at rollout (marlsc/gru.py)."""
        from .gru import gru_step_forward
        return gru_step_forward(self, x, h, reset, group, store_state=store_state, h_out=h_out)

    def sequence(self, x: torch.Tensor, h0: torch.Tensor, keep: Optional[torch.Tensor] = None):
        """x [B, S, in] from the state h0 [B, layers, hidden] through the torch layers (autograd as
        enabled): (y [B, S, out], final state). keep [B, S] multiplies the state entering step s
        (0 = the row starts a new episode there); without resets the whole chunk is one nn.GRU call."""
        g = self["gru"]
        h = h0.transpose(0, 1).contiguous()
        if keep is None:
            o, h = g(x, h)
        else:
            outs = []
            for s in range(x.shape[1]):
                h = h * keep[:, s].to(h.dtype)[None, :, None]
                o, h = g(x[:, s:s + 1], h)
                outs.append(o)
            o = torch.cat(outs, dim=1)
        return self["output_proj"](o), h.transpose(0, 1)


def check_gru_config(nets: Dict[str, Any], actor_obs_type: str, critic_obs_type: str,
                     batch_size: Optional[int] = None, num_minibatches: Optional[int] = None) -> Optional[int]:
    """The schema's recurrent-network rules (config/schema.py:923-957, 969-978, 1143-1151, 1284-1313) on
    a `networks` dict; returns the common max_seq_len, or None when no network is a GRU."""
    nets = nets or {}
    sl = nets.get("shared_layers")
    seq = []
    for name in ("shared_layers", "actor", "critic"):
        d = nets.get(name) or {}
        typ = d.get("type", "mlp") if d else "mlp"
        if name == "shared_layers":
            if not sl:
                continue
            if typ != "gru":
                raise ValueError(f"shared_layers: type '{typ}' is not supported (only gru shared layers)")
        elif typ not in ("mlp", "gru"):
            raise ValueError(f"{name}: network type '{typ}' is not supported (mlp or gru)")
        if typ != "gru":
            continue
        c = d.get("config") or {}
        if c.get("max_seq_len") is None:
            raise ValueError(f"{name}: max_seq_len is required for gru networks")
        if int(c["max_seq_len"]) < 1:
            raise ValueError(f"{name}: max_seq_len must be >= 1")
        if c.get("bidirectional", False):
            raise ValueError(f"{name}: bidirectional GRUs are not supported")
        if float(c.get("dropout", 0.0) or 0.0) > 0.0:
            raise ValueError(f"{name}: dropout > 0 is not supported")
        seq.append(int(c["max_seq_len"]))
    if sl:
        if (sl.get("config") or {}).get("output_dim") is None:
            raise ValueError("shared_layers: config.output_dim is required")
        if actor_obs_type != critic_obs_type:
            raise ValueError("shared_layers requires actor_obs_type == critic_obs_type "
                             f"(got '{actor_obs_type}' and '{critic_obs_type}')")
    if not seq:
        return None
    if len(set(seq)) > 1:
        raise ValueError(f"all gru networks must share one max_seq_len (got {sorted(set(seq))})")
    if batch_size is not None and num_minibatches is not None and \
            int(batch_size) // max(1, int(num_minibatches)) < seq[0]:
        raise ValueError(f"minibatch size batch_size // num_minibatches = {int(batch_size) // max(1, int(num_minibatches))} "
                         f"must be >= max_seq_len = {seq[0]}")
    return seq[0]


LOG_STD_MIN, LOG_STD_MAX = -4.6, 4.6  # MuSigmaHead.LOG_STD_MIN / LOG_STD_MAX (mu_sigma_head.py:22-23)


class MuSigmaHead(nn.Module):
    """The reference's state-dependent Gaussian head (architectures/mu_sigma_head.py:52-82, following
    its code, not its docstring): on the backbone features f, mu = act_mu(mu_head(f)) -- not clamped
    -- and log_std = clamp(act_sigma(sigma_head(f)), -4.6, 4.6). Returns (mu, log_std) instead of
    their concatenation. action_low / action_high are the reference's buffers (unused by forward)."""

    def __init__(self, backbone_dim: int, action_dim: int, output_activation_mu: Optional[str] = None,
                 output_activation_sigma: Optional[str] = None):
        super().__init__()
        self.mu_head = nn.Linear(backbone_dim, action_dim)
        self.sigma_head = nn.Linear(backbone_dim, action_dim)
        self.register_buffer("action_low", torch.full((action_dim,), -1.0))
        self.register_buffer("action_high", torch.full((action_dim,), 1.0))
        self.mu_activation = _act(output_activation_mu) if output_activation_mu else None
        self.sigma_activation = _act(output_activation_sigma) if output_activation_sigma else None

    def forward(self, features: torch.Tensor):
        mu = self.mu_head(features)
        if self.mu_activation is not None:
            mu = self.mu_activation(mu)
        log_std = self.sigma_head(features)
        if self.sigma_activation is not None:
            log_std = self.sigma_activation(log_std)
        return mu, torch.clamp(log_std, LOG_STD_MIN, LOG_STD_MAX)


def check_head_config(nets: Dict[str, Any]) -> bool:
    """ActorCriticConfig._validate_output_activations (config/schema.py:1066-1093) on a `networks`
    dict, plus the head's need for an mlp actor (rlmodules/base.py:217-227 without the GRU);
    returns use_mu_sigma_head."""
    use = bool(nets.get("use_mu_sigma_head", False))
    actor = nets.get("actor") or {}
    acfg, ccfg = actor.get("config") or {}, (nets.get("critic") or {}).get("config") or {}
    for k in ("output_activation_mu", "output_activation_sigma"):
        if ccfg.get(k) is not None:
            raise ValueError(f"{k} is only valid for the actor, not the critic")
        if not use and acfg.get(k) is not None:
            raise ValueError(f"{k} is only valid when use_mu_sigma_head is true")
    if use:
        if actor.get("type", "mlp") != "mlp":
            raise ValueError(f"use_mu_sigma_head is not supported with actor type '{actor.get('type')}'")
        if acfg.get("output_activation") is not None:
            raise ValueError("output_activation must not be set on the actor when use_mu_sigma_head is true. "
                             "Use output_activation_mu and/or output_activation_sigma instead.")
    return use


def build_actor(in_dim: int, action_dim: int, rc: "RolloutConfig", default: Dict[str, Any]):
    """(actor, mu_sigma_head or None) as BaseRLModule builds them (rlmodules/base.py:213-262). With
    the head the actor is the backbone: the hidden layers plus one Linear to hidden_sizes[-1]
    features, every output_activation* key removed."""
    cfg = rc.actor or default
    if not rc.use_mu_sigma_head:
        return MLP(in_dim, action_dim, cfg), None
    cfg = dict(cfg)
    act_mu, act_sigma = cfg.pop("output_activation_mu", None), cfg.pop("output_activation_sigma", None)
    cfg.pop("output_activation", None)
    hidden = cfg.get("hidden_sizes", [256])
    dim = hidden[-1] if hidden else action_dim
    return MLP(in_dim, dim, cfg), MuSigmaHead(dim, action_dim, act_mu, act_sigma)


def network_types(nets: Dict[str, Any]) -> Dict[str, Any]:
    """RolloutConfig's actor_type / critic_type / shared_layers fields of a `networks` dict."""
    sl = (nets or {}).get("shared_layers")
    return {"actor_type": ((nets or {}).get("actor") or {}).get("type", "mlp") or "mlp",
            "critic_type": ((nets or {}).get("critic") or {}).get("type", "mlp") or "mlp",
            "shared_layers": dict(sl.get("config") or {}) if sl else None}


STATE_SLOTS = ("shared_h", "actor_h", "critic_h")  # the reference's state keys (rlmodules/base.py:351-388)


class PolicyNets:
    """One policy's networks as ActorCriticRLModule.setup builds them (rlmodules/base.py:150-262): an
    optional GRU trunk `shared_layers` on the raw actor observation whose output_dim features feed
    both actor and critic (base.py:196-210), an actor (MLP, MLP backbone under `mu_sigma_head`, or
    GRU) and a critic (MLP or GRU), then the free `log_std` unless the head is used. Mixed into the
    nn.Modules that hold them. MLP-only configs build parameter for parameter as before."""

    def _build_nets(self, local_obs_dim: int, global_obs_dim: int, action_dim: int, rc: "RolloutConfig",
                    default_actor: Dict[str, Any], default_critic: Dict[str, Any]) -> None:
        full = local_obs_dim + global_obs_dim
        a_in = full if rc.actor_obs_type == "global" else local_obs_dim
        c_in = full if rc.critic_obs_type == "global" else local_obs_dim
        if rc.shared_layers is not None:
            self.shared_layers = GRUNet(a_in, int(rc.shared_layers["output_dim"]), rc.shared_layers)
            a_in = c_in = int(rc.shared_layers["output_dim"])
        if rc.actor_type == "gru":
            self.actor, head = GRUNet(a_in, action_dim, rc.actor or {}), None
        else:
            self.actor, head = build_actor(a_in, action_dim, rc, default_actor)
        self.head_mode = head is not None
        if self.head_mode:
            self.mu_sigma_head = head
        if rc.critic_type == "gru":
            self.critic = GRUNet(c_in, 1, rc.critic or {})
        else:
            self.critic = MLP(c_in, 1, rc.critic or default_critic)
        if not self.head_mode:
            self.log_std = nn.Parameter(torch.full((action_dim,), float(rc.logstd_init)))

    def gru_slots(self) -> Dict[str, GRUNet]:
        d = {}
        if getattr(self, "shared_layers", None) is not None:
            d["shared_h"] = self.shared_layers
        if isinstance(self.actor, GRUNet):
            d["actor_h"] = self.actor
        if isinstance(self.critic, GRUNet):
            d["critic_h"] = self.critic
        return d

    def step_rows(self, a_x, c_x, state, reset=None, group: int = 1, *, store: bool = True, out_state=None,
                  actor: bool = True, critic: bool = True):
        """One time step over rows: a_x / c_x [n, in] (the raw actor / critic observations), state
        {slot: [n, layers, hidden]} -> (actor input [n, .] when the actor is an MLP else None, the
        GRU actor's means [n, K] else None, values [n] or None, new state per slot -- None entries
        with store False). Trunk, actor and critic run once each."""
        out_state = out_state or {}
        new: Dict[str, Optional[torch.Tensor]] = {}
        a_in, c_in = a_x, c_x
        if "shared_h" in state:
            a_in, new["shared_h"] = self.shared_layers.step(a_x, state["shared_h"], reset, group, store_state=store,
                                                            h_out=out_state.get("shared_h"))
            c_in = a_in
        mean = values = None
        if "actor_h" in state and actor:
            mean, new["actor_h"] = self.actor.step(a_in, state["actor_h"], reset, group, store_state=store,
                                                   h_out=out_state.get("actor_h"))
        if critic:
            if "critic_h" in state:
                values, new["critic_h"] = self.critic.step(c_in, state["critic_h"], reset, group, store_state=store,
                                                           h_out=out_state.get("critic_h"))
            else:
                values = mlp_forward(self.critic, c_in)
            values = values.squeeze(-1)
        return (None if "actor_h" in state else a_in), mean, values, new

    def sequence_rows(self, a_x, c_x, state_in, keep, logstd_floor: float):
        """(mean [B, S, K], log_std, values [B, S]) of chunks a_x / c_x [B, S, in] from the states
        state_in {slot: [B, layers, hidden]}; keep [B, S] (or None) multiplies the state entering
        each step. The torch layers, with autograd as enabled (BPTT over the chunk)."""
        a_in, c_in = a_x, c_x
        if "shared_h" in state_in:
            a_in, _ = self.shared_layers.sequence(a_x, state_in["shared_h"], keep)
            c_in = a_in
        if "actor_h" in state_in:
            mean, _ = self.actor.sequence(a_in, state_in["actor_h"], keep)
        elif self.head_mode:
            mean, log_std = self.mu_sigma_head(self.actor(a_in))
        else:
            mean = self.actor(a_in)
        if not self.head_mode:
            log_std = torch.clamp(self.log_std, min=logstd_floor).expand_as(mean)
        if "critic_h" in state_in:
            values, _ = self.critic.sequence(c_in, state_in["critic_h"], keep)
        else:
            values = self.critic(c_in)
        return mean, log_std, values.squeeze(-1)


def recurrent_step(policies, shared: bool, rc: "RolloutConfig", local_obs, full_obs, state, reset=None, *,
                   store: bool = True, out_state=None, actor: bool = True, critic: bool = True):
    """PolicyNets.step_rows over [E, W, .] observations and {slot: [E, W, layers, hidden]} states for one
    shared policy (all E W rows in one call, the reset flags [E] applying to groups of W rows) or W
    per-agent policies. Returns (actor input [E, W, .] or None, means [E, W, K] or None, values
    [E, W] or None, new state per slot)."""
    a_x = full_obs if rc.actor_obs_type == "global" else local_obs
    c_x = full_obs if rc.critic_obs_type == "global" else local_obs
    E, W = local_obs.shape[0], local_obs.shape[1]
    if shared:
        flat = lambda t: None if t is None else t.reshape(E * W, *t.shape[2:])  # noqa: E731
        a_in, mean, v, new = policies[0].step_rows(
            flat(a_x), flat(c_x), {k: flat(h) for k, h in state.items()}, reset, W, store=store,
            out_state={k: flat(h) for k, h in (out_state or {}).items()}, actor=actor, critic=critic)
        un = lambda t: None if t is None else t.reshape(E, W, *t.shape[1:])  # noqa: E731
        return un(a_in), un(mean), un(v), {k: un(h) for k, h in new.items()}
    # (a slot is None once a step skipped its network, e.g. the critic's in evaluation: as the shared path takes it)
    parts = [p.step_rows(a_x[:, w].contiguous(), c_x[:, w].contiguous(),
                         {k: None if h is None else h[:, w].contiguous() for k, h in state.items()},
                         reset, 1, store=store, actor=actor, critic=critic) for w, p in enumerate(policies)]
    st = lambda i: None if parts[0][i] is None else torch.stack([q[i] for q in parts], dim=1)  # noqa: E731
    new = {}
    for k in state:
        hs = [q[3].get(k) for q in parts]
        new[k] = None if hs[0] is None else torch.stack(hs, dim=1)
        if new[k] is not None and out_state and k in out_state:
            new[k] = out_state[k].copy_(new[k])
    return st(0), st(1), st(2), new


# Inference (no autograd): a whole Linear-ReLU-Linear-ReLU-Linear MLP with hidden sizes 64 / 128 /
# 256 (both actors, the IPPO critic) runs as one f32-MFMA kernel (marlsc/mlp.py, MSC_FUSED_MLP3=0
# turns it off); any other Linear -> ReLU pair runs as one GEMM with the ReLU in the GEMM epilogue
# (torch._addmm_activation -> hipBLASLt). MSC_FUSED_MLP=0 restores the plain layer sequence.
_FUSED = os.environ.get("MSC_FUSED_MLP", "1") != "0"


def _out_rows(out: Optional[torch.Tensor], rows: int, n_out: int) -> Optional[torch.Tensor]:
    """`out` as the fused kernel's [rows, n_out] output buffer, or None when it cannot be one."""
    if out is None or not out.is_contiguous() or out.dtype != torch.float32 or out.numel() != rows * n_out:
        return None
    return out.view(rows, n_out)


def mlp_forward(layers, x: torch.Tensor, start: int = 0, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """layers[start:] applied to x (an nn.Sequential of Linear / activation modules). `out`: a
    buffer the fused kernel may write the result into (the caller checks the returned pointer)."""
    mods = list(layers)[start:]
    if not (_FUSED and x.is_cuda and not torch.is_grad_enabled()):
        for m in mods:
            x = m(x)
        return x
    if mlp3.ENABLED and x.dtype == torch.float32 and mlp3.fusable(mods):
        n_out = mods[-1].out_features
        # the whole MLP as one f32-MFMA kernel (csrc/mlp.hip)
        return mlp3_forward(mods, x, _out_rows(out, x.numel() // x.shape[-1], n_out))
    if mlp3.ENABLED and mlp3.WIDE_ENABLED and x.dtype == torch.float32 and mlp3.wide_layers(mods):
        # 33..128 outputs (the centralised actor's joint action): the wide kernel (csrc/mlp_wide.hip),
        # opt-in with MSC_WIDE_MLP=1
        return mlp3.wide_forward(mods, x, _out_rows(out, x.numel() // x.shape[-1], mods[-1].out_features))
    i = 0
    while i < len(mods):
        m = mods[i]
        if isinstance(m, nn.Linear) and m.bias is not None and i + 1 < len(mods) and isinstance(mods[i + 1], nn.ReLU):
            lead = x.shape[:-1]
            x = torch._addmm_activation(m.bias, x.reshape(-1, x.shape[-1]), m.weight.t()).reshape(*lead, -1)
            i += 2
        else:
            x = m(x)
            i += 1
    return x


@dataclass
class RolloutConfig:
    gamma: float = 0.99
    lam: float = 0.95
    actor_obs_type: str = "local"
    critic_obs_type: str = "global"
    logstd_init: float = -1.0
    logstd_floor: float = -3.5
    actor: Optional[Dict[str, Any]] = None
    critic: Optional[Dict[str, Any]] = None
    # networks.use_mu_sigma_head: the actor is a backbone under a MuSigmaHead (state-dependent
    # log_std; no free log_std parameter, logstd_init / logstd_floor unused)
    use_mu_sigma_head: bool = False
    # networks.{actor,critic}.type ("mlp" or "gru") and networks.shared_layers.config of a gru trunk
    # (None: no shared layers); max_seq_len is derived (the GRUs' common value, None without a GRU)
    actor_type: str = "mlp"
    critic_type: str = "mlp"
    shared_layers: Optional[Dict[str, Any]] = None
    max_seq_len: Optional[int] = None

    def networks(self) -> Dict[str, Any]:
        nets = {"use_mu_sigma_head": self.use_mu_sigma_head, "actor": {"type": self.actor_type, "config": self.actor},
                "critic": {"type": self.critic_type, "config": self.critic}}
        if self.shared_layers is not None:
            nets["shared_layers"] = {"type": "gru", "config": self.shared_layers}
        return nets

    def __post_init__(self):
        check_head_config(self.networks())
        self.max_seq_len = check_gru_config(self.networks(), self.actor_obs_type, self.critic_obs_type)

    @classmethod
    def from_algorithm_config(cls, cfg: Dict[str, Any]) -> "RolloutConfig":
        """From a config_files/algorithms/*.yaml dict (the reference's schema)."""
        a = cfg.get("algorithm", cfg)
        s = a.get("algorithm_specific", {})
        nets = s.get("networks", {}) or {}
        head = check_head_config(nets)
        a_obs = s.get("actor_obs_type", "local")
        c_obs = s.get("critic_obs_type", "global" if a.get("name") == "mappo" else "local")
        check_gru_config(nets, a_obs, c_obs, (a.get("shared") or {}).get("batch_size"),
                         (a.get("shared") or {}).get("num_minibatches"))
        return cls(gamma=float(s.get("gamma", 0.99)), lam=float(s.get("lam", 0.95)),
                   actor_obs_type=s.get("actor_obs_type", "local"),
                   critic_obs_type=s.get("critic_obs_type", "global" if a.get("name") == "mappo" else "local"),
                   logstd_init=float(s.get("logstd_init", -1.0)), logstd_floor=float(s.get("logstd_floor", -3.5)),
                   actor=(nets.get("actor") or {}).get("config"), critic=(nets.get("critic") or {}).get("config"),
                   use_mu_sigma_head=head, **network_types(nets))


class RecurrentAPI:
    """The collector's / learner's view of a module with GRU networks, over [E, W, .] tensors: needs
    `_policy_list()` (one shared policy or W per-agent ones), `shared`, `rc` and `W`."""

    @property
    def recurrent(self) -> bool:
        r = self.__dict__.get("_recurrent")  # (fixed at construction; asked on every stateless call)
        if r is None:
            r = self.__dict__["_recurrent"] = bool(self._policy_list()[0].gru_slots())
        return r

    @property
    def max_seq_len(self) -> Optional[int]:
        return self.rc.max_seq_len

    def _stateless(self) -> None:
        if self.recurrent:
            raise ValueError("GRU networks carry state: use initial_state / step / sequence instead")

    def initial_state(self, n: int, device=None) -> Dict[str, torch.Tensor]:
        """Zeros [n, W, num_layers, hidden] per state slot (get_initial_state, rlmodules/base.py:351-388)."""
        return {k: g.zero_state(n, self.W, device=device) for k, g in self._policy_list()[0].gru_slots().items()}

    def step(self, local_obs, full_obs, state, reset=None, *, store: bool = True, out_state=None, actor: bool = True,
             critic: bool = True):
        """One time step taking and returning the state (see recurrent_step)."""
        return recurrent_step(self._policy_list(), self.shared, self.rc, local_obs, full_obs, state, reset, store=store,
                              out_state=out_state, actor=actor, critic=critic)

    def sequence(self, local_obs, full_obs, state_in, keep=None):
        """(mean, log_std, values) over [B, S, W, .] chunks from {slot: [B, W, layers, hidden]}; keep
        [B, S] (1 - truncated of the previous step, 1 at s = 0) is shared by an env's agents."""
        rc, ps = self.rc, self._policy_list()
        a_x = full_obs if rc.actor_obs_type == "global" else local_obs
        c_x = full_obs if rc.critic_obs_type == "global" else local_obs
        outs = []
        for w in range(local_obs.shape[2]):
            p = ps[0] if self.shared else ps[w]
            outs.append(p.sequence_rows(a_x[:, :, w], c_x[:, :, w], {k: h[:, w] for k, h in state_in.items()}, keep,
                                        rc.logstd_floor))
        return tuple(torch.stack([o[i] for o in outs], dim=2) for i in range(3))


class ActorCritic(RecurrentAPI, PolicyNets, nn.Module):
    shared = True

    def __init__(self, local_obs_dim: int, global_obs_dim: int, action_dim: int, rc: RolloutConfig):
        super().__init__()
        self.local_obs_dim, self.rc = local_obs_dim, rc
        self.W = max(1, global_obs_dim // max(1, local_obs_dim))
        self._build_nets(local_obs_dim, global_obs_dim, action_dim, rc, {"hidden_sizes": [256, 256]},
                         {"hidden_sizes": [64, 64]})

    def _policy_list(self):
        return [self]

    def actor_sample_x(self, x: torch.Tensor, sample) -> bool:
        return fused_actor_sample(self.actor, x, sample)

    def sample_actions_x(self, x, eps, actions, logp) -> torch.Tensor:
        return head_sample(self.actor, self.mu_sigma_head, x, eps, actions, logp)

    def actor_mean_x(self, x: torch.Tensor) -> torch.Tensor:
        return self.actor(x)

    def dist_inputs(self, local_obs: torch.Tensor, full_obs: Optional[torch.Tensor] = None):
        """(mean, log_std) -- ACTION_DIST_INPUTS split in two."""
        self._stateless()
        if self.head_mode:  # the torch layer sequence (per-row log_std), with or without autograd
            return self.mu_sigma_head(self.actor(full_obs if self.rc.actor_obs_type == "global" else local_obs))
        mean = self.actor_mean(local_obs, full_obs)
        log_std = torch.clamp(self.log_std, min=self.rc.logstd_floor).expand_as(mean)
        return mean, log_std

    def actor_mean(self, local_obs: torch.Tensor, full_obs: Optional[torch.Tensor] = None) -> torch.Tensor:
        if self.head_mode:
            return self.dist_inputs(local_obs, full_obs)[0]
        return self.actor(full_obs if self.rc.actor_obs_type == "global" else local_obs)

    def log_std_table(self) -> Optional[torch.Tensor]:
        """[1, K] unclamped log_std for msc_gaussian_sample (the kernel applies logstd_floor); None
        with the mu/sigma head (log_std is per row: sample_actions)."""
        if self.head_mode:
            return None
        return self.log_std.detach().float().reshape(1, -1).contiguous()

    def sample_actions(self, local_obs, full_obs, eps, actions, logp) -> torch.Tensor:
        """Head mode: the rollout step's actor forward and sampling (see head_sample)."""
        x = full_obs if self.rc.actor_obs_type == "global" else local_obs
        return head_sample(self.actor, self.mu_sigma_head, x, eps, actions, logp)

    def actor_sample(self, local_obs: torch.Tensor, full_obs: Optional[torch.Tensor], sample) -> bool:
        """The actor forward with the action sampling fused into its kernel (see fused_actor_sample)."""
        return fused_actor_sample(self.actor, full_obs if self.rc.actor_obs_type == "global" else local_obs, sample)

    def values(self, local_obs: torch.Tensor, full_obs: Optional[torch.Tensor] = None,
               out: Optional[torch.Tensor] = None) -> torch.Tensor:
        """V [..., W]; `out` (contiguous, that shape) receives it when the fused critic runs."""
        self._stateless()
        if self.rc.critic_obs_type == "global" and full_obs is None:
            return split_global_mlp(self.critic, local_obs, out=out).squeeze(-1)
        x = full_obs if self.rc.critic_obs_type == "global" else local_obs
        return mlp_forward(self.critic, x, out=out).squeeze(-1)


def split_global_mlp(mlp: nn.Sequential, local_obs: torch.Tensor, agent: Optional[int] = None,
                     out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """An MLP over the per-agent flat input local_w || (local_0 .. local_{W-1}) evaluated from the
    local observations [..., W, L] without materialising it: the first Linear's columns split into
    a local block (per agent) and a global block (once per env, shared by its W agents) --
    mathematically the same layer, ~W x fewer first-layer flops and no [E, W, L(1+W)] buffer.
    agent=None: all W agents ([..., W, out]); agent=w: agent w only ([..., out]).
    out: a contiguous buffer of the fused kernel's output (rows x outputs), used when it runs."""
    first = mlp[0]
    W, L = local_obs.shape[-2], local_obs.shape[-1]
    glob = local_obs.reshape(*local_obs.shape[:-2], W * L)
    mods = list(mlp)
    if (agent is None and _FUSED and mlp3.ENABLED and local_obs.is_cuda and local_obs.dtype == torch.float32
            and not torch.is_grad_enabled() and mlp3.fusable(mods)):
        # the whole critic as one f32-MFMA kernel over the E*W rows, with the per-env global block
        # (one GEMM over E rows) added to the first layer of each of the env's W rows
        g = torch.nn.functional.linear(glob.reshape(-1, W * L), first.weight[:, L:])  # b1: in the kernel
        o = _out_rows(out, local_obs[..., 0].numel(), mods[-1].out_features)
        return mlp3_forward(mods, local_obs, o, w1=first.weight[:, :L], pre1=g, group=W)
    g = torch.nn.functional.linear(glob, first.weight[:, L:])
    if agent is None:
        h = torch.nn.functional.linear(local_obs, first.weight[:, :L], first.bias) + g.unsqueeze(-2)
    else:
        h = torch.nn.functional.linear(local_obs[..., agent, :], first.weight[:, :L], first.bias) + g
    return mlp_forward(mlp, h, 1)


def fused_actor_sample(actor: nn.Sequential, x: torch.Tensor, sample) -> bool:
    """Run `actor` over x with msc_gaussian_sample fused into the MLP kernel's epilogue (sample =
    (log_std [P, K], logstd_floor, eps, actions, logp, clipped)); False (nothing launched) when the
    fused kernel does not apply, e.g. 9..32 or more than 128 outputs, or a non-ReLU MLP. 33..128 outputs
    (the centralised actor): the wide kernel's epilogue (mlp.wide_forward) with MSC_WIDE_MLP=1."""
    mods = list(actor)
    if not (_FUSED and mlp3.ENABLED and x.is_cuda and x.dtype == torch.float32 and not torch.is_grad_enabled()):
        return False
    if mlp3.sample_fusable(mods):
        mlp3_forward(mods, x, None, sample=sample)
        return True
    if mlp3.WIDE_ENABLED and mlp3.wide_layers(mods):
        mlp3.wide_forward(mods, x, None, sample=sample)
        return True
    return False


def _vp(t: Optional[torch.Tensor]):
    return None if t is None else C.c_void_p(t.data_ptr())


def head_sample(actor: nn.Sequential, head: MuSigmaHead, x: torch.Tensor, eps: torch.Tensor, actions: torch.Tensor,
                logp: torch.Tensor) -> torch.Tensor:
    """One rollout step of a mu/sigma-head policy over x [..., in]: actions / logp written, the
    [-1, 1] clipped actions returned. First path that applies (marlsc/mlp.py:musigma_tier):
    1. K <= 8, fusable ReLU backbone: backbone -> folded dual head -> activations, clamp -> sampling
       in one launch (msc_mlp{2,3}_relu_musigma);
    2. 9 <= K <= 16: the fused MLP kernel on the folded weights (MFMA output layer), activations and
       clamp in torch, msc_gaussian_sample with one log_std row per row;
    3. otherwise the torch layers, then msc_gaussian_sample with one log_std row per row.
    The sampling kernel's floor is the clamp's lower bound, so it changes nothing."""
    tier = 3
    if _FUSED and mlp3.ENABLED and x.is_cuda and x.dtype == torch.float32 and not torch.is_grad_enabled():
        tier = mlp3.musigma_tier(list(actor), head)
    if tier == 1:
        clipped = torch.empty_like(actions)
        mlp3.musigma_forward(list(actor), head, x, sample=(eps, actions, logp, clipped))
        return clipped
    mu, ls = mlp3.musigma_folded(list(actor), head, x) if tier == 2 else head(actor(x))
    return gaussian_sample(mu.contiguous(), ls.contiguous(), LOG_STD_MIN, eps, actions, logp)


def gaussian_sample(mean: torch.Tensor, log_std: torch.Tensor, logstd_floor: float, eps: torch.Tensor,
                    actions: torch.Tensor, logp: torch.Tensor) -> torch.Tensor:
    """msc_gaussian_sample: actions = mean + exp(max(log_std, floor)) * eps, logp = the diagonal
    Gaussian log-density summed over the last dim, into `actions` / `logp`; returns the [-1, 1]
    clipped actions the env receives. mean / eps / actions [..., K], logp [...] (f32 CUDA);
    log_std [K] (shared) or [P, K] repeating every P rows (e.g. [W, K]: one row per agent)."""
    K = mean.shape[-1]
    for t in (mean, eps, actions, logp):
        assert t.is_cuda and t.dtype == torch.float32 and t.is_contiguous()
    assert actions.shape == mean.shape == eps.shape and logp.shape == mean.shape[:-1]
    ls = log_std.detach().float().reshape(-1, K).contiguous()
    assert (mean.numel() // K) % ls.shape[0] == 0
    clipped = torch.empty_like(mean)
    abi.check(abi.lib().msc_gaussian_sample(_vp(mean), _vp(ls), ls.shape[0], C.c_float(logstd_floor), _vp(eps),
                                            mean.numel() // K, K, _vp(actions), _vp(logp), _vp(clipped),
                                            C.c_void_p(torch.cuda.current_stream().cuda_stream)))
    return clipped


def gae(rewards, values, next_values, terminated, truncated, gamma, lam, adv=None, targets=None, stats=None,
        groups: int = 1):
    """msc_gae_grouped over [T, N] (values [T+1, N]); returns (adv, targets, stats [groups, 3] f64 of
    [sum, sum_sq, n] per group; sequence n belongs to group n % groups)."""
    T, N = rewards.shape
    for name, t, shape in (("rewards", rewards, (T, N)), ("values", values, (T + 1, N)),
                           ("next_values", next_values, (T, N))):
        if t.dtype != torch.float32 or not t.is_contiguous() or tuple(t.shape) != shape:
            raise ValueError(f"{name}: expected contiguous float32 {shape}")
    for name, t in (("terminated", terminated), ("truncated", truncated)):
        if t.dtype != torch.uint8 or not t.is_contiguous() or tuple(t.shape) != (T, N):
            raise ValueError(f"{name}: expected contiguous uint8 {(T, N)}")
    adv = torch.empty_like(rewards) if adv is None else adv
    targets = torch.empty_like(rewards) if targets is None else targets
    if stats is None:
        stats = torch.zeros((groups, 3), dtype=torch.float64, device=rewards.device)
    elif tuple(stats.shape) != (groups, 3) or stats.dtype != torch.float64:
        raise ValueError(f"stats: expected float64 {(groups, 3)}")
    else:
        stats.zero_()
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    abi.check(abi.lib().msc_gae_grouped(_vp(rewards), _vp(values), _vp(next_values), _vp(terminated), _vp(truncated),
                                        N, T, C.c_float(gamma), C.c_float(lam), _vp(adv), _vp(targets), int(groups),
                                        _vp(stats), st))
    return adv, targets, stats


def normalize_advantages(adv: torch.Tensor, stats: torch.Tensor) -> torch.Tensor:
    """In place (A - mean_g) / max(1e-4, std_g) with the (already all-reduced) statistics of the
    [groups, 3] table; element i of the flattened [T, N] advantages belongs to group i % groups."""
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    g = stats.numel() // 3
    abi.check(abi.lib().msc_adv_normalize_grouped(_vp(adv), adv.numel(), g, _vp(stats), st))
    return adv


NOISE_CHUNK = 16  # rollout steps whose Gaussian noise is drawn in one launch
_TORCH_NOISE = os.environ.get("MSC_NOISE", "keyed") == "torch"


def keyed_normal(shape, row0: int, seed: int, step0: int) -> torch.Tensor:
    """msc_normal_keyed: f32 standard normals of shape [n_steps, n_envs, ...] on the current stream;
    element (s, e, j) depends only on (seed, global env row0 + e, step step0 + s, flat index j)."""
    n_steps, n_rows = int(shape[0]), int(shape[1])
    row_len = 1
    for d in shape[2:]:
        row_len *= int(d)
    out = torch.empty(tuple(shape), dtype=torch.float32, device=torch.device("cuda", torch.cuda.current_device()))
    abi.check(abi.lib().msc_normal_keyed(_vp(out), n_steps, n_rows, row_len, int(row0), int(seed) & 0xFFFFFFFFFFFFFFFF,
                                         int(step0), C.c_void_p(torch.cuda.current_stream().cuda_stream)))
    return out


class _Lane:
    """One env handle of a collector: its slice [e0, e1) of the buffers' env axis and the HIP stream
    its step chain (policy forward -> sampling -> env step) is issued on (None: the caller's)."""

    def __init__(self, env: VecInventoryEnv, e0: int, stream: Optional[torch.cuda.Stream], flat: Optional[torch.Tensor]):
        self.env, self.e0, self.e1, self.stream, self.flat = env, e0, e0 + env.n_envs, stream, flat
        self.noise: Optional[torch.Tensor] = None
        self.critic_stream: Optional[torch.cuda.Stream] = None  # V(obs_t) off the step chain
        self.obs_filtered = False  # the env's current observation already went through the obs filter

    def ctx(self):
        return torch.cuda.stream(self.stream) if self.stream is not None else contextlib.nullcontext()


class RolloutCollector:
    """T steps of E envs x W agents (N = E*W sequences). Advantages are standardised per module as
    RLlib's GAE connector does: over every agent for one shared policy (adv_groups = 1), per agent
    for one policy per agent (adv_groups = W).

    `env` may be a list of env handles (lanes) covering consecutive env-id ranges, e.g. the two
    halves of a rank's envs: each lane's step chain runs on its own HIP stream, so one lane's env
    kernels (VALU-bound) overlap the other lane's policy GEMMs (MFMA-bound). The buffers' env axis
    is the concatenation of the lanes; each env's trajectory is the same as with one handle (envs
    are independent and seeded by global id), and so is its Gaussian noise (keyed by global env id)."""

    def __init__(self, env, module: ActorCritic, T: int, *, seed: int = 0, adv_groups: int = 1,
                 obs_filter: str = "off"):
        envs = list(env) if isinstance(env, (list, tuple)) else [env]
        e0 = envs[0]
        for x in envs[1:]:
            if x.spec is not e0.spec and (x.W, x.K, x.L) != (e0.W, e0.K, e0.L):
                raise ValueError("rollout lanes must share one env spec")
        self.env, self.envs, self.module, self.T = e0, envs, module, int(T)
        E = sum(x.n_envs for x in envs)
        W, K, L = e0.W, e0.K, e0.local_obs_dim
        dev = e0.device
        self.E, self.N = E, E * W
        # T + 1 observation rows: the env writes step t's result straight into row t + 1 (no copy
        # per step); `obs` is the first T rows, the last one is copied back into the env at the end
        self._obs_all = torch.empty((T + 1, E, W, L), device=dev)
        self.obs = self._obs_all[:T]
        self.actions = torch.empty((T, E, W, K), device=dev)
        self.logp = torch.empty((T, E, W), device=dev)
        self.rewards = torch.empty((T, E, W), device=dev)
        self.values = torch.empty((T + 1, E, W), device=dev)
        self.next_values = torch.zeros((T, E, W), device=dev)
        self.terminated = torch.zeros((T, E, W), dtype=torch.uint8, device=dev)
        self.truncated = torch.zeros((T, E, W), dtype=torch.uint8, device=dev)
        self._trunc_env = torch.zeros((T, E), dtype=torch.uint8, device=dev)  # the env writes these rows
        self.adv = torch.empty((T, E, W), device=dev)
        self.targets = torch.empty((T, E, W), device=dev)
        if adv_groups not in (1, W):
            raise ValueError(f"adv_groups must be 1 (shared policy) or W={W} (one policy per agent)")
        self.adv_groups = int(adv_groups)
        self.stats = torch.zeros((self.adv_groups, 3), dtype=torch.float64, device=dev)
        self._need_flat = module.rc.actor_obs_type == "global"  # the critic splits its first layer
        # The values of obs_t are read only by the GAE after the rollout: with few envs the critic runs
        # on a side stream per lane, after the step that wrote obs_t, beside the actor -> sampling ->
        # env chain (C2 IPPO rollout 136.9 -> 139.5 M agent-steps/s); on a full chip it only takes
        # issue slots from the env kernels (C3 MAPPO 224.7 -> 214.9 M), and not when it reads the
        # lane's flat buffer, which the next step rewrites. MSC_ROLLOUT_CRITIC_SIDE=0|1 forces it.
        cs = os.environ.get("MSC_ROLLOUT_CRITIC_SIDE")
        self._critic_side = (self.N <= 65536 if cs is None else cs != "0") and not self._need_flat
        # Gaussian action noise keyed by (seed, global env id, rollout step): msc_normal_keyed, so an
        # env's noise does not depend on which rank or lane steps it
        self._noise_seed = int(seed) & 0xFFFFFFFFFFFFFFFF
        self.noise_step = 0  # rollout steps drawn so far (checkpointed)
        import inspect
        self._values_out = "out" in inspect.signature(module.values).parameters
        self._ls: Optional[torch.Tensor] = None
        self._head = bool(getattr(module, "head_mode", False))  # mu/sigma-head module (sample_actions)
        # GRU networks: per-env state per slot ([E, W, layers, hidden], zero now, carried across
        # collect() calls like the env's observation) in two buffers that the steps ping-pong, and the
        # learner's state_in[slot] [T / S, E, W, layers, hidden]: the state entering steps 0, S, 2S, ...
        self._recurrent = bool(getattr(module, "recurrent", False))
        self.state_in: Dict[str, torch.Tensor] = {}
        if self._recurrent:
            S = int(module.max_seq_len)
            if T % S != 0:
                raise ValueError(f"rollout length T = {T} must be a multiple of max_seq_len = {S}")
            self.S = S
            self._hbuf = [module.initial_state(E, device=dev), module.initial_state(E, device=dev)]
            self._hcur = 0
            self.state_in = {k: torch.zeros((T // S,) + tuple(h.shape), device=dev) for k, h in self._hbuf[0].items()}
            rc = module.rc
            self._need_flat = "global" in (rc.actor_obs_type, rc.critic_obs_type)
            self._critic_side = False  # the critic shares the trunk / carries state: on the chain
        # obs_normalization "meanstd": RLlib's running filter, one per lane (env runner), synchronised
        # after every collect (marlsc/obs_filter.py)
        self.obs_filter = None
        if obs_filter == "meanstd":
            from .obs_filter import MeanStdObsFilter
            self.obs_filter = MeanStdObsFilter(W * L, dev, n_lanes=len(envs))
        elif obs_filter not in ("off", None):
            raise ValueError(f"obs_filter must be 'off' or 'meanstd', not {obs_filter!r}")
        # Episode-ahead demand beside the policy kernels: at 4,096 envs it lifts the rollout (the
        # per-step demand chain would bound the step), at 32,768 the background generation takes the
        # MLP kernels' CU slots (C3 MAPPO rollout 1.15 -> 1.32 ms per step, profiles/r04/ab_ea_c3.txt),
        # so lanes of >= 16,384 envs step with per-step pipelined demand. MSC_ROLLOUT_EA=0|1 forces it.
        rea = os.environ.get("MSC_ROLLOUT_EA")
        for x in envs:
            if getattr(x, "ea_slots", 0) and hasattr(x, "set_episode_ahead"):
                x.set_episode_ahead(x.n_envs < 16384 if rea is None else rea != "0")
        self._lanes, off = [], 0
        for x in envs:
            st = torch.cuda.Stream(device=dev) if len(envs) > 1 else None
            flat = torch.empty((x.n_envs, W, L * (1 + W)), device=dev) if self._need_flat else None
            self._lanes.append(_Lane(x, off, st, flat))
            off += x.n_envs

    def _full(self, ln: _Lane, obs):
        return ln.env.obs_flat(obs=obs, out=ln.flat) if self._need_flat else None

    def _values_into(self, t: int, sl: slice, obs, full) -> None:
        """V(obs_t) into values[t, sl]: written by the fused critic kernel directly when the module
        takes an output buffer, copied otherwise."""
        dst = self.values[t, sl]
        v = self.module.values(obs, full, out=dst) if self._values_out else self.module.values(obs, full)
        if v.data_ptr() != dst.data_ptr():
            dst.copy_(v)

    def _critic_on_side(self, ln: _Lane, t: int, sl: slice, obs, full) -> None:
        if ln.critic_stream is None:
            ln.critic_stream = torch.cuda.Stream(device=obs.device)
        ev = torch.cuda.Event()
        ev.record()
        ln.critic_stream.wait_event(ev)
        with torch.cuda.stream(ln.critic_stream):
            self._values_into(t, sl, obs, full)

    def _noise_chunk(self, ln: _Lane) -> int:
        per_step = max(1, self.actions[0, ln.e0:ln.e1].numel() * 4)
        if os.environ.get("MSC_NOISE_CHUNK"):
            return max(1, int(os.environ["MSC_NOISE_CHUNK"]))
        return max(NOISE_CHUNK, min(self.T, (1 << 30) // per_step))

    @property
    def state(self) -> Dict[str, torch.Tensor]:
        """The current recurrent state per slot ([E, W, layers, hidden]; empty without GRU networks)."""
        return self._hbuf[self._hcur] if self._recurrent else {}

    def load_state(self, state: Dict[str, torch.Tensor]) -> None:
        for k, h in self.state.items():
            h.copy_(state[k].to(h.device))

    def _lane_noise(self, ln: _Lane, t: int, sl: slice) -> torch.Tensor:
        """Step t's standard-normal noise of the lane, drawn for `chunk` steps at once (one launch instead
        of one per step), keyed by global env id. The whole rollout's noise when it fits 1 GiB: a noise
        launch between step_c and the actor lets the next demand kernel reach the CUs before the actor,
        whose one 384-VGPR wave per SIMD then no longer fits beside the demand waves (the actor of
        that step 378 -> 906 us, profiles/r06/trace_roll_c3_r06il.txt)."""
        chunk = self._noise_chunk(ln)
        if t % chunk == 0:
            n = min(chunk, self.T - t)
            shape = (n,) + tuple(self.actions[t, sl].shape)
            if _TORCH_NOISE:  # A/B only: torch's generator (not shard-invariant)
                dev = self.actions.device
                if not hasattr(self, "_gen"):
                    self._gen = torch.Generator(device=dev).manual_seed(self._noise_seed & 0x7FFFFFFF)
                ln.noise = torch.randn(shape, device=dev, generator=self._gen)
            else:
                ln.noise = keyed_normal(shape, ln.env.env_index_offset, self._noise_seed, self.noise_step + t)
        return ln.noise[t % chunk]

    def _step_recurrent(self, ln: _Lane, t: int) -> None:
        """_step for modules with GRU networks: trunk / actor / critic once each on obs_t from the lane's
        state, with the reset flags of step t - 1 (an env's state is zero for the first observation of
        a new episode); V(final_obs) from the state after step t, which it does not advance."""
        env, m, sl = ln.env, self.module, slice(ln.e0, ln.e1)
        obs = self._obs_all[t, sl]
        full = self._full(ln, obs)
        cur = {k: h[sl] for k, h in self._hbuf[self._hcur].items()}
        nxt = {k: h[sl] for k, h in self._hbuf[self._hcur ^ 1].items()}
        reset = self._trunc_env[t - 1, sl] if t > 0 else None  # (the last collect's flags were applied at its end)
        if t % self.S == 0:  # the learner's chunk starts here: the state as the step reads it
            if reset is not None:
                keep = (reset == 0).to(torch.float32).view(-1, 1, 1, 1)
                for h in cur.values():
                    h.mul_(keep)
                reset = None
            for k, h in cur.items():
                self.state_in[k][t // self.S, sl].copy_(h)
        eps = self._lane_noise(ln, t, sl)
        a_in, mean, v, _ = m.step(obs, full, cur, reset, out_state=nxt)
        self.values[t, sl].copy_(v)
        a = None
        if mean is None:  # MLP actor on the trunk's features (or the raw observation): its fused paths
            if self._head:
                a = m.sample_actions_x(a_in, eps, self.actions[t, sl], self.logp[t, sl])
            else:
                clipped = torch.empty_like(self.actions[t, sl])
                if m.actor_sample_x(a_in, (self._ls, m.rc.logstd_floor, eps, self.actions[t, sl], self.logp[t, sl],
                                           clipped)):
                    a = clipped
                else:
                    mean = m.actor_mean_x(a_in)
        if a is None:
            a = gaussian_sample(mean.contiguous(), self._ls, m.rc.logstd_floor, eps, self.actions[t, sl], self.logp[t, sl])
        may_end = env.may_truncate()
        _, _, trunc, final_obs = env.step(a, obs_out=self._obs_all[t + 1, sl], rewards_out=self.rewards[t, sl],
                                          truncated_out=self._trunc_env[t, sl])
        if self.obs_filter is not None:
            li = self._lanes.index(ln)
            self.obs_filter.apply(li, self._obs_all[t + 1, sl])
            if may_end:
                self.obs_filter.apply(li, final_obs, mask=trunc)
        if may_end:  # RLlib's extra-timestep bootstrap: the state after step t, not advanced
            _, _, vf, _ = m.step(final_obs, self._full(ln, final_obs), nxt, None, store=False, actor=False)
            self.next_values[t, sl] = torch.where(trunc.bool().unsqueeze(-1), vf, torch.zeros((), device=vf.device))

    def _step(self, ln: _Lane, t: int) -> None:
        if self._recurrent:
            return self._step_recurrent(ln, t)
        env, m, sl = ln.env, self.module, slice(ln.e0, ln.e1)
        obs = self._obs_all[t, sl]
        full = self._full(ln, obs)
        if self._critic_side:
            self._critic_on_side(ln, t, sl, obs, full)
        eps = self._lane_noise(ln, t, sl)
        a = None
        if self._head:  # state-dependent log_std: one row per row (head_sample)
            a = m.sample_actions(obs, full, eps, self.actions[t, sl], self.logp[t, sl])
        elif self._ls is not None and hasattr(m, "actor_sample"):
            # actor forward + sampling + log-density + the env's clip in one kernel launch
            clipped = torch.empty_like(self.actions[t, sl])
            if m.actor_sample(obs, full, (self._ls, m.rc.logstd_floor, eps, self.actions[t, sl], self.logp[t, sl],
                                          clipped)):
                a = clipped
        if a is None:
            if self._ls is not None:  # the module's raw log_std rows, taken once per collect
                mean, ls = m.actor_mean(obs, full), self._ls
            else:
                mean, log_std = m.dist_inputs(obs, full)
                ls = log_std[0]
            # sample, log-density and the env's clip in one HIP kernel (msc_gaussian_sample)
            # (log_std rows: one shared row or one per agent, repeating every P rows)
            a = gaussian_sample(mean.contiguous(), ls, m.rc.logstd_floor, eps, self.actions[t, sl], self.logp[t, sl])
        if not self._critic_side:
            self._values_into(t, sl, obs, full)
        may_end = env.may_truncate()
        _, _, trunc, final_obs = env.step(a, obs_out=self._obs_all[t + 1, sl], rewards_out=self.rewards[t, sl],
                                          truncated_out=self._trunc_env[t, sl])
        li = self._lanes.index(ln) if self.obs_filter is not None else 0
        if self.obs_filter is not None:  # the new observations first, then the truncated envs' final ones
            self.obs_filter.apply(li, self._obs_all[t + 1, sl])
            if may_end:
                self.obs_filter.apply(li, final_obs, mask=trunc)
        # truncation bootstrap: V(final_obs) for the envs whose episode ended at this step
        # (skipped while the envs are known to be mid-episode in lockstep; next_values is zeroed
        # once per rollout)
        if may_end:
            full_f = self._full(ln, final_obs)
            self.next_values[t, sl] = torch.where(trunc.bool().unsqueeze(-1), m.values(final_obs, full_f),
                                                  torch.zeros((), device=final_obs.device))

    @torch.no_grad()
    def collect(self, normalize: bool = True) -> Dict[str, torch.Tensor]:
        m, T = self.module, self.T
        main = torch.cuda.current_stream()
        self.next_values.zero_()
        # log_std does not change during a collect: its rows go to the sampling kernel as they are
        # (the kernel clamps at logstd_floor), no clamp / broadcast launches per step
        self._ls = m.log_std_table() if hasattr(m, "log_std_table") and hasattr(m, "actor_mean") else None
        for ln in self._lanes:
            if not getattr(ln, "form_set", False) and hasattr(ln.env, "set_option"):
                # the observation kernel's spill-free form: with policy kernels between the steps it
                # is faster than the form the env stepping uses beside the demand kernel (C3 MAPPO
                # rollout 1.18 -> 1.14 ms per step, profiles/r06/ab_step_c_wpe.txt); results identical
                if os.environ.get("MSC_ROLLOUT_STEP_C_FORM", "4") == "4":
                    ln.env.set_option(ln.env.STEP_C_FORM, 4)
                # the allocation at full priority for its whole run: here the step chain, not the
                # demand kernel beside it, bounds a step (the env stepping's 14/16 split costs the C3
                # MAPPO rollout 1.14 -> 1.18 ms per step, profiles/r06/ab_alloc_prio.txt)
                ln.env.set_option(ln.env.ALLOC_PRIO_SPLIT, int(os.environ.get("MSC_ROLLOUT_AL_PRIO_SPLIT", "16")))
                ln.form_set = True
            if os.environ.get("MSC_ROLLOUT_CHAIN_PRIO", "0") != "0" and not getattr(ln, "prio_set", False):
                # A/B: step chain ahead of the next step's demand kernel (neutral: 1.234 vs 1.228 ms
                # per step; the step kernels wait for CU space, not for issue slots)
                ln.env.set_chain_priority(True)
                ln.prio_set = True
            if ln.stream is not None:
                ln.stream.wait_stream(main)
            with ln.ctx():
                self._obs_all[0, ln.e0:ln.e1].copy_(ln.env.obs)
                if self.obs_filter is not None and not ln.obs_filtered:  # the reset observation
                    self.obs_filter.apply(self._lanes.index(ln), self._obs_all[0, ln.e0:ln.e1])
                ln.obs_filtered = True
        # lanes interleaved per step on the host; each lane's chain is ordered on its own stream
        for t in range(T):
            for ln in self._lanes:
                with ln.ctx():
                    self._step(ln, t)
            if self._recurrent:
                self._hcur ^= 1
        for ln in self._lanes:
            with ln.ctx():
                last = self._obs_all[T, ln.e0:ln.e1]
                if self._recurrent:
                    # V(obs_T) as step T would compute it, state untouched; then the pending resets are
                    # applied, so an env whose episode ended at the last step holds a zero state
                    sl = slice(ln.e0, ln.e1)
                    cur, reset = {k: h[sl] for k, h in self.state.items()}, self._trunc_env[T - 1, sl]
                    self.values[T, sl] = m.step(last, self._full(ln, last), cur, reset, store=False, actor=False)[2]
                    keep = (reset == 0).to(torch.float32).view(-1, 1, 1, 1)
                    for h in cur.values():
                        h.mul_(keep)
                else:
                    self.values[T, ln.e0:ln.e1] = m.values(last, self._full(ln, last))
                ln.env.obs.copy_(last)  # the env's own buffer holds the current observation again
            if ln.stream is not None:
                main.wait_stream(ln.stream)
            if ln.critic_stream is not None:
                main.wait_stream(ln.critic_stream)
        self.noise_step += T
        # the per-env truncation flags of every step to every agent's sequence (one launch)
        self.truncated.copy_(self._trunc_env.unsqueeze(-1).expand_as(self.truncated))
        if self.obs_filter is not None:
            self.obs_filter.sync()
        N = self.N
        gae(self.rewards.view(T, N), self.values.view(T + 1, N), self.next_values.view(T, N),
            self.terminated.view(T, N), self.truncated.view(T, N), m.rc.gamma, m.rc.lam,
            self.adv.view(T, N), self.targets.view(T, N), self.stats, groups=self.adv_groups)
        if normalize:
            allreduce_adv_stats(self.stats)
            normalize_advantages(self.adv, self.stats)
        out = {"obs": self.obs, "actions": self.actions, "logp": self.logp, "rewards": self.rewards,
               "values": self.values, "advantages": self.adv, "value_targets": self.targets}
        if self._recurrent:
            out["state_in"], out["truncated"] = self.state_in, self.truncated
        return out
