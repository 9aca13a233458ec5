"""Host tests of the CPPO configuration and module (marlsc/cppo.py): the config class the algorithm name
selects, cppo.yaml, and the centralised module's dimensions and torch forward on the CPU."""
from pathlib import Path

import pytest
import torch
import yaml

REPO = Path(__file__).resolve().parents[1]


def _raw(name="cppo"):
    return yaml.safe_load(open(REPO / f"config_files/algorithms/{name}.yaml"))


def test_cppo_yaml_parses_into_cppo_config():
    from marlsc.cppo import CPPOConfig
    from marlsc.ppo import PPOConfig
    c = CPPOConfig.from_algorithm_config(_raw())
    assert isinstance(c, PPOConfig) and c.name == "cppo"
    assert c.actor_obs_type == "local" and c.critic_obs_type == "local" and c.parameter_sharing is False
    nets = c.networks
    for k in ("actor", "critic"):
        assert nets[k]["type"] == "mlp" and nets[k]["config"]["hidden_sizes"] == [256]
        assert nets[k]["config"]["activation"] == "relu"
    rc = c.rollout_config()
    assert rc.actor_obs_type == "local" and rc.critic_obs_type == "local" and not rc.use_mu_sigma_head
    assert set(CPPOConfig.__dataclass_fields__) == set(PPOConfig.__dataclass_fields__)  # the same fields


def test_cppo_config_forces_the_centralised_view_and_validates_like_ppo_config():
    from marlsc.cppo import CPPOConfig
    raw = _raw()
    raw["algorithm"]["algorithm_specific"].update(parameter_sharing=True, actor_obs_type="global", critic_obs_type="global")
    c = CPPOConfig.from_algorithm_config(raw)
    assert (c.actor_obs_type, c.critic_obs_type, c.parameter_sharing) == ("local", "local", False)
    raw = _raw()
    raw["algorithm"]["algorithm_specific"]["hysteretic_beta"] = 1.5
    with pytest.raises(ValueError):
        CPPOConfig.from_algorithm_config(raw)
    raw = _raw()
    raw["algorithm"]["algorithm_specific"]["obs_normalization"] = "nope"
    with pytest.raises(ValueError):
        CPPOConfig.from_algorithm_config(raw)


def test_each_config_class_reads_its_own_algorithms():
    from marlsc.cppo import CPPOConfig, CPPOTrainer, config_from_algorithm_config, trainer_class
    from marlsc.ppo import PPOConfig, PPOTrainer
    with pytest.raises(ValueError):
        PPOConfig.from_algorithm_config(_raw())  # cppo
    for name in ("ippo", "mappo"):
        with pytest.raises(ValueError):
            CPPOConfig.from_algorithm_config(_raw(name))
        c = config_from_algorithm_config(_raw(name))
        assert type(c) is PPOConfig and c.name == name and trainer_class(c) is PPOTrainer
    c = config_from_algorithm_config(_raw())
    assert type(c) is CPPOConfig and trainer_class(c) is CPPOTrainer
    assert issubclass(CPPOTrainer, PPOTrainer)


def test_centralised_module_dimensions_and_torch_forward():
    from marlsc.cppo import CentralizedActorCritic, CPPOConfig
    from marlsc.ppo import MultiAgentActorCritic
    W, L, K = 8, 34, 5
    rc = CPPOConfig.from_algorithm_config(_raw()).rollout_config()
    torch.manual_seed(0)
    m = CentralizedActorCritic(W * L, W * K, rc)
    assert isinstance(m, MultiAgentActorCritic) and m.W == 1 and not m.shared and len(m.policies) == 1
    p = m.policies[0]
    lins = [x for x in p.actor if isinstance(x, torch.nn.Linear)]
    assert [(x.in_features, x.out_features) for x in lins] == [(W * L, 256), (256, W * K)]
    lins = [x for x in p.critic if isinstance(x, torch.nn.Linear)]
    assert [(x.in_features, x.out_features) for x in lins] == [(W * L, 256), (256, 1)]
    assert p.log_std.shape == (W * K,)
    assert all(k.startswith("policies.0.") for k in m.state_dict())
    obs = torch.randn(6, 1, W * L)
    mean, log_std = m.dist_inputs(obs)
    assert mean.shape == (6, 1, W * K) and log_std.shape == mean.shape and m.values(obs).shape == (6, 1)
    assert torch.equal(mean[:, 0], p.actor(obs[:, 0]))
    assert m.log_std_table().shape == (1, W * K)
    from marlsc import mlp as M
    assert M.wide_layers(list(p.actor)) == 2 and M.fused_layers(list(p.actor)) == 0  # 40 outputs: the wide kernel
    assert M.fused_layers(list(p.critic)) == 2


def test_lazy_exports():
    import marlsc
    from marlsc import cppo
    for n in ("CPPOConfig", "CPPOTrainer", "CentralizedRolloutEnv", "CentralizedActorCritic"):
        assert n in marlsc.__all__ and getattr(marlsc, n) is getattr(cppo, n)
