"""Host tests of the mu/sigma actor head (use_mu_sigma_head: marlsc/rollout.py MuSigmaHead,
marlsc/ppo.py, marlsc/mlp.py fold_head): config selection and state-dict keys, the schema rules,
the reference's formula, one learner step and the inference fold. No GPU needed."""
import copy

import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F


def _cfg(head, actor=None, critic=None, actor_type="mlp"):
    return {"algorithm": {"name": "mappo", "shared": {}, "algorithm_specific": {
        "parameter_sharing": True, "logstd_init": -1.0, "logstd_floor": -3.5,
        "networks": {"shared_layers": None, "use_mu_sigma_head": head,
                     "actor": {"type": actor_type, "config": actor or {"hidden_sizes": [64, 32], "activation": "relu"}},
                     "critic": {"type": "mlp", "config": critic or {"hidden_sizes": [32], "activation": "relu"}}}}}}


def _rc(raw):
    from marlsc.ppo import PPOConfig
    return PPOConfig.from_algorithm_config(raw).rollout_config()


def test_config_selects_the_head():
    from marlsc.ppo import AgentModule, MultiAgentActorCritic
    from marlsc.rollout import ActorCritic, RolloutConfig
    for make in (_rc, RolloutConfig.from_algorithm_config):
        rc = make(_cfg(True))
        assert rc.use_mu_sigma_head is True
        for mod in (AgentModule(13, 26, 3, rc), ActorCritic(13, 26, 3, rc)):
            keys = set(mod.state_dict())
            # backbone: Linear(13, 64), Linear(64, 32) and the extra output Linear(32, 32)
            assert {f"actor.{i}.{p}" for i in (0, 2, 4) for p in ("weight", "bias")} <= keys
            assert tuple(mod.actor[4].weight.shape) == (32, 32) and len(mod.actor) == 5
            assert {"mu_sigma_head.mu_head.weight", "mu_sigma_head.mu_head.bias", "mu_sigma_head.sigma_head.weight",
                    "mu_sigma_head.sigma_head.bias", "mu_sigma_head.action_low", "mu_sigma_head.action_high"} <= keys
            assert "log_std" not in keys
            assert tuple(mod.mu_sigma_head.mu_head.weight.shape) == (3, 32)
            sd = mod.state_dict()
            assert sd["mu_sigma_head.action_low"].dtype == torch.float32
            assert sd["mu_sigma_head.action_low"].tolist() == [-1.0] * 3 and sd["mu_sigma_head.action_high"].tolist() == [1.0] * 3
        rc0 = make(_cfg(False))
        assert rc0.use_mu_sigma_head is False
        keys0 = set(AgentModule(13, 26, 3, rc0).state_dict())
        assert "log_std" in keys0 and not any(k.startswith("mu_sigma_head") for k in keys0)
        assert tuple(AgentModule(13, 26, 3, rc0).actor[4].weight.shape) == (3, 32)
    m = MultiAgentActorCritic(2, 13, 26, 3, _rc(_cfg(True)), shared=True)
    assert "policies.0.mu_sigma_head.sigma_head.weight" in m.state_dict() and m.log_std_table() is None


def test_modules_without_the_head_keep_their_seeded_initialisation():
    # the free-log_std module is built parameter for parameter as before: actor, critic, log_std
    from marlsc.ppo import AgentModule
    from marlsc.rollout import MLP
    rc = _rc(_cfg(False))
    torch.manual_seed(3)
    mod = AgentModule(13, 26, 3, rc)
    torch.manual_seed(3)
    actor = MLP(13, 3, rc.actor)
    critic = MLP(13 + 26, 1, rc.critic)  # mappo: the critic reads local || global
    assert list(mod.state_dict()) == ["log_std"] + [f"actor.{k}" for k in actor.state_dict()] + \
        [f"critic.{k}" for k in critic.state_dict()]
    for k, v in actor.state_dict().items():
        assert torch.equal(mod.state_dict()[f"actor.{k}"], v)
    for k, v in critic.state_dict().items():
        assert torch.equal(mod.state_dict()[f"critic.{k}"], v)
    assert torch.equal(mod.log_std.detach(), torch.full((3,), -1.0))


def test_schema_rules_raise():
    from marlsc.rollout import RolloutConfig
    a = {"hidden_sizes": [32], "activation": "relu"}
    bad = [
        _cfg(True, actor={**a, "output_activation": "tanh"}),          # output_activation with the head
        _cfg(False, actor={**a, "output_activation_mu": "tanh"}),      # head activations without the head
        _cfg(False, actor={**a, "output_activation_sigma": "tanh"}),
        _cfg(True, critic={**a, "output_activation_mu": "tanh"}),      # ... or on the critic
        _cfg(False, critic={**a, "output_activation_sigma": "tanh"}),
        _cfg(True, actor_type="gru"),                                  # the head needs an mlp actor
    ]
    for raw in bad:
        with pytest.raises(ValueError):
            _rc(raw)
        with pytest.raises(ValueError):
            RolloutConfig.from_algorithm_config(raw)
    with pytest.raises(ValueError):
        RolloutConfig(actor={**a, "output_activation_mu": "tanh"})
    _rc(_cfg(True, actor={**a, "output_activation_mu": "tanh", "output_activation_sigma": "sigmoid"}))
    _rc(_cfg(False, actor={**a, "output_activation": "tanh"}))


_FN = {None: lambda v: v, "tanh": torch.tanh, "bogus": torch.relu}


@pytest.mark.parametrize("act_mu,act_sigma", [(None, None), ("tanh", None), (None, "tanh"), ("bogus", "bogus")])
def test_dist_inputs_equal_the_reference_formula(act_mu, act_sigma):
    from marlsc.ppo import MultiAgentActorCritic
    actor = {"hidden_sizes": [32, 16], "activation": "relu"}
    if act_mu:
        actor["output_activation_mu"] = act_mu
    if act_sigma:
        actor["output_activation_sigma"] = act_sigma
    torch.manual_seed(0)
    m = MultiAgentActorCritic(3, 7, 21, 2, _rc(_cfg(True, actor=actor)), shared=True)
    p = m.policies[0]
    x = torch.randn(5, 3, 7) * 3
    with torch.no_grad():
        mu, ls = m.dist_inputs(x)
        # the formula of the issue / mu_sigma_head.py:52-82, written out
        f = F.linear(F.relu(F.linear(F.relu(F.linear(x, p.actor[0].weight, p.actor[0].bias)), p.actor[2].weight,
                                     p.actor[2].bias)), p.actor[4].weight, p.actor[4].bias)
        h = p.mu_sigma_head
        mu_ref = _FN[act_mu](F.linear(f, h.mu_head.weight, h.mu_head.bias))
        ls_ref = torch.clamp(_FN[act_sigma](F.linear(f, h.sigma_head.weight, h.sigma_head.bias)), -4.6, 4.6)
    assert mu.shape == ls.shape == (5, 3, 2)
    torch.testing.assert_close(mu, mu_ref, rtol=1e-6, atol=1e-6)
    torch.testing.assert_close(ls, ls_ref, rtol=1e-6, atol=1e-6)
    assert torch.equal(m.actor_mean(x), mu)


def test_log_std_clamps_at_exactly_4_6_and_mean_is_not_clamped():
    from marlsc.ppo import MultiAgentActorCritic
    torch.manual_seed(0)
    m = MultiAgentActorCritic(2, 7, 14, 2, _rc(_cfg(True)), shared=False)
    x = torch.randn(4, 2, 7)
    with torch.no_grad():
        for sign in (1.0, -1.0):
            for p in m.policies:
                p.mu_sigma_head.sigma_head.bias.fill_(10.0 * sign)
                p.mu_sigma_head.mu_head.bias.fill_(7.0)
            mu, ls = m.dist_inputs(x)
            assert torch.equal(ls, torch.full_like(ls, 4.6 * sign))
            assert float(mu.min()) > 1.0  # beyond the action bound: forward does not clamp the mean


def _batch(S=8, W=2, L=6, K=2, seed=0):
    g = torch.Generator().manual_seed(seed)
    return {"obs": torch.randn(S, W, L, generator=g), "actions": torch.randn(S, W, K, generator=g),
            "logp": -torch.rand(S, W, generator=g) - 1.0, "advantages": torch.randn(S, W, generator=g),
            "value_targets": torch.randn(S, W, generator=g)}


def _learner(sigma_bias=None, **over):
    from marlsc.ppo import MultiAgentActorCritic, PPOConfig, PPOLearner
    raw = _cfg(True, actor={"hidden_sizes": [32], "activation": "relu", "output_activation_mu": "tanh"})
    raw["algorithm"]["shared"].update({"batch_size": 16, "num_minibatches": 2, "num_epochs": 1, "learning_rate": 1e-2})
    raw["algorithm"]["algorithm_specific"].update(over)
    cfg = PPOConfig.from_algorithm_config(raw)
    torch.manual_seed(1)
    m = MultiAgentActorCritic(2, 6, 12, 2, cfg.rollout_config(), shared=True)
    if sigma_bias is not None:
        with torch.no_grad():
            m.policies[0].mu_sigma_head.sigma_head.bias.fill_(sigma_bias)
    return m, PPOLearner(m, cfg, seed=0)


def test_learner_step_trains_both_heads():
    m, learner = _learner(use_kl_loss=True)
    head = m.policies[0].mu_sigma_head
    before = copy.deepcopy(head.state_dict())
    batch = _batch()
    with torch.no_grad():
        batch["mean_old"], batch["log_std_old"] = m.dist_inputs(batch["obs"])
    out = learner.update(batch)
    for k in ("total_loss", "entropy", "mean_kl", "policy_loss", "vf_loss"):
        assert torch.isfinite(torch.tensor(out[k])), (k, out[k])
    after = head.state_dict()
    assert not torch.equal(before["mu_head.weight"], after["mu_head.weight"])
    assert not torch.equal(before["sigma_head.weight"], after["sigma_head.weight"])
    assert torch.equal(before["action_low"], after["action_low"])
    assert not any(n.endswith("log_std") for n, _ in m.named_parameters())


def test_saturated_clamp_gives_the_sigma_head_a_zero_gradient():
    from marlsc.ppo import ppo_loss
    m, learner = _learner(sigma_bias=10.0)
    batch = _batch()
    S, W = batch["obs"].shape[:2]
    rows = torch.arange(S * W)
    mean, log_std, values = learner._forward(m.policies[0], batch["obs"], rows)
    assert torch.equal(log_std, torch.full_like(log_std, 4.6))
    flat = {k: v.reshape(S * W, *v.shape[2:]) for k, v in batch.items() if k != "obs"}
    loss, _ = ppo_loss(learner.cfg, mean, log_std, values, flat, 0.0)
    loss.backward()
    head = m.policies[0].mu_sigma_head
    assert torch.count_nonzero(head.sigma_head.weight.grad) == 0 and torch.count_nonzero(head.sigma_head.bias.grad) == 0
    assert torch.count_nonzero(head.mu_head.weight.grad) > 0


@pytest.mark.parametrize("L,hidden,K", [(34, [256, 256], 5), (13, [64], 2)])
def test_fold_matches_the_layer_sequence(L, hidden, K):
    """W_eff = [W_mu; W_sigma] W_out and b_eff in f64, rounded once, applied in f32, against the
    torch layer sequence at the fused MLP's tolerance (2e-5 abs / rel)."""
    from marlsc.mlp import fold_head
    from marlsc.rollout import MLP, MuSigmaHead
    torch.manual_seed(5)
    H = hidden[-1]
    actor, head = MLP(L, H, {"hidden_sizes": hidden, "activation": "relu"}), MuSigmaHead(H, K)
    x = torch.randn(512, L)
    with torch.no_grad():
        mu, ls = head(actor(x))
        hid = x
        for mod in list(actor)[:-1]:
            hid = mod(hid)
        w, b = fold_head(actor[-1], head)
        assert w.shape == (2 * K, H) and b.shape == (2 * K,) and w.dtype == b.dtype == torch.float32
        d = F.linear(hid, w, b)
    torch.testing.assert_close(d[:, :K], mu, rtol=2e-5, atol=2e-5)
    torch.testing.assert_close(d[:, K:], ls, rtol=2e-5, atol=2e-5)


def test_layout_query_and_its_errors(monkeypatch):
    # host-only entry point (no HIP call): widths 2 / 4 / 5 / 8, 8 floats per (hidden pair, lane half)
    # up to 4 actions and 16 above; errors carry a message
    from marlsc import abi
    from marlsc.mlp import musigma_layout
    assert [musigma_layout(256, 256, k) for k in range(1, 9)] == \
        [(2, 8), (2, 8), (4, 8), (4, 8), (5, 16), (8, 16), (8, 16), (8, 16)]
    assert musigma_layout(96, 0, 8) == (8, 16) and musigma_layout(1024, 0, 4) == (4, 8)
    for bad in ((256, 256, 0), (256, 256, 9), (96, 96, 5), (100, 0, 5), (1024, 0, 5), (256, 0, -1)):
        assert musigma_layout(*bad) is None
        assert abi.lib().msc_last_error()
    monkeypatch.setenv("MSC_MLP_P8", "4")  # read at each call: a [256, 256] A/B form without a head variant
    assert musigma_layout(256, 256, 5) is None and musigma_layout(64, 64, 5) == (5, 16)


def test_forced_mfma_output_layer_cannot_host_the_head():
    # MSC_MLP_V3=0 (read once per process) forces the MFMA output layer, which cannot sample: the
    # layout query fails with a message and the host falls back to the torch layers
    import os
    import subprocess
    import sys
    from pathlib import Path
    code = ("from marlsc import abi, mlp\n"
            "from marlsc.rollout import MLP, MuSigmaHead\n"
            "assert mlp.musigma_layout(64, 64, 2) is None\n"
            "assert b'VALU' in abi.lib().msc_last_error()\n"
            "assert mlp.musigma_tier(list(MLP(13, 64, {'hidden_sizes': [64, 64]})), MuSigmaHead(64, 2)) == 3\n")
    env = dict(os.environ, MSC_MLP_V3="0", PYTHONPATH=str(Path(__file__).resolve().parents[1] / "marl-sc_amd"))
    r = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr


def test_tier_selection_needs_no_library_for_torch_paths():
    # non-ReLU backbones and heads over 16 actions run the torch layers (tier 3), 9..16 the folded
    # weights on the plain fused MLP (tier 2); neither asks the library for a layout
    from marlsc import mlp
    from marlsc.rollout import MLP, MuSigmaHead
    assert mlp.musigma_tier(list(MLP(34, 64, {"hidden_sizes": [64, 64], "activation": "tanh"})), MuSigmaHead(64, 5)) == 3
    assert mlp.musigma_tier(list(MLP(34, 64, {"hidden_sizes": [64, 64], "activation": "relu"})), MuSigmaHead(64, 17)) == 3
    assert mlp.musigma_tier(list(MLP(34, 64, {"hidden_sizes": [64, 64], "activation": "relu"})), MuSigmaHead(64, 9)) == 2
    assert mlp.musigma_tier(list(MLP(34, 48, {"hidden_sizes": [64, 48], "activation": "relu"})), MuSigmaHead(48, 9)) == 3
    assert isinstance(MuSigmaHead(8, 2, "gelu", "elu").mu_activation, nn.GELU)
