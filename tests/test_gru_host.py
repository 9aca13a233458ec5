"""Host tests of the GRU policy networks (marlsc/rollout.py GRUNet / PolicyNets, marlsc/ppo.py): the
reference's state-dict keys, the schema rules, stepping against nn.GRU over the sequence, resets
inside a chunk, and the learner's sequence minibatches. No GPU needed."""
import copy
from pathlib import Path

import pytest
import torch
import torch.nn as nn
import yaml

REPO = Path(__file__).resolve().parents[1]
GRU = {"num_layers": 2, "hidden_size": 32, "bidirectional": False, "output_dim": 24, "max_seq_len": 4}


def _cfg(shared=None, actor=None, critic=None, name="ippo", **spec):
    nets = {"shared_layers": shared, "use_mu_sigma_head": False,
            "actor": actor or {"type": "mlp", "config": {"hidden_sizes": [16], "activation": "relu"}},
            "critic": critic or {"type": "mlp", "config": {"hidden_sizes": [16], "activation": "relu"}}}
    sp = {"parameter_sharing": True, "logstd_init": -1.0, "logstd_floor": -3.5, "networks": nets}
    sp.update(spec)
    return {"algorithm": {"name": name, "shared": {"batch_size": 16, "num_minibatches": 2, "num_epochs": 1,
                                                   "learning_rate": 1e-2}, "algorithm_specific": sp}}


def _rc(raw):
    from marlsc.ppo import PPOConfig
    return PPOConfig.from_algorithm_config(raw).rollout_config()


def _keys(prefix, mod):
    return {f"{prefix}.{k}" for k in mod.state_dict()}


def test_ippo_gru_yaml_builds_the_reference_state_dict_keys():
    from marlsc.ppo import AgentModule
    from marlsc.rollout import ActorCritic, RolloutConfig
    raw = yaml.safe_load((REPO / "config_files" / "algorithms" / "ippo_gru.yaml").read_text())
    sl = raw["algorithm"]["algorithm_specific"]["networks"]["shared_layers"]
    assert sl == {"type": "gru", "config": {"num_layers": 2, "hidden_size": 128, "bidirectional": False,
                                            "output_dim": 128, "max_seq_len": 20}}
    want = (_keys("shared_layers.gru", nn.GRU(13, 128, 2, batch_first=True)) | _keys("shared_layers.output_proj", nn.Linear(128, 128))
            | _keys("actor.0", nn.Linear(128, 256)) | _keys("actor.2", nn.Linear(256, 3))
            | _keys("critic.0", nn.Linear(128, 256)) | _keys("critic.2", nn.Linear(256, 1)) | {"log_std"})
    for rc in (_rc(raw), RolloutConfig.from_algorithm_config(raw)):
        assert rc.max_seq_len == 20
        for mod in (AgentModule(13, 26, 3, rc), ActorCritic(13, 26, 3, rc)):
            assert set(mod.state_dict()) == want
            assert mod.actor[0].in_features == 128 and mod.critic[0].in_features == 128  # output_dim inputs
            assert tuple(mod.shared_layers["gru"].weight_ih_l0.shape) == (384, 13)


def test_activation_keys_and_gru_actor_critic_keys():
    from marlsc.ppo import AgentModule
    g = dict(GRU, activation="relu", output_activation="tanh")
    mod = AgentModule(13, 26, 3, _rc(_cfg(shared={"type": "gru", "config": g})))
    keys = set(mod.state_dict())
    assert {"shared_layers.output_proj.1.weight", "shared_layers.output_proj.1.bias"} <= keys
    assert not any(k.startswith("shared_layers.output_proj.0") or k == "shared_layers.output_proj.weight" for k in keys)
    assert isinstance(mod.shared_layers["output_proj"][0], nn.ReLU) and isinstance(mod.shared_layers["output_proj"][2], nn.Tanh)
    a = {k: v for k, v in GRU.items() if k != "output_dim"}
    raw = _cfg(actor={"type": "gru", "config": a}, critic={"type": "gru", "config": a}, name="mappo",
               critic_obs_type="global")
    mod = AgentModule(13, 26, 3, _rc(raw))
    want = (_keys("actor.gru", nn.GRU(13, 32, 2, batch_first=True)) | _keys("actor.output_proj", nn.Linear(32, 3))
            | _keys("critic.gru", nn.GRU(39, 32, 2, batch_first=True)) | _keys("critic.output_proj", nn.Linear(32, 1))
            | {"log_std"})
    assert set(mod.state_dict()) == want and mod.critic["gru"].input_size == 39
    assert set(mod.gru_slots()) == {"actor_h", "critic_h"}


def test_mlp_only_modules_keep_their_seeded_initialisation():
    from marlsc.ppo import AgentModule
    from marlsc.rollout import MLP
    rc = _rc(_cfg())
    torch.manual_seed(3)
    mod = AgentModule(13, 26, 3, rc)
    torch.manual_seed(3)
    actor, critic = MLP(13, 3, rc.actor), MLP(13, 1, rc.critic)
    assert torch.equal(mod.actor[0].weight, actor[0].weight) and torch.equal(mod.critic[2].weight, critic[2].weight)
    assert not mod.gru_slots()
    assert list(mod.state_dict()) == ["log_std"] + [f"{n}.{i}.{p}" for n in ("actor", "critic") for i in (0, 2)
                                                    for p in ("weight", "bias")]


def _bad(**kw):
    g = {k: v for k, v in GRU.items() if k != "output_dim"}
    cases = {
        "no_seq_len": _cfg(shared={"type": "gru", "config": {k: v for k, v in GRU.items() if k != "max_seq_len"}}),
        "no_seq_len_actor": _cfg(actor={"type": "gru", "config": {"hidden_size": 32}}),
        "two_seq_lens": _cfg(shared={"type": "gru", "config": GRU}, critic={"type": "gru", "config": dict(g, max_seq_len=8)}),
        "no_output_dim": _cfg(shared={"type": "gru", "config": g}),
        "obs_types": _cfg(shared={"type": "gru", "config": GRU}, name="mappo", critic_obs_type="global"),
        "bidirectional": _cfg(shared={"type": "gru", "config": dict(GRU, bidirectional=True)}),
        "dropout": _cfg(actor={"type": "gru", "config": dict(g, dropout=0.1)}),
        "mlp_shared": _cfg(shared={"type": "mlp", "config": {"hidden_sizes": [16], "output_dim": 8}}),
    }
    return cases


MESSAGES = {"no_seq_len": "max_seq_len is required", "no_seq_len_actor": "max_seq_len is required",
            "two_seq_lens": "share one max_seq_len", "no_output_dim": "output_dim is required",
            "obs_types": "actor_obs_type == critic_obs_type", "bidirectional": "bidirectional",
            "dropout": "dropout", "mlp_shared": "only gru shared layers"}


@pytest.mark.parametrize("case", sorted(MESSAGES))
def test_schema_rules_raise(case):
    from marlsc.rollout import RolloutConfig
    raw = _bad()[case]
    for make in (_rc, RolloutConfig.from_algorithm_config):
        with pytest.raises(ValueError, match=MESSAGES[case]):
            make(raw)


def test_minibatch_must_hold_a_sequence_and_valid_configs_pass():
    raw = _cfg(shared={"type": "gru", "config": dict(GRU, max_seq_len=9)})  # 16 // 2 = 8 < 9
    with pytest.raises(ValueError, match="must be >= max_seq_len"):
        _rc(raw)
    rc = _rc(_cfg(shared={"type": "gru", "config": GRU}))
    assert rc.max_seq_len == 4 and rc.shared_layers["output_dim"] == 24 and rc.actor_type == "mlp"
    assert _rc(_cfg()).max_seq_len is None
    head = _cfg(shared={"type": "gru", "config": GRU})
    head["algorithm"]["algorithm_specific"]["networks"]["use_mu_sigma_head"] = True
    assert _rc(head).use_mu_sigma_head  # the head works on an mlp actor over the trunk
    a = {k: v for k, v in GRU.items() if k != "output_dim"}
    head["algorithm"]["algorithm_specific"]["networks"]["actor"] = {"type": "gru", "config": a}
    with pytest.raises(ValueError, match="use_mu_sigma_head is not supported with actor type"):
        _rc(head)


def _net(**over):
    from marlsc.rollout import GRUNet
    torch.manual_seed(5)
    return GRUNet(6, 3, dict({"hidden_size": 32, "num_layers": 2, "max_seq_len": 4}, **over))


def test_seven_steps_from_zero_equal_nn_gru_over_the_sequence():
    # values bounded by 1, a few f32 roundings apart: 1e-6 absolute
    net = _net()
    x = torch.randn(5, 7, 6)
    with torch.no_grad():
        o, hn = net["gru"](x)
        want = net["output_proj"](o)
        h = net.zero_state(5)
        assert h.shape == (5, 2, 32) and not h.any()
        for s in range(7):
            y, h = net.step(x[:, s], h)
            assert float((y - want[:, s]).abs().max()) <= 1e-6
        assert float((h - hn.transpose(0, 1)).abs().max()) <= 1e-6
        ys, hs = net.sequence(x, net.zero_state(5))
        yk, hk = net.sequence(x, net.zero_state(5), torch.ones(5, 7))
    assert float((ys - want).abs().max()) <= 1e-6 and float((yk - want).abs().max()) <= 1e-6
    assert float((hk - hs).abs().max()) <= 1e-6


@torch.no_grad()
def test_a_reset_inside_the_chunk_equals_two_separate_runs():
    net = _net(activation="tanh")
    x, h0 = torch.randn(4, 7, 6), torch.rand(4, 2, 32) * 2 - 1
    keep = torch.ones(4, 7)
    keep[1, 3] = keep[2, 3] = 0.0  # rows 1 and 2 start a new episode at step 3
    with torch.no_grad():
        y, _ = net.sequence(x, h0, keep)
        g, proj = net["gru"], net["output_proj"]
        a, _ = g(x[:, :3], h0.transpose(0, 1).contiguous())
        b_cont, _ = g(x, h0.transpose(0, 1).contiguous())
        b_zero, _ = g(x[:, 3:])  # from zero
        # the step with the reset flag: the same rows through GRUNet.step
        hs = h0
        for s in range(7):
            ystep, hs = net.step(x[:, s], hs, reset=(keep[:, s] == 0).to(torch.uint8), group=1)
            assert float((ystep - y[:, s]).abs().max()) <= 1e-6
    for r in (1, 2):
        assert float((y[r, :3] - proj(a)[r]).abs().max()) <= 1e-6
        assert float((y[r, 3:] - proj(b_zero)[r]).abs().max()) <= 1e-6
    for r in (0, 3):
        assert float((y[r] - proj(b_cont)[r]).abs().max()) <= 1e-6


def test_initial_state_and_recurrent_step_shapes():
    from marlsc.ppo import MultiAgentActorCritic
    for shared in (True, False):
        torch.manual_seed(0)
        m = MultiAgentActorCritic(2, 6, 12, 3, _rc(_cfg(shared={"type": "gru", "config": GRU})), shared=shared)
        assert m.recurrent and m.max_seq_len == 4
        st = m.initial_state(5)
        assert set(st) == {"shared_h"} and st["shared_h"].shape == (5, 2, 2, 32) and not st["shared_h"].any()
        obs = torch.randn(5, 2, 6)
        with torch.no_grad():
            a_in, mean, v, new = m.step(obs, None, st)
            reset = torch.tensor([0, 1, 0, 0, 1], dtype=torch.uint8)
            _, _, v2, new2 = m.step(obs, None, new, reset)
            _, _, v3, none = m.step(obs, None, new, reset, store=False, actor=False)
        assert a_in.shape == (5, 2, 24) and mean is None and v.shape == (5, 2) and new["shared_h"].shape == (5, 2, 2, 32)
        assert torch.allclose(new2["shared_h"][1], new["shared_h"][1], atol=1e-6)  # reset rows: from zero again
        assert not torch.allclose(new2["shared_h"][0], new["shared_h"][0])
        assert torch.equal(v2, v3) and none["shared_h"] is None
    assert not MultiAgentActorCritic(2, 6, 12, 3, _rc(_cfg()), shared=True).recurrent


E, W, T, S, L, K = 4, 2, 8, 4, 6, 2


def _learner(shared=True, trunc_at=None, **spec):
    from marlsc.ppo import MultiAgentActorCritic, PPOConfig, PPOLearner
    cfg = PPOConfig.from_algorithm_config(_cfg(shared={"type": "gru", "config": GRU}, **spec))
    torch.manual_seed(1)
    m = MultiAgentActorCritic(W, L, L * W, K, cfg.rollout_config(), shared=shared)
    g = torch.Generator().manual_seed(0)
    trunc = torch.zeros(T, E, W, dtype=torch.uint8)
    if trunc_at is not None:
        trunc[trunc_at] = 1
    batch = {"obs": torch.randn(T * E, W, L, generator=g), "actions": torch.randn(T * E, W, K, generator=g),
             "logp": -torch.rand(T * E, W, generator=g) - 1.0, "advantages": torch.randn(T * E, W, generator=g),
             "value_targets": torch.randn(T * E, W, generator=g),
             "seq": {"T": T, "E": E, "S": S, "truncated": trunc,
                     "state_in": {"shared_h": (torch.rand(T // S, E, W, 2, 32, generator=g) * 2 - 1).requires_grad_()}}}
    return m, PPOLearner(m, cfg, seed=0), batch, cfg


@pytest.mark.parametrize("shared", [True, False])
def test_learner_update_trains_the_gru_on_sequence_minibatches(shared):
    from marlsc.ppo import minibatch_rows
    m, learner, batch, cfg = _learner(shared, trunc_at=(1, 2), use_kl_loss=True)
    before = copy.deepcopy(m.policies[0].shared_layers["gru"].weight_hh_l0.detach())
    out = learner.update(batch)
    for k in ("total_loss", "entropy", "mean_kl", "policy_loss", "vf_loss"):
        assert torch.isfinite(torch.tensor(out[k])), (k, out[k])
    assert not torch.equal(before, m.policies[0].shared_layers["gru"].weight_hh_l0)
    assert minibatch_rows(cfg) == 8
    assert learner.last_minibatch_sizes == [8 // S] * len(m.policies)  # sequences, not rows
    assert batch["seq"]["state_in"]["shared_h"].grad is None


def test_sequence_gradient_matches_autograd_through_whole_sequence_nn_gru():
    from marlsc.ppo import ppo_loss
    m, learner, batch, cfg = _learner()
    pol = m.policies[0]
    ids = torch.tensor([3, 9, 14])  # (chunk, env, agent) = (0, 1, 1), (1, 0, 1), (1, 3, 0)
    flat = {k: v.reshape(T * E * W, *v.shape[2:]) for k, v in batch.items() if k not in ("obs", "seq")}
    mean, log_std, values, rows = learner._seq_forward(pol, batch["obs"], batch["seq"], ids)
    loss, _ = ppo_loss(cfg, mean, log_std, values, {k: v[rows] for k, v in flat.items()}, 0.0)
    got = torch.autograd.grad(loss, list(pol.parameters()), allow_unused=True)
    assert batch["seq"]["state_in"]["shared_h"].grad is None
    # the same loss assembled by hand: whole-sequence nn.GRU per sequence, rows in (sequence, step) order
    obs = batch["obs"].reshape(T, E, W, L)
    means, vals, rws = [], [], []
    for c, e, w in [(0, 1, 1), (1, 0, 1), (1, 3, 0)]:
        x = obs[c * S:(c + 1) * S, e, w].unsqueeze(0)
        h0 = batch["seq"]["state_in"]["shared_h"][c, e, w].detach().unsqueeze(1)
        o, _ = pol.shared_layers["gru"](x, h0)
        f = pol.shared_layers["output_proj"](o[0])
        means.append(pol.actor(f))
        vals.append(pol.critic(f).squeeze(-1))
        rws += [((c * S + s) * E + e) * W + w for s in range(S)]
    assert rows.tolist() == rws
    mean2 = torch.cat(means)
    ls2 = torch.clamp(pol.log_std, min=m.rc.logstd_floor).expand_as(mean2)
    loss2, _ = ppo_loss(cfg, mean2, ls2, torch.cat(vals), {k: v[rows] for k, v in flat.items()}, 0.0)
    want = torch.autograd.grad(loss2, list(pol.parameters()), allow_unused=True)
    assert abs(float(loss.detach()) - float(loss2.detach())) <= 1e-6
    names = [n for n, _ in pol.named_parameters()]
    for n, a, b in zip(names, got, want):
        assert (a is None) == (b is None), n
        if a is not None:
            torch.testing.assert_close(a, b, rtol=1e-5, atol=1e-7, msg=n)
    assert got[names.index("shared_layers.gru.weight_hh_l0")].abs().max() > 0


def test_gradient_through_a_reset_matches_two_nn_gru_segments():
    # the stepped path training takes at episode boundaries: env 2 is truncated at step 1, so its chunk 0
    # enters step 2 from zero; the reference runs nn.GRU over steps 0-1 from state_in and over 2-3 from zero
    from marlsc.ppo import ppo_loss
    m, learner, batch, cfg = _learner(trunc_at=(1, 2))
    pol = m.policies[0]
    ids = torch.tensor([4, 5])  # (chunk 0, env 2, agents 0 and 1)
    flat = {k: v.reshape(T * E * W, *v.shape[2:]) for k, v in batch.items() if k not in ("obs", "seq")}
    mean, log_std, values, rows = learner._seq_forward(pol, batch["obs"], batch["seq"], ids)
    loss, _ = ppo_loss(cfg, mean, log_std, values, {k: v[rows] for k, v in flat.items()}, 0.0)
    got = torch.autograd.grad(loss, list(pol.parameters()), allow_unused=True)
    obs = batch["obs"].reshape(T, E, W, L)
    gru, proj = pol.shared_layers["gru"], pol.shared_layers["output_proj"]
    feats = []
    for w in (0, 1):
        h0 = batch["seq"]["state_in"]["shared_h"][0, 2, w].detach().unsqueeze(1)
        a, _ = gru(obs[0:2, 2, w].unsqueeze(0), h0)
        b, _ = gru(obs[2:4, 2, w].unsqueeze(0))
        feats.append(proj(torch.cat([a[0], b[0]])))
    f = torch.cat(feats)
    mean2 = pol.actor(f)
    ls2 = torch.clamp(pol.log_std, min=m.rc.logstd_floor).expand_as(mean2)
    loss2, _ = ppo_loss(cfg, mean2, ls2, pol.critic(f).squeeze(-1), {k: v[rows] for k, v in flat.items()}, 0.0)
    want = torch.autograd.grad(loss2, list(pol.parameters()), allow_unused=True)
    assert abs(float(loss.detach()) - float(loss2.detach())) <= 1e-6
    for (n, _), a, b in zip(pol.named_parameters(), got, want):
        assert (a is None) == (b is None), n
        if a is not None:
            torch.testing.assert_close(a, b, rtol=1e-5, atol=1e-7, msg=n)
    # and it differs from the forward that ignores the reset
    batch["seq"]["truncated"].zero_()
    mean3, _, _, _ = learner._seq_forward(pol, batch["obs"], batch["seq"], ids)
    assert not torch.allclose(mean3, mean, atol=1e-4)


def test_rollout_length_must_be_whole_chunks():
    m, learner, batch, _ = _learner()
    bad = dict(batch)
    bad["seq"] = dict(batch["seq"], T=6, E=E)
    bad["obs"] = batch["obs"][:6 * E]
    with pytest.raises(ValueError, match="multiple of max_seq_len"):
        learner.update(bad)
