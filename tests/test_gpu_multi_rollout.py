"""GPU tests of per-agent policies through the multi-policy MLP kernel (MultiAgentActorCritic(multi_mlp=True),
marlsc/ppo.py -> mlp.multi_forward -> msc_mlp{2,3}_relu_multi): the module's entry points, a rollout of
the collector, and one training iteration with a checkpoint round trip. The kernel itself is pinned in
tests/test_gpu_mlp_multi_exact.py; here the sampled actions are compared on bits with the single-policy
fused actor per policy, and the means / values with the switch-off torch path at the tolerance
tests/test_gpu_rollout.py uses for fused-versus-torch layers (rtol = atol = 2e-5)."""
import copy
from pathlib import Path

import pytest
import torch
import yaml

pytestmark = pytest.mark.gpu
REPO = Path(__file__).resolve().parents[1]
TOL = dict(rtol=2e-5, atol=2e-5)
STYLES = {
    "ippo": dict(actor={"hidden_sizes": [64]}, critic={"hidden_sizes": [64]}, critic_obs_type="local"),
    "mappo": dict(actor={"hidden_sizes": [64, 64]}, critic={"hidden_sizes": [64, 64]}, critic_obs_type="global"),
}


def _env(W, E, ep_len=20, seed=77):
    from marlsc import make_synthetic_env_config
    from marlsc.spec import EnvSpec
    from marlsc.vec_env import VecInventoryEnv
    cfg = make_synthetic_env_config(W, 4, 2, episode_length=ep_len)
    spec = EnvSpec.from_config(cfg, {"include_warehouse_id": False})  # one policy per agent: no id feature
    env = VecInventoryEnv(None, E, spec=spec, device=0, base_seed=seed)
    return spec, env, env.reset()


def _module(env, style, multi, seed=0):
    from marlsc.ppo import MultiAgentActorCritic
    from marlsc.rollout import RolloutConfig
    torch.manual_seed(seed)
    m = MultiAgentActorCritic(env.W, env.local_obs_dim, env.local_obs_dim * env.W, env.K, RolloutConfig(**STYLES[style]),
                              False, multi_mlp=multi).cuda()
    with torch.no_grad():  # distinct log_std rows per agent
        for w, p in enumerate(m.policies):
            p.log_std.add_(0.1 * w - 0.05)
    return m


def _spy(monkeypatch):
    from marlsc import mlp as M
    calls, real = [], M.multi_forward

    def spy(*a, **k):
        calls.append(k.get("sample") is not None)
        return real(*a, **k)
    monkeypatch.setattr(M, "multi_forward", spy)
    return calls


@pytest.mark.parametrize("style", ["ippo", "mappo"])
@pytest.mark.parametrize("W", [2, 3])
def test_module_entry_points_run_one_launch_and_match_the_per_policy_paths(monkeypatch, W, style):
    from marlsc.rollout import fused_actor_sample
    E = 37
    spec, env, obs = _env(W, E)
    m = _module(env, style, True)
    K = env.K
    g = torch.Generator(device="cuda").manual_seed(W)
    obs = (obs + 0.25 * torch.randn(obs.shape, device="cuda", generator=g)).contiguous()
    eps = torch.randn((E, W, K), device="cuda", generator=g)
    ls, floor = m.log_std_table(), m.rc.logstd_floor
    assert ls.shape == (W, K)
    calls = _spy(monkeypatch)
    with torch.no_grad():
        act, logp, clip = torch.empty((E, W, K), device="cuda"), torch.empty((E, W), device="cuda"), torch.empty((E, W, K), device="cuda")
        assert m.actor_sample(obs, None, (ls, floor, eps, act, logp, clip)) is True
        assert calls == [True]  # one launch for W actors and their sampling
        v_on = m.values(obs, None)
        assert calls == [True, False]  # and one for W critics
        mean_on = m.actor_mean(obs, None)
        assert len(calls) == 3 and v_on.shape == (E, W) and mean_on.shape == (E, W, K)
        # the sampled actions: bit-identical to the single-policy fused actor on each policy's rows
        for w, p in enumerate(m.policies):
            a1, l1, c1 = torch.empty((E, K), device="cuda"), torch.empty((E,), device="cuda"), torch.empty((E, K), device="cuda")
            assert fused_actor_sample(p.actor, obs[:, w].contiguous(),
                                      (ls[w:w + 1].contiguous(), floor, eps[:, w].contiguous(), a1, l1, c1))
            assert torch.equal(act[:, w], a1) and torch.equal(logp[:, w], l1) and torch.equal(clip[:, w], c1)
        # the switch-off torch path on the same module
        m.multi_mlp = False
        assert m.actor_sample(obs, None, (ls, floor, eps, act.clone(), logp.clone(), clip.clone())) is False
        v_off, mean_off = m.values(obs, None), m.actor_mean(obs, None)
        assert len(calls) == 3
    torch.testing.assert_close(mean_on, mean_off, **TOL)
    torch.testing.assert_close(v_on, v_off, **TOL)
    if style == "mappo":  # the split first layer of the global critic against float64 torch layers
        L = env.local_obs_dim
        glob = obs.reshape(E, 1, W * L).expand(E, W, W * L)
        full = torch.cat([obs, glob], dim=-1).double()
        with torch.no_grad():
            ref = torch.stack([copy.deepcopy(p.critic).double()(full[:, w]).squeeze(-1) for w, p in enumerate(m.policies)], dim=-1)
        e_on, e_off = (v_on.double() - ref).abs().max().item(), (v_off.double() - ref).abs().max().item()
        print(f"global critic W={W}: multi kernel max err {e_on:.3e}, float32 torch path {e_off:.3e}, ratio {e_on / e_off:.2f}")
        torch.testing.assert_close(v_on.double(), ref, **TOL)


def _collector(style, multi, T=6, E=37, ep_len=3):
    from marlsc.rollout import RolloutCollector
    spec, env, _ = _env(2, E, ep_len=ep_len)
    m = _module(env, style, multi)
    return spec, env, m, RolloutCollector(env, m, T, seed=3, adv_groups=env.W)


@pytest.mark.parametrize("style", ["ippo", "mappo"])
def test_collector_with_per_agent_policies_replays_and_matches_the_torch_path(monkeypatch, style):
    from marlsc.vec_env import VecInventoryEnv
    calls = _spy(monkeypatch)
    spec, env, m, col = _collector(style, True)
    col.collect()
    torch.cuda.synchronize()
    T = col.T
    assert calls.count(True) == T and calls.count(False) >= T + 1  # actor per step; critic per step, bootstraps, last
    assert bool(col.truncated.any())  # episodes of 3 steps: truncation bootstraps inside the rollout
    assert bool((col.next_values[col.truncated.bool()] != 0).any())
    # the env consumed exactly the clipped sampled actions
    env2 = VecInventoryEnv(None, col.E, spec=spec, device=0, base_seed=77)
    obs = env2.reset()
    for t in range(T):
        assert torch.equal(obs, col.obs[t])
        obs, rew, trunc, _ = env2.step(col.actions[t].clamp(-1.0, 1.0).contiguous())
        assert torch.equal(rew, col.rewards[t])
    # step 0 of a switch-off collector with the same seeds: same observations, eps and log_std
    n = len(calls)
    _, _, m0, col0 = _collector(style, False)
    for a, b in zip(m.parameters(), m0.parameters()):
        assert torch.equal(a, b)
    col0.collect()
    torch.cuda.synchronize()
    assert len(calls) == n
    assert torch.equal(col.obs[0], col0.obs[0])
    torch.testing.assert_close(col.values[0], col0.values[0], rtol=2e-5, atol=2e-5)
    torch.testing.assert_close(col.actions[0], col0.actions[0], rtol=1e-5, atol=1e-5)


def test_trainer_iteration_evaluation_and_checkpoint_round_trip(tmp_path, monkeypatch):
    from marlsc import make_synthetic_env_config
    from marlsc.ppo import PPOConfig, PPOTrainer
    raw = yaml.safe_load(open(REPO / "config_files/algorithms/ippo.yaml"))
    raw["algorithm"]["algorithm_specific"].update({"parameter_sharing": False})
    raw["algorithm"]["shared"].update(dict(num_epochs=1, num_minibatches=2, num_eval_episodes=2))
    cfg = PPOConfig.from_algorithm_config(raw)
    env_cfg = make_synthetic_env_config(2, 4, 2, episode_length=5)
    kw = dict(root_seed=7, n_envs=32, rollout_len=8, device=0)
    calls = _spy(monkeypatch)
    tr = PPOTrainer(env_cfg, cfg, multi_mlp=True, **kw)
    assert tr.module.multi_mlp is True and not tr.module.shared
    res = tr.train_iteration()
    assert calls.count(True) == 8  # the rollout's actor steps went through the kernel
    assert all(v == v for v in res.values() if isinstance(v, float))  # no NaN
    n = len(calls)
    ev = tr.evaluate()
    assert len(calls) > n  # evaluation's mean actions too
    ck = tr.save_checkpoint(tmp_path / "ck")
    tr2 = PPOTrainer(env_cfg, cfg, multi_mlp=True, **kw)
    tr2.load_checkpoint(ck)
    assert tr2.iteration == 1 and tr2.timesteps == tr.timesteps
    for a, b in zip(tr.module.state_dict().values(), tr2.module.state_dict().values()):
        assert torch.equal(a, b)
    assert tr2.evaluate() == ev
    off = PPOTrainer(env_cfg, cfg, multi_mlp=False, **kw)
    assert off.module.multi_mlp is False
    assert list(off.module.state_dict().keys()) == list(tr.module.state_dict().keys())  # no new parameters
