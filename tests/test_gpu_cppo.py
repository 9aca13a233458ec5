"""GPU tests of centralised PPO (marlsc/cppo.py): the rollout adapter against VecCentralizedEnv (itself
pinned to the oracle, tests/test_gpu_centralized.py), the collector against its own kernels and a second
env, two trainer iterations with a checkpoint round trip, and the run script with cppo.yaml.
A synthetic 8 x 64 x 5 env: the actor has 40 outputs (the wide fused kernel). E = 64, T = 8.
The learner is parity unpinned against RLlib, as for IPPO / MAPPO."""
import json
from pathlib import Path

import numpy as np
import pytest
import torch
import yaml

pytestmark = pytest.mark.gpu
REPO = Path(__file__).resolve().parents[1]
E, T = 64, 8


def _env_cfg(episode_length=6):
    from marlsc import make_synthetic_env_config
    return make_synthetic_env_config(8, 64, 5, episode_length=episode_length)


def _algo(**specific):
    from marlsc.cppo import CPPOConfig
    raw = yaml.safe_load(open(REPO / "config_files/algorithms/cppo.yaml"))
    raw["algorithm"]["algorithm_specific"].update(specific)
    raw["algorithm"]["shared"].update(num_epochs=2, num_minibatches=2, num_eval_episodes=4)
    return CPPOConfig.from_algorithm_config(raw)


def _trainer(cfg=None, **specific):
    from marlsc.cppo import CPPOTrainer
    cfg = cfg or _algo(**specific)
    return CPPOTrainer(_env_cfg(), cfg, root_seed=7, n_envs=E, rollout_len=T, device=0), cfg


def _bits(t):
    return t.detach().cpu().contiguous().numpy().view(np.uint32)


def test_adapter_matches_vec_centralized_env():
    from marlsc import CentralizedRolloutEnv, VecCentralizedEnv
    from marlsc.spec import EnvSpec
    from marlsc.vec_env import VecInventoryEnv
    spec = EnvSpec.from_config(_env_cfg(), {"include_warehouse_id": False})
    ref = VecCentralizedEnv(VecInventoryEnv(None, E, spec=spec, device=0, base_seed=31))
    env = CentralizedRolloutEnv(VecInventoryEnv(None, E, spec=spec, device=0, base_seed=31))
    W, K, L = 8, 5, ref.L
    assert (env.W, env.K, env.L, env.local_obs_dim, env.n_envs) == (1, W * K, W * L, W * L, E)
    assert env.spec is spec and env.device == ref.venv.device
    g = ref.reset()
    o = env.reset()
    assert o.shape == (E, 1, W * L) and o.data_ptr() == env.venv.obs.data_ptr()  # a view: no copy
    assert torch.equal(o[:, 0], g)
    rng = np.random.default_rng(3)
    obs_rows = torch.full((3, E, 1, W * L), 7.25, device="cuda")
    rew_rows = torch.full((3, E, 1), 7.25, device="cuda")
    tr_rows = torch.zeros((3, E), dtype=torch.uint8, device="cuda")
    ended = 0
    for t in range(14):  # crosses two episode ends
        a = torch.from_numpy(rng.uniform(-1.5, 1.5, size=(E, W * K)).astype(np.float32)).cuda().clamp(-1, 1)
        may = env.may_truncate()
        assert may == ref.venv.may_truncate()
        g, r64, tr, fin = ref.step(a)
        i = t % 3
        o, r, tr2, fin2 = env.step(a.view(E, 1, W * K), obs_out=obs_rows[i], rewards_out=rew_rows[i], truncated_out=tr_rows[i])
        assert o.data_ptr() == obs_rows[i].data_ptr() and r.data_ptr() == rew_rows[i].data_ptr()
        assert torch.equal(o[:, 0], g) and torch.equal(tr2, tr)
        assert np.array_equal(_bits(r[:, 0]), _bits(r64.float()))  # the f32 of the f64 totals
        assert torch.equal(env.rewards_f64, r64)
        if bool(tr.any()):
            ended += 1
            assert may and torch.equal(fin2[:, 0][tr.bool()], fin[tr.bool()])
    assert ended == 2
    # without output rows the adapter's own buffers are written
    a = torch.zeros((E, 1, W * K), device="cuda")
    g, r64, _, _ = ref.step(a[:, 0])
    o, r, _, _ = env.step(a)
    assert o.data_ptr() == env.obs.data_ptr() and torch.equal(o[:, 0], g) and torch.equal(r[:, 0], r64.float())


def _replay(tr, clipped):
    """(obs [T + 1, E, 1, WL], rewards [T, E, 1]) of a second env of the trainer's spec and seeds stepped
    with the clipped actions [T, E, 1, WK]."""
    from marlsc import CentralizedRolloutEnv
    from marlsc.vec_env import VecInventoryEnv
    env = CentralizedRolloutEnv(VecInventoryEnv(None, E, spec=tr.spec, device=0, base_seed=tr.train_seed))
    obs = [env.reset().clone()]
    rew = []
    for t in range(T):
        o, r, _, _ = env.step(clipped[t])
        obs.append(o.clone())
        rew.append(r.clone())
    env.close()
    return torch.stack(obs), torch.stack(rew)


def test_collector_is_consistent_with_its_kernels_and_a_second_env(monkeypatch):
    from marlsc import mlp as M
    from marlsc.rollout import keyed_normal
    monkeypatch.setattr(M, "WIDE_ENABLED", True)  # the wide kernel is opt-in at rollout (MSC_WIDE_MLP=1)
    tr, cfg = _trainer(obs_normalization="off")
    col = tr.collector
    assert (col.E, col.N, col.adv_groups) == (E, E, 1) and col.actions.shape == (T, E, 1, 40)
    mods = list(tr.module.policies[0].actor)
    assert M.wide_layers(mods) == 2
    out = col.collect(normalize=False)
    obs_all = col._obs_all.clone()
    eps = keyed_normal((T, E, 1, 40), tr.env.env_index_offset, tr.train_seed + 1000, 0)  # keyed by global env id
    ls = tr.module.log_std_table()
    clipped = torch.empty_like(out["actions"])
    with torch.no_grad():
        for t in range(T):
            act, logp = torch.empty((E, 40), device="cuda"), torch.empty((E,), device="cuda")
            M.wide_forward(mods, obs_all[t].reshape(E, -1), None,
                           sample=(ls, cfg.logstd_floor, eps[t].reshape(E, 40).contiguous(), act, logp,
                                   clipped[t].view(E, 40)))
            assert np.array_equal(_bits(act), _bits(out["actions"][t, :, 0]))
            assert np.array_equal(_bits(logp), _bits(out["logp"][t, :, 0]))
    # the clip the env received is the clip of the stored actions
    assert np.array_equal(_bits(clipped), _bits(out["actions"].clamp(-1.0, 1.0)))
    obs2, rew2 = _replay(tr, clipped)
    assert torch.equal(obs2, obs_all) and torch.equal(rew2, out["rewards"])
    assert bool(col.truncated.any())  # an episode ended inside the rollout (episode length 6 < T)


def test_collector_runs_on_the_torch_tier_with_the_fused_mlp_off(monkeypatch):
    from marlsc import mlp as M
    monkeypatch.setattr(M, "ENABLED", False)
    monkeypatch.setattr(M, "WIDE_ENABLED", True)  # MSC_FUSED_MLP3=0 wins over the wide kernel's opt-in
    tr, cfg = _trainer(obs_normalization="off")
    out = tr.collector.collect(normalize=False)
    assert bool(torch.isfinite(out["actions"]).all()) and bool(torch.isfinite(out["logp"]).all())
    obs2, rew2 = _replay(tr, out["actions"].clamp(-1.0, 1.0))
    assert torch.equal(obs2, tr.collector._obs_all) and torch.equal(rew2, out["rewards"])


def _mean_tolerance(module, x):
    """8 x the larger error of two CPU float32 evaluations of the actor against float64 on inputs x
    (the real-weights tolerance of tests/test_gpu_mlp_wide.py), and the float64 means."""
    from mlp_ref import f32_chain_forward, f32_matmul_forward, f64_forward
    lins = [m for m in module.policies[0].actor if isinstance(m, torch.nn.Linear)]
    W = [m.weight.detach().cpu().numpy() for m in lins]
    b = [m.bias.detach().cpu().numpy() for m in lins]
    ref = f64_forward(x, W, b)
    return 8.0 * max(np.abs(f(x, W, b) - ref).max() for f in (f32_chain_forward, f32_matmul_forward)), ref


@pytest.mark.parametrize("wide", [True, False], ids=["wide", "torch"])
def test_two_iterations_evaluation_and_checkpoint_round_trip(tmp_path, monkeypatch, wide):
    from marlsc import mlp as M
    from marlsc.cppo import CPPOTrainer
    monkeypatch.setattr(M, "WIDE_ENABLED", wide)  # MSC_WIDE_MLP=1 / the default route
    tr, cfg = _trainer()
    assert tr.spec.include_warehouse_id is False and tr.env.L == 8 * tr.env.venv.L
    p0 = [p.detach().clone() for p in tr.module.parameters()]
    x = tr.collector.obs  # (filled by the first collect)
    mods = list(tr.module.policies[0].actor)
    for _ in range(2):
        res = tr.train_iteration()
        assert all(np.isfinite(v) for k, v in res.items() if k.startswith("learner/"))
    assert res["num_env_steps_sampled_lifetime"] == 2 * T * E
    assert any(not torch.equal(a, b) for a, b in zip(p0, tr.module.parameters()))
    assert not torch.equal(p0[[n for n, _ in tr.module.named_parameters()].index('policies.0.actor.2.weight')], mods[-1].weight)
    # the packs were rebuilt after the optimizer steps: fused means = torch means on the new weights
    xs = x[:2].reshape(-1, x.shape[-1]).contiguous()
    tol, ref = _mean_tolerance(tr.module, xs.cpu().numpy())
    with torch.no_grad():
        fused = M.wide_forward(mods, xs)
    with torch.enable_grad():  # (autograd on: the torch layers)
        plain = tr.module.policies[0].actor(xs).detach()
    print(f"after the update: |fused - torch| {float((fused - plain).abs().max()):.3e}, "
          f"|fused - f64| {np.abs(fused.cpu().numpy() - ref).max():.3e}, tolerance {tol:.3e}")
    assert float((fused - plain).abs().max()) <= tol and np.abs(fused.cpu().numpy() - ref).max() <= tol
    ev = tr.evaluate()
    assert ev["eval/episodes"] == 4 and np.isfinite(ev["eval/episode_return_mean"])
    assert tr.evaluate() == ev
    ck = tr.save_checkpoint(tmp_path / "ck")
    tr.export_module_weights(tmp_path / "module_weights.pt")
    sd = torch.load(tmp_path / "module_weights.pt", weights_only=True)
    assert {"log_std", "actor.0.weight", "critic.0.weight"} <= set(sd) and sd["actor.2.weight"].shape == (40, 256)
    assert json.loads((ck / "state.json").read_text())["algorithm"]["name"] == "cppo"
    res_a = tr.train_iteration()
    tr2 = CPPOTrainer(_env_cfg(), cfg, root_seed=7, n_envs=E, rollout_len=T, device=0)
    tr2.load_checkpoint(ck)
    assert tr2.iteration == 2 and tr2.evaluate() == ev
    res_b = tr2.train_iteration()
    assert torch.equal(tr.collector.obs, tr2.collector.obs) and torch.equal(tr.collector.actions, tr2.collector.actions)
    sa, sb = tr.env.read_state(), tr2.env.read_state()
    for k in ("inventory", "timestep", "episode_counter", "rng"):
        np.testing.assert_array_equal(sa[k], sb[k])
    assert res_a == res_b  # one block of 64 sequences in the GAE statistics: no atomics order to differ in


def test_run_experiment_script_with_cppo(tmp_path):
    # c1 has 2 x 2 = 4 joint actions: the narrow fused kernels serve the centralised actor there
    import os
    import subprocess
    env = dict(os.environ, ENV_CONFIG="./config_files/environments/env_c1_2wh4r2sku.yaml",
               ALGO_CONFIG="./config_files/algorithms/cppo.yaml", STORAGE_DIR=str(tmp_path), EXPERIMENT_NAME="CP",
               ROOT_SEED="42", EVAL_EPISODES="2", NGPUS="1",
               EXTRA_ARGS="--num-iterations 2 --envs 16 --rollout-len 4")
    r = subprocess.run(["bash", str(REPO / "scripts" / "run_experiment.sh")], env=env, cwd=str(tmp_path),
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    out = tmp_path / "CP"
    lines = (out / "training_metrics.jsonl").read_text().strip().splitlines()
    assert len(lines) == 2 and json.loads(lines[-1])["training_iteration"] == 2
    assert json.loads((out / "metadata.json").read_text())["algorithm"] == "cppo"
    assert (out / "checkpoint_final" / "learner_state.pt").exists()
    sd = torch.load(out / "module_weights.pt", weights_only=True)
    assert sd["actor.2.weight"].shape[0] == 4 and sd["actor.0.weight"].shape[1] == 2 * (sd["critic.0.weight"].shape[1] // 2)
    res = json.loads((out / "eval_results.json").read_text())
    assert res["eval/episodes"] == 2 and res["iteration"] == 2


@pytest.mark.parametrize("kind", ["head", "gru_trunk", "gru_nets"])
def test_mu_sigma_head_and_gru_networks_through_the_cppo_trainer(kind):
    # the existing code paths on the centralised view (2 x 4 x 2 env: 4 joint actions): the mu/sigma head on
    # an MLP actor, a shared GRU trunk under MLP heads, GRU actor and critic
    from marlsc import make_synthetic_env_config
    from marlsc.cppo import CPPOConfig, CPPOTrainer
    gru = {"num_layers": 2, "hidden_size": 64, "bidirectional": False, "max_seq_len": 4}
    mlp = {"type": "mlp", "config": {"hidden_sizes": [64], "activation": "relu"}}
    if kind == "head":
        nets = {"shared_layers": None, "use_mu_sigma_head": True, "critic": mlp,
                "actor": {"type": "mlp", "config": {"hidden_sizes": [64], "activation": "relu", "output_activation_mu": "tanh"}}}
    elif kind == "gru_trunk":
        nets = {"shared_layers": {"type": "gru", "config": dict(gru, output_dim=64)}, "use_mu_sigma_head": False,
                "actor": mlp, "critic": mlp}
    else:
        g = {"type": "gru", "config": dict(gru)}
        nets = {"shared_layers": None, "use_mu_sigma_head": False, "actor": g, "critic": g}
    n_envs, steps = 32, 8
    raw = {"algorithm": {"name": "cppo",
                         "shared": {"num_epochs": 2, "num_minibatches": 2, "batch_size": n_envs * steps, "num_eval_episodes": 3,
                                    "learning_rate": 1e-3},
                         "algorithm_specific": {"use_kl_loss": True, "networks": nets}}}
    cfg = CPPOConfig.from_algorithm_config(raw)
    tr = CPPOTrainer(make_synthetic_env_config(2, 4, 2, episode_length=6), cfg, root_seed=3, n_envs=n_envs,
                     rollout_len=steps, device=0)
    assert tr.module.recurrent == (kind != "head") and tr.module.head_mode == (kind == "head")
    for _ in range(2):
        res = tr.train_iteration()
        assert all(np.isfinite(v) for k, v in res.items() if k.startswith("learner/"))
    ev = tr.evaluate()
    assert ev["eval/episodes"] == 3 and np.isfinite(ev["eval/episode_return_mean"]) and tr.evaluate() == ev
