"""GPU tests of the mu/sigma actor head (use_mu_sigma_head): the fused dual-head kernels
(msc_mlp{2,3}_relu_musigma, csrc/mlp_musigma.hip) against the torch layer sequence, their sampling
epilogue against msc_gaussian_sample, the folded tier for 9..16 actions, the collector's paths and a
short training run with a checkpoint round trip. Parity with RLlib itself is unpinned (ray absent)."""
import ctypes as C

import numpy as np
import pytest
import torch
import torch.nn as nn

pytestmark = pytest.mark.gpu

SHAPES = [
    (34, [256, 256], 5, 4099),  # interleaved form, ragged tile, several blocks
    (34, [256], 5, 1000),       # one-hidden-layer kernel
    (13, [64, 64], 2, 31),      # fewer rows than one tile
    (34, [96], 8, 76),          # widest head, odd tile count
    (1, [64, 64], 1, 64),       # single input, single output
    (34, [128, 256], 4, 513),   # unequal layers
]
ACTS = {"none": None, "relu": nn.ReLU, "tanh": nn.Tanh, "sigmoid": nn.Sigmoid, "elu": nn.ELU, "gelu": nn.GELU}
_CACHE = {}


def _case(L, hidden, K, n):
    """Actor backbone, head, inputs and the torch layers' pre-activation head outputs of one shape,
    computed once. The sigma bias spans [-6, 6] so that the clamp at +-4.6 is hit on both sides."""
    key = (L, tuple(hidden), K, n)
    if key not in _CACHE:
        from marlsc.rollout import MLP, MuSigmaHead
        torch.manual_seed(L + K + n)
        actor = MLP(L, hidden[-1], {"hidden_sizes": hidden, "activation": "relu"}).cuda()
        head = MuSigmaHead(hidden[-1], K).cuda()
        with torch.no_grad():
            head.sigma_head.bias.copy_(torch.linspace(-6.0, 6.0, K) if K > 1 else torch.tensor([5.5]))
        g = torch.Generator(device="cuda").manual_seed(7)
        x = torch.randn(n, L, device="cuda", generator=g)
        eps = torch.randn(n, K, device="cuda", generator=g)
        with torch.no_grad():
            f = actor(x)
            raw = (head.mu_head(f), head.sigma_head(f))
        _CACHE[key] = (actor, head, x, eps, raw)
    return _CACHE[key]


def _set_acts(head, act_mu, act_sigma):
    head.mu_activation = ACTS[act_mu]() if ACTS[act_mu] else None
    head.sigma_activation = ACTS[act_sigma]() if ACTS[act_sigma] else None


def _ref(head, raw):
    mu = head.mu_activation(raw[0]) if head.mu_activation is not None else raw[0]
    ls = head.sigma_activation(raw[1]) if head.sigma_activation is not None else raw[1]
    return mu, torch.clamp(ls, -4.6, 4.6)


@pytest.mark.parametrize("act_mu,act_sigma", [("none", "none"), ("relu", "tanh"), ("tanh", "sigmoid"),
                                              ("sigmoid", "elu"), ("elu", "relu"), ("gelu", "gelu")])
@pytest.mark.parametrize("L,hidden,K,n", SHAPES)
def test_fused_dist_inputs_match_torch_layers(L, hidden, K, n, act_mu, act_sigma):
    # 2e-5 abs / rel (the fused MLP's tolerance; fold rounding <= 4.5e-7) for the 1-Lipschitz
    # activations, 3e-5 for GELU (slope up to ~1.13)
    from marlsc.mlp import musigma_forward, musigma_tier
    actor, head, x, _, raw = _case(L, hidden, K, n)
    _set_acts(head, act_mu, act_sigma)
    assert musigma_tier(list(actor), head) == 1
    with torch.no_grad():
        d = musigma_forward(list(actor), head, x)
        mu_ref, ls_ref = _ref(head, raw)
    assert d.shape == (n, 2 * K)
    tol = 3e-5 if "gelu" in (act_mu, act_sigma) else 2e-5
    torch.testing.assert_close(d[:, :K], mu_ref, rtol=tol, atol=tol)
    torch.testing.assert_close(d[:, K:], ls_ref, rtol=tol, atol=tol)
    if act_sigma == "none" and K > 1:  # the clamp is reached on both sides, exactly
        assert float(d[:, K:].min()) == np.float32(-4.6) and float(d[:, K:].max()) == np.float32(4.6)


def test_fused_head_follows_an_in_place_weight_update():
    # the pack cache is keyed by every contributing tensor: heads and the folded output Linear too
    from marlsc.mlp import musigma_forward
    from marlsc.rollout import MLP, MuSigmaHead
    torch.manual_seed(2)
    actor, head = MLP(13, 64, {"hidden_sizes": [64, 64]}).cuda(), MuSigmaHead(64, 2).cuda()
    x = torch.randn(100, 13, device="cuda")
    with torch.no_grad():
        d0 = musigma_forward(list(actor), head, x).clone()
        for p in (head.mu_head.weight, head.sigma_head.bias, actor[4].weight, actor[4].bias):
            p.mul_(1.5).add_(0.01)
            d = musigma_forward(list(actor), head, x)
            mu, ls = head(actor(x))
            assert not torch.equal(d, d0)
            torch.testing.assert_close(d[:, :2], mu, rtol=2e-5, atol=2e-5)
            torch.testing.assert_close(d[:, 2:], ls, rtol=2e-5, atol=2e-5)
            d0 = d.clone()


@pytest.mark.parametrize("hidden", [[64, 64], [96]])
def test_fused_head_with_a_split_first_layer(hidden):
    # a global-obs actor over local_w || global: the first Linear split into its local columns and a
    # per-env term (pre1, shared by the env's W rows), as the fused critic does
    from marlsc.mlp import musigma_forward
    from marlsc.rollout import MLP, MuSigmaHead
    torch.manual_seed(4)
    W, L, E, K = 3, 13, 50, 3
    actor = MLP(L * (1 + W), hidden[-1], {"hidden_sizes": hidden}).cuda()
    head = MuSigmaHead(hidden[-1], K, "tanh", "tanh").cuda()
    local = torch.randn(E, W, L, device="cuda")
    glob = local.reshape(E, 1, W * L).expand(E, W, W * L)
    with torch.no_grad():
        mu, ls = head(actor(torch.cat([local, glob], dim=-1)))
        first = actor[0]
        pre1 = torch.nn.functional.linear(local.reshape(E, W * L), first.weight[:, L:])
        d = musigma_forward(list(actor), head, local, w1=first.weight[:, :L], pre1=pre1, group=W)
    assert d.shape == (E, W, 2 * K)
    torch.testing.assert_close(d[..., :K], mu, rtol=2e-5, atol=2e-5)
    torch.testing.assert_close(d[..., K:], ls, rtol=2e-5, atol=2e-5)


@pytest.mark.parametrize("L,hidden,K,n", SHAPES[:4])
def test_fused_sampling_equals_dist_inputs_then_gaussian_kernel(L, hidden, K, n):
    # the epilogue is msc_gaussian_sample's arithmetic on the kernel's own (mu, log_std): bit for bit
    # the two-launch path, with and without dist_out
    from marlsc.mlp import musigma_forward
    from marlsc.rollout import LOG_STD_MIN, gaussian_sample
    actor, head, x, eps, _ = _case(L, hidden, K, n)
    _set_acts(head, "tanh", "none")
    mods = list(actor)
    new = lambda *s: torch.empty(*s, device="cuda")  # noqa: E731
    with torch.no_grad():
        d = musigma_forward(mods, head, x)
        a_ref, lp_ref = new(n, K), new(n)
        c_ref = gaussian_sample(d[:, :K].contiguous(), d[:, K:].contiguous(), LOG_STD_MIN, eps, a_ref, lp_ref)
        a, lp, c, d2 = new(n, K), new(n), new(n, K), new(n, 2 * K)
        assert musigma_forward(mods, head, x, d2, sample=(eps, a, lp, c)) is not None
        a3, lp3, c3 = new(n, K), new(n), new(n, K)
        assert musigma_forward(mods, head, x, sample=(eps, a3, lp3, c3)) is None  # dist inputs not written
    assert torch.equal(d2, d)
    for got in ((a, lp, c), (a3, lp3, c3)):
        assert torch.equal(got[0], a_ref) and torch.equal(got[1], lp_ref) and torch.equal(got[2], c_ref)
    assert torch.isfinite(lp_ref).all() and float(c_ref.abs().max()) <= 1.0


@pytest.mark.parametrize("form", ["8", "21"])
def test_head_pass_forms_bit_identical(monkeypatch, form):
    from marlsc.mlp import musigma_forward
    actor, head, x, eps, _ = _case(*SHAPES[0])
    _set_acts(head, "none", "none")
    n, K = x.shape[0], 5
    outs = []
    with torch.no_grad():
        for f in ("41", form):
            monkeypatch.setenv("MSC_MLP_P8", f)
            a, lp, c, d = (torch.empty(n, K, device="cuda"), torch.empty(n, device="cuda"),
                           torch.empty(n, K, device="cuda"), torch.empty(n, 2 * K, device="cuda"))
            musigma_forward(list(actor), head, x, d, sample=(eps, a, lp, c))
            torch.cuda.synchronize()
            outs.append((d, a, lp, c))
    for u, v in zip(*outs):
        assert torch.equal(u, v)


@pytest.mark.parametrize("form", ["4", "2"])
def test_losing_ab_forms_have_no_head_variant_and_fall_back(monkeypatch, form):
    from marlsc import abi
    from marlsc.mlp import musigma_forward, musigma_layout, musigma_tier
    from marlsc.rollout import head_sample
    actor, head, x, eps, _ = _case(*SHAPES[0])
    _set_acts(head, "none", "none")
    monkeypatch.setenv("MSC_MLP_P8", form)
    assert musigma_layout(256, 256, 5) is None and b"MSC_MLP_P8" in abi.lib().msc_last_error()
    assert musigma_tier(list(actor), head) == 3
    with torch.no_grad():
        with pytest.raises(ValueError):
            musigma_forward(list(actor), head, x)
        a, lp = torch.empty_like(eps), torch.empty(x.shape[0], device="cuda")
        c = head_sample(actor, head, x, eps, a, lp)  # the torch layers
        mu, ls = head(actor(x))
    torch.testing.assert_close(a, mu + ls.exp() * eps, rtol=1e-5, atol=1e-5)
    assert torch.equal(c, a.clamp(-1.0, 1.0))


def test_folded_tier_for_nine_actions():
    from marlsc.mlp import musigma_folded, musigma_tier
    from marlsc.rollout import LOG_STD_MIN, MLP, MuSigmaHead, gaussian_sample, head_sample
    torch.manual_seed(9)
    actor, head = MLP(34, 64, {"hidden_sizes": [64, 64]}).cuda(), MuSigmaHead(64, 9, "tanh", None).cuda()
    with torch.no_grad():
        head.sigma_head.bias.copy_(torch.linspace(-6.0, 6.0, 9))
    n = 300
    x, eps = torch.randn(n, 34, device="cuda"), torch.randn(n, 9, device="cuda")
    assert musigma_tier(list(actor), head) == 2
    with torch.no_grad():
        mu, ls = musigma_folded(list(actor), head, x)
        mu_ref, ls_ref = head(actor(x))
        torch.testing.assert_close(mu, mu_ref, rtol=2e-5, atol=2e-5)
        torch.testing.assert_close(ls, ls_ref, rtol=2e-5, atol=2e-5)
        a, lp = torch.empty(n, 9, device="cuda"), torch.empty(n, device="cuda")
        c = head_sample(actor, head, x, eps, a, lp)
        # tier 3's sampling (msc_gaussian_sample, one log_std row per row) on the same inputs
        a3, lp3 = torch.empty_like(a), torch.empty_like(lp)
        c3 = gaussian_sample(mu.contiguous(), ls.contiguous(), LOG_STD_MIN, eps, a3, lp3)
    assert torch.equal(a, a3) and torch.equal(lp, lp3) and torch.equal(c, c3)


def _collector(E=128, T=9, ep_len=5):
    from marlsc import make_synthetic_env_config
    from marlsc.rollout import ActorCritic, RolloutCollector, RolloutConfig
    from marlsc.spec import EnvSpec
    from marlsc.vec_env import VecInventoryEnv
    cfg = make_synthetic_env_config(8, 64, 5, episode_length=ep_len)
    spec = EnvSpec.from_config(cfg, {"include_warehouse_id": True})
    env = VecInventoryEnv(None, E, spec=spec, device=0, base_seed=77)
    env.reset()
    rc = RolloutConfig(critic_obs_type="global", use_mu_sigma_head=True,
                       actor={"hidden_sizes": [256, 256], "activation": "relu", "output_activation_mu": "tanh"})
    torch.manual_seed(0)
    m = ActorCritic(env.local_obs_dim, env.local_obs_dim * env.W, env.K, rc).cuda()
    return spec, env, m, RolloutCollector(env, m, T, seed=3)


def test_collector_fused_and_torch_tiers_agree(monkeypatch):
    from marlsc import mlp
    runs = []
    for tier3 in (False, True):
        spec, env, m, col = _collector()
        assert mlp.musigma_tier(list(m.actor), m.mu_sigma_head) == 1
        if tier3:
            monkeypatch.setattr(mlp, "musigma_tier", lambda mods, head: 3)
        b = col.collect()
        runs.append({k: v.clone() for k, v in b.items()})
        monkeypatch.undo()
    f, t = runs
    # identical env trajectories for identical (clipped) actions; the tiers differ by fold rounding
    first = None
    for s in range(f["obs"].shape[0]):
        assert torch.equal(f["obs"][s], t["obs"][s]), f"observations differ at step {s} after equal clipped actions"
        for k in ("actions", "logp"):
            torch.testing.assert_close(f[k][s], t[k][s], rtol=2e-5, atol=2e-5)
        torch.testing.assert_close(f["values"][s], t["values"][s], rtol=2e-5, atol=2e-5)
        if not torch.equal(f["actions"][s].clamp(-1, 1), t["actions"][s].clamp(-1, 1)):
            first = s
            break
        assert torch.equal(f["rewards"][s], t["rewards"][s]), f"rewards differ at step {s} after equal clipped actions"
    print("first step with differing clipped actions:", first)


def test_head_rollout_replays_bit_exact_on_a_fresh_env():
    from marlsc.vec_env import VecInventoryEnv
    spec, env, m, col = _collector(E=128, T=12)
    col.collect()
    assert torch.isfinite(col.logp).all()
    env2 = VecInventoryEnv(None, 128, spec=spec, device=0, base_seed=77)
    obs = env2.reset()
    for t in range(col.T):
        assert torch.equal(obs, col.obs[t])
        obs, rew, trunc, _ = env2.step(col.actions[t].clamp(-1.0, 1.0).contiguous())
        assert torch.equal(rew, col.rewards[t])
    # logp is the density of the unclipped action under the torch layers' distribution inputs
    with torch.no_grad():
        from marlsc.ppo import gaussian_logp
        full = env.obs_flat(obs=col.obs[5].contiguous())
        mu, ls = m.dist_inputs(col.obs[5], full)
        torch.testing.assert_close(gaussian_logp(col.actions[5], mu, ls), col.logp[5], rtol=1e-4, atol=1e-4)


def _head_trainer(E=32, T=8):
    from marlsc import make_synthetic_env_config
    from marlsc.ppo import PPOConfig, PPOTrainer
    raw = {"algorithm": {"name": "mappo", "shared": {"num_epochs": 2, "num_minibatches": 2, "batch_size": E * T,
                                                     "num_eval_episodes": 3, "learning_rate": 1e-3},
                         "algorithm_specific": {"parameter_sharing": True, "use_kl_loss": True, "networks": {
                             "shared_layers": None, "use_mu_sigma_head": True,
                             "actor": {"type": "mlp", "config": {"hidden_sizes": [64, 64], "activation": "relu",
                                                                 "output_activation_mu": "tanh"}},
                             "critic": {"type": "mlp", "config": {"hidden_sizes": [64, 64], "activation": "relu"}}}}}}
    cfg = PPOConfig.from_algorithm_config(raw)
    env_cfg = make_synthetic_env_config(2, 4, 2, episode_length=6)
    return PPOTrainer(env_cfg, cfg, root_seed=11, n_envs=E, rollout_len=T, device=0), env_cfg, cfg


def test_head_config_trains_evaluates_and_checkpoints(tmp_path):
    from marlsc.ppo import PPOTrainer
    tr, env_cfg, cfg = _head_trainer()
    head = tr.module.policies[0].mu_sigma_head
    w0 = (head.mu_head.weight.detach().clone(), head.sigma_head.weight.detach().clone())
    for _ in range(2):
        res = tr.train_iteration()
        for k in ("learner/total_loss", "learner/vf_loss", "learner/entropy", "learner/mean_kl"):
            assert np.isfinite(res[k]), (k, res[k])
    assert not torch.equal(w0[0], head.mu_head.weight) and not torch.equal(w0[1], head.sigma_head.weight)
    ev = tr.evaluate()
    assert ev["eval/episodes"] == 3 and np.isfinite(ev["eval/episode_return_mean"])
    ck = tr.save_checkpoint(tmp_path / "ck")
    w = torch.load(tr.export_module_weights(tmp_path / "module_weights.pt"), weights_only=True)
    assert "mu_sigma_head.mu_head.weight" in w and "mu_sigma_head.action_high" in w and "log_std" not in w
    tr2 = PPOTrainer(env_cfg, cfg, root_seed=11, n_envs=32, rollout_len=8, device=0)
    tr2.load_checkpoint(ck)
    b1, b2 = tr.collector.collect(), tr2.collector.collect()
    for k in b1:
        assert torch.equal(b1[k], b2[k]), k


def test_experiment_cli_with_a_head_config(tmp_path):
    # the shipped MAPPO YAML with the head switched on, through the experiment CLI that
    # scripts/run_experiment.sh drives: single (train, checkpoint, export) then evaluate
    import json
    from pathlib import Path

    import yaml
    from marlsc.experiment import main
    repo = Path(__file__).resolve().parents[1]
    raw = yaml.safe_load(open(repo / "config_files/algorithms/mappo.yaml"))
    nets = raw["algorithm"]["algorithm_specific"]["networks"]
    assert nets["use_mu_sigma_head"] is False  # the shipped configs keep the free log_std
    nets["use_mu_sigma_head"] = True
    nets["actor"]["config"].update({"hidden_sizes": [64, 64], "output_activation_mu": "tanh"})
    algo = tmp_path / "mappo_head.yaml"
    algo.write_text(yaml.safe_dump(raw))
    env = repo / "config_files/environments/env_c1_2wh4r2sku.yaml"
    assert main(["--mode", "single", "--env-config", str(env), "--algorithm-config", str(algo),
                 "--storage-dir", str(tmp_path), "--experiment-name", "H", "--root-seed", "42",
                 "--num-iterations", "2", "--envs", "32", "--rollout-len", "4"]) == 0
    out = tmp_path / "H"
    assert len((out / "training_metrics.jsonl").read_text().strip().splitlines()) == 2
    w = torch.load(out / "module_weights.pt", weights_only=True)
    assert {"actor.4.weight", "mu_sigma_head.mu_head.weight", "mu_sigma_head.sigma_head.bias",
            "mu_sigma_head.action_low"} <= set(w) and "log_std" not in w
    assert tuple(w["actor.4.weight"].shape) == (64, 64)
    assert main(["--mode", "evaluate", "--storage-dir", str(tmp_path), "--experiment-name", "H",
                 "--eval-episodes", "3", "--root-seed", "42"]) == 0
    assert json.loads((out / "eval_results.json").read_text())["eval/episodes"] == 3


def test_bad_arguments_return_errors():
    from marlsc import abi
    L = abi.lib()
    z = torch.zeros(1 << 16, device="cuda")
    n, K = 64, 2
    p = lambda t: C.c_void_p(t.data_ptr())  # noqa: E731
    out = torch.zeros(n * 2 * K, device="cuda")

    def call3(ep, k=K, h1=64, h2=64):
        return L.msc_mlp3_relu_musigma(p(z), n, 13, h1, h2, k, p(z), p(z), p(z), p(z), p(z), p(z), None, 1,
                                       C.byref(ep) if ep is not None else None, None)

    def call2(ep, k=K, h=64):
        return L.msc_mlp2_relu_musigma(p(z), n, 13, h, k, p(z), p(z), p(z), p(z), None, 1, C.byref(ep), None)

    E = abi.MscMuSigmaEpilogue
    good = E(0, 0, -4.6, 4.6, None, None, None, None, p(out))
    assert call3(good) == 0 and call2(good) == 0
    torch.cuda.synchronize()
    for k in (0, 9, 17):  # K out of range
        assert call3(good, k=k) != 0 and b"1..8" in L.msc_last_error()
        assert call2(good, k=k) != 0
    assert call3(good, h1=96, h2=96) != 0 and call2(good, h=100) != 0 and call3(good, h2=0) != 0
    assert call2(E(0, 0, -4.6, 4.6, None, None, None, None, p(out)), k=8, h=1024) != 0  # 64 KiB of staged weights
    assert call3(None) != 0
    assert call3(E(0, 0, -4.6, 4.6, None, p(out), p(out), p(out), None)) != 0  # outputs without eps
    assert b"eps" in L.msc_last_error()
    assert call3(E(0, 0, -4.6, 4.6, p(z), p(out), None, p(out), None)) != 0    # eps with a missing output
    assert call3(E(0, 0, -4.6, 4.6, None, None, None, None, None)) != 0        # nothing to write
    assert call3(E(6, 0, -4.6, 4.6, None, None, None, None, p(out))) != 0      # unknown activation code
    assert call3(E(0, 0, 1.0, -1.0, None, None, None, None, p(out))) != 0      # empty clamp range
    torch.cuda.synchronize()
