"""GPU tests of the GRU networks: the fused step kernel (msc_gru_step, csrc/gru.hip) against an f64
evaluation of the same weights and formulas, its reset / no-store / pack-cache behaviour, the tier
selection, the collector's recurrent rollout against the learner's sequence forward, and a short
training run with a checkpoint round trip. Parity with RLlib itself is unpinned (ray absent)."""
import copy

import numpy as np
import pytest
import torch
import torch.nn as nn

pytestmark = pytest.mark.gpu

# (in_dim, hidden, layers, out_dim, rows)
SHAPES = [
    (34, 128, 2, 128, 4099),  # ragged tile, several blocks
    (13, 64, 1, 5, 31),       # under one tile
    (1, 64, 2, 1, 64),
    (34, 256, 1, 32, 513),
    (70, 128, 2, 256, 76),
    (34, 256, 2, 64, 333),    # the form whose last layer's state lives in LDS
]
EPS23 = 2.0 ** -23
_CACHE = {}


def _case(L, H, layers, out, n):
    """Network (weights scaled x3 so the gates saturate on both sides), inputs, a random state in
    (-1, 1) and an f64 copy of the network, built once per shape."""
    key = (L, H, layers, out, n)
    if key not in _CACHE:
        from marlsc.rollout import GRUNet
        torch.manual_seed(L + H + layers + out + n)
        net = GRUNet(L, out, {"hidden_size": H, "num_layers": layers, "max_seq_len": 20}).cuda()
        with torch.no_grad():
            for p in net.parameters():
                p.mul_(3.0)
        g = torch.Generator(device="cuda").manual_seed(11)
        x = torch.randn(n, L, device="cuda", generator=g)
        h = torch.rand(n, layers, H, device="cuda", generator=g) * 2 - 1
        _CACHE[key] = (net, x, h, copy.deepcopy(net).double())
    return _CACHE[key]


def _r64(net64, x, h):
    """R64: torch double on the device, the same weights and formulas."""
    from marlsc.gru import torch_step
    with torch.no_grad():
        return torch_step(net64, x.double(), h.double())


def _errors(net, net64, x, h):
    from marlsc.gru import gru_step_forward, torch_step
    with torch.no_grad():
        y, hn = gru_step_forward(net, x, h)
        yt, ht = torch_step(net, x, h)
    y64, h64 = _r64(net64, x, h)
    e = lambda a, b: float((a.double() - b).abs().max())  # noqa: E731
    return (e(y, y64), e(yt, y64)), (e(hn, h64), e(ht, h64)), (y, hn)


@pytest.mark.parametrize("L,H,layers,out,n", SHAPES)
def test_fused_step_matches_f64_within_four_times_torch_error(L, H, layers, out, n):
    # the fused path differs from torch's f32 layers only in summation order and the libm variants of
    # sigmoid / tanh: e_fused <= 4 max(e_torch, 2^-23); an indexing or bias bug is >= 1e-3 here
    from marlsc.gru import gru_tier
    net, x, h, net64 = _case(L, H, layers, out, n)
    assert gru_tier(net) == 1
    (ey, eyt), (eh, eht), (y, hn) = _errors(net, net64, x, h)
    print(f"shape {(L, H, layers, out, n)}: y e_fused {ey:.3e} e_torch {eyt:.3e}; h e_fused {eh:.3e} e_torch {eht:.3e}")
    assert y.shape == (n, out) and hn.shape == (n, layers, H)
    assert ey <= 4 * max(eyt, EPS23), (ey, eyt)
    assert eh <= 4 * max(eht, EPS23), (eh, eht)


@pytest.mark.parametrize("L,H,layers,out,n", SHAPES)
def test_25_carried_steps_match_f64(L, H, layers, out, n):
    from marlsc.gru import gru_step_forward, torch_step
    net, x, h, net64 = _case(L, H, layers, out, n)
    g = torch.Generator(device="cuda").manual_seed(5)
    hf, ht, h64 = h, h, h.double()
    with torch.no_grad():
        for _ in range(25):
            xs = torch.randn(n, L, device="cuda", generator=g)
            yf, hf = gru_step_forward(net, xs, hf)
            yt, ht = torch_step(net, xs, ht)
            y64, h64 = torch_step(net64, xs.double(), h64)
    e = lambda a, b: float((a.double() - b).abs().max())  # noqa: E731
    print(f"25 steps {(L, H, layers, out, n)}: y {e(yf, y64):.3e} vs {e(yt, y64):.3e}; h {e(hf, h64):.3e} vs {e(ht, h64):.3e}")
    assert e(yf, y64) <= 4 * max(e(yt, y64), EPS23)
    assert e(hf, h64) <= 4 * max(e(ht, h64), EPS23)


@pytest.mark.parametrize("H,layers,act", [(64, 1, "relu"), (256, 2, "gelu"), (256, 2, None)])
def test_output_projection_activations_match_f64(H, layers, act):
    from marlsc.gru import gru_step_forward, gru_tier, torch_step
    from marlsc.rollout import GRUNet
    torch.manual_seed(3)
    net = GRUNet(34, 5, {"hidden_size": H, "num_layers": layers, "max_seq_len": 4, "activation": act,
                         "output_activation": "tanh"}).cuda()
    assert gru_tier(net) == 1 and isinstance(net["output_proj"], nn.Sequential)
    x, h = torch.randn(100, 34, device="cuda"), torch.rand(100, layers, H, device="cuda") * 2 - 1
    with torch.no_grad():
        y, _ = gru_step_forward(net, x, h)
        yt, _ = torch_step(net, x, h)
        y64, _ = torch_step(copy.deepcopy(net).double(), x.double(), h.double())
    ef, et = float((y.double() - y64).abs().max()), float((yt.double() - y64).abs().max())
    assert ef <= 4 * max(et, EPS23), (ef, et)


def test_reset_flags_equal_a_hand_zeroed_state_bitwise():
    from marlsc.gru import gru_step_forward
    net, x, h, _ = _case(*SHAPES[0])
    n = 4098  # a multiple of the group
    x, h = x[:n].contiguous(), h[:n].contiguous()
    g = torch.Generator(device="cuda").manual_seed(2)
    reset = (torch.rand(n // 3, device="cuda", generator=g) < 0.3).to(torch.uint8)
    rows = reset.bool().repeat_interleave(3)
    assert 0 < int(rows.sum()) < n
    hz = h.clone()
    hz[rows] = 0.0
    with torch.no_grad():
        y0, h0 = gru_step_forward(net, x, h)
        y1, h1 = gru_step_forward(net, x, h, reset, 3)
        y2, h2 = gru_step_forward(net, x, hz)
    assert torch.equal(y1, y2) and torch.equal(h1, h2)
    assert torch.equal(y1[~rows], y0[~rows]) and torch.equal(h1[~rows], h0[~rows])
    assert not torch.equal(y1[rows], y0[rows])


@pytest.mark.parametrize("shape", [SHAPES[3], SHAPES[5]])
def test_no_state_store_gives_the_same_output_and_touches_nothing(shape):
    from marlsc.gru import gru_step_forward
    net, x, h, _ = _case(*shape)
    poison = torch.full_like(h, 12345.0)
    with torch.no_grad():
        y0, _ = gru_step_forward(net, x, h)
        y1, none = gru_step_forward(net, x, h, store_state=False, h_out=poison)
    assert none is None and torch.equal(y0, y1)
    assert bool((poison == 12345.0).all())


@pytest.mark.parametrize("name", ["weight_ih_l0", "bias_hh_l1", "output_proj.weight"])
def test_fused_step_follows_an_in_place_weight_update(name):
    # the pack cache is keyed by every contributing tensor, biases included
    from marlsc.rollout import GRUNet
    torch.manual_seed(9)
    net = GRUNet(34, 128, {"hidden_size": 128, "num_layers": 2, "max_seq_len": 20}).cuda()
    with torch.no_grad():
        for p in net.parameters():
            p.mul_(3.0)
    x, h = torch.randn(200, 34, device="cuda"), torch.rand(200, 2, 128, device="cuda") * 2 - 1
    _, _, (y0, h0) = _errors(net, copy.deepcopy(net).double(), x, h)
    p = dict(net.named_parameters())["gru." + name if "proj" not in name else name]
    with torch.no_grad():
        p.add_(0.05)
    (ey, eyt), (eh, eht), (y1, h1) = _errors(net, copy.deepcopy(net).double(), x, h)
    assert not torch.equal(y0, y1)
    assert ey <= 4 * max(eyt, EPS23) and eh <= 4 * max(eht, EPS23)


@pytest.mark.parametrize("H,layers", [(96, 2), (128, 3)])
def test_sizes_outside_the_fused_set_run_the_torch_layers(H, layers):
    from marlsc.gru import gru_step_forward, gru_supported, gru_tier, torch_step
    from marlsc.rollout import GRUNet
    torch.manual_seed(1)
    net = GRUNet(34, 8, {"hidden_size": H, "num_layers": layers, "max_seq_len": 4}).cuda()
    assert gru_tier(net) == 3 and not gru_supported(34, H, layers, 8)
    x, h = torch.randn(50, 34, device="cuda"), torch.rand(50, layers, H, device="cuda")
    with torch.no_grad():
        y, hn = gru_step_forward(net, x, h)
        yt, ht = torch_step(net, x, h)
    assert torch.equal(y, yt) and torch.equal(hn, ht)


def test_supported_agrees_with_tier():
    from marlsc.gru import gru_supported, gru_tier
    from marlsc.rollout import GRUNet
    for L, H, layers, out in [(34, 64, 1, 1), (34, 128, 2, 128), (1024, 256, 2, 256), (34, 256, 2, 40), (34, 32, 1, 5),
                              (1025, 64, 1, 5), (34, 128, 2, 33), (34, 64, 2, 32)]:
        net = GRUNet(L, out, {"hidden_size": H, "num_layers": layers, "max_seq_len": 4})
        assert (gru_tier(net) == 1) == gru_supported(L, H, layers, out), (L, H, layers, out)


# ----------------------------------------------------------------------------------------------
# collector: 2 warehouses x 4 regions x 2 SKUs, episodes of 10 steps, chunks of S = 8
# ----------------------------------------------------------------------------------------------
# tau: the absolute tolerance of the rollout's fused kernels against the learner's torch layers on the
# distribution inputs and values. 2e-5 is the bound this suite already holds the fused MLP kernels to
# against the torch layer sequence (test_gpu_musigma.py, test_gpu_rollout.py): f32 sums of <= 256 terms
# of magnitude <= 1 in another order differ by about 256 x 2^-24 = 1.5e-5 at worst. Every value / mean
# here ends in such a sum (the 64-unit MLP heads, or a GRU's 64-unit projection). What enters it differs
# by the GRU step's own reordering, which the kernel tests above bound by 4 x the torch f32 layers'
# distance from f64 -- rounding of sums of <= 64 + 34 terms, an order below -- and a state in (-1, 1)
# under default-initialised weights (gains < 1) does not amplify it over the 8 steps of a chunk.
TAU = 2e-5
GRU_CFG = {"num_layers": 2, "hidden_size": 64, "bidirectional": False, "max_seq_len": 8}


def _algo(kind, E, T, **shared):
    mlp = {"type": "mlp", "config": {"hidden_sizes": [64], "activation": "relu"}}
    if kind in ("trunk", "trunk_head"):  # ippo_gru-style: shared GRU trunk, MLP heads, one shared policy
        nets = {"shared_layers": {"type": "gru", "config": dict(GRU_CFG, output_dim=64)}, "actor": mlp, "critic": mlp}
        if kind == "trunk_head":  # the mu/sigma head on the MLP actor over the trunk
            nets["actor"] = {"type": "mlp", "config": {"hidden_sizes": [64], "activation": "relu",
                                                       "output_activation_mu": "tanh"}}
        name, sharing = "ippo", True
    else:  # GRU actor and critic, no trunk, MAPPO observation types, one policy per agent
        g = {"type": "gru", "config": dict(GRU_CFG)}
        nets = {"shared_layers": None, "actor": g, "critic": g}
        name, sharing = "mappo", False
    nets["use_mu_sigma_head"] = kind == "trunk_head"
    sh = {"num_epochs": 2, "num_minibatches": 2, "batch_size": E * T, "num_eval_episodes": 3, "learning_rate": 1e-3}
    sh.update(shared)
    return {"algorithm": {"name": name, "shared": sh,
                          "algorithm_specific": {"parameter_sharing": sharing, "use_kl_loss": True, "networks": nets}}}


def _gru_collector(kind, E=64, T=24, ep_len=10):
    from marlsc import make_synthetic_env_config
    from marlsc.ppo import MultiAgentActorCritic, PPOConfig, PPOLearner
    from marlsc.rollout import RolloutCollector
    from marlsc.spec import EnvSpec
    from marlsc.vec_env import VecInventoryEnv
    cfg = PPOConfig.from_algorithm_config(_algo(kind, E, T))
    spec = EnvSpec.from_config(make_synthetic_env_config(2, 4, 2, episode_length=ep_len),
                               {"include_warehouse_id": cfg.parameter_sharing})
    env = VecInventoryEnv(None, E, spec=spec, device=0, base_seed=77)
    env.reset()
    torch.manual_seed(0)
    m = MultiAgentActorCritic(env.W, env.local_obs_dim, env.local_obs_dim * env.W, env.K, cfg.rollout_config(),
                              cfg.parameter_sharing).cuda()
    col = RolloutCollector(env, m, T, seed=3, adv_groups=1 if cfg.parameter_sharing else env.W)
    return env, m, col, PPOLearner(m, cfg, seed=0)


@pytest.fixture
def fused_only(monkeypatch):
    """The rollout must take the fused step: the torch layers' step raises while this is active, and
    the launches of msc_gru_step are counted."""
    from marlsc import gru

    def no_torch(*a, **k):
        raise AssertionError("the rollout fell back to the torch layers (gru.torch_step)")
    monkeypatch.setattr(gru, "torch_step", no_torch)
    calls = {"n": 0}
    lib = gru.abi.lib()
    real = lib.msc_gru_step

    def counted(*a):
        calls["n"] += 1
        return real(*a)

    class Counting:  # the loaded library with msc_gru_step counted
        msc_gru_step = staticmethod(counted)

        def __getattr__(self, name):
            return getattr(lib, name)
    proxy = Counting()

    def counting_lib():
        return proxy
    monkeypatch.setattr(gru.abi, "lib", counting_lib)
    return calls


def _check_against_sequence_forward(m, col, learner, b, T, E):
    """The learner's sequence forward (no_grad) from the stored state_in + truncated against the
    stored values and logp."""
    from marlsc.ppo import gaussian_logp
    W, S = col.env.W, col.S
    seq = {"T": T, "E": E, "S": S, "state_in": b["state_in"], "truncated": b["truncated"]}
    obs = b["obs"].reshape(T * E, W, -1)
    acts, logp, vals = b["actions"].reshape(T * E * W, -1), b["logp"].reshape(-1), b["values"][:T].reshape(-1)
    with torch.no_grad():
        for pol, ids in zip(m.policies, learner._seq_ids(T // S, E, W, obs.device)):
            mean, log_std, values, rows = learner._seq_forward(pol, obs, seq, ids)
            ev = (values - vals[rows]).abs()
            assert bool((ev <= TAU).all()), float(ev.max())
            a = acts[rows]
            bound = ((a - mean).abs() / (2 * log_std).exp()).sum(-1) * TAU + TAU
            el = (gaussian_logp(a, mean, log_std) - logp[rows]).abs()
            assert bool((el <= bound).all()), float((el - bound).max())
            print(f"sequence forward vs rollout: values {float(ev.max()):.3e}, logp {float(el.max()):.3e} "
                  f"(bound >= {float(bound.min()):.3e})")


@pytest.mark.parametrize("kind", ["trunk", "gru_heads", "trunk_head"])
def test_collector_matches_the_learners_sequence_forward(kind, fused_only):
    from marlsc.gru import gru_tier
    E, T = 64, 24
    env, m, col, learner = _gru_collector(kind, E, T)
    nets = [g for p in m.policies for g in p.gru_slots().values()]
    assert nets and all(gru_tier(g) == 1 for g in nets)
    assert m.recurrent and col.S == 8 and set(col.state) == ({"actor_h", "critic_h"} if kind == "gru_heads" else {"shared_h"})
    for h in col.state.values():
        assert h.shape == (E, env.W, 2, 64) and not h.any()
    # first collect: episodes end at steps 9 and 19 (inside chunks); second: at 29 and 39, so the
    # reset of step 40 falls on a chunk edge
    for it in range(2):
        b = {k: (v.clone() if torch.is_tensor(v) else {s: h.clone() for s, h in v.items()})
             for k, v in col.collect().items()}
        tr = b["truncated"][:, :, 0].bool()
        assert tr.any(dim=1).nonzero().flatten().tolist() == ([9, 19] if it == 0 else [5, 15])
        assert b["state_in"][next(iter(b["state_in"]))].shape == (T // 8, E, env.W, 2, 64)
        if it == 0:
            assert not any(h[0].any() for h in b["state_in"].values())  # the first chunk starts from zero
        else:
            assert all(not h[2].any() for h in b["state_in"].values())  # chunk edge right after an episode end
        assert torch.isfinite(b["logp"]).all() and torch.isfinite(b["advantages"]).all()
        # every network once per step through the fused kernel (plus the bootstrap values)
        assert fused_only["n"] >= (it + 1) * T * len(nets)
        _check_against_sequence_forward(m, col, learner, b, T, E)


def test_states_are_zero_after_a_collect_that_ends_on_an_episode_end():
    env, m, col, _ = _gru_collector("trunk", E=64, T=40)
    col.collect()
    assert bool(col.truncated[-1].all())
    assert all(not h.any() for h in col.state.values())
    env, m, col, _ = _gru_collector("trunk", E=64, T=24)
    col.collect()
    assert all(h.any() for h in col.state.values())


def test_recurrent_rollout_reproduces_bit_for_bit_on_a_fresh_env():
    runs = []
    for _ in range(2):
        env, m, col, _ = _gru_collector("trunk")
        b = col.collect()
        runs.append({k: b[k].clone() for k in ("actions", "obs", "logp", "values")})
    for k in runs[0]:
        assert torch.equal(runs[0][k], runs[1][k]), k


# ----------------------------------------------------------------------------------------------
# training
# ----------------------------------------------------------------------------------------------
def _gru_trainer(E=64, T=16, seq=8):
    from marlsc import make_synthetic_env_config
    from marlsc.ppo import PPOConfig, PPOTrainer
    cfg = PPOConfig.from_algorithm_config(_algo("trunk", E, T))
    env_cfg = make_synthetic_env_config(2, 4, 2, episode_length=6)
    return PPOTrainer(env_cfg, cfg, root_seed=11, n_envs=E, rollout_len=T, device=0), env_cfg, cfg


def test_gru_config_trains_evaluates_and_resumes_exactly(tmp_path, fused_only):
    from marlsc.ppo import PPOTrainer
    tr, env_cfg, cfg = _gru_trainer()
    w0 = tr.module.policies[0].shared_layers["gru"].weight_hh_l0.detach().clone()
    for _ in range(2):
        res = tr.train_iteration()
        for k in ("learner/total_loss", "learner/vf_loss", "learner/entropy", "learner/mean_kl"):
            assert np.isfinite(res[k]), (k, res[k])
    assert not torch.equal(w0, tr.module.policies[0].shared_layers["gru"].weight_hh_l0)
    assert any(h.any() for h in tr.collector.state.values())
    assert fused_only["n"] > 2 * 16  # the rollouts launched the fused step (and never the torch layers)
    n0 = fused_only["n"]
    ev = tr.evaluate()
    assert ev["eval/episodes"] == 3 and np.isfinite(ev["eval/episode_return_mean"])
    assert fused_only["n"] == n0 + 6  # evaluation too: one launch per step of the 6-step episodes
    ck = tr.save_checkpoint(tmp_path / "ck")
    w = torch.load(tr.export_module_weights(tmp_path / "module_weights.pt"), weights_only=True)
    assert {"shared_layers.gru.weight_hh_l1", "shared_layers.output_proj.weight", "actor.0.weight", "log_std"} <= set(w)
    tr2 = PPOTrainer(env_cfg, cfg, root_seed=11, n_envs=64, rollout_len=16, device=0)
    tr2.load_checkpoint(ck)
    r1, r2 = tr.train_iteration(), tr2.train_iteration()
    assert r1 == r2, {k: (r1[k], r2.get(k)) for k in r1 if r1[k] != r2.get(k)}


def test_trainer_rounds_a_derived_rollout_length_up_to_whole_chunks():
    from marlsc import make_synthetic_env_config
    from marlsc.ppo import PPOConfig, PPOTrainer
    cfg = PPOConfig.from_algorithm_config(_algo("trunk", 64, 16, batch_size=64 * 11))
    tr = PPOTrainer(make_synthetic_env_config(2, 4, 2, episode_length=6), cfg, root_seed=1, n_envs=64, device=0)
    assert tr.T == 16 and tr.collector.S == 8
    with pytest.raises(ValueError, match="multiple of max_seq_len"):
        PPOTrainer(make_synthetic_env_config(2, 4, 2, episode_length=6), cfg, root_seed=1, n_envs=64, rollout_len=12, device=0)


def test_experiment_cli_with_the_ippo_gru_config(tmp_path):
    import json
    from pathlib import Path

    from marlsc.experiment import main
    repo = Path(__file__).resolve().parents[1]
    env = repo / "config_files/environments/env_c1_2wh4r2sku.yaml"
    assert main(["--mode", "single", "--env-config", str(env), "--algorithm-config",
                 str(repo / "config_files/algorithms/ippo_gru.yaml"), "--storage-dir", str(tmp_path),
                 "--experiment-name", "G", "--root-seed", "42", "--num-iterations", "2", "--envs", "64",
                 "--rollout-len", "20"]) == 0
    out = tmp_path / "G"
    assert len((out / "training_metrics.jsonl").read_text().strip().splitlines()) == 2
    w = torch.load(out / "module_weights.pt", weights_only=True)
    assert {"shared_layers.gru.weight_ih_l0", "shared_layers.gru.bias_hh_l1", "shared_layers.output_proj.bias",
            "actor.2.weight", "critic.2.weight", "log_std"} <= set(w)
    assert tuple(w["shared_layers.gru.weight_ih_l0"].shape)[0] == 384 and tuple(w["actor.0.weight"].shape) == (256, 128)
    assert main(["--mode", "evaluate", "--storage-dir", str(tmp_path), "--experiment-name", "G",
                 "--eval-episodes", "3", "--root-seed", "42"]) == 0
    assert json.loads((out / "eval_results.json").read_text())["eval/episodes"] == 3


def test_bad_arguments_return_errors():
    import ctypes as C

    from marlsc import abi
    L = abi.lib()
    z = torch.zeros(1 << 18, device="cuda")
    p = lambda t: C.c_void_p(t.data_ptr())  # noqa: E731
    gw = abi.MscGruWeights()
    gw.wi[0] = gw.wh[0] = gw.b[0] = gw.wo = gw.bo = z.data_ptr()
    y, ho = torch.zeros(64 * 8, device="cuda"), torch.zeros(64 * 64, device="cuda")

    def call(hidden=64, layers=1, out=8, h_out=ho, w=gw, reset=None, group=1, act=0, n=64):
        return L.msc_gru_step(p(z), n, 13, hidden, layers, out, p(z), C.byref(w) if w is not None else None, act, 0,
                              reset, group, p(y), None if h_out is None else p(h_out), None)

    assert call() == 0 and call(h_out=None) == 0
    torch.cuda.synchronize()
    assert call(hidden=96) != 0 and b"hidden in {64, 128, 256}" in L.msc_last_error()
    assert call(layers=3) != 0 and call(out=40) != 0 and call(w=None) != 0 and call(act=6) != 0
    assert call(layers=2) != 0 and b"layer 1" in L.msc_last_error()  # the second layer's buffers are missing
    assert call(h_out=z) != 0 and b"ping-pong" in L.msc_last_error()
    r = torch.zeros(64, dtype=torch.uint8, device="cuda")
    assert call(reset=p(r), group=5) != 0 and call(reset=p(r), group=0) != 0 and call(reset=p(r), group=4) == 0
    torch.cuda.synchronize()
