"""PPOLearner.update's one loop over PPOLearner.minibatch_step (marlsc/ppo.py) under every combination of the
learner's switches (fused_loss, fused_mlp, fused_opt), on the GPU: each combination makes exactly one
minibatch_step call and one optimizer step per counted step, returns the same keys in the same order, finite
values, and the same adaptive KL coefficients. How close the combinations' numbers are to one another is the
subject of test_gpu_ppo_loss.py / test_gpu_mlp_backward.py / test_gpu_adam.py (float64 quotients), not of this
file.

Shapes: 2 agents, 7 observation columns, 3 actions, [32] networks, 12 env rows, minibatches of 5 rows over 2
epochs, so that every stream wraps across a reshuffle inside a minibatch: the shared policy's 24 rows take
ceil(48 / 5) = 10 steps, each per-agent policy's 12 rows ceil(24 / 5) = 5. The GRU case (a shared GRU trunk,
max_seq_len 2) has 6 x 9 env rows, 54 sequences, 5 per minibatch: ceil(108 / 5) = 22 steps.
The KL term is on. The MLP cases' old distribution is the initial one with the mean moved by 0.1, a KL of
3 x 0.1^2 / (2 exp(2 logstd_init)) = 0.15 at the first step against 2 kl_target = 0.02: every combination
multiplies its coefficients by 1.5. The GRU case's old distribution is the learner's own first forward: the KL
starts at 0 and 22 steps at lr 5.2e-4 leave it far below kl_target / 2 = 0.005 (x 0.5)."""
import copy
import itertools
from pathlib import Path

import numpy as np
import pytest
import torch
import yaml

pytestmark = pytest.mark.gpu

REPO = Path(__file__).resolve().parents[1]
W, L, K = 2, 7, 3
MLP = {"type": "mlp", "config": {"hidden_sizes": [32], "activation": "relu"}}
GRU = {"type": "gru", "config": {"num_layers": 1, "hidden_size": 32, "bidirectional": False, "max_seq_len": 2,
                                 "output_dim": 32}}
SWITCHES = [dict(zip(("fused_loss", "fused_mlp", "fused_opt"), c)) for c in itertools.product((False, True), repeat=3)]
KEYS = ["policy_loss", "vf_loss", "entropy", "mean_kl", "total_loss", "num_minibatch_steps", "kl_coeff", "learning_rate"]


def _case(sharing, trunk, batch_size):
    """(cfg, module on the CPU)"""
    from marlsc.ppo import MultiAgentActorCritic, PPOConfig
    raw = yaml.safe_load(open(REPO / "config_files/algorithms/ippo.yaml"))
    raw["algorithm"]["algorithm_specific"].update(
        parameter_sharing=sharing, use_kl_loss=True, grad_clip=0.5,
        networks={"shared_layers": trunk, "actor": MLP, "critic": MLP, "use_mu_sigma_head": False})
    raw["algorithm"]["shared"].update(num_epochs=2, num_minibatches=2, batch_size=batch_size)
    cfg = PPOConfig.from_algorithm_config(raw)
    torch.manual_seed(3)
    return cfg, MultiAgentActorCritic(W, L, L * W, K, cfg.rollout_config(), sharing)


def _mlp_batch(m, S=12):
    from marlsc.ppo import gaussian_logp
    g = torch.Generator().manual_seed(7)
    r = lambda *s: torch.randn(s, generator=g)  # noqa: E731
    obs = r(S, W, L)
    with torch.no_grad():
        mean, ls = m.dist_inputs(obs)
        ls = ls.contiguous()
        act = mean + ls.exp() * r(*mean.shape)
        logp = gaussian_logp(act, mean, ls) + 0.1 * r(S, W)
    return {"obs": obs, "actions": act, "logp": logp, "advantages": r(S, W), "value_targets": r(S, W),
            "mean_old": mean + 0.1, "log_std_old": ls.clone()}


def _gru_batch(m, T=6, E=9):
    g = torch.Generator().manual_seed(7)
    r = lambda *s: torch.randn(s, generator=g)  # noqa: E731
    S = T * E
    seq = {"T": T, "E": E, "S": 2, "truncated": torch.zeros((T, E, W), dtype=torch.uint8),
           "state_in": {k: 0.3 * r(T // 2, *h.shape) for k, h in m.initial_state(E, device="cpu").items()}}
    seq["truncated"][2, 4] = 1  # one episode boundary inside a chunk: the masked step-by-step sequence path
    return {"obs": r(S, W, L), "actions": r(S, W, K), "logp": -3.0 + 0.1 * r(S, W), "advantages": r(S, W),
            "value_targets": r(S, W), "seq": seq}


def _cuda(v):
    if isinstance(v, dict):
        return {k: _cuda(x) for k, x in v.items()}
    return v.cuda() if isinstance(v, torch.Tensor) else v


def _counted(obj, name):
    """obj.name wrapped with a call counter, returned as a one-element list."""
    fn, calls = getattr(obj, name), [0]

    def wrapped(*a, **k):
        calls[0] += 1
        return fn(*a, **k)
    setattr(obj, name, wrapped)
    return calls


def _run_all(cfg, module, batch, switches, steps, sizes):
    from marlsc.optim import FusedClipAdam
    from marlsc.ppo import PPOLearner
    batch = _cuda(batch)
    outs, coeffs = [], []
    for sw in switches:
        learner = PPOLearner(copy.deepcopy(module).cuda(), cfg, seed=5, **sw)
        assert isinstance(learner.opt, FusedClipAdam) == sw.get("fused_opt", False)
        n_step, n_opt = _counted(learner, "minibatch_step"), _counted(learner.opt, "step")
        out = learner.update(dict(batch))
        print(sw, {k: float(v) for k, v in out.items()}, learner.kl_coeffs)
        assert out["num_minibatch_steps"] == steps == n_step[0] == n_opt[0], sw
        assert learner.last_minibatch_sizes == sizes
        assert list(out) == KEYS, sw
        assert all(np.isfinite(v) for v in out.values()), (sw, out)
        outs.append(out)
        coeffs.append(list(learner.kl_coeffs))
    assert all(c == coeffs[0] for c in coeffs), coeffs
    assert all(o["kl_coeff"] == outs[0]["kl_coeff"] and o["learning_rate"] == outs[0]["learning_rate"] for o in outs)
    return outs, coeffs[0]


@pytest.mark.parametrize("sharing", [True, False], ids=["shared", "per_agent"])
def test_every_switch_combination_runs_the_one_loop(sharing):
    cfg, module = _case(sharing, None, batch_size=10)
    _, coeffs = _run_all(cfg, module, _mlp_batch(module), SWITCHES, steps=10 if sharing else 5,
                         sizes=[5] * (1 if sharing else W))
    assert coeffs == [cfg.kl_coeff * 1.5] * (1 if sharing else W)


def test_gru_sequences_run_the_one_loop():
    cfg, module = _case(True, GRU, batch_size=20)
    assert module.recurrent
    switches = [dict(fused_loss=a, fused_opt=b) for a in (False, True) for b in (False, True)]
    _, coeffs = _run_all(cfg, module, _gru_batch(module), switches, steps=22, sizes=[5])
    assert coeffs == [cfg.kl_coeff * 0.5]
