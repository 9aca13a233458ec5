"""CPU tests around the fused PPO loss (marlsc/ppo_loss.py, csrc/ppo_loss.hip): the error bound of
tests/ppo_loss_emulation.py is one that torch's own float32 ppo_loss meets and that allows little; torch's
float64 autograd has the conventions at the kinks that the kernel's header states; the learner's switch."""
import numpy as np
import pytest
import torch
import yaml
from pathlib import Path

import ppo_loss_emulation as em

REPO = Path(__file__).resolve().parents[1]
COMBOS = [(shared, use_kl, beta) for shared in (False, True) for use_kl in (False, True) for beta in (None, 0.3)]


@pytest.mark.parametrize("K", em.KS)
def test_torch_f32_meets_the_bound_and_the_bound_allows_little(K):
    """On the generator's inputs torch's float32 ppo_loss (autograd) is inside the elementwise bound for
    every output, and the largest bound is at most 1e-4 of the output's largest magnitude."""
    n = 131
    for shared, use_kl, beta in COMBOS:
        cfg = em.make_cfg(use_kl=use_kl, beta=beta)
        g = np.random.default_rng(K)
        for idx in (None, g.integers(0, n + 40, size=n)):
            inp = em.make_inputs(n, K, B=n + 40, shared=shared, cfg=cfg, seed=1, idx=idx)
            # rows exactly on a clip bound: 2 in 5 are tried; the generator's docstring says why fewer land as
            # K grows and none from about K = 35
            assert inp["planted"] == int((inp["cls"] >= 3).sum())
            assert inp["planted"] >= (10 if K <= 16 else 0), inp["planted"]
            ref = em.run_torch(cfg, inp, dtype=torch.float64)
            got = em.run_torch(cfg, inp, dtype=torch.float32)
            bnd = em.bounds(cfg, inp)
            ob, vac = em.over_bound(got, ref, bnd), em.vacuity(ref, bnd)
            print(f"K {K} shared {shared} kl {use_kl} beta {beta} idx {idx is not None}: error/bound "
                  + " ".join(f"{k} {v:.3f}" for k, v in ob.items()) + " | bound/magnitude "
                  + " ".join(f"{k} {v:.2e}" for k, v in vac.items()))
            assert max(ob.values()) <= 1.0, ob
            assert max(vac.values()) <= 1e-4, vac


def _land(act_row, mean_row, ls_row, bound: float):
    """(action row, logp_old) in float64 with exp(logp - logp_old) == bound exactly: the first action
    coordinate is nudged until the solution or one of its two neighbours lands."""
    from marlsc.ppo import gaussian_logp
    for j in range(2000):
        a = act_row.clone()
        a[0] += j * 1e-9
        logp = float(gaussian_logp(a, mean_row, ls_row))
        x = logp - np.log(bound)
        for cand in (x, x + np.spacing(x), x - np.spacing(x)):
            if float(torch.exp(torch.tensor(logp - cand, dtype=torch.float64))) == bound:
                return a, float(cand)
    raise AssertionError("no float64 row lands the ratio on the bound")


def test_f64_autograd_conventions_at_the_kinks():
    """ppo_loss in float64: a ratio exactly at 1 -+ clip_param keeps the full A r gradient (torch.minimum
    splits the tie, torch.clamp passes the gradient at its bounds), a clipped surrogate and a zero
    advantage give grad_mean exactly 0, a value error exactly at vf_clip_param keeps 2 (v - t), one above
    it gives exactly 0."""
    from marlsc.ppo import gaussian_logp, ppo_loss
    cfg = em.make_cfg(clip_param=0.2, vf_clip_param=4.0, vf_loss_coeff=0.7, entropy_coeff=0.0)
    lo, hi = 1.0 - cfg.clip_param, 1.0 + cfg.clip_param
    T = lambda x: torch.tensor(x, dtype=torch.float64)  # noqa: E731
    n, K = 6, 2
    mean = T([[0.1, -0.2], [0.3, 0.5], [-0.4, 0.2], [0.0, 0.1], [0.7, -0.6], [0.2, 0.2]])
    ls = T([[0.1, -0.1]] * n)
    act = mean + T([[0.5, -0.25]] * n)
    (act[0], lpo0), (act[1], lpo1) = _land(act[0], mean[0], ls[0], hi), _land(act[1], mean[1], ls[1], lo)
    logp = gaussian_logp(act, mean, ls)
    # rows: 0 at hi with A > 0, 1 at lo with A < 0, 2 far above with A > 0 (clipped), 3 far below with
    # A < 0 (clipped), 4 inside with A = 0, 5 inside with A > 0
    lpo = T([lpo0, lpo1, float(logp[2]) - 1.0,
             float(logp[3]) + 1.0, float(logp[4]) - 0.01, float(logp[5]) + 0.05])
    ratio = torch.exp(logp - lpo)
    assert float(ratio[0]) == hi and float(ratio[1]) == lo
    adv = T([1.5, -0.75, 2.0, -1.0, 0.0, 0.5])
    vt = T([0.0, 1.0, -1.0, 0.5, 0.25, 2.0])
    values = vt + T([2.0, -2.0, 3.0, 1.0, -2.5, 0.0])  # vf = 4 (at), 4 (at), 9 (above), 1, 6.25 (above), 0
    m, l, v = mean.clone().requires_grad_(), ls.clone().requires_grad_(), values.clone().requires_grad_()
    total, _ = ppo_loss(cfg, m, l, v, {"actions": act, "logp": lpo, "advantages": adv, "value_targets": vt}, 0.0)
    total.backward()
    var = torch.exp(ls) ** 2
    full = -(adv * ratio / n)[:, None] * (act - mean) / var  # the unclipped surrogate's gradient
    for i in (0, 1, 5):
        torch.testing.assert_close(m.grad[i], full[i], rtol=1e-12, atol=0)
        assert float(m.grad[i].abs().min()) > 0
    for i in (2, 3, 4):
        assert torch.all(m.grad[i] == 0), (i, m.grad[i])
    gv = cfg.vf_loss_coeff / n * 2 * (values - vt)
    for i in (0, 1, 3, 5):
        torch.testing.assert_close(v.grad[i], gv[i], rtol=1e-12, atol=0)
    assert float(v.grad[0]) != 0 and float(v.grad[1]) != 0
    for i in (2, 4):
        assert float(v.grad[i]) == 0.0


def _small_module(device="cpu"):
    from marlsc.ppo import MultiAgentActorCritic, PPOConfig
    raw = yaml.safe_load(open(REPO / "config_files/algorithms/ippo.yaml"))
    cfg = PPOConfig.from_algorithm_config(raw)
    torch.manual_seed(0)
    return MultiAgentActorCritic(2, 6, 12, 3, cfg.rollout_config(), True).to(device), cfg


def test_fused_loss_on_a_cpu_module_raises():
    from marlsc.ppo import PPOLearner
    m, cfg = _small_module()
    with pytest.raises(RuntimeError, match="needs the module on a CUDA device"):
        PPOLearner(m, cfg, seed=0, fused_loss=True)


def test_fused_loss_defaults_to_the_torch_path(monkeypatch):
    from marlsc.ppo import PPOLearner
    m, cfg = _small_module()
    monkeypatch.delenv("MSC_FUSED_LOSS", raising=False)
    assert PPOLearner(m, cfg, seed=0).fused_loss is False
    assert PPOLearner(m, cfg, seed=0, fused_loss=False).fused_loss is False
    monkeypatch.setenv("MSC_FUSED_LOSS", "1")  # the switch is read when the learner is built
    assert PPOLearner(m, cfg, seed=0, fused_loss=False).fused_loss is False
    with pytest.raises(RuntimeError, match="needs the module on a CUDA device"):
        PPOLearner(m, cfg, seed=0)


def test_fused_ppo_loss_rejects_cpu_and_non_f32_inputs():
    from marlsc.ppo_loss import fused_ppo_loss
    cfg = em.make_cfg()
    inp = em.make_inputs(4, 3, cfg=cfg)
    b = {k: torch.from_numpy(v) for k, v in inp["batch"].items()}
    with pytest.raises(RuntimeError, match="must be a CUDA tensor"):
        fused_ppo_loss(cfg, torch.from_numpy(inp["mean"]), torch.from_numpy(inp["log_std"]),
                       torch.from_numpy(inp["values"]), b, None, 0.2)
