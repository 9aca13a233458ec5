"""CPU tests around the fused clip + Adam step (csrc/adam_clip.hip, marlsc/optim.py): the numpy restatement of
its arithmetic (tests/adam_emulation.py) is torch.nn.utils.clip_grad_norm_ + torch.optim.Adam up to float32
rounding, FusedClipAdam's state is torch.optim.Adam's, and the learner's switch refuses a CPU module."""
import copy

import numpy as np
import pytest
import torch

import adam_emulation as em

EPS32 = 2.0 ** -24  # the relative error of one float32 rounding
LR, B1, B2, EPS = 1e-3, 0.9, 0.999, 1e-8
STEPS = 3
SHAPES = [((5, 3), 0), ((7,), 0), ((1,), 1), ((4, 4), 1), ((2, 3, 2), 2)]  # (shape, group)


def _data(seed):
    g = torch.Generator().manual_seed(seed)
    params = [torch.randn(s, generator=g) for s, _ in SHAPES]
    grads = [[torch.randn(s, generator=g) * (10.0 if grp == 0 else 0.05) for s, grp in SHAPES] for _ in range(STEPS)]
    return params, grads


@pytest.mark.parametrize("max_norm", [0.5, 1e3, None], ids=["clip_on", "clip_never_binds", "clip_off"])
def test_emulation_is_torch_clip_and_adam_to_float32_rounding(max_norm):
    """Against clip_grad_norm_ (per group) + torch.optim.Adam on float64 copies, 3 steps, 3 groups (with
    max_norm 0.5 group 0's norm is far above, group 1's far below: both sides of the clip in one call).

    The bound, per element and step k, first order in eps = 2^-24, from the operation count of the header's
    formulas (c, g', ... are the float64 run's values):
      g' = g c                   c rounded + 1 op: relative 2 eps
      m' = m + a1 (g' - m)       a1 rounded + 3 ops, and g' (2 eps): each relative to a term of size at most
                                 |m| + |g'|, so dm' <= 6 eps (|m| + |g'|) per step; an earlier step's dm is
                                 carried with weight b1 < 1: dm' <= 6 k eps max(|m| + |g'|) after k steps
      v' = b2 v + (a2 g') g'     b2, a2 rounded + 4 ops + g' twice (4 eps): 10 eps relative (no cancellation:
                                 every term >= 0), carried: 10 k eps after k steps
      denom = sqrt(v') / r2 + e  sqrt halves v's error (5 k eps) + 1; r2 rounded + 1 op; e rounded + 1 op:
                                 (5 k + 5) eps relative
      u = step_size (m' / denom) step_size rounded + 2 ops: du <= (step_size / denom) dm' + (5 k + 8) eps |u|
      p' = p - u                 1 op: eps |p'|, and p's own error carried
    so dp_k <= eps |p'| + (step_size / denom) 6 k eps max(|m| + |g'|) + (5 k + 8) eps |u|, summed over the
    steps, times 1.01 for the second-order terms. The update term u is ~1e-3 of p here: the p' rounding
    dominates, and the rest is a few units in the last place of u."""
    params, grads = _data(0)
    groups = [grp for _, grp in SHAPES]
    n_groups = max(groups) + 1
    p64 = [torch.nn.Parameter(p.double().clone()) for p in params]
    opt = torch.optim.Adam(p64, lr=LR, betas=(B1, B2), eps=EPS)
    tensors = [{"p": p.numpy().copy(), "g": None, "m": np.zeros(p.shape, np.float32), "v": np.zeros(p.shape, np.float32),
                "group": grp} for p, grp in zip(params, groups)]
    bound = [np.zeros(p.shape) for p in params]
    scale_m = [np.zeros(p.shape) for p in params]
    for k in range(1, STEPS + 1):
        m_before = [opt.state[p]["exp_avg"].detach().abs().numpy().copy() if p in opt.state else np.zeros(p.shape)
                    for p in p64]
        for p, g in zip(p64, grads[k - 1]):
            p.grad = g.double().clone()
        if max_norm:
            for j in range(n_groups):
                torch.nn.utils.clip_grad_norm_([p for p, grp in zip(p64, groups) if grp == j], max_norm)
        opt.step()
        for t, g in zip(tensors, grads[k - 1]):
            t["g"] = g.numpy()
        tensors, norms = em.step(tensors, n_groups, lr=LR, beta1=B1, beta2=B2, eps=EPS, max_norm=max_norm or 0.0, step=k)
        step_size = LR / (1 - B1 ** k)
        for i, p in enumerate(p64):
            st = opt.state[p]
            gc = p.grad.abs().numpy()
            scale_m[i] = np.maximum(scale_m[i], m_before[i] + gc)
            denom = st["exp_avg_sq"].sqrt().numpy() / np.sqrt(1 - B2 ** k) + EPS
            u = step_size * st["exp_avg"].abs().numpy() / denom
            bound[i] += EPS32 * (np.abs(p.detach().numpy()) + step_size / denom * 6 * k * scale_m[i] + (5 * k + 8) * u)
            err = np.abs(tensors[i]["p"].astype(np.float64) - p.detach().numpy())
            assert (err <= 1.01 * bound[i]).all(), (k, i, float((err / bound[i]).max()))
            # the state itself, by the same count: 6 k eps (|m| + |g'|) and 10 k eps v
            em_err = np.abs(tensors[i]["m"].astype(np.float64) - st["exp_avg"].numpy())
            assert (em_err <= 1.01 * 6 * k * EPS32 * scale_m[i]).all(), (k, i)
            ev_err = np.abs(tensors[i]["v"].astype(np.float64) - st["exp_avg_sq"].numpy())
            assert (ev_err <= 1.01 * 10 * k * EPS32 * st["exp_avg_sq"].numpy()).all(), (k, i)
    # the clip bit where it should: group 0 above max_norm 0.5, groups 1 and 2 below; never with 1e3 or off
    c = [float(em.clip_coef(n, max_norm or 0.0)) for n in norms]
    assert (c[0] < 1.0) == (max_norm == 0.5) and c[1] == 1.0 and c[2] == 1.0
    assert all(t["p"].dtype == np.float32 for t in tensors)


def test_emulation_norm_is_exact_on_integers_and_the_clip_coefficient_is_one_at_the_boundary():
    g = [{"g": np.array([3.0, -4.0], np.float32), "group": 0}, {"g": np.array([12.0], np.float32), "group": 0},
         {"g": np.zeros(3, np.float32), "group": 1}]
    norms = em.group_norms(g, 3)
    assert norms.tolist() == [13.0, 0.0, 0.0]
    assert em.clip_coef(13.0, 13.0) == np.float32(13.0 / (13.0 + 1e-6)) < 1  # torch's 1e-6: equal still scales
    assert em.clip_coef(13.0, 0.0) == 1 and em.clip_coef(13.0, -1.0) == 1 and em.clip_coef(0.0, 1.0) == 1


def _cpu_params(seed=1):
    g = torch.Generator().manual_seed(seed)
    return [[torch.nn.Parameter(torch.randn(s, generator=g)) for s, grp in SHAPES if grp == j] for j in range(3)]


def test_state_dict_round_trips_through_torch_adam():
    from marlsc.optim import FusedClipAdam
    lists = _cpu_params()
    flat = [p for ps in lists for p in ps]
    t1 = torch.optim.Adam(flat, lr=3e-4)
    g = torch.Generator().manual_seed(2)
    for _ in range(2):
        for p in flat[:-1]:  # the last parameter never gets a gradient: no state
            p.grad = torch.randn(p.shape, generator=g)
        t1.step()
    sd = copy.deepcopy(t1.state_dict())
    fused = FusedClipAdam(lists, lr=1.0)
    fused.load_state_dict(sd)
    assert fused.param_groups[0]["lr"] == 3e-4 and fused._steps == [2] * (len(flat) - 1) + [0]
    out = fused.state_dict()
    assert sorted(out["state"]) == list(range(len(flat) - 1)) and out["param_groups"][0]["params"] == list(range(len(flat)))
    assert set(out["param_groups"][0]) == set(sd["param_groups"][0])
    for i, st in out["state"].items():
        assert float(st["step"]) == 2.0 and st["step"].dtype == torch.float32
        assert torch.equal(st["exp_avg"], sd["state"][i]["exp_avg"]) and st["exp_avg"].data_ptr() != sd["state"][i]["exp_avg"].data_ptr()
        assert torch.equal(st["exp_avg_sq"], sd["state"][i]["exp_avg_sq"])
    # ... and back: a fresh torch.optim.Adam resumed from FusedClipAdam's state continues t1 bit for bit
    flat2 = [torch.nn.Parameter(p.detach().clone()) for p in flat]
    t2 = torch.optim.Adam(flat2, lr=1.0)
    t2.load_state_dict(copy.deepcopy(out))
    for p, q in zip(flat, flat2):
        p.grad = torch.randn(p.shape, generator=g)
        q.grad = p.grad.clone()
    t1.step(), t2.step()
    for p, q in zip(flat, flat2):
        assert torch.equal(p, q)
    # a fresh FusedClipAdam has no state, and torch.optim.Adam accepts that too
    empty = FusedClipAdam(_cpu_params()).state_dict()
    assert empty["state"] == {}
    torch.optim.Adam(flat2).load_state_dict(empty)
    with pytest.raises(ValueError, match="one parameter group of"):
        FusedClipAdam([lists[0]]).load_state_dict(sd)
    bad = copy.deepcopy(sd)
    bad["param_groups"][0]["weight_decay"] = 0.1
    with pytest.raises(ValueError, match="not supported"):
        fused.load_state_dict(bad)


def test_step_refuses_cpu_parameters():
    from marlsc.optim import FusedClipAdam
    lists = _cpu_params()
    opt = FusedClipAdam(lists)
    for p in lists[0]:
        p.grad = torch.ones_like(p)
    with pytest.raises(RuntimeError, match="HIP kernel and needs the parameters on a CUDA device"):
        opt.step(1e-3, 1.0)
    opt.zero_grad()
    assert all(p.grad is None for p in lists[0])
    with pytest.raises(ValueError, match="appears twice"):
        FusedClipAdam([lists[0], lists[0]])
    with pytest.raises(RuntimeError, match="contiguous float32"):
        FusedClipAdam([[torch.nn.Parameter(torch.zeros(3, dtype=torch.float64))]])


def test_learner_switch_refuses_a_cpu_module(monkeypatch):
    from marlsc.ppo import MultiAgentActorCritic, PPOConfig, PPOLearner
    from marlsc.rollout import RolloutConfig
    rc = RolloutConfig(actor={"hidden_sizes": [32]}, critic={"hidden_sizes": [32]})
    module = MultiAgentActorCritic(2, 7, 14, 3, rc, shared=True)
    cfg = PPOConfig()
    with pytest.raises(RuntimeError, match=r"PPOLearner\(fused_opt=True\): the fused clip \+ Adam step is a HIP kernel"):
        PPOLearner(module, cfg, fused_opt=True)
    learner = PPOLearner(module, cfg)
    assert learner.fused_opt is False and isinstance(learner.opt, torch.optim.Adam)  # the default is off ...
    monkeypatch.setenv("MSC_FUSED_OPT", "1")  # ... and None reads the knob
    with pytest.raises(RuntimeError, match=r"PPOLearner\(fused_opt=True\)"):
        PPOLearner(module, cfg)
    assert PPOLearner(module, cfg, fused_opt=False).fused_opt is False
