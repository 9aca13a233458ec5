"""GPU tests of the learner's multi-policy loss (PPOLearner(fused_multi_loss=True): one msc_ppo_loss_multi call
per minibatch step over all per-agent policies) against the same switches without it, which make one msc_ppo_loss
call per policy. The multi call promises the single call's bits per policy (tests/test_gpu_ppo_loss_multi_exact.py)
and everything around it -- stacking instead of slicing, one clamp of the stacked log_std rows -- moves values
without rounding, so every comparison is torch.equal: returned statistics, gradients, parameters, Adam moments and
the adaptive KL coefficients after one update and after a second. Calls are counted through a proxy on abi.lib()."""
import copy
import inspect

import pytest

torch = pytest.importorskip("torch")

from marlsc import abi  # noqa: E402
from test_gpu_mlp_backward import S_, _mlp, _torch_layer_calls  # noqa: E402
from test_gpu_mlp_multi_backward import NETS, W3, _assert_same_bits, _batch, _module  # noqa: E402

pytestmark = pytest.mark.gpu
KL0 = [0.2, 0.45, 0.1]  # one coefficient per policy, distinct from the first step on


@pytest.fixture
def counted(monkeypatch):
    """Counts the calls of the single-policy and of the multi-policy loss (the library handle marlsc.ppo_loss uses)."""
    calls = {"single": 0, "multi": 0}
    lib = abi.lib()

    def counting(name, key):
        real = getattr(lib, name)

        def f(*a):
            calls[key] += 1
            return real(*a)
        return staticmethod(f)

    class Counting:
        msc_ppo_loss = counting("msc_ppo_loss", "single")
        msc_ppo_loss_multi = counting("msc_ppo_loss_multi", "multi")

        def __getattr__(self, name):
            return getattr(lib, name)
    proxy = Counting()
    monkeypatch.setattr(abi, "lib", lambda: proxy)
    return calls


def _snapshot(m, learner):
    state = learner.opt.state_dict()["state"]
    return ({k: p.grad.detach().clone() for k, p in m.named_parameters() if p.grad is not None},
            {k: p.detach().clone() for k, p in m.named_parameters()},
            {(i, k): v.detach().clone() for i, s in state.items() for k, v in s.items() if torch.is_tensor(v)})


def _two_updates(module, cfg, batches, kl0=KL0, **switches):
    """test_gpu_mlp_multi_backward._two_updates with per-policy KL coefficients set before the first update: [(returned
    values, gradients, parameters, Adam state) after each], torch-layer calls, the learner."""
    from marlsc.ppo import PPOLearner
    m = copy.deepcopy(module)
    hooks = _torch_layer_calls(m)
    learner = PPOLearner(m, cfg, seed=5, **switches)
    learner.kl_coeffs = list(kl0[:len(learner.kl_coeffs)])
    res = []
    for b in batches:
        out = learner.update(b, None, 0)
        assert out["num_minibatch_steps"] == 1
        res.append((out,) + _snapshot(m, learner))
    return res, hooks["n"], learner


@pytest.mark.parametrize("fused_opt", [False, True], ids=["torch_adam", "fused_opt"])
@pytest.mark.parametrize("fused_multi", [False, True], ids=["stack_path", "stacked_path"])
@pytest.mark.parametrize("case", list(NETS))
def test_two_updates_equal_the_per_policy_losses_bit_for_bit(case, fused_multi, fused_opt, counted):
    """ippo and mappo (KL on), the networks' outputs stacked by fused_multi or per policy and stacked here, torch
    Adam and the fused step: one multi call per step instead of P single calls, the same bits everywhere, and the
    adaptive KL coefficients move alike."""
    cfg, module = _module(*NETS[case])
    assert cfg.use_kl_loss and len(module.policies) == W3
    batches = [_batch(cfg, module, 2), _batch(cfg, module, 3)]
    sw = dict(fused_loss=True, fused_mlp=True, fused_multi=fused_multi, fused_opt=fused_opt)
    multi, torch_calls, learner = _two_updates(module, cfg, batches, fused_multi_loss=True, **sw)
    assert counted == {"single": 0, "multi": 2} and torch_calls == 0
    assert all(p.grad is not None and p.grad.is_contiguous() and p.grad.shape == p.shape for p in learner.module.parameters())
    single, torch_calls, ref = _two_updates(module, cfg, batches, **sw)
    assert ref.fused_multi_loss is False
    assert counted == {"single": 2 * W3, "multi": 2} and torch_calls == 0
    _assert_same_bits(multi, single)
    assert learner.kl_coeffs == ref.kl_coeffs and learner.kl_coeffs != KL0  # two updates adapted them
    assert "mean_kl" in multi[0][0] and "kl_coeff" in multi[0][0]
    assert not torch.equal(multi[0][2]["policies.0.actor.0.weight"], multi[1][2]["policies.0.actor.0.weight"])
    assert not torch.equal(multi[0][2]["policies.1.log_std"], multi[1][2]["policies.1.log_std"])


def test_torch_layers_without_any_mlp_switch(counted):
    """fused_loss and the switch alone: the torch layers' per-policy outputs are stacked."""
    cfg, module = _module(*NETS["mappo"])
    batches = [_batch(cfg, module, 2), _batch(cfg, module, 3)]
    multi, calls_multi, _ = _two_updates(module, cfg, batches, fused_loss=True, fused_multi_loss=True)
    assert counted == {"single": 0, "multi": 2} and calls_multi > 0
    single, calls_single, _ = _two_updates(module, cfg, batches, fused_loss=True)
    assert counted == {"single": 2 * W3, "multi": 2} and calls_single == calls_multi
    _assert_same_bits(multi, single)


def test_actors_stacked_by_the_multi_call_critics_per_policy(counted):
    """Critic hidden [48, 48] is outside the multi-policy MLP set: the actors' output arrives stacked, the critics'
    per policy, and the loss takes both."""
    nets = {"shared_layers": None, "actor": _mlp([32]), "critic": _mlp([48, 48]), "use_mu_sigma_head": False}
    cfg, module = _module("mappo", nets)
    batches = [_batch(cfg, module, 2), _batch(cfg, module, 3)]
    sw = dict(fused_loss=True, fused_mlp=True, fused_multi=True)
    mixed, _, _ = _two_updates(module, cfg, batches, fused_multi_loss=True, **sw)
    assert counted == {"single": 0, "multi": 2}
    single, _, _ = _two_updates(module, cfg, batches, **sw)
    assert counted == {"single": 2 * W3, "multi": 2}
    _assert_same_bits(mixed, single)


def test_mu_sigma_head_per_agent_module(counted):
    """Per-row log_std from every policy's mu/sigma head, stacked [n, P, K]."""
    nets = {"shared_layers": None, "actor": _mlp([32]), "critic": _mlp([32]), "use_mu_sigma_head": True}
    cfg, module = _module("ippo", nets)
    assert module.head_mode and all(p.head_mode for p in module.policies) and cfg.use_kl_loss
    batches = [_batch(cfg, module, 2), _batch(cfg, module, 3)]
    multi, _, _ = _two_updates(module, cfg, batches, fused_loss=True, fused_multi_loss=True, fused_multi=True)
    assert counted == {"single": 0, "multi": 2}
    single, _, _ = _two_updates(module, cfg, batches, fused_loss=True, fused_multi=True)
    assert counted == {"single": 2 * W3, "multi": 2}
    _assert_same_bits(multi, single)


def test_shared_module_keeps_the_single_call(counted):
    cfg, module = _module(*NETS["ippo"], sharing=True, W=2)
    batches = [_batch(cfg, module, 2), _batch(cfg, module, 3)]
    on, _, learner = _two_updates(module, cfg, batches, fused_loss=True, fused_multi_loss=True)
    assert learner.fused_multi_loss is True and counted == {"single": 2, "multi": 0}
    off, _, _ = _two_updates(module, cfg, batches, fused_loss=True)
    assert counted == {"single": 4, "multi": 0}
    _assert_same_bits(on, off)


def _hand_step(module, cfg, batch, rows, **switches):
    """One minibatch_step called by hand on the given rows: (statistics, KL sums, gradients, parameters, Adam state)."""
    from marlsc.ppo import PPOLearner
    m = copy.deepcopy(module)
    learner = PPOLearner(m, cfg, seed=5, **switches)
    learner.kl_coeffs = list(KL0)
    obs = batch["obs"]
    S, W = obs.shape[:2]
    flat = {k: v.reshape(S * W, *v.shape[2:]) for k, v in batch.items() if k != "obs"}
    stats = learner.new_stats(obs.device)
    learner.minibatch_step(obs, None, flat, rows, stats)
    out, kl_sum = stats.result(1)
    return [((out, kl_sum),) + _snapshot(m, learner)]


@pytest.mark.parametrize("fused_multi", [False, True], ids=["stack_path", "stacked_path"])
def test_unequal_row_counts_keep_the_single_calls(fused_multi, counted):
    cfg, module = _module(*NETS["ippo"])
    batch = _batch(cfg, module, 2)
    base = torch.arange(S_, device="cuda") * W3
    sw = dict(fused_loss=True, fused_mlp=True, fused_multi=fused_multi)
    ragged = [base[:40], base[:40] + 1, base[:33] + 2]
    on = _hand_step(module, cfg, batch, ragged, fused_multi_loss=True, **sw)
    assert counted == {"single": W3, "multi": 0}
    off = _hand_step(module, cfg, batch, ragged, **sw)
    assert counted == {"single": 2 * W3, "multi": 0}
    _assert_same_bits(on, off)
    equal = [base[5:45], base[:40] + 1, base[24:] + 2]  # equal lengths by hand: the multi call, the same bits
    on = _hand_step(module, cfg, batch, equal, fused_multi_loss=True, **sw)
    assert counted == {"single": 2 * W3, "multi": 1}
    off = _hand_step(module, cfg, batch, equal, **sw)
    assert counted == {"single": 3 * W3, "multi": 1}
    _assert_same_bits(on, off)


def test_without_fused_loss_the_switch_is_a_no_op(counted):
    cfg, module = _module(*NETS["ippo"])
    batches = [_batch(cfg, module, 2), _batch(cfg, module, 3)]
    on, _, learner = _two_updates(module, cfg, batches, fused_multi_loss=True, fused_multi=True)
    assert learner.fused_multi_loss is True and learner.fused_loss is False
    off, _, _ = _two_updates(module, cfg, batches, fused_multi=True)
    assert counted == {"single": 0, "multi": 0}
    _assert_same_bits(on, off)


def test_the_switch_is_opt_in_and_needs_a_cuda_module(monkeypatch):
    from marlsc.ppo import PPOLearner, PPOTrainer
    cfg, module = _module(*NETS["ippo"])
    monkeypatch.delenv("MSC_FUSED_MULTI_LOSS", raising=False)
    assert PPOLearner(module, cfg).fused_multi_loss is False
    assert PPOLearner(module, cfg, fused_multi_loss=True).fused_loss is False  # a switch of its own
    monkeypatch.setenv("MSC_FUSED_MULTI_LOSS", "1")
    assert PPOLearner(module, cfg).fused_multi_loss is True
    assert PPOLearner(module, cfg, fused_multi_loss=False).fused_multi_loss is False
    assert inspect.signature(PPOTrainer.__init__).parameters["fused_multi_loss"].default is None
    cpu = copy.deepcopy(module).cpu()
    with pytest.raises(RuntimeError, match=r"PPOLearner\(fused_multi_loss=True\): the multi-policy PPO loss is a HIP kernel"):
        PPOLearner(cpu, cfg, fused_multi_loss=True)
    with pytest.raises(RuntimeError, match=r"PPOLearner\(fused_multi_loss=True\)"):
        PPOLearner(cpu, cfg)  # from the environment
