"""GPU tests of the learner's fused clip + Adam step on real-valued data (marlsc/optim.py:FusedClipAdam,
PPOLearner(fused_opt=True)) against a float64 copy of the module.

The criterion is the project's error quotient (tests/test_gpu_mlp_backward.py, restated in _Errors): per
parameter tensor, the fused path's error of the updated parameters against the float64 copy, as the root of the
summed squared differences over N_BATCHES = 32 independent batches, is at most twice the torch float32 path's
(clip_grad_norm_ per policy + torch.optim.Adam), and every single batch's fused error is at most twice the
largest single-batch error of the torch path. Both float32 paths run the same forward and backward on the same
bits, so they hand the same gradients to the two optimizers and whatever a ReLU kink or a gradient near zero
does against float64, it does to both alike. Every learner takes two updates (on two batches) and the criterion
holds after each: the first Adam step does not depend on the scale of the gradient, so the clip coefficient
and the state carried over show in the second. grad_clip = 0.5 binds on these batches (the norms are 1 to 10);
the exact tests (tests/test_gpu_adam_exact.py) hold both sides of the clip."""
import copy
from collections import defaultdict
from pathlib import Path

import numpy as np
import pytest
import torch
import torch.nn as nn
import yaml

pytestmark = pytest.mark.gpu
REPO = Path(__file__).resolve().parents[1]
N_BATCHES = 32
L_, K_, S_ = 7, 3, 48
GRU_T, GRU_E = 6, 8  # rollout steps x envs of the GRU case: 48 env rows, sequences of max_seq_len = 2


class _Errors:
    """Squared errors of two float32 paths against float64, per tensor, over the batches."""

    def __init__(self):
        self.sf, self.st, self.mf, self.mt = defaultdict(float), defaultdict(float), defaultdict(float), defaultdict(float)
        self.n = 0

    def add(self, fused, torch32, ref64):
        assert fused.keys() == torch32.keys() == ref64.keys()
        for k, r in ref64.items():
            r = r.double().cpu()
            ef, et = fused[k].double().cpu() - r, torch32[k].double().cpu() - r
            self.sf[k] += float(ef.pow(2).sum())
            self.st[k] += float(et.pow(2).sum())
            self.mf[k], self.mt[k] = max(self.mf[k], float(ef.norm())), max(self.mt[k], float(et.norm()))
        self.n += 1

    def check(self, name):
        assert self.n == N_BATCHES
        worst = max((self.sf[k] ** 0.5 / self.st[k] ** 0.5 if self.st[k] > 0 else 0.0) for k in self.sf)
        print(f"{name}: {len(self.sf)} tensors, largest quotient fused / torch-f32 {worst:.3f}")
        for k in self.sf:
            ef, et = self.sf[k] ** 0.5, self.st[k] ** 0.5
            assert ef <= 2.0 * et, (name, k, ef, et)
            assert self.mf[k] <= 2.0 * self.mt[k], (name, k, self.mf[k], self.mt[k])


def _mlp(hidden):
    return {"type": "mlp", "config": {"hidden_sizes": list(hidden), "activation": "relu"}}


GRU = {"type": "gru", "config": {"num_layers": 1, "hidden_size": 32, "bidirectional": False, "max_seq_len": 2, "output_dim": 32}}
SMALL = {"shared_layers": None, "actor": _mlp([32]), "critic": _mlp([32]), "use_mu_sigma_head": False}
CASES = {  # algo yaml, parameter sharing, networks (None: the yaml's own), KL term
    "shared_ippo": dict(algo="ippo", sharing=True, nets=None, kl=False),
    "per_agent": dict(algo="ippo", sharing=False, nets=SMALL, kl=False),
    "mappo_kl": dict(algo="mappo", sharing=True, nets=None, kl=True),
    "mu_sigma": dict(algo="ippo", sharing=True, nets=dict(SMALL, use_mu_sigma_head=True), kl=False),
    "gru_trunk": dict(algo="ippo", sharing=True, nets=dict(SMALL, shared_layers=GRU), kl=False),
    "cppo": dict(algo="cppo", sharing=False, nets=SMALL, kl=True),
}


def _case(case, W=2, learning_rate=1e-3):
    """(cfg, module on the CPU)"""
    from marlsc.cppo import CentralizedActorCritic, CPPOConfig
    from marlsc.ppo import MultiAgentActorCritic, PPOConfig
    c = CASES[case]
    raw = yaml.safe_load(open(REPO / f"config_files/algorithms/{c['algo']}.yaml"))
    raw["algorithm"]["algorithm_specific"].update(parameter_sharing=c["sharing"], use_kl_loss=c["kl"])
    if c["nets"] is not None:
        raw["algorithm"]["algorithm_specific"]["networks"] = c["nets"]
    raw["algorithm"]["shared"].update(num_epochs=1, num_minibatches=1, batch_size=1 << 20, learning_rate=learning_rate)
    cfg = (CPPOConfig if c["algo"] == "cppo" else PPOConfig).from_algorithm_config(raw)
    cfg.grad_clip = 0.5
    torch.manual_seed(3)
    if c["algo"] == "cppo":
        return cfg, CentralizedActorCritic(W * L_, W * K_, cfg.rollout_config())
    return cfg, MultiAgentActorCritic(W, L_, L_ * W, K_, cfg.rollout_config(), c["sharing"])


def _batch(cfg, m, seed):
    """A synthetic batch [S, W, ...] on the CPU for module m (actions around its own distribution)."""
    from marlsc.cppo import CentralizedActorCritic
    from marlsc.ppo import gaussian_logp
    g = torch.Generator().manual_seed(seed)
    r = lambda *s: torch.randn(s, generator=g)  # noqa: E731
    W = m.W
    L, K = (2 * L_, 2 * K_) if isinstance(m, CentralizedActorCritic) else (L_, K_)  # _case's W = 2 agents as one
    S = GRU_T * GRU_E if m.recurrent else S_
    obs = r(S, W, L)
    batch = {"obs": obs, "advantages": r(S, W), "value_targets": r(S, W)}
    if m.recurrent:
        batch["actions"], batch["logp"] = r(S, W, K), -3.0 + 0.1 * r(S, W)
        batch["seq"] = {"T": GRU_T, "E": GRU_E, "S": 2, "truncated": torch.zeros((GRU_T, GRU_E, W), dtype=torch.uint8),
                        "state_in": {k: 0.3 * r(GRU_T // 2, *h.shape) for k, h in m.initial_state(GRU_E, device="cpu").items()}}
        return batch
    full = torch.cat([obs, obs.reshape(S, 1, W * L).expand(S, W, W * L)], -1)
    with torch.no_grad():
        mean, ls = m.dist_inputs(obs, full)
        ls = ls.contiguous()
        act = mean + ls.exp() * r(*mean.shape)
        batch["actions"], batch["logp"] = act, gaussian_logp(act, mean, ls) + 0.1 * r(S, W)
    if cfg.use_kl_loss:
        batch["mean_old"], batch["log_std_old"] = mean + 0.05, ls.clone()
    return batch


def _to(batch, f64, device):
    def conv(v):
        if isinstance(v, dict):
            return {k: conv(x) for k, x in v.items()}
        if not isinstance(v, torch.Tensor):
            return v
        return (v.double() if f64 and v.is_floating_point() else v).to(device)
    return conv(batch)


def _learner(module, cfg, *, fused_opt, f64=False, **kw):
    from marlsc.ppo import PPOLearner
    m = copy.deepcopy(module)
    m = m.double() if f64 else m.cuda()
    return PPOLearner(m, cfg, seed=5, fused_opt=fused_opt, **({} if f64 else kw))


def _params(learner):
    return {k: p.detach().clone() for k, p in learner.module.named_parameters()}


def _update(learner, batch, timestep=0):
    p = next(learner.module.parameters())
    out = learner.update(_to(batch, p.dtype == torch.float64, p.device), None, timestep)
    assert out["num_minibatch_steps"] == 1 and all(np.isfinite(v) for v in out.values())
    return out


def _quotient_over_two_updates(case, name, **switches):
    cfg, module = _case(case)
    errs = [_Errors(), _Errors()]
    for seed in range(N_BATCHES):
        learners = [_learner(module, cfg, fused_opt=True, **switches), _learner(module, cfg, fused_opt=False, **switches),
                    _learner(module, cfg, fused_opt=False, f64=True)]
        from marlsc.optim import FusedClipAdam
        assert isinstance(learners[0].opt, FusedClipAdam) and isinstance(learners[1].opt, torch.optim.Adam)
        for u in range(2):
            batch = _batch(cfg, module, 100 * seed + u)
            outs = [_update(ln, batch) for ln in learners]
            assert list(outs[0]) == list(outs[1]) and outs[0]["learning_rate"] == outs[1]["learning_rate"] == 1e-3
            errs[u].add(*[_params(ln) for ln in learners])
            # the clipped gradients are left in .grad by both paths (the fused one writes them back)
            for pol in learners[0].module.policies:
                n = float(torch.cat([p.grad.reshape(-1) for p in pol.parameters() if p.grad is not None]).norm())
                assert n <= 0.5 * (1 + 1e-5)
        moved = [k for k, p in learners[0].module.named_parameters() if not torch.equal(p.detach().cpu(), module.state_dict()[k])]
        assert len(moved) >= 4
    for u in range(2):
        errs[u].check(f"{name} update {u + 1}")


@pytest.mark.parametrize("case", list(CASES))
def test_fused_clip_adam_against_torch_and_a_float64_copy(case):
    _quotient_over_two_updates(case, case)


@pytest.mark.parametrize("fused_loss,fused_mlp", [(True, False), (False, True), (True, True)],
                         ids=["fused_loss", "fused_mlp", "fused_loss_and_mlp"])
def test_with_the_fused_loss_and_the_fused_mlp_backward(fused_loss, fused_mlp):
    _quotient_over_two_updates("per_agent", f"per_agent loss={fused_loss} mlp={fused_mlp}", fused_loss=fused_loss,
                               fused_mlp=fused_mlp)


def test_a_checkpoint_of_the_fused_state_resumes_in_torch_adam_within_the_quotient():
    """update 1 fused, its state_dict loaded by a torch.optim.Adam learner, update 2 there: against the float64
    copy's two updates that path's error is within twice the all-torch path's."""
    cfg, module = _case("shared_ippo")
    err = _Errors()
    for seed in range(N_BATCHES):
        fused, t32 = _learner(module, cfg, fused_opt=True), _learner(module, cfg, fused_opt=False)
        f64 = _learner(module, cfg, fused_opt=False, f64=True)
        b1, b2 = _batch(cfg, module, 100 * seed), _batch(cfg, module, 100 * seed + 1)
        for ln in (fused, t32, f64):
            _update(ln, b1)
        resumed = _learner(fused.module.cpu(), cfg, fused_opt=False)
        resumed.opt.load_state_dict(copy.deepcopy(fused.opt.state_dict()))
        for ln in (resumed, t32, f64):
            _update(ln, b2)
        err.add(_params(resumed), _params(t32), _params(f64))
    err.check("fused update, torch resume")


def test_a_parameter_without_a_gradient_is_left_alone_and_gets_no_state():
    cfg, module = _case("per_agent")
    module.policies[1].unused = nn.Parameter(torch.randn(5))
    names = [k for k, _ in module.named_parameters()]
    idx = names.index("policies.1.unused")
    batch = _batch(cfg, module, 1)
    for fused_opt in (True, False):
        ln = _learner(module, cfg, fused_opt=fused_opt)
        _update(ln, batch)
        versions = {k: p._version for k, p in ln.module.named_parameters()}
        _update(ln, _batch(cfg, module, 2))
        # the kernel writes through raw pointers and says so: what is cached per parameter version (the fused
        # kernels' weight packs) is rebuilt after a step
        assert all((p._version > versions[k]) == (k != "policies.1.unused") for k, p in ln.module.named_parameters())
        after = _params(ln)
        assert torch.equal(after["policies.1.unused"].cpu(), module.policies[1].unused.detach())
        assert ln.module.policies[1].unused.grad is None
        state = ln.opt.state_dict()["state"]
        assert sorted(state) == [i for i in range(len(names)) if i != idx], fused_opt
        assert all(float(st["step"]) == 2.0 for st in state.values())
        assert sum(not torch.equal(after[k].cpu(), p.detach()) for k, p in module.named_parameters()) == len(names) - 1


def test_learning_rate_schedule_reaches_the_kernel():
    cfg, module = _case("shared_ippo", learning_rate=[[0, 1e-3], [1000, 1e-4]])
    batch = _batch(cfg, module, 4)
    res = {}
    for t in (0, 500):
        for fused_opt in (True, False):
            ln = _learner(module, cfg, fused_opt=fused_opt)
            out = _update(ln, batch, timestep=t)
            assert out["learning_rate"] == cfg.lr_at(t) == {0: 1e-3, 500: 5.5e-4}[t]
            res[t, fused_opt] = _params(ln)
    k = "policies.0.actor.0.weight"
    p0 = module.state_dict()[k]
    step = {key: (v[k].cpu() - p0).abs().max().item() for key, v in res.items()}
    # the first Adam step moves every element with a gradient by its learning rate
    for fused_opt in (True, False):
        assert step[0, fused_opt] == pytest.approx(1e-3, rel=1e-3) and step[500, fused_opt] == pytest.approx(5.5e-4, rel=1e-3)
    assert not torch.equal(res[0, True][k], res[500, True][k])


def _trainer(fused_opt):
    from marlsc import make_synthetic_env_config
    from marlsc.ppo import PPOConfig, PPOTrainer
    raw = {"algorithm": {"name": "ippo",
                         "shared": {"num_epochs": 2, "num_minibatches": 2, "batch_size": 64, "learning_rate": 1e-3,
                                    "num_eval_episodes": 2},
                         "algorithm_specific": {"parameter_sharing": False, "grad_clip": 0.5, "networks": SMALL}}}
    cfg = PPOConfig.from_algorithm_config(raw)
    return PPOTrainer(make_synthetic_env_config(2, 4, 2, episode_length=6), cfg, root_seed=3, n_envs=16, rollout_len=4,
                      device=0, fused_opt=fused_opt)


def test_trainer_checkpoint_resumes_bit_equal_fused_and_runs_with_torch(tmp_path):
    from marlsc.optim import FusedClipAdam
    tr = _trainer(True)
    assert isinstance(tr.learner.opt, FusedClipAdam)
    tr.train_iteration()
    ck = tr.save_checkpoint(tmp_path / "ck")
    saved = torch.load(ck / "learner_state.pt", weights_only=True)["optimizer"]
    n_params = len(list(tr.module.parameters()))
    assert sorted(saved["state"]) == list(range(n_params)) and float(saved["state"][0]["step"]) == 4.0
    res_a = tr.train_iteration()
    tr2 = _trainer(True)
    tr2.load_checkpoint(ck)
    res_b = tr2.train_iteration()
    assert res_a == res_b
    for (k, a), (_, b) in zip(tr.module.named_parameters(), tr2.module.named_parameters()):
        assert torch.equal(a, b), k
    sa, sb = tr.learner.opt.state_dict()["state"], tr2.learner.opt.state_dict()["state"]
    assert all(torch.equal(sa[i]["exp_avg_sq"], sb[i]["exp_avg_sq"]) and float(sb[i]["step"]) == 8.0 for i in sa)
    tr3 = _trainer(False)  # the torch path from the fused checkpoint
    tr3.load_checkpoint(ck)
    res_c = tr3.train_iteration()
    assert res_c["learner/num_minibatch_steps"] == res_a["learner/num_minibatch_steps"]
    assert all(np.isfinite(v) for k, v in res_c.items() if k.startswith("learner/"))
    assert float(tr3.learner.opt.state_dict()["state"][0]["step"]) == 8.0
    for (k, a), (_, c) in zip(tr.module.named_parameters(), tr3.module.named_parameters()):
        # no float64 yardstick for a whole trainer (the quotient of this resume is the learner-level test above):
        # here only what Adam itself bounds, four steps of at most lr (1 - b1) / sqrt(1 - b2) per path
        assert float((a - c).detach().abs().max()) <= 2 * 4 * 1e-3 * 0.1 / (1 - 0.999) ** 0.5, k
    # ... and a torch checkpoint resumes in the fused path
    ck3 = tr3.save_checkpoint(tmp_path / "ck3")
    tr4 = _trainer(True)
    tr4.load_checkpoint(ck3)
    assert tr4.learner.opt._steps == [8] * n_params
    res_d = tr4.train_iteration()
    assert all(np.isfinite(v) for k, v in res_d.items() if k.startswith("learner/"))
    for tr_ in (tr, tr2, tr3, tr4):
        tr_.env.close()
