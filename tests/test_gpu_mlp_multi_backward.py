"""GPU tests of the learner's multi-policy path (PPOLearner(fused_multi=True): mlp.multi_train_forward, one
msc_mlp{3,2}_relu_multi launch forward and one msc_mlp_relu_backward_multi call backward per net kind) against
the per-policy path fused_mlp=True gives. Both promise the same bits -- the multi forward is bit-identical per
policy to the single-policy kernel, the multi backward to the single-policy call -- so every comparison here is
torch.equal: returned values, gradients, parameters and Adam moments after one update and after a second one.
Launches are counted through a proxy on abi.lib()."""
import copy

import pytest

torch = pytest.importorskip("torch")
import torch.nn as nn  # noqa: E402

from marlsc import mlp as M  # noqa: E402
from test_gpu_mlp_backward import GRU, K_, L_, S_, _mlp, _ppo_cfg, _torch_layer_calls  # noqa: E402

pytestmark = pytest.mark.gpu
W3 = 3
NETS = {  # name: (algorithm config, networks)
    "ippo": ("ippo", {"shared_layers": None, "actor": _mlp([32]), "critic": _mlp([32]), "use_mu_sigma_head": False}),
    "mappo": ("mappo", {"shared_layers": None, "actor": _mlp([32]), "critic": _mlp([64, 64]), "use_mu_sigma_head": False}),
}


@pytest.fixture
def counted(monkeypatch):
    """Counts the calls of the single-policy and of the multi-policy backward (the library handle marlsc.mlp uses)."""
    calls = {"single": 0, "multi": 0}
    lib = M.abi.lib()

    def counting(name, key):
        real = getattr(lib, name)

        def f(*a):
            calls[key] += 1
            return real(*a)
        return staticmethod(f)

    class Counting:
        msc_mlp_relu_backward = counting("msc_mlp_relu_backward", "single")
        msc_mlp_relu_backward_multi = counting("msc_mlp_relu_backward_multi", "multi")

        def __getattr__(self, name):
            return getattr(lib, name)
    proxy = Counting()
    monkeypatch.setattr(M.abi, "lib", lambda: proxy)
    return calls


def _module(algo, nets, *, sharing=False, W=W3, kl=True):
    from marlsc.ppo import MultiAgentActorCritic
    cfg = _ppo_cfg(algo, parameter_sharing=sharing, use_kl_loss=kl, networks=nets)
    cfg.grad_clip = 0.5
    torch.manual_seed(3)
    return cfg, MultiAgentActorCritic(W, L_, L_ * W, K_, cfg.rollout_config(), sharing).cuda()


def _batch(cfg, m, seed=2):
    from marlsc.ppo import gaussian_logp
    g = torch.Generator(device="cuda").manual_seed(seed)
    r = lambda *s: torch.randn(s, device="cuda", generator=g)  # noqa: E731
    W = m.W
    obs = r(S_, W, L_)
    full = torch.cat([obs, obs.reshape(S_, 1, W * L_).expand(S_, W, W * L_)], -1)
    with torch.no_grad():
        mean, ls = m.dist_inputs(obs, full)
        ls = ls.contiguous()
        act = mean + ls.exp() * r(*mean.shape)
    batch = {"obs": obs, "actions": act, "logp": gaussian_logp(act, mean, ls) + 0.1 * r(S_, W),
             "advantages": r(S_, W), "value_targets": r(S_, W)}
    if cfg.use_kl_loss:
        batch["mean_old"], batch["log_std_old"] = mean + 0.05, ls.clone()
    return batch


def _two_updates(module, cfg, batches, **switches):
    """Two updates of a deep copy: [(returned values, gradients, parameters, Adam state) after each], torch-layer calls."""
    from marlsc.ppo import PPOLearner
    m = copy.deepcopy(module)
    hooks = _torch_layer_calls(m)
    learner = PPOLearner(m, cfg, seed=5, **switches)
    res = []
    for b in batches:
        out = learner.update(b, None, 0)
        assert out["num_minibatch_steps"] == 1
        state = learner.opt.state_dict()["state"]
        res.append((out, {k: p.grad.detach().clone() for k, p in m.named_parameters() if p.grad is not None},
                    {k: p.detach().clone() for k, p in m.named_parameters()},
                    {(i, k): v.detach().clone() for i, s in state.items() for k, v in s.items() if torch.is_tensor(v)}))
    return res, hooks["n"], learner


def _assert_same_bits(a, b):
    assert len(a) == len(b)
    for (oa, ga, pa, sa), (ob, gb, pb, sb) in zip(a, b):
        assert oa == ob
        for da, db in ((ga, gb), (pa, pb), (sa, sb)):
            assert da.keys() == db.keys() and len(da) > 0
            for k in da:
                assert torch.equal(da[k], db[k]), k


@pytest.mark.parametrize("fused_opt", [False, True], ids=["torch_adam", "fused_opt"])
@pytest.mark.parametrize("fused_loss", [False, True], ids=["torch_loss", "fused_loss"])
@pytest.mark.parametrize("case", list(NETS))
def test_two_updates_equal_the_per_policy_path_bit_for_bit(case, fused_loss, fused_opt, counted):
    cfg, module = _module(*NETS[case])
    if case == "mappo":
        assert cfg.use_kl_loss and module.policies[0].critic[0].in_features == (W3 + 1) * L_
    batches = [_batch(cfg, module, 2), _batch(cfg, module, 3)]
    sw = dict(fused_loss=fused_loss, fused_opt=fused_opt, fused_mlp=True)
    multi, torch_calls, learner = _two_updates(module, cfg, batches, fused_multi=True, **sw)
    # two multi calls per step (actors, critics), no single-policy call, no torch layer
    assert counted == {"single": 0, "multi": 2 * 2} and torch_calls == 0
    assert all(p.grad is not None and p.grad.is_contiguous() and p.grad.shape == p.shape for p in learner.module.parameters())
    single, torch_calls, _ = _two_updates(module, cfg, batches, **sw)
    assert counted == {"single": 2 * 2 * W3, "multi": 2 * 2} and torch_calls == 0
    _assert_same_bits(multi, single)
    assert not torch.equal(multi[0][2]["policies.0.actor.0.weight"], multi[1][2]["policies.0.actor.0.weight"])


def test_without_fused_mlp_the_switch_alone_takes_the_multi_path(counted):
    """fused_multi is a switch of its own: it does not need fused_mlp, and gives the same bits with it."""
    cfg, module = _module(*NETS["ippo"])
    batches = [_batch(cfg, module, 2)]
    alone, torch_calls, _ = _two_updates(module, cfg, batches, fused_multi=True)
    assert counted == {"single": 0, "multi": 2} and torch_calls == 0
    both, _, _ = _two_updates(module, cfg, batches, fused_multi=True, fused_mlp=True)
    _assert_same_bits(alone, both)


def test_fused_mlp_alone_makes_no_multi_call(counted, monkeypatch):
    monkeypatch.delenv("MSC_FUSED_MULTI_GRAD", raising=False)
    cfg, module = _module(*NETS["ippo"])
    _, torch_calls, learner = _two_updates(module, cfg, [_batch(cfg, module, 2)], fused_mlp=True)
    assert learner.fused_multi is False
    assert counted == {"single": 2 * W3, "multi": 0} and torch_calls == 0  # one call per network, as before


@pytest.mark.parametrize("kind", ["shared", "mu_sigma", "gru_trunk"])
def test_the_switch_is_a_no_op_where_it_does_not_apply(kind, counted):
    nets = {"shared_layers": GRU if kind == "gru_trunk" else None, "actor": _mlp([32]), "critic": _mlp([32]),
            "use_mu_sigma_head": kind == "mu_sigma"}
    cfg, m = _module("ippo", nets, sharing=kind == "shared", W=2, kl=False)
    if kind == "gru_trunk":
        g = torch.Generator(device="cuda").manual_seed(2)
        r = lambda *s: torch.randn(s, device="cuda", generator=g)  # noqa: E731
        T, E = 6, 9
        seq = {"T": T, "E": E, "S": 2, "truncated": torch.zeros((T, E, 2), dtype=torch.uint8, device="cuda"),
               "state_in": {k: 0.3 * r(T // 2, *h.shape) for k, h in m.initial_state(E, device="cuda").items()}}
        batch = {"obs": r(T * E, 2, L_), "actions": r(T * E, 2, K_), "logp": -3.0 + 0.1 * r(T * E, 2),
                 "advantages": r(T * E, 2), "value_targets": r(T * E, 2), "seq": seq}
    else:
        batch = _batch(cfg, m)
    on, calls_on, _ = _two_updates(m, cfg, [batch], fused_mlp=True, fused_multi=True)
    assert counted["multi"] == 0
    single_on = counted["single"]
    off, calls_off, _ = _two_updates(m, cfg, [batch], fused_mlp=True)
    assert counted == {"single": 2 * single_on, "multi": 0} and calls_on == calls_off
    _assert_same_bits(on, off)


def test_actors_through_the_multi_call_critics_through_their_own_path(counted):
    """Critic hidden [48, 48] is outside the two-hidden-layer set: the critics keep the torch layers (what
    fused_mlp gives them), the actors take the multi call."""
    nets = {"shared_layers": None, "actor": _mlp([32]), "critic": _mlp([48, 48]), "use_mu_sigma_head": False}
    cfg, module = _module("mappo", nets)
    assert M.multi_trainable([p.actor for p in module.policies])
    assert not M.multi_trainable([p.critic for p in module.policies])
    batches = [_batch(cfg, module, 2), _batch(cfg, module, 3)]
    mixed, calls_mixed, _ = _two_updates(module, cfg, batches, fused_mlp=True, fused_multi=True)
    assert counted == {"single": 0, "multi": 2} and calls_mixed == 2 * 3 * W3  # the critics' three Linears per step
    single, calls_single, _ = _two_updates(module, cfg, batches, fused_mlp=True)
    assert counted == {"single": 2 * W3, "multi": 2} and calls_single == calls_mixed
    _assert_same_bits(mixed, single)


@pytest.mark.parametrize("hidden", [(32,), (64, 64)], ids=["32", "64x64"])
def test_multi_train_forward_alone(hidden):
    from marlsc.rollout import MLP
    P, n, L, KO = 3, 33, 7, 3
    torch.manual_seed(1)
    nets = [MLP(L, KO, {"hidden_sizes": list(hidden)}).cuda() for _ in range(P)]
    assert M.multi_trainable(nets)
    x = torch.randn(n, P, L, device="cuda")
    y = M.multi_train_forward(nets, x)
    assert y.requires_grad and y.shape == (n, P, KO)
    assert torch.equal(y.detach(), M.multi_forward([list(m) for m in nets], x))
    for p, net in enumerate(nets):  # and the single-policy train_forward's bits on the policy's rows
        assert torch.equal(y.detach()[:, p], M.train_forward(net, x[:, p].contiguous()).detach())
    d = torch.randn(n, P, KO, device="cuda")
    (y * d).sum().backward()
    params = [p for net in nets for p in net.parameters()]
    assert len(params) == P * 2 * (len(hidden) + 1)
    for p in params:
        assert p.grad is not None and p.grad.shape == p.shape and p.grad.is_contiguous() and float(p.grad.abs().max()) > 0
    for p, net in enumerate(nets):  # the gradients are the single-policy call's, bit for bit
        want = M.mlp_backward(list(net), x[:, p].contiguous(), d[:, p].contiguous())
        for q, w in zip(net.parameters(), want):
            assert torch.equal(q.grad, w)
    with pytest.raises(RuntimeError, match="multi_train_forward: x must be torch.float32"):
        M.multi_train_forward(nets, x.double())
    with pytest.raises(RuntimeError, match="computes none for its input"):
        M.multi_train_forward(nets, x.clone().requires_grad_())
    with pytest.raises(ValueError, match="no multi-policy kernel"):
        M.multi_train_forward([nn.Sequential(nn.Linear(7, 30), nn.ReLU(), nn.Linear(30, 3)).cuda()] * 2, x[:, :2].contiguous())
    stacked = [torch.zeros((P,) + tuple(q.shape), device="cuda") for q in nets[0].parameters()]
    views = M.multi_backward(nets, x, d, scale=0.5, grads=stacked)  # adds to the given stacked tensors
    for p, net in enumerate(nets):
        for v, t, q in zip(views[p], stacked, net.parameters()):
            assert v.data_ptr() == t[p].data_ptr() and torch.equal(v, 0.5 * q.grad)
