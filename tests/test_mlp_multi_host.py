"""Host tests of the multi-policy MLP path (marlsc/mlp.py: multi_layers, pack_multi, multi_pack; the
argument checks of msc_mlp{2,3}_relu_multi): the stacked pack is the per-policy packs concatenated,
unsupported policy sets are refused, the pack cache follows every policy's weight versions, and the
switch defaults to off. The kernels themselves are tested on the GPU (tests/test_gpu_mlp_multi_exact.py)."""
import ctypes as C

import pytest
import torch
import torch.nn as nn

from marlsc import abi
from marlsc import mlp as M
from marlsc.rollout import MLP, RolloutConfig


def _nets(P, L, hidden, KO, **kw):
    torch.manual_seed(P + L + KO)
    return [list(MLP(L, KO, {"hidden_sizes": list(hidden), **kw})) for _ in range(P)]


@pytest.mark.parametrize("layout", [0, 1])
@pytest.mark.parametrize("P,L,hidden,KO", [(3, 7, (64, 128), 5), (2, 34, (96,), 1), (16, 9, (64, 64), 8)])
def test_stacked_pack_is_the_concatenation_of_the_single_policy_packs(P, L, hidden, KO, layout):
    nets = _nets(P, L, hidden, KO)
    w1s = [m[0].weight for m in nets]
    w2s = [m[2].weight for m in nets] if len(hidden) == 2 else None
    w3s = [m[-1].weight for m in nets]
    got = M.pack_multi(w1s, w2s, w3s, layout)
    for p in range(P):
        want = M.pack_mlp3(w1s[p], None if w2s is None else w2s[p], w3s[p], layout)
        for g, w in zip(got, want):
            assert (g is None) == (w is None)
            if g is not None:
                assert g.shape[0] == P and g.is_contiguous() and torch.equal(g[p].reshape(-1), w.reshape(-1))
    # consecutive single-policy packs, as the C ABI takes them
    assert torch.equal(got[0].reshape(-1), torch.cat([M.pack_mlp3(w1s[p], None if w2s is None else w2s[p], w3s[p], layout)[0]
                                                      for p in range(P)]))


def test_multi_layers_accepts_equal_shapes_only():
    assert M.multi_layers(_nets(8, 34, (256, 256), 5)) == 3
    assert M.multi_layers(_nets(16, 34, (256,), 1)) == 2
    assert M.multi_layers(_nets(1, 34, (64, 64), 5)) == 3
    assert M.multi_layers(_nets(64, 3, (32,), 1)) == 2
    assert M.multi_layers(_nets(65, 3, (32,), 1)) == 0  # 1..64 policies
    assert M.multi_layers([]) == 0
    assert M.multi_layers(_nets(2, 34, (64, 64), 5) + _nets(1, 34, (64, 128), 5)) == 0   # mixed hidden sizes
    assert M.multi_layers(_nets(2, 34, (64, 64), 5) + _nets(1, 33, (64, 64), 5)) == 0    # mixed inputs
    assert M.multi_layers(_nets(2, 34, (64, 64), 5) + _nets(1, 34, (64, 64), 4)) == 0    # mixed outputs
    assert M.multi_layers(_nets(2, 34, (64, 64), 5) + _nets(1, 34, (64,), 5)) == 0       # mixed depth
    assert M.multi_layers(_nets(2, 34, (96, 96), 5)) == 0                                # no single-policy kernel
    assert M.multi_layers(_nets(2, 34, (64, 64), 5) + _nets(1, 34, (64, 64), 5, activation="tanh")) == 0
    nob = _nets(3, 34, (64, 64), 5)
    nob[2][2] = nn.Linear(64, 64, bias=False)
    assert M.multi_layers(nob) == 0                                                       # a bias-free Linear
    with pytest.raises(ValueError):
        M.multi_pack(nob)


def test_pack_cache_rebuilds_when_any_policy_changes_and_only_then():
    nets = _nets(3, 7, (64, 64), 5)
    first = M.multi_pack(nets)
    assert len(first) == 6 and first[3].shape == (3, 64) and first[5].shape == (3, 5)
    again = M.multi_pack(nets)
    assert all(a is b for a, b in zip(first, again))  # nothing changed: the cached tensors
    with torch.no_grad():
        nets[2][2].weight.mul_(2.0)  # policy 2's second layer
    third = M.multi_pack(nets)
    assert third[1] is not first[1]
    assert torch.equal(third[1][2], first[1][2] * 2.0) and torch.equal(third[1][:2], first[1][:2])
    assert all(a is b for a, b in zip(third, M.multi_pack(nets)))
    with torch.no_grad():
        nets[1][-1].bias.add_(1.0)  # a bias of policy 1: the stacked biases live under the same key
    fourth = M.multi_pack(nets)
    assert torch.equal(fourth[5][1], third[5][1] + 1.0) and torch.equal(fourth[5][0], third[5][0])
    # a first-layer view (the split critic's local columns) has a slot of its own
    local = M.multi_pack(nets, [m[0].weight[:, :4] for m in nets])
    assert local[0] is not fourth[0]
    assert torch.equal(local[0][1], M.pack_mlp3(nets[1][0].weight[:, :4], nets[1][2].weight, nets[1][-1].weight)[0])
    assert all(a is b for a, b in zip(fourth, M.multi_pack(nets)))
    assert all(a is b for a, b in zip(local, M.multi_pack(nets, [m[0].weight[:, :4] for m in nets])))


def test_multi_abi_rejects_bad_arguments_before_any_launch():
    L = abi.lib()
    p = C.c_void_p(256)  # never dereferenced: every call below fails validation first
    ep = lambda rows: C.byref(abi.MscGaussianEpilogue(p, rows, C.c_float(-3.5), p, p, p, p))  # noqa: E731
    f = lambda n=24, np_=3, h1=64, h2=64, ko=5, out=p, s=None: L.msc_mlp3_relu_multi(  # noqa: E731
        p, n, np_, 34, h1, h2, ko, p, p, p, p, p, p, out, None, s, None)
    g = lambda n=24, np_=3, h=96, ko=5, out=p, s=None: L.msc_mlp2_relu_multi(  # noqa: E731
        p, n, np_, 34, h, ko, p, p, p, p, out, None, s, None)
    for fn in (f, g):
        assert fn(n=25) == -1 and b"multiple" in L.msc_last_error()
        assert fn(np_=0) == -1 and b"n_policies" in L.msc_last_error()
        assert fn(n=130, np_=65) == -1 and b"n_policies" in L.msc_last_error()
        assert fn(s=ep(2)) == -1 and b"log_std_rows" in L.msc_last_error()
        assert fn(ko=9, s=ep(3)) == -1 and b"VALU output layer" in L.msc_last_error()
        assert fn(ko=33) == -1 and b"out_dim" in L.msc_last_error()
        assert fn(out=None) == -1 and b"null" in L.msc_last_error()
    assert f(h1=48) == -1 and b"hidden sizes" in L.msc_last_error()
    assert f(h2=0) == -1
    assert g(h=48) == -1 and b"hidden size" in L.msc_last_error()
    q = C.c_void_p(260)  # a misaligned bias
    assert L.msc_mlp2_relu_multi(p, 24, 3, 34, 96, 5, p, q, p, p, p, None, None, None) == -1
    assert b"aligned" in L.msc_last_error()


def test_switch_is_off_by_default_and_passed_through(monkeypatch):
    from marlsc.ppo import MultiAgentActorCritic
    monkeypatch.delenv("MSC_MULTI_MLP", raising=False)
    rc = RolloutConfig(actor={"hidden_sizes": [64]}, critic={"hidden_sizes": [64]}, critic_obs_type="local")
    assert MultiAgentActorCritic(2, 7, 14, 2, rc, False).multi_mlp is False
    assert MultiAgentActorCritic(2, 7, 14, 2, rc, False, multi_mlp=True).multi_mlp is True
    monkeypatch.setenv("MSC_MULTI_MLP", "1")
    assert MultiAgentActorCritic(2, 7, 14, 2, rc, False).multi_mlp is True
    assert MultiAgentActorCritic(2, 7, 14, 2, rc, False, multi_mlp=False).multi_mlp is False
    # on the CPU (and under autograd) the switch changes nothing: the torch layers run
    on = MultiAgentActorCritic(2, 7, 14, 2, rc, False, multi_mlp=True)
    obs = torch.randn(5, 2, 7)
    with torch.no_grad():
        want = torch.stack([p.critic(obs[:, w]).squeeze(-1) for w, p in enumerate(on.policies)], dim=-1)
        assert torch.equal(on.values(obs), want)
        assert on.actor_sample_x(obs, None) is False
