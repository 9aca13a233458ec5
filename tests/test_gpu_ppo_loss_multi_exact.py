"""GPU tests of the multi-policy PPO loss (csrc/ppo_loss.hip: msc_ppo_loss_multi, marlsc/ppo_loss.py:
multi_ppo_loss_launch / fused_ppo_loss_multi) against the single-policy msc_ppo_loss, which
tests/test_gpu_ppo_loss.py pins to the float64 yardstick. The promise is "per policy bit for bit msc_ppo_loss",
so the comparisons are torch.equal: policy p's totals[p], stats[p] and slices of the three gradients against the
single call on policy p's contiguous slices with kl_coeffs[p]. Inputs: ppo_loss_emulation.make_inputs, one seed
per policy, interleaved into one flat batch at rows s P + p."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import ppo_loss_emulation as em

pytestmark = pytest.mark.gpu
P_MAX = 8
COMBOS = [(use_kl, beta) for use_kl in (False, True) for beta in (None, 0.3)]


def _kl(P):
    return [0.05 + 0.11 * p for p in range(P)]  # distinct per policy


def _dev(x, dtype=torch.float32):
    return torch.tensor(np.asarray(x), dtype=dtype, device="cuda")


@functools.lru_cache(maxsize=None)
def _policy(n, K, shared, seed):
    """Policy `seed`'s inputs on the device: (mean [n, K], log_std [K] | [n, K], values [n], batch columns [n, ..])."""
    inp = em.make_inputs(n, K, shared=shared, seed=10 + seed)  # the batch does not depend on use_kl / beta
    return inp, _dev(inp["mean"]), _dev(inp["log_std"]), _dev(inp["values"]), {k: _dev(v) for k, v in inp["batch"].items()}


def _stacked(n, K, shared, P):
    """The P policies' operands stacked for the multi call, and the batch interleaved at rows s P + p."""
    pol = [_policy(n, K, shared, p) for p in range(P)]
    mean = torch.stack([q[1] for q in pol], dim=1).contiguous()                       # [n, P, K]
    log_std = torch.stack([q[2] for q in pol], dim=0 if shared else 1).contiguous()  # [P, K] | [n, P, K]
    values = torch.stack([q[3] for q in pol], dim=1).contiguous()                     # [n, P]
    flat = {k: torch.stack([q[4][k] for q in pol], dim=1).reshape(n * P, *pol[0][4][k].shape[1:]).contiguous()
            for k in pol[0][4]}
    return mean, log_std, values, flat


def _single(cfg, n, K, shared, p, kl_coeff, stats=None):
    from marlsc.ppo_loss import ppo_loss_launch
    _, mean, log_std, values, batch = _policy(n, K, shared, p)
    return ppo_loss_launch(cfg, mean, log_std, values, batch, None, kl_coeff, stats)


def _multi(cfg, ops, kl, idx=None, stats=None):
    from marlsc.ppo_loss import multi_ppo_loss_launch
    mean, log_std, values, flat = ops
    return multi_ppo_loss_launch(cfg, mean, log_std, values, flat, idx, kl, stats)


def _assert_equals_singles(multi, singles, shared, what):
    """multi: the multi call's five outputs; singles: per policy the single call's five outputs."""
    totals, stats, gm, gl, gv = multi
    want = (torch.cat([s[0] for s in singles]), torch.stack([s[1] for s in singles]),
            torch.stack([s[2] for s in singles], dim=1), torch.stack([s[3] for s in singles], dim=0 if shared else 1),
            torch.stack([s[4] for s in singles], dim=1))
    for name, got, w in zip(em.OUTPUTS, (totals, stats, gm, gl, gv), want):
        assert got.shape == w.shape and got.dtype == w.dtype, (what, name)
        assert torch.equal(got, w), (what, name)


@pytest.mark.parametrize("K", em.KS)
def test_every_policy_has_the_single_calls_bits(K):
    """P in {1, 2, 3, 8}, shared and per-row log_std, KL on and off, beta 1 and 0.3, n around the block geometry:
    one row, one less and one more than a block, several blocks with a ragged tail."""
    from marlsc.ppo_loss import grid_blocks, rows_per_block
    rpb = rows_per_block(K)
    ns = sorted({1, rpb - 1, rpb + 1, 3 * rpb + 1})
    assert grid_blocks(rpb - 1, K) == 1 and grid_blocks(rpb + 1, K) == 2 and grid_blocks(3 * rpb + 1, K) == 4
    kl = _kl(P_MAX)
    for n in ns:
        for shared in (False, True):
            for use_kl, beta in COMBOS:
                cfg = em.make_cfg(use_kl=use_kl, beta=beta)
                singles = [_single(cfg, n, K, shared, p, kl[p]) for p in range(P_MAX)]
                for P in (1, 2, 3, 8):
                    multi = _multi(cfg, _stacked(n, K, shared, P), kl[:P])
                    _assert_equals_singles(multi, singles[:P], shared, (n, K, P, shared, use_kl, beta))
                if use_kl:  # the coefficients are in play: policy 1 with policy 0's coefficient differs
                    assert not torch.equal(singles[1][0], _single(cfg, n, K, shared, 1, kl[0])[0])
    _policy.cache_clear()


def test_sixty_four_policies():
    from marlsc.ppo_loss import MAX_POLICIES, rows_per_block
    from marlsc.mlp import MULTI_MAX_POLICIES
    assert MAX_POLICIES == MULTI_MAX_POLICIES == 64
    K, P = 5, 64
    n = rows_per_block(K) + 1
    kl = _kl(P)
    cfg = em.make_cfg(use_kl=True, beta=0.3)
    for shared in (False, True):
        singles = [_single(cfg, n, K, shared, p, kl[p]) for p in range(P)]
        _assert_equals_singles(_multi(cfg, _stacked(n, K, shared, P), kl), singles, shared, (P, shared))
    _policy.cache_clear()


@pytest.mark.parametrize("K,blocks_worth", [(128, 4), (5, 32)])
def test_grid_stride_loop_past_the_grid_cap(K, blocks_worth):
    """n past 2048 blocks' worth of rows with P = 2: every block's grid-stride loop runs more than once."""
    from marlsc.ppo_loss import grid_blocks, rows_per_block
    assert rows_per_block(K) == blocks_worth
    n = 2048 * blocks_worth + (5 if K == 128 else 7)
    assert grid_blocks(n, K) == 2048 == grid_blocks(10 ** 9, K)
    kl = _kl(2)
    cfg = em.make_cfg(use_kl=True, beta=0.3)
    for shared in (False, True):
        singles = [_single(cfg, n, K, shared, p, kl[p]) for p in range(2)]
        _assert_equals_singles(_multi(cfg, _stacked(n, K, shared, 2), kl), singles, shared, (n, K, shared))
    _policy.cache_clear()


def test_idx_forms():
    """NULL is idx[i][p] = i P + p; arbitrary columns (repeats, two policies on the same batch rows) are the single
    call with that column; a permutation equals a torch gather of the batch."""
    from marlsc.ppo_loss import ppo_loss_launch, rows_per_block
    K, P = 5, 3
    n = 3 * rows_per_block(K) + 1
    kl = _kl(P)
    g = torch.Generator().manual_seed(4)
    for shared in (False, True):
        cfg = em.make_cfg(use_kl=True, beta=0.3)
        ops = _stacked(n, K, shared, P)
        mean, log_std, values, flat = ops
        plain = _multi(cfg, ops, kl)
        explicit = _multi(cfg, ops, kl, idx=torch.arange(n * P, device="cuda").reshape(n, P))
        for a, b in zip(plain, explicit):
            assert torch.equal(a, b)
        idx = torch.randint(0, n * P, (n, P), generator=g)
        idx[n // 2:, 0] = idx[:n - n // 2, 0]  # repeats inside one policy's column
        idx[:, 1] = idx[:, 0]                  # two policies on the same batch rows
        idx = idx.cuda()
        assert idx[:, 0].unique().numel() < n
        got = _multi(cfg, ops, kl, idx=idx)
        singles = [ppo_loss_launch(cfg, mean[:, p].contiguous(), log_std[p] if shared else log_std[:, p].contiguous(),
                                   values[:, p].contiguous(), flat, idx[:, p].contiguous(), kl[p]) for p in range(P)]
        _assert_equals_singles(got, singles, shared, ("columns", shared))
        assert not torch.equal(got[2], plain[2])
        perm = torch.randperm(n * P, generator=g).cuda().reshape(n, P)
        assert not torch.equal(perm, torch.arange(n * P, device="cuda").reshape(n, P))
        gathered = _multi(cfg, (mean, log_std, values, {k: v[perm.reshape(-1)] for k, v in flat.items()}), kl)
        for a, b in zip(_multi(cfg, ops, kl, idx=perm), gathered):
            assert torch.equal(a, b)
    _policy.cache_clear()


def test_repeated_calls_give_equal_bits_and_accumulate_adds_in_f64_per_policy():
    from marlsc.ppo_loss import rows_per_block
    K, P = 17, 3
    n = 3 * rows_per_block(K) + 1
    kl = _kl(P)
    cfg = em.make_cfg(use_kl=True)
    for shared in (False, True):
        ops = _stacked(n, K, shared, P)
        first = _multi(cfg, ops, kl)
        for _ in range(3):
            for a, b in zip(first, _multi(cfg, ops, kl)):
                assert torch.equal(a, b)
        start = torch.arange(P * 5, dtype=torch.float64, device="cuda").reshape(P, 5) / 7.0 - 1.0
        acc = start.clone()
        out = _multi(cfg, ops, kl, stats=acc)
        assert out[1].data_ptr() == acc.data_ptr()
        assert torch.equal(acc, start + first[1]) and not torch.equal(acc, first[1])
        _multi(cfg, ops, kl, stats=acc)
        assert torch.equal(acc, (start + first[1]) + first[1])
        for a, b in zip(first[2:], out[2:]):  # the gradients and totals do not depend on it
            assert torch.equal(a, b)
        assert torch.equal(first[0], out[0])
    _policy.cache_clear()


@pytest.mark.parametrize("K", [5, 65])
def test_every_output_within_the_bound_of_the_f64_yardstick(K):
    """One check that does not go through msc_ppo_loss: ppo_loss in float64 per policy, P = 3, every output within
    ppo_loss_emulation.bounds."""
    from marlsc.ppo_loss import rows_per_block
    P = 3
    n = 3 * rows_per_block(K) + 1
    kl = _kl(P)
    cfg = em.make_cfg(use_kl=True, beta=0.3)
    for shared in (False, True):
        totals, stats, gm, gl, gv = (t.double().cpu().numpy() for t in _multi(cfg, _stacked(n, K, shared, P), kl))
        for p in range(P):
            inp = _policy(n, K, shared, p)[0]
            got = {"total": totals[p], "stats": stats[p], "grad_mean": gm[:, p], "grad_log_std": gl[p] if shared else gl[:, p],
                   "grad_values": gv[:, p]}
            ob = em.over_bound(got, em.run_torch(cfg, inp, kl[p]), em.bounds(cfg, inp, kl[p]))
            print(f"K {K} shared {shared} policy {p}: max error/bound " + " ".join(f"{k} {v:.3f}" for k, v in ob.items()))
            assert max(ob.values()) <= 1.0, (K, shared, p, ob)
    _policy.cache_clear()


def _leaves(n, K, shared, P):
    mean, log_std, values, flat = _stacked(n, K, shared, P)
    return mean.clone().requires_grad_(), log_std.clone().requires_grad_(), values.clone().requires_grad_(), flat


@pytest.mark.parametrize("P", [1, 3, 8, 64])
def test_total_is_the_sum_of_the_totals(P):
    """total against sum_p totals[p] formed in float64: at most P float32 additions, each within 2^-24 of a partial
    sum that is at most sum |totals[p]| in magnitude."""
    from marlsc.ppo_loss import fused_ppo_loss_multi
    K, n = 5, 40
    kl = _kl(P)
    cfg = em.make_cfg(use_kl=True)
    ops = _stacked(n, K, True, P)
    total, stats = fused_ppo_loss_multi(cfg, *ops[:3], ops[3], None, kl)
    totals, want_stats = _multi(cfg, ops, kl)[:2]
    assert total.shape == () and total.dtype == torch.float32
    assert stats.shape == (P, 5) and torch.equal(stats, want_stats)  # added to a zeroed buffer
    t64 = totals.double()
    err = abs(float(total.double() - t64.sum()))
    bound = P * 2.0 ** -24 * float(t64.abs().sum())
    print(f"P {P}: |total - sum| {err:.3e} bound {bound:.3e}")
    assert err <= bound
    _policy.cache_clear()


@pytest.mark.parametrize("shared", [False, True], ids=["per_row", "shared"])
def test_autograd_hands_back_the_kernels_gradients_times_the_incoming_one(shared):
    from marlsc.ppo_loss import fused_ppo_loss_multi
    K, P, n = 8, 3, 70
    kl = _kl(P)
    cfg = em.make_cfg(use_kl=True, beta=0.3)
    _, _, gm, gl, gv = _multi(cfg, _stacked(n, K, shared, P), kl)
    idx = torch.arange(n * P, device="cuda").reshape(n, P)
    for g in (1.0, 0.5):
        mean, log_std, values, flat = _leaves(n, K, shared, P)
        v3 = values.reshape(n, P, 1)  # the critics' stacked [n, P, 1] output is taken as it is
        total, _ = fused_ppo_loss_multi(cfg, mean, log_std, v3, flat, idx if g == 0.5 else None, kl)
        assert total.requires_grad
        total.backward(torch.tensor(g, device="cuda"))
        assert torch.equal(mean.grad, gm * g) and torch.equal(log_std.grad, gl * g) and torch.equal(values.grad, gv * g)
        assert float(mean.grad.abs().max()) > 0 and float(log_std.grad.abs().max()) > 0
    _policy.cache_clear()


def test_argument_checks_match_the_single_function():
    from marlsc.ppo_loss import fused_ppo_loss_multi
    K, P, n = 5, 2, 9
    cfg = em.make_cfg(use_kl=True)
    mean, log_std, values, flat = _stacked(n, K, True, P)
    kl = _kl(P)
    idx = torch.arange(n * P, device="cuda").reshape(n, P)
    ok = dict(mean=mean, log_std=log_std, values=values, flat_batch=flat, idx=idx, kl_coeffs=kl)
    bad = [
        (dict(mean=mean.cpu()), "mean must be a CUDA tensor"),
        (dict(mean=mean.double()), "mean must be torch.float32"),
        (dict(log_std=log_std.double()), "log_std must be torch.float32"),
        (dict(values=values.cpu()), "values must be a CUDA tensor"),
        (dict(mean=mean[:, 0]), r"mean must be \[n >= 1, 1 <= P <= 64, 1 <= K <= 128\]"),
        (dict(mean=mean.new_zeros(n, 65, K)), r"mean must be \[n >= 1"),
        (dict(mean=mean.new_zeros(n, P, 129)), r"mean must be \[n >= 1"),
        (dict(log_std=log_std[0]), "log_std must be"),
        (dict(values=values[:, :1]), "values must be"),
        (dict(idx=idx.int()), "idx must be torch.int64"),
        (dict(idx=idx[:, 0]), "idx must be"),
        (dict(idx=None, flat_batch={k: v[:n] for k, v in flat.items()}), "idx is None and the batch has"),
        (dict(kl_coeffs=kl[:1]), "kl_coeffs for 2 policies"),
        (dict(stats=torch.zeros(5, dtype=torch.float64, device="cuda")), "stats must be a contiguous f64"),
        (dict(stats=torch.zeros((P, 5), device="cuda")), "stats must be torch.float64"),
        (dict(flat_batch={**flat, "actions": flat["actions"][:, :4]}), "flat_batch columns must be"),
    ]
    for kw, msg in bad:
        with pytest.raises(RuntimeError, match=msg):
            fused_ppo_loss_multi(cfg, **{**ok, **kw})
    import marlsc
    assert marlsc.fused_ppo_loss_multi is fused_ppo_loss_multi
    total, stats = fused_ppo_loss_multi(cfg, **ok)
    assert bool(torch.isfinite(total)) and stats.shape == (P, 5)
    _policy.cache_clear()


def test_workspace_query_and_argument_errors():
    from marlsc import abi
    from marlsc.ppo_loss import _desc, multi_workspace_bytes, rows_per_block, workspace_bytes
    L = abi.lib()
    for K in em.KS:
        rpb = rows_per_block(K)
        for n in (1, rpb, rpb + 1, 3 * rpb + 1, 10 ** 9):
            for P in (1, 2, 3, 8, 64):
                assert multi_workspace_bytes(n, P, K) == P * workspace_bytes(n, K)
    for n, P, k in ((0, 2, 5), (-1, 2, 5), (8, 0, 5), (8, -1, 5), (8, 65, 5), (8, 2, 0), (8, 2, 129)):
        assert L.msc_ppo_loss_multi_workspace(n, P, k) == -1
    n, P, K = 8, 2, 5
    cfg = em.make_cfg(use_kl=True)
    mean, log_std, values, flat = _stacked(n, K, False, P)
    d = _desc(cfg, 0.0, False, False)
    out = [torch.full_like(mean, 7.0), torch.full_like(log_std, 7.0), torch.full_like(values, 7.0),
           torch.full((P,), 7.0, device="cuda"), torch.full((P, 5), 7.0, dtype=torch.float64, device="cuda")]
    ws = torch.zeros(multi_workspace_bytes(n, P, K) // 8, dtype=torch.float64, device="cuda")
    kl = (C.c_double * P)(*_kl(P))
    p = lambda x: None if x is None else C.c_void_p(x.data_ptr())  # noqa: E731

    def call(desc=d, n=n, P=P, k=K, kl=kl, **null):
        a = dict(mean=mean, log_std=log_std, values=values, actions=flat["actions"], logp=flat["logp"],
                 adv=flat["advantages"], vt=flat["value_targets"], mo=flat["mean_old"], lo=flat["log_std_old"], gm=out[0],
                 gl=out[1], gv=out[2], totals=out[3], stats=out[4], ws=ws)
        a.update(null)
        return L.msc_ppo_loss_multi(None if desc is None else C.byref(desc), kl, p(a["mean"]), p(a["log_std"]),
                                    p(a["values"]), None, p(a["actions"]), p(a["logp"]), p(a["adv"]), p(a["vt"]),
                                    p(a["mo"]), p(a["lo"]), n, P, k, p(a["gm"]), p(a["gl"]), p(a["gv"]), p(a["totals"]),
                                    p(a["stats"]), p(a["ws"]), None)
    bad = [dict(n=0), dict(n=-3), dict(P=0), dict(P=-1), dict(P=65), dict(k=0), dict(k=129), dict(desc=None),
           dict(kl=None), dict(mo=None), dict(lo=None)]
    bad += [{name: None} for name in ("mean", "log_std", "values", "actions", "logp", "adv", "vt", "gm", "gl", "gv",
                                      "totals", "stats", "ws")]
    for kw in bad:
        assert call(**kw) != 0, kw
        msg = L.msc_last_error()
        assert msg and b"msc_ppo_loss_multi" in msg, kw
    torch.cuda.synchronize()
    assert all(bool((o == 7.0).all()) for o in out)  # nothing was launched
    assert call() == 0
    torch.cuda.synchronize()
    assert not any(bool((o == 7.0).any()) for o in out)
    no_kl = _desc(em.make_cfg(use_kl=False), 0.0, False, False)  # without use_kl the three may be null
    assert call(desc=no_kl, kl=None, mo=None, lo=None) == 0
    torch.cuda.synchronize()
    _policy.cache_clear()
