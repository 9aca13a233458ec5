"""GPU tests of the fused PPO loss (csrc/ppo_loss.hip: msc_ppo_loss, marlsc/ppo_loss.py:fused_ppo_loss,
PPOLearner(fused_loss=True)) against the float64 yardstick and the elementwise bound of
tests/ppo_loss_emulation.py, exact pins where the result is determined bit for bit, and the learner's
two paths against a float64 copy of the module. With MSC_PPO_LOSS_PROFILE=<file> the figures measured
here (max error / bound per output for the kernel and for torch float32; the learner's gradient errors)
are written to that file (profiles/ppo_loss/error_over_bound.txt)."""
import copy
import ctypes as C
import os
from pathlib import Path

import numpy as np
import pytest
import torch
import yaml

import ppo_loss_emulation as em

pytestmark = pytest.mark.gpu
REPO = Path(__file__).resolve().parents[1]
COMBOS = [(shared, use_kl, beta) for shared in (False, True) for use_kl in (False, True) for beta in (None, 0.3)]
RECORD = []


@pytest.fixture(scope="module", autouse=True)
def _profile():
    yield
    path = os.environ.get("MSC_PPO_LOSS_PROFILE")
    if path and RECORD:
        Path(path).parent.mkdir(parents=True, exist_ok=True)
        Path(path).write_text("\n".join(RECORD) + "\n")


def _dev(x, dtype=torch.float32):
    return torch.tensor(np.asarray(x), dtype=dtype, device="cuda")


def _batch(inp):
    return {k: _dev(v) for k, v in inp["batch"].items()}


def run_kernel(cfg, inp, kl_coeff=1.0, stats=None, batch=None, idx="inp"):
    """One msc_ppo_loss call on the generator's inputs: device tensors (total, stats, gm, gl, gv)."""
    from marlsc.ppo_loss import ppo_loss_launch
    ix = inp["idx"] if isinstance(idx, str) else idx
    return ppo_loss_launch(cfg, _dev(inp["mean"]), _dev(inp["log_std"]), _dev(inp["values"]), batch or _batch(inp),
                           None if ix is None else _dev(ix, torch.int64), kl_coeff, stats)


def as_numpy(out):
    total, stats, gm, gl, gv = out
    f = lambda t: t.double().cpu().numpy()  # noqa: E731
    return {"total": f(total)[0], "stats": f(stats), "grad_mean": f(gm), "grad_log_std": f(gl), "grad_values": f(gv)}


def test_workspace_query_rows_per_block_and_argument_errors():
    from marlsc import abi
    from marlsc.ppo_loss import grid_blocks, rows_per_block, workspace_bytes
    L = abi.lib()
    per_block = workspace_bytes(1, 1)  # one block's partial
    assert per_block > 0 and per_block % 8 == 0 and per_block >= (5 + 128) * 8  # five statistics and 128 columns, f64
    for K in em.KS:
        rpb = rows_per_block(K)
        assert workspace_bytes(1, K) == workspace_bytes(rpb, K) == per_block
        assert workspace_bytes(rpb + 1, K) == 2 * per_block
        assert workspace_bytes(3 * rpb + 1, K) == 4 * per_block
        assert workspace_bytes(10 ** 9, K) == 2048 * per_block  # the grid cap: a function of (n, K) alone
        assert grid_blocks(3 * rpb + 1, K) == 4
    assert [rows_per_block(k) for k in (1, 2, 5, 16, 17, 64, 65, 128)] == [256, 128, 32, 16, 8, 4, 4, 4]
    for n, k in ((0, 5), (-1, 5), (8, 0), (8, 129)):
        assert L.msc_ppo_loss_workspace(n, k) == -1
    cfg = em.make_cfg(use_kl=True)
    inp = em.make_inputs(8, 5, cfg=cfg)
    from marlsc.ppo_loss import _desc
    d = _desc(cfg, 0.2, False, False)
    t = {k: _dev(inp[k]) for k in ("mean", "log_std", "values")}
    b = _batch(inp)
    out = [torch.full_like(t["mean"], 7.0), torch.full_like(t["mean"], 7.0), torch.full_like(t["values"], 7.0),
           torch.full((1,), 7.0, device="cuda"), torch.full((5,), 7.0, dtype=torch.float64, device="cuda")]
    ws = torch.zeros(per_block // 8, dtype=torch.float64, device="cuda")
    p = lambda x: None if x is None else C.c_void_p(x.data_ptr())  # noqa: E731

    def call(desc=d, n=8, k=5, **null):
        a = dict(mean=t["mean"], log_std=t["log_std"], values=t["values"], actions=b["actions"], logp=b["logp"],
                 adv=b["advantages"], vt=b["value_targets"], mo=b["mean_old"], lo=b["log_std_old"], gm=out[0],
                 gl=out[1], gv=out[2], total=out[3], stats=out[4], ws=ws)
        a.update(null)
        return L.msc_ppo_loss(None if desc is None else C.byref(desc), p(a["mean"]), p(a["log_std"]), p(a["values"]),
                              None, p(a["actions"]), p(a["logp"]), p(a["adv"]), p(a["vt"]), p(a["mo"]), p(a["lo"]), n, k,
                              p(a["gm"]), p(a["gl"]), p(a["gv"]), p(a["total"]), p(a["stats"]), p(a["ws"]), None)
    bad = [dict(n=0), dict(n=-3), dict(k=0), dict(k=129), dict(desc=None), dict(mo=None), dict(lo=None)]
    bad += [{name: None} for name in ("mean", "log_std", "values", "actions", "logp", "adv", "vt", "gm", "gl", "gv",
                                      "total", "stats", "ws")]
    for kw in bad:
        assert call(**kw) != 0, kw
        assert L.msc_last_error(), kw
    torch.cuda.synchronize()
    assert all(bool((o == 7.0).all()) for o in out)  # nothing was launched
    assert call() == 0
    torch.cuda.synchronize()
    assert not bool((out[0] == 7.0).any())


@pytest.mark.parametrize("K", em.KS)
def test_every_output_within_the_bound_of_the_f64_yardstick(K):
    """Every output (f32 total, f64 stats, the three gradients) within the elementwise bound, for shared and
    per-row log_std, KL on and off, hysteretic beta 1 and 0.3, idx NULL / a permutation / repeats with
    B > n, at n in {1, 63, 64, 65, rows-per-block + 1, 3 rows-per-block + 1}."""
    from marlsc.ppo_loss import grid_blocks, rows_per_block
    rpb = rows_per_block(K)
    assert grid_blocks(3 * rpb + 1, K) > 2
    profile = bool(os.environ.get("MSC_PPO_LOSS_PROFILE"))
    worst = {k: 0.0 for k in em.OUTPUTS}
    worst32 = {k: 0.0 for k in em.OUTPUTS}
    g = np.random.default_rng(100 + K)
    for n in sorted({1, 63, 64, 65, rpb + 1, 3 * rpb + 1}):
        B = n + 37
        for shared, use_kl, beta in COMBOS:
            cfg = em.make_cfg(use_kl=use_kl, beta=beta)
            for mode, idx, Bm in (("null", None, n), ("perm", g.permutation(n), n), ("repeat", g.integers(0, B, n), B)):
                inp = em.make_inputs(n, K, B=Bm, shared=shared, cfg=cfg, seed=2, idx=idx)
                ref, bnd = em.run_torch(cfg, inp), em.bounds(cfg, inp)
                ob = em.over_bound(as_numpy(run_kernel(cfg, inp)), ref, bnd)
                for k, v in ob.items():
                    worst[k] = max(worst[k], v)
                if profile:
                    for k, v in em.over_bound(em.run_torch(cfg, inp, dtype=torch.float32, device="cuda"), ref, bnd).items():
                        worst32[k] = max(worst32[k], v)
                assert max(ob.values()) <= 1.0, (n, shared, use_kl, beta, mode, ob)
    line = f"K {K:3d} max error/bound, kernel: " + " ".join(f"{k} {v:.3f}" for k, v in worst.items())
    if profile:
        line += " | torch f32: " + " ".join(f"{k} {v:.3f}" for k, v in worst32.items())
    print(line)
    RECORD.append(line)


def test_grid_stride_loop_past_the_grid_cap():
    """n past 2048 blocks' worth of rows: the grid-stride loop runs more than once (K = 5: 32 rows per block)."""
    from marlsc.ppo_loss import rows_per_block
    K = 5
    n = 2048 * rows_per_block(K) + rows_per_block(K) + 1
    g = np.random.default_rng(9)
    for shared, idx in ((False, None), (True, g.permutation(n))):
        cfg = em.make_cfg(use_kl=True, beta=0.3)
        inp = em.make_inputs(n, K, shared=shared, cfg=cfg, seed=3, idx=idx)
        ob = em.over_bound(as_numpy(run_kernel(cfg, inp)), em.run_torch(cfg, inp), em.bounds(cfg, inp))
        line = f"n {n} K {K} shared {shared}: max error/bound, kernel: " + " ".join(f"{k} {v:.3f}" for k, v in ob.items())
        print(line)
        RECORD.append(line)
        assert max(ob.values()) <= 1.0, ob


def test_gradients_that_must_be_zero_are_zero():
    """Without the KL term: grad_mean is exactly 0 on the rows whose surrogate is clipped or whose advantage
    is 0, grad_values exactly 0 on the rows whose value error is clipped -- the rows where the float64
    yardstick's gradient is exactly 0 -- and non-zero on the others (vf == vf_clip_param among them)."""
    cfg = em.make_cfg(use_kl=False)
    for K in (1, 5, 65):
        inp = em.make_inputs(300, K, cfg=cfg, seed=4)
        ref, got = em.run_torch(cfg, inp), as_numpy(run_kernel(cfg, inp))
        zero_m, zero_v = np.all(ref["grad_mean"] == 0, axis=1), ref["grad_values"] == 0
        adv = inp["batch"]["advantages"]
        assert zero_m.sum() >= 60 and (~zero_m).sum() >= 60 and np.all(zero_m[adv == 0]) and (adv == 0).sum() >= 30
        assert np.array_equal(zero_v, np.abs(inp["dv"]) == 3) and zero_v.sum() >= 90
        assert np.all(got["grad_mean"][zero_m] == 0.0) and np.all(got["grad_values"][zero_v] == 0.0)
        assert np.all(np.any(got["grad_mean"][~zero_m] != 0.0, axis=1)) and np.all(got["grad_values"][~zero_v] != 0.0)
        at = np.abs(inp["dv"]) == 2  # vf exactly at vf_clip_param: the gradient passes
        assert at.sum() >= 90 and np.all(got["grad_values"][at] != 0.0)


def test_tie_at_the_clip_bound_keeps_the_full_gradient():
    """clip_param = 0, K = 1, a - mean = 1, log_std = 0 and logp_old = logp (torch float32 on the CPU: at
    K = 1 the kernel's chain is the same, rounding for rounding), so the ratio is expf(0) = 1 = both clip
    bounds exactly: A r and A clamp(r) tie and the clamp sits on its bounds. The gradient is the full
    -A r / n (d / var) = -A / n, bit for bit, for A > 0 and A < 0, as torch float32 autograd gives it."""
    from marlsc.ppo import gaussian_logp, ppo_loss
    cfg = em.make_cfg(clip_param=0.0, entropy_coeff=0.0)
    n = 4
    mean, ls = torch.tensor([[0.5], [-1.0], [2.0], [0.25]]), torch.zeros(n, 1)
    act = mean + 1.0
    adv = torch.tensor([2.0, -2.0, 0.5, -8.0])
    vt = torch.zeros(n)
    values = torch.tensor([2.0, -2.0, 1.0, 3.0])
    b = {"actions": act, "logp": gaussian_logp(act, mean, ls), "advantages": adv, "value_targets": vt}
    m, l, v = mean.clone().requires_grad_(), ls.clone().requires_grad_(), values.clone().requires_grad_()
    ppo_loss(cfg, m, l, v, b, 0.0)[0].backward()
    from marlsc.ppo_loss import ppo_loss_launch
    total, stats, gm, gl, gv = ppo_loss_launch(cfg, mean.cuda(), ls.cuda(), values.cuda(),
                                               {k: x.cuda() for k, x in b.items()}, None, 0.0)
    want = (-adv / n)[:, None]
    assert torch.equal(gm.cpu(), want) and torch.equal(m.grad, want)
    assert torch.equal(gl.cpu(), l.grad) and torch.equal(gv.cpu(), v.grad)
    assert torch.equal(gv.cpu(), torch.tensor([0.7 / n * 4.0, -0.7 / n * 4.0, 0.7 / n * 2.0, 0.0]))


def test_idx_equals_a_torch_gather_and_calls_repeat_bit_for_bit():
    K, n, B = 17, 200, 300
    g = np.random.default_rng(5)
    idx = g.integers(0, B, n)
    for shared in (False, True):
        cfg = em.make_cfg(use_kl=True, beta=0.3)
        inp = em.make_inputs(n, K, B=B, shared=shared, cfg=cfg, seed=5, idx=idx)
        full = _batch(inp)
        a = run_kernel(cfg, inp, batch=full)
        again = run_kernel(cfg, inp, batch=full)
        ix = _dev(idx, torch.int64)
        gathered = run_kernel(cfg, inp, batch={k: v[ix].contiguous() for k, v in full.items()}, idx=None)
        for x, y, z in zip(a, again, gathered):
            assert torch.equal(x, y) and torch.equal(x, z)


def test_accumulate_stats_adds_in_f64():
    cfg = em.make_cfg(use_kl=True)
    i1, i2 = em.make_inputs(65, 5, cfg=cfg, seed=6), em.make_inputs(130, 5, shared=True, cfg=cfg, seed=7)
    s1, s2 = run_kernel(cfg, i1)[1], run_kernel(cfg, i2)[1]
    acc = torch.zeros(5, dtype=torch.float64, device="cuda")
    run_kernel(cfg, i1, stats=acc)
    assert torch.equal(acc, s1)
    run_kernel(cfg, i2, stats=acc)
    assert torch.equal(acc, s1 + s2) and bool((s2 != 0).all())


def _leaves(inp):
    return [_dev(inp[k]).requires_grad_() for k in ("mean", "log_std", "values")]


def test_shared_row_given_as_k_and_as_an_expanded_view():
    from marlsc.ppo_loss import fused_ppo_loss
    cfg = em.make_cfg(use_kl=True)
    n, K = 70, 8
    inp = em.make_inputs(n, K, shared=True, cfg=cfg, seed=8)
    b = _batch(inp)
    m1, l1, v1 = _leaves(inp)
    t1, s1 = fused_ppo_loss(cfg, m1, l1, v1, b, None, 1.0)
    t1.backward()
    m2, l2, v2 = _leaves(inp)
    view = l2.expand(n, K)
    assert view.stride(0) == 0
    t2, s2 = fused_ppo_loss(cfg, m2, view, v2, b, None, 1.0)
    t2.backward()
    assert torch.equal(t1, t2) and torch.equal(s1, s2) and torch.equal(m1.grad, m2.grad) and torch.equal(v1.grad, v2.grad)
    ref, bnd = em.run_torch(cfg, inp), em.bounds(cfg, inp)
    for l in (l1, l2):
        assert l.grad.shape == (K,)
        assert np.all(np.abs(l.grad.double().cpu().numpy() - ref["grad_log_std"]) <= bnd["grad_log_std"])


@pytest.mark.parametrize("factor", [1.0, 0.5])
@pytest.mark.parametrize("shared", [False, True])
def test_autograd_hands_back_the_kernels_gradients_times_the_incoming_one(shared, factor):
    from marlsc.ppo_loss import fused_ppo_loss
    cfg = em.make_cfg(use_kl=True, beta=0.3)
    g = np.random.default_rng(11)
    inp = em.make_inputs(90, 5, B=120, shared=shared, cfg=cfg, seed=9, idx=g.integers(0, 120, 90))
    tot_k, stats_k, gm, gl, gv = run_kernel(cfg, inp)
    m, l, v = _leaves(inp)
    total, stats = fused_ppo_loss(cfg, m, l, v, _batch(inp), _dev(inp["idx"], torch.int64), 1.0)
    assert total.shape == () and total.requires_grad and not stats.requires_grad
    assert torch.equal(total.detach(), tot_k[0]) and torch.equal(stats, stats_k)
    (total * factor).backward()
    assert torch.equal(m.grad, gm * factor) and torch.equal(l.grad, gl * factor) and torch.equal(v.grad, gv * factor)
    with pytest.raises(RuntimeError, match="must be torch.float32"):
        fused_ppo_loss(cfg, m.double(), l, v, _batch(inp), None, 1.0)


# ----------------------------------------------------------------------------------------------
# the learner: fused_loss=True and False against a float64 copy of the module
# ----------------------------------------------------------------------------------------------
def _ppo_cfg(name="ippo", **specific):
    from marlsc.ppo import PPOConfig
    raw = yaml.safe_load(open(REPO / f"config_files/algorithms/{name}.yaml"))
    raw["algorithm"]["algorithm_specific"].update(specific)
    raw["algorithm"]["shared"].update(num_epochs=1, num_minibatches=1, batch_size=1 << 20, learning_rate=1e-3)
    cfg = PPOConfig.from_algorithm_config(raw)
    cfg.grad_clip = None
    return cfg


def _mlp_batch(m, cfg, S, L, seed, kl_shift=0.0):
    """A synthetic batch [S, W, ...] for module m: actions sampled from its own distribution, the old
    distribution shifted by kl_shift (KL of about K kl_shift^2 / 2 per row)."""
    from marlsc.ppo import gaussian_logp
    g = torch.Generator(device="cuda").manual_seed(seed)
    W = m.W
    obs = torch.randn((S, W, L), device="cuda", generator=g)
    with torch.no_grad():
        full = torch.cat([obs, obs.reshape(S, 1, W * L).expand(S, W, W * L)], -1)
        mean, ls = m.dist_inputs(obs, full)
        ls = ls.contiguous()
        act = mean + ls.exp() * torch.randn(mean.shape, device="cuda", generator=g)
        logp = gaussian_logp(act, mean, ls) + 0.1 * torch.randn((S, W), device="cuda", generator=g)
    batch = {"obs": obs, "actions": act, "logp": logp, "advantages": torch.randn((S, W), device="cuda", generator=g),
             "value_targets": torch.randn((S, W), device="cuda", generator=g)}
    if cfg.use_kl_loss:
        batch["mean_old"], batch["log_std_old"] = mean + kl_shift, ls.clone()
    return batch


def _to64(batch):
    out = {}
    for k, v in batch.items():
        if k == "seq":
            out[k] = dict(v, state_in={s: h.double() for s, h in v["state_in"].items()})
        else:
            out[k] = v.double()
    return out


def _three_updates(module, cfg, batch):
    """update() once with the fused loss, once with the torch loss and once on a float64 copy (torch
    loss): [(returned dict, {parameter name: grad as float64})] in that order."""
    from marlsc.ppo import PPOLearner
    res = []
    for fused, f64 in ((True, False), (False, False), (False, True)):
        m = copy.deepcopy(module)
        if f64:
            m = m.double()
        learner = PPOLearner(m, cfg, seed=5, fused_loss=fused)
        assert learner.fused_loss is fused
        out = learner.update(_to64(batch) if f64 else batch, None, 0)
        assert out["num_minibatch_steps"] == 1
        res.append((out, {k: p.grad.double().clone() for k, p in m.named_parameters() if p.grad is not None},
                    list(learner.kl_coeffs)))
    return res


N_BATCHES = 32


def _compare_learners(name, module, cfg, batches):
    """The fall-back criterion: per parameter tensor, the fused path's error against the float64 copy is at
    most twice the torch float32 path's; the same for every value of the returned dict, there with a floor of
    2^-22 of the value (four float32 roundings: neither path's statistics are known better than float32
    arithmetic on the rows leaves them). A bound propagated through the backward pass of the networks would
    need their absolute Jacobians and a rounding analysis of torch's own backward, which autograd does not
    give.
    The error of a tensor is the root of the summed squared differences of its gradient over N_BATCHES = 32
    independent batches on the same weights. One batch does not carry the comparison: both paths share
    torch's backward and differ by roundings of the same size in the loss's gradients, so on a tensor of one
    or three elements the quotient of the two errors is a quotient of two independent roundings, above 2
    about three times in ten whatever the code does. Over 32 batches the quotient of two equal error
    levels follows an F(32 m, 32 m) law in its square (m elements), above 4 less than once in 10^4 at m = 1.
    So that one grossly wrong batch is not averaged away, every single batch is held too: its fused error on
    a tensor is at most twice the largest error the torch float32 path shows on that tensor in any of the
    32 batches (with equal error levels that asks a rounding to stay below about twice the largest of 32 of
    its kind, some 4.5 standard deviations). Both errors and the largest single-batch figures are recorded."""
    from collections import defaultdict
    sf, st, sg = defaultdict(float), defaultdict(float), defaultdict(float)
    of_sq, ot_sq, last = defaultdict(float), defaultdict(float), None
    mf, mt = defaultdict(float), defaultdict(float)  # the largest single-batch errors
    for batch in batches:
        (of, gf, kf), (ot, gt, kt), (o64, g64, k64) = _three_updates(module, cfg, batch)
        assert list(of) == list(ot) == list(o64)
        assert gf.keys() == gt.keys() == g64.keys() and len(gf) >= 4
        assert kf == kt == k64
        for k in g64:
            sf[k] += float((gf[k] - g64[k]).pow(2).sum())
            st[k] += float((gt[k] - g64[k]).pow(2).sum())
            sg[k] += float(g64[k].pow(2).sum())
            mf[k] = max(mf[k], float((gf[k] - g64[k]).norm()))
            mt[k] = max(mt[k], float((gt[k] - g64[k]).norm()))
        for k in o64:
            of_sq[k] += (of[k] - o64[k]) ** 2
            ot_sq[k] += (ot[k] - o64[k]) ** 2
        last = (of, o64, g64)
    of, o64, g64 = last
    worst = 0.0
    for k in g64:
        ef, et = sf[k] ** 0.5, st[k] ** 0.5
        worst = max(worst, ef / et if et > 0 else (0.0 if ef == 0 else float("inf")))
        RECORD.append(f"learner {name}: {k} {tuple(g64[k].shape)} |grad| {sg[k] ** 0.5:.3e} error fused {ef:.3e} "
                      f"torch-f32 {et:.3e} ({len(batches)} batches; largest single batch: fused {mf[k]:.3e} "
                      f"torch-f32 {mt[k]:.3e})")
        assert sg[k] > 0 and ef <= 2.0 * et, (name, k, ef, et)
        assert mf[k] <= 2.0 * mt[k], (name, k, mf[k], mt[k])
    for k in o64:
        ef, et = of_sq[k] ** 0.5, ot_sq[k] ** 0.5
        RECORD.append(f"learner {name}: returned {k} (last batch {o64[k]:.9g}) error fused {ef:.3e} torch-f32 {et:.3e}")
        assert ef <= max(2.0 * et, 2.0 ** -22 * abs(o64[k]) * len(batches) ** 0.5), (name, k, ef, et, o64[k])
    print(f"learner {name}: worst fused / torch-f32 gradient error ratio {worst:.3f}")


def _module(cfg, W, L, K, shared):
    from marlsc.ppo import MultiAgentActorCritic
    torch.manual_seed(3)
    return MultiAgentActorCritic(W, L, L * W, K, cfg.rollout_config(), shared).cuda()


MLP = {"type": "mlp", "config": {"hidden_sizes": [32], "activation": "relu"}}


@pytest.mark.parametrize("case", ["shared", "per_agent", "mu_sigma"])
def test_learner_fused_and_torch_paths_against_an_f64_copy(case):
    nets = {"shared_layers": None, "actor": MLP, "critic": MLP, "use_mu_sigma_head": case == "mu_sigma"}
    if case == "mu_sigma":
        nets["actor"] = {"type": "mlp", "config": {"hidden_sizes": [32], "activation": "relu",
                                                   "output_activation_mu": "tanh"}}
    sharing = case != "per_agent"
    cfg = _ppo_cfg("mappo" if case == "per_agent" else "ippo", parameter_sharing=sharing, use_kl_loss=True,
                   networks=nets, hysteretic_beta=0.5, vf_clip_param=1.5)
    m = _module(cfg, 3, 7, 3, sharing)
    assert m.head_mode == (case == "mu_sigma") and len(m.policies) == (1 if sharing else 3)
    _compare_learners(case, m, cfg, [_mlp_batch(m, cfg, 50, 7, seed=s, kl_shift=0.05) for s in range(N_BATCHES)])


def test_learner_gru_sequences_of_two_steps():
    gru = {"type": "gru", "config": {"num_layers": 1, "hidden_size": 32, "bidirectional": False, "max_seq_len": 2,
                                     "output_dim": 32}}
    nets = {"shared_layers": gru, "actor": MLP, "critic": MLP, "use_mu_sigma_head": False}
    cfg = _ppo_cfg("ippo", parameter_sharing=True, use_kl_loss=False, networks=nets)
    W, L, K, T, E = 2, 7, 3, 6, 9
    m = _module(cfg, W, L, K, True)
    assert m.recurrent and m.max_seq_len == 2
    g = torch.Generator(device="cuda").manual_seed(2)
    r = lambda *s: torch.randn(s, device="cuda", generator=g)  # noqa: E731
    # actions drawn from the module's own distribution on each sequence, as in the other cases (and as PPO
    # meets them): with actions unrelated to the policy a row's ratio reaches e^5 and more, one such row
    # carries nearly all of a batch's gradient, and the batch's error is that row's one rounding
    from marlsc.ppo import PPOLearner, gaussian_logp
    probe = PPOLearner(m, cfg, seed=0, fused_loss=False)
    ids = torch.arange((T // 2) * E * W, device="cuda")
    batches = []
    for _ in range(N_BATCHES):
        state_in = {k: 0.3 * r(T // 2, *h.shape) for k, h in m.initial_state(E, device="cuda").items()}
        obs = r(T * E, W, L)
        seq = {"T": T, "E": E, "S": 2, "state_in": state_in,
               "truncated": torch.zeros((T, E, W), dtype=torch.uint8, device="cuda")}
        with torch.no_grad():
            mean, ls, _, rows = probe._seq_forward(m.policies[0], obs, seq, ids)
            a = mean + ls.exp() * r(*mean.shape)
            act, logp = torch.empty((T * E * W, K), device="cuda"), torch.empty(T * E * W, device="cuda")
            act[rows], logp[rows] = a, gaussian_logp(a, mean, ls) + 0.1 * r(rows.numel())
        batches.append({"obs": obs, "actions": act.reshape(T * E, W, K), "logp": logp.reshape(T * E, W),
                        "advantages": r(T * E, W), "value_targets": r(T * E, W), "seq": seq})
    _compare_learners("gru", m, cfg, batches)


def test_cppo_trainers_learner_takes_the_switch_at_k_40(monkeypatch):
    from marlsc import make_synthetic_env_config
    from marlsc.cppo import CPPOConfig, CPPOTrainer
    raw = yaml.safe_load(open(REPO / "config_files/algorithms/cppo.yaml"))
    raw["algorithm"]["shared"].update(num_epochs=1, num_minibatches=1, num_eval_episodes=2)
    cfg = CPPOConfig.from_algorithm_config(raw)
    monkeypatch.setenv("MSC_FUSED_LOSS", "1")
    tr = CPPOTrainer(make_synthetic_env_config(8, 64, 5, episode_length=6), cfg, root_seed=7, n_envs=16, rollout_len=8,
                     device=0)
    assert tr.learner.fused_loss is True and tr.env.K == 40 and not tr.module.shared
    res = tr.train_iteration()
    assert all(np.isfinite(v) for k, v in res.items() if k.startswith("learner/")) and res["learner/num_minibatch_steps"] >= 1
    monkeypatch.delenv("MSC_FUSED_LOSS")
    cfg2 = copy.deepcopy(cfg)
    cfg2.batch_size, cfg2.grad_clip = 1 << 20, None
    g = torch.Generator(device="cuda").manual_seed(4)
    S, L, K = 96, tr.env.L, 40
    from marlsc.ppo import gaussian_logp
    batches = []
    for _ in range(N_BATCHES):
        obs = torch.randn((S, 1, L), device="cuda", generator=g)
        with torch.no_grad():
            mean, ls = tr.module.dist_inputs(obs, None)
            ls = ls.contiguous()
            act = mean + ls.exp() * torch.randn(mean.shape, device="cuda", generator=g)
            logp = gaussian_logp(act, mean, ls) + 0.1 * torch.randn((S, 1), device="cuda", generator=g)
        batch = {"obs": obs, "actions": act, "logp": logp, "advantages": torch.randn((S, 1), device="cuda", generator=g),
                 "value_targets": torch.randn((S, 1), device="cuda", generator=g)}
        if cfg2.use_kl_loss:
            batch["mean_old"], batch["log_std_old"] = mean + 0.02, ls.clone()
        batches.append(batch)
    _compare_learners("cppo K=40", tr.module, cfg2, batches)
    tr.env.close()


def test_adaptive_kl_coefficient_moves_the_same_way_on_both_paths():
    nets = {"shared_layers": None, "actor": MLP, "critic": MLP, "use_mu_sigma_head": False}
    cfg = _ppo_cfg("ippo", parameter_sharing=False, use_kl_loss=True, networks=nets)
    cfg.kl_target, cfg.kl_coeff = 0.01, 0.2
    m = _module(cfg, 2, 7, 3, False)
    for shift, moved in ((1.0, 0.2 * 1.5), (1e-4, 0.2 * 0.5)):  # KL about 1.5 per row, and about 1.5e-8
        batch = _mlp_batch(m, cfg, 40, 7, seed=6, kl_shift=shift)
        for out, _, kls in _three_updates(m, cfg, batch):  # fused, torch float32, torch float64
            assert kls == [moved, moved] and out["kl_coeff"] == moved
            assert (out["mean_kl"] > 2 * cfg.kl_target) if shift == 1.0 else (out["mean_kl"] < cfg.kl_target / 2)


def test_full_multi_epoch_update_lowers_the_loss():
    """tests/test_ppo_host.py:test_learner_update_reduces_the_loss_on_a_fixed_batch, on the GPU with the
    fused loss."""
    from marlsc.ppo import MultiAgentActorCritic, PPOLearner, gaussian_logp, ppo_loss
    cfg = _ppo_cfg("ippo")
    cfg.num_epochs, cfg.num_minibatches, cfg.grad_clip, cfg.batch_size = 20, 2, 5.0, 4000
    cfg.learning_rate = 3e-3
    torch.manual_seed(1)
    W, L, K, S = 2, 6, 3, 64
    m = MultiAgentActorCritic(W, L, L * W, K, cfg.rollout_config(), True).cuda()
    obs = torch.randn(S, W, L).cuda()
    with torch.no_grad():
        mean, ls = m.dist_inputs(obs)
        a = mean + ls.exp() * torch.randn(mean.shape).cuda()
        logp = gaussian_logp(a, mean, ls)
    batch = {"obs": obs, "actions": a, "logp": logp, "advantages": torch.randn(S, W).cuda(),
             "value_targets": (torch.randn(S, W) * 3).cuda()}

    def loss_now():
        with torch.no_grad():
            mu, l2 = m.dist_inputs(obs)
            return float(ppo_loss(cfg, mu, l2, m.values(obs), batch, 0.0)[0])
    before = loss_now()
    out = PPOLearner(m, cfg, seed=0, fused_loss=True).update(batch, None, timestep=0)
    assert out["num_minibatch_steps"] >= 20 and out["learning_rate"] == 3e-3
    assert all(np.isfinite(v) for v in out.values())
    assert loss_now() < before
