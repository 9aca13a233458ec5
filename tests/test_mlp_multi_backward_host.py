"""Host-side tests of the multi-policy MLP backward (no GPU): the argument checks of msc_mlp_relu_backward_multi
with their texts (they precede any launch, so made-up device pointers suffice), the workspace query and
msc_mlp_relu_backward_multi_plan against the single-policy query, and the Python entry points' refusals off the
GPU."""
import ctypes as C

import pytest

torch = pytest.importorskip("torch")

from marlsc import abi  # noqa: E402
from marlsc import mlp as M  # noqa: E402

P_ = C.c_void_p(1 << 20)  # a 16-byte aligned non-null "device pointer": never dereferenced
ODD = C.c_void_p((1 << 20) + 4)
SHAPES = [(256, 0), (32, 0), (1024, 0), (64, 64), (256, 256), (512, 512)]


def _call(**kw):
    """msc_mlp_relu_backward_multi on a valid argument set with kw replaced: (return code, msc_last_error())."""
    a = dict(x=P_, n=24, np=3, L=34, h1=64, h2=64, ko=5, w1p=P_, b1=P_, w2p=P_, b2=P_, w2tp=P_, w3=P_, d_out=P_, scale=1.0,
             acc=0, g_w1=P_, g_b1=P_, g_w2=P_, g_b2=P_, g_w3=P_, g_b3=P_, ws=P_)
    assert set(kw) <= set(a) and kw, kw  # (the valid set itself would launch)
    a.update(kw)
    L = abi.lib()
    rc = L.msc_mlp_relu_backward_multi(a["x"], a["n"], a["np"], a["L"], a["h1"], a["h2"], a["ko"], a["w1p"], a["b1"],
                                       a["w2p"], a["b2"], a["w2tp"], a["w3"], a["d_out"], C.c_float(a["scale"]), a["acc"],
                                       a["g_w1"], a["g_b1"], a["g_w2"], a["g_b2"], a["g_w3"], a["g_b3"], a["ws"], None)
    return rc, L.msc_last_error().decode()


ONE = dict(h1=96, h2=0, w2p=None, b2=None, w2tp=None, g_w2=None, g_b2=None)  # a valid one-hidden-layer set


def _arg_cases():
    yield {"np": 0}, "n_policies 0 must be in 1..64"
    yield {"np": 65, "n": 65}, "n_policies 65 must be in 1..64"
    yield {"np": -1}, "n_policies -1 must be in 1..64"
    yield {"n": 25}, "n_rows 25 must be a non-negative multiple of n_policies 3"
    yield {"n": -3}, "n_rows -3 must be a non-negative multiple of n_policies 3"
    for h1, h2 in ((96, 64), (64, 32), (1024, 64), (64, 96)):
        yield {"h1": h1, "h2": h2}, f"hidden sizes {h1}, {h2}: the fused MLP supports [H1, H2] with H1, H2 in {{64, 128, 256, 512}}"
    for h in (0, 16, 100, 1056):
        yield dict(ONE, h1=h), f"hidden size {h}: the fused MLP supports multiples of 32 up to 1024"
    yield {"ko": 33}, "bad shape (n_rows 24, in_dim 34, out_dim 33)"
    yield {"ko": 0}, "bad shape (n_rows 24, in_dim 34, out_dim 0)"
    yield {"L": 0}, "bad shape (n_rows 24, in_dim 0, out_dim 5)"
    yield {"L": 1025}, "bad shape (n_rows 24, in_dim 1025, out_dim 5)"
    for k in ("x", "w1p", "b1", "w2p", "b2", "w2tp", "w3", "d_out", "g_w1", "g_b1", "g_w2", "g_b2", "g_w3", "g_b3", "ws"):
        yield {k: None}, "null argument"
    for k in ("x", "w1p", "b1", "w3", "d_out", "g_w1", "g_b1", "g_w3", "g_b3", "ws"):
        yield dict(ONE, **{k: None}), "null argument"
    for k in ("b1", "b2", "w1p", "w2p", "w3"):
        yield {k: ODD}, "b1, b2, pre1 and the packed weights must be 16-byte aligned"
    for k in ("w2tp", "ws"):
        yield {k: ODD}, "w2tp and the workspace must be 16-byte aligned"


def test_every_argument_check_returns_its_text_before_any_launch():
    n = 0
    for bad, text in _arg_cases():
        rc, err = _call(**bad)
        assert rc == -1 and err == text, (bad, rc, err)
        n += 1
    assert n == 5 + 4 + 4 + 4 + 15 + 10 + 5 + 2


def test_no_rows_accumulate_returns_before_any_launch():
    """n_rows = 0 with accumulate = 1 adds nothing to any of the P outputs: success without touching a GPU or any
    pointer; the workspace may then be NULL."""
    assert _call(n=0, acc=1, ws=None)[0] == 0


def test_workspace_query_is_g_single_workspaces_monotone_and_capped():
    for h1, h2 in SHAPES:
        for L, KO in ((1, 1), (34, 5), (1024, 32)):
            for P in (1, 2, 3, 8, 64):
                prev, G = 0, None
                for rows in [0, 1, 31, 32, 33, 128, 129, 800, 8192, 8193, 16384, 16385, 262144, 1 << 26]:
                    b = M.multi_backward_workspace_bytes(rows * P, P, L, h1, h2, KO)
                    plan = M.multi_backward_plan(rows * P, P, L, h1, h2, KO)
                    assert plan["supported"] == 1 and plan["workspace_bytes"] == b
                    G = plan["group_policies"] if G is None else G
                    assert plan["group_policies"] == G  # a function of the widths alone
                    assert b == G * M.backward_workspace_bytes(rows, L, h1, h2, KO)
                    assert b >= prev and b % 16 == 0 and b > 0
                    prev = b
                assert M.multi_backward_workspace_bytes(P << 36, P, L, h1, h2, KO) == prev  # capped: rows run in rounds
                assert prev <= 1 << 30 or G == 1  # G workspaces at their cap fit 1 GiB (one always runs)
                # the largest such count
                assert G == P or (G + 1) * M.backward_workspace_bytes(1 << 36, L, h1, h2, KO) > 1 << 30


def test_workspace_query_refuses_exactly_what_the_single_query_refuses():
    for rows, L, h1, h2, KO in [(8, 34, 64, 64, 5), (-1, 34, 64, 64, 5), (8, 0, 64, 64, 5), (8, 1025, 64, 64, 5),
                                (8, 34, 96, 64, 5), (8, 34, 100, 0, 5), (8, 34, 96, 0, 5), (8, 34, 64, 64, 33),
                                (8, 34, 64, 64, 0), (0, 34, 64, 64, 5)]:
        single = M.backward_workspace_bytes(rows, L, h1, h2, KO)
        for P in (1, 3, 64):
            multi = M.multi_backward_workspace_bytes(rows * P, P, L, h1, h2, KO)
            assert (multi == -1) == (single == -1), (rows, L, h1, h2, KO, P)
            assert M.multi_backward_plan(rows * P, P, L, h1, h2, KO)["supported"] == (0 if single == -1 else 1)
    for n, P in ((24, 0), (65, 65), (25, 3), (24, -1)):  # a bad policy count, or one that does not divide the rows
        assert M.multi_backward_workspace_bytes(n, P, 34, 64, 64, 5) == -1
        assert set(M.multi_backward_plan(n, P, 34, 64, 64, 5).values()) == {0}


def _single_geometry(rows, L, h1, h2, KO):
    """(rounds, slices per round, row tiles of a full round) of msc_mlp_relu_backward for `rows` rows, read off its
    workspace query: the rows of a round are where the bytes stop growing, and the bytes of a (full) round are
    tiles x 32 x 2 (h1 + h2) floats of operands plus one padded copy of the gradients per slice."""
    top = M.backward_workspace_bytes(1 << 40, L, h1, h2, KO)
    lo, hi = 1, 1 << 22
    while lo < hi:
        mid = (lo + hi) // 2
        lo, hi = (lo, mid) if M.backward_workspace_bytes(mid, L, h1, h2, KO) == top else (mid + 1, hi)
    rr = (lo + 31) // 32 * 32
    tiles = (min(rows, rr) + 31) // 32
    part = h1 * ((L + 31) // 32 * 32) + h1 + h2 * h1 + h2 + 32 * (h2 or h1) + 32
    slices, rem = divmod(M.backward_workspace_bytes(rows, L, h1, h2, KO) // 4 - tiles * 32 * 2 * (h1 + h2), part)
    assert rem == 0
    return -(-rows // rr), slices, tiles


def test_plan_reports_the_single_policy_geometry_per_policy():
    buf = (C.c_int64 * 7)()
    for h1, h2 in SHAPES:
        for rows in (0, 1, 33, 129, 255, 256, 257, 800, 8192, 8193, 16384, 16385, 40000):
            for P in (1, 3, 8, 64):
                plan = M.multi_backward_plan(rows * P, P, 7, h1, h2, 5)
                rounds, slices, tiles = _single_geometry(rows, 7, h1, h2, 5)
                assert (plan["rounds"], plan["slices"], plan["round_tiles"]) == (rounds, slices, tiles), (h1, h2, rows, P)
                G = plan["group_policies"]
                assert 1 <= G <= P and plan["groups"] == -(-P // G)
    assert M.multi_backward_plan(5 * 16384, 5, 7, 256, 256, 5)["groups"] == 1   # 5 x 64 MiB of operands fit
    assert M.multi_backward_plan(64 * 33, 64, 7, 256, 256, 5)["groups"] > 1     # 64 of them do not
    # fewer values on request, none written past them; a NULL buffer is an error
    buf[2] = -7
    assert abi.lib().msc_mlp_relu_backward_multi_plan(24, 3, 34, 64, 64, 5, buf, 2) == 2 and buf[2] == -7
    assert abi.lib().msc_mlp_relu_backward_multi_plan(24, 3, 34, 64, 64, 5, None, 7) == -1
    assert abi.lib().msc_last_error().decode() == "null argument"


def _mlp(i, hidden, o):
    dims, mods = (i, *hidden, o), []
    for a, b in zip(dims[:-2], dims[1:-1]):
        mods += [torch.nn.Linear(a, b), torch.nn.ReLU()]
    return torch.nn.Sequential(*mods, torch.nn.Linear(dims[-2], dims[-1]))


def test_multi_trainable_and_multi_train_forward_off_the_gpu():
    nets = [_mlp(7, (32,), 3) for _ in range(3)]
    assert M.multi_layers(nets) == 2 and not M.multi_trainable(nets)  # CPU parameters
    assert not M.multi_trainable([_mlp(7, (32,), 3), _mlp(7, (64,), 3)])  # mixed shapes
    assert not M.multi_trainable([_mlp(7, (32,), 3), _mlp(7, (32, 32), 3)])
    assert not M.multi_trainable([_mlp(7, (32,), 3)] * 65)
    assert not M.multi_trainable([])
    assert not M.multi_trainable([_mlp(7, (32,), 33)] * 2)
    with pytest.raises(RuntimeError, match="multi_train_forward: x must be a CUDA tensor"):
        M.multi_train_forward(nets, torch.zeros(4, 3, 7))
    with pytest.raises(RuntimeError, match="multi_train_forward: x must be"):  # (not float32 either)
        M.multi_train_forward(nets, torch.zeros(4, 3, 7, dtype=torch.float64))


def test_head_mode_and_gru_networks_are_not_multi_trainable():
    from marlsc.ppo import MultiAgentActorCritic
    from marlsc.rollout import RolloutConfig
    mlp = {"hidden_sizes": [32]}
    head = MultiAgentActorCritic(2, 7, 14, 3, RolloutConfig(actor=mlp, critic=mlp, use_mu_sigma_head=True), shared=False)
    assert not M.multi_trainable([p.actor for p in head.policies])
    gru = {"num_layers": 1, "hidden_size": 32, "bidirectional": False, "max_seq_len": 2, "output_dim": 32}
    rec = MultiAgentActorCritic(2, 7, 14, 3, RolloutConfig(actor=gru, critic=gru, actor_type="gru", critic_type="gru",
                                                           critic_obs_type="local"), shared=False)
    assert rec.recurrent and not isinstance(rec.policies[0].actor, torch.nn.Sequential)
    assert not M.multi_trainable([p.actor for p in rec.policies])
    assert not M.multi_trainable([p.critic for p in rec.policies])
    assert not M.multi_trainable([torch.nn.GRU(7, 32, batch_first=True)] * 2)


def test_learner_switch_refuses_a_cpu_module_and_defaults_to_off(monkeypatch):
    from marlsc.ppo import MultiAgentActorCritic, PPOConfig, PPOLearner
    from marlsc.rollout import RolloutConfig
    rc = RolloutConfig(actor={"hidden_sizes": [32]}, critic={"hidden_sizes": [32]})
    module = MultiAgentActorCritic(2, 7, 14, 3, rc, shared=False)
    cfg = PPOConfig()
    with pytest.raises(RuntimeError, match=r"PPOLearner\(fused_multi=True\): the multi-policy MLP backward is a HIP kernel"):
        PPOLearner(module, cfg, fused_multi=True)
    monkeypatch.delenv("MSC_FUSED_MULTI_GRAD", raising=False)
    assert PPOLearner(module, cfg).fused_multi is False  # the default is off ...
    assert PPOLearner(module, cfg, fused_multi=None).fused_multi is False
    monkeypatch.setenv("MSC_FUSED_MULTI_GRAD", "1")      # ... and None reads the knob
    with pytest.raises(RuntimeError, match=r"PPOLearner\(fused_multi=True\)"):
        PPOLearner(module, cfg)
    assert PPOLearner(module, cfg, fused_multi=False).fused_multi is False
    monkeypatch.setenv("MSC_FUSED_MLP_GRAD", "0")
    assert PPOLearner(module, cfg, fused_multi=False).fused_mlp is False  # a switch of its own
