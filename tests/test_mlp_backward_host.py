"""Host-side tests of the fused MLP backward (no GPU): the W2^T pack against a direct index formula, the
argument checks of msc_mlp_relu_backward with their full texts (they precede any launch, so made-up device
pointers suffice), the workspace query, and the Python entry points' refusals off the GPU."""
import ctypes as C

import numpy as np
import pytest

torch = pytest.importorskip("torch")

from marlsc import abi  # noqa: E402
from marlsc import mlp as M  # noqa: E402

P_ = C.c_void_p(1 << 20)  # a 16-byte aligned non-null "device pointer": never dereferenced
ODD = C.c_void_p((1 << 20) + 4)
SIZES = (64, 128, 256, 512)


def _rho(r, h):
    return (r & 3) + 8 * (r >> 2) + 4 * h


@pytest.mark.parametrize("H2,H1", [(64, 64), (64, 128), (128, 64), (256, 512)])
def test_w2t_pack_against_the_index_formula(H2, H1):
    """w2tp[t1][s4][lane][i] = W2[32 t2 + rho(r, h)][32 t1 + c] with 4 s4 + i = 16 t2 + r, c = lane & 31,
    h = lane >> 5: what the dgrad pass reads as the A operand of d1 = W2^T d2."""
    w2 = torch.arange(H2 * H1, dtype=torch.float32).reshape(H2, H1)  # every entry names its own index
    got = M.pack_w2t(w2).numpy().reshape(H1 // 32, H2 // 32 * 4, 64, 4)
    t1, s4, lane, i = np.meshgrid(np.arange(H1 // 32), np.arange(H2 // 32 * 4), np.arange(64), np.arange(4), indexing="ij")
    s = 4 * s4 + i
    want = (32 * (s // 16) + _rho(s % 16, lane >> 5)) * H1 + 32 * t1 + (lane & 31)
    assert np.array_equal(got, want.astype(np.float32))
    # and it is pack_mlp3's layer-2 pack of the transposed matrix
    ref = M.pack_mlp3(torch.zeros(H2, 3), w2.t().contiguous(), torch.zeros(1, H1), layout=0)[1]
    assert torch.equal(M.pack_w2t(w2), ref)


def _call(**kw):
    """msc_mlp_relu_backward on a valid argument set with kw replaced: (return code, msc_last_error())."""
    a = dict(x=P_, n=24, L=34, h1=64, h2=64, ko=5, w1p=P_, b1=P_, w2p=P_, b2=P_, w2tp=P_, w3=P_, d_out=P_, scale=1.0,
             acc=0, g_w1=P_, g_b1=P_, g_w2=P_, g_b2=P_, g_w3=P_, g_b3=P_, ws=P_)
    assert set(kw) <= set(a) and kw, kw  # (the valid set itself would launch)
    a.update(kw)
    L = abi.lib()
    rc = L.msc_mlp_relu_backward(a["x"], a["n"], a["L"], a["h1"], a["h2"], a["ko"], a["w1p"], a["b1"], a["w2p"], a["b2"],
                                 a["w2tp"], a["w3"], a["d_out"], C.c_float(a["scale"]), a["acc"], a["g_w1"], a["g_b1"],
                                 a["g_w2"], a["g_b2"], a["g_w3"], a["g_b3"], a["ws"], None)
    return rc, L.msc_last_error().decode()


ONE = dict(h1=96, h2=0, w2p=None, b2=None, w2tp=None, g_w2=None, g_b2=None)  # a valid one-hidden-layer set


def _arg_cases():
    for k in ("x", "w1p", "b1", "w2p", "b2", "w2tp", "w3", "d_out", "g_w1", "g_b1", "g_w2", "g_b2", "g_w3", "g_b3", "ws"):
        yield {k: None}, "null argument"
    for k in ("x", "w1p", "b1", "w3", "d_out", "g_w1", "g_b1", "g_w3", "g_b3", "ws"):
        yield dict(ONE, **{k: None}), "null argument"
    for k in ("b1", "b2", "w1p", "w2p", "w3"):
        yield {k: ODD}, "b1, b2, pre1 and the packed weights must be 16-byte aligned"
    for k in ("w2tp", "ws"):
        yield {k: ODD}, "w2tp and the workspace must be 16-byte aligned"
    yield {"n": -1}, "bad shape (n_rows -1, in_dim 34, out_dim 5)"
    yield {"L": 0}, "bad shape (n_rows 24, in_dim 0, out_dim 5)"
    yield {"L": 1025}, "bad shape (n_rows 24, in_dim 1025, out_dim 5)"
    yield {"ko": 0}, "bad shape (n_rows 24, in_dim 34, out_dim 0)"
    yield {"ko": 33}, "bad shape (n_rows 24, in_dim 34, out_dim 33)"
    for h1, h2 in ((96, 64), (64, 32), (1024, 64), (64, 96)):
        yield {"h1": h1, "h2": h2}, f"hidden sizes {h1}, {h2}: the fused MLP supports [H1, H2] with H1, H2 in {{64, 128, 256, 512}}"
    for h in (0, 16, 100, 1056):
        yield dict(ONE, h1=h), f"hidden size {h}: the fused MLP supports multiples of 32 up to 1024"


def test_every_argument_check_keeps_its_text():
    n = 0
    for bad, text in _arg_cases():
        rc, err = _call(**bad)
        assert rc == -1 and err == text, (bad, rc, err)
        n += 1
    assert n == 15 + 10 + 5 + 2 + 5 + 4 + 4


def test_no_rows_accumulate_returns_before_any_launch():
    """n_rows = 0 with accumulate = 1 adds nothing: success without touching a GPU or any pointer; the
    workspace may then be NULL."""
    assert _call(n=0, acc=1, ws=None)[0] == 0


def test_workspace_query_is_monotone_and_capped():
    for h1, h2 in [(256, 0), (32, 0), (1024, 0), (64, 64), (256, 256), (512, 512)]:
        for L, KO in ((1, 1), (34, 5), (1024, 32)):
            prev = 0
            for n in [0, 1, 31, 32, 33, 128, 129, 800, 4096, 8192, 8193, 16384, 16385, 262144, 1 << 30]:
                b = M.backward_workspace_bytes(n, L, h1, h2, KO)
                assert b >= prev and b % 16 == 0 and b > 0
                prev = b
            assert M.backward_workspace_bytes(1 << 40, L, h1, h2, KO) == prev  # capped: rows run in rounds
            hl = h2 or h1
            params = h1 * ((L + 31) // 32 * 32) + h1 + h2 * h1 + h2 + 32 * hl + 32  # the six gradients, padded
            assert prev <= 64 * 2 ** 20 + 8 * 4 * params  # the header's cap: 64 MiB of operands + 8 slices
    for bad in [(-1, 34, 64, 64, 5), (8, 0, 64, 64, 5), (8, 1025, 64, 64, 5), (8, 34, 96, 64, 5), (8, 34, 100, 0, 5),
                (8, 34, 64, 64, 33), (8, 34, 64, 64, 0)]:
        assert M.backward_workspace_bytes(*bad) == -1


def test_train_forward_refuses_cpu_tensors_and_other_dtypes():
    net = torch.nn.Sequential(torch.nn.Linear(7, 32), torch.nn.ReLU(), torch.nn.Linear(32, 3))
    with pytest.raises(RuntimeError, match="train_forward: x must be a CUDA tensor"):
        M.train_forward(net, torch.zeros(4, 7))
    with pytest.raises(RuntimeError, match="train_forward: x must be a CUDA tensor"):
        M.train_forward(net, np.zeros((4, 7), np.float32))
    assert not M.trainable(net)  # CPU parameters
    assert not M.trainable(torch.nn.Sequential(torch.nn.Linear(7, 30), torch.nn.ReLU(), torch.nn.Linear(30, 3)))


def test_learner_switch_refuses_a_cpu_module(monkeypatch):
    from marlsc.ppo import MultiAgentActorCritic, PPOConfig, PPOLearner
    from marlsc.rollout import RolloutConfig
    rc = RolloutConfig(actor={"hidden_sizes": [32]}, critic={"hidden_sizes": [32]})
    module = MultiAgentActorCritic(2, 7, 14, 3, rc, shared=True)
    cfg = PPOConfig()
    with pytest.raises(RuntimeError, match=r"PPOLearner\(fused_mlp=True\): the fused MLP backward is a HIP kernel"):
        PPOLearner(module, cfg, fused_mlp=True)
    assert PPOLearner(module, cfg).fused_mlp is False  # the default is off ...
    monkeypatch.setenv("MSC_FUSED_MLP_GRAD", "1")   # ... and None reads the knob
    with pytest.raises(RuntimeError, match=r"PPOLearner\(fused_mlp=True\)"):
        PPOLearner(module, cfg)
    assert PPOLearner(module, cfg, fused_mlp=False).fused_mlp is False
