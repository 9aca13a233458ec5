"""GPU tests of the multi-policy MLP kernels (msc_mlp{2,3}_relu_multi, csrc/mlp_multi.hip; the MULTI
instantiations of csrc/mlp_kernels.hpp) and of marlsc.mlp.multi_forward.

The header's contract is that policy p's rows of one multi-policy launch over rows laid out [E][P] are,
bit for bit, what the single-policy entry point returns for policy p's rows gathered contiguously. It is
checked twice: against the single-policy kernels on random float32 networks (every output compared on
its bit pattern), and, independently of those kernels, against the int64 evaluation of integer networks
under the header's 2^24 headroom condition (oracle/mlp_ref.py), with per-policy weights and per-row
inputs chosen so that a row evaluated with another policy's weights, or another row's input, gives a
different integer. Then: nothing is written past the rows, a poisoned row changes no other row, and
every violated argument condition is an error that writes nothing."""
import ctypes as C

import numpy as np
import pytest

torch = pytest.importorskip("torch")

from marlsc import abi  # noqa: E402
from marlsc import mlp as M  # noqa: E402
from mlp_ref import case_forward, int_case, int_forward  # noqa: E402

pytestmark = pytest.mark.gpu
SENTINEL = 7.25
PAD = 70  # guard rows behind every output
POLICIES = [2, 3, 8, 16]
ENVS = [1, 31, 32, 33, 65]  # one row, a partial tile, a full one, a tile and a row, two tiles and a row
HIDDEN = [(64, 64), (256, 256), (128, 64), (96,), (1024,)]
OUT_DIMS = [1, 5, 8, 9, 32]  # VALU widths 1, 5, 8 and the MFMA tile twice
IN_DIMS = [1, 7, 34]


def _hid(h):
    return "x".join(map(str, h))


def _id(v):
    return _hid(v) if isinstance(v, tuple) else str(v)


def _subset():
    """Every hidden form with every policy count, the env counts, output widths and input widths cycled
    so that each value is reached with several forms."""
    cases = []
    for i, hidden in enumerate(HIDDEN):
        for j, P in enumerate(POLICIES):
            cases.append((P, ENVS[(i + j) % 5], hidden, OUT_DIMS[(i + 2 * j) % 5], IN_DIMS[(i + j) % 3]))
    return cases


def _bits(t):
    torch.cuda.synchronize()
    return np.ascontiguousarray(t.detach().cpu().numpy(), dtype=np.float32).view(np.uint32)


def _same_bits(a, b):
    return np.array_equal(_bits(a), _bits(b))


def _p(t):
    return None if t is None else C.c_void_p(t.data_ptr())


def _nets(P, L, hidden, KO, seed):
    """P policies with different default-initialised float32 weights, on the GPU."""
    from marlsc.rollout import MLP
    torch.manual_seed(seed)
    return [list(MLP(L, KO, {"hidden_sizes": list(hidden)}).cuda()) for _ in range(P)]


def _sample_buffers(E, P, KO):
    return (torch.full((E, P, KO), SENTINEL, device="cuda"), torch.full((E, P), SENTINEL, device="cuda"),
            torch.full((E, P, KO), SENTINEL, device="cuda"))


# ---- 1. bit identity with the single-policy kernels -------------------------------------------------------------

@pytest.mark.parametrize("P,E,hidden,KO,L", _subset(), ids=_id)
def test_rows_equal_the_single_policy_kernels_bit_for_bit(P, E, hidden, KO, L):
    nets = _nets(P, L, hidden, KO, seed=1000 * P + E + KO)
    assert M.multi_layers(nets) == (3 if len(hidden) == 2 else 2)
    g = torch.Generator(device="cuda").manual_seed(E * P + L)
    x = torch.randn((E, P, L), device="cuda", generator=g)
    pre1 = torch.randn((E, P, hidden[0]), device="cuda", generator=g)
    with torch.no_grad():
        for pre in (None, pre1):
            got = M.multi_forward(nets, x, pre1=None if pre is None else pre.reshape(E * P, -1))
            assert got.shape == (E, P, KO)
            for p in range(P):
                want = M.mlp3_forward(nets[p], x[:, p].contiguous(),
                                      pre1=None if pre is None else pre[:, p].contiguous(), group=1)
                assert _same_bits(got[:, p], want), (p, pre is not None)
        if KO > 8:
            return
        eps = torch.randn((E, P, KO), device="cuda", generator=g)
        table = torch.rand((P, KO), device="cuda", generator=g) * 2.0 - 1.0  # the floor binds on some entries
        floor = -0.25
        for ls in (table[1:2].contiguous(), table):  # log_std_rows 1, then P
            act, logp, clip = _sample_buffers(E, P, KO)
            assert M.multi_forward(nets, x, None, pre1=pre1.reshape(E * P, -1), sample=(ls, floor, eps, act, logp, clip)) is None
            for p in range(P):
                a1, l1, c1 = (torch.empty((E, KO), device="cuda"), torch.empty((E,), device="cuda"),
                              torch.empty((E, KO), device="cuda"))
                row = ls if ls.shape[0] == 1 else ls[p:p + 1].contiguous()
                M.mlp3_forward(nets[p], x[:, p].contiguous(), None, pre1=pre1[:, p].contiguous(), group=1,
                               sample=(row, floor, eps[:, p].contiguous(), a1, l1, c1))
                assert _same_bits(act[:, p], a1) and _same_bits(logp[:, p], l1) and _same_bits(clip[:, p], c1), (p, ls.shape)


@pytest.mark.parametrize("order", ["0", "1"])
def test_block_orders_give_the_same_bits(monkeypatch, order):
    # MSC_MULTI_ORDER (read at each launch): policy-major and policy-minor blocks, several blocks per policy
    P, E, L, KO = 8, 161, 34, 5
    nets = _nets(P, L, (256, 256), KO, seed=5)
    x = torch.randn((E, P, L), device="cuda", generator=torch.Generator(device="cuda").manual_seed(9))
    monkeypatch.setenv("MSC_MULTI_ORDER", order)
    with torch.no_grad():
        got = M.multi_forward(nets, x)
        for p in range(P):
            assert _same_bits(got[:, p], M.mlp3_forward(nets[p], x[:, p].contiguous())), p


# ---- 2. integer ground truth, independent of the single-policy kernels -------------------------------------------

def _int_policies(P, E, L, hidden, KO):
    """Policy p = int_case with seed p + 1: its own integer weights, biases, input rows and pre1 rows.
    Returns (modules, x [E, P, L], pre1 [E P, H1], want [E, P, KO] int64) after asserting that the
    weights and the rows identify themselves: row (e, p) evaluated with another policy's weights, with
    the input of the same env's next policy or with the next env's input gives another integer vector."""
    from marlsc.rollout import MLP
    cases = [int_case(L, hidden, KO, "A", E, seed=p + 1, pre1_group=1) for p in range(P)]
    want = np.stack([case_forward(c) for c in cases], axis=1)
    for p, c in enumerate(cases):
        q = cases[(p + 1) % P]
        wrong_w = int_forward(c["x"], q["W"], q["b"], c["pre1"], 1)[0]
        wrong_x = int_forward(q["x"], c["W"], c["b"], c["pre1"], 1)[0]
        assert np.all(np.any(wrong_w != want[:, p], axis=1)) and np.all(np.any(wrong_x != want[:, p], axis=1))
        if E > 1:
            shifted = int_forward(np.roll(c["x"], 1, axis=0), c["W"], c["b"], c["pre1"], 1)[0]
            assert np.all(np.any(shifted != want[:, p], axis=1))
    nets = []
    for c in cases:
        net = MLP(L, KO, {"hidden_sizes": list(hidden)})
        with torch.no_grad():
            for lin, w, b in zip(list(net)[0::2], c["W"], c["b"]):
                lin.weight.copy_(torch.from_numpy(w))
                lin.bias.copy_(torch.from_numpy(b))
        nets.append(list(net.cuda()))
    x = torch.from_numpy(np.stack([c["x"] for c in cases], axis=1)).cuda()
    pre1 = torch.from_numpy(np.stack([c["pre1"] for c in cases], axis=1)).cuda().reshape(E * P, hidden[0])
    return nets, x, pre1, want


@pytest.mark.parametrize("hidden,KO", [((64, 64), 5), ((64, 64), 9), ((256, 256), 5), ((128, 64), 32), ((96,), 3),
                                       ((1024,), 9)], ids=_id)
def test_integer_networks_equal_int64(hidden, KO):
    # both output-layer layouts (VALU for 3 and 5 outputs, MFMA for 9 and 32), the interleaved pass form of
    # [256, 256] and both one-hidden-layer output layers; 3 policies x 33 envs: a full tile and one row
    P, E, L = 3, 33, 7
    nets, x, pre1, want = _int_policies(P, E, L, hidden, KO)
    with torch.no_grad():
        got = M.multi_forward(nets, x, pre1=pre1)
    assert np.array_equal(_bits(got), _bits(torch.from_numpy(want.astype(np.float32))))


# ---- 3. nothing past the rows ------------------------------------------------------------------------------------

@pytest.mark.parametrize("hidden,KO", [((256, 256), 5), ((128, 64), 9), ((96,), 8)], ids=_id)
def test_every_row_is_written_and_nothing_behind_them(hidden, KO):
    P, E, L = 3, 33, 7
    n = E * P
    nets, x, pre1, want = _int_policies(P, E, L, hidden, KO)
    out = torch.full((n + PAD, KO), SENTINEL, device="cuda")
    bufs = [out]
    sample = None
    if KO <= 8:
        act, logp, clip = (torch.full((n + PAD, KO), SENTINEL, device="cuda"), torch.full((n + PAD,), SENTINEL, device="cuda"),
                           torch.full((n + PAD, KO), SENTINEL, device="cuda"))
        ls, eps = torch.zeros((P, KO), device="cuda"), torch.ones((n, KO), device="cuda")
        sample = (ls, -20.0, eps, act[:n], logp[:n], clip[:n])
        bufs += [act, logp, clip]
    with torch.no_grad():
        M.multi_forward(nets, x, out[:n], pre1=pre1, sample=sample)
    torch.cuda.synchronize()
    for b in bufs:
        assert bool(torch.all(b[n:] == SENTINEL))
    # integer means, and with log_std 0 and eps 1 integer actions: a sentinel of 7.25 cannot survive a write
    assert np.array_equal(_bits(out[:n]), _bits(torch.from_numpy(want.reshape(n, KO).astype(np.float32))))
    if sample is not None:
        assert np.array_equal(_bits(act[:n]), _bits(torch.from_numpy((want.reshape(n, KO) + 1).astype(np.float32))))
        assert not bool(torch.any(logp[:n] == SENTINEL))
        assert bool(torch.all(clip[:n].abs() <= 1.0))


# ---- 4. isolation ------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("poison", ["nan", "inf"])
@pytest.mark.parametrize("hidden,KO", [((256, 256), 5), ((64, 64), 9), ((96,), 8)], ids=_id)
def test_a_poisoned_row_leaves_every_other_row_alone(hidden, KO, poison):
    # rows (env 0, policy 1), (env 17, policy 1) and the last row poisoned, in x and in pre1: the rows of
    # policy 1 in the same 32-row tile and the rows of the other policies at the same envs must not move.
    # L is odd, so the slot past a row's end is the next row's first feature (another policy's row).
    P, E, L = 3, 33, 7
    nets, x, pre1, want = _int_policies(P, E, L, hidden, KO)
    bad = [(0, 1), (17, 1), (E - 1, P - 1)]
    xb, pb = x.clone(), pre1.clone().reshape(E, P, -1)
    fill = float("nan") if poison == "nan" else float("inf")
    for e, p in bad:
        xb[e, p] = fill
        xb[e, p, 1::2] = -fill if poison == "inf" else fill
        pb[e, p] = fill
    with torch.no_grad():
        clean = M.multi_forward(nets, x, pre1=pre1)
        got = M.multi_forward(nets, xb, pre1=pb.reshape(E * P, -1))
    keep = np.ones((E, P), bool)
    for e, p in bad:
        keep[e, p] = False
    assert np.array_equal(_bits(clean), _bits(torch.from_numpy(want.astype(np.float32))))
    assert np.array_equal(_bits(got)[keep], _bits(clean)[keep])


# ---- 5. argument errors -------------------------------------------------------------------------------------------

def test_violated_conditions_are_errors_that_write_nothing():
    P, E, L, H, KO = 3, 4, 7, 64, 5
    n = E * P
    lib = abi.lib()
    z = lambda *s: torch.zeros(s, device="cuda")  # noqa: E731
    x, w1p, w2p, w3p = z(n + 4, L), z(P * 64 * 64 * 4), z(P * H * H), z(P * H * 16)
    b1, b2, b3, pre1 = z(P * H), z(P * H), z(P * 32), z(n + 4, H)
    out = torch.full((n + 4, 32), SENTINEL, device="cuda")
    act, logp, clip = torch.full((n + 4, 8), SENTINEL, device="cuda"), torch.full((n + 4,), SENTINEL, device="cuda"), \
        torch.full((n + 4, 8), SENTINEL, device="cuda")
    ls, eps = z(P, 8), z(n + 4, 8)

    def ep(rows):
        return C.byref(abi.MscGaussianEpilogue(_p(ls), rows, C.c_float(-20.0), _p(eps), _p(act), _p(logp), _p(clip)))

    def f3(rows=n, pol=P, h1=H, h2=H, ko=KO, sample=None):
        return lib.msc_mlp3_relu_multi(_p(x), rows, pol, L, h1, h2, ko, _p(w1p), _p(b1), _p(w2p), _p(b2), _p(w3p), _p(b3),
                                       _p(out), _p(pre1), sample, None)

    def f2(rows=n, pol=P, h1=H, ko=KO, sample=None):
        return lib.msc_mlp2_relu_multi(_p(x), rows, pol, L, h1, ko, _p(w1p), _p(b1), _p(w3p), _p(b3), _p(out), _p(pre1),
                                       sample, None)

    for f in (f3, f2):
        assert f(rows=n + 1) != 0 and b"multiple" in lib.msc_last_error()
        assert f(pol=0) != 0 and b"n_policies" in lib.msc_last_error()
        assert f(rows=65 * 2, pol=65) != 0 and b"n_policies" in lib.msc_last_error()
        assert f(sample=ep(2)) != 0 and b"log_std_rows" in lib.msc_last_error()
        assert f(sample=ep(0)) != 0 and b"log_std_rows" in lib.msc_last_error()
        assert f(ko=9, sample=ep(P)) != 0 and b"VALU output layer" in lib.msc_last_error()
        assert f(h1=48) != 0 and b"hidden size" in lib.msc_last_error()
    assert f3(h2=48) != 0 and f3(h2=0) != 0
    assert lib.msc_mlp3_relu_multi(_p(x), n, P, L, H, H, KO, _p(w1p), _p(b1), _p(w2p), _p(b2), _p(w3p), _p(b3), None,
                                   None, None, None) != 0  # neither out nor sample
    torch.cuda.synchronize()
    for t in (out, act, logp, clip):
        assert bool(torch.all(t == SENTINEL))
    # the same buffers with nothing violated: the call goes through and writes
    assert f3(sample=ep(P)) == 0 and f2(sample=ep(1)) == 0
    torch.cuda.synchronize()
    flat = out.view(-1)  # n rows of KO floats from the start of the buffer
    assert not bool(torch.any(flat[:n * KO] == SENTINEL)) and bool(torch.all(flat[n * KO:] == SENTINEL))
