"""GPU tests of the wide-output fused MLP (csrc/mlp_wide.hpp / mlp_wide.hip, marlsc/mlp.py:pack_wide /
wide_forward) and of msc_reward_team_sum.

Means are held to the int64 reference of oracle/mlp_ref.py on bits (integer networks with headroom
below 2^24: every float32 partial sum is exact in any order). The sampling epilogue sums a row's
log-probability terms sequentially in k after staging, as msc_gaussian_sample does, so actions, logp
and clipped are all held to bit equality with msc_gaussian_sample run on the means; logp is also held
to the float64 restatement with the bound (KO + 8) 2^-24 sum_k(quad_k + |ls_k| + 1/2 log 2 pi) (at most
7 roundings per term plus KO - 1 additions, to first order). The real-valued check anchors its tolerance
on two CPU float32 evaluations (pytest -s prints max err / tolerance)."""
import ctypes as C

import numpy as np
import pytest

torch = pytest.importorskip("torch")

from gae_ref import U32  # noqa: E402
from marlsc import abi  # noqa: E402
from marlsc import mlp as M  # noqa: E402
from mlp_emulation import live_units  # noqa: E402
from mlp_ref import (case_forward, f32_chain_forward, f32_matmul_forward, f64_forward, int_case,  # noqa: E402
                     truncate_mantissa)

pytestmark = pytest.mark.gpu
N = 161  # one full block (4 waves of 32 rows), then a block with one full wave and a wave of one row
SENTINEL = 7.25
PAD = 70  # guard rows behind every output
OUT_DIMS = [33, 40, 64, 65, 96, 128]  # 2, 2, 2, 3, 3, 4 output tiles: one row into a tile, and full tiles
HIDDEN = [(256,), (96,), (256, 256), (64, 128)]  # TB = 4 and 1 of the one-layer kernel; P = 4 passes of 2 and 1
_CASES = {}


def _hid(h):
    return "x".join(map(str, h))


def _id(v):
    return _hid(v) if isinstance(v, tuple) else str(v)


def _case(L, hidden, KO, recipe="A", n=N, group=0):
    """An integer case and its int64 outputs (conditions asserted), built once and never modified."""
    key = (L, tuple(hidden), KO, recipe, n, group)
    if key not in _CASES:
        case = int_case(L, tuple(hidden), KO, recipe, n, pre1_group=group)
        _CASES[key] = (case, case_forward(case))
    return _CASES[key]


def _dev(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _p(t):
    return None if t is None else C.c_void_p(t.data_ptr())


def _bits(a):
    if isinstance(a, torch.Tensor):
        torch.cuda.synchronize()
        a = a.cpu().numpy()
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _same(got, want_int):
    return np.array_equal(_bits(got), _bits(np.asarray(want_int).astype(np.float32)))


def _modules(case):
    """The project's MLP module holding a case's integer weights, on the GPU."""
    from marlsc.rollout import MLP
    W = case["W"]
    net = MLP(W[0].shape[1], W[-1].shape[0], {"hidden_sizes": [w.shape[0] for w in W[:-1]]})
    with torch.no_grad():
        for lin, w, b in zip(list(net)[0::2], W, case["b"]):
            lin.weight.copy_(torch.from_numpy(w))
            lin.bias.copy_(torch.from_numpy(b))
    return list(net.cuda())


class _Net:
    """A case's packed weights on the device, run through the C ABI (msc_mlp{2,3}_relu_wide)."""

    def __init__(self, case):
        W = [_dev(w) for w in case["W"]]
        self.L, self.H1 = case["W"][0].shape[1], case["W"][0].shape[0]
        self.H2 = case["W"][1].shape[0] if len(W) == 3 else 0
        self.KO = case["W"][-1].shape[0]
        self.w1p, self.w2p, self.w3p = M.pack_wide(W[0], W[1] if self.H2 else None, W[-1])
        self.b = [_dev(b) for b in case["b"]]

    def call(self, x, n, out, pre1=None, group=1, ep=None):
        lib = abi.lib()
        epp = None if ep is None else C.byref(ep)
        if self.H2:
            return lib.msc_mlp3_relu_wide(_p(x), n, self.L, self.H1, self.H2, self.KO, _p(self.w1p), _p(self.b[0]),
                                          _p(self.w2p), _p(self.b[1]), _p(self.w3p), _p(self.b[2]), _p(out), _p(pre1),
                                          group, epp, None)
        return lib.msc_mlp2_relu_wide(_p(x), n, self.L, self.H1, self.KO, _p(self.w1p), _p(self.b[0]), _p(self.w3p),
                                      _p(self.b[1]), _p(out), _p(pre1), group, epp, None)

    def forward(self, x, n, out, pre1=None, group=1, ep=None):
        abi.check(self.call(x, n, out, pre1, group, ep))
        torch.cuda.synchronize()


def _guarded(n, *tail):
    """(buffer of n + PAD rows filled with the sentinel, the guard rows behind the first n)."""
    buf = torch.full((n + PAD, *tail), SENTINEL, device="cuda")
    return buf, buf[n:]


# ---- means against int64 ----------------------------------------------------------------------------------

@pytest.mark.parametrize("L", [7, 272, 1024])
@pytest.mark.parametrize("KO", OUT_DIMS)
@pytest.mark.parametrize("hidden", HIDDEN, ids=_hid)
def test_means_equal_int64(hidden, KO, L):
    case, want = _case(L, hidden, KO)
    out, tail = _guarded(N, KO)
    _Net(case).forward(_dev(case["x"]), N, out)  # the C ABI
    assert _same(out[:N], want) and bool(torch.all(tail == SENTINEL))
    mods = _modules(case)
    assert M.wide_layers(mods) == len(hidden) + 1
    with torch.no_grad():
        assert _same(M.wide_forward(mods, _dev(case["x"])), want)  # wide_forward on the project's MLP module


@pytest.mark.parametrize("recipe", ["Bx", "Bw"])
@pytest.mark.parametrize("L,hidden,KO", [(1, (32,), 33), (7, (96,), 65), (33, (64, 64), 33), (9, (128, 64), 96),
                                         (34, (256, 256), 64), (272, (256,), 40), (672, (256,), 80),
                                         (272, (256, 256), 128), (17, (512, 512), 128), (1024, (1024,), 128)], ids=_id)
def test_wide_operands_equal_int64(L, hidden, KO, recipe):
    # operands of 12 to 20 significant bits at every layer: a product that is not exact cannot give int64
    case, want = _case(L, hidden, KO, recipe)
    with torch.no_grad():
        assert _same(M.wide_forward(_modules(case), _dev(case["x"])), want)


@pytest.mark.parametrize("hidden,n", [((64,), N), ((128,), N), ((256,), 32768), ((256,), 32768 + 33), ((512,), 32768 + 33)], ids=_id)
def test_one_layer_group_forms_equal_int64(hidden, n):
    # the one-hidden-layer kernel's groups of 2, 4 and 8 hidden tiles: 8 where the hidden size allows up to
    # 1,024 waves of 32 rows (32,768 rows), 4 past that -- both sides of the threshold, same int64 outputs
    case, want = _case(7, hidden, 40, n=n)
    out, tail = _guarded(n, 40)
    _Net(case).forward(_dev(case["x"]), n, out)
    assert _same(out[:n], want) and bool(torch.all(tail == SENTINEL))


@pytest.mark.parametrize("KO", [1, 5, 32])
@pytest.mark.parametrize("hidden", [(96,), (64, 128)], ids=_hid)
def test_one_output_tile_through_the_abi(hidden, KO):
    # the entry points accept 1 <= out_dim <= 128: the single-tile instantiations
    case, want = _case(7, hidden, KO)
    out, tail = _guarded(N, KO)
    _Net(case).forward(_dev(case["x"]), N, out)
    assert _same(out[:N], want) and bool(torch.all(tail == SENTINEL))


def test_unsupported_shapes_are_errors():
    case, _ = _case(7, (96,), 40)
    net, x, out = _Net(case), _dev(case["x"]), torch.empty((N, 40), device="cuda")
    lib = abi.lib()
    a = (_p(net.w1p), _p(net.b[0]), _p(net.w3p), _p(net.b[1]), _p(out), None, 1, None, None)
    assert lib.msc_mlp2_relu_wide(_p(x), N, 7, 96, 129, *a) != 0
    assert lib.msc_mlp2_relu_wide(_p(x), N, 7, 96, 0, *a) != 0
    assert lib.msc_mlp2_relu_wide(_p(x), N, 7, 100, 40, *a) != 0
    assert lib.msc_mlp2_relu_wide(_p(x), N, 1025, 96, 40, *a) != 0
    assert lib.msc_mlp2_relu_wide(_p(x), -1, 7, 96, 40, *a) != 0
    assert lib.msc_mlp3_relu_wide(_p(x), N, 7, 96, 64, 40, _p(net.w1p), _p(net.b[0]), _p(net.w3p), _p(net.b[0]),
                                  _p(net.w3p), _p(net.b[1]), _p(out), None, 1, None, None) != 0
    assert lib.msc_mlp2_relu_wide(_p(x), N, 7, 96, 40, _p(net.w1p), _p(net.b[0]), _p(net.w3p), _p(net.b[1]), None, None, 1,
                                  None, None) != 0  # neither out nor sample
    from marlsc.rollout import MLP
    with pytest.raises(ValueError):
        M.wide_forward(list(MLP(7, 32, {"hidden_sizes": [96]}).cuda()), x)


# ---- rows and guards ----------------------------------------------------------------------------------------

@pytest.mark.parametrize("hidden,KO", [((256,), 40), ((64, 128), 33), ((96,), 128), ((256, 256), 65)], ids=_id)
@pytest.mark.parametrize("n", [0, 1, 31, 32, 33, 161])
def test_row_counts_write_nothing_past_their_rows(n, hidden, KO):
    case, want = _case(7, hidden, KO)
    net, x = _Net(case), _dev(case["x"])
    (out, out_tail), (act, act_tail), (logp, logp_tail), (clip, clip_tail) = (_guarded(n, KO), _guarded(n, KO), _guarded(n),
                                                                            _guarded(n, KO))
    ls = torch.zeros((1, KO), device="cuda")
    eps = torch.ones((max(n, 1), KO), device="cuda")
    ep = abi.MscGaussianEpilogue(_p(ls), 1, C.c_float(-20.0), _p(eps), _p(act), _p(logp), _p(clip))
    net.forward(x, n, out, ep=ep)
    assert _same(out[:n], want[:n])
    assert _same(act[:n], want[:n] + 1)  # mean + exp(0) * 1
    assert not bool(torch.any(logp[:n] == SENTINEL))
    for t in (out_tail, act_tail, logp_tail, clip_tail):
        assert bool(torch.all(t == SENTINEL))
    means_only, tail = _guarded(n, KO)
    net.forward(x, n, means_only)
    assert np.array_equal(_bits(means_only[:n]), _bits(out[:n])) and bool(torch.all(tail == SENTINEL))


@pytest.mark.parametrize("hidden,KO", [((256,), 40), ((64, 128), 96)], ids=_id)
def test_rows_do_not_depend_on_their_position(hidden, KO):
    case, want = _case(7, hidden, KO)
    other, _ = _case(7, hidden, KO, n=N + 1)
    net = _Net(case)
    outs = []
    for off in (0, 1, 37):
        x = other["x"][:N].copy()
        x[off:off + 70] = case["x"][:70]
        out = torch.empty((N, KO), device="cuda")
        net.forward(_dev(x), N, out)
        outs.append(_bits(out)[off:off + 70])
    assert _same(outs[0].view(np.float32), want[:70])
    assert np.array_equal(outs[0], outs[1]) and np.array_equal(outs[0], outs[2])


@pytest.mark.parametrize("poison", ["nan", "inf"])
@pytest.mark.parametrize("L,hidden,KO", [(7, (256,), 40), (33, (64, 128), 65)], ids=_id)
def test_a_poisoned_row_leaves_the_others_alone(L, hidden, KO, poison):
    # odd L: the slot past a row's end is the next row's first feature. The sampled call too: the poisoned
    # rows' terms pass through the staging area of their wave.
    case, want = _case(L, hidden, KO)
    net = _Net(case)
    x = case["x"].copy()
    bad = [0, 77, N - 1]
    x[bad] = np.nan if poison == "nan" else np.where(np.arange(L) % 2 == 0, np.inf, -np.inf).astype(np.float32)
    ls, eps = torch.zeros((1, KO), device="cuda"), torch.ones((N, KO), device="cuda")
    res = []
    for xs in (case["x"], x):
        out, act, logp, clip = (torch.empty((N, KO), device="cuda"), torch.empty((N, KO), device="cuda"),
                                torch.empty((N,), device="cuda"), torch.empty((N, KO), device="cuda"))
        ep = abi.MscGaussianEpilogue(_p(ls), 1, C.c_float(-20.0), _p(eps), _p(act), _p(logp), _p(clip))
        net.forward(_dev(xs), N, out, ep=ep)
        res.append([_bits(t) for t in (out, act, logp, clip)])
    keep = np.setdiff1d(np.arange(N), bad)
    assert _same(res[0][0].view(np.float32), want)
    for clean, dirty in zip(*res):
        assert np.array_equal(clean[keep], dirty[keep])


# ---- pre1 and packing -------------------------------------------------------------------------------------------

@pytest.mark.parametrize("hidden,KO", [((256,), 40), ((64, 128), 65)], ids=_id)
@pytest.mark.parametrize("group,n", [(1, N), (8, N)])
def test_pre1_groups_equal_int64(group, n, hidden, KO):
    assert group == 1 or n % group != 0  # a partial last group (legal at the C ABI)
    case, want = _case(7, hidden, KO, n=n, group=group)
    assert case["pre1"].shape[0] == -(-n // group)
    out, tail = _guarded(n, KO)
    _Net(case).forward(_dev(case["x"]), n, out, pre1=_dev(case["pre1"]), group=group)
    assert _same(out[:n], want) and bool(torch.all(tail == SENTINEL))


def test_swapped_w3p_entries_are_seen_on_the_device():
    case, want = _case(33, (64, 64), 33)
    net = _Net(case)
    out = torch.empty((N, 33), device="cuda")
    net.forward(_dev(case["x"]), N, out)
    assert _same(out, want)
    idx, valid = (t.numpy() for t in M._wide_index(64, 33, torch.device("cpu")))
    (_, live2), _ = live_units(case)
    W3 = case["W"][-1]
    u = next(int(h) for h in np.flatnonzero(live2) if any(W3[a, h] != W3[32, h] for a in range(32)))
    a = next(a for a in range(32) if W3[a, u] != W3[32, u])
    pos = [int(np.flatnonzero((idx == row * 64 + u) & valid)[0]) for row in (a, 32)]
    w3p = net.w3p.cpu().numpy().copy()
    w3p[pos[0]], w3p[pos[1]] = w3p[pos[1]], w3p[pos[0]]
    net.w3p = _dev(w3p)
    net.forward(_dev(case["x"]), N, out)
    got = _bits(out)
    ref = _bits(want.astype(np.float32))
    assert np.any(got[:, a] != ref[:, a]) and np.any(got[:, 32] != ref[:, 32])


# ---- sampling epilogue ---------------------------------------------------------------------------------------------

def _gaussian_sample(mean, ls, floor, eps):
    n, K = mean.shape
    act, clip, logp = torch.empty((n, K), device="cuda"), torch.empty((n, K), device="cuda"), torch.empty((n,), device="cuda")
    abi.check(abi.lib().msc_gaussian_sample(_p(mean), _p(ls), ls.shape[0], C.c_float(floor), _p(eps), n, K, _p(act), _p(logp),
                                            _p(clip), None))
    torch.cuda.synchronize()
    return act, logp, clip


@pytest.mark.parametrize("hidden", [(256,), (64, 128)], ids=_hid)
@pytest.mark.parametrize("KO", [33, 40, 128])
def test_sampling_epilogue_matches_the_separate_kernel(KO, hidden):
    f = np.float32
    case, want = _case(7, hidden, KO)
    net, x = _Net(case), _dev(case["x"])
    rng = np.random.default_rng([KO, len(hidden)])
    eps_h = rng.normal(size=(N, KO)).astype(f)
    eps, mean = _dev(eps_h), _dev(want.astype(f))
    for rows, floor in ((1, -20.0), (3, 0.25), (N, -20.0), (1, 1.5)):
        ls_h = rng.uniform(-1.0, 1.0, size=(rows, KO)).astype(f)
        lsf = np.maximum(ls_h, f(floor))
        if floor == 0.25:
            assert np.any(lsf != ls_h) and np.any(lsf == ls_h)  # the floor binds on some entries (on all for 1.5)
        ls = _dev(ls_h)
        (act, at), (logp, lt), (clip, ct) = _guarded(N, KO), _guarded(N), _guarded(N, KO)
        ep = abi.MscGaussianEpilogue(_p(ls), rows, C.c_float(floor), _p(eps), _p(act), _p(logp), _p(clip))
        out = torch.empty((N, KO), device="cuda") if rows == 1 and floor == -20.0 else None
        net.forward(x, N, out, ep=ep)
        if out is not None:
            assert _same(out, want)
        for t in (at, lt, ct):
            assert bool(torch.all(t == SENTINEL))
        a_ref, lp_ref, c_ref = _gaussian_sample(mean, ls, floor, eps)
        assert np.array_equal(_bits(act[:N]), _bits(a_ref))
        assert np.array_equal(_bits(clip[:N]), _bits(c_ref))
        assert np.array_equal(_bits(logp[:N]), _bits(lp_ref))  # sequential sum in k: bit equality
        # float64 restatement on the device's actions and std (a zero-mean, unit-eps call returns std)
        sd = _gaussian_sample(torch.zeros_like(mean), ls, floor, torch.ones_like(eps))[0].cpu().numpy().astype(np.float64)
        lsr = np.tile(lsf, (-(-N // rows), 1))[:N].astype(np.float64)
        d = act[:N].cpu().numpy().astype(np.float64) - want
        quad = d * d / (2.0 * sd * sd)
        half_log_2pi = float(f(0.91893853320467274178))
        ref = (-quad - lsr - half_log_2pi).sum(axis=1)
        bound = (KO + 8) * U32 * (quad + np.abs(lsr) + half_log_2pi).sum(axis=1)
        assert np.all(np.abs(logp[:N].cpu().numpy() - ref) <= bound)
    # wide_forward with sampling on the module gives the same
    mods = _modules(case)
    ls = _dev(rng.uniform(-1.0, 1.0, size=(1, KO)).astype(f))
    act, logp, clip = torch.empty((N, KO), device="cuda"), torch.empty((N,), device="cuda"), torch.empty((N, KO), device="cuda")
    with torch.no_grad():
        assert M.wide_forward(mods, x, None, sample=(ls, -3.5, eps, act, logp, clip)) is None
    a_ref, lp_ref, c_ref = _gaussian_sample(mean, ls, -3.5, eps)
    assert np.array_equal(_bits(act), _bits(a_ref)) and np.array_equal(_bits(logp), _bits(lp_ref))
    assert np.array_equal(_bits(clip), _bits(c_ref))


# ---- real weights ------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("L,hidden,KO", [(272, (256,), 40), (672, (256, 256), 80)], ids=_id)
def test_default_initialised_wide_mlp_against_float64(L, hidden, KO):
    # tolerance: 8 x the larger maximum error of two CPU float32 evaluations against float64, asserted to be
    # at least 4 x below the error of the same network on inputs cut to a 10-bit mantissa
    # (the method of test_gpu_mlp_exact.py:test_default_initialised_mlp_against_float64)
    from marlsc.rollout import MLP
    torch.manual_seed(L + KO + len(hidden))
    net = MLP(L, KO, {"hidden_sizes": list(hidden)})
    x = torch.randn(N, L)
    W = [m.weight.detach().numpy() for m in list(net)[0::2]]
    b = [m.bias.detach().numpy() for m in list(net)[0::2]]
    ref = f64_forward(x.numpy(), W, b)
    cpu_err = max(np.abs(f(x.numpy(), W, b) - ref).max() for f in (f32_chain_forward, f32_matmul_forward))
    tol = 8.0 * cpu_err
    cut = np.abs(f64_forward(truncate_mantissa(x.numpy(), 10), W, b) - ref).max()
    assert 4.0 * tol <= cut
    with torch.no_grad():
        got = M.wide_forward(list(net.cuda()), x.cuda()).cpu().numpy()
    err = np.abs(got - ref).max()
    print(f"wide mlp {L}->{_hid(hidden)}->{KO}: max err {err:.3e} / tolerance {tol:.3e} = {err / tol:.3f} "
          f"(10-bit inputs: {cut / tol:.0f} x tolerance)")
    assert err <= tol


# ---- team reward ---------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("E", [1, 65])
@pytest.mark.parametrize("W", [1, 2, 8, 32])
def test_reward_team_sum_is_the_sequential_f64_sum(W, E):
    from marlsc.cppo import reward_team_sum
    rng = np.random.default_rng([W, E])
    r = rng.normal(size=(E, W)) * 10.0 ** rng.integers(-3, 6, size=(E, W))
    want = r[:, 0].copy()
    for w in range(1, W):
        want = want + r[:, w]
    (o32, t32), (o64, t64) = _guarded(E), (torch.full((E + PAD,), SENTINEL, dtype=torch.float64, device="cuda"), None)
    out32, out64 = reward_team_sum(_dev(r), o32[:E], o64[:E])
    torch.cuda.synchronize()
    assert np.array_equal(out64.cpu().numpy().view(np.uint64), want.view(np.uint64))
    assert np.array_equal(_bits(out32), _bits(want.astype(np.float32)))
    assert bool(torch.all(t32 == SENTINEL)) and bool(torch.all(o64[E:] == SENTINEL))
