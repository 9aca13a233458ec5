"""GPU tests that pin the fused policy-MLP kernels (csrc/mlp_kernels.hpp, mlp.hip, mlp_musigma.hip and
the fragment packing of marlsc/mlp.py) to exact references.

The integer method (oracle/mlp_ref.py): integer inputs, weights and biases whose per-layer headroom
|b| (+ |pre1|) + sum |w| |h| stays below 2^24 make every float32 partial sum exact in any order, so
the kernels' outputs are compared with an int64 numpy evaluation on bits. Every case asserts the
headroom, that 25-75 % of the hidden units are active and that the outputs differ before it compares.
tests/test_mlp_exact_host.py shows on the CPU that the method is sound and that it sees every mutant
of the packing. The real-valued check at the end anchors its tolerance on the measured error of two
CPU float32 evaluations of the same network (pytest -s prints max err / tolerance)."""
import ctypes as C
import os
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

torch = pytest.importorskip("torch")

from gae_ref import U32  # noqa: E402
from marlsc import abi  # noqa: E402
from marlsc import mlp as M  # noqa: E402
from mlp_emulation import live_units, swap_packed  # noqa: E402
from mlp_ref import (case_forward, f32_chain_forward, f32_matmul_forward, f64_forward, int_case, int_head_case,  # noqa: E402
                     truncate_mantissa)

pytestmark = pytest.mark.gpu
REPO = Path(__file__).resolve().parents[1]
N = 161  # one full block (4 waves of 32 rows), then a block with one full wave and a wave of one row
SENTINEL = 7.25
PAD = 70  # guard rows behind every output
SIZES = (64, 128, 256, 512)
PAIRS = [(a, b) for a in SIZES for b in SIZES]
ONE_LAYER = [32, 64, 96, 128, 160, 256, 768, 1024]  # TB = 1, 2, 1, 4, 1, 8, 8, 8: one and several groups of tiles
OUT_DIMS = [1, 2, 3, 5, 7, 8, 9, 32]  # VALU widths 1, 2, 4, 5, 8, 8 and the MFMA tile twice
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
    """Bit equality of a float32 result with an int64 reference (every value is below 2^24: exact)."""
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
    """A case's packed weights on the device, run through the C ABI."""

    def __init__(self, case):
        W = [_dev(w) for w in case["W"]]
        self.L, self.H1 = case["W"][0].shape[1], case["W"][0].shape[0]
        self.H2 = case["W"][1].shape[0] if len(W) == 3 else 0
        self.KO = case["W"][-1].shape[0]
        self.w1p, self.w2p, self.w3p = M.pack_mlp3(W[0], W[1] if self.H2 else None, W[-1])
        self.b = [_dev(b) for b in case["b"]]

    def forward(self, x, n, out, pre1=None, group=1, ep=None):
        lib = abi.lib()
        if self.H2:
            f = lib.msc_mlp3_relu_forward_sampled if ep is not None else lib.msc_mlp3_relu_forward
            args = (_p(x), n, self.L, self.H1, self.H2, self.KO, _p(self.w1p), _p(self.b[0]), _p(self.w2p), _p(self.b[1]),
                    _p(self.w3p), _p(self.b[2]), _p(out), _p(pre1), group)
        else:
            f = lib.msc_mlp2_relu_forward_sampled if ep is not None else lib.msc_mlp2_relu_forward
            args = (_p(x), n, self.L, self.H1, self.KO, _p(self.w1p), _p(self.b[0]), _p(self.w3p), _p(self.b[1]), _p(out),
                    _p(pre1), group)
        abi.check(f(*args, C.byref(ep), None) if ep is not None else f(*args, None))
        torch.cuda.synchronize()


def _guarded(n, *tail):
    """(buffer of n + PAD rows filled with the sentinel, the guard rows behind the first n)."""
    buf = torch.full((n + PAD, *tail), SENTINEL, device="cuda")
    return buf, buf[n:]


def _forward_modules(case):
    with torch.no_grad():
        return M.mlp3_forward(_modules(case), _dev(case["x"]))


# ---- every dispatch form ------------------------------------------------------------------------------

@pytest.mark.parametrize("KO", OUT_DIMS)
@pytest.mark.parametrize("hidden", PAIRS + [(h,) for h in ONE_LAYER], ids=_hid)
def test_every_dispatch_form_equals_int64(hidden, KO):
    # all 16 (H1, H2) branches of launch_mlp3_relu and the TB = 1, 2, 4, 8 forms of launch_mlp2_relu,
    # each with every output-layer variant (VALU 1, 2, 4, 5, 8 and the MFMA tile)
    case, want = _case(34, hidden, KO)
    assert _same(_forward_modules(case), want)


def _wide_subset():
    """Recipe B cases: every (H1, H2) pair and every one-layer TB once per variant, the output-layer
    variants cycled so that each is reached."""
    kos = [1, 2, 3, 5, 8, 9]  # VKO 1, 2, 4, 5, 8, MFMA
    forms = PAIRS + [(32,), (96,), (128,), (160,), (256,), (1024,)]
    return [(h, kos[(i + (r == "Bw")) % 6], r) for i, h in enumerate(forms) for r in ("Bx", "Bw")]


@pytest.mark.parametrize("hidden,KO,recipe", _wide_subset(), ids=_id)
def test_wide_operands_equal_int64(hidden, KO, recipe):
    # operands of 12 to 20 significant bits at every layer: a product that is not exact (an operand cut
    # to a shorter mantissa on its way into the MFMA) cannot give the int64 result
    case, want = _case(34, hidden, KO, recipe)
    assert _same(_forward_modules(case), want)


@pytest.mark.parametrize("KO", [5, 9])
@pytest.mark.parametrize("form", ["41", "21", "8", "4", "2"])
def test_pass_forms_equal_int64(monkeypatch, form, KO):
    # MSC_MLP_P8 (read at each launch): each [256, 256] pass form against int64, not against another form
    monkeypatch.setenv("MSC_MLP_P8", form)
    case, want = _case(34, (256, 256), KO)
    assert _same(_forward_modules(case), want)


def probe():
    """Run in a fresh process with MSC_MLP_V3=0 (read once per process): the MFMA output layer for
    out_dim 1, 5 and 8 on a three-layer and a two-layer form, against int64."""
    for hidden in ((256, 256), (96,)):
        for KO in (1, 5, 8):
            assert M.w3_layout(KO) == 0
            case, want = _case(34, hidden, KO)
            assert _same(_forward_modules(case), want), (hidden, KO)
    print("probe ok")


def test_mfma_output_layer_for_small_out_dim():
    paths = os.pathsep.join(str(REPO / d) for d in ("marl-sc_amd", "oracle", "tests"))
    env = dict(os.environ, MSC_MLP_V3="0", PYTHONPATH=paths)
    r = subprocess.run(["timeout", "-k", "10", "120", sys.executable, "-c", "import test_gpu_mlp_exact as t; t.probe()"],
                       env=env, capture_output=True, text=True, timeout=150)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]


# ---- input widths, row counts, stray writes -------------------------------------------------------------

@pytest.mark.parametrize("hidden", [(64, 64), (256, 256), (96,)], ids=_hid)
@pytest.mark.parametrize("L", [1, 2, 3, 7, 8, 9, 15, 16, 17, 33, 1023, 1024])
def test_input_widths_equal_int64(L, hidden):
    # the layer-1 split KS1 = ceil(L / 2), M4 = ceil(KS1 / 4): one feature, odd widths (a slot past the
    # row's end), k-step padding, and the widest input
    case, want = _case(L, hidden, 5)
    assert _same(_forward_modules(case), want)


ROWS = [0, 1, 31, 32, 33, 63, 64, 65, 127, 128, 129, 257]


@pytest.mark.parametrize("hidden,KO", [((256, 256), 5), ((64, 128), 3), ((96,), 7), ((128, 64), 9), ((160,), 32)],
                         ids=_id)
@pytest.mark.parametrize("n", ROWS)
def test_row_counts_write_nothing_past_their_rows(n, hidden, KO):
    # every output is the first n rows of a larger buffer filled with a sentinel; the sampled entry
    # points (VALU output layer) also write actions, logp and clipped
    case, want = _case(34, hidden, KO, n=257)
    net, x = _Net(case), _dev(case["x"])
    out, out_tail = _guarded(n, KO)
    if KO > 8:
        net.forward(x, n, out)
        tails = [out_tail]
    else:
        (act, act_tail), (logp, logp_tail), (clip, clip_tail) = _guarded(n, KO), _guarded(n), _guarded(n, KO)
        ls = torch.zeros((1, KO), device="cuda")
        eps = torch.ones((max(n, 1), KO), device="cuda")
        ep = abi.MscGaussianEpilogue(_p(ls), 1, C.c_float(-20.0), _p(eps), _p(act), _p(logp), _p(clip))
        net.forward(x, n, out, ep=ep)
        tails = [out_tail, act_tail, logp_tail, clip_tail]
        assert _same(act[:n], want[:n] + 1)  # mean + exp(0) * 1
        assert not bool(torch.any(logp[:n] == SENTINEL))
    assert _same(out[:n], want[:n])
    for t in tails:
        assert bool(torch.all(t == SENTINEL))


@pytest.mark.parametrize("hidden,KO", [((256, 256), 5), ((64, 64), 9), ((96,), 3)], ids=_id)
def test_rows_do_not_depend_on_their_position(hidden, KO):
    # the same 70 rows at offsets 0, 1 and 37 of the batch (other lanes, waves and blocks), among other rows
    case, want = _case(34, hidden, KO)
    other, _ = _case(34, hidden, KO, n=N + 1)
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
@pytest.mark.parametrize("L,hidden,KO", [(7, (256, 256), 5), (33, (64, 64), 9), (7, (96,), 8), (34, (128, 64), 2)],
                         ids=_id)
def test_a_poisoned_row_leaves_the_others_alone(L, hidden, KO, poison):
    # rows 0, 77 and the last replaced by NaN (or by +-Inf): with an odd L the slot past a row's end is
    # the next row's first feature, and 0 * NaN is not 0, so a missing guard on that load shows here.
    # What the poisoned rows themselves return is unspecified (include/marlsc.h) and not asserted.
    case, want = _case(L, hidden, KO)
    net = _Net(case)
    x = case["x"].copy()
    bad = [0, 77, N - 1]
    x[bad] = np.nan if poison == "nan" else np.where(np.arange(L) % 2 == 0, np.inf, -np.inf).astype(np.float32)
    clean, out = torch.empty((N, KO), device="cuda"), torch.empty((N, KO), device="cuda")
    net.forward(_dev(case["x"]), N, clean)
    net.forward(_dev(x), N, out)
    keep = np.setdiff1d(np.arange(N), bad)
    assert _same(clean, want)
    assert np.array_equal(_bits(out)[keep], _bits(clean)[keep])


# ---- pre1 -------------------------------------------------------------------------------------------------

def _pre1_rows():
    rows = []
    for g in (1, 3, 5, 32, 33, 50):
        whole = g * (N // g)
        rows.append((g, whole))
        if g > 1:
            rows.append((g, whole + max(1, g // 2)))  # a partial last group (legal at the C ABI)
    return rows


@pytest.mark.parametrize("hidden,KO", [((128, 256), 5), ((160,), 9)], ids=_id)
@pytest.mark.parametrize("group,n", _pre1_rows())
def test_pre1_groups_equal_int64(group, n, hidden, KO):
    # groups that divide a 32-row tile, straddle it (3, 5, 33, 50) or fill it, with n a multiple of the
    # group and not (mlp3_forward refuses a partial group: through the ABI)
    assert (n % group == 0) or group > 1
    case, want = _case(34, hidden, KO, n=n, group=group)
    assert case["pre1"].shape[0] == -(-n // group)
    out, tail = _guarded(n, KO)
    _Net(case).forward(_dev(case["x"]), n, out, pre1=_dev(case["pre1"]), group=group)
    assert _same(out[:n], want) and bool(torch.all(tail == SENTINEL))


# ---- sampling epilogue --------------------------------------------------------------------------------------

def _gaussian_sample(mean, ls, floor, eps):
    n, K = mean.shape
    act, clip, logp = torch.empty((n, K), device="cuda"), torch.empty((n, K), device="cuda"), torch.empty((n,), device="cuda")
    abi.check(abi.lib().msc_gaussian_sample(_p(mean), _p(ls), ls.shape[0], C.c_float(floor), _p(eps), n, K, _p(act), _p(logp),
                                            _p(clip), None))
    torch.cuda.synchronize()
    return act, logp, clip


@pytest.mark.parametrize("hidden", [(256, 256), (128, 64), (96,)], ids=_hid)  # interleaved, plain, one-layer
@pytest.mark.parametrize("KO", [1, 2, 3, 4, 5, 6, 7, 8])
def test_sampling_epilogue_matches_the_separate_kernel(KO, hidden):
    # out_dim 3, 4, 6 and 7 run on a wider VALU output layer (VKO 4 and 8): the `a < KO` guard on logp
    # and on the action stores. Means bit-equal to int64; actions / logp / clipped bit-equal to
    # msc_gaussian_sample on those means; logp also against the float64 restatement with
    # test_gaussian_sample_vs_f64's bound.
    f = np.float32
    case, want = _case(34, hidden, KO)
    net, x = _Net(case), _dev(case["x"])
    rng = np.random.default_rng([KO, len(hidden)])
    eps_h = rng.normal(size=(N, KO)).astype(f)
    eps, mean = _dev(eps_h), _dev(want.astype(f))
    for rows, floor in ((1, -20.0), (3, 0.25), (N, -20.0), (1, 1.5)):
        ls_h = rng.uniform(-1.0, 1.0, size=(rows, KO)).astype(f)
        lsf = np.maximum(ls_h, f(floor))
        if floor == 0.25:
            assert np.any(lsf != ls_h)  # the floor binds (on every entry for 1.5)
        ls = _dev(ls_h)
        (act, _), (logp, _), (clip, _) = _guarded(N, KO), _guarded(N), _guarded(N, KO)
        ep = abi.MscGaussianEpilogue(_p(ls), rows, C.c_float(floor), _p(eps), _p(act), _p(logp), _p(clip))
        out = torch.empty((N, KO), device="cuda") if rows == 1 and floor == -20.0 else None
        net.forward(x, N, out, ep=ep)
        if out is not None:
            assert _same(out, want)
        a_ref, lp_ref, c_ref = _gaussian_sample(mean, ls, floor, eps)
        assert np.array_equal(_bits(act[:N]), _bits(a_ref))
        assert np.array_equal(_bits(logp[:N]), _bits(lp_ref))
        assert np.array_equal(_bits(clip[:N]), _bits(c_ref))
        # float64 restatement on the device's actions and std (a zero-mean, unit-eps call returns std)
        sd = _gaussian_sample(torch.zeros_like(mean), ls, floor, torch.ones_like(eps))[0].cpu().numpy().astype(np.float64)
        lsr = np.tile(lsf, (-(-N // rows), 1))[:N].astype(np.float64)
        d = act[:N].cpu().numpy().astype(np.float64) - want
        quad = d * d / (2.0 * sd * sd)
        half_log_2pi = float(f(0.91893853320467274178))
        ref = (-quad - lsr - half_log_2pi).sum(axis=1)
        bound = 8 * U32 * (quad + np.abs(lsr) + half_log_2pi).sum(axis=1)
        assert np.all(np.abs(logp[:N].cpu().numpy() - ref) <= bound)


# ---- dual head ------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("hidden", [(256, 256), (96,)], ids=_hid)
@pytest.mark.parametrize("K", [1, 3, 5, 8])
def test_dual_head_equals_int64(monkeypatch, K, hidden):
    # MSC_ACT_NONE on both heads: [mu || log_std] is int64 mu and int64 sigma clamped, exactly. The clamp
    # limits sit between integers at the quartiles of sigma, so they bind on some entries and not on others.
    import marlsc.rollout as R
    case = int_head_case(34, hidden, K, N)
    want = case_forward(case)
    mu, sg = want[:, :K], want[:, K:]
    lo, hi = float(np.floor(np.percentile(sg, 25))) + 0.5, float(np.ceil(np.percentile(sg, 75))) + 0.5
    assert np.any(sg < lo) and np.any(sg > hi) and np.any((sg > lo) & (sg < hi))
    monkeypatch.setattr(R, "LOG_STD_MIN", lo)
    monkeypatch.setattr(R, "LOG_STD_MAX", hi)
    H = hidden[-1]
    actor = R.MLP(34, H, {"hidden_sizes": list(hidden)})
    head = R.MuSigmaHead(H, K)
    with torch.no_grad():
        for lin, (w, b) in zip(list(actor)[0::2] + [head.mu_head, head.sigma_head],
                               list(zip(case["W"][:-1], case["b"][:-1])) + [case["out"], case["mu"], case["sigma"]]):
            lin.weight.copy_(torch.from_numpy(w))
            lin.bias.copy_(torch.from_numpy(b))
        actor, head = actor.cuda(), head.cuda()
        assert M.musigma_tier(list(actor), head) == 1
        w_eff, b_eff = M.fold_head(list(actor)[-1], head)
        assert _same(w_eff, case["W"][-1]) and _same(b_eff, case["b"][-1])  # the fold is an exact integer matrix
        buf, tail = _guarded(N, 2 * K)
        d = M.musigma_forward(list(actor), head, _dev(case["x"]), buf[:N])
    assert bool(torch.all(tail == SENTINEL))
    assert _same(d[:, :K], mu)
    assert np.array_equal(_bits(d[:, K:]), _bits(np.clip(sg.astype(np.float32), np.float32(lo), np.float32(hi))))


# ---- the comparison is not vacuous ------------------------------------------------------------------------------

def test_swapped_w2p_entries_are_seen_on_the_device():
    # packed correctly, then two entries of w2p exchanged on the host side of the ABI call: a different
    # network, which the int64 comparison must see
    case, want = _case(34, (256, 256), 5)
    net = _Net(case)
    out = torch.empty((N, 5), device="cuda")
    net.forward(_dev(case["x"]), N, out)
    assert _same(out, want)
    (_, live2), (act1, _) = live_units(case)
    i2 = M._index_maps(34, 256, 256, 5, torch.device("cpu"), M.w3_layout(5))[2].numpy()
    w2p = swap_packed(net.w2p.cpu().numpy(), i2, np.ones_like(i2, bool), case["W"][1], int(np.flatnonzero(live2)[0]), act1)
    net.w2p = _dev(w2p)
    net.forward(_dev(case["x"]), N, out)
    assert not _same(out, want)


# ---- more than 2^31 elements ------------------------------------------------------------------------------------

def _big(L, KO, n):
    """One-layer kernel at hidden 32 over n rows of integers in [-3, 3] filled on the device in
    chunks; the last 200 rows and a strided sample of 1,000 against int64."""
    free, _ = torch.cuda.mem_get_info()
    if free < 12 << 30:
        pytest.skip(f"{free >> 30} GiB free: the case needs 12 GiB")
    assert max(n * L, n * KO) > 2 ** 31
    case = int_case(L, (32,), KO, "A", 1)
    net = _Net(case)
    g = torch.Generator(device="cuda").manual_seed(L + KO)
    x = torch.empty((n, L), device="cuda")
    step = max(1, (1 << 28) // L)
    for a in range(0, n, step):
        x[a:a + step].random_(0, 7, generator=g).sub_(3.0)
    out = torch.empty((n, KO), device="cuda")
    net.forward(x, n, out)
    idx = torch.cat([torch.arange(0, n, n // 1000)[:1000], torch.arange(n - 200, n)]).cuda()
    xs, got = x[idx].cpu().numpy(), out[idx]
    want = case_forward(dict(case, x=xs))
    ok = _same(got, want)
    del x, out, got
    torch.cuda.empty_cache()
    return ok


def test_buffers_of_more_than_2_31_elements():
    # x of 2^31 + 33 * 1024 floats (8 GiB), then, the first freed, out of 2^31 + 224 floats (8 GiB)
    assert _big(1024, 1, 2 ** 21 + 33)
    assert _big(1, 32, 2 ** 26 + 7)


# ---- real-valued check --------------------------------------------------------------------------------------------

@pytest.mark.parametrize("L,hidden,KO", [(34, (256, 256), 5), (306, (64, 64), 1), (34, (256,), 5), (306, (1024,), 1)],
                         ids=_id)
def test_default_initialised_mlp_against_float64(L, hidden, KO):
    # tolerance: 8 x the larger maximum error of two CPU float32 evaluations (a sequential fma chain and
    # numpy's matmul) against float64. All three are sums of the same number of float32 roundings in
    # different orders; their maxima over ~10^3 outputs differ by a small factor, which the 8 covers.
    # The tolerance must still see a reduced-precision product: it is asserted to be at least 4 x below
    # the error of the same network on inputs cut to a 10-bit mantissa.
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
        got = M.mlp3_forward(list(net.cuda()), x.cuda()).cpu().numpy()
    err = np.abs(got - ref).max()
    print(f"mlp {L}->{_hid(hidden)}->{KO}: max err {err:.3e} / tolerance {tol:.3e} = {err / tol:.3f} "
          f"(10-bit inputs: {cut / tol:.0f} x tolerance)")
    assert err <= tol
