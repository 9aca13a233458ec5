"""GPU tests that pin the dual mu / sigma-head kernels (msc_mlp{2,3}_relu_musigma: the EP = MlpMuSigma
instantiations of csrc/mlp_musigma.hip, musigma_row and head_act in csrc/mlp_kernels.hpp) to exact
references, through the C ABI. The method is tests/musigma_emulation.py's (numpy and math only):

* integer part: [mu || log_std] on bits against int64, sigma clamped at limits between integers;
* dyadic part: the folded head scaled by powers of two, so every pre-activation is a known number;
  head_act against float64 within 4 max(e32, 1) units of 2^-24 s_f(v), NONE / RELU / ELU's positive
  branch and the clamp limits on bits;
* sampling: actions, logp and clipped bit-equal to msc_gaussian_sample on the launch's own dist_out
  (one log_std row per row, floor = log_std_min), with dist_out given and with NULL.

Every launch writes into buffers with 70 guard rows of a sentinel; eps carries other draws behind each
row. tests/test_musigma_exact_host.py shows on the CPU that these checks see every mutant of
musigma_row. pytest -s prints error / bound per activation.

Instantiations (launch_mlp3_musigma / launch_mlp2_musigma: form x per-head width 2 / 4 / 5 / 8) and
the integer-exact cases that reach them, all with sampling:
  16 (H1, H2) branches x widths 2, 4, 5, 8
      test_two_layer_forms_equal_int64: K = 1..8 run as width 2, 2, 4, 4, 5, 8, 8, 8 on every pair
      ([256, 256] in its default form, MSC_MLP_P8 = 41)
  [256, 256] pass forms MSC_MLP_P8 = 41, 21 (interleaved) and 8 (one pass) x widths 2, 4, 5, 8
      test_pass_forms_equal_int64: K = 1, 3, 5, 7
  one layer, TB = 1 (32, 96, 160, 544), 2 (64), 4 (128), 8 (256, 512, 1024) x widths 2, 4, 5, 8
      test_one_layer_forms_equal_int64: K = 1..8 (544 and 1024: K <= 4; above, refused)
Padded K (1, 3, 6, 7) with sampling: on every two-layer pair, on both interleaved forms (K = 1, 3, 7) and
on every one-layer TB. Activations, row counts, pre1, input widths and the whp mutants reuse these forms.
"""
import ctypes as C

import numpy as np
import pytest

torch = pytest.importorskip("torch")

import musigma_emulation as E  # noqa: E402
from marlsc import abi  # noqa: E402
from marlsc import mlp as M  # noqa: E402
from musigma_emulation import N, PAD, SAMPLE_LIMITS, SENTINEL  # noqa: E402
from test_gpu_mlp_exact import PAIRS, ROWS, _bits, _dev, _guarded, _hid, _id, _p, _pre1_rows, _same  # noqa: E402

import test_gpu_mlp_exact as X  # noqa: E402

assert (N, PAD, SENTINEL) == (X.N, X.PAD, X.SENTINEL)  # the plain-MLP file's row count, guard rows and sentinel
pytestmark = pytest.mark.gpu
ONE_LAYER = [32, 96, 64, 128, 160, 256, 512, 544, 1024]  # TB = 1, 1, 2, 4, 1, 8, 8, 1, 8
KS = [1, 2, 3, 4, 5, 6, 7, 8]
DEFAULT = (-4.6, 4.6)
_HEADS = {}


class _Head:
    """A case's packed weights on the device and the dual-head entry points."""

    def __init__(self, case, K):
        W = case["W"]
        self.K, self.L, self.H1 = K, W[0].shape[1], W[0].shape[0]
        self.H2 = W[1].shape[0] if len(W) == 3 else 0
        w_eff = _dev(W[-1])
        self.w1p, self.w2p, _ = M.pack_mlp3(_dev(W[0]), _dev(W[1]) if self.H2 else None, w_eff, layout=0)
        self.width, self.stride = M.musigma_layout(self.H1, self.H2, K)
        idx, valid = M._head_index(W[-1].shape[1], K, self.stride, w_eff.device)
        self.valid = valid
        self.whp = torch.where(valid, w_eff.reshape(-1)[idx], torch.zeros((), device="cuda")).contiguous()
        self.b = [_dev(b) for b in case["b"]]
        self.pre1, self.group = _dev(case["pre1"]), case["group"]

    def call(self, x, n, ep, pre1=None, group=1):
        lib = abi.lib()
        if self.H2:
            return lib.msc_mlp3_relu_musigma(_p(x), n, self.L, self.H1, self.H2, self.K, _p(self.w1p), _p(self.b[0]),
                                             _p(self.w2p), _p(self.b[1]), _p(self.whp), _p(self.b[2]), _p(pre1), group,
                                             C.byref(ep), None)
        return lib.msc_mlp2_relu_musigma(_p(x), n, self.L, self.H1, self.K, _p(self.w1p), _p(self.b[0]), _p(self.whp),
                                         _p(self.b[1]), _p(pre1), group, C.byref(ep), None)

    def run(self, x, n, acts, lim, eps=None, dist=True):
        """One launch into fresh guarded buffers: {"dist", "act", "logp", "clip"} (None where not asked for)."""
        K = self.K
        out = {k: None for k in ("dist", "act", "logp", "clip")}
        if dist:
            out["dist"] = _guarded(n, 2 * K)[0]
        if eps is not None:
            out["act"], out["logp"], out["clip"] = _guarded(n, K)[0], _guarded(n)[0], _guarded(n, K)[0]
        ep = abi.MscMuSigmaEpilogue(acts[0], acts[1], C.c_float(lim[0]), C.c_float(lim[1]), _p(eps), _p(out["act"]),
                                    _p(out["logp"]), _p(out["clip"]), _p(out["dist"]))
        abi.check(self.call(x, n, ep, self.pre1, self.group))
        torch.cuda.synchronize()
        return out


def _head(case, K, key=None):
    if key is None:
        return _Head(case, K)
    key = key + (M.musigma_layout(case["W"][0].shape[0], case["W"][1].shape[0] if len(case["W"]) == 3 else 0, K),)
    if key not in _HEADS:
        _HEADS[key] = _Head(case, K)
    return _HEADS[key]


def _tails_clean(out, n):
    return all(bool(torch.all(t[n:] == SENTINEL)) and t.shape[0] == n + PAD for t in out.values() if t is not None)


def _gaussian_sample(dist, n, K, floor, eps):
    mean, ls = dist[:n, :K].contiguous(), dist[:n, K:].contiguous()
    act, clip, logp = torch.empty((n, K), device="cuda"), torch.empty((n, K), device="cuda"), torch.empty((n,), device="cuda")
    abi.check(abi.lib().msc_gaussian_sample(_p(mean), _p(ls), n, C.c_float(floor), _p(eps), n, K, _p(act), _p(logp), _p(clip),
                                            None))
    torch.cuda.synchronize()
    return {"act": act, "logp": logp, "clip": clip}


def _same_bits(a, b):
    return np.array_equal(_bits(a), _bits(b))


def _full(head, x, v, n, acts, lim_dist, lim_sample, label=None):
    """The three forms of one case on rows [0, n): dist_out only (clamp lim_dist), sampling with dist_out
    and sampling with dist_out = NULL (clamp lim_sample). dist_out by check_dist on the exact
    pre-activations v; the samples bit-equal to msc_gaussian_sample on the launch's dist_out, and the
    same with NULL; every guard row untouched. Returns the sampling launch's outputs."""
    K = head.K
    eps = _dev(E.eps_buffer(N if n <= N else n, K))
    only = head.run(x, n, acts, lim_dist, None, True)
    both = head.run(x, n, acts, lim_sample, eps, True)
    null = head.run(x, n, acts, lim_sample, eps, False)
    for out in (only, both, null):
        assert _tails_clean(out, n)
    if n == 0:
        return both
    reps = []
    for out, lim in ((only, lim_dist), (both, lim_sample)):
        rep = E.check_dist(out["dist"][:n].cpu().numpy(), v[:n], K, acts[0], acts[1], *lim)
        assert rep["ok"], rep["why"]
        reps.append(rep)
    ref = _gaussian_sample(both["dist"], n, K, lim_sample[0], eps)
    for k in ("act", "logp", "clip"):
        assert _same_bits(both[k][:n], ref[k]), k
        assert _same_bits(null[k][:n], both[k][:n]), k
    assert null["dist"] is None and bool(torch.all(torch.isfinite(both["logp"][:n])))
    if label:
        print(f"{label}: error / bound mu {max(r['mu'] for r in reps):.3f} sigma {max(r['sigma'] for r in reps):.3f} "
              f"(e32 {reps[0]['e32']['mu']:.2f}, {reps[0]['e32']['sigma']:.2f})")
    return both


def _int_full(L, hidden, K, n=N, rows=N, group=0, share=True):
    """The integer part of one shape: quartile limits for the dist_out launch, SAMPLE_LIMITS when sampling."""
    case, want = E.head_case(L, hidden, K, rows, group)
    sg = want[:, K:]
    lim = E.int_limits(sg)
    lo, hi = SAMPLE_LIMITS
    assert np.any(sg < lo) and np.any(sg > hi) and np.any((sg > lo) & (sg < hi))
    head = _head(case, K, (L, tuple(hidden), K, rows, group) if share else None)
    return _full(head, _dev(case["x"]), want.astype(np.float64), n, (0, 0), lim, SAMPLE_LIMITS)


# ---- every dispatch form x every K --------------------------------------------------------------------------

@pytest.mark.parametrize("K", KS)
@pytest.mark.parametrize("hidden", PAIRS, ids=_hid)
def test_two_layer_forms_equal_int64(hidden, K):
    _int_full(34, hidden, K)


@pytest.mark.parametrize("K", KS)
@pytest.mark.parametrize("H", ONE_LAYER)
def test_one_layer_forms_equal_int64(H, K):
    refused = H in (544, 1024) and K >= 5  # more than 32 KiB of staged head weights
    assert (M.musigma_layout(H, 0, K) is None) == refused
    assert (H * 4 * (8 if K <= 4 else 16) > 32768) == refused
    if not refused:
        _int_full(34, (H,), K)
        return
    # no kernel: the tier is the torch layers', the ABI call returns an error and writes nothing
    import marlsc.rollout as R
    actor, head = R.MLP(34, H, {"hidden_sizes": [H]}), R.MuSigmaHead(H, K)
    assert M.musigma_tier(list(actor), head) == 3
    z = torch.zeros(1 << 16, device="cuda")
    bufs = {k: _guarded(N, w)[0] for k, w in (("dist", 2 * K), ("act", K), ("clip", K))}
    bufs["logp"] = _guarded(N)[0]
    ep = abi.MscMuSigmaEpilogue(0, 0, C.c_float(-4.6), C.c_float(4.6), _p(z), _p(bufs["act"]), _p(bufs["logp"]),
                                _p(bufs["clip"]), _p(bufs["dist"]))
    rc = abi.lib().msc_mlp2_relu_musigma(_p(z), N, 34, H, K, _p(z), _p(z), _p(z), _p(z), None, 1, C.byref(ep), None)
    torch.cuda.synchronize()
    assert rc != 0 and all(bool(torch.all(t == SENTINEL)) for t in bufs.values())


def test_layout_limits_are_exactly_32_kib():
    # 1024 units for K <= 4 and 512 for K = 5..8 stage exactly 32 KiB; the next multiple of 32 is refused
    for K in KS:
        top = 1024 if K <= 4 else 512
        w, s = M.musigma_layout(top, 0, K)
        assert (w, s) == (E.head_width(K), 8 if K <= 4 else 16) and top * s * 4 == 32768
        assert M.musigma_layout(top + 32, 0, K) is None
        assert all(M.musigma_layout(a, b, K) == (w, s) for a, b in PAIRS)
    assert M.musigma_layout(64, 64, 0) is None and M.musigma_layout(64, 64, 9) is None


@pytest.mark.parametrize("K", [1, 3, 5, 7])
@pytest.mark.parametrize("form", ["41", "21", "8"])
def test_pass_forms_equal_int64(monkeypatch, form, K):
    # MSC_MLP_P8 (read at each launch): both interleaved forms and the one-pass form of [256, 256]
    # against int64, not against each other
    monkeypatch.setenv("MSC_MLP_P8", form)
    _int_full(34, (256, 256), K)


# ---- activations ---------------------------------------------------------------------------------------------

def _act_case(L, hidden, K, am, asg):
    case = E.dyadic_case(L, hidden, K)
    for part in (case["v"][:, :K], case["v"][:, K:]):
        assert all(E.coverage(part).values()), E.coverage(part)
    ref = E.act64(asg, case["v"][:, K:])
    assert np.any(np.abs(ref) > 0.25) and np.any(np.abs(ref) < 0.25)  # -+0.25 binds on some entries, not on others
    head = _head(case, K, ("dyadic", L, tuple(hidden), K))
    tag = f"musigma {_hid(hidden)} K={K} mu={E.ACT_NAMES[am]} sigma={E.ACT_NAMES[asg]}"
    x = _dev(case["x"])
    _full(head, x, case["v"], N, (am, asg), DEFAULT, DEFAULT, tag + " clamp 4.6")
    _full(head, x, case["v"], N, (am, asg), (-0.25, 0.25), (-0.25, 0.25), tag + " clamp 0.25")


@pytest.mark.parametrize("asg", range(6), ids=E.ACT_NAMES)
@pytest.mark.parametrize("am", range(6), ids=E.ACT_NAMES)
@pytest.mark.parametrize("hidden,K", [((64, 64), 3), ((96,), 7)], ids=_id)
def test_every_activation_pair_within_the_bound(hidden, K, am, asg):
    _act_case(34, hidden, K, am, asg)


@pytest.mark.parametrize("act", range(6), ids=E.ACT_NAMES)
@pytest.mark.parametrize("hidden,K", [((256, 256), 5), ((512,), 8)], ids=_id)
def test_activations_on_the_widest_forms(hidden, K, act):
    _act_case(34, hidden, K, act, act)


@pytest.mark.parametrize("codes", [(6, 0), (0, 6), (-1, 0), (0, -1), (2, 255)], ids=str)
def test_an_unknown_activation_code_is_refused(codes):
    # capi.hip refuses codes outside MSC_ACT_* 0..5 (it does not run them as NONE): nothing is written
    for hidden, K in (((64, 64), 3), ((96,), 7)):
        case, _ = E.head_case(34, hidden, K)
        head = _head(case, K, (34, hidden, K, N, 0))
        out = {"dist": _guarded(N, 2 * K)[0], "act": _guarded(N, K)[0], "logp": _guarded(N)[0], "clip": _guarded(N, K)[0]}
        ep = abi.MscMuSigmaEpilogue(codes[0], codes[1], C.c_float(-4.6), C.c_float(4.6), _p(_dev(E.eps_buffer(N, K))),
                                    _p(out["act"]), _p(out["logp"]), _p(out["clip"]), _p(out["dist"]))
        assert head.call(_dev(case["x"]), N, ep) != 0 and b"activation" in abi.lib().msc_last_error()
        torch.cuda.synchronize()
        assert all(bool(torch.all(t == SENTINEL)) for t in out.values())


# ---- row counts, stray writes ------------------------------------------------------------------------------------

@pytest.mark.parametrize("hidden,K", [((256, 256), 5), ((64, 128), 3), ((96,), 7), ((128,), 1)], ids=_id)
@pytest.mark.parametrize("n", ROWS)
def test_row_counts_write_nothing_past_their_rows(n, hidden, K):
    # dist_out only, sampling only and both on the first n of 257 rows; sentinels behind all four
    # buffers (n = 0: nothing is touched at all)
    _int_full(34, hidden, K, n=n, rows=257)


# ---- row independence, poisoned rows --------------------------------------------------------------------------------

ODD = [(7, (256, 256), 5), (33, (64, 64), 3), (7, (96,), 7), (33, (128, 64), 2)]
TANH_MU = (2, 0)


def _four(out, rows):
    return [_bits(out[k])[rows] for k in ("dist", "act", "logp", "clip")]


@pytest.mark.parametrize("L,hidden,K", ODD, ids=_id)
def test_rows_do_not_depend_on_their_position(L, hidden, K):
    # the same 70 rows (and their eps) at offsets 0, 1 and 37 of the batch, among other rows: tanh on mu,
    # sampling on, all four outputs
    case = E.dyadic_case(L, hidden, K)
    other, _ = E.head_case(L, hidden, K, N + 1)
    head = _head(case, K, ("dyadic", L, tuple(hidden), K))
    eps0, got = E.eps_buffer(N, K), []
    for off in (0, 1, 37):
        x, eps = other["x"][:N].copy(), E.eps_buffer(N, K, 1)
        x[off:off + 70], eps[off:off + 70] = case["x"][:70], eps0[:70]
        out = head.run(_dev(x), N, TANH_MU, DEFAULT, _dev(eps), True)
        got.append(_four(out, slice(off, off + 70)))
    rep = E.check_dist(got[0][0].view(np.float32), case["v"][:70], K, *TANH_MU, *DEFAULT)
    assert rep["ok"], rep["why"]
    for k in range(4):
        assert np.array_equal(got[0][k], got[1][k]) and np.array_equal(got[0][k], got[2][k])


@pytest.mark.parametrize("poison", ["nan", "inf"])
@pytest.mark.parametrize("L,hidden,K", ODD, ids=_id)
def test_a_poisoned_row_leaves_the_others_alone(L, hidden, K, poison):
    # rows 0, 77 and the last replaced by NaN (or +-Inf): with an odd L the slot past a row's end is the
    # next row's first feature. What the poisoned rows return is unspecified and not asserted.
    case = E.dyadic_case(L, hidden, K)
    head = _head(case, K, ("dyadic", L, tuple(hidden), K))
    x, bad = case["x"].copy(), [0, 77, N - 1]
    x[bad] = np.nan if poison == "nan" else np.where(np.arange(L) % 2 == 0, np.inf, -np.inf).astype(np.float32)
    eps = _dev(E.eps_buffer(N, K))
    clean = head.run(_dev(case["x"]), N, TANH_MU, DEFAULT, eps, True)
    out = head.run(_dev(x), N, TANH_MU, DEFAULT, eps, True)
    keep = np.setdiff1d(np.arange(N), bad)
    rep = E.check_dist(clean["dist"][:N].cpu().numpy(), case["v"], K, *TANH_MU, *DEFAULT)
    assert rep["ok"], rep["why"]
    for a, b in zip(_four(clean, keep), _four(out, keep)):
        assert np.array_equal(a, b)
    assert _tails_clean(out, N)


# ---- pre1, input widths ------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("hidden,K", [((128, 256), 4), ((160,), 6)], ids=_id)
@pytest.mark.parametrize("group,n", _pre1_rows())
def test_pre1_groups_equal_int64(group, n, hidden, K):
    # groups that divide a 32-row tile, straddle it or fill it, whole and with a partial last group
    case, _ = E.head_case(34, hidden, K, n, group)
    assert case["pre1"].shape[0] == -(-n // group) and case["group"] == group
    _int_full(34, hidden, K, n=n, rows=n, group=group, share=False)


@pytest.mark.parametrize("hidden,K", [((64, 64), 2), ((96,), 8)], ids=_id)
@pytest.mark.parametrize("L", [1, 2, 3, 15, 16, 17, 33, 1024])
def test_input_widths_equal_int64(L, hidden, K):
    _int_full(L, hidden, K, share=False)


# ---- folded tier ------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("hidden", [(64, 64), (96,)], ids=_hid)
@pytest.mark.parametrize("K", [9, 16])
def test_folded_tier_equals_int64(monkeypatch, K, hidden):
    # 9..16 actions: the plain fused MLP on the folded weights. mu and the unclamped sigma against int64;
    # head_sample's outputs against msc_gaussian_sample on musigma_folded's (clamped) distribution inputs
    import marlsc.rollout as R
    case, want = E.head_case(34, hidden, K)
    H = hidden[-1]
    actor, head = R.MLP(34, H, {"hidden_sizes": list(hidden)}), R.MuSigmaHead(H, K)
    with torch.no_grad():
        for lin, (w, b) in zip(list(actor)[0::2] + [head.mu_head, head.sigma_head],
                               list(zip(case["W"][:-1], case["b"][:-1])) + [case["out"], case["mu"], case["sigma"]]):
            lin.weight.copy_(torch.from_numpy(w))
            lin.bias.copy_(torch.from_numpy(b))
        actor, head = actor.cuda(), head.cuda()
        assert M.musigma_tier(list(actor), head) == 2
        x = _dev(case["x"])
        monkeypatch.setattr(R, "LOG_STD_MIN", -float(1 << 24))
        monkeypatch.setattr(R, "LOG_STD_MAX", float(1 << 24))
        mu, ls = M.musigma_folded(list(actor), head, x)
        assert _same(mu, want[:, :K]) and _same(ls, want[:, K:])
        monkeypatch.undo()
        mu, ls = M.musigma_folded(list(actor), head, x)
        sg = want[:, K:]
        assert np.any(sg < -4.6) and np.any(sg > 4.6) and np.any(np.abs(sg) < 4.6)
        assert _same(mu, want[:, :K]) and _same_bits(ls, np.clip(sg.astype(np.float32), np.float32(-4.6), np.float32(4.6)))
        eps = _dev(E.eps_buffer(N, K))[:N].contiguous()
        act, logp = _guarded(N, K)[0], _guarded(N)[0]
        clip = R.head_sample(actor, head, x, eps, act[:N], logp[:N])
        ref = _gaussian_sample(torch.cat([mu, ls], dim=1), N, K, R.LOG_STD_MIN, eps)
    assert _same_bits(act[:N], ref["act"]) and _same_bits(logp[:N], ref["logp"]) and _same_bits(clip, ref["clip"])
    assert bool(torch.all(act[N:] == SENTINEL)) and bool(torch.all(logp[N:] == SENTINEL))
    assert bool(torch.all(torch.isfinite(logp[:N])))


# ---- the comparison is not vacuous ---------------------------------------------------------------------------------------------

@pytest.mark.parametrize("hidden,K", [((64, 64), 3), ((96,), 7), ((256, 256), 5)], ids=_id)
def test_swapped_and_padded_whp_columns(hidden, K):
    # packed correctly, then on the host side of the ABI call (1) mu column 0 exchanged with sigma column 0
    # of whp: another network, which the comparison must see; (2) a non-zero value in every padded column
    # (c mod stride / 2 >= K): the kernel sums them into registers it never stores, so nothing may change
    case, want = E.head_case(34, hidden, K)
    head = _Head(case, K)
    x, v = _dev(case["x"]), want.astype(np.float64)
    lim = E.int_limits(want[:, K:])
    base = _full(head, x, v, N, (0, 0), lim, SAMPLE_LIMITS)
    good = head.whp.clone()
    half = head.stride // 2
    w = good.clone().reshape(-1, 2, head.stride)
    w[:, :, 0], w[:, :, half] = good.reshape(-1, 2, head.stride)[:, :, half], good.reshape(-1, 2, head.stride)[:, :, 0]
    head.whp = w.reshape(-1).contiguous()
    assert not torch.equal(head.whp, good)
    out = head.run(x, N, (0, 0), lim, None, True)
    rep = E.check_dist(out["dist"][:N].cpu().numpy(), v, K, 0, 0, *lim)
    assert not rep["ok"] and _tails_clean(out, N)
    if half > K:
        assert not bool(head.valid.all())
        head.whp = torch.where(head.valid, good, torch.full((), 5.0, device="cuda")).contiguous()
        assert not torch.equal(head.whp, good)
        again = _full(head, x, v, N, (0, 0), lim, SAMPLE_LIMITS)
        for a, b in zip(_four(again, slice(0, N + PAD)), _four(base, slice(0, N + PAD))):
            assert np.array_equal(a, b)
    else:
        assert bool(head.valid.all())
