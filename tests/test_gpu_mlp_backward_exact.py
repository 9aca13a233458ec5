"""GPU tests that pin msc_mlp_relu_backward (csrc/mlp_backward.hip) to an exact reference.

The integer method of tests/test_gpu_mlp_exact.py, carried to the gradients: integer x, weights, biases in
[-3, 3] and d_out in [-2, 2] whose absolute-value evaluation (every |.| propagated through the forward, the
dgrad and the wgrad sums) stays below 2^24 make every float32 product and partial sum exact in any order, so
all six gradients are compared with an int64 numpy evaluation on bits. Integer data makes z == 0 frequent
(hidden unit 0 of layer 1 is 0 on every row by construction), which pins the mask convention z > 0: each
case asserts that exact zeros occur. Outputs are pre-filled with NaN (accumulate = 0 ignores them) and
followed by guard words; the workspace is followed by guard words as well."""
import ctypes as C

import numpy as np
import pytest

torch = pytest.importorskip("torch")

from marlsc import abi  # noqa: E402
from marlsc import mlp as M  # noqa: E402

pytestmark = pytest.mark.gpu
SENTINEL = 7.25
PAD = 64  # guard floats behind every output and the workspace
IN_DIMS = (1, 7, 34)
ROWS = (1, 31, 32, 33, 129)
HIDDEN = [(32,), (96,), (256,), (64, 64), (64, 128), (128, 64), (256, 256)]
OUT_DIMS = [1, 5, 8, 9, 32]
LIMIT = 1 << 24


def _hid(h):
    return "x".join(map(str, h)) if isinstance(h, tuple) else str(h)


def _case(L, hidden, KO, n, seed=0):
    """Integer x [n, L], W / b per layer in [-3, 3], d_out [n, KO] in [-2, 2]; unit 0 of layer 1 has zero
    weights and bias (z == 0 on every row)."""
    rng = np.random.default_rng([seed, L, KO, n, *hidden])
    dims = (L, *hidden, KO)
    W = [rng.integers(-3, 4, size=(dims[i + 1], dims[i])).astype(np.int64) for i in range(len(dims) - 1)]
    b = [rng.integers(-3, 4, size=(dims[i + 1],)).astype(np.int64) for i in range(len(dims) - 1)]
    if len(hidden) == 2:
        # thin the second layer so that the wgrad sums over many rows keep their headroom
        W[1] *= rng.integers(0, 2, size=W[1].shape)
    W[0][0, :] = 0
    b[0][0] = 0
    x = rng.integers(-3, 4, size=(n, L)).astype(np.int64)
    d = rng.integers(-2, 3, size=(n, KO)).astype(np.int64)
    d[0, 0] = d[0, 0] or 2  # (a single row of one zero would make every gradient zero)
    return {"x": x, "W": W, "b": b, "d": d}


def _reference(case):
    """(gradients in parameter order, largest absolute-value partial sum, number of exact-zero pre-activations)."""
    x, W, b, d = case["x"], case["W"], case["b"], case["d"]
    hs, zs, ah = [x], [], [np.abs(x)]
    for w, bb in zip(W[:-1], b[:-1]):
        z = hs[-1] @ w.T + bb
        zs.append(z)
        hs.append(np.maximum(z, 0))
        ah.append(ah[-1] @ np.abs(w).T + np.abs(bb))
    grads, peak = [], max(int(a.max(initial=0)) for a in ah)
    delta, adelta = d, np.abs(d)
    for i in range(len(W) - 1, -1, -1):
        grads[:0] = [delta.T @ hs[i], delta.sum(axis=0)]
        peak = max(peak, int((adelta.T @ ah[i]).max(initial=0)), int(adelta.sum(axis=0).max(initial=0)))
        if i > 0:
            adelta = adelta @ np.abs(W[i])
            delta = (delta @ W[i]) * (zs[i - 1] > 0)
            peak = max(peak, int(adelta.max(initial=0)))
    zeros = sum(int((z == 0).sum()) for z in zs)
    return grads, peak, zeros


def _dev(a, dtype=np.float32):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=dtype)).cuda()


def _p(t):
    return None if t is None else C.c_void_p(t.data_ptr())


def _bits(t):
    return t.detach().cpu().numpy().view(np.uint32)


class _Net:
    """A case's packs on the device and msc_mlp_relu_backward through the C ABI, guard words everywhere."""

    def __init__(self, case):
        W = [_dev(w) for w in case["W"]]
        self.W, self.b = W, [_dev(v) for v in case["b"]]
        self.H1, self.L = W[0].shape
        self.H2 = W[1].shape[0] if len(W) == 3 else 0
        self.KO = W[-1].shape[0]
        self.w1p, self.w2p, self.w3p = M.pack_mlp3(W[0], W[1] if self.H2 else None, W[-1])
        self.w2tp = M.pack_w2t(W[1]) if self.H2 else None
        self.shapes = [s for w, v in zip(W, self.b) for s in (tuple(w.shape), tuple(v.shape))]

    def outputs(self, fill=float("nan")):
        outs = []
        for s in self.shapes:
            t = torch.full((int(np.prod(s)) + PAD,), SENTINEL, device="cuda")
            t[:int(np.prod(s))] = fill
            outs.append(t)
        return outs

    def run(self, x, d, n, outs, scale=1.0, accumulate=0):
        nbytes = M.backward_workspace_bytes(n, self.L, self.H1, self.H2, self.KO)
        assert nbytes >= 0 and nbytes % 4 == 0
        ws = torch.full((nbytes // 4 + PAD,), SENTINEL, device="cuda")
        g = outs if self.H2 else [outs[0], outs[1], None, None, outs[2], outs[3]]
        rc = abi.lib().msc_mlp_relu_backward(_p(x), n, self.L, self.H1, self.H2, self.KO, _p(self.w1p), _p(self.b[0]),
                                             _p(self.w2p), _p(self.b[1]) if self.H2 else None, _p(self.w2tp), _p(self.W[-1]),
                                             _p(d), C.c_float(scale), accumulate, *[_p(t) for t in g], _p(ws), None)
        abi.check(rc)
        torch.cuda.synchronize()
        assert bool((ws[nbytes // 4:] == SENTINEL).all()), "the kernels wrote past the workspace"
        for t, s in zip(outs, self.shapes):
            assert bool((t[int(np.prod(s)):] == SENTINEL).all()), "the kernels wrote past an output"
        return [t[:int(np.prod(s))].reshape(s) for t, s in zip(outs, self.shapes)]


def _check_case(L, hidden, KO, n, seed=0):
    case = _case(L, hidden, KO, n, seed)
    want, peak, zeros = _reference(case)
    assert peak < LIMIT, f"headroom: peak {peak}"
    assert zeros >= 1
    net = _Net(case)
    got = net.run(_dev(case["x"]), _dev(case["d"]), n, net.outputs())
    names = ("g_w1", "g_b1", "g_w2", "g_b2", "g_w3", "g_b3") if len(hidden) == 2 else ("g_w1", "g_b1", "g_w3", "g_b3")
    for name, g, w in zip(names, got, want):
        assert np.array_equal(_bits(g), w.astype(np.float32).view(np.uint32)), \
            f"{name} differs from the int64 evaluation (in {L}, hidden {hidden}, out {KO}, rows {n})"
    assert any(np.any(w != 0) for w in want)


@pytest.mark.parametrize("KO", OUT_DIMS)
@pytest.mark.parametrize("hidden", HIDDEN, ids=_hid)
def test_gradients_equal_the_int64_evaluation(hidden, KO):
    for L in IN_DIMS:
        for n in ROWS:
            _check_case(L, hidden, KO, n)


@pytest.mark.parametrize("hidden", [(512, 64), (64, 512), (512, 512)], ids=_hid)
def test_forms_with_a_512_wide_layer(hidden):
    """The register-heaviest forms (hidden1 = 512 holds 256 accumulators per lane) at a few rows."""
    for n in (5, 33):
        _check_case(7, hidden, 5, n)


def test_one_hidden_layer_with_w3_read_from_l2():
    """32 outputs over 1,024 hidden units: w3 is past what a block stages in LDS, the kernel reads it in place."""
    for n in (5, 33):
        _check_case(7, (1024,), 32, n)


def test_python_entry_point_adds_to_given_gradients():
    """mlp.mlp_backward(..., grads=...) is accumulate = 1: prior integers plus half the int64 gradients."""
    from marlsc.rollout import MLP
    case = _case(7, (64, 64), 5, 33)
    want, peak, _ = _reference(case)
    assert 2 * peak + 64 < LIMIT
    net = MLP(7, 5, {"hidden_sizes": [64, 64]})
    with torch.no_grad():
        for lin, w, b in zip(list(net)[0::2], case["W"], case["b"]):
            lin.weight.copy_(torch.from_numpy(w.astype(np.float32)))
            lin.bias.copy_(torch.from_numpy(b.astype(np.float32)))
    mods = list(net.cuda())
    x, d = _dev(case["x"]), _dev(case["d"])
    fresh = M.mlp_backward(mods, x, d)
    for g, w in zip(fresh, want):
        assert np.array_equal(_bits(g), w.astype(np.float32).view(np.uint32))
    rng = np.random.default_rng(7)
    prior = [rng.integers(-9, 10, size=w.shape).astype(np.float32) for w in want]
    grads = tuple(_dev(p) for p in prior)
    out = M.mlp_backward(mods, x, d, scale=0.5, grads=grads)
    assert all(o is g for o, g in zip(out, grads))
    torch.cuda.synchronize()
    for g, w, p in zip(grads, want, prior):
        assert np.array_equal(_bits(g), (p + 0.5 * w.astype(np.float64)).astype(np.float32).view(np.uint32))
    with pytest.raises(ValueError, match="grads must be contiguous float32 CUDA tensors"):
        M.mlp_backward(mods, x, d, grads=grads[:-1])


def _tile_step(L, hidden, KO):
    """The workspace's growth per row tile while nothing else changes, read off the library's query."""
    H1, H2 = hidden[0], hidden[1] if len(hidden) == 2 else 0
    return M.backward_workspace_bytes(64, L, H1, H2, KO) - M.backward_workspace_bytes(32, L, H1, H2, KO)


def slice_boundary_rows(L, hidden, KO):
    """The largest row count before the per-tile growth of the workspace first changes: up to there every
    further row tile has added (or has not added) a split-K slice of partials, and from the next row on it
    no longer does the same -- the slice count has reached its maximum and slices begin to hold two tiles."""
    H1, H2 = hidden[0], hidden[1] if len(hidden) == 2 else 0
    step, t = _tile_step(L, hidden, KO), 1
    while M.backward_workspace_bytes(32 * (t + 1), L, H1, H2, KO) - M.backward_workspace_bytes(32 * t, L, H1, H2, KO) == step:
        t += 1
        assert t < 4096
    return 32 * t


def round_rows(L, hidden, KO):
    """The smallest row count from which the workspace no longer grows: the rows of one round."""
    H1, H2 = hidden[0], hidden[1] if len(hidden) == 2 else 0
    top = M.backward_workspace_bytes(1 << 22, L, H1, H2, KO)
    lo, hi = 1, 1 << 22
    while lo < hi:
        mid = (lo + hi) // 2
        if M.backward_workspace_bytes(mid, L, H1, H2, KO) == top:
            hi = mid
        else:
            lo = mid + 1
    return (lo + 31) // 32 * 32  # (rows are processed in tiles of 32: the last tile's rows cost the same)


# (the widths keep the 2^24 headroom over a whole round of rows: the two-hidden-layer sums grow with every width)
@pytest.mark.parametrize("hidden,L,KO", [((32,), 7, 5), ((64, 64), 1, 1)], ids=["32", "64x64"])
def test_just_past_the_slice_and_round_boundaries(hidden, L, KO):
    s, r = slice_boundary_rows(L, hidden, KO), round_rows(L, hidden, KO)
    assert 32 <= s < r < (1 << 20)
    _check_case(L, hidden, KO, s + 1)
    _check_case(L, hidden, KO, r + 1)  # a second round of one row, accumulated onto the first


@pytest.mark.parametrize("hidden", [(96,), (128, 64)], ids=_hid)
def test_scale_and_accumulate(hidden):
    L, KO, n = 7, 5, 33
    case = _case(L, hidden, KO, n)
    want, peak, _ = _reference(case)
    assert 2 * peak + 64 < LIMIT
    net = _Net(case)
    x, d = _dev(case["x"]), _dev(case["d"])
    outs = net.outputs()
    rng = np.random.default_rng(5)
    prior = [rng.integers(-9, 10, size=s).astype(np.float32) for s in net.shapes]
    for t, p in zip(outs, prior):
        t[:p.size] = _dev(p.reshape(-1))
    got = net.run(x, d, n, outs, scale=0.5, accumulate=1)
    for g, w, p in zip(got, want, prior):  # halves of integers below 2^24 and their sums with integers: exact
        assert np.array_equal(_bits(g), (p + 0.5 * w.astype(np.float64)).astype(np.float32).view(np.uint32))
    got = net.run(x, d, n, outs, scale=2.0, accumulate=0)  # the previous results are ignored
    for g, w in zip(got, want):
        assert np.array_equal(_bits(g), (2 * w).astype(np.float32).view(np.uint32))


@pytest.mark.parametrize("hidden", [(256,), (64, 128)], ids=_hid)
def test_two_calls_on_real_data_give_the_same_bits(hidden):
    L, KO, n = 34, 5, 700
    g = torch.Generator().manual_seed(3)
    dims = (L, *hidden, KO)
    case = {"W": [torch.randn(dims[i + 1], dims[i], generator=g).numpy() / np.sqrt(dims[i]) for i in range(len(dims) - 1)],
            "b": [0.1 * torch.randn(dims[i + 1], generator=g).numpy() for i in range(len(dims) - 1)]}
    net = _Net(case)
    x, d = torch.randn(n, L, generator=g).cuda(), torch.randn(n, KO, generator=g).cuda()
    a = [t.clone() for t in net.run(x, d, n, net.outputs())]
    b = net.run(x, d, n, net.outputs(0.0))
    for u, v in zip(a, b):
        assert bool(torch.isfinite(u).all()) and float(u.abs().max()) > 0
        assert np.array_equal(_bits(u), _bits(v))


def test_no_rows():
    case = _case(7, (64, 64), 5, 1)
    net = _Net(case)
    outs = net.outputs()
    x, d = torch.full((1,), float("nan"), device="cuda"), torch.full((1,), float("nan"), device="cuda")  # not read
    for g in net.run(x, d, 0, outs, accumulate=0):
        assert bool((g == 0).all())
    outs = net.outputs(3.0)
    for g in net.run(x, d, 0, outs, accumulate=1):
        assert bool((g == 3.0).all())


@pytest.mark.parametrize("two", [False, True], ids=["one_hidden", "two_hidden"])
def test_masks_are_the_forward_kernels(two):
    """Unit u of layer 1 has pre-activation x (in_dim 1, weight 1, bias 0) with x in {-1, 0, 1}: with every
    later weight 1 on its path and d_out = 1, g_b1[u] counts the rows whose mask is set. The forward kernel
    on the same packs gives relu(x) per row; the two counts agree and equal the number of rows with x = 1."""
    n, u, H = 97, 5, 64
    rng = np.random.default_rng(11)
    x = rng.integers(-1, 2, size=(n, 1)).astype(np.int64)
    assert {-1, 0, 1} <= set(x.ravel().tolist())
    W1, b1 = np.zeros((H, 1), np.int64), np.zeros(H, np.int64)
    W1[u, 0] = 1
    if two:  # unit u of layer 2 copies unit u of layer 1 (bias 1 elsewhere keeps the other units' masks set, weights 0)
        W2, b2 = np.zeros((H, H), np.int64), np.ones(H, np.int64)
        W2[u, u], b2[u] = 1, 0
        W3 = np.zeros((1, H), np.int64)
        W3[0, u] = 1
        case = {"x": x, "W": [W1, W2, W3], "b": [b1, b2, np.zeros(1, np.int64)], "d": np.ones((n, 1), np.int64)}
    else:
        W3 = np.zeros((1, H), np.int64)
        W3[0, u] = 1
        case = {"x": x, "W": [W1, W3], "b": [b1, np.zeros(1, np.int64)], "d": np.ones((n, 1), np.int64)}
    net = _Net(case)
    xd = _dev(x)
    got = net.run(xd, _dev(case["d"]), n, net.outputs())
    out = torch.empty(n, 1, device="cuda")
    lib = abi.lib()
    if two:
        abi.check(lib.msc_mlp3_relu_forward(_p(xd), n, 1, H, H, 1, _p(net.w1p), _p(net.b[0]), _p(net.w2p), _p(net.b[1]),
                                            _p(net.w3p), _p(net.b[2]), _p(out), None, 1, None))
    else:
        abi.check(lib.msc_mlp2_relu_forward(_p(xd), n, 1, H, 1, _p(net.w1p), _p(net.b[0]), _p(net.w3p), _p(net.b[1]),
                                            _p(out), None, 1, None))
    torch.cuda.synchronize()
    positive = int((x > 0).sum())
    assert int((out > 0).sum()) == positive  # the forward's relu(x) per row
    g_b1 = got[1].cpu().numpy()
    assert g_b1[u] == positive  # zero gradient at z == 0, none at z < 0
    assert np.count_nonzero(g_b1) == 1
    if two:
        g_b2 = got[3].cpu().numpy()
        assert g_b2[u] == positive and np.count_nonzero(g_b2) == 1
