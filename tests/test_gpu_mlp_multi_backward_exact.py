"""GPU tests that pin msc_mlp_relu_backward_multi (csrc/mlp_backward.hip's multi kernels) to its contract: for
every policy, bit for bit what msc_mlp_relu_backward returns for the policy's rows gathered contiguously.

Two references, both exact: the int64 evaluation of tests/test_gpu_mlp_backward_exact.py on integer data (its
cases, one per policy with its own seed, so weights and data differ between the policies), and the single-policy
call itself on real data. Rows lie [rows per policy][P] and are never gathered for the multi call. Every stacked
output, and the workspace, is followed by guard words; outputs are pre-filled with NaN where accumulate = 0."""
import ctypes as C

import numpy as np
import pytest

torch = pytest.importorskip("torch")

from marlsc import abi  # noqa: E402
from marlsc import mlp as M  # noqa: E402
from test_gpu_mlp_backward_exact import (LIMIT, PAD, SENTINEL, _Net, _bits, _case, _dev, _hid, _p, _reference,  # noqa: E402
                                         round_rows, slice_boundary_rows)

pytestmark = pytest.mark.gpu


class _Multi:
    """P same-shaped single-policy nets (_Net) stacked as msc_mlp_relu_backward_multi takes them."""

    def __init__(self, nets):
        self.nets, self.P = nets, len(nets)
        n0 = nets[0]
        self.L, self.H1, self.H2, self.KO, self.shapes = n0.L, n0.H1, n0.H2, n0.KO, n0.shapes
        cat = lambda ts: torch.stack([t.reshape(-1) for t in ts]).contiguous()  # noqa: E731
        self.w1p = cat([n.w1p for n in nets])
        self.b1 = cat([n.b[0] for n in nets])
        self.w3 = cat([n.W[-1] for n in nets])
        self.w2p = cat([n.w2p for n in nets]) if self.H2 else None
        self.b2 = cat([n.b[1] for n in nets]) if self.H2 else None
        self.w2tp = cat([n.w2tp for n in nets]) if self.H2 else None

    def outputs(self, fill=float("nan")):
        outs = []
        for s in self.shapes:
            k = self.P * int(np.prod(s))
            t = torch.full((k + PAD,), SENTINEL, device="cuda")
            t[:k] = fill
            outs.append(t)
        return outs

    def run(self, x, d, rows, outs, scale=1.0, accumulate=0):
        """x [rows, P, L], d [rows, P, KO] -> per policy the list of gradients (views of the stacked outputs)."""
        n = rows * self.P
        nbytes = M.multi_backward_workspace_bytes(n, self.P, self.L, self.H1, self.H2, self.KO)
        assert nbytes >= 0 and nbytes % 4 == 0
        ws = torch.full((nbytes // 4 + PAD,), SENTINEL, device="cuda")
        g = outs if self.H2 else [outs[0], outs[1], None, None, outs[2], outs[3]]
        rc = abi.lib().msc_mlp_relu_backward_multi(_p(x), n, self.P, self.L, self.H1, self.H2, self.KO, _p(self.w1p),
                                                   _p(self.b1), _p(self.w2p), _p(self.b2), _p(self.w2tp), _p(self.w3), _p(d),
                                                   C.c_float(scale), accumulate, *[_p(t) for t in g], _p(ws), None)
        abi.check(rc)
        torch.cuda.synchronize()
        assert bool((ws[nbytes // 4:] == SENTINEL).all()), "the kernels wrote past the workspace"
        for t, s in zip(outs, self.shapes):
            assert bool((t[self.P * int(np.prod(s)):] == SENTINEL).all()), "the kernels wrote past a stacked output"
        stacked = [t[:self.P * int(np.prod(s))].reshape((self.P,) + s) for t, s in zip(outs, self.shapes)]
        return [[t[p] for t in stacked] for p in range(self.P)]


def _interleave(arrays):
    """P arrays [rows, C] -> [rows, P, C] on the device: row r of policy p lies at row r P + p."""
    return _dev(np.stack(arrays, axis=1))


_REF = {}


def _int_cases(L, hidden, KO, rows, P):
    """P integer cases of one shape (seed = policy index) with their int64 gradients, computed once per shape."""
    key = (L, hidden, KO, rows, P)
    if key not in _REF:
        cases = [_case(L, hidden, KO, rows, seed=p) for p in range(P)]
        refs = [_reference(c) for c in cases]
        assert all(peak < LIMIT for _, peak, _ in refs), "headroom"
        assert all(zeros >= 1 for _, _, zeros in refs)
        _REF[key] = (cases, [g for g, _, _ in refs])
    return _REF[key]


def _check_int(L, hidden, KO, rows, P):
    cases, want = _int_cases(L, hidden, KO, rows, P)
    if P > 1:
        assert any(not np.array_equal(a, b) for a, b in zip(want[0], want[1]))  # the policies differ
    multi = _Multi([_Net(c) for c in cases])
    got = multi.run(_interleave([c["x"] for c in cases]), _interleave([c["d"] for c in cases]), rows, multi.outputs())
    for p in range(P):
        for i, (g, w) in enumerate(zip(got[p], want[p])):
            assert np.array_equal(_bits(g), w.astype(np.float32).view(np.uint32)), \
                f"policy {p} of {P}, gradient {i} differs from the int64 evaluation (in {L}, hidden {hidden}, out {KO}, rows {rows})"


# every listed value of P, rows per policy, hidden form, in_dim and out_dim at least once, each with P = 3
INT_CASES = [  # (P, rows per policy, hidden, in_dim, out_dim)
    (3, 1, (32,), 1, 1),
    (3, 31, (96,), 7, 5),
    (3, 33, (64, 64), 34, 9),
    (3, 129, (128, 64), 7, 32),
    (3, 33, (256, 256), 34, 5),
    (1, 33, (96,), 7, 5),
    (2, 129, (64, 64), 1, 9),
    (8, 31, (32,), 34, 32),
    (8, 33, (128, 64), 7, 1),
]


def test_the_integer_cases_cover_every_listed_value_with_three_policies():
    for i, values in enumerate([(1, 2, 3, 8), (1, 31, 33, 129), [(32,), (96,), (64, 64), (128, 64), (256, 256)], (1, 7, 34),
                                (1, 5, 9, 32)]):
        assert {c[i] for c in INT_CASES} == set(values)
        if i > 0:
            assert {c[i] for c in INT_CASES if c[0] == 3} == set(values)


@pytest.mark.parametrize("P,rows,hidden,L,KO", INT_CASES, ids=lambda v: _hid(v))
def test_gradients_equal_the_int64_evaluation_per_policy(P, rows, hidden, L, KO):
    _check_int(L, hidden, KO, rows, P)


@pytest.mark.parametrize("accumulate", [0, 1])
@pytest.mark.parametrize("hidden", [(256,), (64, 128)], ids=_hid)
def test_real_data_gives_the_single_policy_calls_bits(hidden, accumulate):
    L, KO, rows, P, scale = 34, 5, 33, 3, 0.5
    g = torch.Generator().manual_seed(3)
    dims = (L, *hidden, KO)
    nets = [_Net({"W": [torch.randn(dims[i + 1], dims[i], generator=g).numpy() / np.sqrt(dims[i]) for i in range(len(dims) - 1)],
                  "b": [0.1 * torch.randn(dims[i + 1], generator=g).numpy() for i in range(len(dims) - 1)]}) for _ in range(P)]
    multi = _Multi(nets)
    x, d = torch.randn(rows, P, L, generator=g).cuda(), torch.randn(rows, P, KO, generator=g).cuda()
    prior = [[torch.randn(s, generator=g).cuda() for s in multi.shapes] for _ in range(P)]
    outs = multi.outputs()
    if accumulate:
        for i, s in enumerate(multi.shapes):
            outs[i][:P * int(np.prod(s))] = torch.stack([prior[p][i] for p in range(P)]).reshape(-1)
    got = multi.run(x, d, rows, outs, scale=scale, accumulate=accumulate)
    for p, net in enumerate(nets):
        single = net.outputs()
        if accumulate:
            for t, pr in zip(single, prior[p]):
                t[:pr.numel()] = pr.reshape(-1)
        want = net.run(x[:, p].contiguous(), d[:, p].contiguous(), rows, single, scale=scale, accumulate=accumulate)
        for i, (a, b) in enumerate(zip(got[p], want)):
            assert bool(torch.isfinite(b).all()) and float(b.abs().max()) > 0
            assert np.array_equal(_bits(a), _bits(b)), f"policy {p}, gradient {i} (accumulate = {accumulate})"


def test_just_past_the_slice_and_round_boundaries():
    """Rows per policy one past the last row count at which every slice holds one tile, and one past a full
    round (a second round of one row per policy, accumulated onto the first); both read off the plan and the
    single-policy geometry."""
    L, hidden, KO, P = 1, (32,), 1, 2
    s, r = slice_boundary_rows(L, hidden, KO), round_rows(L, hidden, KO)
    assert 32 <= s < r < (1 << 20)
    at, past = (M.multi_backward_plan(n * P, P, L, 32, 0, KO) for n in (s, s + 1))
    assert at["slices"] == past["slices"] == at["round_tiles"] == past["round_tiles"] - 1  # slices begin to hold two tiles
    full, over = (M.multi_backward_plan(n * P, P, L, 32, 0, KO) for n in (r, r + 1))
    assert (full["rounds"], over["rounds"]) == (1, 2) and full["round_tiles"] == over["round_tiles"] == r // 32
    assert over["groups"] == 1
    _check_int(L, hidden, KO, s + 1, P)
    _check_int(L, hidden, KO, r + 1, P)


def test_two_groups_with_a_smaller_last_group():
    """More policies than one set of launches takes: G from the plan, P = G + max(1, G // 2) policies, so the last
    group is smaller than G. Bit-equal per policy to the single-policy call (real data)."""
    L, hidden, KO, rows = 7, (256, 256), 5, 33
    G = M.multi_backward_plan(64 * rows, 64, L, *hidden, KO)["group_policies"]
    assert 2 <= G < 42
    P = G + G // 2
    plan = M.multi_backward_plan(P * rows, P, L, *hidden, KO)
    assert plan["group_policies"] == G and plan["groups"] == 2 and 0 < P - G < G
    g = torch.Generator().manual_seed(5)
    dims = (L, *hidden, KO)
    nets = [_Net({"W": [torch.randn(dims[i + 1], dims[i], generator=g).numpy() / np.sqrt(dims[i]) for i in range(len(dims) - 1)],
                  "b": [0.1 * torch.randn(dims[i + 1], generator=g).numpy() for i in range(len(dims) - 1)]}) for _ in range(P)]
    multi = _Multi(nets)
    x, d = torch.randn(rows, P, L, generator=g).cuda(), torch.randn(rows, P, KO, generator=g).cuda()
    got = multi.run(x, d, rows, multi.outputs())
    for p, net in enumerate(nets):
        want = net.run(x[:, p].contiguous(), d[:, p].contiguous(), rows, net.outputs())
        for i, (a, b) in enumerate(zip(got[p], want)):
            assert float(b.abs().max()) > 0 and np.array_equal(_bits(a), _bits(b)), f"policy {p} of {P}, gradient {i}"


def test_no_rows():
    cases, _ = _int_cases(7, (64, 64), 5, 1, 3)
    multi = _Multi([_Net(c) for c in cases])
    x, d = torch.full((1,), float("nan"), device="cuda"), torch.full((1,), float("nan"), device="cuda")  # not read
    for per_policy in multi.run(x, d, 0, multi.outputs(), accumulate=0):
        assert all(bool((g == 0).all()) for g in per_policy)
    for per_policy in multi.run(x, d, 0, multi.outputs(3.0), accumulate=1):
        assert all(bool((g == 3.0).all()) for g in per_policy)


@pytest.mark.parametrize("two", [False, True], ids=["one_hidden", "two_hidden"])
def test_masks_are_the_multi_forward_kernels_per_policy(two):
    """As test_masks_are_the_forward_kernels, over three policies that share the weights (unit u of layer 1 has
    pre-activation x, every later weight on its path is 1, d_out = 1) but see different x in {-1, 0, 1}: policy 1's
    rows are all 0 or -1 -- pre-activations exactly 0 and below -- so its g_b1[u] is 0 while the others count
    their own rows with x = 1, as the multi forward kernel's relu(x) does on the same packs."""
    n, u, H, P = 97, 5, 64, 3
    rng = np.random.default_rng(11)
    xs = [rng.integers(-1, 2, size=(n, 1)).astype(np.int64) for _ in range(P)]
    xs[1] = -np.abs(xs[1])
    assert all({0, -1} <= set(x.ravel().tolist()) for x in xs) and 1 not in xs[1]
    W1, b1 = np.zeros((H, 1), np.int64), np.zeros(H, np.int64)
    W1[u, 0] = 1
    W3 = np.zeros((1, H), np.int64)
    W3[0, u] = 1
    if two:
        W2, b2 = np.zeros((H, H), np.int64), np.ones(H, np.int64)
        W2[u, u], b2[u] = 1, 0
        Ws, bs = [W1, W2, W3], [b1, b2, np.zeros(1, np.int64)]
    else:
        Ws, bs = [W1, W3], [b1, np.zeros(1, np.int64)]
    nets = [_Net({"W": Ws, "b": bs}) for _ in range(P)]
    multi = _Multi(nets)
    xd = _interleave(xs)
    got = multi.run(xd, torch.ones(n, P, 1, device="cuda"), n, multi.outputs())
    out = torch.empty(n, P, 1, device="cuda")
    w3p, b3 = torch.stack([m.w3p for m in nets]).contiguous(), torch.stack([m.b[-1] for m in nets]).contiguous()
    if two:
        abi.check(abi.lib().msc_mlp3_relu_multi(_p(xd), n * P, P, 1, H, H, 1, _p(multi.w1p), _p(multi.b1), _p(multi.w2p),
                                                _p(multi.b2), _p(w3p), _p(b3), _p(out), None, None, None))
    else:
        abi.check(abi.lib().msc_mlp2_relu_multi(_p(xd), n * P, P, 1, H, 1, _p(multi.w1p), _p(multi.b1), _p(w3p), _p(b3),
                                                _p(out), None, None, None))
    torch.cuda.synchronize()
    for p in range(P):
        positive = int((xs[p] > 0).sum())
        assert (positive == 0) == (p == 1)
        assert int((out[:, p] > 0).sum()) == positive  # the multi forward's relu(x) per row of this policy
        g_b1 = got[p][1].cpu().numpy()
        assert g_b1[u] == positive and np.count_nonzero(g_b1) == (1 if positive else 0)
        if two:
            g_b2 = got[p][3].cpu().numpy()
            assert g_b2[u] == positive and np.count_nonzero(g_b2) == (1 if positive else 0)
