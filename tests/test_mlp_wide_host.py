"""Host tests of the wide-output fused MLP's packing (marlsc/mlp.py:pack_wide, csrc/mlp_wide.hpp): the
lane-by-lane emulation of tests/mlp_emulation.py, run once per 32-row output tile over the tile's slice
of the packed w3 (the layout-0 fragment order, slices concatenated), equals the int64 reference of
oracle/mlp_ref.py exactly; mutants of the packing change an output; the predicates that route a
network to the wide kernel leave every narrower network where it was."""
import numpy as np
import pytest
import torch
import torch.nn as nn

from marlsc import mlp as M
from mlp_emulation import emulate_packed, live_units
from mlp_ref import RECIPES, case_forward, int_case

# (L, hidden, KO): a subset of the shapes whose int_case conditions were checked for A / Bx / Bw at n = 161
SHAPES = [(1, (32,), 33), (7, (96,), 65), (33, (64, 64), 33), (9, (128, 64), 96), (34, (256, 256), 64),
          (272, (256,), 40), (17, (512, 512), 128)]


def _dims(case):
    W = case["W"]
    return W[0].shape[1], W[0].shape[0], (W[1].shape[0] if len(W) == 3 else 0), W[-1].shape[0]


def _pack(case):
    W = [torch.from_numpy(w) for w in case["W"]]
    return [None if t is None else t.numpy() for t in M.pack_wide(W[0], W[1] if len(W) == 3 else None, W[-1])]


def emulate_wide(case, packed=None):
    """[32, KO] of rows 0..31: emulate_packed(layout=0) per output tile on that tile's w3 slice and bias rows."""
    L, H1, H2, KO = _dims(case)
    w1p, w2p, w3p = packed if packed is not None else _pack(case)
    HL = H2 or H1
    nto = (KO + 31) // 32
    w3t = np.asarray(w3p).reshape(nto, HL // 8 * 64 * 4)
    b = case["b"]
    pre1_rows = None if case["pre1"] is None else case["pre1"][np.arange(32) // case["group"]]
    cols = []
    for o in range(nto):
        ko = min(32, KO - 32 * o)
        cols.append(emulate_packed(case["x"], L, H1, H2, ko, w1p, w2p, w3t[o], b[0], b[1] if H2 else None,
                                   b[-1][32 * o:32 * o + ko], 0, pre1_rows=pre1_rows))
    return np.concatenate(cols, axis=1)


# the two largest forms run recipe A only here (emulation time)
CASES = [(s, r) for s in SHAPES for r in RECIPES if r == "A" or s[1] not in ((512, 512), (256, 256))]


@pytest.mark.parametrize("shape,recipe", CASES, ids=lambda v: "x".join(map(str, v)).replace(" ", "") if isinstance(v, tuple) else v)
def test_wide_emulation_equals_int64(shape, recipe):
    L, hidden, KO = shape
    case = int_case(L, hidden, KO, recipe, 32, pre1_group=3 if L == 7 else 0)
    want = case_forward(case)
    got = emulate_wide(case)
    assert got.shape == want.shape and np.array_equal(got, want.astype(np.float64))


def test_packed_w3_shape_and_zero_rows():
    for H, KO in ((32, 33), (96, 65), (256, 40), (256, 128)):
        w3 = torch.arange(1, KO * H + 1, dtype=torch.float32).reshape(KO, H)
        w1 = torch.ones(H, 3)
        _, w2p, w3p = M.pack_wide(w1, None, w3)
        nto = (KO + 31) // 32
        assert w2p is None and w3p.numel() == nto * (H // 8) * 64 * 4
        v = w3p.reshape(nto, H // 8, 64, 4)
        lane_row = (torch.arange(64) & 31)[None, None, :, None] + 32 * torch.arange(nto)[:, None, None, None]
        assert bool((v[(lane_row >= KO).expand_as(v)] == 0).all())
        # every weight sits in exactly one slot
        assert sorted(v[(lane_row < KO).expand_as(v)].tolist()) == list(range(1, KO * H + 1))
    with pytest.raises(ValueError):
        M.pack_wide(torch.ones(32, 3), None, torch.ones(129, 32))


@pytest.mark.parametrize("recipe", RECIPES)
def test_wide_mutants_change_an_output(recipe):
    # two-hidden-layer form, 33 outputs: output 32 is the only row of the second tile
    case = int_case(33, (64, 64), 33, recipe, 32)
    want = case_forward(case).astype(np.float64)
    assert np.array_equal(emulate_wide(case), want)
    L, H1, H2, KO = _dims(case)
    w1p, w2p, w3p = _pack(case)
    idx, valid = (t.numpy() for t in M._wide_index(H2, KO, torch.device("cpu")))
    (_, live2), _ = live_units(case)
    W3 = case["W"][-1]
    # (1) two packed w3 entries of different output tiles exchanged: the weights of one live hidden unit
    # to an output of tile 0 and to output 32 (tile 1), different and not both zero
    u = next(int(h) for h in np.flatnonzero(live2) if any(W3[a, h] != W3[32, h] for a in range(32)))
    a = next(a for a in range(32) if W3[a, u] != W3[32, u])
    pos = []
    for row in (a, 32):
        hit = np.flatnonzero((idx == row * H2 + u) & valid)
        assert hit.size == 1
        pos.append(int(hit[0]))
    assert pos[0] // (H2 // 8 * 256) == 0 and pos[1] // (H2 // 8 * 256) == 1  # different tiles
    sw = w3p.copy().reshape(-1)
    sw[pos[0]], sw[pos[1]] = sw[pos[1]], sw[pos[0]]
    got = emulate_wide(case, (w1p, w2p, sw))
    moved = got != want
    print(f"mutant [w3p: entries of two output tiles swapped] recipe {recipe}: {int(moved.sum())} of {want.size} differ")
    assert moved[:, a].any() and moved[:, 32].any()
    # (2) the row guard zeroing one row too many at out_dim 33 (rows < 32 kept): output 32 loses its weights
    cut = np.where((idx // H2 < 32) & valid, W3.reshape(-1)[idx], np.float32(0))
    assert not np.array_equal(cut, w3p.reshape(-1))
    got = emulate_wide(case, (w1p, w2p, cut))
    print(f"mutant [row guard at 32 instead of 33] recipe {recipe}: {int((got != want).sum())} of {want.size} differ")
    assert (got[:, 32] != want[:, 32]).any() and np.array_equal(got[:, :32], want[:, :32])


def _mlp(L, hidden, KO, act=nn.ReLU, bias=True):
    mods, d = [], L
    for h in hidden:
        mods += [nn.Linear(d, h, bias=bias), act()]
        d = h
    return mods + [nn.Linear(d, KO, bias=bias)]


def test_wide_layers_predicate_table():
    assert M.wide_layers(_mlp(20, (256,), 32)) == 0
    assert M.wide_layers(_mlp(20, (256,), 33)) == 2
    assert M.wide_layers(_mlp(20, (256,), 128)) == 2
    assert M.wide_layers(_mlp(20, (256,), 129)) == 0
    assert M.wide_layers(_mlp(20, (256, 64), 33)) == 3
    assert M.wide_layers(_mlp(20, (256, 64), 128)) == 3
    assert M.wide_layers(_mlp(20, (256,), 40, act=nn.Tanh)) == 0
    assert M.wide_layers(_mlp(20, (256,), 40, bias=False)) == 0
    assert M.wide_layers(_mlp(20, (100,), 40)) == 0          # hidden not a multiple of 32
    assert M.wide_layers(_mlp(20, (256, 96), 40)) == 0       # second hidden size not in {64, 128, 256, 512}
    assert M.wide_layers(_mlp(1025, (256,), 40)) == 0
    assert M.wide_layers(_mlp(20, (256, 256, 256), 40)) == 0
    assert M.wide_layers([]) == 0


def test_narrow_predicates_unchanged():
    """fused_layers / fusable for 1..33 outputs are what they were: the wide kernel adds no narrow path."""
    assert M.MAX_OUT == 32
    for KO in range(1, 34):
        want2, want3 = (2, 3) if KO <= 32 else (0, 0)
        assert M.fused_layers(_mlp(20, (256,), KO)) == want2
        assert M.fused_layers(_mlp(20, (256, 64), KO)) == want3
        assert M.fusable(_mlp(20, (256,), KO)) == (KO <= 32)
        assert (M.wide_layers(_mlp(20, (256,), KO)) > 0) == (KO > 32)
    for KO in range(1, 33):
        assert M.w3_layout(KO) == (1 if KO <= 8 else 0)
    with pytest.raises(ValueError):
        M.w3_layout(33)
    lib = M.abi.lib()
    assert lib.msc_mlp3_w3_layout(33) == -1
    assert lib.msc_mlp_wide_supported(256, 0, 40) == 1 and lib.msc_mlp_wide_supported(256, 256, 128) == 1
    assert lib.msc_mlp_wide_supported(256, 0, 129) == 0 and lib.msc_mlp_wide_supported(256, 96, 40) == 0
    assert lib.msc_mlp_wide_supported(100, 0, 40) == 0 and lib.msc_mlp_wide_supported(256, 0, 0) == 0
