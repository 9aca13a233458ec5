"""Host tests of the integer method that pins the fused policy MLP (oracle/mlp_ref.py): the lane-by-lane
emulation of the kernels over pack_mlp3's fragments (tests/mlp_emulation.py) equals the int64
evaluation exactly; every mutant of the packing or of the kernel's guards changes an output under
both recipes (pytest -s names each and how many outputs it moved); a float32 summation in a random
order still equals int64 under the headroom condition, and stops doing so once the headroom is gone."""
import numpy as np
import pytest
import torch

from marlsc import mlp as M
from mlp_emulation import emulate_packed, live_units, swap_packed
from mlp_ref import (LIMIT, RECIPES, case_forward, f32_chain_forward, f32_matmul_forward, int_case, int_forward,
                     shuffled_f32_sum_forward)

FORMS = [(64, 64), (128, 64), (64, 128), (96,)]  # three two-hidden-layer forms and the one-layer kernel
WIDTHS = [1, 2, 7, 9, 34, 1023]


def _dims(case):
    W = case["W"]
    return W[0].shape[1], W[0].shape[0], (W[1].shape[0] if len(W) == 3 else 0), W[-1].shape[0]


def _pack(case, layout):
    W = [torch.from_numpy(w) for w in case["W"]]
    return [None if t is None else t.numpy() for t in M.pack_mlp3(W[0], W[1] if len(W) == 3 else None, W[-1], layout)]


def _run(case, layout, packed=None, biases=None, pre1_rows=None, guard_x=True, x=None):
    L, H1, H2, KO = _dims(case)
    w1p, w2p, w3p = packed if packed is not None else _pack(case, layout)
    b = biases if biases is not None else case["b"]
    if pre1_rows is None and case["pre1"] is not None:
        pre1_rows = case["pre1"][np.arange(32) // case["group"]]
    return emulate_packed(case["x"] if x is None else x, L, H1, H2, KO, w1p, w2p, w3p, b[0], b[1] if H2 else None,
                          b[-1], layout, pre1_rows=pre1_rows, guard_x=guard_x)


@pytest.mark.parametrize("layout", [0, 1])
@pytest.mark.parametrize("recipe", RECIPES)
@pytest.mark.parametrize("hidden", FORMS, ids=lambda h: "x".join(map(str, h)))
@pytest.mark.parametrize("L", WIDTHS)
def test_emulation_equals_int64(L, hidden, recipe, layout):
    for KO in (5, 8):
        case = int_case(L, hidden, KO, recipe, 32, pre1_group=3 if L == 7 else 0)
        want = case_forward(case)
        got = _run(case, layout)
        assert np.array_equal(got, want.astype(np.float64))


# ---- mutants ------------------------------------------------------------------------------------------

def _mutants(case, layout):
    """name -> emulation outputs of each mutant (two-hidden-layer form, KO = 8, odd L, pre1 in groups of 3)."""
    L, H1, H2, KO = _dims(case)
    maps = M._index_maps(L, H1, H2, KO, torch.device("cpu"), layout)
    i1, v1, i2, i3, v3 = (None if t is None else t.numpy() for t in maps)
    w1p, w2p, w3p = _pack(case, layout)
    W1, W2, W3 = case["W"]
    (live1, live2), (act1, act2) = live_units(case)
    u1, u2 = int(np.flatnonzero(live1)[0]), int(np.flatnonzero(live2)[0])
    a3 = int(np.flatnonzero((W3[:, live2] != 0).sum(axis=1) >= 2)[0])
    out = {}
    out["w1p: two entries swapped"] = _run(case, layout, (swap_packed(w1p, i1, v1, W1, u1, np.ones(L, bool)), w2p, w3p))
    out["w2p: two entries swapped"] = _run(case, layout, (w1p, swap_packed(w2p, i2, np.ones_like(i2, bool), W2, u2, act1), w3p))
    out["w3p: two entries swapped"] = _run(case, layout, (w1p, w2p, swap_packed(w3p, i3, v3, W3, a3, live2)))
    for name, idx, units in (("b1", 0, live1), ("b2", 1, live2), ("b3", 2, np.ones(KO, bool))):
        b = [v.copy() for v in case["b"]]
        i = next(i for i in range(len(b[idx]) - 1) if b[idx][i] != b[idx][i + 1] and units[i] and units[i + 1])
        b[idx][i], b[idx][i + 1] = b[idx][i + 1], b[idx][i]
        out[f"{name}: one entry moved by one position"] = _run(case, layout, biases=b)
    g = case["group"]
    out["pre1 indexed with n // (group + 1)"] = _run(case, layout, pre1_rows=case["pre1"][np.arange(32) // (g + 1)])
    return out


@pytest.mark.parametrize("layout", [0, 1])
@pytest.mark.parametrize("recipe", RECIPES)
def test_every_mutant_changes_an_output(recipe, layout):
    case = int_case(7, (128, 64), 8, recipe, 32, pre1_group=3)
    want = case_forward(case).astype(np.float64)
    assert np.array_equal(_run(case, layout), want)
    for name, got in _mutants(case, layout).items():
        moved = int((got != want).sum())
        print(f"mutant [{name}] recipe {recipe} layout {layout}: {moved} of {want.size} outputs differ")
        assert moved > 0, name


@pytest.mark.parametrize("recipe", RECIPES)
def test_output_layer_packed_for_one_more_output_is_caught(recipe):
    # w3p packed for KO + 1 outputs (the matrix plus one more row). At KO = 8 that is the other layout
    # (MFMA fragments [H2/8][64][4] instead of VALU rows [H2/2][2][8]: a larger buffer), whose first
    # 8 H2 floats the VALU output layer reads as its rows. Below 8 the extra row lands in a slot the kernels' `a < KO` guard drops, so the mutant
    # computes the same network there; that equivalence is asserted too, so it is known, not assumed.
    case = int_case(7, (128, 64), 8, recipe, 32)
    want = case_forward(case).astype(np.float64)
    extra = case["W"][-1][:1] + 1.0
    w1p, w2p, _ = _pack(case, 1)
    wide = dict(case, W=case["W"][:-1] + [np.concatenate([case["W"][-1], extra])])
    assert M.w3_layout(8) == 1 and M.w3_layout(9) == 0
    got = _run(case, 1, (w1p, w2p, _pack(wide, M.w3_layout(9))[2].reshape(-1)[:8 * 64]))
    moved = int((got != want).sum())
    print(f"mutant [w3p packed for KO + 1] recipe {recipe}: {moved} of {want.size} outputs differ")
    assert moved > 0
    small = int_case(7, (128, 64), 5, recipe, 32)
    wide = dict(small, W=small["W"][:-1] + [np.concatenate([small["W"][-1], small["W"][-1][:1] + 1.0])])
    for layout in (0, 1):
        w1p, w2p, _ = _pack(small, layout)
        assert np.array_equal(_run(small, layout, (w1p, w2p, _pack(wide, layout)[2])), case_forward(small))


@pytest.mark.parametrize("recipe", RECIPES)
def test_zero_mask_past_in_dim(recipe):
    # For an odd in_dim the upper lane half has one slot past the row's end. Two guards cover it: the
    # packing stores a zero weight there and the kernel loads x = 0 (`k < L`). For finite inputs either
    # one alone suffices (asserted: which is why the GPU suite poisons a neighbouring row with NaN / Inf,
    # where 0 * x is no longer 0); with both removed the slot multiplies the next row's first feature
    # by W1[.][L - 1], and the integer comparison sees it.
    L = 7
    assert ((L + 1) // 2) % 4 == 0  # no k-step padding: the slot past in_dim is the only masked one
    case = int_case(L, (128, 64), 8, recipe, 33)
    want = case_forward(case)[:32].astype(np.float64)
    i1 = M._index_maps(L, 128, 64, 8, torch.device("cpu"), 1)[0].numpy()
    w1p, w2p, w3p = _pack(case, 1)
    unmasked = case["W"][0].reshape(-1)[i1]
    assert not np.array_equal(unmasked, w1p)
    assert np.array_equal(_run(case, 1), want)
    assert np.array_equal(_run(case, 1, (unmasked, w2p, w3p)), want)
    assert np.array_equal(_run(case, 1, guard_x=False), want)
    got = _run(case, 1, (unmasked, w2p, w3p), guard_x=False)
    moved = int((got != want).sum())
    print(f"mutant [zero mask past in_dim removed, odd L] recipe {recipe}: {moved} of {want.size} outputs differ")
    assert moved > 0


# ---- why the summation order cannot matter ------------------------------------------------------------

@pytest.mark.parametrize("L,hidden,KO,recipe", [
    (34, (256, 256), 5, "A"), (34, (64, 64), 5, "Bx"), (34, (128, 64), 8, "Bw"), (306, (256,), 1, "A"), (1023, (96,), 9, "Bx")])
def test_shuffled_float32_summation_equals_int64(L, hidden, KO, recipe):
    case = int_case(L, hidden, KO, recipe, 16)
    want = case_forward(case)
    for seed in (0, 1):
        got = shuffled_f32_sum_forward(case["x"], case["W"], case["b"], np.random.default_rng(seed))
        assert got.dtype == np.float32 and np.array_equal(got.astype(np.int64), want)
    for f in (f32_chain_forward, f32_matmul_forward):
        assert np.array_equal(f(case["x"], case["W"], case["b"]).astype(np.int64), want)


def test_without_headroom_float32_is_not_exact():
    # the contrast: the same dense network with 12-bit odd inputs and first-layer weights has first-layer
    # sums of 34 products of ~2^24 each; float32 then rounds, in any order
    case = int_case(34, (64, 64), 5, "A", 32)
    rng = np.random.default_rng(5)
    case["x"] = (2 * rng.integers(-2048, 2048, size=case["x"].shape) + 1).astype(np.float32)
    case["W"][0] = (2 * rng.integers(-2048, 2048, size=case["W"][0].shape) + 1).astype(np.float32)
    want, headroom, _ = int_forward(case["x"], case["W"], case["b"])
    assert headroom[0] > LIMIT
    for f in (f32_chain_forward, f32_matmul_forward):
        assert not np.array_equal(f(case["x"], case["W"], case["b"]).astype(np.float64), want.astype(np.float64))
