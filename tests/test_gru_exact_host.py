"""Host tests of the exact method that pins the fused GRU step (oracle/gru_ref.py): the lane-by-lane
emulation of gru_step_kernel over pack_gru's fragments (tests/gru_emulation.py) equals the int64
evaluation of recipe S on bits for all six kernel forms; plain float32 evaluations of S in two
summation orders do too; every mutant of the packing changes the emulated output (pytest -s names each
and how many values it moved); and under recipe G the smallest change any of them makes to h' is at
least 100 x the bound the GPU test holds the kernel to (printed)."""
import numpy as np
import pytest

import gru_emulation as E
from gru_ref import UNIT, f32_forward, g_forward, gru_case, rows_of, s_forward, s_reference, same_bits

FORMS = [(H, layers) for H in (64, 128, 256) for layers in (1, 2)]
_id = lambda v: "x".join(map(str, v)) if isinstance(v, tuple) else str(v)  # noqa: E731


@pytest.mark.parametrize("form", FORMS, ids=_id)
@pytest.mark.parametrize("L,KO", [(1, 1), (7, 5), (34, 32), (9, 96)])
def test_emulation_equals_int64(L, KO, form):
    # 33 rows: a full wave and a wave of one row; reset rows and both projection activations once
    H, layers = form
    case = gru_case(L, H, layers, KO, 33)
    packed = E.pack_cpu(case)
    hw, yw = s_reference(case)
    h, y = E.emulate_gru(case, packed)
    assert same_bits(h, hw) and same_bits(y, yw)
    if L == 7:
        live = np.arange(33) % 5 != 1
        hw, yw = s_reference(case, 1, 1, live)
        h, y = E.emulate_gru(case, packed, act_pre=1, act_out=1, live=live)
        assert same_bits(h, hw) and same_bits(y, yw)


@pytest.mark.parametrize("L,H,layers,KO", [(34, 64, 2, 5), (1, 64, 1, 1), (1024, 256, 2, 256), (7, 128, 2, 32)])
def test_plain_float32_evaluations_equal_int64_in_either_order(L, H, layers, KO):
    # float32 sums term by term, forward and reversed, np.exp / np.tanh in float32: the gates saturate to
    # exactly 0 / 1 / +-1 and the sums are exact, so the order cannot matter
    case = gru_case(L, H, layers, KO, 161)
    hw, yw = s_reference(case)
    sub = rows_of(case, slice(0, 12))
    for reverse in (False, True):
        h, y = f32_forward(sub, reverse)
        assert h.dtype == np.float32 and same_bits(h, hw[:12]) and same_bits(y, yw[:12])
    live = np.arange(12) % 2 == 0
    hz, yz = s_reference(case, live=np.arange(161) % 2 == 0)
    h, y = f32_forward(sub, True, live)
    assert same_bits(h, hz[:12]) and same_bits(y, yz[:12])


def test_the_restated_x_index_is_the_packings():
    for L in (1, 2, 7, 9, 34, 1023):
        idx, valid = E.index_of("x", 192, L)
        i2, v2 = E.x_index(192, L, (L + 1) // 2)
        assert np.array_equal(valid, v2) and np.array_equal(idx[valid], i2[valid])


# ---- mutants --------------------------------------------------------------------------------------------

ML, MH, MKO, MN = 7, 64, 5, 64  # odd input width, two layers, out_dim below a pass of 32
POS = {"wi[0]": (0, "w_ih", 0), "wh[0]": (1, "w_hh", 0), "wi[1]": (3, "w_ih", 1), "wh[1]": (4, "w_hh", 1)}


def _mutants(case):
    """name -> (packed tuple of the mutant, the mutated network when the mutant is one, else None)."""
    H, L, KO = MH, ML, MKO
    NT = H // 32
    packed = E.pack_cpu(case)
    out = {}
    out["rho: lane halves contiguous instead of alternating"] = (E.pack_with_rho(case, E.halves_contiguous), None)
    for name, (pos, _, _) in POS.items():
        out[f"{name}: gate tiles r and z swapped"] = (E.replaced(packed, pos, E.swap_gate_tiles(packed[pos], NT)), None)
    for l in (0, 1):
        b = packed[3 * l + 2].copy()
        b[2 * H:3 * H], b[3 * H:] = packed[3 * l + 2][3 * H:], packed[3 * l + 2][2 * H:3 * H]
        out[f"b[{l}]: b_in and b_hn swapped"] = (E.replaced(packed, 3 * l + 2, b), None)
        b = packed[3 * l + 2].copy()
        b[:H] = case["b_ih"][l][:H]
        out[f"b[{l}]: b_hr left out of the fold"] = (E.replaced(packed, 3 * l + 2, b), None)
    wi0 = E.gather(case["w_ih"][0], *E.x_index(3 * H, L, L // 2))
    out["wi[0]: lane-half column split off by one (odd L)"] = (E.replaced(packed, 0, wi0), None)
    for name, (pos, key, l) in POS.items():
        kind = "x" if name == "wi[0]" else "h"
        W = case[key][l]
        idx, valid = E.index_of(kind, *W.shape)
        r, ka, kb, mut = E.find_swap(case, key, l, range(3 * H))
        out[f"{name}: two entries of row {r} swapped"] = (
            E.replaced(packed, pos, E.swap_in_packed(packed[pos], idx, valid, W.shape[1], r, ka, kb)), mut)
    idx, valid = E.index_of("h", KO, H)
    r, ka, kb, mut = E.find_swap(case, "w_o", None, range(KO))
    out[f"wo: two entries of row {r} swapped"] = (
        E.replaced(packed, 6, E.swap_in_packed(packed[6], idx, valid, H, r, ka, kb)), mut)
    return out


def test_every_mutant_changes_the_emulated_output():
    case = gru_case(ML, MH, 2, MKO, MN)
    hw, yw = s_reference(case)
    h, y = E.emulate_gru(case, E.pack_cpu(case))
    assert same_bits(h, hw) and same_bits(y, yw)
    for name, (packed, mut) in _mutants(case).items():
        hm, ym = E.emulate_gru(case, packed)
        moved = int((hm != hw).sum()), int((ym != yw).sum())
        print(f"mutant [{name}]: {moved[0]} of {hw.size} state values, {moved[1]} of {yw.size} outputs differ")
        assert moved[0] + moved[1] > 0, name
        if mut is not None:  # an exchange inside the fragments is the network with those two weights exchanged
            hx, yx, _ = s_forward(mut)
            assert same_bits(hm, hx * UNIT) and same_bits(ym, yx * UNIT), name


def test_rows_past_out_dim():
    # pack_gru zeroes the fragment rows past out_dim and the kernel stores only rows < out_dim. Either
    # guard alone gives the same y (asserted: so the mutant "non-zero rows past out_dim" is known to be
    # the same network, not assumed); with both removed the stray rows hold row out_dim - 1's products,
    # and the comparison sees them. On the GPU those rows are the next batch row's outputs or the guard
    # rows behind y.
    case = gru_case(ML, MH, 2, MKO, MN)
    _, yw = s_reference(case)
    packed = E.pack_cpu(case)
    idx, valid = E.index_of("h", MKO, MH)
    assert not valid.all()
    unmasked = E.replaced(packed, 6, case["w_o"].reshape(-1)[idx])
    assert not np.array_equal(unmasked[6], packed[6])
    wide = np.concatenate([yw, np.zeros((MN, 32 - MKO), np.float32)], axis=1)
    assert same_bits(E.emulate_gru(case, unmasked)[1], yw)
    assert same_bits(E.emulate_gru(case, packed, guard_store=False)[1], wide)
    got = E.emulate_gru(case, unmasked, guard_store=False)[1]
    moved = int((got != wide).sum())
    print(f"mutant [non-zero rows past out_dim, store guard removed]: {moved} of {wide.size} values differ")
    assert moved > 0


def test_recipe_g_separates_every_mutant_from_the_bound():
    # float64 gates on both sides: what a mutant moves, against the bound 4 max(e32, 2^-24) on the last
    # layer's h' (for the output projection's mutant: on y against y's bound)
    case = gru_case(ML, MH, 2, MKO, MN, "G")
    g = g_forward(case)
    base_h, base_y = E.emulate_gru(case, E.pack_cpu(case), gate_dtype=np.float64)
    assert same_bits(base_h[:, 0], g["h_exact"][:, 0])
    assert np.abs(base_h[:, 1] - g["h"]).max() <= 2.0 ** -50 and np.abs(base_y - g["y"]).max() <= 2.0 ** -40
    ratios = {}
    for name, (packed, _) in _mutants(case).items():
        hm, ym = E.emulate_gru(case, packed, gate_dtype=np.float64)
        if name.startswith("wo"):
            ry = float((np.abs(ym - base_y) / g["y_bound"]).max())
            print(f"G mutant [{name}]: max |dy| / bound = {ry:.0f}")
            assert ry >= 100, name
            continue
        ratios[name] = float(np.abs(hm[:, 1] - base_h[:, 1]).max() / g["h_bound"])
        print(f"G mutant [{name}]: max |dh'| / bound = {ratios[name]:.0f}")
    worst = min(ratios, key=ratios.get)
    print(f"G separation: bound {g['h_bound']:.3e} (e32 {g['e32']:.3e}); smallest ratio {ratios[worst]:.0f} [{worst}]")
    assert ratios[worst] >= 100
