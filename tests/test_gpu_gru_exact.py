"""GPU tests that pin the fused GRU step (msc_gru_step, csrc/gru.hip, and the fragment packing of
marlsc/gru.py) to exact references.

Recipe S (oracle/gru_ref.py): integer inputs, dyadic states, gate weights 2^14 w and biases on a
granule of 128 make every float32 partial sum exact in any order and every gate saturate to exactly
0, 1 or +-1, so h_out and y are compared with an int64 numpy evaluation on bits (+0 = -0). Every case
asserts the headroom, min |a| >= 128, that each gate is open on 25-75 % of the units and that the
outputs differ before it compares. tests/test_gru_exact_host.py shows on the CPU that the method is
sound and sees every mutant of the packing. Recipe G leaves the last layer's gates soft and holds the
kernel to 4 max(e32, 2^-24) of a float64 evaluation, e32 measured on a numpy float32 evaluation of the
same exact pre-activations (pytest -s prints error / bound). Every output is the first n rows of a
buffer with 70 sentinel rows behind them, asserted intact on every case."""
import ctypes as C

import numpy as np
import pytest

torch = pytest.importorskip("torch")

import gru_emulation as E  # noqa: E402
from gru_ref import UNIT, check_s, g_forward, gru_case, rows_of, s_forward, s_reference, same_bits  # noqa: E402
from marlsc import abi  # noqa: E402
from marlsc import gru as G  # noqa: E402

pytestmark = pytest.mark.gpu
N = 161  # one full block (4 waves of 32 rows), then a block with one full wave and a wave of one row
SENTINEL = 7.25
PAD = 70  # guard rows behind every output
FORMS = [(H, layers) for H in (64, 128, 256) for layers in (1, 2)]  # gru_step_kernel<2|4|8, 1|2>
_NETS = {}


def _id(v):
    return "x".join(map(str, v)) if isinstance(v, tuple) else str(v)


def _dev(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _p(t):
    return None if t is None else C.c_void_p(t.data_ptr())


def _np(t):
    torch.cuda.synchronize()
    return t.cpu().numpy()


class _Net:
    """A case's network packed on the device, stepped through the C ABI into guarded buffers."""

    def __init__(self, case):
        self.case = case
        self.L, self.H = case["w_ih"][0].shape[1], case["w_hh"][0].shape[1]
        self.layers, self.KO = len(case["w_ih"]), case["w_o"].shape[0]
        self.packed = list(G.pack_gru(E.as_net(case).cuda()))

    def step(self, x, h, n=None, reset=None, group=1, act_pre=0, act_out=0, store=True, packed=None):
        """(h_out [n, layers, H], y [n, KO]) as numpy; x / h: device tensors of at least n rows. The
        guard rows behind both outputs are asserted intact; without `store` h_out must stay untouched."""
        n = x.shape[0] if n is None else n
        packed = self.packed if packed is None else packed
        y = torch.full((n + PAD, self.KO), SENTINEL, device="cuda")
        ho = torch.full((n + PAD, self.layers, self.H), SENTINEL, device="cuda")
        gw = abi.MscGruWeights()
        for l in range(self.layers):
            gw.wi[l], gw.wh[l], gw.b[l] = (t.data_ptr() for t in packed[3 * l:3 * l + 3])
        gw.wo, gw.bo = packed[-2].data_ptr(), packed[-1].data_ptr()
        abi.check(abi.lib().msc_gru_step(_p(x), n, self.L, self.H, self.layers, self.KO, _p(h), C.byref(gw), act_pre, act_out,
                                         _p(reset), group, _p(y), _p(ho) if store else None, None))
        y, ho = _np(y), _np(ho)
        assert np.all(y[n:] == SENTINEL) and np.all(ho[n if store else 0:] == SENTINEL), "a write outside the first n rows"
        return ho[:n], y[:n]


def _net(L, H, layers, KO, n=N, recipe="S"):
    """A case and its packed network, built once and never modified."""
    key = (L, H, layers, KO, n, recipe)
    if key not in _NETS:
        _NETS[key] = _Net(gru_case(L, H, layers, KO, n, recipe))
    return _NETS[key]


def _exact(net, n=None, **kw):
    """One step of the case's own rows against the int64 reference (conditions asserted), on bits."""
    case = net.case
    hw, yw = s_reference(case, kw.get("act_pre", 0), kw.get("act_out", 0))
    h, y = net.step(_dev(case["x"]), _dev(case["h"]), n, **kw)
    n = len(case["x"]) if n is None else n
    return same_bits(h, hw[:n]) and same_bits(y, yw[:n])


# ---- every form, width and row count -----------------------------------------------------------------

@pytest.mark.parametrize("KO", [1, 2, 3, 4, 5, 7, 8, 31, 32, 64, 96, 160, 256])
@pytest.mark.parametrize("form", FORMS, ids=_id)
def test_every_form_equals_int64(form, KO):
    # scalar stores (out_dim % 4 != 0), float4 stores, one pass of 32 outputs and several
    assert _exact(_net(34, *form, KO))


@pytest.mark.parametrize("form", [(64, 1), (128, 2), (256, 2)], ids=_id)
@pytest.mark.parametrize("L", [1, 2, 3, 7, 8, 9, 15, 16, 17, 33, 1023, 1024])
def test_input_widths_equal_int64(L, form):
    # the first layer's split KS1 = ceil(L / 2), M4 = ceil(KS1 / 4): one feature, odd widths (the `k < L`
    # guard), k-step padding, and the widest input
    assert _exact(_net(L, *form, 5))


@pytest.mark.parametrize("form,KO", [((64, 2), 5), ((128, 1), 32), ((256, 2), 64)], ids=_id)
@pytest.mark.parametrize("n", [0, 1, 31, 32, 33, 127, 128, 129, 161])
def test_row_counts_write_nothing_past_their_rows(n, form, KO):
    # the first n rows of the 161-row case; for n = 0 nothing is written at all (step asserts that the
    # rows from n on keep the sentinel)
    assert _exact(_net(34, *form, KO), n)


@pytest.mark.parametrize("form,KO", [((64, 2), 5), ((128, 1), 32), ((256, 2), 64)], ids=_id)
def test_rows_do_not_depend_on_their_position(form, KO):
    # the same 40 rows at offsets 0 and 57 of the batch (other lanes, waves and blocks), among other rows
    net = _net(34, *form, KO)
    case, other = net.case, gru_case(34, *form, KO, N, seed=1)
    hw, yw = s_reference(case)
    outs = []
    for off in (0, 57):
        x, h = other["x"].copy(), other["h"].copy()
        x[off:off + 40], h[off:off + 40] = case["x"][:40], case["h"][:40]
        ho, y = net.step(_dev(x), _dev(h))
        outs.append((ho[off:off + 40], y[off:off + 40]))
    assert same_bits(outs[0][0], hw[:40]) and same_bits(outs[0][1], yw[:40])
    assert same_bits(outs[1][0], hw[:40]) and same_bits(outs[1][1], yw[:40])


@pytest.mark.parametrize("where", ["x", "h"])
@pytest.mark.parametrize("poison", ["nan", "inf"])
@pytest.mark.parametrize("L,form,KO", [(7, (256, 2), 5), (33, (64, 2), 7), (7, (128, 1), 8)], ids=_id)
def test_a_poisoned_row_leaves_the_others_alone(L, form, KO, poison, where):
    # rows 0, 77 and the last get NaN (or +-Inf) as input or as old state. With an odd L the slot past a
    # row's end is the next row's first feature, and rows past n read row 0: 0 * NaN is not 0, so a
    # missing guard on either load shows in a clean row. What the poisoned rows return is not asserted.
    net = _net(L, *form, KO)
    case = net.case
    hw, yw = s_reference(case)
    bad = [0, 77, N - 1]
    a = case[where].copy()
    fill = np.nan if poison == "nan" else np.where(np.arange(a[0].size) % 2 == 0, np.inf, -np.inf).reshape(a[0].shape)
    a[bad] = fill
    x, h = (a, case["h"]) if where == "x" else (case["x"], a)
    ho, y = net.step(_dev(x), _dev(h))
    keep = np.setdiff1d(np.arange(N), bad)
    assert same_bits(ho[keep], hw[keep]) and same_bits(y[keep], yw[keep])


# ---- resets ----------------------------------------------------------------------------------------------

def _flags(group, n):
    """Reset flags of n // group groups: every third group set, so that with group 3 the groups over
    rows 30..32 (set) and 63..65 (clear) straddle a 32-row tile; one set flag for group n."""
    g = np.arange(n // group)
    return ((g % 3 == 1) if n // group > 1 else g == 0).astype(np.uint8)


@pytest.mark.parametrize("form,KO", [((64, 2), 5), ((256, 2), 64), ((128, 1), 3)], ids=_id)
@pytest.mark.parametrize("group", [1, 3, 8, "n"])
def test_reset_rows_start_from_a_zero_state(group, form, KO):
    n = N if group in (1, "n") else N - N % group
    group = n if group == "n" else group
    net = _net(34, *form, KO)
    case = rows_of(net.case, slice(0, n))
    flags = _flags(group, n)
    live = np.repeat(flags == 0, group)
    if group == 3:
        assert not live[30:33].any() and live[63:66].all()
    assert flags.any()
    hz, yz, stats = s_forward(case, live=live)  # the reference of the reset rows: S from a zero state,
    check_s(stats, yz)                          # asserted to stay saturated
    hz, yz = (hz * UNIT).astype(np.float32), (yz * UNIT).astype(np.float32)
    x, h, r = _dev(case["x"]), _dev(case["h"]), _dev(flags)
    h1, y1 = net.step(x, h, reset=r, group=group)
    assert same_bits(h1, hz) and same_bits(y1, yz)
    zeroed = case["h"] * live[:, None, None]
    h2, y2 = net.step(x, _dev(zeroed.astype(np.float32)))
    assert same_bits(h1, h2) and same_bits(y1, y2)
    _, y3 = net.step(x, h, reset=r, group=group, store=False)  # (step asserts that h_out stays untouched)
    assert same_bits(y3, yz)
    # the old state of the reset rows is never read: NaN there changes nothing
    h_nan = case["h"].copy()
    h_nan[~live] = np.nan
    h4, y4 = net.step(x, _dev(h_nan), reset=r, group=group)
    assert same_bits(h4, hz) and same_bits(y4, yz)


@pytest.mark.parametrize("form,KO", [((64, 2), 5), ((256, 2), 64)], ids=_id)
def test_both_tiers_select_the_reset_rows(form, KO):
    # NaN in the old state of the reset rows, through gru_step_forward (fused) and through torch_step
    # (which multiplied by the mask until it selected too: 0 * NaN survived as NaN)
    case = _net(34, *form, KO).case
    net = E.as_net(case).cuda()
    assert G.gru_tier(net) == 1
    flags = _flags(3, 159)
    live = np.repeat(flags == 0, 3)
    sub = rows_of(case, slice(0, 159))
    h_nan = sub["h"].copy()
    h_nan[~live] = np.nan
    x, r = _dev(sub["x"]), _dev(flags)
    zeroed = _dev((sub["h"] * live[:, None, None]).astype(np.float32))
    with torch.no_grad():
        for step in (G.gru_step_forward, G.torch_step):
            y0, h0 = step(net, x, zeroed)
            y1, h1 = step(net, x, _dev(h_nan), r, 3)
            assert same_bits(_np(y1), _np(y0)) and same_bits(_np(h1), _np(h0)), step.__name__
            assert not np.isnan(_np(h1)).any()


# ---- through the module path -------------------------------------------------------------------------------

@pytest.mark.parametrize("acts", [(None, None), ("relu", None), (None, "relu"), ("relu", "relu")], ids=_id)
@pytest.mark.parametrize("form,KO", [((64, 1), 7), ((128, 2), 32), ((256, 2), 5)], ids=_id)
def test_module_path_equals_int64_on_both_tiers(form, KO, acts):
    case = _net(34, *form, KO).case
    net = E.as_net(case, *acts).cuda()
    assert G.gru_tier(net) == 1
    hw, yw = s_reference(case, int(acts[0] is not None), int(acts[1] is not None))
    x, h = _dev(case["x"]), _dev(case["h"])
    with torch.no_grad():
        y, hn = G.gru_step_forward(net, x, h)
        yt, ht = G.torch_step(net, x, h)
    assert y.shape == (N, KO) and hn.shape == (N, form[1], form[0])
    assert same_bits(_np(hn), hw) and same_bits(_np(y), yw)
    assert same_bits(_np(ht), hw) and same_bits(_np(yt), yw)


# ---- the comparison is not vacuous ----------------------------------------------------------------------------

@pytest.mark.parametrize("which", ["wh[1]", "wo"])
def test_swapped_packed_entries_are_seen_on_the_device(which):
    # packed correctly, then two entries of a fragment tensor exchanged on the host side of the ABI
    # call: a different network, which the comparison must see (and which is exactly the network with
    # those two weights exchanged)
    net = _net(34, 256, 2, 5)
    case = net.case
    assert _exact(net)
    key, l, pos, rows = ("w_hh", 1, 4, range(3 * 256)) if which == "wh[1]" else ("w_o", None, 6, range(5))
    W = case[key] if l is None else case[key][l]
    r, ka, kb, mut = E.find_swap(case, key, l, rows)
    idx, valid = E.index_of("h", *W.shape)
    packed = list(net.packed)
    packed[pos] = _dev(E.swap_in_packed(_np(packed[pos]), idx, valid, W.shape[1], r, ka, kb))
    h, y = net.step(_dev(case["x"]), _dev(case["h"]), packed=packed)
    hw, yw = s_reference(case)
    assert not (same_bits(h, hw) and same_bits(y, yw))
    hm, ym, _ = s_forward(mut)
    assert same_bits(h, hm * UNIT) and same_bits(y, ym * UNIT)


# ---- recipe G: soft gates ------------------------------------------------------------------------------------

@pytest.mark.parametrize("KO", [5, 64])
@pytest.mark.parametrize("form", FORMS, ids=_id)
def test_soft_gates_stay_within_four_times_the_float32_error(form, KO):
    # the earlier layer bit-exact; the last layer's h' within 4 max(e32, 2^-24) of float64 gate math on
    # the exact pre-activations; y within the bound derived in gru_ref.g_forward
    net = _net(34, *form, KO, recipe="G")
    g = g_forward(net.case)
    h, y = net.step(_dev(net.case["x"]), _dev(net.case["h"]))
    eh = float(np.abs(h[:, -1].astype(np.float64) - g["h"]).max())
    ry = float((np.abs(y.astype(np.float64) - g["y"]) / g["y_bound"]).max())
    ey = float(np.abs(y.astype(np.float64) - g["y"]).max())
    print(f"G {form[0]} x {form[1]} -> {KO}: h' err {eh:.3e} / bound {g['h_bound']:.3e} (e32 {g['e32']:.3e}); "
          f"y err {ey:.3e}, max err / bound {ry:.4f} (bound <= {g['y_bound'].max():.3e})")
    assert same_bits(h[:, :-1], g["h_exact"])
    assert eh <= g["h_bound"]
    assert ry <= 1.0


# ---- more than 2^31 elements -----------------------------------------------------------------------------------

def _big(L, H, layers, KO, n, need_gib):
    """n rows of S-valued data filled on the device in chunks; a strided sample of 1,000 rows and the
    last 200 against the int64 reference evaluated for those rows only."""
    free, _ = torch.cuda.mem_get_info()
    if free < need_gib << 30:
        pytest.skip(f"{free >> 30} GiB free: the case needs {need_gib} GiB")
    net = _net(L, H, layers, KO, 1)
    g = torch.Generator(device="cuda").manual_seed(L + H + KO)
    x = torch.empty((n, L), device="cuda").random_(0, 9, generator=g).sub_(4.0)
    h = torch.empty((n, layers, H), device="cuda")
    step = (1 << 27) // (layers * H)
    for a in range(0, n, step):  # non-zero multiples of 2^-6 in (-1, 1)
        c = h[a:a + step]
        c.random_(1, 64, generator=g).mul_(UNIT)
        c.mul_(torch.empty_like(c).random_(0, 2, generator=g).mul_(2.0).sub_(1.0))
    y, ho = torch.empty((n, KO), device="cuda"), torch.empty((n, layers, H), device="cuda")
    assert max(h.numel(), y.numel()) > 2 ** 31
    gw = abi.MscGruWeights()
    for l in range(layers):
        gw.wi[l], gw.wh[l], gw.b[l] = (t.data_ptr() for t in net.packed[3 * l:3 * l + 3])
    gw.wo, gw.bo = net.packed[-2].data_ptr(), net.packed[-1].data_ptr()
    abi.check(abi.lib().msc_gru_step(_p(x), n, L, H, layers, KO, _p(h), C.byref(gw), 0, 0, None, 1, _p(y), _p(ho), None))
    idx = torch.cat([torch.arange(0, n, n // 1000)[:1000], torch.arange(n - 200, n)]).cuda()
    case = dict(net.case, x=_np(x[idx]), h=_np(h[idx]))
    got_h, got_y = _np(ho[idx]), _np(y[idx])
    del x, h, y, ho
    torch.cuda.empty_cache()
    hw, yw = s_reference(case)
    return same_bits(got_h, hw) and same_bits(got_y, yw)


def test_states_of_more_than_2_31_elements():
    # h_in and h_out of (2^22 + 33) x 2 x 256 floats each (8 GiB): jc * LAYERS * H past 2^31
    assert _big(1, 256, 2, 1, 2 ** 22 + 33, 20)


def test_outputs_of_more_than_2_31_elements():
    # y of (2^23 + 33) x 256 floats (8 GiB): j * KO past 2^31
    assert _big(1, 64, 1, 256, 2 ** 23 + 33, 16)
