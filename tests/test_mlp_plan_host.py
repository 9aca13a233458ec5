"""CPU tests of the fused-MLP launchers' host side: which instantiation, output-layer width, LDS size and
grid each family picks (csrc/mlp_dispatch.hpp through msc_mlp_plan), and the full error text of every
argument check of the ten MLP entry points (capi.hip). All forms of a family give bit-identical results,
so no parity test can see a launcher that drifted to another form; the tables below are transcribed from
the four launchers as they were written out per family, and the error texts were recorded from that
library. No GPU call is made: every entry-point call below fails validation before any launch."""
import ctypes as C
import os
import subprocess
import sys

import pytest

from marlsc import abi
from marlsc.mlp import PLAN_KEYS, plan

SIZES = (64, 128, 256, 512)
# (H1, H2) -> (NT1, NT2, P, WPE) of the plain-output kernels; [256, 256] by MSC_MLP_P8, with the IL flag
RELU3 = {(128, 128): (4, 4, 4, 2), (64, 64): (2, 2, 2, 4), (64, 128): (2, 4, 2, 4), (64, 256): (2, 8, 2, 4),
         (64, 512): (2, 16, 2, 4), (128, 64): (4, 2, 2, 2), (128, 256): (4, 8, 4, 2), (128, 512): (4, 16, 4, 2),
         (256, 64): (8, 2, 2, 2), (256, 128): (8, 4, 4, 2), (256, 512): (8, 16, 8, 1), (512, 64): (16, 2, 2, 1),
         (512, 128): (16, 4, 4, 1), (512, 256): (16, 8, 4, 1), (512, 512): (16, 16, 4, 1)}
P8 = {41: (8, 8, 4, 1, 1), 21: (8, 8, 2, 1, 1), 8: (8, 8, 8, 1, 0), 4: (8, 8, 4, 2, 0), 2: (8, 8, 2, 2, 0)}
# (H1, H2) -> P of the wide kernels (NT = H / 32); waves per SIMD from the register estimate
WIDE3_P = {(64, 64): 2, (64, 128): 4, (64, 256): 4, (64, 512): 4, (128, 64): 2, (128, 128): 4, (128, 256): 4,
           (128, 512): 4, (256, 64): 2, (256, 128): 4, (256, 256): 4, (256, 512): 4, (512, 64): 2, (512, 128): 2,
           (512, 256): 2, (512, 512): 2}
RELU_WIDTH = {1: 1, 2: 2, 3: 4, 5: 5, 6: 8, 8: 8, 9: 0, 32: 0}    # out_dim -> VKO (0: MFMA output layer)
HEAD_WIDTH = {1: 2, 2: 2, 3: 4, 4: 4, 5: 5, 6: 8, 7: 8, 8: 8}      # k -> per-head width
WIDE_TILES = {1: 1, 32: 1, 33: 2, 96: 3, 97: 4, 128: 4}            # out_dim -> output tiles
TB = {32: 1, 64: 2, 96: 1, 128: 4, 256: 8, 1024: 8}
N = 1000                                                           # rows: 32 tiles, 8 blocks
NONE = dict.fromkeys(PLAN_KEYS, 0)


def _wide3_wpe(nt1, p, nto):
    return 2 if 16 * (nt1 + p + nto) + 8 * (p + nto) + 48 <= 240 else 1


def _want(**kw):
    return dict(NONE, supported=1, grid_blocks=8, **kw)


@pytest.fixture(autouse=True)
def no_knobs(monkeypatch):
    monkeypatch.delenv("MSC_MLP_P8", raising=False)


def _relu3(pair, p8=41):
    nt1, nt2, p, wpe, il = P8[p8] if pair == (256, 256) else RELU3[pair] + (0,)
    return dict(nt1=nt1, nt2=nt2, p=p, wpe=wpe, il=il)


@pytest.mark.parametrize("family", ["relu", "multi"])
def test_two_hidden_layers_plain_output(family):
    assert len(RELU3) == 15
    for h1 in SIZES:
        for h2 in SIZES:
            for ko, vko in RELU_WIDTH.items():
                form = _relu3((h1, h2))
                if vko == 0:
                    form["il"] = 0  # the MFMA output layer has no interleaved form
                assert plan(family, h1, h2, ko, N) == _want(width=vko, **form), (h1, h2, ko)
    for bad in [(96, 64), (64, 96), (1024, 64), (64, 32)]:
        assert plan(family, *bad, 5, N) == NONE


def test_two_hidden_layers_dual_head():
    for h1 in SIZES:
        for h2 in SIZES:
            for k, vk in HEAD_WIDTH.items():
                assert plan("musigma", h1, h2, k, N) == _want(width=vk, **_relu3((h1, h2))), (h1, h2, k)
    assert plan("musigma", 96, 64, 5, N)["supported"] == 0
    assert plan("musigma", 64, 64, 9, N)["supported"] == 0


def test_two_hidden_layers_wide_output():
    assert len(WIDE3_P) == 16
    for (h1, h2), p in WIDE3_P.items():
        for ko, nto in WIDE_TILES.items():
            want = _want(nt1=h1 // 32, nt2=h2 // 32, p=p, wpe=_wide3_wpe(h1 // 32, p, nto), width=nto)
            assert plan("wide", h1, h2, ko, N) == want, (h1, h2, ko)
    assert plan("wide", 64, 96, 40, N)["supported"] == 0
    assert plan("wide", 64, 64, 129, N)["supported"] == 0


def test_one_hidden_layer():
    for h, tb in TB.items():
        nt1, wpe = h // 32, 2 if tb == 8 else 4
        for family in ("relu", "multi"):
            for ko, vko in RELU_WIDTH.items():
                want = _want(nt1=nt1, tb=tb, wpe=wpe, width=vko, lds_bytes=nt1 * 16 * 2 * 2 * 16 if vko else 0)
                assert plan(family, h, 0, ko, N) == want, (family, h, ko)
        for k, vk in HEAD_WIDTH.items():
            lds = h * (8 if vk <= 4 else 16) * 4  # the staged head weights: H1 x stride floats, at most 32 KiB
            want = _want(nt1=nt1, tb=tb, wpe=wpe, width=vk, lds_bytes=lds) if lds <= 32768 else NONE
            assert plan("musigma", h, 0, k, N) == want, (h, k)
        for ko, nto in WIDE_TILES.items():
            assert plan("wide", h, 0, ko, N) == _want(nt1=nt1, tb=tb, wpe=1 if tb == 8 else 2, width=nto), (h, ko)
    for family in ("relu", "multi", "musigma", "wide"):
        for h in (0, 48, 1056):
            assert plan(family, h, 0, 5, N)["supported"] == 0, (family, h)


@pytest.mark.parametrize("p8", [None, 41, 21, 8, 4, 2, 7])
def test_p8_forms_of_256_256(monkeypatch, p8):
    if p8 is not None:
        monkeypatch.setenv("MSC_MLP_P8", str(p8))  # read at each launch
    form = _relu3((256, 256), p8 if p8 in P8 else 41)
    for family in ("relu", "multi"):
        assert plan(family, 256, 256, 5, N) == _want(width=5, **form)
        assert plan(family, 256, 256, 9, N) == _want(width=0, **dict(form, il=0))
        assert plan(family, 128, 256, 5, N) == _want(width=5, **_relu3((128, 256)))
    if p8 in (4, 2):  # the two-waves-per-SIMD A/B forms have no dual-head variant
        assert plan("musigma", 256, 256, 5, N) == NONE
    else:
        assert plan("musigma", 256, 256, 5, N) == _want(width=5, **form)
    assert plan("musigma", 256, 128, 5, N)["supported"] == 1
    assert plan("wide", 256, 256, 40, N) == _want(nt1=8, nt2=8, p=4, wpe=1, width=2)


_V3_CHILD = """
from marlsc.mlp import plan
N = 1000
for family in ("relu", "multi"):
    for shape in ((256, 256), (64, 64), (256, 0), (96, 0)):
        for ko in (1, 5, 8, 9):
            p = plan(family, *shape, ko, N)
            assert p["supported"] == 1 and p["width"] == 0 and p["il"] == 0 and p["lds_bytes"] == 0, (family, shape, ko, p)
    p = plan(family, 256, 256, 5, N)
    assert (p["nt1"], p["nt2"], p["p"], p["wpe"]) == (8, 8, 4, 1), p
for shape in ((256, 256), (64, 64), (256, 0)):
    for k in (1, 5, 8):
        assert plan("musigma", *shape, k, N)["supported"] == 0
p = plan("wide", 256, 0, 40, N)
assert p["supported"] == 1 and p["width"] == 2, p
print("ok")
"""


def test_v3_off_forces_the_mfma_output_layer():
    env = dict(os.environ, MSC_MLP_V3="0", PYTHONPATH=os.pathsep.join(sys.path))
    env.pop("MSC_MLP_P8", None)
    r = subprocess.run([sys.executable, "-c", _V3_CHILD], env=env, capture_output=True, text=True)  # the knob is read once
    assert r.returncode == 0 and r.stdout.strip() == "ok", r.stderr


def test_wide_one_hidden_layer_deep_tiles_threshold():
    at, past = plan("wide", 256, 0, 40, 32 * 1024), plan("wide", 256, 0, 40, 32 * 1024 + 1)
    assert (at["tb"], at["wpe"], at["grid_blocks"]) == (8, 1, 256)
    assert (past["tb"], past["wpe"], past["grid_blocks"]) == (4, 2, 257)
    assert plan("wide", 128, 0, 40, 32 * 1024 + 1)["tb"] == 4 and plan("wide", 192, 0, 40, 32)["tb"] == 2
    assert plan("relu", 256, 0, 5, 32 * 1024 + 1)["tb"] == 8  # the threshold is the wide family's only


def test_multi_grid_and_refusal():
    for rows, np_, blocks in [(24, 3, 3), (129 * 16, 16, 2 * 16), (128 * 64, 64, 64), (0, 5, 0)]:
        for shape in ((64, 64), (96, 0)):
            p = plan("multi", *shape, 5, rows, np_)
            assert p["supported"] == 1 and p["grid_blocks"] == blocks, (rows, np_, shape)
    per_policy = 128 * ((0x7fffffff // 64) + 1)  # one block more per policy than fits
    assert plan("multi", 64, 64, 5, 64 * per_policy, 64)["supported"] == 0
    assert plan("multi", 96, 0, 5, 64 * per_policy, 64)["supported"] == 0
    assert plan("multi", 64, 64, 5, 64 * (per_policy - 128), 64) == dict(_want(width=5, **_relu3((64, 64))),
                                                                          grid_blocks=64 * (0x7fffffff // 64))
    L = abi.lib()
    buf = (C.c_int32 * len(PLAN_KEYS))()
    for bad in [(1, 64, 64, 5, 25, 3), (1, 64, 64, 5, 24, 0), (0, 64, 64, 5, -1, 1), (4, 64, 64, 5, 24, 1)]:
        assert L.msc_mlp_plan(*bad, buf, len(PLAN_KEYS)) == -1


# ---- the argument checks: one bad argument at a time x each of the ten entry points ------------------
P_ = 256       # a pointer value that is never dereferenced
Q_ = 260       # a misaligned one
ALIGN2 = "b1, pre1 and the packed weights must be 16-byte aligned"
ALIGN3 = "b1, b2, pre1 and the packed weights must be 16-byte aligned"
SHAPE = "bad shape (n_rows %d, in_dim %d, out_dim %d)"
SHAPE_H = "bad shape (n_rows %d, in_dim %d)"
HID3 = "hidden sizes %d, %d: the %s MLP supports [H1, H2] with H1, H2 in {64, 128, 256, 512}"
HID2 = "hidden size %d: the %s MLP supports multiples of 32 up to 1024"
NO_H2 = "hidden2 must be one of {64, 128, 256, 512} (one hidden layer: %s)"
VALU = "sampling epilogue needs the VALU output layer (out_dim %d <= 8)"
TWO = ("mlp3", "mlp3_sampled", "multi3", "wide3", "musigma3")
ENTRIES = ("mlp3", "mlp3_sampled", "mlp2", "mlp2_sampled", "multi3", "multi2", "wide3", "wide2", "musigma3", "musigma2")


def _gauss(log_std=P_, rows=1, eps=P_, actions=P_, logp=P_, clipped=P_):
    return abi.MscGaussianEpilogue(log_std, rows, C.c_float(-3.5), eps, actions, logp, clipped)


def _head(act_mu=0, act_sigma=0, lo=-5.0, hi=2.0, eps=P_, actions=P_, logp=P_, clipped=P_, dist=P_):
    return abi.MscMuSigmaEpilogue(act_mu, act_sigma, C.c_float(lo), C.c_float(hi), eps, actions, logp, clipped, dist)


def _call(entry, **kw):
    """The entry point on a valid argument set with kw replaced: (return code, msc_last_error())."""
    L = abi.lib()
    two = entry in TWO
    a = dict(x=P_, n=24, np=3, L=34, h1=64 if two else 96, h2=64, ko=5, w1=P_, b1=P_, w2=P_, b2=P_, w3=P_, b3=P_, out=P_,
             pre1=None, grp=1, ep=_gauss() if entry.endswith("sampled") else _head() if entry.startswith("musigma") else None)
    assert set(kw) <= set(a) and kw, kw  # (the valid set itself would launch)
    a.update(kw)
    ep = None if a["ep"] is None else C.byref(a["ep"])
    hid = (a["h1"], a["h2"]) if two else (a["h1"],)
    mid = (a["w1"], a["b1"], a["w2"], a["b2"], a["w3"], a["b3"]) if two else (a["w1"], a["b1"], a["w3"], a["b3"])
    if entry.startswith("multi"):
        rc = getattr(L, f"msc_mlp{3 if two else 2}_relu_multi")(a["x"], a["n"], a["np"], a["L"], *hid, a["ko"], *mid, a["out"],
                                                               a["pre1"], ep, None)
    elif entry.startswith("musigma"):
        rc = getattr(L, f"msc_mlp{3 if two else 2}_relu_musigma")(a["x"], a["n"], a["L"], *hid, a["ko"], *mid, a["pre1"],
                                                                 a["grp"], ep, None)
    elif entry.startswith("wide"):
        rc = getattr(L, f"msc_mlp{3 if two else 2}_relu_wide")(a["x"], a["n"], a["L"], *hid, a["ko"], *mid, a["out"],
                                                              a["pre1"], a["grp"], ep, None)
    elif entry.endswith("sampled"):
        rc = getattr(L, f"msc_mlp{3 if two else 2}_relu_forward_sampled")(a["x"], a["n"], a["L"], *hid, a["ko"], *mid,
                                                                         a["out"], a["pre1"], a["grp"], ep, None)
    else:
        rc = getattr(L, f"msc_mlp{3 if two else 2}_relu_forward")(a["x"], a["n"], a["L"], *hid, a["ko"], *mid, a["out"],
                                                                 a["pre1"], a["grp"], None)
    return rc, L.msc_last_error().decode()


def _arg_cases():
    """(entry, replaced arguments, the full error text)"""
    for e in ENTRIES:
        two, multi, head, wide = e in TWO, e.startswith("multi"), e.startswith("musigma"), e.startswith("wide")
        word = "wide" if wide else "fused"
        # multi2 and wide2 share their two-layer entry points' check, b2 in its text included
        align = ALIGN3 if two or multi or wide else ALIGN2
        for k in ("b1", "w1", "w3") + (("b2", "w2") if two else ()):
            yield e, {k: Q_}, align
        yield e, {"pre1": Q_}, align
        for k in ("x", "w1", "b1", "w3", "b3") + (("w2", "b2") if two else ()):
            yield e, {k: None}, "null argument"
        if e.endswith("sampled") or head:
            yield e, {"ep": None}, "null argument"
        else:
            yield e, {"out": None}, "null argument"
        if not multi:
            yield e, {"pre1": P_, "grp": 0}, "pre1_group 0 must be >= 1"
            yield e, {"pre1": P_, "grp": -2}, "pre1_group -2 must be >= 1"
        for bad in ({"L": 0}, {"L": 1025}) + (() if multi else ({"n": -1},)):
            n, L = bad.get("n", 24), bad.get("L", 34)
            yield e, bad, SHAPE_H % (n, L) if head else SHAPE % (n, L, 5)
        if head:
            yield e, {"ko": 0}, "k 0: the fused mu/sigma head supports 1..8 actions"
            yield e, {"ko": 9}, "k 9: the fused mu/sigma head supports 1..8 actions"
        else:
            for ko in (0, 129 if wide else 33):
                yield e, {"ko": ko}, SHAPE % (24, 34, ko)
        if two:
            if head:
                text = "hidden sizes %d, %d: no fused mu/sigma head (H1, H2 in {64, 128, 256, 512}; not the MSC_MLP_P8 = 4 / 2 forms of [256, 256])"
                yield e, {"h1": 48}, text % (48, 64)
                yield e, {"h2": 96}, text % (64, 96)
            else:
                yield e, {"h1": 48}, HID3 % (48, 64, word)
                yield e, {"h2": 96}, HID3 % (64, 96, word)
            if e in ("mlp3", "mlp3_sampled"):
                yield e, {"h2": 0}, HID3 % (64, 0, word)
            else:
                yield e, {"h2": 0}, NO_H2 % {"multi3": "msc_mlp2_relu_multi", "wide3": "msc_mlp2_relu_wide",
                                             "musigma3": "msc_mlp2_relu_musigma"}[e]
        elif head:
            yield e, {"h1": 48}, "hidden size 48: the fused mu/sigma head supports multiples of 32 up to 512 for k = 5"
            yield e, {"h1": 1024}, "hidden size 1024: the fused mu/sigma head supports multiples of 32 up to 512 for k = 5"
            yield e, {"h1": 1056, "ko": 4}, "hidden size 1056: the fused mu/sigma head supports multiples of 32 up to 1024 for k = 4"
        else:
            for h in (0, 48, 1056):
                yield e, {"h1": h}, HID2 % (h, word)
        if multi:
            yield e, {"np": 0}, "n_policies 0 must be in 1..64"
            yield e, {"np": 65, "n": 130}, "n_policies 65 must be in 1..64"
            yield e, {"n": 25}, "n_rows 25 must be a non-negative multiple of n_policies 3"
            yield e, {"n": -3}, "n_rows -3 must be a non-negative multiple of n_policies 3"
            big = 3 * 128 * (0x7fffffff // 3 + 1)
            yield e, {"n": big}, "n_rows %d: too many rows for one launch" % big
            yield e, {"ep": _gauss(rows=2)}, "log_std_rows 2 must be 1 or n_policies 3"
        if head:
            yield e, {"ep": _head(act_mu=6)}, "activation codes 6, 0: must be MSC_ACT_* (0..5)"
            yield e, {"ep": _head(act_sigma=-1)}, "activation codes 0, -1: must be MSC_ACT_* (0..5)"
            yield e, {"ep": _head(lo=2.5)}, "log_std_min must be <= log_std_max"
            yield e, {"ep": _head(eps=None)}, "sampling outputs given without eps"
            yield e, {"ep": _head(logp=None)}, "null sampling buffer"
            yield e, {"ep": _head(eps=None, actions=None, logp=None, clipped=None, dist=None)}, \
                "nothing to write: neither dist_out nor sampling buffers"
        elif e not in ("mlp3", "mlp2"):  # (these two take no epilogue)
            for k in ("log_std", "eps", "actions", "logp", "clipped"):
                yield e, {"ep": _gauss(**{k: None})}, "null sampling buffer"
            yield e, {"ep": _gauss(rows=0)}, "log_std_rows 0 must be >= 1"
            if not wide:  # (the wide kernels sample at any width)
                yield e, {"ko": 9, "ep": _gauss()}, VALU % 9
                yield e, {"ko": 32, "ep": _gauss()}, VALU % 32


def test_every_argument_check_keeps_its_text():
    n = 0
    for entry, bad, text in _arg_cases():
        rc, got = _call(entry, **bad)
        assert (rc, got) == (-1, text), (entry, bad)
        n += 1
    assert n == 282
