"""CPU tests of the references the GPU rollout-math tests rely on (oracle/gae_ref.py,
oracle/philox_ref.py): Philox known answers, the float32 emulation of the GAE kernels against the
float64 recurrence and its derived bound, mutants of the recurrence that the bound must reject, the
normalisation bound against an emulation of adv_norm_kernel, and the keyed normals' properties."""
import numpy as np
import pytest

from gae_ref import U32, adv_norm_f32, gae, gae_bounded, gae_f32, normalize_bounded, normalize_grouped, stats_of, target_bound
from philox_ref import normal_keyed_ref, philox4x32_10

GAMMA, LAM = 0.99, 0.95


@pytest.mark.parametrize("ctr, key, want", [
    ((0, 0, 0, 0), (0, 0), (0x6627E8D5, 0xE169C58D, 0xBC57AC4C, 0x9B00DBD8)),
    ((0xFFFFFFFF,) * 4, (0xFFFFFFFF,) * 2, (0x408F276D, 0x41C83B0E, 0xA20BC7C6, 0x6D5451FD)),
    ((0x243F6A88, 0x85A308D3, 0x13198A2E, 0x03707344), (0xA4093822, 0x299F31D0),
     (0xD16CFE09, 0x94FDCCEB, 0x5001E420, 0x24126EA1)),
])
def test_philox_known_answers(ctr, key, want):
    # Random123's kat_vectors for philox4x32-10
    assert tuple(int(x) for x in philox4x32_10(ctr, key)) == want
    # arrays give what scalars give, element by element
    got = philox4x32_10([np.array([c, 0], np.uint64) for c in ctr], [np.array([k, 0], np.uint64) for k in key])
    assert tuple(int(x[0]) for x in got) == want
    assert tuple(int(x[1]) for x in got) == (0x6627E8D5, 0xE169C58D, 0xBC57AC4C, 0x9B00DBD8)


def gae_inputs(N=5000, T=100):
    """The inputs of tests/test_gpu_parity.py::test_gae_kernel_vs_numpy."""
    rng = np.random.default_rng(0)
    r = rng.normal(size=(T, N)).astype(np.float32)
    v = rng.normal(size=(T + 1, N)).astype(np.float32)
    nv = rng.normal(size=(T, N)).astype(np.float32)
    te = (rng.random((T, N)) < 0.01).astype(np.uint8)
    tr = np.zeros((T, N), np.uint8)
    tr[49] = 1
    return r, v, nv, te, tr


@pytest.fixture(scope="module")
def case():
    r, v, nv, te, tr = gae_inputs()
    tr[20, ::3] = 1
    A, tgt, B = gae_bounded(r, v, nv, te, tr, GAMMA, LAM)
    for x in (r, v, nv, te, tr, A, tgt, B):
        x.setflags(write=False)
    return dict(r=r, v=v, nv=nv, te=te, tr=tr, A=A, tgt=tgt, B=B)


def _recurrence(c, mutant=None):
    """gae_f32 restated with one switch per mutant."""
    f = np.float32
    r, v, nv = c["r"], c["v"], c["nv"]
    te, tr = c["te"].astype(bool), c["tr"].astype(bool)
    T, N = r.shape
    g, l = f(GAMMA), f(LAM)
    gl = l if mutant == "lam_for_gamma_lam" else f(g * l)
    zero = np.zeros(N, f)
    adv = np.empty((T, N), f)
    a = zero
    for t in range(T - 1, -1, -1):
        v_next = v[min(t + 2, T)] if mutant == "v_next_one_row_late" else v[t + 1]
        cut = te[t] if mutant == "truncation_does_not_cut" else te[t] | tr[t]
        boot = v_next if mutant == "truncation_bootstraps_v_next" else np.where(tr[t], nv[t], v_next)
        boot = np.where(te[t], zero, boot)
        delta = ((r[t] + (g * boot).astype(f)).astype(f) - v[t]).astype(f)
        a = (delta + np.where(cut, zero, (gl * a).astype(f))).astype(f)
        adv[t] = a
    return adv


def test_gae_f32_within_bound_of_f64(case):
    c = case
    a32, t32 = gae_f32(c["r"], c["v"], c["nv"], c["te"], c["tr"], GAMMA, LAM)
    assert a32.dtype == np.float32 and t32.dtype == np.float32
    assert np.array_equal(a32, _recurrence(c))
    ea, et = np.abs(a32 - c["A"]), np.abs(t32 - c["tgt"])
    Bt = target_bound(c["B"], c["tgt"])
    print(f"max err/B {np.max(ea / c['B']):.3f} (targets {np.max(et / Bt):.3f}), median B {np.median(c['B']):.3g}, "
          f"max B {c['B'].max():.3g}")
    assert np.all(ea <= 2 * c["B"]) and np.all(et <= 2 * Bt)
    # the bound is what float32 needs, not the old 1e-4: tight enough to separate the double
    # 0.99 / 0.95 of gae() from the float32 constants the kernel receives
    assert c["B"].max() < 5e-5 and np.median(c["B"]) < 1e-5
    a64, _ = gae(c["r"].astype(np.float64), c["v"].astype(np.float64), c["nv"].astype(np.float64), c["te"],
                 c["tr"], GAMMA, LAM)
    assert np.abs(a64 - c["A"]).max() > 1e-6


def test_gae_none_arguments(case):
    c = case
    z = np.zeros_like(c["te"])
    for kw, eq in ((dict(nv=None), dict(nv=np.zeros_like(c["nv"]))), (dict(te=None), dict(te=z)),
                   (dict(tr=None), dict(tr=z)), (dict(te=None, tr=None), dict(te=z, tr=z))):
        a = {k: c[k] for k in ("r", "v", "nv", "te", "tr")}
        got = gae_f32(**{**a, **kw}, gamma=GAMMA, lam=LAM)
        want = gae_f32(**{**a, **eq}, gamma=GAMMA, lam=LAM)
        assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])
        gb, wb = gae_bounded(**{**a, **kw}, gamma=GAMMA, lam=LAM), gae_bounded(**{**a, **eq}, gamma=GAMMA, lam=LAM)
        assert all(np.array_equal(x, y) for x, y in zip(gb, wb))


@pytest.mark.parametrize("mutant", ["lam_for_gamma_lam", "truncation_bootstraps_v_next", "truncation_does_not_cut",
                                    "v_next_one_row_late"])
def test_mutants_break_the_bound(case, mutant):
    bad = _recurrence(case, mutant)
    frac = float(np.mean(np.abs(bad - case["A"]) > 2 * case["B"]))
    print(f"{mutant}: {100 * frac:.1f} % of the elements outside 2 B")
    assert frac >= 0.10


@pytest.mark.parametrize("groups, shift", [(1, 0.0), (8, 0.0), (1, 1e3), (8, 1e3)])
def test_normalize_bound_holds_for_the_f32_kernel_emulation(case, groups, shift):
    c = case
    r = (c["r"] + np.float32(shift)).astype(np.float32)
    A, _, B = gae_bounded(r, c["v"], c["nv"], c["te"], c["tr"], GAMMA, LAM)
    a32, _ = gae_f32(r, c["v"], c["nv"], c["te"], c["tr"], GAMMA, LAM)
    assert np.all(np.abs(a32 - A) <= 2 * B)
    x, tol = normalize_bounded(A, B, groups)
    np.testing.assert_allclose(x, normalize_grouped(A, groups), rtol=1e-12, atol=1e-12)
    x32 = adv_norm_f32(a32, stats_of(a32, groups), groups)
    ratio = np.abs(x32 - x) / tol
    print(f"G={groups} shift={shift}: max err/tol {ratio.max():.3f}, median tol {np.median(tol):.3g}, max tol {tol.max():.3g}")
    assert np.all(ratio <= 1.0)
    assert tol.max() < 1e-4  # 10x under the 1e-3 it replaces, at either scale


def test_adv_norm_emulation_guards():
    a = np.full((3, 4), 2.5, np.float32)
    # constant advantages: std 0 -> clamp 1e-4; zero table: count guard, mean 0, no NaN
    assert np.array_equal(adv_norm_f32(a, stats_of(a)), np.zeros_like(a))
    out = adv_norm_f32(a, np.zeros((1, 3)))
    assert np.array_equal(out, (a * np.float32(1e4)).astype(np.float32)) and np.isfinite(out).all()


def test_normal_keyed_ref_moments():
    out, rad = normal_keyed_ref(10, 2000, 10, 0, 12345, 0)
    n = out.size
    assert n == 200_000 and out.shape == rad.shape
    assert abs(out.mean()) <= 4 / np.sqrt(n)
    assert abs(out.var() - 1) <= 4 * np.sqrt(2 / n)
    assert np.all(np.abs(out) <= rad)
    # cos and sin halves are uncorrelated
    assert abs(np.mean(out[..., 0::2] * out[..., 1::2])) <= 4 / np.sqrt(n / 2)


def test_normal_keyed_ref_layout():
    o5, _ = normal_keyed_ref(2, 7, 5, 3, 99, 4)
    o6, _ = normal_keyed_ref(2, 7, 6, 3, 99, 4)
    assert np.array_equal(o5[..., 0::2], o6[..., 0::2])  # even elements: row_len 5 or 6 alike
    assert np.array_equal(o5, o6[..., :5])
    # every element depends on (seed, row0 + row, step0 + s, j) only
    big, _ = normal_keyed_ref(4, 9, 5, 10, 99, 100)
    part, _ = normal_keyed_ref(2, 4, 5, 13, 99, 101)
    assert np.array_equal(big[1:3, 3:7], part)
    # rows past 2^32 use the counter's high word; the step word wraps mod 2^32
    lo, _ = normal_keyed_ref(1, 1, 4, 5, 99, 0)
    hi, _ = normal_keyed_ref(1, 1, 4, 2 ** 32 + 5, 99, 0)
    assert not np.array_equal(lo, hi)
    w, _ = normal_keyed_ref(2, 3, 4, 0, 99, 2 ** 32 - 1)
    z, _ = normal_keyed_ref(1, 3, 4, 0, 99, 0)
    assert np.array_equal(w[1:], z)
    a, _ = normal_keyed_ref(1, 2, 4, 0, 1, 0)
    b, _ = normal_keyed_ref(1, 2, 4, 0, 1 << 32, 0)
    assert not np.array_equal(a, b)  # both key words are used
    assert U32 == 2.0 ** -24
