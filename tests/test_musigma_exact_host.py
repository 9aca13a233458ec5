"""Host tests of the method that pins the dual mu / sigma-head kernels (tests/musigma_emulation.py, used
by tests/test_gpu_musigma_exact.py): the float64 head activations agree with mpmath, the float32
restatement's error e32 is printed per activation, the dyadic cases reach every range the GPU test
asserts, the numpy restatement of musigma_row passes every check the GPU test applies to the device,
and each mutant of it fails one (pytest -s names the quantity that sees it)."""
import numpy as np
import pytest

import musigma_emulation as E

# the activation cases of the GPU file: (L, hidden, K)
ACT_CASES = [(34, (64, 64), 3), (34, (96,), 7), (34, (256, 256), 5), (34, (512,), 8)]
_id = lambda v: "x".join(map(str, v)) if isinstance(v, tuple) else str(v)  # noqa: E731


def test_float64_activations_agree_with_mpmath():
    # to 2^-50 of s_f(v), the scale the bound's unit is built on: on the arguments of two dyadic cases
    # and on a grid through the saturated ranges
    mp = pytest.importorskip("mpmath")
    mp.mp.prec = 200
    fn = {2: mp.tanh, 3: lambda t: t if t > 0 else mp.expm1(t), 4: lambda t: t * mp.erfc(-t / mp.sqrt(2)) / 2,
          5: lambda t: 1 / (1 + mp.exp(-t))}
    v = np.concatenate([E.dyadic_case(*ACT_CASES[0])["v"].reshape(-1), E.dyadic_case(*ACT_CASES[1])["v"].reshape(-1)[::3],
                        np.linspace(-16, 16, 513), [2.0 ** -20, -2.0 ** -20, 100.0, 240.0]])
    for code, f in fn.items():
        ref = E.act64(code, v)
        worst = 0.0
        for t, r in zip(v, ref):
            exact = f(mp.mpf(float(t)))
            s = max(abs(exact), abs(mp.mpf(float(t))) / 2) if code == 4 else abs(exact)
            if s != 0:
                worst = max(worst, float(abs(mp.mpf(float(r)) - exact) / s))
            else:
                assert r == 0
        print(f"float64 {E.ACT_NAMES[code]}: {worst / 2.0 ** -53:.2f} x 2^-53 of s_f over {v.size} arguments")
        assert worst <= 2.0 ** -50


@pytest.mark.parametrize("L,hidden,K", ACT_CASES, ids=_id)
def test_dyadic_cases_reach_every_range_and_e32_is_small(L, hidden, K):
    case = E.dyadic_case(L, hidden, K)
    for head in (case["v"][:, :K], case["v"][:, K:]):
        assert all(E.coverage(head).values()), E.coverage(head)
    for code in range(6):
        ref, tol, e32 = E.head_bound(code, case["v"])
        print(f"e32 {E.ACT_NAMES[code]:8s} {_id(hidden)} K={K}: {e32:.3f} units of 2^-24 s_f")
        assert e32 == 0.0 if code < 2 else 0.5 <= e32 <= 8.0  # a float32 evaluation: a few roundings, not more
        assert np.array_equal(E.bits(E.act32(3, case["v"])[case["v"] > 0]), E.bits(case["v"][case["v"] > 0]))


def _int_run(hidden, K, lim=None, **kw):
    case, want = E.head_case(34, hidden, K)
    b = case["b"][-1]
    lo, hi = lim or E.int_limits(want[:, K:])
    eps = E.eps_buffer(E.N, K)
    out = E.emulate_head((want - b.astype(np.int64)).astype(E.F), E.bias_buffer(b), K, 0, 0, lo, hi, eps, **kw)
    rep = E.check_dist(out["dist"][:E.N], want.astype(np.float64), K, 0, 0, lo, hi)
    return rep["ok"], E.sampling_matches(out, E.N, K, lo, eps), E.tails_clean(out, E.N), rep


def _dyadic_run(L, hidden, K, acts, lim, **kw):
    case = E.dyadic_case(L, hidden, K)
    eps = E.eps_buffer(E.N, K)
    out = E.emulate_head(case["dot"], E.bias_buffer(case["b"][-1]), K, acts[0], acts[1], lim[0], lim[1], eps, **kw)
    rep = E.check_dist(out["dist"][:E.N], case["v"], K, acts[0], acts[1], *lim)
    return rep["ok"], E.sampling_matches(out, E.N, K, lim[0], eps), E.tails_clean(out, E.N), rep


@pytest.mark.parametrize("hidden,K", [((64, 64), 3), ((96,), 7), ((256, 256), 5), ((128,), 1), ((160,), 6)], ids=_id)
def test_the_emulation_passes_the_integer_checks(hidden, K):
    for lim in (None, E.SAMPLE_LIMITS):
        dist_ok, sample_ok, tails_ok, rep = _int_run(hidden, K, lim)
        assert dist_ok and sample_ok and tails_ok, rep["why"]
    case, want = E.head_case(34, hidden, K)
    sg, (lo, hi) = want[:, K:], E.SAMPLE_LIMITS
    assert np.any(sg < lo) and np.any(sg > hi) and np.any((sg > lo) & (sg < hi))
    out = E.emulate_head((want - case["b"][-1].astype(np.int64)).astype(E.F), E.bias_buffer(case["b"][-1]), K, 0, 0, lo, hi,
                         E.eps_buffer(E.N, K), want_dist=False)
    assert out["dist"] is None and E.tails_clean(out, E.N) and np.all(np.isfinite(out["logp"][:E.N]))


@pytest.mark.parametrize("lim", [(-4.6, 4.6), (-0.25, 0.25)], ids=str)
@pytest.mark.parametrize("L,hidden,K", ACT_CASES[:2], ids=_id)
def test_the_emulation_passes_the_dyadic_checks(L, hidden, K, lim):
    worst = {}
    for am in range(6):
        for asg in range(6):
            dist_ok, sample_ok, tails_ok, rep = _dyadic_run(L, hidden, K, (am, asg), lim)
            assert dist_ok and sample_ok and tails_ok, rep["why"]
            worst[am] = max(worst.get(am, 0.0), rep["mu"])
            worst[asg] = max(worst.get(asg, 0.0), rep["sigma"])
    # the restatement is its own e32: at most 1 / 4 of the bound
    print(f"float32 restatement {_id(hidden)} K={K} clamp {lim}: error / bound " +
          ", ".join(f"{E.ACT_NAMES[c]} {worst[c]:.3f}" for c in range(2, 6)))
    assert max(worst.values()) <= 0.25


# mutant -> the case of the GPU file that must see it: ("int", hidden, K, limits) or ("dyadic", case, acts, limits)
MUTANT_CASES = {
    "logp_guard": ("int", (96,), 7, E.SAMPLE_LIMITS),
    "dist_guard": ("int", (96,), 7, E.SAMPLE_LIMITS),
    "swap_halves": ("int", (64, 64), 3, None),
    "clamp_first": ("dyadic", ACT_CASES[0], (2, 2), (-4.6, 4.6)),
    "clamp_mu": ("int", (64, 64), 3, None),
    "elu_exp": ("dyadic", ACT_CASES[0], (3, 3), (-4.6, 4.6)),
    "sigmoid_ratio": ("dyadic", ACT_CASES[1], (5, 5), (-4.6, 4.6)),
    "gelu_tanh": ("dyadic", ACT_CASES[0], (4, 4), (-4.6, 4.6)),
    "ls_row0": ("int", (96,), 7, E.SAMPLE_LIMITS),
    "bias_vk": ("int", (96,), 7, None),
}


@pytest.mark.parametrize("mutant", E.MUTANTS)
def test_every_mutant_fails_a_check_the_gpu_test_makes(mutant):
    kind, *args = MUTANT_CASES[mutant]
    run = (lambda **kw: _int_run(*args, **kw)) if kind == "int" else (lambda **kw: _dyadic_run(*args[0], *args[1:], **kw))
    assert all(run()[:3])
    dist_ok, sample_ok, tails_ok, rep = run(mutant=mutant)
    seen = [name for name, ok in (("dist_out against the reference", dist_ok), ("sampling bit-equality", sample_ok),
                                  ("guard rows", tails_ok)) if not ok]
    print(f"mutant [{mutant}] on {args[:2]}: seen by {', '.join(seen) or 'nothing'}" + (f" ({rep['why']})" if rep["why"] else ""))
    assert seen, mutant


def test_padded_guards_decide_only_below_the_head_width():
    # K equal to its width (2, 4, 5, 8): the guards never decide, and removing them changes nothing,
    # which is why the suite could not see them before K = 1, 3, 6, 7 sampled
    for K in (2, 4, 5, 8):
        assert E.head_width(K) == K
        for mutant in ("logp_guard", "dist_guard", "bias_vk"):
            assert all(_int_run((96,), K, E.SAMPLE_LIMITS, mutant=mutant)[:3])
    for K in (1, 3, 6, 7):
        assert E.head_width(K) > K
        for mutant in ("logp_guard", "dist_guard", "bias_vk"):
            assert not all(_int_run((96,), K, E.SAMPLE_LIMITS, mutant=mutant)[:3]), (K, mutant)
