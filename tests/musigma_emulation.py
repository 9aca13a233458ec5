"""TEST INFRASTRUCTURE ONLY: what pins the dual mu / sigma-head kernels (msc_mlp{2,3}_relu_musigma:
musigma_row and head_act in csrc/mlp_kernels.hpp) to exact references. numpy and math only.

Integer part. oracle/mlp_ref.py:int_head_case folds to an exact integer matrix; head_case() recentres
the sigma biases (integers) so that every sigma column holds a value near 0, and with both activations
MSC_ACT_NONE [mu || log_std] is the int64 evaluation on bits, the sigma half clamped.

Dyadic part. dyadic_case() multiplies the folded head by an integer and scales each of its rows by a
power of two, 2^-shift[c]: products and sums stay exact, so pre-activation c of a row is the known
number num / 2^shift[c]. The scales spread the values over about [-16, 16] in steps of 2^-7 or finer;
every column but the last of each head has one value at +-2^-shift, and the last column of each head
is 8 x wider and starts at -16 (up to ~240), which reaches the range where expf(v) overflows (88.7):
nothing nearer 0 tells exp(v) / (1 + exp(v)) from the kernel's sigmoid. (The wide column stays above
-16 because 1 / (1 + expf(-v)) is 0 below -88.7 where the sigmoid is a float32 denormal: a relative
bound cannot hold there, and neither the kernel nor its float32 restatement claims it.)

  act64 / act32     head_act in float64 (erfc for GELU: 1 + erf cancels) and operation by operation in float32
  head_bound        unit(v) = 2^-24 s_f(v), e32, and the bound 4 max(e32, 1) units
  check_dist        what the GPU test asserts of a dist_out; the host test runs it on the emulation
  emulate_head      musigma_row's stores and sampling on flat buffers with guard rows, and its mutants
  gaussian_np       msc_gaussian_sample's arithmetic in numpy float32 (the emulation's reference)
"""
import math

import numpy as np

from mlp_ref import LIMIT, check_conditions, int_forward, int_head_case

F = np.float32
U24 = 2.0 ** -24
N = 161          # tests/test_gpu_mlp_exact.py's row count
PAD = 70         # guard rows behind every output
SENTINEL = 7.25
HALF_LOG_2PI = F(0.91893853320467274178)
ACT_NAMES = ("none", "relu", "tanh", "elu", "gelu", "sigmoid")  # MSC_ACT_* 0..5
SAMPLE_LIMITS = (-2.5, 1.5)  # integer part, sampling launches: exp(log_std) stays a usable number
_CASES = {}


def head_width(K):
    return 2 if K <= 2 else 4 if K <= 4 else 5 if K == 5 else 8


def bits(a):
    return np.ascontiguousarray(a, dtype=F).view(np.uint32)


# ---- cases ------------------------------------------------------------------------------------------------

def _checked(case):
    out, headroom, active = int_forward(case["x"], case["W"], case["b"], case["pre1"], case["group"])
    check_conditions(out, headroom, active)
    return out


def head_case(L, hidden, K, n=N, group=0):
    """(case, int64 outputs [n, 2K]) of int_head_case with the sigma biases moved (by integers) so
    that the median row of sigma column c holds (0, -1, 1, -2)[c % 4]: inside SAMPLE_LIMITS, so that
    clamp binds on most entries and not on all. Conditions asserted; built once, never modified."""
    key = (L, tuple(hidden), K, n, group)
    if key not in _CASES:
        case = int_head_case(L, tuple(hidden), K, n, pre1_group=group)
        out = _checked(case)
        b = case["b"][-1].astype(np.int64)
        for c in range(K):
            col = out[:, K + c]
            b[K + c] += (0, -1, 1, -2)[c % 4] - np.sort(col)[len(col) // 2]
        delta = (b - case["b"][-1].astype(np.int64))[K:]
        case["sigma"] = (case["sigma"][0], (case["sigma"][1].astype(np.int64) + delta).astype(F))  # the module's bias too
        case["b"][-1] = b.astype(F)
        assert np.array_equal(case["b"][-1].astype(np.int64), b)
        _CASES[key] = (case, _checked(case))
    return _CASES[key]


def int_limits(sg):
    """Clamp limits between integers at the quartiles of sigma: they bind on some entries, not on others."""
    lo, hi = float(np.floor(np.percentile(sg, 25))) + 0.5, float(np.ceil(np.percentile(sg, 75))) + 0.5
    assert lo < hi and np.any(sg < lo) and np.any(sg > hi) and np.any((sg > lo) & (sg < hi))
    return lo, hi


def int_expected(want, K, lo, hi):
    """[mu || clamp(sigma)] as float32 (exact: integers below 2^24 and limits at half integers)."""
    return np.concatenate([want[:, :K], np.clip(want[:, K:].astype(np.float64), lo, hi)], axis=1).astype(F)


def dyadic_case(L, hidden, K, n=N):
    """The folded head of head_case times an integer m, bias moved by integers, row c scaled by
    2^-shift[c] (module docstring). Returns the case (W[-1], b[-1] scaled, float32, exact) with
    "v" [n, 2K] float64: the exact pre-activations, "num" / "shift": their numerators and exponents."""
    key = ("dyadic", L, tuple(hidden), K, n)
    if key in _CASES:
        return _CASES[key]
    base, want = head_case(L, hidden, K, n)
    W, b0 = base["W"][-1].astype(np.int64), base["b"][-1].astype(np.int64)
    dot = want - b0
    narrow = [c for c in range(2 * K) if c % K != K - 1]
    mid = {c: np.sort(dot[:, c])[n // 2] for c in narrow}
    spread = max(int(np.abs(dot[:, c] - mid[c]).max()) for c in narrow)
    s = max(7, int(math.ceil(math.log2(spread / 16.0))))
    m = max(1, (16 << s) // spread)
    shift, b = np.full(2 * K, s), np.zeros(2 * K, np.int64)
    for c in range(2 * K):
        if c in mid:
            b[c] = -m * mid[c] + (1 if c % 2 == 0 else -1)  # the median row lands on +-2^-s
        else:
            shift[c] = s - 3
            b[c] = -m * dot[:, c].min() - (16 << (s - 3))   # the column starts at -16
    case = dict(base, W=base["W"][:-1] + [(m * W).astype(F)], b=base["b"][:-1] + [b.astype(F)])
    num = _checked(case)  # headroom of the integer network, before the scaling by powers of two
    assert np.array_equal(case["W"][-1].astype(np.int64), m * W) and np.array_equal(case["b"][-1].astype(np.int64), b)
    scale = 2.0 ** -shift.astype(np.float64)
    case["W"][-1] = (case["W"][-1].astype(np.float64) * scale[:, None]).astype(F)
    case["b"][-1] = (b * scale).astype(F)
    assert np.array_equal(case["b"][-1].astype(np.float64), b * scale)
    assert shift.min() >= 4  # steps of at most 1/16
    case.update(num=num, shift=shift, v=num * scale[None, :], mult=m, dot=((num - b) * scale[None, :]).astype(F))
    assert np.array_equal(case["dot"].astype(np.float64), (num - b) * scale[None, :])
    _CASES[key] = case
    return case


def coverage(v):
    """The ranges a head's pre-activations must reach (asserted before anything is compared)."""
    a = np.abs(v)
    return {"both signs": bool((v > 0).any() and (v < 0).any()), "0 < |v| < 2^-6": bool(((a > 0) & (a < 2.0 ** -6)).any()),
            "v > 9 and v < -9": bool((v > 9).any() and (v < -9).any()), "v in [-6, -3]": bool(((v >= -6) & (v <= -3)).any()),
            "expf(v) overflows": bool((v > 89).any())}


# ---- head_act -----------------------------------------------------------------------------------------------

_erfc = np.vectorize(math.erfc, otypes=[np.float64])
_erf = np.vectorize(math.erf, otypes=[np.float64])


def act64(code, v):
    """head_act on float64 arguments. GELU as 0.5 v erfc(-v / sqrt 2): 1 + erf loses everything below -3."""
    v = np.asarray(v, np.float64)
    with np.errstate(over="ignore", under="ignore"):
        if code == 1:
            return np.maximum(v, 0.0)
        if code == 2:
            return np.tanh(v)
        if code == 3:
            return np.where(v > 0, v, np.expm1(np.minimum(v, 0.0)))
        if code == 4:
            return 0.5 * v * _erfc(-v * math.sqrt(0.5))
        if code == 5:
            return 1.0 / (1.0 + np.exp(-v))
    assert code == 0
    return v


def act32(code, v, mutant=None):
    """head_act operation by operation in numpy float32 (erff: math.erf rounded to float32).
    mutant: "elu_exp" exp(v) - 1, "sigmoid_ratio" exp(v) / (1 + exp(v)), "gelu_tanh" the tanh form."""
    v = np.ascontiguousarray(v, F)
    one = F(1)
    with np.errstate(over="ignore", under="ignore", invalid="ignore"):
        if code == 1:
            return np.maximum(v, F(0))
        if code == 2:
            return np.tanh(v)
        if code == 3:
            neg = np.minimum(v, F(0))
            return np.where(v > 0, v, np.exp(neg) - one if mutant == "elu_exp" else np.expm1(neg))
        if code == 4:
            if mutant == "gelu_tanh":
                return F(0.5) * v * (one + np.tanh(F(0.7978845608028654) * (v + F(0.044715) * v * v * v)))
            return F(0.5) * v * (one + _erf(v * F(0.70710678118654752440)).astype(F))
        if code == 5:
            if mutant == "sigmoid_ratio":
                e = np.exp(v)
                return e / (one + e)
            return one / (one + np.exp(-v))
    assert code == 0
    return v


def scale_of(code, v, f):
    """s_f(v): |f(v)|; for GELU max(|f(v)|, 0.5 |v|), the absolute error of 1 + erf enters through 0.5 v."""
    return np.maximum(np.abs(f), 0.5 * np.abs(v)) if code == 4 else np.abs(f)


def head_bound(code, v):
    """(float64 reference, bound, e32) on exact arguments v: unit = 2^-24 s_f(v), e32 the float32
    restatement's largest error in units, bound = 4 max(e32, 1) units (the GRU tests' 4 max(e32, 2^-24))."""
    ref = act64(code, v)
    unit = U24 * scale_of(code, v, ref)
    d = np.abs(act32(code, v).astype(np.float64) - ref)
    assert np.all(d[unit == 0] == 0)
    e32 = float((d[unit > 0] / unit[unit > 0]).max()) if np.any(unit > 0) else 0.0
    return ref, 4.0 * max(e32, 1.0) * unit, e32


def _worst(name, code, v, got, ref, err, tol):
    r = np.where(tol > 0, err / np.where(tol > 0, tol, 1.0), np.where(err > 0, np.inf, 0.0))
    i = np.unravel_index(int(np.argmax(r)), r.shape)
    why = f"{name} {ACT_NAMES[code]}({float(v[i])!r}) = {float(got[i])!r}, float64 {float(ref[i])!r}: {float(r[i]):.3f} bounds"
    return float(r[i]), why


def check_dist(dist, v, K, act_mu, act_sigma, lo, hi):
    """What a [mu || log_std] result must satisfy on exact pre-activations v [n, 2K] (float64).
    NONE and RELU on bits, ELU's positive branch on bits, the others within head_bound; log_std entries
    whose float64 value lies outside a limit by more than the bound are the limit's float32 bits, the
    others within the bound of the clamped reference (|clamp a - clamp b| <= |a - b|).
    Returns {"ok", "why" (the first violation), "mu" / "sigma" (largest error / bound), "e32"}."""
    dist = np.asarray(dist, F)
    rep = {"ok": True, "why": "", "mu": 0.0, "sigma": 0.0, "e32": {}}

    def fail(msg):
        if rep["ok"]:
            rep["ok"], rep["why"] = False, msg

    if dist.shape != v.shape or not np.all(np.isfinite(dist)):
        fail(f"shape {dist.shape} or non-finite values")
        return rep
    lo32, hi32 = float(F(lo)), float(F(hi))
    for name, code, vv, got in (("mu", act_mu, v[:, :K], dist[:, :K]), ("sigma", act_sigma, v[:, K:], dist[:, K:])):
        ref, tol, e32 = head_bound(code, vv)
        rep["e32"][name] = e32
        want = np.clip(ref, lo32, hi32) if name == "sigma" else ref
        if code in (0, 1):
            if not np.array_equal(bits(got), bits(want)):
                fail(f"{name}: {ACT_NAMES[code]} is not bit-exact at {int((bits(got) != bits(want)).sum())} entries")
            continue
        pos = vv > 0
        if code == 3 and not np.array_equal(bits(got[pos]), bits(want[pos])):
            fail(f"{name}: elu(v) is not v on bits for v > 0")
        if name == "sigma":
            for must, lim in ((ref < lo32 - tol, lo32), (ref > hi32 + tol, hi32)):
                if not np.all(bits(got[must]) == bits(F(lim))):
                    fail(f"sigma: entries past the limit {lim} by more than the bound are not the limit")
        err = np.abs(got.astype(np.float64) - want)
        rep[name], why = _worst(name, code, vv, got, want, err, tol)
        if rep[name] > 1.0:
            fail(why)
    return rep


# ---- musigma_row ------------------------------------------------------------------------------------------------

def _exp32(a):
    with np.errstate(over="ignore", under="ignore"):
        return np.exp(np.ascontiguousarray(a, F))


def gaussian_np(mean, ls, floor, eps):
    """msc_gaussian_sample (sample_row's arithmetic, one log_std row per row) in numpy float32:
    (actions [n, K], logp [n], clipped [n, K])."""
    mean, eps = np.ascontiguousarray(mean, F), np.ascontiguousarray(eps, F)
    lsf = np.maximum(np.ascontiguousarray(ls, F), F(floor))
    sd = _exp32(lsf)
    with np.errstate(all="ignore"):
        act = mean + sd * eps
        d = act - mean
        term = (-(d * d) / (F(2) * sd * sd) - lsf) - HALF_LOG_2PI
    lp = np.zeros(len(mean), F)
    for a in range(mean.shape[1]):
        lp = lp + term[:, a]
    return act, lp, np.minimum(np.maximum(act, F(-1)), F(1))


MUTANTS = ("logp_guard", "dist_guard", "swap_halves", "clamp_first", "clamp_mu", "elu_exp", "sigmoid_ratio",
           "gelu_tanh", "ls_row0", "bias_vk")


def emulate_head(dot, b3, K, act_mu, act_sigma, lo, hi, eps=None, want_dist=True, mutant=None):
    """musigma_row over n rows in ascending order, in numpy float32, on flat buffers of n + PAD rows
    filled with SENTINEL, as the kernels reach it: o[a] = b3[a] + dot[a], o[VK + a] = b3[K + a] +
    dot[K + a] for a < K and 0 for the padded columns (b3 guarded, whp's columns zero); dot [n, 2K] is
    the exact output-layer sum without the bias, b3 a buffer of at least 2 VK floats (b_eff first), eps
    a flat buffer of at least (n + 1) K + 8 floats.
    mutant: logp_guard / dist_guard (the `a < K` guard of the sampling loop / of the dist_out stores
    removed), swap_halves, clamp_first, clamp_mu, ls_row0 (the sampling reads row j % 1's log_std),
    bias_vk (sigma's bias read at VK + a), elu_exp / sigmoid_ratio / gelu_tanh (act32's).
    Returns {"dist" [(n + PAD), 2K] or None, "act", "logp", "clip"} (None without eps)."""
    assert mutant is None or mutant in MUTANTS
    dot, b3 = np.asarray(dot, F), np.asarray(b3, F).reshape(-1)
    n, VK = dot.shape[0], head_width(K)
    lo32, hi32 = F(lo), F(hi)
    o = np.zeros((n, 2 * VK), F)
    for a in range(K):
        o[:, a] = b3[a] + dot[:, a]
        o[:, VK + a] = b3[(VK if mutant == "bias_vk" else K) + a] + dot[:, K + a]
    if mutant == "swap_halves":
        o = np.concatenate([o[:, VK:], o[:, :VK]], axis=1)
    clamp = lambda t: np.minimum(np.maximum(t, lo32), hi32)  # noqa: E731
    mu = act32(act_mu, o[:, :VK], mutant)
    if mutant == "clamp_first":
        ls = act32(act_sigma, clamp(o[:, VK:]), mutant)
    else:
        ls = clamp(act32(act_sigma, o[:, VK:], mutant))
    if mutant == "clamp_mu":
        mu = clamp(mu)
    new = lambda *shape: np.full(shape, F(SENTINEL), F)  # noqa: E731
    out = {"dist": None, "act": None, "logp": None, "clip": None}
    if want_dist:
        dist = new((n + PAD) * 2 * K)
        for j in range(n):
            for a in range(VK):
                if a < K or mutant == "dist_guard":
                    dist[j * 2 * K + a] = mu[j, a]
                    dist[j * 2 * K + K + a] = ls[j, a]
        out["dist"] = dist.reshape(n + PAD, 2 * K)
    if eps is not None:
        eps = np.asarray(eps, F).reshape(-1)
        act, clip, logp = new((n + PAD) * K), new((n + PAD) * K), new(n + PAD)
        cols = VK if mutant == "logp_guard" else K
        idx = np.arange(n)[:, None] * K + np.arange(cols)[None, :]
        lsr = ls[np.zeros(n, int) if mutant == "ls_row0" else np.arange(n)][:, :cols]
        lsf = np.maximum(lsr, lo32)
        sd = _exp32(lsf)
        with np.errstate(all="ignore"):
            v = mu[:, :cols] + sd * eps[idx]
            d = v - mu[:, :cols]
            term = (-(d * d) / (F(2) * sd * sd) - lsf) - HALF_LOG_2PI
        lp = np.zeros(n, F)
        for a in range(cols):
            lp = lp + term[:, a]
        cl = np.minimum(np.maximum(v, F(-1)), F(1))
        for j in range(n):
            for a in range(cols):
                act[idx[j, a]], clip[idx[j, a]] = v[j, a], cl[j, a]
            logp[j] = lp[j]
        out.update(act=act.reshape(n + PAD, K), clip=clip.reshape(n + PAD, K), logp=logp)
    return out


def sampling_matches(out, n, K, lo, eps):
    """The GPU test's sampling assertion on an emulated result: actions, logp and clipped are bit-equal
    to the sampling kernel's arithmetic on the result's own dist_out, and nothing is written past row n."""
    dist = out["dist"]
    a, lp, c = gaussian_np(dist[:n, :K], dist[:n, K:], lo, np.asarray(eps, F).reshape(-1)[:n * K].reshape(n, K))
    same = all(np.array_equal(bits(u[:n]), bits(w)) for u, w in ((out["act"], a), (out["logp"], lp), (out["clip"], c)))
    return same and tails_clean(out, n)


def tails_clean(out, n):
    return all(np.all(t[n:] == F(SENTINEL)) for t in out.values() if t is not None)


def eps_buffer(n, K, seed=0):
    """[n + PAD, K] standard-normal draws: the eight entries past a row's K are unlike any inside it."""
    e = np.random.default_rng([n, K, seed, 5]).normal(size=(n + PAD, K)).astype(F)
    flat = e.reshape(-1)
    win = flat[np.arange(n)[:, None] * K + np.arange(K + 8)[None, :]]
    assert all(np.unique(w).size == w.size for w in win)
    return e


def bias_buffer(b):
    """b_eff followed by eight values that are no bias (what a read past 2K would find)."""
    return np.concatenate([np.asarray(b, F), 1000.0 + 37.0 * np.arange(8)]).astype(F)


assert LIMIT == 1 << 24
