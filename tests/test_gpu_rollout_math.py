"""GPU tests of the kernels that turn a rollout into a training batch (csrc/gae.hip), through the C
ABI: GAE against a float32 emulation of the recurrence (bit for bit) and against the float64
recurrence with its derived error bound, the advantage statistics and their normalisation, the
keyed Philox / Box-Muller normals against a numpy Philox, and the Gaussian action sampling against a
float64 restatement. The references and bounds are oracle/gae_ref.py and oracle/philox_ref.py;
tests/test_rollout_math_host.py shows on the CPU that they are sound and sharp enough.

Every test prints the largest error as a fraction of its bound (pytest -s shows it)."""
import ctypes as C

import numpy as np
import pytest

torch = pytest.importorskip("torch")

from gae_ref import (U32, adv_norm_f32, gae_blocks, gae_bounded, gae_f32, normalize_bounded, stats_bounded,  # noqa: E402
                     target_bound)
from marlsc import abi  # noqa: E402
from philox_ref import normal_keyed_ref  # noqa: E402

pytestmark = pytest.mark.gpu
GAMMA, LAM = 0.99, 0.95
SENTINEL = 7.0


def _dev(x):
    return None if x is None else torch.from_numpy(np.array(x, order="C")).cuda()


def _p(t):
    return None if t is None else C.c_void_p(t.data_ptr())


def _np(t):
    torch.cuda.synchronize()
    return t.cpu().numpy()


def _bits(x):
    return np.ascontiguousarray(x, dtype=np.float32).view(np.uint32)


def _call(d, N, T, adv, tgt, stats, G=1, grouped=False):
    """msc_gae (G == 1) or msc_gae_grouped on device tensors / None; returns the return code."""
    L = abi.lib()
    head = (_p(d["r"]), _p(d["v"]), _p(d["nv"]), _p(d["te"]), _p(d["tr"]), N, T, C.c_float(GAMMA), C.c_float(LAM),
            _p(adv), _p(tgt))
    if G == 1 and not grouped:
        return L.msc_gae(*head, _p(stats), None)
    return L.msc_gae_grouped(*head, G, _p(stats), None)


def _inputs(T, N, pattern, seed=0):
    rng = np.random.default_rng([T, N % 65521, seed])
    r = rng.normal(size=(T, N)).astype(np.float32)
    v = rng.normal(size=(T + 1, N)).astype(np.float32)
    nv = rng.normal(size=(T, N)).astype(np.float32)
    te = np.zeros((T, N), np.uint8)
    tr = np.zeros((T, N), np.uint8)
    if pattern == "te_last":
        te[T - 1] = 1
    elif pattern == "tr_last":
        tr[T - 1] = 1
    elif pattern == "te_and_tr":  # on the same elements: termination wins (bootstrap 0, not nv)
        te[:] = rng.random((T, N)) < 0.2
        te[0, 0] = te[T - 1, N - 1] = 1
        tr[:] = te
    elif pattern == "all_tr":
        tr[:] = 1
    elif pattern == "random":
        te[:] = rng.random((T, N)) < 0.05
        tr[T // 2] = 1
    else:
        assert pattern == "none"
    return dict(r=r, v=v, nv=nv, te=te, tr=tr)


def _check_stats(s, a32, T, N, G, vec, calls=1, what=""):
    """count exact; |sum - sum of the emulation's values| <= d 2^-53 sum |a| with d = T + 16 + blocks
    (the adds of the longest chain: a lane's T steps, the lane / wave / block combination, one atomic
    per block), likewise the squares. `calls` accumulated calls: `calls` times each."""
    ref, tol = stats_bounded(a32, G, T + 16 + gae_blocks(N, vec))
    s = np.asarray(s).reshape(G, 3)
    assert np.array_equal(s[:, 2], calls * ref[:, 2]), what
    err = np.abs(s[:, :2] - calls * ref[:, :2])
    print(f"{what} stats: max err/bound {np.max(err / (calls * tol)):.2e}")
    assert np.all(err <= calls * tol), what


def _check_gae(h, T, N, G=1, grouped=False, vec=None, what=""):
    """Run the kernel on host inputs h and assert the three properties; returns (gpu adv, device adv,
    device stats, A, B)."""
    d = {k: _dev(x) for k, x in h.items()}
    adv = torch.full((T, N), SENTINEL, device="cuda")
    tgt = torch.full((T, N), SENTINEL, device="cuda")
    stats = torch.zeros((G, 3), dtype=torch.float64, device="cuda")
    assert _call(d, N, T, adv, tgt, stats, G, grouped) == 0
    a_gpu, t_gpu = _np(adv), _np(tgt)
    a32, t32 = gae_f32(h["r"], h["v"], h["nv"], h["te"], h["tr"], GAMMA, LAM)
    A, tg, B = gae_bounded(h["r"], h["v"], h["nv"], h["te"], h["tr"], GAMMA, LAM)
    Bt = target_bound(B, tg)
    ea, et = np.abs(a_gpu - A), np.abs(t_gpu - tg)
    print(f"{what} T={T} N={N} G={G}: max err/(2B) adv {np.max(ea / (2 * B)):.3f} tgt {np.max(et / (2 * Bt)):.3f}; "
          f"bits differ adv {np.count_nonzero(_bits(a_gpu) != _bits(a32))} tgt {np.count_nonzero(_bits(t_gpu) != _bits(t32))}")
    assert np.all(ea <= 2 * B) and np.all(et <= 2 * Bt), what
    assert np.array_equal(_bits(a_gpu), _bits(a32)), what
    assert np.array_equal(_bits(t_gpu), _bits(t32)), what
    if vec is None:
        vec = N % 4 == 0 and h["te"] is not None and h["tr"] is not None
    _check_stats(_np(stats), a32, T, N, G, vec, what=what)
    return a_gpu, adv, stats, A, B


SHAPES = [(1, 4, 1), (7, 4, 1),  # vector kernel, fewer steps than its chunk of 8
          (8, 1024, 1),  # exactly one chunk, exactly one full block
          (9, 1028, 1),  # one lane into a second block, one step into a second chunk
          (17, 1, 1), (17, 255, 1), (17, 257, 1),  # scalar kernel
          (100, 4998, 1), (100, 5000, 1),
          (3, 699732, 3)]  # 684 blocks, the last partial
PATTERNS = ["none", "te_last", "tr_last", "te_and_tr", "all_tr", "random"]


@pytest.mark.parametrize("pattern", PATTERNS)
@pytest.mark.parametrize("T, N, G", SHAPES)
def test_gae_bit_exact_and_bounded(T, N, G, pattern):
    _check_gae(_inputs(T, N, pattern), T, N, G, what=pattern)


AT, AN = 17, 1024


@pytest.fixture(scope="module")
def aligned():
    """The aligned (17, 1024) call every argument form is compared with."""
    h = _inputs(AT, AN, "random")
    a_gpu, _, stats, _, _ = _check_gae(h, AT, AN, what="aligned")
    a32, t32 = gae_f32(h["r"], h["v"], h["nv"], h["te"], h["tr"], GAMMA, LAM)
    for x in list(h.values()) + [a32, t32]:
        x.setflags(write=False)
    return h, a32, t32, _np(stats)


@pytest.mark.parametrize("drop", [("nv",), ("te",), ("tr",), ("te", "tr"), ("nv", "te", "tr")])
def test_gae_null_inputs(aligned, drop):
    # NULL next_values: truncated rows bootstrap 0; NULL flags: none set (scalar kernel)
    h = dict(aligned[0])
    assert h["tr"].any() and h["te"].any()
    for k in drop:
        h[k] = None
    _check_gae(h, AT, AN, what="NULL " + "+".join(drop))


def test_gae_null_outputs(aligned):
    h, a32, t32, s_ref = aligned
    d = {k: _dev(x) for k, x in h.items()}
    for no_tgt, no_stats in ((True, False), (False, True), (True, True)):
        adv = torch.full((AT, AN), SENTINEL, device="cuda")
        tgt = None if no_tgt else torch.full((AT, AN), SENTINEL, device="cuda")
        stats = None if no_stats else torch.zeros(3, dtype=torch.float64, device="cuda")
        assert _call(d, AN, AT, adv, tgt, stats) == 0
        assert np.array_equal(_bits(_np(adv)), _bits(a32))
        if tgt is not None:
            assert np.array_equal(_bits(_np(tgt)), _bits(t32))
        if stats is not None:
            _check_stats(_np(stats), a32, AT, AN, 1, True, what="targets NULL")


@pytest.mark.parametrize("which", ["r", "adv", "tgt", "te"])
def test_gae_misaligned_pointers_fall_back_to_the_scalar_kernel(aligned, which):
    # one float (one byte for the flags) into a larger buffer: not 16-byte (4-byte) aligned
    h, a32, t32, _ = aligned
    d = {k: _dev(x) for k, x in h.items()}
    n = AT * AN

    def shifted(src, dtype):
        buf = torch.full((n + 8,), SENTINEL, dtype=dtype, device="cuda")
        view = buf[1:1 + n]
        if src is not None:
            view.copy_(src.reshape(-1))
        assert view.data_ptr() % (16 if dtype == torch.float32 else 4) != 0
        return buf, view

    adv = torch.full((n,), SENTINEL, device="cuda")
    tgt = torch.full((n,), SENTINEL, device="cuda")
    buf = None
    if which == "r":
        buf, d["r"] = shifted(d["r"], torch.float32)
    elif which == "te":
        buf, d["te"] = shifted(d["te"], torch.uint8)
    elif which == "adv":
        buf, adv = shifted(None, torch.float32)
    else:
        buf, tgt = shifted(None, torch.float32)
    stats = torch.zeros(3, dtype=torch.float64, device="cuda")
    assert _call(d, AN, AT, adv, tgt, stats) == 0
    assert np.array_equal(_bits(_np(adv)), _bits(a32).ravel())
    assert np.array_equal(_bits(_np(tgt)), _bits(t32).ravel())
    _check_stats(_np(stats), a32, AT, AN, 1, False, what="misaligned " + which)
    if which in ("adv", "tgt"):  # nothing written outside the [1, 1 + n) window
        b = _np(buf)
        assert b[0] == SENTINEL and np.all(b[1 + n:] == SENTINEL)


def test_gae_statistics_accumulate(aligned):
    h, a32, _, _ = aligned
    d = {k: _dev(x) for k, x in h.items()}
    adv = torch.empty((AT, AN), device="cuda")
    stats = torch.zeros(3, dtype=torch.float64, device="cuda")
    for _ in range(2):
        assert _call(d, AN, AT, adv, None, stats) == 0
    _check_stats(_np(stats), a32, AT, AN, 1, True, calls=2, what="two calls")


GROUPED = [(11, 12, 3), (11, 1285, 5), (11, 256, 64), (11, 8, 8)]


@pytest.mark.parametrize("T, N, G", GROUPED)
def test_gae_grouped_statistics(T, N, G):
    _check_gae(_inputs(T, N, "random"), T, N, G, grouped=True, what="grouped")


@pytest.mark.parametrize("why", ["G=0", "G=65", "G=7 does not divide N", "N<0", "rewards NULL"])
def test_gae_refusals_leave_outputs_untouched(why):
    T, N = 3, 1285
    h = _inputs(T, N, "random")
    d = {k: _dev(x) for k, x in h.items()}
    adv = torch.full((T, N), SENTINEL, device="cuda")
    tgt = torch.full((T, N), SENTINEL, device="cuda")
    stats = torch.zeros((64, 3), dtype=torch.float64, device="cuda")
    G = {"G=0": 0, "G=65": 65, "G=7 does not divide N": 7}.get(why, 5)
    if why == "rewards NULL":
        d["r"] = None
    rc = _call(d, -N if why == "N<0" else N, T, adv, tgt, stats, G, grouped=True)
    assert rc != 0
    with pytest.raises(RuntimeError):
        abi.check(rc)
    assert np.all(_np(adv) == SENTINEL) and np.all(_np(tgt) == SENTINEL) and not _np(stats).any()


# ---- normalisation ------------------------------------------------------------------------------

def _normalise(adv, n, G, stats):
    L = abi.lib()
    if G == 1:
        return L.msc_adv_normalize(_p(adv), n, _p(stats), None)
    return L.msc_adv_normalize_grouped(_p(adv), n, G, _p(stats), None)


@pytest.mark.parametrize("T, N, G, shift", [
    (100, 5000, 1, 0.0),
    (3, 699732, 3, 0.0),  # 2,099,196 elements > 8192 * 256: the kernel's second grid-stride pass
    (11, 1285, 5, 0.0), (11, 256, 64, 0.0),
    (50, 1024, 1, 1e3)])  # mean >> spread: the casts of the mean and E[a^2] - mean^2 matter
def test_normalise_within_derived_bound(T, N, G, shift):
    h = _inputs(T, N, "random")
    h["r"] = (h["r"] + np.float32(shift)).astype(np.float32)
    a_gpu, adv, stats, A, B = _check_gae(h, T, N, G, grouped=G > 1, what="normalise")
    s = _np(stats)
    assert _normalise(adv, T * N, G, stats) == 0
    x_gpu = _np(adv)
    x, tol = normalize_bounded(A, B, G)
    ratio = np.abs(x_gpu - x) / tol
    emu = adv_norm_f32(a_gpu, s, G)
    print(f"normalise T={T} N={N} G={G} shift={shift}: max err/tol {ratio.max():.3f}, max tol {tol.max():.3g}; "
          f"bits differ from the emulation on the device's statistics: {np.count_nonzero(_bits(x_gpu) != _bits(emu))}")
    assert np.isfinite(x_gpu).all() and np.all(ratio <= 1.0)
    assert np.array_equal(_bits(x_gpu), _bits(emu))


@pytest.mark.parametrize("c", [2.5, 0.1, -1e3])
def test_normalise_constant_advantages_take_the_std_clamp(c):
    # every row truncated, no next_values, V = 0: A = r = c everywhere, through the kernel's own statistics
    T, N = 5, 1000
    h = dict(r=np.full((T, N), c, np.float32), v=np.zeros((T + 1, N), np.float32), nv=None, te=None,
             tr=np.ones((T, N), np.uint8))
    a_gpu, adv, stats, _, _ = _check_gae(h, T, N, what="constant")
    assert np.all(a_gpu == np.float32(c))
    s = _np(stats)
    assert _normalise(adv, T * N, 1, stats) == 0
    x = _np(adv)
    emu = adv_norm_f32(a_gpu, s)
    # std is 0 or rounding noise, below the 1e-4 clamp: (a - mean) * 1e4 with the float32 mean
    m = np.float32(s[0, 0] / s[0, 2])
    want = ((np.float32(c) - m) * np.float32(1e4)).astype(np.float32)
    assert np.array_equal(_bits(x), _bits(emu)) and np.all(x == want) and abs(want) <= abs(c) * 2 * U32 * 1e4


def test_normalise_zero_statistics_take_the_count_guard():
    n = 1000
    a = np.random.default_rng(5).normal(size=(1, n)).astype(np.float32)
    for G in (1, 8):
        adv = _dev(a)
        stats = torch.zeros((G, 3), dtype=torch.float64, device="cuda")
        assert _normalise(adv, n, G, stats) == 0
        x = _np(adv)
        assert np.isfinite(x).all()
        assert np.array_equal(_bits(x), _bits(adv_norm_f32(a, np.zeros((G, 3)), G)))
        assert np.array_equal(x, (a * np.float32(1e4)).astype(np.float32))


def test_normalise_refusals():
    adv = torch.full((70,), SENTINEL, device="cuda")
    stats = torch.zeros((64, 3), dtype=torch.float64, device="cuda")
    L = abi.lib()
    for n, G, a, s in ((70, 0, adv, stats), (70, 65, adv, stats), (70, 4, adv, stats), (-70, 1, adv, stats),
                       (70, 1, None, stats), (70, 1, adv, None)):
        assert L.msc_adv_normalize_grouped(_p(a), n, G, _p(s), None) != 0
    assert np.all(_np(adv) == SENTINEL)


# ---- keyed normals ------------------------------------------------------------------------------

def _keyed(n_steps, n_rows, row_len, row0, seed, step0, pad=0):
    out = torch.full((n_steps * n_rows * row_len + pad,), SENTINEL, device="cuda")
    rc = abi.lib().msc_normal_keyed(_p(out), n_steps, n_rows, row_len, row0, seed, step0, None)
    return rc, out


@pytest.mark.parametrize("case", [
    (2, 3, 5, 0, 0, 0),  # odd row_len: the last pair writes one element
    (1, 1, 1, 7, 1, 9),
    (3, 70, 40, 2 ** 32 - 35, 0xDEADBEEF12345678, 2 ** 32 - 1),  # rows cross 2^32, the step word wraps
    (3, 350000, 8, 0, 5, 0),  # 4.2 M pairs > 16384 * 256: the second grid-stride pass
], ids=["odd", "single", "hi-words", "grid-stride"])
def test_normal_keyed_vs_numpy_philox(case):
    """|gpu - ref| <= 6 * 2^-23 * rad: <= 2 ulp of logf halved by the square root, 1 ulp sqrtf, 2 ulp
    sincosf, 1/2 ulp for the product, rounded up (HIP's documented device-function limits)."""
    n_steps, n_rows, row_len = case[:3]
    rc, out = _keyed(*case, pad=3)
    assert rc == 0
    g = _np(out)
    assert np.all(g[-3:] == SENTINEL)  # the odd tail writes nothing past the buffer
    g = g[:-3].reshape(n_steps, n_rows, row_len).astype(np.float64)
    ref, rad = normal_keyed_ref(*case)
    err, bound = np.abs(g - ref), 6 * 2.0 ** -23 * rad
    print(f"normal_keyed {case}: max err/(6 eps rad) {np.max(err[rad > 0] / bound[rad > 0]):.3f}, "
          f"mean {g.mean():.2e} var {g.var():.5f}")
    assert np.all(err <= bound)


def test_normal_keyed_slices_equal_shifted_calls():
    rc, big = _keyed(5, 300, 7, 2 ** 32 - 100, 42, 2 ** 32 - 2)
    assert rc == 0
    big = _np(big).reshape(5, 300, 7)
    for s0, s1, r0, r1 in ((0, 5, 0, 300), (1, 4, 90, 130), (3, 5, 299, 300), (2, 3, 0, 1)):
        rc, part = _keyed(s1 - s0, r1 - r0, 7, 2 ** 32 - 100 + r0, 42, 2 ** 32 - 2 + s0)
        assert rc == 0
        assert np.array_equal(_bits(_np(part).reshape(s1 - s0, r1 - r0, 7)), _bits(big[s0:s1, r0:r1]))
    # the step word is (step0 + s) mod 2^32
    rc, wrapped = _keyed(2, 300, 7, 2 ** 32 - 100, 42, 1)
    assert rc == 0 and np.array_equal(_bits(_np(wrapped).reshape(2, 300, 7)), _bits(big[3:5]))


def test_normal_keyed_refusals_and_empty_calls():
    L = abi.lib()
    out = torch.full((64,), SENTINEL, device="cuda")
    for args in ((None, 1, 1, 4, 0), (out, -1, 1, 4, 0), (out, 1, -1, 4, 0), (out, 1, 1, 0, 0), (out, 1, 1, -3, 0),
                 (out, 1, 1, 4, -1)):
        assert L.msc_normal_keyed(_p(args[0]), *args[1:], 1, 0, None) != 0
    for args in ((out, 0, 5, 4, 0), (out, 5, 0, 4, 0)):  # nothing to draw: accepted, nothing written
        assert L.msc_normal_keyed(_p(args[0]), *args[1:], 1, 0, None) == 0
    assert np.all(_np(out) == SENTINEL)


# ---- Gaussian action sampling -------------------------------------------------------------------

def _sample(mean, log_std, floor, eps):
    N, K = mean.shape
    act, clip = torch.empty((N, K), device="cuda"), torch.empty((N, K), device="cuda")
    logp = torch.empty((N,), device="cuda")
    m, ls, e = _dev(mean), _dev(log_std), _dev(eps)  # kept alive over the call
    abi.check(abi.lib().msc_gaussian_sample(_p(m), _p(ls), log_std.shape[0], C.c_float(floor), _p(e), N, K, _p(act),
                                            _p(logp), _p(clip), None))
    return _np(act), _np(logp), _np(clip)


@pytest.mark.parametrize("rows, floor", [(1, -20.0), (1, 1.5), (3, -20.0), (3, -0.25)],
                         ids=["shared", "shared-floor-binds", "per-agent", "per-agent-floor-mixed"])
@pytest.mark.parametrize("K", [1, 5, 9])
@pytest.mark.parametrize("N", [1, 255, 257])
def test_gaussian_sample_vs_f64(N, K, rows, floor):
    f = np.float32
    if N % rows:
        N = N // rows * rows + rows  # whole groups of agents: 3, 255, 258
    rng = np.random.default_rng([N, K, rows])
    mean = rng.normal(size=(N, K)).astype(f)
    eps = rng.normal(size=(N, K)).astype(f)
    log_std = rng.uniform(-1.0, 1.0, size=(rows, K)).astype(f)
    ls = np.maximum(log_std, f(floor))  # exact
    if floor == 1.5:
        assert np.all(ls == f(floor))  # the floor binds on every entry
    # the device's own std = expf(ls): a zero-mean, unit-eps call returns it as the action
    sd, lp0, _ = _sample(np.zeros((N, K), f), log_std, floor, np.ones((N, K), f))
    sd_ref = np.exp(np.tile(ls, (N // rows, 1)).astype(np.float64))
    assert np.all(np.abs(sd - sd_ref) <= 2.0 ** -23 * sd_ref)  # expf: 1 ulp (HIP's documented limit)
    act, logp, clip = _sample(mean, log_std, floor, eps)
    want = (mean + (sd * eps).astype(f)).astype(f)
    assert np.array_equal(_bits(act), _bits(want))
    assert np.array_equal(_bits(clip), _bits(np.clip(act, f(-1), f(1))))
    # log-density in float64 on the device's actions and std; every float32 operation of the kernel
    # rounds a quantity no larger than |quad| + |log_std| + |log sqrt(2 pi)| of its term
    d = act.astype(np.float64) - mean
    s64 = sd.astype(np.float64)
    lsr = np.tile(ls, (N // rows, 1)).astype(np.float64)
    quad = d * d / (2.0 * s64 * s64)
    half_log_2pi = float(f(0.91893853320467274178))
    ref = (-quad - lsr - half_log_2pi).sum(axis=1)
    bound = 8 * U32 * (quad + np.abs(lsr) + half_log_2pi).sum(axis=1)
    err = np.abs(logp - ref)
    print(f"gaussian_sample N={N} K={K} rows={rows} floor={floor}: max logp err/bound {np.max(err / bound):.3f}")
    assert np.all(err <= bound)
    # zero-mean unit-eps call: quad = 1/2 up to the rounding of sd * sd
    assert np.all(np.abs(lp0 - (-0.5 - lsr - half_log_2pi).sum(axis=1)) <= 8 * U32 * (0.5 + np.abs(lsr) + half_log_2pi).sum(axis=1))


def test_gaussian_sample_refusals():
    L = abi.lib()
    t = torch.zeros((8,), device="cuda")
    ok = [_p(t), _p(t), 1, C.c_float(-20.0), _p(t), 2, 4, _p(t), _p(t), _p(t), None]
    for i, bad in ((0, None), (1, None), (4, None), (7, None), (8, None), (9, None), (2, 0), (5, -1), (6, 0)):
        args = list(ok)
        args[i] = bad
        assert L.msc_gaussian_sample(*args) != 0
