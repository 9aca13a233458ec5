"""TEST INFRASTRUCTURE ONLY: numpy float64 emulation of the three kernels of csrc/obs_filter.hip
(of_segment_kernel, of_apply_kernel, of_commit_kernel behind msc_meanstd_filter) as written, and the
cases that tests/test_meanstd_exact_host.py and tests/test_gpu_meanstd_exact.py share.

The library is built with -ffp-contract=off and float64 + - * / and sqrt are correctly rounded on
the host and on the device, so a restatement with the kernels' plan and operation order has to equal
the device bit for bit, in `out` and in `state`. The emulation runs every thread (segment p, column c)
of a kernel at once: arrays [P, C], one loop over the G rows of a segment and one over the P merges.

`mut` selects one deliberate mistake (MUTANTS); the host tests show that each one is seen."""
import numpy as np

OF_MAX_SEG = 64
CLIP, EPS = 10.0, 1e-6

MUTANTS = ("merge_le", "segment_ignores_mask", "apply_ignores_mask", "normalise_first", "var_over_n",
           "single_push_var_zero", "buffer_skips_segment", "neighbour_fin", "plan_g_plus_1", "race")


def meanstd_plan(E):
    """(G rows per segment, P segments): meanstd_plan of csrc/obs_filter.hip."""
    p = min(int(E), OF_MAX_SEG)
    G = (E + p - 1) // p
    return G, (E + G - 1) // G


def scratch_doubles(E, C):
    """msc_meanstd_scratch_doubles: seg [P][C][3], fin [C][3], the buffer count before the call."""
    return meanstd_plan(E)[1] * C * 3 + C * 3 + 1


def new_state(C, n=0.0, M=None, S=None):
    """{n, buffer n, 0, 0, M[C], S[C], buffer M[C], buffer S[C]}."""
    st = np.zeros(4 + 4 * C)
    st[0] = n
    if M is not None:
        st[4:4 + C] = M
    if S is not None:
        st[4 + C:4 + 2 * C] = S
    return st


def _push(n, m, s, x, act):
    """rs_push where `act`; n [P, 1] (or broadcastable), m / s / x [P, C]."""
    n1 = n + 1.0
    delta = x - m
    m2 = np.where(n1 == 1.0, x, m + delta / n1)
    s2 = np.where(n1 == 1.0, s, s + delta * delta * (n1 - 1.0) / n1)
    return np.where(act, n1, n), np.where(act, m2, m), np.where(act, s2, s)


def _merge(n1, m1, s1, n2, m2, s2):
    """rs_merge: a <- a (+) b, in its operation order."""
    n = n1 + n2
    delta = m1 - m2
    delta2 = delta * delta
    m = (n1 * m1 + n2 * m2) / n
    s = s1 + s2 + (delta2 / n) * n1 * n2
    return n, np.where(n == 0.0, m1, m), np.where(n == 0.0, s1, s)


def _norm(x, n, m, s, clip, eps, mut):
    d = n if mut == "var_over_n" else n - 1.0
    var = np.where(n > 1.0, s / d, 0.0 if mut == "single_push_var_zero" else m * m)
    y = (x - m) / (np.sqrt(var) + eps)
    if clip > 0.0:
        y = np.where(y < -clip, -clip, np.where(y > clip, clip, y))
    return y.astype(np.float32)


def emulate(state, x, mask=None, update=True, clip=CLIP, eps=EPS, mut=None, skip_empty=True):
    """One msc_meanstd_filter call: (out float32 [E, C], the state after it). `state` is not modified.
    skip_empty=False merges segments without a push too, as the kernels did before they skipped them."""
    assert mut is None or mut in MUTANTS
    E, C = x.shape
    st = np.array(state, np.float64)
    run_m, run_s = st[4:4 + C].copy(), st[4 + C:4 + 2 * C].copy()
    buf_m, buf_s = st[4 + 2 * C:4 + 3 * C].copy(), st[4 + 3 * C:].copy()
    G, P = meanstd_plan(E)
    if mut == "plan_g_plus_1":
        G = G + 1
        P = (E + G - 1) // G
    rows = np.arange(P * G)
    live = (rows < E).reshape(P, G)
    pushed = np.ones(E, bool) if mask is None else np.asarray(mask).reshape(E) != 0
    pushed = np.concatenate([pushed, np.zeros(P * G - E, bool)]).reshape(P, G)
    xp = np.concatenate([x.astype(np.float64), np.zeros((P * G - E, C))]).reshape(P, G, C)
    out = np.empty((P, G, C), np.float32)
    with np.errstate(all="ignore"):
        # of_segment_kernel: thread (p, c), the RunningStat of its rows from zero
        sn, sm, ss = np.zeros((P, 1)), np.zeros((P, C)), np.zeros((P, C))
        if update:
            act = live if mut == "segment_ignores_mask" else pushed
            for g in range(G):
                sn, sm, ss = _push(sn, sm, ss, xp[:, g], act[:, g, None])
        # of_apply_kernel: the running state merged with segments 0 .. p-1, in that order
        pn, pm, ps = np.empty((P, 1)), np.empty((P, C)), np.empty((P, C))
        n, m, s = st[0], run_m, run_s
        for p in range(P):
            if mut != "merge_le":
                pn[p], pm[p], ps[p] = n, m, s
            if update and (sn[p, 0] != 0.0 or not skip_empty):
                n, m, s = _merge(n, m, s, sn[p, 0], sm[p], ss[p])
            if mut == "merge_le":
                pn[p], pm[p], ps[p] = n, m, s
        # ... then its own rows pushed and normalised one by one
        act = (live if mut == "apply_ignores_mask" else pushed) if update else np.zeros((P, G), bool)
        n, m, s = pn, pm, ps
        for g in range(G):
            if mut == "normalise_first":
                out[:, g] = _norm(xp[:, g], n, m, s, clip, eps, mut)
            n, m, s = _push(n, m, s, xp[:, g], act[:, g, None])
            if mut != "normalise_first":
                out[:, g] = _norm(xp[:, g], n, m, s, clip, eps, mut)
        out = out.reshape(P * G, C)[:E]
        if not update:
            return out, st
        # of_commit_kernel: thread c; the buffer absorbs segments 0 .. P-1
        bn, bm, bs = st[1], buf_m, buf_s
        if mut == "race":  # columns of later waves read the count that thread 0 has already written
            bn = np.where(np.arange(C) >= 64, st[1] + sn.sum(), st[1])
        for q in range(P):
            if mut == "buffer_skips_segment" and q == P // 2:
                continue
            if sn[q, 0] != 0.0 or not skip_empty:
                bn, bm, bs = _merge(bn, bm, bs, sn[q, 0], sm[q], ss[q])
        fm, fs = m[P - 1], s[P - 1]
        if mut == "neighbour_fin":
            fm, fs = np.roll(fm, -1), np.roll(fs, -1)
    st[0], st[1] = n[P - 1, 0], np.ravel(bn)[0]
    st[4:4 + C], st[4 + C:4 + 2 * C], st[4 + 2 * C:4 + 3 * C], st[4 + 3 * C:] = fm, fs, bm, bs
    return out, st


def merge_packed(a, b):
    """marlsc.obs_filter.merge_stats on packed float64 [1 + 2C] rows (n, M[C], S[C])."""
    C = (len(a) - 1) // 2
    if a[0] + b[0] == 0:
        return a.copy()
    n, m, s = _merge(a[0], a[1:1 + C], a[1 + C:], b[0], b[1:1 + C], b[1 + C:])
    return np.concatenate([[n], m, s])


def lane_buffer(st):
    C = (len(st) - 4) // 4
    return np.concatenate([st[1:2], st[4 + 2 * C:]])


def lane_from_driver(driver):
    C = (len(driver) - 1) // 2
    st = np.zeros(4 + 4 * C)
    st[0] = driver[0]
    st[4:4 + 2 * C] = driver[1:]
    return st


def bits(a):
    """The bit patterns of a float32 / float64 array."""
    a = np.ascontiguousarray(a)
    return a.view(np.uint32 if a.dtype == np.float32 else np.uint64)


def nan_bits(a):
    """bits() with every NaN replaced by one quiet NaN: IEEE 754 leaves the sign and payload of a
    generated NaN open (x86 produces the negative quiet NaN for inf - inf, gfx950 the positive one), so
    NaNs are compared by position."""
    a = np.array(a)
    a[np.isnan(a)] = np.nan
    return bits(a)


# ---- the shared cases -------------------------------------------------------------------------------------

ROW_CASES = [(E, 70) for E in (1, 2, 63, 64, 65, 127, 128, 129, 4096, 4097)]
COL_CASES = [(E, C) for C in (1, 63, 64, 65, 255, 256, 257, 272, 1000) for E in (37, 130)]


def case_steps(E, C, shift=2.0, steps=3, seed=None):
    """Three calls of f32(N(shift, 1) * scale_c), scale_c in [0.1, 50]; the second is masked to about
    half of its rows with mask[0] = 0 (a masked first row), so the second and third calls start from
    a non-zero state. -> [(x [E, C] float32, mask or None)]"""
    rng = np.random.default_rng(1000003 * E + C if seed is None else seed)
    scale = rng.uniform(0.1, 50.0, C)
    out = []
    for k in range(steps):
        x = (rng.normal(shift, 1.0, (E, C)) * scale).astype(np.float32)
        mask = None
        if k == 1:
            mask = (rng.uniform(size=E) < 0.5).astype(np.uint8)
            mask[0] = 0
        out.append((x, mask))
    return out


def long_run_case(C=70, E=130):
    """A state after 2^30 pushes of N(mu_c, sigma_c) (M = mu_c, S = (n - 1) sigma_c^2 to rounding) and
    130 more rows of the same distribution."""
    rng = np.random.default_rng(30)
    n = float(2 ** 30)
    mu, sigma = rng.normal(2.0, 5.0, C), rng.uniform(0.1, 50.0, C)
    st = new_state(C, n, mu, (n - 1.0) * sigma * sigma)
    x = (mu + sigma * rng.normal(0.0, 1.0, (E, C))).astype(np.float32)
    return st, x
