"""TEST INFRASTRUCTURE ONLY: numpy restatement of the advantage estimation the rollout uses.

The reference delegates GAE to RLlib 2.52.1 (not vendored, not installed: parity unpinned
against RLlib itself). This restates the textbook GAE(gamma, lambda) with RLlib's conventions:
terminated -> bootstrap 0, truncated -> bootstrap V(terminal obs), value targets = A + V,
then (A - mean) / max(1e-4, std) over each module's batch: the whole batch for one shared policy,
every agent's column (sequence n % W) on its own for one policy per agent."""
from math import fsum

import numpy as np


def gae(rewards, values, next_values, terminated, truncated, gamma, lam):
    """rewards/terminated/truncated/next_values: [T, N]; values: [T+1, N]. float64 math."""
    T, N = rewards.shape
    adv = np.zeros((T, N), np.float64)
    a = np.zeros(N, np.float64)
    v_next = values[T].astype(np.float64)
    for t in range(T - 1, -1, -1):
        te = terminated[t].astype(bool)
        tr = truncated[t].astype(bool)
        boot = np.where(tr, next_values[t], v_next)
        boot = np.where(te, 0.0, boot)
        delta = rewards[t] + gamma * boot - values[t]
        a = delta + np.where(te | tr, 0.0, gamma * lam * a)
        adv[t] = a
        v_next = values[t].astype(np.float64)
    return adv, adv + values[:T]


U32 = 2.0 ** -24  # unit roundoff of float32


def _flags(te, tr, shape):
    z = np.zeros(shape, bool)
    return (z if te is None else np.asarray(te).astype(bool)), (z if tr is None else np.asarray(tr).astype(bool))


def gae_f32(r, v, nv, te, tr, gamma, lam):
    """The kernels' recurrence (csrc/gae.hip, built with -ffp-contract=off) operation by operation
    in np.float32; returns float32 (adv, targets). nv / te / tr may be None (NULL pointers)."""
    f = np.float32
    r, v = np.asarray(r, f), np.asarray(v, f)
    T, N = r.shape
    te, tr = _flags(te, tr, (T, N))
    g, l = f(gamma), f(lam)
    gl = f(g * l)
    zero = np.zeros(N, f)
    adv, tgt = np.empty((T, N), f), np.empty((T, N), f)
    a, v_next = zero, v[T]
    for t in range(T - 1, -1, -1):
        cut = te[t] | tr[t]
        boot = np.where(tr[t], zero if nv is None else np.asarray(nv[t], f), v_next)
        boot = np.where(te[t], zero, boot)
        delta = ((r[t] + (g * boot).astype(f)).astype(f) - v[t]).astype(f)
        a = (delta + np.where(cut, zero, (gl * a).astype(f))).astype(f)
        adv[t] = a
        tgt[t] = a + v[t]
        v_next = v[t]
    return adv, tgt


def gae_bounded(r, v, nv, te, tr, gamma, lam):
    """The same recurrence in float64 with the float32-rounded gamma, lam and gamma * lam, and a
    first-order forward error bound of the float32 recurrence (one term per rounding, inputs exact):
      B_t = u (|g boot| + |r + g boot| + |delta| + |q| + |A_t|) + (0 if cut else gl B_{t+1}),
    q = 0 if cut else gl A_{t+1}, u = 2^-24. Returns (A, targets, B)."""
    f = np.float32
    r, v = np.asarray(r, f).astype(np.float64), np.asarray(v, f).astype(np.float64)
    T, N = r.shape
    te, tr = _flags(te, tr, (T, N))
    g, l = f(gamma), f(lam)
    gl = float(f(g * l))
    g = float(g)
    A, B = np.empty((T, N)), np.empty((T, N))
    a, b, v_next = np.zeros(N), np.zeros(N), v[T]
    for t in range(T - 1, -1, -1):
        cut = te[t] | tr[t]
        boot = np.where(tr[t], 0.0 if nv is None else np.asarray(nv[t], f).astype(np.float64), v_next)
        boot = np.where(te[t], 0.0, boot)
        gb = g * boot
        delta = r[t] + gb - v[t]
        q = np.where(cut, 0.0, gl * a)
        a = delta + q
        b = U32 * (np.abs(gb) + np.abs(r[t] + gb) + np.abs(delta) + np.abs(q) + np.abs(a)) + np.where(cut, 0.0, gl * b)
        A[t], B[t] = a, b
        v_next = v[t]
    return A, A + v[:T], B


def target_bound(B, targets):
    """Bound of the float32 targets: the advantage's plus the rounding of a + v."""
    return B + U32 * np.abs(targets)


def normalize_bounded(A, B, groups=1):
    """float64 standardisation of A [T, N] per group (sequence n in group n % groups) and the bound
    of the float32 kernel's result on advantages that are within B of A:
      tol = (B + 2u (|A| + |m|) + mean_g(B) + |x| rms_g(B)) / max(1e-4, s) + 4u |x|
    (mean_g(B): the mean moves by at most that; rms_g(B): so does the std, by the reverse triangle
    inequality in L2; the rest: float32 casts of mean and 1 / std, the subtract, the multiply)."""
    A, B = np.asarray(A, np.float64), np.asarray(B, np.float64)
    x, tol = np.empty_like(A), np.empty_like(A)
    for k in range(groups):
        a, b = A[:, k::groups], B[:, k::groups]
        m, s = a.mean(), a.std()
        sc = max(1e-4, s)
        xg = (a - m) / sc
        x[:, k::groups] = xg
        tol[:, k::groups] = ((b + 2 * U32 * (np.abs(a) + abs(m)) + b.mean() + np.abs(xg) * np.sqrt((b * b).mean())) / sc
                             + 4 * U32 * np.abs(xg))
    return x, tol


def stats_of(a32, groups=1):
    """[groups, 3] float64 {sum A, sum A^2, count} of float32 advantages [T, N], as the kernels define it."""
    a = np.asarray(a32, np.float32).astype(np.float64)
    return np.array([[a[:, k::groups].sum(), (a[:, k::groups] ** 2).sum(), a[:, k::groups].size]
                     for k in range(groups)])


def stats_bounded(a32, groups, d):
    """Exactly rounded {sum A, sum A^2, count} per group of float32 advantages [T, N] (math.fsum; the
    squares of float32 values are exact in float64) and the bound d 2^-53 sum |x| of a float64
    summation whose longest chain has d adds. Returns (ref [groups, 3], tol [groups, 2])."""
    a = np.asarray(a32, np.float32).astype(np.float64)
    ref, tol = np.empty((groups, 3)), np.empty((groups, 2))
    for k in range(groups):
        x = a[:, k::groups].ravel()
        ref[k] = fsum(x), fsum(x * x), x.size
        tol[k] = d * 2.0 ** -53 * fsum(np.abs(x)), d * 2.0 ** -53 * ref[k, 1]
    return ref, tol


def gae_blocks(N, vectorised):
    """Thread blocks of the GAE launch: 256 lanes of 4 sequences (vectorised) or of 1."""
    return -(-(N // 4 if vectorised else N) // 256)


def adv_norm_f32(a32, stats, groups=1):
    """adv_norm_kernel operation by operation: float64 mean / std from the statistics table, both cast
    to float32, then (a - mean) * (1 / std) in float32."""
    f = np.float32
    a32 = np.asarray(a32, f)
    st = np.asarray(stats, np.float64).reshape(groups, 3)
    out = np.empty_like(a32)
    for k in range(groups):
        cnt = st[k, 2] if st[k, 2] > 0 else 1.0
        mean = st[k, 0] / cnt
        var = max(st[k, 1] / cnt - mean * mean, 0.0)
        sd = max(np.sqrt(var), 1e-4)
        out[:, k::groups] = ((a32[:, k::groups] - f(mean)).astype(f) * f(1.0 / sd)).astype(f)
    return out


def normalize(adv):
    return (adv - adv.mean()) / max(1e-4, adv.std())


def normalize_grouped(adv, groups):
    """adv [T, N]; sequence n standardised with the statistics of group n % groups."""
    out = np.empty_like(adv, dtype=np.float64)
    for g in range(groups):
        out[:, g::groups] = normalize(adv[:, g::groups])
    return out
