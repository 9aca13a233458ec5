"""The arithmetic of msc_adam_clip_step (include/marlsc.h, csrc/adam_clip.hip) restated in numpy, operation by
operation. A helper, not a test: tests/test_adam_host.py and tests/test_gpu_adam_exact.py use it.

Per group the norm is float64 (math.fsum of the float64 squares: exact where the sum is exactly
representable, which is what the exact GPU tests arrange, and correctly rounded otherwise); the clip
coefficient is formed in float64 and rounded once to float32; every elementwise operation is a float32
operation with one rounding (numpy float32 arrays: no wider intermediate, nothing contracted; numpy's
float32 sqrt and / are correctly rounded)."""
import math

import numpy as np

F = np.float32


def scalars(lr, beta1, beta2, eps, step):
    """(b2, 1 - b1, 1 - b2, eps, step_size, sqrt(1 - b2^step)) formed in float64, each rounded once to float32"""
    bc1 = 1.0 - beta1 ** step
    bc2 = 1.0 - beta2 ** step
    return F(beta2), F(1.0 - beta1), F(1.0 - beta2), F(eps), F(lr / bc1), F(math.sqrt(bc2))


def group_norms(tensors, n_groups):
    """float64 norm of every group over its tensors' gradients; tensors: dicts with 'g' and 'group'"""
    sq = [[] for _ in range(n_groups)]
    for t in tensors:
        g = np.asarray(t["g"], dtype=np.float32).astype(np.float64).ravel()
        sq[t["group"]].extend((g * g).tolist())
    return np.array([math.sqrt(math.fsum(s)) for s in sq], dtype=np.float64)


def clip_coef(norm, max_norm):
    """c = (float)min(1, max_norm / (norm + 1e-6)); exactly 1 with the clip off"""
    if not max_norm > 0:
        return F(1.0)
    return F(min(1.0, float(max_norm) / (float(norm) + 1e-6)))


def step(tensors, n_groups, *, lr, beta1=0.9, beta2=0.999, eps=1e-8, max_norm=0.0, step=1):
    """One call: returns (new tensors [{'p', 'g' (clipped), 'm', 'v', 'group'}], norms f64[n_groups]).
    The inputs are left as they are."""
    b2, a1, a2, e, step_size, r2 = scalars(lr, beta1, beta2, eps, step)
    norms = group_norms(tensors, n_groups)
    out = []
    for t in tensors:
        c = clip_coef(norms[t["group"]], max_norm)
        p, g, m, v = (np.asarray(t[k], dtype=np.float32) for k in ("p", "g", "m", "v"))
        g1 = g * c
        m1 = m + a1 * (g1 - m)
        v1 = b2 * v + (a2 * g1) * g1
        denom = np.sqrt(v1) / r2 + e
        p1 = p - step_size * (m1 / denom)
        assert all(x.dtype == np.float32 for x in (g1, m1, v1, denom, p1))
        out.append({"p": p1, "g": g1, "m": m1, "v": v1, "group": t["group"]})
    return out, norms
