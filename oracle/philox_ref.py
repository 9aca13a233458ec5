"""TEST INFRASTRUCTURE ONLY: numpy Philox4x32-10 (Salmon et al., Random123) and the rollout's keyed
standard normals (include/marlsc.h, msc_normal_keyed) built on it.

All words are carried in uint64 arrays and masked to 32 bits, so the 32 x 32 -> 64 bit products are
exact."""
import numpy as np

M0, M1 = np.uint64(0xD2511F53), np.uint64(0xCD9E8D57)
W0, W1 = np.uint64(0x9E3779B9), np.uint64(0xBB67AE85)
MASK = np.uint64(0xFFFFFFFF)
S32 = np.uint64(32)


def philox4x32_10(counter, key):
    """counter: 4 uint64 arrays (or ints) of 32-bit words, key: 2; returns the 4 output words."""
    c = [np.asarray(x, np.uint64) & MASK for x in counter]
    k0, k1 = (np.asarray(x, np.uint64) & MASK for x in key)
    for _ in range(10):
        p0, p1 = M0 * c[0], M1 * c[2]
        c = [(p1 >> S32) ^ c[1] ^ k0, p1 & MASK, (p0 >> S32) ^ c[3] ^ k1, p0 & MASK]
        k0, k1 = (k0 + W0) & MASK, (k1 + W1) & MASK
    return c


def normal_keyed_ref(n_steps, n_rows, row_len, row0, seed, step0):
    """out [n_steps, n_rows, row_len] float64 and rad (same shape): element (s, row, j) from
    counter {j // 2, lo32(row0 + row), hi32(row0 + row), lo32(step0 + s)} and key {lo32(seed),
    hi32(seed)}; output words 0 and 1 give the uniforms, formed in float32 exactly as the kernel
    forms them; Box-Muller's log / sqrt / cos / sin in float64 (cos: even j, sin: odd j)."""
    f = np.float32
    pairs = (row_len + 1) // 2
    jp = np.arange(pairs, dtype=np.uint64)[None, None, :]
    g = (np.uint64(row0) + np.arange(n_rows, dtype=np.uint64))[None, :, None]
    st = ((np.uint64(step0 & 0xFFFFFFFFFFFFFFFF) + np.arange(n_steps, dtype=np.uint64)) & MASK)[:, None, None]
    shape = (n_steps, n_rows, pairs)
    ctr = [np.broadcast_to(x, shape) for x in (jp, g & MASK, g >> S32, st)]
    seed = int(seed) & 0xFFFFFFFFFFFFFFFF
    c = philox4x32_10(ctr, (seed & 0xFFFFFFFF, seed >> 32))
    two_m32 = f(2.0 ** -32)
    u1 = ((c[0].astype(f) + f(0.5)).astype(f) * two_m32).astype(f)
    u2 = (c[1].astype(f) * two_m32).astype(f)
    theta = (f(6.283185307179586) * u2).astype(f).astype(np.float64)
    rad = np.sqrt(-2.0 * np.log(u1.astype(np.float64)))
    out = np.empty((n_steps, n_rows, 2 * pairs))
    out[..., 0::2] = rad * np.cos(theta)
    out[..., 1::2] = rad * np.sin(theta)
    return out[..., :row_len], np.repeat(rad, 2, axis=-1)[..., :row_len]
