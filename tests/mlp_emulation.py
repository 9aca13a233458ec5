"""Host emulation of the fused policy MLP's data flow (csrc/mlp_kernels.hpp) over the packed weight
fragments of marlsc/mlp.py:pack_mlp3, lane by lane, for one wave of 32 rows in float64.

MFMA operand maps (v_mfma_f32_32x32x2_f32): lane l holds A[l & 31][k = l >> 5] and
B[k = l >> 5][l & 31]; accumulator register r of lane l is D[(r & 3) + 8 (r >> 2) + 4 (l >> 5)][l & 31].
Shared by tests/test_mlp_host.py (random real weights against torch) and tests/test_mlp_exact_host.py
(integer weights against the int64 reference, and the mutants that must not survive it)."""
import numpy as np

LANE = np.arange(64)
COL, HALF = LANE & 31, LANE >> 5


def mfma(a_lane, b_lane, d):
    """D += A B with A [32 x 2] and B [2 x 32] given per lane."""
    return d + a_lane.reshape(2, 32).T @ b_lane.reshape(2, 32)


def rho(r, h):
    return (r & 3) + 8 * (r >> 2) + 4 * h


def regs(tile, r):
    """Register r of every lane of a [32 rows x 32 samples] accumulator tile."""
    return tile[rho(r, HALF), COL]


def emulate_packed(x, L, H1, H2, KO, w1p, w2p, w3p, b1, b2, b3, layout, pre1_rows=None, guard_x=True):
    """Outputs [32, KO] of rows 0..31 of x ([>= 32, L], read as the kernel does: a flat buffer).
    H2 = 0: the one-hidden-layer kernel (w2p / b2 unused). layout: 0 = MFMA output layer fragments,
    1 = VALU rows. pre1_rows [32, H1]: the pre1 row each sample adds to its first layer (the kernel's
    pre1[n // group]). guard_x=False: the kernel's `k < L` guard on the x load removed, so the slot past
    in_dim of an odd L reads the next row's first feature."""
    KS1 = (L + 1) // 2
    M4 = (KS1 + 3) // 4
    xf = np.asarray(x, np.float64).reshape(-1)
    assert xf.size >= 32 * L
    w1p = np.asarray(w1p, np.float64).reshape(H1 // 32, M4, 64, 4)
    b1, b3 = np.asarray(b1, np.float64), np.asarray(b3, np.float64)
    h1 = []
    for t in range(H1 // 32):
        d = np.zeros((32, 32))
        for m in range(M4 * 4):
            k = HALF * KS1 + m
            ok = (k < L) if guard_x else np.ones(64, bool)
            ok = ok & (m < KS1)
            xb = np.where(ok, xf[np.minimum(COL * L + k, xf.size - 1)], 0.0)
            d = mfma(w1p[t, m // 4, :, m % 4], xb, d)
        d = d + b1[t * 32:(t + 1) * 32, None]
        if pre1_rows is not None:
            d = d + np.asarray(pre1_rows, np.float64)[:, t * 32:(t + 1) * 32].T
        h1.append(np.maximum(d, 0))
    hl, HL = h1, H1
    if H2:
        w2p = np.asarray(w2p, np.float64).reshape(H2 // 32, H1 // 8, 64, 4)
        b2 = np.asarray(b2, np.float64)
        hl, HL = [], H2
        for t2 in range(H2 // 32):
            d = np.zeros((32, 32))
            for s in range((H1 // 32) * 16):
                d = mfma(w2p[t2, s // 4, :, s % 4], regs(h1[s // 16], s % 16), d)
            hl.append(np.maximum(d + b2[t2 * 32:(t2 + 1) * 32, None], 0))
    w3p = np.asarray(w3p, np.float64)
    if layout == 1:  # VALU output layer: lane half h sums its rows rho(r, h) of every tile
        w3v = w3p.reshape((HL // 32) * 16, 2, 8)
        o = np.zeros((64, 8))
        for s in range((HL // 32) * 16):
            o += w3v[s, HALF] * regs(hl[s // 16], s % 16)[:, None]
        return o[:32, :KO] + o[32:, :KO] + b3[None, :]
    w3p = w3p.reshape(HL // 8, 64, 4)
    d = np.zeros((32, 32))
    for q in range((HL // 32) * 4):
        for i in range(4):
            d = mfma(w3p[q, :, i], regs(hl[q // 4], (q % 4) * 4 + i), d)
    return (d[:KO] + b3[:, None]).T


# ---- choosing mutants that must matter ----------------------------------------------------------------

def live_units(case):
    """Per layer, the units a change of whose pre-activation must reach an output: positive on at least
    a quarter of the rows (taken from the int64 reference) and wired by a non-zero weight to a live
    unit of the next layer (to any output for the last hidden layer)."""
    h, acts = case["x"].astype(np.int64), []
    for i, (w, b) in enumerate(zip(case["W"][:-1], case["b"][:-1])):
        z = h @ w.astype(np.int64).T + b.astype(np.int64)
        if i == 0 and case["pre1"] is not None:
            z = z + case["pre1"].astype(np.int64)[np.arange(len(z)) // case["group"]]
        acts.append((z > 0).sum(axis=0) >= len(z) // 4)
        h = np.maximum(z, 0)
    live = [None] * len(acts)
    nxt = np.ones(case["W"][-1].shape[0], bool)
    for i in range(len(acts) - 1, -1, -1):
        live[i] = acts[i] & (case["W"][i + 1][nxt] != 0).any(axis=0)
        nxt = live[i]
    return live, acts


def swap_packed(packed_w, index, valid, W, unit, inputs_ok):
    """The packed array with two entries of row `unit` of W exchanged: non-zero, different, and
    (inputs_ok) multiplying inputs that are live themselves. Located through the packing's index map."""
    row = W[unit]
    ks = [k for k in range(W.shape[1]) if row[k] != 0 and inputs_ok[k]]
    ka = ks[0]
    kb = next(k for k in ks if row[k] != row[ka])
    pos = []
    for k in (ka, kb):
        hit = np.flatnonzero((index == unit * W.shape[1] + k) & valid)
        assert hit.size == 1  # every weight sits in exactly one packed slot
        pos.append(hit[0])
    out = packed_w.copy().reshape(-1)
    out[pos[0]], out[pos[1]] = out[pos[1]], out[pos[0]]
    assert not np.array_equal(out, packed_w.reshape(-1))
    return out
