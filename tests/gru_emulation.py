"""Host emulation of how gru_step_kernel (csrc/gru.hip) consumes marlsc/gru.py:pack_gru's tensors: the
loops of gru_layer and gru_project over the packed fragments, lane by lane, every wave of 32 rows at
once. The sums are taken in float64 (exact under both recipes of oracle/gru_ref.py); the gate math
runs in `gate_dtype`.

MFMA operand maps (v_mfma_f32_32x32x2_f32, as tests/mlp_emulation.py): lane l holds A[l & 31][l >> 5]
and B[l >> 5][l & 31]; accumulator register r of lane l is D[rho(r, l >> 5)][l & 31]. gru_acc_load's
register 4g + i of lane half hf is element 8g + 4hf + i = rho(4g + i, hf) of a 32-float tile, so a
bias tile or a state tile loaded by it is an accumulator tile: D[u][c] = tile_of_row_c[u].

Also here: the packing's mutants (tests/test_gru_exact_host.py must see each one)."""
import numpy as np
import torch

import gru_ref as R
from marlsc import gru as G
from mlp_emulation import COL, HALF, rho


def pack_cpu(case):
    """pack_gru on CPU tensors of a case's weights, as numpy arrays (wi_0, wh_0, b_0[, ...], wo, bo)."""
    return tuple(t.numpy() for t in G.pack_gru(as_net(case)))


def as_net(case, act_pre=None, act_out=None):
    """A GRUNet holding a case's weights (CPU)."""
    from marlsc.rollout import GRUNet
    H, L, KO = case["w_hh"][0].shape[1], case["w_ih"][0].shape[1], case["w_o"].shape[0]
    net = GRUNet(L, KO, {"hidden_size": H, "num_layers": len(case["w_ih"]), "activation": act_pre,
                         "output_activation": act_out})
    lin = G.proj_parts(net["output_proj"])[1]
    with torch.no_grad():
        for l in range(len(case["w_ih"])):
            for name, key in (("weight_ih", "w_ih"), ("weight_hh", "w_hh"), ("bias_ih", "b_ih"), ("bias_hh", "b_hh")):
                getattr(net["gru"], f"{name}_l{l}").copy_(torch.from_numpy(case[key][l]))
        lin.weight.copy_(torch.from_numpy(case["w_o"]))
        lin.bias.copy_(torch.from_numpy(case["b_o"]))
    return net


def _mfma(a_lane, b_lane, d):
    """D += A B: A [32 x 2] per lane, B [2 x 32] per lane and wave ([64, waves]), D [32, waves, 32]."""
    nw = b_lane.shape[1]
    return d + np.einsum("rk,kwc->rwc", a_lane.reshape(2, 32).T, b_lane.reshape(2, 32, nw).transpose(0, 2, 1))


def _regs(tile, r):
    """Register r of every lane of every wave of an accumulator tile [32, waves, 32]: [64, waves]."""
    return tile[rho(r, HALF)[:, None], np.arange(tile.shape[1])[None, :], COL[:, None]]


def _sigmoid(v):
    one = v.dtype.type(1)
    with np.errstate(over="ignore"):  # expf(128) = inf in float32, and 1 / inf = 0: the kernel's value too
        return one / (one + np.exp(-v))


def _relu(code, v):
    assert code in (0, 1)
    return np.maximum(v, 0) if code == 1 else v


def emulate_gru(case, packed, n=None, act_pre=0, act_out=0, live=None, gate_dtype=np.float32, guard_store=True):
    """(h' [n, layers, H], y [n, KO]) of the first n rows of a case from the packed fragments only.
    live [n] bool: False rows read a zero state (the kernel's reset rows). guard_store=False: the
    projection's `row < KO` store guards removed -- y comes back [n, 32 ceil(KO / 32)] wide."""
    L, H, layers, KO = case["w_ih"][0].shape[1], case["w_hh"][0].shape[1], len(case["w_ih"]), case["w_o"].shape[0]
    n = len(case["x"]) if n is None else n
    nw = (n + 31) // 32
    NT, S4, KS1 = H // 32, H // 8, (L + 1) // 2
    M4 = (KS1 + 3) // 4
    j = np.arange(nw)[None, :] * 32 + COL[:, None]  # row of lane l of wave w
    jv = j < n
    jc = np.where(jv, j, 0)
    x, h0 = np.asarray(case["x"], np.float64), np.asarray(case["h"], np.float64)
    hf = HALF[:, None]

    def tile_of(vec, t):
        """gru_acc_load of the 32 floats vec[t * 32 ...] (the same for every lane: a bias tile)."""
        return np.broadcast_to(np.asarray(vec, np.float64)[t * 32:(t + 1) * 32, None, None], (32, nw, 32)).copy()

    def state_tile(l, t):
        """load_h: tile t of the row's old state of layer l, zero where not live, as [32, waves, 32]."""
        rows = np.arange(nw * 32)
        ok = rows < n
        if live is not None:
            ok = ok & np.asarray(live, bool)[np.where(rows < n, rows, 0)]
        v = np.where(ok[:, None], h0[np.where(rows < n, rows, 0), l, t * 32:(t + 1) * 32], 0.0)  # [cols, 32]
        return v.reshape(nw, 32, 32).transpose(2, 0, 1)

    hprev, out_h = None, []
    for l in range(layers):
        wi, wh, b = packed[3 * l], packed[3 * l + 1], np.asarray(packed[3 * l + 2], np.float64)
        wi = np.asarray(wi, np.float64).reshape(3 * NT, M4 if l == 0 else S4, 64, 4)
        wh = np.asarray(wh, np.float64).reshape(3 * NT, S4, 64, 4)
        hnew = []
        for t in range(NT):
            ar, az, ai, ah = (tile_of(b[g * H:(g + 1) * H], t) for g in range(4))
            if l == 0:
                for m in range(M4 * 4):
                    k = hf * KS1 + m
                    ok = jv & (m < KS1) & (k < L)
                    xb = np.where(ok, x[jc, np.minimum(k, L - 1)], 0.0)
                    ar = _mfma(wi[0 * NT + t, m // 4, :, m % 4], xb, ar)
                    az = _mfma(wi[1 * NT + t, m // 4, :, m % 4], xb, az)
                    ai = _mfma(wi[2 * NT + t, m // 4, :, m % 4], xb, ai)
            else:
                for s in range(S4 * 4):
                    bv = _regs(hprev[s // 16], s % 16)
                    ar = _mfma(wi[0 * NT + t, s // 4, :, s % 4], bv, ar)
                    az = _mfma(wi[1 * NT + t, s // 4, :, s % 4], bv, az)
                    ai = _mfma(wi[2 * NT + t, s // 4, :, s % 4], bv, ai)
            for kt in range(NT):
                hc = state_tile(l, kt)
                for q in range(4):
                    for i in range(4):
                        bv = _regs(hc, 4 * q + i)
                        s4 = kt * 4 + q
                        ar = _mfma(wh[0 * NT + t, s4, :, i], bv, ar)
                        az = _mfma(wh[1 * NT + t, s4, :, i], bv, az)
                        ah = _mfma(wh[2 * NT + t, s4, :, i], bv, ah)
            dt = gate_dtype
            ho = state_tile(l, t).astype(dt)
            rg, zg = _sigmoid(ar.astype(dt)), _sigmoid(az.astype(dt))
            ng = np.tanh(ai.astype(dt) + rg * ah.astype(dt))
            hnew.append(((dt(1) - zg) * ng + zg * ho).astype(np.float64))
        hprev = hnew
        out_h.append(np.concatenate([t.transpose(1, 2, 0).reshape(nw * 32, 32) for t in hnew], axis=1)[:n])
    hl = [_relu(act_pre, t) for t in hprev]
    OT = (KO + 31) // 32
    wo, bo = np.asarray(packed[-2], np.float64).reshape(OT, S4, 64, 4), np.asarray(packed[-1], np.float64)
    y = np.zeros((nw * 32, OT * 32))
    for q in range(OT):
        a3 = np.zeros((32, nw, 32))
        rows = q * 32 + np.arange(32)
        a3[rows < KO] = bo[rows[rows < KO], None, None]
        for s in range(S4 * 4):
            a3 = _mfma(wo[q, s // 4, :, s % 4], _regs(hl[s // 16], s % 16), a3)
        y[:, q * 32:(q + 1) * 32] = _relu(act_out, a3).transpose(1, 2, 0).reshape(nw * 32, 32)
    return np.stack(out_h, axis=1), (y[:n, :KO] if guard_store else y[:n])


# ---- the packing and its mutants --------------------------------------------------------------------

def index_of(kind, rows, cols):
    """marlsc.gru._index on the CPU as numpy (flat index, validity)."""
    idx, valid = G._index(kind, rows, cols, torch.device("cpu"))
    return idx.numpy(), valid.numpy()


def x_index(rows, cols, ks):
    """Kind "x" restated with the lane-half split `ks` as a parameter (the kernel's KS1 = (cols + 1) // 2
    fixes the fragment count M4; the test asserts that ks = KS1 reproduces marlsc.gru._index)."""
    m4 = ((cols + 1) // 2 + 3) // 4
    lane = np.arange(64)
    c, h = (lane & 31)[None, None, :, None], (lane >> 5)[None, None, :, None]
    i4 = np.arange(4)[None, None, None, :]
    nt = rows // 32
    row = np.arange(nt)[:, None, None, None] * 32 + c
    m = np.arange(m4)[None, :, None, None] * 4 + i4
    f = h * ks + m
    idx = row * cols + np.minimum(f, cols - 1)
    valid = np.broadcast_to((f < cols) & (m < ks), (nt, m4, 64, 4))
    return idx.reshape(-1), valid.reshape(-1)


def gather(w, idx, valid):
    return np.where(valid, np.asarray(w, np.float32).reshape(-1)[idx], np.float32(0))


def pack_with_rho(case, rho_fn):
    """pack_gru with another register-to-row map in place of marlsc.mlp._rho."""
    saved, keys = G._rho, [k for k in G._IDX if k[0] == "gru"]
    stash = {k: G._IDX.pop(k) for k in keys}
    G._rho = rho_fn
    try:
        return pack_cpu(case)
    finally:
        G._rho = saved
        for k in [k for k in G._IDX if k[0] == "gru"]:
            del G._IDX[k]
        G._IDX.update(stash)


def halves_contiguous(r, h):
    """A wrong rho: the lane halves own rows 0..15 and 16..31 instead of alternating groups of four."""
    return (r & 3) + 4 * (r >> 2) + 16 * h


def swap_gate_tiles(frag, NT, a=0, b=1):
    """A gate-carrying fragment tensor with the tiles of gates a and b exchanged."""
    v = np.array(frag).reshape(3, NT, -1)
    v[[a, b]] = v[[b, a]]
    return v.reshape(-1)


def replaced(packed, pos, value):
    out = list(packed)
    out[pos] = value
    return tuple(out)


def swap_in_packed(frag, index, valid, cols, row, ka, kb):
    """frag with the slots of W[row][ka] and W[row][kb] exchanged, located through the index map."""
    pos = []
    for k in (ka, kb):
        hit = np.flatnonzero((index == row * cols + k) & valid)
        assert hit.size == 1  # every weight sits in exactly one packed slot
        pos.append(hit[0])
    out = np.array(frag).reshape(-1)
    out[pos[0]], out[pos[1]] = out[pos[1]], out[pos[0]]
    assert not np.array_equal(out, np.asarray(frag).reshape(-1))
    return out


def ref_of(case):
    """(h' [n, layers, H], y) of either recipe as float64: int64 for the saturated part, float64 gates for
    a soft last layer."""
    if not case["soft"]:
        h, y, _ = R.s_forward(case)
        return h * R.UNIT, y * R.UNIT
    g = R.g_forward(case)
    return np.concatenate([g["h_exact"].astype(np.float64), g["h"][:, None]], axis=1), g["y"]


def with_weight(case, key, l, w):
    out = dict(case)
    if l is None:
        out[key] = w
    else:
        out[key] = list(case[key])
        out[key][l] = w
    return out


def find_swap(case, key, l, rows):
    """(row, ka, kb, mutated case): two different entries of one row of a weight matrix whose exchange
    changes the reference's output -- a live unit's row, by construction."""
    W = case[key] if l is None else case[key][l]
    base = ref_of(case)
    for r in rows:
        for ka in range(min(W.shape[1], 6)):
            for kb in range(ka + 1, min(W.shape[1], 7)):
                if W[r, ka] == W[r, kb]:
                    continue
                w = W.copy()
                w[r, ka], w[r, kb] = W[r, kb], W[r, ka]
                mut = with_weight(case, key, l, w)
                got = ref_of(mut)
                if not (np.array_equal(got[0], base[0]) and np.array_equal(got[1], base[1])):
                    return r, ka, kb, mut
    raise AssertionError(f"no live swap in {key}[{l}]")
