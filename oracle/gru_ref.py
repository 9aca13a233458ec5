"""TEST INFRASTRUCTURE ONLY: numpy references for the fused GRU step (csrc/gru.hip, marlsc/gru.py).

Recipe S (saturated gates, everything exact). The inputs x are integers in [-4, 4], the old state is
a non-zero multiple of 2^-6 in (-1, 1), the gate weights are 2^14 w with w an integer in [-3, 3], the
biases are b_ih = 128 + 256 k and b_hh = 256 k with k in [-512, 512) (up to 2^17: of the size of the
weighted sums, 2^17 to 2^19, so that a bias in the wrong slot flips gates as readily as a weight in
the wrong slot; with k in [-8, 8) a misplaced bias moved under 1 % of the gates). Every product and
bias of a layer is then a multiple of the granule g = 128 and, for each of the kernel's four
accumulators of every unit
(a_r and a_z with the folded bias b_i + b_h, a_in, a_hn), sum |terms| < 2^24 g -- the *headroom* -- so
every float32 partial sum is exact in any order. a_r, a_z and a_in are odd multiples of 128, a_hn is
a multiple of 256, so |a_r|, |a_z| and |a_in + r a_hn| are at least 128: in float32
1 / (1 + expf(-a)) is exactly 1 or 0 (expf underflows to 0 or overflows to inf) and tanhf is exactly
+-1. h' = (1 - z) n + z h is then exactly n = +-1 or the old state, the second layer reads exact
values, and y = W_o act(h') + b_o with integer W_o, b_o is an exact multiple of 2^-6. The int64
evaluation below works in units of 2^-6 and the comparison is on bits (+0 and -0 read as equal): one
misplaced weight, bias slot, state element or gate changes a sign somewhere.

Recipe G (soft last layer). The earlier layer, if any, is as in S (its h' is exact). The last layer
has weights w 2^-4 and biases k 2^-4: its four pre-activations are exact multiples of 2^-10 of
magnitude of a few units, exact in float32 in any order, and at least half of each gate's
pre-activations have |a| < 4. What is left to float32 is the gate math alone: the reference applies
the float64 formulas to the exact pre-activations, and the bound is anchored on a numpy float32
evaluation of the same formulas from the same pre-activations.

  gru_case          a network and its inputs (float32 arrays), recipe "S" or "G"
  s_forward         the int64 evaluation with its statistics; check_s asserts the method's conditions
  g_forward         float64 / float32 gate math on the exact pre-activations, the bounds
  f32_forward       a plain float32 evaluation (np.exp / np.tanh), summed forward or reversed
"""
import numpy as np

LIMIT = 1 << 24
UNIT = 2.0 ** -6      # the state's (and, scaled, every input's) unit
GRANULE = 128         # recipe S: every term of a gate accumulator is a multiple of it
SOFT = 2.0 ** -4      # recipe G: the last layer's weight and bias unit
U32 = 2.0 ** -24      # float32 unit roundoff
BIAS_K = 512          # recipe S: biases 128 + 256 k and 256 k with k in [-512, 512)


def _units(a, unit):
    """a / unit as int64, asserted exact."""
    v = np.asarray(a, np.float64) / unit
    assert np.all(v == np.rint(v)), f"not a multiple of {unit}"
    return v.astype(np.int64)


def gru_case(L, H, layers, KO, n, recipe="S", seed=0):
    """A GRU network L -> hidden H x layers -> KO with n input rows and old states.
    Returns a dict of float32 arrays: x [n, L], h [n, layers, H], w_ih / w_hh / b_ih / b_hh (lists per
    layer, nn.GRU's [3H, in] gate order r, z, n), w_o [KO, H], b_o [KO]; "soft": whether the last
    layer is recipe G's."""
    assert recipe in ("S", "G")
    rng = np.random.default_rng([L, H, layers, KO, n, seed, recipe == "G"])
    f = np.float32
    case = {"w_ih": [], "w_hh": [], "b_ih": [], "b_hh": [], "soft": recipe == "G"}
    for l in range(layers):
        din = L if l == 0 else H
        wi, wh = rng.integers(-3, 4, size=(3 * H, din)), rng.integers(-3, 4, size=(3 * H, H))
        if recipe == "G" and l == layers - 1:
            ki, kh = rng.integers(-8, 8, size=3 * H), rng.integers(-8, 8, size=3 * H)
            w_scale, bi, bh = SOFT, ki * SOFT, kh * SOFT
        else:
            ki, kh = rng.integers(-BIAS_K, BIAS_K, size=3 * H), rng.integers(-BIAS_K, BIAS_K, size=3 * H)
            w_scale, bi, bh = 2.0 ** 14, 128 + 256 * ki, 256 * kh
        case["w_ih"].append((wi * w_scale).astype(f))
        case["w_hh"].append((wh * w_scale).astype(f))
        case["b_ih"].append(np.asarray(bi, f))
        case["b_hh"].append(np.asarray(bh, f))
    case["w_o"] = rng.integers(-3, 4, size=(KO, H)).astype(f)
    case["b_o"] = rng.integers(-8, 9, size=KO).astype(f)
    case["x"] = rng.integers(-4, 5, size=(n, L)).astype(f)
    m = rng.integers(1, 64, size=(n, layers, H)) * (rng.integers(0, 2, size=(n, layers, H)) * 2 - 1)
    case["h"] = (m * UNIT).astype(f)
    return case


def rows_of(case, idx):
    """The same network on the rows idx of its inputs."""
    return dict(case, x=case["x"][idx], h=case["h"][idx])


def _pre(case, l, inp, h64, w_unit):
    """The kernel's four accumulators of layer l as int64 in units of w_unit 2^-6, and their headroom
    (max over rows and units of sum |terms|, same unit). inp / h64: the layer's input and old state in
    units of 2^-6."""
    H = h64.shape[1]
    wi, wh = _units(case["w_ih"][l], w_unit), _units(case["w_hh"][l], w_unit)
    bi, bh = _units(case["b_ih"][l], w_unit * UNIT), _units(case["b_hh"][l], w_unit * UNIT)
    gi, gh = inp @ wi.T, h64 @ wh.T
    ri, rh = np.abs(inp) @ np.abs(wi).T, np.abs(h64) @ np.abs(wh).T
    rz = slice(0, 2 * H)
    nn = slice(2 * H, 3 * H)
    a_rz = gi[:, rz] + gh[:, rz] + (bi + bh)[rz]
    a_in, a_hn = gi[:, nn] + bi[nn], gh[:, nn] + bh[nn]
    room = max(int((ri[:, rz] + rh[:, rz] + np.abs(bi + bh)[rz]).max()), int((ri[:, nn] + np.abs(bi[nn])).max()),
               int((rh[:, nn] + np.abs(bh[nn])).max())) if len(inp) else 0
    return a_rz[:, :H], a_rz[:, H:], a_in, a_hn, room


def _act_int(code, v):
    assert code in (0, 1), "exact only for MSC_ACT_NONE / MSC_ACT_RELU"
    return np.maximum(v, 0) if code == 1 else v


def s_forward(case, act_pre=0, act_out=0, live=None, upto=None):
    """The int64 evaluation of recipe-S layers. live [n] bool: rows whose flag is False read a zero
    state (reset rows). upto: evaluate only that many layers (recipe G's exact part) and no projection.
    Returns (h [n, layers, H] int64 in units of 2^-6, y [n, KO] int64 in units of 2^-6 or None, stats):
    stats = {"min_a": the smallest |a_r|, |a_z|, |a_in + r a_hn| seen, "headroom": per layer, in
    granules, "gates": per layer the shares of r = 1, z = 1, n = +1, "y_room": the projection's}."""
    x64 = _units(case["x"], 1.0) * 64
    h0 = _units(case["h"], UNIT)
    if live is not None:
        h0 = h0 * np.asarray(live, bool)[:, None, None]
    layers = len(case["w_ih"]) if upto is None else upto
    inp, hs = x64, []
    stats = {"min_a": np.inf, "headroom": [], "gates": [], "y_room": 0}
    for l in range(layers):
        a_r, a_z, a_in, a_hn, room = _pre(case, l, inp, h0[:, l], 1.0)
        r, z = a_r > 0, a_z > 0
        a_n = a_in + r * a_hn
        for a in (a_r, a_z, a_in, a_n):
            assert np.all(a % (2 * GRANULE * 64) == GRANULE * 64), "not an odd multiple of the granule"
        assert np.all(a_hn % (2 * GRANULE * 64) == 0)
        if a_r.size:
            stats["min_a"] = min(stats["min_a"], float(min(np.abs(a_r).min(), np.abs(a_z).min(), np.abs(a_n).min())) * UNIT)
        stats["headroom"].append(room / (GRANULE * 64))
        stats["gates"].append(tuple(float(g.mean()) if g.size else 0.5 for g in (r, z, a_n > 0)))
        inp = np.where(z, h0[:, l], np.where(a_n > 0, 64, -64))
        hs.append(inp)
    hn = np.stack(hs, axis=1) if hs else h0[:, :0]
    if upto is not None:
        return hn, None, stats
    wo, bo = _units(case["w_o"], 1.0), _units(case["b_o"], 1.0) * 64
    hp = _act_int(act_pre, inp)
    y = hp @ wo.T + bo
    stats["y_room"] = int((np.abs(hp) @ np.abs(wo).T + np.abs(bo)).max()) if len(hp) else 0
    return hn, _act_int(act_out, y), stats


def check_s(stats, y=None):
    """The conditions under which the comparison on bits is exact and not vacuous."""
    assert all(r < LIMIT for r in stats["headroom"]) and stats["y_room"] < LIMIT, f"headroom {stats['headroom']} reaches 2^24"
    assert stats["min_a"] >= 128, f"min |a| = {stats['min_a']}: a gate may not saturate in float32"
    for g in stats["gates"]:
        assert all(0.25 <= s <= 0.75 for s in g), f"gate shares (r, z, n) {stats['gates']}: every gate must matter both ways"
    if y is not None:
        assert y.size and y.min() != y.max(), "all outputs equal"


def s_reference(case, act_pre=0, act_out=0, live=None):
    """s_forward with check_s asserted: (h', y) as float32 arrays (exact: multiples of 2^-6 below 2^18)."""
    h, y, stats = s_forward(case, act_pre, act_out, live)
    check_s(stats, y)
    return (h * UNIT).astype(np.float32), (y * UNIT).astype(np.float32)


def same_bits(got, want):
    """Bit equality of two float32 arrays, +0 and -0 read as equal."""
    a = np.ascontiguousarray(got, np.float32) + np.float32(0)  # -0 + 0 = +0; NaN stays NaN
    b = np.ascontiguousarray(want, np.float32) + np.float32(0)
    return a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


# ---- recipe G ---------------------------------------------------------------------------------------

def _gates(a_r, a_z, a_in, a_hn, h, dt):
    """PyTorch's GRU cell from its four pre-activations, every operation in dtype dt."""
    a_r, a_z, a_in, a_hn, h = (np.asarray(v, dt) for v in (a_r, a_z, a_in, a_hn, h))
    one = dt(1)
    with np.errstate(over="ignore"):
        r = one / (one + np.exp(-a_r))
        z = one / (one + np.exp(-a_z))
    n = np.tanh(a_in + r * a_hn)
    return ((one - z) * n + z * h).astype(dt)


def g_forward(case, live=None):
    """Recipe G. Returns a dict: "h_exact" [n, layers - 1, H] float32 (the saturated layers' h', bit
    exact), "h" [n, H] and "y" [n, KO] float64 references of the last layer and the projection (no
    activations), "e32": the maximum error of the numpy float32 evaluation of the same formulas from the
    same exact pre-activations, "h_bound" = 4 max(e32, 2^-24) (the 4: the project's allowance for
    another libm's expf / tanhf), "y_bound" [n, KO].

    y_bound: the kernel holds h^ with |h^ - h'| <= h_bound and computes fl(b_o + sum_k w_o,k h^_k), a
    float32 dot product of H + 1 terms in some order: each term takes part in at most H + 1 roundings
    (its product and at most H additions), so
      |y^ - y| <= h_bound sum_k |w_o,k|  +  gamma (|b_o| + sum_k |w_o,k| (|h'_k| + h_bound)),
    gamma = (H + 1) 2^-24 / (1 - (H + 1) 2^-24) (Higham, Accuracy and Stability, section 3.1)."""
    assert case["soft"]
    layers = len(case["w_ih"])
    hx, _, stats = s_forward(case, live=live, upto=layers - 1)
    if layers > 1:
        check_s(stats)
    h0 = _units(case["h"], UNIT)
    if live is not None:
        h0 = h0 * np.asarray(live, bool)[:, None, None]
    inp = hx[:, -1] if layers > 1 else _units(case["x"], 1.0) * 64
    unit = SOFT * UNIT
    pre = _pre(case, layers - 1, inp, h0[:, -1], SOFT)
    room = pre[4]
    assert room < LIMIT, "the soft layer's pre-activations are not exact in float32"
    a_r, a_z, a_in, a_hn = (a * unit for a in pre[:4])  # exact in float64 and in float32
    hold = h0[:, -1] * UNIT
    h64 = _gates(a_r, a_z, a_in, a_hn, hold, np.float64)
    h32 = _gates(a_r, a_z, a_in, a_hn, hold, np.float32)
    r64 = 1.0 / (1.0 + np.exp(-a_r))
    soft = [float((np.abs(a) < 4).mean()) for a in (a_r, a_z, a_in + r64 * a_hn)]
    assert all(s >= 0.5 for s in soft), f"share of |a| < 4 per gate {soft}: the gates must be soft"
    e32 = float(np.abs(h32.astype(np.float64) - h64).max())
    hb = 4.0 * max(e32, U32)
    wo, bo = case["w_o"].astype(np.float64), case["b_o"].astype(np.float64)
    H = h64.shape[1]
    gamma = (H + 1) * U32 / (1.0 - (H + 1) * U32)
    y = h64 @ wo.T + bo
    yb = hb * np.abs(wo).sum(axis=1)[None, :] + gamma * (np.abs(bo)[None, :] + (np.abs(h64) + hb) @ np.abs(wo).T)
    return {"h_exact": (hx * UNIT).astype(np.float32), "h": h64, "y": y, "e32": e32, "h_bound": hb, "y_bound": yb,
            "soft_share": soft}


# ---- plain float32 evaluation -------------------------------------------------------------------------

def f32_forward(case, reverse=False, live=None):
    """A plain float32 evaluation of the whole step (no activations on the projection): every sum taken
    term by term in float32, in k order or reversed, bias first; gates with np.exp / np.tanh in float32.
    Returns (h' [n, layers, H], y [n, KO]) float32."""
    f = np.float32

    def dot(acc, w, v):
        ks = range(w.shape[1] - 1, -1, -1) if reverse else range(w.shape[1])
        for k in ks:
            acc = (acc + v[:, k:k + 1] * w[None, :, k]).astype(f)
        return acc

    h0 = case["h"].astype(f)
    if live is not None:
        h0 = h0 * np.asarray(live, f)[:, None, None]
    inp, hs = case["x"].astype(f), []
    n = len(inp)
    for l in range(len(case["w_ih"])):
        H = h0.shape[2]
        wi, wh, bi, bh = (case[k][l].astype(f) for k in ("w_ih", "w_hh", "b_ih", "b_hh"))
        a_rz = dot(dot(np.tile((bi + bh)[:2 * H], (n, 1)), wi[:2 * H], inp), wh[:2 * H], h0[:, l])
        a_in = dot(np.tile(bi[2 * H:], (n, 1)), wi[2 * H:], inp)
        a_hn = dot(np.tile(bh[2 * H:], (n, 1)), wh[2 * H:], h0[:, l])
        inp = _gates(a_rz[:, :H], a_rz[:, H:], a_in, a_hn, h0[:, l], f)
        hs.append(inp)
    y = dot(np.tile(case["b_o"].astype(f), (n, 1)), case["w_o"].astype(f), inp)
    return np.stack(hs, axis=1), y
