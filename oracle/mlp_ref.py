"""TEST INFRASTRUCTURE ONLY: numpy references for the fused policy MLP (csrc/mlp_kernels.hpp).

The integer method. Every product of the f32 MFMA (and of the VALU output layer's fma) is exact and
every accumulation is float32. When x, the weights, the biases (and pre1) are integers and at every
layer  |b| (+ |pre1|) + sum_k |w_k| |h_k| < 2^24  -- the *headroom* -- every partial sum, taken in any
order, fused or not, is an integer below 2^24 and therefore exact in float32. The kernel's output is
then the int64 evaluation bit for bit, whatever its accumulation order, lane split or pass form, and
the comparison needs no tolerance: one misplaced weight, one wrong guard or one reduced-precision
operand changes an integer.

  int_case / int_head_case   integer networks and inputs (float32 arrays holding integers)
  int_forward                the int64 evaluation, the headroom and the share of active hidden units
  check_conditions           what every test asserts before it compares anything
  f64_forward, f32_chain_forward, f32_matmul_forward, truncate_mantissa
                             the real-valued check: a float64 reference and two CPU float32
                             evaluations whose own error anchors the tolerance
"""
import numpy as np

LIMIT = 1 << 24  # integers of magnitude < 2^24 are exact in float32, and so are their sums below it


def _ints(a):
    a = np.asarray(a)
    assert np.all(a == np.rint(a)), "not an integer array"
    return a.astype(np.int64)


def _sparse_signs(rng, shape, density):
    """Entries in {-1, 0, 1}: non-zero with probability `density`."""
    return (rng.integers(0, 2, size=shape) * 2 - 1) * (rng.random(shape) < density)


def _odd(rng, shape, bound=4096):
    """Odd integers of magnitude < bound: up to 12 significant bits, the lowest one set."""
    return 2 * rng.integers(-bound // 2, bound // 2, size=shape) + 1


RECIPES = ("A", "Bx", "Bw")


def int_case(L, hidden, KO, recipe, n, seed=0, pre1_group=0):
    """An integer network L -> hidden[0] (-> hidden[1]) -> KO with n integer input rows.

    recipe "A" (dense): every entry of x, W and b uniform in [-3, 3]; about half of the hidden units
      are active, and every weight position matters.
    recipe "Bx" / "Bw" (wide operands): operands of 12 to 20 significant bits at every layer, which a
      product that is not exact (a reduced-precision MFMA operand) cannot survive. Bx: x odd with
      |x| < 4096 and W1 in {-1, 0, 1}; Bw: W1 odd with |w| < 4096 and x in {-1, 0, 1}. W1 has density
      min(1, 32 / L), the later layers are {-1, 0, 1} at density 1/8, biases are in {-1, 0, 1}. The
      hidden activations then carry 15 to 20 bits into the later layers.
    pre1_group > 0: also an integer pre1 [ceil(n / pre1_group), hidden[0]] in [-3, 3].

    No shape used by the tests needed narrower ranges or densities than these (check_conditions is
    asserted for every case); a shape that does must narrow them here, not be skipped.
    Returns a dict: x [n, L], W (list of [out, in]), b (list), pre1 / group, all float32 but pre1=None
    without a group."""
    assert recipe in RECIPES
    rng = np.random.default_rng([L, KO, n, seed, RECIPES.index(recipe)] + list(hidden))
    dims = [L] + list(hidden) + [KO]
    W, b = [], []
    for i, (din, dout) in enumerate(zip(dims[:-1], dims[1:])):
        if recipe == "A":
            W.append(rng.integers(-3, 4, size=(dout, din)))
            b.append(rng.integers(-3, 4, size=dout))
            continue
        if i == 0:
            w = _sparse_signs(rng, (dout, din), min(1.0, 32.0 / L))
            if recipe == "Bw":
                w = w * np.abs(_odd(rng, (dout, din)))
        else:
            w = _sparse_signs(rng, (dout, din), 1.0 / 8.0)
        W.append(w)
        b.append(rng.integers(-1, 2, size=dout))
    if recipe == "A":
        x = rng.integers(-3, 4, size=(n, L))
    elif recipe == "Bx":
        x = _odd(rng, (n, L))
    else:
        x = rng.integers(-1, 2, size=(n, L))
    f = np.float32
    case = {"x": x.astype(f), "W": [w.astype(f) for w in W], "b": [v.astype(f) for v in b], "pre1": None, "group": 1}
    if pre1_group > 0:
        case["pre1"] = rng.integers(-3, 4, size=((n + pre1_group - 1) // pre1_group, hidden[0])).astype(f)
        case["group"] = pre1_group
    return case


def int_head_case(L, hidden, K, n, seed=0, pre1_group=0):
    """An integer mu / sigma-head actor: recipe-A hidden layers, a sparse integer backbone output
    Linear W_out [H, H] ({-1, 0, 1}, four non-zeros per row on average) and integer heads in [-2, 2],
    so that the fold W_eff = [W_mu; W_sigma] W_out, b_eff = [W_mu; W_sigma] b_out + [b_mu; b_sigma]
    is an exact integer matrix of small entries and the folded network keeps the headroom.
    pre1_group > 0: int_case's integer pre1 (drawn after everything else: the weights do not change).
    Returns the case of the folded network (W[-1] = W_eff [2K, H]) plus the module weights under
    "out" (W_out, b_out), "mu" and "sigma" ((W, b) each)."""
    rng = np.random.default_rng([L, K, n, seed, 77] + list(hidden))
    case = int_case(L, hidden, 2 * K, "A", n, seed, pre1_group)
    H = hidden[-1]
    w_out = _sparse_signs(rng, (H, H), 4.0 / H)
    b_out = rng.integers(-3, 4, size=H)
    w_mu, w_sg = rng.integers(-2, 3, size=(K, H)), rng.integers(-2, 3, size=(K, H))
    b_mu, b_sg = rng.integers(-3, 4, size=K), rng.integers(-3, 4, size=K)
    wh = np.concatenate([w_mu, w_sg])
    f = np.float32
    case["W"][-1] = (wh @ w_out).astype(f)
    case["b"][-1] = (wh @ b_out + np.concatenate([b_mu, b_sg])).astype(f)
    case["out"] = (w_out.astype(f), b_out.astype(f))
    case["mu"] = (w_mu.astype(f), b_mu.astype(f))
    case["sigma"] = (w_sg.astype(f), b_sg.astype(f))
    return case


def int_forward(x, W, b, pre1=None, group=1):
    """The int64 evaluation of Linear -> ReLU -> ... -> Linear on integer arrays.
    Returns (out [n, KO] int64, headroom, active): headroom[i] = max over rows and units of
    |b| (+ |pre1|) + sum_k |w_k| |h_k| at layer i; active[i] = share of positive units of hidden layer i."""
    h = _ints(x)
    n = h.shape[0]
    headroom, active = [], []
    for i, (w, v) in enumerate(zip(W, b)):
        wi, bi = _ints(w), _ints(v)
        z = h @ wi.T + bi
        room = np.abs(h) @ np.abs(wi).T + np.abs(bi)
        if i == 0 and pre1 is not None:
            p = _ints(pre1)[np.arange(n) // group]
            z = z + p
            room = room + np.abs(p)
        headroom.append(int(room.max()) if room.size else 0)
        if i + 1 < len(W):
            active.append(float((z > 0).mean()) if z.size else 0.5)
            h = np.maximum(z, 0)
    return z, headroom, active


def check_conditions(out, headroom, active):
    """The conditions under which the integer comparison is exact and not vacuous."""
    assert all(r < LIMIT for r in headroom), f"headroom {headroom} reaches 2^24: partial sums may round"
    assert all(0.25 <= a <= 0.75 for a in active), f"active hidden units {active}: ReLU must matter both ways"
    assert out.size and out.min() != out.max(), "all outputs equal"


def case_forward(case):
    """int_forward of a case dict with check_conditions asserted; returns the int64 outputs."""
    out, headroom, active = int_forward(case["x"], case["W"], case["b"], case["pre1"], case["group"])
    check_conditions(out, headroom, active)
    return out


# ---- the real-valued check ------------------------------------------------------------------------

def f64_forward(x, W, b):
    h = np.asarray(x, np.float64)
    for i, (w, v) in enumerate(zip(W, b)):
        h = h @ np.asarray(w, np.float64).T + np.asarray(v, np.float64)
        if i + 1 < len(W):
            h = np.maximum(h, 0.0)
    return h


def f32_chain_forward(x, W, b):
    """float32 evaluation as one sequential chain in k order per output: acc = f32(acc + w_k h_k)
    with the product in float64 (i.e. a fused multiply-add chain starting from the bias)."""
    h = np.asarray(x, np.float32)
    for i, (w, v) in enumerate(zip(W, b)):
        w64 = np.asarray(w, np.float64)
        acc = np.broadcast_to(np.asarray(v, np.float32), (h.shape[0], w64.shape[0])).copy()
        for k in range(w64.shape[1]):
            acc = (acc.astype(np.float64) + h[:, k:k + 1].astype(np.float64) * w64[None, :, k]).astype(np.float32)
        h = np.maximum(acc, np.float32(0)) if i + 1 < len(W) else acc
    return h


def f32_matmul_forward(x, W, b):
    """float32 evaluation with numpy's float32 matmul (its own blocked summation order)."""
    h = np.asarray(x, np.float32)
    for i, (w, v) in enumerate(zip(W, b)):
        h = h @ np.asarray(w, np.float32).T + np.asarray(v, np.float32)
        if i + 1 < len(W):
            h = np.maximum(h, np.float32(0))
    return h


def truncate_mantissa(a, bits=10):
    """float32 array with the mantissa cut to `bits` explicit bits (toward zero)."""
    u = np.ascontiguousarray(a, np.float32).view(np.uint32)
    return (u & np.uint32((0xFFFFFFFF << (23 - bits)) & 0xFFFFFFFF)).view(np.float32)


def shuffled_f32_sum_forward(x, W, b, rng):
    """float32 evaluation of an integer network whose every sum is taken term by term in a random
    order (bias included as a term): under the headroom condition it equals int_forward."""
    h = np.asarray(x, np.float32)
    for i, (w, v) in enumerate(zip(W, b)):
        w = np.asarray(w, np.float32)
        terms = np.concatenate([h[:, None, :] * w[None, :, :],
                                np.broadcast_to(np.asarray(v, np.float32)[None, :, None], (h.shape[0], w.shape[0], 1))], axis=2)
        acc = np.zeros(terms.shape[:2], np.float32)
        for k in rng.permutation(terms.shape[2]):
            acc = acc + terms[:, :, k]
        h = np.maximum(acc, np.float32(0)) if i + 1 < len(W) else acc
    return h
