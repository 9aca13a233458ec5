"""The demand generators' draw (csrc/demand_common.hpp: gen_uniform / gen_advance, driven through
msc_gen_draws) against Python-integer arithmetic, bit for bit: the state advances as
(s * M^G + C) mod 2^128 and the uniform is (x >> 11) * 2^-53 of the XSL-RR output x of the state.

Lanes 0-31 start from random states and increments (some with chosen rotations and outputs), lanes
32-63 from words of {0, 1, 0x7FFFFFFF, 0x80000000, 0xFFFFFFFF} picked so that the first step meets
every combination of the carries of the 128-bit multiply-add: the three of the word-by-word schedule
(k0: s0 m0 + (c1:c0); k1: s0 m1 + (c2:t1); k2: s1 m0 + (q2:q1)) and the three of the schedule the
kernel uses (kO of the odd pair, ca and ca' of the closing adds).

Not every combination exists for every stride. k1 + k2 (and likewise kO) is the part above 2^64 of
s0 m1 + s1 m0 + an addend below 2^64, at most (2^32 - 1)(m0 + m1) + 2^64 - 1, which is below 2^65
(for kO: below 2^64) whenever m0 + m1 <= 2^32 - 1. That holds for the low words of M^1, M^2 and M^7,
so at those strides k1 and k2 never fire together and kO never fires, whatever the state; the six
(four) combinations that remain are required there, all eight at strides 3 (the kernels') and 5
(for the kernel's own schedule at stride 5: the four without kO, and kO at least once)."""
import ctypes as C
import itertools

import numpy as np
import pytest

torch = pytest.importorskip("torch")

pytestmark = pytest.mark.gpu

M64, M32, M128 = (1 << 64) - 1, (1 << 32) - 1, (1 << 128) - 1
PCG_MUL = (2549297995355413924 << 64) | 4865540595714422341
EDGE_WORDS = (0, 1, 0x7FFFFFFF, 0x80000000, 0xFFFFFFFF)
STRIDES = (1, 2, 3, 5, 7)
ROTATIONS = (0, 1, 31, 32, 33, 63)
# first outputs x: the 21 bits below the high word all ones (and the low 21 bits with them), the high
# word zero, the largest and the smallest uniform
OUTPUTS = (0x13579BDFFFFFFFFF, 0x00000000DEADBEEF, M64, 0)


def words(v):
    return [(v >> (32 * i)) & M32 for i in range(4)]


def carries(s, c, m):
    """(k0, k1, k2) of the word-by-word schedule and (kO, ca, ca') of the kernel's, for one step."""
    s0, s1, s2, _ = words(s)
    m0, m1, m2, _ = words(m)
    c0, c1, c2, c3 = words(c)
    t = s0 * m0 + ((c1 << 32) | c0)
    q = s0 * m1 + ((c2 << 32) | ((t >> 32) & M32))
    r = s1 * m0 + (q & M64)
    o1 = s0 * m1 + c1
    o = s1 * m0 + o1
    e01 = s0 * m0 + c0
    e23 = (s0 * m2 + s1 * m1 + s2 * m0 + ((c3 << 32) | c2)) & M64
    assert o1 >> 64 == 0 and e01 >> 64 == 0
    ca = ((e01 >> 32) + (o & M32)) >> 32
    cb = ((e23 & M32) + ((o >> 32) & M32) + ca) >> 32
    return (t >> 64, q >> 64, r >> 64), (o >> 64, ca, cb)


def possible_carries(stride, m):
    """The (k0, k1, k2) and (kO, ca, ca') combinations some state and increment produce (module docstring)."""
    every = set(itertools.product((0, 1), repeat=3))
    if (m & M32) + ((m >> 32) & M32) <= M32:
        assert stride in (1, 2, 7)
        return {k for k in every if not (k[1] and k[2])}, {k for k in every if not k[0]}
    assert stride in (3, 5)
    return set(every), (set(every) if stride == 3 else {k for k in every if not k[0]})


def uniform_bits(s):
    hi, lo = s >> 64, s & M64
    x, rot = hi ^ lo, hi >> 58
    x = ((x >> rot) | (x << ((64 - rot) & 63))) & M64
    return int((np.float64(x >> 11) * np.float64(2.0 ** -53)).view(np.uint64))  # exact: x >> 11 < 2^53


def state_with_output(rng, x):
    """A state whose XSL-RR output is x (random high half, rotation from its top six bits)."""
    hi = int(rng.integers(0, 1 << 64, dtype=np.uint64))
    rot = hi >> 58
    unrot = ((x << rot) | (x >> ((64 - rot) & 63))) & M64
    return (hi << 64) | (hi ^ unrot)


def make_lanes(stride):
    rng = np.random.default_rng(1000 + stride)
    m = pow(PCG_MUL, stride, 1 << 128)
    rand128 = lambda: (int(rng.integers(0, 1 << 64, dtype=np.uint64)) << 64) | int(rng.integers(0, 1 << 64, dtype=np.uint64))
    states = [rand128() for _ in range(32)]
    incs = [rand128() for _ in range(32)]
    for lane, rot in enumerate(ROTATIONS):
        states[lane] = (states[lane] & ((1 << 122) - 1)) | (rot << 122)
    for lane, x in enumerate(OUTPUTS, start=len(ROTATIONS)):
        states[lane] = state_with_output(rng, x)
    # lanes 32-63: edge words, first the lanes that complete the two sets of carry combinations
    pool = [(sum(int(w) << (32 * i) for i, w in enumerate(rng.choice(EDGE_WORDS, 4))),
             sum(int(w) << (32 * i) for i, w in enumerate(rng.choice(EDGE_WORDS, 4)))) for _ in range(6000)]
    need = list(possible_carries(stride, m))
    at_least_one_kO = stride == 5
    edge = []
    for s, c in pool:
        got = carries(s, c, m)
        new_kO = at_least_one_kO and got[1][0] == 1
        if (new_kO or any(got[i] in need[i] for i in range(2))) and len(edge) < 32:
            edge.append((s, c))
            at_least_one_kO = at_least_one_kO and not new_kO
            for i in range(2):
                need[i].discard(got[i])
    assert not need[0] and not need[1] and not at_least_one_kO, f"stride {stride}: carry combinations not met: {need}"
    edge += pool[:32 - len(edge)]
    states += [s for s, _ in edge]
    incs += [c for _, c in edge]
    return m, states, incs


def reference(m, states, incs, n):
    out = np.empty((64, n), dtype=np.uint64)
    fin = []
    for lane, (s, c) in enumerate(zip(states, incs)):
        for i in range(n):
            out[lane, i] = uniform_bits(s)
            s = (s * m + c) & M128
        fin.append(s)
    return out, fin


def halves(vals):
    return np.array([[v >> 64, v & M64] for v in vals], dtype=np.uint64)


def device(stride, states, incs, n):
    from marlsc import abi
    st, inc = halves(states), halves(incs)
    out = np.zeros((64, max(n, 1)), dtype=np.uint64)
    fin = np.zeros((64, 2), dtype=np.uint64)
    vp = lambda a: a.ctypes.data_as(C.c_void_p)
    abi.check(abi.lib().msc_gen_draws(vp(st), vp(inc), stride, n, vp(out), vp(fin)))
    return out.reshape(-1)[:64 * n].reshape(64, n), fin


def test_uniform_reference_is_numpys():
    # the Python-integer reference itself against numpy's PCG64 random() (stride 1, the stream's own increment)
    bg = np.random.PCG64(7)
    st = bg.state["state"]
    want = np.random.Generator(bg).random(50)
    s, c = st["state"], st["inc"]
    for w in want:
        s = (s * PCG_MUL + c) & M128
        assert uniform_bits(s) == int(np.float64(w).view(np.uint64))


@pytest.mark.parametrize("stride", STRIDES)
def test_gen_draw_bit_exact(stride):
    m, states, incs = make_lanes(stride)
    # the lanes hold what they were built for
    assert [s >> 122 for s in states[:len(ROTATIONS)]] == list(ROTATIONS)
    first = [uniform_bits(s) for s in states[len(ROTATIONS):len(ROTATIONS) + len(OUTPUTS)]]
    assert first == [int(np.float64((x >> 11) * 2.0 ** -53).view(np.uint64)) for x in OUTPUTS]
    met = [{carries(s, c, m)[i] for s, c in zip(states[32:], incs[32:])} for i in range(2)]
    must = possible_carries(stride, m)
    assert met[0] >= must[0] and met[1] >= must[1], (stride, met)
    if stride in (3, 5):
        assert len(met[0]) == 8 and any(k[0] for k in met[1])
    if stride == 3:
        assert len(met[1]) == 8
    want, want_fin = reference(m, states, incs, 256)
    for n in (256, 255, 1):  # (an odd count and a single draw: the loop's tail)
        got, fin = device(stride, states, incs, n)
        bad = np.argwhere(got != want[:, :n])
        assert bad.size == 0, f"stride {stride}, n {n}: first mismatches (lane, draw) {bad[:5].tolist()}"
        ref_fin = want_fin if n == 256 else reference(m, states, incs, n)[1]
        assert np.array_equal(fin, halves(ref_fin)), f"stride {stride}, n {n}: final states differ"


def test_gen_draw_rejects_other_strides():
    from marlsc import abi
    z = np.zeros((64, 2), dtype=np.uint64)
    vp = lambda a: a.ctypes.data_as(C.c_void_p)
    assert abi.lib().msc_gen_draws(vp(z), vp(z), 4, 1, vp(z), vp(z)) != 0
