"""GPU tests of msc_adam_clip_step (csrc/adam_clip.hip) against its numpy restatement (tests/adam_emulation.py),
bit for bit. The gradients are integers of magnitude at most 1024: every square and every partial sum of
squares is then exact in float64 in any order, so the group norms are determined exactly and p, m, v (arbitrary
floats) and the clipped gradients leave no room either: every elementwise operation is one float32 rounding.

Every buffer sits between guard words that must come back untouched, the workspace too."""
import ctypes as C

import numpy as np
import pytest
import torch

import adam_emulation as em

pytestmark = pytest.mark.gpu
GUARD = 4           # floats in front of and behind every buffer
SENTINEL = -77.25
LR = 1e-3


def _geometry():
    from marlsc import optim
    g = optim.geometry()
    return g["chunk"], g["table_capacity"]


def _tensor(rng, n, group, misalign=False, zeros=False):
    """p, m, v arbitrary floats (v >= 0, some exactly 0), g integers in [-1024, 1024] (some exactly 0)"""
    g = rng.integers(-1024, 1025, size=n).astype(np.float32)
    v = rng.random(n).astype(np.float32) ** 2
    if n > 2:
        g[rng.integers(0, n)] = 0.0
        v[rng.integers(0, n)] = 0.0
    if zeros:
        g[:] = 0.0
    return {"p": rng.standard_normal(n).astype(np.float32), "g": g, "m": (0.1 * rng.standard_normal(n)).astype(np.float32),
            "v": v, "group": group, "misalign": misalign}


class _Device:
    """The tensors' buffers on the device, each inside guard words, and the host table over them."""

    def __init__(self, tensors):
        from marlsc import optim
        self.tensors = tensors
        self.bufs = []
        self.table = np.zeros(len(tensors), dtype=optim.TABLE_DTYPE)
        for i, t in enumerate(tensors):
            n, off = t["p"].size, GUARD + (1 if t.get("misalign") else 0)
            row = {}
            for k in ("p", "g", "m", "v"):
                host = np.full(n + 2 * GUARD + 1, SENTINEL, np.float32)
                host[off:off + n] = t[k]
                row[k] = torch.from_numpy(host).cuda()
                ptr = row[k].data_ptr() + 4 * off
                assert ptr % 16 == (4 if t.get("misalign") else 0)
                self.table[k][i] = ptr
            self.table["n"][i], self.table["group"][i] = n, t["group"]
            self.bufs.append((row, off, n))
        total = int(sum(t["p"].size for t in tensors))
        nbytes = optim.workspace_bytes(len(tensors), total)
        assert nbytes > 0 and nbytes % 8 == 0
        self.ws_words = nbytes // 8
        self.ws = torch.full((self.ws_words + 8,), SENTINEL, dtype=torch.float64, device="cuda")

    def read(self):
        """the tensors as they are on the device now; asserts the guards"""
        out = []
        for (row, off, n), t in zip(self.bufs, self.tensors):
            o = {"group": t["group"], "misalign": t.get("misalign", False)}
            for k in ("p", "g", "m", "v"):
                host = row[k].cpu().numpy()
                assert (host[:off] == SENTINEL).all() and (host[off + n:] == SENTINEL).all(), "a write outside a buffer"
                o[k] = host[off:off + n].copy()
            out.append(o)
        assert bool((self.ws[self.ws_words:] == SENTINEL).all()), "a write behind the workspace"
        return out


def _call(dev, n_groups, *, step, max_norm, write=True, lr=LR, norms=True):
    from marlsc import optim
    nout = torch.full((n_groups,), float("nan"), dtype=torch.float64, device="cuda") if norms else None
    optim.adam_clip_launch(dev.table, n_groups, lr=lr, beta1=0.9, beta2=0.999, eps=1e-8, max_norm=max_norm, step=step,
                           write_clipped_grads=write, workspace=dev.ws, norms_out=nout)
    torch.cuda.synchronize()
    return dev.read(), (nout.cpu().numpy() if norms else None)


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _assert_equal(got, want, keys=("p", "g", "m", "v"), what=""):
    for i, (a, b) in enumerate(zip(got, want)):
        for k in keys:
            assert np.array_equal(_bits(a[k]), _bits(b[k])), (what, "tensor", i, k, a[k].size)


def _check(tensors, n_groups, *, steps=(1,), max_norm, write=True, rng=None):
    """Consecutive calls at the given step counts, fresh integer gradients before each; everything bit-equal."""
    dev = _Device(tensors)
    cur = tensors
    for s in steps:
        want, norms = em.step(cur, n_groups, lr=LR, max_norm=max_norm, step=s)
        got, gn = _call(dev, n_groups, step=s, max_norm=max_norm, write=write)
        assert np.array_equal(gn, norms), (gn, norms)  # the exact norms, 0 for a group without elements
        _assert_equal(got, want, keys=("p", "m", "v") + (("g",) if write else ()), what=f"step {s}")
        if not write:
            _assert_equal(got, cur, keys=("g",), what="g untouched")
        cur = [dict(w, misalign=t.get("misalign", False)) for w, t in zip(want, tensors)]
        if rng is not None:  # the next step's gradients, written to the device buffers
            for (row, off, n), t in zip(dev.bufs, cur):
                t["g"] = rng.integers(-1024, 1025, size=n).astype(np.float32)
                row["g"][off:off + n] = torch.from_numpy(t["g"]).cuda()
        elif not write:
            for t, old in zip(cur, tensors):
                t["g"] = old["g"]
    return cur


def test_lengths_around_the_vector_width_and_the_block_chunk_three_steps():
    chunk, _ = _geometry()
    rng = np.random.default_rng(0)
    lengths = [1, 3, 4, 5, chunk - 1, chunk, chunk + 1, 0, 2 * chunk + 3, 7]
    tensors = [_tensor(rng, n, 0) for n in lengths]
    tensors += [_tensor(rng, chunk + 1, 0, misalign=True), _tensor(rng, 5, 0, misalign=True),
                _tensor(rng, 4, 0, misalign=True), _tensor(rng, 2 * chunk, 0, misalign=True)]
    norm = float(em.group_norms(tensors, 1)[0])
    _check(tensors, 1, steps=(1, 2, 3), max_norm=norm / 7.0, rng=rng)  # the clip binds at every step


def test_step_1000_and_the_clip_off_without_writing_gradients():
    chunk, _ = _geometry()
    rng = np.random.default_rng(1)
    tensors = [_tensor(rng, n, grp) for n, grp in ((chunk + 5, 0), (9, 1), (1, 1))]
    _check(tensors, 2, steps=(1000,), max_norm=3.0)
    _check(tensors, 2, steps=(1000, 1001), max_norm=3.0, write=False)
    for off in (0.0, -1.0):  # max_norm <= 0: c is exactly 1, g' = g
        out = _check(tensors, 2, steps=(7,), max_norm=off)
        _assert_equal(out, tensors, keys=("g",))


@pytest.mark.parametrize("count", ["one", "cap-1", "cap", "cap+1", "2cap+1"])
def test_tensor_counts_around_the_table_capacity_in_one_and_eight_groups(count):
    chunk, cap = _geometry()
    n_t = {"one": 1, "cap-1": cap - 1, "cap": cap, "cap+1": cap + 1, "2cap+1": 2 * cap + 1}[count]
    rng = np.random.default_rng(2)
    for n_groups in (1, 8):
        if n_t == 1:
            tensors = [_tensor(rng, 6, n_groups - 1)]  # with 8 groups: seven of them without a tensor, norm 0
        else:
            # groups interleaved over the table (the kernel's slots are per group: the call orders them); group 7
            # is one tensor of one element, in the middle of the table
            groups = [i % max(1, n_groups - 1) for i in range(n_t)]
            lens = [1 + (5 * i) % 11 for i in range(n_t)]
            if n_groups == 8:
                groups[n_t // 2], lens[n_t // 2] = 7, 1
            lens[1] = chunk + 2  # one tensor of two blocks, so block and tensor numbering differ
            tensors = [_tensor(rng, n, g, misalign=(i % 5 == 3)) for i, (n, g) in enumerate(zip(lens, groups))]
        norms = em.group_norms(tensors, n_groups)
        _check(tensors, n_groups, steps=(1, 2), max_norm=float(np.median(norms[norms > 0])), rng=rng)


def test_norm_below_above_and_exactly_at_max_norm():
    rng = np.random.default_rng(3)

    def tensors():
        t = [_tensor(rng, 2, 0), _tensor(rng, 1, 0), _tensor(rng, 3, 1, zeros=True), _tensor(rng, 0, 2)]
        t[0]["g"][:] = [3.0, -4.0]
        t[1]["g"][:] = [12.0]
        return t
    for max_norm, binds in ((20.0, False), (5.0, True), (13.0, True)):  # at max_norm torch's 1e-6 still scales
        t = tensors()
        assert em.group_norms(t, 3).tolist() == [13.0, 0.0, 0.0]
        assert (em.clip_coef(13.0, max_norm) < 1) == binds
        out = _check(t, 3, steps=(1,), max_norm=max_norm)
        assert np.array_equal(_bits(out[0]["g"]), _bits(t[0]["g"])) == (not binds)


def test_equal_calls_on_real_valued_data_give_equal_bits():
    chunk, cap = _geometry()
    rng = np.random.default_rng(4)
    tensors = [_tensor(rng, n, g) for n, g in ((5 * chunk + 17, 0), (chunk, 0), (33, 1), (3 * chunk - 1, 1), (2, 0))]
    for t in tensors:
        t["g"] = rng.standard_normal(t["g"].size).astype(np.float32)
    runs = [_call(_Device(tensors), 2, step=3, max_norm=0.5) for _ in range(2)]
    (a, na), (b, nb) = runs
    _assert_equal(a, b)
    assert np.array_equal(na, nb)
    # and the emulation's float64 norm (fsum: correctly rounded) within the reordering of a float64 sum
    want = em.group_norms(tensors, 2)
    assert np.all(np.abs(na - want) <= 2.0 ** -40 * want)
    assert not np.array_equal(_bits(a[0]["p"]), _bits(tensors[0]["p"]))


def test_error_paths_return_nonzero_set_the_message_and_launch_nothing():
    from marlsc import abi
    L = abi.lib()
    rng = np.random.default_rng(5)
    tensors = [_tensor(rng, 9, 0), _tensor(rng, 4, 1)]
    dev = _Device(tensors)
    good = abi.MscAdamClipDesc(1e-3, 0.9, 0.999, 1e-8, 1.0, 1, 1)
    norms = torch.full((2,), SENTINEL, dtype=torch.float64, device="cuda")
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)

    def call(desc=good, table=dev.table, n_tensors=2, n_groups=2, ws=dev.ws):
        return L.msc_adam_clip_step(None if desc is None else C.byref(desc),
                                    None if table is None else C.c_void_p(table.ctypes.data), n_tensors, n_groups,
                                    C.c_void_p(norms.data_ptr()), None if ws is None else C.c_void_p(ws.data_ptr()), stream)

    def edited(field, value, row=0):
        t = dev.table.copy()
        t[field][row] = value
        return t
    step0 = abi.MscAdamClipDesc(1e-3, 0.9, 0.999, 1e-8, 1.0, 0, 1)
    cases = {"null desc": dict(desc=None), "null table": dict(table=None), "null workspace": dict(ws=None),
             "n_tensors 0": dict(n_tensors=0), "n_tensors -1": dict(n_tensors=-1), "n_groups 0": dict(n_groups=0),
             "group below": dict(table=edited("group", -1)), "group above": dict(table=edited("group", 2, 1)),
             "step 0": dict(desc=step0), "n negative": dict(table=edited("n", -1)),
             "null p": dict(table=edited("p", 0)), "null g": dict(table=edited("g", 0, 1)),
             "null m": dict(table=edited("m", 0)), "null v": dict(table=edited("v", 0, 1))}
    for name, kw in cases.items():
        assert call(**kw) != 0, name
        assert b"msc_adam_clip" in L.msc_last_error(), name
    with pytest.raises(RuntimeError, match="msc_adam_clip_step"):
        abi.check(call(desc=step0))
    torch.cuda.synchronize()
    _assert_equal(dev.read(), tensors, what="untouched after the refused calls")
    assert bool((norms == SENTINEL).all()) and bool((dev.ws == SENTINEL).all())
    assert L.msc_adam_clip_workspace(0, 10) == -1 and L.msc_adam_clip_workspace(1, -1) == -1
    assert L.msc_adam_clip_geometry(None, None) != 0
    # a null pointer with n = 0 is no error: the entry is skipped, the other one stepped
    t = edited("n", 0)
    t["p"][0] = 0
    assert call(table=t, n_tensors=2) == 0
    torch.cuda.synchronize()
    got = dev.read()
    _assert_equal(got[:1], tensors[:1], what="the skipped entry")
    want, _ = em.step(tensors[1:], 2, lr=1e-3, max_norm=1.0, step=1)
    _assert_equal(got[1:], want)
