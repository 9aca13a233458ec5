"""Host tests of the method that pins the running observation filter kernels (csrc/obs_filter.hip):
the float64 emulation of the three kernels (tests/meanstd_emulation.py), which the device has to equal
bit for bit (tests/test_gpu_meanstd_exact.py), against the long double reference of
oracle/meanstd_ref.py at every shape the GPU tests run, and the mutants of the emulation.

Bounds (fixed from the number formats, not from what the emulation gives):
* counts are integers below 2^53: exact;
* outputs: within 1 float32 ulp of the reference (half an ulp of it is the final rounding); the share
  that is not float32(reference) itself is printed and at most 1 %, for the emulation and for the
  sequential float64 restatement (MeanStdFilter);
* M and S, running and buffer: |value - reference| <= 4 max(e_seq, 2^-53) scale_c, with e_seq the
  largest error of the sequential restatement over the columns of the same case relative to scale_c,
  scale_c = |M_c| + std_c for M (a mean near zero still carries the rounding of its terms) and S_c for
  S. This is the rule the GRU tests use for their float32 evaluation: the segmented evaluation may
  lose a small factor against the sequential one, and never less than a few roundings of the format.
pytest -s prints the measured figures of every case (DESIGN.md section 4 records them)."""
import numpy as np
import pytest

import meanstd_emulation as EM
from meanstd_ref import LD, LongdoubleFilter, LongdoubleStat, MeanStdFilter, filter_rows, two_pass

U53 = 2.0 ** -53
_id = lambda v: "x".join(map(str, v)) if isinstance(v, tuple) else str(v)  # noqa: E731


def run_emulation(steps, C, st=None, mut=None, **kw):
    st = EM.new_state(C) if st is None else st
    outs = []
    for x, mask in steps:
        out, st = EM.emulate(st, x, mask, mut=mut, **kw)
        outs.append(out)
    return outs, st


def run_reference(steps, C, pre=None):
    f = LongdoubleFilter(C)
    if pre is not None:
        f.rs = LongdoubleStat(C, *pre)
    return [f.rows(x, mask) for x, mask in steps], f


def run_sequential(steps, C, pre=None):
    f = MeanStdFilter((C,))
    if pre is not None:
        f.rs.n, f.rs.M, f.rs.S = int(pre[0]), np.array(pre[1], np.float64), np.array(pre[2], np.float64)
    outs = [filter_rows(f, x, mask) for x, mask in steps]
    C_ = C
    st = np.zeros(4 + 4 * C_)
    st[0], st[1] = f.rs.n, f.buffer.n
    st[4:4 + C_], st[4 + C_:4 + 2 * C_], st[4 + 2 * C_:4 + 3 * C_], st[4 + 3 * C_:] = f.rs.M, f.rs.S, f.buffer.M, f.buffer.S
    return outs, st


def ulp_errors(out, ref):
    """|out - ref| in float32 ulps of ref (the spacing at float32(ref), not below the least subnormal)."""
    with np.errstate(all="ignore"):
        ulp = np.spacing(np.abs(ref.astype(np.float32))).astype(LD)
        return np.abs(out.astype(LD) - ref) / ulp


def state_errors(st, ref):
    """Per quantity (M, S, buffer M, buffer S): |value - reference| / scale_c over the columns."""
    C = (len(st) - 4) // 4
    errs = []
    for k, rs in enumerate((ref.rs, ref.buffer)):
        std = np.sqrt(np.maximum(rs.var, 0)) if rs.n > 0 else np.zeros(C, LD)
        for j, (want, scale) in enumerate(((rs.M, np.abs(rs.M) + std), (rs.S, rs.S))):
            got = st[4 + (2 * k + j) * C:4 + (2 * k + j + 1) * C].astype(LD)
            d = np.abs(got - want)
            with np.errstate(all="ignore"):
                errs.append(np.where(d == 0, LD(0), d / scale).astype(np.float64))
    return errs


def verdict(outs, st, refs, ref, e_seq):
    """What of the bounds above a result breaks: a list of words, empty when it holds them all."""
    bad = []
    if st[0] != ref.rs.n or st[1] != ref.buffer.n:
        bad.append("count")
    if max(float(ulp_errors(o, r).max()) for o, r in zip(outs, refs)) > 1.0:
        bad.append("out")
    for name, e, es in zip(("M", "S", "buffer M", "buffer S"), state_errors(st, ref), e_seq):
        if not e.max() <= 4.0 * max(es.max(), U53):
            bad.append(name)
    return bad


def check_case(name, steps, C, st0=None, pre=None):
    outs, st = run_emulation(steps, C, st0)
    refs, ref = run_reference(steps, C, pre)
    souts, sst = run_sequential(steps, C, pre)
    e_seq = state_errors(sst, ref)
    e_emu = state_errors(st, ref)
    assert st[0] == ref.rs.n and st[1] == ref.buffer.n
    worst = max(float(ulp_errors(o, r).max()) for o, r in zip(outs, refs))
    total = sum(o.size for o in outs)
    miss = sum(int((o != r.astype(np.float32)).sum()) for o, r in zip(outs, refs))
    smiss = sum(int((o != r.astype(np.float32)).sum()) for o, r in zip(souts, refs))
    last = int((outs[-1] != refs[-1].astype(np.float32)).sum())
    print(f"meanstd {name}: out {worst:.3f} ulp, not float32(ref) {miss}/{total} (last call {last}; sequential {smiss}); "
          + "; ".join(f"{q} {e.max() / U53:.2f} (seq {s.max() / U53:.2f})"
                      for q, e, s in zip(("M", "S", "bM", "bS"), e_emu, e_seq)) + " x 2^-53 scale")
    assert worst <= 1.0
    assert miss <= 0.01 * total and smiss <= 0.01 * total
    assert verdict(outs, st, refs, ref, e_seq) == []
    return outs, st


# every GPU shape at mean 2 sigma; mean 1000 sigma (cancellation in x - M) at three small shapes. Not at
# thousands of rows: M carries a rounding of 2^-53 * 1000 sigma, 1e-13 of an output, and among 10^6
# outputs some are below 1e-5, where a float32 ulp is smaller than that -- there "1 ulp of the reference"
# asks more of any float64 evaluation than its format holds (the sequential restatement misses it too).
@pytest.mark.parametrize("E,C,shift", [(E, C, 2.0) for E, C in EM.ROW_CASES + EM.COL_CASES]
                         + [(65, 70, 1000.0), (300, 70, 1000.0), (130, 272, 1000.0)], ids=lambda v: f"{v:g}")
def test_emulation_against_the_long_double_reference(E, C, shift):
    check_case(f"E={E} C={C} shift={shift:g}", EM.case_steps(E, C, shift), C)


def test_long_run_state_against_the_long_double_reference():
    st0, x = EM.long_run_case()
    C = x.shape[1]
    pre = (2 ** 30, st0[4:4 + C], st0[4 + C:4 + 2 * C])
    check_case("n=2^30 + 130 rows", [(x, None)], C, st0, pre)


def test_welford_state_equals_two_pass_statistics():
    # the reference itself: its sequential long double Welford state against a two-pass mean and centred
    # sum of squares over all pushed rows, to a few roundings of the 64-bit mantissa per pushed row
    for E, C, shift in ((300, 70, 2.0), (4097, 70, 1000.0)):
        steps = EM.case_steps(E, C, shift)
        _, ref = run_reference(steps, C)
        rows = np.concatenate([x if m is None else x[m != 0] for x, m in steps])
        n, mean, css = two_pass(rows)
        assert ref.rs.n == ref.buffer.n == n
        u = np.finfo(LD).eps
        for rs in (ref.rs, ref.buffer):
            assert np.all(np.abs(rs.M - mean) <= 4 * u * np.sqrt(LD(n)) * (np.abs(mean) + np.sqrt(css / n)))
            assert np.all(np.abs(rs.S - css) <= 4 * u * np.sqrt(LD(n)) * css * (1 + np.abs(mean) / np.sqrt(css / n)))


def test_plan_and_scratch_size():
    assert [EM.meanstd_plan(E) for E in (1, 2, 63, 64, 65, 127, 128, 129, 4096, 4097)] == [
        (1, 1), (1, 2), (1, 63), (1, 64), (2, 33), (2, 64), (2, 64), (3, 43), (64, 64), (65, 64)]
    assert 4097 - 63 * 65 == 2  # the short last segment
    assert EM.meanstd_plan(524289) == (8193, 64)
    assert EM.scratch_doubles(4097, 70) == 64 * 70 * 3 + 70 * 3 + 1


def test_masks_and_update_off_leave_what_they_must():
    E, C = 130, 70
    (x, _), (x2, _), _ = EM.case_steps(E, C)
    fresh = EM.new_state(C)
    zero = np.zeros(E, np.uint8)
    out, st = EM.emulate(fresh, x, zero)
    assert np.array_equal(EM.bits(st), EM.bits(fresh))
    assert np.array_equal(out, np.where(x > 0, 10.0, -10.0).astype(np.float32))  # x / eps, clipped
    _, warm = EM.emulate(fresh, x[:111])  # (111 m) / 111 != m for about one m in nine
    out, st = EM.emulate(warm, x2, zero)
    assert np.array_equal(EM.bits(st), EM.bits(warm))
    off, st = EM.emulate(warm, x2, update=False)
    assert np.array_equal(EM.bits(st), EM.bits(warm)) and np.array_equal(EM.bits(out), EM.bits(off))
    # merging the segments without a push as well is not the identity: (n1 * m1 + 0) / n1 != m1 (once; the
    # moved M is a fixed point of further empty merges)
    _, st = EM.emulate(warm, x2, zero, skip_empty=False)
    moved = int((EM.bits(st) != EM.bits(warm)).sum())
    print(f"meanstd: an all-zero mask with empty segments merged moves {moved} of {4 * C} statistics")
    assert moved > 0
    # a first push: (x - x) / (|x| + eps) = 0 exactly
    out, _ = EM.emulate(fresh, x[:1])
    assert not out.any() and x[:1].all()


# ---- mutants ----------------------------------------------------------------------------------------------

def _fresh_first_row_only():
    mask = np.zeros(130, np.uint8)
    mask[0] = 1
    return [(EM.case_steps(130, 70)[0][0], mask)]


MUTANT_CASES = {  # mutant -> (the listed case that sees it, its calls)
    "merge_le": ("rows E=65 C=70", lambda: EM.case_steps(65, 70)),
    "segment_ignores_mask": ("columns E=130 C=65 (second call masked)", lambda: EM.case_steps(130, 65)),
    "apply_ignores_mask": ("columns E=130 C=65 (second call masked)", lambda: EM.case_steps(130, 65)),
    "normalise_first": ("columns E=37 C=65", lambda: EM.case_steps(37, 65)),
    "var_over_n": ("columns E=37 C=65", lambda: EM.case_steps(37, 65)),
    "single_push_var_zero": ("masks: E=130 C=70, fresh state, only the first row pushed", _fresh_first_row_only),
    "buffer_skips_segment": ("rows E=65 C=70", lambda: EM.case_steps(65, 70)),
    "neighbour_fin": ("columns E=37 C=65", lambda: EM.case_steps(37, 65)),
    "race": ("columns E=37 C=65 (one column past the first wave)", lambda: EM.case_steps(37, 65)),
}


@pytest.mark.parametrize("mut", list(MUTANT_CASES))
def test_mutant_leaves_the_bound(mut):
    name, make = MUTANT_CASES[mut]
    steps = make()
    C = steps[0][0].shape[1]
    refs, ref = run_reference(steps, C)
    e_seq = state_errors(run_sequential(steps, C)[1], ref)
    outs, st = run_emulation(steps, C)
    assert verdict(outs, st, refs, ref, e_seq) == []
    mouts, mst = run_emulation(steps, C, mut=mut)
    bad = verdict(mouts, mst, refs, ref, e_seq)
    sep = max(float(e.max()) / (4.0 * max(float(s.max()), U53)) for e, s in zip(state_errors(mst, ref), e_seq))
    ulps = max(float(ulp_errors(o, r).max()) for o, r in zip(mouts, refs))
    print(f"meanstd mutant {mut} on {name}: breaks {bad}; state error {sep:.3g} x bound, out {ulps:.3g} ulp")
    assert bad
    if mut == "race":  # the wrong count reaches the buffer's M and S only, by orders of magnitude
        assert set(bad) == {"buffer M", "buffer S"} and sep >= 1e4


@pytest.mark.parametrize("E,C", [(65, 70), (300, 70), (4097, 70)], ids=lambda v: str(v))
def test_another_plan_stays_inside_the_bound_but_not_bit_equal(E, C):
    # what bit equality buys: segments of G + 1 rows are as good an evaluation (inside every bound above),
    # and only the comparison on bits tells it from the documented plan
    steps = EM.case_steps(E, C)
    refs, ref = run_reference(steps, C)
    e_seq = state_errors(run_sequential(steps, C)[1], ref)
    outs, st = run_emulation(steps, C)
    mouts, mst = run_emulation(steps, C, mut="plan_g_plus_1")
    assert verdict(mouts, mst, refs, ref, e_seq) == []
    assert not np.array_equal(EM.bits(st), EM.bits(mst))
    rel = np.abs(mst[4:] - st[4:]) / np.abs(st[4:])
    nout = sum(int((a != b).sum()) for a, b in zip(outs, mouts))
    print(f"meanstd plan G+1 at E={E}: state moves by at most {rel.max():.2e} relative, {nout} outputs differ")
    assert rel.max() < 1e-12
