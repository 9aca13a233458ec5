"""GPU tests that pin the running observation filter (msc_meanstd_filter: of_segment_kernel,
of_apply_kernel, of_commit_kernel of csrc/obs_filter.hip) to the float64 emulation of the three
kernels in tests/meanstd_emulation.py.

The library is built with -ffp-contract=off and float64 + - * / and sqrt are correctly rounded on the
host and on the device, so every comparison is on bits, of `out` and of `state`, unless a test says
otherwise. tests/test_meanstd_exact_host.py holds the emulation to the long double reference at the
same cases and shows that each mutant of it is seen. Every call goes through the C ABI into buffers
with sentinel values behind `out`, `state` and `scratch`, asserted intact after every call."""
import ctypes as C

import numpy as np
import pytest

torch = pytest.importorskip("torch")

import meanstd_emulation as EM  # noqa: E402
from marlsc import abi  # noqa: E402

pytestmark = pytest.mark.gpu
PAD = 97  # guard elements behind every buffer
S32, S64 = np.float32(-7.25), -7.25e3
_STEPS = {}


def _p(t):
    return None if t is None else C.c_void_p(t.data_ptr())


def _dev(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _steps(E, Cn, **kw):
    """A case's calls, built once and never modified."""
    key = (E, Cn) + tuple(sorted(kw.items()))
    if key not in _STEPS:
        _STEPS[key] = EM.case_steps(E, Cn, **kw)
    return _STEPS[key]


def _same(a, b):
    return np.array_equal(EM.bits(a), EM.bits(b))


class _Filter:
    """A lane state on the device behind the C ABI, every buffer guarded."""

    def __init__(self, Cn, state=None):
        self.C = Cn
        self.state = torch.full((4 + 4 * Cn + PAD,), S64, dtype=torch.float64, device="cuda")
        self.state[:4 + 4 * Cn] = _dev(EM.new_state(Cn) if state is None else state)

    def host_state(self):
        torch.cuda.synchronize()
        st = self.state.cpu().numpy()
        assert np.all(st[4 + 4 * self.C:] == S64), "a write behind state"
        return st[:4 + 4 * self.C].copy()

    def call(self, x, mask=None, update=True, clip=EM.CLIP, eps=EM.EPS, inplace=True, null_scratch=False):
        """-> out [E, C] float32 (numpy). Separate `out`: obs asserted bit-unchanged."""
        E, Cn = x.shape
        assert Cn == self.C
        buf = torch.full((E * Cn + PAD,), float(S32), device="cuda")
        buf[:E * Cn] = _dev(x).reshape(-1)
        obs = buf if inplace else _dev(x)
        n_s = int(abi.lib().msc_meanstd_scratch_doubles(E, Cn))
        assert n_s == EM.scratch_doubles(E, Cn)
        scratch = None if null_scratch else torch.full((n_s + PAD,), S64, dtype=torch.float64, device="cuda")
        m = None if mask is None else _dev(np.asarray(mask, np.uint8))
        abi.check(abi.lib().msc_meanstd_filter(_p(obs), _p(buf), E, Cn, _p(m), 1 if update else 0, _p(self.state),
                                               _p(scratch), clip, eps, None))
        torch.cuda.synchronize()
        out = buf.cpu().numpy()
        assert np.all(out[E * Cn:] == S32), "a write behind out"
        if scratch is not None:
            assert np.all(scratch[n_s:].cpu().numpy() == S64), "a write behind scratch"
        if not inplace:
            assert _same(obs.cpu().numpy(), x), "obs modified"
        self.host_state()
        return out[:E * Cn].reshape(E, Cn).copy()


def _run_exact(steps, Cn, state=None, **kw):
    """Every call of a case against the emulation on bits: out and the whole state after each call."""
    st = EM.new_state(Cn) if state is None else state
    f = _Filter(Cn, st)
    for k, (x, mask) in enumerate(steps):
        want, st = EM.emulate(st, x, mask, **{a: b for a, b in kw.items() if a in ("clip", "eps", "update")})
        got = f.call(x, mask, **kw)
        gst = f.host_state()
        assert _same(gst, st), f"call {k}: state differs at {np.flatnonzero(EM.bits(gst) != EM.bits(st))[:8]}"
        bad = np.argwhere(EM.bits(got) != EM.bits(want))
        assert len(bad) == 0, f"call {k}: {len(bad)} of {got.size} outputs differ, first at {bad[:4].tolist()}"
    return st


# ---- shapes ---------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("E,Cn", EM.ROW_CASES, ids=lambda v: str(v))
def test_rows_across_the_segment_plan(E, Cn):
    # E = 64 -> 65: G 1 -> 2, P 64 -> 33; 4097: G = 65, P = 64, a last segment of 2 rows. Three calls,
    # the second masked with mask[0] = 0; the second and third start from a non-zero state.
    _run_exact(_steps(E, Cn), Cn)


@pytest.mark.parametrize("E,Cn", EM.COL_CASES, ids=lambda v: str(v))
def test_columns_across_waves_and_blocks(E, Cn):
    # more than one wave (C > 64), more than one commit block (C > 256), P * C no multiple of 256
    # (37 * 63, 43 * 65 ...); 272 is the bench shape's W * L
    _run_exact(_steps(E, Cn), Cn, inplace=(Cn % 2 == 0))


def test_shifted_data():
    # a mean of 1000 sigma: the cancellation in x - M
    _run_exact(_steps(130, 272, shift=1000.0), 272)


def test_the_buffer_count_is_read_before_it_is_written():
    # The regression case of the commit race: 2^20 columns are 4,096 blocks of of_commit_kernel, more than
    # are resident at once, so blocks that start late read state[1] after thread 0 has written the new
    # count, and would merge their columns' buffer M and S from the wrong n1. Buffer statistics of every
    # column after a first call on a fresh state and after a second call. (With the read of state[1]
    # put back this case still passed on the MI355X: the read is a scalar load and the scalar caches keep
    # the line they filled before the store -- DESIGN.md section 4. A late read that does see the store
    # is the emulation's `race` mutant.)
    E, Cn = 2, 1 << 20
    rng = np.random.default_rng(20)
    st = EM.new_state(Cn)
    f = _Filter(Cn)
    for k in range(2):
        x = rng.normal(2.0, 3.0, (E, Cn)).astype(np.float32)
        _, st = EM.emulate(st, x)
        f.call(x)
        gst = f.host_state()
        assert gst[0] == st[0] and gst[1] == st[1] == 2 * (k + 1)
        wrong = np.flatnonzero(EM.bits(gst[4 + 2 * Cn:]) != EM.bits(st[4 + 2 * Cn:])) % Cn
        assert len(wrong) == 0, f"call {k}: buffer M / S of {len(wrong)} columns differ, first column {wrong.min()}"
        assert _same(gst, st)


# ---- masks ------------------------------------------------------------------------------------------------------

def _warm(Cn=70, rows=111):
    x = _steps(130, Cn)[0][0][:rows]
    return x, EM.emulate(EM.new_state(Cn), x)[1]


@pytest.mark.parametrize("E", [1, 65, 130, 4097])
def test_an_all_zero_mask_pushes_nothing(E):
    # the collector's apply(final_obs, mask = trunc) on a step that truncates nothing: the state stays as
    # it is on bits, fresh or warm (111 pushes: (111 m) / 111 != m for one m in nine, so merging the
    # empty segments would show), and the rows are still normalised
    Cn = 70
    x = _steps(E, Cn)[0][0]
    zero = np.zeros(E, np.uint8)
    for st in (EM.new_state(Cn), _warm()[1]):
        f = _Filter(Cn, st)
        got = f.call(x, zero)
        assert _same(f.host_state(), st)
        assert _same(got, EM.emulate(st, x, zero)[0]) and _same(got, EM.emulate(st, x, update=False)[0])
    assert np.abs(got).max() > 0.5


def test_masked_first_row_whole_segments_and_last_row_only():
    E, Cn = 130, 70  # G = 3, P = 44
    x = _steps(E, Cn)[0][0]
    rng = np.random.default_rng(5)
    first = np.ones(E, np.uint8)
    first[0] = 0
    segs = np.ones(E, np.uint8)
    segs[0:9] = 0  # segments 0-2
    segs[60:66] = 0  # segments 20, 21
    segs[129:] = 0  # the last, short segment
    last = np.zeros(E, np.uint8)
    last[-1] = 1
    only_first = np.zeros(E, np.uint8)  # on a fresh state every later row meets n = 1: var = M^2
    only_first[0] = 1
    half = (rng.uniform(size=E) < 0.5).astype(np.uint8)
    for mask in (first, segs, last, only_first, half):
        for st in (EM.new_state(Cn), _warm()[1]):
            _run_exact([(x, mask)], Cn, st)
    # rows with mask 0 are still normalised: with the statistics up to them
    st = _warm()[1]
    got = _Filter(Cn, st).call(x, last)
    assert _same(got[:-1], EM.emulate(st, x[:-1], update=False)[0])


# ---- fresh state, aliasing, update = 0, parameters ----------------------------------------------------------

def test_fresh_state():
    Cn = 70
    x = _steps(130, Cn)[0][0]
    fresh = EM.new_state(Cn)
    # update = 0 with n = 0: var = M^2 = 0, x / eps clipped
    f = _Filter(Cn)
    got = f.call(x, update=False, null_scratch=True)
    assert _same(f.host_state(), fresh) and _same(got, EM.emulate(fresh, x, update=False)[0])
    assert np.array_equal(got, np.where(x > 0, 10.0, -10.0).astype(np.float32))
    # a first push: (x - x) / (|x| + eps) = 0 exactly where x != 0
    f = _Filter(Cn)
    got = f.call(x[:1])
    assert x[:1].all() and not got.any()
    assert _same(f.host_state(), EM.emulate(fresh, x[:1])[1])


@pytest.mark.parametrize("inplace", [True, False])
@pytest.mark.parametrize("E", [37, 4097])
def test_in_place_and_separate_out(E, inplace):
    _run_exact(_steps(E, 70), 70, inplace=inplace)


@pytest.mark.parametrize("E", [1, 130, 4097])
def test_update_off_with_a_null_scratch_leaves_the_state(E):
    Cn = 70
    x = _steps(E, Cn)[1][0]
    for st in (_warm()[1], _warm(rows=1)[1]):  # n = 1: the single-push variance M^2
        f = _Filter(Cn, st)
        got = f.call(x, update=False, null_scratch=True, inplace=False)
        assert _same(f.host_state(), st)
        assert _same(got, EM.emulate(st, x, update=False)[0])


def test_clip_and_eps():
    E, Cn = 130, 70
    steps = [(x.copy(), m) for x, m in _steps(E, Cn)]
    steps[1][0][0] *= np.float32(1000.0)  # outliers in a row that is normalised and not pushed
    _run_exact(steps, Cn, clip=0.5)
    _run_exact(steps, Cn, clip=0.0)
    st, top = EM.new_state(Cn), 0.0
    for x, m in steps:
        out, st = EM.emulate(st, x, m, clip=0.0)
        top = max(top, float(np.abs(out).max()))
    assert top > 1000.0  # no clipping: values far beyond 10 appear
    # eps = 0 on constant columns: 0 / 0 and x / 0 exactly as float64 arithmetic gives them
    x = steps[0][0].copy()
    x[:, 3], x[:, 7], x[1:, 9] = 2.5, 0.0, x[0, 9]
    for clip in (0.0, 10.0):
        st = EM.new_state(Cn)
        f = _Filter(Cn)
        for k in range(2):
            want, st = EM.emulate(st, x, clip=clip, eps=0.0)
            got = f.call(x, clip=clip, eps=0.0)
            # a first push is 0 / |x|; from the second row on S = 0: 0 / 0. A column of zeros: 0 / 0 at once
            assert np.isnan(want[1 - k:, 3]).all() and np.isnan(want[:, 7]).all() and np.isnan(want[1 - k:, 9]).all()
            assert want[0, 3] == 0 or k
            assert np.array_equal(EM.nan_bits(got), EM.nan_bits(want))
            assert _same(f.host_state(), st)
        ev = f.call(x + np.float32(1.0), update=False, clip=clip, eps=0.0, null_scratch=True)
        want = EM.emulate(st, x + np.float32(1.0), update=False, clip=clip, eps=0.0)[0]
        assert np.isinf(want[:, 3]).all() if clip == 0.0 else np.all(want[:, 3] == 10.0)
        assert np.array_equal(EM.nan_bits(ev), EM.nan_bits(want))


# ---- guards -----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("E", [1, 65, 4097])
def test_nothing_is_written_behind_out_state_or_scratch(E):
    # _Filter.call asserts the sentinels behind all three buffers; the scratch size is the documented plan's
    # [P][C][3] segments + [C][3] final statistics + the buffer count before the call
    for Cn in (70, 257):
        G, P = EM.meanstd_plan(E)
        assert int(abi.lib().msc_meanstd_scratch_doubles(E, Cn)) == P * Cn * 3 + Cn * 3 + 1
        x = _steps(E, 257)[0][0][:, :Cn]
        f = _Filter(Cn)
        f.call(np.ascontiguousarray(x))
        f.call(np.ascontiguousarray(x), np.arange(E) % 3 == 1, inplace=False)
    assert abi.lib().msc_meanstd_scratch_doubles(0, 70) == -1 and abi.lib().msc_meanstd_scratch_doubles(5, 0) == -1


# ---- long run, non-finite ---------------------------------------------------------------------------------

def test_after_two_to_the_thirty_pushes():
    # n = 2^30: delta / n and (n - 1) / n at a large count. On bits against the emulation, which the host
    # test holds to the long double reference under its bound; here the same bound on the device's state.
    from meanstd_ref import LongdoubleFilter, LongdoubleStat
    from test_meanstd_exact_host import run_sequential, state_errors, ulp_errors, verdict
    st0, x = EM.long_run_case()
    Cn = x.shape[1]
    _run_exact([(x, None)], Cn, st0)
    f = _Filter(Cn, st0)
    got = f.call(x)
    pre = (2 ** 30, st0[4:4 + Cn], st0[4 + Cn:4 + 2 * Cn])
    ref = LongdoubleFilter(Cn)
    ref.rs = LongdoubleStat(Cn, *pre)
    want = ref.rows(x)
    e_seq = state_errors(run_sequential([(x, None)], Cn, pre)[1], ref)
    assert f.host_state()[0] == 2 ** 30 + 130
    assert verdict([got], f.host_state(), [want], ref, e_seq) == []
    print(f"meanstd long run: out {float(ulp_errors(got, want).max()):.3f} ulp of the long double reference")


def test_non_finite_observations_stay_in_their_column():
    E, Cn = 130, 70
    steps = _steps(E, Cn)
    x = steps[0][0].copy()
    x[40, 11], x[77, 11] = np.nan, np.inf
    x[5, 30] = -np.inf
    st, clean = EM.new_state(Cn), EM.new_state(Cn)
    f = _Filter(Cn)
    keep = np.ones(Cn, bool)
    keep[[11, 30]] = False
    for xs, m in [(x, None)] + steps[1:]:
        want, st = EM.emulate(st, xs, m)
        cw, clean = EM.emulate(clean, steps[0][0] if xs is x else xs, m)
        got = f.call(xs, m)
        gst = f.host_state()
        assert np.array_equal(EM.nan_bits(got), EM.nan_bits(want))  # NaN where the emulation has NaN
        assert np.array_equal(EM.nan_bits(gst), EM.nan_bits(st))
        # every other column as if nothing had happened
        assert _same(got[:, keep], cw[:, keep])
        assert _same(gst[4:].reshape(4, Cn)[:, keep], clean[4:].reshape(4, Cn)[:, keep])
    assert np.isnan(st[4 + 11]) and np.isnan(want[:, 11]).all() and np.isnan(want[:, 30]).all()


# ---- refusals -------------------------------------------------------------------------------------------------

def test_refusals_touch_nothing():
    E, Cn = 37, 70
    x = _steps(E, Cn)[0][0]
    st = _warm()[1]
    state, obs = _dev(st), _dev(x)
    out = torch.full((E, Cn), float(S32), device="cuda")
    scratch = torch.zeros(EM.scratch_doubles(E, Cn), dtype=torch.float64, device="cuda")
    nan = float("nan")
    ok = dict(obs=obs, out=out, E=E, C=Cn, update=1, state=state, scratch=scratch, clip=10.0, eps=1e-6)
    bad = [dict(obs=None), dict(out=None), dict(state=None), dict(scratch=None), dict(E=0), dict(E=-3), dict(C=0),
           dict(C=-1), dict(eps=-1e-6), dict(eps=nan), dict(clip=-1.0), dict(clip=nan)]
    for change in bad:
        a = dict(ok, **change)
        rc = abi.lib().msc_meanstd_filter(_p(a["obs"]), _p(a["out"]), a["E"], a["C"], None, a["update"], _p(a["state"]),
                                          _p(a["scratch"]), a["clip"], a["eps"], None)
        torch.cuda.synchronize()
        assert rc != 0, change
        assert abi.lib().msc_last_error()
        assert torch.all(out == float(S32)) and _same(state.cpu().numpy(), st) and _same(obs.cpu().numpy(), x), change
    # legal: no scratch without update
    assert abi.lib().msc_meanstd_filter(_p(obs), _p(out), E, Cn, None, 0, _p(state), None, 10.0, 1e-6, None) == 0
    torch.cuda.synchronize()
    assert _same(out.cpu().numpy(), EM.emulate(st, x, update=False)[0]) and _same(state.cpu().numpy(), st)


# ---- more than 2^31 elements ------------------------------------------------------------------------------

def test_more_than_2_31_elements_in_place():
    # obs of 524,289 x 4,096 = 2^31 + 4,096 floats (8 GiB), in place: G = 8,193, P = 64, a last segment of
    # 8,130 rows. Eight spread columns (the last one included, so the last row's last element, index
    # 2^31 + 4,095) against the emulation restricted to those columns; row 0 and the last row whole.
    free, _ = torch.cuda.mem_get_info()
    if free < 10 << 30:
        pytest.skip(f"{free >> 30} GiB free: the case needs 10 GiB")
    E, Cn = 524289, 4096
    assert E * Cn > 2 ** 31 and EM.meanstd_plan(E) == (8193, 64)
    g = torch.Generator(device="cuda").manual_seed(31)
    x = torch.empty((E, Cn), device="cuda")
    step = 1 << 15
    for a in range(0, E, step):
        x[a:a + step].normal_(2.0, 3.0, generator=g)
    cols = torch.tensor([0, 1, 63, 64, 257, 2048, 4094, 4095], device="cuda")
    xs = x[:, cols].cpu().numpy()
    ends = x[[0, E - 1]].cpu().numpy()
    mask = (torch.arange(E, device="cuda") % 7 != 3).to(torch.uint8)
    state = torch.zeros(4 + 4 * Cn, dtype=torch.float64, device="cuda")
    scratch = torch.empty(EM.scratch_doubles(E, Cn), dtype=torch.float64, device="cuda")
    abi.check(abi.lib().msc_meanstd_filter(_p(x), _p(x), E, Cn, _p(mask), 1, _p(state), _p(scratch), 10.0, 1e-6, None))
    torch.cuda.synchronize()
    got, gends, gst = x[:, cols].cpu().numpy(), x[[0, E - 1]].cpu().numpy(), state.cpu().numpy()
    del x
    torch.cuda.empty_cache()
    want, st = EM.emulate(EM.new_state(8), xs, mask.cpu().numpy())
    assert _same(got, want)
    c = cols.cpu().numpy()
    assert gst[0] == st[0] and gst[1] == st[1]
    assert _same(gst[4:].reshape(4, Cn)[:, c], st[4:].reshape(4, 8))
    # row 0 (a first push: zeros) and the last row from the device's own final statistics
    assert not gends[0].any()
    M, S = gst[4:4 + Cn], gst[4 + Cn:4 + 2 * Cn]
    y = (ends[1].astype(np.float64) - M) / (np.sqrt(S / (gst[0] - 1.0)) + 1e-6)
    assert _same(gends[1], np.clip(y, -10.0, 10.0).astype(np.float32))


# ---- the collector's push order ---------------------------------------------------------------------------

@pytest.mark.parametrize("n_lanes", [1, 2])
def test_collector_pushes_in_the_documented_order(n_lanes):
    # RolloutCollector(obs_filter="meanstd") at the 8 x 64 x 5 synthetic shape, 96 envs, T = 9, episodes of
    # 5 steps, two collects (a sync in between), one lane or two of 48. The stored clamped actions replayed
    # on twin envs with the same seeds give the raw observations, final observations and truncations;
    # the emulation is fed in the documented order: the reset observation first, then per step every new
    # observation, then the final observations masked by trunc; one state per lane, the lanes synchronised
    # in lane order through merge_stats after each collect. The stored (filtered) observations, every lane
    # state and the driver's statistics have to match on bits.
    from marlsc import make_synthetic_env_config
    from marlsc.rollout import ActorCritic, RolloutCollector, RolloutConfig
    from marlsc.spec import EnvSpec
    from marlsc.vec_env import VecInventoryEnv
    cfg = make_synthetic_env_config(8, 64, 5, episode_length=5)
    spec = EnvSpec.from_config(cfg, {"include_warehouse_id": True})
    E, T = 96, 9
    n = E // n_lanes

    def lanes():
        out = [VecInventoryEnv(None, n, spec=spec, device=0, base_seed=77, env_index_offset=j * n) for j in range(n_lanes)]
        return out

    envs, twins = lanes(), lanes()
    for e in envs:
        e.reset()
    torch.manual_seed(0)
    m = ActorCritic(spec.local_obs_dim, spec.local_obs_dim * spec.W, spec.K, RolloutConfig()).cuda()
    col = RolloutCollector(envs if n_lanes > 1 else envs[0], m, T, seed=3, obs_filter="meanstd")
    Cn = spec.W * spec.local_obs_dim
    states = [EM.new_state(Cn) for _ in range(n_lanes)]
    driver = np.zeros(1 + 2 * Cn)
    raw = [tw.reset().cpu().numpy().reshape(n, Cn) for tw in twins]
    before_sync, sync = [], col.obs_filter.sync

    def recording_sync(group=None):
        torch.cuda.synchronize()
        before_sync.append([s.cpu().numpy() for s in col.obs_filter.lanes])
        sync(group)

    col.obs_filter.sync = recording_sync
    cur = [None] * n_lanes
    pushes = 0
    for it in range(2):
        col.collect(normalize=False)
        torch.cuda.synchronize()
        acts = col.actions.clamp(-1.0, 1.0)
        want = np.empty((T, E, Cn), np.float32)
        for j, tw in enumerate(twins):
            sl = slice(j * n, (j + 1) * n)
            if it == 0:  # the reset observation
                cur[j], states[j] = EM.emulate(states[j], raw[j])
                pushes += n
            for t in range(T):
                want[t, sl] = cur[j]
                may_end = tw.may_truncate()
                obs, _, trunc, final = tw.step(acts[t, sl].contiguous())
                torch.cuda.synchronize()
                cur[j], states[j] = EM.emulate(states[j], obs.cpu().numpy().reshape(n, Cn))
                pushes += n
                if may_end:
                    tr = trunc.cpu().numpy()
                    _, states[j] = EM.emulate(states[j], final.cpu().numpy().reshape(n, Cn), tr)
                    pushes += int(tr.sum())
        assert _same(col.obs.cpu().numpy().reshape(T, E, Cn), want), f"collect {it}: stored observations"
        for j in range(n_lanes):  # the lane states as the steps left them, then through the sync
            assert _same(before_sync[it][j], states[j]), f"collect {it}: lane {j} before the sync"
        for j in range(n_lanes):
            driver = EM.merge_packed(driver, EM.lane_buffer(states[j]))
        states = [EM.lane_from_driver(driver) for _ in range(n_lanes)]
        assert driver[0] == pushes and col.obs_filter.count == pushes
        assert _same(col.obs_filter.driver.cpu().numpy(), driver), f"collect {it}: driver"
        for j in range(n_lanes):
            assert _same(col.obs_filter.lanes[j].cpu().numpy(), states[j]), f"collect {it}: lane {j}"
    assert pushes > 2 * T * E + E  # final observations of truncated episodes were pushed
    for e in envs + twins:
        e.close()
