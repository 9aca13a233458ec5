"""CPU tests of the create-time kernel plan (csrc/env_plan.hpp through msc_env_plan): which kernels,
forms and buffers a handle gets. Results are identical under every choice, so no parity test can see a
wrong default; these pin the defaults at the shapes bench.py runs, both sides of every threshold, the
overrides the GPU suite forces, the rejections and the byte counts. No GPU call is made."""
import math
from pathlib import Path

import numpy as np
import pytest

from marlsc import EnvSpec, load_environment_config, make_synthetic_env_config
from marlsc.vec_env import PLAN_KEYS, plan

REPO = Path(__file__).resolve().parents[1]
KNOBS = ("MSC_DEMAND_UNI", "MSC_DEMAND_IMPL", "MSC_OBS_STAGE", "MSC_OBS_RING_REG", "MSC_ALLOC_IMPL", "MSC_ALLOC_LPE",
         "MSC_ALLOC_SORT", "MSC_FUSE_C", "MSC_FUSE_A", "MSC_STEP_C_FORM", "MSC_AL_PRIO_SPLIT", "MSC_SC_TAB", "MSC_SB_GW",
         "MSC_SB_TAB", "MSC_SCAN_DEFER", "MSC_EA", "MSC_EA_SLOTS", "MSC_EA_MEM_FRAC", "MSC_EA_BATCH", "MSC_EA_CHUNK",
         "MSC_CHAIN_PRIO", "MSC_PIPELINE", "MSC_EV_SCOPE", "MSC_EV_ELIDE", "MSC_EA_PRIO")
WID = {"include_warehouse_id": True}
LANE, GROUP, SCAN = 0, 1, 2


@pytest.fixture(autouse=True)
def no_knobs(monkeypatch):
    for k in KNOBS:
        monkeypatch.delenv(k, raising=False)


def _c1(**kw):
    return EnvSpec.from_config(make_synthetic_env_config(2, 4, 2, **kw), WID)


def _arena_bytes(W, K, RING, E, stochastic=False):
    """The 22 fields of the state arena (env.hpp EnvState, in arena_layout's order), each rounded up to 256 bytes."""
    WK = W * K
    sizes = [4 * WK * E, 4 * WK * RING * E, WK * RING * E if stochastic else 1, 4 * 5 * WK * E, 4 * WK * E, 4 * WK * E,
             8 * 8 * E, 4 * 4 * E, 8 * 4 * E, 4 * 2 * E] + [4 * E] * 6 + [4 * 4] + [4 * WK * E] * 2 + [8 * W * E] * 3
    assert len(sizes) == 22
    return sum((s + 255) // 256 * 256 for s in sizes)


def _order_cap(lam_sum):
    return math.ceil(lam_sum + 12.0 * math.sqrt(lam_sum + 1.0) + 64.0)  # 12-sigma margin + 64


def _order_bytes(K, lam_sum, E):
    nv = (1 + K + 7) // 8  # uint4 words per record: region + K 16-bit quantities
    return (16 * nv * _order_cap(lam_sum) * E + 4 * E + 255) // 256 * 256


def _c5_spec():
    from marlsc.synthetic import make_synthetic_trace
    cfg = make_synthetic_env_config(16, 256, 5)
    cfg["components"]["demand_sampler"] = {"type": "empirical", "params": None}
    meta = dict(WID, demand_trace=make_synthetic_trace(256, 5, 300, orders_per_step=(200, 1000), seed=0))
    nf = EnvSpec.from_config(cfg, meta).n_features
    g = np.random.default_rng(21)
    meta.update(obs_normalization="meanstd_custom",
                obs_stats=(g.uniform(-2, 30, nf).astype(np.float32), g.uniform(0.5, 12, nf).astype(np.float32)))
    return EnvSpec.from_config(cfg, meta)


# ---- the shapes bench.py runs: n_cus = 256, every create knob unset --------------------------------
# The first nine values (msc_env_kernel_choice's) are the parent commit's kernel_choice() on an MI355X
# (profiles/env_plan/gpu_dump_parent.txt); the rest follow the rules named beside them.
def _c1_yaml():
    cfg = load_environment_config(str(REPO / "config_files/environments/env_c1_2wh4r2sku.yaml"), allow_nr_ne_nw=True)
    return EnvSpec.from_config(cfg, WID, allow_nr_ne_nw=True)


def _c23():
    return EnvSpec.from_config(make_synthetic_env_config(8, 64, 5), WID)


def test_bench_shape_c1_128():
    got = plan(_c1_yaml(), 128)
    assert got == dict(
        alloc=SCAN, alloc_sort=0, fuse_a=1, fuse_c=1, group_tables_lds=1, group_width=0, ea_slots=16, demand_impl=9,
        demand_uni=1,
        obs_stage=0,        # 64 x (2 x 13 | 1) floats fit 80 KB -> 2 phases per step, but off while EA is on
        obs_ring_reg=1,     # below 16,384 envs
        alloc_lpe=0, sort_shift=0,  # order_cap < 1,024 buckets
        scan_defer=1, sc_tab=1, sc_form=5, al_psplit=14,
        demand_ptrs=0,      # every rate < 10
        order_cap=130,      # ceil(16 + 12 sqrt(17) + 64)
        ring=4,             # lead time 3 + 1
        ea_cap=2145,        # ceil(1600 + 12 sqrt(1601) + 64) records per episode
        ea_batch=8,         # slots / 2 at <= 8,192 envs
        ea_chunk=50, pipeline=1,
        arena_bytes=53760, order_bytes=266752)
    assert got["arena_bytes"] == _arena_bytes(2, 2, 4, 128) and got["order_bytes"] == _order_bytes(2, 16.0, 128)
    assert tuple(got) == PLAN_KEYS


def test_bench_shape_c2_4096():
    assert plan(_c23(), 4096) == dict(
        alloc=SCAN, alloc_sort=0, fuse_a=1, fuse_c=1, group_tables_lds=1, group_width=0, ea_slots=16, demand_impl=9,
        demand_uni=1,
        obs_stage=0,        # 64 x (8 x 34 | 1) floats = 69,888 B fit -> 2 phases per step, off while EA is on
        obs_ring_reg=1, alloc_lpe=0, sort_shift=0, scan_defer=1, sc_tab=1, sc_form=5, al_psplit=14, demand_ptrs=0,
        order_cap=513,      # ceil(256 + 12 sqrt(257) + 64)
        ring=4,
        ea_cap=27585,       # ceil(25600 + 12 sqrt(25601) + 64)
        ea_batch=8, ea_chunk=50, pipeline=1,
        arena_bytes=_arena_bytes(8, 5, 4, 4096), order_bytes=_order_bytes(5, 256.0, 4096))


def test_bench_shape_c3_32768():
    want = dict(
        alloc=LANE, alloc_sort=0, fuse_a=0, fuse_c=0, group_tables_lds=1, group_width=0, ea_slots=0, demand_impl=9,
        demand_uni=1,
        obs_stage=2,        # fits, two phases; no EA above 8,192 envs
        obs_ring_reg=0,     # off from 16,384 envs
        alloc_lpe=0, sort_shift=0, scan_defer=1, sc_tab=1, sc_form=5, al_psplit=14, demand_ptrs=0, order_cap=513, ring=4,
        ea_cap=0, ea_batch=1, ea_chunk=50,  # (a handle's values without EA)
        pipeline=1,
        arena_bytes=_arena_bytes(8, 5, 4, 32768), order_bytes=_order_bytes(5, 256.0, 32768))
    assert plan(_c23(), 32768) == want
    # as bench.py creates it for its steady-state line (episode_ahead=16): EA wanted whatever the env count,
    # a quarter of the slots per refill and whole-episode generation launches above 8,192 envs
    want.update(ea_slots=16, obs_stage=0, ea_cap=27585, ea_batch=4, ea_chunk=100)
    assert plan(_c23(), 32768, episode_ahead=16) == want


def test_bench_shape_c5_8192():
    spec = _c5_spec()
    counts = np.diff(spec.trace["offsets"])
    shift = 0
    while (int(counts.max()) >> shift) >= 1024:  # 1,024 counting-sort buckets over the busiest trace row
        shift += 1
    assert plan(spec, 8192) == dict(
        alloc=GROUP, alloc_sort=1, fuse_a=0, fuse_c=1,
        group_tables_lds=1,  # 66,560 B of tables + 32 KB of windows: one 8-wave block per CU (256 blocks, 256 CUs)
        group_width=16, ea_slots=0, demand_impl=9, demand_uni=0,
        obs_stage=0,         # 64 x (16 x 42 | 1) floats = 172,288 B do not fit 80 KB
        obs_ring_reg=1, alloc_lpe=0, sort_shift=shift, scan_defer=1, sc_tab=1, sc_form=5, al_psplit=14, demand_ptrs=0,
        order_cap=1, ring=4, ea_cap=0, ea_batch=1, ea_chunk=50,
        pipeline=0,          # no demand kernel to pipeline
        arena_bytes=_arena_bytes(16, 5, 4, 8192), order_bytes=0)
    # the tables stop fitting when a CU has to hold two blocks
    assert plan(spec, 8192, n_cus=128)["group_tables_lds"] == 0
    assert plan(spec, 8193)["group_tables_lds"] == 0


# ---- both sides of every threshold -----------------------------------------------------------------
def test_thresholds_in_the_env_count():
    spec = _c1()
    assert [plan(spec, E)["ea_slots"] for E in (8192, 8193)] == [16, 0]
    assert [plan(spec, E)["obs_stage"] for E in (8192, 8193)] == [0, 2]
    lo, hi = plan(spec, 16383), plan(spec, 16384)
    assert (lo["alloc"], lo["obs_ring_reg"], lo["fuse_c"], lo["fuse_a"]) == (SCAN, 1, 1, 1)
    assert (hi["alloc"], hi["obs_ring_reg"], hi["fuse_c"], hi["fuse_a"]) == (LANE, 0, 0, 0)


@pytest.mark.parametrize("W,K,alloc,gw,fuse_c", [(8, 6, SCAN, 0, 1), (9, 6, GROUP, 16, 1), (8, 7, GROUP, 8, 1)])
def test_thresholds_of_the_scan_allocator(W, K, alloc, gw, fuse_c):
    got = plan(EnvSpec.from_config(make_synthetic_env_config(W, 16, K), WID), 128)
    assert (got["alloc"], got["group_width"], got["fuse_c"], got["fuse_a"]) == (alloc, gw, fuse_c, int(alloc == SCAN))


def test_scan_allocator_forced_beyond_its_default(monkeypatch):
    monkeypatch.setenv("MSC_ALLOC_IMPL", "scan")
    w9 = plan(EnvSpec.from_config(make_synthetic_env_config(9, 16, 6), WID), 128)
    assert (w9["alloc"], w9["fuse_c"], w9["fuse_a"]) == (SCAN, 0, 0)  # runs 9-16 warehouses, fuses phase C up to 8
    k7 = plan(EnvSpec.from_config(make_synthetic_env_config(8, 16, 7), WID), 128)
    assert k7["alloc"] == GROUP  # no scan instantiation above 6 SKUs: the group kernel
    big = plan(_c1(), 32768)
    assert big["alloc"] == SCAN  # (and it overrides the lane default)


def test_thresholds_in_the_lead_times():
    r4, r5 = plan(_c1(lead_time=3), 128), plan(_c1(lead_time=4), 128)
    assert (r4["ring"], r4["fuse_c"], r4["fuse_a"]) == (4, 1, 1)
    assert (r5["ring"], r5["alloc"], r5["fuse_c"], r5["fuse_a"]) == (5, SCAN, 0, 0)
    spec = _c1()
    spec.lead_type, spec.max_deviation, spec.max_dev_per_sku = "stochastic", np.zeros(1, np.int32), False
    st = plan(spec, 128)
    assert (st["ring"], st["fuse_c"], st["fuse_a"]) == (4, 1, 0)  # phase A draws lead times: stays in step_a
    assert st["arena_bytes"] == _arena_bytes(2, 2, 4, 128, stochastic=True)


def test_thresholds_in_the_rates():
    assert plan(_c1(lambda_quantity=9.99), 128)["demand_ptrs"] == 0
    assert plan(_c1(lambda_quantity=10.0), 128)["demand_ptrs"] == 1
    assert plan(_c1(lambda_orders=10.0), 128)["demand_ptrs"] == 1
    spec = _c1()
    assert plan(spec, 128)["demand_uni"] == 1
    spec.lambda_orders[3] = 4.5
    assert plan(spec, 128)["demand_uni"] == 0
    spec = _c1()
    spec.lambda_quantity[1, 0] = 5.5
    assert plan(spec, 128)["demand_uni"] == 0


# ---- overrides: what the GPU suite forces (_set_alloc), and the remaining selection knobs ------------
@pytest.mark.parametrize("param,want", [
    ("lane", dict(alloc=LANE, alloc_lpe=0, fuse_c=0, fuse_a=0, ea_slots=0, obs_ring_reg=0, obs_stage=2)),
    ("lane2", dict(alloc=LANE, alloc_lpe=2, ea_slots=0, obs_ring_reg=0)),
    ("lane4", dict(alloc=LANE, alloc_lpe=4, ea_slots=0, obs_ring_reg=0)),
    # (MSC_OBS_STAGE=1: one phase, and kept with EA on)
    ("group", dict(alloc=GROUP, alloc_sort=0, fuse_c=1, fuse_a=0, group_width=2, ea_slots=16, obs_ring_reg=1, obs_stage=1)),
    ("group_sorted", dict(alloc=GROUP, alloc_sort=1, fuse_c=1)),
    ("group_nofc", dict(alloc=GROUP, fuse_c=0, fuse_a=0)),
    ("group_unsorted_ea1", dict(alloc=GROUP, alloc_sort=0, ea_slots=16)),
    ("scan", dict(alloc=SCAN, fuse_c=1, fuse_a=1, ea_slots=16, obs_stage=0, obs_ring_reg=1, group_width=0)),
    ("scan_ea0", dict(alloc=SCAN, fuse_c=1, fuse_a=1, ea_slots=0, obs_stage=2, ea_batch=1)),
    ("scan_nofc", dict(alloc=SCAN, fuse_c=0, fuse_a=0)),
    ("scan_nofa", dict(alloc=SCAN, fuse_c=1, fuse_a=0)),
])
def test_overrides_of_the_gpu_suite(monkeypatch, param, want):
    from test_gpu_parity import _set_alloc
    _set_alloc(monkeypatch, param)
    got = plan(_c1(), 300)
    assert {k: got[k] for k in want} == want


def test_overrides_of_the_other_selection_knobs(monkeypatch):
    spec = _c1()
    monkeypatch.setenv("MSC_ALLOC_IMPL", "group")
    for v, gw in (("16", 16), ("32", 32), ("4", 4), ("5", 2), ("1", 2)):  # only 4, 8, 16, 32, and only wider
        monkeypatch.setenv("MSC_SB_GW", v)
        assert plan(spec, 300)["group_width"] == gw
    monkeypatch.delenv("MSC_SB_GW")
    assert plan(spec, 300)["group_tables_lds"] == 1
    monkeypatch.setenv("MSC_SB_TAB", "0")
    assert plan(spec, 300)["group_tables_lds"] == 0
    monkeypatch.delenv("MSC_ALLOC_IMPL")
    monkeypatch.setenv("MSC_DEMAND_IMPL", "unit")
    assert plan(spec, 300)["demand_impl"] == 0
    monkeypatch.setenv("MSC_DEMAND_IMPL", "v3")
    assert plan(spec, 300)["demand_impl"] == 9
    monkeypatch.setenv("MSC_EA_SLOTS", "4")
    got = plan(spec, 300)
    assert (got["ea_slots"], got["ea_batch"]) == (4, 2)
    for v, s in (("1", 2), ("40", 32)):  # clamped to 2 .. 32
        monkeypatch.setenv("MSC_EA_SLOTS", v)
        assert plan(spec, 300)["ea_slots"] == s
    monkeypatch.setenv("MSC_PIPELINE", "0")
    assert plan(spec, 300)["pipeline"] == 0


# ---- rejections, with msc_env_create's texts ---------------------------------------------------------
def _rejected(spec, n_envs=128):
    with pytest.raises(RuntimeError) as e:
        plan(spec, n_envs)
    return str(e.value)


def test_rejections(monkeypatch):
    spec = _c1()
    spec.K = 17
    assert _rejected(spec) == "libmarlsc error -1: n_skus must be in [1, 16]"
    spec = _c1()
    spec.lambda_orders[2] = 1e6
    assert _rejected(spec) == "libmarlsc error -1: lambda_orders[2]=1e+06: must be in (0, 1e6)"
    spec = _c1()
    spec.lambda_quantity[3, 1] = 0.0
    assert _rejected(spec) == "libmarlsc error -1: lambda_quantity[3,1]=0: must be in (0, 20000)"
    spec = EnvSpec.from_config(make_synthetic_env_config(2, 32, 1), WID)
    spec.lambda_orders[:] = 9e5
    lam = 32 * 9e5
    assert _order_cap(lam) > 1 << 24
    assert _rejected(spec) == ("libmarlsc error -1: sum of lambda_orders %g: per-step order capacity %.0f exceeds %d "
                               "records per env" % (lam, _order_cap(lam), 1 << 24))
    assert _rejected(_c1(), n_envs=0) == "libmarlsc error -1: n_envs must be positive"
    monkeypatch.setenv("MSC_DEMAND_IMPL", "v2")
    assert _rejected(_c1()) == "libmarlsc error -1: MSC_DEMAND_IMPL=v2: accepted values are v3 (the default) and unit"
    # a descriptor's own fault wins over the knob's, as in msc_env_create
    spec = _c1()
    spec.K = 0
    assert _rejected(spec) == "libmarlsc error -1: n_skus must be in [1, 16]"


# ---- the episode-ahead memory fit ---------------------------------------------------------------------
def test_episode_ahead_memory_fit():
    spec = _c1_yaml()
    E, T, cap = 128, 100, 2145
    slot = 16 * cap * E + 4 * (T + 1) * E + 4 * T * E + 4 * E + 1024  # records, offsets, positions, counter, slack
    assert slot == 4497408
    free = lambda slots: 4 * slots * slot  # the default budget is a quarter of the free memory
    assert plan(spec, E, free_bytes=free(16))["ea_slots"] == 16
    assert plan(spec, E, free_bytes=free(16) - 4)["ea_slots"] == 15
    three = plan(spec, E, free_bytes=free(3))
    assert (three["ea_slots"], three["ea_batch"], three["obs_stage"]) == (3, 1, 0)
    assert plan(spec, E, free_bytes=free(3) - 4)["ea_slots"] == 2
    one = plan(spec, E, free_bytes=free(1))
    assert (one["ea_slots"], one["ea_batch"], one["obs_stage"]) == (0, 1, 2)  # below 2 slots EA stays off
    assert plan(spec, E, free_bytes=0)["ea_slots"] == 0
    assert plan(spec, E, free_bytes=2 * 3 * slot, ea_mem_fraction=0.5)["ea_slots"] == 3


# ---- the arena: its layout is the checkpoint format ------------------------------------------------------
def test_arena_bytes_by_hand():
    # W = 2, K = 2, RING = 3, E = 128, fixed lead times: the 22 fields in order, each rounded up to 256
    by_hand = (2048 + 6144 + 256 + 10240 + 2048 + 2048      # inv, ring_q, ring_l (1 byte), hist, inc, fc
               + 8192 + 2048 + 4096 + 1024                   # rng, rbuf, rng_pre, rbuf_pre
               + 512 * 6 + 256                               # t, counter, orig_root, root, emp_start, perm; err (16 bytes)
               + 2048 + 2048 + 2048 * 3)                     # sc_sht, sc_shh; sc_pen, sc_out, sc_inb
    assert by_hand == 51712 == _arena_bytes(2, 2, 3, 128)
    got = plan(_c1(lead_time=2), 128)
    assert (got["ring"], got["arena_bytes"]) == (3, 51712)


# ---- the group width, defined once for the plan, kernel_choice() and the launcher ------------------------
@pytest.mark.parametrize("sb_gw,want", [(0, [2, 2, 4, 4, 8, 8, 16, 16, 32, 32]), (32, [32] * 10)])
def test_step_b_group_width(monkeypatch, sb_gw, want):
    # step_b_group_width(W, sb_gw) as the plan reports it for the group kernel (7 SKUs: no scan allocator)
    if sb_gw:
        monkeypatch.setenv("MSC_SB_GW", str(sb_gw))
    got = [plan(EnvSpec.from_config(make_synthetic_env_config(W, 8, 7), WID), 64)["group_width"]
           for W in (1, 2, 3, 4, 5, 8, 9, 16, 17, 32)]
    assert got == want
