"""GPU: the lane allocator's sold-out tail (alloc_lane_kernel, MSC_OPT_ALLOC_TAIL). A wave whose
envs have all sold out, or run out of orders, finishes its remaining orders in a loop that only
counts them as lost. Every case runs the lane allocator with the tail on and off, with and without
msc_step_info, in lockstep with the C oracle; the two settings must agree bit for bit, and the
order index at which each block entered the tail (alloc_tail_entry) must be the one a CPU replay of
the step's orders through tests/alloc_emulation.py gives.

The traces are hand-built like those of tests/alloc_cases.py (empirical sampler, episode length =
trace length, action -1 on a `demand_centered` space that then orders nothing, so stock only falls):
`unit` cases give every env the same stock and ask one unit of every SKU per order, so the env sells
out after exactly W * stock orders and the entry index is designed; `spread` cases draw the stock
per env, so the lanes of a block sell out at different orders, or not at all. The coverage
conditions the cases were built for are asserted from the CPU replay (test_coverage), so the suite
cannot pass without meeting them.
"""
import functools
from dataclasses import dataclass
from typing import Tuple

import numpy as np
import pytest

torch = pytest.importorskip("torch")

import alloc_cases as ac  # noqa: E402
import alloc_emulation as emu  # noqa: E402
import parity_util  # noqa: E402
from marlsc import make_synthetic_env_config  # noqa: E402
from marlsc.spec import EnvSpec  # noqa: E402
from parity_util import REW_ATOL, _lockstep, _np, _set_alloc, _vec  # noqa: E402

pytestmark = pytest.mark.gpu

AL_CH = 8              # alloc_kernels.hip: order records per window
TAIL_AT_WINDOWS = False  # the shipped form tests for the tail at every order (MSC_AL_TAIL_WIN 0)
E = ac.E               # 130 envs: two full blocks and a two-lane one
NB = (E + 63) // 64


@dataclass(frozen=True)
class Drain:
    name: str
    W: int
    R: int
    K: int
    lost: str
    pen_per_sku: bool
    kind: str                 # unit / spread
    stock: Tuple[int, int]    # uniform(min, max) initial inventory of every (warehouse, SKU)
    regions: Tuple[int, ...]  # the regions that receive orders, in turn
    per_region: Tuple[int, ...]  # unit: orders per region of the sell-out step; spread: orders per region and step
    T: int = 6
    split: int = 14           # MSC_OPT_ALLOC_PRIO_SPLIT
    zero_region: int = -1     # a region whose orders all have zero quantities


# home region of warehouse w: region w where w < R, else region R - 1 (ac.distance_table), so R < W
# shares home regions (the kernel's SH form) and R >= W does not; closest[r] = r % W where R >= W
CASES = [
    # (unit cases: step 0 serves two orders per region, step 1 sells out, later steps start sold out)
    # 2 x 12 units, 8 gone in step 0: entry 16, a window start and a region boundary (8 + 8 | 4 + 4); split 8
    Drain("unit_w2k1", 2, 4, 1, "shipment", True, "unit", (12, 12), (0, 1, 2, 3), (8, 8, 4, 4), split=8),
    # 3 x 7 units, 6 gone: entry 15 (7 mod 8), inside region 3 after 5 shipments to it; regions 0, 3, 6 share
    # their closest warehouse 0; home regions 1 and 2 have no orders
    Drain("unit_w3k5", 3, 7, 5, "closest", False, "unit", (7, 7), (0, 3, 6), (10, 9, 6)),
    # 8 x 4 units, 6 gone, 27 orders: entry 26, the last order
    Drain("unit_w8k8", 8, 4, 8, "cost", True, "unit", (4, 4), (0, 1, 3), (10, 10, 7)),
    # 16 x 1 units, 8 gone: entry 8
    Drain("unit_w16k5", 16, 5, 5, "shipment", False, "unit", (1, 1), (0, 2, 3, 4), (6, 6, 6, 7), split=16),
    Drain("spread_w8k5", 8, 12, 5, "shipment", True, "spread", (0, 14), (0, 2, 3, 5, 8, 10, 11), (4, 3, 5, 2, 4, 3, 3),
          T=8, zero_region=10),
    Drain("spread_w3k1", 3, 2, 1, "cost", False, "spread", (0, 40), (0, 1), (9, 8), T=7),
    Drain("spread_w16k8", 16, 16, 8, "closest", True, "spread", (0, 6), (1, 4, 5, 9, 15), (5, 4, 6, 3, 4), T=7,
          zero_region=9),
    Drain("spread_w2k5", 2, 1, 5, "shipment", False, "spread", (0, 60), (0,), (19,), T=9, split=8),
]
BY_NAME = {c.name: c for c in CASES}


def _steps(c: Drain):
    """Per step a list of (region, quantities [K]), region-major."""
    rng = np.random.default_rng(sum(map(ord, c.name)))
    steps = []
    for t in range(c.T):
        orders = []
        for r, n in zip(c.regions, c.per_region):
            if c.kind == "unit":
                n = n if t == 1 else 2 if t == 0 else 1 + (r + t) % 3
            for i in range(n):
                if c.kind == "unit":
                    q = np.ones(c.K, np.int64)
                else:
                    q = np.zeros(c.K, np.int64)
                    k = int(rng.integers(1, min(c.K, 3) + 1))
                    q[rng.choice(c.K, k, replace=False)] = rng.integers(1, 5, k)
                    if i % 5 == 3:
                        q[:] = 0  # an empty order inside a run
                if r == c.zero_region:
                    q[:] = 0
                orders.append((r, q))
        steps.append(orders)
    return steps


def _frame(c: Drain):
    cols = {k: [] for k in ("timestep", "region_id", "order_id", "sku_id", "quantity")}
    n = 0
    for t, orders in enumerate(_steps(c)):
        for r, q in orders:
            for s, v in [(s, int(q[s])) for s in range(c.K) if q[s] > 0] or [(0, 0)]:
                for k, x in zip(cols, (t, r, f"o{n:07d}", s, v)):
                    cols[k].append(x)
            n += 1
    return {k: np.asarray(v) for k, v in cols.items()}


@functools.lru_cache(maxsize=None)
def _spec(name) -> EnvSpec:
    c = BY_NAME[name]
    cfg = make_synthetic_env_config(c.W, c.R, c.K, episode_length=c.T, lost_sales=c.lost,
                                    max_quantity_adjustment=ac.MAX_ADJ)
    of, ov = ac.cost_tables("class_ties", c.W, c.R)
    cs = cfg["cost_structure"]
    cs["shipment_cost"]["outbound_fixed"] = of.tolist()
    cs["shipment_cost"]["outbound_variable"] = ov.tolist()
    cs["distances"] = ac.distance_table(c.W, c.R, True).tolist()
    if not c.pen_per_sku:
        cs["penalty_cost"] = 7.5
    cfg["initial_inventory"] = {"type": "uniform", "params": {"min": c.stock[0], "max": c.stock[1]}}
    cfg["components"]["demand_sampler"] = {"type": "empirical", "params": None}
    spec = EnvSpec.from_config(cfg, {"include_warehouse_id": True, "demand_trace": _frame(c)})
    assert bool(spec.penalty_per_sku) == c.pen_per_sku
    assert (len(set(spec.home_regions.tolist())) < c.W) == (c.R < c.W)
    return spec


@functools.lru_cache(maxsize=None)
def _oracle(name):
    """The oracle's episode under action -1 (once per session): reset observations and inventory, and
    per step the observations, f64 rewards, flags, final observations, inventory and step info."""
    import oracle as orc
    spec = _spec(name)
    ref = orc.OracleEnv(spec, E, base_seed=ac.BASE_SEED)
    out = {"reset_obs": ref.reset().copy(), "inv0": ref.read_state()["inventory"].copy(), "steps": []}
    act = -np.ones((E, spec.W, spec.K), np.float32)
    for _ in range(spec.episode_length):
        info = ref.alloc_info()
        obs, rew, tr, fo = ref.step(act, info=info, final_obs=True, n_threads=4)
        out["steps"].append({"obs": obs, "rew": rew, "tr": tr, "fo": fo, "info": info,
                             "inventory": ref.read_state()["inventory"].copy()})
    return out


@functools.lru_cache(maxsize=None)
def _replay(name):
    """Per step of the first episode: the regions of the step's orders, each env's done index (the
    first order index at which its stock is all zero, the order count if there is none), each env's
    units shipped to the region of the order at its done index before that index, and the inventory
    after the step. Orders go through alloc_emulation.allocate one at a time."""
    spec = _spec(name)
    inv = _oracle(name)["inv0"].astype(np.int64)
    out = []
    for t in range(spec.episode_length):
        reg, qty = ac.step_orders(spec, t)
        n = len(reg)
        done = np.full(E, n, np.int64)
        shipped_here = np.zeros(E, np.int64)  # units shipped to the current region so far
        at_done = np.zeros(E, np.int64)
        for oi in range(n):
            if oi > 0 and reg[oi] != reg[oi - 1]:
                shipped_here[:] = 0
            sold = (inv.reshape(E, -1) == 0).all(axis=1) & (done == n)
            done[sold] = oi
            at_done[sold] = shipped_here[sold]
            after, _ = emu.allocate(reg[oi:oi + 1], qty[oi:oi + 1], inv, spec.outbound_fixed, spec.outbound_variable,
                                    spec.sku_weights, spec.max_splits, n_regions=spec.R)
            shipped_here += (inv - after).sum(axis=(1, 2))
            inv = after
        out.append({"reg": np.asarray(reg), "qty": np.asarray(qty), "done": done, "at_done": at_done, "inventory": inv})
    return out


def _entries(name):
    """[T][NB] the expected alloc_tail_entry: the block's entry is the latest done index of its envs,
    at the next window start if the kernel only tests there, and -1 if that is not before the last
    iteration of the general loop (index n, where every list has ended anyway)."""
    out = []
    for st in _replay(name):
        n = len(st["reg"])
        row = []
        for b in range(NB):
            at = int(st["done"][b * 64:(b + 1) * 64].max())
            if TAIL_AT_WINDOWS:
                at = (at + AL_CH - 1) // AL_CH * AL_CH
            row.append(at if at < n else -1)
        out.append(row)
    return np.asarray(out)


def _run(monkeypatch, name, tail, with_info):
    """One episode on the GPU against the oracle; returns what the run produced, for the on / off comparison."""
    c, spec, ref = BY_NAME[name], _spec(name), _oracle(name)
    _set_alloc(monkeypatch, "lane")
    env = _vec(spec, E, base_seed=ac.BASE_SEED)
    assert env.kernel_choice()["alloc"] == 0
    env.set_option(env.ALLOC_PRIO_SPLIT, c.split)
    env.set_option(env.ALLOC_TAIL, 1 if tail else 0)
    np.testing.assert_array_equal(_np(env.reset()), ref["reset_obs"])
    np.testing.assert_array_equal(env.read_state()["inventory"], ref["inv0"])
    act = -torch.ones((E, spec.W, spec.K), dtype=torch.float32, device="cuda")
    want_entry = _entries(name)
    got = []
    for t, st in enumerate(ref["steps"]):
        msg = f"{name} tail={tail} info={with_info} t={t}"
        info = env.alloc_info() if with_info else None
        obs, _, tr, fo = env.step(act, want_f64=True, info=info)
        entry = env.alloc_tail_entry()
        trn = _np(tr).astype(bool)
        rec = {"obs": _np(obs), "rew": _np(env.rewards_f64), "tr": trn, "fo": _np(fo),
               "inventory": env.read_state()["inventory"], "entry": entry}
        np.testing.assert_array_equal(trn, st["tr"], err_msg=msg)
        np.testing.assert_array_equal(rec["obs"], st["obs"], err_msg=f"{msg} obs")
        if trn.any():
            np.testing.assert_array_equal(rec["fo"][trn], st["fo"][trn], err_msg=f"{msg} final obs")
        np.testing.assert_allclose(rec["rew"], st["rew"], rtol=0, atol=REW_ATOL, err_msg=msg)
        np.testing.assert_array_equal(rec["inventory"], st["inventory"], err_msg=f"{msg} inventory")
        if not trn.any():  # (the last step ends in the auto-reset)
            np.testing.assert_array_equal(rec["inventory"], _replay(name)[t]["inventory"], err_msg=f"{msg} replay")
        np.testing.assert_array_equal(entry, want_entry[t] if tail else np.full(NB, -1), err_msg=f"{msg} tail entry")
        if with_info:
            rec["info"] = {k: _np(v) for k, v in info.items()}
            for k, v in st["info"].items():
                if k == "lost_sales":
                    np.testing.assert_allclose(rec["info"][k], v, rtol=1e-9, atol=1e-9, err_msg=f"{msg} {k}")
                elif k == "costs":
                    np.testing.assert_allclose(rec["info"][k], v, rtol=1e-9, atol=1e-7, err_msg=f"{msg} {k}")
                else:
                    np.testing.assert_array_equal(rec["info"][k], v, err_msg=f"{msg} {k}")
        got.append(rec)
    env.check()
    env.close()
    return got


def _same(a, b, msg):
    for t, (x, y) in enumerate(zip(a, b)):
        for k in ("obs", "rew", "tr", "fo", "inventory"):
            np.testing.assert_array_equal(x[k], y[k], err_msg=f"{msg} t={t} {k}")
        for k in x.get("info", {}):
            np.testing.assert_array_equal(x["info"][k], y["info"][k], err_msg=f"{msg} t={t} info {k}")


@pytest.mark.parametrize("name", [c.name for c in CASES])
def test_designed_case(monkeypatch, name):
    runs = {(tail, info): _run(monkeypatch, name, tail, info) for tail in (True, False) for info in (True, False)}
    _same(runs[True, True], runs[False, True], f"{name} tail on / off with info")
    _same(runs[True, False], runs[False, False], f"{name} tail on / off")
    _same(runs[True, False], runs[True, True], f"{name} with / without info")


def test_coverage():
    """The conditions the cases were built for, from the CPU replay alone."""
    for name, at in (("unit_w2k1", 16), ("unit_w3k5", 15), ("unit_w8k8", 26), ("unit_w16k5", 8)):
        np.testing.assert_array_equal(_entries(name)[:3], [[-1] * NB, [at] * NB, [0] * NB], err_msg=name)
    seen = set()
    for c in CASES:
        spec = _spec(c.name)
        closest = np.argmin(spec.distances, axis=0)
        homes = set(spec.home_regions.tolist())
        for st, row in zip(_replay(c.name), _entries(c.name)):
            reg, qty, n = st["reg"], st["qty"], len(st["reg"])
            for b, at in enumerate(row.tolist()):
                done = st["done"][b * 64:(b + 1) * 64]
                if at < 0:
                    if (done < n).sum() >= len(done) // 2 and (done == n).any():
                        seen.add("never: one env keeps stock in a mostly sold-out block")
                    continue
                seen.add(f"block {b}")
                last = int(np.argmax(done))  # an env that sets the block's entry
                if at == 0:
                    seen.add("entry at order 0")
                elif reg[at] != reg[at - 1]:
                    seen.add("entry at a region boundary")
                elif st["at_done"][b * 64 + last] > 0:
                    seen.add("entry inside a region with shipments")
                if at > 0:
                    seen.add(f"entry {at % AL_CH} mod {AL_CH}")
                if at == n - 1:
                    seen.add("entry at the last order")
                if at <= (n * c.split) >> 4 < n and c.split < 16:
                    seen.add(f"split {c.split} inside the tail")
                if c.split == 16:
                    seen.add("split 16")
                # regions that begin inside the tail
                starts = [i for i in range(max(at, 1), n) if reg[i] != reg[i - 1]] + ([0] if at == 0 else [])
                tail_regs = [int(reg[i]) for i in sorted(starts)]
                for r in tail_regs:
                    if r in homes:
                        seen.add("home region with orders in the tail")
                    if (qty[reg == r] == 0).all():
                        seen.add("all-zero region in the tail")
                if homes - set(reg.tolist()):
                    seen.add("home region without orders")
                lossy = [r for r in tail_regs if (qty[reg == r] != 0).any()]
                if any(closest[a] == closest[z] for a, z in zip(lossy, lossy[1:])):
                    seen.add("consecutive tail regions with the same closest warehouse")
    want = {"never: one env keeps stock in a mostly sold-out block", "block 0", "block 1", "block 2", "entry at order 0",
            "entry at a region boundary", "entry inside a region with shipments", f"entry 0 mod {AL_CH}",
            f"entry 7 mod {AL_CH}", "entry at the last order", "split 8 inside the tail", "split 16",
            "home region with orders in the tail", "all-zero region in the tail", "home region without orders",
            "consecutive tail regions with the same closest warehouse"}
    assert want <= seen, sorted(want - seen)


def _poisson_spec(space="demand_centered"):
    cfg = make_synthetic_env_config(8, 12, 5, episode_length=20, initial_inventory=20)
    if space == "direct":
        cfg["action_space"] = {"type": "direct", "params": {"max_order_quantities": [60] * 5}}
    return EnvSpec.from_config(cfg, {"include_warehouse_id": True})


@pytest.mark.parametrize("tail", [1, 0])
@pytest.mark.parametrize("src", ["per_step", "episode_ahead"])
def test_poisson_random_actions(monkeypatch, tail, src):
    # 192 envs x 30 steps over the boundary of 20-step episodes: arrivals refill the stock between
    # sold-out steps, and the in-kernel reset falls between them
    _set_alloc(monkeypatch, "lane")
    if src == "episode_ahead":
        monkeypatch.setenv("MSC_EA", "1")
    spec = _poisson_spec()

    def vec(*a, **k):  # _lockstep's handle, with the option set before its first step
        env = _vec(*a, **k)
        env.set_option(env.ALLOC_TAIL, tail)
        return env

    monkeypatch.setattr(parity_util, "_vec", vec)
    env, _ = _lockstep(spec, 192, 30, seed=5, check_every=3)
    assert env.kernel_choice()["alloc"] == 0
    assert (env.kernel_choice()["ea_slots"] > 0) == (src == "episode_ahead")
    entries = env.alloc_tail_entry()
    assert entries.shape == (3,) and (tail == 1 or (entries == -1).all())
    env.close()


def test_poisson_never_sold_out(monkeypatch):
    # a `direct` action space at +1 orders the maximum every step: no env sells out, no block enters the tail
    import oracle as orc
    _set_alloc(monkeypatch, "lane")
    spec = _poisson_spec("direct")
    Ep = 192
    env = _vec(spec, Ep, base_seed=31)
    ref = orc.OracleEnv(spec, Ep, base_seed=31)
    np.testing.assert_array_equal(_np(env.reset()), ref.reset())
    a = np.ones((Ep, spec.W, spec.K), np.float32)
    for t in range(12):
        og, _, _, _ = env.step(torch.from_numpy(a).cuda(), want_f64=True)
        orr, rr, _, _ = ref.step(a, final_obs=True, n_threads=8)
        np.testing.assert_array_equal(_np(og), orr, err_msg=f"obs t={t}")
        np.testing.assert_allclose(_np(env.rewards_f64), rr, rtol=0, atol=REW_ATOL, err_msg=f"t={t}")
        inv = env.read_state()["inventory"]
        np.testing.assert_array_equal(inv, ref.read_state()["inventory"])
        if t >= 4:  # (the first arrivals are in: lead time 3)
            assert (inv.reshape(Ep, -1).sum(axis=1) > 0).all(), t
            np.testing.assert_array_equal(env.alloc_tail_entry(), np.full(3, -1), err_msg=f"t={t}")
    env.check()
    env.close()
