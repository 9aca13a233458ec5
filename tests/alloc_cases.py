"""Hand-built allocation cases: tied and near-tied cost tables, order traces written order by order,
and the emulated episode each case is checked against (tests/alloc_emulation.py).

The empirical sampler replays a trace; with exactly `episode_length` timesteps its window start is
always 0, so every order of every step is the test author's. Action -1 on every component of a
`demand_centered` action space whose adjustment exceeds any home demand orders nothing, lead
times are fixed, so inventory only falls and the inventory at allocation time is the previous
step's. Initial inventory is `uniform`, so the 130 envs of a batch (a partial last wave) differ,
and each episode runs from abundant stock through partial fills and splits into starvation.

`pack_demand_trace` sorts a step's orders by (region, order id), so a step is a sequence of
region runs; a run's orders differ in quantity and hence, in the crossing / near-tie tables, in
ranking. The packer takes its timesteps from the frame's rows, so a timestep with no order at all
cannot be written; an order whose quantities are all zero can, and `counts_*` holds some.

The table is shared by tests/test_alloc_ties_host.py (oracle against emulation, on the CPU) and
tests/test_gpu_alloc_ties.py (every allocation kernel against both).
"""
from __future__ import annotations

import functools
from dataclasses import dataclass, field
from typing import Optional, Tuple

import numpy as np

import alloc_emulation as emu
from marlsc import make_synthetic_env_config
from marlsc.spec import EnvSpec

E = 130
BASE_SEED = 4242
MAX_ADJ = 1_000_000  # demand_centered adjustment: above any home demand below, so action -1 orders nothing

# near_tie (profiles/alloc_ties/near_tie_search.txt): one SKU of weight 0.3, row A = (of 20.007,
# ov 0.18352). An order of 4 units (tw = 1.2) costs 20.227224 with two roundings and one ulp more
# fused; one of 12 units (tw = 3.5999999999999996) costs 20.667672000000003 and one ulp less fused.
# Row B has ov = 0 and of = the two-rounding value, so A and B tie exactly in the reference's
# arithmetic and an FMA orders them either way round, by region.
NT_W0, NT_OF, NT_OV = 0.3, 20.007, 0.18352
NT_Q = (4, 12)
NT_TWO_ROUNDING = (20.227224, 20.667672000000003)


@dataclass(frozen=True)
class Case:
    name: str
    table: str  # all_tied / class_ties / crossing / near
    W: int
    R: int
    K: int
    T: int = 8
    trace: str = "phased"  # phased / counts / wide / starve
    max_splits: Optional[int] = None  # None: W - 1
    lost: str = "shipment"
    init_min: int = 1
    unshared: bool = False  # R == W, every warehouse its own home region: the lane kernel's 2 / 4 lanes per env run
    orders: Tuple[int, ...] = field(default=())  # trace "counts": the orders of each step


def _cases():
    out = []
    # all warehouse counts, tied in every region / within classes w % 3; K = 9 past 16 warehouses
    for W, R, K in ((4, 3, 1), (5, 5, 2), (8, 4, 5), (12, 3, 2), (16, 5, 5), (17, 4, 9), (24, 3, 5), (32, 5, 9)):
        out.append(Case(f"all_tied_w{W}k{K}", "all_tied", W, R, K, unshared=W == 5))
    for W, R, K in ((4, 4, 2), (5, 3, 5), (8, 5, 1), (12, 4, 5), (16, 3, 1), (17, 5, 2), (24, 4, 9), (32, 3, 5)):
        out.append(Case(f"class_ties_w{W}k{K}", "class_ties", W, R, K))
    # R == W: no shared home region, so the lane kernel runs its 2- and 4-lanes-per-env merge
    for W, K in ((8, 2), (12, 5), (16, 1)):
        out.append(Case(f"all_tied_unshared_w{W}k{K}", "all_tied", W, W, K, unshared=True))
        out.append(Case(f"class_ties_unshared_w{W}k{K}", "class_ties", W, W, K, unshared=True))
    for W in (4, 8, 16, 24):
        out.append(Case(f"crossing_tie_w{W}", "crossing", W, 3, 2))
    for W in (4, 8, 12, 32):
        out.append(Case(f"near_tie_w{W}", "near", W, 3, 1))
    for W, ms in ((5, 0), (5, 1), (5, 4), (12, 1), (24, 0)):
        out.append(Case(f"splits_w{W}ms{ms}", "all_tied", W, 4, 2, max_splits=ms, init_min=0))
    for W, K in ((4, 2), (16, 5), (32, 9)):
        for lost in ("shipment", "cost", "closest"):
            out.append(Case(f"starved_{lost}_w{W}", "all_tied", W, 3, K, T=6, trace="starve", lost=lost))
    out.append(Case("counts_w8", "crossing", 8, 3, 2, T=9, trace="counts", orders=(1, 63, 64, 65, 129, 64, 128, 2, 65)))
    out.append(Case("counts_w16", "class_ties", 16, 4, 5, T=9, trace="counts", orders=(129, 1, 65, 64, 63, 128, 64, 1, 130)))
    out.append(Case("counts_w32", "all_tied", 32, 5, 9, T=6, trace="counts", orders=(1, 63, 64, 65, 129, 64)))
    for W, K in ((4, 2), (16, 5), (32, 9)):
        out.append(Case(f"wide_w{W}k{K}", "all_tied", W, 3, K, T=5, trace="wide"))
    return out


CASES = _cases()
CASE_BY_NAME = {c.name: c for c in CASES}


# ---- cost tables -------------------------------------------------------------------------------
def sku_weights(c: Case):
    if c.table == "near":
        return [NT_W0]
    if c.table == "crossing":
        return [1.0, 2.0]
    return [0.5 + 0.7 * s for s in range(c.K)]  # not dyadic: equal rows still cost the same bit for bit


def cost_tables(table, W, R):
    of, ov = np.zeros((W, R)), np.zeros((W, R))
    for w in range(W):
        for r in range(R):
            if table == "all_tied":
                of[w, r], ov[w, r] = 10.0 + r, 0.3 + 0.1 * r
            elif table == "class_ties":
                # classes w % 3, ordered alike in of and ov (they never cross), rotated by region
                cl = (w + r) % 3
                of[w, r], ov[w, r] = (3.0, 5.0, 8.0)[cl], (0.25, 0.5, 0.75)[cl]
            elif table == "crossing":
                # (4, 1) and (2, 1.5): equal at tw = 4, odd warehouses cheaper below, even above;
                # every product and sum is exact. Regions swap the roles.
                of[w, r], ov[w, r] = ((4.0, 1.0), (2.0, 1.5))[(w + r) % 2]
            elif table == "near":
                if w % 2 == 0:
                    of[w, r], ov[w, r] = NT_OF, NT_OV
                else:
                    of[w, r], ov[w, r] = NT_TWO_ROUNDING[r % 2], 0.0
    return of, ov


def distance_table(W, R, unshared):
    d = np.zeros((W, R))
    for w in range(W):
        for r in range(R):
            d[w, r] = 100.0 + 10.0 * ((w - r) % W)
    if not unshared:
        for r in range(R):  # warehouses r and r + 2 tie for closest: argmin takes the first
            d[(r + 2) % W, r] = 100.0
    return d


# ---- traces ------------------------------------------------------------------------------------
def _order(rng, K, qmax):
    q = np.zeros(K, np.int64)
    n = int(rng.integers(1, min(K, 3) + 1))
    q[rng.choice(K, n, replace=False)] = rng.integers(1, qmax + 1, n)
    return q


def _steps(c: Case):
    """Per step a list of (region, quantities [K]) in writing order."""
    rng = np.random.default_rng(sum(map(ord, c.name)))
    W, R, K, T = c.W, c.R, c.K, c.T
    steps = []
    if c.table == "near":
        # steps 0-2: the near-tie quantities of both regions' tables among small orders, few enough
        # that no warehouse runs out (_init_range), so the two evaluations cannot end the step alike;
        # from step 3 on W orders of 100 units a step drain every warehouse
        for t in range(T):
            orders = [(r, np.array([q])) for r in (0, 1) for q in (4, 12, 3, 4)]
            orders += [(i % R, _order(rng, K, 2)) for i in range(6)]
            if t >= 3:
                orders += [(i % R, np.array([100])) for i in range(W)]
            steps.append(orders)
    elif c.trace in ("phased", "starve"):
        n = max(6, W // 2) * (2 if c.trace == "starve" else 1)
        for t in range(T):
            orders = []
            for i in range(n):
                # even steps: long runs in two regions; odd steps: the regions in turn
                r = (t // 2 + (i * 2) // n) % R if t % 2 == 0 else i % R
                orders.append((r, _order(rng, K, 4 + W // 8)))
            if c.table == "crossing":  # tw below, at and above the tie (weights 1, 2; tie at tw = 4)
                orders += [(t % R, np.array(q)) for q in ((1, 1), (2, 1), (0, 2), (4, 0), (1, 2), (3, 2))]
            steps.append(orders)
    elif c.trace == "counts":
        for t, n in enumerate(c.orders):
            orders = []
            for i in range(n):
                if t % 3 == 0:    # one long run of one region
                    r = t % R
                elif t % 3 == 1:  # runs of equal length
                    r = (i * R) // n
                else:             # short runs: the regions in turn
                    r = i % R
                q = _order(rng, K, 3)
                if i % 17 == 5:
                    q[:] = 0      # an empty order
                if c.table == "crossing" and i % 2:
                    q = np.array(((2, 1), (4, 0), (1, 2))[(i // 2) % 3])  # rankings alternate inside a run
                orders.append((r, q))
            steps.append(orders)
    elif c.trace == "wide":
        big = 65535  # the largest quantity a 16-bit record field and msc_env_create's trace check admit
        for t in range(T):  # W orders a step; two in three ask the field's maximum of half the SKUs
            orders = []
            for i in range(W):
                q = _order(rng, K, 3)
                if i % 3 != 2:
                    q[:] = 0
                    q[[(t + i + j) % K for j in range((K + 1) // 2)]] = big
                orders.append(((t + i) % R, q))
            steps.append(orders)
    return steps


def trace_frame(c: Case):
    cols = {k: [] for k in ("timestep", "region_id", "order_id", "sku_id", "quantity")}
    n = 0
    for t, orders in enumerate(_steps(c)):
        for r, q in orders:
            lines = [(s, int(q[s])) for s in range(c.K) if q[s] > 0] or [(0, 0)]
            for s, v in lines:
                for k, x in zip(cols, (t, r, f"o{n:07d}", s, v)):
                    cols[k].append(x)
            n += 1
    return {k: np.asarray(v) for k, v in cols.items()}


@functools.lru_cache(maxsize=None)
def _init_range(c: Case):
    """uniform(min, max) initial inventory: wide cases straddle the 16-bit edge; otherwise a SKU's
    stock over all warehouses is 0.45 to 0.75 of the least-wanted SKU's demand over the episode
    (0 to 1.2 where warehouses shall start empty), so every SKU runs out inside the episode."""
    if c.trace == "wide":
        return 60000, 70000
    if c.table == "near":  # more than step 0 asks for in all: no warehouse runs out in it
        lo = int(sum(q.sum() for _, q in _steps(c)[0])) + 1
        return lo, lo + lo // 2
    tot = sum((q for orders in _steps(c) for _, q in orders), np.zeros(c.K, np.int64))
    per = float(tot.min()) / c.W
    if c.init_min == 0:
        return 0, max(1, int(round(1.2 * per)))
    lo = max(1, int(round(0.45 * per)))
    return lo, max(lo + 1, int(round(0.75 * per)))


def make_spec(c: Case, *, demand="empirical", episode_length=None) -> EnvSpec:
    W, R, K = c.W, c.R, c.K
    cfg = make_synthetic_env_config(W, R, K, episode_length=episode_length or c.T, lost_sales=c.lost,
                                    max_quantity_adjustment=MAX_ADJ)
    of, ov = cost_tables(c.table, W, R)
    cs = cfg["cost_structure"]
    cs["shipment_cost"]["outbound_fixed"] = of.tolist()
    cs["shipment_cost"]["outbound_variable"] = ov.tolist()
    cs["distances"] = distance_table(W, R, c.unshared).tolist()
    meta = {"include_warehouse_id": True}
    if demand == "empirical":
        cs["sku_weights"] = sku_weights(c)
        lo, hi = _init_range(c)
        cfg["initial_inventory"] = {"type": "uniform", "params": {"min": lo, "max": hi}}
        cfg["components"]["demand_sampler"] = {"type": "empirical", "params": None}
        cfg["components"]["demand_allocator"]["params"]["max_splits"] = "default" if c.max_splits is None else c.max_splits
        meta["demand_trace"] = trace_frame(c)
    return EnvSpec.from_config(cfg, meta)


def step_orders(spec: EnvSpec, t: int):
    """Step t's orders as the packed CSR trace holds them."""
    tr = spec.trace
    lo, hi = int(tr["offsets"][t]), int(tr["offsets"][t + 1])
    return tr["regions"][lo:hi], tr["quantities"][lo:hi]


def emulate_episode(spec: EnvSpec, inventory, *, tie="low", fused=False, steps=None):
    """The whole episode from the inventory after reset: per step a dict with the info arrays,
    `inventory_before`, `inventory` (after), `lost_sales` [E, W, K] and `costs` [E, 4, W]."""
    inv = np.asarray(inventory, np.int64)
    out = []
    for t in range(spec.episode_length if steps is None else steps):
        reg, qty = step_orders(spec, t)
        after, info = emu.allocate(reg, qty, inv, spec.outbound_fixed, spec.outbound_variable, spec.sku_weights,
                                   spec.max_splits, n_regions=spec.R, tie=tie, fused=fused)
        lost = emu.lost_sales(spec.lost_type, info, spec.outbound_fixed, spec.outbound_variable, spec.sku_weights,
                              spec.distances, spec.lost_alpha)
        cost = emu.costs(after, lost, info, spec.outbound_fixed, spec.outbound_variable, spec.sku_weights,
                         float(spec.holding[0]), spec.penalty)
        out.append(dict(info, inventory_before=inv, inventory=after, lost_sales=lost, costs=cost, n_orders=len(reg)))
        inv = after
    return out


@functools.lru_cache(maxsize=None)
def reference_episode(name: str):
    """(spec, oracle reset inventory, emulated episode) of a case, computed once per session. The
    initial inventory is the oracle's after reset (its PCG64 draws are pinned by the golden
    fixtures); the GPU tests check the device's reset inventory against it before they step."""
    import oracle as orc
    c = CASE_BY_NAME[name]
    spec = make_spec(c)
    ref = orc.OracleEnv(spec, E, base_seed=BASE_SEED)
    ref.reset()
    inv0 = ref.read_state()["inventory"].copy()
    return spec, inv0, emulate_episode(spec, inv0)


@functools.lru_cache(maxsize=None)
def oracle_episode(name: str):
    """The C oracle's episode of a case under action -1, computed once per session: per step the
    observations, float64 rewards, truncation flags, final observations, inventory and step info."""
    import oracle as orc
    spec, inv0, _ = reference_episode(name)
    ref = orc.OracleEnv(spec, E, base_seed=BASE_SEED)
    out = {"reset_obs": ref.reset().copy(), "steps": []}
    act = -np.ones((E, spec.W, spec.K), np.float32)
    for _ in range(spec.episode_length + 1):  # one step past the episode boundary (the auto-reset)
        info = ref.alloc_info()
        obs, rew, tr, fo = ref.step(act, info=info, final_obs=True, n_threads=4)
        out["steps"].append({"obs": obs, "rew": rew, "tr": tr, "fo": fo, "info": info,
                             "inventory": ref.read_state()["inventory"].copy()})
    return out


def poisson_spec(table: str, W: int) -> EnvSpec:
    """The synthetic Poisson config with its cost and distance tables overwritten by a tied table:
    the replenished regime and the Poisson record path. Up to 16 warehouses every warehouse has
    its own home region (R = W), so the lane kernel's 2 / 4 lanes per env run as well."""
    c = Case(f"poisson_{table}_w{W}", table, W, W if W <= 16 else 6, 3 if W <= 16 else 9, unshared=W <= 16)
    return make_spec(c, demand="poisson", episode_length=20)
