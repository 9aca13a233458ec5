"""Designed cases for the two phases around the allocator: order placement and arrivals (phase A)
and costs, reward, forecast, history and observations (phase C), checked against the numpy
restatement of the reference in tests/step_emulation.py.

Every case runs 130 envs (a partial last wave) through one short episode and one step past its
end. Actions are a designed table [T][E][W][K] in which the env index selects the pattern, so
every pattern of a SKU's list occurs in every step: -1, +1, +0 and -0; every dyadic action that
puts `prm * (a + 1) / 2` (direct, base_stock) or `prm * a` (demand_centered) exactly on x.5, for
parameters 20, 25, 30 and 7 so that x is odd and even; the two float32 neighbours of -1 and of each
tie; and finite |a| up to 4. Envs 0-3 hold -1, +1, +0 and -0 on every component for the whole
episode (nothing ordered at all / a full order every step). In base_stock the home demand and the
pending total subtracted from a tied target are integers, so the tie stays and its parity moves
with the trace.

Traces follow tests/alloc_cases.py (`trace_frame`, exactly `episode_length` timesteps, so every
order is the author's): region 0 asks one unit of SKU 0 in steps 0-2, nothing in step 3 and two
units in step 4, so the rolling mean of its home warehouses is exactly 1.0 at n_hist = 1, 2, 3 and
5; the last region orders in steps 0 and 1 only, so its home warehouses see all-zero demand, a
forecast that decays from 0.3 and history that empties again; step 3 holds only zero-quantity
orders. Initial inventories are custom with zeros, one warehouse empty, so the ratio
denominators vanish.

Shared by tests/test_step_cases_host.py (oracle against emulation, mutants; CPU) and
tests/test_gpu_step_cases.py (every kernel form against both).
"""
from __future__ import annotations

import functools
from dataclasses import dataclass
from fractions import Fraction
from typing import Optional, Tuple, Union

import numpy as np

import alloc_emulation as alloc
import step_emulation as se
from marlsc import make_synthetic_env_config
from marlsc.config import FEATURE_DEFAULTS
from marlsc.spec import EnvSpec

E = 130
BASE_SEED = 90210
PARAMS = (20, 25, 30, 7)
BIG = 2 ** 24 - 1  # the largest pending total the float32 accumulation still holds exactly

ALL_ON = {k: True for k in FEATURE_DEFAULTS}
NO_AGG = {k: not k.endswith("_aggregate") for k in FEATURE_DEFAULTS}


def _only(*groups):
    f = {k: k in ("inventory", "pipeline") or k in groups for k in FEATURE_DEFAULTS}
    return f


FEATURES = {
    "all": ALL_ON, "noagg": NO_AGG, "default": dict(FEATURE_DEFAULTS),
    "supply": _only("days_of_supply", "net_inventory_position"),
    "history": _only("demand_variability", "demand_history"),
    "forecast": _only("rolling_demand_mean", "demand_forecast", "rolling_demand_mean_aggregate", "demand_forecast_aggregate"),
}


@dataclass(frozen=True)
class Case:
    name: str
    W: int
    R: int
    K: int
    action: str  # direct / demand_centered / base_stock
    lead: Union[int, str] = 3  # a fixed lead time, or "mixed": expected 1 ... 6 per component
    T: int = 8
    deviation: Optional[Union[int, Tuple[int, ...]]] = None  # stochastic: scalar or per-SKU list; expected 1 ... 4
    features: str = "all"
    norm: str = "ratio"
    scope: str = "agent"
    big: bool = False  # base_stock with max_stock_level 2^24 - 1, |a| <= 1, one ordering SKU per warehouse


def _cases():
    c = []
    for act in ("direct", "demand_centered", "base_stock"):
        c.append(Case(f"w4k2_lead1_{act}", 4, 3, 2, act, lead=1, T=7))  # RING 2
    # the register-ring and low-register forms, the group's fused C, the scan's fused A and C
    c.append(Case("w8k5_lead3_direct", 8, 4, 5, "direct", T=9))
    c.append(Case("w8k5_lead3_demand_centered", 8, 4, 5, "demand_centered", T=9, scope="team"))
    c.append(Case("w8k5_lead3_base_stock", 8, 4, 5, "base_stock", T=9))
    c.append(Case("w8k5_lead3_default_off", 8, 4, 5, "direct", T=7, features="default", norm="off"))
    c.append(Case("w8k5_lead3_noagg", 8, 4, 5, "base_stock", T=7, features="noagg"))
    c.append(Case("w8k5_lead3_noagg_off", 8, 4, 5, "demand_centered", T=7, features="noagg", norm="off", scope="team"))
    for grp, act in (("supply", "base_stock"), ("history", "demand_centered"), ("forecast", "direct")):
        c.append(Case(f"w4k2_lead1_{grp}", 4, 3, 2, act, lead=1, T=7, features=grp))
    # (8 warehouses whose observations still fit step_c's LDS stage: staged in 1, 2 and 8 phases)
    c.append(Case("w8k2_lead3_default", 8, 4, 2, "direct", T=7, features="default"))
    c.append(Case("w8k6_lead3_base_stock", 8, 4, 6, "base_stock"))  # past the register form, at the scan fuse's edge
    c.append(Case("w8k5_mixed_base_stock", 8, 4, 5, "base_stock", lead="mixed", T=12))  # RING 7: the generic loop, no fused C
    c.append(Case("w8k5_mixed_direct", 8, 4, 5, "direct", lead="mixed", T=12, features="default"))
    c.append(Case("w16k8_lead3_demand_centered", 16, 5, 8, "demand_centered", T=7))  # either side of the warehouse loop
    c.append(Case("w17k3_lead3_base_stock", 17, 5, 3, "base_stock", T=7, scope="team"))
    c.append(Case("w8k9_lead3_direct", 8, 4, 9, "direct", T=6))  # the four-wave loop blocks, both wide units
    c.append(Case("w24k12_lead3_demand_centered", 24, 5, 12, "demand_centered", T=6))
    c.append(Case("w32k16_lead3_base_stock", 32, 6, 16, "base_stock", T=6, scope="team"))
    # stochastic: expected 1 ... 4, so the clip to 1, early and overdue arrivals all occur
    c.append(Case("w8k5_stoch_scalar_base_stock", 8, 4, 5, "base_stock", lead="stoch", deviation=2, T=12))
    c.append(Case("w8k5_stoch_list_direct", 8, 4, 5, "direct", lead="stoch", deviation=(2, 0, 1, 3, 2), T=12, scope="team"))
    c.append(Case("w17k10_stoch_list_demand_centered", 17, 5, 10, "demand_centered", lead="stoch",
                  deviation=(2, 0, 1, 3, 2, 1, 0, 2, 3, 1), T=10))
    c.append(Case("w17k10_stoch_scalar_base_stock", 17, 5, 10, "base_stock", lead="stoch", deviation=3, T=10, features="noagg"))
    c.append(Case("w8k5_lead3_base_stock_full", 8, 4, 5, "base_stock", T=9, big=True))
    return c


CASES = _cases()
CASE_BY_NAME = {c.name: c for c in CASES}


# ---- actions ----------------------------------------------------------------------------------
def ties(kind: str, prm: int):
    """Every dyadic a = j / 64 in [-1, 1] whose scaled value lies exactly on x.5, with that value."""
    out = []
    for j in range(-64, 65):
        a = Fraction(j, 64)
        v = prm * a if kind == "demand_centered" else prm * (a + 1) / 2
        if v.denominator == 2:
            out.append((float(a), v))
    return out


@functools.lru_cache(maxsize=None)
def patterns(kind: str, prm: int, wide: bool = True) -> np.ndarray:
    f = np.float32
    vals = [f(-1.0), f(1.0), f(0.0), f(-0.0), np.nextafter(f(-1), f(0)), np.nextafter(f(1), f(0))]
    if wide:
        vals += [np.nextafter(f(-1), f(-2)), np.nextafter(f(1), f(2)), f(-1.5), f(1.5), f(2.75), f(-4.0), f(4.0), f(3.999)]
    for a, _ in ties(kind, prm):
        vals += [f(a), np.nextafter(f(a), f(-8)), np.nextafter(f(a), f(8))]
    vals += [f(0.1), f(-0.3), f(0.61803), f(-0.7071)]  # and a few that are nothing special
    return np.array(vals, np.float32)


def params(c: Case):
    return [BIG] * c.K if c.big else [PARAMS[k % len(PARAMS)] for k in range(c.K)]


@functools.lru_cache(maxsize=None)
def actions(name: str, steps: Optional[int] = None) -> np.ndarray:
    """[T + 1][E, W, K] float32 (one step past the episode's end)."""
    c = CASE_BY_NAME[name]
    n = (c.T + 1) if steps is None else steps
    out = np.zeros((n, E, c.W, c.K), np.float32)
    for k, prm in enumerate(params(c)):
        p = patterns(c.action, prm, wide=not c.big)
        assert len(p) <= E - 4
        for t in range(n):
            for w in range(c.W):
                out[t, :, w, k] = p[(np.arange(E) + 5 * t + 3 * w + k) % len(p)]
    for e in range(4):  # -1, +1, +0, -0 on every component, every step
        out[:, e] = patterns(c.action, 20)[e]
    if c.big:
        # one SKU per warehouse orders, the others hold -1 (a target of 0): the limit is on the pending
        # total of a warehouse, the observation's float32 sum over all its SKUs and slots
        for w in range(c.W):
            out[:, :, w, [k for k in range(c.K) if k != w % c.K]] = -1.0
    return out


def random_actions(name: str, steps: int = 30) -> np.ndarray:
    c = CASE_BY_NAME[name]
    return np.random.default_rng(11).uniform(-1, 1, size=(steps, E, c.W, c.K)).astype(np.float32)


# ---- traces -----------------------------------------------------------------------------------
def _steps(c: Case):
    rng = np.random.default_rng(sum(map(ord, c.name)))
    K, R = c.K, c.R

    def unit(s, q):
        v = np.zeros(K, np.int64)
        v[s] = q
        return v

    steps = []
    for t in range(c.T):
        if t == 3:  # nothing but zero-quantity orders
            steps.append([(r, np.zeros(K, np.int64)) for r in range(R)] + [(1, np.zeros(K, np.int64))])
            continue
        orders = [(0, unit(0, 2 if t == 4 else 1))]
        for r in range(1, R - 1):
            for _ in range(int(rng.integers(2, 5))):
                q = np.zeros(K, np.int64)
                n = int(rng.integers(1, min(K, 3) + 1))
                q[rng.choice(K, n, replace=False)] = rng.integers(1, 9 + 3 * c.W, n)  # enough to run some stock out
                orders.append((r, q))
        if t < 2:
            orders.append((R - 1, unit(K - 1, 1)))
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


def initial_inventory(c: Case):
    inv = [[0 if (w + k) % 3 == 0 or w == 1 else 5 + (7 * w + 3 * k) % 20 for k in range(c.K)] for w in range(c.W)]
    return inv


def expected_lead_times(c: Case):
    if c.lead == "mixed":
        return [[1 + (w + 2 * k) % 6 for k in range(c.K)] for w in range(c.W)]
    if c.lead == "stoch":
        return [[1 + (w + k) % 4 for k in range(c.K)] for w in range(c.W)]
    return [[int(c.lead)] * c.K for _ in range(c.W)]


@functools.lru_cache(maxsize=None)
def make_spec(name: str, demand: str = "empirical", episode_length: Optional[int] = None) -> EnvSpec:
    c = CASE_BY_NAME[name]
    cfg = make_synthetic_env_config(c.W, c.R, c.K, episode_length=episode_length or c.T, features=FEATURES[c.features],
                                    scope=c.scope)
    key = {"direct": "max_order_quantities", "demand_centered": "max_quantity_adjustment", "base_stock": "max_stock_level"}
    cfg["action_space"] = {"type": c.action, "params": {key[c.action]: params(c)}}
    cfg["initial_inventory"] = {"type": "custom", "params": {"values": initial_inventory(c)}}
    lt = {"expected_lead_times": expected_lead_times(c)}
    if c.deviation is not None:
        dev = list(c.deviation) if isinstance(c.deviation, tuple) else c.deviation
        lt["deviation"] = {"type": "uniform", "max_deviation": dev}
    cfg["components"]["lead_time_sampler"] = {"type": "stochastic" if c.deviation is not None else "fixed", "params": lt}
    meta = {"include_warehouse_id": True, "obs_normalization": c.norm}
    if demand == "empirical":
        cfg["components"]["demand_sampler"] = {"type": "empirical", "params": None}
        meta["demand_trace"] = trace_frame(c)
    return EnvSpec.from_config(cfg, meta)


# ---- phase B's record ---------------------------------------------------------------------------
def trace_provider(spec: EnvSpec):
    """Phase B from tests/alloc_emulation.py on the spec's trace: independent of the project."""
    def provide(t, inventory):
        tr = spec.trace
        lo, hi = int(tr["offsets"][t]), int(tr["offsets"][t + 1])
        after, info = alloc.allocate(tr["regions"][lo:hi], tr["quantities"][lo:hi], inventory, spec.outbound_fixed,
                                     spec.outbound_variable, spec.sku_weights, spec.max_splits, n_regions=spec.R)
        lost = alloc.lost_sales(spec.lost_type, info, spec.outbound_fixed, spec.outbound_variable, spec.sku_weights,
                                spec.distances, spec.lost_alpha)
        cost = alloc.costs(after, lost, info, spec.outbound_fixed, spec.outbound_variable, spec.sku_weights,
                           float(spec.holding[0]), spec.penalty)
        return {"shipped": info["shipment_quantities_by_sku"], "demand_per_region": info["demand_per_region"],
                "lost_sales": lost, "penalty": cost[:, 1], "outbound": cost[:, 2]}
    return provide


def info_provider(infos):
    """Phase B from the msc_step_info arrays of a twin handle (a list of per-step dicts of numpy
    arrays, indexed by the call, not by the timestep)."""
    it = iter(infos)

    def provide(t, inventory):
        h = next(it)
        return {"shipped": h["shipment_quantities_by_sku"], "demand_per_region": h["demand_per_region"],
                "lost_sales": h["lost_sales"], "penalty": h["costs"][:, 1], "outbound": h["costs"][:, 2]}
    return provide


@functools.lru_cache(maxsize=None)
def emulated(name: str, mutant: Optional[str] = None, random: bool = False):
    """(reset obs, per-step dicts, lead-time generator states [E, 6]) of a trace-driven case under
    its designed actions (T + 1 steps) or 30 steps of uniform random ones."""
    spec = make_spec(name)
    act = random_actions(name) if random else actions(name)
    reset_obs, steps, em = se.run(spec, E, act, trace_provider(spec), base_seed=BASE_SEED, mutant=mutant)
    return reset_obs, steps, np.stack([se.generator_words(g) for g in em.lead_rng])


@functools.lru_cache(maxsize=None)
def oracle_episode(name: str, random: bool = False):
    """The C oracle on the same case and actions, with its step info."""
    import oracle as orc
    spec = make_spec(name)
    act = random_actions(name) if random else actions(name)
    ref = orc.OracleEnv(spec, E, base_seed=BASE_SEED)
    out = {"reset_obs": ref.reset().copy(), "steps": []}
    for a in act:
        info = ref.alloc_info()
        obs, rew, tr, fo = ref.step(a, info=info, final_obs=True, n_threads=4)
        out["steps"].append({"obs": obs, "rew": rew, "tr": tr, "fo": fo, "info": info,
                             "inventory": ref.read_state()["inventory"].copy()})
    out["rng"] = ref.read_state()["rng"].copy()
    return out
