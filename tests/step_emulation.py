"""An independent restatement of what the reference does around its allocator, in plain numpy:
placing replenishment orders and receiving them (multi_env.py:795-919, "phase A"), the stochastic
lead times (lead_time_sampler.py:169-197), and costs, reward, forecast, history and observations
(multi_env.py:548-793, 941-968, reward_calculator.py:127-190, "phase C"), with the reset and the step
across the episode boundary (multi_env.py:192-251). Written from the reference's behaviour and
vectorised over the envs of a batch, which step in lockstep.

It keeps no ring. A pending order is an entry (quantity, actual arrival, expected arrival) of the
queue of its (warehouse, SKU); the queues of a batch are held as one list of the orders placed per
step, each a set of [E, W, K] arrays with a `live` mask, so "for entry in queue" is a loop over
that list in placing order, which is the order every float32 accumulation below depends on.

Every operation has the dtype the reference gives it under numpy >= 2 promotion: `(action + 1.0) /
2.0` stays float32, its product with the float64 parameter is float64, `np.round` rounds half to
even, pending and pipeline totals are float32 sums taken entry by entry, a numpy float32 scalar
plus the python float `eps` stays float32 while a python float plus `eps` is float64, and sums
over SKUs are numpy's own `sum` over a contiguous last axis (pairwise from 8 elements on), checked
against the one-row form in tests/test_step_cases_host.py.

Phase B enters as a record (see `settle`), from tests/alloc_emulation.py on trace-driven cases, so
that the whole episode is independent of the project, or from the msc_step_info arrays of a twin
handle. Lead times are drawn by numpy's own Generator from the reference's seed derivation.

`mutant` names one deliberate defect (MUTANTS); it exists only to show that a designed case is
sensitive to that defect, never as a reference.
"""
from __future__ import annotations

from collections import deque

import numpy as np
from numpy.random import SeedSequence, default_rng

f32, f64 = np.float32, np.float64
ROLLING_WINDOW = 5  # multi_env.py:147
EMA_ALPHA = 0.3     # multi_env.py:150

MUTANTS = {
    "round_half_up": "rescale rounds x.5 up instead of to even",
    "half_in_f64": "(a + 1) / 2 evaluated in float64",
    "direct_unclamped": "direct: no clamp to max_order_quantities",
    "others_clamped": "demand_centered / base_stock: quantity clamped to the parameter",
    "pending_ignored": "base_stock: pending orders not subtracted",
    "arrival_ge": "an order arrives when timestep >= actual arrival (equivalent: see the host test)",
    "arrival_first": "arrivals received before the action is rescaled and the order queued",
    "bucket_off_by_one": "pipeline slot counted from the next timestep",
    "overdue_dropped": "orders past their expected arrival left out of the pipeline",
    "eps_width": "float32 eps where the reference has float64 and the reverse",
    "history_oldest_first": "demand history oldest first",
    "std_ddof1": "demand variability divided by n_hist - 1",
    "inbound_fixed_on_zero": "inbound fixed cost charged on a zero order",
    "team_sum_reversed": "team reward summed from the last warehouse down, one at a time",
    "draws_warehouse_major": "per-SKU deviations drawn warehouse by warehouse",
}


def component_seed(base_seed: int, env: int, counter: int, child: int) -> SeedSequence:
    """SeedManager: derive_env_seed -> advance_episode -> _spawn_seeds (seed_manager.py:100-224);
    children are (preprocessing, inventory, demand_sampler, lead_time_sampler)."""
    root = int(SeedSequence([base_seed, 0, env]).generate_state(1, dtype=np.uint32)[0])
    episode_root = int(SeedSequence([root, counter]).generate_state(1, dtype=np.uint32)[0])
    return SeedSequence(episode_root).spawn(4)[child]


def generator_words(g) -> np.ndarray:
    """A numpy PCG64 Generator's state as [state_hi, state_lo, inc_hi, inc_lo, has_uint32, uinteger]."""
    st = g.bit_generator.state
    s, i, m = st["state"]["state"], st["state"]["inc"], (1 << 64) - 1
    return np.array([s >> 64, s & m, i >> 64, i & m, st["has_uint32"], st["uinteger"]], dtype=np.uint64)


class StepEmulation:
    def __init__(self, spec, n_envs: int, *, base_seed: int, mutant: str | None = None):
        assert mutant is None or mutant in MUTANTS, mutant
        assert spec.obs_normalization in ("off", "ratio")
        self.spec, self.E, self.base_seed, self.mutant = spec, n_envs, base_seed, mutant
        self.param = np.asarray(spec.action_param, f64)
        self.expected = np.asarray(spec.expected_lead_times, np.int64)
        self.horizon = int(self.expected.max())
        self.home = np.argmin(spec.distances, axis=1)
        self.counter = 0

    # ---- reset (multi_env.py:192-251) ------------------------------------------------------
    def reset(self) -> np.ndarray:
        sp, E = self.spec, self.E
        shape = (E, sp.W, sp.K)
        self.lead_rng = [default_rng(component_seed(self.base_seed, e, self.counter, 3)) for e in range(E)]
        if sp.init_type == "uniform":
            inv = np.stack([default_rng(component_seed(self.base_seed, e, self.counter, 1))
                            .integers(sp.init_min, sp.init_max + 1, size=shape[1:]) for e in range(E)])
        elif sp.init_type == "custom":
            inv = np.broadcast_to(np.asarray(sp.init_values, np.int64), shape)
        else:
            inv = np.zeros(shape, np.int64)
        self.counter += 1
        self.inventory = inv.astype(f64)
        self.queue = []
        self.demand_home = np.zeros(shape, f32)
        self.shipped_home = np.zeros(shape, f32)
        self.shipped_away = np.zeros(shape, f32)
        self.stockout = np.zeros(shape, f32)
        self.rolling_mean = np.zeros(shape, f32)
        self.forecast = np.zeros(shape, f32)
        self.history = deque(maxlen=ROLLING_WINDOW)
        self.t = 0
        return self._observations()

    # ---- phase A ----------------------------------------------------------------------------
    def _pending(self) -> np.ndarray:
        p = np.zeros((self.E, self.spec.W, self.spec.K), f32)
        for en in self.queue:  # sku_pending[sku] += entry.quantity, a float32 sum entry by entry
            p = p + np.where(en["live"], en["quantity"], 0.0).astype(f32)
        return p

    def _round(self, x):
        return np.floor(x + 0.5) if self.mutant == "round_half_up" else np.round(x)

    def _quantities(self, a: np.ndarray) -> np.ndarray:
        """_rescale_actions_to_quantities (multi_env.py:795-848); a is float32 [E, W, K]."""
        kind, prm, m = self.spec.action_type, self.param, self.mutant
        half = (a.astype(f64) + 1.0) / 2.0 if m == "half_in_f64" else ((a + f32(1.0)) / f32(2.0)).astype(f64)
        if kind == "direct":
            q = self._round(half * prm).astype(np.int64)
            q = np.maximum(q, 0) if m == "direct_unclamped" else np.clip(q, 0, prm)
        elif kind == "demand_centered":
            adjustment = self._round(prm * a.astype(f64)).astype(np.int64)
            q = np.maximum(0, adjustment + self.demand_home.astype(np.int64))
        else:
            target = half * prm
            pending = np.zeros_like(self._pending()) if m == "pending_ignored" else self._pending()
            q = np.maximum(0, self._round(target - self.demand_home - pending)).astype(np.int64)
        if m == "others_clamped" and kind != "direct":
            q = np.minimum(q, prm)
        return np.asarray(q, f64)

    def _lead_times(self) -> np.ndarray:
        """lead_time_sampler.sample() of every env, drawn whether or not anything is ordered."""
        sp = self.spec
        if sp.lead_type != "stochastic":
            return np.broadcast_to(self.expected, (self.E, sp.W, sp.K))
        out = np.empty((self.E, sp.W, sp.K), np.int64)
        for e, g in enumerate(self.lead_rng):
            if sp.max_dev_per_sku and self.mutant == "draws_warehouse_major":
                dev = np.array([[g.integers(-d, d + 1) for d in sp.max_deviation.tolist()] for _ in range(sp.W)])
            elif sp.max_dev_per_sku:
                dev = np.column_stack([g.integers(-d, d + 1, size=sp.W) for d in sp.max_deviation.tolist()])
            else:
                d = int(sp.max_deviation[0])
                dev = g.integers(-d, d + 1, size=(sp.W, sp.K))
            out[e] = np.maximum(1, self.expected + dev)
        return out

    def _arrivals(self):
        for en in self.queue:
            due = (en["actual"] <= self.t) if self.mutant == "arrival_ge" else (en["actual"] == self.t)
            due = due & en["live"]
            self.inventory = self.inventory + np.where(due, en["quantity"], 0.0)
            en["live"] = en["live"] & ~due
        self.queue = [en for en in self.queue if en["live"].any()]

    def place_and_receive(self, actions) -> dict:
        """Steps 1 and 2 of step() (multi_env.py:287-292). Returns what collect_step_info records
        before the step, the quantities ordered and the inventory the allocator then sees."""
        a = np.ascontiguousarray(actions, f32).reshape(self.E, self.spec.W, self.spec.K)
        before, pending = self.inventory.copy(), self._pending()
        if self.mutant == "arrival_first":
            self._arrivals()
        q = self._quantities(a)
        lead = self._lead_times()
        valid = q > 0
        if valid.any():
            self.queue.append({"quantity": q, "actual": self.t + lead, "expected": self.t + self.expected,
                               "live": valid})
        self.ordered = np.where(valid, q, 0.0)
        if self.mutant != "arrival_first":
            self._arrivals()
        return {"inventory_before": before.astype(np.int64), "pending_total": pending.astype(np.int64),
                "order_quantities": self.ordered.astype(np.int64), "inventory": self.inventory.astype(np.int64)}

    # ---- phase C ----------------------------------------------------------------------------
    def settle(self, rec: dict) -> dict:
        """Steps 5 to 10 of step() (multi_env.py:306-327) from phase B's record: `shipped`
        [E, W, R, K] units, `demand_per_region` [E, R, K], `lost_sales` [E, W, K], `penalty` and
        `outbound` [E, W] costs. Returns obs, float64 rewards, costs [E, 4, W], the truncation flag
        and, at the episode's end, the final observation (obs is then the next episode's first)."""
        sp, E = self.spec, self.E
        shipped = np.asarray(rec["shipped"], f64)
        self.inventory = np.maximum(self.inventory - shipped.sum(axis=2), 0.0)
        # _update_observations
        demand = np.asarray(rec["demand_per_region"]).astype(f32)
        self.demand_home = demand[:, self.home, :]
        self.shipped_home = shipped[:, np.arange(sp.W), self.home, :]
        self.shipped_away = shipped.sum(axis=2) - self.shipped_home
        self.stockout = np.maximum(self.demand_home - self.shipped_home, 0.0).astype(f32)
        self.history.append(self.demand_home.copy())
        self.rolling_mean = np.array(self.history).mean(axis=0).astype(f32)
        self.forecast = (EMA_ALPHA * self.demand_home + (1 - EMA_ALPHA) * self.forecast).astype(f32)
        # CostRewardCalculator.calculate
        skw = np.asarray(sp.sku_weights, f64)
        if sp.holding_per_sku:
            holding = (self.inventory * np.asarray(sp.holding, f64)).sum(axis=2)
        else:
            holding = (self.inventory * skw * float(sp.holding[0])).sum(axis=2)
        counts = (self.ordered > 0).astype(np.int64)
        if self.mutant == "inbound_fixed_on_zero":
            counts = np.ones_like(counts)
        inbound = (counts * sp.inbound_fixed).sum(axis=2) + ((self.ordered * skw) * sp.inbound_variable).sum(axis=2)
        penalty, outbound = np.asarray(rec["penalty"], f64), np.asarray(rec["outbound"], f64)
        total = holding + penalty + outbound + inbound
        if sp.scale_factor:
            total = total * sp.scale_factor
        rewards = -total
        if sp.scope == "team":
            if self.mutant == "team_sum_reversed":
                s = np.zeros(E)
                for w in reversed(range(sp.W)):
                    s = s + rewards[:, w]
            else:
                s = np.ascontiguousarray(rewards).sum(axis=1)
            rewards = np.repeat(s[:, None], sp.W, axis=1)
        obs = self._observations()
        self.t += 1
        out = {"obs": obs, "rewards": rewards, "costs": np.stack([holding, penalty, outbound, inbound], axis=1),
               "truncated": self.t >= sp.episode_length, "final_obs": None,
               "inventory": self.inventory.astype(np.int64)}
        if out["truncated"]:
            out["final_obs"] = obs
            out["obs"] = self.reset()
        return out

    # ---- observations (multi_env.py:548-745, 941-968) -----------------------------------------
    def _pipeline(self) -> np.ndarray:
        sp, H, m = self.spec, self.horizon, self.mutant
        pipe = np.zeros((self.E, sp.W, H, sp.K), f32)
        now = self.t + 1 if m == "bucket_off_by_one" else self.t
        for en in self.queue:
            slot = en["expected"] - now  # [W, K]
            for b in range(1, H + 1):
                pipe[:, :, b - 1, :] += np.where(en["live"] & (slot == b), en["quantity"], 0.0).astype(f32)
            if m != "overdue_dropped":
                pipe[:, :, 0, :] += np.where(en["live"] & (slot <= 0), en["quantity"], 0.0).astype(f32)
        return pipe

    def _observations(self) -> np.ndarray:
        sp, E, ft = self.spec, self.E, self.spec.features
        W, K = sp.W, sp.K
        ratio = sp.obs_normalization == "ratio"
        swap = self.mutant == "eps_width"
        eps = 1e-8

        def plus_eps32(total):  # a numpy float32 scalar + eps: float32
            return (total.astype(f64) + eps) if swap else (total + f32(eps))

        def plus_eps64(total):  # a python float or float64 + eps: float64
            return (total + f64(f32(eps))) if swap else (total + eps)

        def block(x, denom, agg=None):
            x = x / denom[..., None] if ratio else x
            return [x] if agg is None else [x, agg.astype(f32)[..., None]]

        inv = self.inventory
        pipe = self._pipeline()
        flat = np.ascontiguousarray(pipe.reshape(E, W, self.horizon * K))
        pending_total = flat.sum(axis=2).astype(f64)  # float(pipeline_flat.sum())
        inv_total = inv.sum(axis=2)
        demand_total = np.ascontiguousarray(self.demand_home).sum(axis=2)
        shipped_total = (self.shipped_home + self.shipped_away).sum(axis=2)
        rolling_total = self.rolling_mean.sum(axis=2)
        forecast_total = self.forecast.sum(axis=2)
        blocks = []
        blocks += block(inv, plus_eps64(inv_total), inv_total if ft["inventory_aggregate"] else None)
        # a float32 array over a python float: the divisor is cast to float32
        blocks += [flat / plus_eps64(pending_total).astype(f32)[..., None] if ratio else flat]
        if ft["pipeline_aggregate"]:
            blocks += [pending_total[..., None]]
        demand_denom = plus_eps32(demand_total)
        if ft["incoming_demand_home"]:
            blocks += block(self.demand_home, demand_denom, demand_total if ft["incoming_demand_home_aggregate"] else None)
        if ft["units_shipped_home"]:
            blocks += block(self.shipped_home, demand_denom.astype(f64))
        if ft["units_shipped_away"]:
            share = self.shipped_away.sum(axis=2) / plus_eps64(shipped_total)
            blocks += block(self.shipped_away, plus_eps64(shipped_total), share if ft["units_shipped_away_aggregate"] else None)
        if ft["stockout"]:
            blocks += block(self.stockout, demand_denom)
        if ft["rolling_demand_mean"]:
            blocks += block(self.rolling_mean, plus_eps32(rolling_total),
                            rolling_total if ft["rolling_demand_mean_aggregate"] else None)
        if ft["demand_forecast"]:
            blocks += block(self.forecast, plus_eps32(forecast_total),
                            forecast_total if ft["demand_forecast_aggregate"] else None)
        if ft["days_of_supply"]:
            blocks += [(inv / np.maximum(self.rolling_mean, 1.0)).astype(f32)]
        if ft["net_inventory_position"]:
            per_sku = np.zeros((E, W, K), f32)
            for b in range(self.horizon):  # pipeline.sum(axis=0): row after row
                per_sku = per_sku + pipe[:, :, b, :]
            blocks += [(inv + per_sku - self.forecast * self.expected).astype(f32)]
        if ft["demand_variability"]:
            if len(self.history) > 1:
                stack = np.array(self.history)
                std = stack.std(axis=0, ddof=1) if self.mutant == "std_ddof1" else stack.std(axis=0)
            else:
                std = np.zeros((E, W, K), f32)
            blocks += [std.astype(f32)]
        if ft["demand_history"]:
            hist = np.zeros((E, W, ROLLING_WINDOW, K), f32)
            past = list(self.history) if self.mutant == "history_oldest_first" else list(reversed(self.history))
            for i, d in enumerate(past):
                hist[:, :, i, :] = d
            blocks += [hist.reshape(E, W, ROLLING_WINDOW * K)]
        local = np.concatenate([np.asarray(b, f64) if b.dtype != f32 else b for b in blocks], axis=2).astype(f32)
        if sp.include_warehouse_id:
            onehot = np.broadcast_to(np.eye(W, dtype=f32), (E, W, W))
            local = np.concatenate([onehot, local], axis=2)
        return local


def run(spec, n_envs, actions, provider, *, base_seed, mutant=None):
    """Reset, then one step per entry of `actions` ([T][E, W, K] float32), across as many episode
    boundaries as that takes. provider(t, inventory [E, W, K] at allocation time) gives phase B's
    record of the step. Returns (reset obs, per-step dicts, emulation)."""
    em = StepEmulation(spec, n_envs, base_seed=base_seed, mutant=mutant)
    reset_obs, steps = em.reset(), []
    for a in actions:
        placed = em.place_and_receive(a)
        rec = provider(em.t, placed["inventory"])
        out = em.settle(rec)
        out.update(inventory_at_allocation=placed["inventory"], inventory_before=placed["inventory_before"],
                   pending_total=placed["pending_total"], order_quantities=placed["order_quantities"])
        steps.append(out)
    return reset_obs, steps, em
