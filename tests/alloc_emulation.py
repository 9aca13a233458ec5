"""An independent restatement of the reference's greedy demand allocation
(src/environment/components/demand_allocator.py:118-217), of its three lost-sales handlers
(lost_sales_handler.py:71-210) and of the cost breakdown (reward_calculator.py:127-152) in plain
numpy, written from the reference's behaviour and vectorised over the envs of a batch.

The reference ranks the warehouses of an order with `np.argsort(of[:, r] + ov[:, r] * tw)`, whose
order among equal costs depends on the host (parity hazard 1). The project's rule is
the stable one, lowest warehouse index first, and this module states it as
`np.argsort(kind="stable")`. `tie="high"` is the opposite rule (highest index first) and
`fused=True` ranks by the cost evaluated with one rounding (exact product and sum, rounded once,
as an FMA would); both exist only to prove that a test case is sensitive to the rule or to the
two-rounding evaluation, never as a reference.

The ranking of an order does not depend on the env, only the stock does, so an order is ranked
once and each warehouse of the ranking serves all envs at once.
"""
from __future__ import annotations

from fractions import Fraction

import numpy as np

INT_KEYS = ("shipment_counts", "shipment_quantities", "shipment_quantities_by_sku", "unfulfilled_demands",
            "lost_order_counts", "demand_per_region")


def order_weight(q, sku_weights) -> float:
    """sku_demands.dot(sku_weights) in float64, one product and one sum at a time."""
    tw = 0.0
    for s in range(len(q)):
        tw += float(q[s]) * float(sku_weights[s])
    return tw


def order_costs(of_r, ov_r, tw, *, fused=False) -> np.ndarray:
    """Cost of every warehouse for an order of weight tw in one region: the product rounded, then
    the sum rounded (numpy's `of + ov * tw`); fused: the exact value rounded once."""
    if not fused:
        return np.asarray(of_r, np.float64) + np.asarray(ov_r, np.float64) * np.float64(tw)
    return np.array([float(Fraction(float(a)) + Fraction(float(b)) * Fraction(float(tw))) for a, b in zip(of_r, ov_r)])


def ranking(costs, tie="low") -> np.ndarray:
    """Warehouses by ascending cost; equal costs by ascending (tie="low") or descending index."""
    if tie == "low":
        return np.argsort(costs, kind="stable")
    n = len(costs)
    return n - 1 - np.argsort(np.asarray(costs)[::-1], kind="stable")


def allocate(regions, quantities, inventory, of, ov, sku_weights, max_splits, *, n_regions, tie="low", fused=False):
    """One step's allocation for a batch of envs that receive the same orders.

    regions [n], quantities [n, K]: the step's orders in their packed order; inventory [E, W, K]
    at allocation time; of / ov [W, R]. Returns (inventory after, info) with info's arrays shaped
    [E, ...] like msc_step_info's, all integer."""
    inv = np.array(inventory, dtype=np.int64)
    E, W, K = inv.shape
    R = n_regions
    cnt = np.zeros((E, W, R), np.int64)
    qbys = np.zeros((E, W, R, K), np.int64)
    unf = np.zeros((E, R, K), np.int64)
    lost_n = np.zeros((E, R), np.int64)
    dpr = np.zeros((R, K), np.int64)
    max_wh = max_splits + 1
    for r, q in zip(np.asarray(regions).tolist(), np.asarray(quantities, np.int64)):
        dpr[r] += q
        rank = ranking(order_costs(of[:, r], ov[:, r], order_weight(q, sku_weights), fused=fused), tie)
        rem = np.broadcast_to(q, (E, K)).copy()
        used = np.zeros(E, np.int64)
        for w in rank.tolist():
            # an order is open while it still wants something and may use another warehouse
            open_ = (used < max_wh) & (rem > 0).any(axis=1)
            if not open_.any():
                break
            fill = np.minimum(rem, inv[:, w]) * open_[:, None]
            ships = (fill > 0).any(axis=1)  # a warehouse with nothing to give is no shipment
            cnt[:, w, r] += ships
            qbys[:, w, r] += fill
            rem -= fill
            inv[:, w] -= fill
            used += ships
        left = (rem > 0).any(axis=1)
        unf[:, r] += rem * left[:, None]
        lost_n[:, r] += left
    info = {"shipment_counts": cnt, "shipment_quantities": qbys.sum(axis=3), "shipment_quantities_by_sku": qbys,
            "unfulfilled_demands": unf, "lost_order_counts": lost_n,
            "demand_per_region": np.broadcast_to(dpr, (E, R, K)).copy()}
    return inv, info


def lost_sales(kind, info, of, ov, sku_weights, distances, alpha=None) -> np.ndarray:
    """Unfulfilled demand assigned to warehouses, [E, W, K] float64: `closest` gives a region's to
    its closest warehouse (first minimum of the distance column), `shipment` shares it by units
    shipped to the region and falls back to the closest warehouse when nothing was shipped there,
    `cost` shares it by a softmax of -(of * lost orders + ov * lost weight) / alpha."""
    unf = info["unfulfilled_demands"].astype(np.float64)
    E, R, K = unf.shape
    W = of.shape[0]
    closest = np.argmin(distances, axis=0)
    out = np.zeros((E, W, K))
    for r in range(R):
        if kind == "closest":
            wts = np.zeros((E, W))
            wts[:, closest[r]] = 1.0
        elif kind == "shipment":
            shipped = info["shipment_quantities"][:, :, r].astype(np.float64)
            tot = shipped.sum(axis=1)
            wts = np.zeros((E, W))
            wts[:, closest[r]] = 1.0
            some = tot > 0
            wts[some] = shipped[some] / tot[some, None]
        else:
            lw = np.zeros(E)
            for s in range(K):
                lw = lw + unf[:, r, s] * sku_weights[s]
            logits = -(of[None, :, r] * info["lost_order_counts"][:, r, None].astype(np.float64)
                       + ov[None, :, r] * lw[:, None]) / alpha
            ex = np.exp(logits - logits.max(axis=1, keepdims=True))
            wts = ex / ex.sum(axis=1, keepdims=True)
        out += wts[:, :, None] * unf[:, None, r, :]
    return out


def costs(inv_after, lost, info, of, ov, sku_weights, holding, penalty) -> np.ndarray:
    """[E, 4, W]: holding, penalty, outbound and inbound cost per warehouse of a step in which
    nothing is ordered (inbound is zero); holding is the scalar rate per unit weight, penalty the
    per-SKU list."""
    skw = np.asarray(sku_weights, np.float64)
    hold = (inv_after * skw * holding).sum(axis=2)
    pen = (lost * np.asarray(penalty, np.float64)).sum(axis=2)
    fixed = (info["shipment_counts"] * of).sum(axis=2)
    var = ((info["shipment_quantities_by_sku"] * skw).sum(axis=3) * ov).sum(axis=2)
    return np.stack([hold, pen, fixed + var, np.zeros_like(hold)], axis=1)
