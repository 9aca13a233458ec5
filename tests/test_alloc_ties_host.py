"""The allocators' tie rule and stock edges on hand-built order traces, on the CPU: the C oracle
step for step against the numpy restatement of the reference's allocator
(tests/alloc_emulation.py), over the case table of tests/alloc_cases.py.

The reference's own `np.argsort` is not stable at four or more warehouses on every host, so the
project's rule -- lowest warehouse index first on equal cost -- is pinned here on costs that
actually tie. Each tie case must be sensitive to the rule (the emulation under the opposite rule
leaves another inventory after step 0) and the near-tie case to the two-rounding cost (a fused
evaluation ranks at least one order differently): a case that is not is a broken case.
"""
from fractions import Fraction

import numpy as np
import pytest

import alloc_cases as ac
import alloc_emulation as emu
import oracle as orc

IDS = [c.name for c in ac.CASES]


def test_near_tie_numbers_have_the_property():
    # the hard-coded search result: fused and two-rounding values differ by one ulp, in opposite
    # directions for the two quantities, and row B's exact cost equals the two-rounding value
    for q, want, sign in zip(ac.NT_Q, ac.NT_TWO_ROUNDING, (1, -1)):
        tw = emu.order_weight([q], [ac.NT_W0])
        two = ac.NT_OF + ac.NT_OV * tw
        fused = float(Fraction(ac.NT_OF) + Fraction(ac.NT_OV) * Fraction(tw))
        assert two == want
        assert (fused > two) if sign > 0 else (fused < two)
        assert abs(fused - two) == np.spacing(min(fused, two))
        of, ov = ac.cost_tables("near", 4, 3)
        r = ac.NT_Q.index(q)
        c2 = emu.order_costs(of[:, r], ov[:, r], tw)
        cf = emu.order_costs(of[:, r], ov[:, r], tw, fused=True)
        assert c2[0] == c2[1] == c2[2] == c2[3]
        assert list(emu.ranking(c2)) == [0, 1, 2, 3]
        assert list(emu.ranking(cf)) == ([1, 3, 0, 2] if sign > 0 else [0, 2, 1, 3])


def test_case_table_covers_the_shapes():
    by = lambda f: {f(c) for c in ac.CASES}  # noqa: E731
    assert by(lambda c: c.W) >= {4, 5, 8, 12, 16, 17, 24, 32}
    assert by(lambda c: c.K) >= {1, 2, 5, 9} and all(c.W > 16 for c in ac.CASES if c.K == 9)
    assert {c.max_splits for c in ac.CASES if c.name.startswith("splits")} >= {0, 1}
    assert any(c.max_splits == c.W - 1 for c in ac.CASES if c.name.startswith("splits"))
    assert {c.lost for c in ac.CASES if c.trace == "starve"} == {"shipment", "cost", "closest"}
    counts = {n for c in ac.CASES if c.trace == "counts" for n in c.orders}
    assert counts >= {1, 63, 64, 65, 129}
    assert len(IDS) == len(set(IDS))
    for c in ac.CASES:
        d = ac.distance_table(c.W, c.R, c.unshared)
        homes = np.argmin(d, axis=1)
        assert (len(set(homes.tolist())) == c.W) == c.unshared, c.name
        if c.trace == "starve":  # two warehouses tie for closest in every region
            assert all((d[:, r] == d[:, r].min()).sum() == 2 for r in range(c.R)), c.name


@pytest.mark.parametrize("name", IDS)
def test_oracle_matches_emulation(name):
    c = ac.CASE_BY_NAME[name]
    spec, inv0, epi = ac.reference_episode(name)
    assert spec.trace["n_rows"] == spec.episode_length == c.T
    ref = orc.OracleEnv(spec, ac.E, base_seed=ac.BASE_SEED)
    ref.reset()
    np.testing.assert_array_equal(ref.read_state()["inventory"], inv0)
    assert len(np.unique(inv0.reshape(ac.E, -1), axis=0)) > ac.E // 2, "the envs of the batch must differ"
    act = -np.ones((ac.E, spec.W, spec.K), np.float32)
    for t, want in enumerate(epi):
        assert want["demand_per_region"].max() < ac.MAX_ADJ
        info = ref.alloc_info()
        _, _, tr, _ = ref.step(act, info=info, n_threads=4)
        msg = f"{name} t={t}"
        assert not info["order_quantities"].any(), msg  # nothing is ever replenished
        np.testing.assert_array_equal(info["inventory_before"], want["inventory_before"], err_msg=msg)
        np.testing.assert_array_equal(info["n_orders"], want["n_orders"], err_msg=msg)
        for k in emu.INT_KEYS:
            np.testing.assert_array_equal(info[k], want[k], err_msg=f"{msg} {k}")
        np.testing.assert_array_equal(info["fulfilled_per_warehouse"], want["inventory_before"] - want["inventory"], err_msg=msg)
        np.testing.assert_allclose(info["lost_sales"], want["lost_sales"], rtol=1e-9, atol=1e-9, err_msg=msg)
        np.testing.assert_allclose(info["costs"], want["costs"], rtol=1e-9, atol=1e-7, err_msg=msg)
        assert tr.all() == (t == c.T - 1) and tr.all() == tr.any()
        if not tr.any():
            np.testing.assert_array_equal(ref.read_state()["inventory"], want["inventory"], err_msg=msg)


@pytest.mark.parametrize("name", IDS)
def test_case_reaches_its_states(name):
    # what each case is for, shown on the emulation alone
    c = ac.CASE_BY_NAME[name]
    spec, inv0, epi = ac.reference_episode(name)
    lost = np.stack([s["lost_order_counts"].sum(axis=1) for s in epi])  # [T, E]
    splits = np.stack([(s["shipment_counts"].sum(axis=(1, 2)) > s["n_orders"]) for s in epi])
    if c.max_splits is None:
        assert (lost[0] == 0).mean() > 0.5, "abundant stock at the start"
    # (with a split limit an env may keep enough in single warehouses to the end)
    assert (lost[-1] > 0).mean() > (0.9 if c.max_splits is not None else 0.999), "orders are lost by the end of the episode"
    if c.max_splits != 0:
        assert splits.any(axis=0).mean() > 0.5, "orders are split between warehouses"
    other = ac.emulate_episode(spec, inv0, tie="high", steps=1)  # every case holds tied costs
    differs = (other[0]["inventory"] != epi[0]["inventory"]).any(axis=(1, 2))
    assert differs.all(), f"the opposite tie rule must show at step 0 in every env ({differs.mean():.2f})"
    if c.table == "near":
        fused = ac.emulate_episode(spec, inv0, fused=True, steps=1)
        assert (fused[0]["inventory"] != epi[0]["inventory"]).any(axis=(1, 2)).all(), "a fused cost must show at step 0"
        n_flip = 0
        for reg, qty in zip(*ac.step_orders(spec, 0)):
            tw = emu.order_weight(qty, spec.sku_weights)
            a = emu.ranking(emu.order_costs(spec.outbound_fixed[:, reg], spec.outbound_variable[:, reg], tw))
            b = emu.ranking(emu.order_costs(spec.outbound_fixed[:, reg], spec.outbound_variable[:, reg], tw, fused=True))
            n_flip += int(not np.array_equal(a, b))
        assert n_flip >= 2
    if c.table == "crossing":  # orders below, at and above the tie weight in every step with more than two orders
        for t in (t for t in range(c.T) if epi[t]["n_orders"] > 2):
            tws = {emu.order_weight(q, spec.sku_weights) for q in ac.step_orders(spec, t)[1]}
            assert min(tws) < 4.0 and 4.0 in tws and max(tws) > 4.0
    if c.trace == "starve":
        assert not epi[-1]["inventory"].any(), "every warehouse is empty at the end"
        # a step that starts with every warehouse empty in some env: nothing shipped to any region
        assert any((~s["inventory_before"].any(axis=(1, 2))).any() for s in epi)
    if c.name.startswith("splits"):
        # a tied lower-index warehouse that holds none of the wanted SKUs is passed over, and the
        # limit leaves orders unfilled while other warehouses still hold what they want
        passed_over = 0
        for t, s in enumerate(epi):  # the step's first order: warehouse 0 holds none of its SKUs, a later one does
            need = ac.step_orders(spec, t)[1][0] > 0
            before = s["inventory_before"][:, :, need]
            passed_over += int(((before[:, 0] == 0).all(axis=1) & (before[:, 1:] > 0).any(axis=(1, 2))).sum())
        assert passed_over > ac.E, "empty tied lower-index warehouses must be passed over"
        if c.max_splits < c.W - 1:
            left = np.stack([(s["lost_order_counts"].sum(axis=1) > 0) & s["inventory"].any(axis=(1, 2)) for s in epi])
            assert left.any(), "max_splits must end an order while stock remains"
    if c.trace == "counts":
        assert tuple(s["n_orders"] for s in epi) == c.orders
        assert any((q == 0).all() for t in range(c.T) for q in ac.step_orders(spec, t)[1]), "an empty order"
    if c.trace == "wide":
        assert max(int(ac.step_orders(spec, t)[1].max()) for t in range(c.T)) == 65535
        assert inv0.min() < 65535 < inv0.max()
        assert any((s["shipment_quantities_by_sku"] == 65535).any() for s in epi), "a fill of the whole field"
