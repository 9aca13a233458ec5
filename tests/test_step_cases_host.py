"""Order placement, arrivals and observations on designed actions, on the CPU: the C oracle step
for step against the numpy restatement of the reference (tests/step_emulation.py) over the case
table of tests/step_cases.py, and the mutants of the restatement that show what each case is for.

Bars: order quantities, pending totals, inventories, observations (reset, final and the next
episode's first) and the lead-time generator's state on bits; rewards within REW_ATOL, costs within
rtol 1e-9 / atol 1e-7, as everywhere else in the suite.

Each mutant (step_emulation.MUTANTS) must change the outputs of a named designed case, and the
test also says whether the comparison with the oracle at the bars above then fails and whether 30
steps of uniform random actions on the same case see the mutant at all: the ones they miss are
the gap these cases close. Two mutants cannot fail the comparison and the reason is stated where
they are listed: `arrival_ge` is no defect at all, and `team_sum_reversed` moves a float64 sum by
an ulp, far below REW_ATOL.
"""
import numpy as np
import pytest

import step_cases as sc
import step_emulation as se
from parity_util import REW_ATOL

IDS = [c.name for c in sc.CASES]


def mismatches(name, got, ref):
    """Where an emulated episode (reset obs, steps, generator words) leaves the oracle's, at the bars."""
    reset_obs, steps, words = got
    bad = []

    def bits(what, a, b):
        if not np.array_equal(a, b):
            bad.append(what)

    bits("reset obs", reset_obs, ref["reset_obs"])
    for t, (s, q) in enumerate(zip(steps, ref["steps"])):
        for k in ("order_quantities", "pending_total", "inventory_before"):
            bits(f"t={t} {k}", s[k], q["info"][k])
        bits(f"t={t} truncated", np.full(sc.E, s["truncated"]), q["tr"])
        bits(f"t={t} obs", s["obs"], q["obs"])
        if s["truncated"]:
            bits(f"t={t} final obs", s["final_obs"], q["fo"])
        else:
            bits(f"t={t} inventory", s["inventory"], q["inventory"])
        if not np.allclose(s["rewards"], q["rew"], rtol=0, atol=REW_ATOL):
            bad.append(f"t={t} rewards")
        if not np.allclose(s["costs"], q["info"]["costs"], rtol=1e-9, atol=1e-7):
            bad.append(f"t={t} costs")
    bits("lead-time generator", words, ref["rng"][:, 1, :])
    return bad


def changed(a, b):
    """Whether two emulated episodes differ in any bit of what is compared."""
    if not np.array_equal(a[0], b[0]) or not np.array_equal(a[2], b[2]):
        return True
    for s, q in zip(a[1], b[1]):
        for k in ("order_quantities", "pending_total", "inventory", "obs", "rewards", "costs"):
            if not np.array_equal(s[k], q[k]):
                return True
        if s["truncated"] and not np.array_equal(s["final_obs"], q["final_obs"]):
            return True
    return False


def test_last_axis_sums_are_numpys_row_sums():
    # the restatement sums [E, W, n] arrays over their contiguous last axis where the reference sums
    # one row: the same pairwise routine, shown on every length the cases reach
    rng = np.random.default_rng(0)
    for n in list(range(1, 40)) + [48, 80, 96]:
        for dt in (np.float32, np.float64):
            x = (rng.uniform(0, 1000, size=(3, 5, n)) * rng.integers(0, 2, size=(3, 5, n))).astype(dt)
            rows = np.array([[x[i, j].copy().sum() for j in range(5)] for i in range(3)], dt)
            np.testing.assert_array_equal(x.sum(axis=2), rows)
    h = rng.uniform(0, 9, size=(5, 3, 4, 6)).astype(np.float32)  # history: mean / std over the leading axis
    for i in range(3):
        for w in range(4):
            np.testing.assert_array_equal(h.mean(axis=0)[i, w], np.array(list(h[:, i]))[:, w, :].mean(axis=0))
            np.testing.assert_array_equal(h.std(axis=0)[i, w], np.array(list(h[:, i]))[:, w, :].std(axis=0))


def test_case_table_covers_the_issue():
    by = lambda f: {f(c) for c in sc.CASES}  # noqa: E731
    assert by(lambda c: (c.W, c.K)) >= {(4, 2), (8, 5), (8, 6), (16, 8), (17, 3), (8, 9), (24, 12), (32, 16), (17, 10)}
    assert by(lambda c: c.action) == {"direct", "demand_centered", "base_stock"}
    assert {c.action for c in sc.CASES if (c.W, c.K, c.lead) == (8, 5, 3)} == {"direct", "demand_centered", "base_stock"}
    assert by(lambda c: c.features) == set(sc.FEATURES) and by(lambda c: c.norm) == {"ratio", "off"}
    assert by(lambda c: c.scope) == {"agent", "team"} and all(6 <= c.T <= 12 for c in sc.CASES)
    assert {type(c.deviation) for c in sc.CASES if c.deviation is not None} == {int, tuple}
    assert all(0 in c.deviation for c in sc.CASES if isinstance(c.deviation, tuple))
    assert len(IDS) == len(set(IDS))
    # the ties: odd and even x for every action type, and each parameter ties somewhere
    for kind in ("direct", "demand_centered"):
        xs = [int(v - sc.Fraction(1, 2)) for p in sc.PARAMS for _, v in sc.ties(kind, p)]
        assert any(x % 2 for x in xs) and any(x % 2 == 0 for x in xs)
        assert all(sc.ties(kind, p) for p in sc.PARAMS)
    assert [a for a, _ in sc.ties("direct", 20)] == [-0.75, -0.25, 0.25, 0.75]
    assert [float(v) for _, v in sc.ties("direct", 25)] == [12.5] and [float(v) for _, v in sc.ties("direct", 7)] == [3.5]
    for c in sc.CASES:  # every pattern of every SKU in every step
        act = sc.actions(c.name)
        for k, prm in enumerate(sc.params(c)[:1 if c.big else None]):  # (big: SKU 0 is warehouse 0's ordering one)
            want = set(sc.patterns(c.action, prm, wide=not c.big).view(np.uint32).tolist())
            for t in range(c.T + 1):
                assert set(act[t, 4:, 0, k].view(np.uint32).tolist()) == want, (c.name, t, k)
        assert np.isfinite(act).all() and np.abs(act).max() == (1.0 if c.big else 4.0)
        spec = sc.make_spec(c.name)
        assert spec.trace["n_rows"] == spec.episode_length == c.T
        assert (np.asarray(sc.initial_inventory(c))[1] == 0).all()


@pytest.mark.parametrize("name", IDS)
def test_oracle_matches_emulation(name):
    assert mismatches(name, sc.emulated(name), sc.oracle_episode(name)) == []


@pytest.mark.parametrize("name", IDS)
def test_case_reaches_its_states(name):
    # what the cases are for, shown on the emulation alone
    c = sc.CASE_BY_NAME[name]
    spec = sc.make_spec(name)
    _, steps, _ = sc.emulated(name)
    act = sc.actions(name)
    first = steps[:c.T]
    oq = np.stack([s["order_quantities"] for s in first])  # [T, E, W, K]
    prm = np.asarray(sc.params(c))
    assert (oq[:, 4:].reshape(c.T, -1) == 0).any(axis=1).all() and (oq > 0).any(), "zero and non-zero orders in every step"
    if c.action == "direct":
        assert not oq[:, 0].any(), "env 0 orders nothing, ever"
        assert (oq[:, 1] == prm).all(), "env 1 orders max_order_quantities of everything"
        assert oq.max() == prm.max() and (oq <= prm).all()
    else:
        assert (oq > prm).any() or c.big, "no upper clamp outside direct"
    if c.big:  # the full order, and a warehouse's pending total at the limit and never past it
        per_warehouse = np.stack([s["pending_total"] for s in first]).sum(axis=3)
        assert per_warehouse.max() == sc.BIG and oq.max() == sc.BIG
    # exact ties reach np.round in every step (the target / adjustment before the integer terms)
    half = ((act[:c.T] + np.float32(1)) / np.float32(2)).astype(np.float64)
    scaled = prm * act[:c.T].astype(np.float64) if c.action == "demand_centered" else half * prm
    frac = scaled - np.floor(scaled)
    tied = frac == 0.5
    assert tied.reshape(c.T, -1).any(axis=1).all()
    if not c.big:
        x = np.floor(scaled[tied])
        assert (x % 2 == 0).any() and (x % 2 == 1).any(), "ties with even and with odd x"
    # zero denominators: some warehouse with no stock, no pending order, no home demand, no shipment
    reset_obs, _, _ = sc.emulated(name)
    assert np.isfinite(reset_obs).all() and all(np.isfinite(s["obs"]).all() for s in steps)
    assert any((s["inventory"].sum(axis=2) == 0).any() for s in first)
    assert any((s["pending_total"].sum(axis=2) == 0).any() for s in first[1:])
    lost = [s["costs"][:, 1] for s in first]
    assert max(x.max() for x in lost) > 0, "lost sales are charged"
    assert steps[c.T - 1]["truncated"] and not steps[c.T - 2]["truncated"] and not steps[c.T]["truncated"]
    if c.deviation is not None:
        em = se.StepEmulation(spec, sc.E, base_seed=sc.BASE_SEED)
        em.reset()
        lead = np.stack([em._lead_times() for _ in range(c.T)])
        exp = np.asarray(spec.expected_lead_times)
        assert (lead < exp).any() and (lead > exp).any(), "early and overdue arrivals"
        dev = np.broadcast_to(np.asarray(spec.max_deviation), (c.K,))
        assert ((exp - dev < 1) & (lead == 1)).any(), "the clip to a lead time of 1"
        # two orders of one component due in the same step: placed at t and t + 1, leads L and L - 1
        due = np.arange(c.T)[:, None, None, None] + lead
        assert ((due[:-1] == due[1:]) & (oq[:-1] > 0) & (oq[1:] > 0)).any()


# mutant -> the designed cases it must change
MUTANT_CASES = {
    "round_half_up": ("w8k5_lead3_direct", "w8k5_lead3_demand_centered", "w8k5_lead3_base_stock"),
    "half_in_f64": ("w8k5_lead3_direct", "w8k5_lead3_base_stock"),
    "direct_unclamped": ("w8k5_lead3_direct",),
    "others_clamped": ("w8k5_lead3_demand_centered", "w8k5_lead3_base_stock"),
    "pending_ignored": ("w8k5_lead3_base_stock", "w8k5_lead3_base_stock_full"),
    "arrival_first": ("w4k2_lead1_base_stock",),
    "bucket_off_by_one": ("w8k5_lead3_direct", "w8k5_mixed_direct"),
    "overdue_dropped": ("w8k5_stoch_scalar_base_stock", "w17k10_stoch_list_demand_centered"),
    "eps_width": ("w4k2_lead1_forecast", "w8k5_lead3_direct"),
    "history_oldest_first": ("w4k2_lead1_history",),
    "std_ddof1": ("w4k2_lead1_history",),
    "inbound_fixed_on_zero": ("w8k5_lead3_direct",),
    "team_sum_reversed": ("w32k16_lead3_base_stock",),
    "draws_warehouse_major": ("w8k5_stoch_list_direct", "w17k10_stoch_list_demand_centered"),
}
# changes bits of the float64 team reward only, by an ulp: below REW_ATOL by construction
BELOW_THE_BAR = {"team_sum_reversed"}


def test_every_mutant_is_listed():
    assert set(MUTANT_CASES) | {"arrival_ge"} == set(se.MUTANTS)


@pytest.mark.parametrize("mutant", list(MUTANT_CASES))
def test_mutant_changes_its_designed_cases(mutant):
    for name in MUTANT_CASES[mutant]:
        plain, mut = sc.emulated(name), sc.emulated(name, mutant)
        assert changed(plain, mut), f"{mutant} must change {name}"
        bad = mismatches(name, mut, sc.oracle_episode(name))
        assert bool(bad) != (mutant in BELOW_THE_BAR), (mutant, name, bad[:3])
        seen = changed(sc.emulated(name, None, True), sc.emulated(name, mutant, True))
        fails = bool(mismatches(name, sc.emulated(name, mutant, True), sc.oracle_episode(name, True)))
        print(f"MUTANT {mutant:24s} {name:36s} designed: changes, comparison {'fails' if bad else 'passes'}"
              f" (first: {bad[0] if bad else '-'}); 30 random steps: {'changes' if seen else 'UNCHANGED'},"
              f" comparison {'fails' if fails else 'PASSES'}")


def test_arrival_on_ge_is_no_defect():
    # every queue entry is examined at every step from the one after its placing, and its arrival
    # lies at least one step after that, so the first step with timestep >= arrival is the step of
    # equality: `>=` and `==` are the same program. Kept in the table so that nobody adds it again.
    for name in ("w4k2_lead1_base_stock", "w8k5_stoch_scalar_base_stock", "w17k10_stoch_list_demand_centered"):
        assert not changed(sc.emulated(name), sc.emulated(name, "arrival_ge"))
