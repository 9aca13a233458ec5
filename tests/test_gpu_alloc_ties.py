"""GPU: every allocation kernel on costs that tie. The case table of tests/alloc_cases.py (tied,
class-tied, crossing and near-tied cost tables; split limits, starvation with each lost-sales
handler, order counts around the scan kernel's 64-order window, quantities at the 16-bit field
edge) runs through each allocator variant against the numpy restatement of the reference's
allocator (tests/alloc_emulation.py) and against the C oracle in lockstep; Poisson configs with
the tied tables cover the replenished regime. The rule pinned is the project's: lowest warehouse
index first on equal cost (SURVEY.md parity hazard 1).

Each variant runs twice: with msc_step_info, comparing the info arrays, and without, because a
requested info forces the lane kernel to one lane per env and selects the instrumented forms of
the others, so only a run without it reaches the 2- and 4-lanes-per-env merge and the plain paths.
"""
import numpy as np
import pytest

torch = pytest.importorskip("torch")

import alloc_cases as ac  # noqa: E402
import alloc_emulation as emu  # noqa: E402
from parity_util import REW_ATOL, _lockstep, _np, _set_alloc, _vec  # noqa: E402

pytestmark = pytest.mark.gpu

# the parity suite's alloc_impl_lpe set, plus scan_nofa
VARIANTS = ["lane", "lane2", "lane4", "group", "group_sorted", "group_unsorted_ea1", "scan", "scan_ea0", "scan_nofc",
            "scan_nofa"]
ALLOC = {"lane": 0, "group": 1, "scan": 2}


def _group_width(W):
    return 2 if W <= 2 else 4 if W <= 4 else 8 if W <= 8 else 16 if W <= 16 else 32


def _runs(W, K, shared_homes, lost, variant, with_info):
    """Whether the library runs `variant` as such at this shape. It compiles the lane allocator up to
    16 warehouses x 8 SKUs and the scan allocator up to 16 x 6 and runs the group kernel elsewhere
    (what the `group` variants test); it runs the lane kernel with one lane per env where warehouses
    share a home region, with cost lost sales, below 5 warehouses or when step info is asked for
    (what the `lane` variant tests)."""
    impl = variant.split("_")[0]
    if impl.startswith("lane") and not (W <= 16 and K <= 8):
        return False
    if impl == "scan" and not (W <= 16 and K <= 6):
        return False
    if impl in ("lane2", "lane4") and (with_info or shared_homes or lost == "cost" or W <= 4):
        return False
    return True


DESIGNED = [pytest.param(c.name, v, i, id=f"{c.name}-{v}-{'info' if i else 'plain'}")
            for c in ac.CASES for v in VARIANTS for i in (True, False)
            if _runs(c.W, c.K, not c.unshared, c.lost, v, i)]
POISSON = [pytest.param(t, W, v, id=f"{t}-{W}-{v}")
           for t in ("all_tied", "class_ties") for W in (4, 8, 12, 16, 24, 32) for v in VARIANTS
           if _runs(W, 3 if W <= 16 else 9, W > 16, "shipment", v, False)]


def _check_choice(env, spec, variant):
    kc = env.kernel_choice()
    impl = variant.split("_")[0]
    assert kc["alloc"] == ALLOC["lane" if impl.startswith("lane") else impl], (variant, kc)
    if impl == "group":
        assert kc["group_width"] == _group_width(spec.W), kc
        assert kc["alloc_sort"] == (0 if "unsorted" in variant else 1), kc  # (sorted: the default for traces)


@pytest.mark.parametrize("name,variant,with_info", DESIGNED)
def test_designed_case(monkeypatch, name, variant, with_info):
    spec, inv0, epi = ac.reference_episode(name)
    assert (len(set(spec.home_regions.tolist())) == spec.W) == ac.CASE_BY_NAME[name].unshared
    _set_alloc(monkeypatch, variant)
    orc_epi = ac.oracle_episode(name)
    env = _vec(spec, ac.E, base_seed=ac.BASE_SEED)
    _check_choice(env, spec, variant)
    np.testing.assert_array_equal(_np(env.reset()), orc_epi["reset_obs"])
    np.testing.assert_array_equal(env.read_state()["inventory"], inv0)
    act = -torch.ones((ac.E, spec.W, spec.K), dtype=torch.float32, device="cuda")
    for t, ref in enumerate(orc_epi["steps"]):
        msg = f"{name} {variant} t={t}"
        info = env.alloc_info() if with_info else None
        obs, _, tr, fo = env.step(act, want_f64=True, info=info)
        trn = _np(tr).astype(bool)
        np.testing.assert_array_equal(trn, ref["tr"], err_msg=msg)
        np.testing.assert_array_equal(_np(obs), ref["obs"], err_msg=f"{msg} obs")
        if trn.any():
            np.testing.assert_array_equal(_np(fo)[trn], ref["fo"][trn], err_msg=f"{msg} final obs")
        np.testing.assert_allclose(_np(env.rewards_f64), ref["rew"], rtol=0, atol=REW_ATOL, err_msg=msg)
        inv = env.read_state()["inventory"]
        np.testing.assert_array_equal(inv, ref["inventory"], err_msg=f"{msg} inventory")
        want = epi[t] if t < len(epi) else None  # the emulation covers the first episode
        if want is not None and not trn.any():
            np.testing.assert_array_equal(inv, want["inventory"], err_msg=f"{msg} inventory (emulation)")
        if with_info:
            h = {k: _np(v) for k, v in info.items()}
            for k, v in ref["info"].items():
                if k == "lost_sales":
                    np.testing.assert_allclose(h[k], v, rtol=1e-9, atol=1e-9, err_msg=f"{msg} {k}")
                elif k == "costs":
                    np.testing.assert_allclose(h[k], v, rtol=1e-9, atol=1e-7, err_msg=f"{msg} {k}")
                else:
                    np.testing.assert_array_equal(h[k], v, err_msg=f"{msg} {k}")
            if want is not None:
                for k in emu.INT_KEYS + ("inventory_before", "n_orders"):
                    np.testing.assert_array_equal(h[k], want[k], err_msg=f"{msg} {k} (emulation)")
                np.testing.assert_allclose(h["lost_sales"], want["lost_sales"], rtol=1e-9, atol=1e-9, err_msg=msg)
                np.testing.assert_allclose(h["costs"], want["costs"], rtol=1e-9, atol=1e-7, err_msg=msg)
    env.check()
    env.close()


@pytest.mark.parametrize("table,W,variant", POISSON)
def test_poisson_tied_tables_vs_oracle(monkeypatch, table, W, variant):
    # random actions, 192 envs, 30 steps across the boundary of 20-step episodes
    spec = ac.poisson_spec(table, W)
    assert (spec.K, len(set(spec.home_regions.tolist())) < W) == (3 if W <= 16 else 9, W > 16)
    _set_alloc(monkeypatch, variant)
    env, _ = _lockstep(spec, 192, 30, seed=W, check_every=3)
    kc = env.kernel_choice()
    assert kc["alloc"] == ALLOC["lane" if variant.startswith("lane") else variant.split("_")[0]], (variant, kc)
    if variant.startswith("group"):
        assert kc["group_width"] == _group_width(W), kc
    env.close()
