"""GPU: order placement, arrivals and observations on designed actions. Every case of
tests/step_cases.py runs through every form of phases A and C that the library runs at its shape:
the allocator variants (lane, group, scan and the two without their fused phases), crossed where
the step_a / step_c kernels run with the pending ring in registers or not, the observation stage
off / whole / in 2 / in W phases and step_c's two register forms; where phase C is fused only the
ring form of step_a is left to cross. Each combination runs with msc_step_info (the instrumented
instantiations) and without, against the numpy restatement of the reference
(tests/step_emulation.py) and the C oracle in lockstep, at the bars of
tests/test_step_cases_host.py, and asserts through kernel_choice() and the plan query that the
intended form ran.

Poisson demand, the only way into the scan allocator's fused phase A, takes phase B's record from
the msc_step_info arrays of a twin handle on the same seeds.
"""
import numpy as np
import pytest

torch = pytest.importorskip("torch")

import oracle as orc  # noqa: E402
import step_cases as sc  # noqa: E402
import step_emulation as se  # noqa: E402
from marlsc.vec_env import plan  # noqa: E402
from parity_util import REW_ATOL, _np, _set_alloc, _vec  # noqa: E402

pytestmark = pytest.mark.gpu

ALLOC = {"lane": 0, "group": 1, "scan": 2}


def _ring(c):
    elt = np.asarray(sc.expected_lead_times(c))
    dev = 0 if c.deviation is None else np.asarray(c.deviation)
    return int((elt + dev).max()) + 1


def _fuses_c(c, variant):
    """Whether phase C runs inside the allocator (env_plan.hpp): the scan allocator up to 8 warehouses,
    6 SKUs and 4 ring slots, the group allocator up to 8 SKUs and 4 ring slots."""
    impl, *opts = variant.split("_")
    if "nofc" in opts or impl == "lane":
        return False
    if impl == "scan":
        return c.W <= 8 and c.K <= 6 and _ring(c) <= 4
    return c.K <= 8 and _ring(c) <= 4


def _variants(c):
    """The library compiles the lane allocator up to 16 warehouses x 8 SKUs, the scan allocator up to
    16 x 6, and the group allocator everywhere; `nofc` is another form only where phase C fuses."""
    out = ["group"]
    if c.W <= 16 and c.K <= 8:
        out.append("lane")
    if c.W <= 16 and c.K <= 6:
        out.append("scan")
    return out + [v + "_nofc" for v in out if _fuses_c(c, v)]


def _stage_fits(c):
    """step_c stages a block's observations (64 envs x W x L floats) in at most 80 KB of LDS; where
    they do not fit the unstaged form runs whatever is asked (the 4 x 2 and 8 x 2 cases stage)."""
    return 64 * ((c.W * sc.make_spec(c.name).local_obs_dim) | 1) * 4 <= 80 * 1024


def _knobs(c, variant):
    """(MSC_OBS_RING_REG, MSC_OBS_STAGE, MSC_STEP_C_FORM), crossed in full where step_c runs."""
    if _fuses_c(c, variant):  # no step_c: only step_a's ring form is left
        return [(0, None, None), (1, None, None)]
    return [(r, s, f) for r in (0, 1) for s in (("0", "1", "2", "W") if _stage_fits(c) else ("0",)) for f in (4, 5)]


DESIGNED = [pytest.param(c.name, v, k, i, id=f"{c.name}-{v}-r{k[0]}s{k[1]}f{k[2]}-{'info' if i else 'plain'}")
            for c in sc.CASES for v in _variants(c) for k in _knobs(c, v) for i in (True, False)]
POISSON = [pytest.param(f"w8k5_lead3_{a}", v, id=f"{a}-{v}") for a in ("direct", "demand_centered", "base_stock")
           for v in ("lane", "group", "group_nofc", "scan", "scan_nofa", "scan_nofc")]


def _set_form(monkeypatch, c, variant, knobs):
    _set_alloc(monkeypatch, variant)
    ring_reg, stage, form = knobs
    monkeypatch.setenv("MSC_OBS_RING_REG", str(ring_reg))
    if stage is not None:
        monkeypatch.setenv("MSC_OBS_STAGE", str(c.W) if stage == "W" else stage)
        monkeypatch.setenv("MSC_STEP_C_FORM", str(form))


def _check_form(env, spec, c, variant, knobs, *, poisson=False):
    kc, pl = env.kernel_choice(), plan(spec, sc.E)
    impl, *opts = variant.split("_")
    assert kc["alloc"] == pl["alloc"] == ALLOC[impl], (variant, kc)
    assert pl["ring"] == _ring(c)
    assert kc["fuse_c"] == pl["fuse_c"] == int(_fuses_c(c, variant)), (variant, kc)
    fuse_a = impl == "scan" and _fuses_c(c, variant) and poisson and c.deviation is None and "nofa" not in opts
    assert kc["fuse_a"] == pl["fuse_a"] == int(fuse_a), (variant, kc)
    ring_reg, stage, form = knobs
    assert pl["obs_ring_reg"] == ring_reg
    if stage is not None:
        assert pl["sc_form"] == form
        assert pl["obs_stage"] == min(c.W, {"0": 0, "1": 1, "2": 2, "W": c.W}[stage])


def _compare_step(msg, env, got, info, ref, emu, worst):
    obs, tr, fo = got
    trn = _np(tr).astype(bool)
    np.testing.assert_array_equal(trn, ref["tr"], err_msg=msg)
    assert trn.all() == trn.any() == bool(emu["truncated"]), msg
    for want, who in ((ref["obs"], "oracle"), (emu["obs"], "emulation")):
        np.testing.assert_array_equal(_np(obs), want, err_msg=f"{msg} obs ({who})")
    if trn.any():
        np.testing.assert_array_equal(_np(fo), ref["fo"], err_msg=f"{msg} final obs (oracle)")
        np.testing.assert_array_equal(_np(fo), emu["final_obs"], err_msg=f"{msg} final obs (emulation)")
    rew = _np(env.rewards_f64)
    np.testing.assert_allclose(rew, ref["rew"], rtol=0, atol=REW_ATOL, err_msg=f"{msg} rewards (oracle)")
    np.testing.assert_allclose(rew, emu["rewards"], rtol=0, atol=REW_ATOL, err_msg=f"{msg} rewards (emulation)")
    inv = env.read_state()["inventory"]
    np.testing.assert_array_equal(inv, ref["inventory"], err_msg=f"{msg} inventory (oracle)")
    if not trn.any():
        np.testing.assert_array_equal(inv, emu["inventory"], err_msg=f"{msg} inventory (emulation)")
    if info is not None:
        h = {k: _np(v) for k, v in info.items()}
        for k, v in ref["info"].items():
            if k == "lost_sales":
                np.testing.assert_allclose(h[k], v, rtol=1e-9, atol=1e-9, err_msg=f"{msg} {k}")
            elif k == "costs":
                np.testing.assert_allclose(h[k], v, rtol=1e-9, atol=1e-7, err_msg=f"{msg} {k}")
            else:
                np.testing.assert_array_equal(h[k], v, err_msg=f"{msg} {k}")
        for k in ("order_quantities", "pending_total", "inventory_before"):
            np.testing.assert_array_equal(h[k], emu[k], err_msg=f"{msg} {k} (emulation)")
        worst[0] = max(worst[0], float((np.abs(h["costs"] - emu["costs"]) / (1e-7 + 1e-9 * np.abs(emu["costs"]))).max()))
        np.testing.assert_allclose(h["costs"], emu["costs"], rtol=1e-9, atol=1e-7, err_msg=f"{msg} costs (emulation)")
        return h
    return None


@pytest.mark.parametrize("name,variant,knobs,with_info", DESIGNED)
def test_designed_case(monkeypatch, name, variant, knobs, with_info):
    c, spec = sc.CASE_BY_NAME[name], sc.make_spec(name)
    _set_form(monkeypatch, c, variant, knobs)
    ref = sc.oracle_episode(name)
    reset_obs, steps, words = sc.emulated(name)
    env = _vec(spec, sc.E, base_seed=sc.BASE_SEED)
    _check_form(env, spec, c, variant, knobs)
    obs0 = _np(env.reset())
    np.testing.assert_array_equal(obs0, ref["reset_obs"])
    np.testing.assert_array_equal(obs0, reset_obs)
    worst = [0.0]
    for t, a in enumerate(sc.actions(name)):
        info = env.alloc_info() if with_info else None
        obs, _, tr, fo = env.step(torch.from_numpy(a).cuda(), want_f64=True, info=info)
        _compare_step(f"{name} {variant} {knobs} t={t}", env, (obs, tr, fo), info, ref["steps"][t], steps[t], worst)
    rng = env.read_state()["rng"]
    np.testing.assert_array_equal(rng, ref["rng"])
    np.testing.assert_array_equal(rng[:, 1, :], words, err_msg="lead-time generator against numpy's")
    env.check()
    env.close()
    if with_info:
        print(f"COSTERR {name} {variant} {worst[0]:.3e} of the bar")


@pytest.mark.parametrize("name,variant", POISSON)
def test_poisson_twin(monkeypatch, name, variant):
    # Poisson demand on the case's shape, parameters, inventories and designed actions: a twin
    # handle with msc_step_info gives phase B's record, the emulation turns it into the episode, and
    # the twin, a handle without info and the oracle are all held to it
    c = sc.CASE_BY_NAME[name]
    spec = sc.make_spec(name, "poisson", c.T)
    knobs = (1, None, None)
    _set_form(monkeypatch, c, variant, knobs)
    act = sc.actions(name)
    twin, env = _vec(spec, sc.E, base_seed=sc.BASE_SEED), _vec(spec, sc.E, base_seed=sc.BASE_SEED)
    for h in (twin, env):
        _check_form(h, spec, c, variant, knobs, poisson=True)
    orac = orc.OracleEnv(spec, sc.E, base_seed=sc.BASE_SEED)
    ref = {"reset_obs": orac.reset().copy(), "steps": []}
    got = {"reset": _np(twin.reset()).copy(), "steps": [], "infos": []}
    for a in act:
        info = twin.alloc_info()
        obs, _, tr, fo = twin.step(torch.from_numpy(a).cuda(), want_f64=True, info=info)
        got["steps"].append((_np(obs).copy(), _np(tr).copy(), _np(fo).copy(), _np(twin.rewards_f64).copy(),
                             twin.read_state()["inventory"].copy()))
        got["infos"].append({k: _np(v).copy() for k, v in info.items()})
        oi = orac.alloc_info()
        o, r, trr, f = orac.step(a, info=oi, final_obs=True, n_threads=4)
        ref["steps"].append({"obs": o, "rew": r, "tr": trr, "fo": f, "info": oi,
                             "inventory": orac.read_state()["inventory"].copy()})
    reset_obs, steps, em = se.run(spec, sc.E, act, sc.info_provider(got["infos"]), base_seed=sc.BASE_SEED)
    np.testing.assert_array_equal(got["reset"], reset_obs)
    np.testing.assert_array_equal(got["reset"], ref["reset_obs"])
    np.testing.assert_array_equal(_np(env.reset()), reset_obs)
    for t, a in enumerate(act):
        msg = f"{name} poisson {variant} t={t}"
        emu, q = steps[t], ref["steps"][t]
        tobs, ttr, tfo, trew, tinv = got["steps"][t]
        obs, _, tr, fo = env.step(torch.from_numpy(a).cuda(), want_f64=True)
        _compare_step(msg, env, (obs, tr, fo), None, q, emu, [0.0])
        np.testing.assert_array_equal(tobs, emu["obs"], err_msg=f"{msg} twin obs")
        np.testing.assert_array_equal(ttr.astype(bool), q["tr"], err_msg=msg)
        if emu["truncated"]:
            np.testing.assert_array_equal(tfo, emu["final_obs"], err_msg=f"{msg} twin final obs")
        else:
            np.testing.assert_array_equal(tinv, emu["inventory"], err_msg=f"{msg} twin inventory")
        np.testing.assert_allclose(trew, emu["rewards"], rtol=0, atol=REW_ATOL, err_msg=f"{msg} twin rewards")
        h = got["infos"][t]
        for k in ("order_quantities", "pending_total", "inventory_before"):
            np.testing.assert_array_equal(h[k], emu[k], err_msg=f"{msg} twin {k}")
            np.testing.assert_array_equal(h[k], q["info"][k], err_msg=f"{msg} twin {k} (oracle)")
        np.testing.assert_allclose(h["costs"], emu["costs"], rtol=1e-9, atol=1e-7, err_msg=f"{msg} twin costs")
        np.testing.assert_allclose(h["costs"], q["info"]["costs"], rtol=1e-9, atol=1e-7, err_msg=f"{msg} twin costs (oracle)")
    for h in (twin, env):
        np.testing.assert_array_equal(h.read_state()["rng"], orac.read_state()["rng"])
        h.check()
        h.close()
