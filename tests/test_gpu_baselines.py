"""The baseline policies' action kernel (csrc/policy.hip, msc_policy_act) and the rollouts built on it
(marlsc/baselines.py), on the GPU, against the C oracle env driven by the numpy restatement in
tests/baselines_emulation.py.

Lockstep runs: the GPU env + msc_policy_act and the oracle env + the restatement step side by side;
at every step the f32 actions must be bit-equal, inventory / timestep / truncation flags equal, and
rewards within 1e-9 (the bound the parity tests use for cost terms). Shapes are the smallest that
still reach each hazard: a tail block (E not a multiple of 64), in-step auto-resets (the adaptive
window clears, the output is -1 at timestep 0), stochastic lead times (arrived ring slots must not
count as pending), more components than one LDS stage chunk holds, per-env candidates, windows
longer than the episode.
"""
import os
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest
import yaml

import baselines_emulation as emu
import oracle as orc
from marlsc import baselines as bl
from marlsc import make_synthetic_env_config
from marlsc.spec import EnvSpec
from marlsc.synthetic import FEATURE_CONFIG_YAML

pytestmark = pytest.mark.gpu
REPO = Path(__file__).resolve().parent.parent


def _cfg(W, R, K, T, maxq, *, stochastic=False, lead=None):
    cfg = make_synthetic_env_config(W, R, K, episode_length=T, features=emu.emu_features(FEATURE_CONFIG_YAML))
    cfg["action_space"] = {"type": "direct", "params": {"max_order_quantities": list(maxq)}}
    cfg["initial_inventory"] = {"type": "uniform", "params": {"min": 0, "max": 40}}
    elt = lead if lead is not None else [[1 + (w + k) % 4 for k in range(K)] for w in range(W)]
    if stochastic:
        cfg["components"]["lead_time_sampler"] = {"type": "stochastic", "params": {
            "expected_lead_times": elt, "deviation": {"type": "uniform", "max_deviation": 2}}}
    else:
        cfg["components"]["lead_time_sampler"]["params"]["expected_lead_times"] = elt
    return cfg


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _lockstep(cfg, E, n_steps, make_policy, make_emu, base_seed=77):
    """Step the GPU env under make_policy(env) and the oracle under make_emu(spec) side by side."""
    from marlsc.vec_env import VecInventoryEnv
    spec = EnvSpec.from_config(cfg, {"obs_normalization": "off"})
    gpu = VecInventoryEnv(None, E, spec=spec, device=0, base_seed=base_seed)
    ref = orc.OracleEnv(spec, E, base_seed=base_seed)
    pol = None
    seen = {"resets": 0, "lo": 0, "mid": 0}  # auto-resets; actions at -1; actions strictly inside (-1, 1)
    try:
        gpu.reset()
        obs = ref.reset()
        pol, em = make_policy(gpu), make_emu(spec)
        for s in range(n_steps):
            t = s % spec.episode_length
            a_g = pol.act(gpu)
            a_r = em.act(t, *emu.split_obs(spec, obs))
            ag = a_g.cpu().numpy()
            assert ag.shape == a_r.shape == (E, spec.W, spec.K)
            bad = np.argwhere(_bits(ag) != _bits(a_r))
            assert bad.size == 0, f"step {s}: {len(bad)} actions differ, first at {bad[0]}: {ag[tuple(bad[0])]!r} vs {a_r[tuple(bad[0])]!r}"
            seen["lo"] += int((ag == -1.0).sum())
            seen["mid"] += int(((ag > -1.0) & (ag < 1.0)).sum())
            _, _, tg, _ = gpu.step(a_g, want_f64=True)
            obs, rr, tr, _ = ref.step(a_r)
            assert np.allclose(gpu.rewards_f64.cpu().numpy(), rr, atol=1e-9, rtol=0), f"rewards, step {s}"
            assert np.array_equal(tg.cpu().numpy().astype(bool), tr), f"truncation, step {s}"
            seen["resets"] += int(tr.all())
            sg, sr = gpu.read_state(), ref.read_state()
            assert np.array_equal(sg["inventory"], sr["inventory"]), f"inventory, step {s}"
            assert np.array_equal(sg["timestep"], sr["timestep"]), f"timestep, step {s}"
        gpu.check()
    finally:
        if pol is not None:
            pol.close()
        gpu.close()
    return seen


def _levels(cfg, z):
    return bl.newsvendor_levels(cfg, z)


# ---- cases 1-3: both rules on the tail / ring_l / wide shapes ----------------------------------
SHAPES = {
    "w2k2_tail_resets": dict(cfg=lambda: _cfg(2, 4, 2, 6, [30, 45]), E=67, steps=14),
    "w8k5_stochastic": dict(cfg=lambda: _cfg(8, 64, 5, 8, [30, 45, 7, 25, 60], stochastic=True), E=130, steps=10),
    "w17k9_wide": dict(cfg=lambda: _cfg(17, 17, 9, 5, [30, 45, 7, 25, 60, 11, 90, 33, 19]), E=65, steps=7),
}


@pytest.mark.parametrize("shape", list(SHAPES))
def test_base_stock_lockstep(shape):
    sh = SHAPES[shape]
    cfg = sh["cfg"]()
    S = _levels(cfg, 1.25) + 0.3  # fractional levels
    seen = _lockstep(cfg, sh["E"], sh["steps"], lambda env: bl.BaseStockPolicy(env, S),
                     lambda spec: emu.BaseStockEmulation(spec, S, np.zeros(sh["E"], np.int64)))
    assert seen["resets"] >= 1 and seen["mid"] > 0


@pytest.mark.parametrize("shape", list(SHAPES))
def test_adaptive_lockstep(shape):
    sh = SHAPES[shape]
    cfg = sh["cfg"]()
    seen = _lockstep(cfg, sh["E"], sh["steps"], lambda env: bl.AdaptiveBaseStockPolicy(env, 1.5, 3),
                     lambda spec: emu.AdaptiveEmulation(spec, [1.5], [3], np.zeros(sh["E"], np.int64)))
    assert seen["resets"] >= 1 and seen["mid"] > 0
    # timestep 0 of the first episode and of each one an auto-reset started: every action is -1
    assert seen["lo"] >= (1 + seen["resets"]) * sh["E"] * cfg["n_warehouses"] * cfg["n_skus"]


# ---- case 4: candidate table -------------------------------------------------------------------
def test_base_stock_candidate_table():
    E = 67
    cfg = _cfg(2, 4, 3, 6, [7, 30, 45])
    S = np.stack([np.zeros((2, 3)), np.full((2, 3), 1e6), _levels(cfg, 0.0), _levels(cfg, 2.0) + 0.37,
                  np.array([[12.3, 3.0, 41.9], [6.5, 29.99, 17.25]])])
    cand = np.arange(E) % 5

    class Spy(emu.BaseStockEmulation):
        def act(self, t, inv, pend, dem):
            a = super().act(t, inv, pend, dem)
            assert np.all(a[cand == 0] == -1.0) and np.all(a[cand == 1] == 1.0)  # levels 0 and 1e6
            return a
    seen = _lockstep(cfg, E, 8, lambda env: bl.BaseStockPolicy(env, S, cand), lambda spec: Spy(spec, S, cand))
    assert seen["mid"] > 0 and seen["resets"] == 1


def test_set_tables_replaces_levels_and_candidates():
    import torch
    from marlsc.vec_env import VecInventoryEnv
    E = 67
    cfg = _cfg(2, 4, 3, 6, [7, 30, 45])
    spec = EnvSpec.from_config(cfg, {"obs_normalization": "off"})
    env = VecInventoryEnv(None, E, spec=spec, device=0, base_seed=5)
    ref = orc.OracleEnv(spec, E, base_seed=5)
    env.reset()
    obs = ref.reset()
    S0 = np.stack([np.zeros((2, 3)), np.full((2, 3), 1e6)])
    pol = bl.BaseStockPolicy(env, S0, np.arange(E) % 2)
    try:
        a = pol.act(env).cpu().numpy()
        assert np.all(a[0::2] == -1.0) and np.all(a[1::2] == 1.0)
        S1 = np.stack([_levels(cfg, 1.0) + 0.21, np.zeros((2, 3))])
        cand = (np.arange(E) % 3 == 0).astype(np.int32)
        pol.set_levels(S1, cand)
        want = emu.BaseStockEmulation(spec, S1, cand).act(0, *emu.split_obs(spec, obs))
        assert np.array_equal(_bits(pol.act(env).cpu().numpy()), _bits(want))
        with pytest.raises(RuntimeError, match="outside"):
            pol.set_levels(S1, np.full(E, 2, np.int32))
        with pytest.raises(ValueError):
            pol.set_levels(S1[:1], np.zeros(E, np.int32))
        torch.cuda.synchronize()
    finally:
        pol.close()
        env.close()


# ---- case 5: adaptive, per-candidate (z, H), windows longer than the episode --------------------
def test_adaptive_candidates_window_longer_than_episode():
    E = 67
    cfg = _cfg(2, 4, 2, 12, [30, 45])
    z, H = np.array([0.0, 1.5, 0.25, 3.0]), np.array([1, 2, 5, 100])
    cand = np.arange(E) % 4
    seen = _lockstep(cfg, E, 26, lambda env: bl.AdaptiveBaseStockPolicy(env, z, H, cand, h_max=100),
                     lambda spec: emu.AdaptiveEmulation(spec, z, H, cand))
    assert seen["resets"] == 2 and seen["mid"] > 0


# ---- case 6: random ----------------------------------------------------------------------------
def test_random_policy_matches_numpy_stream():
    E, T = 3, 6
    cfg = _cfg(2, 4, 2, T, [30, 45])
    seen = _lockstep(cfg, E, 2 * T, lambda env: bl.RandomPolicy(env, seed=100),
                     lambda spec: emu.RandomEmulation(spec, 100, E, 2 * T))
    assert seen["resets"] == 2 and seen["mid"] >= E * 2 * T * 4 - 1


def test_random_policy_wide_shape_chunks():
    E, T = 65, 3
    cfg = _cfg(17, 17, 9, T, [30, 45, 7, 25, 60, 11, 90, 33, 19])
    _lockstep(cfg, E, 2, lambda env: bl.RandomPolicy(env, seed=7), lambda spec: emu.RandomEmulation(spec, 7, E, 2))


# ---- rollouts ----------------------------------------------------------------------------------
def test_sweep_independence():
    cfg = _cfg(2, 4, 2, 6, [30, 45])
    zs = [0.0, 0.5, 1.0, 2.5]
    S = np.stack([_levels(cfg, z) for z in zs])
    means, best, per = bl.validation_sweep(cfg, 4242, 3, 4, lambda env, c: bl.BaseStockPolicy(env, S, c),
                                           return_episodes=True)
    assert per.shape == (4, 3) and per.dtype == np.float64
    for c in range(4):
        m1, b1, p1 = bl.validation_sweep(cfg, 4242, 3, 1, lambda env, cd, c=c: bl.BaseStockPolicy(env, S[c], cd),
                                         return_episodes=True)
        assert np.array_equal(p1[0], per[c]), c
        assert m1[0] == means[c] and b1 == 0
    assert best == bl.first_strict_argmax(means) and np.all(per < 0) and len(set(means)) > 1
    za, Ha = np.array([0.5, 2.0]), np.array([2, 4])
    _, _, pa = bl.validation_sweep(cfg, 4242, 3, 2, lambda env, c: bl.AdaptiveBaseStockPolicy(env, za, Ha, c),
                                   return_episodes=True)
    for c in range(2):
        _, _, p1 = bl.validation_sweep(cfg, 4242, 3, 1,
                                       lambda env, cd, c=c: bl.AdaptiveBaseStockPolicy(env, za[c], Ha[c], cd),
                                       return_episodes=True)
        assert np.array_equal(p1[0], pa[c]), c


@pytest.mark.parametrize("kind", ["base_stock", "adaptive"])
def test_episode_accounting_vs_oracle(kind):
    n, root = 3, 123
    cfg = _cfg(3, 5, 2, 8, [30, 45])
    S = _levels(cfg, 1.0) + 0.4
    if kind == "base_stock":
        factory = lambda env: bl.BaseStockPolicy(env, S)  # noqa: E731
        make_emu = lambda spec: emu.BaseStockEmulation(spec, S, [0])  # noqa: E731
    else:
        factory = lambda env: bl.AdaptiveBaseStockPolicy(env, 1.0, 4)  # noqa: E731
        make_emu = lambda spec: emu.AdaptiveEmulation(spec, [1.0], [4], [0])  # noqa: E731
    res = bl.rollout_episodes(cfg, factory, root, n, return_episodes=True)
    spec = EnvSpec.from_config(cfg, {"data_mode": "val", "num_eval_episodes": n})
    ref = orc.OracleEnv(spec, 1, env_seeds=[root])
    rets, costs = emu.oracle_episode_totals(ref, spec, make_emu(spec), n)
    print("returns", res["episode_returns"], rets, "costs", res["episode_costs"], costs)
    assert np.all(rets < 0) and np.all(costs.sum(axis=1) > 0)
    assert np.allclose(res["episode_returns"], rets, rtol=1e-10, atol=0)
    assert np.allclose(res["episode_costs"], costs, rtol=1e-10, atol=0)
    want = bl.aggregate_results(rets, costs)
    assert res["num_episodes"] == n
    for k in ("episode_return_mean", "episode_return_std", "episode_return_min", "episode_return_max"):
        assert res[k] == pytest.approx(want[k], rel=1e-10)
    for k, v in want["cost_components"].items():
        assert res["cost_components"][k] == pytest.approx(v, rel=1e-9), k


def test_calibrate_demand_is_the_home_demand_mean():
    cfg = _cfg(2, 4, 2, 6, [30, 45])
    got = bl.calibrate_demand(cfg, 99, 3)
    spec = EnvSpec.from_config(cfg, {"data_mode": "train"})
    ref = orc.OracleEnv(spec, 1, env_seeds=[99])  # its episodes 0..2, one after another
    ref.reset()
    info = ref.alloc_info()
    tot = np.zeros((2, 2))
    for _ in range(3 * 6):
        ref.step(np.full((1, 2, 2), -1.0, np.float32), info=info)
        tot += info["demand_per_region"][0][spec.home_regions]
    assert tot.sum() > 0 and np.allclose(got, tot / 18.0, rtol=1e-12, atol=0)


# ---- error paths -------------------------------------------------------------------------------
def test_error_paths_return_a_code_and_message():
    from marlsc import abi
    from marlsc.vec_env import VecInventoryEnv
    E = 5
    nd = make_synthetic_env_config(2, 4, 2, episode_length=6)  # demand_centered
    env = VecInventoryEnv(None, E, spec=EnvSpec.from_config(nd, {}), device=0, base_seed=1)
    try:
        with pytest.raises(RuntimeError, match="direct"):
            bl.BaseStockPolicy(env, np.ones((2, 2)))
        with pytest.raises(RuntimeError, match="direct"):
            bl.AdaptiveBaseStockPolicy(env, 1.0, 5)
    finally:
        env.close()
    env = VecInventoryEnv(None, E, spec=EnvSpec.from_config(_cfg(2, 4, 2, 6, [30, 45]), {}), device=0, base_seed=1)
    try:
        with pytest.raises(RuntimeError, match=r"H\[0\] = 0"):
            bl.AdaptiveBaseStockPolicy(env, 1.0, 0)
        with pytest.raises(RuntimeError, match="exceeds h_max"):
            bl.AdaptiveBaseStockPolicy(env, [1.0, 2.0], [3, 9], np.zeros(E, np.int32), h_max=8)
        with pytest.raises(RuntimeError, match=r"candidate index 2 of env 3"):
            bl.BaseStockPolicy(env, np.ones((2, 2, 2)), np.array([0, 1, 0, 2, 1]))
        with pytest.raises(RuntimeError, match="candidate index -1"):
            bl.BaseStockPolicy(env, np.ones((2, 2, 2)), np.array([0, 1, 0, -1, 1]))
        # the C entry points themselves: a negative code, a message, no handle
        import ctypes as C
        h = C.c_void_p()
        H0 = np.zeros(1, np.int32)
        z0 = np.ones(1, np.float64)
        rc = abi.lib().msc_policy_create(env._h, abi.POLICY_ADAPTIVE, 1, 0, None, z0.ctypes.data_as(C.c_void_p),
                                         H0.ctypes.data_as(C.c_void_p), None, None, C.byref(h))
        assert rc < 0 and not h.value and b"must be >= 1" in abi.lib().msc_last_error()
        assert abi.lib().msc_policy_act(None, env._h, None, None) < 0
    finally:
        env.close()


# ---- command line ------------------------------------------------------------------------------
def test_entry_point_bs_newsvendor(tmp_path):
    with open(REPO / "config_files/environments/env_c1_2wh4r2sku.yaml") as fh:
        doc = yaml.safe_load(fh)
    # the C1 shape; the baselines need the `direct` action space
    doc["environment"]["action_space"] = {"type": "direct", "params": {"max_order_quantities": [40, 40]}}
    cfg_path = tmp_path / "env_c1_direct.yaml"
    cfg_path.write_text(yaml.safe_dump(doc))
    env = dict(os.environ)
    env["PATH"] = str(Path(sys.executable).parent) + os.pathsep + env.get("PATH", "")  # `python` = this interpreter
    p = subprocess.run([str(REPO / "scripts/run_baselines.sh"), "--mode", "single", "--baseline", "bs_newsvendor",
                        "--root-seed", "100", "--eval-episodes", "4", "--env-config", str(cfg_path),
                        "--storage-dir", str(tmp_path / "runs"), "--experiment-name", "t"],
                       capture_output=True, text=True, env=env, timeout=300)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-2000:]
    f = tmp_path / "runs/t/seed_evaluation/BSNewsvendor_Seed100/eval_results_best.yaml"
    res = yaml.safe_load(f.read_text())
    assert res["selected_hparams"]["best_z"] in bl.DEFAULT_Z_VALUES
    assert np.isfinite(res["episode_return_mean"]) and res["episode_return_mean"] < 0
    assert res["num_episodes"] == 4 and res["root_seed"] == 100 and res["eval_seed"] == 123
    assert res["display_name"] == "BSNewsvendor" and res["baseline"] == "bs_newsvendor"
    v = res["validation"]
    assert v["validation_seed"] == bl.baseline_train_seeds("bs_newsvendor", 100)[0]
    assert len(v["validation_rewards"]) == 25 and v["best_idx"] == bl.first_strict_argmax(v["validation_rewards"])
    assert set(res["cost_components"]) == {"holding_mean", "penalty_mean", "outbound_mean", "inbound_mean",
                                           "total_cost_mean", "total_cost_std"}


# ---- bs_optimized ------------------------------------------------------------------------------
def test_bs_optimized_search_is_elitist_and_deterministic():
    cfg = _cfg(2, 4, 2, 6, [30, 45])
    kw = dict(n_generations=2, population=16, n_obj_episodes=3, upper_bound=60.0, z_values=[0.0, 1.0, 2.0, 4.0])
    S1, hist1, start1 = bl.optimize_levels(cfg, 31, **kw)
    S2, hist2, start2 = bl.optimize_levels(cfg, 31, **kw)
    assert np.array_equal(S1, S2) and hist1 == hist2 and start1 == start2
    assert S1.shape == (2, 2) and np.all(S1 >= 0.0) and np.all(S1 <= 60.0)
    nv = np.clip(np.stack([_levels(cfg, z) for z in kw["z_values"]]), 0.0, 60.0)
    obj_nv = bl.evaluate_levels(cfg, nv, 31, 3)
    obj = bl.evaluate_levels(cfg, S1[None], 31, 3)[0]
    assert start1 == obj_nv.max() and len(hist1) == 2 and hist1[0] <= hist1[1]
    assert obj == hist1[-1] and obj >= obj_nv.max()
