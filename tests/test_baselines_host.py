"""Host-side checks of marlsc.baselines (no GPU): parameter helpers, seed derivation, the sweep's tie
rule, the command line's mode / flag rules, the result dict, skip-if-done, and the numpy restatement
the GPU tests compare the kernel against (tests/baselines_emulation.py)."""
import numpy as np
import pytest
import yaml
from numpy.random import SeedSequence

import baselines_emulation as emu
from marlsc import baselines as bl
from marlsc import make_synthetic_env_config


def _cfg_2x2():
    cfg = make_synthetic_env_config(2, 3, 2, episode_length=6)
    cfg["action_space"] = {"type": "direct", "params": {"max_order_quantities": [7, 30]}}
    # regions 0 and 2 are nobody's home; both warehouses share region 1
    cfg["cost_structure"]["distances"] = [[5.0, 1.0, 9.0], [4.0, 2.0, 3.0]]
    cfg["components"]["demand_sampler"]["params"] = {
        "lambda_orders": [9.0, 2.0, 7.0], "probability_skus": [0.9, 0.5, 0.1],
        "lambda_quantity": [[1.0, 1.0], [4.0, 9.0], [2.0, 2.0]]}
    cfg["components"]["lead_time_sampler"]["params"]["expected_lead_times"] = [[1, 4], [9, 2]]
    return cfg


def test_newsvendor_levels_hand_computed():
    cfg = _cfg_2x2()
    # home region 1 for both: D = 2 * 0.5 * {4, 9} = {4, 9}
    assert np.array_equal(bl.newsvendor_levels(cfg, 0.0), [[4.0, 36.0], [36.0, 18.0]])
    # z = 1.5: L D + 1.5 sqrt(L D) with L D = {4, 36; 36, 18}
    want = [[4 + 1.5 * 2, 36 + 1.5 * 6], [36 + 1.5 * 6, 18 + 1.5 * np.sqrt(18.0)]]
    assert np.array_equal(bl.newsvendor_levels(cfg, 1.5), want)


def test_newsvendor_levels_rejects_empirical_sampler():
    cfg = _cfg_2x2()
    cfg["components"]["demand_sampler"] = {"type": "empirical", "params": {}}
    with pytest.raises(ValueError, match="poisson"):
        bl.newsvendor_levels(cfg, 1.0)


def test_non_direct_action_space_is_refused(tmp_path):
    cfg = make_synthetic_env_config(2, 3, 2)  # demand_centered
    with pytest.raises(ValueError, match="direct"):
        bl.run_single_baseline_seed_eval("bs_newsvendor", cfg, 100, 123, 2, tmp_path)  # before any env is built
    assert not (tmp_path / "eval_results_best.yaml").exists()


@pytest.mark.parametrize("baseline,n", [("random", 0), ("constant", 2), ("bs_newsvendor", 1), ("bs_adaptive", 1),
                                        ("bs_optimized", 1)])
def test_train_seed_derivation(baseline, n):
    root = 300
    # SeedManager: the experiment registry's children of SeedSequence(root); "train" is the fourth
    train = SeedSequence(root).spawn(6)[3]
    want = [int(c.generate_state(1, dtype=np.uint32)[0]) for c in train.spawn(n)]
    assert bl.baseline_train_seeds(baseline, root) == want
    assert len(set(want)) == n


def test_first_strict_argmax_tie_rule():
    assert bl.first_strict_argmax([-3.0, -1.0, -1.0, -2.0]) == 1   # the later equal value does not win
    assert bl.first_strict_argmax([-1.0, -1.0]) == 0
    assert bl.first_strict_argmax([-5.0, -4.0, -3.0]) == 2
    assert bl.first_strict_argmax([float("-inf")]) == 0


def test_default_grids():
    assert bl.DEFAULT_ALPHA_VALUES[0] == 0.05 and bl.DEFAULT_ALPHA_VALUES[-1] == 2.0 and len(bl.DEFAULT_ALPHA_VALUES) == 40
    assert bl.DEFAULT_Z_VALUES[0] == 0.0 and bl.DEFAULT_Z_VALUES[-1] == 6.0 and len(bl.DEFAULT_Z_VALUES) == 25
    assert bl.DEFAULT_H_VALUES == [5, 10, 20, 30, 40, 50, 100]


def test_cli_mode_and_flag_rules(capsys):
    base = ["--env-config", "x.yaml"]
    a = bl.parse_args(base + ["--mode", "single", "--baseline", "random", "--root-seed", "100"])
    assert (a.mode, a.baseline, a.root_seed, a.eval_seed, a.eval_episodes) == ("single", "random", 100, 123, 100)
    a = bl.parse_args(base + ["--baselines", "random", "constant", "--n-seeds", "3"])
    assert (a.mode, a.baselines, a.n_seeds) == ("all-seeds", ["random", "constant"], 3)
    for bad in (["--mode", "single", "--baseline", "random"],                       # no root seed
                ["--mode", "single", "--root-seed", "100"],                         # no baseline
                ["--mode", "single", "--baseline", "random", "--root-seed", "1", "--baselines", "random"],
                ["--mode", "all-seeds", "--baseline", "random"],
                ["--mode", "all-seeds", "--root-seed", "100"],
                ["--mode", "single", "--baseline", "bs_independent", "--root-seed", "1"]):
        with pytest.raises(SystemExit):
            bl.parse_args(base + bad)
    with pytest.raises(SystemExit):
        bl.parse_args(["--mode", "all-seeds"])  # --env-config is required
    capsys.readouterr()


def test_result_dict_keys_and_ddof():
    r = np.array([-10.0, -14.0, -12.0])
    c = np.array([[1.0, 2.0, 3.0, 4.0], [2.0, 2.0, 2.0, 2.0], [0.0, 1.0, 5.0, 6.0]])
    d = bl.aggregate_results(r, c)
    assert list(d) == ["episode_return_mean", "episode_return_std", "episode_return_min", "episode_return_max",
                       "num_episodes", "cost_components"]
    assert list(d["cost_components"]) == ["holding_mean", "penalty_mean", "outbound_mean", "inbound_mean",
                                          "total_cost_mean", "total_cost_std"]
    assert d["episode_return_mean"] == -12.0 and d["episode_return_std"] == 2.0  # ddof = 1
    assert (d["episode_return_min"], d["episode_return_max"], d["num_episodes"]) == (-14.0, -10.0, 3)
    assert d["cost_components"]["total_cost_mean"] == 10.0
    assert d["cost_components"]["total_cost_std"] == np.std([10.0, 8.0, 12.0], ddof=1)
    one = bl.aggregate_results(r[:1], c[:1])
    assert one["episode_return_std"] == 0.0 and one["cost_components"]["total_cost_std"] == 0.0


def test_skip_if_done(tmp_path, capsys):
    f = tmp_path / "eval_results_best.yaml"
    assert bl.existing_result(f) is None
    f.write_text(yaml.safe_dump({"episode_return_mean": None}))
    assert bl.existing_result(f) is None
    f.write_text(yaml.safe_dump({"episode_return_mean": "nan?"}))
    assert bl.existing_result(f) is None
    f.write_text("{ not yaml")
    assert bl.existing_result(f) is None
    f.write_text(yaml.safe_dump({"episode_return_mean": -12.5, "baseline": "random"}))
    assert bl.existing_result(f)["episode_return_mean"] == -12.5
    # a finished pair returns the stored dict without building an env (the config is not even direct)
    cfg = make_synthetic_env_config(2, 3, 2)
    got = bl.run_single_baseline_seed_eval("random", cfg, 100, 123, 4, tmp_path)
    assert got == {"episode_return_mean": -12.5, "baseline": "random"}
    assert "[SKIP]" in capsys.readouterr().out


def test_constant_actions():
    a = bl.constant_actions(np.array([[0.0, 45.0], [3.0, -2.0]]), np.array([7.0, 30.0]))
    assert a.dtype == np.float32
    want = np.array([[-1.0, 1.0], [np.float32(2.0 * 3.0 / 7.0 - 1.0), -1.0]], np.float32)
    assert np.array_equal(a, want)


def test_emulation_window_stats_against_literal_loop():
    rng = np.random.default_rng(5)
    for n in (1, 2, 3, 7, 8, 9, 16, 33, 100):
        window = [rng.integers(0, 60, size=(2, 3)).astype(np.float32) for _ in range(n)]
        m, v = emu.window_stats(window)
        ml, vl = emu.window_stats_loop(window)
        assert m.dtype == np.float32 and v.dtype == np.float32
        assert np.array_equal(m.view(np.uint32), ml.view(np.uint32)), n
        assert np.array_equal(v.view(np.uint32), vl.view(np.uint32)), n
    one = [np.array([[3.0, 0.0]], np.float32)]
    m, v = emu.window_stats(one)
    assert np.array_equal(m, one[0]) and np.array_equal(v, m)  # n == 1: the variance is the mean


def test_emulation_adaptive_rule_tiny_window():
    from marlsc.spec import EnvSpec
    cfg = _cfg_2x2()
    spec = EnvSpec.from_config(cfg, {})
    pol = emu.AdaptiveEmulation(spec, [2.0], [2], [0])
    inv, pend = np.array([[[1.0, 2.0], [0.0, 3.0]]]), np.array([[[0.0, 1.0], [2.0, 0.0]]])
    d = [np.array([[[4.0, 9.0], [1.0, 0.0]]], np.float32), np.array([[[2.0, 5.0], [3.0, 0.0]]], np.float32),
         np.array([[[8.0, 1.0], [5.0, 2.0]]], np.float32)]
    assert np.array_equal(pol.act(0, inv, pend, d[0]), np.full((1, 2, 2), -1.0, np.float32))
    lead, maxq = np.array([[1.0, 4.0], [9.0, 2.0]]), np.array([7.0, 30.0])

    def want(mean, var):
        S = lead * mean + 2.0 * np.sqrt(lead * var)
        return (2.0 * np.clip(S - inv[0] - pend[0], 0.0, maxq) / maxq - 1.0).astype(np.float32)
    assert np.array_equal(pol.act(1, inv, pend, d[0])[0], want(d[0][0], d[0][0]))          # n = 1
    m = (d[0][0] + d[1][0]) / np.float32(2)
    v = ((d[0][0] - m) ** 2 + (d[1][0] - m) ** 2) / np.float32(2)
    assert np.array_equal(pol.act(2, inv, pend, d[1])[0], want(m, v))                      # n = 2
    m = (d[1][0] + d[2][0]) / np.float32(2)
    v = ((d[1][0] - m) ** 2 + (d[2][0] - m) ** 2) / np.float32(2)
    assert np.array_equal(pol.act(3, inv, pend, d[2])[0], want(m, v))                      # window slides
    assert np.array_equal(pol.act(0, inv, pend, d[2])[0], np.full((2, 2), -1.0, np.float32))  # reset clears
    assert pol.buf[0] == []


def test_random_stream_offsets_against_one_long_stream():
    seed, n_envs, T, W, K = 100, 3, 5, 2, 3
    per = T * W * K
    long = np.random.default_rng(seed).uniform(-1.0, 1.0, size=n_envs * per + 7)
    st = bl.random_stream_states(seed, n_envs, per)
    assert st.shape == (n_envs, 4) and st.dtype == np.uint64
    for k in range(n_envs):
        bg = np.random.PCG64()
        s = bg.state
        s["state"] = {"state": (int(st[k, 0]) << 64) | int(st[k, 1]), "inc": (int(st[k, 2]) << 64) | int(st[k, 3])}
        s["has_uint32"], s["uinteger"] = 0, 0
        bg.state = s
        g = np.random.Generator(bg)
        # the reference draws uniform(-1, 1, size=K) per agent and step
        got = np.concatenate([g.uniform(-1.0, 1.0, size=K) for _ in range(T * W)])
        assert np.array_equal(got, long[k * per:(k + 1) * per]), k


def test_random_emulation_matches_offsets():
    from marlsc.spec import EnvSpec
    spec = EnvSpec.from_config(_cfg_2x2(), {})
    T, wk = spec.episode_length, spec.W * spec.K
    r = emu.RandomEmulation(spec, 9, 3, 2 * T)
    long = np.random.default_rng(9).uniform(-1.0, 1.0, size=4 * T * wk).astype(np.float32)
    for s in range(2 * T):
        a = r.act(s % T, None, None, None)
        for k in range(3):
            o = k * T * wk + s * wk
            assert np.array_equal(a[k].ravel(), long[o:o + wk])


def test_public_names_are_reexported():
    import marlsc
    for n in ("RandomPolicy", "ConstantPolicy", "BaseStockPolicy", "AdaptiveBaseStockPolicy", "newsvendor_levels",
              "rollout_episodes", "calibrate_demand", "validation_sweep", "evaluate_levels", "optimize_levels"):
        assert getattr(marlsc, n) is getattr(bl, n)
