"""The lane throttle of the short-round demand parser (csrc/demand_v3.hip): a lane whose ring holds
less than a chunk's worth of generated positions sits that chunk out while its ring refills, instead
of holding its block for a generator top-up. The order records, counts, episode-ahead offsets and
the RNG state depend only on the consumed sequence, so every case is an oracle lockstep, bit-exact
on observations and state, per step and episode-ahead (4-step chunks)."""
import numpy as np
import pytest

torch = pytest.importorskip("torch")

import oracle as orc  # noqa: E402
from marlsc import make_synthetic_env_config  # noqa: E402
from marlsc.spec import EnvSpec  # noqa: E402
from marlsc.vec_env import VecInventoryEnv  # noqa: E402

pytestmark = pytest.mark.gpu
REW_ATOL = 1e-6  # (the parity suite's bar: rewards are float64 sums in another order)

CASES = {
    # 8 SKUs, every SKU drawn, quantity rate 9.9: mask units of 8 draws and Poisson units that run
    # past a round -- 8 draws in most rounds, against a refill of 21 per 4 rounds: the lanes
    # throttle nearly every chunk. 130 envs: a partial last wave.
    "throttle_always": dict(shape=(5, 24, 8), E=130, steps=16, seed=8,
                            cfg=dict(episode_length=7, lambda_orders=1.5, lambda_quantity=9.9, probability_skus=1.0)),
    # one SKU, quantity rate 0.4: 1-2 draws per round, the ring never runs short
    "throttle_never": dict(shape=(5, 24, 1), E=130, steps=16, seed=1,
                           cfg=dict(episode_length=7, lambda_orders=9.9, lambda_quantity=0.4)),
    # the headline's rates (4 / 0.667 / 5) and shape: throttled and unthrottled lanes share waves
    "c3_rates": dict(shape=(8, 64, 5), E=192, steps=21, seed=9, cfg=dict(episode_length=9)),
}


def _np(t):
    return t.detach().cpu().numpy()


@pytest.mark.parametrize("ea", ["0", "1"])
@pytest.mark.parametrize("case", list(CASES))
def test_throttled_demand_vs_oracle(monkeypatch, case, ea):
    monkeypatch.setenv("MSC_DEMAND_IMPL", "v3")
    monkeypatch.setenv("MSC_EA", ea)
    monkeypatch.setenv("MSC_EA_CHUNK", "4")
    c = CASES[case]
    (W, R, K), E = c["shape"], c["E"]
    spec = EnvSpec.from_config(make_synthetic_env_config(W, R, K, **c["cfg"]), {"include_warehouse_id": True})
    env = VecInventoryEnv(None, E, spec=spec, device=0, base_seed=777)
    choice = env.kernel_choice()
    assert choice["demand_impl"] == 9
    assert (choice["ea_slots"] > 0) == (ea == "1")
    ref = orc.OracleEnv(spec, E, base_seed=777)
    np.testing.assert_array_equal(_np(env.reset()), ref.reset())
    rng = np.random.default_rng(c["seed"])
    for t in range(c["steps"]):
        a = rng.uniform(-1, 1, size=(E, W, K)).astype(np.float32)
        og, _, tg, fg = env.step(torch.from_numpy(a).cuda(), want_f64=True)
        orr, rr, tr, fr = ref.step(a, final_obs=True, n_threads=8)
        assert np.array_equal(_np(tg).astype(bool), tr), f"truncation t={t}"
        np.testing.assert_array_equal(_np(og), orr, err_msg=f"obs t={t}")
        np.testing.assert_allclose(_np(env.rewards_f64), rr, rtol=0, atol=REW_ATOL, err_msg=f"t={t}")
        if tr.any():
            np.testing.assert_array_equal(_np(fg)[tr], fr[tr], err_msg=f"final obs t={t}")
        if t % 3 == 0 or t == c["steps"] - 1:
            sg, sr = env.read_state(), ref.read_state()
            for k in ("inventory", "rng", "timestep"):
                np.testing.assert_array_equal(sg[k], sr[k], err_msg=f"{k} t={t}")
    env.check()
