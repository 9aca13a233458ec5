"""A/B of the baseline policies' action step at the C3 shape (8 warehouses x 64 regions x 5 SKUs), 32,768 envs:
  (a) msc_policy_act (csrc/policy.hip), one launch on the env's own device state: fixed base-stock levels,
      and the adaptive rule with a full window of H = 20;
  (b) the same actions composed from torch ops on msc_step_info tensors (inventory_before, pending_total,
      demand_per_region of a step taken with the info dump): what a caller without the kernel would run;
      the adaptive rule keeps its window as a [H, E, W, K] f32 tensor and takes torch's mean / var over it;
  (c) the env step alone (msc_env_step on the caller's stream, actions resident).
The policy variants run on a handle parked 25 steps into an episode, (c) on a second handle that keeps
stepping. HIP-event timed, warmed up, the variants alternated in one process; medians and the 5th .. 95th
percentile per variant, the ratios (a)/(c) and (b)/(a), and whether the (a) and (b) bands are disjoint.
One further line: agent-steps/s of a base-stock rollout (act + step, no host sync inside) on the parked handle.

  python tools/ab_baseline.py [--rounds 200] [--warmup 20] [--envs 32768] [--out profiles/baselines/ab_baseline.txt]"""
import argparse
import json
import sys
import time
from pathlib import Path

import numpy as np
import torch

REPO = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(REPO / "marl-sc_amd"))


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--envs", type=int, default=32768)
    ap.add_argument("--rollout-steps", type=int, default=300)
    ap.add_argument("--out", type=str, default=None)
    args = ap.parse_args()
    from marlsc import baselines as bl
    from marlsc import load_environment_config
    from marlsc.spec import EnvSpec
    from marlsc.vec_env import VecInventoryEnv
    cfg = load_environment_config(str(REPO / "config_files/environments/env_c3_8wh64r5sku.yaml"), allow_nr_ne_nw=True)
    cfg = cfg.to_dict()
    cfg["action_space"] = {"type": "direct", "params": {"max_order_quantities": [40] * cfg["n_skus"]}}
    spec = EnvSpec.from_config(cfg, {"include_warehouse_id": True})
    E, H = args.envs, 20
    env = VecInventoryEnv(None, E, spec=spec, device=0, base_seed=1234)
    env_c = VecInventoryEnv(None, E, spec=spec, device=0, base_seed=4321)
    W, K, dev = env.W, env.K, env.device
    S = bl.newsvendor_levels(cfg, 1.0)
    bs = bl.BaseStockPolicy(env, S)
    ad = bl.AdaptiveBaseStockPolicy(env, 1.0, H)
    info = env.alloc_info()
    env.reset()
    env_c.reset()
    for _ in range(25):  # park the policy handle mid-episode, the adaptive window full
        env.step(ad.act(env), want_final_obs=False, info=info)
    for _ in range(H):
        ad.act(env)
    act_c = bs.act(env).clone()

    S_t = torch.from_numpy(S).to(dev)
    maxq = torch.from_numpy(np.asarray(spec.action_param, np.float64)).to(dev)
    lead = torch.from_numpy(np.asarray(spec.expected_lead_times, np.float64).reshape(W, K)).to(dev)
    home = torch.from_numpy(np.asarray(spec.home_regions, np.int64)).to(dev)
    window = torch.zeros((H, E, W, K), dtype=torch.float32, device=dev)
    slot = [0]

    def order_up_to(level):
        x = level - info["inventory_before"].double() - info["pending_total"].double()
        return (2.0 * torch.minimum(x.clamp_min(0.0), maxq) / maxq - 1.0).float()

    def torch_bs():
        return order_up_to(S_t)

    def torch_ad():
        window[slot[0] % H] = info["demand_per_region"][:, home, :].float()
        slot[0] += 1
        mean, var = window.mean(0), window.var(0, unbiased=False)
        return order_up_to(lead * mean.double() + 1.0 * torch.sqrt(lead * var.double()))

    variants = {"a_kernel_base_stock": lambda: bs.act(env), "a_kernel_adaptive_h20": lambda: ad.act(env),
                "b_torch_base_stock": torch_bs, "b_torch_adaptive_h20": torch_ad,
                "c_env_step": lambda: env_c.step(act_c, want_final_obs=False)}
    times = {k: [] for k in variants}
    with torch.no_grad():
        for _ in range(args.warmup):
            for fn in variants.values():
                fn()
        torch.cuda.synchronize()
        for _ in range(args.rounds):
            for k, fn in variants.items():
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                fn()
                e1.record()
                e1.synchronize()
                times[k].append(e0.elapsed_time(e1) * 1e3)  # us
    lines = [f"device: {torch.cuda.get_device_name(0)}   C3 shape {W} x {env.R} x {K}, {E} envs, ring of "
             f"{int(spec.expected_lead_times.max())}+ slots   rounds {args.rounds}, warmup {args.warmup}, variants alternated"]
    res = {}
    for k, v in times.items():
        v = np.asarray(v)
        res[k] = {"median_us": float(np.median(v)), "p05_us": float(np.percentile(v, 5)),
                  "p95_us": float(np.percentile(v, 95)), "min_us": float(v.min()), "max_us": float(v.max())}
        lines.append(f"  {k:24s} median {res[k]['median_us']:8.1f} us   p05 {res[k]['p05_us']:8.1f}   p95 {res[k]['p95_us']:8.1f}"
                     f"   range {res[k]['min_us']:.1f} .. {res[k]['max_us']:.1f}")
    for rule in ("base_stock", "adaptive_h20"):
        a, b, c = res[f"a_kernel_{rule}"], res[f"b_torch_{rule}"], res["c_env_step"]
        res[f"ratio_a_over_c_{rule}"] = a["median_us"] / c["median_us"]
        res[f"ratio_b_over_a_{rule}"] = b["median_us"] / a["median_us"]
        res[f"bands_disjoint_{rule}"] = bool(a["p95_us"] < b["p05_us"])
        lines.append(f"  {rule}: (a)/(c) = {res[f'ratio_a_over_c_{rule}']:.4f}   (b)/(a) = {res[f'ratio_b_over_a_{rule}']:.2f}"
                     f"   kernel p95 below torch p05 (disjoint bands): {res[f'bands_disjoint_{rule}']}")
    n = args.rollout_steps
    for _ in range(10):
        env.step(bs.act(env), want_final_obs=False)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(n):
        env.step(bs.act(env), want_final_obs=False)
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    env.check()
    res["rollout_agent_steps_per_s"] = E * W * n / dt
    lines.append(f"  base-stock rollout (act + step), {n} steps: {E * W * n / dt / 1e6:.1f} M agent-steps/s"
                 f"   ({dt / n * 1e3:.4f} ms per step)")
    text = "\n".join(lines) + "\n"
    print(text)
    print(json.dumps(res))
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text(text)
    for p in (bs, ad):
        p.close()
    env.close()
    env_c.close()
    return 0


if __name__ == "__main__":
    sys.exit(main())
