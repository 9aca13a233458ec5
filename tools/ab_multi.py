"""A/B of per-agent policies (parameter_sharing: false) at rollout: the torch path (W layer sequences on
strided slices, two stacks and msc_gaussian_sample: what MultiAgentActorCritic runs with the switch off)
against the multi-policy kernel (mlp.multi_forward -> msc_mlp{2,3}_relu_multi, one launch for the W actors
with their sampling and one for the W critics), the latter in both block orders (MSC_MULTI_ORDER = 0
policy-major, 1 policy-minor, the default; read at each launch).
Networks: ippo.yaml (actor / critic [256], local critic) and mappo.yaml (actor [256, 256], critic [64, 64]
on the global observation, split first layer), one policy per agent. Shapes: C3 (32,768 envs x 8 agents)
and C5 (8,192 x 16). Timed per variant: the actor step (forward + sampling + clip), the critic, and one
full RolloutCollector step (collect() of --steps steps on the real env, per step).
HIP-event timed, warmed up, the variants alternated in one process; median, 5th .. 95th percentile and the
spread (p95 - p05) / median per variant, and torch / multi ratios. A default flip needs the multi kernel
faster at both shapes and for both configs by more than the spread of repeated runs of the same path.

  python tools/ab_multi.py [--rounds 100] [--warmup 10] [--steps 8] [--rollout-rounds 6] [--shapes c3,c5]
                           [--out profiles/mlp_multi/ab_multi.json]"""
import argparse
import json
import os
import sys
from pathlib import Path

import numpy as np
import torch
import yaml

REPO = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(REPO / "marl-sc_amd"))

SHAPES = {"c3": ("env_c3_8wh64r5sku.yaml", 32768), "c5": ("env_c5_16wh256r5sku.yaml", 8192)}
VARIANTS = [("torch", False, "0"), ("multi_policy_major", True, "0"), ("multi_policy_minor", True, "1")]


def _stats(v):
    v = np.asarray(v)
    med = float(np.median(v))
    p05, p95 = float(np.percentile(v, 5)), float(np.percentile(v, 95))
    return {"median_us": med, "p05_us": p05, "p95_us": p95, "min_us": float(v.min()), "max_us": float(v.max()),
            "spread": (p95 - p05) / med}


def _timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) * 1e3  # us


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--steps", type=int, default=8)
    ap.add_argument("--rollout-rounds", type=int, default=6)
    ap.add_argument("--shapes", type=str, default="c3,c5")
    ap.add_argument("--algos", type=str, default="ippo,mappo")
    ap.add_argument("--out", type=str, default=None)
    args = ap.parse_args()
    from marlsc import load_environment_config
    from marlsc.ppo import MultiAgentActorCritic, PPOConfig
    from marlsc.rollout import RolloutCollector, gaussian_sample
    from marlsc.spec import EnvSpec
    from marlsc.vec_env import VecInventoryEnv
    results = []
    lines = [f"device: {torch.cuda.get_device_name(0)}   rounds {args.rounds}, warmup {args.warmup}, variants alternated"]
    for shape in args.shapes.split(","):
        env_yaml, E = SHAPES[shape]
        env_cfg = load_environment_config(str(REPO / "config_files/environments" / env_yaml), allow_nr_ne_nw=True)
        spec = EnvSpec.from_config(env_cfg, {"include_warehouse_id": False})
        for algo in args.algos.split(","):
            raw = yaml.safe_load(open(REPO / f"config_files/algorithms/{algo}.yaml"))
            raw["algorithm"]["algorithm_specific"]["parameter_sharing"] = False
            rc = PPOConfig.from_algorithm_config(raw).rollout_config()
            env = VecInventoryEnv(None, E, spec=spec, device=0, base_seed=1)
            obs = env.reset()
            W, K, L = env.W, env.K, env.local_obs_dim
            torch.manual_seed(0)
            m = MultiAgentActorCritic(W, L, L * W, K, rc, False, multi_mlp=True).cuda()
            col = RolloutCollector(env, m, args.steps, seed=3, adv_groups=W)
            eps = torch.randn(E, W, K, device="cuda")
            act, logp, clip = torch.empty(E, W, K, device="cuda"), torch.empty(E, W, device="cuda"), torch.empty(E, W, K, device="cuda")
            ls, floor = m.log_std_table(), rc.logstd_floor
            vout = torch.empty(E, W, device="cuda")

            def actor():
                if not m.actor_sample(obs, None, (ls, floor, eps, act, logp, clip)):
                    gaussian_sample(m.actor_mean(obs, None).contiguous(), ls, floor, eps, act, logp)

            def critic():
                m.values(obs, None, out=vout)

            def rollout():
                col.collect(normalize=False)

            def select(multi, order):
                m.multi_mlp = multi
                os.environ["MSC_MULTI_ORDER"] = order

            res = {"shape": shape, "algo": algo, "envs": E, "agents": W, "local_obs": L, "actions": K,
                   "actor": list((rc.actor or {}).get("hidden_sizes", [])), "critic": list((rc.critic or {}).get("hidden_sizes", [])),
                   "critic_obs": rc.critic_obs_type, "rollout_steps": args.steps}
            lines.append(f"{shape} {algo}: {E} envs x {W} agents, L {L}, K {K}, actor {res['actor']}, critic {res['critic']} ({rc.critic_obs_type})")
            with torch.no_grad():
                for what, fn, rounds, div in (("actor", actor, args.rounds, 1), ("critic", critic, args.rounds, 1),
                                              ("rollout_step", rollout, args.rollout_rounds, args.steps)):
                    times = {k: [] for k, _, _ in VARIANTS}
                    for _ in range(max(1, args.warmup if div == 1 else 1)):
                        for k, multi, order in VARIANTS:
                            select(multi, order)
                            fn()
                    torch.cuda.synchronize()
                    for _ in range(rounds):
                        for k, multi, order in VARIANTS:
                            select(multi, order)
                            times[k].append(_timed(fn) / div)
                    res[what] = {k: _stats(v) for k, v in times.items()}
                    t = res[what]["torch"]["median_us"]
                    for k, _, _ in VARIANTS:
                        s = res[what][k]
                        s["torch_over_this"] = t / s["median_us"]
                        lines.append(f"  {what:12s} {k:20s} median {s['median_us']:9.1f} us   p05 {s['p05_us']:9.1f}   p95 {s['p95_us']:9.1f}"
                                     f"   spread {100 * s['spread']:5.1f} %   torch / this = {s['torch_over_this']:.3f}")
            os.environ.pop("MSC_MULTI_ORDER", None)
            results.append(res)
            del col, m, env
            torch.cuda.empty_cache()
    # the rule for a default flip, per block order: faster everywhere by more than the measured spread
    verdict = {}
    for k, _, _ in VARIANTS[1:]:
        verdict[k] = all(r[w][k]["torch_over_this"] - 1.0 > max(r[w][k]["spread"], r[w]["torch"]["spread"])
                         for r in results for w in ("actor", "critic", "rollout_step"))
        lines.append(f"{k}: faster than the torch path everywhere by more than the spread: {verdict[k]}")
    text = "\n".join(lines) + "\n"
    print(text)
    out = {"device": torch.cuda.get_device_name(0), "rounds": args.rounds, "warmup": args.warmup, "results": results,
           "faster_everywhere_beyond_spread": verdict}
    print(json.dumps(out))
    if args.out:
        p = Path(args.out)
        p.parent.mkdir(parents=True, exist_ok=True)
        p.write_text(json.dumps(out, indent=1) + "\n")
        p.with_suffix(".txt").write_text(text)
    return 0


if __name__ == "__main__":
    sys.exit(main())
