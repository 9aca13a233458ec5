"""A/B of the centralised (CPPO) actor's rollout step, forward + action sampling:
  (a) the wide fused kernel: mlp.wide_forward with the sampling epilogue (msc_mlp{2,3}_relu_wide), one launch;
  (b) the torch layers (Linear + ReLU as one GEMM with the ReLU in its epilogue, then the output Linear:
      what rollout.mlp_forward runs when no fused kernel applies) plus msc_gaussian_sample -- the only
      route a policy with more than 32 outputs has without the wide kernel.
Shapes: 32,768 rows of 8 L -> 256 -> 40 (C3) and 8,192 rows of 16 L -> 256 -> 80 (C5), L the env config's
local observation without the warehouse one-hot, and the [256, 256] forms of both.
HIP-event timed, warmed up, the variants alternated in one process; medians and the 5th .. 95th percentile
per variant, the ratio (b)/(a), and the achieved FLOP/s of (a) against the 157.3 TFLOP/s f32 matrix peak
(2 FLOP per weight per row; biases and the sampling arithmetic not counted).

  python tools/ab_cppo.py [--rounds 200] [--warmup 20] [--out profiles/cppo/ab_cppo.txt]"""
import argparse
import json
import sys
from pathlib import Path

import numpy as np
import torch

REPO = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(REPO / "marl-sc_amd"))

F32_MFMA_PEAK = 157.3e12  # FLOP/s


def _local_obs_dim(env_yaml: str) -> int:
    from marlsc import load_environment_config
    from marlsc.spec import EnvSpec
    cfg = load_environment_config(str(REPO / "config_files/environments" / env_yaml), allow_nr_ne_nw=True)
    return EnvSpec.from_config(cfg, {"include_warehouse_id": False}).local_obs_dim


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--out", type=str, default=None)
    args = ap.parse_args()
    from marlsc import mlp as M
    from marlsc.rollout import MLP, gaussian_sample, mlp_forward
    l3, l5 = _local_obs_dim("env_c3_8wh64r5sku.yaml"), _local_obs_dim("env_c5_16wh256r5sku.yaml")
    shapes = [("c3", 32768, 8 * l3, [256], 40), ("c5", 8192, 16 * l5, [256], 80),
              ("c3", 32768, 8 * l3, [256, 256], 40), ("c5", 8192, 16 * l5, [256, 256], 80)]
    lines = [f"device: {torch.cuda.get_device_name(0)}   rounds {args.rounds}, warmup {args.warmup}, variants alternated"]
    results = []
    torch.manual_seed(0)
    for name, n, L, hidden, K in shapes:
        net = MLP(L, K, {"hidden_sizes": hidden}).cuda()
        mods = list(net)
        assert M.wide_layers(mods) == len(hidden) + 1
        x, eps = torch.randn(n, L, device="cuda"), torch.randn(n, K, device="cuda")
        ls = torch.full((1, K), -1.0, device="cuda")
        act, logp, clip = torch.empty(n, K, device="cuda"), torch.empty(n, device="cuda"), torch.empty(n, K, device="cuda")

        def fused():
            M.wide_forward(mods, x, None, sample=(ls, -3.5, eps, act, logp, clip))

        def torch_layers():
            M.ENABLED = False  # mlp_forward's route without a fused kernel
            try:
                mean = mlp_forward(net, x)
            finally:
                M.ENABLED = True
            gaussian_sample(mean.contiguous(), ls, -3.5, eps, act, logp)

        variants = {"a_wide_fused": fused, "b_torch_plus_sample": torch_layers}
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
        dims = [L] + hidden + [K]
        flop = 2.0 * n * sum(a * b for a, b in zip(dims[:-1], dims[1:]))
        res = {"env": name, "rows": n, "shape": dims, "gflop": flop / 1e9}
        lines.append(f"{name}: {n} rows of {' -> '.join(map(str, dims))}   ({flop / 1e9:.2f} GFLOP)")
        for k, v in times.items():
            v = np.asarray(v)
            res[k] = {"median_us": float(np.median(v)), "p05_us": float(np.percentile(v, 5)),
                      "p95_us": float(np.percentile(v, 95)), "min_us": float(v.min()), "max_us": float(v.max())}
            tf = flop / (res[k]["median_us"] * 1e-6)
            res[k]["tflops"] = tf / 1e12
            lines.append(f"  {k:20s} median {res[k]['median_us']:8.1f} us   p05 {res[k]['p05_us']:8.1f}   p95 {res[k]['p95_us']:8.1f}"
                         f"   range {res[k]['min_us']:.1f} .. {res[k]['max_us']:.1f}   {tf / 1e12:6.2f} TFLOP/s = "
                         f"{100 * tf / F32_MFMA_PEAK:.1f} % of the f32 matrix peak")
        res["ratio_b_over_a"] = res["b_torch_plus_sample"]["median_us"] / res["a_wide_fused"]["median_us"]
        lines.append(f"  (b)/(a) = {res['ratio_b_over_a']:.3f}")
        results.append(res)
    ok = all(r["ratio_b_over_a"] >= 1.0 for r in results[:2])  # the default needs (a) not slower at both [256] shapes
    lines.append(f"wide kernel not slower than the torch route at both one-hidden-layer shapes: {ok}")
    text = "\n".join(lines) + "\n"
    print(text)
    print(json.dumps(results))
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text(text)
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
