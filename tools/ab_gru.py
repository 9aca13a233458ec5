"""A/B of the GRU trunk step at the C3 rollout shape (262,144 rows of 34 -> 2 x GRU 128 -> 128):
  (a) the fused step: msc_gru_step (both layers and the output projection in one launch);
  (b) the torch layers: nn.GRU + output_proj under no_grad;
  (c) the yardstick: msc_mlp3_relu_forward 34 -> 256 -> 256 -> 5 (the fused actor MLP).
HIP-event timed, warmed up, the variants alternated in one process; medians and the run-to-run
spread (5th .. 95th percentile) per variant, the ratio (b)/(a), and the fraction of the 157.3 TFLOP/s
f32-MFMA peak (a) and (c) reach on their useful FLOP (2 FLOP per weight per row, biases and gate math
not counted).

  python tools/ab_gru.py [--rows 262144] [--rounds 200] [--warmup 20] [--hidden 128] [--out FILE]"""
import argparse
import json
import sys
from pathlib import Path

import numpy as np
import torch

sys.path.insert(0, str(Path(__file__).resolve().parents[1] / "marl-sc_amd"))

F32_MFMA_PEAK = 157.3e12  # FLOP/s


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=262144)
    ap.add_argument("--rounds", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--hidden", type=int, default=128, help="GRU hidden size (and output_dim) of (a) / (b)")
    ap.add_argument("--out", type=str, default=None)
    args = ap.parse_args()
    from marlsc.gru import gru_step_forward, gru_tier, torch_step
    from marlsc.mlp import mlp3_forward
    from marlsc.rollout import MLP, GRUNet
    n, L, H, O, K = args.rows, 34, args.hidden, args.hidden, 5
    torch.manual_seed(0)
    net = GRUNet(L, O, {"hidden_size": H, "num_layers": 2, "max_seq_len": 20}).cuda()
    mlp = list(MLP(L, K, {"hidden_sizes": [256, 256]}).cuda())
    assert gru_tier(net) == 1
    x = torch.randn(n, L, device="cuda")
    h = torch.rand(n, 2, H, device="cuda") * 2 - 1
    y, h_out = torch.empty(n, O, device="cuda"), torch.empty(n, 2, H, device="cuda")
    out = torch.empty(n, K, device="cuda")
    variants = {"a_fused_step": lambda: gru_step_forward(net, x, h, h_out=h_out, y=y),
                "b_torch_layers": lambda: torch_step(net, x, h),
                "c_mlp3_34_256_256_5": lambda: mlp3_forward(mlp, x, out)}
    flop = {"a_fused_step": 2.0 * n * (3 * H * (L + H) + 3 * H * (H + H) + H * O),
            "c_mlp3_34_256_256_5": 2.0 * n * (L * 256 + 256 * 256 + 256 * K)}
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
    res = {"rows": n, "shape": [L, H, H, O], "rounds": args.rounds, "device": torch.cuda.get_device_name(0)}
    for k, v in times.items():
        v = np.asarray(v)
        res[k] = {"median_us": float(np.median(v)), "p05_us": float(np.percentile(v, 5)),
                  "p95_us": float(np.percentile(v, 95))}
        line = f"{k:22s} median {res[k]['median_us']:9.1f} us   p05 {res[k]['p05_us']:9.1f}   p95 {res[k]['p95_us']:9.1f}"
        if k in flop:
            res[k]["gflop"] = flop[k] / 1e9
            res[k]["mfma_peak_fraction"] = flop[k] / (res[k]["median_us"] * 1e-6) / F32_MFMA_PEAK
            line += f"   {res[k]['gflop']:.1f} GFLOP, {100 * res[k]['mfma_peak_fraction']:.1f} % of the f32-MFMA peak"
        print(line)
    res["ratio_b_over_a"] = res["b_torch_layers"]["median_us"] / res["a_fused_step"]["median_us"]
    res["bands_disjoint"] = res["a_fused_step"]["p95_us"] < res["b_torch_layers"]["p05_us"]
    print(f"(b)/(a) = {res['ratio_b_over_a']:.3f}   p05-p95 bands disjoint: {res['bands_disjoint']}")
    print(json.dumps(res))
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text(json.dumps(res, indent=1) + "\n")
    return 0 if res["bands_disjoint"] else 1


if __name__ == "__main__":
    sys.exit(main())
