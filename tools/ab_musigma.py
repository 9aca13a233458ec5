"""A/B of the mu/sigma-head actor step at the C3 actor shape (262,144 rows of 34 -> [256, 256] -> K = 5):
  (a) free log_std: msc_mlp3_relu_forward_sampled (actor + sampling in one launch);
  (b) head, tier 1: msc_mlp3_relu_musigma (backbone -> folded dual head -> activations -> sampling);
  (c) head, tier 3: the torch layers, then msc_gaussian_sample with one log_std row per row.
HIP-event timed, warmed up, the variants alternated in one process; medians and the run-to-run
spread (5th .. 95th percentile) per variant, and the ratios (b)/(a), (c)/(b).

  python tools/ab_musigma.py [--rows 262144] [--rounds 200] [--warmup 20] [--out FILE] [--probe]"""
import argparse
import json
import os
import sys
from pathlib import Path

import numpy as np
import torch

sys.path.insert(0, str(Path(__file__).resolve().parents[1] / "marl-sc_amd"))


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=262144)
    ap.add_argument("--rounds", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--out", type=str, default=None)
    ap.add_argument("--probe", action="store_true", help="also time (b) without tanh and the one-pass forms")
    args = ap.parse_args()
    from marlsc.mlp import mlp3_forward, musigma_forward, musigma_tier
    from marlsc.rollout import LOG_STD_MIN, MLP, MuSigmaHead, gaussian_sample
    n, L, K = args.rows, 34, 5
    torch.manual_seed(0)
    free = list(MLP(L, K, {"hidden_sizes": [256, 256]}).cuda())
    actor = MLP(L, 256, {"hidden_sizes": [256, 256]}).cuda()
    head = MuSigmaHead(256, K, "tanh", None).cuda()
    assert musigma_tier(list(actor), head) == 1
    x = torch.randn(n, L, device="cuda")
    eps = torch.randn(n, K, device="cuda")
    ls = torch.full((1, K), -1.0, device="cuda")
    a, lp, c = torch.empty(n, K, device="cuda"), torch.empty(n, device="cuda"), torch.empty(n, K, device="cuda")

    def run_a():
        mlp3_forward(free, x, None, sample=(ls, -3.5, eps, a, lp, c))

    def run_b():
        musigma_forward(list(actor), head, x, sample=(eps, a, lp, c))

    def run_c():
        mu, s = head(actor(x))
        gaussian_sample(mu.contiguous(), s.contiguous(), LOG_STD_MIN, eps, a, lp)

    variants = {"a_free_logstd_fused": run_a, "b_head_fused": run_b, "c_head_torch_layers": run_c}
    if args.probe:
        # where (b) - (a) goes: the head without its tanh, and (a) / (b) with the output layer after
        # the layer-2 MFMAs instead of interleaved into them (MSC_MLP_P8=8, read at each launch)
        # (its own backbone copy: the pack cache lives on the backbone and holds one head's fold)
        plain, actor2 = MuSigmaHead(256, K).cuda(), MLP(L, 256, {"hidden_sizes": [256, 256]}).cuda()
        actor2.load_state_dict(actor.state_dict())

        def with_form(fn, form):
            def run():
                os.environ["MSC_MLP_P8"] = form
                fn()
                os.environ.pop("MSC_MLP_P8")
            return run

        variants["b_head_fused_no_tanh"] = lambda: musigma_forward(list(actor2), plain, x, sample=(eps, a, lp, c))
        variants["a_free_logstd_one_pass"] = with_form(run_a, "8")
        variants["b_head_fused_one_pass"] = with_form(run_b, "8")
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
    res = {"rows": n, "shape": [L, 256, 256, K], "rounds": args.rounds, "device": torch.cuda.get_device_name(0)}
    for k, v in times.items():
        v = np.asarray(v)
        res[k] = {"median_us": float(np.median(v)), "p05_us": float(np.percentile(v, 5)),
                  "p95_us": float(np.percentile(v, 95))}
        print(f"{k:22s} median {res[k]['median_us']:9.1f} us   p05 {res[k]['p05_us']:9.1f}   p95 {res[k]['p95_us']:9.1f}")
    med = lambda k: res[k]["median_us"]  # noqa: E731
    res["ratio_b_over_a"] = med("b_head_fused") / med("a_free_logstd_fused")
    res["ratio_c_over_b"] = med("c_head_torch_layers") / med("b_head_fused")
    print(f"(b)/(a) = {res['ratio_b_over_a']:.3f}   (c)/(b) = {res['ratio_c_over_b']:.3f}")
    print(json.dumps(res))
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text(json.dumps(res, indent=1) + "\n")
    return 0 if med("b_head_fused") < med("c_head_torch_layers") else 1


if __name__ == "__main__":
    sys.exit(main())
