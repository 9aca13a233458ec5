"""CPU probe (C oracle, no GPU): how early in a step's region-major order list the envs of the bench
workloads sell out, i.e. how much of the list a sold-out tail would take over.

  python tools/probe_drain.py > profiles/alloc_drain/probe_drain.txt

c3: make_synthetic_env_config(8, 64, 5), Poisson demand, uniform[-1, 1] actions, steps 8-39 of an
episode; once with ENVS_C3 envs (lane allocator: 64 envs per wave) and once with the C2 env count
(scan allocator: one env per wave). c5: 16 x 256 x 5 with bench.py's synthetic trace (step_b: 4 envs
per wave at 16 lanes per env). Per step and env: the last region that received a shipment, as a share
of the regions (an env with no shipment: 0); the same for groups of envs (a wave switches when its
last env has); shipments per order; the fraction of orders lost."""
import os
import sys
from pathlib import Path

REPO = Path(__file__).resolve().parents[1]
sys.path[:0] = [str(REPO / "marl-sc_amd"), str(REPO / "oracle")]
import numpy as np  # noqa: E402

import oracle as orc  # noqa: E402
from marlsc import make_synthetic_env_config  # noqa: E402
from marlsc.spec import EnvSpec  # noqa: E402
from marlsc.synthetic import make_synthetic_trace  # noqa: E402


def probe(label, spec, E, groups, seed=4321, act_seed=0, steps=range(8, 40)):
    ref = orc.OracleEnv(spec, E, base_seed=seed)
    ref.reset()
    rng = np.random.default_rng(act_seed)
    share, zero_start, ships, orders, lost = [], [], 0, 0, 0
    for t in range(steps.stop):
        a = rng.uniform(-1, 1, size=(E, spec.W, spec.K)).astype(np.float32)
        inv = ref.read_state()["inventory"]
        info = ref.alloc_info()
        ref.step(a, info=info, n_threads=8)
        if t not in steps:
            continue
        zero_start.append(float((inv.reshape(E, -1).sum(axis=1) == 0).mean()))
        got = info["shipment_counts"].sum(axis=1) > 0  # [E, R]
        last = np.where(got.any(axis=1), spec.R - np.argmax(got[:, ::-1], axis=1), 0)  # regions up to the last shipment
        share.append(last / spec.R)
        ships += int(info["shipment_counts"].sum())
        orders += int(info["n_orders"].sum())
        lost += int(info["lost_order_counts"].sum())
    share = np.asarray(share)  # [steps, E]
    print(f"{label}: {E} envs, steps {steps.start}-{steps.stop - 1}")
    print(f"  envs with zero inventory at the start of the step (before arrivals): {np.mean(zero_start):.3f}")
    print(f"  share of regions up to the last shipment, per env: mean {share.mean():.3f}  p95 {np.percentile(share, 95):.3f}"
          f"  max {share.max():.3f}")
    for g in groups:
        if E % g == 0 and E >= g:
            gs = share.reshape(len(share), E // g, g).max(axis=2)
            print(f"  per group of {g} envs (the latest of the group): mean {gs.mean():.3f}  worst group-step {gs.max():.3f}")
    print(f"  shipments per order {ships / orders:.3f}; orders lost {lost / orders:.3f}")
    return share.mean()


def main():
    meta = {"include_warehouse_id": True}
    c3 = EnvSpec.from_config(make_synthetic_env_config(8, 64, 5), meta)
    probe("c3 (lane allocator, 64 envs per wave)", c3, int(os.environ.get("ENVS_C3", "2048")), (64,))
    c2 = probe("c3 shape at the C2 env count (scan allocator, one env per wave)", c3, int(os.environ.get("ENVS_C2", "4096")),
               (64,))
    cfg = make_synthetic_env_config(16, 256, 5)
    cfg["components"]["demand_sampler"] = {"type": "empirical", "params": None}
    c5 = EnvSpec.from_config(cfg, dict(meta, demand_trace=make_synthetic_trace(256, 5, 300, orders_per_step=(200, 1000), seed=0)))
    probe("c5 (step_b, 4 envs per wave)", c5, int(os.environ.get("ENVS_C5", "512")), (4, 64))
    print(f"""reading: the orders are region-major, so the share of regions is close to the share of the order list.
An env's own switch point is what a one-env-per-wave kernel would gain from, a group's what a kernel with that many envs
per wave gains from. alloc_scan_kernel (C2) switches each wave at its own env's point: on average {1 - c2:.2f} of the list
is tail there, more than the lane kernel's 64-env waves see, so the same treatment is worth building for it. step_b (C5,
groups of 4) sees nearly the per-env share as well and is worth it too, with the caveat that its trace steps differ in
length (200-1,000 orders) and the per-step share says nothing about which steps dominate the time.""")


main()
