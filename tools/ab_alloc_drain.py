"""A/B: what alloc_lane_kernel's sold-out test costs where it never triggers. C3 shape (8 x 64 x 5, ENVS
envs, per-step pipelined demand) on a `direct` action space at constant +1, which orders more than the
demand every step, so no env sells out and no block enters the tail (asserted). One handle, the option
MSC_OPT_ALLOC_TAIL alternated 1 / 0 every round of STEPS steps, HIP events around each round."""
import os
import sys
from pathlib import Path

REPO = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(REPO / "marl-sc_amd"))
import numpy as np  # noqa: E402
import torch  # noqa: E402

from marlsc import make_synthetic_env_config  # noqa: E402
from marlsc.spec import EnvSpec  # noqa: E402
from marlsc.vec_env import VecInventoryEnv  # noqa: E402

E = int(os.environ.get("ENVS", "32768"))
STEPS = int(os.environ.get("STEPS", "8"))
ROUNDS, WARM = int(os.environ.get("ROUNDS", "200")), int(os.environ.get("WARM", "20"))
cfg = make_synthetic_env_config(8, 64, 5)
cfg["action_space"] = {"type": "direct", "params": {"max_order_quantities": [250] * 5}}
spec = EnvSpec.from_config(cfg, {"include_warehouse_id": True})
env = VecInventoryEnv(None, E, spec=spec, device=0, base_seed=1234)
assert env.kernel_choice()["alloc"] == 0, env.kernel_choice()
act = torch.ones((E, 8, 5), device="cuda")
env.reset()
ms = {1: [], 0: []}
for rnd in range(WARM + ROUNDS):
    for tail in (1, 0):
        env.set_option(env.ALLOC_TAIL, tail)
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(STEPS):
            env.step(act)
        b.record()
        b.synchronize()
        if rnd >= WARM:
            ms[tail].append(a.elapsed_time(b) / STEPS)
            at = env.alloc_tail_entry()
            assert (at == -1).all(), (rnd, tail, at[at >= 0][:8])
env.close()
print(f"{E} envs, {ROUNDS} rounds of {STEPS} steps per setting after {WARM}; no block entered the tail; ms per step")
for tail in (1, 0):
    v = np.asarray(ms[tail])
    print(f"MSC_OPT_ALLOC_TAIL {tail}: median {np.median(v):.4f}  p05 {np.percentile(v, 5):.4f}  p95 {np.percentile(v, 95):.4f}")
