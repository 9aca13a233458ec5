"""A/B of the learner's minibatch step with the torch loss (marlsc/ppo.py:ppo_loss under autograd, the default)
and with the fused loss kernel (msc_ppo_loss, PPOLearner(fused_loss=True), opt-in):
  step:  PPOLearner.minibatch_step itself, the step PPOLearner.update runs, on fixed rows -- gather, forward, loss,
         backward, gradient clip, Adam, and the per-step statistics (the torch path reads them on the host every
         step, the fused path adds them up on the device); one learner per switch combination over one module;
  loss:  the loss with its backward alone, from given network outputs to their gradients (torch: the v[idx]
         gathers, ppo_loss, backward; fused: fused_ppo_loss, backward), no statistic read on the host.
Shapes: the reference ippo.yaml networks (actor / critic [256], local observations) and the mappo.yaml networks
(actor [256, 256], global critic [64, 64], KL term on) with the C3 observation width and K = 5, 8 agents
sharing one policy; a minibatch of 800 rows out of an 8,000-step batch (64,000 rows), and one of 262,144 rows
(32,768 envs x 8 agents, the whole batch).
Each step also runs with the fused MLP backward (msc_mlp_relu_backward, PPOLearner(fused_mlp=True), opt-in): step_mlp is
the torch loss with the MLPs through mlp.train_forward, step_fused_mlp the fused loss with them (the intended fast
path). A last row runs 8 per-agent policies (ippo.yaml networks) at 800 rows each, one backward call per network.
Each of step_torch, step_fused and step_fused_mlp also runs with the fused clip + Adam step (msc_adam_clip_step,
marlsc/optim.py:FusedClipAdam, PPOLearner(fused_opt=True), opt-in) in place of clip_grad_norm_ + torch.optim.Adam.step:
step_torch_opt, step_fused_opt, step_fused_mlp_opt. A third split times the clip and the Adam step alone from the
gradients a backward left, through the learner's own clip_and_step (opt_torch: clip_grad_norm_ per policy +
Adam.step; opt_fused: one FusedClipAdam.step). The per-agent row's step_torch / step_fused / step_mlp /
step_fused_mlp clip per policy, as the learner does: they are not comparable with the same rows of
profiles/{ppo_loss,mlp_backward,adam_clip}/ab_learner.txt, which a hand-written step with one clip_grad_norm_
call over all policies produced (profiles/learner_loop/ab_learner.txt is the first record of this step).
The per-agent rows (8 ippo.yaml policies, 8 mappo.yaml policies, 16 ippo.yaml policies -- the C5 agent count --
at 800 rows each) also run step_fused_mlp_opt_multi: all four switches on, the P actors and the P critics
through one mlp.multi_train_forward each (msc_mlp_relu_backward_multi, PPOLearner(fused_multi=True), opt-in),
compared with step_fused_mlp_opt of the same run. A fourth split times the MLP backward alone at these shapes on
one d_out: bwd_single is P mlp.mlp_backward calls on each policy's gathered rows (the gather not timed), bwd_multi
one mlp.multi_backward call.
They also run step_fused_mlp_opt_multi_loss: all five switches on, the P losses from one msc_ppo_loss_multi call on
the stacked outputs (PPOLearner(fused_multi_loss=True), opt-in), compared with step_fused_mlp_opt_multi of the same
run. A fifth split times the loss with its backward alone from given stacked network outputs: loss_single is P
fused_ppo_loss calls on each policy's contiguous slices (the slicing not timed), summed, and one backward();
loss_multi one fused_ppo_loss_multi call and its backward().
The variants are alternated in one process after a warm-up; each sample is one step between two device
events, the device idle before the first (synchronised). Medians, the 5th .. 95th percentile and the range.

  python tools/ab_learner.py [--rounds 100] [--rounds-large 20] [--warmup 10] [--out profiles/learner_loop/ab_learner.txt]
  python tools/ab_learner.py --per-agent-only    # the per-agent rows alone
  python tools/ab_learner.py --count-launches   # a few steps of each variant at 800 rows, for a kernel trace
  python tools/ab_learner.py --count-launches --variant step_fused_mlp_opt_multi --steps 12
      # --steps steps of one per-agent variant (8 ippo.yaml policies): the kernel records of two traces with
      # different --steps, subtracted and divided by the difference in steps, are the launches of one step"""
import argparse
import json
import sys
from pathlib import Path

import numpy as np
import torch
import yaml

REPO = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(REPO / "marl-sc_amd"))


def _local_obs_dim() -> int:
    from marlsc import load_environment_config
    from marlsc.spec import EnvSpec
    cfg = load_environment_config(str(REPO / "config_files/environments/env_c3_8wh64r5sku.yaml"), allow_nr_ne_nw=True)
    return EnvSpec.from_config(cfg, {"include_warehouse_id": True}).local_obs_dim


def _setup(name: str, S: int, W: int, L: int, K: int, shared: bool = True):
    """(cfg, module, batch [S, W, ...]) for config_files/algorithms/<name>.yaml with a shared policy (or W)."""
    from marlsc.ppo import MultiAgentActorCritic, PPOConfig, gaussian_logp
    cfg = PPOConfig.from_algorithm_config(yaml.safe_load(open(REPO / f"config_files/algorithms/{name}.yaml")))
    torch.manual_seed(0)
    m = MultiAgentActorCritic(W, L, L * W, K, cfg.rollout_config(), shared).cuda()
    obs = torch.randn(S, W, L, device="cuda")
    with torch.no_grad():
        mean = torch.cat([m.policies[0].actor(o) for o in obs.split(4096)])  # (policy 0's mean serves every agent)
        ls = torch.clamp(m.policies[0].log_std, min=m.rc.logstd_floor).expand_as(mean).contiguous()
        act = mean + ls.exp() * torch.randn_like(mean)
        logp = gaussian_logp(act, mean, ls) + 0.1 * torch.randn(S, W, device="cuda")
    batch = {"actions": act, "logp": logp, "advantages": torch.randn(S, W, device="cuda"),
             "value_targets": torch.randn(S, W, device="cuda")}
    if cfg.use_kl_loss:
        batch["mean_old"], batch["log_std_old"] = mean + 0.02, ls.clone()
    return cfg, m, obs, batch


# the step variants: name -> (fused_loss, fused_mlp, fused_opt, fused_multi[, fused_multi_loss]) of the PPOLearner that
# runs them
SWITCHES = {"step_torch": (False, False, False, False), "step_fused": (True, False, False, False),
            "step_mlp": (False, True, False, False), "step_fused_mlp": (True, True, False, False),
            "step_torch_opt": (False, False, True, False), "step_fused_opt": (True, False, True, False),
            "step_fused_mlp_opt": (True, True, True, False)}
MULTI = "step_fused_mlp_opt_multi"  # per-agent rows only (a no-op on a shared policy)
MULTI_LOSS = "step_fused_mlp_opt_multi_loss"  # the same


class Steps:
    """PPOLearner.minibatch_step on fixed rows (one index tensor per policy), one learner per switch combination
    over the same module, each with its own optimizer and statistics accumulator."""

    def __init__(self, cfg, m, obs, batch, rows, multi=False):
        from marlsc.ppo import PPOLearner
        self.cfg, self.obs, self.rows = cfg, obs, rows
        self.switches = dict(SWITCHES, **({MULTI: (True, True, True, True),
                                           MULTI_LOSS: (True, True, True, True, True)} if multi else {}))
        S, W = obs.shape[0], obs.shape[1]
        self.flat = {k: v.reshape(S * W, *v.shape[2:]) for k, v in batch.items()}
        self.learners = {k: PPOLearner(m, cfg, seed=0, fused_loss=fl, fused_mlp=fm, fused_opt=fo, fused_multi=mu,
                                       fused_multi_loss=bool(ml))
                         for k, (fl, fm, fo, mu, *ml) in self.switches.items()}
        self.stats = {k: ln.new_stats(obs.device) for k, ln in self.learners.items()}
        self.dev_stats = torch.zeros(5, dtype=torch.float64, device="cuda")
        # the clip and the Adam step alone, on the gradients the last backward left in place
        self.opt_torch = self.learners["step_torch"].clip_and_step
        self.opt_fused = self.learners["step_torch_opt"].clip_and_step

    def step_variants(self):
        return {k: (lambda k=k: self.learners[k].minibatch_step(self.obs, None, self.flat, self.rows, self.stats[k]))
                for k in self.switches}

    def backward_variants(self):
        """The MLP backward alone, actors then critics, on one upstream gradient: P single-policy calls on each
        policy's gathered rows against one multi-policy call on the rows where they lie."""
        from marlsc import mlp as M
        ln = self.learners[MULTI]
        S, W, L = self.obs.shape
        idx = torch.stack(list(self.rows), dim=1)
        local = self.obs.reshape(S * W, L)[idx]
        full = torch.cat([local, self.obs.reshape(S, W * L)[torch.div(idx, W, rounding_mode="floor")]], dim=-1)
        jobs = []
        for kind, nets in ((ln.module.rc.actor_obs_type, [list(p.actor) for p in ln.module.policies]),
                           (ln.module.rc.critic_obs_type, [list(p.critic) for p in ln.module.policies])):
            x = (full if kind == "global" else local).contiguous()
            d = torch.randn(*x.shape[:2], nets[0][-1].out_features, device="cuda") / x.shape[0]
            xs, ds = [x[:, p].contiguous() for p in range(len(nets))], [d[:, p].contiguous() for p in range(len(nets))]
            jobs.append((nets, x, d, xs, ds))

        def single():
            for nets, _, _, xs, ds in jobs:
                for net, xp, dp in zip(nets, xs, ds):
                    M.mlp_backward(net, xp, dp)

        def multi():
            for nets, x, d, _, _ in jobs:
                M.multi_backward(nets, x, d)
        return {"bwd_single": single, "bwd_multi": multi}

    def loss_variants(self):
        """The loss with its backward alone, from the P policies' stacked outputs (leaves): P single-policy calls on
        each policy's contiguous slices, summed as the learner sums them, against one multi-policy call."""
        from marlsc.ppo_loss import fused_ppo_loss, fused_ppo_loss_multi
        ln = self.learners[MULTI]
        pols, rc = ln.module.policies, ln.module.rc
        with torch.no_grad():
            outs = [ln._forward(pol, self.obs, r) for pol, r in zip(pols, self.rows)]
            mean = torch.stack([o[0] for o in outs], dim=1)
            values = torch.stack([o[2] for o in outs], dim=1)
            log_std = torch.clamp(torch.stack([pol.log_std for pol in pols]), min=rc.logstd_floor)
        idx = torch.stack(list(self.rows), dim=1)
        P = len(pols)
        kl = [0.2] * P
        stacked = [t.detach().clone().requires_grad_() for t in (mean, log_std, values)]
        per = [[t.detach().clone().requires_grad_() for t in (mean[:, p], log_std[p], values[:, p])] for p in range(P)]
        rows = [r.contiguous() for r in self.rows]
        dev1, devP = torch.zeros((P, 5), dtype=torch.float64, device="cuda"), torch.zeros((P, 5), dtype=torch.float64, device="cuda")

        def single():
            total = None
            for p, (m_, l_, v_) in enumerate(per):
                loss = fused_ppo_loss(self.cfg, m_, l_, v_, self.flat, rows[p], kl[p], stats=dev1[p])[0]
                total = loss if total is None else total + loss
            total.backward()

        def multi():
            fused_ppo_loss_multi(self.cfg, *stacked, self.flat, idx, kl, stats=devP)[0].backward()
        return {"loss_single": single, "loss_multi": multi}

    def outputs(self):
        with torch.no_grad():
            ln = self.learners["step_torch"]
            mean, log_std, values = ln._forward(ln.module.policies[0], self.obs, self.rows[0])
        return [t.detach().clone().requires_grad_() for t in (mean, log_std[0], values)]

    def loss_torch(self, leaves):
        from marlsc.ppo import ppo_loss
        mean, ls, values = leaves
        b = {k: v[self.rows[0]] for k, v in self.flat.items()}
        ppo_loss(self.cfg, mean, ls.expand_as(mean), values, b, 0.2)[0].backward()

    def loss_fused(self, leaves):
        from marlsc.ppo_loss import fused_ppo_loss
        mean, ls, values = leaves
        fused_ppo_loss(self.cfg, mean, ls, values, self.flat, self.rows[0], 0.2, stats=self.dev_stats)[0].backward()


def _time(variants, rounds, warmup):
    times = {k: [] for k in variants}
    for _ in range(warmup):
        for fn in variants.values():
            fn()
    for _ in range(rounds):
        for k, fn in variants.items():
            torch.cuda.synchronize()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            e1.synchronize()
            times[k].append(e0.elapsed_time(e1) * 1e3)  # us
    return {k: np.asarray(v) for k, v in times.items()}


def _opt_lines(res, lines):
    """Every step variant over the same variant with the fused clip + Adam step, and whether the fused one's p95 is
    below the parent's p05 (the bar for turning the switch on by default)."""
    for base in ("step_torch", "step_fused", "step_fused_mlp"):
        k = base + "_opt"
        res[f"{base}_over_{k}"] = res[base]["median_us"] / res[k]["median_us"]
        clear = res[k]["p95_us"] < res[base]["p05_us"]
        res[f"{k}_p95_below_{base}_p05"] = bool(clear)
        lines.append(f"  {base} / {k} = {res[f'{base}_over_{k}']:.3f}   ({k} p95 {res[k]['p95_us']:.1f} "
                     f"{'<' if clear else '>='} {base} p05 {res[base]['p05_us']:.1f})")


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=100)
    ap.add_argument("--rounds-large", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--out", type=str, default=None)
    ap.add_argument("--count-launches", action="store_true",
                    help="run 10 torch steps, then 10 fused steps of the ippo networks at 800 rows and exit")
    ap.add_argument("--variant", type=str, default=None, help="with --count-launches: one per-agent variant instead")
    ap.add_argument("--steps", type=int, default=10, help="with --count-launches --variant: steps to run")
    ap.add_argument("--per-agent-only", action="store_true", help="skip the shared-policy rows")
    args = ap.parse_args()
    W, K, L = 8, 5, _local_obs_dim()
    if args.count_launches and args.variant:
        cfg, m, obs, batch = _setup("ippo", 8000, W, L, K, shared=False)
        st = Steps(cfg, m, obs, batch, [torch.randperm(8000, device="cuda")[:800] * W + w for w in range(W)], multi=True)
        fn = st.step_variants()[args.variant]
        for _ in range(args.steps):
            fn()
        torch.cuda.synchronize()
        return 0
    if args.count_launches:
        cfg, m, obs, batch = _setup("ippo", 8000, W, L, K)
        st = Steps(cfg, m, obs, batch, [torch.randperm(8000 * W, device="cuda")[:800]])
        for fn in (st.step_variants()[k] for k in ("step_torch", "step_fused")):
            for _ in range(10):
                fn()
            torch.cuda.synchronize()
        return 0
    lines = [f"device: {torch.cuda.get_device_name(0)}   warmup {args.warmup}, variants alternated, one step per sample, us",
             f"observation width {L} (C3, with the warehouse one-hot), K = {K}, {W} agents on one shared policy"]
    results = []
    for name in () if args.per_agent_only else ("ippo", "mappo"):
        for S, rows, rounds in ((8000, 800, args.rounds), (32768, 32768 * W, args.rounds_large)):
            cfg, m, obs, batch = _setup(name, S, W, L, K)
            st = Steps(cfg, m, obs, batch, [torch.randperm(S * W, device="cuda")[:rows]])
            leaves = st.outputs()
            t = _time(st.step_variants(), rounds, args.warmup)
            t.update(_time({"loss_torch": lambda: st.loss_torch(leaves), "loss_fused": lambda: st.loss_fused(leaves)},
                           rounds, args.warmup))
            t.update(_time({"opt_torch": st.opt_torch, "opt_fused": st.opt_fused}, rounds, args.warmup))
            res = {"config": name, "rows": rows, "rounds": rounds}
            lines.append(f"{name}.yaml networks, minibatch of {rows} rows (batch {S * W} rows), {rounds} rounds")
            for k, v in t.items():
                res[k] = {"median_us": float(np.median(v)), "p05_us": float(np.percentile(v, 5)),
                          "p95_us": float(np.percentile(v, 95)), "min_us": float(v.min()), "max_us": float(v.max())}
                lines.append(f"  {k:18s} median {res[k]['median_us']:9.1f}   p05 {res[k]['p05_us']:9.1f}   p95 "
                             f"{res[k]['p95_us']:9.1f}   range {res[k]['min_us']:.1f} .. {res[k]['max_us']:.1f}")
            for kind in ("step", "loss", "opt"):
                res[f"{kind}_torch_over_fused"] = res[f"{kind}_torch"]["median_us"] / res[f"{kind}_fused"]["median_us"]
                lines.append(f"  {kind}: torch / fused = {res[f'{kind}_torch_over_fused']:.3f}")
            for k, base in (("step_mlp", "step_torch"), ("step_fused_mlp", "step_fused"), ("step_fused_mlp", "step_torch")):
                res[f"{base}_over_{k}"] = res[base]["median_us"] / res[k]["median_us"]
                lines.append(f"  {base} / {k} = {res[f'{base}_over_{k}']:.3f}")
            _opt_lines(res, lines)
            results.append(res)
            del st, leaves, cfg, m, obs, batch
            torch.cuda.empty_cache()
    # per-agent policies, 800 rows each out of each agent's 8,000
    for name, W in (("ippo", 8), ("mappo", 8), ("ippo", 16)):
        cfg, m, obs, batch = _setup(name, 8000, W, L, K, shared=False)
        idx = [torch.randperm(8000, device="cuda")[:800] * W + w for w in range(W)]
        st = Steps(cfg, m, obs, batch, idx, multi=True)
        t = _time(st.step_variants(), args.rounds, args.warmup)
        t.update(_time({"opt_torch": st.opt_torch, "opt_fused": st.opt_fused}, args.rounds, args.warmup))
        t.update(_time(st.backward_variants(), args.rounds, args.warmup))
        t.update(_time(st.loss_variants(), args.rounds, args.warmup))
        res = {"config": f"{name} per-agent", "rows": 800, "policies": W, "rounds": args.rounds}
        lines.append(f"{name}.yaml networks, {W} per-agent policies, minibatches of 800 rows each, {args.rounds} rounds")
        for k, v in t.items():
            res[k] = {"median_us": float(np.median(v)), "p05_us": float(np.percentile(v, 5)),
                      "p95_us": float(np.percentile(v, 95)), "min_us": float(v.min()), "max_us": float(v.max())}
            lines.append(f"  {k:30s} median {res[k]['median_us']:9.1f}   p05 {res[k]['p05_us']:9.1f}   p95 "
                         f"{res[k]['p95_us']:9.1f}   range {res[k]['min_us']:.1f} .. {res[k]['max_us']:.1f}")
        for k, base in (("step_mlp", "step_torch"), ("step_fused_mlp", "step_fused"), ("step_fused_mlp", "step_torch")):
            res[f"{base}_over_{k}"] = res[base]["median_us"] / res[k]["median_us"]
            lines.append(f"  {base} / {k} = {res[f'{base}_over_{k}']:.3f}")
        res["opt_torch_over_fused"] = res["opt_torch"]["median_us"] / res["opt_fused"]["median_us"]
        lines.append(f"  opt: torch / fused = {res['opt_torch_over_fused']:.3f}")
        _opt_lines(res, lines)
        for k, base in ((MULTI, "step_fused_mlp_opt"), ("bwd_multi", "bwd_single"), (MULTI_LOSS, MULTI),
                        ("loss_multi", "loss_single")):
            res[f"{base}_over_{k}"] = res[base]["median_us"] / res[k]["median_us"]
            clear = res[k]["p95_us"] < res[base]["p05_us"]
            res[f"{k}_p95_below_{base}_p05"] = bool(clear)
            lines.append(f"  {base} / {k} = {res[f'{base}_over_{k}']:.3f}   ({k} p95 {res[k]['p95_us']:.1f} "
                         f"{'<' if clear else '>='} {base} p05 {res[base]['p05_us']:.1f})")
        results.append(res)
        del st, cfg, m, obs, batch
        torch.cuda.empty_cache()
    text = "\n".join(lines) + "\n"
    print(text)
    print(json.dumps(results))
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text(text)
    return 0


if __name__ == "__main__":
    sys.exit(main())
