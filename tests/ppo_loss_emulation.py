"""Yardstick, error bound and input generator for the fused PPO loss kernel (csrc/ppo_loss.hip,
msc_ppo_loss). A helper, not a test: tests/test_ppo_loss_host.py and tests/test_gpu_ppo_loss.py use it.

Yardstick. marlsc/ppo.py:ppo_loss (unchanged, pinned by tests/test_ppo_host.py) run in float64 under
torch autograd on the float32 inputs cast up: its total, its five statistics and the .grad of mean,
log_std and values.

Bound. For every output element |got - yardstick| <= 2^-24 * W, W a weighted sum of the absolute
values of the terms that enter the element (the C * 2^-24 * M form with the constant C taken inside
the sum, because the terms of one element carry different operation counts). u = 2^-24 is the relative
error of one float32 + - * / (round to nearest, nothing contracted: the library is built with
-ffp-contract=off). expf: at most 1 ulp = 2 u. That is the limit HIP documents for its device expf
(HIP programming guide, math API, "expf: 1 ULP"); the ROCm tree this project builds against ships no
device-library accuracy document, so the figure is taken from there, as
tests/test_gpu_rollout_math.py already does. The chain, first order in u, per column k of a row
(D = 7 bounds the depth of the kernel's sum over columns: log2 of at most 64 lanes, plus one add for the
lane's second column when K > 64):
  std = expf(ls) 2u; var = std std 5u; d = a - m 1u; t = d d / (2 var) 3 + 5 + 1 = 9u
  -t - ls: 9u |t| + 1u (|t| + |ls|); the sum over k adds D u per term:   (10 + D)|t| + (1 + D)|ls|
  logp = sum - K c: K c carries 2u (the float32 constant, the product), the subtraction 1u |logp|:
      E_logp = sum_k [(11 + D)|t| + (2 + D)|ls|] + 3 K c,   c = log(2 pi) / 2
  lr = logp - logp_old: + 1u |lr|;  r = expf(lr): relative AMP = E_logp + |lr| + 2   (the ratio's
      amplification of the absolute error of logp - logp_old; about 3 K c u for small t, ls)
  A' = beta A 1u; s = A' r or A' bound (bound = float32(1 -+ clip), 1u): |surr| (AMP + 3)
  vf = (v - t)^2 3u, the clip bound 1u: 4 vfc
  ent = sum_k (ls + c'), c' = log(2 pi e) / 2 (1u as a float32 constant): E_ent = (1 + D) sum|ls + c'| + K c'
  u_k = (expf(2 ls0) + dm^2) / (2 expf(2 ls)): 2, (1, 3) -> 4, 2, 1 -> 7u; kl_k = ((ls - ls0) + u_k) - 1/2:
      E_kl = sum_k [3|ls - ls0| + 9 u_k + 1/2 + D |kl_k|]
  row loss (-surr + c_v vfc) - c_e ent: |surr| (AMP + 5) + 7 c_v vfc + c_e (E_ent + 4 (sum|ls| + K c'))
  total = mean(row) + kl_coeff mean(kl), rounded to float32: one more u on every term, and
      kl_coeff (float32) mean(kl): kl_coeff (E_kl + 3 (sum|ls - ls0| + sum u_k + K / 2))
  g = (-w / n) r: 1 / n 1u, w 1u, two products: |g| (AMP + 4)
  grad_mean = g d / var + gk kmu (gk = kl_coeff / n 3u, kmu = -dm / v1 4u):
      |g d / var| (AMP + 4 + 7 + 1 + 1) + |gk kmu| (3 + 4 + 1 + 1)
  grad_log_std = g (2t - 1) - c_e / n + gk (1 - 2 u_k): 2t - 1 within 10u (2t + 1), 1 - 2 u_k within
      8u (1 + 2 u_k): |g| (2t + 1) (AMP + 17) + 5 c_e / n + 14 gk (1 + 2 u_k); the shared row's [K] sum
      over rows is float64 and rounded once: + 1 on every coefficient
  grad_values = (c_v / n) 2 (v - t): 3 + 1 + 1 -> 6 |grad_values|
Terms of second order in u are covered by a factor 1.01 on every bound (AMP u < 1e-3 here). The
float64 sums over rows add errors of order 2^-53 and are not counted.

The bound holds only where kernel and yardstick are on the same side of every kink, so the generator
keeps the random rows a margin away from the clip bounds, and plants the rows that sit on a kink so that
both sides agree (below).

Generator (seeded). Ratios come from solving logp_old = logp64 - log(target) in float64 on the
float32 inputs; classes, cycled over the rows: inside the clip range, far below and far above it
(|logp - logp_old| in [0.5, 1.5]), and exactly at 1 - clip_param and 1 + clip_param. An at-bound row is
kept as such only if the float32 ratio, as torch computes it on the CPU, lands exactly on the float32
bound (logp_old and three float32 neighbours on each side are tried); a row that does not land becomes
an inside row, and `planted` says how many landed. About three in four land while |logp| < 8; none can
once |logp| >= 32 (K of about 35 and more), where logp - logp_old is a multiple of 2^-18 and the window
of arguments that expf maps onto the bound is 2^-23 wide and holds no such multiple for clip_param 0.2. On an at-bound row the advantage has the sign for which the surrogate's
gradient is the same on both sides of the bound (A < 0 at the upper bound, A > 0 at the lower one: the
unclipped term is the minimum outside the range), because a float64 yardstick of float32 inputs cannot
be made to land on the same side of a discontinuity; the discontinuous tie itself is pinned exactly
where it can be produced exactly (float64 rows in tests/test_ppo_loss_host.py, the ratio-1 /
clip_param-0 rows of tests/test_gpu_ppo_loss.py). Advantages: positive, negative and exactly 0. Value
errors: v - t in {1 (below), 2 (vf exactly vf_clip_param = 4), 3 (above)}, exact in float32 and float64.
The spread of actions and log_std is scaled down (0.6; 0.3 for K > 16) so that the amplification stays
small and the sums that can cancel (the shared row's gradient, the mean surrogate, the KL) do not, for
the bound to mean something (tests/test_ppo_loss_host.py holds it to 1e-4 of each output's largest
magnitude).
"""
from __future__ import annotations

import math
from types import SimpleNamespace
from typing import Dict, Optional

import numpy as np
import torch

U = 2.0 ** -24
DEPTH = 7
SLACK = 1.01
C_LOGP = 0.5 * math.log(2 * math.pi)
C_ENT = 0.5 * math.log(2 * math.pi * math.e)
KS = (1, 5, 8, 16, 17, 40, 64, 65, 128)
OUTPUTS = ("total", "stats", "grad_mean", "grad_log_std", "grad_values")
STAT_KEYS = ("total_loss", "policy_loss", "vf_loss", "entropy", "mean_kl")


def make_cfg(use_kl: bool = False, beta: Optional[float] = None, clip_param: float = 0.2, vf_clip_param: float = 4.0,
             vf_loss_coeff: float = 0.7, entropy_coeff: float = 0.004):
    """The fields ppo_loss and fused_ppo_loss read."""
    return SimpleNamespace(clip_param=clip_param, vf_clip_param=vf_clip_param, vf_loss_coeff=vf_loss_coeff,
                           entropy_coeff=entropy_coeff, use_kl_loss=use_kl, hysteretic_beta=beta)


def _logp64(a, m, ls):
    a, m, ls = (np.asarray(x, dtype=np.float64) for x in (a, m, ls))
    return (-((a - m) ** 2) / (2 * np.exp(ls) ** 2) - ls - C_LOGP).sum(-1)


def _ratio32(a, m, ls, lpo):
    """The float32 ratio as torch forms it on the CPU (gaussian_logp's chain)."""
    from marlsc.ppo import gaussian_logp
    T = lambda x: torch.from_numpy(np.ascontiguousarray(x, dtype=np.float32))  # noqa: E731
    return torch.exp(gaussian_logp(T(a), T(m), T(ls)) - T(lpo)).numpy()


def make_inputs(n: int, K: int, *, B: Optional[int] = None, shared: bool = False, cfg=None, seed: int = 0,
                idx=None) -> Dict:
    """Batch columns for B >= n rows, and the network outputs of the n rows the minibatch holds: those of
    batch rows idx (an int array of n entries in [0, B), repeats allowed), or of rows 0..n-1. The batch
    depends on (seed, B, K, shared) only, so calls that differ in idx share it."""
    cfg = cfg or make_cfg()
    B = n if B is None else B
    sel = np.arange(n) if idx is None else np.asarray(idx, dtype=np.int64)
    assert sel.shape == (n,) and sel.min() >= 0 and sel.max() < B
    g = np.random.default_rng([seed, B, K, int(shared)])
    f32 = np.float32
    sc = 0.6 if K <= 16 else 0.3  # below 1: E[2t - 1] = sc^2 - 1, the shared row's gradient does not cancel
    mean = g.normal(size=(B, K)).astype(f32)
    ls_row = (g.uniform(-0.5, 0.3, size=K) * sc).astype(f32)
    ls = np.broadcast_to(ls_row, (B, K)).copy() if shared else (g.uniform(-0.5, 0.3, size=(B, K)) * sc).astype(f32)
    actions = (mean + np.exp(ls) * g.normal(size=(B, K)) * sc).astype(f32)
    lo, hi = f32(1.0 - cfg.clip_param), f32(1.0 + cfg.clip_param)
    margin = 0.02
    cls = np.arange(B) % 5  # 0 inside, 1 far below, 2 far above, 3 at lo, 4 at hi
    target = np.empty(B)
    u = g.uniform(size=B)
    target[cls == 0] = (float(lo) + margin + u * (float(hi) - float(lo) - 2 * margin))[cls == 0]
    target[cls == 1] = np.exp(-(0.5 + u))[cls == 1]
    target[cls == 2] = np.exp(0.5 + u)[cls == 2]
    target[cls == 3], target[cls == 4] = float(lo), float(hi)
    lp64 = _logp64(actions, mean, ls)
    lpo = (lp64 - np.log(target)).astype(f32)
    at = cls >= 3
    bound = np.where(cls == 3, lo, hi).astype(f32)
    landed = np.zeros(B, dtype=bool)
    for step in (0, 1, -1, 2, -2, 3, -3):  # logp_old and its float32 neighbours
        c = lpo.copy()
        for _ in range(abs(step)):
            c = np.nextafter(c, f32(np.inf if step > 0 else -np.inf)).astype(f32)
        hit = at & ~landed & (_ratio32(actions, mean, ls, c) == bound)
        lpo[hit] = c[hit]
        landed |= hit
    lpo[at & ~landed] = (lp64 - np.log(target)).astype(f32)[at & ~landed]
    miss = at & ~landed  # not on the bound in float32: an inside row instead
    cls[miss] = 0
    lpo[miss] = (lp64 - np.log(float(lo) + margin + u * (float(hi) - float(lo) - 2 * margin)))[miss].astype(f32)
    r32 = _ratio32(actions, mean, ls, lpo)
    assert np.all((r32 == bound)[cls >= 3])
    planted = int((cls[sel] >= 3).sum())
    # advantages: the sign cycles against the ratio class (7 and 5 are coprime), every third-of-seven is 0
    k7 = np.arange(B) % 7
    adv = 2.0 * np.abs(g.normal(size=B)) + 0.2
    adv[k7 % 2 == 1] *= -0.1  # the negative ones smaller (they meet the large ratios unclipped): the sums over rows do not cancel
    adv[k7 == 6] = 0.0
    adv[(cls == 3) & (adv < 0)] *= -1.0  # the continuous side of each bound (see the module docstring)
    adv[(cls == 4) & (adv > 0)] *= -1.0
    adv = adv.astype(f32)
    vt = (g.integers(-256, 256, size=B) / 64.0).astype(f32)  # multiples of 1/64: v = t + dv is exact
    dv = np.array([1.0, 2.0, 3.0, -2.0, -1.0, -3.0], dtype=f32)[np.arange(B) % 6]
    values = (vt + dv).astype(f32)
    assert np.all((values - vt) == dv) and np.all(values.astype(np.float64) - vt.astype(np.float64) == dv)
    # the old distribution well away from the new one (kl = sum(..) - K / 2 cancels to nothing otherwise)
    # and narrower, so that the KL's gradient on log_std has the sign of the surrogate's over the rows
    mean_old = (mean + g.normal(size=(B, K)) * 0.3).astype(f32)
    ls_old = (ls - g.uniform(0.2, 0.5, size=(B, K))).astype(f32)
    return {"n": n, "K": K, "B": B, "shared": shared, "planted": planted, "cls": cls[sel], "dv": dv[sel], "idx": idx,
            "mean": mean[sel].copy(), "log_std": ls_row.copy() if shared else ls[sel].copy(), "values": values[sel].copy(),
            "batch": {"actions": actions, "logp": lpo, "advantages": adv, "value_targets": vt, "mean_old": mean_old,
                      "log_std_old": ls_old}}


def gather(inp: Dict) -> Dict[str, np.ndarray]:
    """The batch columns the n output rows pair with: rows idx, or rows 0..n-1."""
    sel = np.arange(inp["n"]) if inp["idx"] is None else np.asarray(inp["idx"])
    return {k: v[sel] for k, v in inp["batch"].items()}


def run_torch(cfg, inp: Dict, kl_coeff: float = 1.0, dtype=torch.float64, device="cpu") -> Dict:
    """ppo_loss under autograd in `dtype`: {'total', 'stats' [5], 'grad_mean', 'grad_log_std',
    'grad_values'} as float64 numpy. A shared log_std row is a [K] leaf expanded over the rows."""
    from marlsc.ppo import ppo_loss
    T = lambda x: torch.tensor(np.asarray(x), dtype=dtype, device=device)  # noqa: E731
    mean, values = T(inp["mean"]).requires_grad_(), T(inp["values"]).requires_grad_()
    ls = T(inp["log_std"]).requires_grad_()
    b = {k: T(v) for k, v in gather(inp).items()}
    total, st = ppo_loss(cfg, mean, ls.expand_as(mean) if inp["shared"] else ls, values, b, kl_coeff)
    total.backward()
    stats = [float(st[k].detach()) if k in st else 0.0 for k in STAT_KEYS]
    f = lambda t: t.detach().double().cpu().numpy()  # noqa: E731
    return {"total": np.array(float(total.detach())), "stats": np.array(stats), "grad_mean": f(mean.grad),
            "grad_log_std": f(ls.grad), "grad_values": f(values.grad)}


def bounds(cfg, inp: Dict, kl_coeff: float = 1.0) -> Dict[str, np.ndarray]:
    """The elementwise bound of every output (module docstring), from float64 values of the terms."""
    n, K, D = inp["n"], inp["K"], DEPTH
    b = {k: v.astype(np.float64) for k, v in gather(inp).items()}
    m, v = inp["mean"].astype(np.float64), inp["values"].astype(np.float64)
    ls = np.broadcast_to(inp["log_std"].astype(np.float64), (n, K))
    var = np.exp(ls) ** 2
    d = b["actions"] - m
    t = d * d / (2 * var)
    logp = (-t - ls - C_LOGP).sum(-1)
    lr = logp - b["logp"]
    amp = ((11 + D) * np.abs(t) + (2 + D) * np.abs(ls)).sum(-1) + 3 * K * C_LOGP + np.abs(lr) + 2
    r = np.exp(lr)
    A = b["advantages"].copy()
    if cfg.hysteretic_beta is not None and cfg.hysteretic_beta < 1.0:
        A = np.where(A >= 0, A, A * cfg.hysteretic_beta)
    lo, hi = 1.0 - cfg.clip_param, 1.0 + cfg.clip_param
    s1, s2 = A * r, A * np.clip(r, lo, hi)
    surr = np.minimum(s1, s2)
    inr = (r >= lo) & (r <= hi)
    w = np.where(s1 < s2, A, np.where(inr, A, 0.0))  # a planted row has the same w on both sides of its bound
    g = np.abs(w) / n * r
    dv = v - b["value_targets"]
    vf = dv * dv
    vfc = np.clip(vf, 0, cfg.vf_clip_param)
    sum_ls, ent_abs = np.abs(ls).sum(-1), np.abs(ls).sum(-1) + K * C_ENT
    e_ent = (1 + D) * np.abs(ls + C_ENT).sum(-1) + K * C_ENT
    c_v, c_e = cfg.vf_loss_coeff, cfg.entropy_coeff
    klc = float(kl_coeff) if cfg.use_kl_loss else 0.0
    if cfg.use_kl_loss:
        v1 = np.exp(2 * ls)
        dm = b["mean_old"] - m
        uk = (np.exp(2 * b["log_std_old"]) + dm * dm) / (2 * v1)
        dls0 = np.abs(ls - b["log_std_old"])
        e_kl = (3 * dls0 + 9 * uk + 0.5 + D * np.abs(ls - b["log_std_old"] + uk - 0.5)).sum(-1)
        kl_abs = (dls0 + uk).sum(-1) + 0.5 * K
        kmu = np.abs(dm / v1)
    else:
        uk, kmu = np.zeros((n, K)), np.zeros((n, K))
        e_kl = kl_abs = np.zeros(n)
    row = np.abs(surr) * (amp + 6) + 8 * c_v * vfc + c_e * (e_ent + 5 * ent_abs)
    total = row.mean() + klc * (e_kl + 4 * kl_abs).mean()
    stats = np.array([total, (np.abs(surr) * (amp + 4)).mean(), 5 * vfc.mean(), (e_ent + ent_abs).mean(),
                      (e_kl + kl_abs).mean()])
    gk = klc / n
    gm = (g * (amp + 13))[:, None] * np.abs(d / var) + 9 * gk * kmu
    gl = (g * (amp + 17))[:, None] * (2 * t + 1) + 5 * c_e / n + 14 * gk * (1 + 2 * uk) * (1.0 if cfg.use_kl_loss else 0.0)
    if inp["shared"]:
        gl = (gl + (g[:, None] * (2 * t + 1) + c_e / n + gk * (1 + 2 * uk))).sum(0)
    gv = 6 * np.where(vf <= cfg.vf_clip_param, c_v / n * 2 * np.abs(dv), 0.0)
    s = U * SLACK
    return {"total": np.array(total * s), "stats": stats * s, "grad_mean": gm * s, "grad_log_std": gl * s,
            "grad_values": gv * s}


def over_bound(got: Dict, ref: Dict, bnd: Dict) -> Dict[str, float]:
    """max |got - ref| / bound per output (0 / 0 counts as 0, x / 0 as inf)."""
    out = {}
    for k in OUTPUTS:
        e = np.abs(np.asarray(got[k], dtype=np.float64) - ref[k])
        with np.errstate(divide="ignore", invalid="ignore"):
            q = np.where(e == 0, 0.0, e / bnd[k])
        out[k] = float(np.max(q))
    return out


def vacuity(ref: Dict, bnd: Dict) -> Dict[str, float]:
    """max bound / max |output| per output array: how much the bound allows."""
    return {k: float(np.max(bnd[k]) / np.max(np.abs(ref[k]))) for k in OUTPUTS}
