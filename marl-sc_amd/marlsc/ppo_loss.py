"""The fused PPO loss (csrc/ppo_loss.hip, msc_ppo_loss): loss, statistics and the gradients with respect
to mean / log_std / values in one launch that gathers the minibatch rows itself, as a torch autograd
function. marlsc/ppo.py:ppo_loss stays the definition (and the tests' float64 yardstick); PPOLearner
takes this path with fused_loss=True or MSC_FUSED_LOSS=1 (opt-in)."""
from __future__ import annotations

import ctypes as C
import os
from typing import Dict, Optional, Tuple

import torch

from . import abi

STAT_KEYS = ("total_loss", "policy_loss", "vf_loss", "entropy", "mean_kl")  # the order of msc_ppo_loss's stats
MAX_K = 128


def fused_loss_default() -> bool:
    """MSC_FUSED_LOSS=1 turns the fused loss on where PPOLearner is built with fused_loss=None."""
    return os.environ.get("MSC_FUSED_LOSS", "0") == "1"


def workspace_bytes(n_rows: int, k: int) -> int:
    return int(abi.lib().msc_ppo_loss_workspace(int(n_rows), int(k)))


# The kernel's geometry, read off the library's own workspace query (one partial per block) so that nothing
# here restates csrc/ppo_loss.hip's constants.
def grid_blocks(n_rows: int, k: int) -> int:
    """Blocks the kernel launches for (n_rows, k): a function of the two alone, capped by the library."""
    return workspace_bytes(n_rows, k) // workspace_bytes(1, k)


def rows_per_block(k: int) -> int:
    """Rows one block covers per grid-stride step: the largest n that still takes one block."""
    r = 1
    while grid_blocks(2 * r, k) == 1:
        r *= 2
    while grid_blocks(r + 1, k) == 1:  # (a power of two today; this keeps the answer right if it is not)
        r += 1
    return r


_WORKSPACES: Dict[Tuple[int, int], torch.Tensor] = {}


def _workspace(device: torch.device, nbytes: int) -> torch.Tensor:
    """One workspace per (device, stream), grown on demand and kept for the life of the process (at most
    2,048 partials, 2.2 MB): calls on one stream are ordered, so the finalize kernel of a call has read the
    partials before the next call writes them. The key is the raw stream handle; a handle reused by a
    later stream after the first was destroyed finds the old tensor, which is still safe: whatever runs
    under that handle is ordered on it."""
    key = (device.index if device.index is not None else torch.cuda.current_device(),
           torch.cuda.current_stream(device).cuda_stream)
    w = _WORKSPACES.get(key)
    if w is None or w.numel() * 8 < nbytes:
        w = torch.empty(-(-nbytes // 8), dtype=torch.float64, device=device)
        _WORKSPACES[key] = w
    return w


def _desc(cfg, kl_coeff: float, shared: bool, accumulate: bool) -> abi.MscPpoLossDesc:
    beta = getattr(cfg, "hysteretic_beta", None)
    return abi.MscPpoLossDesc(float(cfg.clip_param), float(cfg.vf_clip_param), float(cfg.vf_loss_coeff),
                              float(cfg.entropy_coeff), float(kl_coeff), 1.0 if beta is None else float(beta),
                              1 if cfg.use_kl_loss else 0, 1 if shared else 0, 1 if accumulate else 0)


def _ptr(t: Optional[torch.Tensor]):
    return None if t is None else C.c_void_p(t.data_ptr())


def ppo_loss_launch(cfg, mean, log_std, values, flat_batch, idx, kl_coeff, stats=None):
    """One msc_ppo_loss call on raw tensors (no autograd): returns (total [1] f32, stats f64[5],
    grad_mean, grad_log_std, grad_values). Inputs must be CUDA, contiguous, f32 (idx int64); log_std
    [K] (shared row) or [n, K]. stats given: the call adds to it."""
    n, K = mean.shape
    shared = log_std.dim() == 1
    dev = mean.device
    grad_mean = torch.empty_like(mean)
    grad_ls = torch.empty_like(log_std)
    grad_values = torch.empty_like(values)
    total = torch.empty(1, dtype=torch.float32, device=dev)
    accumulate = stats is not None
    if stats is None:
        stats = torch.empty(5, dtype=torch.float64, device=dev)
    ws = _workspace(dev, workspace_bytes(n, K))
    use_kl = bool(cfg.use_kl_loss)
    d = _desc(cfg, kl_coeff, shared, accumulate)
    abi.check(abi.lib().msc_ppo_loss(
        C.byref(d), _ptr(mean), _ptr(log_std), _ptr(values), _ptr(idx), _ptr(flat_batch["actions"]),
        _ptr(flat_batch["logp"]), _ptr(flat_batch["advantages"]), _ptr(flat_batch["value_targets"]),
        _ptr(flat_batch["mean_old"]) if use_kl else None, _ptr(flat_batch["log_std_old"]) if use_kl else None,
        n, K, _ptr(grad_mean), _ptr(grad_ls), _ptr(grad_values), _ptr(total), _ptr(stats), _ptr(ws),
        C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)))
    return total, stats, grad_mean, grad_ls, grad_values


class _FusedPPOLoss(torch.autograd.Function):
    """total only: stats is written (or added to) by the launch, outside autograd."""

    @staticmethod
    def forward(ctx, mean, log_std, values, cfg, flat_batch, idx, kl_coeff, stats):
        total, _, gm, gl, gv = ppo_loss_launch(cfg, mean, log_std, values, flat_batch, idx, kl_coeff, stats)
        ctx.save_for_backward(gm, gl, gv)
        return total.reshape(())

    @staticmethod
    def backward(ctx, g_total):
        gm, gl, gv = torch._foreach_mul(list(ctx.saved_tensors), g_total)
        return gm, gl, gv, None, None, None, None, None


def _check(name: str, t: torch.Tensor, dtype=torch.float32) -> torch.Tensor:
    if not isinstance(t, torch.Tensor) or not t.is_cuda:
        raise RuntimeError(f"fused_ppo_loss: {name} must be a CUDA tensor (the fused loss is a HIP kernel; "
                           f"use ppo_loss on {getattr(t, 'device', type(t).__name__)})")
    if t.dtype != dtype:
        raise RuntimeError(f"fused_ppo_loss: {name} must be {dtype}, not {t.dtype}")
    return t


def fused_ppo_loss(cfg, mean: torch.Tensor, log_std: torch.Tensor, values: torch.Tensor,
                   flat_batch: Dict[str, torch.Tensor], idx: Optional[torch.Tensor], kl_coeff: float,
                   stats: Optional[torch.Tensor] = None):
    """ppo_loss(cfg, mean, log_std, values, {k: v[idx]}, kl_coeff) in one kernel launch, with autograd.

    mean [n, K], values [n] (or [n, 1]); log_std [K] (the shared row, clamped by the caller), [n, K], or
    an expanded [n, K] view with stride 0, which is taken as its shared row. flat_batch holds the whole
    batch's columns "actions" [B, K], "logp", "advantages", "value_targets" [B] (and "mean_old",
    "log_std_old" [B, K] with cfg.use_kl_loss); idx ([n] int64, or None for rows 0..n-1) selects the
    minibatch, repeats allowed, every index in [0, B) (the caller's contract, not checked).
    Returns (total, stats): total a 0-dim f32 tensor to call backward() on (the gradients were computed
    in the forward launch and are scaled by the incoming gradient), stats a device f64[5] in
    STAT_KEYS order, the minibatch means ppo_loss returns. With `stats` given (device f64[5]) the
    call adds to it and returns it, so a learner accumulates on the device and reads once.
    Raises RuntimeError for non-CUDA or non-float32 inputs."""
    _check("mean", mean), _check("log_std", log_std), _check("values", values)
    if mean.dim() != 2 or not (1 <= mean.shape[1] <= MAX_K) or mean.shape[0] < 1:
        raise RuntimeError(f"fused_ppo_loss: mean must be [n >= 1, 1 <= K <= {MAX_K}], not {tuple(mean.shape)}")
    n, K = mean.shape
    if log_std.dim() == 2 and log_std.shape == mean.shape and log_std.stride(0) == 0:
        log_std = log_std[0]  # an expanded shared row: autograd sums the [K] gradient back through the view
    if tuple(log_std.shape) not in ((K,), (n, K)):
        raise RuntimeError(f"fused_ppo_loss: log_std must be [{K}] or [{n}, {K}], not {tuple(log_std.shape)}")
    values = values.reshape(n)
    keys = ["actions", "logp", "advantages", "value_targets"] + (["mean_old", "log_std_old"] if cfg.use_kl_loss else [])
    cols = {k: _check(f"flat_batch['{k}']", flat_batch[k]).contiguous() for k in keys}
    B = cols["logp"].numel()
    if cols["actions"].shape != (B, K) or any(cols[k].numel() != B for k in ("advantages", "value_targets")):
        raise RuntimeError("fused_ppo_loss: flat_batch columns must be [B, K] / [B] over the same B rows")
    if idx is None:
        if B < n:
            raise RuntimeError(f"fused_ppo_loss: idx is None and the batch has {B} rows for {n} outputs")
    else:
        idx = _check("idx", idx, torch.int64).contiguous()
        if idx.numel() != n:
            raise RuntimeError(f"fused_ppo_loss: idx has {idx.numel()} entries for {n} rows")
    if stats is not None:
        _check("stats", stats, torch.float64)
        if stats.numel() != 5 or not stats.is_contiguous():
            raise RuntimeError("fused_ppo_loss: stats must be a contiguous f64[5]")
    if stats is None:  # a zeroed buffer the launch adds to: the same call form with and without `stats`
        stats = torch.zeros(5, dtype=torch.float64, device=mean.device)
    total = _FusedPPOLoss.apply(mean.contiguous(), log_std.contiguous(), values.contiguous(), cfg, cols, idx,
                                float(kl_coeff), stats)
    return total, stats


# -- P policies' losses in one call (msc_ppo_loss_multi): per policy bit for bit the single call --
MAX_POLICIES = 64  # the kernel arguments' kl_coeff capacity (mlp.MULTI_MAX_POLICIES)


def fused_multi_loss_default() -> bool:
    """MSC_FUSED_MULTI_LOSS=1 turns the multi-policy loss on where PPOLearner is built with
    fused_multi_loss=None."""
    return os.environ.get("MSC_FUSED_MULTI_LOSS", "0") == "1"


def multi_workspace_bytes(n_rows: int, n_policies: int, k: int) -> int:
    return int(abi.lib().msc_ppo_loss_multi_workspace(int(n_rows), int(n_policies), int(k)))


def multi_ppo_loss_launch(cfg, mean, log_std, values, flat_batch, idx, kl_coeffs, stats=None):
    """One msc_ppo_loss_multi call on raw tensors (no autograd): returns (totals [P] f32, stats f64[P, 5],
    grad_mean, grad_log_std, grad_values). Inputs must be CUDA, contiguous, f32: mean [n, P, K], values
    [n, P], log_std [P, K] (one shared row per policy) or [n, P, K]; idx [n, P] int64 or None (row i P + p);
    kl_coeffs P host floats. stats given: the call adds to it."""
    n, P, K = mean.shape
    shared = log_std.dim() == 2
    dev = mean.device
    grad_mean = torch.empty_like(mean)
    grad_ls = torch.empty_like(log_std)
    grad_values = torch.empty_like(values)
    totals = torch.empty(P, dtype=torch.float32, device=dev)
    accumulate = stats is not None
    if stats is None:
        stats = torch.empty((P, 5), dtype=torch.float64, device=dev)
    ws = _workspace(dev, multi_workspace_bytes(n, P, K))
    use_kl = bool(cfg.use_kl_loss)
    d = _desc(cfg, 0.0, shared, accumulate)
    kl = (C.c_double * P)(*[float(x) for x in kl_coeffs]) if use_kl else None
    abi.check(abi.lib().msc_ppo_loss_multi(
        C.byref(d), kl, _ptr(mean), _ptr(log_std), _ptr(values), _ptr(idx), _ptr(flat_batch["actions"]),
        _ptr(flat_batch["logp"]), _ptr(flat_batch["advantages"]), _ptr(flat_batch["value_targets"]),
        _ptr(flat_batch["mean_old"]) if use_kl else None, _ptr(flat_batch["log_std_old"]) if use_kl else None,
        n, P, K, _ptr(grad_mean), _ptr(grad_ls), _ptr(grad_values), _ptr(totals), _ptr(stats), _ptr(ws),
        C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)))
    return totals, stats, grad_mean, grad_ls, grad_values


class _FusedPPOLossMulti(torch.autograd.Function):
    """The sum of the P totals: every policy's loss gets the incoming gradient, as in a sum of P single calls."""

    @staticmethod
    def forward(ctx, mean, log_std, values, cfg, flat_batch, idx, kl_coeffs, stats):
        totals, _, gm, gl, gv = multi_ppo_loss_launch(cfg, mean, log_std, values, flat_batch, idx, kl_coeffs, stats)
        ctx.save_for_backward(gm, gl, gv)
        return totals.sum()

    @staticmethod
    def backward(ctx, g_total):
        gm, gl, gv = torch._foreach_mul(list(ctx.saved_tensors), g_total)
        return gm, gl, gv, None, None, None, None, None


def fused_ppo_loss_multi(cfg, mean: torch.Tensor, log_std: torch.Tensor, values: torch.Tensor,
                         flat_batch: Dict[str, torch.Tensor], idx: Optional[torch.Tensor], kl_coeffs,
                         stats: Optional[torch.Tensor] = None):
    """sum_p fused_ppo_loss(cfg, mean[:, p], log_std[p] or [:, p], values[:, p], flat_batch, idx[:, p],
    kl_coeffs[p]) in one msc_ppo_loss_multi call (two launches), with autograd; per policy bit for bit that call.

    mean [n, P, K], values [n, P] (or [n, P, 1]); log_std [P, K] (one shared row per policy, clamped by the
    caller) or [n, P, K]. flat_batch: the columns fused_ppo_loss reads, one set for all policies; idx
    ([n, P] int64; None: policy p's i-th sample is batch row i P + p) selects every policy's rows, repeats and
    rows common to several policies allowed, every index in [0, B) (the caller's contract, not checked).
    kl_coeffs: P host floats (ignored without cfg.use_kl_loss).
    Returns (total, stats): total a 0-dim f32 tensor, the sum of the P totals, to call backward() on; stats a
    device f64[P, 5], per policy in STAT_KEYS order. With `stats` given (contiguous device f64[P, 5]) the call
    adds to it and returns it. Raises RuntimeError for non-CUDA or non-float32 inputs and wrong shapes."""
    name = "fused_ppo_loss_multi"
    _check("mean", mean), _check("log_std", log_std), _check("values", values)
    if mean.dim() != 3 or mean.shape[0] < 1 or not (1 <= mean.shape[1] <= MAX_POLICIES) \
            or not (1 <= mean.shape[2] <= MAX_K):
        raise RuntimeError(f"{name}: mean must be [n >= 1, 1 <= P <= {MAX_POLICIES}, 1 <= K <= {MAX_K}], "
                           f"not {tuple(mean.shape)}")
    n, P, K = mean.shape
    if tuple(log_std.shape) not in ((P, K), (n, P, K)):
        raise RuntimeError(f"{name}: log_std must be [{P}, {K}] or [{n}, {P}, {K}], not {tuple(log_std.shape)}")
    if values.numel() != n * P:
        raise RuntimeError(f"{name}: values must be [{n}, {P}], not {tuple(values.shape)}")
    values = values.reshape(n, P)
    if len(kl_coeffs) != P:
        raise RuntimeError(f"{name}: {len(kl_coeffs)} kl_coeffs for {P} policies")
    keys = ["actions", "logp", "advantages", "value_targets"] + (["mean_old", "log_std_old"] if cfg.use_kl_loss else [])
    cols = {k: _check(f"flat_batch['{k}']", flat_batch[k]).contiguous() for k in keys}
    B = cols["logp"].numel()
    if cols["actions"].shape != (B, K) or any(cols[k].numel() != B for k in ("advantages", "value_targets")):
        raise RuntimeError(f"{name}: flat_batch columns must be [B, K] / [B] over the same B rows")
    if idx is None:
        if B < n * P:
            raise RuntimeError(f"{name}: idx is None and the batch has {B} rows for {n} x {P} outputs")
    else:
        idx = _check("idx", idx, torch.int64).contiguous()
        if tuple(idx.shape) != (n, P):
            raise RuntimeError(f"{name}: idx must be [{n}, {P}], not {tuple(idx.shape)}")
    if stats is not None:
        _check("stats", stats, torch.float64)
        if tuple(stats.shape) != (P, 5) or not stats.is_contiguous():
            raise RuntimeError(f"{name}: stats must be a contiguous f64[{P}, 5]")
    if stats is None:
        stats = torch.zeros((P, 5), dtype=torch.float64, device=mean.device)
    total = _FusedPPOLossMulti.apply(mean.contiguous(), log_std.contiguous(), values.contiguous(), cfg, cols, idx,
                                     [float(x) for x in kl_coeffs], stats)
    return total, stats
