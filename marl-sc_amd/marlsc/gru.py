"""Fused GRU-network inference step for the rollout (msc_gru_step, csrc/gru.hip).

The reference's `gru` architecture (src/algorithms/models/architectures/gru.py:14-85) is an
nn.ModuleDict {"gru": nn.GRU(batch_first), "output_proj": [act,] Linear [, act]} that
BaseRLModule._forward_gru (src/algorithms/models/rlmodules/base.py:99-141) steps on a [B, obs_dim]
input with the state [B, num_layers, hidden]. At rollout (inference, no autograd) one time step of the
whole network runs as ONE HIP kernel on the f32 MFMA for hidden sizes 64 / 128 / 256, one or two
layers, up to 1024 inputs and up to 32 outputs or a multiple of 32 up to 256 (`gru_tier` = 1);
anything else, autograd enabled, or CPU tensors run the torch layers with the same semantics
(`torch_step`). `pack_gru` builds the kernel's lane-major weight fragments, cached per weight version
on the network (biases included in the key: they are folded into the packed bias rows).
"""
from __future__ import annotations

import ctypes as C
import os
from typing import Optional, Tuple

import torch
import torch.nn as nn

from . import abi
from .mlp import _ACT_CODE, _IDX, _cached_pack, _rho

ENABLED = os.environ.get("MSC_FUSED_GRU", "1") != "0"


def proj_parts(op: nn.Module):
    """(act_pre, Linear, act_out) of an output_proj as GRUArchitecture builds it (a bare Linear, or a
    Sequential [act,] Linear [, act]); None when it is something else."""
    if isinstance(op, nn.Linear):
        return None, op, None
    mods = list(op) if isinstance(op, nn.Sequential) else None
    if not mods:
        return None
    k = [i for i, m in enumerate(mods) if isinstance(m, nn.Linear)]
    if len(k) != 1 or k[0] > 1 or len(mods) - k[0] > 2:
        return None
    return (mods[0] if k[0] == 1 else None), mods[k[0]], (mods[k[0] + 1] if k[0] + 1 < len(mods) else None)


def _dims(net) -> Optional[Tuple[int, int, int, int]]:
    """(in_dim, hidden, layers, out_dim) of a GRU network the step kernel's math covers, else None."""
    g, parts = net["gru"], proj_parts(net["output_proj"])
    if parts is None or not isinstance(g, nn.GRU) or g.bidirectional or not g.bias or getattr(g, "proj_size", 0):
        return None
    pre, lin, post = parts
    if type(pre) not in _ACT_CODE or type(post) not in _ACT_CODE or lin.bias is None or lin.in_features != g.hidden_size:
        return None
    return g.input_size, g.hidden_size, g.num_layers, lin.out_features


def gru_supported(in_dim: int, hidden: int, layers: int, out_dim: int) -> bool:
    """msc_gru_supported: whether the library has a fused step kernel for these sizes."""
    return bool(abi.lib().msc_gru_supported(int(in_dim), int(hidden), int(layers), int(out_dim)))


def gru_tier(net) -> int:
    """Inference path of a GRU network: 1 = one fused launch per step (gru_step_forward's kernel),
    3 = torch layers."""
    d = _dims(net)
    return 1 if d is not None and gru_supported(*d) else 3


def _index(kind: str, rows: int, cols: int, device):
    """Gather maps (flat index into the [rows, cols] matrix, validity) of the kernel's fragments.
    kind "x": [rows/32][M4][64][4], the lane halves split the columns (w1p of the fused MLP);
    kind "h": [ceil(rows/32)][cols/8][64][4], columns in accumulator order (w2p), rows past `rows` zero."""
    key = ("gru", kind, rows, cols, str(device))
    if key in _IDX:
        return _IDX[key]
    lane = torch.arange(64, device=device)
    c, h = (lane & 31)[None, None, :, None], (lane >> 5)[None, None, :, None]
    i4 = torch.arange(4, device=device)[None, None, None, :]
    nt = (rows + 31) // 32
    t = torch.arange(nt, device=device)[:, None, None, None]
    row = t * 32 + c
    if kind == "x":
        ks = (cols + 1) // 2
        m4 = (ks + 3) // 4
        m = torch.arange(m4, device=device)[None, :, None, None] * 4 + i4
        f = h * ks + m
        idx = row * cols + f.clamp(max=cols - 1)
        valid = ((f < cols) & (m < ks)).expand(nt, m4, 64, 4)
    else:
        s = torch.arange(cols // 8, device=device)[None, :, None, None] * 4 + i4
        idx = row.clamp(max=rows - 1) * cols + (s // 16) * 32 + _rho(s % 16, h)
        valid = (row < rows).expand(nt, cols // 8, 64, 4)
    _IDX[key] = (idx.reshape(-1), valid.reshape(-1))
    return _IDX[key]


def _gather(w: torch.Tensor, kind: str) -> torch.Tensor:
    idx, valid = _index(kind, w.shape[0], w.shape[1], w.device)
    flat = w.detach().float().reshape(-1)
    return torch.where(valid, flat[idx], torch.zeros((), device=w.device)).contiguous()


def pack_gru(net):
    """The fused step's weight set of a GRU network (include/marlsc.h: msc_gru_weights), as a tuple
    (wi_0, wh_0, b_0[, wi_1, wh_1, b_1], wo, bo) of contiguous f32 tensors."""
    g = net["gru"]
    _, lin, _ = proj_parts(net["output_proj"])
    H, out = g.hidden_size, []
    for l in range(g.num_layers):
        w_ih, w_hh = getattr(g, f"weight_ih_l{l}"), getattr(g, f"weight_hh_l{l}")
        b_ih, b_hh = getattr(g, f"bias_ih_l{l}").detach().float(), getattr(g, f"bias_hh_l{l}").detach().float()
        b = torch.cat([b_ih[:2 * H] + b_hh[:2 * H], b_ih[2 * H:], b_hh[2 * H:]]).contiguous()
        out += [_gather(w_ih, "x" if l == 0 else "h"), _gather(w_hh, "h"), b]
    out += [_gather(lin.weight, "h"), lin.bias.detach().float().contiguous()]
    return tuple(out)


def _weights(net):
    g = net["gru"]
    _, lin, _ = proj_parts(net["output_proj"])
    ws = []
    for l in range(g.num_layers):
        ws += [getattr(g, f"{n}_l{l}") for n in ("weight_ih", "weight_hh", "bias_ih", "bias_hh")]
    return tuple(ws) + (lin.weight, lin.bias)


def _reset_mask(reset: torch.Tensor, group: int, n: int) -> torch.Tensor:
    return (reset.reshape(-1) == 0).repeat_interleave(group)[:n]


def torch_step(net, x: torch.Tensor, h: torch.Tensor, reset: Optional[torch.Tensor] = None, group: int = 1):
    """One step through the torch layers: x [..., in], h [..., layers, hidden] -> (y [..., out],
    h' [..., layers, hidden]); rows whose group's reset flag is non-zero start from a zero state
    (selected, not multiplied: whatever their old state holds is not read, as in the kernel)."""
    g = net["gru"]
    lead = x.shape[:-1]
    xf = x.reshape(-1, x.shape[-1])
    hf = h.reshape(-1, g.num_layers, g.hidden_size)
    if reset is not None:  # a select, as the kernel's: a reset row never reads its old state (NaN / Inf included)
        zero = torch.zeros((), dtype=hf.dtype, device=hf.device)
        hf = torch.where(_reset_mask(reset, group, hf.shape[0])[:, None, None], hf, zero)
    o, hn = g(xf.unsqueeze(1), hf.transpose(0, 1).contiguous())
    y = net["output_proj"](o[:, 0])
    return y.reshape(*lead, -1), hn.transpose(0, 1).reshape(*lead, g.num_layers, g.hidden_size)


def gru_step_forward(net, x: torch.Tensor, h: torch.Tensor, reset: Optional[torch.Tensor] = None, group: int = 1,
                     *, store_state: bool = True, h_out: Optional[torch.Tensor] = None, y: Optional[torch.Tensor] = None):
    """One time step of a GRU network: x [..., in], h [..., layers, hidden] -> (y [..., out], h' or None).
    reset (uint8 [rows / group]): rows whose group's flag is non-zero read h as zero. store_state False:
    the new state is not produced (returns None for it). h_out / y: buffers the fused kernel writes into
    (h_out must not be h). Fused (gru_tier(net) == 1) for f32 CUDA tensors without autograd; the torch
    layers otherwise, with identical semantics."""
    if not (ENABLED and x.is_cuda and x.dtype == torch.float32 and not torch.is_grad_enabled() and gru_tier(net) == 1):
        yy, hn = torch_step(net, x, h, reset, group)
        if y is not None:
            yy = y.copy_(yy.reshape(y.shape))
        if not store_state:
            return yy, None
        if h_out is not None:
            hn = h_out.copy_(hn.reshape(h_out.shape))
        return yy, hn
    L, H, NL, KO = _dims(net)
    pre, lin, post = proj_parts(net["output_proj"])
    if x.shape[-1] != L:
        raise ValueError(f"input has {x.shape[-1]} features, the GRU expects {L}")
    lead = x.shape[:-1]
    xf = x.reshape(-1, L)
    if not xf.is_contiguous():
        xf = xf.contiguous()
    n = xf.shape[0]
    hf = h.reshape(-1, NL, H)
    if hf.dtype != torch.float32 or not hf.is_contiguous():
        hf = hf.float().contiguous()
    if hf.shape[0] != n:
        raise ValueError(f"state has {hf.shape[0]} rows, the input {n}")
    if reset is not None:
        if reset.dtype != torch.uint8 or not reset.is_contiguous() or not reset.is_cuda:
            raise ValueError("reset must be a contiguous uint8 CUDA tensor")
        if group < 1 or n % group or reset.numel() != n // group:
            raise ValueError(f"reset must hold {n // max(group, 1)} flags for {n} rows in groups of {group}")
    cur = torch.cuda.current_stream(x.device)
    packed = _cached_pack(net["gru"], "gru_step", _weights(net), cur, lambda: pack_gru(net))
    gw = abi.MscGruWeights()
    for l in range(NL):
        gw.wi[l], gw.wh[l], gw.b[l] = (t.data_ptr() for t in packed[3 * l:3 * l + 3])
    gw.wo, gw.bo = packed[-2].data_ptr(), packed[-1].data_ptr()
    for name, t, numel in (("y", y, n * KO), ("h_out", h_out, n * NL * H)):
        if t is not None and not (t.is_cuda and t.dtype == torch.float32 and t.is_contiguous() and t.numel() == numel):
            raise ValueError(f"{name} must be a contiguous float32 CUDA tensor of {numel} elements")
    if y is None:
        y = torch.empty((n, KO), device=x.device, dtype=torch.float32)
    if store_state and h_out is None:
        h_out = torch.empty((n, NL, H), device=x.device, dtype=torch.float32)
    vp = lambda t: None if t is None else C.c_void_p(t.data_ptr())  # noqa: E731
    abi.check(abi.lib().msc_gru_step(vp(xf), n, L, H, NL, KO, vp(hf), C.byref(gw), _ACT_CODE[type(pre)],
                                     _ACT_CODE[type(post)], vp(reset), int(group), vp(y),
                                     vp(h_out) if store_state else None, C.c_void_p(cur.cuda_stream)))
    return y.reshape(*lead, KO), (h_out.reshape(*lead, NL, H) if store_state else None)
