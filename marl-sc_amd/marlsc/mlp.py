"""Fused policy-MLP inference for the rollout (msc_mlp3_relu_forward / msc_mlp2_relu_forward,
csrc/mlp.hip).

The reference's actor / critic networks are `MLPArchitecture.build` MLPs
(src/algorithms/models/architectures/mlp.py:14-60): Linear -> ReLU per hidden size, then an output
Linear. At rollout (inference, no autograd) the ReLU MLPs of the reference's algorithm configs run
as ONE HIP kernel on the f32 MFMA with the hidden activations in registers:
* two hidden layers [H1, H2], H1, H2 in {64, 128, 256, 512} (MAPPO actor [256, 256] and critic
  [64, 64], config_files/algorithms/mappo.yaml; the test configs' [256, 256] actors);
* one hidden layer [H], H a multiple of 32 up to 1024 (IPPO actor and critic [256],
  config_files/algorithms/ippo.yaml; the test configs' [128] and [1024] critics).
The kernels stream the weights in a lane-major fragment order; `pack_mlp3` builds it from the
torch [out, in] matrices (index maps cached per shape, packs cached per weight version, so the
learner's updates are picked up and the pack is rebuilt at most once per optimizer step). A pack
built on one HIP stream and used on another is ordered by an event (rollout lanes).

Actors with the reference's mu/sigma head (`use_mu_sigma_head`) run through the same kernels with a
dual-head output layer (msc_mlp{2,3}_relu_musigma, csrc/mlp_musigma.hip), and networks with 33..128
outputs (the centralised CPPO actor) have a multi-tile output layer with its own sampling epilogue
(msc_mlp{2,3}_relu_wide, csrc/mlp_wide.hip): see the sections at the end of this file.

With one policy per agent (parameter_sharing: false) the W same-shaped actors, and the W critics, run as
one launch each over the rows [..., W, L] (msc_mlp{2,3}_relu_multi, csrc/mlp_multi.hip; multi_forward at
the end of this file; opt-in, MSC_MULTI_MLP=1).

The plain MLPs can also be trained through the kernels (train_forward: the inference kernel forward, one
msc_mlp_relu_backward call backward, csrc/mlp_backward.hip; opt-in, MSC_FUSED_MLP_GRAD=1), and the P networks of
per-agent policies through one call each way (multi_train_forward: multi_forward forward, one
msc_mlp_relu_backward_multi call backward; opt-in, MSC_FUSED_MULTI_GRAD=1): the last two sections.

There is no CPU fallback: a CUDA tensor on a build without libmarlsc raises (abi.lib()).
"""
from __future__ import annotations

import ctypes as C
import os
from typing import Dict, Optional, Tuple

import torch
import torch.nn as nn

from . import abi

HIDDEN_SIZES = (64, 128, 256, 512)  # two-hidden-layer form
MAX_HIDDEN_1 = 1024                  # one-hidden-layer form: multiples of 32 up to this
MAX_OUT = 32
MAX_IN = 1024
ENABLED = os.environ.get("MSC_FUSED_MLP3", "1") != "0"

_IDX: Dict[Tuple, Tuple[torch.Tensor, ...]] = {}


def _rho(r: torch.Tensor, h: torch.Tensor) -> torch.Tensor:
    """Row of register r in lane half h of a 32x32 f32 MFMA accumulator."""
    return (r & 3) + 8 * (r >> 2) + 4 * h


def _index_maps(L: int, H1: int, H2: int, KO: int, device, w3_layout: int) -> Tuple[torch.Tensor, ...]:
    """H2 = 0: the one-hidden-layer form (no w2; the output layer reads H1)."""
    key = (L, H1, H2, KO, str(device), w3_layout)
    if key in _IDX:
        return _IDX[key]
    KS1 = (L + 1) // 2
    M4 = (KS1 + 3) // 4
    lane = torch.arange(64, device=device)
    c, h = lane & 31, lane >> 5
    # w1p[t][m4][lane][i] = W1[32 t + c][h KS1 + m], m = 4 m4 + i  (0 for m >= KS1 or past in_dim)
    t = torch.arange(H1 // 32, device=device)[:, None, None, None]
    m = torch.arange(M4, device=device)[None, :, None, None] * 4 + torch.arange(4, device=device)[None, None, None, :]
    f = h[None, None, :, None] * KS1 + m
    i1 = ((t * 32 + c[None, None, :, None]) * L + f.clamp(max=L - 1)).reshape(-1)
    v1 = ((f < L) & (m < KS1)).expand(H1 // 32, M4, 64, 4).reshape(-1)
    # w2p[t2][s4][lane][i] = W2[32 t2 + c][32 t1 + rho(r, h)], s = 4 s4 + i = 16 t1 + r
    i2 = None
    if H2:
        S = (H1 // 32) * 16
        t2 = torch.arange(H2 // 32, device=device)[:, None, None, None]
        s = (torch.arange(S // 4, device=device)[None, :, None, None] * 4 + torch.arange(4, device=device)[None, None, None, :])
        hh = h[None, None, :, None]
        cc = c[None, None, :, None]
        i2 = ((t2 * 32 + cc) * H1 + (s // 16) * 32 + _rho(s % 16, hh)).reshape(-1)
    H2 = H2 or H1  # the output layer reads the last hidden layer
    if w3_layout == 0:
        # w3p[q][lane][i] = W3[c][32 (q // 4) + rho(4 (q % 4) + i, h)]  (0 for output rows >= KO)
        q = torch.arange((H2 // 32) * 4, device=device)[:, None, None]
        r = (q % 4) * 4 + torch.arange(4, device=device)[None, None, :]
        c3, h3 = c[None, :, None], h[None, :, None]
        i3 = (c3.clamp(max=KO - 1) * H2 + (q // 4) * 32 + _rho(r, h3)).reshape(-1)
        v3 = (c3 < KO).expand((H2 // 32) * 4, 64, 4).reshape(-1)
    else:
        # VALU output layer: w3p[s][h][a] = W3[a][32 (s // 16) + rho(s % 16, h)]  (0 for a >= KO)
        sv = torch.arange((H2 // 32) * 16, device=device)[:, None, None]
        hv = torch.arange(2, device=device)[None, :, None]
        av = torch.arange(8, device=device)[None, None, :]
        i3 = (av.clamp(max=KO - 1) * H2 + (sv // 16) * 32 + _rho(sv % 16, hv)).reshape(-1)
        v3 = (av < KO).expand((H2 // 32) * 16, 2, 8).reshape(-1)
    _IDX[key] = (i1, v1, i2, i3, v3)
    return _IDX[key]


def w3_layout(out_dim: int) -> int:
    """Packed layout of the output layer the kernel uses for out_dim outputs (msc_mlp3_w3_layout):
    0 = MFMA fragments [H2/8][64][4], 1 = VALU rows [H2/2][2][8]."""
    v = abi.lib().msc_mlp3_w3_layout(int(out_dim))
    if v < 0:
        raise ValueError(f"the fused MLP supports 1..{MAX_OUT} outputs, not {out_dim}")
    return v


PLAN_FAMILIES = {"relu": 0, "multi": 1, "musigma": 2, "wide": 3}  # MSC_MLP_*
# msc_mlp_plan's list (include/marlsc.h)
PLAN_KEYS = ("supported", "nt1", "nt2", "p", "wpe", "il", "width", "tb", "lds_bytes", "grid_blocks")


def plan(family: str, hidden1: int, hidden2: int, out_dim: int, n_rows: int, n_policies: int = 1) -> Dict[str, int]:
    """The kernel instantiation and launch geometry a family's entry points would pick under the current
    knobs (msc_mlp_plan): host code only, no GPU is touched. hidden2 = 0: one hidden layer; out_dim: k for
    "musigma"; n_policies: "multi" only."""
    buf = (C.c_int32 * len(PLAN_KEYS))()
    n = abi.lib().msc_mlp_plan(PLAN_FAMILIES[family], int(hidden1), int(hidden2), int(out_dim), int(n_rows),
                               int(n_policies), buf, len(PLAN_KEYS))
    if n < 0:
        abi.check(n)
    return dict(zip(PLAN_KEYS, buf))


def pack_mlp3(w1: torch.Tensor, w2: Optional[torch.Tensor], w3: torch.Tensor, layout: Optional[int] = None):
    """Torch Linear weights ([H1, L], [H2, H1], [KO, H2]) -> (w1p, w2p, w3p) fragment order;
    w2 None: the one-hidden-layer form ([H1, L], [KO, H1] -> (w1p, None, w3p)).
    layout: the output layer's (w3_layout(KO) when None)."""
    H1, L = w1.shape
    H2, KO = (w2.shape[0] if w2 is not None else 0), w3.shape[0]
    i1, v1, i2, i3, v3 = _index_maps(L, H1, H2, KO, w1.device, w3_layout(KO) if layout is None else layout)
    zero = torch.zeros((), device=w1.device, dtype=torch.float32)
    w1p = torch.where(v1, w1.detach().float().reshape(-1)[i1], zero)
    w2p = w2.detach().float().reshape(-1)[i2].contiguous() if w2 is not None else None
    w3p = torch.where(v3, w3.detach().float().reshape(-1)[i3], zero)
    return w1p.contiguous(), w2p, w3p.contiguous()


def pack_w2t(w2: torch.Tensor) -> torch.Tensor:
    """Torch Linear weight [H2, H1] -> the pack of its transpose for msc_mlp_relu_backward's dgrad pass
    d1 = W2^T d2: pack_mlp3's layer-2 index map (the `i2` of _index_maps) on the [H1, H2] matrix W2^T, i.e.
    w2tp[t1][s4][lane][i] = W2[32 t2 + rho(r, h)][32 t1 + c], 4 s4 + i = 16 t2 + r."""
    H2, H1 = w2.shape
    i2 = _index_maps(1, H2, H1, 1, w2.device, 0)[2]  # (layer 1 and the output layer of the key are not used)
    return w2.detach().float().t().contiguous().reshape(-1)[i2].contiguous()


def fused_layers(mods, max_out: int = MAX_OUT) -> int:
    """2 or 3 when mods (Linear, ReLU, ..., Linear) has a fused kernel: one hidden layer of a
    multiple of 32 up to 1024 units, or two of {64, 128, 256, 512}; <= 1024 inputs, <= 32 outputs
    (max_out: the bound on the last Linear, wider for a backbone whose last Linear is folded into
    the mu/sigma head). 0 otherwise (the caller runs the torch layers)."""
    n = len(mods)
    if n not in (3, 5):
        return 0
    lins, acts = mods[0::2], mods[1::2]
    if not all(isinstance(m, nn.Linear) and m.bias is not None for m in lins):
        return 0
    if not all(isinstance(a, nn.ReLU) for a in acts):
        return 0
    for a, b in zip(lins[:-1], lins[1:]):
        if b.in_features != a.out_features:
            return 0
    if lins[0].in_features > MAX_IN or lins[-1].out_features > max_out:
        return 0
    if n == 3:
        H = lins[0].out_features
        return 2 if (H % 32 == 0 and 32 <= H <= MAX_HIDDEN_1) else 0
    return 3 if (lins[0].out_features in HIDDEN_SIZES and lins[1].out_features in HIDDEN_SIZES) else 0


def fusable(mods) -> bool:
    return fused_layers(mods) > 0


class _Pack:
    __slots__ = ("key", "tensors", "stream", "event")

    def __init__(self):
        self.key, self.tensors, self.stream, self.event = None, None, None, None

    def __deepcopy__(self, memo):  # a copied module packs its own weights (streams / events do not copy)
        return _Pack()


def _cached_pack(l1: nn.Module, slot, weights, cur, build):
    """A pack cached on the first Linear under `slot`: rebuilt by build() when any of `weights` changed
    (version counters) or moved. cur: the stream the pack is used on (a pack built on another stream is
    ordered after its packing kernels); None: on the host, nothing to order."""
    packs = getattr(l1, "_msc_packs", None)
    if packs is None:
        packs = l1._msc_packs = {}
    pk = packs.setdefault(slot, _Pack())
    key = tuple((p.data_ptr(), p._version) for p in weights)
    if pk.key != key:
        pk.tensors = build()
        pk.key = key
        pk.stream = cur
        if cur is not None:
            pk.event = torch.cuda.Event()
            pk.event.record(cur)
    elif pk.stream != cur and cur is not None:
        # packed on another stream (e.g. the main stream of a multi-lane rollout): order this
        # stream after the packing kernels, and keep the pack's memory alive for this stream's use
        cur.wait_event(pk.event)
        for t in pk.tensors:
            if t is not None:
                t.record_stream(cur)
    return pk.tensors


def sample_fusable(mods) -> bool:
    """True when the fused kernel for mods can also sample the actions (VALU output layer)."""
    return fused_layers(mods) > 0 and w3_layout(mods[-1].out_features) == 1


def _pre1_rows(pre1: torch.Tensor, n: int, group: int, H1: int) -> torch.Tensor:
    """pre1 as the kernels read it: f32 [n / group, H1]."""
    pre1 = pre1.float().contiguous()
    if group < 1 or n % group or pre1.shape != (n // group, H1):
        raise ValueError(f"pre1 must be [{n // max(group, 1)}, {H1}] for {n} rows in groups of {group}")
    return pre1


def _vp(t):
    return None if t is None else C.c_void_p(t.data_ptr())


def _gaussian_epilogue(sample, n: int, KO: int, n_policies: Optional[int] = None):
    """MscGaussianEpilogue of sample = (log_std [rows, KO], logstd_floor, eps, actions, logp, clipped) for n
    rows of KO outputs; n_policies: log_std has one row, or one per policy."""
    ls, floor, eps, act, logp, clipped = sample
    for t in (ls, eps, act, logp, clipped):
        if not (t.is_cuda and t.dtype == torch.float32 and t.is_contiguous()):
            raise ValueError("sampling buffers must be contiguous float32 CUDA tensors")
    if eps.numel() != n * KO or act.numel() != n * KO or clipped.numel() != n * KO or logp.numel() != n \
            or ls.dim() != 2 or ls.shape[1] != KO or (n_policies is not None and ls.shape[0] not in (1, n_policies)):
        raise ValueError("sampling buffers do not match the MLP's rows / outputs" if n_policies is None else
                         "sampling buffers do not match the MLPs' rows / outputs / policies")
    return abi.MscGaussianEpilogue(_vp(ls), int(ls.shape[0]), C.c_float(floor), _vp(eps), _vp(act), _vp(logp), _vp(clipped))


def mlp3_forward(mods, x: torch.Tensor, out: Optional[torch.Tensor] = None, *, w1: Optional[torch.Tensor] = None,
                 pre1: Optional[torch.Tensor] = None, group: int = 1, sample=None) -> torch.Tensor:
    """The fused kernel over x [..., L] (f32 CUDA) -> [..., KO]; mods as accepted by fusable()
    (Linear-ReLU-Linear-ReLU-Linear or Linear-ReLU-Linear).
    w1: a first-layer weight to use instead of mods[0].weight (e.g. its local-feature columns);
    pre1 [rows / group, H1]: added to the first layer's pre-activation of row n as pre1[n // group].
    sample: (log_std [P, KO], logstd_floor, eps, actions, logp, clipped) -- msc_gaussian_sample fused
    into the kernel's epilogue (sample_fusable(mods) must hold); the means then go to `out` only when
    it is given (returns `out`, possibly None)."""
    nl = fused_layers(mods)
    if nl == 0:
        raise ValueError("no fused kernel for this layer sequence (see fused_layers)")
    l1, l3 = mods[0], mods[-1]
    l2 = mods[2] if nl == 3 else None
    w1 = l1.weight if w1 is None else w1
    L, KO = w1.shape[1], l3.out_features
    if x.shape[-1] != L:
        raise ValueError(f"input has {x.shape[-1]} features, the MLP expects {L}")
    # pack cache on the first Linear (one per first-layer weight view): rebuilt when any weight
    # changes (version counters) or moves
    weights = (w1, l3.weight) if l2 is None else (w1, l2.weight, l3.weight)
    cur = torch.cuda.current_stream(x.device)
    w1p, w2p, w3p = _cached_pack(l1, (w1.shape, w1.stride(), w1.storage_offset()), weights, cur,
                                 lambda: pack_mlp3(w1, None if l2 is None else l2.weight, l3.weight))
    lead, xf = x.shape[:-1], _rows(x, L)
    n = xf.shape[0]
    if pre1 is not None:
        pre1 = _pre1_rows(pre1, n, group, l1.out_features)
    st = C.c_void_p(cur.cuda_stream)
    b1, b3 = (m.bias.detach().float().contiguous() for m in (l1, l3))
    if sample is not None:
        ep = _gaussian_epilogue(sample, n, KO)
        if l2 is None:
            abi.check(abi.lib().msc_mlp2_relu_forward_sampled(_vp(xf), n, L, l1.out_features, KO, _vp(w1p), _vp(b1), _vp(w3p),
                                                              _vp(b3), _vp(out), _vp(pre1), int(group), C.byref(ep), st))
        else:
            b2 = l2.bias.detach().float().contiguous()
            abi.check(abi.lib().msc_mlp3_relu_forward_sampled(_vp(xf), n, L, l1.out_features, l2.out_features, KO,
                                                              _vp(w1p), _vp(b1), _vp(w2p), _vp(b2), _vp(w3p), _vp(b3), _vp(out),
                                                              _vp(pre1), int(group), C.byref(ep), st))
        return None if out is None else out.reshape(*lead, KO)
    if out is None:
        out = torch.empty((n, KO), device=x.device, dtype=torch.float32)
    if l2 is None:
        abi.check(abi.lib().msc_mlp2_relu_forward(_vp(xf), n, L, l1.out_features, KO, _vp(w1p), _vp(b1), _vp(w3p), _vp(b3),
                                                  _vp(out), _vp(pre1), int(group), st))
    else:
        b2 = l2.bias.detach().float().contiguous()
        abi.check(abi.lib().msc_mlp3_relu_forward(_vp(xf), n, L, l1.out_features, l2.out_features, KO, _vp(w1p), _vp(b1),
                                                  _vp(w2p), _vp(b2), _vp(w3p), _vp(b3), _vp(out), _vp(pre1), int(group), st))
    return out.reshape(*lead, KO)


# ----------------------------------------------------------------------------------------------
# mu/sigma-head actors (use_mu_sigma_head): backbone Linear-ReLU(-Linear-ReLU)-Linear, then two
# Linear heads with no nonlinearity in between. For inference the backbone's last Linear is folded
# into the heads: W_eff = [W_mu; W_sigma] W_out ([2K, H]), b_eff = [W_mu; W_sigma] b_out +
# [b_mu; b_sigma], computed in f64 and rounded once to f32, so a head actor costs the MFMA work of
# a plain actor with 2K outputs.
# ----------------------------------------------------------------------------------------------
HEAD_MAX_FUSED = 8     # K of msc_mlp{2,3}_relu_musigma (VALU dual-head output layer)
HEAD_MAX_FOLDED = 16   # 2K <= 32: the plain fused MLP on the folded weights (MFMA output layer)
_ACT_CODE = {type(None): 0, nn.ReLU: 1, nn.Tanh: 2, nn.ELU: 3, nn.GELU: 4, nn.Sigmoid: 5}  # MSC_ACT_*


def fold_head(out_lin: nn.Linear, head):
    """(W_eff [2K, H], b_eff [2K]) f32: `out_lin` folded into head.mu_head / head.sigma_head."""
    wh = torch.cat([head.mu_head.weight, head.sigma_head.weight]).detach().double()
    bh = torch.cat([head.mu_head.bias, head.sigma_head.bias]).detach().double()
    w = wh @ out_lin.weight.detach().double()
    b = wh @ out_lin.bias.detach().double() + bh
    return w.float().contiguous(), b.float().contiguous()


def musigma_layout(H1: int, H2: int, K: int):
    """msc_mlp_musigma_layout: (per-head width, floats per (hidden pair, lane half)) of the packed
    dual-head weights for hidden sizes [H1, H2] (H2 = 0: one hidden layer) and K actions; None when
    the library has no fused head kernel for them."""
    w, s = C.c_int32(0), C.c_int32(0)
    if abi.lib().msc_mlp_musigma_layout(int(H1), int(H2), int(K), C.byref(w), C.byref(s)) != 0:
        return None
    return w.value, s.value


def _head_ok(mods, head) -> int:
    """fused_layers of a head actor's backbone (its last Linear is folded: any width), 0 when the
    head does not sit on it as the reference builds it."""
    nl = fused_layers(mods, max_out=MAX_HIDDEN_1)
    if nl == 0 or type(head.mu_activation) not in _ACT_CODE or type(head.sigma_activation) not in _ACT_CODE:
        return 0
    H, K = mods[-1].out_features, head.mu_head.out_features
    if head.mu_head.in_features != H or head.sigma_head.in_features != H or head.sigma_head.out_features != K \
            or mods[-1].in_features != H or head.mu_head.bias is None or head.sigma_head.bias is None:
        return 0
    return nl


def musigma_tier(mods, head) -> int:
    """Inference path of a head actor (backbone mods, MuSigmaHead): 1 = one fused launch
    (musigma_forward), 2 = folded weights through the plain fused MLP (musigma_folded), 3 = torch
    layers."""
    nl = _head_ok(mods, head)
    if nl == 0:
        return 3
    K = head.mu_head.out_features
    if K <= HEAD_MAX_FUSED:
        H2 = mods[2].out_features if nl == 3 else 0
        return 1 if musigma_layout(mods[0].out_features, H2, K) is not None else 3
    return 2 if K <= HEAD_MAX_FOLDED else 3


def _head_index(H: int, K: int, stride: int, device):
    """whp[s][h][c] = W_eff[c < stride / 2 ? c : K + c - stride / 2][32 (s // 16) + rho(s % 16, h)]
    (0 where the head's column index is >= K): mu weights in the first half, sigma's in the second."""
    key = ("head", H, K, stride, str(device))
    if key not in _IDX:
        sv = torch.arange((H // 32) * 16, device=device)[:, None, None]
        hv = torch.arange(2, device=device)[None, :, None]
        cv = torch.arange(stride, device=device)[None, None, :]
        a = cv % (stride // 2)
        row = a.clamp(max=K - 1) + K * (cv // (stride // 2))
        idx = (row * H + (sv // 16) * 32 + _rho(sv % 16, hv)).reshape(-1)
        _IDX[key] = (idx, (a < K).expand((H // 32) * 16, 2, stride).reshape(-1))
    return _IDX[key]


def _head_pack(mods, head, nl: int, w1: torch.Tensor, cur, fused: bool):
    """(w1p, w2p, whp, b_eff) of the folded head actor: whp in the dual-head VALU layout (fused) or
    the MFMA fragments of the 2K-row folded matrix. The cache key holds every contributing tensor,
    biases included (they enter b_eff)."""
    l1, lo = mods[0], mods[-1]
    l2 = mods[2] if nl == 3 else None
    hs = (lo.weight, lo.bias, head.mu_head.weight, head.mu_head.bias, head.sigma_head.weight, head.sigma_head.bias)
    weights = ((w1,) if l2 is None else (w1, l2.weight)) + hs

    def build():
        w_eff, b_eff = fold_head(lo, head)
        w1p, w2p, w3p = pack_mlp3(w1, None if l2 is None else l2.weight, w_eff, layout=0)
        if fused:
            H, K = lo.out_features, head.mu_head.out_features
            _, stride = musigma_layout(l1.out_features, l2.out_features if l2 is not None else 0, K)
            idx, valid = _head_index(H, K, stride, w1.device)
            w3p = torch.where(valid, w_eff.reshape(-1)[idx], torch.zeros((), device=w1.device)).contiguous()
        return w1p, w2p, w3p, b_eff

    slot = ("musigma" if fused else "musigma_folded", w1.shape, w1.stride(), w1.storage_offset())
    return _cached_pack(l1, slot, weights, cur, build)


def _rows(x: torch.Tensor, L: int) -> torch.Tensor:
    xf = x.reshape(-1, L)
    if xf.dtype != torch.float32 or not xf.is_contiguous():
        xf = xf.float().contiguous()
    return xf


def musigma_forward(mods, head, x: torch.Tensor, dist_out: Optional[torch.Tensor] = None, *, sample=None,
                    w1: Optional[torch.Tensor] = None, pre1: Optional[torch.Tensor] = None, group: int = 1):
    """msc_mlp{2,3}_relu_musigma over x [..., L] (f32 CUDA): backbone -> folded dual head -> head
    activations and the log_std clamp in one launch (musigma_tier(mods, head) must be 1).
    sample: (eps, actions, logp, clipped) -- msc_gaussian_sample's arithmetic on each row's
    (mu, log_std) while they are in registers; the distribution inputs [mu || log_std] ([..., 2K])
    then go to `dist_out` only when it is given. Without `sample` they are always written (to a new
    buffer when dist_out is None). w1 / pre1 / group as in mlp3_forward. Returns dist_out or None."""
    nl = _head_ok(mods, head)
    K = head.mu_head.out_features
    if musigma_tier(mods, head) != 1:
        raise ValueError("no fused mu/sigma-head kernel for this actor (see musigma_tier)")
    l1 = mods[0]
    l2 = mods[2] if nl == 3 else None
    w1 = l1.weight if w1 is None else w1
    L = w1.shape[1]
    if x.shape[-1] != L:
        raise ValueError(f"input has {x.shape[-1]} features, the MLP expects {L}")
    cur = torch.cuda.current_stream(x.device)
    w1p, w2p, whp, b_eff = _head_pack(mods, head, nl, w1, cur, True)
    lead, xf = x.shape[:-1], _rows(x, L)
    n = xf.shape[0]
    if pre1 is not None:
        pre1 = _pre1_rows(pre1, n, group, l1.out_features)
    if sample is None and dist_out is None:
        dist_out = torch.empty((n, 2 * K), device=x.device, dtype=torch.float32)
    if dist_out is not None and not (dist_out.is_cuda and dist_out.dtype == torch.float32
                                     and dist_out.is_contiguous() and dist_out.numel() == n * 2 * K):
        raise ValueError("dist_out must be a contiguous float32 CUDA tensor of rows x 2K")
    eps = act = logp = clipped = None
    if sample is not None:
        eps, act, logp, clipped = sample
        for t in sample:
            if not (t.is_cuda and t.dtype == torch.float32 and t.is_contiguous()):
                raise ValueError("sampling buffers must be contiguous float32 CUDA tensors")
        if eps.numel() != n * K or act.numel() != n * K or clipped.numel() != n * K or logp.numel() != n:
            raise ValueError("sampling buffers do not match the MLP's rows / actions")
    from .rollout import LOG_STD_MAX, LOG_STD_MIN
    ep = abi.MscMuSigmaEpilogue(_ACT_CODE[type(head.mu_activation)], _ACT_CODE[type(head.sigma_activation)],
                                C.c_float(LOG_STD_MIN), C.c_float(LOG_STD_MAX), _vp(eps), _vp(act), _vp(logp),
                                _vp(clipped), _vp(dist_out))
    st = C.c_void_p(cur.cuda_stream)
    b1 = l1.bias.detach().float().contiguous()
    if l2 is None:
        abi.check(abi.lib().msc_mlp2_relu_musigma(_vp(xf), n, L, l1.out_features, K, _vp(w1p), _vp(b1), _vp(whp), _vp(b_eff),
                                                  _vp(pre1), int(group), C.byref(ep), st))
    else:
        b2 = l2.bias.detach().float().contiguous()
        abi.check(abi.lib().msc_mlp3_relu_musigma(_vp(xf), n, L, l1.out_features, l2.out_features, K, _vp(w1p), _vp(b1),
                                                  _vp(w2p), _vp(b2), _vp(whp), _vp(b_eff), _vp(pre1), int(group),
                                                  C.byref(ep), st))
    return None if dist_out is None else dist_out.reshape(*lead, 2 * K)


def musigma_folded(mods, head, x: torch.Tensor):
    """(mu, log_std) [..., K] of a head actor with up to 16 actions: msc_mlp{2,3}_relu_forward on the
    folded weights (2K <= 32 rows of the MFMA output layer), head activations and clamp in torch."""
    nl = _head_ok(mods, head)
    K = head.mu_head.out_features
    if nl == 0 or K > HEAD_MAX_FOLDED:
        raise ValueError("no folded mu/sigma-head path for this actor (see musigma_tier)")
    l1 = mods[0]
    l2 = mods[2] if nl == 3 else None
    L = l1.in_features
    cur = torch.cuda.current_stream(x.device)
    w1p, w2p, w3p, b_eff = _head_pack(mods, head, nl, l1.weight, cur, False)
    lead, xf = x.shape[:-1], _rows(x, L)
    n = xf.shape[0]
    out = torch.empty((n, 2 * K), device=x.device, dtype=torch.float32)
    st = C.c_void_p(cur.cuda_stream)
    b1 = l1.bias.detach().float().contiguous()
    if l2 is None:
        abi.check(abi.lib().msc_mlp2_relu_forward(_vp(xf), n, L, l1.out_features, 2 * K, _vp(w1p), _vp(b1), _vp(w3p),
                                                  _vp(b_eff), _vp(out), None, 1, st))
    else:
        b2 = l2.bias.detach().float().contiguous()
        abi.check(abi.lib().msc_mlp3_relu_forward(_vp(xf), n, L, l1.out_features, l2.out_features, 2 * K, _vp(w1p), _vp(b1),
                                                  _vp(w2p), _vp(b2), _vp(w3p), _vp(b_eff), _vp(out), None, 1, st))
    from .rollout import LOG_STD_MAX, LOG_STD_MIN
    mu, ls = out[:, :K], out[:, K:]
    if head.mu_activation is not None:
        mu = head.mu_activation(mu)
    if head.sigma_activation is not None:
        ls = head.sigma_activation(ls)
    return mu.reshape(*lead, K), torch.clamp(ls, LOG_STD_MIN, LOG_STD_MAX).reshape(*lead, K)


# ----------------------------------------------------------------------------------------------
# Wide-output MLPs (33..128 outputs: the centralised CPPO actor's joint action, W K = 40 at C3 and
# 80 at C5): msc_mlp{2,3}_relu_wide (csrc/mlp_wide.hip), the output layer on ceil(KO / 32) MFMA tiles
# and msc_gaussian_sample's arithmetic in an LDS-staged epilogue. Taken only where no kernel above
# applies (KO > 32): every narrower network keeps the path it had. Opt-in at rollout (WIDE_ENABLED).
# ----------------------------------------------------------------------------------------------
WIDE_MAX_OUT = 128
# The rollout dispatch (rollout.fused_actor_sample / mlp_forward) takes the wide kernel only with
# MSC_WIDE_MLP=1: measured against the torch layers + msc_gaussian_sample it is 1.27x faster at the C3
# shape (32,768 rows of 208 -> 256 -> 40) and 0.92x at the C5 shape (8,192 rows of 416 -> 256 -> 80: 256
# waves of 32 rows on 1,024 SIMDs), and the default needs both.
# wide_forward itself does not look at the switch.
WIDE_ENABLED = os.environ.get("MSC_WIDE_MLP", "0") == "1"


def _wide_index(H: int, KO: int, device):
    """w3p[o][q][lane][i] = W3[32 o + c][32 (q // 4) + rho(4 (q % 4) + i, h)] (0 for rows >= KO): the
    layout-0 fragment order of _index_maps once per 32-row slice of W3, slices concatenated."""
    key = ("wide", H, KO, str(device))
    if key not in _IDX:
        lane = torch.arange(64, device=device)
        c, h = (lane & 31)[None, None, :, None], (lane >> 5)[None, None, :, None]
        NTO = (KO + 31) // 32
        o = torch.arange(NTO, device=device)[:, None, None, None]
        q = torch.arange((H // 32) * 4, device=device)[None, :, None, None]
        r = (q % 4) * 4 + torch.arange(4, device=device)[None, None, None, :]
        row = o * 32 + c
        idx = (row.clamp(max=KO - 1) * H + (q // 4) * 32 + _rho(r, h)).reshape(-1)
        _IDX[key] = (idx, (row < KO).expand(NTO, (H // 32) * 4, 64, 4).reshape(-1))
    return _IDX[key]


def pack_wide(w1: torch.Tensor, w2: Optional[torch.Tensor], w3: torch.Tensor):
    """Torch Linear weights -> (w1p, w2p, w3p) for msc_mlp{2,3}_relu_wide: w1p / w2p as pack_mlp3's,
    w3p [ceil(KO / 32)][H_last / 8][64][4] (see _wide_index). w2 None: one hidden layer."""
    H1, L = w1.shape
    H2, KO = (w2.shape[0] if w2 is not None else 0), w3.shape[0]
    if not 1 <= KO <= WIDE_MAX_OUT:
        raise ValueError(f"the wide MLP supports 1..{WIDE_MAX_OUT} outputs, not {KO}")
    i1, v1, i2, _, _ = _index_maps(L, H1, H2, min(KO, MAX_OUT), w1.device, 0)
    i3, v3 = _wide_index(H2 or H1, KO, w1.device)
    zero = torch.zeros((), device=w1.device, dtype=torch.float32)
    w1p = torch.where(v1, w1.detach().float().reshape(-1)[i1], zero)
    w2p = w2.detach().float().reshape(-1)[i2].contiguous() if w2 is not None else None
    w3p = torch.where(v3, w3.detach().float().reshape(-1)[i3], zero)
    return w1p.contiguous(), w2p, w3p.contiguous()


def wide_layers(mods) -> int:
    """2 or 3 when mods has a wide kernel: fused_layers' Linear / ReLU / bias / hidden-size
    conditions with 32 < out_dim <= 128; 0 otherwise."""
    if not mods or not isinstance(mods[-1], nn.Linear) or not MAX_OUT < mods[-1].out_features <= WIDE_MAX_OUT:
        return 0
    return fused_layers(mods, max_out=WIDE_MAX_OUT)


def wide_forward(mods, x: torch.Tensor, out: Optional[torch.Tensor] = None, *, sample=None,
                 w1: Optional[torch.Tensor] = None, pre1: Optional[torch.Tensor] = None, group: int = 1):
    """msc_mlp{2,3}_relu_wide over x [..., L] (f32 CUDA) -> [..., KO]; wide_layers(mods) must hold.
    sample: (log_std [P, KO], logstd_floor, eps, actions, logp, clipped) -- msc_gaussian_sample's
    arithmetic in the kernel's epilogue, bit-identical to the separate call on the means; the means
    then go to `out` only when it is given (returns `out`, possibly None). w1 / pre1 / group as in
    mlp3_forward."""
    nl = wide_layers(mods)
    if nl == 0:
        raise ValueError("no wide kernel for this layer sequence (see wide_layers)")
    l1, l3 = mods[0], mods[-1]
    l2 = mods[2] if nl == 3 else None
    w1 = l1.weight if w1 is None else w1
    L, KO = w1.shape[1], l3.out_features
    if x.shape[-1] != L:
        raise ValueError(f"input has {x.shape[-1]} features, the MLP expects {L}")
    cur = torch.cuda.current_stream(x.device)
    weights = (w1, l3.weight) if l2 is None else (w1, l2.weight, l3.weight)
    w1p, w2p, w3p = _cached_pack(l1, ("wide", w1.shape, w1.stride(), w1.storage_offset()), weights, cur,
                                 lambda: pack_wide(w1, None if l2 is None else l2.weight, l3.weight))
    lead, xf = x.shape[:-1], _rows(x, L)
    n = xf.shape[0]
    if pre1 is not None:
        pre1 = _pre1_rows(pre1, n, group, l1.out_features)
    ep = None
    if sample is not None:
        ep = C.byref(_gaussian_epilogue(sample, n, KO))
    elif out is None:
        out = torch.empty((n, KO), device=x.device, dtype=torch.float32)
    if out is not None and not (out.is_cuda and out.dtype == torch.float32 and out.is_contiguous()
                                and out.numel() == n * KO):
        raise ValueError("out must be a contiguous float32 CUDA tensor of rows x outputs")
    st = C.c_void_p(cur.cuda_stream)
    b1, b3 = (m.bias.detach().float().contiguous() for m in (l1, l3))
    if l2 is None:
        abi.check(abi.lib().msc_mlp2_relu_wide(_vp(xf), n, L, l1.out_features, KO, _vp(w1p), _vp(b1), _vp(w3p), _vp(b3),
                                               _vp(out), _vp(pre1), int(group), ep, st))
    else:
        b2 = l2.bias.detach().float().contiguous()
        abi.check(abi.lib().msc_mlp3_relu_wide(_vp(xf), n, L, l1.out_features, l2.out_features, KO, _vp(w1p), _vp(b1),
                                               _vp(w2p), _vp(b2), _vp(w3p), _vp(b3), _vp(out), _vp(pre1), int(group), ep, st))
    return None if out is None else out.reshape(*lead, KO)


# ----------------------------------------------------------------------------------------------
# Per-agent policies (parameter_sharing: false, one module per warehouse): P same-shaped MLPs with P
# weight sets over rows laid out [..., P, L] in one launch, msc_mlp{2,3}_relu_multi (csrc/mlp_multi.hip).
# Row (e, p) is bit-identical to mlp3_forward on policy p's rows gathered contiguously. Opt-in at
# rollout (MSC_MULTI_MLP=1 / MultiAgentActorCritic(multi_mlp=True)); multi_forward itself does not look
# at the switch. Not covered: GRU policies, mu/sigma-head actors, the wide (33..128 outputs) kernel.
# ----------------------------------------------------------------------------------------------
MULTI_MAX_POLICIES = 64


def multi_default() -> bool:
    """MSC_MULTI_MLP=1 turns the multi-policy kernel on where MultiAgentActorCritic is built with
    multi_mlp=None. Off by default: see DESIGN.md section 8 for the measured A/B and the rule for a flip."""
    return os.environ.get("MSC_MULTI_MLP", "0") == "1"


def multi_layers(mods_list) -> int:
    """2 or 3 when every layer list of mods_list passes fused_layers with the same form and the same
    Linear shapes (1..64 policies); 0 otherwise (the caller runs the policies one by one)."""
    mods_list = [list(m) for m in mods_list]
    if not 1 <= len(mods_list) <= MULTI_MAX_POLICIES:
        return 0
    nl = fused_layers(mods_list[0])
    if nl == 0:
        return 0
    shapes = [tuple(m.weight.shape) for m in mods_list[0][0::2]]
    for mods in mods_list[1:]:
        if fused_layers(mods) != nl or [tuple(m.weight.shape) for m in mods[0::2]] != shapes:
            return 0
    return nl


def pack_multi(w1s, w2s, w3s, layout: Optional[int] = None):
    """P policies' torch Linear weights (lists of [H1, L], [H2, H1] or None, [KO, H2]) -> (w1p, w2p, w3p),
    each [P, ...]: row p is pack_mlp3 of policy p (one gather over the stacked weights with the
    cached index maps)."""
    H1, L = w1s[0].shape
    H2, KO = (w2s[0].shape[0] if w2s is not None else 0), w3s[0].shape[0]
    i1, v1, i2, i3, v3 = _index_maps(L, H1, H2, KO, w1s[0].device, w3_layout(KO) if layout is None else layout)
    n = len(w1s)
    zero = torch.zeros((), device=w1s[0].device, dtype=torch.float32)
    flat = lambda ws: torch.stack([w.detach().float() for w in ws]).reshape(n, -1)  # noqa: E731
    w1p = torch.where(v1, flat(w1s)[:, i1], zero)
    w2p = flat(w2s)[:, i2].contiguous() if w2s is not None else None
    w3p = torch.where(v3, flat(w3s)[:, i3], zero)
    return w1p.contiguous(), w2p, w3p.contiguous()


def multi_pack(mods_list, w1s=None, cur=None):
    """(w1p, w2p, w3p, b1, b2, b3) of P policies: stacked packs [P, ...] and stacked biases [P, H] (w2p /
    b2 None for one hidden layer), cached on policy 0's first Linear under a key holding every
    policy's (data_ptr, _version) of every weight and bias: rebuilt when any one of them changes or
    moves, and only then. w1s: first-layer weights to use instead of each mods[0].weight. cur: the
    stream the pack is used on (_cached_pack's ordering); None on the host."""
    mods_list = [list(m) for m in mods_list]
    nl = multi_layers(mods_list)
    if nl == 0:
        raise ValueError("no multi-policy kernel for these layer sequences (see multi_layers)")
    l1 = mods_list[0][0]
    w1s = [m[0].weight for m in mods_list] if w1s is None else list(w1s)
    w2s = [m[2].weight for m in mods_list] if nl == 3 else None
    w3s = [m[-1].weight for m in mods_list]
    lins = [[m for m in mods[0::2]] for mods in mods_list]
    weights = tuple(w1s) + tuple(w2s or ()) + tuple(w3s) + tuple(m.bias for ls in lins for m in ls)

    def build():
        w1p, w2p, w3p = pack_multi(w1s, w2s, w3s)
        bs = [torch.stack([ls[i].bias.detach().float() for ls in lins]).contiguous() for i in range(nl)]
        return (w1p, w2p, w3p, bs[0], bs[1] if nl == 3 else None, bs[-1])

    slot = ("multi", len(mods_list), w1s[0].shape, w1s[0].stride(), w1s[0].storage_offset())
    return _cached_pack(l1, slot, weights, cur, build)


def multi_forward(mods_list, x: torch.Tensor, out: Optional[torch.Tensor] = None, *, w1=None,
                  pre1: Optional[torch.Tensor] = None, sample=None) -> Optional[torch.Tensor]:
    """msc_mlp{2,3}_relu_multi over x [..., P, L] (f32 CUDA) -> [..., P, KO]: policy p (mods_list[p], as
    accepted by multi_layers) evaluates the rows x[..., p, :], all in one launch.
    w1: a list of first-layer weights to use instead of each policy's mods[0].weight; pre1 [rows, H1]:
    added to the first layer's pre-activation, one row per row; sample: (log_std [1 or P, KO],
    logstd_floor, eps, actions, logp, clipped) -- msc_gaussian_sample in the epilogue, log_std row p for
    policy p (needs the VALU output layer, KO <= 8); the means then go to `out` only when it is given
    (returns `out`, possibly None)."""
    mods_list = [list(m) for m in mods_list]
    nl = multi_layers(mods_list)
    if nl == 0:
        raise ValueError("no multi-policy kernel for these layer sequences (see multi_layers)")
    NP = len(mods_list)
    l1, l3 = mods_list[0][0], mods_list[0][-1]
    H1, KO = l1.out_features, l3.out_features
    H2 = mods_list[0][2].out_features if nl == 3 else 0
    L = l1.in_features if w1 is None else w1[0].shape[1]
    if x.dim() < 2 or x.shape[-2] != NP or x.shape[-1] != L:
        raise ValueError(f"input must be [..., {NP}, {L}], not {tuple(x.shape)}")
    cur = torch.cuda.current_stream(x.device)
    w1p, w2p, w3p, b1, b2, b3 = multi_pack(mods_list, w1, cur)
    lead, xf = x.shape[:-1], _rows(x, L)
    n = xf.shape[0]
    if pre1 is not None:
        pre1 = pre1.float().contiguous()
        if pre1.shape != (n, H1):
            raise ValueError(f"pre1 must be [{n}, {H1}]")
    ep = None
    if sample is not None:
        ep = C.byref(_gaussian_epilogue(sample, n, KO, NP))
    elif out is None:
        out = torch.empty((n, KO), device=x.device, dtype=torch.float32)
    if out is not None and not (out.is_cuda and out.dtype == torch.float32 and out.is_contiguous()
                                and out.numel() == n * KO):
        raise ValueError("out must be a contiguous float32 CUDA tensor of rows x outputs")
    st = C.c_void_p(cur.cuda_stream)
    if nl == 2:
        abi.check(abi.lib().msc_mlp2_relu_multi(_vp(xf), n, NP, L, H1, KO, _vp(w1p), _vp(b1), _vp(w3p), _vp(b3), _vp(out),
                                                _vp(pre1), ep, st))
    else:
        abi.check(abi.lib().msc_mlp3_relu_multi(_vp(xf), n, NP, L, H1, H2, KO, _vp(w1p), _vp(b1), _vp(w2p), _vp(b2), _vp(w3p),
                                                _vp(b3), _vp(out), _vp(pre1), ep, st))
    return None if out is None else out.reshape(*lead, KO)


# ----------------------------------------------------------------------------------------------
# Training through the fused kernels (opt-in: PPOLearner(fused_mlp=True) / MSC_FUSED_MLP_GRAD=1): the forward
# is mlp3_forward, the inference kernel, so the learner's forward equals the collector's bit for bit; the
# backward is one msc_mlp_relu_backward call (csrc/mlp_backward.hip) that recomputes the hidden layers and
# returns the six parameter gradients in torch's layouts. No input gradient. Not covered (they keep the torch
# layers): mu/sigma-head backbones, GRU networks and MLP heads over a GRU trunk, and the wide (33..128 outputs)
# actor. Per-agent policies make one call each here; the section after this one runs them in one.
# ----------------------------------------------------------------------------------------------
def fused_mlp_default() -> bool:
    """MSC_FUSED_MLP_GRAD=1 turns the fused MLP backward on where PPOLearner is built with fused_mlp=None."""
    return os.environ.get("MSC_FUSED_MLP_GRAD", "0") == "1"


def backward_workspace_bytes(n_rows: int, in_dim: int, hidden1: int, hidden2: int, out_dim: int) -> int:
    """msc_mlp_relu_backward_workspace: bytes for n_rows rows (monotone in n_rows, capped), -1 when the shape
    has no backward kernel. hidden2 = 0: one hidden layer."""
    return int(abi.lib().msc_mlp_relu_backward_workspace(int(n_rows), int(in_dim), int(hidden1), int(hidden2), int(out_dim)))


_BWD_WORKSPACES: Dict[Tuple[int, int], torch.Tensor] = {}


def _bwd_workspace(device: torch.device, nbytes: int) -> torch.Tensor:
    """One workspace per (device, stream), grown on demand and kept (ppo_loss.py:_workspace's rule: calls on
    one stream are ordered, so a call's last kernel has read the workspace before the next call writes it)."""
    key = (device.index if device.index is not None else torch.cuda.current_device(),
           torch.cuda.current_stream(device).cuda_stream)
    w = _BWD_WORKSPACES.get(key)
    if w is None or w.numel() * 4 < nbytes:
        w = torch.empty(-(-nbytes // 4), dtype=torch.float32, device=device)
        _BWD_WORKSPACES[key] = w
    return w


def trainable(mods) -> bool:
    """True when train_forward covers mods: fused_layers' set with at most 32 outputs, f32 CUDA parameters."""
    mods = list(mods)
    if fused_layers(mods) == 0:
        return False
    return all(p.is_cuda and p.dtype == torch.float32 for m in mods[0::2] for p in (m.weight, m.bias))


def mlp_backward(mods, x: torch.Tensor, d_out: torch.Tensor, *, scale: float = 1.0, grads=None):
    """One msc_mlp_relu_backward call: the gradients of mods' parameters for the upstream gradient d_out
    [..., KO] at the inputs x [..., L] (f32 CUDA), in parameter order (w1, b1[, w2, b2], w3, b3), each in its
    parameter's shape. grads given (that tuple of contiguous f32 tensors): the call adds to them."""
    mods = list(mods)
    nl = fused_layers(mods)
    if nl == 0:
        raise ValueError("no fused kernel for this layer sequence (see fused_layers)")
    l1, l3 = mods[0], mods[-1]
    l2 = mods[2] if nl == 3 else None
    L, H1, KO = l1.in_features, l1.out_features, l3.out_features
    H2 = l2.out_features if l2 is not None else 0
    if x.shape[-1] != L or d_out.shape[-1] != KO:
        raise ValueError(f"x / d_out have {x.shape[-1]} / {d_out.shape[-1]} columns, the MLP has {L} inputs and {KO} outputs")
    xf, df = _rows(x, L), _rows(d_out, KO)
    n = xf.shape[0]
    if df.shape[0] != n:
        raise ValueError(f"d_out has {df.shape[0]} rows for {n} rows of x")
    cur = torch.cuda.current_stream(xf.device)
    w1 = l1.weight
    weights = (w1, l3.weight) if l2 is None else (w1, l2.weight, l3.weight)
    w1p, w2p, _ = _cached_pack(l1, (w1.shape, w1.stride(), w1.storage_offset()), weights, cur,
                               lambda: pack_mlp3(w1, None if l2 is None else l2.weight, l3.weight))
    w2tp = None
    if l2 is not None:
        (w2tp,) = _cached_pack(l1, "w2t", (l2.weight,), cur, lambda: (pack_w2t(l2.weight),))
    lins = (l1, l3) if l2 is None else (l1, l2, l3)
    params = [p for m in lins for p in (m.weight, m.bias)]
    accumulate = grads is not None
    if grads is None:
        grads = tuple(torch.empty(p.shape, dtype=torch.float32, device=xf.device) for p in params)
    elif len(grads) != len(params) or any(not (g.is_cuda and g.dtype == torch.float32 and g.is_contiguous()
                                               and g.shape == p.shape) for g, p in zip(grads, params)):
        raise ValueError("grads must be contiguous float32 CUDA tensors in the parameters' shapes")
    ws = _bwd_workspace(xf.device, backward_workspace_bytes(n, L, H1, H2, KO)) if n > 0 else None
    b1 = l1.bias.detach().float().contiguous()
    b2 = l2.bias.detach().float().contiguous() if l2 is not None else None
    w3 = l3.weight.detach().float().contiguous()
    g = list(grads)
    gw2, gb2 = (g[2], g[3]) if l2 is not None else (None, None)
    abi.check(abi.lib().msc_mlp_relu_backward(_vp(xf), n, L, H1, H2, KO, _vp(w1p), _vp(b1), _vp(w2p), _vp(b2), _vp(w2tp),
                                              _vp(w3), _vp(df), C.c_float(scale), 1 if accumulate else 0, _vp(g[0]), _vp(g[1]),
                                              _vp(gw2), _vp(gb2), _vp(g[-2]), _vp(g[-1]), _vp(ws), C.c_void_p(cur.cuda_stream)))
    return tuple(grads)


class _TrainForward(torch.autograd.Function):
    """mods' forward through the inference kernel; the parameters enter as inputs so that autograd hands their
    gradients on (and checks that none was modified between forward and backward)."""

    @staticmethod
    def forward(ctx, x, mods, *params):
        ctx.mods = mods
        ctx.save_for_backward(x, *params)
        return mlp3_forward(mods, x)

    @staticmethod
    def backward(ctx, g):
        x = ctx.saved_tensors[0]
        return (None, None) + mlp_backward(ctx.mods, x, g)


def train_forward(mods, x: torch.Tensor) -> torch.Tensor:
    """mods (Linear-ReLU(-Linear-ReLU)-Linear as accepted by fused_layers, at most 32 outputs) applied to x
    [..., L] under autograd: msc_mlp{3,2}_relu_forward now, one msc_mlp_relu_backward call in backward().
    x is a leaf of the graph: no gradient flows into it. Raises RuntimeError for non-CUDA or non-float32
    input (there is no CPU path), ValueError for a layer sequence without a kernel."""
    mods = list(mods)
    if not isinstance(x, torch.Tensor) or not x.is_cuda:
        raise RuntimeError("train_forward: x must be a CUDA tensor (the fused MLP backward is a HIP kernel; run the "
                           f"torch layers on {getattr(x, 'device', type(x).__name__)})")
    if x.dtype != torch.float32:
        raise RuntimeError(f"train_forward: x must be torch.float32, not {x.dtype}")
    if x.requires_grad:
        raise RuntimeError("train_forward: x requires a gradient, and the fused backward computes none for its input")
    if fused_layers(mods) == 0:
        raise ValueError("no fused kernel for this layer sequence (see fused_layers)")
    if not trainable(mods):
        raise RuntimeError("train_forward: the parameters must be float32 CUDA tensors")
    params = [p for m in mods[0::2] for p in (m.weight, m.bias)]
    return _TrainForward.apply(x, tuple(mods), *params)


# ----------------------------------------------------------------------------------------------
# The same for per-agent policies (opt-in: PPOLearner(fused_multi=True) / MSC_FUSED_MULTI_GRAD=1): the P
# same-shaped actors (or critics) over rows [n, P, L] as one autograd function -- multi_forward forward, so
# policy p's output is mlp3_forward's on its own rows bit for bit, and ONE msc_mlp_relu_backward_multi call
# backward (csrc/mlp_backward.hip's multi kernels), whose gradients are per policy bit for bit those of
# msc_mlp_relu_backward on the policy's gathered rows. Not covered: what train_forward does not cover.
# ----------------------------------------------------------------------------------------------
def fused_multi_default() -> bool:
    """MSC_FUSED_MULTI_GRAD=1 turns the multi-policy MLP backward on where PPOLearner is built with
    fused_multi=None."""
    return os.environ.get("MSC_FUSED_MULTI_GRAD", "0") == "1"


# msc_mlp_relu_backward_multi_plan's list (include/marlsc.h)
BWD_MULTI_PLAN_KEYS = ("supported", "group_policies", "groups", "rounds", "slices", "round_tiles", "workspace_bytes")


def multi_backward_plan(n_rows: int, n_policies: int, in_dim: int, hidden1: int, hidden2: int, out_dim: int) -> Dict[str, int]:
    """msc_mlp_relu_backward_multi_plan (no GPU is touched): whether the call exists for these sizes, the policies
    per set of launches G and the groups, and per policy the rounds, the slices per round and the row tiles of a
    full round -- the single-policy geometry of n_rows / n_policies rows -- and the workspace bytes."""
    buf = (C.c_int64 * len(BWD_MULTI_PLAN_KEYS))()
    n = abi.lib().msc_mlp_relu_backward_multi_plan(int(n_rows), int(n_policies), int(in_dim), int(hidden1), int(hidden2),
                                                   int(out_dim), buf, len(BWD_MULTI_PLAN_KEYS))
    if n < 0:
        abi.check(n)
    return dict(zip(BWD_MULTI_PLAN_KEYS, (int(v) for v in buf)))


def multi_backward_workspace_bytes(n_rows: int, n_policies: int, in_dim: int, hidden1: int, hidden2: int, out_dim: int) -> int:
    """msc_mlp_relu_backward_multi_workspace: G x the single-policy bytes of n_rows / n_policies rows (monotone in
    n_rows, capped), -1 where the single query is or for a policy count that is not 1..64 or does not divide n_rows."""
    return int(abi.lib().msc_mlp_relu_backward_multi_workspace(int(n_rows), int(n_policies), int(in_dim), int(hidden1),
                                                               int(hidden2), int(out_dim)))


def multi_trainable(mods_list) -> bool:
    """True when multi_train_forward covers mods_list: multi_layers accepts it (same form and shapes, 1..64
    policies), every list passes trainable, and there are at most 32 outputs. A network that is no layer
    sequence (a GRU) is not covered."""
    mods_list = list(mods_list)
    if not all(isinstance(m, (nn.Sequential, list, tuple)) for m in mods_list):
        return False
    mods_list = [list(m) for m in mods_list]
    if multi_layers(mods_list) == 0 or mods_list[0][-1].out_features > MAX_OUT:
        return False
    return all(trainable(mods) for mods in mods_list)


def _multi_bwd_pack(mods_list, nl: int, cur):
    """(w2tp [P, ...] or None, w3 [P, KO, H_last], b1 [P, H1], b2 [P, H2] or None) for the multi backward, cached as
    multi_pack caches the forward's: keyed on every policy's (data_ptr, _version), rebuilt only when one changes."""
    lins = [mods[0::2] for mods in mods_list]
    weights = tuple(p for ls in lins for m in ls for p in (m.weight, m.bias))

    def build():
        w2tp = torch.stack([pack_w2t(ls[1].weight) for ls in lins]).contiguous() if nl == 3 else None
        w3 = torch.stack([ls[-1].weight.detach().float() for ls in lins]).contiguous()
        b1 = torch.stack([ls[0].bias.detach().float() for ls in lins]).contiguous()
        b2 = torch.stack([ls[1].bias.detach().float() for ls in lins]).contiguous() if nl == 3 else None
        return (w2tp, w3, b1, b2)

    return _cached_pack(mods_list[0][0], ("multi_bwd", len(mods_list)), weights, cur, build)


def multi_backward(mods_list, x: torch.Tensor, d_out: torch.Tensor, *, scale: float = 1.0, grads=None):
    """One msc_mlp_relu_backward_multi call: the gradients of P policies' parameters (mods_list as accepted by
    multi_trainable) for the upstream gradient d_out [..., P, KO] at the inputs x [..., P, L] (f32 CUDA). Returns,
    per policy, the tuple in parameter order (w1, b1[, w2, b2], w3, b3): views g[p] of the stacked outputs
    [P, ...], each contiguous and in its parameter's shape. grads given (the 4 or 6 stacked contiguous f32
    tensors): the call adds to them, and the views are of them."""
    mods_list = [list(m) for m in mods_list]
    nl = multi_layers(mods_list)
    if nl == 0:
        raise ValueError("no multi-policy kernel for these layer sequences (see multi_layers)")
    NP = len(mods_list)
    l1, l3 = mods_list[0][0], mods_list[0][-1]
    L, H1, KO = l1.in_features, l1.out_features, l3.out_features
    H2 = mods_list[0][2].out_features if nl == 3 else 0
    if x.dim() < 2 or tuple(x.shape[-2:]) != (NP, L) or d_out.dim() < 2 or tuple(d_out.shape[-2:]) != (NP, KO):
        raise ValueError(f"x / d_out must be [..., {NP}, {L}] / [..., {NP}, {KO}], not {tuple(x.shape)} / {tuple(d_out.shape)}")
    xf, df = _rows(x, L), _rows(d_out, KO)
    n = xf.shape[0]
    if df.shape[0] != n:
        raise ValueError(f"d_out has {df.shape[0]} rows for {n} rows of x")
    cur = torch.cuda.current_stream(xf.device)
    w1p, w2p = multi_pack(mods_list, None, cur)[:2]
    w2tp, w3, b1, b2 = _multi_bwd_pack(mods_list, nl, cur)
    shapes = [tuple(p.shape) for m in mods_list[0][0::2] for p in (m.weight, m.bias)]
    accumulate = grads is not None
    if grads is None:
        grads = tuple(torch.empty((NP,) + s, dtype=torch.float32, device=xf.device) for s in shapes)
    elif len(grads) != len(shapes) or any(not (g.is_cuda and g.dtype == torch.float32 and g.is_contiguous()
                                               and tuple(g.shape) == (NP,) + s) for g, s in zip(grads, shapes)):
        raise ValueError("grads must be contiguous float32 CUDA tensors [P, ...] in the parameters' shapes")
    ws = _bwd_workspace(xf.device, multi_backward_workspace_bytes(n, NP, L, H1, H2, KO)) if n > 0 else None
    g = list(grads)
    gw2, gb2 = (g[2], g[3]) if nl == 3 else (None, None)
    abi.check(abi.lib().msc_mlp_relu_backward_multi(
        _vp(xf), n, NP, L, H1, H2, KO, _vp(w1p), _vp(b1), _vp(w2p), _vp(b2), _vp(w2tp), _vp(w3), _vp(df), C.c_float(scale),
        1 if accumulate else 0, _vp(g[0]), _vp(g[1]), _vp(gw2), _vp(gb2), _vp(g[-2]), _vp(g[-1]), _vp(ws),
        C.c_void_p(cur.cuda_stream)))
    return [tuple(t[p] for t in g) for p in range(NP)]


class _MultiTrainForward(torch.autograd.Function):
    """P policies' forward through the multi inference kernel; all their parameters enter as inputs (policy by
    policy, each in parameter order), so autograd hands every one its gradient."""

    @staticmethod
    def forward(ctx, x, mods_list, *params):
        ctx.mods_list = mods_list
        ctx.save_for_backward(x, *params)
        return multi_forward(mods_list, x)

    @staticmethod
    def backward(ctx, g):
        x = ctx.saved_tensors[0]
        per_policy = multi_backward(ctx.mods_list, x, g)
        return (None, None) + tuple(t for gp in per_policy for t in gp)


def multi_train_forward(mods_list, x: torch.Tensor) -> torch.Tensor:
    """P same-shaped MLPs (mods_list as accepted by multi_layers, at most 32 outputs) applied to x [n, P, L] under
    autograd -> [n, P, KO]: msc_mlp{3,2}_relu_multi now (policy p's rows equal mlp3_forward's and train_forward's
    on them bit for bit), one msc_mlp_relu_backward_multi call in backward(). x is a leaf of the graph. Refusals as
    train_forward's: RuntimeError for non-CUDA, non-float32 or gradient-requiring input and for parameters that are
    not float32 CUDA tensors, ValueError for layer sequences without a kernel."""
    mods_list = [list(m) for m in mods_list]
    if not isinstance(x, torch.Tensor) or not x.is_cuda:
        raise RuntimeError("multi_train_forward: x must be a CUDA tensor (the fused MLP backward is a HIP kernel; run "
                           f"the torch layers on {getattr(x, 'device', type(x).__name__)})")
    if x.dtype != torch.float32:
        raise RuntimeError(f"multi_train_forward: x must be torch.float32, not {x.dtype}")
    if x.requires_grad:
        raise RuntimeError("multi_train_forward: x requires a gradient, and the fused backward computes none for its input")
    if multi_layers(mods_list) == 0:
        raise ValueError("no multi-policy kernel for these layer sequences (see multi_layers)")
    if not multi_trainable(mods_list):
        raise RuntimeError("multi_train_forward: the parameters must be float32 CUDA tensors")
    if x.dim() != 3:
        raise ValueError(f"multi_train_forward: x must be [n, {len(mods_list)}, L], not {tuple(x.shape)}")
    params = [p for mods in mods_list for m in mods[0::2] for p in (m.weight, m.bias)]
    return _MultiTrainForward.apply(x, tuple(tuple(m) for m in mods_list), *params)
