"""The learner's gradient clip and Adam step as one HIP call (csrc/adam_clip.hip, msc_adam_clip_step):
torch.nn.utils.clip_grad_norm_ per policy followed by torch.optim.Adam.step, for every parameter tensor of
every policy at once. PPOLearner takes this path with fused_opt=True or MSC_FUSED_OPT=1 (opt-in, DESIGN.md
section 8); the arithmetic is pinned in include/marlsc.h."""
from __future__ import annotations

import ctypes as C
import os
from typing import Any, Dict, Iterable, List, Optional, Sequence

import numpy as np
import torch

from . import abi

# msc_opt_tensor as a numpy record: the host table is one array, and a column (the gradient pointers, new
# every step after zero_grad(set_to_none=True)) is written with one assignment
TABLE_DTYPE = np.dtype({"names": ["p", "g", "m", "v", "n", "group"], "formats": ["u8", "u8", "u8", "u8", "i8", "i4"],
                        "offsets": [0, 8, 16, 24, 32, 40], "itemsize": C.sizeof(abi.MscOptTensor)})
assert all(getattr(abi.MscOptTensor, f).offset == TABLE_DTYPE.fields[f][1] for f in TABLE_DTYPE.names)


def fused_opt_default() -> bool:
    """MSC_FUSED_OPT=1 turns the fused clip + Adam step on where PPOLearner is built with fused_opt=None."""
    return os.environ.get("MSC_FUSED_OPT", "0") == "1"


def geometry() -> Dict[str, int]:
    """{'chunk': elements per block, 'table_capacity': tensors per launch} of the library's kernels."""
    c, t = C.c_int32(), C.c_int32()
    abi.check(abi.lib().msc_adam_clip_geometry(C.byref(c), C.byref(t)))
    return {"chunk": c.value, "table_capacity": t.value}


def workspace_bytes(n_tensors: int, total_elems: int) -> int:
    return int(abi.lib().msc_adam_clip_workspace(int(n_tensors), int(total_elems)))


def adam_clip_launch(table: np.ndarray, n_groups: int, *, lr: float, beta1: float, beta2: float, eps: float,
                     max_norm: float, step: int, write_clipped_grads: bool, workspace: torch.Tensor,
                     norms_out: Optional[torch.Tensor] = None) -> None:
    """One msc_adam_clip_step call on a host table (a TABLE_DTYPE record array) on workspace's device and its
    current stream."""
    d = abi.MscAdamClipDesc(float(lr), float(beta1), float(beta2), float(eps), float(max_norm), int(step),
                            1 if write_clipped_grads else 0)
    abi.check(abi.lib().msc_adam_clip_step(
        C.byref(d), C.c_void_p(table.ctypes.data), int(table.shape[0]), int(n_groups),
        None if norms_out is None else C.c_void_p(norms_out.data_ptr()), C.c_void_p(workspace.data_ptr()),
        C.c_void_p(torch.cuda.current_stream(workspace.device).cuda_stream)))


class FusedClipAdam:
    """torch.optim.Adam (no weight decay, no amsgrad) with the per-policy global-norm clip in front of it, one
    msc_adam_clip_step call per step.

    param_lists: one parameter list per policy (a clip group), contiguous float32 parameters on one device.
    step() is a HIP kernel and raises RuntimeError unless that device is a CUDA device; the state and its
    (de)serialisation work anywhere. The parameters are numbered in the order given, which for
    `[list(p.parameters()) for p in module.policies]` is the order of torch.optim.Adam(module.parameters()):
    state_dict() / load_state_dict() use that optimizer's format, so either one resumes from the other's
    checkpoint. `param_groups` is one group as torch's (a learner sets its 'lr'); `zero_grad` is torch's.

    The state (exp_avg, exp_avg_sq, the step count) of a parameter is created at its first step with a
    gradient; a parameter whose .grad is None is skipped and its state is not advanced, as in torch. The
    kernel takes one step count per call: parameters that take part in one step() with different step
    counts (some skipped earlier, others not) raise RuntimeError. The workspace is the optimizer's own and
    calls on one stream are ordered; do not step one optimizer from two streams at once."""

    def __init__(self, param_lists: Sequence[Iterable[torch.nn.Parameter]], lr: float = 1e-3,
                 betas=(0.9, 0.999), eps: float = 1e-8, write_clipped_grads: bool = True):
        self.groups = [list(ps) for ps in param_lists]
        self.params: List[torch.nn.Parameter] = [p for ps in self.groups for p in ps]
        if not self.params:
            raise ValueError("FusedClipAdam: no parameters")
        if len({id(p) for p in self.params}) != len(self.params):
            raise ValueError("FusedClipAdam: a parameter appears twice")
        dev = self.params[0].device
        for p in self.params:
            if p.device != dev or p.dtype != torch.float32 or not p.is_contiguous():
                raise RuntimeError("FusedClipAdam: the parameters must be contiguous float32 tensors on one device "
                                   f"({dev}), not {p.dtype} on {p.device}")
        self.device = dev
        self.write_clipped_grads = bool(write_clipped_grads)
        # torch.optim.Adam's own defaults (whatever keys this torch has), so that its load_state_dict finds them
        defaults = dict(torch.optim.Adam([torch.nn.Parameter(torch.zeros(1))], lr=float(lr), betas=tuple(betas),
                                         eps=float(eps)).defaults)
        self.param_groups: List[Dict[str, Any]] = [{**defaults, "params": self.params}]
        N = len(self.params)
        self._m: List[Optional[torch.Tensor]] = [None] * N
        self._v: List[Optional[torch.Tensor]] = [None] * N
        self._steps = [0] * N
        self._n_state = 0  # parameters with exp_avg / exp_avg_sq
        self._table = np.zeros(N, dtype=TABLE_DTYPE)
        self._table["n"] = [p.numel() for p in self.params]
        self._table["group"] = [j for j, ps in enumerate(self.groups) for _ in ps]
        self._workspace: Optional[torch.Tensor] = None

    # -- torch.optim.Optimizer's surface, as far as the learner and the trainer use it --
    def zero_grad(self, set_to_none: bool = True) -> None:
        for p in self.params:
            if p.grad is not None:
                if set_to_none:
                    p.grad = None
                else:
                    p.grad.detach_().zero_()

    def state_dict(self) -> Dict[str, Any]:
        state = {i: {"step": torch.tensor(float(s)), "exp_avg": self._m[i], "exp_avg_sq": self._v[i]}
                 for i, s in enumerate(self._steps) if self._m[i] is not None}
        group = {k: v for k, v in self.param_groups[0].items() if k != "params"}
        group["params"] = list(range(len(self.params)))
        return {"state": state, "param_groups": [group]}

    def load_state_dict(self, sd: Dict[str, Any]) -> None:
        groups = sd["param_groups"]
        if len(groups) != 1 or len(groups[0]["params"]) != len(self.params):
            raise ValueError("FusedClipAdam.load_state_dict: expected one parameter group of "
                             f"{len(self.params)} parameters")
        g = groups[0]
        if g.get("weight_decay", 0) or g.get("amsgrad", False) or g.get("maximize", False):
            raise ValueError("FusedClipAdam.load_state_dict: weight_decay, amsgrad and maximize are not supported")
        self.param_groups[0].update({k: v for k, v in g.items() if k != "params"})
        pos = {pid: i for i, pid in enumerate(g["params"])}
        N = len(self.params)
        self._m, self._v, self._steps = [None] * N, [None] * N, [0] * N
        self._n_state = len(sd["state"])
        for pid, st in sd["state"].items():
            i = pos[pid]
            p = self.params[i]
            self._steps[i] = int(round(float(st["step"])))
            self._m[i] = st["exp_avg"].detach().to(device=p.device, dtype=torch.float32).reshape(p.shape).contiguous().clone()
            self._v[i] = st["exp_avg_sq"].detach().to(device=p.device, dtype=torch.float32).reshape(p.shape).contiguous().clone()
            self._table["m"][i], self._table["v"][i] = self._m[i].data_ptr(), self._v[i].data_ptr()

    # -- the step --
    def step(self, lr: Optional[float] = None, max_norm: Optional[float] = None,
             norms_out: Optional[torch.Tensor] = None) -> None:
        """Clip every policy's gradients by its own global norm (max_norm None or <= 0: no clip) and take the
        Adam step with learning rate lr (None: param_groups[0]['lr']) on the current stream. norms_out: a
        device f64[len(param_lists)] that receives every policy's gradient norm (0 without gradients)."""
        params, table = self.params, self._table
        if self.device.type != "cuda":
            raise RuntimeError("FusedClipAdam.step: the fused clip + Adam step is a HIP kernel and needs the parameters "
                               f"on a CUDA device, not {self.device}")
        if self._workspace is None:
            nbytes = workspace_bytes(len(params), int(table["n"].sum()))
            self._workspace = torch.empty(max(1, nbytes // 8), dtype=torch.float64, device=self.device)
        # the host work per step is a few list passes over the parameters and nothing per element of the table
        # beyond them: torch itself keeps a .grad on its parameter's device, with its dtype and shape (the
        # assignment checks), so only the strides are looked at here
        grads = [p.grad for p in params]
        if any([g is None for g in grads]):  # (not `None in grads`: that compares tensors with ==)
            active = [i for i, g in enumerate(grads) if g is not None]
            if not active:
                return
        else:
            active = None
        if not all([g is None or g.is_contiguous() for g in grads]):
            for i, g in enumerate(grads):
                if g is not None and not g.is_contiguous():
                    grads[i] = params[i].grad = g.contiguous()
        if self._n_state < len(params):
            for i in (range(len(params)) if active is None else active):
                if self._m[i] is None:
                    self._m[i], self._v[i] = torch.zeros_like(params[i]), torch.zeros_like(params[i])
                    table["m"][i], table["v"][i] = self._m[i].data_ptr(), self._v[i].data_ptr()
                    self._n_state += 1
        table["p"] = [p.data_ptr() for p in params]
        if active is None:
            table["g"] = [g.data_ptr() for g in grads]
            steps = set(self._steps)
        else:
            table["g"][active] = [grads[i].data_ptr() for i in active]
            steps = {self._steps[i] for i in active}
            table = table[active]
        if len(steps) != 1:
            raise RuntimeError(f"FusedClipAdam.step: the parameters of this step have step counts {sorted(steps)}; "
                               "the kernel takes one step count per call")
        step = steps.pop() + 1
        g0 = self.param_groups[0]
        if norms_out is not None and (not norms_out.is_cuda or norms_out.dtype != torch.float64
                                      or norms_out.numel() != len(self.groups) or not norms_out.is_contiguous()):
            raise RuntimeError(f"FusedClipAdam.step: norms_out must be a contiguous CUDA f64[{len(self.groups)}]")
        adam_clip_launch(table, len(self.groups), lr=g0["lr"] if lr is None else lr, beta1=g0["betas"][0],
                         beta2=g0["betas"][1], eps=g0["eps"], max_norm=max_norm or 0.0, step=step,
                         write_clipped_grads=self.write_clipped_grads, workspace=self._workspace, norms_out=norms_out)
        # the kernel wrote through raw pointers: tell torch, so that whatever is keyed by a parameter's version
        # (the fused kernels' weight packs, autograd's saved-tensor checks) sees the change
        if active is None:
            self._steps = [step] * len(params)
            torch.autograd.graph.increment_version(params)
        else:
            for i in active:
                self._steps[i] = step
            torch.autograd.graph.increment_version([params[i] for i in active])
        if self.write_clipped_grads:
            torch.autograd.graph.increment_version([g for g in grads if g is not None])
