"""FusedAdamW: gradient clipping + AdamW as one multi-tensor step on the gfx950 kernels (include/gmlm_hip_optim.h).

``clip_grad_norm_`` + ``torch.optim.AdamW.step`` walk the parameters many times (a norm per tensor, a norm of norms, a scaling
pass over every gradient, then about ten element-wise passes of the for-each AdamW).  ``FusedAdamW.step(max_grad_norm=...)`` is
three launches: a sum of squares per chunk of the gradients, one workgroup that turns those into norm, clip coefficient and the
skip decision, and one update pass: 32 bytes per parameter, no host synchronisation.  Differences from the stock pair:
  * ``.grad`` is NOT scaled in place: the clip coefficient is applied inside the update;
  * a step whose gradients hold an infinity or a NaN (or whose norm overflows) changes nothing, neither parameters nor moments
    nor step counts (GradScaler's skip, decided on the device); ``skipped_steps()`` counts them;
  * the per-parameter ``step`` lives in a device counter and is written into ``state`` when ``state_dict()`` asks for it.
State keys are torch's (``step``, ``exp_avg``, ``exp_avg_sq``): a state dict moves between the two optimisers either way.
"""
from __future__ import annotations

from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np
import torch

from . import _lib, ops
from ._lib import lib


def chunk_elems() -> int:
    """C, the number of elements one workgroup covers (read from the library)."""
    return int(lib().gmlm_adamw_chunk_elems())


def chunk_plan(numels: Sequence[int], chunk: Optional[int] = None) -> np.ndarray:
    """The chunk table of the header: int32 [N, 2] rows (tensor, chunk of that tensor), tensor-major, ceil(numel / C) per tensor."""
    c = chunk_elems() if chunk is None else int(chunk)
    n = np.asarray(list(numels), dtype=np.int64)
    if n.size and int(n.min()) < 1:
        raise ValueError("chunk_plan: every tensor needs at least one element")
    per = (n + c - 1) // c
    total = int(per.sum())
    if total >= 1 << 31:
        raise ValueError(f"chunk_plan: {total} chunks, the chunk table is indexed with 31 bits")
    tensor = np.repeat(np.arange(n.size, dtype=np.int64), per)
    first = np.repeat(np.cumsum(per) - per, per)
    return np.stack([tensor, np.arange(total, dtype=np.int64) - first], 1).astype(np.int32).reshape(-1, 2)


def _up16(nbytes: int) -> int:
    return (nbytes + 15) // 16 * 16


class _Plan:
    """Device tables that depend only on WHICH parameters take part (their element counts, groups and step slots)."""

    def __init__(self, numels, groups, slots, device):
        t = len(numels)
        chunks = chunk_plan(numels)
        self.num_tensors, self.num_chunks = t, int(chunks.shape[0])
        parts = [np.asarray(numels, np.int64).view(np.uint8), np.asarray(groups, np.int32).view(np.uint8),
                 np.asarray(slots, np.int32).view(np.uint8), chunks.reshape(-1).view(np.uint8)]
        offs, size = [], 0
        for part in parts:
            offs.append(size)
            size += _up16(part.size)
        host = np.zeros(size, np.uint8)
        for off, part in zip(offs, parts):
            host[off:off + part.size] = part
        self.static = torch.from_numpy(host).to(device)                 # synchronous small copy, once per set of parameters
        base = self.static.data_ptr()
        self.numel, self.group, self.slot, self.chunks = (base + o for o in offs)
        # workspaces: partial [N] f32, nonfinite [N] i32, bias_corr [T, 2] f32
        n4 = _up16(4 * self.num_chunks)
        self.work = torch.empty(2 * n4 + _up16(8 * t), dtype=torch.uint8, device=device)
        self.partial = self.work.data_ptr()
        self.nonfinite = self.partial + n4
        self.bias_corr = self.nonfinite + n4
        self.addr_bytes = _up16(32 * t)


class FusedAdamW(torch.optim.Optimizer):
    """``torch.optim.AdamW`` (decoupled weight decay) with ``clip_grad_norm_`` folded in, on the HIP kernels.

    Parameters are fp32, contiguous and on one device; ``amsgrad`` and ``maximize`` are not supported (``ValueError``).
    ``step(max_grad_norm=m)`` clips the global L2 norm of all gradients to ``m`` (``None``, 0 or infinity: no clipping) and
    updates every parameter whose ``.grad`` is not ``None``; a parameter that never had a gradient gets no state.  After a
    step ``last_grad_norm`` is a 0-d device tensor, a VIEW of the status block: read or clone it before the next step.
    LR schedulers work unchanged (the group table is rebuilt from ``param_groups`` at every step).  Not for hipGraph capture."""

    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=1e-2, *, amsgrad=False, maximize=False):
        if amsgrad:
            raise ValueError("FusedAdamW does not support amsgrad")
        if maximize:
            raise ValueError("FusedAdamW does not support maximize")
        if not 0.0 <= float(lr):
            raise ValueError(f"Invalid learning rate: {lr}")
        if not 0.0 <= float(eps):
            raise ValueError(f"Invalid epsilon value: {eps}")
        if not (0.0 <= betas[0] < 1.0 and 0.0 <= betas[1] < 1.0):
            raise ValueError(f"Invalid beta parameters: {betas}")
        if not 0.0 <= float(weight_decay):
            raise ValueError(f"Invalid weight_decay value: {weight_decay}")
        # the keys (and the order) of torch.optim.AdamW's groups, so that a state dict loads into either class
        defaults = dict(lr=lr, betas=betas, eps=eps, weight_decay=weight_decay, amsgrad=False, maximize=False, foreach=None,
                        capturable=False, differentiable=False, fused=None, decoupled_weight_decay=True)
        super().__init__(params, defaults)
        self._steps: Optional[torch.Tensor] = None        # int32 [S] device step counters, S = number of parameters
        self._status: Optional[torch.Tensor] = None       # the 32-byte status block, as 8 int32
        self._plans: Dict[Tuple[int, ...], _Plan] = {}
        self._stage: List[Optional[Tuple[torch.Tensor, torch.Tensor, torch.cuda.Event]]] = [None, None]
        self._turn = 0
        self._skipped_before = 0                          # skipped steps of status blocks that were replaced (device change)
        self.last_grad_norm: Optional[torch.Tensor] = None

    def add_param_group(self, param_group):
        super().add_param_group(param_group)
        group = self.param_groups[-1]
        if group.get("amsgrad") or group.get("maximize"):
            raise ValueError("FusedAdamW does not support amsgrad or maximize")
        for p in group["params"]:
            if p.dtype != torch.float32:
                raise ValueError(f"FusedAdamW takes float32 parameters, got {p.dtype}")
            if not p.is_contiguous():
                raise ValueError(f"FusedAdamW takes contiguous parameters, got strides {tuple(p.stride())} for shape {tuple(p.shape)}")
        devices = {p.device for g in self.param_groups for p in g["params"]}
        if len(devices) > 1:
            raise ValueError(f"FusedAdamW takes parameters on one device, got {sorted(map(str, devices))}")
        if getattr(self, "_steps", None) is not None:     # slots are positions in the flattened parameter list: start over
            self._sync_steps_to_state()
            self._steps = None
        self._plans = {}

    # ------------------------------------------------------------------------------------------------------- device state
    def _params(self):
        return [p for g in self.param_groups for p in g["params"]]

    def _device_state(self, device):
        """Step counters and status block on ``device``; the counters start from whatever ``state`` holds (a loaded dict)."""
        if self._steps is not None and self._steps.device == device:
            return
        if self._status is not None:
            self._skipped_before = self.skipped_steps()
        steps = [int(self.state[p]["step"]) if "step" in self.state.get(p, {}) else 0 for p in self._params()]
        self._steps = torch.tensor(steps + [0] * (-len(steps) % 4), dtype=torch.int32).to(device)
        self._status = torch.zeros(8, dtype=torch.int32, device=device)
        self._plans, self._stage = {}, [None, None]

    def _sync_steps_to_state(self):
        if self._steps is None:
            return
        host = self._steps.cpu()                          # the one device read of state_dict()
        for i, p in enumerate(self._params()):
            if p in self.state:
                self.state[p]["step"] = torch.tensor(float(host[i]), dtype=torch.float32)

    def state_dict(self):
        self._sync_steps_to_state()
        return super().state_dict()

    def load_state_dict(self, state_dict):
        super().load_state_dict(state_dict)
        for p, st in self.state.items():
            for k in ("exp_avg", "exp_avg_sq"):
                if k in st and (st[k].dtype != torch.float32 or not st[k].is_contiguous() or st[k].shape != p.shape):
                    st[k] = st[k].to(torch.float32).contiguous().view_as(p)
            if "step" in st:
                st["step"] = torch.as_tensor(st["step"], dtype=torch.float32).detach().cpu().reshape(())
        self._steps = None                                # rebuilt from the loaded steps at the next step()
        self._plans = {}

    def skipped_steps(self) -> int:
        """Steps that changed nothing because a gradient or the norm was not finite (reads the device counter)."""
        return self._skipped_before + (0 if self._status is None else int(self._status[4]))

    # ------------------------------------------------------------------------------------------------------------ the step
    def _staging(self, nbytes: int, device):
        """Two pinned buffers taken in turn, each with the event of its last copy: a buffer is rewritten only after the copy
        that last read it has finished (by then that copy is two steps old, so the wait is normally already over)."""
        slot = self._stage[self._turn]
        if slot is None or slot[0].numel() < nbytes:
            host = torch.empty(max(nbytes, 4096), dtype=torch.uint8).pin_memory()
            slot = (host, torch.empty(host.numel(), dtype=torch.uint8, device=device), torch.cuda.Event())
            self._stage[self._turn] = slot
        else:
            slot[2].synchronize()
        self._turn ^= 1
        return slot

    @torch.no_grad()
    def step(self, closure=None, *, max_grad_norm: Optional[float] = None):
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        active, groups = [], []
        slot = 0
        for gi, group in enumerate(self.param_groups):
            for p in group["params"]:
                if p.grad is not None:
                    active.append((slot, p))
                    groups.append(gi)
                slot += 1
        if not active:
            return loss
        device = active[0][1].device
        if device.type != "cuda":
            raise _lib.GmlmHipError(f"FusedAdamW.step runs on the GPU only (parameters on {device}); there is no CPU path")
        _lib.require_gfx950(device.index if device.index is not None else torch.cuda.current_device())
        for _, p in active:
            g = p.grad
            if p.device != device or g.device != device:
                raise ValueError("FusedAdamW takes parameters and gradients on one device")
            if g.is_sparse or g.dtype != torch.float32 or not g.is_contiguous() or g.shape != p.shape:
                raise ValueError(f"FusedAdamW takes dense contiguous float32 gradients of the parameter's shape, got {g.dtype} "
                                 f"{tuple(g.shape)} strides {tuple(g.stride())}")
            if p.dtype != torch.float32 or not p.is_contiguous():
                raise ValueError("FusedAdamW takes contiguous float32 parameters")
            st = self.state[p]
            if "exp_avg" not in st:
                st["step"] = torch.tensor(0.0, dtype=torch.float32)
                st["exp_avg"] = torch.zeros_like(p, memory_format=torch.preserve_format)
                st["exp_avg_sq"] = torch.zeros_like(p, memory_format=torch.preserve_format)
            elif st["exp_avg"].device != device:
                st["exp_avg"], st["exp_avg_sq"] = st["exp_avg"].to(device), st["exp_avg_sq"].to(device)
        self._device_state(device)
        key = tuple(s for s, _ in active)
        plan = self._plans.get(key)
        if plan is None:
            if len(self._plans) >= 8:
                self._plans.clear()
            plan = self._plans[key] = _Plan([p.numel() for _, p in active], groups, list(key), device)

        # per step: the address table (gradient addresses move: zero_grad(set_to_none=True)) and the group rows
        ng = len(self.param_groups)
        nbytes = plan.addr_bytes + 64 * ng
        host, dev_buf, event = self._staging(nbytes, device)
        table = host.numpy()
        addr = table[:32 * plan.num_tensors].view(np.uint64).reshape(-1, 4)
        ptrs = []
        for _, p in active:
            st = self.state[p]
            ptrs += (p.data_ptr(), p.grad.data_ptr(), st["exp_avg"].data_ptr(), st["exp_avg_sq"].data_ptr())
        addr[:] = np.array(ptrs, dtype=np.uint64).reshape(-1, 4)
        hyper = table[plan.addr_bytes:nbytes].view(np.float64).reshape(ng, 8)
        for gi, group in enumerate(self.param_groups):
            hyper[gi] = (float(group["lr"]), float(group["weight_decay"]), float(group["betas"][0]), float(group["betas"][1]),
                         float(group["eps"]), 0.0, 0.0, 0.0)
        dev_buf[:nbytes].copy_(host[:nbytes], non_blocking=True)
        event.record()
        addr_d = dev_buf.data_ptr()
        hyper_d = addr_d + plan.addr_bytes
        mx = 0.0 if max_grad_norm is None else float(max_grad_norm)
        ops.adamw_step(addr_d, plan.numel, plan.group, plan.slot, plan.chunks, plan.num_chunks, plan.num_tensors, hyper_d, ng,
                       self._steps.data_ptr(), slot, plan.partial, plan.nonfinite, plan.bias_corr, self._status.data_ptr(), mx)
        self.last_grad_norm = self._status.view(torch.float32)[0]
        return loss
