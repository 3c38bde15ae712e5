"""The training step's update on the GPU: clip_grad_norm_ + torch.optim.Adam as two launches.

``ClipAdam(opt).step(max_norm)`` does what ``torch.nn.utils.clip_grad_norm_(params, max_norm)`` followed by
``opt.step()`` does for an ``Adam`` over fp32 CUDA tensors (train_simbev.py:245-248): it keeps the
optimizer's own state tensors (``step``, ``exp_avg``, ``exp_avg_sq``, created as torch creates them), so
``opt.state_dict()`` stays what torch would save and either path can continue the other. The gradient
norm is fp32 over all the tensors' gradients; the gradients themselves are left unclipped (nothing reads
them after the step). Kernels: ``lss_clip_adam`` (include/lss_convs.h), or
``lss_clip_adam_guarded`` when the caller passes a skip counter (a non-finite gradient then skips the step), or
``lss_clip_adam_sched`` when the ClipAdam was built with an ``LRSchedule`` and / or EMA tensors: the learning rate is
then computed on the device from Adam's own step count (so a captured update follows the schedule, a skipped step does
not advance it, and a resumed run continues it from the checkpoint's Adam state) and the exponential moving average
of the weights is written in the same pass. Anything it does not cover
(amsgrad, maximize, several parameter groups, tensor learning rates, CPU tensors, other dtypes, an Adam
that is neither ``capturable`` nor ``fused``, whose ``step`` torch keeps on the host) keeps torch's path
(``supported``).
"""
from __future__ import annotations

import ctypes
import math
from typing import Optional, Sequence

import torch

from . import _lib

USE_HIP_ADAM = True
MAX_TENSORS = 32  # LSS_ADAM_MAX_TENSORS


def supported(opt: torch.optim.Optimizer, params: Sequence[torch.Tensor]) -> bool:
    if not USE_HIP_ADAM or type(opt) is not torch.optim.Adam or len(opt.param_groups) != 1:
        return False
    g = opt.param_groups[0]
    if g.get("amsgrad") or g.get("maximize") or g.get("differentiable") or g.get("decoupled_weight_decay"):
        return False
    if not (g.get("capturable") or g.get("fused")):
        # torch keeps such an Adam's `step` on the host; the device step this path keeps would change
        # its state_dict and cost the next torch step a sync per tensor
        return False
    if any(isinstance(g[k], torch.Tensor) for k in ("lr", "eps", "weight_decay")) or \
            any(isinstance(b, torch.Tensor) for b in g["betas"]):
        return False
    ps = list(g["params"])
    if len(ps) != len(params) or any(a is not b for a, b in zip(ps, params)) or not 0 < len(ps) <= MAX_TENSORS:
        return False
    for p in ps:
        if not (p.is_cuda and p.dtype == torch.float32 and p.is_contiguous() and p.grad is not None
                and p.grad.dtype == torch.float32 and p.grad.is_contiguous() and p.grad.device == p.device):
            return False
    return True


class LRSchedule:
    """lr_t = base * factor(t): a linear warm-up over ``warmup_steps`` updates from ``warmup_factor`` to 1, times a
    decay from 1 to ``min_factor`` between ``warmup_steps`` and ``total_steps`` (constant: none; linear; cosine),
    flat at ``min_factor`` afterwards. ``t`` is Adam's step count of the update (1 for the first), s = t - 1:

        warm  = warmup_factor + (1 - warmup_factor) * min(s, W) / W        (1 without a warm-up)
        x     = clamp((s - W) / (T - W), 0, 1)
        decay = 1 | min_factor + (1 - min_factor) (1 - x) | min_factor + (1 - min_factor) * 0.5 (1 + cos(pi x))

    ``lss_clip_adam_sched`` computes the same in fp32 on the device (include/lss_convs.h) and refuses the same
    arguments; here the arithmetic is float64."""

    KINDS = ("constant", "linear", "cosine")

    def __init__(self, kind: str = "constant", warmup_steps: int = 0, warmup_factor: float = 0.0,
                 total_steps: int = 0, min_factor: float = 0.0):
        if kind not in self.KINDS:
            raise ValueError(f"LRSchedule: kind {kind!r}: one of {', '.join(self.KINDS)}")
        for name, v in (("warmup_steps", warmup_steps), ("total_steps", total_steps)):
            if isinstance(v, bool) or int(v) != v:
                raise ValueError(f"LRSchedule: {name} {v!r}: an integer")
        warmup_steps, total_steps = int(warmup_steps), int(total_steps)
        if warmup_steps < 0:
            raise ValueError(f"LRSchedule: warmup_steps {warmup_steps}: not negative")
        if not 0.0 <= float(warmup_factor) <= 1.0:
            raise ValueError(f"LRSchedule: warmup_factor {warmup_factor!r}: in [0, 1]")
        if not 0.0 <= float(min_factor) <= 1.0:
            raise ValueError(f"LRSchedule: min_factor {min_factor!r}: in [0, 1]")
        if kind != "constant" and total_steps <= warmup_steps:
            raise ValueError(f"LRSchedule: total_steps {total_steps} must exceed warmup_steps {warmup_steps} "
                             f"for a {kind} decay")
        self.kind, self.warmup_steps, self.warmup_factor = kind, warmup_steps, float(warmup_factor)
        self.total_steps, self.min_factor = total_steps, float(min_factor)

    @property
    def code(self) -> int:
        return self.KINDS.index(self.kind)

    def factor(self, t) -> float:
        """lr_t / base for the update whose Adam step count is t (>= 1)."""
        s = float(t) - 1.0
        W, T, m = float(self.warmup_steps), float(self.total_steps), self.min_factor
        warm = self.warmup_factor + (1.0 - self.warmup_factor) * min(s, W) / W if W > 0 else 1.0
        if self.kind == "constant":
            return warm
        x = min(max((s - W) / (T - W), 0.0), 1.0)
        if self.kind == "linear":
            return warm * (m + (1.0 - m) * (1.0 - x))
        return warm * (m + (1.0 - m) * 0.5 * (1.0 + math.cos(math.pi * x)))

    def lr(self, base: float, t) -> float:
        return float(base) * self.factor(t)

    def __repr__(self) -> str:
        return (f"LRSchedule({self.kind!r}, warmup_steps={self.warmup_steps}, warmup_factor={self.warmup_factor}, "
                f"total_steps={self.total_steps}, min_factor={self.min_factor})")


class ClipAdam:
    def __init__(self, opt: torch.optim.Adam, schedule: Optional[LRSchedule] = None,
                 ema: Optional[Sequence[torch.Tensor]] = None, ema_decay: float = 0.999, ema_warmup: bool = True):
        """schedule: an LRSchedule the device evaluates from Adam's step count (``param_groups[0]["lr"]`` stays the
        base rate). ema: one fp32 tensor per parameter, created by the caller (e.g. FlatParams.enable_ema), updated
        in the Adam pass as e += (1 - d) (p_new - e), d = min(ema_decay, (1 + t) / (10 + t)) with ema_warmup, else
        ema_decay. With neither, ``step`` calls what it always called. ``self.lr``: one fp32 on the device, the
        learning rate of the last applied update (tensor 0's); allocated here, so its address is fixed before any
        capture."""
        self.opt = opt
        self._partial = None
        self.schedule = schedule
        self.ema = None if ema is None else list(ema)
        self.ema_decay, self.ema_warmup = float(ema_decay), bool(ema_warmup)
        self.lr = None
        if schedule is not None or self.ema is not None:
            if schedule is not None and not isinstance(schedule, LRSchedule):
                raise TypeError("ClipAdam: schedule must be an optim.LRSchedule")
            if not 0.0 <= self.ema_decay < 1.0:
                raise ValueError(f"ClipAdam: ema_decay {ema_decay!r}: in [0, 1)")
            ps = list(opt.param_groups[0]["params"])
            if self.ema is not None:
                if len(self.ema) != len(ps):
                    raise ValueError(f"ClipAdam: {len(self.ema)} EMA tensors for {len(ps)} parameters")
                for e, p in zip(self.ema, ps):
                    if not (e.device == p.device and e.dtype == torch.float32 and e.is_contiguous()
                            and e.numel() == p.numel() and not e.requires_grad):
                        raise ValueError("ClipAdam: each EMA tensor must be a contiguous fp32 tensor of its "
                                         "parameter's size on its device, without requires_grad")
            self.lr = torch.zeros((), device=ps[0].device, dtype=torch.float32)

    def _state(self, p: torch.Tensor):
        st = self.opt.state[p]
        if len(st) == 0:  # as torch.optim.Adam initialises it (fused / capturable: the step on the device)
            st["step"] = torch.zeros((), dtype=torch.float32, device=p.device)
            st["exp_avg"] = torch.zeros_like(p, memory_format=torch.preserve_format)
            st["exp_avg_sq"] = torch.zeros_like(p, memory_format=torch.preserve_format)
        elif st["step"].device != p.device or st["step"].dtype != torch.float32:
            st["step"] = st["step"].to(device=p.device, dtype=torch.float32)
        return st

    def step(self, max_norm: float, skipped: Optional[torch.Tensor] = None) -> None:
        """skipped (one int32 on the device): the guarded update, ``lss_clip_adam_guarded`` -- a step whose
        gradient norm is a NaN or an infinity writes nothing and adds one to it; a finite step is the same
        update bit for bit. None: torch's behaviour (a non-finite gradient poisons every parameter)."""
        lib = _lib.load()
        g = self.opt.param_groups[0]
        ps = list(g["params"])
        n = len(ps)
        sts = [self._state(p) for p in ps]
        dev = ps[0].device
        if self._partial is None or self._partial.device != dev:
            self._partial = torch.empty(int(lib.lss_clip_adam_partials()), device=dev, dtype=torch.float32)
        arr = lambda ts: (ctypes.c_void_p * n)(*[t.data_ptr() for t in ts])  # noqa: E731
        numel = (ctypes.c_int64 * n)(*[p.numel() for p in ps])
        b1, b2 = g["betas"]
        if skipped is not None:
            if not (skipped.is_cuda and skipped.device == dev and skipped.dtype == torch.int32 and skipped.numel() == 1):
                raise RuntimeError("ClipAdam.step: skipped must be one int32 on the parameters' device")
        if self.lr is not None:  # a schedule and / or EMA: lss_clip_adam_sched, guarded or not
            sc = self.schedule or LRSchedule()
            _lib.check(lib.lss_clip_adam_sched(
                n, arr(ps), arr([p.grad for p in ps]), arr([s["exp_avg"] for s in sts]),
                arr([s["exp_avg_sq"] for s in sts]), arr([s["step"] for s in sts]), numel, float(max_norm),
                float(g["lr"]), float(b1), float(b2), float(g["eps"]), float(g["weight_decay"]),
                _lib.ptr(self._partial), None if skipped is None else _lib.ptr(skipped), sc.code, sc.warmup_steps,
                sc.warmup_factor, sc.total_steps, sc.min_factor, _lib.ptr(self.lr),
                None if self.ema is None else arr(self.ema), self.ema_decay, int(self.ema_warmup),
                _lib.stream_handle(dev)), "lss_clip_adam_sched")
            return
        if skipped is not None:
            _lib.check(lib.lss_clip_adam_guarded(
                n, arr(ps), arr([p.grad for p in ps]), arr([s["exp_avg"] for s in sts]),
                arr([s["exp_avg_sq"] for s in sts]), arr([s["step"] for s in sts]), numel, float(max_norm),
                float(g["lr"]), float(b1), float(b2), float(g["eps"]), float(g["weight_decay"]),
                _lib.ptr(self._partial), _lib.ptr(skipped), _lib.stream_handle(dev)), "lss_clip_adam_guarded")
            return
        _lib.check(lib.lss_clip_adam(n, arr(ps), arr([p.grad for p in ps]), arr([s["exp_avg"] for s in sts]),
                                     arr([s["exp_avg_sq"] for s in sts]), arr([s["step"] for s in sts]), numel,
                                     float(max_norm), float(g["lr"]), float(b1), float(b2), float(g["eps"]),
                                     float(g["weight_decay"]), _lib.ptr(self._partial), _lib.stream_handle(dev)),
                   "lss_clip_adam")
