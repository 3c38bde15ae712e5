"""The training step of train_simbev.py:229-248 -- forward, SimpleLoss, backward,
clip_grad_norm_(max_grad_norm), Adam -- eager, or replayed as two HIP graphs.

A B=8 step launches ~2000 kernels (conv stacks, BN, the lift/splat path, optimizer); eager, the
host's Python + launch cost per kernel is longer than many of the kernels, so the GPU idles.
Captured (``torch.cuda.CUDAGraph``, i.e. hipGraph), the step is two graph launches:

  graph A  forward under bf16 autocast, loss, backward
  (eager)  all-reduce of the gradients over RCCL (world size > 1)
  graph B  divide by the world size, clip_grad_norm_, fused Adam (capturable)

With ``overlap_all_reduce`` (and ``flat_params.FlatParamGroups``: one master per parameter group, in
the order the backward completes them) each group's all-reduce starts from its post-accumulate hook
on a side stream while the backward continues, captured into graph A; the eager all-reduce between
the graphs is then skipped.

With ``flat_params.FlatParams`` the trainable parameters are one fp32 tensor, so the gradient is one
tensor too: one ~50 MB ring all-reduce over xGMI per step (the same averaged gradient as DDP), a
single-tensor Adam and norm. Every op of the LSS path is capturable: its kernels take device
pointers only and the plan's sizes come from the static shapes; the one host round trip of the
reference (torch.inverse on the CPU, src/models.py:180,186) moves out of the captured region:
``pre_step`` inverts the host copy of the rig with the same call and stages the results into static
device buffers (ops.HostInverses) before each replay, so the captured step reads bit-identical
inverses. (A device fp64 adjugate inverse, not bit-exact, was removed in round 4 with the other
off-by-default options; its measurements stay in profiles/r03.)
"""
from __future__ import annotations

import time
from typing import Callable, Optional, Sequence

import torch
import torch.distributed as dist


def _with_inverses(model, inverses, forward, inputs):
    """forward(*inputs) with `inverses` installed as model.static_inverses (None: nothing is touched), the
    previous value restored afterwards, as predict.Predictor._forward does."""
    if inverses is None:
        return forward(*inputs)
    saved = model.static_inverses
    model.static_inverses = inverses
    try:
        return forward(*inputs)
    finally:
        model.static_inverses = saved


class TrainStep:
    """forward(*inputs) -> preds; params: what the optimizer updates (e.g. [FlatParams.master]);
    all_reduce: average params' gradients over the process group here (False under DDP)."""

    def __init__(self, forward: Callable[..., torch.Tensor], inputs: Sequence[torch.Tensor], labels: torch.Tensor,
                 loss_fn: Callable, opt: torch.optim.Optimizer, params: Sequence[torch.Tensor],
                 all_reduce: bool = False, amp_dtype: Optional[torch.dtype] = torch.bfloat16,
                 max_grad_norm: float = 5.0, pre_step: Optional[Callable[[], None]] = None,
                 overlap_all_reduce: bool = False, force_collectives: bool = False,
                 skip_nonfinite: bool = False, keep_preds: bool = False, lr_schedule=None, ema=None,
                 ema_decay: float = 0.999, ema_warmup: bool = True, valid: Optional[torch.Tensor] = None,
                 inverses=None, model: Optional[torch.nn.Module] = None):
        """overlap_all_reduce: all-reduce each parameter's gradient (e.g. each FlatParamGroups
        master) from its post-accumulate hook, on a side stream, while the backward continues -- inside
        the captured graph too; the step waits for them before the update. force_collectives: issue
        the collectives even at world size 1 (tests of the captured path on one GPU). skip_nonfinite: a
        step whose gradient norm is a NaN or an infinity leaves parameters and optimizer state untouched
        and is counted in ``self.skipped`` (one int32 on the device; needs the HIP update, optim.supported).
        keep_preds: keep the step's detached logits as ``self.static_preds`` (captured: a static tensor
        every replay rewrites), for the caller's training IoU. lr_schedule (an optim.LRSchedule): the update
        computes the learning rate on the device from Adam's step count, so replays follow it (``self.lr``: the
        last applied rate, one fp32 on the device); ema: one fp32 tensor per entry of params (e.g.
        FlatParamGroups.enable_ema()), averaged in the Adam pass with ema_decay / ema_warmup (optim.ClipAdam).
        Either needs the HIP update, as skip_nonfinite does. valid: the static (B, X, Y) uint8 valid-cell mask (e.g.
        ``BatchStager.valid``): the step then calls ``loss_fn(preds, labels, valid)`` -- tools.SimpleLoss / FocalLoss
        average over the valid cells only. The step stays captured: the mask is read on the device and so is the count
        of valid elements. inverses: a (pinv, kinv) pair of static device buffers (ops.HostInverses) installed as
        ``model.static_inverses`` around this step's forward and restored afterwards (it needs ``model``) -- a step
        whose inputs have another camera count than the module's other steps brings its own; None: the module's
        attribute as it stands."""
        self.forward, self.inputs, self.labels = forward, tuple(inputs), labels
        self.valid = valid
        if inverses is not None and model is None:
            raise ValueError("TrainStep(inverses=...) needs model=: the module whose static_inverses it installs")
        self.inverses, self.model = (None if inverses is None else tuple(inverses)), model
        # host work staged into the step's static device inputs before each step is launched
        # (e.g. ops.HostInverses.update: the reference's host torch.inverse of the rig)
        self.pre_step = pre_step
        self.loss_fn, self.opt, self.params = loss_fn, opt, list(params)
        self.amp_dtype, self.max_grad_norm = amp_dtype, max_grad_norm
        on = all_reduce and dist.is_available() and dist.is_initialized()
        self.world = dist.get_world_size() if on else 1
        self.collectives = on and (self.world > 1 or force_collectives)
        self.overlap = bool(overlap_all_reduce) and self.collectives
        self._works = []
        self._side = None
        if self.overlap:
            for p in self.params:
                p.register_post_accumulate_grad_hook(self._reduce_ready)
        self.graphs = None
        self.graph_grads = None
        self.static_loss = None
        self.keep_preds, self.static_preds = bool(keep_preds), None
        self.skipped = torch.zeros(1, device=labels.device, dtype=torch.int32) if skip_nonfinite else None
        self.lr_schedule, self.ema = lr_schedule, (None if ema is None else list(ema))
        self.ema_decay, self.ema_warmup = ema_decay, ema_warmup
        self._clip_adam = None

    @property
    def lr(self) -> Optional[torch.Tensor]:
        """The device scalar holding the last applied learning rate (a schedule or EMA asked for, after the
        first update); None otherwise."""
        return None if self._clip_adam is None else self._clip_adam.lr

    @property
    def captured(self) -> bool:
        return self.graphs is not None

    def forward_backward(self) -> torch.Tensor:
        self.opt.zero_grad(set_to_none=True)  # backward's gradient is stolen, not accumulated
        dev_type = self.labels.device.type
        # autocast's cast cache must be off while capturing (its entries would outlive the capture)
        capturing = dev_type == "cuda" and torch.cuda.is_current_stream_capturing()
        with torch.autocast(dev_type, dtype=self.amp_dtype or torch.bfloat16, enabled=self.amp_dtype is not None,
                            cache_enabled=not capturing):
            preds = _with_inverses(self.model, self.inverses, self.forward, self.inputs)
        if self.keep_preds:
            self.static_preds = preds.detach()
        # (a loss that computes in fp32 itself, tools.SimpleLoss, takes the bf16 logits: no cast kernels)
        logits = preds if getattr(self.loss_fn, "computes_in_fp32", False) else preds.float()
        loss = self.loss_fn(logits, self.labels) if self.valid is None else self.loss_fn(logits, self.labels, self.valid)
        loss.backward()
        if self.overlap:  # the collectives the hooks started: the update waits for them
            for w in self._works:
                w.wait()
            if self._side is not None:
                torch.cuda.current_stream(self.labels.device).wait_stream(self._side)
            self._works = []
        return loss

    def _reduce_ready(self, p: torch.Tensor) -> None:
        """post-accumulate-grad hook: p.grad is final; start its all-reduce beside the backward."""
        if p.grad is None:
            return
        if p.grad.is_cuda:
            dev = p.grad.device
            if self._side is None:
                self._side = torch.cuda.Stream(dev)
            self._side.wait_stream(torch.cuda.current_stream(dev))
            with torch.cuda.stream(self._side):
                self._works.append(dist.all_reduce(p.grad, async_op=True))
        else:
            self._works.append(dist.all_reduce(p.grad, async_op=True))

    def all_reduce(self, grads=None) -> None:
        """Sum the gradients over ranks (eager: outside any capture); no-op when the hooks did it."""
        if self.collectives and not self.overlap:
            for g in (grads if grads is not None else [p.grad for p in self.params]):
                if g is not None:
                    dist.all_reduce(g)

    def update(self) -> None:
        if self.world > 1:
            for p in self.params:
                if p.grad is not None:
                    p.grad.mul_(1.0 / self.world)
        from . import optim
        if optim.supported(self.opt, self.params):  # both in two launches on the GPU (lss_clip_adam)
            if self._clip_adam is None or self._clip_adam.opt is not self.opt:
                self._clip_adam = optim.ClipAdam(self.opt, schedule=self.lr_schedule, ema=self.ema,
                                                 ema_decay=self.ema_decay, ema_warmup=self.ema_warmup)
            self._clip_adam.step(self.max_grad_norm, skipped=self.skipped)
            return
        if self.lr_schedule is not None or self.ema is not None:
            raise RuntimeError("TrainStep(lr_schedule=..., ema=...) needs the HIP update (a fused / capturable "
                               "torch.optim.Adam over fp32 device tensors, optim.supported)")
        if self.skipped is not None:
            raise RuntimeError("TrainStep(skip_nonfinite=True) needs the HIP update (a fused / capturable "
                               "torch.optim.Adam over fp32 device tensors, optim.supported)")
        torch.nn.utils.clip_grad_norm_(self.params, self.max_grad_norm)
        self.opt.step()

    def eager(self) -> torch.Tensor:
        if self.pre_step is not None:
            self.pre_step()
        loss = self.forward_backward()
        self.all_reduce()
        self.update()
        return loss

    def capture(self, warmup: int = 2, on_warmup: Optional[Callable[[int], None]] = None,
                error_mode: Optional[str] = None) -> None:
        """`warmup` eager steps on a side stream (MIOpen find, optimizer state, allocator), then
        capture (the optimizer must be built with capturable=True). error_mode: the capture's
        capture_error_mode ("thread_local" when other threads of the process use the runtime meanwhile,
        e.g. a DataLoader's pinning thread); None: "global", or "thread_local" with collectives."""
        dev = self.labels.device
        side = torch.cuda.Stream(dev)
        side.wait_stream(torch.cuda.current_stream(dev))
        with torch.cuda.stream(side):
            for i in range(max(warmup, 1)):
                self.eager()
                if on_warmup is not None:
                    on_warmup(i)
        torch.cuda.current_stream(dev).wait_stream(side)
        torch.cuda.synchronize(dev)
        mode = "global"
        if self.collectives:
            # the process group's watchdog thread polls the warm-up's all-reduce events (every 100 ms)
            # until it reaps them; one such query during a global-mode capture aborts the process
            # ("operation not permitted when stream is capturing", seen in a world-size-1 RCCL run).
            # Let it reap the completed works, and restrict the capture's checks to this thread.
            time.sleep(0.5)
            mode = "thread_local"
        mode = error_mode or mode
        g_fb, g_up = torch.cuda.CUDAGraph(), torch.cuda.CUDAGraph()
        with torch.cuda.graph(g_fb, capture_error_mode=mode):
            # detached: holding the captured autograd graph would keep its AccumulateGrad nodes
            # (bound to the capture stream) alive into later eager steps. The gradients allocated
            # here (graph pool) are what graph B and the all-reduce read on every replay.
            self.static_loss = self.forward_backward().detach()
        self.graph_grads = [p.grad for p in self.params]
        with torch.cuda.graph(g_up, pool=g_fb.pool(), capture_error_mode=mode):
            self.update()
        self.graphs = (g_fb, g_up)

    def __call__(self) -> torch.Tensor:
        if self.graphs is None:
            return self.eager()
        g_fb, g_up = self.graphs
        if self.pre_step is not None:
            self.pre_step()
        g_fb.replay()  # with overlap_all_reduce the collectives are inside this graph
        self.all_reduce(self.graph_grads)
        g_up.replay()
        return self.static_loss


class EvalStep:
    """The validation step of get_val_info (src/tools.py:243-270) over static inputs: forward only, the
    model in eval mode, no_grad, the training step's autocast dtype, then ``tools.val_accumulate`` into
    ``totals`` (1 + 2 K float64 on the device for K = labels.shape[1] classes: loss x samples, the K
    intersections, the K unions; K = 1: the reference's three) -- eager, or one HIP graph.

    forward: the callable the training step runs (e.g. ``FlatParams.bind(model)``: every call, and every
    replay, materialises the current masters). n_valid (one int32 on the device, e.g.
    ``BatchStager.n_valid``): how many leading samples of the static batch count; it is read on the
    device, so one graph serves full and partial batches. The training graphs are not affected by the
    module's mode flag: a captured graph replays the kernels it recorded."""

    def __init__(self, model: torch.nn.Module, forward: Callable[..., torch.Tensor], inputs: Sequence[torch.Tensor],
                 labels: torch.Tensor, n_valid: Optional[torch.Tensor] = None, pos_weight=2.13,
                 amp_dtype: Optional[torch.dtype] = torch.bfloat16, n_samples: Optional[int] = None,
                 loss=None, thresholds=None, valid: Optional[torch.Tensor] = None, inverses=None):
        """loss: a tools.FocalLoss whose term the loss total sums (its ``focal_params`` buffer is read on the device;
        None: SimpleLoss(pos_weight)). thresholds: a ladder of probability thresholds to count the IoU at. With
        either, the step accumulates through ``tools.seg_metrics_accumulate`` (``lss_seg_metrics_accum``) at the
        ladder and 0.5, sorted, into 1 + K + 2 K T totals; ``read()`` keeps its keys -- the IoU from the 0.5 column --
        and, for a ladder, adds ``tools.seg_metrics_summary``'s. With neither, nothing differs from before.
        valid: the static (B, X, Y) uint8 valid-cell mask (e.g. ``BatchStager.valid``): the step always accumulates
        through the seg-metrics path (the 0.5 column present), masked -- ``lss_seg_metrics_accum_masked`` -- so the loss
        and every IoU are over valid cells, and ``read()`` adds ``valid_fraction``: valid cells / cells, over the
        samples counted. inverses: as TrainStep's -- installed as ``model.static_inverses`` around the forward.
        loss a tools.SoftmaxLoss (``exclusive``): labels is the (B, X, Y) uint8 class map and the step accumulates
        through ``tools.confusion_accumulate`` (``lss_confusion_accum``) into 1 + C C totals with the loss's
        ``class_weight`` buffer, masked when valid is given; ``read()`` returns ``tools.confusion_summary``'s dict.
        thresholds= with such a loss is a ValueError: an argmax has no threshold."""
        self.exclusive = bool(getattr(loss, "exclusive", False))
        if self.exclusive:
            if thresholds is not None:
                raise ValueError("EvalStep: thresholds= with an exclusive loss (the prediction is an argmax)")
            self.model, self.forward, self.inputs, self.labels = model, forward, tuple(inputs), labels
            self.inverses = None if inverses is None else tuple(inverses)
            self.n_samples, self.n_valid, self.amp_dtype = n_samples, n_valid, amp_dtype
            self.classes = int(loss.classes)
            w = loss.class_weight
            self.class_weight = w if w.device == labels.device else w.to(labels.device)
            self.totals = torch.zeros(1 + self.classes ** 2, device=labels.device, dtype=torch.float64)
            self.ladder = self.columns = self.params = self.thetas = self.valid_cells = None
            self.valid = valid
            self.graph = None
            self.static_preds = None
            return
        self.model, self.forward, self.inputs, self.labels = model, forward, tuple(inputs), labels
        self.inverses = None if inverses is None else tuple(inverses)
        self.n_samples = n_samples  # len(valloader.dataset): what read() divides the loss total by
        self.n_valid, self.amp_dtype = n_valid, amp_dtype
        # K = labels.shape[1] classes: 1 + 2 K totals (loss, K intersections, K unions) and, for K > 1 or a
        # sequence of weights, the class weights as a device buffer made here, outside any capture
        self.classes = int(labels.shape[1]) if labels.dim() >= 2 else 1
        from . import tools
        if self.classes > 1 or not tools.is_scalar_weight(pos_weight):
            self.pos_weight = tools.class_weights(pos_weight, self.classes, labels.device)
        else:
            self.pos_weight = float(pos_weight)
        self.totals = torch.zeros(1 + 2 * self.classes, device=labels.device, dtype=torch.float64)
        self.ladder = None if thresholds is None else [float(v) for v in thresholds]
        self.columns = self.params = self.thetas = None
        self.valid = valid
        self.valid_cells = None if valid is None else torch.zeros(1, device=labels.device, dtype=torch.float64)
        if loss is not None or thresholds is not None or valid is not None:
            from .predict import threshold_logit
            K, dev = self.classes, labels.device
            self.columns = sorted(set((self.ladder or []) + [0.5]))
            if not 1 <= len(self.columns) <= 16:
                raise ValueError(f"EvalStep: {len(self.columns)} thresholds (0.5 included); at most 16")
            self.thetas = torch.tensor([threshold_logit(v) for v in self.columns], device=dev, dtype=torch.float32)
            if loss is not None:
                params = getattr(loss, "focal_params", None)
                if params is None or tuple(params.shape) != (K, 3):
                    raise ValueError(f"EvalStep: loss must be a tools.FocalLoss of {K} classes")
                self.params = params if params.device == dev else params.to(dev)
            else:
                w = tools.class_weights(pos_weight, K, dev)
                self.params = torch.stack([w, torch.ones_like(w), torch.zeros_like(w)], dim=1).contiguous()
            self.totals = torch.zeros(1 + K + 2 * K * len(self.columns), device=dev, dtype=torch.float64)
        self.graph = None
        self.static_preds = None

    @property
    def captured(self) -> bool:
        return self.graph is not None

    def eager(self) -> None:
        from . import tools
        was_training = self.model.training
        self.model.eval()
        try:
            dev_type = self.labels.device.type
            capturing = dev_type == "cuda" and torch.cuda.is_current_stream_capturing()
            with torch.no_grad():
                with torch.autocast(dev_type, dtype=self.amp_dtype or torch.bfloat16,
                                    enabled=self.amp_dtype is not None, cache_enabled=not capturing):
                    preds = _with_inverses(self.model, self.inverses, self.forward, self.inputs)
                self.static_preds = preds
                if self.exclusive:
                    tools.confusion_accumulate(preds, self.labels, self.totals, self.n_valid, self.class_weight,
                                               valid=self.valid)
                elif self.columns is None:
                    tools.val_accumulate(preds, self.labels, self.totals, n_valid=self.n_valid,
                                         pos_weight=self.pos_weight)
                else:
                    tools.seg_metrics_accumulate(preds, self.labels, self.totals, self.n_valid, self.params,
                                                 self.thetas, valid=self.valid, valid_cells=self.valid_cells)
        finally:
            self.model.train(was_training)

    def capture(self, warmup: int = 1, error_mode: str = "global") -> None:
        """`warmup` eager steps on a side stream, then capture; the totals are reset afterwards and the
        module's mode is what it was. error_mode: as TrainStep.capture's."""
        dev = self.labels.device
        side = torch.cuda.Stream(dev)
        side.wait_stream(torch.cuda.current_stream(dev))
        with torch.cuda.stream(side):
            for _ in range(max(warmup, 1)):
                self.eager()
        torch.cuda.current_stream(dev).wait_stream(side)
        torch.cuda.synchronize(dev)
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, capture_error_mode=error_mode):
            self.eager()
        self.graph = g
        self.reset()

    def __call__(self) -> None:
        if self.graph is None:
            self.eager()
        else:
            self.graph.replay()

    def reset(self) -> None:
        self.totals.zero_()
        if self.valid_cells is not None:
            self.valid_cells.zero_()

    def read(self, n_samples: Optional[int] = None) -> dict:
        """get_val_info's dict {"loss", "iou", "iou_per_class"}: the loss total over ``n_samples``
        (``len(valloader.dataset)``; default: the constructor's), intersection / union per class (None for a
        class with an empty union) and their mean over the classes seen -- for one class the reference's
        intersection / union; every union empty raises ZeroDivisionError, as the reference's does. The one
        host read of a validation pass."""
        from . import tools
        t = self.totals.tolist()
        K = self.classes
        n = self.n_samples if n_samples is None else n_samples
        if self.exclusive:  # (valid_fraction: counted cells over the cells of the samples counted, with a mask)
            cells = None if self.valid is None or not n else n * (self.valid.numel() // self.valid.shape[0])
            return tools.confusion_summary(t, K, n, cells=cells)
        if self.columns is None:
            return {"loss": t[0] / n, **tools.iou_summary(t[1:1 + K], t[1 + K:1 + 2 * K])}
        # the ladder's totals: intersection = TP, union = PP + P - TP, at the 0.5 column for today's keys
        P, TP, PP = tools.seg_metrics_counts(t, K, len(self.columns))
        c = self.columns.index(0.5)
        info = {"loss": t[0] / n, **tools.iou_summary([TP[k][c] for k in range(K)],
                                                      [PP[k][c] + P[k] - TP[k][c] for k in range(K)])}
        if self.ladder is not None:
            cols = [self.columns.index(v) for v in self.ladder]
            sub = t[:1 + K] + [TP[k][j] for k in range(K) for j in cols] + [PP[k][j] for k in range(K) for j in cols]
            extra = tools.seg_metrics_summary(sub, K, self.ladder, n)
            info.update({k: v for k, v in extra.items() if k != "loss"})
        if self.valid is not None:  # valid cells over the cells of the samples counted
            info["valid_fraction"] = float(self.valid_cells.item()) / (n * (self.valid.numel() // self.valid.shape[0]))
        return info
