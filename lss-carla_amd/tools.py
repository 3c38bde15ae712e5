"""Training-side helpers with the reference's names (src/tools.py).

What the LiftSplatShoot training step and its callers use: the grid helper, the op-level
segmented sum (``QuickCumsum`` / ``cumsum_trick``, HIP-backed), the loss and the IoU metric. The
reference's nuScenes/visualisation helpers are out of scope; its
image/label helpers live in ``simbev.py``.
"""
from __future__ import annotations

import torch


def gen_dx_bx(xbound, ybound, zbound):
    """Cell size, first-cell centre and cell count per axis (src/tools.py:174-179)."""
    rows = (xbound, ybound, zbound)
    dx = torch.tensor([r[2] for r in rows], dtype=torch.float32)
    bx = torch.tensor([r[0] + r[2] / 2.0 for r in rows], dtype=torch.float32)
    nx = torch.tensor([int((r[1] - r[0]) / r[2]) for r in rows], dtype=torch.long)
    return dx, bx, nx


# ----------------------------------------------------------------------------- op-level segmented sum
class QuickCumsum(torch.autograd.Function):
    """``QuickCumsum.apply(x, geom_feats, ranks)`` of src/tools.py:193-219 on HIP kernels.

    x (n, C) rows sorted by ``ranks`` (n,) int64; geom_feats (n, k) int64. Returns one row per run
    of equal ranks: (x_seg (nseg, C), geom_seg (nseg, k)) with geom_seg = the geom_feats row of the
    run's last row, as the reference's ``geom_feats[kept]``. Forward: lss_segment_build +
    lss_segment_sum (each run summed in row order in fp32 -- the reference differences two
    fp32-rounded prefix sums, which is off the exact sum by ~ulp(prefix); this is not). Backward:
    lss_segment_gather, the reference's ``gradx[back]`` (identical values). The number of runs is
    read back once, as the reference's boolean indexing does. Device tensors only.
    """

    @staticmethod
    def forward(ctx, x, geom_feats, ranks):
        from . import ops
        if x.dim() != 2 or ranks.dim() != 1 or ranks.shape[0] != x.shape[0] or geom_feats.shape[0] != x.shape[0]:
            raise RuntimeError(f"QuickCumsum: x {tuple(x.shape)}, geom_feats {tuple(geom_feats.shape)} and ranks "
                               f"{tuple(ranks.shape)} do not describe the same rows")
        ops._require_cuda(x, geom_feats, ranks)
        n, C = x.shape
        if n == 0:
            seg_of = torch.empty(0, device=x.device, dtype=torch.int32)
            out, gout = x.new_empty(0, C), geom_feats.new_empty((0,) + tuple(geom_feats.shape[1:]))
        else:
            seg_of, seg_start, nseg = ops.segment_runs(ranks)
            out, gout = ops.segment_sum(x, seg_start, nseg, geom_feats)
            out = out.to(x.dtype)
        ctx.save_for_backward(seg_of)
        ctx.x_dtype = x.dtype
        ctx.mark_non_differentiable(gout)
        return out, gout

    @staticmethod
    def backward(ctx, gradx, gradgeom):
        from . import ops
        seg_of, = ctx.saved_tensors
        if seg_of.numel() == 0:
            return gradx.new_empty(0, gradx.shape[1]), None, None
        return ops.segment_gather(gradx, seg_of).to(ctx.x_dtype), None, None


def cumsum_trick(x, geom_feats, ranks):
    """src/tools.py:182-190: the same segmented sum, differentiable in x (the reference reaches the
    same gradient through autograd of cumsum / indexing / cat; here it is the gather directly)."""
    return QuickCumsum.apply(x, geom_feats, ranks)


# ----------------------------------------------------------------------------- loss / metrics
def _fused_loss(ctx, x, entry: str, head, tail, scaled: bool = False):
    """What the fused training losses share. Allocates the block partials, the loss scalar and the stored gradient,
    runs ``entry(x, dtype, *head, n, *tail, partial, loss, [scale,] grad, stream)`` (include/lss_convs.h) and saves
    the gradient for _stored_grad_backward -- `scaled`: with the device scalar n / max(M, 1) the entry's fold writes,
    and a second row of partials for its per-block counts."""
    from . import _lib
    lib = _lib.load()
    n = x.numel()
    partial = torch.empty((2 if scaled else 1) * int(lib.lss_bce_partials(n)), device=x.device, dtype=torch.float32)
    loss = torch.empty((), device=x.device, dtype=torch.float32)
    scale = (torch.empty((), device=x.device, dtype=torch.float32),) if scaled else ()
    grad = torch.empty_like(x)
    _lib.check(getattr(lib, entry)(_lib.ptr(x), _lib.dtype_code(x.dtype), *head, n, *tail, _lib.ptr(partial),
                                   _lib.ptr(loss), *(_lib.ptr(v) for v in scale), _lib.ptr(grad),
                                   _lib.stream_handle(x.device)), entry)
    ctx.save_for_backward(grad, *scale)
    return loss


def _stored_grad_backward(ctx, g) -> torch.Tensor:
    """dx = the stored gradient times the incoming one (read on the device): ``lss_bce_logits_bwd``, or, when a scale
    was saved beside the gradient, ``lss_seg_loss_masked_bwd``, which multiplies by it too."""
    from . import _lib
    grad, *scale = ctx.saved_tensors
    g = g.float().contiguous()
    dx = torch.empty_like(grad)
    entry = "lss_seg_loss_masked_bwd" if scale else "lss_bce_logits_bwd"
    _lib.check(getattr(_lib.load(), entry)(_lib.ptr(grad), _lib.dtype_code(grad.dtype), grad.numel(), _lib.ptr(g),
                                           *(_lib.ptr(v) for v in scale), _lib.ptr(dx),
                                           _lib.stream_handle(grad.device)), entry)
    return dx


class _BceLogits(torch.autograd.Function):
    """BCEWithLogitsLoss(pos_weight), mean, on ``lss_bce_logits`` (include/lss_convs.h): the loss and
    its input gradient in one pass plus a fixed-order fold of the block sums -- two launches where
    torch's decomposition runs about twenty elementwise / reduction kernels per step. The backward
    scales the stored gradient by the incoming one (``lss_bce_logits_bwd``, read on the device)."""

    @staticmethod
    def forward(ctx, x, target, pos_weight: float):
        from . import _lib
        return _fused_loss(ctx, x, "lss_bce_logits", (_lib.ptr(target),), (float(pos_weight),))

    @staticmethod
    def backward(ctx, g):
        return _stored_grad_backward(ctx, g), None, None


def is_scalar_weight(w) -> bool:
    """One pos_weight for every class (a number, a numpy scalar or a 0-d tensor: what float() took before
    per-class weights existed), as opposed to a sequence / tensor of K."""
    return isinstance(w, (int, float)) or getattr(w, "ndim", None) == 0


def _class_plane(x, K: int) -> tuple:
    """(plane, K) as the per-class entries take them, for (N, K, ...) logits: plane = the elements of one class of one
    sample."""
    return x.numel() // (x.shape[0] * K), K


class _BceLogitsPerClass(torch.autograd.Function):
    """_BceLogits with one positive-class weight per channel of (N, K, H, W) logits, ``lss_bce_logits_pc``:
    the K weights are a device buffer the kernel indexes by (i / (H W)) % K."""

    @staticmethod
    def forward(ctx, x, target, pos_weight: torch.Tensor):
        from . import _lib
        return _fused_loss(ctx, x, "lss_bce_logits_pc", (_lib.ptr(target),),
                           (*_class_plane(x, x.shape[1]), _lib.ptr(pos_weight)))

    @staticmethod
    def backward(ctx, g):
        return _stored_grad_backward(ctx, g), None, None


def masked_mean_loss(x: torch.Tensor, target: torch.Tensor, valid: torch.Tensor, params: torch.Tensor):
    """(loss, d loss / dx) of the masked loss in torch, fp32: focal_terms per element with the rows (w_pos, w_neg,
    gamma) of params (K, 3), elements whose cell has valid == 0 selected out by torch.where -- a NaN or an infinity
    there reaches neither the loss nor another element's gradient -- and the sum divided by max(M, 1), M the number
    of valid elements. valid: (batch, X, Y) (or (batch, 1, X, Y)), one plane for the K classes of a sample."""
    p = params.to(device=x.device, dtype=torch.float32)
    if p.shape[0] > 1:
        p = p.view(p.shape[0], 1, 1, 3)
    on = _broadcast_valid(valid, x)
    l, g = focal_terms(x.detach().float(), target != 0, p[..., 0], p[..., 1], p[..., 2])
    zero = torch.zeros((), device=x.device, dtype=torch.float32)
    m = on.sum().clamp(min=1).to(torch.float32)
    return torch.where(on, l, zero).sum() / m, torch.where(on, g, zero) / m


def _broadcast_valid(valid: torch.Tensor, x: torch.Tensor) -> torch.Tensor:
    """The (batch, plane) mask as booleans of x's shape (batch, K, ...)."""
    if x.dim() < 2 or valid.numel() * x.shape[1] != x.numel() or valid.shape[0] != x.shape[0]:
        raise RuntimeError(f"valid {tuple(valid.shape)} is not one plane per sample of logits {tuple(x.shape)}")
    v = (valid != 0).to(x.device).reshape(x.shape[0], 1, *x.shape[2:])
    return v.expand_as(x)


class _SegLossMaskedTorch(torch.autograd.Function):
    """The masked loss where the kernel does not apply (CPU, strided or misaligned tensors): masked_mean_loss."""

    @staticmethod
    def forward(ctx, x, target, valid, params: torch.Tensor):
        loss, g = masked_mean_loss(x, target, valid, params)
        ctx.save_for_backward(g.to(x.dtype))
        return loss

    @staticmethod
    def backward(ctx, g):
        (grad,) = ctx.saved_tensors
        return (grad.float() * g.float()).to(grad.dtype), None, None, None


class _SegLossMasked(torch.autograd.Function):
    """``lss_seg_loss_masked``: the loss over the valid cells and its gradient over n in one pass (the count of valid
    elements M is not known yet), the fold writing n / max(M, 1) to a device scalar; the backward
    (``lss_seg_loss_masked_bwd``) multiplies by it and by the incoming gradient. params: the (K, 3) device rows; valid: (batch, plane) uint8 on the device, read there."""

    @staticmethod
    def forward(ctx, x, target, valid, params: torch.Tensor):
        from . import _lib
        return _fused_loss(ctx, x, "lss_seg_loss_masked", (_lib.ptr(target), _lib.ptr(valid)),
                           (*_class_plane(x, params.shape[0]), _lib.ptr(params)), scaled=True)

    @staticmethod
    def backward(ctx, g):
        return _stored_grad_backward(ctx, g), None, None, None


def _masked_loss(ypred, ytgt, valid, params: torch.Tensor):
    """The masked loss of SimpleLoss / FocalLoss: the kernel under their conditions (and a contiguous uint8 device
    mask), else the same formula in torch."""
    if ytgt.shape != ypred.shape:
        raise RuntimeError(f"labels {tuple(ytgt.shape)} for logits {tuple(ypred.shape)}")
    _broadcast_valid(valid, ypred)  # (the shape check)
    K = params.shape[0]
    if (ypred.is_cuda and ypred.dtype in (torch.float32, torch.bfloat16) and ytgt.dtype == torch.float32
            and ytgt.device == ypred.device and ypred.is_contiguous() and ytgt.is_contiguous()
            and ypred.data_ptr() % 16 == 0 and ytgt.data_ptr() % 16 == 0 and ypred.numel() > 0 and ypred.dim() >= 2
            and ypred.shape[1] == K and valid.dtype == torch.uint8 and valid.device == ypred.device
            and valid.is_contiguous() and params.device == ypred.device and params.dtype == torch.float32
            and params.is_contiguous()):
        return _SegLossMasked.apply(ypred, ytgt, valid, params)
    return _SegLossMaskedTorch.apply(ypred, ytgt, valid, params)


class SimpleLoss(torch.nn.Module):
    """BCE-with-logits with a positive-class weight (src/tools.py:222-230).

    On the GPU (fp32 or bf16 logits, fp32 labels of the same shape, contiguous) the loss and its
    gradient come from the fused ``lss_bce_logits`` kernel, computed in fp32 (a bf16 input gives the
    loss of its exact fp32 cast); otherwise ``loss_fn`` (the reference's ``BCEWithLogitsLoss``). The
    weight is the constructor's value (reading the module's device buffer back would synchronise)."""

    computes_in_fp32 = True  # callers may pass bf16 logits without casting them first (train_step)

    def __init__(self, pos_weight):
        """pos_weight: a float, or a sequence of K floats -- one weight per class of (N, K, H, W) logits
        (``BCEWithLogitsLoss(pos_weight=w.view(K, 1, 1))``; on the fused path ``lss_bce_logits_pc`` reads
        them from the module's device buffer ``pos_weight_classes``, so they can be changed in place
        under a captured graph)."""
        super().__init__()
        if is_scalar_weight(pos_weight):
            self.loss_fn = torch.nn.BCEWithLogitsLoss(pos_weight=torch.tensor([float(pos_weight)]))
            self.pos_weight_value = float(pos_weight)
            self.pos_weight_classes = None
        else:
            w = torch.as_tensor([float(v) for v in pos_weight], dtype=torch.float32)
            if w.numel() == 0:
                raise ValueError("SimpleLoss: pos_weight is an empty sequence")
            self.loss_fn = torch.nn.BCEWithLogitsLoss(pos_weight=w.view(-1, 1, 1))
            self.pos_weight_value = None
            self.register_buffer("pos_weight_classes", w.clone(), persistent=False)

    def masked_params(self, K: int, device) -> torch.Tensor:
        """The (K, 3) rows (pw_k, 1, 0) of the masked loss on `device`, rebuilt only when the class weights' buffer
        changed (its version) -- so a captured step builds them once, before the capture."""
        pc = self.pos_weight_classes
        key = (K, torch.device(device), None if pc is None else (pc.data_ptr(), pc._version))
        if getattr(self, "_masked_key", None) != key:
            w = class_weights(self.pos_weight_value if pc is None else pc, K, device)
            self._masked_rows = torch.stack([w, torch.ones_like(w), torch.zeros_like(w)], dim=1).contiguous()
            self._masked_key = key
        return self._masked_rows

    def forward(self, ypred, ytgt, valid=None):
        """valid: None, or the (batch, X, Y) uint8 valid-cell mask (simbev.valid_mask): the loss is then the mean
        over the valid cells' elements only -- ``lss_seg_loss_masked`` with the rows (pw, 1, 0) on the GPU, the same
        formula in torch elsewhere; labels are read as hard (t != 0)."""
        pc = self.pos_weight_classes
        if pc is not None and not (ypred.dim() == 4 and ypred.shape[1] == pc.numel()):
            raise RuntimeError(f"SimpleLoss: {pc.numel()} class weights for logits {tuple(ypred.shape)}")
        if valid is not None:
            if ypred.dim() < 2:
                raise RuntimeError(f"SimpleLoss: a mask needs (batch, K, ...) logits, got {tuple(ypred.shape)}")
            return _masked_loss(ypred, ytgt, valid, self.masked_params(int(ypred.shape[1]), ypred.device))
        if (ypred.is_cuda and ypred.dtype in (torch.float32, torch.bfloat16) and ytgt.dtype == torch.float32
                and ytgt.device == ypred.device and ytgt.shape == ypred.shape and ypred.is_contiguous()
                and ytgt.is_contiguous() and ypred.data_ptr() % 16 == 0 and ytgt.data_ptr() % 16 == 0
                and ypred.numel() > 0):
            if pc is None:
                return _BceLogits.apply(ypred, ytgt, self.pos_weight_value)
            if pc.device == ypred.device and pc.dtype == torch.float32:
                return _BceLogitsPerClass.apply(ypred, ytgt, pc)
        if pc is not None:  # (the (K, 1, 1) view of the current class weights)
            self.loss_fn.pos_weight.copy_(pc.view(-1, 1, 1))
        return self.loss_fn(ypred.float() if ypred.dtype == torch.bfloat16 else ypred, ytgt)


def focal_terms(x: torch.Tensor, q: torch.Tensor, w_pos, w_neg, gamma):
    """(l, dl/dx) of the focal loss per element, in x's dtype, from the closed form (include/lss_convs.h,
    lss_focal_logits_pc): q the boolean labels, w_pos / w_neg / gamma numbers or tensors broadcasting against x.
    exp(-gamma softplus(z)) is (1 - p_t)^gamma; nothing here divides or subtracts near-equal terms, so the
    gradient is finite where autograd through ``(1 - p_t) ** gamma`` is not (0 < gamma < 1, saturated logits)."""
    z = torch.where(q, x, -x)
    e = torch.exp(-x.abs())
    lp = torch.log1p(e)
    spz, spm = lp + z.clamp(min=0), lp + (-z).clamp(min=0)  # softplus(z), softplus(-z)
    sp, sn = 1.0 / (1.0 + e), e / (1.0 + e)                 # sigmoid(|x|), sigmoid(-|x|)
    sz, sm = torch.where(z >= 0, sp, sn), torch.where(z >= 0, sn, sp)
    mw = torch.exp(-gamma * spz) * torch.where(q, torch.as_tensor(w_pos, dtype=x.dtype, device=x.device),
                                               torch.as_tensor(w_neg, dtype=x.dtype, device=x.device))
    gz = mw * (gamma * sz * spm + sm)
    return mw * spm, torch.where(q, -gz, gz)


class _FocalTorch(torch.autograd.Function):
    """The focal loss where the kernel does not apply (CPU, strided or misaligned logits): focal_terms in fp32,
    mean over the elements, the gradient (times 1 / n) kept in the logits' type."""

    @staticmethod
    def forward(ctx, x, target, params: torch.Tensor):
        p = params.to(device=x.device, dtype=torch.float32)
        if p.shape[0] > 1:
            p = p.view(p.shape[0], 1, 1, 3)
        l, g = focal_terms(x.detach().float(), target != 0, p[..., 0], p[..., 1], p[..., 2])
        ctx.save_for_backward((g / x.numel()).to(x.dtype))
        return l.mean()

    @staticmethod
    def backward(ctx, g):
        (grad,) = ctx.saved_tensors
        return (grad.float() * g.float()).to(grad.dtype), None, None


class _FocalLogits(torch.autograd.Function):
    """``lss_focal_logits_pc``: loss and gradient in one pass plus the fold, as _BceLogitsPerClass; params is the
    (K, 3) device buffer of (w_pos, w_neg, gamma) rows, read by the kernel."""

    @staticmethod
    def forward(ctx, x, target, params: torch.Tensor):
        from . import _lib
        return _fused_loss(ctx, x, "lss_focal_logits_pc", (_lib.ptr(target),),
                           (*_class_plane(x, params.shape[0]), _lib.ptr(params)))

    @staticmethod
    def backward(ctx, g):
        return _stored_grad_backward(ctx, g), None, None


def _per_class(value, K: int, name: str) -> list:
    """K floats from a number or a sequence of K."""
    vals = [float(value)] * K if is_scalar_weight(value) else [float(v) for v in value]
    if len(vals) != K:
        raise ValueError(f"FocalLoss: {name} names {len(vals)} classes, not {K}")
    return vals


def focal_rows(classes: int, gamma=2.0, alpha=None, pos_weight=None) -> list:
    """The K rows (w_pos, w_neg, gamma) of the focal loss's parameters: focal(alpha, gamma) is
    (alpha, 1 - alpha, gamma), a pos_weight (pw, 1, gamma), neither (1, 1, gamma); SimpleLoss(pw) is (pw, 1, 0).
    gamma, alpha, pos_weight: a float or `classes` floats each."""
    K = int(classes)
    if K < 1:
        raise ValueError(f"FocalLoss: {classes!r} classes")
    if alpha is not None and pos_weight is not None:
        raise ValueError("FocalLoss: alpha and pos_weight both set the class balance: give one")
    g = _per_class(gamma, K, "gamma")
    if any(not v >= 0.0 for v in g):
        raise ValueError(f"FocalLoss: gamma {gamma!r} is negative")
    if alpha is not None:
        a = _per_class(alpha, K, "alpha")
        if any(not 0.0 < v < 1.0 for v in a):
            raise ValueError(f"FocalLoss: alpha {alpha!r} is not strictly between 0 and 1")
        return [(v, 1.0 - v, gk) for v, gk in zip(a, g)]
    w = [1.0] * K if pos_weight is None else _per_class(pos_weight, K, "pos_weight")
    return [(v, 1.0, gk) for v, gk in zip(w, g)]


class FocalLoss(torch.nn.Module):
    """Focal loss on logits for imbalanced classes: mean of (1 - p_t)^gamma x weighted BCE over hard labels
    (t != 0), per class k of (N, K, H, W) logits the row (w_pos, w_neg, gamma) of the device buffer
    ``focal_params`` (K, 3) -- changed in place, a captured step follows. On the GPU under SimpleLoss's conditions
    (fp32 or bf16 contiguous 16-B aligned logits, fp32 labels of the same shape) loss and gradient come from
    ``lss_focal_logits_pc``, computed in fp32; otherwise from the same closed form in torch (focal_terms), which
    is finite where autograd through the power is not. Drops in wherever SimpleLoss does."""

    computes_in_fp32 = True

    def __init__(self, classes: int, gamma=2.0, alpha=None, pos_weight=None):
        super().__init__()
        rows = focal_rows(classes, gamma, alpha, pos_weight)
        self.classes = len(rows)
        self.register_buffer("focal_params", torch.tensor(rows, dtype=torch.float32), persistent=False)

    def forward(self, ypred, ytgt, valid=None):
        """valid: None, or the (batch, X, Y) uint8 valid-cell mask (simbev.valid_mask): the mean is then over the
        valid cells' elements only (``lss_seg_loss_masked`` on the GPU, the same formula in torch elsewhere)."""
        K, p = self.classes, self.focal_params
        if K > 1 and not (ypred.dim() == 4 and ypred.shape[1] == K):
            raise RuntimeError(f"FocalLoss: {K} classes for logits {tuple(ypred.shape)}")
        if ytgt.shape != ypred.shape:
            raise RuntimeError(f"FocalLoss: labels {tuple(ytgt.shape)} for logits {tuple(ypred.shape)}")
        if valid is not None:
            if ypred.dim() < 2 or ypred.shape[1] != K:
                raise RuntimeError(f"FocalLoss: a mask needs (batch, {K}, ...) logits, got {tuple(ypred.shape)}")
            return _masked_loss(ypred, ytgt, valid, p)
        if (ypred.is_cuda and ypred.dtype in (torch.float32, torch.bfloat16) and ytgt.dtype == torch.float32
                and ytgt.device == ypred.device and ypred.is_contiguous() and ytgt.is_contiguous()
                and ypred.data_ptr() % 16 == 0 and ytgt.data_ptr() % 16 == 0 and ypred.numel() > 0 and ypred.dim() >= 1
                and p.device == ypred.device and p.dtype == torch.float32 and p.is_contiguous()):
            return _FocalLogits.apply(ypred, ytgt, p)
        return _FocalTorch.apply(ypred, ytgt, p)


def get_batch_iou(preds: torch.Tensor, binimgs: torch.Tensor):
    """Intersection, union and IoU of (logit > 0) vs the labels, as Python floats (src/tools.py:232-240)."""
    intersect, union = get_batch_iou_device(preds, binimgs)
    intersect, union = intersect.item(), union.item()
    return intersect, union, intersect / union if (union > 0) else 1.0


def get_batch_iou_device(preds: torch.Tensor, binimgs: torch.Tensor):
    """Same counts as device tensors, without a host sync."""
    with torch.no_grad():
        pred = preds > 0
        tgt = binimgs.bool()
        return (pred & tgt).sum().float(), (pred | tgt).sum().float()


def get_batch_iou_per_class(preds: torch.Tensor, binimgs: torch.Tensor):
    """(intersection, union) per class of (N, K, H, W) logits and labels, as float device tensors of shape
    (K,), without a host sync (the trainer's training-IoU event reads them at its own cadence)."""
    with torch.no_grad():
        pred = preds > 0
        tgt = binimgs.bool()
        return (pred & tgt).sum(dim=(0, 2, 3)).float(), (pred | tgt).sum(dim=(0, 2, 3)).float()


def iou_summary(inter, union) -> dict:
    """{"iou", "iou_per_class"} from per-class counts (sequences of numbers): inter / union per class, None
    for a class whose union is empty, and their mean over the classes with a non-empty union; every union
    empty raises ZeroDivisionError, as the reference's single division does."""
    per = [float(i) / float(u) if u > 0 else None for i, u in zip(inter, union)]
    seen = [v for v in per if v is not None]
    if len(per) == 1:
        return {"iou": float(inter[0]) / float(union[0]), "iou_per_class": per}
    if not seen:
        raise ZeroDivisionError("every class has an empty union")
    return {"iou": sum(seen) / len(seen), "iou_per_class": per}


def class_weights(pos_weight, K: int, device) -> torch.Tensor:
    """K fp32 class weights on `device` from a float, a sequence of K floats or a tensor of K."""
    if is_scalar_weight(pos_weight):
        w = torch.full((K,), float(pos_weight), device=device, dtype=torch.float32)
    elif torch.is_tensor(pos_weight):
        w = pos_weight.detach().to(device=device, dtype=torch.float32).reshape(-1)
    else:
        w = torch.tensor([float(v) for v in pos_weight], device=device, dtype=torch.float32)
    if w.numel() != K:
        raise RuntimeError(f"{w.numel()} class weights for {K} classes")
    return w.contiguous()


_VAL_PARTIAL = {}


def val_accumulate(preds: torch.Tensor, binimgs: torch.Tensor, totals: torch.Tensor, n_valid=None,
                   pos_weight=2.13) -> torch.Tensor:
    """One validation batch into get_val_info's accumulators, ``lss_bce_iou_accum`` (include/lss_convs.h):
    totals (3 float64 on the device) += (mean loss x samples, intersection, union) over the first
    ``n_valid`` samples (one int32 on the device, read there; None: all of them). preds: fp32 or bf16
    logits, binimgs: fp32 labels of the same shape. Two launches, no host synchronisation, capturable
    (the scratch is kept per device and size: one stream at a time).

    K = labels.shape[1] > 1 classes: totals is 1 + 2 K float64 -- the loss term, then the K intersections,
    then the K unions -- and pos_weight a float, K floats or a device tensor of K (pass the tensor when
    capturing: building it is a host-to-device copy), ``lss_bce_iou_accum_pc``."""
    from . import _lib
    if not (preds.is_cuda and binimgs.device == preds.device and totals.device == preds.device):
        raise RuntimeError("val_accumulate: device tensors only (no CPU fallback)")
    K = preds.shape[1] if preds.dim() >= 2 else 1
    if (binimgs.dtype != torch.float32 or binimgs.shape != preds.shape or totals.dtype != torch.float64
            or totals.numel() != 1 + 2 * K or not totals.is_contiguous() or preds.dim() < 1 or preds.numel() == 0):
        raise RuntimeError(f"val_accumulate: preds {tuple(preds.shape)} {preds.dtype}, labels {tuple(binimgs.shape)} "
                           f"{binimgs.dtype}, totals {tuple(totals.shape)} {totals.dtype}")
    if n_valid is not None and not (n_valid.device == preds.device and n_valid.dtype == torch.int32
                                    and n_valid.numel() == 1):
        raise RuntimeError("val_accumulate: n_valid must be one int32 on the logits' device")
    lib = _lib.load()
    x, t = preds.detach().contiguous(), binimgs.contiguous()
    batch = x.shape[0]
    per_sample = x.numel() // batch
    per_class = K > 1 or not is_scalar_weight(pos_weight)
    nbytes = int(lib.lss_bce_iou_pc_partial_bytes(x.numel(), K) if per_class else
                 lib.lss_bce_iou_partial_bytes(x.numel()))
    key = (x.device, nbytes)
    partial = _VAL_PARTIAL.get(key)
    if partial is None:
        partial = _VAL_PARTIAL[key] = torch.empty(nbytes // 8, device=x.device, dtype=torch.float64)
    if per_class:
        w = class_weights(pos_weight, K, x.device)
        _lib.check(lib.lss_bce_iou_accum_pc(_lib.ptr(x), _lib.dtype_code(x.dtype), _lib.ptr(t), per_sample, batch,
                                            _lib.ptr(n_valid), per_sample // K, K, _lib.ptr(w), _lib.ptr(totals),
                                            _lib.ptr(partial), _lib.stream_handle(x.device)), "lss_bce_iou_accum_pc")
        return totals
    _lib.check(lib.lss_bce_iou_accum(_lib.ptr(x), _lib.dtype_code(x.dtype), _lib.ptr(t), per_sample, batch,
                                     _lib.ptr(n_valid), float(pos_weight), _lib.ptr(totals), _lib.ptr(partial),
                                     _lib.stream_handle(x.device)), "lss_bce_iou_accum")
    return totals


def seg_metrics_accumulate(preds: torch.Tensor, binimgs: torch.Tensor, totals: torch.Tensor, n_valid, params: torch.Tensor,
                           thetas: torch.Tensor, valid=None, valid_cells=None) -> torch.Tensor:
    """One validation batch into the accumulators of a threshold ladder, ``lss_seg_metrics_accum``
    (include/lss_convs.h): params the (K, 3) fp32 device rows (w_pos, w_neg, gamma) of the loss term
    (FocalLoss.focal_params; (pw, 1, 0) is SimpleLoss), thetas T ascending fp32 logit thresholds on the device.
    totals (1 + K + 2 K T float64 on the device) += the loss term, P_k, TP_kj, PP_kj over the first ``n_valid``
    samples (one int32 on the device; None: all). Device tensors only; two launches, no host synchronisation,
    capturable (the scratch is kept per device and size, as val_accumulate's).

    valid: the (batch, X, Y) uint8 device valid-cell mask (simbev.valid_mask) -- ``lss_seg_metrics_accum_masked``: only
    valid cells of the first n_valid samples are counted, and totals[0] += n_valid x the mean loss over their
    elements; valid_cells (one float64 on the device, optional) += the number of valid cells counted."""
    from . import _lib
    if not (preds.is_cuda and all(v.device == preds.device for v in (binimgs, totals, params, thetas))):
        raise RuntimeError("seg_metrics_accumulate: device tensors only (no CPU fallback)")
    K = preds.shape[1] if preds.dim() >= 2 else 1
    T = thetas.numel()
    if (binimgs.dtype != torch.float32 or binimgs.shape != preds.shape or totals.dtype != torch.float64
            or not 1 <= T <= 16 or not 1 <= K <= 32 or totals.numel() != 1 + K + 2 * K * T
            or not totals.is_contiguous() or preds.numel() == 0 or tuple(params.shape) != (K, 3)
            or params.dtype != torch.float32 or thetas.dtype != torch.float32 or not params.is_contiguous()
            or not thetas.is_contiguous()):
        raise RuntimeError(f"seg_metrics_accumulate: preds {tuple(preds.shape)} {preds.dtype}, labels "
                           f"{tuple(binimgs.shape)} {binimgs.dtype}, totals {tuple(totals.shape)} {totals.dtype}, "
                           f"params {tuple(params.shape)} {params.dtype}, thetas {tuple(thetas.shape)} {thetas.dtype}")
    if n_valid is not None and not (n_valid.device == preds.device and n_valid.dtype == torch.int32
                                    and n_valid.numel() == 1):
        raise RuntimeError("seg_metrics_accumulate: n_valid must be one int32 on the logits' device")
    if valid is None and valid_cells is not None:
        raise RuntimeError("seg_metrics_accumulate: valid_cells counts the cells of valid=")
    if valid is not None:
        if not (valid.device == preds.device and valid.dtype == torch.uint8 and valid.is_contiguous() and preds.dim() >= 2
                and valid.shape[0] == preds.shape[0] and valid.numel() * K == preds.numel()):
            raise RuntimeError(f"seg_metrics_accumulate: valid {tuple(valid.shape)} {valid.dtype} is not one contiguous "
                               f"uint8 plane per sample of logits {tuple(preds.shape)} on their device")
        if valid_cells is not None and not (valid_cells.device == preds.device and valid_cells.dtype == torch.float64
                                            and valid_cells.numel() == 1):
            raise RuntimeError("seg_metrics_accumulate: valid_cells must be one float64 on the logits' device")
    lib = _lib.load()
    x, t = preds.detach().contiguous(), binimgs.contiguous()
    batch = x.shape[0]
    per_sample = x.numel() // batch
    nbytes = int((lib.lss_seg_metrics_partial_bytes if valid is None else lib.lss_seg_metrics_masked_partial_bytes)(
        x.numel(), K, T))
    key = (x.device, nbytes)
    partial = _VAL_PARTIAL.get(key)
    if partial is None:
        partial = _VAL_PARTIAL[key] = torch.empty(nbytes // 8, device=x.device, dtype=torch.float64)
    if valid is not None:
        _lib.check(lib.lss_seg_metrics_accum_masked(_lib.ptr(x), _lib.dtype_code(x.dtype), _lib.ptr(t), _lib.ptr(valid),
                                                    per_sample, batch, _lib.ptr(n_valid), per_sample // K, K,
                                                    _lib.ptr(params), _lib.ptr(thetas), T, _lib.ptr(totals),
                                                    _lib.ptr(valid_cells), _lib.ptr(partial),
                                                    _lib.stream_handle(x.device)), "lss_seg_metrics_accum_masked")
        return totals
    _lib.check(lib.lss_seg_metrics_accum(_lib.ptr(x), _lib.dtype_code(x.dtype), _lib.ptr(t), per_sample, batch,
                                         _lib.ptr(n_valid), per_sample // K, K, _lib.ptr(params), _lib.ptr(thetas), T,
                                         _lib.ptr(totals), _lib.ptr(partial), _lib.stream_handle(x.device)),
               "lss_seg_metrics_accum")
    return totals


def seg_metrics_counts(totals, K: int, T: int):
    """(P[k], TP[k][j], PP[k][j]) as lists from the 1 + K + 2 K T totals of lss_seg_metrics_accum."""
    t = [float(v) for v in (totals.tolist() if torch.is_tensor(totals) else totals)]
    P = t[1:1 + K]
    TP = [t[1 + K + k * T:1 + K + (k + 1) * T] for k in range(K)]
    PP = [t[1 + K + K * T + k * T:1 + K + K * T + (k + 1) * T] for k in range(K)]
    return P, TP, PP


def seg_metrics_summary(totals, K: int, thresholds, n_samples) -> dict:
    """The totals of lss_seg_metrics_accum (a sequence or a tensor of 1 + K + 2 K T numbers; `thresholds`: the T
    probabilities of its columns) as a report: "loss" (the total over n_samples), "iou_at" (per threshold, a list
    over classes of TP / (PP + P - TP), None where that union is 0), "iou_max_per_class" and
    "best_threshold_per_class" (the largest IoU of a class over the ladder; ties go to the threshold nearest 0.5,
    then to the lower one; None for a class without any), "iou_max" (their mean over the classes that have one,
    None if none has). Never raises for counts of any value: what cannot be computed is None."""
    K, th = int(K), [float(v) for v in thresholds]
    T = len(th)
    t = [float(v) for v in (totals.tolist() if torch.is_tensor(totals) else totals)]
    t += [0.0] * max(0, 1 + K + 2 * K * T - len(t))
    P, TP, PP = seg_metrics_counts(t, K, T)
    iou_at = []
    for j in range(T):
        row = []
        for k in range(K):
            union = PP[k][j] + P[k] - TP[k][j]
            row.append(TP[k][j] / union if union > 0 else None)
        iou_at.append(row)
    best_iou, best_th = [], []
    for k in range(K):
        # (the distance rounded: 0.45 and 0.55 are equally near 0.5, whatever their binary fractions say)
        cand = [(-iou_at[j][k], round(abs(th[j] - 0.5), 9), th[j]) for j in range(T) if iou_at[j][k] is not None]
        if cand:
            top = min(cand)
            best_iou.append(-top[0])
            best_th.append(top[2])
        else:
            best_iou.append(None)
            best_th.append(None)
    seen = [v for v in best_iou if v is not None]
    return {"loss": t[0] / n_samples if n_samples else None, "iou_at": iou_at, "iou_max_per_class": best_iou,
            "best_threshold_per_class": best_th, "iou_max": sum(seen) / len(seen) if seen else None}


# ----------------------------------------------------------------------------- exclusive classes
IGNORE_LABEL = 255   # a class-map value >= C means "ignore"; 255 by convention (F.cross_entropy's ignore_index here)
MAX_CLASSES = 8      # the K-channel head's width: C = label groups + 1 <= 8
USE_HIP_SOFTMAX = True  # SoftmaxLoss takes ``lss_softmax_ce`` where it applies; False: always the torch composition


def _check_class_map(x: torch.Tensor, labels: torch.Tensor, valid, C: int, who: str):
    """Logits (batch, C, ...) against a (batch, ...) uint8 class map and an optional uint8 mask of the same cells."""
    if x.dim() < 2 or x.shape[1] != C:
        raise RuntimeError(f"{who}: {C} classes for logits {tuple(x.shape)}")
    cells = (x.shape[0],) + tuple(x.shape[2:])
    if labels.dtype != torch.uint8 or tuple(labels.shape) != cells:
        raise RuntimeError(f"{who}: labels must be the {cells} uint8 class map, got {labels.dtype} {tuple(labels.shape)}")
    if valid is not None and (valid.shape[0] != x.shape[0] or valid.numel() != labels.numel()):
        raise RuntimeError(f"{who}: valid {tuple(valid.shape)} is not one plane per sample of logits {tuple(x.shape)}")


def counted_cells(labels: torch.Tensor, valid, C: int) -> torch.Tensor:
    """The cell selection of the exclusive forms as booleans of labels' shape: label < C and (no mask or mask != 0)."""
    on = labels < C
    if valid is not None:
        on = on & (valid.to(labels.device).reshape(labels.shape) != 0)
    return on


def softmax_ce_terms(x: torch.Tensor, labels: torch.Tensor, valid, weight: torch.Tensor):
    """(loss, d loss / dx) of the exclusive-class loss in torch, in x's dtype (fp32 or fp64): per counted cell
    l = w_y (m + log S - x_y) and dl/dx_c = w_y (p_c - [c = y]) as ``lss_softmax_ce`` writes them (the c = y element
    as minus the other classes' share), cells that do not count selected out by torch.where -- a NaN there reaches
    nothing -- and both divided by max(W, tiny), W the counted cells' summed weights (W = 0: loss 0, gradient 0)."""
    C = x.shape[1]
    on = counted_cells(labels, valid, C)
    y = torch.where(on, labels, torch.zeros_like(labels)).long().unsqueeze(1)
    w = weight.to(device=x.device, dtype=x.dtype)
    m = x.max(dim=1, keepdim=True).values
    e = torch.exp(x - m)
    S = e.sum(dim=1, keepdim=True)
    hot = torch.zeros_like(x, dtype=torch.bool).scatter_(1, y, True)
    wy = w[y.squeeze(1)].unsqueeze(1)
    xy = x.gather(1, y)
    l = wy * ((m - xy) + torch.log(S))
    others = torch.where(hot, torch.zeros_like(e), e).sum(dim=1, keepdim=True)
    g = wy * torch.where(hot, -(others / S), e / S)
    zero = torch.zeros((), device=x.device, dtype=x.dtype)
    on1 = on.unsqueeze(1)
    W = torch.where(on1, wy, zero).sum()
    d = W.clamp(min=torch.finfo(torch.float32).tiny)
    live = (W > 0).to(x.dtype)
    return torch.where(on1, l, zero).sum() / d * live, torch.where(on1, g, zero) / d * live


class _SoftmaxCeTorch(torch.autograd.Function):
    """The exclusive-class loss where the kernel does not apply (CPU, strided logits, other dtypes): softmax_ce_terms
    in fp32 (fp64 logits: in fp64), the gradient kept in the logits' type."""

    @staticmethod
    def forward(ctx, x, labels, valid, weight):
        xd = x.detach()
        loss, g = softmax_ce_terms(xd if xd.dtype == torch.float64 else xd.float(), labels, valid, weight)
        ctx.save_for_backward(g.to(x.dtype))
        return loss

    @staticmethod
    def backward(ctx, g):
        (grad,) = ctx.saved_tensors
        return (grad.to(g.dtype if g.dtype == torch.float64 else torch.float32) * g).to(grad.dtype), None, None, None


class _SoftmaxCe(torch.autograd.Function):
    """``lss_softmax_ce``: loss, stored gradient (dl/dx / n_cells) and the device scalar n_cells / W in two launches;
    the backward is ``lss_seg_loss_masked_bwd`` over the batch * C * plane gradient elements."""

    @staticmethod
    def forward(ctx, x, labels, valid, weight):
        from . import _lib
        lib = _lib.load()
        batch, C = x.shape[0], x.shape[1]
        plane = x.numel() // (batch * C)
        partial = torch.empty(int(lib.lss_softmax_ce_partials(batch * plane)), device=x.device, dtype=torch.float32)
        loss = torch.empty((), device=x.device, dtype=torch.float32)
        scale = torch.empty((), device=x.device, dtype=torch.float32)
        grad = torch.empty_like(x)
        _lib.check(lib.lss_softmax_ce(_lib.ptr(x), _lib.dtype_code(x.dtype), _lib.ptr(labels), _lib.ptr(valid), batch,
                                      plane, C, _lib.ptr(weight), _lib.ptr(partial), _lib.ptr(loss), _lib.ptr(scale),
                                      _lib.ptr(grad), _lib.stream_handle(x.device)), "lss_softmax_ce")
        ctx.save_for_backward(grad, scale)
        return loss

    @staticmethod
    def backward(ctx, g):
        return _stored_grad_backward(ctx, g), None, None, None


def softmax_ce_arm(x: torch.Tensor, labels: torch.Tensor, valid=None, grad=None) -> int:
    """``lss_softmax_ce_arm``: 0 (one cell per thread) or 1 (8 cells per thread, vector loads) for a call on these
    tensors. grad None: the fresh allocation SoftmaxLoss makes (16-B aligned, so x's own address stands in)."""
    from . import _lib
    batch, C = x.shape[0], x.shape[1]
    arm = _lib.load().lss_softmax_ce_arm(_lib.ptr(x), _lib.dtype_code(x.dtype), _lib.ptr(labels), _lib.ptr(valid), batch,
                                         x.numel() // (batch * C), C, _lib.ptr(x if grad is None else grad))
    if arm < 0:
        raise RuntimeError(f"lss_softmax_ce_arm refuses logits {tuple(x.shape)} {x.dtype}")
    return arm


class SoftmaxLoss(torch.nn.Module):
    """Softmax cross-entropy over exclusive classes: ``F.cross_entropy(logits, labels, weight=w, ignore_index=255,
    reduction="mean")`` for (N, C, H, W) logits and an (N, H, W) uint8 class map (simbev.class_index; every value
    >= C is ignored, 255 by convention), with an optional uint8 valid-cell mask. ``class_weight``: the C fp32 class
    weights, a device buffer the kernel reads -- changed in place, a captured step follows. On the GPU under
    SimpleLoss's conditions (fp32 or bf16 contiguous logits, contiguous uint8 labels and mask on their device) loss
    and gradient come from ``lss_softmax_ce``, computed in fp32; otherwise from the same definition in torch
    (softmax_ce_terms). Drops in wherever SimpleLoss / FocalLoss do; ``exclusive`` marks the label format."""

    computes_in_fp32 = True
    exclusive = True

    def __init__(self, classes: int, weight=None):
        super().__init__()
        C = int(classes)
        if not 2 <= C <= MAX_CLASSES:
            raise ValueError(f"SoftmaxLoss: {classes!r} classes (2..{MAX_CLASSES}: the background and 1..7 groups)")
        w = [1.0] * C if weight is None else [float(v) for v in (weight.tolist() if torch.is_tensor(weight) else weight)]
        if len(w) != C or any(not (v >= 0.0 and v < float("inf")) for v in w):
            raise ValueError(f"SoftmaxLoss: class weights {w!r}: {C} finite numbers >= 0")
        self.classes = C
        self.register_buffer("class_weight", torch.tensor(w, dtype=torch.float32), persistent=False)

    def forward(self, ypred, ytgt, valid=None):
        C, w = self.classes, self.class_weight
        _check_class_map(ypred, ytgt, valid, C, "SoftmaxLoss")
        if (USE_HIP_SOFTMAX and ypred.is_cuda and ypred.dtype in (torch.float32, torch.bfloat16)
                and ytgt.device == ypred.device and ypred.is_contiguous() and ytgt.is_contiguous()
                and ypred.numel() > 0 and w.device == ypred.device and w.dtype == torch.float32 and w.is_contiguous()
                and (valid is None or (valid.dtype == torch.uint8 and valid.device == ypred.device
                                       and valid.is_contiguous()))):
            return _SoftmaxCe.apply(ypred, ytgt, valid, w)
        return _SoftmaxCeTorch.apply(ypred, ytgt, valid, w)


def argmax_classes(preds: torch.Tensor, out=None) -> torch.Tensor:
    """The (N, H, W) uint8 class map of (N, C, H, W) device logits, ``lss_argmax_classes``: argmax over the classes
    compared in fp32 with a strict > from class 0 up (ties to the lowest class, a NaN never wins, all-NaN gives 0)."""
    from . import _lib
    if not (preds.is_cuda and preds.dim() >= 2 and 2 <= preds.shape[1] <= MAX_CLASSES and preds.numel() > 0):
        raise RuntimeError(f"argmax_classes: device logits (N, 2..{MAX_CLASSES}, ...), got {tuple(preds.shape)} on "
                           f"{preds.device}")
    x = preds.detach().contiguous()
    batch, C = x.shape[0], x.shape[1]
    cells = (batch,) + tuple(x.shape[2:])
    if out is None:
        out = torch.empty(cells, device=x.device, dtype=torch.uint8)
    elif not (out.device == x.device and out.dtype == torch.uint8 and out.is_contiguous()
              and out.numel() * C == x.numel()):
        raise RuntimeError(f"argmax_classes: out= must be a contiguous uint8 device tensor of {cells}")
    _lib.check(_lib.load().lss_argmax_classes(_lib.ptr(x), _lib.dtype_code(x.dtype), batch, x.numel() // (batch * C), C,
                                              _lib.ptr(out), _lib.stream_handle(x.device)), "lss_argmax_classes")
    return out


def argmax_classes_host(x) -> "numpy.ndarray":
    """argmax_classes' rule on the host for (N, C, ...) logits (a tensor or an array), as uint8."""
    import numpy as np
    a = np.asarray(x.detach().float().cpu() if torch.is_tensor(x) else x, dtype=np.float32)
    best = np.zeros((a.shape[0],) + a.shape[2:], dtype=np.uint8)
    bv = np.full(best.shape, -np.inf, dtype=np.float32)
    for c in range(a.shape[1]):
        with np.errstate(invalid="ignore"):
            gt = a[:, c] > bv
        best[gt] = c
        bv = np.where(gt, a[:, c], bv)
    return best


def confusion_accumulate(preds: torch.Tensor, labels: torch.Tensor, totals: torch.Tensor, n_valid, weight: torch.Tensor,
                         valid=None) -> torch.Tensor:
    """One validation batch of exclusive classes into its accumulators, ``lss_confusion_accum``: totals (1 + C C
    float64 on the device) += the batch's mean loss times the samples counted, then the confusion counts
    conf[y][pred] over the counted cells (label < C, mask != 0) of the first ``n_valid`` samples (one int32 on the
    device; None: all). preds (N, C, H, W) fp32 or bf16, labels (N, H, W) uint8, weight the C fp32 class weights
    (SoftmaxLoss.class_weight), valid an optional (N, H, W) uint8 mask. Device tensors only; two launches, no host
    synchronisation, capturable (the scratch is kept per device and size, as val_accumulate's)."""
    from . import _lib
    if not (preds.is_cuda and all(v.device == preds.device for v in (labels, totals, weight))):
        raise RuntimeError("confusion_accumulate: device tensors only (no CPU fallback)")
    C = preds.shape[1] if preds.dim() >= 2 else 0
    if not 2 <= C <= MAX_CLASSES or preds.numel() == 0:
        raise RuntimeError(f"confusion_accumulate: logits (N, 2..{MAX_CLASSES}, ...), got {tuple(preds.shape)}")
    _check_class_map(preds, labels, valid, C, "confusion_accumulate")
    if (totals.dtype != torch.float64 or totals.numel() != 1 + C * C or not totals.is_contiguous()
            or weight.dtype != torch.float32 or weight.numel() != C or not weight.is_contiguous()):
        raise RuntimeError(f"confusion_accumulate: totals {tuple(totals.shape)} {totals.dtype} (1 + {C * C} float64), "
                           f"weight {tuple(weight.shape)} {weight.dtype} ({C} float32)")
    if n_valid is not None and not (n_valid.device == preds.device and n_valid.dtype == torch.int32
                                    and n_valid.numel() == 1):
        raise RuntimeError("confusion_accumulate: n_valid must be one int32 on the logits' device")
    if valid is not None and not (valid.device == preds.device and valid.dtype == torch.uint8 and valid.is_contiguous()):
        raise RuntimeError("confusion_accumulate: valid must be a contiguous uint8 mask on the logits' device")
    lib = _lib.load()
    x, t = preds.detach().contiguous(), labels.contiguous()
    batch = x.shape[0]
    plane = x.numel() // (batch * C)
    nbytes = int(lib.lss_confusion_partial_bytes(batch * plane, C))
    key = (x.device, "confusion", nbytes)
    partial = _VAL_PARTIAL.get(key)
    if partial is None:  # (an odd C's histogram ends on a 4-byte boundary: rounded up to whole doubles)
        partial = _VAL_PARTIAL[key] = torch.empty((nbytes + 7) // 8, device=x.device, dtype=torch.float64)
    _lib.check(lib.lss_confusion_accum(_lib.ptr(x), _lib.dtype_code(x.dtype), _lib.ptr(t), _lib.ptr(valid), batch, plane,
                                       C, _lib.ptr(n_valid), _lib.ptr(weight), _lib.ptr(totals), _lib.ptr(partial),
                                       _lib.stream_handle(x.device)), "lss_confusion_accum")
    return totals


def confusion_summary(totals, C: int, n_samples, cells=None) -> dict:
    """The totals of ``lss_confusion_accum`` (a sequence or a tensor of 1 + C C numbers) as a report:
    "loss" (the total over n_samples), "confusion" (C lists of C ints, conf[y][pred]), "iou_per_class" (TP / (TP + FP
    + FN), None for an empty union), "iou" (the mean over the foreground classes 1..C-1 that were seen -- the number
    a best checkpoint is chosen by, comparable with the sigmoid mode's), "miou_all" (the background included),
    "pixel_acc", "precision_per_class" and "recall_per_class". cells: the number of cells the counted ones are a
    fraction of (samples x plane, with a mask in use) -- adds "valid_fraction". Never raises for counts of any value:
    what cannot be computed is None."""
    C = int(C)
    t = [float(v) for v in (totals.tolist() if torch.is_tensor(totals) else totals)]
    t += [0.0] * max(0, 1 + C * C - len(t))
    conf = [[int(t[1 + y * C + p]) for p in range(C)] for y in range(C)]
    tp = [conf[c][c] for c in range(C)]
    row = [sum(conf[c]) for c in range(C)]                          # cells labelled c: TP + FN
    col = [sum(conf[y][c] for y in range(C)) for c in range(C)]     # cells predicted c: TP + FP
    per = [tp[c] / (row[c] + col[c] - tp[c]) if row[c] + col[c] - tp[c] > 0 else None for c in range(C)]
    fg = [v for v in per[1:] if v is not None]
    seen = [v for v in per if v is not None]
    total = sum(row)
    info = {"loss": t[0] / n_samples if n_samples else None,
            "iou": sum(fg) / len(fg) if fg else None,
            "iou_per_class": per,
            "miou_all": sum(seen) / len(seen) if seen else None,
            "pixel_acc": sum(tp) / total if total > 0 else None,
            "precision_per_class": [tp[c] / col[c] if col[c] > 0 else None for c in range(C)],
            "recall_per_class": [tp[c] / row[c] if row[c] > 0 else None for c in range(C)],
            "confusion": conf}
    if cells is not None:
        info["valid_fraction"] = total / cells if cells else None
    return info


def val_totals(model, loader, loss_fn, device):
    """The device accumulators of get_val_info: (sum of loss x batch size, intersection, union) as
    float64 device tensors; nothing in the loop synchronises the host. The counts
    are per class, sized by the labels: scalars for one label channel, (K,) tensors for K > 1."""
    total_loss = torch.zeros((), device=device, dtype=torch.float64)
    total_intersect = total_union = None
    with torch.no_grad():
        for batch in loader:
            allimgs, rots, trans, intrins, post_rots, post_trans, binimgs = batch
            preds = model(allimgs.to(device), rots.to(device), trans.to(device), intrins.to(device),
                          post_rots.to(device), post_trans.to(device))
            binimgs = binimgs.to(device)
            total_loss += loss_fn(preds, binimgs).double() * preds.shape[0]
            if binimgs.dim() == 4 and binimgs.shape[1] > 1:
                i, u = get_batch_iou_per_class(preds, binimgs)
            else:
                i, u = get_batch_iou_device(preds, binimgs)
            total_intersect = i.double() if total_intersect is None else total_intersect + i.double()
            total_union = u.double() if total_union is None else total_union + u.double()
    if total_intersect is None:
        total_intersect = torch.zeros((), device=device, dtype=torch.float64)
        total_union = torch.zeros((), device=device, dtype=torch.float64)
    return total_loss, total_intersect, total_union


def get_val_info(model, valloader, loss_fn, device, use_tqdm=True):
    """Validation loss / IoU over a loader (src/tools.py:243-270).

    Same results as the reference, but the per-batch ``.item()`` syncs are gone: loss (x batch size) and the
    intersection / union counts accumulate on the device in float64 (val_totals) and are read once at the
    end. As in the reference, the loss is divided by ``len(valloader.dataset)`` and an empty union raises
    ZeroDivisionError. One label channel: the reference's {"loss", "iou"}. K > 1 label channels:
    {"loss", "iou", "iou_per_class"} -- inter_k / union_k per class, None for a class with an empty union,
    and "iou" their mean over the classes seen (iou_summary).
    """
    model.eval()
    print("running eval...")
    loader = valloader
    if use_tqdm:
        from tqdm import tqdm
        loader = tqdm(valloader, desc="Validation")
    total_loss, total_intersect, total_union = val_totals(model, loader, loss_fn, device)
    model.train()
    inter, union = total_intersect.reshape(-1).tolist(), total_union.reshape(-1).tolist()
    info = {"loss": total_loss.item() / len(valloader.dataset), **iou_summary(inter, union)}
    if len(inter) == 1:
        del info["iou_per_class"]  # one label channel: exactly the reference's dict
    return info
