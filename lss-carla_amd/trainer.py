"""The training loop of train_simbev.py:23-458 on the captured step, fed by ``simbev.compile_data``.

``train(dataroot, ...)`` takes the reference's arguments and behaves as its loop does -- same model,
loss, clipping and Adam, validation every ``val_step`` steps with a best-IoU checkpoint, a checkpoint
every ``save_step`` steps and at the end, resume from either trainer's checkpoints -- but each step is
two HIP graph replays (train_step.TrainStep over flat fp32 masters, as bench.py builds it) whose static
inputs ``staging.BatchStager`` fills from the loader's raw batches, one batch ahead:

    stage(batch k+1)  staging stream: H2D copies + the two SimBEV kernels, while step k runs
    commit()          slot -> static tensors, host torch.inverse of the rig staged (ops.HostInverses)
    step()            graph A (forward, loss, backward), graph B (clip + Adam, guarded)

The host reads the device at the reference's cadence only: the loss every 10 steps, the training IoU and
the count of skipped (non-finite) steps every 100, validation totals once per validation
(train_step.EvalStep: one more graph, over the same static tensors), checkpoints. Nothing else
synchronises. Events go to ``logdir/metrics.jsonl`` (one JSON object per line) and, when importable, to
tensorboardX / wandb. ``graph=False`` runs the same loop eagerly on the same stager.

    python -m lss_carla_amd.trainer --dataroot /data/simbev --bsz 8 --final_h 128 --final_w 352

Differences from the reference, all deliberate: the matplotlib figures are not drawn; the first
validation always writes ``model_best.pt`` (the reference skips it while the IoU is 0); a step whose
bf16 gradient is not finite is skipped and counted instead of poisoning the weights (``skip_nonfinite``).

``ncams=k`` (1 <= k <= 6) is the reference's ``Ncams``: every training sample holds k cameras drawn at random
(sorted, ``simbev.SimBEVDataset.choose_cams``; only their k JPEGs are decoded) and validation uses all six. The
training step then runs over a stager of N = k cameras and the validation step over a second one of N = 6, each
with its own static tensors, labels, valid mask and host-inverted rig -- two captured shapes, one set of weights.
The dropped cameras are absent from the tensors, not masked: their images never reach the trunk's batch
statistics, as in the reference (``LiftSplatShoot.camera_alive`` is the inference-time mask).
"""
from __future__ import annotations

import argparse
import json
import os
import time
from typing import Callable, Optional

from . import miopen_db

miopen_db.use_committed()  # the committed MIOpen find results, as bench.py uses them (before torch starts)

import numpy as np  # noqa: E402
import torch  # noqa: E402


class _Log:
    """metrics.jsonl plus the optional writers (neither is required to be installed)."""

    def __init__(self, logdir: str, use_wandb: bool, wandb_kwargs: dict, config: dict):
        self.f = open(os.path.join(logdir, "metrics.jsonl"), "a")
        self.tb, self.wandb = None, None
        try:
            from tensorboardX import SummaryWriter
            self.tb = SummaryWriter(logdir=logdir)
        except ImportError:
            pass
        if use_wandb:
            try:
                import wandb
                wandb.init(config=config, dir=logdir, **wandb_kwargs)
                self.wandb = wandb
            except ImportError:
                print("wandb is not installed: logging to metrics.jsonl only")

    def event(self, kind: str, counter: int, **values) -> None:
        self.f.write(json.dumps({"event": kind, "counter": counter, **values}) + "\n")
        self.f.flush()
        scalars = {f"{kind}/{k}": v for k, v in values.items() if isinstance(v, (int, float))}
        if self.tb is not None:
            for k, v in scalars.items():
                self.tb.add_scalar(k, v, counter)
        if self.wandb is not None:
            self.wandb.log({**scalars, "iteration": counter})

    def close(self) -> None:
        self.f.close()
        if self.tb is not None:
            self.tb.close()
        if self.wandb is not None:
            self.wandb.finish()


class _Cycle:
    """`n` pre-decoded raw batches of a loader, cycled for the loader's length (measurement: the loop
    without the decode)."""

    def __init__(self, loader, n: int):
        self.batches, self.length = [], len(loader)
        for b in loader:
            self.batches.append(b)
            if len(self.batches) >= n:
                break

    def __len__(self):
        return self.length

    def __iter__(self):
        for i in range(self.length):
            yield self.batches[i % len(self.batches)]


def parse_label_groups(text):
    """``--label_groups "0;1,2,3;6,7"`` -> [[0], [1, 2, 3], [6, 7]]: semicolons between the groups, commas
    inside one. None or an empty string: None (the reference's single vehicle mask)."""
    if text is None or not str(text).strip():
        return None
    groups = []
    for part in str(text).split(";"):
        items = [v.strip() for v in part.split(",") if v.strip()]
        if not items:
            raise ValueError(f"--label_groups {text!r}: an empty group")
        groups.append([int(v) for v in items])
    return groups


def parse_pos_weight(text):
    """``--pos_weight 2.13`` -> 2.13; ``--pos_weight 1.0,2.13,5.0`` -> [1.0, 2.13, 5.0] (one per class)."""
    items = [v.strip() for v in str(text).split(",") if v.strip()]
    if not items:
        raise ValueError(f"--pos_weight {text!r}: no value")
    vals = [float(v) for v in items]
    return vals[0] if len(vals) == 1 else vals


def parse_per_class(text, name="value"):
    """A flag that takes one number or one per class, as --pos_weight: "2.0" -> 2.0; "2.0,1.5,0.5" -> [2.0, 1.5, 0.5]."""
    items = [v.strip() for v in str(text).split(",") if v.strip()]
    if not items:
        raise ValueError(f"{name} {text!r}: no value")
    vals = [float(v) for v in items]
    return vals[0] if len(vals) == 1 else vals


def _weights_list(text, name="--class_weight") -> list:
    """``--class_weight 0.5,1,2`` -> [0.5, 1.0, 2.0]: always a list, one weight per class."""
    v = parse_per_class(text, name)
    return [v] if isinstance(v, float) else v


def parse_pair(text, name="value"):
    """``--bev_rot_lim -22.5,22.5`` -> (-22.5, 22.5): the two ends of a range, as the loader's *_lim keys."""
    items = [v.strip() for v in str(text).split(",") if v.strip()]
    if len(items) != 2:
        raise ValueError(f"{name} {text!r}: two numbers, lo,hi")
    return float(items[0]), float(items[1])


def photo_conf(brightness=0.0, contrast=(1.0, 1.0), saturation=(1.0, 1.0), hue=0.0, noise=(0.0, 0.0), prob=0.5,
               per_camera=True) -> dict:
    """The loader's photo_* keys from the trainer's arguments: brightness (0..255 units) and hue (degrees) are
    symmetric half-widths (32 -> (-32, 32)); contrast, saturation and the noise sigma are (lo, hi) ranges. ValueError
    for a negative half-width or a limit simbev.photo_enabled refuses."""
    from . import simbev
    b, h = float(brightness), float(hue)
    if not (b >= 0.0 and h >= 0.0):
        raise ValueError(f"photo_brightness {brightness!r} / photo_hue {hue!r}: half-widths, not negative")
    conf = {"photo_brightness_lim": (-b, b), "photo_contrast_lim": tuple(float(v) for v in contrast),
            "photo_saturation_lim": tuple(float(v) for v in saturation), "photo_hue_lim": (-h, h),
            "photo_noise_lim": tuple(float(v) for v in noise), "photo_prob": float(prob),
            "photo_per_camera": int(bool(per_camera))}
    simbev.photo_enabled(conf)
    return conf


def parse_thresholds(text):
    """``--iou_thresholds 0.35,0.4,0.45,0.5,0.55,0.6,0.65`` (or a sequence of numbers) -> the ladder as an ascending
    list of distinct probabilities, each strictly between 0 and 1, 15 at most (0.5 makes 16); None or empty: None."""
    if text is None or (isinstance(text, str) and not text.strip()):
        return None
    items = [v for v in text.split(",") if v.strip()] if isinstance(text, str) else list(text)
    vals = sorted({float(v) for v in items})
    if not vals:
        return None
    if any(not 0.0 < v < 1.0 for v in vals):
        raise ValueError(f"--iou_thresholds {text!r}: probabilities strictly between 0 and 1")
    if len(set(vals + [0.5])) > 16:
        raise ValueError(f"--iou_thresholds {text!r}: at most 16 thresholds, 0.5 included")
    return vals


def parse_heights(text, name="--fov_z"):
    """``--fov_z 0.0`` -> (0.0,); ``--fov_z 0.0,1.5`` -> (0.0, 1.5): the heights a cell is tested at (1 to 8); a
    sequence of numbers passes through the same check."""
    from . import simbev
    items = [v for v in str(text).split(",") if v.strip()] if isinstance(text, str) else text
    try:
        return simbev.fov_heights({"fov_z": [float(v) for v in items] if not isinstance(items, (int, float)) else items})
    except (TypeError, ValueError):
        raise ValueError(f"{name} {text!r}: 1 to 8 finite heights in metres, comma separated") from None


def _loss_setup(loss, pos_weight, focal_gamma, focal_alpha):
    """(pos_weight, focal): the weight SimpleLoss / validation take (None: the reference's 2.13) and, for
    loss == "focal", tools.FocalLoss's keyword arguments -- pos_weight becomes w_pos unless focal_alpha is given;
    giving both is an error."""
    if loss not in ("bce", "focal"):
        raise ValueError(f"loss {loss!r}: bce or focal")
    if loss == "bce":
        if focal_alpha is not None:
            raise ValueError("focal_alpha is the focal loss's: it needs loss=focal")
        return (2.13 if pos_weight is None else pos_weight), None
    if focal_alpha is not None and pos_weight is not None:
        raise ValueError("loss=focal: pos_weight and focal_alpha both set the class balance: give one")
    return (1.0 if pos_weight is None else pos_weight), {"gamma": focal_gamma, "alpha": focal_alpha,
                                                          "pos_weight": pos_weight}


def _schedule_setup(lr, lr_schedule, warmup_steps, warmup_factor, lr_min, lr_total_steps, ema_decay):
    """Check the schedule's and the EMA's arguments (ValueError, before anything is looked for or built); returns
    whether a schedule is asked for -- anything but a constant rate without warm-up. lr_min is absolute: the
    decay ends at lr_min / lr. lr_total_steps None (the run's length, known once the loader is): checked later."""
    from .optim import LRSchedule
    if not float(lr) > 0.0:
        raise ValueError(f"lr {lr!r}: positive")
    if not 0.0 <= float(lr_min) <= float(lr):
        raise ValueError(f"lr_min {lr_min!r}: between 0 and lr ({lr})")
    if lr_total_steps is not None and int(lr_total_steps) <= 0:
        raise ValueError(f"lr_total_steps {lr_total_steps!r}: positive")
    total = int(lr_total_steps) if lr_total_steps is not None else max(int(warmup_steps), 0) + 1
    LRSchedule(lr_schedule, warmup_steps, warmup_factor, total, float(lr_min) / float(lr))
    if not 0.0 <= float(ema_decay) < 1.0:
        raise ValueError(f"ema_decay {ema_decay!r}: in [0, 1) (0: no EMA)")
    return lr_schedule != "constant" or int(warmup_steps) > 0


def _class_setup(label_groups, pos_weight):
    """(groups or None, K, the loss's pos_weight): a list of weights must name one per class; a single-class
    run keeps a float (the one-weight kernels), a list of one collapsing to it."""
    from . import simbev, tools
    groups = None if label_groups is None else [[int(c) for c in g] for g in label_groups]
    if groups is not None:
        simbev.group_bits(groups)
    K = 1 if groups is None else len(groups)
    if not tools.is_scalar_weight(pos_weight):
        pos_weight = [float(v) for v in pos_weight]
        if len(pos_weight) != K:
            raise ValueError(f"pos_weight names {len(pos_weight)} classes, label_groups {K}")
        if K == 1:
            pos_weight = pos_weight[0]
    return groups, K, pos_weight


EXCLUSIVE_KEYS = ("iou_per_class", "miou_all", "pixel_acc", "precision_per_class", "recall_per_class", "confusion")


def _exclusive_setup(label_groups, class_weight, pos_weight=None, loss="bce", focal_gamma=2.0, focal_alpha=None,
                     iou_thresholds=None) -> list:
    """The C = K + 1 class weights of an exclusive run (default all 1), after its argument errors: exclusive classes
    need 1..7 label_groups, and the sigmoid mode's options -- pos_weight, the focal loss and its parameters, a
    threshold ladder -- do not apply to a softmax over the classes (ValueError, before anything is built)."""
    from . import simbev
    if label_groups is None:
        raise ValueError("exclusive classes need label_groups (class 0 is the background, class k + 1 is group k)")
    simbev.exclusive_bits(label_groups)
    for given, name in ((pos_weight is not None, "pos_weight"), (loss != "bce", "loss=focal"),
                        (focal_alpha is not None, "focal_alpha"),
                        (not (isinstance(focal_gamma, (int, float)) and float(focal_gamma) == 2.0), "focal_gamma"),
                        (iou_thresholds is not None, "iou_thresholds")):
        if given:
            raise ValueError(f"{name} does not apply to exclusive classes (softmax cross-entropy with class_weight; "
                             "the prediction is an argmax)")
    C = len(label_groups) + 1
    w = [1.0] * C if class_weight is None else [float(v) for v in class_weight]
    if len(w) != C or any(not (0.0 <= v < float("inf")) for v in w):
        raise ValueError(f"class_weight {class_weight!r}: {C} finite weights >= 0 (the background, then one per group)")
    return w


def _check_ncams(ncams) -> int:
    """The reference's ``Ncams``: an integer from 1 to the rig's six cameras, else ValueError."""
    from . import simbev
    n_all = len(simbev.CAMERA_ORDER)
    if isinstance(ncams, bool) or not isinstance(ncams, (int, np.integer)) or not 1 <= int(ncams) <= n_all:
        raise ValueError(f"ncams {ncams!r}: an integer from 1 to {n_all}")
    return int(ncams)


def build_step(grid_conf, data_aug_conf, bsz, device, *, dtype="bf16", lr=1e-3, weight_decay=1e-7,
               max_grad_norm=5.0, pos_weight=2.13, skip_nonfinite=True, n_val=None, label_groups=None,
               loss="bce", focal_gamma=2.0, focal_alpha=None, iou_thresholds=None, lr_schedule=None,
               ema_decay=0.0, ema_warmup=True, ncams=6, exclusive=False, class_weight=None) -> dict:
    """The model and its steps as bench.py's train branch builds them -- unused parameters frozen, one flat
    fp32 master per backward group, fused capturable Adam, TrainStep without a pre_step (the stager's
    commit stages the inverses) -- plus the stager and the EvalStep over the same static tensors. Nothing is
    captured yet. label_groups: K lists of BEV channels -> a model with outC = K and (B, K, X, Y) labels
    (None: the reference's vehicle mask, outC = 1); pos_weight: a float, or one weight per class.
    loss: "bce" (SimpleLoss) or "focal" (tools.FocalLoss(outC, focal_gamma, focal_alpha), pos_weight its w_pos
    when focal_alpha is None); iou_thresholds: a ladder of probabilities the EvalStep also counts the IoU at.
    lr_schedule: an optim.LRSchedule the captured update follows (None: the constant ``lr``). ema_decay > 0: the
    masters get EMA twins (FlatParamGroups.enable_ema) the update averages into, and the EvalStep runs on them
    (``forward_ema``: the working copies materialised from the EMA by the same launch).
    A data_aug_conf that asks for the BEV-space augmentation (simbev.bev_aug_enabled) makes the stager expect the
    label index matrices in its raw batches, as ``compile_data``'s loaders of the same conf provide them. One that
    asks for a valid-cell mask (simbev.valid_mask_mode: ``valid_mask`` "grid" / "fov", heights ``fov_z``) makes the
    stager keep the mask, the TrainStep average its loss over valid cells and the EvalStep count valid cells only.
    ncams: the cameras of a training batch (1..6). Below 6, the TrainStep runs over a training stager of N = ncams
    and the EvalStep over a second stager of N = 6 (``"val_stager"``), each step with its own labels, ``n_valid``, valid
    mask and HostInverses, which it installs as ``model.static_inverses`` around its own forward. With "fov" each
    stager's mask comes from the cameras its batch holds: a cell only a dropped camera would see is invalid in that
    training sample. At 6, ``"val_stager"`` is ``"stager"`` and nothing is allocated or launched differently.
    exclusive: the K label_groups are painted into one (B, X, Y) uint8 class map (simbev.class_index: 0 the
    background, k + 1 group k, a later group wins), the model has outC = K + 1, the loss is
    tools.SoftmaxLoss(K + 1, class_weight) and the EvalStep accumulates a confusion matrix; pos_weight, loss and
    iou_thresholds are not used.
    A data_aug_conf that asks for the photometric augmentation (simbev.photo_enabled) makes both stagers expect the
    photo records in their raw batches and run ``lss_simbev_images_photo``; the captured steps do not change."""
    import lss_carla_amd as L
    from . import parallel, simbev, tools
    from .flat_params import FlatParamGroups, lss_backward_groups
    from .staging import BatchStager
    from .train_step import EvalStep, TrainStep

    ncams, n_all = _check_ncams(ncams), len(simbev.CAMERA_ORDER)  # (before anything is built)
    amp_dtype = torch.bfloat16 if dtype == "bf16" else None
    label_groups, outC, pos_weight = _class_setup(label_groups, pos_weight)
    excl_args = {}
    if exclusive:
        class_weight = _exclusive_setup(label_groups, class_weight)
        outC, excl_args = outC + 1, {"exclusive": True}
    model = L.compile_model(grid_conf, data_aug_conf, outC=outC).to(device)
    model.bevencode.to(memory_format=torch.channels_last)
    model.camencode.up1.to(memory_format=torch.channels_last)
    model.train()
    parallel.freeze_unused(model)
    flat = FlatParamGroups(model, lss_backward_groups(), cast_dtype=amp_dtype)
    masters = flat.masters
    opt = torch.optim.Adam(masters, lr=lr, weight_decay=weight_decay, fused=True, capturable=True)
    mask_mode = simbev.valid_mask_mode(data_aug_conf)
    mask_args = {} if mask_mode is None else {"valid_mask": mask_mode, "fov_z": simbev.fov_heights(data_aug_conf)}
    if simbev.photo_enabled(data_aug_conf):  # both stagers: validation's raw batches carry (neutral) records too
        excl_args = {**excl_args, "photo": True}
    stager = BatchStager(data_aug_conf["final_dim"], bsz, ncams,
                         (data_aug_conf["H"], data_aug_conf["W"]), grid_conf, device, label_groups=label_groups,
                         bev_aug=simbev.bev_aug_enabled(data_aug_conf), **mask_args, **excl_args)
    step_mask = {} if mask_mode is None else {"valid": stager.valid}
    val_stager, val_mask, step_inv, val_inv = stager, step_mask, {}, {}
    if ncams < n_all:  # validation at every camera: static tensors of its own
        val_stager = BatchStager(data_aug_conf["final_dim"], bsz, n_all, (data_aug_conf["H"], data_aug_conf["W"]),
                                 grid_conf, device, label_groups=label_groups,
                                 bev_aug=simbev.bev_aug_enabled(data_aug_conf), **mask_args, **excl_args)
        val_mask = {} if mask_mode is None else {"valid": val_stager.valid}
        step_inv = {"inverses": (stager.hinv.pinv, stager.hinv.kinv), "model": model}
        val_inv = {"inverses": (val_stager.hinv.pinv, val_stager.hinv.kinv)}
    model.static_inverses = (stager.hinv.pinv, stager.hinv.kinv)  # staged by the stager's commit
    if loss not in ("bce", "focal"):
        raise ValueError(f"loss {loss!r}: bce or focal")
    if exclusive:
        loss_fn = tools.SoftmaxLoss(outC, class_weight).to(device)
    elif loss == "focal":
        loss_fn = tools.FocalLoss(outC, gamma=focal_gamma, alpha=focal_alpha,
                                  pos_weight=None if focal_alpha is not None else pos_weight).to(device)
    else:
        loss_fn = tools.SimpleLoss(pos_weight).to(device)
    iou_thresholds = parse_thresholds(iou_thresholds)
    forward = flat.bind(model)
    emas = flat.enable_ema() if ema_decay else None
    forward_eval = flat.bind(model, source="ema") if emas is not None else forward
    step = TrainStep(forward, stager.inputs, stager.binimgs, loss_fn, opt, masters, all_reduce=False,
                     amp_dtype=amp_dtype, max_grad_norm=max_grad_norm, pre_step=None,
                     skip_nonfinite=bool(skip_nonfinite), keep_preds=True, lr_schedule=lr_schedule, ema=emas,
                     ema_decay=float(ema_decay) if emas is not None else 0.999, ema_warmup=bool(ema_warmup),
                     **step_mask, **step_inv)
    evaluate = EvalStep(model, forward_eval, val_stager.inputs, val_stager.binimgs, n_valid=val_stager.n_valid,
                        pos_weight=pos_weight, amp_dtype=amp_dtype, n_samples=n_val,
                        loss=loss_fn if (loss == "focal" or exclusive) else None, thresholds=iou_thresholds,
                        **val_mask, **val_inv)
    return {"model": model, "flat": flat, "masters": masters, "opt": opt, "stager": stager, "val_stager": val_stager,
            "step": step,
            "evaluate": evaluate, "loss_fn": loss_fn, "forward": forward, "label_groups": label_groups,
            "emas": emas, "forward_eval": forward_eval}


def train(
    dataroot,
    nepochs=100,
    gpuid=0,
    H=224,
    W=480,
    resize_lim=(1.0, 1.0),
    final_dim=(128, 352),
    bot_pct_lim=(0.0, 0.0),
    rot_lim=(0.0, 0.0),
    rand_flip=False,
    ncams=6,
    max_grad_norm=5.0,
    pos_weight=None,
    logdir="./runs/simbev",
    xbound=[-50.0, 50.0, 0.5],
    ybound=[-50.0, 50.0, 0.5],
    zbound=[-10.0, 10.0, 20.0],
    dbound=[4.0, 45.0, 1.0],
    bsz=4,
    nworkers=4,
    lr=1e-3,
    weight_decay=1e-7,
    val_step=500,
    save_step=1000,
    resume=None,
    use_wandb=True,
    wandb_project="lift-splat-shoot",
    wandb_name=None,
    wandb_entity=None,
    *,
    graph=True,
    dtype="bf16",
    miopen_find=True,
    seed=None,
    max_steps=None,
    skip_nonfinite=True,
    loss_step=10,
    iou_step=100,
    cycle_batches=0,
    on_start: Optional[Callable[[dict], None]] = None,
    label_groups=None,
    loss="bce",
    focal_gamma=2.0,
    focal_alpha=None,
    iou_thresholds=None,
    lr_schedule="constant",
    warmup_steps=0,
    warmup_factor=0.0,
    lr_min=0.0,
    lr_total_steps=None,
    ema_decay=0.0,
    ema_warmup=True,
    bev_rot_lim=(0.0, 0.0),
    bev_scale_lim=(1.0, 1.0),
    bev_flip=False,
    valid_mask=None,
    fov_z=(0.0,),
    exclusive=False,
    class_weight=None,
    photo_brightness=0.0,
    photo_contrast=(1.0, 1.0),
    photo_saturation=(1.0, 1.0),
    photo_hue=0.0,
    photo_noise=(0.0, 0.0),
    photo_prob=0.5,
    photo_per_camera=True,
):
    """Train LiftSplatShoot on a SimBEV tree; the reference's arguments (train_simbev.py:23-98) plus:

    graph: replay the step as HIP graphs (False: the same loop, eager). dtype: "bf16" (autocast) or
    "fp32". miopen_find: torch.backends.cudnn.benchmark for this process. seed: torch's seed, and
    np.random is reseeded with ``seed + epoch`` at every epoch (None: as the reference, from the OS).
    max_steps: stop after this many steps of this call. skip_nonfinite: the guarded update.
    loss_step / iou_step: the cadence of the loss and of the IoU / skipped-step reads (the reference's
    10 and 100). cycle_batches: cycle this many pre-decoded batches instead of reading the loader
    (measurement). on_start: called once, before the first step, with the loop's objects.
    label_groups: K lists of BEV channels, one output class each (outC = K; None: the reference's vehicle
    mask [[1, 2, 3]], outC = 1); pos_weight is then a float or a list of K. With K > 1 the ``val`` and
    ``train_iou`` events carry ``iou_per_class`` and ``iou`` is the mean over the classes seen.
    pos_weight: None is the reference's 2.13. loss: "bce", or "focal" -- tools.FocalLoss(K, focal_gamma,
    focal_alpha), each a float or a list of K; pos_weight is then the focal loss's w_pos (None: 1) unless
    focal_alpha is given, and giving both raises ValueError before anything is built. iou_thresholds: a ladder of
    probability thresholds; validation then also counts the IoU at each, and the ``val`` events carry ``iou_max``,
    ``iou_max_per_class`` and ``best_threshold_per_class``. ``model_best.pt`` is chosen by ``iou`` (at 0.5) all the
    same. With either option metrics.jsonl starts with a ``config`` event naming the loss and the ladder.
    lr_schedule: "constant", "linear" or "cosine" (optim.LRSchedule): a linear warm-up over warmup_steps updates from
    lr * warmup_factor, then the decay to lr_min (absolute) at update lr_total_steps (default: the run's length,
    nepochs * batches per epoch), flat afterwards. The captured update computes the rate on the device from Adam's
    own step count, so a skipped step does not advance the schedule and a resumed run continues it; the ``train``
    events then carry ``lr``. ema_decay > 0: an exponential moving average of the weights, kept by the same
    optimizer pass (ema_warmup: decay min(ema_decay, (1 + t) / (10 + t))); validation then runs on the averaged
    weights (``val`` events carry ``"weights": "ema"``, ``model_best.pt`` is chosen by that IoU) and checkpoints gain
    ``ema_state_dict``. With either, metrics.jsonl starts with the ``config`` event.
    bev_rot_lim (degrees), bev_scale_lim, bev_flip: the BEV-space augmentation of the training samples -- one rotation
    about the ego z axis, one isotropic scale and, with bev_flip, a coin each for x and y, drawn per sample after the
    image augmentation's values; the rig is composed with it on the host and the labels are warped by the staging
    stream's label kernel (simbev.class_masks, index_mats=). Validation is never augmented, the captured step and the
    checkpoints do not change, and the neutral defaults leave the loader exactly as it was. When on, the ``config``
    event carries the three values.
    valid_mask: None / "none", "grid" or "fov" -- the loss and every metric then count valid cells only: cells whose
    label source lies inside the labelled grid under the BEV-space augmentation ("grid") and that some camera sees at
    one of the heights fov_z, metres ("fov": inside the frustum of dbound and final_dim). The mask is made per batch on
    the staging stream (simbev.valid_mask), for validation batches too; the step stays captured. The ``config`` event
    then carries ``valid_mask`` and ``fov_z``, ``val`` events gain ``valid_fraction``, and the training IoU counts
    valid cells. Off, nothing differs. Argument errors raise ValueError before anything is looked for or built.
    ncams: 1 to 6 cameras per training sample, drawn at random per sample (the reference's ``Ncams``; see the module
    docstring); validation always runs at six. With valid_mask "fov" a training sample's mask comes from the cameras
    it holds, so a cell only a dropped camera would see is invalid in that sample. Checkpoints do not depend on it: a
    run resumes at any ncams.
    exclusive: every cell has exactly one class -- 0 the background, k + 1 label group k, the groups painted in order
    so that a later group wins (needs label_groups, 1 to 7 groups). The labels are the (B, X, Y) uint8 class map
    (simbev.class_index on the staging stream), the model has outC = K + 1, the loss is tools.SoftmaxLoss with
    class_weight (K + 1 weights, default all 1) and the metrics come from a confusion matrix (``lss_confusion_accum``):
    ``val`` and ``train_iou`` events carry tools.confusion_summary's keys, ``iou`` is the mean IoU of the foreground
    classes seen (None when there is none: such a validation never replaces the best). pos_weight, loss="focal",
    focal_gamma / focal_alpha and iou_thresholds with it raise ValueError before anything is built. The ``config``
    event records ``exclusive`` and ``class_weight``. Works with the BEV-space augmentation, the valid-cell mask,
    ncams, the schedules, the EMA and resume as the sigmoid mode does.
    photo_brightness (+-, 0..255 units), photo_contrast (lo, hi), photo_saturation (lo, hi), photo_hue (+- degrees),
    photo_noise (sigma lo, hi; 0..255 units): the photometric augmentation of the training images -- per camera
    (photo_per_camera False: per sample), each colour op applied with probability photo_prob at a value drawn from its
    range, the noise always at a drawn sigma, all drawn after the sample's other draws (simbev.draw_photo_augmentation)
    and applied by the staging stream's image kernel (``lss_simbev_images_photo``) to the resampled pixel before the
    normalisation. Validation is never augmented, the captured step and the checkpoints do not change, and the neutral
    defaults leave the loader exactly as it was. When on, the ``config`` event carries the seven values.
    Returns a summary dict (counter, epoch, best_val_iou, skipped, frames_per_s of the training steps)."""
    from . import checkpoint, simbev, tools

    ncams = _check_ncams(ncams)
    exclusive = bool(exclusive)
    if exclusive:
        class_weight = _exclusive_setup(label_groups, class_weight, pos_weight, loss, focal_gamma, focal_alpha,
                                        parse_thresholds(iou_thresholds))
    elif class_weight is not None:
        raise ValueError("class_weight is the exclusive loss's: it needs exclusive=True")
    pos_weight, focal = _loss_setup(loss, pos_weight, focal_gamma, focal_alpha)
    iou_thresholds = parse_thresholds(iou_thresholds)
    label_groups, n_out, pos_weight = _class_setup(label_groups, pos_weight)
    if exclusive:
        n_out += 1  # the background
    if focal is not None:
        tools.focal_rows(n_out, **focal)  # (argument errors come before anything is looked for or built)
    sched_on = _schedule_setup(lr, lr_schedule, warmup_steps, warmup_factor, lr_min, lr_total_steps, ema_decay)
    ema_on = float(ema_decay) > 0.0
    bev_aug_conf = {"bev_rot_lim": tuple(float(v) for v in bev_rot_lim),
                    "bev_scale_lim": tuple(float(v) for v in bev_scale_lim), "bev_flip": bool(bev_flip)}
    bev_on = simbev.bev_aug_enabled(bev_aug_conf)
    photo_aug_conf = photo_conf(photo_brightness, photo_contrast, photo_saturation, photo_hue, photo_noise, photo_prob,
                                photo_per_camera)
    photo_on = simbev.photo_draws(photo_aug_conf)
    mask_conf = {"valid_mask": valid_mask, "fov_z": parse_heights(fov_z, "fov_z")}
    mask_mode = simbev.valid_mask_mode(mask_conf)
    if gpuid < 0 or not torch.cuda.is_available():
        raise RuntimeError("lss_carla_amd.trainer: needs an MI355X (the hot path has no CPU fallback)")
    if dtype not in ("bf16", "fp32"):
        raise ValueError(f"dtype {dtype!r}: bf16 or fp32")
    if resume is not None and os.path.exists(resume):
        _check_head_classes(resume, n_out)  # before anything is built, loaded or captured
    os.makedirs(logdir, exist_ok=True)
    grid_conf = {"xbound": xbound, "ybound": ybound, "zbound": zbound, "dbound": dbound}
    data_aug_conf = {"resize_lim": resize_lim, "final_dim": final_dim, "rot_lim": rot_lim, "H": H, "W": W,
                     "rand_flip": rand_flip, "bot_pct_lim": bot_pct_lim, "Ncams": ncams}
    if bev_on:
        data_aug_conf.update(bev_aug_conf)
    if mask_mode is not None:
        data_aug_conf.update({"valid_mask": mask_mode, "fov_z": mask_conf["fov_z"]})
    if photo_on:
        data_aug_conf.update(photo_aug_conf)
    config = {"dataroot": str(dataroot), "nepochs": nepochs, "batch_size": bsz, "learning_rate": lr,
              "weight_decay": weight_decay, "num_workers": nworkers, "num_cameras": ncams, "image_H": H, "image_W": W,
              "final_dim": list(final_dim), "max_grad_norm": max_grad_norm, "pos_weight": pos_weight,
              "grid_conf": grid_conf, "val_step": val_step, "save_step": save_step, "graph": bool(graph),
              "dtype": dtype, "seed": seed}
    if label_groups is not None:
        config["label_groups"] = label_groups
    if focal is not None or iou_thresholds is not None:
        config["loss"] = loss
        config["iou_thresholds"] = iou_thresholds
        if focal is not None:
            config["focal_gamma"], config["focal_alpha"] = focal_gamma, focal_alpha
            if focal_alpha is not None:
                config["pos_weight"] = None  # (alpha sets the class balance)
    if sched_on:
        config.update({"lr_schedule": lr_schedule, "warmup_steps": int(warmup_steps), "warmup_factor": float(warmup_factor),
                       "lr_min": float(lr_min), "lr_total_steps": lr_total_steps})
    if ema_on:
        config.update({"ema_decay": float(ema_decay), "ema_warmup": bool(ema_warmup)})
    if bev_on:
        config.update({k: list(v) if isinstance(v, tuple) else v for k, v in bev_aug_conf.items()})
    if mask_mode is not None:
        config.update({"valid_mask": mask_mode, "fov_z": list(mask_conf["fov_z"])})
    if exclusive:
        config.update({"exclusive": True, "class_weight": class_weight, "pos_weight": None})
    if photo_on:
        config.update({"photo_brightness": float(photo_brightness), "photo_contrast": list(photo_aug_conf["photo_contrast_lim"]),
                       "photo_saturation": list(photo_aug_conf["photo_saturation_lim"]), "photo_hue": float(photo_hue),
                       "photo_noise": list(photo_aug_conf["photo_noise_lim"]), "photo_prob": float(photo_prob),
                       "photo_per_camera": bool(photo_per_camera)})
    log = _Log(logdir, use_wandb, {"project": wandb_project, "name": wandb_name, "entity": wandb_entity}, config)

    if ("loss" in config or bev_on or mask_mode is not None or exclusive or photo_on) and not (sched_on or ema_on):
        log.event("config", 0, **config)

    device = torch.device(f"cuda:{gpuid}")
    torch.cuda.set_device(device)
    torch.backends.cudnn.benchmark = bool(miopen_find)
    if seed is not None:
        torch.manual_seed(seed)
        np.random.seed(seed)
    trainloader, valloader = simbev.compile_data("unused", dataroot, data_aug_conf, grid_conf, bsz, nworkers,
                                                 "segmentationdata", device=device)
    train_raw, val_raw = trainloader.loader, valloader.loader  # raw batches: the stager finishes them
    if len(train_raw) == 0:
        raise RuntimeError(f"the training split has fewer than bsz={bsz} samples")
    if cycle_batches:
        train_raw = _Cycle(train_raw, int(cycle_batches))
    n_val = len(valloader.dataset)
    schedule = None
    if sched_on:
        from .optim import LRSchedule
        if lr_total_steps is None:
            lr_total_steps = config["lr_total_steps"] = int(nepochs) * len(train_raw)
        schedule = LRSchedule(lr_schedule, warmup_steps, warmup_factor, lr_total_steps, float(lr_min) / float(lr))
    if sched_on or ema_on:
        log.event("config", 0, **config)  # (the schedule's length is known only now)
    print(f"Train batches: {len(train_raw)}  Val batches: {len(val_raw)}  device {device}  graph {bool(graph)} {dtype}")

    ctx = build_step(grid_conf, data_aug_conf, bsz, device, dtype=dtype, lr=lr, weight_decay=weight_decay,
                     max_grad_norm=max_grad_norm, pos_weight=pos_weight, skip_nonfinite=skip_nonfinite,
                     n_val=n_val, label_groups=label_groups, loss=loss, focal_gamma=focal_gamma,
                     focal_alpha=focal_alpha, iou_thresholds=iou_thresholds, lr_schedule=schedule,
                     ema_decay=float(ema_decay), ema_warmup=ema_warmup, ncams=ncams,
                     **({"exclusive": True, "class_weight": class_weight} if exclusive else {}))
    emas = ctx["emas"]
    model, flat, masters, opt = ctx["model"], ctx["flat"], ctx["masters"], ctx["opt"]
    stager, step, evaluate = ctx["stager"], ctx["step"], ctx["evaluate"]
    val_stager = ctx["val_stager"]  # the stager itself at ncams = 6

    counter, start_epoch = 0, 0
    if resume is not None and os.path.exists(resume):
        counter, start_epoch = checkpoint.load_checkpoint(resume, model, flat, opt)
        print(f"Resumed from epoch {start_epoch}, iteration {counter}")
    start_counter = counter
    for m in masters:
        checkpoint.init_state(opt, m)  # the state tensors exist (at fixed addresses) before any capture

    def snapshot():
        return ([t.detach().clone() for t in model.state_dict().values()],
                [{k: v.detach().clone() for k, v in opt.state[m].items()} for m in masters],
                [e.clone() for e in emas or []])

    def restore(snap):
        with torch.no_grad():
            for t, s in zip(model.state_dict().values(), snap[0]):
                t.copy_(s)
            for m, st in zip(masters, snap[1]):
                for k, v in st.items():
                    opt.state[m][k].copy_(v)
            for e, s in zip(emas or [], snap[2]):
                e.copy_(s)
            if step.skipped is not None:
                step.skipped.zero_()

    def save(path, epoch, val_iou=None):
        checkpoint.save_checkpoint(path, model, flat, opt, counter, epoch, val_iou)

    def validate():
        """EvalStep over the val loader through the validation stager (at ncams = 6 the training stager: no
        training batch is staged meanwhile)."""
        it = iter(val_raw)
        val_stager.stage(next(it))
        first = True
        for _ in range(len(val_raw)):
            val_stager.commit()
            if first and graph and not evaluate.captured:
                evaluate.capture(warmup=1, error_mode="thread_local")  # on the first validation batch; resets the totals
            if first:
                evaluate.reset()
                first = False
            evaluate()
            nxt = next(it, None)
            if nxt is not None:
                val_stager.stage(nxt)
        return evaluate.read()

    best_val_iou = -1.0
    last_loss = None
    t_train, n_timed, t_mark = 0.0, 0, None
    started = False
    done = False
    epoch = start_epoch
    for epoch in range(start_epoch, nepochs):
        np.random.seed(None if seed is None else seed + epoch)
        it = iter(train_raw)
        nxt = next(it, None)
        if nxt is not None:
            stager.stage(nxt)
        while nxt is not None:
            stager.commit()
            if not started:
                started = True
                if graph:
                    # the warm-up steps of the capture are real updates: undo them
                    snap = snapshot()
                    step.capture(warmup=2, error_mode="thread_local")
                    restore(snap)
                    del snap
                if on_start is not None:
                    on_start({"model": model, "flat": flat, "opt": opt, "step": step, "stager": stager,
                              "val_stager": val_stager, "counter": counter, "epoch": epoch})
                torch.cuda.synchronize(device)
                t_mark = time.perf_counter()
            will_val = (counter + 1) % val_step == 0
            loss = step()
            counter += 1
            n_timed += 1
            nxt = None
            if max_steps is not None and counter - start_counter >= max_steps:
                done = True
            elif not will_val:
                nxt = next(it, None)  # staged while the step runs
                if nxt is not None:
                    stager.stage(nxt)
            if counter % loss_step == 0:
                last_loss = float(loss.item())
                extra = {"lr": float(step.lr.item())} if schedule is not None else {}
                log.event("train", counter, epoch=epoch, loss=last_loss, **extra)
            if counter % iou_step == 0:
                extra = {}
                iou_pred, iou_tgt = step.static_preds, stager.binimgs
                if exclusive:  # the batch's confusion matrix, on the tensors the sigmoid path reads
                    tot = torch.zeros(1 + n_out * n_out, device=device, dtype=torch.float64)
                    tools.confusion_accumulate(iou_pred, iou_tgt, tot, None, ctx["loss_fn"].class_weight,
                                               valid=stager.valid if mask_mode is not None else None)
                    binfo = tools.confusion_summary(tot, n_out, bsz)
                    iou = binfo["iou"]
                    extra = {k: binfo[k] for k in EXCLUSIVE_KEYS}
                elif mask_mode is not None:  # valid cells only: masked-out cells are neither predicted nor labelled
                    on = (stager.valid != 0).unsqueeze(1)
                    iou_pred = torch.where(on, iou_pred.float(), torch.full((), -1.0, device=device))
                    iou_tgt = torch.where(on, iou_tgt, torch.zeros((), device=device))
                if exclusive:
                    pass
                elif n_out > 1:
                    ci, cu = tools.get_batch_iou_per_class(iou_pred, iou_tgt)
                    ci, cu = ci.tolist(), cu.tolist()
                    extra["iou_per_class"] = [i / u if u > 0 else None for i, u in zip(ci, cu)]
                    seen = [v for v in extra["iou_per_class"] if v is not None]
                    iou = sum(seen) / len(seen) if seen else 1.0  # (get_batch_iou's value for an empty union)
                else:
                    _, _, iou = tools.get_batch_iou(iou_pred, iou_tgt)
                skipped = int(step.skipped.item()) if step.skipped is not None else 0
                log.event("train_iou", counter, epoch=epoch, iou=iou, skipped=skipped, **extra)
            if will_val or counter % save_step == 0:
                torch.cuda.synchronize(device)
                t_train += time.perf_counter() - t_mark
            if will_val:
                info = validate()
                print(f"  Validation at {counter} - Loss: {info['loss']:.4f}, IoU: "
                      + ("none" if info["iou"] is None else f"{info['iou']:.4f}"))
                extra = {"iou_per_class": info["iou_per_class"]} if n_out > 1 else {}
                if exclusive:
                    extra = {k: info[k] for k in EXCLUSIVE_KEYS}
                if iou_thresholds is not None:
                    extra.update({k: info[k] for k in ("iou_max", "iou_max_per_class", "best_threshold_per_class")})
                if ema_on:
                    extra["weights"] = "ema"
                if mask_mode is not None:
                    extra["valid_fraction"] = info["valid_fraction"]
                log.event("val", counter, epoch=epoch, loss=info["loss"], iou=info["iou"], **extra)
                if info["iou"] is not None and info["iou"] > best_val_iou:
                    best_val_iou = info["iou"]
                    save(os.path.join(logdir, "model_best.pt"), epoch, best_val_iou)
            if counter % save_step == 0:
                save(os.path.join(logdir, f"model_{counter:06d}.pt"), epoch)
            if will_val or counter % save_step == 0:
                t_mark = time.perf_counter()
            if will_val and not done:
                nxt = next(it, None)
                if nxt is not None:
                    stager.stage(nxt)
            if done:
                break
        if done:
            break
    torch.cuda.synchronize(device)
    if t_mark is not None:
        t_train += time.perf_counter() - t_mark
    final_epoch = epoch if done else nepochs
    save(os.path.join(logdir, "model_final.pt"), final_epoch)
    skipped = int(step.skipped.item()) if step.skipped is not None else 0
    if started:
        last_loss = float((step.static_loss if step.captured else loss).item())
    fps = n_timed * bsz / t_train if t_train > 0 else 0.0
    log.event("final", counter, epoch=final_epoch, loss=last_loss, skipped=skipped, frames_per_s=fps,
              best_val_iou=best_val_iou if best_val_iou >= 0 else None)
    log.close()
    print(f"Training complete at iteration {counter}; best validation IoU: {max(best_val_iou, 0.0):.4f}")
    return {"counter": counter, "epoch": final_epoch, "best_val_iou": best_val_iou if best_val_iou >= 0 else None,
            "skipped": skipped, "frames_per_s": fps, "loss": last_loss}


def _check_head_classes(path, n_out: int) -> None:
    """A checkpoint whose head (bevencode.up2.4) has another number of output classes than this run's
    label_groups ask for cannot be resumed: say so with both numbers."""
    ckpt = torch.load(path, map_location="cpu")
    sd = ckpt["model_state_dict"] if isinstance(ckpt, dict) and "model_state_dict" in ckpt else ckpt
    w = sd.get("bevencode.up2.4.weight") if isinstance(sd, dict) else None
    if w is not None and int(w.shape[0]) != n_out:
        raise RuntimeError(f"resume: the checkpoint {path} has a head of {int(w.shape[0])} output classes "
                           f"(bevencode.up2.4.weight {tuple(w.shape)}), this run's label_groups ask for {n_out}")


def main(argv=None):
    p = argparse.ArgumentParser(description="Train LSS on a SimBEV dataset (captured step on the MI355X)")
    p.add_argument("--dataroot", type=str, required=True, help="SimBEV dataset root directory")
    p.add_argument("--nepochs", type=int, default=100)
    p.add_argument("--gpuid", type=int, default=0)
    p.add_argument("--bsz", type=int, default=4)
    p.add_argument("--nworkers", type=int, default=4)
    p.add_argument("--lr", type=float, default=1e-3)
    p.add_argument("--weight_decay", type=float, default=1e-7)
    p.add_argument("--H", type=int, default=224)
    p.add_argument("--W", type=int, default=480)
    p.add_argument("--final_h", type=int, default=128)
    p.add_argument("--final_w", type=int, default=352)
    p.add_argument("--ncams", type=int, default=6)
    p.add_argument("--logdir", type=str, default="./runs/simbev")
    p.add_argument("--val_step", type=int, default=500)
    p.add_argument("--save_step", type=int, default=1000)
    p.add_argument("--resume", type=str, default=None)
    p.add_argument("--use_wandb", action="store_true", default=False)
    p.add_argument("--wandb_project", type=str, default="lift-splat-shoot")
    p.add_argument("--wandb_name", type=str, default=None)
    p.add_argument("--wandb_entity", type=str, default=None)
    # beyond the reference's flags
    p.add_argument("--graph", type=int, default=1, help="0: the same loop, eager")
    p.add_argument("--dtype", default="bf16", choices=["bf16", "fp32"])
    p.add_argument("--miopen_find", type=int, default=1)
    p.add_argument("--seed", type=int, default=None)
    p.add_argument("--max_steps", type=int, default=None)
    p.add_argument("--skip_nonfinite", type=int, default=1)
    p.add_argument("--label_groups", type=str, default=None,
                   help='BEV channel groups, one output class each: "0;1,2,3;6,7" (default: the vehicle mask 1,2,3)')
    p.add_argument("--pos_weight", type=str, default=None,
                   help="one positive-class weight, or one per class: 1.0,2.13,5.0 (default 2.13; with --loss focal: w_pos, default 1)")
    p.add_argument("--loss", default="bce", choices=["bce", "focal"])
    p.add_argument("--focal_gamma", type=str, default="2.0", help="focal loss: one gamma, or one per class: 2.0,2.0,1.0")
    p.add_argument("--focal_alpha", type=str, default=None,
                   help="focal loss: one alpha in (0, 1), or one per class (instead of --pos_weight)")
    p.add_argument("--iou_thresholds", type=str, default=None,
                   help="validation also reports the IoU at these probability thresholds and the best per class: "
                        "0.35,0.4,0.45,0.5,0.55,0.6,0.65")
    p.add_argument("--lr_schedule", default="constant", choices=["constant", "linear", "cosine"],
                   help="the decay after the warm-up, computed on the device from Adam's step count")
    p.add_argument("--warmup_steps", type=int, default=0, help="linear warm-up over this many updates")
    p.add_argument("--warmup_factor", type=float, default=0.0, help="the warm-up starts at lr * this")
    p.add_argument("--lr_min", type=float, default=0.0, help="the learning rate the decay ends at (absolute)")
    p.add_argument("--lr_total_steps", type=int, default=None,
                   help="the update the decay ends at (default: nepochs * batches per epoch)")
    p.add_argument("--ema_decay", type=float, default=0.0,
                   help="> 0: keep an EMA of the weights; validation and model_best.pt use it")
    p.add_argument("--ema_warmup", type=int, default=1, help="EMA decay min(ema_decay, (1 + t) / (10 + t))")
    p.add_argument("--bev_rot_lim", type=str, default="0,0",
                   help="BEV-space augmentation: rotation about the ego z axis, degrees, lo,hi (e.g. -22.5,22.5)")
    p.add_argument("--bev_scale_lim", type=str, default="1,1",
                   help="BEV-space augmentation: isotropic scale of the ego frame, lo,hi (e.g. 0.9,1.1)")
    p.add_argument("--bev_flip", type=int, default=0, choices=[0, 1],
                   help="BEV-space augmentation: flip x and y of the ego frame, a coin each")
    p.add_argument("--valid_mask", default="none", choices=["none", "grid", "fov"],
                   help="count only valid cells in the loss and the metrics: inside the labelled grid under the BEV-space "
                        "augmentation (grid), and seen by a camera (fov)")
    p.add_argument("--fov_z", type=str, default="0.0",
                   help="--valid_mask fov: the heights (metres) a cell is tested at, 1 to 8: 0.0[,1.5,...]")
    p.add_argument("--exclusive", type=int, default=0, choices=[0, 1],
                   help="1: exclusive classes -- the label groups painted in order into one class map (0 the background), "
                        "softmax cross-entropy, confusion-matrix mIoU; needs --label_groups")
    p.add_argument("--class_weight", type=str, default=None,
                   help="--exclusive 1: one weight per class, the background first: w0,...,wK (default all 1)")
    p.add_argument("--photo_brightness", type=float, default=0.0,
                   help="photometric augmentation: brightness shift, +- this many 0..255 units (e.g. 32)")
    p.add_argument("--photo_contrast", type=str, default="1,1",
                   help="photometric augmentation: contrast about mid-grey, lo,hi (e.g. 0.5,1.5)")
    p.add_argument("--photo_saturation", type=str, default="1,1",
                   help="photometric augmentation: saturation, lo,hi (e.g. 0.5,1.5)")
    p.add_argument("--photo_hue", type=float, default=0.0, help="photometric augmentation: hue rotation, +- degrees (e.g. 18)")
    p.add_argument("--photo_noise", type=str, default="0,0",
                   help="photometric augmentation: sensor noise sigma in 0..255 units, lo,hi (e.g. 0,8)")
    p.add_argument("--photo_prob", type=float, default=0.5, help="the probability of each colour op")
    p.add_argument("--photo_per_camera", type=int, default=1, choices=[0, 1],
                   help="1: one draw per camera; 0: one per sample, shared by its cameras")
    a = p.parse_args(argv)
    if a.exclusive:  # the sigmoid mode's flags are errors here, before anything is built
        _exclusive_setup(parse_label_groups(a.label_groups),
                         None if a.class_weight is None else _weights_list(a.class_weight),
                         None if a.pos_weight is None else parse_pos_weight(a.pos_weight), a.loss,
                         parse_per_class(a.focal_gamma, "--focal_gamma"),
                         None if a.focal_alpha is None else parse_per_class(a.focal_alpha, "--focal_alpha"),
                         parse_thresholds(a.iou_thresholds))
    elif a.class_weight is not None:
        raise ValueError("--class_weight needs --exclusive 1")
    return train(dataroot=a.dataroot, nepochs=a.nepochs, gpuid=a.gpuid, H=a.H, W=a.W, final_dim=(a.final_h, a.final_w),
                 ncams=a.ncams, bsz=a.bsz, nworkers=a.nworkers, lr=a.lr, weight_decay=a.weight_decay, logdir=a.logdir,
                 val_step=a.val_step, save_step=a.save_step, resume=a.resume, use_wandb=a.use_wandb,
                 wandb_project=a.wandb_project, wandb_name=a.wandb_name, wandb_entity=a.wandb_entity,
                 graph=bool(a.graph), dtype=a.dtype, miopen_find=bool(a.miopen_find), seed=a.seed,
                 max_steps=a.max_steps, skip_nonfinite=bool(a.skip_nonfinite),
                 label_groups=parse_label_groups(a.label_groups),
                 pos_weight=parse_pos_weight(a.pos_weight) if a.pos_weight is not None
                 else (None if a.loss == "focal" or a.exclusive else 2.13), loss=a.loss,
                 focal_gamma=parse_per_class(a.focal_gamma, "--focal_gamma"),
                 focal_alpha=None if a.focal_alpha is None else parse_per_class(a.focal_alpha, "--focal_alpha"),
                 iou_thresholds=parse_thresholds(a.iou_thresholds), lr_schedule=a.lr_schedule,
                 warmup_steps=a.warmup_steps, warmup_factor=a.warmup_factor, lr_min=a.lr_min,
                 lr_total_steps=a.lr_total_steps, ema_decay=a.ema_decay, ema_warmup=bool(a.ema_warmup),
                 bev_rot_lim=parse_pair(a.bev_rot_lim, "--bev_rot_lim"),
                 bev_scale_lim=parse_pair(a.bev_scale_lim, "--bev_scale_lim"), bev_flip=bool(a.bev_flip),
                 valid_mask=a.valid_mask, fov_z=parse_heights(a.fov_z),
                 photo_brightness=a.photo_brightness, photo_contrast=parse_pair(a.photo_contrast, "--photo_contrast"),
                 photo_saturation=parse_pair(a.photo_saturation, "--photo_saturation"), photo_hue=a.photo_hue,
                 photo_noise=parse_pair(a.photo_noise, "--photo_noise"), photo_prob=a.photo_prob,
                 photo_per_camera=bool(a.photo_per_camera),
                 **({"exclusive": True, "class_weight": None if a.class_weight is None else _weights_list(a.class_weight)}
                    if a.exclusive else {}))


if __name__ == "__main__":
    main()
