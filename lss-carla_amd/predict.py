"""Inference: ``Predictor`` and ``python -m lss_carla_amd.predict``.

What the reference's users do with a trained network (``src/explore.py:244-246`` eval_model_iou, ``:317-328``
viz_model_preds: ``model.eval()``, ``no_grad``, ``out.sigmoid()``), built from the pieces the training loop
already has -- static inputs, ``ops.HostInverses`` behind ``model.static_inverses``, ``FlatParams`` for the
bf16 working weights and the prepacked depthnet weight, autocast, one HIP graph -- so a caller does not have to
rebuild ``EvalStep`` by hand:

    p = L.Predictor(model, bsz, device, amp_dtype=torch.bfloat16, threshold=0.5, graph=True)
    p.load(path)                     # explore.py's plain state_dict, or train_simbev.py's {"model_state_dict": ...}
                                     # (weights="auto": a trainer checkpoint's EMA weights when it carries them)
    logits = p(imgs, rots, trans, intrins, post_rots, post_trans)    # host or device tensors, b <= bsz samples
    p.probs(); p.masks()             # sigmoid as fp32; uint8 (b, K, X, Y) = logits > logit(threshold)

The forward runs in eval mode without gradients, so every batch norm takes ``lss_bn_eval`` (norm.py), the
MBConv skips ride in bn2's pass and BevEncode's tail never writes its normalised map. The working parameters
are materialised once (construction, ``load()``, ``refresh()``): the replayed graph holds no weight casts.
Eval mode has no op across samples, so a batch of b < bsz samples fills samples 0..b-1 of the static inputs and
reads the first b of the outputs; the rest keep whatever they held. Returned tensors are views of static
buffers, valid until the next call. A call does not synchronise the host, HostInverses' bounded wait (two
calls ahead at most) apart -- except for a rig handed over as device tensors without host copies attached
(``t._lss_host``, as simbev.finish_batch attaches them), which is read back once: pass the rig on the host.

Dead cameras. ``Predictor(..., camera_mask=True)`` captures the forward with the masked plan kernels
(``LiftSplatShoot.camera_alive``): the Predictor owns a static (bsz, N) uint8 ``alive`` tensor, all ones, that the
plan reads on the device, so ONE captured graph serves every pattern of dead cameras, per sample:

    p = L.Predictor(model, bsz, device, camera_mask=True)
    p.set_alive([1, 1, 0, 1, 1, 1])          # (N,) for every sample, or (b, N); bool / uint8, host or device
    logits = p(imgs, ..., alive=mask)        # the same, per call

A dead camera's frustum points are dropped from the splat, exactly as if they fell outside the grid; its images
still pass through the trunk and the lift (eval mode has no op across images, so they change nothing else). A
Predictor built without ``camera_mask`` captures the unmasked graph, as before, and refuses both calls.

The model's parameters are moved into the Predictor's flat fp32 master (FlatParams; same values, same
state_dict): build it on a model no training step is bound to. The hot path has no CPU fallback.

    python -m lss_carla_amd.predict --modelf CKPT --dataroot ROOT --out DIR [--bsz N] [--label_groups "0;1,2,3"]
                                    [--dtype bf16|fp32] [--graph 0|1] [--threshold 0.5 | 0.45,0.5,0.35]
                                    [--loss bce|focal] [--focal_gamma G] [--focal_alpha A] [--iou_thresholds 0.35,...]
                                    [--weights auto|ema|model] [--valid_mask none|grid|fov] [--fov_z 0.0[,1.5,...]]
                                    [--drop_cams front,back_left] [--drop_each 0|1]
                                    [--exclusive 0|1] [--class_weight w0,...,wK]
                                    [--photo "brightness=-40,contrast=0.8,noise=8"]

runs the val split through ``BatchStager`` and the Predictor and writes one uint8 mask array per sample
(``DIR/<index>.npy``, (K, X, Y)) and ``DIR/metrics.json``: loss, IoU and per-class IoU from get_val_info's
accumulators (``tools.val_accumulate``), and frames/s. ``--threshold`` takes one probability or one per class.
With ``--loss focal`` or ``--iou_thresholds`` the totals come from ``tools.seg_metrics_accumulate`` instead: the loss
is the chosen one (``loss_kind``), the IoU keys are the 0.5 column's, and a ladder adds ``iou_at``,
``iou_max_per_class``, ``best_threshold_per_class`` and ``iou_max``. With ``--valid_mask grid|fov`` the totals come from
the masked form of that accumulate (``lss_seg_metrics_accum_masked``): loss and IoU are over valid cells (simbev.valid_mask),
``metrics.json`` gains ``valid_mask`` and ``valid_fraction``, and each sample's mask is written to ``DIR/valid/<index>.npy``
((X, Y) uint8); the written prediction masks are unchanged. The matplotlib figures of explore.py are not drawn.
``--drop_cams`` (names of ``simbev.CAMERA_ORDER``, or indices) runs the split with those cameras dead in every sample
(``metrics.json`` gains ``dropped_cams``). ``--drop_each 1`` runs the split once more per camera after the normal pass,
that camera dead (besides any of --drop_cams), on the same graph, and writes ``"drop_each": {name: {"loss", "iou", ...}}``
-- the missing-camera table; prediction masks are written for the normal pass only. With ``--valid_mask fov`` a dead
camera makes no cell valid (simbev.fov_cameras(alive=)).
``--exclusive 1`` (with ``--label_groups``, 1 to 7 groups; ``--class_weight`` the K + 1 loss weights, default 1) runs a
model of exclusive classes: the labels are the painted class map (simbev.class_index), each sample's argmax class map
((X, Y) uint8, ``lss_argmax_classes``) is written to ``DIR/preds/<index>.npy``, and ``metrics.json`` -- and each
``drop_each`` entry -- carries ``tools.confusion_summary``'s keys (loss, iou over the foreground classes, iou_per_class,
miou_all, pixel_acc, precision / recall per class, confusion) from ``lss_confusion_accum``. ``--threshold``,
``--pos_weight``, ``--loss focal``, ``--focal_*`` and ``--iou_thresholds`` with it are errors before anything is built.
``--photo "brightness=-40,contrast=0.8,noise=8"`` (entries: brightness, contrast, saturation, hue, noise, seed) runs the
split with that one photometric shift applied to every image by the staging stream's image kernel
(``lss_simbev_images_photo``; the loader's ``photo_fixed``): how the metrics move at dusk, or with a noisy sensor.
``metrics.json`` gains ``photo`` (the parsed dict); without the flag nothing changes.
"""
from __future__ import annotations

import argparse
import json
import math
import os
import time
from typing import Optional, Sequence

import torch

HEAD_WEIGHT = "bevencode.up2.4.weight"  # BevEncode's last conv (src/models.py:115): (outC, 128, 1, 1)


def threshold_logit(threshold: float) -> float:
    """The logit a probability threshold corresponds to: sigmoid(x) > t  <=>  x > log(t / (1 - t)).
    0.5 -> 0.0 exactly, get_batch_iou's predicate (src/tools.py:232-240: ``preds > 0``)."""
    t = float(threshold)
    if not 0.0 < t < 1.0:
        raise ValueError(f"threshold {threshold!r}: a probability strictly between 0 and 1")
    return 0.0 if t == 0.5 else math.log(t / (1.0 - t))


WEIGHTS = ("auto", "ema", "model")


def model_state_dict(ckpt, weights: str = "model") -> dict:
    """The model's state dict out of either checkpoint format: train_simbev.py's dict with
    ``"model_state_dict"`` (train_simbev.py:206-212), or explore.py's plain ``model.state_dict()``.
    weights: "model"; "ema": the trainer checkpoint's ``ema_state_dict`` (ValueError when it has none);
    "auto": the EMA when the file has one, else the model's."""
    if weights not in WEIGHTS:
        raise ValueError(f"weights {weights!r}: one of {', '.join(WEIGHTS)}")
    if isinstance(ckpt, dict) and "model_state_dict" in ckpt:
        if weights == "ema" and "ema_state_dict" not in ckpt:
            raise ValueError("weights='ema': the checkpoint has no ema_state_dict")
        ckpt = ckpt["ema_state_dict" if weights != "model" and "ema_state_dict" in ckpt else "model_state_dict"]
    elif weights == "ema":
        raise ValueError("weights='ema': a bare state dict has no ema_state_dict")
    if not isinstance(ckpt, dict) or not ckpt or not all(isinstance(k, str) and torch.is_tensor(v)
                                                         for k, v in ckpt.items()):
        raise ValueError("not a model checkpoint: neither a state_dict nor a dict holding 'model_state_dict'")
    return ckpt


def checkpoint_format(ckpt) -> str:
    """'trainer' (a dict holding "model_state_dict") or 'state_dict' (the bare dict); ValueError otherwise."""
    model_state_dict(ckpt)
    return "trainer" if "model_state_dict" in ckpt else "state_dict"


def check_head(sd: dict, n_out: int, what: str = "checkpoint") -> None:
    """A state dict whose head has another number of output classes than the model cannot be loaded: say so
    with both numbers, before anything else happens."""
    w = sd.get(HEAD_WEIGHT)
    if w is not None and int(w.shape[0]) != int(n_out):
        raise RuntimeError(f"{what}: a head of {int(w.shape[0])} output classes ({HEAD_WEIGHT} {tuple(w.shape)}), "
                           f"the model has {int(n_out)}")


def _require_gpu(device) -> torch.device:
    dev = torch.device(device)
    if dev.type != "cuda" or not torch.cuda.is_available():
        raise RuntimeError("lss_carla_amd.predict: needs an MI355X (the hot path has no CPU fallback)")
    return dev


class Predictor:
    RIG = ("rots", "trans", "intrins", "post_rots", "post_trans")

    def __init__(self, model: torch.nn.Module, bsz: int, device, amp_dtype: Optional[torch.dtype] = torch.bfloat16,
                 threshold=0.5, graph: bool = True, ncams: Optional[int] = None, stager=None,
                 camera_mask: bool = False, exclusive: bool = False):
        """model: a LiftSplatShoot on `device` (memory formats as the caller set them). bsz: the static batch.
        threshold: one probability, or one per output class (a sequence of K: e.g. the
        ``best_threshold_per_class`` of a validation over a ladder; ``masks()`` then compares in fp32 with the
        K logit thresholds, the predicate ``lss_seg_metrics_accum`` counts with).
        amp_dtype: autocast dtype (None: fp32). stager: a staging.BatchStager whose static tensors and
        inverses to run on (``run(b)`` after its ``commit()``); None: buffers of the Predictor's own, filled by
        ``__call__``. The graph is captured by the first call, on that call's inputs. camera_mask: run the masked
        plan kernels over the static ``alive`` tensor (``set_alive`` / ``alive=``); False: the unmasked forward.
        exclusive: the head's C outputs are exclusive classes (class 0 the background; trained with
        tools.SoftmaxLoss): ``classes()`` is the (b, X, Y) uint8 argmax map (``lss_argmax_classes``), ``probs()`` a
        softmax over the classes and ``masks()`` the (b, C - 1, X, Y) planes ``classes() == k + 1``. A threshold other
        than the default 0.5 is then a ValueError: an argmax has none."""
        if exclusive and not (isinstance(threshold, (int, float)) and float(threshold) == 0.5):  # (before any GPU work)
            raise ValueError("Predictor(exclusive=True): threshold= does not apply (the prediction is an argmax)")
        from . import ops
        from .flat_params import FlatParams

        dev = _require_gpu(device)
        per_class = not isinstance(threshold, (int, float)) and getattr(threshold, "ndim", None) != 0
        self.exclusive = bool(exclusive)
        self.logit = None if per_class else threshold_logit(threshold)
        self.thetas = None
        self.model, self.device, self.bsz, self.amp_dtype = model, dev, int(bsz), amp_dtype
        self.use_graph = bool(graph)
        conf = model.data_aug_conf
        N = int(ncams if ncams is not None else conf.get("Ncams", 6))
        fH, fW = (int(v) for v in conf["final_dim"])
        self.ncams = N
        self.n_out = int(model.state_dict()[HEAD_WEIGHT].shape[0])
        if self.exclusive and not 2 <= self.n_out <= 8:
            raise ValueError(f"Predictor(exclusive=True): a head of {self.n_out} outputs (2..8 classes)")
        if per_class:
            logits = [threshold_logit(v) for v in threshold]
            if len(logits) != self.n_out:
                raise ValueError(f"Predictor: {len(logits)} thresholds for {self.n_out} output classes")
            self.thetas = torch.tensor(logits, device=dev, dtype=torch.float32)
        self.stager = stager
        if stager is not None:
            if stager.B != self.bsz or stager.N != N or tuple(stager.final_dim) != (fH, fW):
                raise ValueError("Predictor: the stager's batch, cameras or image size differ from the model's")
            self.inputs = tuple(stager.inputs)
            self.hinv = stager.hinv
        else:
            B = self.bsz
            eye = torch.eye(3, device=dev).expand(B, N, 3, 3)
            self.inputs = (torch.zeros(B, N, 3, fH, fW, device=dev), eye.clone(), torch.zeros(B, N, 3, device=dev),
                           eye.clone(), eye.clone(), torch.zeros(B, N, 3, device=dev))
            self.hinv = ops.HostInverses(B * N, dev)
            # the host rig HostInverses inverts: samples past a partial batch keep their previous matrices
            self._host_post_rots = torch.eye(3).repeat(B, N, 1, 1)
            self._host_intrins = torch.eye(3).repeat(B, N, 1, 1)
        was_training = model.training
        try:
            self.flat = FlatParams(model, cast_dtype=amp_dtype)
            self.params = None
            self.refresh()
        finally:
            model.train(was_training)
        self.graph = None
        self._out = None
        self._b = 0
        # (bsz, N) uint8, all ones: what the masked plan kernels read; None: the unmasked forward
        self.alive = torch.ones(self.bsz, N, device=dev, dtype=torch.uint8) if camera_mask else None

    # ------------------------------------------------------------------ dead cameras
    def set_alive(self, mask) -> None:
        """Which cameras the splat uses from the next run on: (N,) for every sample, or (b, N) for the first b
        samples (the rest keep theirs); bool / uint8 / numbers (0 = dead), host or device. Copied into the static
        ``alive`` tensor on the current stream: no recapture."""
        if self.alive is None:
            raise RuntimeError("Predictor: built without camera_mask=True -- its forward has no camera mask")
        m = torch.as_tensor(mask)
        if m.dim() not in (1, 2) or m.shape[-1] != self.ncams or (m.dim() == 2 and not 0 < m.shape[0] <= self.bsz):
            raise ValueError(f"Predictor: an alive mask of shape {tuple(m.shape)}; ({self.ncams},) or "
                             f"(b <= {self.bsz}, {self.ncams})")
        m = (m != 0).to(torch.uint8)
        if m.dim() == 1:
            self.alive.copy_(m.to(self.device, non_blocking=True).expand_as(self.alive))
        else:
            self.alive[:m.shape[0]].copy_(m, non_blocking=True)

    # ------------------------------------------------------------------ weights
    def refresh(self) -> None:
        """Materialise the working parameters from the module's current ones (after changing them in place)."""
        with torch.no_grad():
            params = self.flat.tensors()  # writes work16 / work32 (and the packed depthnet weight) in place
        if self.params is None:
            self.params = {k: v.detach() for k, v in params.items()}  # views of the static working buffers

    def load(self, path, weights: str = "auto") -> None:
        """Load a checkpoint of either format into the module in place and refresh the working parameters; the
        head's width is checked first (nothing is loaded, materialised or captured when it differs). weights:
        "auto" takes a trainer checkpoint's ``ema_state_dict`` (the averaged weights validation chose the file by)
        when it has one, "ema" insists on it, "model" takes ``model_state_dict``."""
        sd = model_state_dict(torch.load(path, map_location="cpu"), weights)
        check_head(sd, self.n_out, f"checkpoint {path}")
        self.model.load_state_dict(sd)  # copies into the parameters (the master's memory) and the buffers
        self.refresh()

    # ------------------------------------------------------------------ forward
    def _forward(self) -> torch.Tensor:
        """One forward over the static inputs: eval mode, no_grad, autocast; the mode flag restored."""
        model = self.model
        was_training = model.training
        saved_inv = model.static_inverses
        saved_alive = getattr(model, "camera_alive", None)
        model.eval()
        model.static_inverses = (self.hinv.pinv, self.hinv.kinv)
        if self.alive is not None:
            model.camera_alive = self.alive
        try:
            capturing = torch.cuda.is_current_stream_capturing()
            with torch.no_grad(), torch.autocast("cuda", dtype=self.amp_dtype or torch.bfloat16,
                                                 enabled=self.amp_dtype is not None, cache_enabled=not capturing):
                return torch.func.functional_call(model, self.params, self.inputs, strict=False)
        finally:
            model.static_inverses = saved_inv
            if self.alive is not None:
                model.camera_alive = saved_alive
            model.train(was_training)

    def _capture(self) -> None:
        dev = self.device
        side = torch.cuda.Stream(dev)
        side.wait_stream(torch.cuda.current_stream(dev))
        with torch.cuda.stream(side):
            self._forward()  # warm-up: allocations, MIOpen's choices, the per-device workspaces
        torch.cuda.current_stream(dev).wait_stream(side)
        torch.cuda.synchronize(dev)
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            self._out = self._forward()
        self.graph = g

    def run(self, b: Optional[int] = None) -> torch.Tensor:
        """Launch the forward over the static inputs as they are (a stager's commit() filled them and staged
        the inverses); the first b samples' logits."""
        b = self.bsz if b is None else int(b)
        if not 0 < b <= self.bsz:
            raise ValueError(f"Predictor: a batch of {b} samples against bsz={self.bsz}")
        if not self.use_graph:
            self._out = self._forward()
        else:
            if self.graph is None:
                self._capture()
            self.graph.replay()
        self._b = b
        return self._out[:b]

    def __call__(self, imgs, rots, trans, intrins, post_rots, post_trans, alive=None) -> torch.Tensor:
        if self.stager is not None:
            raise RuntimeError("Predictor: built on a stager -- stage / commit there, then run(b)")
        if alive is not None and self.alive is None:
            raise RuntimeError("Predictor: built without camera_mask=True -- its forward has no camera mask")
        b = int(imgs.shape[0])
        if not 0 < b <= self.bsz:
            raise ValueError(f"Predictor: a batch of {b} samples against bsz={self.bsz}")
        for dst, src in zip(self.inputs, (imgs, rots, trans, intrins, post_rots, post_trans)):
            if tuple(src.shape) != (b,) + tuple(dst.shape[1:]):
                raise ValueError(f"Predictor: an input of shape {tuple(src.shape)}, expected {(b,) + tuple(dst.shape[1:])}")
            dst[:b].copy_(src, non_blocking=True)
        self._host_post_rots[:b].copy_(_host(post_rots))
        self._host_intrins[:b].copy_(_host(intrins))
        self.hinv.update(self._host_post_rots, self._host_intrins)
        if alive is not None:
            self.set_alive(alive)
        return self.run(b)

    # ------------------------------------------------------------------ outputs of the last call
    def logits(self) -> torch.Tensor:
        if self._out is None:
            raise RuntimeError("Predictor: no call yet")
        return self._out[:self._b]

    def probs(self) -> torch.Tensor:
        """sigmoid of the last call's logits, fp32 (``out.sigmoid()``, src/explore.py:322); exclusive classes: the
        softmax over dim 1."""
        if self.exclusive:
            return torch.softmax(self.logits().float(), dim=1)
        return self.logits().float().sigmoid()

    def classes(self) -> torch.Tensor:
        """Exclusive classes: the (b, X, Y) uint8 class map of the last call, ``lss_argmax_classes`` (ties to the
        lowest class, a NaN never wins). A fresh tensor."""
        if not self.exclusive:
            raise RuntimeError("Predictor: classes() needs exclusive=True (sigmoid channels have no argmax)")
        from . import tools
        return tools.argmax_classes(self.logits())

    def masks(self) -> torch.Tensor:
        """uint8 (b, K, X, Y): probability > threshold, as logits > logit(threshold) (per class: in fp32)."""
        if self.exclusive:  # (b, C - 1, X, Y): plane k = classes() == k + 1, one plane per label group
            cls = self.classes().unsqueeze(1)
            ks = torch.arange(1, self.n_out, device=cls.device, dtype=torch.uint8).view(1, -1, 1, 1)
            return (cls == ks).to(torch.uint8)
        if self.thetas is not None:
            return (self.logits().float() > self.thetas.view(-1, 1, 1)).to(torch.uint8)
        return (self.logits() > self.logit).to(torch.uint8)


def _host(t: torch.Tensor) -> torch.Tensor:
    """A rig tensor's host values: itself, its attached host copy while still valid (ops.camera_inverses'
    rule), or one device read."""
    if not t.is_cuda:
        return t
    h = getattr(t, "_lss_host", None)
    if (h is not None and tuple(h.shape) == tuple(t.shape) and not h.is_cuda
            and getattr(t, "_lss_host_version", None) == t._version):
        return h
    return t.detach().cpu()


# ---------------------------------------------------------------------- command line
def threshold_arg(text):
    """``--threshold 0.5`` -> 0.5; ``--threshold 0.5,0.4,0.35`` -> [0.5, 0.4, 0.35] (one per class)."""
    try:
        vals = [float(v) for v in str(text).split(",") if v.strip()]
    except ValueError:
        vals = []
    if not vals:
        raise argparse.ArgumentTypeError(f"--threshold {text!r}: a probability, or a comma list of one per class")
    return vals[0] if len(vals) == 1 else vals


def parse_drop_cams(text) -> list:
    """``--drop_cams front,back_left`` (names of simbev.CAMERA_ORDER) or ``--drop_cams 1,3`` (indices) -> the sorted
    distinct camera indices; None or empty: []. ValueError for an unknown name or an index out of range."""
    from .simbev import CAMERA_ORDER
    if text is None:
        return []
    items = [v.strip() for v in text.split(",")] if isinstance(text, str) else [v for v in text]
    out = set()
    for v in items:
        if isinstance(v, str) and not v:
            continue
        if isinstance(v, str) and v in CAMERA_ORDER:
            out.add(CAMERA_ORDER.index(v))
            continue
        try:
            i = int(v)
        except (TypeError, ValueError):
            i = -1
        if isinstance(v, bool) or not 0 <= i < len(CAMERA_ORDER):
            raise ValueError(f"--drop_cams {text!r}: {v!r} is neither one of {', '.join(CAMERA_ORDER)} nor an index "
                             f"0..{len(CAMERA_ORDER) - 1}")
        out.add(i)
    return sorted(out)


def parse_photo(text):
    """``--photo "brightness=-40,contrast=0.8,noise=8"`` -> {"brightness": -40.0, "contrast": 0.8, "noise": 8.0}: the
    loader's ``photo_fixed`` dict (entries brightness, contrast, saturation, hue, noise: numbers; seed: an integer).
    None or empty: None. A dict passes through the same checks. ValueError for an unknown entry or a bad value."""
    from .simbev import photo_fixed_record
    if text is None or (isinstance(text, str) and not text.strip()):
        return None
    if isinstance(text, dict):
        out = dict(text)
    else:
        out = {}
        for part in str(text).split(","):
            if not part.strip():
                continue
            name, eq, value = part.partition("=")
            name = name.strip()
            if not eq or not value.strip() or name in out:
                raise ValueError(f"--photo {text!r}: name=value entries, each once, comma separated")
            try:
                out[name] = int(value) if name == "seed" else float(value)
            except ValueError:
                raise ValueError(f"--photo {text!r}: {name}={value.strip()!r} is not a number") from None
    if not out:
        return None
    photo_fixed_record({"photo_fixed": out})  # (unknown entries and bad values fail here)
    return out


def parser() -> argparse.ArgumentParser:
    p = argparse.ArgumentParser(prog="python -m lss_carla_amd.predict",
                                description="Run a trained LSS over a SimBEV val split on the MI355X: masks and metrics")
    p.add_argument("--modelf", type=str, required=True, help="checkpoint: a state_dict or a trainer checkpoint")
    p.add_argument("--dataroot", type=str, required=True, help="SimBEV dataset root directory")
    p.add_argument("--out", type=str, required=True, help="directory for <index>.npy and metrics.json")
    p.add_argument("--bsz", type=int, default=4)
    p.add_argument("--label_groups", type=str, default=None,
                   help='BEV channel groups, one output class each: "0;1,2,3;6,7" (default: the vehicle mask 1,2,3)')
    p.add_argument("--pos_weight", type=str, default=None,
                   help="one positive-class weight, or one per class (default 2.13; with --loss focal: w_pos, default 1)")
    p.add_argument("--loss", default="bce", choices=["bce", "focal"], help="the loss metrics.json reports")
    p.add_argument("--focal_gamma", type=str, default="2.0", help="focal loss: one gamma, or one per class")
    p.add_argument("--focal_alpha", type=str, default=None,
                   help="focal loss: one alpha in (0, 1), or one per class (instead of --pos_weight)")
    p.add_argument("--iou_thresholds", type=str, default=None,
                   help="also report the IoU at these probability thresholds: 0.35,0.4,0.45,0.5,0.55,0.6,0.65")
    p.add_argument("--dtype", default="bf16", choices=["bf16", "fp32"])
    p.add_argument("--graph", type=int, default=1, choices=[0, 1], help="0: the same forward, eager")
    p.add_argument("--threshold", type=threshold_arg, default=0.5,
                   help="the masks' probability threshold, or one per class: 0.5,0.4,0.35")
    p.add_argument("--weights", default="auto", choices=list(WEIGHTS),
                   help="which weights of a trainer checkpoint: its EMA (auto: when it has one) or the model's")
    p.add_argument("--valid_mask", default="none", choices=["none", "grid", "fov"],
                   help="count only valid cells in loss and IoU (fov: cells some camera sees); also writes DIR/valid/")
    p.add_argument("--fov_z", type=str, default="0.0",
                   help="--valid_mask fov: the heights (metres) a cell is tested at, 1 to 8: 0.0[,1.5,...]")
    p.add_argument("--drop_cams", type=str, default=None,
                   help="cameras dead in every sample, names or indices: front,back_left")
    p.add_argument("--drop_each", type=int, default=0, choices=[0, 1],
                   help="1: after the normal pass, the split once more per camera with that camera dead (same graph)")
    p.add_argument("--exclusive", type=int, default=0, choices=[0, 1],
                   help="1: exclusive classes (argmax class maps in DIR/preds/, confusion-matrix metrics); needs --label_groups")
    p.add_argument("--class_weight", type=str, default=None,
                   help="--exclusive 1: the loss's weight per class, the background first: w0,...,wK (default all 1)")
    p.add_argument("--photo", type=str, default=None,
                   help='one photometric shift for every image: "brightness=-40,contrast=0.8,saturation=1,hue=0,noise=8,seed=0"')
    p.add_argument("--gpuid", type=int, default=0)
    p.add_argument("--nworkers", type=int, default=4)
    p.add_argument("--H", type=int, default=224)
    p.add_argument("--W", type=int, default=480)
    p.add_argument("--final_h", type=int, default=128)
    p.add_argument("--final_w", type=int, default=352)
    p.add_argument("--miopen_find", type=int, default=1)
    return p


def confs(a) -> tuple:
    """(grid_conf, data_aug_conf) of the reference's defaults (train_simbev.py:23-98) at the given sizes; the
    val split draws no augmentation."""
    grid_conf = {"xbound": [-50.0, 50.0, 0.5], "ybound": [-50.0, 50.0, 0.5], "zbound": [-10.0, 10.0, 20.0],
                 "dbound": [4.0, 45.0, 1.0]}
    data_aug_conf = {"resize_lim": (1.0, 1.0), "final_dim": (a.final_h, a.final_w), "rot_lim": (0.0, 0.0), "H": a.H,
                     "W": a.W, "rand_flip": False, "bot_pct_lim": (0.0, 0.0), "Ncams": 6}
    return grid_conf, data_aug_conf


def predict(a, grid_conf=None, data_aug_conf=None, model: Optional[torch.nn.Module] = None) -> dict:
    """The command line's work for parsed arguments `a`; returns metrics.json's dict. grid_conf / data_aug_conf
    override the defaults of ``confs``; model: an already built (and loaded) module instead of --modelf."""
    dropped = parse_drop_cams(getattr(a, "drop_cams", None))  # (a bad name fails before anything else)
    exclusive = bool(getattr(a, "exclusive", 0))
    class_weight = None
    if exclusive:  # (argument errors before anything is built, the GPU included)
        from .trainer import _exclusive_setup, _weights_list, parse_label_groups as _groups, parse_per_class as _pc
        th = threshold_arg(a.threshold) if isinstance(a.threshold, str) else a.threshold
        if not (isinstance(th, (int, float)) and float(th) == 0.5):
            raise ValueError("--threshold does not apply to exclusive classes (the prediction is an argmax)")
        cw = getattr(a, "class_weight", None)
        class_weight = _exclusive_setup(
            _groups(a.label_groups), None if cw is None else (_weights_list(cw) if isinstance(cw, str) else list(cw)),
            getattr(a, "pos_weight", None), getattr(a, "loss", "bce"), _pc(getattr(a, "focal_gamma", "2.0"), "--focal_gamma"),
            getattr(a, "focal_alpha", None), getattr(a, "iou_thresholds", None) or None)
    elif getattr(a, "class_weight", None) is not None:
        raise ValueError("--class_weight needs --exclusive 1")
    photo = parse_photo(getattr(a, "photo", None))  # (a bad entry fails before anything is built)
    if a.gpuid < 0:
        raise RuntimeError("lss_carla_amd.predict: needs an MI355X (the hot path has no CPU fallback)")
    dev = _require_gpu(f"cuda:{a.gpuid}")

    import numpy as np

    import lss_carla_amd as L
    from . import simbev, tools
    from .staging import BatchStager
    from .trainer import (_class_setup, _loss_setup, parse_heights, parse_label_groups, parse_per_class,
                          parse_thresholds)

    torch.cuda.set_device(dev)
    torch.backends.cudnn.benchmark = bool(a.miopen_find)
    gc, dac = confs(a)
    grid_conf, data_aug_conf = grid_conf or gc, data_aug_conf or dac
    if photo is not None:  # the validation loader then emits that record for every image (simbev.photo_fixed_records)
        data_aug_conf = {**data_aug_conf, "photo_fixed": photo}
    loss_kind = getattr(a, "loss", "bce")
    pw_arg = getattr(a, "pos_weight", None)
    pos_weight, focal = _loss_setup(loss_kind, None if pw_arg is None else parse_per_class(pw_arg, "--pos_weight"),
                                    parse_per_class(getattr(a, "focal_gamma", "2.0"), "--focal_gamma"),
                                    None if getattr(a, "focal_alpha", None) is None
                                    else parse_per_class(a.focal_alpha, "--focal_alpha"))
    ladder = parse_thresholds(getattr(a, "iou_thresholds", None))
    threshold = threshold_arg(a.threshold) if isinstance(a.threshold, str) else a.threshold
    groups, K, pos_weight = _class_setup(parse_label_groups(a.label_groups), pos_weight)
    if focal is not None:
        focal = tools.focal_rows(K, **focal)  # (argument errors before anything is built)
    if not tools.is_scalar_weight(threshold) and len(threshold) != K:
        raise ValueError(f"--threshold names {len(threshold)} classes, label_groups {K}")
    mask_mode = simbev.valid_mask_mode({"valid_mask": getattr(a, "valid_mask", None),
                                        "fov_z": parse_heights(getattr(a, "fov_z", "0.0"))})
    fov_z = parse_heights(getattr(a, "fov_z", "0.0"))
    drop_each = bool(getattr(a, "drop_each", 0))
    use_mask = bool(dropped) or drop_each
    amp_dtype = torch.bfloat16 if a.dtype == "bf16" else None
    n_out = K + 1 if exclusive else K  # exclusive classes: the background and the K groups
    if model is None:
        sd = model_state_dict(torch.load(a.modelf, map_location="cpu"), getattr(a, "weights", "auto"))
        check_head(sd, n_out, f"checkpoint {a.modelf}")  # before anything is built
        model = L.compile_model(grid_conf, data_aug_conf, outC=n_out).to(dev)
        model.load_state_dict(sd)
    model.bevencode.to(memory_format=torch.channels_last)
    model.camencode.up1.to(memory_format=torch.channels_last)
    _, valloader = simbev.compile_data("unused", a.dataroot, data_aug_conf, grid_conf, a.bsz, a.nworkers,
                                       "segmentationdata", device=dev, label_groups=groups)
    val_raw, n_val = valloader.loader, len(valloader.dataset)
    stager = BatchStager(data_aug_conf["final_dim"], a.bsz, len(simbev.CAMERA_ORDER),
                         (data_aug_conf["H"], data_aug_conf["W"]), grid_conf, dev, label_groups=groups,
                         **({} if mask_mode is None else {"valid_mask": mask_mode, "fov_z": fov_z}),
                         **({"exclusive": True} if exclusive else {}),
                         **({"photo": True} if simbev.photo_enabled(data_aug_conf) else {}))
    p = Predictor(model, a.bsz, dev, amp_dtype=amp_dtype, threshold=threshold, graph=bool(a.graph), stager=stager,
                  **({"camera_mask": True} if use_mask else {}), **({"exclusive": True} if exclusive else {}))
    if K > 1 or not tools.is_scalar_weight(pos_weight):
        pos_weight = tools.class_weights(pos_weight, K, dev)
    totals = torch.zeros(1 + 2 * K, device=dev, dtype=torch.float64)
    ladder_mode = focal is not None or ladder is not None or mask_mode is not None  # (masked: always this path)
    valid_cells = torch.zeros(1, device=dev, dtype=torch.float64) if mask_mode is not None else None
    if ladder_mode:  # lss_seg_metrics_accum at the ladder and 0.5: either loss term, every threshold, one pass
        columns = sorted(set((ladder or []) + [0.5]))
        if len(columns) > 16:
            raise ValueError(f"--iou_thresholds: {len(columns)} thresholds (0.5 included); at most 16")
        thetas = torch.tensor([threshold_logit(v) for v in columns], device=dev, dtype=torch.float32)
        if focal is not None:
            params = torch.tensor(focal, device=dev, dtype=torch.float32)
        else:
            w = tools.class_weights(pos_weight, K, dev)
            params = torch.stack([w, torch.ones_like(w), torch.zeros_like(w)], dim=1).contiguous()
        totals = torch.zeros(1 + K + 2 * K * len(columns), device=dev, dtype=torch.float64)
    if exclusive:  # lss_confusion_accum: 1 + C C totals, the loss with the class weights
        ladder_mode, valid_cells = False, None
        totals = torch.zeros(1 + n_out * n_out, device=dev, dtype=torch.float64)
        weight_dev = torch.tensor(class_weight, device=dev, dtype=torch.float32)
    os.makedirs(a.out, exist_ok=True)
    n_cams = len(simbev.CAMERA_ORDER)

    def run_split(dead, keep_masks):
        """One pass over the split with the cameras `dead` dead in every sample: (masks, valids, frames, seconds);
        the totals (and valid_cells) are zeroed first and hold the pass's sums afterwards."""
        totals.zero_()
        if valid_cells is not None:
            valid_cells.zero_()
        if use_mask:
            on = [0 if c in dead else 1 for c in range(n_cams)]
            p.set_alive(on)
            stager.cam_alive = torch.tensor(on, dtype=torch.uint8)  # --valid_mask fov: a dead camera sees no cell
        masks, valids, frames = [], [], 0
        it = iter(val_raw)
        nxt = next(it, None)
        if nxt is not None:
            stager.stage(nxt)
        torch.cuda.synchronize(dev)
        t0 = None
        while nxt is not None:
            b = stager.commit()
            p.run(b)  # (the first call captures the graph: timed from the second batch on)
            if exclusive:
                tools.confusion_accumulate(p._out, stager.binimgs, totals, stager.n_valid, weight_dev,
                                           valid=stager.valid)
            elif ladder_mode:
                tools.seg_metrics_accumulate(p._out, stager.binimgs, totals, stager.n_valid, params, thetas,
                                             valid=stager.valid, valid_cells=valid_cells)
            else:
                tools.val_accumulate(p._out, stager.binimgs, totals, n_valid=stager.n_valid, pos_weight=pos_weight)
            if keep_masks:
                masks.append(p.classes() if exclusive else p.masks())  # a fresh tensor per batch; the logits are static
                if mask_mode is not None:
                    valids.append(stager.valid[:b].clone())
            nxt = next(it, None)
            if nxt is not None:
                stager.stage(nxt)
            if t0 is None:
                torch.cuda.synchronize(dev)
                t0 = time.perf_counter()
            else:
                frames += b
        torch.cuda.synchronize(dev)
        return masks, valids, frames, (time.perf_counter() - t0 if t0 is not None else 0.0)

    def summary(t):
        """loss, the IoU keys and the ladder's keys out of a pass's totals (a list)."""
        if exclusive:
            cells = None if mask_mode is None else n_val * (stager.valid.numel() // stager.valid.shape[0])
            return tools.confusion_summary(t, n_out, n_val, cells=cells)
        extra = {}
        if ladder_mode:
            P, TP, PP = tools.seg_metrics_counts(t, K, len(columns))
            c = columns.index(0.5)
            inter, union = [TP[k][c] for k in range(K)], [PP[k][c] + P[k] - TP[k][c] for k in range(K)]
            if ladder is not None:
                cols = [columns.index(v) for v in ladder]
                sub = (t[:1 + K] + [TP[k][j] for k in range(K) for j in cols]
                       + [PP[k][j] for k in range(K) for j in cols])
                extra = {k: v for k, v in tools.seg_metrics_summary(sub, K, ladder, n_val).items() if k != "loss"}
                extra["iou_thresholds"] = ladder
        else:
            inter, union = t[1:1 + K], t[1 + K:1 + 2 * K]
        out = {"loss": t[0] / n_val, **tools.iou_summary(inter, union), **extra, "intersection": inter, "union": union}
        if mask_mode is not None:
            cells = stager.valid.numel() // stager.valid.shape[0]
            out["valid_fraction"] = float(valid_cells.item()) / (n_val * cells) if n_val else None
        return out

    masks, valids, frames, elapsed = run_split(set(dropped), True)
    main_info = summary(totals.tolist())
    each = {}
    if drop_each:
        for c, name in enumerate(simbev.CAMERA_ORDER):
            run_split(set(dropped) | {c}, False)
            each[name] = summary(totals.tolist())
    index = 0
    pred_dir = os.path.join(a.out, "preds") if exclusive else a.out  # exclusive classes: the (X, Y) class maps
    os.makedirs(pred_dir, exist_ok=True)
    for m in masks:
        for s in m.cpu().numpy():
            np.save(os.path.join(pred_dir, f"{index}.npy"), s)
            index += 1
    if mask_mode is not None:
        os.makedirs(os.path.join(a.out, "valid"), exist_ok=True)
        vi = 0
        for m in valids:
            for s in m.cpu().numpy():
                np.save(os.path.join(a.out, "valid", f"{vi}.npy"), s)
                vi += 1
    valid_fraction = main_info.pop("valid_fraction", None)
    if exclusive:
        info = {**main_info, "loss_kind": "softmax", "exclusive": True, "class_weight": class_weight, "samples": index,
                "classes": n_out, "dtype": a.dtype, "graph": bool(a.graph), "bsz": a.bsz,
                "frames_per_s": frames / elapsed if frames and elapsed > 0 else None}
    else:
        inter, union = main_info.pop("intersection"), main_info.pop("union")
        info = {**main_info, "loss_kind": loss_kind,
                "threshold": threshold, "intersection": inter, "union": union, "samples": index, "classes": K,
                "dtype": a.dtype, "graph": bool(a.graph), "bsz": a.bsz,
                "frames_per_s": frames / elapsed if frames and elapsed > 0 else None}
    if mask_mode is not None:
        info.update({"valid_mask": mask_mode, "fov_z": list(fov_z), "valid_fraction": valid_fraction})
    if photo is not None:
        info["photo"] = photo
    if use_mask:
        info["dropped_cams"] = [simbev.CAMERA_ORDER[c] for c in dropped]
    if drop_each:
        info["drop_each"] = each
    with open(os.path.join(a.out, "metrics.json"), "w") as f:
        json.dump(info, f, indent=1)
    return info


def main(argv: Optional[Sequence[str]] = None) -> dict:
    a = parser().parse_args(argv)
    info = predict(a)
    print(json.dumps(info))
    return info


if __name__ == "__main__":
    main()
