"""SimBEV input path with the pixel work on the MI355X.

Drop-in for ``src/data_simbev.py`` of shdragron/LSS-Carla: ``SimBEVDataset`` / ``SegmentationData`` /
``VizData`` / ``compile_data(version, dataroot, data_aug_conf, grid_conf, bsz, nworkers, parser_name)``
with the same directory layout, split, augmentation draws and returned 7-tuple
``(imgs, rots, trans, intrins, post_rots, post_trans, binimgs)``.

Where the work runs:
  host (DataLoader workers)  meta.json parsing, JPEG decode (PIL), the augmentation draws
                             (``sample_augmentation``, np.random, src/data_simbev.py:119-145) and the
                             post-homography arithmetic (torch, src/tools.py:130-142), the BEV npz read
  device (main process)      ``lss_simbev_images``: Image.resize (bicubic) -> crop -> flip -> rotate
                             -> ToTensor -> Normalize per camera, bit for bit with Pillow / torchvision
                             (``lss_simbev_images_photo``: the same with colour jitter and sensor noise on the
                             resampled pixel, for a conf with ``photo_*`` keys);
                             ``lss_simbev_vehicle_mask``: classes 1-3 merged + np.flipud (or, with
                             ``label_groups``, ``lss_simbev_class_masks``: one label channel per group)
So a training step at hundreds of frames/s is not bound by PIL's per-camera resampling on the CPU:
the workers only decode. The loader yields device tensors; the reference's ``.to(device)`` calls in
train_simbev.py become no-ops.
"""
from __future__ import annotations

import ctypes
import json
import math
import os
from functools import lru_cache
from pathlib import Path
from typing import Dict, List, Sequence, Tuple

import numpy as np
import torch

from . import _lib

CAMERA_ORDER = ["front_left", "front", "front_right", "back_left", "back", "back_right"]  # src/data_simbev.py:17-20


# ----------------------------------------------------------------------------- augmentation arithmetic (host)
def get_rot(h):
    """src/tools.py:113-117."""
    return torch.Tensor([[np.cos(h), np.sin(h)], [-np.sin(h), np.cos(h)]])


def draw_augmentation(conf: dict, train: bool):
    """One sample's augmentation (src/data_simbev.py:119-145): (scale, (W', H') after scaling, crop box
    (left, top, right, bottom) of final_dim, flip, rotation in degrees).

    The crop keeps the image's bottom band: its top edge sits `bottom` of the scaled height above the
    bottom minus the final height; horizontally the window starts `left` pixels in. Training draws,
    in order, from np.random: scale ~ U(resize_lim), bottom ~ U(bot_pct_lim), left ~ U(0, slack), a
    flip coin only when rand_flip is set, rotation ~ U(rot_lim). Validation: the scale that fits the
    final width, the mean of bot_pct_lim, the window centred, no flip or rotation."""
    src_h, src_w = conf["H"], conf["W"]
    out_h, out_w = conf["final_dim"]
    rnd = np.random
    scale = rnd.uniform(*conf["resize_lim"]) if train else max(out_h / src_h, out_w / src_w)
    scaled = (int(src_w * scale), int(src_h * scale))
    slack = max(0, scaled[0] - out_w)
    bottom = rnd.uniform(*conf["bot_pct_lim"]) if train else np.mean(conf["bot_pct_lim"])
    top = int((1 - bottom) * scaled[1]) - out_h
    left = int(rnd.uniform(0, slack)) if train else int(slack / 2)
    flip = bool(train and conf["rand_flip"] and rnd.choice([0, 1]))
    rotate = rnd.uniform(*conf["rot_lim"]) if train else 0
    return scale, scaled, (left, top, left + out_w, top + out_h), flip, rotate


def post_homography(resize, crop, flip, rotate):
    """(post_rot (3, 3), post_tran (3,)) of one camera: img_transform's post-homography arithmetic
    (src/tools.py:130-142) then the 3x3 embedding of get_image_data (src/data_simbev.py:204-208),
    with the same torch fp32 ops in the same order."""
    post_rot = torch.eye(2)
    post_tran = torch.zeros(2)
    post_rot *= resize
    post_tran -= torch.Tensor(crop[:2])
    if flip:
        A = torch.Tensor([[-1, 0], [0, 1]])
        b = torch.Tensor([crop[2] - crop[0], 0])
        post_rot = A.matmul(post_rot)
        post_tran = A.matmul(post_tran) + b
    A = get_rot(rotate / 180 * np.pi)
    b = torch.Tensor([crop[2] - crop[0], crop[3] - crop[1]]) / 2
    b = A.matmul(-b) + b
    post_rot = A.matmul(post_rot)
    post_tran = A.matmul(post_tran) + b
    post_tran_3 = torch.zeros(3)
    post_rot_3 = torch.eye(3)
    post_tran_3[:2] = post_tran
    post_rot_3[:2, :2] = post_rot
    return post_rot_3, post_tran_3


# ----------------------------------------------------------------------------- BEV-space augmentation (host)
# One transform of the ego frame per sample, A = s * Rz(theta) * diag(fx, fy, 1) with fx, fy in {+1, -1}, applied
# to ego-frame points as p' = A p (z is scaled by s too). The rig takes it as rots' = A rots, trans' = A trans, so
# the frustum points move with it; the labels take it as a nearest-neighbour gather (class_masks, index_mats=).
BEV_AUG_IDENTITY = (0.0, 1.0, False, False)


def _bev_aug_lims(conf: dict):
    """(rot_lim, scale_lim, flip) of a data_aug_conf: the keys bev_rot_lim (degrees), bev_scale_lim, bev_flip, absent
    ones neutral; ValueError for a pair that is not finite and ascending or a scale that is not positive."""
    rot = tuple(float(v) for v in conf.get("bev_rot_lim", (0.0, 0.0)))
    scale = tuple(float(v) for v in conf.get("bev_scale_lim", (1.0, 1.0)))
    for name, lim in (("bev_rot_lim", rot), ("bev_scale_lim", scale)):
        if len(lim) != 2 or not all(math.isfinite(v) for v in lim) or lim[0] > lim[1]:
            raise ValueError(f"{name} {lim!r}: a finite (lo, hi) with lo <= hi")
    if scale[0] <= 0.0:
        raise ValueError(f"bev_scale_lim {scale!r}: positive scales")
    return rot, scale, bool(conf.get("bev_flip", False))


def bev_aug_enabled(conf: dict) -> bool:
    """Whether a data_aug_conf asks for the BEV-space augmentation: any of bev_rot_lim / bev_scale_lim / bev_flip
    present and not neutral ((0, 0), (1, 1), False). The training and the validation samples of such a conf carry
    the label index matrix (SimBEVDataset.__getitem__), and this is the flag their consumers are given."""
    rot, scale, flip = _bev_aug_lims(conf)
    return rot != (0.0, 0.0) or scale != (1.0, 1.0) or flip


def draw_bev_augmentation(conf: dict, train: bool):
    """One sample's BEV-space augmentation (theta_deg, scale, flip_x, flip_y). Off -- validation, or a conf that does
    not ask for it -- it is the identity and draws nothing. On, it draws from np.random, after the sample's other
    draws: theta ~ U(bev_rot_lim), scale ~ U(bev_scale_lim), then the x coin and the y coin only when bev_flip is on."""
    if not train or not bev_aug_enabled(conf):
        return BEV_AUG_IDENTITY
    rot, scale, flip = _bev_aug_lims(conf)
    rnd = np.random
    theta = float(rnd.uniform(*rot))
    s = float(rnd.uniform(*scale))
    flip_x = bool(flip and rnd.choice([0, 1]))
    flip_y = bool(flip and rnd.choice([0, 1]))
    return theta, s, flip_x, flip_y


def bev_aug_matrix(theta_deg, scale, flip_x, flip_y) -> np.ndarray:
    """A = scale * Rz(theta) * diag(fx, fy, 1) as (3, 3) fp32: built in float64, rounded once."""
    t = math.radians(float(theta_deg))
    c, s = math.cos(t), math.sin(t)
    rz = np.array([[c, -s, 0.0], [s, c, 0.0], [0.0, 0.0, 1.0]], dtype=np.float64)
    f = np.diag([-1.0 if flip_x else 1.0, -1.0 if flip_y else 1.0, 1.0])
    return (float(scale) * (rz @ f)).astype(np.float32)


def compose_rig(A, rots: torch.Tensor, trans: torch.Tensor):
    """The rig in the augmented ego frame: (A @ rots, A @ trans) for rots (..., 3, 3) and trans (..., 3), fp32 on the
    host -- camera points then land at A (R x + t). intrins / post_rots / post_trans are not touched (nor are the
    host inverses ops.HostInverses takes of them)."""
    A = torch.as_tensor(np.asarray(A), dtype=torch.float32)
    return A.matmul(rots), A.matmul(trans.unsqueeze(-1)).squeeze(-1)


def label_index_matrix(A, grid_conf: dict) -> np.ndarray:
    """The (2, 3) fp32 affine map of the label warp under A: from the centre of output cell (i, j) in index units,
    (i + 0.5, j + 0.5), to the source position in index units -- row i of a label is x cell i, column j is y cell j,
    the layout of the model's logits. With A2 the xy block of A, D = diag(dx, dy) and lo = bx - dx / 2 (ops.GridSpec):
    M = D^-1 A2^-1 D and b = D^-1 (A2^-1 lo - lo), in float64, rounded once. ValueError for a non-finite or singular A."""
    a = np.asarray(A, dtype=np.float64)
    if a.shape != (3, 3) or not np.isfinite(a).all():
        raise ValueError(f"label_index_matrix: a finite (3, 3) matrix, got {a!r}")
    det = a[0, 0] * a[1, 1] - a[0, 1] * a[1, 0]
    if det == 0.0 or not math.isfinite(1.0 / det):
        raise ValueError(f"label_index_matrix: the xy block of {a!r} is singular")
    inv = np.array([[a[1, 1], -a[0, 1]], [-a[1, 0], a[0, 0]]], dtype=np.float64) / det
    from .ops import GridSpec
    gs = GridSpec.from_conf(grid_conf)
    d = np.array(gs.dx[:2], dtype=np.float64)
    lo = np.array(gs.lo[:2], dtype=np.float64)
    out = np.empty((2, 3), dtype=np.float64)
    for r in range(2):
        for c in range(2):
            out[r, c] = inv[r, c] * d[c] / d[r]
        out[r, 2] = ((inv[r, 0] * lo[0] + inv[r, 1] * lo[1]) - lo[r]) / d[r]
    if not np.isfinite(out).all():
        raise ValueError(f"label_index_matrix: {a!r} has no finite inverse map")
    return out.astype(np.float32)


# ----------------------------------------------------------------------------- photometric augmentation (host)
# Per image, an affine map of (R, G, B) in 0..255 units -- brightness, contrast, saturation, hue composed into one
# 3 x 3 matrix and one offset -- plus a noise amplitude and the Philox key of the image's noise: the 16 words of
# lss_img_photo_t (include/lss_simbev.h). ``lss_simbev_images_photo`` applies it to the resampled integer pixel in
# registers and clamps once, at the end.
PHOTO_NEUTRAL = (0.0, 1.0, 1.0, 0.0, 0.0, 0, 0)  # brightness, contrast, saturation, hue (deg), noise sigma, seed words
PHOTO_WORDS = 16                                  # sizeof(lss_img_photo_t) / 4
_LUMA = (0.299, 0.587, 0.114)
_YIQ = ((0.299, 0.587, 0.114), (0.595716, -0.274453, -0.321263), (0.211456, -0.522591, 0.311135))
_PHOTO_LIMS = (("photo_brightness_lim", (0.0, 0.0)), ("photo_contrast_lim", (1.0, 1.0)),
               ("photo_saturation_lim", (1.0, 1.0)), ("photo_hue_lim", (0.0, 0.0)), ("photo_noise_lim", (0.0, 0.0)))
_PHOTO_FIXED_KEYS = ("brightness", "contrast", "saturation", "hue", "noise", "seed")


def photo_matrix(brightness=0.0, contrast=1.0, saturation=1.0, hue_deg=0.0):
    """(M (3, 3), t (3,)) fp32 of the colour map v = M (r, g, b) + t in 0..255 units: composed in float64 in the fixed
    order brightness, contrast, saturation, hue, rounded to fp32 once. An op at its neutral value (0, 1, 1, 0) is
    skipped, not multiplied in, so the neutral record is exactly (I, 0).
      brightness d   t += d
      contrast a     about mid-grey: M <- a M, t <- a (t - 127.5) + 127.5
      saturation s   S = s I + (1 - s) 1 L^T, L = (0.299, 0.587, 0.114): M <- S M, t <- S t
      hue h degrees  H = T^-1 R(h) T, T the RGB -> YIQ matrix, R(h) the rotation of the I/Q plane: M <- H M, t <- H t
    There is no clamp between the ops: the kernel clamps once, after the noise."""
    vals = [float(v) for v in (brightness, contrast, saturation, hue_deg)]
    if not all(math.isfinite(v) for v in vals):
        raise ValueError(f"photo_matrix: finite values, got {vals!r}")
    b, a, s, h = vals
    M, t = np.eye(3, dtype=np.float64), np.zeros(3, dtype=np.float64)
    if b != 0.0:
        t = t + b
    if a != 1.0:
        M, t = a * M, a * (t - 127.5) + 127.5
    if s != 1.0:
        S = s * np.eye(3) + (1.0 - s) * np.outer(np.ones(3), np.array(_LUMA, dtype=np.float64))
        M, t = S @ M, S @ t
    if h != 0.0:
        T = np.array(_YIQ, dtype=np.float64)
        c, sn = math.cos(math.radians(h)), math.sin(math.radians(h))
        R = np.array([[1.0, 0.0, 0.0], [0.0, c, -sn], [0.0, sn, c]], dtype=np.float64)
        H = np.linalg.inv(T) @ R @ T
        M, t = H @ M, H @ t
    return M.astype(np.float32), t.astype(np.float32)


def _photo_lims(conf: dict):
    """(the five (lo, hi) limits in _PHOTO_LIMS' order, photo_prob, photo_per_camera) of a data_aug_conf, absent keys
    neutral; ValueError for a pair that is not finite and ascending, a negative contrast, saturation or sigma, or a
    probability outside [0, 1]."""
    lims = []
    for name, neutral in _PHOTO_LIMS:
        lim = tuple(float(v) for v in conf.get(name, neutral))
        if len(lim) != 2 or not all(math.isfinite(v) for v in lim) or lim[0] > lim[1]:
            raise ValueError(f"{name} {lim!r}: a finite (lo, hi) with lo <= hi")
        if name in ("photo_contrast_lim", "photo_saturation_lim", "photo_noise_lim") and lim[0] < 0.0:
            raise ValueError(f"{name} {lim!r}: not negative")
        lims.append(lim)
    prob = float(conf.get("photo_prob", 0.5))
    if not 0.0 <= prob <= 1.0:
        raise ValueError(f"photo_prob {prob!r}: a probability")
    return tuple(lims), prob, bool(int(conf.get("photo_per_camera", 1)))


def photo_fixed_record(conf: dict):
    """The ``photo_fixed`` dict of a data_aug_conf as (brightness, contrast, saturation, hue, noise, seed), absent
    entries neutral (seed 0); None when the conf has none. ValueError for an unknown entry, a value that is not finite,
    a negative contrast, saturation or noise, or a seed outside 0..2^64-1."""
    fixed = conf.get("photo_fixed")
    if fixed is None:
        return None
    unknown = sorted(set(fixed) - set(_PHOTO_FIXED_KEYS))
    if unknown:
        raise ValueError(f"photo_fixed: unknown entries {unknown} (one of {', '.join(_PHOTO_FIXED_KEYS)})")
    vals = [float(fixed.get(k, d)) for k, d in zip(_PHOTO_FIXED_KEYS[:5], PHOTO_NEUTRAL[:5])]
    if not all(math.isfinite(v) for v in vals) or vals[1] < 0.0 or vals[2] < 0.0 or vals[4] < 0.0:
        raise ValueError(f"photo_fixed {fixed!r}: finite values; contrast, saturation and noise not negative")
    seed = int(fixed.get("seed", 0))
    if not 0 <= seed < 1 << 64:
        raise ValueError(f"photo_fixed: seed {seed!r} outside 0..2^64-1")
    return (*vals, seed)


def photo_draws(conf: dict) -> bool:
    """Whether training samples of a data_aug_conf draw a photometric augmentation: some photo_*_lim present and not
    neutral ((0, 0) for brightness, hue and noise, (1, 1) for contrast and saturation)."""
    lims, _, _ = _photo_lims(conf)
    return any(lim != neutral for lim, (_, neutral) in zip(lims, _PHOTO_LIMS))


def photo_enabled(conf: dict) -> bool:
    """Whether a data_aug_conf asks for the photometric augmentation: a photo_*_lim that is not neutral (photo_draws)
    or a ``photo_fixed`` record. The training and the validation samples of such a conf carry the (N, 16) photo
    records (SimBEVDataset.__getitem__), and this is the flag their consumers are given. A bad limit raises here."""
    return photo_draws(conf) or photo_fixed_record(conf) is not None


def draw_photo_augmentation(conf: dict, train: bool):
    """One unit's photometric augmentation (brightness, contrast, saturation, hue_deg, sigma, seed0, seed1) -- a unit
    is a camera, or a whole sample with photo_per_camera 0. Off -- validation, or a conf without a photo_*_lim -- it is
    PHOTO_NEUTRAL and draws nothing. On, it draws from np.random, after the sample's other draws, always the same
    number of values: for each of the four colour ops a coin U(0, 1) < photo_prob and then a value U(lim), drawn
    even when the coin fails (the op is then neutral); sigma ~ U(photo_noise_lim); two uint32 seed words."""
    if not train or not photo_draws(conf):
        return PHOTO_NEUTRAL
    lims, prob, _ = _photo_lims(conf)
    rnd = np.random
    ops = []
    for lim, neutral in zip(lims[:4], PHOTO_NEUTRAL[:4]):
        coin = rnd.uniform(0.0, 1.0) < prob
        value = float(rnd.uniform(*lim))
        ops.append(value if coin else neutral)
    sigma = float(rnd.uniform(*lims[4]))
    seed0 = int(rnd.randint(0, 1 << 32, dtype=np.uint32))
    seed1 = int(rnd.randint(0, 1 << 32, dtype=np.uint32))
    return (*ops, sigma, seed0, seed1)


def photo_record(brightness=0.0, contrast=1.0, saturation=1.0, hue_deg=0.0, noise=0.0, seed0=0, seed1=0) -> np.ndarray:
    """The 16 fp32 words of one lss_img_photo_t: photo_matrix's M (9) and t (3), sigma, the two seed words bit-cast,
    a zero pad. (Seed words are bits, not numbers: move a record by copies only.)"""
    M, t = photo_matrix(brightness, contrast, saturation, hue_deg)
    rec = np.zeros(PHOTO_WORDS, dtype=np.float32)
    rec[:9], rec[9:12], rec[12] = M.reshape(9), t, np.float32(noise)
    rec.view(np.uint32)[13:15] = (int(seed0) & 0xFFFFFFFF, int(seed1) & 0xFFFFFFFF)
    return rec


def photo_fixed_records(fixed, n: int) -> np.ndarray:
    """(n, 16) records of one fixed shift (photo_fixed_record's tuple) for the images 0..n-1 of a sample: the same
    matrix, offset and sigma, and per image the key (seed's low word + image index mod 2^32, seed's high word)."""
    b, a, s, h, noise, seed = fixed
    return np.stack([photo_record(b, a, s, h, noise, (seed + i) & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF)
                     for i in range(n)])


def rotation_mode(angle: float, w: int, h: int) -> Tuple[int, Tuple[int, ...]]:
    """(rot_mode, 16.16 affine coefficients) for Image.rotate(angle) of a w x h image (NEAREST,
    expand=False): the fast paths of Image.rotate, else its inverse matrix (Python doubles, as
    Pillow computes it) in ImagingTransformAffine's fixed point."""
    angle = angle % 360.0
    if angle == 0:
        return 0, (0,) * 6
    if angle == 180:
        return 1, (0,) * 6
    if angle in (90, 270) and w == h:
        return (3 if angle == 90 else 4), (0,) * 6
    center = (w / 2, h / 2)
    a = -math.radians(angle)
    m = [round(math.cos(a), 15), round(math.sin(a), 15), 0.0, round(-math.sin(a), 15), round(math.cos(a), 15), 0.0]
    x, y = -center[0], -center[1]
    m[2], m[5] = m[0] * x + m[1] * y + m[2], m[3] * x + m[4] * y + m[5]
    m[2] += center[0]
    m[5] += center[1]
    fix = lambda v: int(math.floor(v * 65536.0 + 0.5))  # noqa: E731  (Geometry.c FIX)
    coeffs = (fix(m[0]), fix(m[1]), fix(m[2] + m[1] * 0.5 + m[0] * 0.5), fix(m[3]), fix(m[4]),
              fix(m[5] + m[4] * 0.5 + m[3] * 0.5))
    # check_fixed: the fixed-point walk is Pillow's path while every corner maps inside +-32768
    for cx, cy in ((0, 0), (w, h), (0, h), (w, 0)):
        if abs(m[0] * cx + m[1] * cy + m[2]) >= 32768.0 or abs(m[3] * cx + m[4] * cy + m[5]) >= 32768.0:
            raise NotImplementedError("rotation outside Pillow's fixed-point range (image > 32k pixels)")
    return 2, coeffs


@lru_cache(maxsize=64)
def resample_table(in_size: int, out_size: int) -> Tuple[int, np.ndarray]:
    """(ksize, int32 table) of one Image.resize pass (lss_resample_coeffs: Pillow's bicubic coefficients);
    ksize 0 = the pass is skipped (same size)."""
    if in_size == out_size:
        return 0, np.zeros(0, dtype=np.int32)
    lib = _lib.load()
    k = int(lib.lss_resample_ksize(in_size, out_size))
    tab = np.zeros(out_size * (2 + k), dtype=np.int32)
    _lib.check(lib.lss_resample_coeffs(in_size, out_size, ctypes.c_void_p(tab.ctypes.data)), "lss_resample_coeffs")
    return k, tab


_DEVICE_TABLES: Dict[Tuple[int, int, int], torch.Tensor] = {}


def _device_table(inn: int, outn: int, dev: torch.device) -> Tuple[int, torch.Tensor]:
    """(ksize, device int32 table) of one resize pass, uploaded once per (device, in, out) through
    pinned memory without blocking the host (the pinned block is not reused before the copy ran)."""
    key = (dev.index if dev.index is not None else torch.cuda.current_device(), inn, outn)
    k, tab = resample_table(inn, outn)
    t = _DEVICE_TABLES.get(key)
    if t is None:
        host = torch.from_numpy(tab if tab.size else np.zeros(1, dtype=np.int32)).pin_memory()
        t = host.to(dev, non_blocking=True)
        _DEVICE_TABLES[key] = t
    return k, t


def _to_device_pinned(buf: bytes, dev: torch.device) -> torch.Tensor:
    """Host bytes -> a device uint8 tensor through a pinned staging block, non-blocking."""
    host = torch.empty(len(buf), dtype=torch.uint8, pin_memory=True)
    host.numpy()[:] = np.frombuffer(buf, dtype=np.uint8)
    return host.to(dev, non_blocking=True)


# ----------------------------------------------------------------------------- device kernels
def augment_images(imgs_u8: torch.Tensor, augs: Sequence[dict], final_dim: Sequence[int], out=None,
                   keep=None, photo=None) -> torch.Tensor:
    """(n, H, W, 3) uint8 device images + one aug dict per image (resize_dims, crop, flip, rotate) ->
    (n, 3, fH, fW) fp32 = normalize_img(img_transform(img)) (src/tools.py:120-128, 167-171).

    out: a contiguous fp32 device tensor of n * 3 * fH * fW elements to write instead of a new one.
    keep: a list that receives the device tensors allocated here (the parameter block, the table
    concatenation, the source) -- a caller running this on a side stream holds them until its event.
    photo: None (``lss_simbev_images``), or the (n, 16) fp32 HOST tensor of the images' photometric records
    (photo_record: the byte layout of lss_img_photo_t), uploaded pinned on the current stream and applied by
    ``lss_simbev_images_photo``; neutral records give the same output bit for bit."""
    if not imgs_u8.is_cuda:
        raise RuntimeError("lss_carla_amd.simbev: images must be on the MI355X (no CPU fallback)")
    if imgs_u8.dtype != torch.uint8 or imgs_u8.dim() != 4 or imgs_u8.shape[-1] != 3:
        raise RuntimeError(f"expected (n, H, W, 3) uint8 images, got {imgs_u8.dtype} {tuple(imgs_u8.shape)}")
    n, H, W, _ = imgs_u8.shape
    if len(augs) != n:
        raise RuntimeError(f"{len(augs)} augmentation records for {n} images")
    fH, fW = int(final_dim[0]), int(final_dim[1])
    lib = _lib.load()
    dev = imgs_u8.device
    params = (_lib.ImgAug * n)()
    # the batch's resize tables: device-resident per (in, out) size, concatenated on the device (no
    # host round trip per batch; the first use of a size uploads it without blocking)
    tables: List[torch.Tensor] = []
    offsets: Dict[Tuple[int, int], Tuple[int, int]] = {}
    off = 0

    def table(inn, outn):
        nonlocal off
        key = (inn, outn)
        if key not in offsets:
            k, tab = _device_table(inn, outn, dev)
            offsets[key] = (off, k)
            if k:
                tables.append(tab)
                off += tab.numel()
        return offsets[key]

    for i, a in enumerate(augs):
        rs_w, rs_h = (int(v) for v in a["resize_dims"])
        crop = [int(round(v)) for v in a["crop"]]
        if crop[2] - crop[0] != fW or crop[3] - crop[1] != fH:
            raise RuntimeError(f"crop {crop} is not final_dim {final_dim}")
        p = params[i]
        p.src_h, p.src_w, p.rs_w, p.rs_h = H, W, rs_w, rs_h
        for j in range(4):
            p.crop[j] = crop[j]
        p.flip = 1 if a["flip"] else 0
        mode, co = rotation_mode(float(a["rotate"]), fW, fH)
        p.rot_mode = mode
        for j in range(6):
            p.affine[j] = co[j]
        p.h_off, p.h_ksize = table(W, rs_w)
        p.v_off, p.v_ksize = table(H, rs_h)
    tab_d = (tables[0] if len(tables) == 1 else torch.cat(tables)) if tables else \
        torch.zeros(1, device=dev, dtype=torch.int32)
    par_d = _to_device_pinned(bytes(params), dev)
    photo_d = None
    if photo is not None:
        ph = torch.as_tensor(photo)
        if ph.is_cuda or ph.dtype != torch.float32 or tuple(ph.shape) != (n, PHOTO_WORDS):
            raise RuntimeError(f"photo= must be a host fp32 tensor of {(n, PHOTO_WORDS)}, got {ph.device} {ph.dtype} "
                               f"{tuple(ph.shape)}")
        photo_d = _to_device_pinned(ph.contiguous().numpy().tobytes(), dev)
    src = imgs_u8.contiguous()
    if out is None:
        out = torch.empty(n, 3, fH, fW, device=dev, dtype=torch.float32)
    elif not (out.is_cuda and out.device == dev and out.dtype == torch.float32 and out.is_contiguous()
              and out.numel() == n * 3 * fH * fW):
        raise RuntimeError(f"out= must be a contiguous fp32 device tensor of {(n, 3, fH, fW)}")
    if keep is not None:
        keep.extend([par_d, tab_d, src] if photo_d is None else [par_d, tab_d, src, photo_d])
    if photo_d is not None:
        _lib.check(lib.lss_simbev_images_photo(_lib.ptr(src), n, H, W, _lib.ptr(par_d), _lib.ptr(photo_d),
                                               _lib.ptr(tab_d), fH, fW, _lib.ptr(out), _lib.stream_handle(dev)),
                   "lss_simbev_images_photo")
        return out
    _lib.check(lib.lss_simbev_images(_lib.ptr(src), n, H, W, _lib.ptr(par_d), _lib.ptr(tab_d), fH, fW,
                                     _lib.ptr(out), _lib.stream_handle(dev)), "lss_simbev_images")
    return out


def vehicle_masks(bev_u8: torch.Tensor, out=None) -> torch.Tensor:
    """(n, C, X, Y) uint8 device BEV maps -> (n, 1, X, Y) fp32 binimgs (src/data_simbev.py:236-244);
    out: a contiguous fp32 device tensor of n * X * Y elements to write instead of a new one."""
    if not bev_u8.is_cuda:
        raise RuntimeError("lss_carla_amd.simbev: BEV maps must be on the MI355X (no CPU fallback)")
    if bev_u8.dtype == torch.bool:
        bev_u8 = bev_u8.view(torch.uint8)
    if bev_u8.dtype != torch.uint8:
        bev_u8 = (bev_u8 > 0).to(torch.uint8)
    n, C, X, Y = bev_u8.shape
    if out is None:
        out = torch.empty(n, 1, X, Y, device=bev_u8.device, dtype=torch.float32)
    elif not (out.is_cuda and out.device == bev_u8.device and out.dtype == torch.float32 and out.is_contiguous()
              and out.numel() == n * X * Y):
        raise RuntimeError(f"out= must be a contiguous fp32 device tensor of {(n, 1, X, Y)}")
    b = bev_u8.contiguous()
    _lib.check(_lib.load().lss_simbev_vehicle_mask(_lib.ptr(b), n, C, X, Y, _lib.ptr(out),
                                                   _lib.stream_handle(b.device)), "lss_simbev_vehicle_mask")
    return out


MAX_LABEL_GROUPS = 8  # LSS_SIMBEV_MAX_GROUPS of include/lss_simbev.h


def group_bits(label_groups, n_classes: int = 32) -> List[int]:
    """One bit mask over the npz channels per group of ``label_groups`` (a list of lists of channel
    indices); raises ValueError for an empty list, an empty group or a channel outside [0, n_classes)."""
    groups = [list(g) for g in label_groups]
    if not 1 <= len(groups) <= MAX_LABEL_GROUPS:
        raise ValueError(f"label_groups: 1..{MAX_LABEL_GROUPS} groups, got {len(groups)}")
    bits = []
    for g in groups:
        if not g:
            raise ValueError(f"label_groups {groups}: an empty group")
        m = 0
        for c in g:
            if int(c) != c or not 0 <= int(c) < n_classes:
                raise ValueError(f"label_groups {groups}: channel {c!r} is outside 0..{n_classes - 1}")
            m |= 1 << int(c)
        bits.append(m)
    return bits


VEHICLE_GROUPS = [[1, 2, 3]]  # get_binimg's merge (src/data_simbev.py:236-244) as label groups


def class_masks(bev_u8: torch.Tensor, label_groups=None, out=None, index_mats=None, keep=None) -> torch.Tensor:
    """(n, C, X, Y) uint8 device BEV maps -> (n, K, X, Y) fp32 labels, one channel per group of
    ``label_groups`` (K lists of npz channel indices): out[:, k] = flipud(any(bev[:, c] > 0 for c in group
    k)), ``lss_simbev_class_masks``. None: the reference's single vehicle mask [[1, 2, 3]] through
    ``vehicle_masks``, as before. out: a contiguous fp32 device tensor of n * K * X * Y elements to write.

    index_mats: (n, 2, 3) fp32, host or device -- each sample's ``label_index_matrix``: the labels under the
    BEV-space augmentation, gathered by ``lss_simbev_class_masks_warp`` (nearest neighbour, 0 outside the grid);
    label_groups None is then [[1, 2, 3]] through that kernel. keep: a list that receives the device copy of host
    matrices -- a caller on a side stream holds it until its event, as with ``augment_images``."""
    if label_groups is None:
        if index_mats is None:
            return vehicle_masks(bev_u8, out=out)
        label_groups = VEHICLE_GROUPS
    if not bev_u8.is_cuda:
        raise RuntimeError("lss_carla_amd.simbev: BEV maps must be on the MI355X (no CPU fallback)")
    if bev_u8.dtype == torch.bool:
        bev_u8 = bev_u8.view(torch.uint8)
    if bev_u8.dtype != torch.uint8:
        bev_u8 = (bev_u8 > 0).to(torch.uint8)
    n, C, X, Y = bev_u8.shape
    bits = group_bits(label_groups)  # (the channel range is the kernel entry's check: it knows C)
    K = len(bits)
    if out is None:
        out = torch.empty(n, K, X, Y, device=bev_u8.device, dtype=torch.float32)
    elif not (out.is_cuda and out.device == bev_u8.device and out.dtype == torch.float32 and out.is_contiguous()
              and out.numel() == n * K * X * Y):
        raise RuntimeError(f"out= must be a contiguous fp32 device tensor of {(n, K, X, Y)}")
    b = bev_u8.contiguous()
    host = (ctypes.c_uint32 * K)(*bits)
    if index_mats is None:
        _lib.check(_lib.load().lss_simbev_class_masks(_lib.ptr(b), n, C, X, Y, ctypes.cast(host, ctypes.c_void_p), K,
                                                      _lib.ptr(out), _lib.stream_handle(b.device)),
                   "lss_simbev_class_masks")
        return out
    mats = torch.as_tensor(index_mats)
    if mats.dtype != torch.float32 or tuple(mats.shape) != (n, 2, 3):
        raise RuntimeError(f"index_mats= must be {(n, 2, 3)} fp32, got {mats.dtype} {tuple(mats.shape)}")
    if not mats.is_cuda:
        mats = mats.contiguous().pin_memory().to(b.device, non_blocking=True)
    elif mats.device != b.device:
        raise RuntimeError(f"index_mats= is on {mats.device}, the BEV maps on {b.device}")
    mats = mats.contiguous()
    if keep is not None:
        keep.extend([mats, b])
    _lib.check(_lib.load().lss_simbev_class_masks_warp(_lib.ptr(b), n, C, X, Y, ctypes.cast(host, ctypes.c_void_p), K,
                                                       _lib.ptr(mats), _lib.ptr(out), _lib.stream_handle(b.device)),
               "lss_simbev_class_masks_warp")
    return out


MAX_EXCLUSIVE_GROUPS = 7  # LSS_SIMBEV_MAX_EXCLUSIVE_GROUPS: C = K + 1 classes on the K-channel head (C <= 8)
IGNORE_LABEL = 255        # the class-map value no class has: losses and metrics skip the cell


def exclusive_bits(label_groups) -> List[int]:
    """group_bits for the exclusive class map: 1..7 groups (class 0 is the background, class k + 1 is group k)."""
    bits = group_bits(label_groups)
    if len(bits) > MAX_EXCLUSIVE_GROUPS:
        raise ValueError(f"exclusive classes: 1..{MAX_EXCLUSIVE_GROUPS} label groups, got {len(bits)}")
    return bits


def class_index(bev_u8: torch.Tensor, label_groups, out=None, index_mats=None, keep=None) -> torch.Tensor:
    """(n, C, X, Y) uint8 device BEV maps -> the (n, X, Y) uint8 exclusive class map of K = len(label_groups) groups,
    ``lss_simbev_class_index``: 0 where no group has a set channel (background), else 1 + the highest such group --
    the groups are painted in order and a later one wins, so with "0;1,2,3;6,7" a road cell under a vehicle is
    vehicle. Equal to that rule applied to ``class_masks``' planes. out: a contiguous uint8 device tensor of
    n * X * Y elements to write. index_mats / keep: as ``class_masks`` -- the map under the BEV-space augmentation;
    a cell whose source is outside the grid is 0 (``valid_mask`` mode "grid" is what ignores it)."""
    if not bev_u8.is_cuda:
        raise RuntimeError("lss_carla_amd.simbev: BEV maps must be on the MI355X (no CPU fallback)")
    if bev_u8.dtype == torch.bool:
        bev_u8 = bev_u8.view(torch.uint8)
    if bev_u8.dtype != torch.uint8:
        bev_u8 = (bev_u8 > 0).to(torch.uint8)
    n, C, X, Y = bev_u8.shape
    bits = exclusive_bits(label_groups)
    K = len(bits)
    if out is None:
        out = torch.empty(n, X, Y, device=bev_u8.device, dtype=torch.uint8)
    elif not (out.is_cuda and out.device == bev_u8.device and out.dtype == torch.uint8 and out.is_contiguous()
              and out.numel() == n * X * Y):
        raise RuntimeError(f"out= must be a contiguous uint8 device tensor of {(n, X, Y)}")
    b = bev_u8.contiguous()
    host = (ctypes.c_uint32 * K)(*bits)
    mats = None
    if index_mats is not None:
        mats = torch.as_tensor(index_mats)
        if mats.dtype != torch.float32 or tuple(mats.shape) != (n, 2, 3):
            raise RuntimeError(f"index_mats= must be {(n, 2, 3)} fp32, got {mats.dtype} {tuple(mats.shape)}")
        if not mats.is_cuda:
            mats = mats.contiguous().pin_memory().to(b.device, non_blocking=True)
        elif mats.device != b.device:
            raise RuntimeError(f"index_mats= is on {mats.device}, the BEV maps on {b.device}")
        mats = mats.contiguous()
        if keep is not None:
            keep.extend([mats, b])
    _lib.check(_lib.load().lss_simbev_class_index(_lib.ptr(b), n, C, X, Y, ctypes.cast(host, ctypes.c_void_p), K,
                                                  _lib.ptr(mats), _lib.ptr(out), _lib.stream_handle(b.device)),
               "lss_simbev_class_index")
    return out


def class_index_from_masks(masks) -> "np.ndarray":
    """The paint-order rule on (n, K, X, Y) group planes (a tensor or an array, any value != 0 = set), on the host:
    0 where no plane is set, else 1 + the highest set plane. What ``class_index`` equals bit for bit."""
    m = np.asarray(masks.detach().cpu() if torch.is_tensor(masks) else masks) != 0
    out = np.zeros((m.shape[0],) + m.shape[2:], dtype=np.uint8)
    for k in range(m.shape[1]):
        out[m[:, k]] = k + 1
    return out


# ----------------------------------------------------------------------------- valid-cell mask
VALID_MASK_MODES = ("grid", "fov")   # LSS_SIMBEV_VALID_GRID / LSS_SIMBEV_VALID_FOV of include/lss_simbev.h
MAX_FOV_HEIGHTS = 8                  # LSS_SIMBEV_MAX_HEIGHTS


def valid_mask_mode(conf: dict):
    """The valid-cell mask a data_aug_conf asks for: None (the key ``valid_mask`` absent, None or "none"), "grid"
    (cells whose label source lies inside the labelled grid under the BEV-space augmentation) or "fov" (those that
    some camera also sees, at one of the heights ``fov_z``). ValueError for another value or bad heights. The batches
    of such a conf carry the mask after the labels, and this is the flag their consumers are given."""
    mode = conf.get("valid_mask")
    if mode is None or mode == "none":
        return None
    if mode not in VALID_MASK_MODES:
        raise ValueError(f"valid_mask {mode!r}: none, grid or fov")
    fov_heights(conf)
    return mode


def fov_heights(conf: dict) -> Tuple[float, ...]:
    """The heights (metres, ego frame) a cell is tested at: ``fov_z`` of a data_aug_conf, default (0.0,); 1 to 8
    finite numbers, else ValueError."""
    z = conf.get("fov_z", (0.0,))
    z = (float(z),) if isinstance(z, (int, float)) else tuple(float(v) for v in z)
    if not 1 <= len(z) <= MAX_FOV_HEIGHTS or not all(math.isfinite(v) for v in z):
        raise ValueError(f"fov_z {z!r}: 1 to {MAX_FOV_HEIGHTS} finite heights")
    return z


def fov_cameras(rots, trans, intrins, post_rots, post_trans=None, alive=None) -> torch.Tensor:
    """The (..., N, 16) fp32 camera blocks ``lss_simbev_valid_mask`` projects cell centres with, from the host rig
    (rots (..., N, 3, 3), trans (..., N, 3), intrins, post_rots): per camera M = intrins rots^-1 (9, row-major),
    o = -M trans (3) and P = post_rots[:2, :2] (4) -- get_geometry (src/models.py:170-192) inverted: an ego point p
    is the camera point M p + o = (u' d, v' d, d), and its pixel is P (u', v') + post_trans[:2]. Computed in
    float64, rounded once. A rig composed with the BEV-space augmentation needs nothing more:
    (A rots)^-1 (A p - A t) is the original camera point. post_trans is not used (valid_mask takes it beside the
    blocks); it is accepted so that a batch's five rig tensors can be passed as they come. alive: a (..., N) or (N,)
    mask (bool / uint8 / numbers, 0 = dead): a dead camera's 16 floats are all zero, and a zero block sees nothing --
    every cell projects to depth d = 0, which ``lss_simbev_valid_mask`` (d >= d_lo > 0) rejects."""
    r, t = torch.as_tensor(rots).detach().cpu().double(), torch.as_tensor(trans).detach().cpu().double()
    k, p = torch.as_tensor(intrins).detach().cpu().double(), torch.as_tensor(post_rots).detach().cpu().double()
    M = k.matmul(torch.linalg.inv(r))
    o = -M.matmul(t.unsqueeze(-1)).squeeze(-1)
    P = p[..., :2, :2]
    lead = M.shape[:-2]
    cams = torch.cat([M.reshape(*lead, 9), o, P.reshape(*lead, 4)], dim=-1).to(torch.float32)
    if alive is not None:
        on = torch.as_tensor(alive).detach().cpu() != 0
        if on.dim() < 1 or on.shape[-1] != cams.shape[-2]:
            raise ValueError(f"fov_cameras: alive {tuple(on.shape)} for {cams.shape[-2]} cameras")
        cams = torch.where(on.expand(lead).unsqueeze(-1), cams, torch.zeros((), dtype=torch.float32))
    return cams.contiguous()


def valid_mask(cams, post_trans, grid_conf, final_dim, heights=(0.0,), index_mats=None, mode="fov", out=None,
               keep=None) -> torch.Tensor:
    """The (n, X, Y) uint8 valid-cell mask of a batch, ``lss_simbev_valid_mask``: 1 where a cell is in the grid --
    index_mats (n, 2, 3) fp32, the batch's ``label_index_matrix`` rows; None: every cell is -- and, with mode "fov",
    some camera sees its centre at one of `heights`: cams (n, N, 16) from ``fov_cameras``, post_trans (n, N, 3) or
    (n, N, 2), the frustum dbound of grid_conf and final_dim (fH, fW). mode "grid": cams and post_trans may be None
    (n then comes from index_mats or out). Host tensors are uploaded pinned, without blocking; keep: a list that
    receives what was allocated here -- a caller on a side stream holds it until its event. out: a contiguous uint8
    device tensor of n * X * Y elements to write. Row i is x cell i, column j is y cell j, as the logits."""
    if mode not in VALID_MASK_MODES:
        raise ValueError(f"valid_mask: mode {mode!r}: grid or fov")
    from .ops import GridSpec
    from .tools import gen_dx_bx
    z = fov_heights({"fov_z": heights})
    X, Y, _ = GridSpec.from_conf(grid_conf).nx
    dx, bx, _ = gen_dx_bx(grid_conf["xbound"], grid_conf["ybound"], grid_conf["zbound"])
    d_lo, d_hi = float(grid_conf["dbound"][0]), float(grid_conf["dbound"][1])
    fH, fW = int(final_dim[0]), int(final_dim[1])
    fov = mode == "fov"
    dev = next((t.device for t in (out, cams, index_mats, post_trans) if torch.is_tensor(t) and t.is_cuda), None)
    if dev is None:
        raise RuntimeError("lss_carla_amd.simbev: valid_mask runs on the MI355X (pass out= or a device tensor)")

    def device(t, shape_tail, what):
        t = torch.as_tensor(t)
        if t.dtype != torch.float32 or tuple(t.shape[1:]) != shape_tail:
            raise RuntimeError(f"valid_mask: {what} must be (n, {', '.join(map(str, shape_tail))}) fp32, got "
                               f"{t.dtype} {tuple(t.shape)}")
        if not t.is_cuda:
            t = t.contiguous().pin_memory().to(dev, non_blocking=True)
        elif t.device != dev:
            raise RuntimeError(f"valid_mask: {what} is on {t.device}, not {dev}")
        t = t.contiguous()
        if keep is not None:
            keep.append(t)
        return t

    n = N = None
    cams_d = q_d = mats_d = None
    if fov:
        if cams is None or post_trans is None:
            raise RuntimeError("valid_mask: mode 'fov' needs the camera blocks and post_trans")
        cams = torch.as_tensor(cams)
        if cams.dim() != 3 or cams.shape[1] < 1:
            raise RuntimeError(f"valid_mask: cams must be (n, N, 16) with N >= 1, got {tuple(cams.shape)}")
        n, N = int(cams.shape[0]), int(cams.shape[1])
        cams_d = device(cams, (N, 16), "cams")
        q = torch.as_tensor(post_trans)
        if q.dim() == 3 and q.shape[-1] == 3:
            q = q[..., :2]
        q_d = device(q, (N, 2), "post_trans")
        if q_d.shape[0] != n:
            raise RuntimeError(f"valid_mask: post_trans of {q_d.shape[0]} samples for cams of {n}")
    if index_mats is not None:
        mats_d = device(index_mats, (2, 3), "index_mats")
        if n is not None and mats_d.shape[0] != n:
            raise RuntimeError(f"valid_mask: index_mats of {mats_d.shape[0]} samples for cams of {n}")
        n = int(mats_d.shape[0])
    if n is None:
        if out is None:
            raise RuntimeError("valid_mask: mode 'grid' without index_mats needs out= (it gives the batch size)")
        n = out.numel() // (X * Y)
    if out is None:
        out = torch.empty(n, X, Y, device=dev, dtype=torch.uint8)
    elif not (out.is_cuda and out.device == dev and out.dtype == torch.uint8 and out.is_contiguous()
              and out.numel() == n * X * Y and n > 0):
        raise RuntimeError(f"out= must be a contiguous uint8 device tensor of {(n, X, Y)}")
    hz = (ctypes.c_float * len(z))(*z)
    with torch.cuda.device(dev):
        _lib.check(_lib.load().lss_simbev_valid_mask(
            _lib.ptr(cams_d), _lib.ptr(q_d), n, N or 0, X, Y, float(bx[0]), float(dx[0]), float(bx[1]), float(dx[1]),
            ctypes.cast(hz, ctypes.c_void_p), len(z), d_lo, d_hi, fH, fW, _lib.ptr(mats_d),
            VALID_MASK_MODES.index(mode), _lib.ptr(out), _lib.stream_handle(dev)), "lss_simbev_valid_mask")
    return out


# ----------------------------------------------------------------------------- dataset (host side)
class SimBEVDataset(torch.utils.data.Dataset):
    """src/data_simbev.py:23-265: same layout (SimBEV_cvt_label/scene_*/yaw0pitch0/meta.json, 80/20
    scene split), same augmentation draws. ``__getitem__`` returns the raw sample (decoded uint8
    images + calibration + augmentation + uint8 BEV); ``compile_data``'s loader finishes it on the device."""

    def __init__(self, dataroot, is_train, data_aug_conf, grid_conf):
        self.dataroot = Path(dataroot)
        self.is_train = is_train
        self.data_aug_conf = data_aug_conf
        self.grid_conf = grid_conf
        self.samples = self._load_all_samples()
        from .tools import gen_dx_bx
        dx, bx, nx = gen_dx_bx(grid_conf["xbound"], grid_conf["ybound"], grid_conf["zbound"])
        self.dx, self.bx, self.nx = dx.numpy(), bx.numpy(), nx.numpy()
        # the conf asks for the BEV-space augmentation: every sample (validation's too, with the identity) then
        # carries its label index matrix directly before the BEV map
        self.bev_aug = bev_aug_enabled(data_aug_conf)
        # the conf asks for the photometric augmentation: every sample (validation's with the neutral record, or the
        # ``photo_fixed`` one) then carries its (N, 16) photo records before the label index matrix / the BEV map
        self.photo = photo_enabled(data_aug_conf)
        self.photo_fixed = photo_fixed_record(data_aug_conf) if self.photo else None
        self.photo_per_camera = _photo_lims(data_aug_conf)[2] if self.photo else True
        print(self)

    def _load_all_samples(self):
        labels_dir = self.dataroot / "SimBEV_cvt_label"
        if not labels_dir.exists():
            raise FileNotFoundError(f"Labels directory not found: {labels_dir}")
        scene_dirs = sorted([d for d in labels_dir.iterdir() if d.is_dir() and d.name.startswith("scene_")])
        if not scene_dirs:
            raise FileNotFoundError(f"No scene directories found in {labels_dir}")
        train_split = int(0.8 * len(scene_dirs))
        selected = scene_dirs[:train_split] if self.is_train else scene_dirs[train_split:]
        out = []
        for scene_dir in selected:
            meta_path = scene_dir / "yaw0pitch0" / "meta.json"
            if not meta_path.exists():
                continue
            with open(meta_path) as f:
                for s in json.load(f):
                    s["scene_dir"] = scene_dir
                    s["meta_dir"] = meta_path.parent
                    out.append(s)
        if not out:
            raise FileNotFoundError(f"No samples found for {'train' if self.is_train else 'val'} split in {labels_dir}")
        return out

    def sample_augmentation(self):
        """(resize, resize_dims, crop box, flip, rotate) of one sample (src/data_simbev.py:119-145).

        Training draws from numpy's global generator in the reference's order -- scale, bottom-crop
        fraction, horizontal crop offset, the flip coin (only when rand_flip is on), rotation -- so a
        seeded run reproduces the reference loader's augmentations; validation uses the fixed
        fit-to-width scale, the mean bottom fraction and a centred window."""
        return draw_augmentation(self.data_aug_conf, self.is_train)

    def sample_bev_augmentation(self):
        """(theta_deg, scale, flip_x, flip_y) of one sample's BEV-space augmentation (draw_bev_augmentation): drawn
        after sample_augmentation's values; the identity, and no draw, for validation or a conf without it."""
        return draw_bev_augmentation(self.data_aug_conf, self.is_train)

    def sample_photo_augmentation(self, n_cams: int) -> np.ndarray:
        """The (n_cams, 16) photo records of one sample: training draws one per camera (one per sample with
        photo_per_camera 0) after the sample's other draws (draw_photo_augmentation); validation draws nothing and
        carries the neutral record, or the conf's ``photo_fixed`` one (which training ignores)."""
        if not self.is_train:
            if self.photo_fixed is not None:
                return photo_fixed_records(self.photo_fixed, n_cams)
            return np.stack([photo_record()] * n_cams)
        if self.photo_per_camera:
            return np.stack([photo_record(*draw_photo_augmentation(self.data_aug_conf, True)) for _ in range(n_cams)])
        return np.stack([photo_record(*draw_photo_augmentation(self.data_aug_conf, True))] * n_cams)

    def get_image_data(self, sample, cam_indices):
        """Decoded images and calibration (src/data_simbev.py:147-218 without the pixel work); with the BEV-space
        augmentation on, rots / trans are the composed ones (compose_rig)."""
        return self._image_data(sample, cam_indices)[0]

    def _image_data(self, sample, cam_indices):
        """(get_image_data's tuple, the sample's label index matrix (2, 3) or None without the BEV augmentation,
        the sample's (N, 16) photo records or None without the photometric augmentation)."""
        from PIL import Image
        resize, resize_dims, crop, flip, rotate = self.sample_augmentation()
        bev_aug = self.sample_bev_augmentation() if self.bev_aug else None
        photo = torch.from_numpy(self.sample_photo_augmentation(len(cam_indices))) if self.photo else None
        imgs, rots, trans, intrins, post_rots, post_trans = [], [], [], [], [], []
        for cam_idx in cam_indices:
            img = Image.open(self.dataroot / sample["images"][cam_idx]).convert("RGB")
            imgs.append(torch.from_numpy(np.asarray(img, dtype=np.uint8).copy()))
            intrins.append(torch.Tensor(sample["intrinsics"][cam_idx]))
            extrin = np.array(sample["extrinsics"][cam_idx])
            rots.append(torch.Tensor(extrin[:3, :3]))
            trans.append(torch.Tensor(extrin[:3, 3]))
            pr, pt = post_homography(resize, crop, flip, rotate)
            post_rots.append(pr)
            post_trans.append(pt)
        aug = torch.tensor([resize_dims[0], resize_dims[1], crop[0], crop[1], crop[2], crop[3], int(flip)],
                           dtype=torch.int64)
        rots, trans, index_mat = torch.stack(rots), torch.stack(trans), None
        if bev_aug is not None:
            A = bev_aug_matrix(*bev_aug)
            if tuple(bev_aug) != BEV_AUG_IDENTITY:  # (validation: the rig as it is, the identity for the labels)
                rots, trans = compose_rig(A, rots, trans)
            index_mat = torch.from_numpy(label_index_matrix(A, self.grid_conf))
        return (torch.stack(imgs), rots, trans, torch.stack(intrins), torch.stack(post_rots), torch.stack(post_trans),
                aug, torch.tensor(float(rotate), dtype=torch.float64)), index_mat, photo

    def get_bev_raw(self, sample):
        """The BEV npz's (n_classes, X, Y) map as uint8 (value > 0 kept), src/data_simbev.py:227-232."""
        bev = np.load(sample["meta_dir"] / sample["bev"])["bev"]
        return torch.from_numpy((bev > 0).astype(np.uint8) if bev.dtype != np.uint8 else bev.copy())

    def _labels(self, sample, index_mat, photo=None):
        """The sample's tail: the BEV map, last; directly before it the label index matrix when the conf asks
        for the BEV-space augmentation; before those the photo records when it asks for the photometric one."""
        bev = self.get_bev_raw(sample)
        tail = (bev,) if index_mat is None else (index_mat, bev)
        return tail if photo is None else (photo,) + tail

    def choose_cams(self):
        all_cams = list(range(len(CAMERA_ORDER)))
        if self.is_train and "Ncams" in self.data_aug_conf:
            Ncams = self.data_aug_conf["Ncams"]
            if Ncams < len(CAMERA_ORDER):
                return sorted(np.random.choice(all_cams, Ncams, replace=False).tolist())
        return all_cams

    def __len__(self):
        return len(self.samples)

    def __str__(self):
        return f"SimBEVDataset ({'train' if self.is_train else 'val'}): {len(self)} samples"


class VizData(SimBEVDataset):
    def __getitem__(self, index):
        sample = self.samples[index]
        raw, index_mat, photo = self._image_data(sample, self.choose_cams())
        return raw + (torch.empty(3, 0),) + self._labels(sample, index_mat, photo)


class SegmentationData(SimBEVDataset):
    def __getitem__(self, index):
        sample = self.samples[index]
        raw, index_mat, photo = self._image_data(sample, self.choose_cams())
        return raw + self._labels(sample, index_mat, photo)


def worker_rnd_init(x):
    np.random.seed(13 + x)  # src/data_simbev.py:310-312


def finish_batch(batch, final_dim, device, label_groups=None, bev_aug=False, valid_mask_conf=None, exclusive=False,
                 photo=False):
    """A collated raw batch -> the reference's (imgs, rots, trans, intrins, post_rots, post_trans,
    [lidar,] binimgs) on `device`, the pixel work done by the HIP kernels. label_groups: K lists of BEV
    channels -> binimgs (B, K, X, Y) (class_masks); None: the reference's vehicle mask, (B, 1, X, Y).
    bev_aug: the batch comes from a conf with the BEV-space augmentation (bev_aug_enabled): the element before
    the BEV maps is the (B, 2, 3) label index matrices, which warp the labels; the rig is already composed.
    valid_mask_conf: None (the tuple is as above), or (mode, grid_conf, heights) -- the finished batch then carries,
    after the labels, the (B, X, Y) uint8 valid-cell mask of ``valid_mask`` on the batch's host rig.
    exclusive: binimgs is the (B, X, Y) uint8 exclusive class map of the groups (class_index) instead.
    photo: the batch comes from a conf with the photometric augmentation (photo_enabled): the element before the label
    index matrices (before the BEV maps without bev_aug) is the (B, N, 16) photo records, which the image kernel
    applies (augment_images, photo=); the finished tuple does not change."""
    if exclusive and label_groups is None:
        raise ValueError("exclusive classes need label_groups")
    imgs_u8, rots, trans, intrins, post_rots, post_trans, aug, rot = batch[:8]
    rest = batch[8:]
    index_mats = None
    if bev_aug:
        index_mats, rest = rest[-2], tuple(rest[:-2]) + tuple(rest[-1:])
    records = None
    if photo:
        records, rest = rest[-2], tuple(rest[:-2]) + tuple(rest[-1:])
    B, N = imgs_u8.shape[:2]
    src = imgs_u8.reshape(B * N, *imgs_u8.shape[2:]).to(device, non_blocking=True)
    augs = []
    for b in range(B):
        a = aug[b].tolist()
        rec = {"resize_dims": (a[0], a[1]), "crop": tuple(a[2:6]), "flip": bool(a[6]), "rotate": float(rot[b])}
        augs.extend([rec] * N)
    if records is None:
        imgs = augment_images(src, augs, final_dim)
    else:
        imgs = augment_images(src, augs, final_dim, photo=records.reshape(B * N, PHOTO_WORDS))
    imgs = imgs.view(B, N, 3, int(final_dim[0]), int(final_dim[1]))
    out = [imgs] + [t.to(device, non_blocking=True) for t in (rots, trans, intrins, post_rots, post_trans)]
    # the host copies ride along: the model's host torch.inverse (src/models.py:180,186) reads them
    # instead of copying the device tensors back (ops.camera_inverses), so no batch syncs the host
    out[3]._lss_host, out[3]._lss_host_version = intrins, out[3]._version
    out[4]._lss_host, out[4]._lss_host_version = post_rots, out[4]._version
    for t in rest[:-1]:
        out.append(t)  # lidar placeholder (VizData)
    if exclusive:
        out.append(class_index(rest[-1].to(device, non_blocking=True), label_groups, index_mats=index_mats))
    else:
        out.append(class_masks(rest[-1].to(device, non_blocking=True), label_groups, index_mats=index_mats))
    if valid_mask_conf is not None:
        mode, grid_conf, heights = valid_mask_conf
        X, Y = out[-1].shape[-2:]
        mask = torch.empty(B, X, Y, device=device, dtype=torch.uint8)
        cams = fov_cameras(rots, trans, intrins, post_rots) if mode == "fov" else None
        out.append(valid_mask(cams, post_trans if mode == "fov" else None, grid_conf, final_dim, heights,
                              index_mats=index_mats, mode=mode, out=mask))
    return tuple(out)


class DeviceLoader:
    """Iterates a DataLoader of raw samples and yields finished device batches (finish_batch)."""

    def __init__(self, loader, final_dim, device, label_groups=None, bev_aug=False, valid_mask_conf=None,
                 exclusive=False, photo=False):
        self.loader, self.final_dim, self.device = loader, final_dim, torch.device(device)
        self.label_groups, self.bev_aug = label_groups, bool(bev_aug)
        self.exclusive = bool(exclusive)  # the labels are the (B, X, Y) uint8 class map (class_index)
        self.valid_mask_conf = valid_mask_conf  # None, or (mode, grid_conf, heights): finish_batch appends the mask
        self.photo = bool(photo)  # the raw batches hold the (B, N, 16) photo records (photo_enabled)
        self.dataset = loader.dataset
        self.batch_size = loader.batch_size

    def __len__(self):
        return len(self.loader)

    def __iter__(self):
        for batch in self.loader:
            if self.photo:
                yield finish_batch(batch, self.final_dim, self.device, self.label_groups, self.bev_aug,
                                   self.valid_mask_conf, exclusive=self.exclusive, photo=True)
            elif self.exclusive:
                yield finish_batch(batch, self.final_dim, self.device, self.label_groups, self.bev_aug,
                                   self.valid_mask_conf, exclusive=True)
            elif self.valid_mask_conf is None:
                yield finish_batch(batch, self.final_dim, self.device, self.label_groups, self.bev_aug)
            else:
                yield finish_batch(batch, self.final_dim, self.device, self.label_groups, self.bev_aug,
                                   self.valid_mask_conf)


def compile_data(version, dataroot, data_aug_conf, grid_conf, bsz, nworkers, parser_name, device="cuda",
                 label_groups=None, exclusive=False):
    """src/data_simbev.py:315-354 with the same loaders' settings; returns DeviceLoaders. label_groups: the
    BEV channel groups of a multi-class model's labels (finish_batch); None: the reference's vehicle mask.
    A data_aug_conf with bev_rot_lim / bev_scale_lim / bev_flip (bev_aug_enabled) adds the BEV-space augmentation to
    the training loader -- the rig composed, the labels warped -- and never to the validation loader; both loaders
    carry the flag (``bev_aug``) that says their raw batches hold the label index matrices. A data_aug_conf with
    ``valid_mask`` "grid" or "fov" (valid_mask_mode; heights ``fov_z``) makes both loaders' finished batches carry the
    valid-cell mask after the labels -- validation's too: that is the point of a masked metric. exclusive: the labels
    of both loaders are the (B, X, Y) uint8 exclusive class map of the 1..7 label_groups (class_index).
    A data_aug_conf with a photo_*_lim (photo_brightness_lim, photo_contrast_lim, photo_saturation_lim, photo_hue_lim,
    photo_noise_lim; photo_prob, photo_per_camera) adds the photometric augmentation to the training loader's images --
    drawn per camera on the host, applied by ``lss_simbev_images_photo`` -- and never to the validation loader, whose
    records are neutral unless ``photo_fixed`` (a dict of brightness, contrast, saturation, hue, noise, seed) names one
    shift for every validation image; both loaders carry the flag (``photo``) that says their raw batches hold the
    records. Without any of these keys the loaders draw, return and launch exactly what they did before."""
    bev_aug = bev_aug_enabled(data_aug_conf)  # (a bad limit fails here)
    photo = photo_enabled(data_aug_conf)
    mask_mode = valid_mask_mode(data_aug_conf)
    mask_conf = None if mask_mode is None else (mask_mode, grid_conf, fov_heights(data_aug_conf))
    if label_groups is not None:
        group_bits(label_groups)  # a bad group list fails here, not in the first batch
    if exclusive:
        if label_groups is None:
            raise ValueError("exclusive classes need label_groups")
        exclusive_bits(label_groups)
    parser = {"vizdata": VizData, "segmentationdata": SegmentationData}[parser_name]
    traindata = parser(dataroot, is_train=True, data_aug_conf=data_aug_conf, grid_conf=grid_conf)
    valdata = parser(dataroot, is_train=False, data_aug_conf=data_aug_conf, grid_conf=grid_conf)
    trainloader = torch.utils.data.DataLoader(traindata, batch_size=bsz, shuffle=True, num_workers=nworkers,
                                              drop_last=True, worker_init_fn=worker_rnd_init, pin_memory=True)
    valloader = torch.utils.data.DataLoader(valdata, batch_size=bsz, shuffle=False, num_workers=nworkers,
                                            pin_memory=True)
    fd = data_aug_conf["final_dim"]
    if photo:
        return (DeviceLoader(trainloader, fd, device, label_groups, bev_aug, mask_conf, exclusive=exclusive, photo=True),
                DeviceLoader(valloader, fd, device, label_groups, bev_aug, mask_conf, exclusive=exclusive, photo=True))
    if exclusive:
        return (DeviceLoader(trainloader, fd, device, label_groups, bev_aug, mask_conf, exclusive=True),
                DeviceLoader(valloader, fd, device, label_groups, bev_aug, mask_conf, exclusive=True))
    return (DeviceLoader(trainloader, fd, device, label_groups, bev_aug, mask_conf),
            DeviceLoader(valloader, fd, device, label_groups, bev_aug, mask_conf))
