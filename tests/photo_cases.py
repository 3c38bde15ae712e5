"""Numpy restatements the photometric-augmentation tests share (no GPU, no import of the code under test):
``photo_matrix`` in float64, Philox4x32-10 in uint64 arithmetic, the byte-sum noise, and the kernel's per-pixel
fp32 chain in ``np.float32`` operations in the order include/lss_simbev.h states; plus the augmentation cases of
tests/test_gpu_photo.py."""
import math

import numpy as np

LUMA = np.array([0.299, 0.587, 0.114], dtype=np.float64)
YIQ = np.array([[0.299, 0.587, 0.114], [0.595716, -0.274453, -0.321263], [0.211456, -0.522591, 0.311135]],
               dtype=np.float64)
MEAN = np.array([0.485, 0.456, 0.406], dtype=np.float32)
STD = np.array([0.229, 0.224, 0.225], dtype=np.float32)
INV_STD = np.float32(1.0 / math.sqrt(4.0 * (256.0 ** 2 - 1.0) / 12.0))  # 0.006765875f


def photo_matrix(brightness=0.0, contrast=1.0, saturation=1.0, hue_deg=0.0):
    """(M (3, 3), t (3,)) fp32: brightness, contrast, saturation, hue in that order, float64, rounded once; a neutral
    op is skipped."""
    M, t = np.eye(3), np.zeros(3)
    if brightness != 0.0:
        t = t + float(brightness)
    if contrast != 1.0:
        M, t = contrast * M, contrast * (t - 127.5) + 127.5
    if saturation != 1.0:
        S = saturation * np.eye(3) + (1.0 - saturation) * np.outer(np.ones(3), LUMA)
        M, t = S @ M, S @ t
    if hue_deg != 0.0:
        c, s = math.cos(math.radians(hue_deg)), math.sin(math.radians(hue_deg))
        R = np.array([[1.0, 0.0, 0.0], [0.0, c, -s], [0.0, s, c]])
        H = np.linalg.inv(YIQ) @ R @ YIQ
        M, t = H @ M, H @ t
    return M.astype(np.float32), t.astype(np.float32)


def record(brightness=0.0, contrast=1.0, saturation=1.0, hue_deg=0.0, noise=0.0, seed0=0, seed1=0):
    """The 16 words of lss_img_photo_t as fp32, the seed words bit-cast."""
    M, t = photo_matrix(brightness, contrast, saturation, hue_deg)
    rec = np.zeros(16, dtype=np.float32)
    rec[:9], rec[9:12], rec[12] = M.reshape(9), t, np.float32(noise)
    rec.view(np.uint32)[13:15] = (seed0, seed1)
    return rec


def philox4x32_10(key, counter):
    """Philox4x32-10 on arrays: key (2,) and counter (..., 4) of integers -> (..., 4) uint32; uint64 arithmetic."""
    m32 = np.uint64(0xFFFFFFFF)
    c = [np.asarray(counter[..., i], dtype=np.uint64) & m32 for i in range(4)]
    k0, k1 = np.uint64(int(key[0]) & 0xFFFFFFFF), np.uint64(int(key[1]) & 0xFFFFFFFF)
    M0, M1 = np.uint64(0xD2511F53), np.uint64(0xCD9E8D57)
    for _ in range(10):
        p0, p1 = M0 * c[0], M1 * c[2]  # 32 x 32 -> 64 bits: no overflow in uint64
        hi0, lo0, hi1, lo1 = p0 >> np.uint64(32), p0 & m32, p1 >> np.uint64(32), p1 & m32
        c = [hi1 ^ c[1] ^ k0, lo1, hi0 ^ c[3] ^ k1, lo0]
        k0, k1 = (k0 + np.uint64(0x9E3779B9)) & m32, (k1 + np.uint64(0xBB67AE85)) & m32
    return np.stack(c, axis=-1).astype(np.uint32)


def noise_z(key, img, n_pix):
    """z (n_pix, 3) fp32 of image `img`: counter (pix, img, 0, 0); s_c = the sum of the four bytes of word c;
    z_c = float32(s_c - 510) * INV_STD, one fp32 product."""
    ctr = np.zeros((n_pix, 4), dtype=np.uint64)
    ctr[:, 0], ctr[:, 1] = np.arange(n_pix), img
    w = philox4x32_10(key, ctr)[:, :3].astype(np.int64)
    s = (w & 255) + ((w >> 8) & 255) + ((w >> 16) & 255) + ((w >> 24) & 255)
    return (s - 510).astype(np.float32) * INV_STD


def apply_photo(u8, inside, rec, img):
    """The kernel's chain on one image: u8 (H, W, 3) uint8 resampled pixels, inside (H, W) bool, rec the 16-word
    record, img the image's index in the launch -> (3, H, W) fp32 normalised output. Every product and sum is one
    np.float32 operation, in the header's order; fill pixels get the plain normalisation of 0."""
    f = np.float32
    H, W, _ = u8.shape
    m, t, sigma = rec[:9].astype(f), rec[9:12].astype(f), f(rec[12])
    seeds = rec.view(np.uint32)[13:15]
    r, g, b = (u8[..., c].astype(f) for c in range(3))
    v = []
    for c in range(3):
        v.append(((m[3 * c] * r + m[3 * c + 1] * g) + m[3 * c + 2] * b) + t[c])
    if sigma != 0:
        z = noise_z(seeds, img, H * W).reshape(H, W, 3)
        v = [v[c] + sigma * z[..., c] for c in range(3)]
    out = np.empty((3, H, W), dtype=f)
    for c in range(3):
        x = np.minimum(np.maximum(v[c], f(0)), f(255)).astype(f)
        x = np.where(inside, x, f(0)).astype(f)
        out[c] = ((x / f(255)) - MEAN[c]) / STD[c]
    assert out.dtype == f and all(a.dtype == f for a in v)
    return out


# ---- the augmentation cases of the GPU tests: n = 3 images of 24 x 40, final_dim 13 x 21 (273 pixels: one full and
# one partial 256-thread block)
SRC_HW, FINAL, N_IMG = (24, 40), (13, 21), 3
SQUARE = (13, 13)


def _aug(rd, crop0, fd, flip, rot):
    return {"resize_dims": rd, "crop": (crop0[0], crop0[1], crop0[0] + fd[1], crop0[1] + fd[0]), "flip": flip,
            "rotate": rot}


# name -> (final_dim, aug): rot_mode 0 / 1 / 2, flip on and off, resize in both passes / one / none, a crop that hangs
# outside the resized image, and one square case each for rot_mode 3 and 4
CASES = {
    "copy_noresize": (FINAL, _aug((40, 24), (10, 6), FINAL, False, 0.0)),
    "copy_flip_resize": (FINAL, _aug((32, 19), (5, 3), FINAL, True, 0.0)),
    "rot180": (FINAL, _aug((32, 19), (4, 2), FINAL, False, 180.0)),
    "rot180_flip_hpass": (FINAL, _aug((30, 24), (3, 5), FINAL, True, 180.0)),
    "affine": (FINAL, _aug((36, 21), (7, 4), FINAL, False, 5.4)),
    "affine_flip_upscale": (FINAL, _aug((52, 31), (9, 11), FINAL, True, 5.4)),
    "crop_outside": (FINAL, _aug((30, 18), (15, 10), FINAL, False, 0.0)),
    "crop_outside_affine_flip": (FINAL, _aug((30, 18), (-4, -3), FINAL, True, 5.4)),
    "square_rot90": (SQUARE, _aug((32, 19), (6, 2), SQUARE, False, 90.0)),
    "square_rot270_flip": (SQUARE, _aug((32, 19), (6, 2), SQUARE, True, 270.0)),
}


def sources(seed=0):
    return np.random.default_rng(seed).integers(0, 256, (N_IMG,) + SRC_HW + (3,), dtype=np.uint8)
