/*
 * lss_simbev.h -- C ABI of the SimBEV input path on MI355X (gfx950): per-camera image augmentation
 * and BEV label decoding on the device.
 *
 * Replaces, per camera, the pixel work of the reference's loader (shdragron/LSS-Carla):
 *   img_transform(img, ...)   src/tools.py:120-128   Image.resize -> crop -> FLIP_LEFT_RIGHT -> rotate
 *   normalize_img(img)        src/tools.py:167-171   ToTensor + Normalize(ImageNet mean / std)
 *   get_binimg(sample)        src/data_simbev.py:220-246   (bev[1] | bev[2] | bev[3]) > 0, np.flipud
 * bit for bit with Pillow's published algorithms (libImaging/Resample.c bicubic fixed-point resample,
 * libImaging/Geometry.c 16.16 fixed-point nearest affine) and torchvision's fp32 normalisation. JPEG
 * decoding and the augmentation draws (np.random, src/data_simbev.py:119-145) stay on the host.
 * Conventions as lss_hip.h: device pointers, asynchronous on `stream`, 0 = success, negative LSS_E*
 * codes for bad arguments, positive hipError_t for launch failures.
 */
#ifndef LSS_SIMBEV_H
#define LSS_SIMBEV_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* One camera image's augmentation (sample_augmentation's draws, src/data_simbev.py:119-145). */
typedef struct lss_img_aug {
    int32_t src_h, src_w;          /* decoded image (H, W), 3 channels, uint8 HWC */
    int32_t rs_w, rs_h;            /* resize_dims (W', H') of Image.resize */
    int32_t crop[4];               /* PIL crop box (x0, y0, x1, y1) in the resized image; outside -> 0 */
    int32_t flip;                  /* FLIP_LEFT_RIGHT after the crop */
    int32_t rot_mode;              /* 0: rotate % 360 == 0 (copy), 1: ROTATE_180, 2: affine nearest,
                                      3 / 4: ROTATE_90 / ROTATE_270 (square images, 90 / 270 degrees) */
    int32_t affine[6];             /* rot_mode 2: a0..a5 of ImagingTransformAffine's fixed-point walk */
    int32_t h_off, h_ksize;        /* horizontal pass: table offset (in int32) and taps; h_ksize 0 = no pass */
    int32_t v_off, v_ksize;        /* vertical pass, likewise */
} lss_img_aug_t;

/* Pillow's precompute_coeffs + normalize_coeffs_8bpc for one pass of Image.resize (BICUBIC):
 * out_size rows of (xmin, count, k_0 .. k_{ksize-1}) int32, written to `table` (host memory,
 * out_size * (2 + ksize) ints, ksize from lss_resample_ksize). Host-only, no device work. */
int lss_resample_ksize(int32_t in_size, int32_t out_size);
int lss_resample_coeffs(int32_t in_size, int32_t out_size, int32_t* table);

/* n images (src: n * src_h * src_w * 3 uint8, every image the same size) -> out (n, 3, out_h, out_w)
 * fp32 = normalize_img(img_transform(img)) with the per-image parameters aug[n] and the coefficient
 * tables (device memory) they point into. out_h / out_w = the crop size (final_dim). */
int lss_simbev_images(const uint8_t* src, int32_t n, int32_t src_h, int32_t src_w, const lss_img_aug_t* aug,
                      const int32_t* tables, int32_t out_h, int32_t out_w, float* out, void* stream);

/* (ABI 36) One camera image's photometric augmentation: colour jitter as an affine map of (R, G, B) and sensor
 * noise. 64 bytes, one per image, parallel to lss_img_aug_t[n]. */
typedef struct lss_img_photo {
    float    m[9];                 /* row-major 3x3 colour matrix on (R, G, B) in 0..255 units */
    float    t[3];                 /* offset, same units */
    float    noise;                /* noise amplitude sigma, 0..255 units; 0 = none (no RNG work) */
    uint32_t seed[2];              /* Philox key of this image's noise */
    uint32_t pad;
} lss_img_photo_t;

/* lss_simbev_images with the photometric augmentation photo[n] (DEVICE memory) applied to the resampled integer
 * (r, g, b) of each output pixel, before the normalisation. A pixel is "inside" when it passed the rotation's
 * inside test and the crop-inside-the-resized-image test; a fill pixel stays the reference's black (the
 * normalisation of 0), bit for bit as lss_simbev_images writes it. For an inside pixel pix = y * out_w + x of
 * image img, every product and sum one correctly rounded fp32 operation in this order (no FMA):
 *   v[c] = ((m[3c] r + m[3c+1] g) + m[3c+2] b) + t[c]
 *   if noise != 0:  w = philox4x32_10(key = seed, counter = (pix, img, 0, 0)); s_c = the sum of the four bytes of
 *                   word c of w (0..1020); z_c = (float)(s_c - 510) * 0.006765875f (Irwin-Hall, n = 4: mean 0,
 *                   variance 1, |z| <= 3.46); v[c] = v[c] + noise * z_c
 *   v[c] = fminf(fmaxf(v[c], 0), 255)                       the one clamp
 *   out = ((v[c] / 255) - mean[c]) / std[c]                 as lss_simbev_images
 * The neutral record (m = I, t = 0, noise = 0) gives lss_simbev_images' output bit for bit. Same checks and codes
 * as lss_simbev_images (-1 bad argument, -2 n > 65535), and -1 for a NULL photo. */
int lss_simbev_images_photo(const uint8_t* src, int32_t n, int32_t src_h, int32_t src_w, const lss_img_aug_t* aug,
                            const lss_img_photo_t* photo, const int32_t* tables, int32_t out_h, int32_t out_w,
                            float* out, void* stream);

/* BEV labels: bev (n, n_classes, X, Y) uint8 (any value > 0 = set) -> out (n, 1, X, Y) fp32 =
 * flipud((bev[1] > 0) | (bev[2] > 0) | (bev[3] > 0)). n_classes >= 4. */
int lss_simbev_vehicle_mask(const uint8_t* bev, int32_t n, int32_t n_classes, int32_t X, int32_t Y, float* out,
                            void* stream);

/* (ABI 25) BEV labels by class group, for a multi-class head: out (n, K, X, Y) fp32, NCHW contiguous,
 *   out[b, k, i, j] = any over the channels c of group k of (bev[b, c, X-1-i, j] > 0)
 * -- get_binimg's merge and np.flipud, applied per group. group_bits: K bit masks over the npz channels in
 * HOST memory (bit c = channel c), read here and passed to the kernel by value (no device allocation);
 * 1 <= K <= LSS_SIMBEV_MAX_GROUPS, n_classes <= 32, every mask non-zero and within n_classes, else -1.
 * One launch, coalesced along j; a pixel reads each channel some group names once, for all K groups.
 * K = 1, group_bits = {0xE} gives lss_simbev_vehicle_mask's output. */
#define LSS_SIMBEV_MAX_GROUPS 8
int lss_simbev_class_masks(const uint8_t* bev, int32_t n, int32_t n_classes, int32_t X, int32_t Y,
                           const uint32_t* group_bits, int32_t K, float* out, void* stream);

/* (ABI 31) lss_simbev_class_masks under a BEV-space augmentation of the ego frame -- one rotation about z, one
 * isotropic scale, flips of x and y, p' = A p -- applied to the labels as a nearest-neighbour gather in the same
 * pass. index_mats: n x 6 fp32 in DEVICE memory, sample b's row-major 2 x 3 affine map from the centre of an
 * output cell in index units, (i + 0.5, j + 0.5), to the source position in index units (for a grid of cell
 * D = diag(dx, dy) and lower corner lo: M = D^-1 A2^-1 D, b = D^-1 (A2^-1 lo - lo), A2 the xy block of A). Row i of
 * a label is x cell i, column j is y cell j, as the model's logits. With ci = i + 0.5f, cj = j + 0.5f:
 *   su = (m00*ci + m01*cj) + m02;  sv = (m10*ci + m11*cj) + m12       each product and sum rounded once, fp32
 *   inside = su >= 0 && su < X && sv >= 0 && sv < Y                   tested on the floats; a NaN is outside
 *   out[b, k, i, j] = inside && any over c of group k of (bev[b, c, X-1-floor(su), floor(sv)] > 0)
 * -- the X-1-. is lss_simbev_class_masks' flipud. A cell whose source falls outside the grid is 0: no camera point
 * lands there (the corners past the grid under rotation, the ring past s times its half width). Every output
 * element is written exactly once. The identity {1, 0, 0, 0, 1, 0} gives lss_simbev_class_masks' output bit for bit.
 * -1 for what lss_simbev_class_masks refuses, for a NULL index_mats and for X or Y above 2^23 (i + 0.5 exact). */
int lss_simbev_class_masks_warp(const uint8_t* bev, int32_t n, int32_t n_classes, int32_t X, int32_t Y,
                                const uint32_t* group_bits, int32_t K, const float* index_mats, float* out,
                                void* stream);

/* (ABI 34) The exclusive class map of K label groups (1 <= K <= LSS_SIMBEV_MAX_EXCLUSIVE_GROUPS, so C = K + 1 <= 8
 * classes fit the K-channel head): out (n, X, Y) uint8, row i = x cell i, column j = y cell j,
 *   out[b, i, j] = 0 if no group has a set channel at bev[b, ., X-1-i, j], else 1 + the highest such group index
 * -- class 0 is the background, class k + 1 is group k, and the groups are painted in order: a later group wins over an
 * earlier one. Equal, bit for bit, to that rule applied to lss_simbev_class_masks' K planes. group_bits: HOST bit masks
 * passed by value, exactly as lss_simbev_class_masks takes them. index_mats: NULL, or n x 6 fp32 in DEVICE memory --
 * then the source cell is lss_simbev_class_masks_warp's su / sv and inside test, operation for operation, and a cell
 * whose source falls outside the grid is 0 (that entry's convention; lss_simbev_valid_mask's grid mode is what makes
 * a loss ignore those cells). The identity gives the un-warped map. One launch, thread = pixel along j; each channel
 * some group names is read once, every byte written exactly once. -1 without launching for what
 * lss_simbev_class_masks refuses, K > 7, X or Y above 2^23, n * X * Y past the grid limit, a misaligned index_mats. */
#define LSS_SIMBEV_MAX_EXCLUSIVE_GROUPS 7
int lss_simbev_class_index(const uint8_t* bev, int32_t n, int32_t n_classes, int32_t X, int32_t Y,
                           const uint32_t* group_bits, int32_t K, const float* index_mats, uint8_t* out, void* stream);

/* (ABI 32) Valid-cell mask for the losses and metrics: out (n, X, Y) uint8, row i = x cell i, column j = y cell j
 * (one class plane of the logits); out[b, i, j] = 1 iff cell (i, j) of sample b is in the grid and, in FOV mode,
 * seen by at least one of the sample's N cameras.
 *   in the grid  index_mats NULL: always. Otherwise (n x 6 fp32, DEVICE memory) lss_simbev_class_masks_warp's own
 *                su, sv and test 0 <= su < X, 0 <= sv < Y: the mask is 0 exactly where that entry writes its
 *                out-of-grid 0.
 *   seen         the cell centre x = x0 + i dx, y = y0 + j dy (x0, y0: the first cell's centre) at a height z of
 *                `heights` (n_heights <= LSS_SIMBEV_MAX_HEIGHTS floats in HOST memory, passed by value), through
 *                camera n's block of `cams` (n x N x 16 fp32, DEVICE: M = intrins rots^-1 row-major (9), o = -M trans
 *                (3), P = post_rots[:2, :2] row-major (4)) and of `post_trans` (n x N x 2 fp32, DEVICE: q):
 *                  c_r = ((m_r0 x + m_r1 y) + m_r2 z) + o_r,  d = c_2,  u' = c_0 / d,  v' = c_1 / d,
 *                  u = (p00 u' + p01 v') + q0,  v = (p10 u' + p11 v') + q1
 *                every product, sum and quotient rounded once to fp32 in that order; seen iff, on the floats (a NaN
 *                fails), d_lo <= d < d_hi, 0 <= u <= fW - 1, 0 <= v <= fH - 1 for some height and camera -- the
 *                frustum of create_frustum (dbound, final_dim), get_geometry inverted, so it holds for a rig
 *                composed with the BEV-space augmentation as it is.
 * mode: LSS_SIMBEV_VALID_GRID (the first test only; cams, post_trans, heights may be NULL) or LSS_SIMBEV_VALID_FOV.
 * One launch, one thread per cell, a block inside one sample, the camera blocks in LDS; every byte written exactly
 * once, no atomics, no workspace. -1 without launching for: NULL out, n outside 1..65535, X or Y outside 1..2^23,
 * another mode, n_heights > 8, d_lo <= 0 or d_hi <= d_lo; in FOV mode also NULL cams / post_trans / heights,
 * N outside 1..LSS_SIMBEV_MAX_CAMERAS, n_heights < 1, fH or fW < 1. */
#define LSS_SIMBEV_MAX_HEIGHTS 8
#define LSS_SIMBEV_MAX_CAMERAS 256
#define LSS_SIMBEV_VALID_GRID 0
#define LSS_SIMBEV_VALID_FOV 1
int lss_simbev_valid_mask(const float* cams, const float* post_trans, int32_t n, int32_t N, int32_t X, int32_t Y,
                          float x0, float dx, float y0, float dy, const float* heights, int32_t n_heights, float d_lo,
                          float d_hi, int32_t fH, int32_t fW, const float* index_mats, int32_t mode, uint8_t* out,
                          void* stream);

#ifdef __cplusplus
}
#endif
#endif /* LSS_SIMBEV_H */
