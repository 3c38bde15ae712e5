// lss_simbev.hip -- gfx950 kernels of the SimBEV input path (include/lss_simbev.h).
//
// One thread per output pixel of a camera image computes, with integer arithmetic identical to
// Pillow's, exactly the pixel the reference's PIL chain produces (src/tools.py:120-128):
//   rotate   inverse map of the output pixel through ImagingTransformAffine's 16.16 fixed-point walk
//            (nearest; outside -> 0), or ROTATE_180, or nothing;
//   flip     FLIP_LEFT_RIGHT of the cropped image;
//   crop     offset into the resized image (outside the resized image -> 0);
//   resize   Resample.c's two passes evaluated at that one pixel: for each vertical tap (source row),
//            the horizontal pass's value at that row, clipped to uint8 as Pillow's intermediate image
//            stores it, then the vertical accumulation, clipped again;
//   photo    (lss_simbev_images_photo only) colour matrix + offset, sensor noise, one clamp to [0, 255], fp32;
//   normalize ToTensor (/255) and Normalize((x - mean) / std), fp32, IEEE division.
// The horizontal values are recomputed per output row (<= ksize_v times each): a few hundred integer
// MACs per pixel, against reading a 322 KB image -- the kernel is bound by its fp32 output writes.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "lss_simbev.h"
#include "lss_device.h"

namespace {

constexpr int kPrecisionBits = 32 - 8 - 2;  // Resample.c PRECISION_BITS
constexpr int kThreads = 256;

__device__ __forceinline__ int clip8(int acc) {
    const int v = acc >> kPrecisionBits;  // arithmetic shift: floor, as Pillow's clip8 lookup
    return v < 0 ? 0 : (v > 255 ? 255 : v);
}

// Horizontal pass value of source row r at resized column xr (or the source pixel when no pass).
__device__ __forceinline__ void hpass(const uint8_t* __restrict__ img, int src_w, int r, int xr,
                                      const int32_t* __restrict__ th, int hk, int* rgb) {
    const uint8_t* row = img + (size_t)r * src_w * 3;
    if (hk == 0) {
        rgb[0] = row[3 * xr];
        rgb[1] = row[3 * xr + 1];
        rgb[2] = row[3 * xr + 2];
        return;
    }
    const int32_t* t = th + (size_t)xr * (2 + hk);
    const int xmin = t[0], cnt = t[1];
    int a0 = 1 << (kPrecisionBits - 1), a1 = a0, a2 = a0;
    for (int k = 0; k < cnt; ++k) {
        const int c = t[2 + k];
        const uint8_t* px = row + 3 * (xmin + k);
        a0 += (int)px[0] * c;
        a1 += (int)px[1] * c;
        a2 += (int)px[2] * c;
    }
    rgb[0] = clip8(a0);
    rgb[1] = clip8(a1);
    rgb[2] = clip8(a2);
}

// Photometric augmentation (ABI 36), on the pixel's integer rgb while it is in registers: the colour matrix and
// offset of the image's lss_img_photo_t, the sensor noise, one clamp, then the normalisation below. Only for a
// pixel that came from the source image ("lit": inside the rotation and inside the resized image); a fill pixel
// stays the reference's black. Every product and sum is one correctly rounded fp32 operation in the order written
// (the numpy restatement of the tests does the same roundings). The record is uniform over the block (blockIdx.y).
constexpr float kNoiseInvStd = 0.006765875f;  // (float)(1 / sqrt(4 * (256^2 - 1) / 12)): four bytes summed, variance 1

__device__ __forceinline__ int byte_sum(unsigned w) {
    return (int)((w & 255u) + ((w >> 8) & 255u) + ((w >> 16) & 255u) + (w >> 24));
}

__device__ __forceinline__ void photo_apply(const lss_img_photo_t* __restrict__ q, int pix, int img, float* v) {
    const float r = v[0], g = v[1], b = v[2];
#pragma unroll
    for (int c = 0; c < 3; ++c)
        v[c] = __fadd_rn(__fadd_rn(__fadd_rn(__fmul_rn(q->m[3 * c], r), __fmul_rn(q->m[3 * c + 1], g)),
                                   __fmul_rn(q->m[3 * c + 2], b)),
                         q->t[c]);
    const float sigma = q->noise;
    if (sigma != 0.0f) {
        const uint4 w = philox4x32(make_uint2(q->seed[0], q->seed[1]), make_uint4((unsigned)pix, (unsigned)img, 0u, 0u));
        const unsigned word[3] = {w.x, w.y, w.z};
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            const float z = __fmul_rn((float)(byte_sum(word[c]) - 510), kNoiseInvStd);
            v[c] = __fadd_rn(v[c], __fmul_rn(sigma, z));
        }
    }
#pragma unroll
    for (int c = 0; c < 3; ++c) v[c] = fminf(fmaxf(v[c], 0.0f), 255.0f);
}

// kPhoto false: lss_simbev_images, `photo` not read. true: lss_simbev_images_photo.
template <bool kPhoto>
__global__ __launch_bounds__(kThreads) void k_simbev_images(const uint8_t* __restrict__ src, int src_h, int src_w,
                                                            const lss_img_aug_t* __restrict__ augs,
                                                            const int32_t* __restrict__ tables, int out_h,
                                                            int out_w, float* __restrict__ out,
                                                            const lss_img_photo_t* __restrict__ photo) {
    const int img = blockIdx.y;
    const int pix = blockIdx.x * kThreads + threadIdx.x;
    if (pix >= out_h * out_w) return;
    const lss_img_aug_t p = augs[img];
    const int y = pix / out_w, x = pix - y * out_w;
    int rgb[3] = {0, 0, 0};
    int xs = x, ys = y;
    bool inside = true;
    [[maybe_unused]] bool lit = false;  // the pixel comes from the source image (kPhoto)
    if (p.rot_mode == 1) {  // ROTATE_180
        xs = out_w - 1 - x;
        ys = out_h - 1 - y;
    } else if (p.rot_mode == 3) {  // ROTATE_90 (square images only, as Image.rotate takes it)
        xs = out_w - 1 - y;
        ys = x;
    } else if (p.rot_mode == 4) {  // ROTATE_270
        xs = y;
        ys = out_h - 1 - x;
    } else if (p.rot_mode == 2) {
        // xx = a2 + y*a1 + x*a0 (the C loop's running int32 sums; no overflow: check_fixed)
        const long long xx = (long long)p.affine[2] + (long long)y * p.affine[1] + (long long)x * p.affine[0];
        const long long yy = (long long)p.affine[5] + (long long)y * p.affine[4] + (long long)x * p.affine[3];
        xs = (int)(xx >> 16);
        ys = (int)(yy >> 16);
        inside = xs >= 0 && xs < out_w && ys >= 0 && ys < out_h;
    }
    if (inside) {
        if (p.flip) xs = out_w - 1 - xs;
        const int xr = xs + p.crop[0], yr = ys + p.crop[1];
        if (xr >= 0 && xr < p.rs_w && yr >= 0 && yr < p.rs_h) {
            lit = true;
            const uint8_t* im = src + (size_t)img * src_h * src_w * 3;
            const int32_t* th = tables + p.h_off;
            if (p.v_ksize == 0) {
                hpass(im, src_w, yr, xr, th, p.h_ksize, rgb);
            } else {
                const int32_t* tv = tables + p.v_off + (size_t)yr * (2 + p.v_ksize);
                const int ymin = tv[0], cnt = tv[1];
                int a0 = 1 << (kPrecisionBits - 1), a1 = a0, a2 = a0;
                for (int k = 0; k < cnt; ++k) {
                    int h[3];
                    hpass(im, src_w, ymin + k, xr, th, p.h_ksize, h);
                    const int c = tv[2 + k];
                    a0 += h[0] * c;
                    a1 += h[1] * c;
                    a2 += h[2] * c;
                }
                rgb[0] = clip8(a0);
                rgb[1] = clip8(a1);
                rgb[2] = clip8(a2);
            }
        }
    }
    // ToTensor + Normalize (torchvision: float32(uint8) / 255, then (x - mean) / std, fp32)
    const float mean[3] = {0.485f, 0.456f, 0.406f};
    const float stdv[3] = {0.229f, 0.224f, 0.225f};
    float* o = out + (size_t)img * 3 * out_h * out_w + pix;
    if constexpr (kPhoto) {
        float val[3] = {(float)rgb[0], (float)rgb[1], (float)rgb[2]};
        if (lit) photo_apply(photo + img, pix, img, val);
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            const float v = __fdiv_rn(val[c], 255.0f);
            o[(size_t)c * out_h * out_w] = __fdiv_rn(__fsub_rn(v, mean[c]), stdv[c]);
        }
    } else {  // (the statements lss_simbev_images has always compiled from: its instruction stream is unchanged)
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            const float v = __fdiv_rn((float)rgb[c], 255.0f);
            o[(size_t)c * out_h * out_w] = __fdiv_rn(__fsub_rn(v, mean[c]), stdv[c]);
        }
    }
}

// flipud of the vehicle classes 1..3 of one BEV: out[b, 0, i, j] = any(bev[b, 1..3, X-1-i, j] > 0).
__global__ __launch_bounds__(kThreads) void k_vehicle_mask(const uint8_t* __restrict__ bev, int ncls, int X, int Y,
                                                           long total, float* __restrict__ out) {
    const long i = (long)blockIdx.x * kThreads + threadIdx.x;
    if (i >= total) return;
    const long XY = (long)X * Y;
    const long b = i / XY;
    const long r = i - b * XY;
    const int row = (int)(r / Y), col = (int)(r - (long)row * Y);
    const uint8_t* s = bev + (size_t)b * ncls * XY + (size_t)(X - 1 - row) * Y + col;
    const bool v = s[XY] > 0 || s[2 * XY] > 0 || s[3 * XY] > 0;
    out[i] = v ? 1.0f : 0.0f;
}

// K class groups of one BEV, flipud per group: out[b, k, i, j] = any(bev[b, c, X-1-i, j] > 0 for c in group k).
// Thread = pixel (consecutive threads along j: coalesced byte reads and fp32 writes); it reads each channel
// some group names once, as a bit of `set`, and writes its K values, one per output plane. The groups are
// bit masks over the channels, passed in the kernel arguments.
struct ClassGroups {
    uint32_t bits[LSS_SIMBEV_MAX_GROUPS];
};
__global__ __launch_bounds__(kThreads) void k_class_masks(const uint8_t* __restrict__ bev, int ncls, int X, int Y,
                                                          long total, ClassGroups groups, uint32_t used, int K,
                                                          float* __restrict__ out) {
    const long i = (long)blockIdx.x * kThreads + threadIdx.x;
    if (i >= total) return;
    const long XY = (long)X * Y;
    const long b = i / XY;
    const long r = i - b * XY;
    const int row = (int)(r / Y), col = (int)(r - (long)row * Y);
    const uint8_t* s = bev + (size_t)b * ncls * XY + (size_t)(X - 1 - row) * Y + col;
    uint32_t set = 0;
    for (int c = 0; c < ncls; ++c)
        if ((used >> c) & 1u) set |= (s[(size_t)c * XY] > 0 ? 1u : 0u) << c;
    float* o = out + (size_t)b * K * XY + r;
#pragma unroll
    for (int k = 0; k < LSS_SIMBEV_MAX_GROUPS; ++k)
        if (k < K) o[(size_t)k * XY] = (set & groups.bits[k]) ? 1.0f : 0.0f;
}

// k_class_masks under a BEV-space augmentation of the ego frame (rotation about z, isotropic scale, flips): a
// nearest-neighbour gather. Sample b's index matrix m (2 x 3, row-major) takes the centre of output cell (i, j), in
// index units, to its source position; the label is the source cell's, 0 where the position is outside the grid:
//   su = (m00*ci + m01*cj) + m02, sv = (m10*ci + m11*cj) + m12 with ci = i + 0.5, cj = j + 0.5,
//   out[b, k, i, j] = inside && any(bev[b, c, X-1-floor(su), floor(sv)] > 0 for c in group k).
// Every product and sum is one correctly rounded fp32 operation in that order (no FMA: the numpy restatement of the
// tests does the same five roundings). The range test is on the floats, before any conversion, and a NaN fails it;
// su < X then bounds floor(su) by X - 1 (X, Y <= 2^23, the entry's check: i + 0.5 and (float)X are exact).
// Thread = output cell, consecutive threads along j: coalesced writes; the reads are a rotated line of the source,
// bytes of a 40-KB plane that stays in L2.
__global__ __launch_bounds__(kThreads) void k_class_masks_warp(const uint8_t* __restrict__ bev, int ncls, int X, int Y,
                                                               long total, ClassGroups groups, uint32_t used, int K,
                                                               const float* __restrict__ mats,
                                                               float* __restrict__ out) {
    const long i = (long)blockIdx.x * kThreads + threadIdx.x;
    if (i >= total) return;
    const long XY = (long)X * Y;
    const long b = i / XY;
    const long r = i - b * XY;
    const int row = (int)(r / Y), col = (int)(r - (long)row * Y);
    const float* m = mats + 6 * b;
    const float ci = __fadd_rn((float)row, 0.5f), cj = __fadd_rn((float)col, 0.5f);
    const float su = __fadd_rn(__fadd_rn(__fmul_rn(m[0], ci), __fmul_rn(m[1], cj)), m[2]);
    const float sv = __fadd_rn(__fadd_rn(__fmul_rn(m[3], ci), __fmul_rn(m[4], cj)), m[5]);
    const bool inside = su >= 0.0f && su < (float)X && sv >= 0.0f && sv < (float)Y;
    uint32_t set = 0;
    if (inside) {
        const int si = (int)floorf(su), sj = (int)floorf(sv);
        const uint8_t* s = bev + (size_t)b * ncls * XY + (size_t)(X - 1 - si) * Y + sj;
        for (int c = 0; c < ncls; ++c)
            if ((used >> c) & 1u) set |= (s[(size_t)c * XY] > 0 ? 1u : 0u) << c;
    }
    float* o = out + (size_t)b * K * XY + r;
#pragma unroll
    for (int k = 0; k < LSS_SIMBEV_MAX_GROUPS; ++k)
        if (k < K) o[(size_t)k * XY] = (set & groups.bits[k]) ? 1.0f : 0.0f;
}

// The exclusive class map (ABI 34): k_class_masks / k_class_masks_warp (mats != NULL: the same su, sv and range test,
// operation for operation) with the K planes painted in order into one byte -- 0 where no group has a set channel,
// else 1 + the highest such group: a later group wins. Each channel some group names is read once, each byte
// written once; a cell whose source is outside the grid is 0, as the warp kernel's planes are.
__global__ __launch_bounds__(kThreads) void k_class_index(const uint8_t* __restrict__ bev, int ncls, int X, int Y,
                                                          long total, ClassGroups groups, uint32_t used, int K,
                                                          const float* __restrict__ mats, uint8_t* __restrict__ out) {
    const long i = (long)blockIdx.x * kThreads + threadIdx.x;
    if (i >= total) return;
    const long XY = (long)X * Y;
    const long b = i / XY;
    const long r = i - b * XY;
    const int row = (int)(r / Y), col = (int)(r - (long)row * Y);
    int si = row, sj = col;
    bool inside = true;
    if (mats) {
        const float* m = mats + 6 * b;
        const float ci = __fadd_rn((float)row, 0.5f), cj = __fadd_rn((float)col, 0.5f);
        const float su = __fadd_rn(__fadd_rn(__fmul_rn(m[0], ci), __fmul_rn(m[1], cj)), m[2]);
        const float sv = __fadd_rn(__fadd_rn(__fmul_rn(m[3], ci), __fmul_rn(m[4], cj)), m[5]);
        inside = su >= 0.0f && su < (float)X && sv >= 0.0f && sv < (float)Y;
        si = (int)floorf(su);
        sj = (int)floorf(sv);
    }
    uint32_t set = 0;
    if (inside) {
        const uint8_t* s = bev + (size_t)b * ncls * XY + (size_t)(X - 1 - si) * Y + sj;
        for (int c = 0; c < ncls; ++c)
            if ((used >> c) & 1u) set |= (s[(size_t)c * XY] > 0 ? 1u : 0u) << c;
    }
    int cls = 0;
#pragma unroll
    for (int k = 0; k < LSS_SIMBEV_MAX_GROUPS; ++k)
        if (k < K && (set & groups.bits[k])) cls = k + 1;
    out[i] = (uint8_t)cls;
}

// ---- Valid-cell mask: valid[b, i, j] = in the grid && seen by a camera, the layout of one class plane of the logits.
// In the grid: k_class_masks_warp's own su / sv and range test on sample b's index matrix (NULL: every cell is).
// Seen: the cell centre (x, y) = (x0 + i dx, y0 + j dy) at one of the heights z, taken back through the rig --
// get_geometry inverted: c = M p + o with M = intrins rots^-1, o = -M trans (the host's fov_cameras), depth d = c_2,
// (u', v') = (c_0, c_1) / d, (u, v) = P (u', v') + q with P, q the image augmentation's post_rots / post_trans --
// lands inside some camera's frustum: d_lo <= d < d_hi, 0 <= u <= u_max, 0 <= v <= v_max. Every product, sum and
// quotient is one correctly rounded fp32 operation in the order written (the numpy restatement of the tests does
// the same roundings); the tests are on the floats, so a NaN is unseen.
// Block = 256 cells of one sample (blockIdx.y), consecutive threads along j; the sample's N camera blocks
// (16 + 2 floats each) are copied to LDS once per block and every lane reads the same word (a broadcast). One byte
// store per cell, each byte written once.
struct FovHeights {
    float z[LSS_SIMBEV_MAX_HEIGHTS];
};
constexpr int kCamFloats = 18;  // M (9), o (3), P (4), q (2)
__global__ __launch_bounds__(kThreads) void k_valid_mask(const float* __restrict__ cams,
                                                         const float* __restrict__ post_trans, int N, int X, int Y,
                                                         float x0, float dx, float y0, float dy, FovHeights hs, int nh,
                                                         float d_lo, float d_hi, float u_max, float v_max,
                                                         const float* __restrict__ mats, int fov,
                                                         uint8_t* __restrict__ out) {
    extern __shared__ float s_cam[];
    const int b = blockIdx.y;
    if (fov) {
        const float* c = cams + (size_t)b * N * 16;
        const float* q = post_trans + (size_t)b * N * 2;
        for (int t = threadIdx.x; t < N * 16; t += kThreads) s_cam[(t >> 4) * kCamFloats + (t & 15)] = c[t];
        for (int t = threadIdx.x; t < N * 2; t += kThreads) s_cam[(t >> 1) * kCamFloats + 16 + (t & 1)] = q[t];
        __syncthreads();
    }
    const long XY = (long)X * Y;
    const long r = (long)blockIdx.x * kThreads + threadIdx.x;
    if (r >= XY) return;
    const int row = (int)(r / Y), col = (int)(r - (long)row * Y);
    bool ok = true;
    if (mats) {
        const float* m = mats + 6 * b;
        const float ci = __fadd_rn((float)row, 0.5f), cj = __fadd_rn((float)col, 0.5f);
        const float su = __fadd_rn(__fadd_rn(__fmul_rn(m[0], ci), __fmul_rn(m[1], cj)), m[2]);
        const float sv = __fadd_rn(__fadd_rn(__fmul_rn(m[3], ci), __fmul_rn(m[4], cj)), m[5]);
        ok = su >= 0.0f && su < (float)X && sv >= 0.0f && sv < (float)Y;
    }
    if (fov && ok) {
        const float x = __fadd_rn(x0, __fmul_rn((float)row, dx)), y = __fadd_rn(y0, __fmul_rn((float)col, dy));
        bool seen = false;
        for (int h = 0; h < nh && !seen; ++h) {
            const float z = hs.z[h];
            for (int n = 0; n < N && !seen; ++n) {
                const float* p = s_cam + n * kCamFloats;
                float c[3];
#pragma unroll
                for (int k = 0; k < 3; ++k)
                    c[k] = __fadd_rn(__fadd_rn(__fadd_rn(__fmul_rn(p[3 * k], x), __fmul_rn(p[3 * k + 1], y)),
                                               __fmul_rn(p[3 * k + 2], z)),
                                     p[9 + k]);
                const float d = c[2];
                const float up = __fdiv_rn(c[0], d), vp = __fdiv_rn(c[1], d);
                const float u = __fadd_rn(__fadd_rn(__fmul_rn(p[12], up), __fmul_rn(p[13], vp)), p[16]);
                const float v = __fadd_rn(__fadd_rn(__fmul_rn(p[14], up), __fmul_rn(p[15], vp)), p[17]);
                seen = d >= d_lo && d < d_hi && u >= 0.0f && u <= u_max && v >= 0.0f && v <= v_max;
            }
        }
        ok = seen;
    }
    out[(size_t)b * XY + r] = ok ? 1 : 0;
}

// ---- host: Pillow's bicubic coefficient tables (Resample.c precompute_coeffs / normalize_coeffs_8bpc)
double bicubic_filter(double x) {
    const double a = -0.5;
    if (x < 0.0) x = -x;
    if (x < 1.0) return ((a + 2.0) * x - (a + 3.0)) * x * x + 1;
    if (x < 2.0) return (((x - 5) * x + 8) * x - 4) * a;
    return 0.0;
}

// What both class-mask entries refuse, and the groups as the kernels take them (g, used = the union of the groups).
bool class_mask_args(const uint8_t* bev, int n, int n_classes, int X, int Y, const uint32_t* group_bits, int K,
                     const float* out, ClassGroups* g, uint32_t* used) {
    if (!bev || !out || !group_bits || n <= 0 || n_classes <= 0 || n_classes > 32 || X <= 0 || Y <= 0 || K <= 0 ||
        K > LSS_SIMBEV_MAX_GROUPS)
        return false;
    const uint32_t valid = n_classes == 32 ? 0xFFFFFFFFu : ((1u << n_classes) - 1u);
    for (int k = 0; k < K; ++k) {
        if (group_bits[k] == 0 || (group_bits[k] & ~valid)) return false;  // an empty group, a channel out of range
        g->bits[k] = group_bits[k];
        *used |= group_bits[k];
    }
    return true;
}

int ksize_of(int in_size, int out_size) {
    double filterscale = (double)((float)in_size - 0.0f) / out_size;  // box (0, in) as floats, as Pillow
    if (filterscale < 1.0) filterscale = 1.0;
    const double support = 2.0 * filterscale;
    return (int)ceil(support) * 2 + 1;
}

}  // namespace

extern "C" {

int lss_resample_ksize(int32_t in_size, int32_t out_size) {
    if (in_size <= 0 || out_size <= 0) return -1;
    return ksize_of(in_size, out_size);
}

int lss_resample_coeffs(int32_t in_size, int32_t out_size, int32_t* table) {
    if (in_size <= 0 || out_size <= 0 || !table) return -1;
    const float in0 = 0.0f, in1 = (float)in_size;
    const double scale = (double)(in1 - in0) / out_size;
    double filterscale = scale;
    if (filterscale < 1.0) filterscale = 1.0;
    const double support = 2.0 * filterscale;
    const int ksize = (int)ceil(support) * 2 + 1;
    double* k = new double[ksize];
    for (int xx = 0; xx < out_size; ++xx) {
        const double center = in0 + (xx + 0.5) * scale;
        double ww = 0.0;
        const double ss = 1.0 / filterscale;
        int xmin = (int)(center - support + 0.5);
        if (xmin < 0) xmin = 0;
        int xmax = (int)(center + support + 0.5);
        if (xmax > in_size) xmax = in_size;
        xmax -= xmin;
        for (int x = 0; x < xmax; ++x) {
            const double w = bicubic_filter((x + xmin - center + 0.5) * ss);
            k[x] = w;
            ww += w;
        }
        for (int x = 0; x < xmax; ++x)
            if (ww != 0.0) k[x] /= ww;
        for (int x = xmax; x < ksize; ++x) k[x] = 0.0;
        int32_t* t = table + (size_t)xx * (2 + ksize);
        t[0] = xmin;
        t[1] = xmax;
        for (int x = 0; x < ksize; ++x)
            t[2 + x] = k[x] < 0 ? (int32_t)(-0.5 + k[x] * (1 << kPrecisionBits))
                                : (int32_t)(0.5 + k[x] * (1 << kPrecisionBits));
    }
    delete[] k;
    return 0;
}

int lss_simbev_images(const uint8_t* src, int32_t n, int32_t src_h, int32_t src_w, const lss_img_aug_t* aug,
                      const int32_t* tables, int32_t out_h, int32_t out_w, float* out, void* stream) {
    if (!src || !aug || !tables || !out || n <= 0 || src_h <= 0 || src_w <= 0 || out_h <= 0 || out_w <= 0) return -1;
    if (n > 65535) return -2;
    const dim3 grid((unsigned)((out_h * out_w + kThreads - 1) / kThreads), (unsigned)n);
    hipLaunchKernelGGL(k_simbev_images<false>, grid, dim3(kThreads), 0, (hipStream_t)stream, src, src_h, src_w, aug,
                       tables, out_h, out_w, out, (const lss_img_photo_t*)nullptr);
    return launch_status();
}

int lss_simbev_images_photo(const uint8_t* src, int32_t n, int32_t src_h, int32_t src_w, const lss_img_aug_t* aug,
                            const lss_img_photo_t* photo, const int32_t* tables, int32_t out_h, int32_t out_w,
                            float* out, void* stream) {
    if (!src || !aug || !photo || !tables || !out || n <= 0 || src_h <= 0 || src_w <= 0 || out_h <= 0 || out_w <= 0)
        return -1;
    if (n > 65535) return -2;
    const dim3 grid((unsigned)((out_h * out_w + kThreads - 1) / kThreads), (unsigned)n);
    hipLaunchKernelGGL(k_simbev_images<true>, grid, dim3(kThreads), 0, (hipStream_t)stream, src, src_h, src_w, aug,
                       tables, out_h, out_w, out, photo);
    return launch_status();
}

int lss_simbev_vehicle_mask(const uint8_t* bev, int32_t n, int32_t n_classes, int32_t X, int32_t Y, float* out,
                            void* stream) {
    if (!bev || !out || n <= 0 || n_classes < 4 || X <= 0 || Y <= 0) return -1;
    const long total = (long)n * X * Y;
    hipLaunchKernelGGL(k_vehicle_mask, dim3((unsigned)((total + kThreads - 1) / kThreads)), dim3(kThreads), 0,
                       (hipStream_t)stream, bev, n_classes, X, Y, total, out);
    return launch_status();
}

int lss_simbev_class_masks(const uint8_t* bev, int32_t n, int32_t n_classes, int32_t X, int32_t Y,
                           const uint32_t* group_bits, int32_t K, float* out, void* stream) {
    ClassGroups g{};
    uint32_t used = 0;
    if (!class_mask_args(bev, n, n_classes, X, Y, group_bits, K, out, &g, &used)) return -1;
    const long total = (long)n * X * Y;
    hipLaunchKernelGGL(k_class_masks, dim3((unsigned)((total + kThreads - 1) / kThreads)), dim3(kThreads), 0,
                       (hipStream_t)stream, bev, n_classes, X, Y, total, g, used, K, out);
    return launch_status();
}

int lss_simbev_class_masks_warp(const uint8_t* bev, int32_t n, int32_t n_classes, int32_t X, int32_t Y,
                                const uint32_t* group_bits, int32_t K, const float* index_mats, float* out,
                                void* stream) {
    ClassGroups g{};
    uint32_t used = 0;
    if (!class_mask_args(bev, n, n_classes, X, Y, group_bits, K, out, &g, &used) || !index_mats) return -1;
    if (X > (1 << 23) || Y > (1 << 23)) return -1;  // i + 0.5 and (float)X exact: the range test bounds the gather
    const long total = (long)n * X * Y;
    hipLaunchKernelGGL(k_class_masks_warp, dim3((unsigned)((total + kThreads - 1) / kThreads)), dim3(kThreads), 0,
                       (hipStream_t)stream, bev, n_classes, X, Y, total, g, used, K, index_mats, out);
    return launch_status();
}

int lss_simbev_class_index(const uint8_t* bev, int32_t n, int32_t n_classes, int32_t X, int32_t Y,
                           const uint32_t* group_bits, int32_t K, const float* index_mats, uint8_t* out, void* stream) {
    ClassGroups g{};
    uint32_t used = 0;
    if (K > LSS_SIMBEV_MAX_EXCLUSIVE_GROUPS ||
        !class_mask_args(bev, n, n_classes, X, Y, group_bits, K, reinterpret_cast<const float*>(out), &g, &used))
        return -1;
    if (X > (1 << 23) || Y > (1 << 23) || (reinterpret_cast<uintptr_t>(index_mats) & 3)) return -1;
    const long total = (long)n * X * Y;
    if ((total + kThreads - 1) / kThreads > 0x7FFFFFFFL) return -1;
    hipLaunchKernelGGL(k_class_index, dim3((unsigned)((total + kThreads - 1) / kThreads)), dim3(kThreads), 0,
                       (hipStream_t)stream, bev, n_classes, X, Y, total, g, used, K, index_mats, out);
    return launch_status();
}

int lss_simbev_valid_mask(const float* cams, const float* post_trans, int32_t n, int32_t N, int32_t X, int32_t Y,
                          float x0, float dx, float y0, float dy, const float* heights, int32_t n_heights, float d_lo,
                          float d_hi, int32_t fH, int32_t fW, const float* index_mats, int32_t mode, uint8_t* out,
                          void* stream) {
    if (!out || n <= 0 || n > 65535 || X <= 0 || Y <= 0 || X > (1 << 23) || Y > (1 << 23)) return -1;
    if (mode != LSS_SIMBEV_VALID_GRID && mode != LSS_SIMBEV_VALID_FOV) return -1;
    if (n_heights > LSS_SIMBEV_MAX_HEIGHTS || !(d_lo > 0.0f) || !(d_hi > d_lo)) return -1;  // (a NaN bound too)
    const int fov = mode == LSS_SIMBEV_VALID_FOV;
    FovHeights hs{};
    if (fov) {
        if (!cams || !post_trans || !heights || N < 1 || N > LSS_SIMBEV_MAX_CAMERAS || n_heights < 1 || fH < 1 ||
            fW < 1)
            return -1;
        for (int h = 0; h < n_heights; ++h) hs.z[h] = heights[h];
    }
    const long XY = (long)X * Y;
    const long bps = (XY + kThreads - 1) / kThreads;
    if (bps > 0x7FFFFFFFL) return -1;
    const size_t lds = fov ? (size_t)N * kCamFloats * sizeof(float) : 0;
    hipLaunchKernelGGL(k_valid_mask, dim3((unsigned)bps, (unsigned)n), dim3(kThreads), lds, (hipStream_t)stream, cams,
                       post_trans, fov ? N : 0, X, Y, x0, dx, y0, dy, hs, fov ? n_heights : 0, d_lo, d_hi,
                       (float)(fW - 1), (float)(fH - 1), index_mats, fov, out);
    return launch_status();
}

}  // extern "C"
