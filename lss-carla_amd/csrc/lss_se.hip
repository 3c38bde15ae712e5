// lss_se.hip -- squeeze-and-excitation of the EfficientNet-B0 MBConv blocks (efficientnet_pytorch
// MBConvBlock: x * sigmoid(se_expand(swish(se_reduce(avg_pool(x))))), used by CamEncode's trunk,
// src/models.py:43, 63-84), NCHW bf16 activations as the trunk runs under bf16 autocast.
//
// PyTorch runs it as ~7 forward and ~20 backward launches per block (pooling, two 1x1 convs on
// 1x1 maps with MIOpen's set/cast kernels, swish, sigmoid, the broadcast multiply, its two-sided
// backward with a materialised g*x, the pooling backward and a gradient add). Here, five launches where the
// MLP tails pay (se_tails: the narrow blocks of the trunk), nine (the fallback sequence below) elsewhere:
//   forward   k_se_mean_tail (one wave per (n, c) plane; the LAST block of an image to finish also
//             runs both 1x1 convs, swish and sigmoid for that image; values rounded to bf16 where
//             autocast rounds them) -> k_se_scale (y = x * sig)
//   backward  k_se_dot_tail (t = sum_hw g*x per plane; the last block of an image also runs the
//             sigmoid, expand, swish and reduce backward -> de, dr, dm) -> k_se_dx
//             (dx = g*sig + dm/HW); k_se_wgrad: the four weight / bias gradients in one launch.
// All sums fp32 in a fixed order (deterministic).
//
// The per-image tails. The MLPs work on a few KB per image and were four launches of their own
// (k_se_mlp1 / k_se_mlp2 / k_se_mlpb1 / k_se_mlpb2) at the ~5 us floor of a launch in the replayed
// graph. They now ride in the reductions that feed them, with the hand-off of the depthwise
// weight-gradient fold (dw_finish, lss_dwconv.hip) and of the batch-norm clusters (lss_bnorm.hip):
//   * a block holds planes of ONE image (grid N x bpi, se_tail_grid); it publishes its m (or t) values with
//     agent-scope write-through stores, every storing wave retires them (vmcnt(0)), the block meets at
//     a barrier, and one lane draws a ticket on the image's counter (relaxed agent-scope fetch_add);
//   * the block that draws the last ticket re-zeroes the counter and computes the image's MLP, reading
//     the published values with agent-scope loads (the 8 XCDs share no L2, and a CU's L1 is never
//     refreshed by other CUs' stores). Nothing waits on anything: no spin, no co-residency needed.
//   * the arithmetic and its association are those of the four MLP kernels, which stay below as the
//     fallback launch sequence: both paths call the same __device__ bodies (se_fc1_dots, se_fc2,
//     se_de, se_dh16, se_dr, se_dm_range), so their results are equal bit for bit.
// Counters: kSeBanks banks of kSeBankImages words in the code object (zero at load, left zero by every
// call); a call takes the next bank round-robin. That only reduces the hazard of two calls in flight
// at once on two streams of one device, it does not remove it: the supported use is one stream per
// device (as for the batch-norm sync workspace). N > kSeBankImages, lss_se_tails(0), or a shape the static
// rule of se_tails sends there, takes the fallback sequence (nine launches per block).

#include <hip/hip_runtime.h>
#include <limits.h>
#include <math.h>
#include <stdint.h>

#include <algorithm>
#include <atomic>

#include "lss_convs.h"
#include "lss_device.h"

// The library is built with -ffp-contract=off for the geometry's reference op order (lss_hip.hip);
// the conv-stack kernels here have no bit-exact contract, so they keep FMA contraction.
#pragma clang fp contract(fast)

#ifndef LSS_SE_TAILS_DEFAULT
#define LSS_SE_TAILS_DEFAULT 1  // 0: a tuning build that starts on the fallback sequence (A/B timing)
#endif

namespace {

constexpr int kBlock = 256;
constexpr int kMaxC = 2048;  // channels of the widest MBConv block: 1152

__device__ __forceinline__ float bf(unsigned short b) { return __uint_as_float((unsigned)b << 16); }
__device__ __forceinline__ float rbf(float x) { return bf(bf16_bits_select(x)); }  // round through bf16

// Uses a loaded value where it stands. Without it the compiler sinks each load of an unrolled batch into the
// branch that consumes it, and the batch becomes one memory round trip per element.
__device__ __forceinline__ void pin(float& v) { asm volatile("" : "+v"(v)); }

// 4 consecutive bf16 (8 bytes) <-> fp32
__device__ __forceinline__ void ld4(const unsigned short* p, float* o) { unpack4(*reinterpret_cast<const uint2*>(p), o); }
__device__ __forceinline__ void st4(unsigned short* p, const float* v) {
    uint2 u;
    u.x = (unsigned)bf16_bits_select(v[0]) | ((unsigned)bf16_bits_select(v[1]) << 16);
    u.y = (unsigned)bf16_bits_select(v[2]) | ((unsigned)bf16_bits_select(v[3]) << 16);
    *reinterpret_cast<uint2*>(p) = u;
}

// ---- the arithmetic both launch sequences share ------------------------------------------------------
// Contraction is off inside these bodies and every fused multiply-add is written out, so the tails and
// the fallback kernels round alike whatever the compiler would make of either context.

// one wave, one (n, c) plane of HW elements (HW % 4 == 0): mean, rounded to bf16 (the pooled map's type)
__device__ __forceinline__ float se_plane_mean(const unsigned short* xp, int HW, int lane) {
#pragma clang fp contract(off)
    float s = 0.f;
    for (int i = lane * 4; i < HW; i += kWave * 4) {
        float v[4];
        ld4(xp + i, v);
        s += (v[0] + v[1]) + (v[2] + v[3]);
    }
    s = wave_sum(s);
    return rbf(s / (float)HW);
}

// one wave, one plane: sum_hw g * x (fp32)
__device__ __forceinline__ float se_plane_dot(const unsigned short* gp, const unsigned short* xp, int HW, int lane) {
    float s = 0.f;
    for (int i = lane * 4; i < HW; i += kWave * 4) {
        float a[4], b[4];
        ld4(gp + i, a);
        ld4(xp + i, b);
#pragma unroll
        for (int k = 0; k < 4; ++k) s = fmaf(a[k], b[k], s);
    }
    return wave_sum(s);
}

// The same for up to P planes of one wave at once (plane p at xp + p * pstride, np <= P of them live): each
// plane's sum is the one above, element for element; only the planes' loads are issued together. A plane
// past the last re-reads the last one, its sum unused.
template <int P>
__device__ __forceinline__ void se_planes_mean(const unsigned short* xp, size_t pstride, int np, int HW, int lane,
                                               float (&out)[P]) {
#pragma clang fp contract(off)
    float s[P];
    const unsigned short* pp[P];
#pragma unroll
    for (int p = 0; p < P; ++p) {
        s[p] = 0.f;
        pp[p] = xp + (size_t)min(p, np - 1) * pstride;
    }
    for (int i = lane * 4; i < HW; i += kWave * 4) {
        float v[P][4];
#pragma unroll
        for (int p = 0; p < P; ++p) ld4(pp[p] + i, v[p]);
#pragma unroll
        for (int p = 0; p < P; ++p) s[p] += (v[p][0] + v[p][1]) + (v[p][2] + v[p][3]);
    }
#pragma unroll
    for (int p = 0; p < P; ++p) out[p] = rbf(wave_sum(s[p]) / (float)HW);
}
template <int P>
__device__ __forceinline__ void se_planes_dot(const unsigned short* gp, const unsigned short* xp, size_t pstride,
                                              int np, int HW, int lane, float (&out)[P]) {
    float s[P];
    size_t off[P];
#pragma unroll
    for (int p = 0; p < P; ++p) {
        s[p] = 0.f;
        off[p] = (size_t)min(p, np - 1) * pstride;
    }
    for (int i = lane * 4; i < HW; i += kWave * 4) {
        uint2 ga[P], xa[P];  // kept packed until used: 4 P registers, not 8 P
#pragma unroll
        for (int p = 0; p < P; ++p) {
            ga[p] = *reinterpret_cast<const uint2*>(gp + off[p] + i);
            xa[p] = *reinterpret_cast<const uint2*>(xp + off[p] + i);
        }
#pragma unroll
        for (int p = 0; p < P; ++p) {
            float a[4], b[4];
            unpack4(ga[p], a);
            unpack4(xa[p], b);
#pragma unroll
            for (int k = 0; k < 4; ++k) s[p] = fmaf(a[k], b[k], s[p]);
        }
    }
#pragma unroll
    for (int p = 0; p < P; ++p) out[p] = wave_sum(s[p]);
}

// Reduce conv, one wave: out[u] = sum_c bf16(W1[j_u][c]) m[c] for the rows j_u = j0 + u * jstride < sq
// (u < JB), lanes over C, four independent partial sums per row; the JB rows' loads are issued together.
// mn: the image's pooled means (global or LDS).
template <int JB>
__device__ __forceinline__ void se_fc1_dots(const float* __restrict__ w1, const float* mn, int C, int sq, int j0,
                                            int jstride, int lane, float (&out)[JB]) {
#pragma clang fp contract(off)
    float a[JB][4];
    const float* wr[JB];
#pragma unroll
    for (int u = 0; u < JB; ++u) {
        const int j = j0 + u * jstride;
        wr[u] = w1 + (size_t)(j < sq ? j : 0) * C;  // a row past the last: row 0 again, its sum unused
#pragma unroll
        for (int k = 0; k < 4; ++k) a[u][k] = 0.f;
    }
    int c = lane;
    for (; c + 3 * kWave < C; c += 4 * kWave) {
        float wv[JB][4];
#pragma unroll
        for (int u = 0; u < JB; ++u)
#pragma unroll
            for (int k = 0; k < 4; ++k) wv[u][k] = wr[u][c + k * kWave];
#pragma unroll
        for (int u = 0; u < JB; ++u)
#pragma unroll
            for (int k = 0; k < 4; ++k) a[u][k] = fmaf(rbf(wv[u][k]), mn[c + k * kWave], a[u][k]);
    }
    for (; c < C; c += kWave) {
        float wv[JB];
#pragma unroll
        for (int u = 0; u < JB; ++u) wv[u] = wr[u][c];
#pragma unroll
        for (int u = 0; u < JB; ++u) a[u][0] = fmaf(rbf(wv[u]), mn[c], a[u][0]);
    }
#pragma unroll
    for (int u = 0; u < JB; ++u) out[u] = wave_sum((a[u][0] + a[u][1]) + (a[u][2] + a[u][3]));
}
// r = bf16(W1 m + b1), h = bf16(swish(r))
__device__ __forceinline__ void se_fc1_finish(float a, float b1j, float& r, float& h) {
#pragma clang fp contract(off)
    r = rbf(a + rbf(b1j));
    h = rbf(r * sigmoid(r));
}

// Expand conv, one thread per channel: wr = the channel's row of W2 (LDS, rounded to bf16), the sq
// products summed in order: e = bf16(W2 h + b2), sig = bf16(sigmoid(e))
__device__ __forceinline__ float se_fc2(const float* wr, const float* s_h, int sq, float b2c) {
#pragma clang fp contract(off)
    float e = 0.f;
#pragma unroll 4
    for (int j = 0; j < sq; ++j) e = fmaf(wr[j], s_h[j], e);
    e = rbf(e + rbf(b2c));
    return rbf(sigmoid(e));
}

// de = t sig (1 - sig)
__device__ __forceinline__ float se_de(float t, float s) {
#pragma clang fp contract(off)
    return t * s * (1.f - s);
}

constexpr int kMlpC = 256;  // channels per k_se_mlp2 block
constexpr int kMlpbC = 64;  // channels per chunk of the MLP backward (16 per wave: short dependent chains)
constexpr int kPer = kMlpbC / (kBlock / kWave);  // 16
constexpr int kMaxSq = kWave;

// Partial dh of the 16 channels ca0 .. ca0 + 15 (those < C), lane = j (a row element of W2 (C, sq)):
// sum_i bf16(W2[ca0 + i][j]) de16[i], in sequence; de16: the channels' de (LDS)
__device__ __forceinline__ float se_dh16(const float* __restrict__ w2, const float* de16, int ca0, int C, int sq,
                                         int lane) {
#pragma clang fp contract(off)
    float a[kPer], w[kPer];
    // the loads are unconditional (clamped, valid addresses; C * sq < 2^17) and all issued before the first use
#pragma unroll
    for (int i = 0; i < kPer; ++i) w[i] = w2[min(ca0 + i, C - 1) * sq + min(lane, sq - 1)];
#pragma unroll
    for (int i = 0; i < kPer; ++i) pin(w[i]);
#pragma unroll
    for (int i = 0; i < kPer; ++i) a[i] = (lane < sq && ca0 + i < C) ? rbf(w[i]) * de16[i] : 0.f;
    float sum = 0.f;
#pragma unroll
    for (int i = 0; i < kPer; ++i) sum += a[i];
    return sum;
}

// dr = dh swish'(r)
__device__ __forceinline__ float se_dr(float dh, float rv) {
#pragma clang fp contract(off)
    const float s = sigmoid(rv);
    return dh * s * fmaf(rv, 1.f - s, 1.f);
}

// One j-range [j0, j1) (at most 16 rows: sq <= 64 in four ranges) of dm[c] = sum_j bf16(W1[j][c]) dr[j],
// in sequence; the range's loads are issued together. c >= C: the value is not used.
__device__ __forceinline__ float se_dm_range(const float* __restrict__ w1, const float* s_dr, int C, int sq, int c,
                                             int j0, int j1) {
#pragma clang fp contract(off)
    float w[kMaxSq / 4];
#pragma unroll
    for (int u = 0; u < kMaxSq / 4; ++u) w[u] = w1[min(j0 + u, sq - 1) * C + min(c, C - 1)];  // clamped, not skipped
#pragma unroll
    for (int u = 0; u < kMaxSq / 4; ++u) pin(w[u]);
    float a = 0.f;
#pragma unroll
    for (int u = 0; u < kMaxSq / 4; ++u) {
        const float f = fmaf(rbf(w[u]), s_dr[min(j0 + u, sq - 1)], a);
        a = j0 + u < j1 ? f : a;
    }
    return a;
}

__device__ __forceinline__ float sum4(float s0, float s1, float s2, float s3) {
#pragma clang fp contract(off)
    return (s0 + s1) + (s2 + s3);
}

// ---- the fallback launch sequence: one kernel per stage ----------------------------------------------

__global__ __launch_bounds__(kBlock) void k_se_mean(const unsigned short* __restrict__ x, int planes, int HW,
                                                    float* __restrict__ m) {
    const int pl = blockIdx.x * (kBlock / kWave) + (int)(threadIdx.x >> 6);
    if (pl >= planes) return;
    const int lane = threadIdx.x & 63;
    const float v = se_plane_mean(x + (size_t)pl * HW, HW, lane);
    if (lane == 0) m[pl] = v;
}

// The two 1x1 convs on the pooled (N, C) map, split so that every weight read is coalesced:
//   k_se_mlp1: one wave per (image, output j), lanes over C (rows of W1 (sq, C)):
//              r = bf16(W1 m + b1), h = bf16(swish(r))
//   k_se_mlp2: one block per (image, 256 channels), the block's rows of W2 (C, sq) staged in LDS:
//              e = bf16(W2 h + b2), sig = bf16(sigmoid(e))
// Weights are fp32 masters, used rounded to bf16 as the autocast conv uses them.
__global__ __launch_bounds__(kBlock) void k_se_mlp1(const float* __restrict__ m, const float* __restrict__ w1,
                                                    const float* __restrict__ b1, int C, int sq,
                                                    float* __restrict__ r_out, float* __restrict__ h_out) {
    const int wpi = (sq + 3) / 4;  // blocks per image
    const int n = blockIdx.x / wpi, j = (blockIdx.x % wpi) * 4 + (int)(threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    if (j >= sq) return;
    float a[1];
    se_fc1_dots<1>(w1, m + (size_t)n * C, C, sq, j, 1, lane, a);
    if (lane == 0) {
        float r, h;
        se_fc1_finish(a[0], b1[j], r, h);
        r_out[(size_t)n * sq + j] = r;
        h_out[(size_t)n * sq + j] = h;
    }
}

__global__ __launch_bounds__(kBlock) void k_se_mlp2(const float* __restrict__ h, const float* __restrict__ w2,
                                                    const float* __restrict__ b2, int C, int sq,
                                                    float* __restrict__ sig) {
    __shared__ float s_w[kMlpC * (kMaxSq + 1)];  // rows of W2, padded
    __shared__ float s_h[kMaxSq];
    const int nchunk = (C + kMlpC - 1) / kMlpC;
    const int n = blockIdx.x / nchunk, c0 = (blockIdx.x % nchunk) * kMlpC;
    const int nc = min(kMlpC, C - c0);
    for (int i = threadIdx.x; i < nc * sq; i += kBlock) {
        const int cl = i / sq, j = i - cl * sq;
        s_w[cl * (sq + 1) + j] = rbf(w2[(size_t)c0 * sq + i]);
    }
    if ((int)threadIdx.x < sq) s_h[threadIdx.x] = h[(size_t)n * sq + threadIdx.x];
    __syncthreads();
    if ((int)threadIdx.x < nc) {
        const int c = c0 + threadIdx.x;
        sig[(size_t)n * C + c] = se_fc2(s_w + threadIdx.x * (sq + 1), s_h, sq, b2[c]);
    }
}

__global__ __launch_bounds__(kBlock) void k_se_dot(const unsigned short* __restrict__ g,
                                                   const unsigned short* __restrict__ x, int planes, int HW,
                                                   float* __restrict__ t) {
    const int pl = blockIdx.x * (kBlock / kWave) + (int)(threadIdx.x >> 6);
    if (pl >= planes) return;
    const int lane = threadIdx.x & 63;
    const size_t off = (size_t)pl * HW;
    const float s = se_plane_dot(g + off, x + off, HW, lane);
    if (lane == 0) t[pl] = s;
}

// MLP backward, coalesced like the forward, one block per (image, 64 channels):
//   k_se_mlpb1: de = t sig (1 - sig) for the block's channels; partial dh = W2^T de over them
//               (waves over 16-channel ranges, lanes over j = rows of W2; wave order fixed)
//   k_se_mlpb2: dh = sum of the image's partials (chunk order), dr = dh swish'(r) (the first block
//               of an image stores it), dm = W1^T dr for the block's 64 channels (lanes over C)
__global__ __launch_bounds__(kBlock) void k_se_mlpb1(const float* __restrict__ t, const float* __restrict__ sig,
                                                     const float* __restrict__ w2, int C, int sq,
                                                     float* __restrict__ de, float* __restrict__ dh_part) {
    __shared__ float s_de[kMlpbC];
    __shared__ float s_part[kBlock / kWave][kMaxSq];
    const int nchunk = (C + kMlpbC - 1) / kMlpbC;
    const int n = blockIdx.x / nchunk, k = blockIdx.x % nchunk, c0 = k * kMlpbC;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    if ((int)threadIdx.x < kMlpbC) {
        const int c = c0 + (int)threadIdx.x;
        float d = 0.f;
        if (c < C) {
            d = se_de(t[(size_t)n * C + c], sig[(size_t)n * C + c]);
            de[(size_t)n * C + c] = d;
        }
        s_de[threadIdx.x] = d;
    }
    __syncthreads();
    const int cb = wave * kPer;
    s_part[wave][lane] = se_dh16(w2, s_de + cb, c0 + cb, C, sq, lane);
    __syncthreads();
    if ((int)threadIdx.x < sq) {
        const int j = threadIdx.x;
        dh_part[((size_t)n * nchunk + k) * sq + j] = sum4(s_part[0][j], s_part[1][j], s_part[2][j], s_part[3][j]);
    }
}

__global__ __launch_bounds__(kBlock) void k_se_mlpb2(const float* __restrict__ dh_part, const float* __restrict__ r,
                                                     const float* __restrict__ w1, int C, int sq,
                                                     float* __restrict__ dr, float* __restrict__ dm) {
    __shared__ float s_dr[kMaxSq];
    __shared__ float s_acc[kBlock / kWave][kWave];
    const int nchunk = (C + kMlpbC - 1) / kMlpbC, npart = nchunk;
    const int n = blockIdx.x / nchunk, k = blockIdx.x % nchunk;
    if ((int)threadIdx.x < sq) {
        const int j = threadIdx.x;
        float dh = 0.f;
        for (int q = 0; q < npart; ++q) dh += dh_part[((size_t)n * npart + q) * sq + j];
        const float d = se_dr(dh, r[(size_t)n * sq + j]);
        s_dr[j] = d;
        if (k == 0) dr[(size_t)n * sq + j] = d;
    }
    __syncthreads();
    // 64 channels per block: lane = channel, wave w sums the j in [w sq / 4, (w+1) sq / 4); waves
    // combined in order
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int c = k * kMlpbC + lane;
    s_acc[wave][lane] = se_dm_range(w1, s_dr, C, sq, c, wave * sq / 4, (wave + 1) * sq / 4);
    __syncthreads();
    if (wave == 0 && c < C)
        dm[(size_t)n * C + c] = sum4(s_acc[0][lane], s_acc[1][lane], s_acc[2][lane], s_acc[3][lane]);
}

// ---- the reductions with the per-image tails ---------------------------------------------------------

constexpr int kTail = 1024;                 // threads of a tail kernel's block: 16 waves = 16 planes of one image
constexpr int kTailWaves = kTail / kWave;
constexpr int kTailW = 16 * kTail;          // floats of LDS for W2 rows (forward) or the partial sums (backward)
constexpr int kTailUnits = 4 * ((kMaxC + kMlpbC - 1) / kMlpbC);  // (64-channel chunk, wave-of-four) pairs: 128
static_assert(2 * kTailUnits * kWave <= kTailW, "the backward tail keeps both partial arrays in s_buf");
constexpr int kSeBanks = 4;
constexpr int kSeBankImages = LSS_SE_TAIL_MAX_IMAGES;

// arrival counters, one word per image and bank; zero at load and between calls
__device__ unsigned g_se_ctr[kSeBanks][kSeBankImages];

// Called by every thread of a block after its published stores. True, in every thread, in the block whose
// ticket is the last of the `expected` of this counter; that block has re-zeroed the counter.
__device__ __forceinline__ bool last_arrival(unsigned* ctr, int expected, int* s_last) {
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // this wave's published stores have left
    __syncthreads();                                  // ... and every other wave's of the block
    if (threadIdx.x == 0) {
        const unsigned prev = __hip_atomic_fetch_add(ctr, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        const int last = prev == (unsigned)expected - 1u;
        if (last) __hip_atomic_store(ctr, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        *s_last = last;
    }
    __syncthreads();  // the other waves load published values only behind this barrier
    return *s_last != 0;
}

// k_se_mlp1 + k_se_mlp2 for image n by one 1024-thread block. W2 goes through LDS in chunks of cpc
// channels (all of C for sq <= 15), sixteen loads in flight per thread.
__device__ __forceinline__ void se_fwd_tail(int n, const float* m, const float* __restrict__ w1,
                                            const float* __restrict__ b1, const float* __restrict__ w2,
                                            const float* __restrict__ b2, int C, int sq, float* __restrict__ r_out,
                                            float* __restrict__ h_out, float* __restrict__ sig, float* s_buf,
                                            float* s_m, float* s_h) {
    const int t = threadIdx.x, lane = t & 63, wave = __builtin_amdgcn_readfirstlane(t >> 6);  // in SGPRs
    const int cpc = min(kTail, kTailW / (sq + 1));  // channels per chunk
    constexpr int kLd = 16;                         // loads in flight per thread while a chunk is staged
#pragma unroll 2  // at most kMaxC / kTail = 2 passes
    for (int c = t; c < C; c += kTail) s_m[c] = ld_agent(m + (size_t)n * C + c);
    __syncthreads();
    constexpr int JB = 4;  // rows per wave and pass (all of them, sq <= 64): 16 loads in flight per lane
    for (int j0 = wave; j0 < sq; j0 += JB * kTailWaves) {
        float a[JB], bj[JB];
#pragma unroll
        for (int u = 0; u < JB; ++u) bj[u] = b1[min(j0 + u * kTailWaves, sq - 1)];  // ahead of the dots, not behind
        se_fc1_dots<JB>(w1, s_m, C, sq, j0, kTailWaves, lane, a);
        if (lane == 0) {
#pragma unroll
            for (int u = 0; u < JB; ++u) {
                const int j = j0 + u * kTailWaves;
                if (j < sq) {
                    float r, h;
                    se_fc1_finish(a[u], bj[u], r, h);
                    r_out[(size_t)n * sq + j] = r;
                    h_out[(size_t)n * sq + j] = h;
                    s_h[j] = h;
                }
            }
        }
    }
    // element i = t + u * kTail of a chunk is column j of its row cl: stepped, not divided, per u
    const int cl0 = t / sq, jj0 = t - cl0 * sq, dcl = kTail / sq, dj = kTail - dcl * sq;
    for (int c0 = 0; c0 < C; c0 += cpc) {
        const int nc = min(cpc, C - c0);
        const float* wp = w2 + (size_t)c0 * sq;
        int cl = cl0, j = jj0;
        for (int i0 = t; i0 < nc * sq; i0 += kLd * kTail) {
            float v[kLd];
#pragma unroll
            for (int u = 0; u < kLd; ++u) v[u] = wp[min(i0 + u * kTail, nc * sq - 1)];  // all issued, then stored
#pragma unroll
            for (int u = 0; u < kLd; ++u) {
                if (i0 + u * kTail < nc * sq) s_buf[cl * (sq + 1) + j] = rbf(v[u]);
                cl += dcl;
                j += dj;
                if (j >= sq) {
                    j -= sq;
                    ++cl;
                }
            }
        }
        const float bc = b2[c0 + min(t, nc - 1)];
        __syncthreads();  // the chunk's rows (and, the first time, s_h) are in LDS
        if (t < nc) sig[(size_t)n * C + c0 + t] = se_fc2(s_buf + t * (sq + 1), s_h, sq, bc);
        __syncthreads();
    }
}

// k_se_mlpb1 + k_se_mlpb2 for image n by one 1024-thread block. A unit g = 4 k + w is what wave w of the
// fallback's block k (64 channels) did; the 16 waves take the units in turn, 16 loads in flight each.
__device__ __forceinline__ void se_bwd_tail(int n, const float* t_in, const float* __restrict__ sig,
                                            const float* __restrict__ r, const float* __restrict__ w1,
                                            const float* __restrict__ w2, int C, int sq, float* __restrict__ de,
                                            float* __restrict__ dr, float* __restrict__ dm, float* s_buf, float* s_de,
                                            float* s_dr) {
    const int t = threadIdx.x, lane = t & 63, wave = __builtin_amdgcn_readfirstlane(t >> 6);  // in SGPRs
    const int nchunk = (C + kMlpbC - 1) / kMlpbC, units = 4 * nchunk;
    float* s_part = s_buf;                      // [units][64]: partial dh
    float* s_acc = s_buf + kTailUnits * kWave;  // [units][64]: partial dm
    const float rv = t < sq ? r[(size_t)n * sq + t] : 0.f;
#pragma unroll 2  // at most kMaxC / kTail = 2 passes
    for (int c = t; c < C; c += kTail) {
        const float d = se_de(ld_agent(t_in + (size_t)n * C + c), sig[(size_t)n * C + c]);
        de[(size_t)n * C + c] = d;
        s_de[c] = d;
    }
    __syncthreads();
    for (int g = wave; g < units; g += kTailWaves)
        s_part[g * kWave + lane] = se_dh16(w2, s_de + g * kPer, g * kPer, C, sq, lane);
    __syncthreads();
    if (t < sq) {
        float dh = 0.f;
        for (int q = 0; q < nchunk; ++q) {
            const float* p = s_part + 4 * q * kWave + t;
            dh += sum4(p[0], p[kWave], p[2 * kWave], p[3 * kWave]);
        }
        const float d = se_dr(dh, rv);
        s_dr[t] = d;
        dr[(size_t)n * sq + t] = d;
    }
    __syncthreads();
    for (int g = wave; g < units; g += kTailWaves) {
        const int w = g & 3, c = (g >> 2) * kMlpbC + lane;
        s_acc[g * kWave + lane] = se_dm_range(w1, s_dr, C, sq, c, w * sq / 4, (w + 1) * sq / 4);
    }
    __syncthreads();
#pragma unroll 2  // at most kMaxC / kTail = 2 passes
    for (int c = t; c < C; c += kTail) {
        const float* p = s_acc + 4 * (c >> 6) * kWave + (c & 63);
        dm[(size_t)n * C + c] = sum4(p[0], p[kWave], p[2 * kWave], p[3 * kWave]);
    }
}

// block = (image n, cpb channels), wave w the channels c0 + w, c0 + w + 16, ...: one wave per plane as
// k_se_mean, four planes' loads at a time where a wave has several; then the image's last block runs the MLP
constexpr int kTailP = 4, kTailPDot = 2;  // planes a wave takes at once (the dot holds two operands per plane)
__global__ __launch_bounds__(kTail, 8) void k_se_mean_tail(const unsigned short* __restrict__ x, int C, int HW, int bpi,
                                                           int cpb, int bank, const float* __restrict__ w1,
                                                           const float* __restrict__ b1, const float* __restrict__ w2,
                                                           const float* __restrict__ b2, int sq, float* m,
                                                           float* __restrict__ r, float* __restrict__ h,
                                                           float* __restrict__ sig) {
    __shared__ float s_buf[kTailW];
    __shared__ float s_m[kMaxC];
    __shared__ float s_h[kMaxSq];
    __shared__ int s_last;
    const int n = blockIdx.x / bpi, c0 = (blockIdx.x % bpi) * cpb, cend = min(c0 + cpb, C);
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const size_t pstride = (size_t)kTailWaves * HW;
    for (int c = c0 + wave; c < cend; c += kTailP * kTailWaves) {
        const size_t pl = (size_t)n * C + c;
        const int np = min(kTailP, (cend - c + kTailWaves - 1) / kTailWaves);
        if (np == 1) {
            const float v = se_plane_mean(x + pl * HW, HW, lane);
            if (lane == 0) st_agent(m + pl, v);
        } else {
            float v[kTailP];
            se_planes_mean<kTailP>(x + pl * HW, pstride, np, HW, lane, v);
#pragma unroll
            for (int p = 0; p < kTailP; ++p)
                if (lane == 0 && p < np) st_agent(m + pl + p * kTailWaves, v[p]);
        }
    }
    if (!last_arrival(&g_se_ctr[bank][n], bpi, &s_last)) return;
    se_fwd_tail(n, m, w1, b1, w2, b2, C, sq, r, h, sig, s_buf, s_m, s_h);
}

__global__ __launch_bounds__(kTail, 8) void k_se_dot_tail(const unsigned short* __restrict__ g,
                                                          const unsigned short* __restrict__ x, int C, int HW, int bpi,
                                                          int cpb, int bank, const float* __restrict__ sig,
                                                          const float* __restrict__ r, const float* __restrict__ w1,
                                                          const float* __restrict__ w2, int sq, float* t,
                                                          float* __restrict__ de, float* __restrict__ dr,
                                                          float* __restrict__ dm) {
    __shared__ float s_buf[kTailW];
    __shared__ float s_de[kMaxC];
    __shared__ float s_dr[kMaxSq];
    __shared__ int s_last;
    const int n = blockIdx.x / bpi, c0 = (blockIdx.x % bpi) * cpb, cend = min(c0 + cpb, C);
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const size_t pstride = (size_t)kTailWaves * HW;
    for (int c = c0 + wave; c < cend; c += kTailPDot * kTailWaves) {
        const size_t pl = (size_t)n * C + c;
        const int np = min(kTailPDot, (cend - c + kTailWaves - 1) / kTailWaves);
        if (np == 1) {
            const float v = se_plane_dot(g + pl * HW, x + pl * HW, HW, lane);
            if (lane == 0) st_agent(t + pl, v);
        } else {
            float v[kTailPDot];
            se_planes_dot<kTailPDot>(g + pl * HW, x + pl * HW, pstride, np, HW, lane, v);
#pragma unroll
            for (int p = 0; p < kTailPDot; ++p)
                if (lane == 0 && p < np) st_agent(t + pl + p * kTailWaves, v[p]);
        }
    }
    if (!last_arrival(&g_se_ctr[bank][n], bpi, &s_last)) return;
    se_bwd_tail(n, t, sig, r, w1, w2, C, sq, de, dr, dm, s_buf, s_de, s_dr);
}

// y = bf16(x * sig[plane]), 4 elements per thread
__global__ __launch_bounds__(kBlock) void k_se_scale(const unsigned short* __restrict__ x,
                                                     const float* __restrict__ sig, int HW, int n4,
                                                     unsigned short* __restrict__ y) {
    const int t = blockIdx.x * kBlock + threadIdx.x;
    if (t >= n4) return;
    const int i = t * 4;
    const float s = sig[i / HW];
    float v[4];
    ld4(x + i, v);
#pragma unroll
    for (int k = 0; k < 4; ++k) v[k] *= s;
    st4(y + i, v);
}

// dx = bf16(g * sig + dm / HW), 4 elements per thread
__global__ __launch_bounds__(kBlock) void k_se_dx(const unsigned short* __restrict__ g, const float* __restrict__ sig,
                                                  const float* __restrict__ dm, int HW, int n4,
                                                  unsigned short* __restrict__ dx) {
    const int t = blockIdx.x * kBlock + threadIdx.x;
    if (t >= n4) return;
    const int i = t * 4;
    const int pl = i / HW;
    const float s = sig[pl], b = dm[pl] / (float)HW;
    float v[4];
    ld4(g + i, v);
#pragma unroll
    for (int k = 0; k < 4; ++k) v[k] = fmaf(v[k], s, b);
    st4(dx + i, v);
}

// The four parameter gradients of the two 1x1 convs in one launch, one thread per output, the N
// images summed in order (deterministic; the loops unrolled so 16 images' loads are in flight at once,
// the sums still one dependent chain in image order): dw2[c][j] = sum_n de[n][c] h[n][j] (C, sq),
// dw1[j][c] = sum_n dr[n][j] m[n][c] (sq, C), db1[j] = sum_n dr[n][j], db2[c] = sum_n de[n][c].
__global__ __launch_bounds__(kBlock) void k_se_wgrad(const float* __restrict__ de, const float* __restrict__ h,
                                                     const float* __restrict__ dr, const float* __restrict__ m,
                                                     int N, int C, int sq, float* __restrict__ dw1,
                                                     float* __restrict__ db1, float* __restrict__ dw2,
                                                     float* __restrict__ db2) {
    const int t = blockIdx.x * kBlock + threadIdx.x;
    const int cs = C * sq;
    float a = 0.f;
    if (t < cs) {  // dw2, lanes over j: de broadcast, h coalesced
        const int c = t / sq, j = t - c * sq;
#pragma unroll 16
        for (int n = 0; n < N; ++n) a = fmaf(de[(size_t)n * C + c], h[(size_t)n * sq + j], a);
        dw2[t] = a;
    } else if (t < 2 * cs) {  // dw1, lanes over c: m coalesced
        const int u = t - cs, j = u / C, c = u - j * C;
#pragma unroll 16
        for (int n = 0; n < N; ++n) a = fmaf(dr[(size_t)n * sq + j], m[(size_t)n * C + c], a);
        dw1[u] = a;
    } else if (t < 2 * cs + sq) {
        const int j = t - 2 * cs;
#pragma unroll 16
        for (int n = 0; n < N; ++n) a += dr[(size_t)n * sq + j];
        db1[j] = a;
    } else if (t < 2 * cs + sq + C) {
        const int c = t - 2 * cs - sq;
#pragma unroll 16
        for (int n = 0; n < N; ++n) a += de[(size_t)n * C + c];
        db2[c] = a;
    }
}

inline bool se_ok(int N, int C, int HW, int sq) {
    return N > 0 && C > 0 && C <= kMaxC && sq > 0 && sq <= kWave && HW > 0 && HW % 4 == 0 &&
           (long)N * C * HW < INT_MAX;
}

// x / y / dy / dx are read and written four bf16 (8 B) at a time; the fp32 arrays by element
inline bool se_aligned(const void* a, const void* b, const void* c = nullptr) {
    return ((reinterpret_cast<uintptr_t>(a) | reinterpret_cast<uintptr_t>(b) | reinterpret_cast<uintptr_t>(c)) & 7) == 0;
}

std::atomic<int> g_se_tails{LSS_SE_TAILS_DEFAULT};
std::atomic<unsigned> g_se_bank{0};

// The tails, or the fallback sequence? One counter word per image bounds N. Beyond that a static rule on
// the shape, from the per-shape table of the c3 step (profiles/r08/se_tails_per_shape.txt): the hand-off and
// the tail's chain of dependent loads cost 6 to 10 us whatever the shape, and one block then moves both
// weight matrices that the MLP launches spread over many CUs. The tail wins only while the matrices are
// small. Forward the largest C * sq that won was 864 (MBConv blocks 0-3) and the smallest that lost 2400 (by
// 0.1-0.6 us); backward 2400 won (blocks 0-5) and 9600 lost (by 0.2-0.7 us). The limits below, 1024 and 4096,
// sit between those. HW does not enter: the gain was the same at 11264 and at 704 elements a plane.
// Setting 2 (lss_se_tails) skips the rule: every shape the counters admit takes the tails.
constexpr int kSeTailFwdMaxW = 1024, kSeTailBwdMaxW = 4096;  // elements of one weight matrix, C * sq
inline bool se_tails(int N, int C, int sq, int /*HW*/, bool backward) {
    const int mode = g_se_tails.load(std::memory_order_relaxed);
    if (mode == 0 || N > kSeBankImages) return false;
    return mode >= 2 || C * sq <= (backward ? kSeTailBwdMaxW : kSeTailFwdMaxW);
}
// Blocks per image and channels per block of a tail kernel. Every block pays the hand-off once (its stores
// drained, a ticket drawn: two memory round trips that nothing hides), so there are no more blocks than are
// resident at once -- two per CU -- however many planes that gives a wave.
constexpr int kTailSlots = 512;
inline void se_tail_grid(int N, int C, int* bpi, int* cpb) {
    const int want = std::min(grid_blocks(C, kTailWaves), std::max(1, kTailSlots / N));
    *cpb = grid_blocks(grid_blocks(C, want), kTailWaves) * kTailWaves;  // whole rounds of the 16 waves
    *bpi = grid_blocks(C, *cpb);
}
inline int se_next_bank() { return (int)(g_se_bank.fetch_add(1u, std::memory_order_relaxed) % kSeBanks); }

// Everything a launch of lss_se_fwd / lss_se_bwd depends on, decided once: both launchers read it and lss_se_arm
// reports it (include/lss_convs.h), so the query cannot differ from what this build launches.
inline int se_arm(int pass, int N, int C, int HW, int sq, lss_se_arm_t* a) {
    if (!a || (pass != LSS_SE_FWD && pass != LSS_SE_BWD) || !se_ok(N, C, HW, sq)) return LSS_CONV_EINVAL;
    const bool bwd = pass == LSS_SE_BWD;
    const int planes = N * C, n4 = planes * HW / 4;
    *a = lss_se_arm_t{};
    a->tails = se_tails(N, C, sq, HW, bwd) ? 1 : 0;
    if (a->tails) {
        se_tail_grid(N, C, &a->bpi, &a->cpb);
        a->launches = 2;
        a->grid[0] = N * a->bpi;
        a->grid[1] = grid_blocks(n4, kBlock);
        // a block of nch channels: wave w takes the planes w, w + 16, ...
        a->planes_max = grid_blocks(std::min(a->cpb, C), kTailWaves);
        a->planes_min = (C - (a->bpi - 1) * a->cpb) / kTailWaves;
        a->w2_chunks = bwd ? 0 : grid_blocks(C, std::min(kTail, kTailW / (sq + 1)));
    } else {
        a->launches = 4;
        a->grid[0] = grid_blocks(planes, kBlock / kWave);
        a->grid[1] = bwd ? N * grid_blocks(C, kMlpbC) : N * grid_blocks(sq, 4);
        a->grid[2] = N * grid_blocks(C, bwd ? kMlpbC : kMlpC);
        a->grid[3] = grid_blocks(n4, kBlock);
        a->planes_max = 1;
        a->planes_min = planes % (kBlock / kWave) ? 0 : 1;  // the last block's idle waves
        a->w2_chunks = bwd ? 0 : grid_blocks(C, kMlpC);
    }
    a->chunks64 = bwd ? grid_blocks(C, kMlpbC) : 0;
    a->planes_class = std::min(a->planes_max, (int)LSS_SE_PLANES_MANY);
    a->ragged = a->planes_min < a->planes_max;
    if (bwd)
        a->chunk_class = C <= kMlpbC ? LSS_SE_BWD_ONE_CHUNK
                         : 4 * a->chunks64 <= kTailWaves ? LSS_SE_BWD_UNIT_A_WAVE
                         : C <= kTail ? LSS_SE_BWD_UNITS_A_WAVE : LSS_SE_BWD_TWO_PASSES;
    else
        a->chunk_class = a->w2_chunks == 1 ? LSS_SE_FWD_ONE_CHUNK
                         : a->tails && C > kTail ? LSS_SE_FWD_TWO_PASSES : LSS_SE_FWD_CHUNKS;
    return 0;
}

}  // namespace

extern "C" {

int lss_se_tails(int on) { return g_se_tails.exchange(on <= 0 ? 0 : on >= 2 ? 2 : 1, std::memory_order_relaxed); }

int lss_se_arm(int32_t pass, int32_t N, int32_t C, int32_t HW, int32_t sq, lss_se_arm_t* arm) {
    return se_arm(pass, N, C, HW, sq, arm);
}

int lss_se_fwd(const void* x, int32_t N, int32_t C, int32_t HW, const float* w1, const float* b1, const float* w2,
               const float* b2, int32_t sq, float* m, float* r, float* h, float* sig, void* y, void* stream) {
    if (!x || !w1 || !b1 || !w2 || !b2 || !m || !r || !h || !sig || !y || !se_ok(N, C, HW, sq)) return LSS_CONV_EINVAL;
    if (!se_aligned(x, y)) return LSS_CONV_EINVAL;
    hipStream_t s = (hipStream_t)stream;
    lss_se_arm_t a;
    if (se_arm(LSS_SE_FWD, N, C, HW, sq, &a) != 0) return LSS_CONV_EINVAL;
    const int planes = N * C, n4 = planes * HW / 4;
    if (a.tails) {
        hipLaunchKernelGGL(k_se_mean_tail, dim3(a.grid[0]), dim3(kTail), 0, s, (const unsigned short*)x, C, HW, a.bpi,
                           a.cpb, se_next_bank(), w1, b1, w2, b2, sq, m, r, h, sig);
    } else {
        hipLaunchKernelGGL(k_se_mean, dim3(a.grid[0]), dim3(kBlock), 0, s, (const unsigned short*)x, planes, HW, m);
        hipLaunchKernelGGL(k_se_mlp1, dim3(a.grid[1]), dim3(kBlock), 0, s, m, w1, b1, C, sq, r, h);
        hipLaunchKernelGGL(k_se_mlp2, dim3(a.grid[2]), dim3(kBlock), 0, s, h, w2, b2, C, sq, sig);
    }
    hipLaunchKernelGGL(k_se_scale, dim3(a.grid[a.launches - 1]), dim3(kBlock), 0, s, (const unsigned short*)x, sig, HW, n4,
                       (unsigned short*)y);
    return launch_status();
}

int lss_se_bwd(const void* dy, const void* x, int32_t N, int32_t C, int32_t HW, const float* w1, const float* w2,
               int32_t sq, const float* r, const float* sig, float* t, float* dh_part, float* de, float* dr, float* dm,
               void* dx, void* stream) {
    if (!dy || !x || !w1 || !w2 || !r || !sig || !t || !dh_part || !de || !dr || !dm || !dx || !se_ok(N, C, HW, sq))
        return LSS_CONV_EINVAL;
    if (!se_aligned(dy, x, dx)) return LSS_CONV_EINVAL;
    hipStream_t s = (hipStream_t)stream;
    lss_se_arm_t a;
    if (se_arm(LSS_SE_BWD, N, C, HW, sq, &a) != 0) return LSS_CONV_EINVAL;
    const int planes = N * C, n4 = planes * HW / 4;
    if (a.tails) {  // the chunk partials stay in LDS: dh_part is not touched
        hipLaunchKernelGGL(k_se_dot_tail, dim3(a.grid[0]), dim3(kTail), 0, s, (const unsigned short*)dy,
                           (const unsigned short*)x, C, HW, a.bpi, a.cpb, se_next_bank(), sig, r, w1, w2, sq, t, de, dr,
                           dm);
    } else {
        hipLaunchKernelGGL(k_se_dot, dim3(a.grid[0]), dim3(kBlock), 0, s, (const unsigned short*)dy,
                           (const unsigned short*)x, planes, HW, t);
        hipLaunchKernelGGL(k_se_mlpb1, dim3(a.grid[1]), dim3(kBlock), 0, s, t, sig, w2, C, sq, de, dh_part);
        hipLaunchKernelGGL(k_se_mlpb2, dim3(a.grid[2]), dim3(kBlock), 0, s, dh_part, r, w1, C, sq, dr, dm);
    }
    hipLaunchKernelGGL(k_se_dx, dim3(a.grid[a.launches - 1]), dim3(kBlock), 0, s, (const unsigned short*)dy, sig, dm, HW,
                       n4, (unsigned short*)dx);
    return launch_status();
}

int lss_se_wgrad(const float* de, const float* h, const float* dr, const float* m, int32_t N, int32_t C, int32_t sq,
                 float* dw1, float* db1, float* dw2, float* db2, void* stream) {
    if (!de || !h || !dr || !m || !dw1 || !db1 || !dw2 || !db2 || N <= 0 || C <= 0 || C > kMaxC || sq <= 0 ||
        sq > kWave)
        return LSS_CONV_EINVAL;
    const int total = 2 * C * sq + sq + C;
    hipLaunchKernelGGL(k_se_wgrad, dim3(grid_blocks(total, kBlock)), dim3(kBlock), 0, (hipStream_t)stream, de, h, dr, m, N,
                       C, sq, dw1, db1, dw2, db2);
    return launch_status();
}

}  // extern "C"
