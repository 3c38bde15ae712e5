// lss_elementwise.hip -- the conv stack's small elementwise and reduction kernels: per-sample scale (+ add),
// dropout, the weight flip of a transposed convolution, per-channel sums.

#include <limits.h>

#include "lss_convs.h"
#include "lss_device.h"

// The library is built with -ffp-contract=off for the geometry's reference op order (lss_hip.hip);
// the conv-stack kernels here have no bit-exact contract, so they keep FMA contraction.
#pragma clang fp contract(fast)

namespace {

constexpr int kBlock = 256;

// ----------------------------------------------------------------------------- per-sample scale (+ add)
// y = bf16(x * scale[n] (+ r)) over sample-major bf16 tensors, scale[n] from the sample's draw, 8 elements (16 B) per thread: the
// MBConv residual with stochastic depth (efficientnet_pytorch drop_connect, x / keep * mask +
// inputs) in one pass instead of three; with r == nullptr, its backward dx = bf16(dy * scale[n]).

// the sample's scale from its uniform draw u (bf16): mask = floor(bf16(keep + u)) as torch computes
// floor(keep + rand(..., dtype=bf16)), scale = mask / keep
__device__ __forceinline__ float drop_scale(const bf16* u, long long n, float keep) {
    const float t = __bfloat162float(__float2bfloat16(keep + __bfloat162float(u[n])));
    return floorf(t) / keep;
}

__global__ __launch_bounds__(kBlock) void k_scale_add(const uint4* __restrict__ x, const bf16* __restrict__ u,
                                                      float keep, const uint4* __restrict__ r, long long per8,
                                                      long long n8, uint4* __restrict__ y) {
    const long long i = (long long)blockIdx.x * kBlock + threadIdx.x;
    if (i >= n8) return;
    const float sc = drop_scale(u, i / per8, keep);
    float v[8], w[8];
    unpack8(x[i], v);
    if (r) {
        unpack8(r[i], w);
#pragma unroll
        for (int k = 0; k < 8; ++k) v[k] = fmaf(v[k], sc, w[k]);
    } else {
#pragma unroll
        for (int k = 0; k < 8; ++k) v[k] *= sc;
    }
    y[i] = make_uint4(pack2(v[0], v[1]), pack2(v[2], v[3]), pack2(v[4], v[5]), pack2(v[6], v[7]));
}


// ---- dropout (CamEncode.dropout, src/models.py:44, 53) on a counter-based RNG, laid out for the next kernel
// philox4x32 (lss_device.h) is a pure function of (key, counter), so the backward regenerates the forward's
// mask from the same seed.

// Elements of 16-B vector v (8 bf16 or 4 fp32) kept: bit j = element j; uniform u = top 24 bits / 2^24,
// kept when u < keep (P = keep). Counter (v, 0, 0, 0): 4 draws, a second block (v, 0, 1, 0) for bf16.
template <int EPV>
__device__ __forceinline__ unsigned keep_bits(uint2 key, long long v, unsigned thresh) {
    unsigned bits = 0;
#pragma unroll
    for (int h = 0; h < EPV / 4; ++h) {
        const uint4 r = philox4x32(key, make_uint4((unsigned)v, (unsigned)(v >> 32), (unsigned)h, 0u));
        bits |= ((r.x >> 8) < thresh ? 1u : 0u) << (4 * h);
        bits |= ((r.y >> 8) < thresh ? 1u : 0u) << (4 * h + 1);
        bits |= ((r.z >> 8) < thresh ? 1u : 0u) << (4 * h + 2);
        bits |= ((r.w >> 8) < thresh ? 1u : 0u) << (4 * h + 3);
    }
    return bits;
}

constexpr int kDropVpt = 2;  // 16-B vectors per thread
// XCD x (blockIdx & 7) writes one contiguous eighth of the tensor, the eighth the fused lift's blocks on
// that XCD read (k_depthnet_lift3: pixel tiles in XCD-contiguous runs), so the lift finds its features
// in its own L2 instead of another XCD's; the blocks also touch `pf` (the lift's packed weights), one
// slice per block of each XCD, so every XCD's L2 holds them before the lift starts.
template <typename T>
__global__ __launch_bounds__(kBlock) void k_dropout(const uint4* __restrict__ x, long long nv,
                                                    const unsigned long long* __restrict__ seed, unsigned thresh,
                                                    float scale, uint4* __restrict__ y, const uint4* __restrict__ pf,
                                                    long long pf16) {
    constexpr int EPV = 16 / (int)sizeof(T);
    const int bpx = gridDim.x >> 3;                                         // blocks per XCD
    const long long lb = (long long)(blockIdx.x & 7) * bpx + (blockIdx.x >> 3);  // XCD-contiguous
    uint4 warm = make_uint4(0u, 0u, 0u, 0u);
    if (pf) {
        const long long per = (pf16 + bpx - 1) / bpx;  // 16-B pieces per block
        const long long i = (long long)(blockIdx.x >> 3) * per + threadIdx.x;
        if (threadIdx.x < per && i < pf16) warm = pf[i];
    }
    const unsigned long long sd = *seed;
    const uint2 key = make_uint2((unsigned)sd, (unsigned)(sd >> 32));
    uint4 in[kDropVpt];
    long long vi[kDropVpt];
#pragma unroll
    for (int k = 0; k < kDropVpt; ++k) {
        vi[k] = (lb * kDropVpt + k) * kBlock + threadIdx.x;
        in[k] = vi[k] < nv ? x[vi[k]] : make_uint4(0u, 0u, 0u, 0u);
    }
#pragma unroll
    for (int k = 0; k < kDropVpt; ++k) {
        if (vi[k] >= nv) continue;
        const unsigned bits = keep_bits<EPV>(key, vi[k], thresh);
        uint4 o;
        if constexpr (EPV == 8) {
            float v[8];
            unpack8(in[k], v);
#pragma unroll
            for (int j = 0; j < 8; ++j) v[j] = ((bits >> j) & 1u) ? v[j] * scale : 0.f;
            o = make_uint4(pack2(v[0], v[1]), pack2(v[2], v[3]), pack2(v[4], v[5]), pack2(v[6], v[7]));
        } else {
            const float v[4] = {__uint_as_float(in[k].x), __uint_as_float(in[k].y), __uint_as_float(in[k].z),
                                __uint_as_float(in[k].w)};
            o = make_uint4(__float_as_uint((bits & 1u) ? v[0] * scale : 0.f),
                           __float_as_uint((bits & 2u) ? v[1] * scale : 0.f),
                           __float_as_uint((bits & 4u) ? v[2] * scale : 0.f),
                           __float_as_uint((bits & 8u) ? v[3] * scale : 0.f));
        }
        y[vi[k]] = o;
    }
    asm volatile("" : : "v"(warm.x), "v"(warm.y), "v"(warm.z), "v"(warm.w));  // (the prefetch must land)
}

// Per-channel sums of an NCHW tensor (the depthnet bias gradient from d(logits), src/models.py:47):
// block = channel, the (image, pixel) elements strided over the threads, 4 loads in flight per thread,
// then a fixed-order block reduction (deterministic).
template <typename T>
__global__ __launch_bounds__(kBlock) void k_channel_sums(const T* __restrict__ x, int N, int C, int HW,
                                                         float* __restrict__ out) {
    __shared__ float s_w[kBlock / kWave];
    const int c = blockIdx.x;
    const int total = N * HW;
    float s = 0.f;
    int e = threadIdx.x;
    for (; e + 3 * kBlock < total; e += 4 * kBlock) {
        float v[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int i = e + u * kBlock, n = i / HW, p = i - n * HW;
            v[u] = ld(x + ((size_t)n * C + c) * HW + p);
        }
        s += (v[0] + v[1]) + (v[2] + v[3]);
    }
    for (; e < total; e += kBlock) {
        const int n = e / HW, p = e - n * HW;
        s += ld(x + ((size_t)n * C + c) * HW + p);
    }
#pragma unroll
    for (int o = kWave / 2; o > 0; o >>= 1) s += __shfl_xor(s, o, kWave);
    if ((threadIdx.x & (kWave - 1)) == 0) s_w[threadIdx.x / kWave] = s;
    __syncthreads();
    if (threadIdx.x == 0) {
        float b = 0.f;
#pragma unroll
        for (int w = 0; w < kBlock / kWave; ++w) b += s_w[w];
        out[c] = b;
    }
}

// wt[i][o][a][b] = w[o][i][K-1-a][K-1-b], written channels-last ([i][a][b][o] in memory): the weight of a
// stride-1 transposed convolution as a forward one (models._Conv3x3's backward-data). One thread per
// output element, consecutive threads along o (coalesced writes; the reads are a 1.2 MB weight, in L2).
template <typename T>
__global__ __launch_bounds__(kBlock) void k_conv_flip_weight(const T* __restrict__ w, int O, int I, int K, int cl_in,
                                                             T* __restrict__ wt) {
    const long e = (long)blockIdx.x * kBlock + threadIdx.x;
    const long n = (long)O * I * K * K;
    if (e >= n) return;
    const int o = (int)(e % O);
    long r = e / O;
    const int b = (int)(r % K);
    r /= K;
    const int a = (int)(r % K);
    const int i = (int)(r / K);
    const int ka = K - 1 - a, kb = K - 1 - b;
    const long src = cl_in ? (((long)o * K + ka) * K + kb) * I + i : (((long)o * I + i) * K + ka) * K + kb;
    wt[e] = w[src];
}

// The tiled form: per tap, a 64 x 64 (o, i) tile read along i (coalesced for channels-last weights,
// whose innermost index is i; 9-element strides for contiguous ones) and written along o (wt's innermost)
// through an LDS transpose (odd row stride); each thread's 16 loads are issued together (a loop that
// loaded and stored one element per iteration took 11 us per weight: 16 dependent round trips).
template <typename T>
__global__ __launch_bounds__(kBlock) void k_conv_flip_weight_cl(const T* __restrict__ w, int O, int I, int K, int cl,
                                                                T* __restrict__ wt) {
    __shared__ T tile[64][65];
    const int ti = (I + 63) / 64, to = (O + 63) / 64;
    int b = blockIdx.x;
    const int it = b % ti;
    b /= ti;
    const int ot = b % to;
    const int tap = b / to;  // output tap (a, b) = (tap / K, tap % K); source tap K*K - 1 - tap
    const int i0 = it * 64, o0 = ot * 64, src_tap = K * K - 1 - tap;
    const long so = (long)K * K * I, si = cl ? 1 : K * K, st = cl ? I : 1;
    const int c = threadIdx.x & 63, r0 = threadIdx.x >> 6;
    constexpr int R = 64 / (kBlock / 64);
    T v[R];
#pragma unroll
    for (int k = 0; k < R; ++k) {  // rows o, columns i (clamped addresses, all loads in flight)
        const int o = min(o0 + r0 + k * (kBlock / 64), O - 1), i = min(i0 + c, I - 1);
        v[k] = w[o * so + src_tap * st + i * si];
    }
#pragma unroll
    for (int k = 0; k < R; ++k) tile[r0 + k * (kBlock / 64)][c] = v[k];
    __syncthreads();
#pragma unroll
    for (int k = 0; k < R; ++k) {  // rows i, columns o
        const int i = i0 + r0 + k * (kBlock / 64), o = o0 + c;
        if (o < O && i < I) wt[((long)i * K * K + tap) * O + o] = tile[c][r0 + k * (kBlock / 64)];
    }
}

}  // namespace

extern "C" {

int lss_scale_add(const void* x, const void* u, float keep, const void* res, int64_t N, int64_t per, void* y,
                  void* stream) {
    if (!x || !u || !y || !(keep > 0.f && keep <= 1.f) || N <= 0 || per <= 0 || per % 8 != 0 ||
        ((reinterpret_cast<uintptr_t>(x) | reinterpret_cast<uintptr_t>(res) | reinterpret_cast<uintptr_t>(y)) & 15))
        return LSS_CONV_EINVAL;
    const long long n8 = (long long)N * per / 8;
    const long long nb = (n8 + kBlock - 1) / kBlock;
    if (nb > INT_MAX) return LSS_CONV_EINVAL;
    hipLaunchKernelGGL(k_scale_add, dim3((unsigned)nb), dim3(kBlock), 0, (hipStream_t)stream, (const uint4*)x, (const bf16*)u,
                       keep, (const uint4*)res, (long long)(per / 8), n8, (uint4*)y);
    return launch_status();
}

int lss_conv_flip_weight(const void* w, int32_t dtype, int32_t O, int32_t I, int32_t K, int32_t w_layout, void* wt,
                         void* stream) {
    if (!w || !wt || O <= 0 || I <= 0 || K <= 0 || (dtype != LSS_CONV_BF16 && dtype != LSS_CONV_F32) ||
        (w_layout != LSS_CONV_NCHW && w_layout != LSS_CONV_NHWC))
        return LSS_CONV_EINVAL;
    const long n = (long)O * I * K * K;
    if (n >= INT_MAX) return LSS_CONV_EINVAL;
    const int cl = w_layout == LSS_CONV_NHWC;
    const unsigned grid = (unsigned)((n + kBlock - 1) / kBlock);
    hipStream_t s = (hipStream_t)stream;
    if (O >= 64 && I >= 64) {
        const unsigned gcl = (unsigned)(((I + 63) / 64) * ((O + 63) / 64) * K * K);
        if (dtype == LSS_CONV_BF16)
            hipLaunchKernelGGL(k_conv_flip_weight_cl<bf16>, dim3(gcl), dim3(kBlock), 0, s, (const bf16*)w, O, I, K, cl,
                               (bf16*)wt);
        else
            hipLaunchKernelGGL(k_conv_flip_weight_cl<float>, dim3(gcl), dim3(kBlock), 0, s, (const float*)w, O, I, K,
                               cl, (float*)wt);
    } else if (dtype == LSS_CONV_BF16)
        hipLaunchKernelGGL(k_conv_flip_weight<bf16>, dim3(grid), dim3(kBlock), 0, s, (const bf16*)w, O, I, K, cl, (bf16*)wt);
    else
        hipLaunchKernelGGL(k_conv_flip_weight<float>, dim3(grid), dim3(kBlock), 0, s, (const float*)w, O, I, K, cl,
                           (float*)wt);
    return launch_status();
}

int lss_dropout(const void* x, int32_t dtype, int64_t n, const uint64_t* seed, float keep, void* y, const void* prefetch,
                int64_t prefetch_bytes, void* stream) {
    const int esz = dtype == LSS_CONV_BF16 ? 2 : dtype == LSS_CONV_F32 ? 4 : 0;
    if (!x || !y || !seed || !esz || n <= 0 || (n * esz) % 16 != 0 || !(keep > 0.f && keep <= 1.f) ||
        prefetch_bytes < 0 || (prefetch && prefetch_bytes % 16 != 0) ||
        ((reinterpret_cast<uintptr_t>(x) | reinterpret_cast<uintptr_t>(y) | reinterpret_cast<uintptr_t>(prefetch)) & 15))
        return LSS_CONV_EINVAL;
    const long long nv = n * esz / 16;
    const long long nb = (nv + (long long)kBlock * kDropVpt - 1) / ((long long)kBlock * kDropVpt);
    const long long grid = 8 * ((nb + 7) / 8);  // logical blocks past nb write nothing
    if (grid > INT_MAX) return LSS_CONV_EINVAL;
    // keep when (24 random bits) < keep * 2^24; the kept elements are scaled by 1 / keep (torch's dropout)
    const unsigned thresh = (unsigned)fminf(keep * 16777216.0f, 16777216.0f);
    const float scale = 1.0f / keep;
    hipStream_t s = (hipStream_t)stream;
    const uint4* pf = prefetch_bytes > 0 ? (const uint4*)prefetch : nullptr;
    if (esz == 2)
        hipLaunchKernelGGL(k_dropout<bf16>, dim3((unsigned)grid), dim3(kBlock), 0, s, (const uint4*)x, nv,
                           (const unsigned long long*)seed, thresh, scale, (uint4*)y, pf, prefetch_bytes / 16);
    else
        hipLaunchKernelGGL(k_dropout<float>, dim3((unsigned)grid), dim3(kBlock), 0, s, (const uint4*)x, nv,
                           (const unsigned long long*)seed, thresh, scale, (uint4*)y, pf, prefetch_bytes / 16);
    return launch_status();
}

int lss_channel_sums(const void* x, int32_t dtype, int32_t N, int32_t C, int32_t HW, float* out, void* stream) {
    if (!x || !out || N <= 0 || C <= 0 || HW <= 0 || (long long)N * C * HW >= INT_MAX ||
        (dtype != LSS_CONV_BF16 && dtype != LSS_CONV_F32))
        return LSS_CONV_EINVAL;
    hipStream_t s = (hipStream_t)stream;
    if (dtype == LSS_CONV_BF16)
        hipLaunchKernelGGL(k_channel_sums<bf16>, dim3(C), dim3(kBlock), 0, s, (const bf16*)x, N, C, HW, out);
    else
        hipLaunchKernelGGL(k_channel_sums<float>, dim3(C), dim3(kBlock), 0, s, (const float*)x, N, C, HW, out);
    return launch_status();
}

}  // extern "C"
