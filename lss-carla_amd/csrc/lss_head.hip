// lss_head.hip -- 1x1 convolution to ONE output channel over channels-last rows (BevEncode's last conv, up2.4:
// 128 -> outC = 1, src/models.py:115). As a GEMM it is a GEMV: its weight gradient is a K = B*X*Y
// reduction that hipBLASLt ran on 8 workgroups (MT16x16x512, ~210 us of a c3 step). Here a wave
// reads 4 rows per instruction (16 lanes x 16 B = one 128-channel row), fp32 accumulation.

#include "lss_convs.h"
#include "lss_device.h"

// The library is built with -ffp-contract=off for the geometry's reference op order (lss_hip.hip);
// the conv-stack kernels here have no bit-exact contract, so they keep FMA contraction.
#pragma clang fp contract(fast)

namespace {

constexpr int kBlock = 256;
constexpr int kHeadRows = 256;  // rows per block (64 per wave)

// BN mode (bnst = a batch norm's saved (4, C) statistics, NHWC): the input row is the batch norm's INPUT and
// each value goes through the apply pass's arithmetic first -- bf16(relu(fmaf(x, scale, shift))), what
// lss_bn_fwd's ReLU apply would have stored -- so the normalised map is never materialised.
__device__ __forceinline__ void head_bn8(const float* __restrict__ bnst, int C, int c0, float* sc, float* sh) {
#pragma unroll
    for (int i = 0; i < 8; ++i) {
        sc[i] = bnst ? bnst[2 * C + c0 + i] : 1.f;
        sh[i] = bnst ? bnst[3 * C + c0 + i] : 0.f;
    }
}
__device__ __forceinline__ float head_in(float v, bool bn, float sc, float sh) {
    return bn ? __bfloat162float(__float2bfloat16(fmaxf(fmaf(v, sc, sh), 0.f))) : v;
}

template <int LPR>  // lanes per row: C / 8
__global__ __launch_bounds__(kBlock) void k_head1_fwd(const uint4* __restrict__ x, const float* __restrict__ w,
                                                      const float* __restrict__ bias, int P, bf16* __restrict__ y,
                                                      const float* __restrict__ bnst) {
    constexpr int RPI = kWave / LPR;  // rows per wave instruction
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int col = lane % LPR, sub = lane / LPR;
    float wv[8], sc[8], sh[8];
#pragma unroll
    for (int i = 0; i < 8; ++i) wv[i] = w[col * 8 + i];
    const bool bn = bnst != nullptr;
    head_bn8(bnst, LPR * 8, col * 8, sc, sh);
    const float b = bias ? *bias : 0.f;  // (a device value: a captured graph replays with the current bias)
    const int r0 = blockIdx.x * kHeadRows + wave * (kHeadRows / 4);
#pragma unroll 4
    for (int it = 0; it < kHeadRows / 4 / RPI; ++it) {
        const int r = r0 + it * RPI + sub;
        float acc = 0.f;
        if (r < P) {
            const uint4 v = x[(size_t)r * LPR + col];
            const unsigned u[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                acc = fmaf(head_in(__uint_as_float(u[i] << 16), bn, sc[2 * i], sh[2 * i]), wv[2 * i], acc);
                acc = fmaf(head_in(__uint_as_float(u[i] & 0xFFFF0000u), bn, sc[2 * i + 1], sh[2 * i + 1]), wv[2 * i + 1],
                           acc);
            }
        }
#pragma unroll
        for (int o = LPR / 2; o > 0; o >>= 1) acc += __shfl_xor(acc, o, kWave);
        if (col == 0 && r < P) y[r] = __float2bfloat16(acc + b);
    }
}

// dx[r, c] = dy[r] * w[c] (bf16); partial[block][c] = sum over the block's rows of dy[r] * x[r, c],
// partial[block][C] = sum of dy[r] (fixed reduction order: deterministic).
// (BN mode as k_head1_fwd's; dx == NULL: no input gradient written -- the batch norm's backward takes it
// as the rank-1 product bf16(dy[r] w[c]) itself, lss_bn_bwd_rank1)
template <int LPR>
__global__ __launch_bounds__(kBlock) void k_head1_bwd(const uint4* __restrict__ x, const bf16* __restrict__ dy,
                                                      const float* __restrict__ w, int P, uint4* __restrict__ dx,
                                                      float* __restrict__ partial, const float* __restrict__ bnst) {
    constexpr int RPI = kWave / LPR;
    constexpr int C = LPR * 8;
    __shared__ float s_part[4][C + 1];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int col = lane % LPR, sub = lane / LPR;
    float wv[8], acc[8] = {}, sc[8], sh[8];
    float dsum = 0.f;
#pragma unroll
    for (int i = 0; i < 8; ++i) wv[i] = w[col * 8 + i];
    const bool bn = bnst != nullptr;
    head_bn8(bnst, C, col * 8, sc, sh);
    const int r0 = blockIdx.x * kHeadRows + wave * (kHeadRows / 4);
#pragma unroll 4
    for (int it = 0; it < kHeadRows / 4 / RPI; ++it) {
        const int r = r0 + it * RPI + sub;
        if (r < P) {
            const float g = __bfloat162float(dy[r]);
            const uint4 v = x[(size_t)r * LPR + col];
            const unsigned u[4] = {v.x, v.y, v.z, v.w};
            unsigned o[4];
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const float lo = head_in(__uint_as_float(u[i] << 16), bn, sc[2 * i], sh[2 * i]);
                const float hi = head_in(__uint_as_float(u[i] & 0xFFFF0000u), bn, sc[2 * i + 1], sh[2 * i + 1]);
                acc[2 * i] = fmaf(g, lo, acc[2 * i]);
                acc[2 * i + 1] = fmaf(g, hi, acc[2 * i + 1]);
                const bf16 a = __float2bfloat16(g * wv[2 * i]), c = __float2bfloat16(g * wv[2 * i + 1]);
                o[i] = (unsigned)*reinterpret_cast<const unsigned short*>(&a) |
                       ((unsigned)*reinterpret_cast<const unsigned short*>(&c) << 16);
            }
            if (dx) dx[(size_t)r * LPR + col] = make_uint4(o[0], o[1], o[2], o[3]);
            if (col == 0) dsum += g;
        }
    }
    // lanes of one column slice: reduce over the wave's row groups, then over the waves via LDS
#pragma unroll
    for (int i = 0; i < 8; ++i)
#pragma unroll
        for (int off = LPR; off < kWave; off <<= 1) acc[i] += __shfl_xor(acc[i], off, kWave);
#pragma unroll
    for (int off = LPR; off < kWave; off <<= 1) dsum += __shfl_xor(dsum, off, kWave);
    if (sub == 0) {
#pragma unroll
        for (int i = 0; i < 8; ++i) s_part[wave][col * 8 + i] = acc[i];
        if (col == 0) s_part[wave][C] = dsum;
    }
    __syncthreads();
    for (int c = threadIdx.x; c <= C; c += kBlock)
        partial[(size_t)blockIdx.x * (C + 1) + c] = ((s_part[0][c] + s_part[1][c]) + s_part[2][c]) + s_part[3][c];
}

// ---- The same 1x1 convolution to K = 2..8 output channels (a multi-class BevEncode: up2.4 with outC = K).
// Rows in, K NCHW planes out: y / dy are (N, K, H, W) contiguous, so a block's 256 rows x K values cross
// LDS and reach memory as K runs along the pixel axis (a block may straddle an image boundary: row r is
// pixel q = r % HW of image n = r / HW, at (n K + k) HW + q). Per channel k the arithmetic is k_head1_*'s,
// instruction for instruction: the 8 fmas in channel order, the same butterflies, the same fold of the
// waves -- the lane keeps its 8 channels x K weights in registers and reads each row once for all K.
template <int LPR, int K>
__global__ __launch_bounds__(kBlock) void k_headk_fwd(const uint4* __restrict__ x, const float* __restrict__ w,
                                                      const float* __restrict__ bias, int P, int HW,
                                                      bf16* __restrict__ y, const float* __restrict__ bnst) {
    constexpr int RPI = kWave / LPR;
    constexpr int C = LPR * 8;
    __shared__ bf16 s_y[K][kHeadRows];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int col = lane % LPR, sub = lane / LPR;
    float wv[K][8], sc[8], sh[8], b[K];
#pragma unroll
    for (int k = 0; k < K; ++k) {
#pragma unroll
        for (int i = 0; i < 8; ++i) wv[k][i] = w[k * C + col * 8 + i];
        b[k] = bias ? bias[k] : 0.f;
    }
    const bool bn = bnst != nullptr;
    head_bn8(bnst, C, col * 8, sc, sh);
    const int l0 = wave * (kHeadRows / 4);
    const int r0 = blockIdx.x * kHeadRows + l0;
#pragma unroll 4
    for (int it = 0; it < kHeadRows / 4 / RPI; ++it) {
        const int r = r0 + it * RPI + sub;
        float acc[K];
#pragma unroll
        for (int k = 0; k < K; ++k) acc[k] = 0.f;
        if (r < P) {
            const uint4 v = x[(size_t)r * LPR + col];
            const unsigned u[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const float lo = head_in(__uint_as_float(u[i] << 16), bn, sc[2 * i], sh[2 * i]);
                const float hi = head_in(__uint_as_float(u[i] & 0xFFFF0000u), bn, sc[2 * i + 1], sh[2 * i + 1]);
#pragma unroll
                for (int k = 0; k < K; ++k) {
                    acc[k] = fmaf(lo, wv[k][2 * i], acc[k]);
                    acc[k] = fmaf(hi, wv[k][2 * i + 1], acc[k]);
                }
            }
        }
#pragma unroll
        for (int k = 0; k < K; ++k) {
#pragma unroll
            for (int o = LPR / 2; o > 0; o >>= 1) acc[k] += __shfl_xor(acc[k], o, kWave);
        }
        if (col == 0) {
#pragma unroll
            for (int k = 0; k < K; ++k) s_y[k][l0 + it * RPI + sub] = __float2bfloat16(acc[k] + b[k]);
        }
    }
    __syncthreads();
    const int r = blockIdx.x * kHeadRows + threadIdx.x;  // thread = row: each plane's run is contiguous in q
    if (r < P) {
        const int n = r / HW, q = r - n * HW;
        bf16* o = y + (size_t)n * K * HW + q;
#pragma unroll
        for (int k = 0; k < K; ++k) o[(size_t)k * HW] = s_y[k][threadIdx.x];
    }
}

// dx[r, c] = bf16(sum_k dy[r, k] w[k, c]) (fp32, k ascending); partial[block][k][c] = sum over the block's
// rows of dy[r, k] in[r, c], partial[block][k][C] = sum of dy[r, k] -- k_head1_bwd's row partition and
// reduction order per channel k.
template <int LPR, int K>
__global__ __launch_bounds__(kBlock) void k_headk_bwd(const uint4* __restrict__ x, const bf16* __restrict__ dy,
                                                      const float* __restrict__ w, int P, int HW,
                                                      uint4* __restrict__ dx, float* __restrict__ partial,
                                                      const float* __restrict__ bnst) {
    constexpr int RPI = kWave / LPR;
    constexpr int C = LPR * 8;
    __shared__ float s_dy[K][kHeadRows];
    __shared__ float s_part[K][C + 1];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int col = lane % LPR, sub = lane / LPR;
    {
        const int r = blockIdx.x * kHeadRows + threadIdx.x;
        const int n = r < P ? r / HW : 0, q = r < P ? r - n * HW : 0;
        const bf16* g = dy + (size_t)n * K * HW + q;
#pragma unroll
        for (int k = 0; k < K; ++k) s_dy[k][threadIdx.x] = r < P ? __bfloat162float(g[(size_t)k * HW]) : 0.f;
    }
    float wv[K][8], acc[K][8], dsum[K], sc[8], sh[8];
#pragma unroll
    for (int k = 0; k < K; ++k) {
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            wv[k][i] = w[k * C + col * 8 + i];
            acc[k][i] = 0.f;
        }
        dsum[k] = 0.f;
    }
    const bool bn = bnst != nullptr;
    head_bn8(bnst, C, col * 8, sc, sh);
    const int l0 = wave * (kHeadRows / 4);
    const int r0 = blockIdx.x * kHeadRows + l0;
    __syncthreads();
#pragma unroll 2
    for (int it = 0; it < kHeadRows / 4 / RPI; ++it) {
        const int l = l0 + it * RPI + sub;
        const int r = r0 + it * RPI + sub;
        if (r < P) {
            float g[K];
#pragma unroll
            for (int k = 0; k < K; ++k) g[k] = s_dy[k][l];
            const uint4 v = x[(size_t)r * LPR + col];
            const unsigned u[4] = {v.x, v.y, v.z, v.w};
            unsigned o[4];
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const float lo = head_in(__uint_as_float(u[i] << 16), bn, sc[2 * i], sh[2 * i]);
                const float hi = head_in(__uint_as_float(u[i] & 0xFFFF0000u), bn, sc[2 * i + 1], sh[2 * i + 1]);
                float da = g[0] * wv[0][2 * i], dc = g[0] * wv[0][2 * i + 1];
#pragma unroll
                for (int k = 0; k < K; ++k) {
                    acc[k][2 * i] = fmaf(g[k], lo, acc[k][2 * i]);
                    acc[k][2 * i + 1] = fmaf(g[k], hi, acc[k][2 * i + 1]);
                    if (k > 0) {
                        da = fmaf(g[k], wv[k][2 * i], da);
                        dc = fmaf(g[k], wv[k][2 * i + 1], dc);
                    }
                }
                const bf16 a = __float2bfloat16(da), c = __float2bfloat16(dc);
                o[i] = (unsigned)*reinterpret_cast<const unsigned short*>(&a) |
                       ((unsigned)*reinterpret_cast<const unsigned short*>(&c) << 16);
            }
            dx[(size_t)r * LPR + col] = make_uint4(o[0], o[1], o[2], o[3]);
            if (col == 0) {
#pragma unroll
                for (int k = 0; k < K; ++k) dsum[k] += g[k];
            }
        }
    }
#pragma unroll
    for (int k = 0; k < K; ++k) {
#pragma unroll
        for (int i = 0; i < 8; ++i)
#pragma unroll
            for (int off = LPR; off < kWave; off <<= 1) acc[k][i] += __shfl_xor(acc[k][i], off, kWave);
#pragma unroll
        for (int off = LPR; off < kWave; off <<= 1) dsum[k] += __shfl_xor(dsum[k], off, kWave);
    }
    // the waves in order into one LDS copy, ((w0 + w1) + w2) + w3 as k_head1_bwd folds its four
    for (int v = 0; v < kBlock / kWave; ++v) {
        if (wave == v && sub == 0) {
#pragma unroll
            for (int k = 0; k < K; ++k) {
#pragma unroll
                for (int i = 0; i < 8; ++i) {
                    float* p = &s_part[k][col * 8 + i];
                    *p = v == 0 ? acc[k][i] : *p + acc[k][i];
                }
                if (col == 0) s_part[k][C] = v == 0 ? dsum[k] : s_part[k][C] + dsum[k];
            }
        }
        __syncthreads();
    }
    for (int e = threadIdx.x; e < K * (C + 1); e += kBlock)
        partial[(size_t)blockIdx.x * K * (C + 1) + e] = (&s_part[0][0])[e];
}

}  // namespace

extern "C" {

int lss_head1_blocks(int32_t P) { return P > 0 ? (P + kHeadRows - 1) / kHeadRows : 0; }

int lss_head1_fwd(const void* x, const float* w, const float* bias, int32_t P, int32_t C, void* y, void* stream) {
    return lss_head1_fwd2(x, w, bias, P, C, nullptr, y, stream);
}
int lss_head1_fwd2(const void* x, const float* w, const float* bias, int32_t P, int32_t C, const float* bn_stats,
                   void* y, void* stream) {
    if (!x || !w || !y || P <= 0 || C <= 0 || C % 8 != 0 || 64 % (C / 8) != 0) return LSS_CONV_EINVAL;
    if (!aligned16(x) || (reinterpret_cast<uintptr_t>(y) & 1)) return LSS_CONV_EINVAL;  // uint4 rows; y by element
    const dim3 gr(lss_head1_blocks(P)), bl(kBlock);
    hipStream_t s = (hipStream_t)stream;
#define LSS_HEAD1_FWD(L) \
    hipLaunchKernelGGL((k_head1_fwd<L>), gr, bl, 0, s, (const uint4*)x, w, bias, P, (bf16*)y, bn_stats)
    switch (C / 8) {
        case 16: LSS_HEAD1_FWD(16); break;
        case 8: LSS_HEAD1_FWD(8); break;
        case 32: LSS_HEAD1_FWD(32); break;
        case 64: LSS_HEAD1_FWD(64); break;
        case 4: LSS_HEAD1_FWD(4); break;
        case 2: LSS_HEAD1_FWD(2); break;
        case 1: LSS_HEAD1_FWD(1); break;
        default: return LSS_CONV_EINVAL;
    }
#undef LSS_HEAD1_FWD
    return launch_status();
}
int lss_head1_bwd(const void* x, const void* dy, const float* w, int32_t P, int32_t C, void* dx, float* partial,
                  void* stream) {
    if (!dx) return LSS_CONV_EINVAL;
    return lss_head1_bwd2(x, dy, w, P, C, nullptr, dx, partial, stream);
}
int lss_head1_bwd2(const void* x, const void* dy, const float* w, int32_t P, int32_t C, const float* bn_stats, void* dx,
                   float* partial, void* stream) {
    if (!x || !dy || !w || (!dx && !bn_stats) || !partial || P <= 0 || C <= 0 || C % 8 != 0 || 64 % (C / 8) != 0)
        return LSS_CONV_EINVAL;
    if (!aligned16(x, dx) || (reinterpret_cast<uintptr_t>(dy) & 1)) return LSS_CONV_EINVAL;
    const dim3 gr(lss_head1_blocks(P)), bl(kBlock);
    hipStream_t s = (hipStream_t)stream;
#define LSS_HEAD1_BWD(L)                                                                                          \
    hipLaunchKernelGGL((k_head1_bwd<L>), gr, bl, 0, s, (const uint4*)x, (const bf16*)dy, w, P, (uint4*)dx, partial, \
                       bn_stats)
    switch (C / 8) {
        case 16: LSS_HEAD1_BWD(16); break;
        case 8: LSS_HEAD1_BWD(8); break;
        case 32: LSS_HEAD1_BWD(32); break;
        case 64: LSS_HEAD1_BWD(64); break;
        case 4: LSS_HEAD1_BWD(4); break;
        case 2: LSS_HEAD1_BWD(2); break;
        case 1: LSS_HEAD1_BWD(1); break;
        default: return LSS_CONV_EINVAL;
    }
#undef LSS_HEAD1_BWD
    return launch_status();
}

namespace {
bool headk_args_ok(int32_t P, int32_t HW, int32_t C, int32_t K) {
    return P > 0 && HW > 0 && P % HW == 0 && C > 0 && C % 8 == 0 && 64 % (C / 8) == 0 && K >= 2 && K <= 8;
}
// the <lanes per row, K> instance: LSS_HEADK(L, K) launches it
#define LSS_HEADK_K(L)          \
    switch (K) {                \
        case 2: LSS_HEADK(L, 2); break; \
        case 3: LSS_HEADK(L, 3); break; \
        case 4: LSS_HEADK(L, 4); break; \
        case 5: LSS_HEADK(L, 5); break; \
        case 6: LSS_HEADK(L, 6); break; \
        case 7: LSS_HEADK(L, 7); break; \
        default: LSS_HEADK(L, 8); break; \
    }
#define LSS_HEADK_DISPATCH()                  \
    switch (C / 8) {                          \
        case 16: LSS_HEADK_K(16); break;      \
        case 8: LSS_HEADK_K(8); break;        \
        case 32: LSS_HEADK_K(32); break;      \
        case 64: LSS_HEADK_K(64); break;      \
        case 4: LSS_HEADK_K(4); break;        \
        case 2: LSS_HEADK_K(2); break;        \
        case 1: LSS_HEADK_K(1); break;        \
        default: return LSS_CONV_EINVAL;      \
    }
}  // namespace

int lss_headk_fwd(const void* x, const float* w, const float* bias, int32_t P, int32_t HW, int32_t C, int32_t K,
                  const float* bn_stats, void* y, void* stream) {
    if (!x || !w || !y || !headk_args_ok(P, HW, C, K)) return LSS_CONV_EINVAL;
    if (!aligned16(x) || (reinterpret_cast<uintptr_t>(y) & 1)) return LSS_CONV_EINVAL;  // uint4 rows; y by element
    const dim3 gr(lss_head1_blocks(P)), bl(kBlock);
    hipStream_t s = (hipStream_t)stream;
#define LSS_HEADK(L, KK) \
    hipLaunchKernelGGL((k_headk_fwd<L, KK>), gr, bl, 0, s, (const uint4*)x, w, bias, P, HW, (bf16*)y, bn_stats)
    LSS_HEADK_DISPATCH()
#undef LSS_HEADK
    return launch_status();
}
int lss_headk_bwd(const void* x, const void* dy, const float* w, int32_t P, int32_t HW, int32_t C, int32_t K,
                  const float* bn_stats, void* dx, float* partial, void* stream) {
    if (!x || !dy || !w || !dx || !partial || !headk_args_ok(P, HW, C, K)) return LSS_CONV_EINVAL;
    if (!aligned16(x, dx) || (reinterpret_cast<uintptr_t>(dy) & 1)) return LSS_CONV_EINVAL;
    const dim3 gr(lss_head1_blocks(P)), bl(kBlock);
    hipStream_t s = (hipStream_t)stream;
#define LSS_HEADK(L, KK)                                                                                             \
    hipLaunchKernelGGL((k_headk_bwd<L, KK>), gr, bl, 0, s, (const uint4*)x, (const bf16*)dy, w, P, HW, (uint4*)dx, \
                       partial, bn_stats)
    LSS_HEADK_DISPATCH()
#undef LSS_HEADK
    return launch_status();
}
#undef LSS_HEADK_DISPATCH
#undef LSS_HEADK_K

}  // extern "C"
