// lss_pointwise.hip -- 1x1 convolution weight gradient over NCHW activations (the MBConv expand / project convs of
// the trunk, src/models.py:43 via efficientnet_pytorch): dW[co][ci] = sum over images n and pixels q
// of dy[n][co][q] * x[n][ci][q]. A GEMM whose K index (n, q) runs along q in BOTH operands, so the
// v_mfma_f32_16x16x32_bf16 fragments (8 consecutive k per lane) load straight from global memory --
// no LDS staging, no transposes, no fp32 workspace to zero and cast (MIOpen's atomic NHWC solver
// needs both, plus NCHW <-> NHWC transposes). Block = 64 x 64 dW tile x one K range (a split); its
// 4 waves take the range's 32-wide K steps in turn, double-buffered (the next step's 8 fragment loads
// in flight behind the current step's 16 MFMAs), and are summed in LDS in a fixed order; the splits'
// partials are summed by k_pw_wrw_reduce in split order (deterministic).

#include <algorithm>
#include <limits.h>

#include "lss_convs.h"
#include "lss_device.h"

// The library is built with -ffp-contract=off for the geometry's reference op order (lss_hip.hip);
// the conv-stack kernels here have no bit-exact contract, so they keep FMA contraction.
#pragma clang fp contract(fast)

namespace {

constexpr int kPwWaves = 4;
constexpr int kPwThreads = kPwWaves * kWave;

using pw_bf16x8 = __attribute__((ext_vector_type(8))) short;
using pw_f32x4 = __attribute__((ext_vector_type(4))) float;

// A lane's fragment of one K step: KS consecutive k (8 or 16) of one row, as KS / 8 MFMA operands. Any
// assignment of k to MFMA slots is a valid GEMM as long as A and B use the same one, so with KS = 16
// a lane's 32 contiguous bytes feed two MFMAs and a row's 4 lanes read one whole 128-B line.
template <int VEC, int KS>  // VEC 8: 16-B loads (HW % 8 == 0); VEC 4: 8-B loads (HW % 4 == 0)
struct PwFrag {
    pw_bf16x8 v[KS / 8];
};

template <int VEC, int KS>
__device__ __forceinline__ PwFrag<VEC, KS> pw_frag(const bf16* __restrict__ p, int q, int HW, bool live) {
    PwFrag<VEC, KS> f;
#pragma unroll
    for (int h = 0; h < KS / 8; ++h) {
        if constexpr (VEC == 8) {
            const bool ok = live && q + 8 * h < HW;
            const uint4 v = ok ? *reinterpret_cast<const uint4*>(p + 8 * h) : make_uint4(0u, 0u, 0u, 0u);
            f.v[h] = __builtin_bit_cast(pw_bf16x8, v);
        } else {
            const bool ok0 = live && q + 8 * h < HW, ok1 = live && q + 8 * h + 4 < HW;
            const uint2 lo = ok0 ? *reinterpret_cast<const uint2*>(p + 8 * h) : make_uint2(0u, 0u);
            const uint2 hi = ok1 ? *reinterpret_cast<const uint2*>(p + 8 * h + 4) : make_uint2(0u, 0u);
            f.v[h] = __builtin_bit_cast(pw_bf16x8, make_uint4(lo.x, lo.y, hi.x, hi.y));
        }
    }
    return f;
}

template <int VEC, int KS>
__global__ __launch_bounds__(kPwThreads) void k_pw_wrw(const bf16* __restrict__ x, const bf16* __restrict__ dy,
                                                      int Cin, int Cout, int HW, int spi, int nsteps, int tiles_n,
                                                      int ntiles, int nsplit, float* __restrict__ partial) {
    constexpr int SW = 4 * KS;                // k per step: 4 lane groups x KS
    __shared__ pw_f32x4 s_red[2][16][kWave];  // two waves' 64 x 64 tiles (16 fragments x 64 lanes)
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    // XCD-contiguous logical block: consecutive tiles of one split (one K range, whose activation rows
    // the tiles share) run on one XCD and meet in its L2
    const int bpx = gridDim.x >> 3;
    const int lb = (blockIdx.x & 7) * bpx + (blockIdx.x >> 3);
    const int split = lb / ntiles, tile = lb - split * ntiles;
    if (split >= nsplit) return;  // block-uniform (grid padded to a multiple of 8)
    const int m0 = (tile / tiles_n) * 64, n0 = (tile % tiles_n) * 64;
    const int fm = min(4, (Cout - m0 + 15) >> 4), fn = min(4, (Cin - n0 + 15) >> 4);  // live 16-row fragments
    const int t0 = (int)((long long)nsteps * split / nsplit), t1 = (int)((long long)nsteps * (split + 1) / nsplit);
    const int r16 = lane & 15, kq = KS * (lane >> 4);
    int arow[4], brow[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        arow[i] = min(m0 + 16 * i + r16, Cout - 1);  // clamped rows feed only discarded outputs
        brow[i] = min(n0 + 16 * i + r16, Cin - 1);
    }
    pw_f32x4 acc[4][4];
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[i][j] = pw_f32x4{0.f, 0.f, 0.f, 0.f};
    PwFrag<VEC, KS> a[2][4], b[2][4];
    auto load = [&](int t, PwFrag<VEC, KS>* av, PwFrag<VEC, KS>* bv) {
        const bool live = t < t1;
        t = min(t, nsteps - 1);
        const int n = t / spi;
        const int q = (t - n * spi) * SW + kq;
        const int qq = q < HW ? q : 0;  // (masked halves read nothing; the address stays in the tensor)
        const bf16* ap = dy + (size_t)n * Cout * HW + qq;
        const bf16* bp = x + (size_t)n * Cin * HW + qq;
#pragma unroll
        for (int i = 0; i < 4; ++i)
            if (i < fm) av[i] = pw_frag<VEC, KS>(ap + (size_t)arow[i] * HW, q, HW, live);
#pragma unroll
        for (int j = 0; j < 4; ++j)
            if (j < fn) bv[j] = pw_frag<VEC, KS>(bp + (size_t)brow[j] * HW, q, HW, live);
    };
    auto mma = [&](const PwFrag<VEC, KS>* av, const PwFrag<VEC, KS>* bv) {
#pragma unroll
        for (int h = 0; h < KS / 8; ++h)
#pragma unroll
            for (int i = 0; i < 4; ++i)
#pragma unroll
                for (int j = 0; j < 4; ++j)
                    if (i < fm && j < fn)
                        acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(av[i].v[h], bv[j].v[h], acc[i][j], 0, 0, 0);
    };
    int t = t0 + wave;
    if (t < t1) load(t, a[0], b[0]);
    for (; t < t1; t += 2 * kPwWaves) {
        load(t + kPwWaves, a[1], b[1]);  // (past t1: zeros)
        mma(a[0], b[0]);
        if (t + kPwWaves >= t1) break;
        load(t + 2 * kPwWaves, a[0], b[0]);
        mma(a[1], b[1]);
    }
    // waves (0 + 2) and (1 + 3) in LDS, then every wave sums the two for its 16-row block
    if (wave >= 2) {
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
            for (int j = 0; j < 4; ++j) s_red[wave - 2][4 * i + j][lane] = acc[i][j];
    }
    __syncthreads();
    if (wave < 2) {
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
            for (int j = 0; j < 4; ++j) s_red[wave][4 * i + j][lane] += acc[i][j];
    }
    __syncthreads();
    const int i = wave;  // this wave writes rows m0 + 16 i + 4 (lane >> 4) + r
    if (i >= fm) return;
    float* out = partial + (size_t)split * Cout * Cin;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int ci = n0 + 16 * j + r16;
        if (j >= fn || ci >= Cin) continue;
        const pw_f32x4 v = s_red[0][4 * i + j][lane] + s_red[1][4 * i + j][lane];
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int co = m0 + 16 * i + 4 * (lane >> 4) + r;
            if (co < Cout) out[(size_t)co * Cin + ci] = v[r];
        }
    }
}

// ---- 1x1 convolution forward / backward-data over NCHW bf16 activations (the trunk's MBConv expand /
// project convs): Y[n][m][p] = sum_k A[m][k] X[n][k][p], A = W (forward, [m][k]) or W^T (backward-data,
// W given as [k][m]). MIOpen runs these as batched GEMMs of one image each (15-50 us per layer at c3).
// Here the MFMA rows are PIXELS: D[px][m] = sum_k X^T[px][k] A^T[k][m], so a lane's 4 accumulators are 4
// consecutive pixels of one channel (one 8-B store). Block = 64 pixels (flattened over images) x 64
// channels, 4 waves of 16 channels; the X tile (KC k x 64 px) is staged in LDS as it lies in memory and
// read transposed by ds_read_tr16_b64 (8 consecutive k of one pixel per lane); A comes straight from
// global ([m][k] rows, forward) or through a second LDS tile ([k][m] rows, backward-data). The next
// stage's global loads are in flight while the current stage's MFMAs run.
constexpr int kPgPx = 64, kPgM = 64;
constexpr int kPgRow = kPgPx * 2 + 8;  // LDS bytes per staged k row (+8: spread the banks)

template <int VEC, bool WT, int KC>  // VEC: pixels per X load (8: P % 8 == 0, else 4); WT: A given as [k][m]
__global__ __launch_bounds__(256) void k_pw_gemm(const bf16* __restrict__ X, const bf16* __restrict__ A, int M, int K,
                                                 int P, int ncols, int mtiles, bf16* __restrict__ Y) {
    using v4s = __attribute__((ext_vector_type(4))) short;
    constexpr int XL = KC * (kPgPx / VEC) / 256;            // X loads per thread per stage
    constexpr int WL = WT ? KC * (kPgM / 8) / 256 : KC / 32;  // A loads per thread (WT) / per lane (forward)
    static_assert(XL >= 1 && WL >= 1, "whole loads per thread");
    __shared__ __attribute__((aligned(16))) unsigned char s_x[KC * kPgRow];
    __shared__ __attribute__((aligned(16))) unsigned char s_w[WT ? KC * kPgRow : 16];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int c16 = lane & 15, g = lane >> 4, tq = c16 >> 2, tp = c16 & 3;
    // XCD-contiguous logical block, m-tiles fastest: the m-tiles of one pixel tile (same X rows) share an L2
    const int bpx = gridDim.x >> 3;
    const int lb = (blockIdx.x & 7) * bpx + (blockIdx.x >> 3);
    const int mt = lb % mtiles, jt = lb / mtiles;
    const int j0 = jt * kPgPx, m0 = mt * kPgM;
    if (j0 >= ncols) return;  // block-uniform (grid padded to a multiple of 8)
    // this thread's X chunks: (row, pixel chunk) -> global address (pixels of a chunk never straddle images)
    const uint2 z2 = make_uint2(0u, 0u);
    uint4 xr[XL];
    uint2 xr2[XL];
    uint4 wr[WL], wcur[WT ? 1 : WL];
    auto gload = [&](int kb) {
#pragma unroll
        for (int i = 0; i < XL; ++i) {
            const int c = threadIdx.x + 256 * i;
            const int row = c / (kPgPx / VEC), ch = c - row * (kPgPx / VEC);
            const int col = j0 + ch * VEC, k = kb + row;
            const bool ok = col < ncols && k < K;
            const int n = ok ? col / P : 0, pp = ok ? col - n * P : 0;
            const bf16* src = X + ((size_t)n * K + (ok ? k : 0)) * P + pp;
            if constexpr (VEC == 8) xr[i] = ok ? *reinterpret_cast<const uint4*>(src) : make_uint4(0u, 0u, 0u, 0u);
            else xr2[i] = ok ? *reinterpret_cast<const uint2*>(src) : z2;
        }
        if constexpr (WT) {  // A^T tile rows k, 64 channels each: A[k][m0 .. m0 + 63], 8 per load (M % 8 == 0)
#pragma unroll
            for (int i = 0; i < WL; ++i) {
                const int c = threadIdx.x + 256 * i;
                const int row = c >> 3, ch = c & 7;
                const int k = kb + row, m = m0 + 8 * ch;
                wr[i] = (k < K && m < M) ? *reinterpret_cast<const uint4*>(A + (size_t)k * M + m) : make_uint4(0u, 0u, 0u, 0u);
            }
        } else {  // forward: this lane's B fragments straight from A's rows (K % 8 == 0)
            const int m = m0 + 16 * wave + c16;
#pragma unroll
            for (int i = 0; i < WL; ++i) {
                const int k = kb + 32 * i + 8 * g;
                wr[i] = (m < M && k < K) ? *reinterpret_cast<const uint4*>(A + (size_t)m * K + k) : make_uint4(0u, 0u, 0u, 0u);
            }
        }
    };
    auto lstore = [&]() {
#pragma unroll
        for (int i = 0; i < XL; ++i) {
            const int c = threadIdx.x + 256 * i;
            const int row = c / (kPgPx / VEC), ch = c - row * (kPgPx / VEC);
            if constexpr (VEC == 8) *reinterpret_cast<uint4*>(s_x + row * kPgRow + ch * 16) = xr[i];
            else *reinterpret_cast<uint2*>(s_x + row * kPgRow + ch * 8) = xr2[i];
        }
        if constexpr (WT) {
#pragma unroll
            for (int i = 0; i < WL; ++i) {
                const int c = threadIdx.x + 256 * i;
                *reinterpret_cast<uint4*>(s_w + (c >> 3) * kPgRow + (c & 7) * 16) = wr[i];
            }
        } else {
#pragma unroll
            for (int i = 0; i < WL; ++i) wcur[i] = wr[i];
        }
    };
    auto tr8 = [&](const unsigned char* s, int step, int col0) {  // 8 consecutive k (step) of column col0 + c16
        const unsigned char* base = s + (32 * step + 8 * g + tq) * kPgRow + (col0 + 4 * tp) * 2;
        const v4s lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) v4s*)(base));
        const v4s hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) v4s*)(base + 4 * kPgRow));
        return pw_bf16x8{lo.x, lo.y, lo.z, lo.w, hi.x, hi.y, hi.z, hi.w};
    };
    pw_f32x4 acc[4];
#pragma unroll
    for (int t = 0; t < 4; ++t) acc[t] = pw_f32x4{0.f, 0.f, 0.f, 0.f};
    gload(0);
    for (int kb = 0; kb < K; kb += KC) {
        __syncthreads();  // the previous stage's reads of s_x / s_w are done
        lstore();
        __syncthreads();
        if (kb + KC < K) gload(kb + KC);  // in flight behind this stage's MFMAs
#pragma unroll
        for (int st = 0; st < KC / 32; ++st) {
            if (kb + 32 * st >= K) break;
            pw_bf16x8 b;
            if constexpr (WT) b = tr8(s_w, st, 16 * wave);
            else b = __builtin_bit_cast(pw_bf16x8, wcur[st]);
#pragma unroll
            for (int t = 0; t < 4; ++t) acc[t] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(tr8(s_x, st, 16 * t), b, acc[t], 0, 0, 0);
        }
    }
    // D[px][m]: this lane holds channel m0 + 16 wave + c16, pixels 16 t + 4 g + 0..3
    const int m = m0 + 16 * wave + c16;
    if (m >= M) return;
#pragma unroll
    for (int t = 0; t < 4; ++t) {
        const int col = j0 + 16 * t + 4 * g;
        if (col >= ncols) continue;
        const int n = col / P, pp = col - n * P;
        *reinterpret_cast<uint2*>(Y + ((size_t)n * M + m) * P + pp) =
            make_uint2(pack2(acc[t][0], acc[t][1]), pack2(acc[t][2], acc[t][3]));
    }
}

// dw[e] = sum over splits s (in order) of partial[s][e], nsplit <= kPwMaxSplit. Four consecutive
// elements per lane (16-B loads); the splits of a lane's elements are shared by G waves of the block
// (G = 1 for nsplit <= 16, else 16), each summing its run of <= 16 consecutive splits with every
// load in flight at once, then the G sums in order.
constexpr int kPwMaxSplit = 256;
template <typename T, int G>
__global__ __launch_bounds__(G == 1 ? 256 : 1024) void k_pw_wrw_reduce(const float* __restrict__ partial, int nsplit,
                                                                       int E, T* __restrict__ dw) {
    constexpr int kThreads = G == 1 ? 256 : 1024;
    __shared__ float4 s_sum[G][kWave];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int chunk = G == 1 ? blockIdx.x * (kThreads / kWave) + wave : blockIdx.x;  // 64 lanes x 4 elements
    const int e = (chunk * kWave + lane) * 4;
    const int gw = G == 1 ? 0 : wave;
    const int per = (nsplit + G - 1) / G, s0 = gw * per, s1 = min(s0 + per, nsplit);
    float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
    if (e < E) {
        float4 p[16];
#pragma unroll
        for (int k = 0; k < 16; ++k) {
            if (s0 + k < s1) {
                const float* src = partial + (size_t)(s0 + k) * E + e;
                p[k] = (E & 3) == 0 ? *reinterpret_cast<const float4*>(src)  // (16-B aligned rows)
                                    : make_float4(src[0], e + 1 < E ? src[1] : 0.f, e + 2 < E ? src[2] : 0.f,
                                                  e + 3 < E ? src[3] : 0.f);
            } else {
                p[k] = make_float4(0.f, 0.f, 0.f, 0.f);
            }
        }
#pragma unroll
        for (int k = 0; k < 16; ++k) {
            v.x += p[k].x;
            v.y += p[k].y;
            v.z += p[k].z;
            v.w += p[k].w;
        }
    }
    if constexpr (G > 1) {
        s_sum[wave][lane] = v;
        __syncthreads();
        if (wave != 0) return;
        v = make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll
        for (int w = 0; w < G; ++w) {
            const float4 t = s_sum[w][lane];
            v.x += t.x;
            v.y += t.y;
            v.z += t.z;
            v.w += t.w;
        }
    }
    if (e >= E) return;
    const float o[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
    for (int k = 0; k < 4; ++k)
        if (e + k < E) st(dw + e + k, o[k]);
}

}  // namespace

extern "C" {

// split count of lss_pw_wrw: about 512 blocks (2 per CU) and >= 2 K steps per wave, at most
// kPwMaxSplit, and the fp32 partials at most half the activation bytes (or one split)
static void pw_plan(int N, int Cin, int Cout, int HW, int* spi, int* nsteps, int* tiles_n, int* ntiles, int* nsplit) {
    *spi = (HW + 63) / 64;
    *nsteps = N * *spi;
    *tiles_n = (Cin + 63) / 64;
    *ntiles = ((Cout + 63) / 64) * *tiles_n;
    long s = (512 + *ntiles - 1) / *ntiles;
    s = std::min(s, (long)std::max(1, *nsteps / (2 * kPwWaves)));
    const long in_bytes = 2L * N * HW * (Cin + Cout), per_split = 4L * Cin * Cout;
    s = std::min(s, std::max(1L, in_bytes / (2 * per_split)));
    *nsplit = (int)std::max(1L, std::min(s, (long)kPwMaxSplit));
}

int64_t lss_pw_wrw_workspace_bytes(int32_t N, int32_t Cin, int32_t Cout, int32_t HW) {
    if (N <= 0 || Cin <= 0 || Cout <= 0 || HW <= 0) return 0;
    int spi, nsteps, tiles_n, ntiles, nsplit;
    pw_plan(N, Cin, Cout, HW, &spi, &nsteps, &tiles_n, &ntiles, &nsplit);
    return (int64_t)nsplit * Cout * Cin * (int64_t)sizeof(float);
}

int lss_pw_wrw(const void* x, const void* dy, int32_t N, int32_t Cin, int32_t Cout, int32_t HW, void* dw,
               int32_t dw_dtype, void* workspace, int64_t workspace_bytes, void* stream) {
    if (!x || !dy || !dw || !workspace || N <= 0 || Cin <= 0 || Cout <= 0 || HW <= 0 || HW % 4 != 0 ||
        (dw_dtype != LSS_CONV_F32 && dw_dtype != LSS_CONV_BF16) || (long)N * ((HW + 31) / 32) >= INT_MAX ||
        (long)N * std::max(Cin, Cout) * HW >= INT_MAX ||
        ((reinterpret_cast<uintptr_t>(x) | reinterpret_cast<uintptr_t>(dy)) & 7) ||
        workspace_bytes < lss_pw_wrw_workspace_bytes(N, Cin, Cout, HW))
        return LSS_CONV_EINVAL;
    int spi, nsteps, tiles_n, ntiles, nsplit;
    pw_plan(N, Cin, Cout, HW, &spi, &nsteps, &tiles_n, &ntiles, &nsplit);
    const long blocks = 8L * (((long)ntiles * nsplit + 7) / 8);
    hipStream_t s = (hipStream_t)stream;
    float* part = (float*)workspace;
    const bool v8 = HW % 8 == 0 && ((reinterpret_cast<uintptr_t>(x) | reinterpret_cast<uintptr_t>(dy)) & 15) == 0;
    if (v8)
        hipLaunchKernelGGL((k_pw_wrw<8, 16>), dim3((unsigned)blocks), dim3(kPwThreads), 0, s, (const bf16*)x,
                           (const bf16*)dy, Cin, Cout, HW, spi, nsteps, tiles_n, ntiles, nsplit, part);
    else
        hipLaunchKernelGGL((k_pw_wrw<4, 16>), dim3((unsigned)blocks), dim3(kPwThreads), 0, s, (const bf16*)x,
                           (const bf16*)dy, Cin, Cout, HW, spi, nsteps, tiles_n, ntiles, nsplit, part);
    const int E = Cout * Cin;
    const int chunks = (E + 4 * kWave - 1) / (4 * kWave);  // 64 lanes x 4 elements
#define LSS_PW_REDUCE(T)                                                                                          \
    if (nsplit <= 16)                                                                                             \
        hipLaunchKernelGGL((k_pw_wrw_reduce<T, 1>), dim3((chunks + 3) / 4), dim3(256), 0, s, (const float*)part,  \
                           nsplit, E, (T*)dw);                                                                    \
    else                                                                                                          \
        hipLaunchKernelGGL((k_pw_wrw_reduce<T, 16>), dim3(chunks), dim3(1024), 0, s, (const float*)part, nsplit, E, \
                           (T*)dw)
    if (dw_dtype == LSS_CONV_BF16) {
        LSS_PW_REDUCE(bf16);
    } else {
        LSS_PW_REDUCE(float);
    }
#undef LSS_PW_REDUCE
    return launch_status();
}

int lss_pw_conv(const void* x, const void* a, int32_t a_layout, int32_t N, int32_t K, int32_t M, int32_t HW, void* y,
                void* stream) {
    if (!x || !a || !y || N <= 0 || K <= 0 || M <= 0 || HW <= 0 || HW % 4 != 0 || K % 8 != 0 || M % 8 != 0 ||
        (a_layout != LSS_PW_MK && a_layout != LSS_PW_KM) || (long)N * HW >= INT_MAX ||
        (long)N * std::max(K, M) * HW >= INT_MAX ||
        ((reinterpret_cast<uintptr_t>(x) | reinterpret_cast<uintptr_t>(y) | reinterpret_cast<uintptr_t>(a)) & 15))
        return LSS_CONV_EINVAL;
    const int ncols = N * HW, mtiles = (M + kPgM - 1) / kPgM;
    const long tiles = (long)mtiles * ((ncols + kPgPx - 1) / kPgPx);
    const long blocks = 8L * ((tiles + 7) / 8);
    if (blocks > INT_MAX) return LSS_CONV_EINVAL;
    hipStream_t s = (hipStream_t)stream;
    const bool v8 = HW % 8 == 0, wt = a_layout == LSS_PW_KM, small = K <= 64;
#define LSS_PW_GEMM(V, W, KC)                                                                                      \
    hipLaunchKernelGGL((k_pw_gemm<V, W, KC>), dim3((unsigned)blocks), dim3(256), 0, s, (const bf16*)x, (const bf16*)a, \
                       M, K, HW, ncols, mtiles, (bf16*)y)
    if (v8) {
        if (wt) { if (small) LSS_PW_GEMM(8, true, 32); else LSS_PW_GEMM(8, true, 128); }
        else { if (small) LSS_PW_GEMM(8, false, 32); else LSS_PW_GEMM(8, false, 128); }
    } else {
        if (wt) { if (small) LSS_PW_GEMM(4, true, 32); else LSS_PW_GEMM(4, true, 128); }
        else { if (small) LSS_PW_GEMM(4, false, 32); else LSS_PW_GEMM(4, false, 128); }
    }
#undef LSS_PW_GEMM
    return launch_status();
}

}  // extern "C"
