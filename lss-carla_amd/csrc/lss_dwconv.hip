// lss_dwconv.hip -- gfx950 kernels for the conv stack in front of the Lift-Splat hot path: the
// depthwise convolutions of CamEncode's EfficientNet-B0 trunk (src/models.py:43, 63-84; 16 MBConv
// blocks, 3x3 / 5x5, stride 1 / 2, TF "same" padding). MIOpen has no bf16 NCHW depthwise solver and
// falls back to naive kernels (≈5 ms of a 27 ms training step at config 3).
//
// NCHW planes, fp32 accumulation, activations fp32 or bf16, weights fp32 (the parameter itself: no
// per-step cast, and the weight gradient stays fp32).
//
// Forward / stride-1 backward-data: a thread owns a strip of TH output rows of one column; lanes run
// along the row, so every input-row load instruction of a wave is contiguous, and each input row
// loaded into registers feeds every output of the strip it overlaps. Index math is 32-bit (element
// counts are checked < 2^31); a wave whose lanes share one channel reads the weights with scalar
// loads. Stride-1 backward-data is the
// forward correlation with the kernel flipped and the padding mirrored. Stride-2 backward-data: a
// thread per 2 x 4 input elements with compile-time tap offsets. Backward-weight: a block per (channel, group
// of images) accumulates the K*K tap sums of its elements in registers, reduces them over the block
// in a fixed order and writes one partial per group; the caller sums the groups.

#include <algorithm>
#include <limits.h>

#include "lss_convs.h"
#include "lss_device.h"

// The library is built with -ffp-contract=off for the geometry's reference op order (lss_hip.hip);
// the conv-stack kernels here have no bit-exact contract, so they keep FMA contraction.
#pragma clang fp contract(fast)

namespace {

constexpr int kBlock = 256;
// output tile per thread (rows x columns)
template <int S> struct Tile { static constexpr int TH = S == 1 ? 8 : 4, TW = S == 1 ? 4 : 2; };

struct DwGeo {
    int C, Hi, Wi, Ho, Wo, pt, pl, nplanes;  // input (Hi, Wi) -> output (Ho, Wo); nplanes = N * C
};

// Weights of channel c for a wave: when every lane of the wave works on the same channel (planes
// of >= 64 outputs per row strip), the channel index is wave-uniform and the weights come in with
// scalar loads (SGPR operands of the FMAs); otherwise per lane.
template <int K, typename F>
__device__ __forceinline__ void with_weights(const float* __restrict__ w, int c, bool flip, F&& body) {
    const int cu = __builtin_amdgcn_readfirstlane(c);
    if (__ballot(c != cu) == 0) {
        const float* wc = w + (size_t)cu * K * K;
        float wk[K * K];
#pragma unroll
        for (int i = 0; i < K * K; ++i) wk[i] = wc[flip ? K * K - 1 - i : i];
        body(wk);
    } else {
        const float* wc = w + (size_t)c * K * K;
        float wk[K * K];
#pragma unroll
        for (int i = 0; i < K * K; ++i) wk[i] = wc[flip ? K * K - 1 - i : i];
        body(wk);
    }
}

// y[p][oh][ow] = sum_{kh, kw} x[p][oh*S - pt + kh][ow*S - pl + kw] * w[c][kh][kw] (zero outside x);
// flip: w[c][K-1-kh][K-1-kw] (stride-1 backward-data). Thread = (plane, TH x TW output tile): each
// input row segment it loads ((TW-1)*S + K values) feeds every output of the tile under it.
template <int K, int S, int TH, int TW, typename T>
__global__ __launch_bounds__(kBlock) void k_dw_fwd(const T* __restrict__ x, const float* __restrict__ w, DwGeo g,
                                                   int flip, T* __restrict__ y) {
    const int t = blockIdx.x * kBlock + threadIdx.x;
    const int ncol = (g.Wo + TW - 1) / TW, nrow = (g.Ho + TH - 1) / TH;
    const int per_plane = nrow * ncol;
    const bool live = t < g.nplanes * per_plane;
    const int plane = live ? t / per_plane : 0;
    const int rem = t - plane * per_plane;
    const int tr = rem / ncol, tc = rem - tr * ncol;
    const int c = plane % g.C;
    const int oh0 = tr * TH, ow0 = tc * TW;
    const int ih0 = oh0 * S - g.pt, iw0 = ow0 * S - g.pl;
    const T* xp = x + (size_t)plane * g.Hi * g.Wi;
    with_weights<K>(w, c, flip != 0, [&](const float* wk) {
        if (!live) return;
        float acc[TH][TW];
#pragma unroll
        for (int i = 0; i < TH; ++i)
#pragma unroll
            for (int j = 0; j < TW; ++j) acc[i][j] = 0.f;
        constexpr int R = (TH - 1) * S + K, CW = (TW - 1) * S + K;
#pragma unroll
        for (int rr = 0; rr < R; ++rr) {
            const int ih = ih0 + rr;
            const bool row_ok = ih >= 0 && ih < g.Hi;
            float v[CW];
#pragma unroll
            for (int q = 0; q < CW; ++q) {
                const int iw = iw0 + q;
                v[q] = (row_ok && iw >= 0 && iw < g.Wi) ? ld(xp + ih * g.Wi + iw) : 0.f;
            }
#pragma unroll
            for (int i = 0; i < TH; ++i) {
                const int kh = rr - i * S;
                if (kh >= 0 && kh < K) {
#pragma unroll
                    for (int j = 0; j < TW; ++j)
#pragma unroll
                        for (int kw = 0; kw < K; ++kw) acc[i][j] = fmaf(v[j * S + kw], wk[kh * K + kw], acc[i][j]);
                }
            }
        }
        T* yp = y + (size_t)plane * g.Ho * g.Wo;
#pragma unroll
        for (int i = 0; i < TH; ++i)
#pragma unroll
            for (int j = 0; j < TW; ++j)
                if (oh0 + i < g.Ho && ow0 + j < g.Wo) st(yp + (oh0 + i) * g.Wo + ow0 + j, acc[i][j]);
    });
}

// Stride-2 backward-data. Thread = 2 rows x 4 columns of dx: ih = 2m + a, iw = 4j + b. With
// pt = 2 PT2 + PT1, pl = 2 PL2 + PL1 (PT1, PL1 template parameters) the taps that reach dx[ih][iw]
// have kh = a + PT1 (mod 2), kw = b + PL1 (mod 2), at dy[m + PT2 + (a + PT1 - kh) / 2]
// [2j + PL2 + (b + PL1 - kw) / 2]: every offset is a compile-time constant, so the thread loads one
// small dy window and runs straight-line FMAs. g describes the forward conv.
template <int K, int PT1, int PL1, typename T>
__global__ __launch_bounds__(kBlock) void k_dw_bwd_data_s2(const T* __restrict__ dy, const float* __restrict__ w,
                                                           DwGeo g, T* __restrict__ dx) {
    constexpr int H0 = -(K - 1) / 2, H1 = 1;      // dy row offsets reached (relative to m + PT2)
    constexpr int W0 = -(K - 1) / 2, W1 = 2;      // dy column offsets reached (relative to 2j + PL2)
    const int t = blockIdx.x * kBlock + threadIdx.x;
    const int ncol = (g.Wi + 3) / 4, nrow = (g.Hi + 1) / 2;
    const int per_plane = nrow * ncol;
    const bool live = t < g.nplanes * per_plane;
    const int plane = live ? t / per_plane : 0;
    const int rem = t - plane * per_plane;
    const int m = rem / ncol, j = rem - m * ncol;
    const int c = plane % g.C;
    const int hb = m + (g.pt >> 1), wb = 2 * j + (g.pl >> 1);
    const T* dp = dy + (size_t)plane * g.Ho * g.Wo;
    with_weights<K>(w, c, false, [&](const float* wk) {
        if (!live) return;
        float win[H1 - H0 + 1][W1 - W0 + 1];
#pragma unroll
        for (int r = H0; r <= H1; ++r) {
            const int oh = hb + r;
#pragma unroll
            for (int q = W0; q <= W1; ++q) {
                const int ow = wb + q;
                win[r - H0][q - W0] = (oh >= 0 && oh < g.Ho && ow >= 0 && ow < g.Wo) ? ld(dp + oh * g.Wo + ow) : 0.f;
            }
        }
        T* xp = dx + (size_t)plane * g.Hi * g.Wi;
#pragma unroll
        for (int a = 0; a < 2; ++a) {
#pragma unroll
            for (int b = 0; b < 4; ++b) {
                float acc = 0.f;
#pragma unroll
                for (int kh = (a + PT1) & 1; kh < K; kh += 2)
#pragma unroll
                    for (int kw = (b + PL1) & 1; kw < K; kw += 2)
                        acc = fmaf(win[(a + PT1 - kh) / 2 - H0][(b + PL1 - kw) / 2 - W0], wk[kh * K + kw], acc);
                const int ih = 2 * m + a, iw = 4 * j + b;
                if (ih < g.Hi && iw < g.Wi) st(xp + ih * g.Wi + iw, acc);
            }
        }
    });
}

// Weight-gradient fold (optional, DwFold.sync != NULL): the ngroups partials of a channel are summed by the
// LAST of its blocks to finish, in group order, into dw[c][tap] -- the separate fold launch (a torch sum,
// 5-8 us at c3) is gone. Hand-off as the batch-norm cluster kernels': the partials written through with
// agent-scope stores and retired (vmcnt counts stores) before the agent-scope counter add; the last block
// reads them with agent-scope loads and re-zeroes the counter. Nothing waits, so nothing can stall. The
// counter of channel c is word c * kDwSyncStride + 2 of the batch-norm sync workspace (lss_bn_sync_words:
// zero-filled, left zero-filled by every user; words 0 and 1 of a channel's line are the BN clusters').
struct DwFold {
    unsigned* sync;
    float* dw;
};
constexpr int kDwSyncStride = 32;
constexpr int kDwSyncMaxC = 4096;
template <int KK>
__device__ __forceinline__ void dw_finish(float* __restrict__ partial, int c, int q, int ngroups, float v,
                                          const DwFold& f) {
    const int t = threadIdx.x;
    const size_t base = (size_t)c * ngroups * KK;
    if (!f.sync) {
        if (t < KK) partial[base + (size_t)q * KK + t] = v;
        return;
    }
    if (ngroups == 1) {  // the block is the channel: no hand-off
        if (t < KK) f.dw[(size_t)c * KK + t] = v;
        return;
    }
    if (t >= kWave) return;  // wave 0 (KK <= 25 lanes hold the block's values)
    unsigned* pu = reinterpret_cast<unsigned*>(partial);
    if (t < KK) __hip_atomic_store(pu + base + (size_t)q * KK + t, __float_as_uint(v), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    __builtin_amdgcn_s_waitcnt(0x0F70);  // vmcnt(0): this wave's partial stores retired
    unsigned* ctr = f.sync + (size_t)c * kDwSyncStride + 2;
    int last = 0;
    if (t == 0) last = __hip_atomic_fetch_add(ctr, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == (unsigned)ngroups - 1u;
    last = __shfl(last, 0, kWave);
    if (!last) return;
    // lanes over groups (each lane's KK partials loaded together), then a butterfly per tap: fixed order
    float a[KK];
#pragma unroll
    for (int k = 0; k < KK; ++k) a[k] = 0.f;
    for (int qq = t; qq < ngroups; qq += kWave) {
        unsigned u[KK];
#pragma unroll
        for (int k = 0; k < KK; ++k)
            u[k] = __hip_atomic_load(pu + base + (size_t)qq * KK + k, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
#pragma unroll
        for (int k = 0; k < KK; ++k) a[k] += __uint_as_float(u[k]);
    }
    float mine = 0.f;
#pragma unroll
    for (int k = 0; k < KK; ++k) {
        float s = a[k];
#pragma unroll
        for (int o = kWave / 2; o > 0; o >>= 1) s += __shfl_xor(s, o, kWave);
        if (t == k) mine = s;
    }
    if (t < KK) f.dw[(size_t)c * KK + t] = mine;
    if (t == 0) __hip_atomic_store(ctr, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// Backward-weight partials: block (group q, channel c) sums, over images n in its group and every
// output element, dy[n][c][oh][ow] * x[n][c][oh*S - pt + kh][ow*S - pl + kw] for each tap; a thread
// takes TH x TW output tiles of the group's flat (image, tile) space.
// partial[(c * ngroups + q) * K*K + tap]; fixed reduction order (wave shuffles, then waves in order).
template <int K, int S, int TH, int TW, typename T>
__global__ __launch_bounds__(kBlock) void k_dw_bwd_weight(const T* __restrict__ x, const T* __restrict__ dy, DwGeo g,
                                                          int nimg, int ngroups, float* __restrict__ partial,
                                                          DwFold fold) {
    __shared__ float s_red[kBlock / kWave][K * K];
    const int c = blockIdx.x % g.C, q = blockIdx.x / g.C;
    const int n0 = (int)((long)nimg * q / ngroups), n1 = (int)((long)nimg * (q + 1) / ngroups);
    const int ncol = (g.Wo + TW - 1) / TW, nrow = (g.Ho + TH - 1) / TH;
    const int per_img = nrow * ncol;
    const int count = per_img * (n1 - n0);
    float acc[K * K];
#pragma unroll
    for (int i = 0; i < K * K; ++i) acc[i] = 0.f;
    constexpr int R = (TH - 1) * S + K, CW = (TW - 1) * S + K;
    for (int e = threadIdx.x; e < count; e += kBlock) {
        const int nl = e / per_img;
        const int rem = e - nl * per_img;
        const int tr = rem / ncol, tc = rem - tr * ncol;
        const int plane = (n0 + nl) * g.C + c;
        const T* xp = x + (size_t)plane * g.Hi * g.Wi;
        const T* dp = dy + (size_t)plane * g.Ho * g.Wo;
        const int oh0 = tr * TH, ow0 = tc * TW;
        float d[TH][TW];
#pragma unroll
        for (int i = 0; i < TH; ++i)
#pragma unroll
            for (int j = 0; j < TW; ++j)
                d[i][j] = (oh0 + i < g.Ho && ow0 + j < g.Wo) ? ld(dp + (oh0 + i) * g.Wo + ow0 + j) : 0.f;
        const int ih0 = oh0 * S - g.pt, iw0 = ow0 * S - g.pl;
#pragma unroll
        for (int rr = 0; rr < R; ++rr) {
            const int ih = ih0 + rr;
            const bool row_ok = ih >= 0 && ih < g.Hi;
            float v[CW];
#pragma unroll
            for (int qq = 0; qq < CW; ++qq) {
                const int iw = iw0 + qq;
                v[qq] = (row_ok && iw >= 0 && iw < g.Wi) ? ld(xp + ih * g.Wi + iw) : 0.f;
            }
#pragma unroll
            for (int i = 0; i < TH; ++i) {
                const int kh = rr - i * S;
                if (kh >= 0 && kh < K) {
#pragma unroll
                    for (int j = 0; j < TW; ++j)
#pragma unroll
                        for (int kw = 0; kw < K; ++kw)
                            acc[kh * K + kw] = fmaf(d[i][j], v[j * S + kw], acc[kh * K + kw]);
                }
            }
        }
    }
    const int lane = threadIdx.x & (kWave - 1), wave = threadIdx.x / kWave;
#pragma unroll
    for (int i = 0; i < K * K; ++i) {
        float v = acc[i];
#pragma unroll
        for (int o = kWave / 2; o > 0; o >>= 1) v += __shfl_xor(v, o, kWave);
        if (lane == 0) s_red[wave][i] = v;
    }
    __syncthreads();
    float s = 0.f;
    if (threadIdx.x < K * K) {
#pragma unroll
        for (int jw = 0; jw < kBlock / kWave; ++jw) s += s_red[jw][threadIdx.x];
    }
    dw_finish<K * K>(partial, c, q, ngroups, s, fold);
}

inline bool geo_ok(int N, int C, int Hi, int Wi, int K, int S, int Ho, int Wo) {
    return N > 0 && C > 0 && Hi > 0 && Wi > 0 && Ho > 0 && Wo > 0 && (K == 3 || K == 5) && (S == 1 || S == 2) &&
           (long)N * C * Hi * Wi < INT_MAX && (long)N * C * Ho * Wo < INT_MAX;
}

// ---- LDS-staged depthwise kernels (round 5). The kernels above read every input element about twice
// with 2-byte loads whose lanes stride by the thread tile (4 or 8 bytes apart): the load count, not
// the bytes, bounded them (10-20 % of HBM on the trunk's large planes). Here a block stages a band of
// rows of PB planes into LDS (fp32, zero-padded so the taps need no bounds checks), with 16-B loads
// when a row holds a multiple of 8 elements and coalesced 2-B / 4-B loads otherwise; each thread then
// computes row segments of SEG consecutive outputs (SEG | Wo: one vector store per segment) from LDS.
#ifndef LSS_DW_LDS
#define LSS_DW_LDS 1  // experiment switch: 0 = the register-tiled kernels above
#endif
constexpr int kDwLdsFloats = 8192;  // staged input per block (32 KB)

struct DwBand {
    int BHo, PB, LW, LHmax, nbands;  // output rows per band, planes per block, LDS row stride / rows
};

// LDS column of input column iw: iw + kDwCol (so the 8-element chunks of a row land 8-B aligned:
// vector LDS writes); the left padding columns sit just below kDwCol, zero-filled with the right ones.
constexpr int kDwCol = 4;
// staged 16-B input chunks per thread per round: every load of a round in flight together (the loop
// that loaded, converted and wrote one chunk per iteration waited a memory round trip per iteration)
constexpr int kDwStageU = 8;

// Stage np planes (global plane stride gps elements) x LH rows from input row ih0 into LDS planes of
// lps floats (row stride LW): LDS (pl, r, c) = x[plane pl][ih0 + r][c - kDwCol], zero outside x.
template <typename T>
__device__ __forceinline__ void dw_stage(const T* __restrict__ xp, size_t gps, int np, int Hi, int Wi, int ih0, int LH,
                                         int LW, int lps, float* __restrict__ dst) {
    if (Wi % 8 == 0) {  // 8-element row chunks: 16-B (bf16) / 2 x 16-B (fp32) loads, all of a round in flight
        const int cpr = Wi / 8, per = LH * cpr, n = np * per;
        constexpr int U = sizeof(T) == 2 ? kDwStageU : kDwStageU / 2;
        constexpr int NV = sizeof(T) == 2 ? 1 : 2;  // 16-B pieces per chunk
        for (int i0 = threadIdx.x; i0 < n; i0 += U * kBlock) {
            uint4 raw[U][NV];
            const int nu = (n - (i0 - (int)threadIdx.x) + kBlock - 1) / kBlock;  // loads this round (block-uniform)
#pragma unroll
            for (int u = 0; u < U; ++u) {  // clamped addresses, unconditional loads, masked values
                if (u >= nu) break;
                const int i = min(i0 + u * kBlock, n - 1);
                const int pl = i / per, rem = i - pl * per, r = rem / cpr, ch = rem - r * cpr;
                const int ih = ih0 + r;
                const bool ok = ih >= 0 && ih < Hi;
                const uint4* src = reinterpret_cast<const uint4*>(xp + pl * gps + (size_t)min(max(ih, 0), Hi - 1) * Wi + 8 * ch);
#pragma unroll
                for (int h = 0; h < NV; ++h) raw[u][h] = keep_if(ok, src[h]);
            }
#pragma unroll
            for (int u = 0; u < U; ++u) {  // every load issued before the first LDS write (no sinking)
                if (u >= nu) break;
#pragma unroll
                for (int h = 0; h < NV; ++h) asm volatile("" : : "v"(raw[u][h].x), "v"(raw[u][h].y), "v"(raw[u][h].z), "v"(raw[u][h].w));
            }
#pragma unroll
            for (int u = 0; u < U; ++u) {  // (a clamped chunk rewrites chunk n - 1 with its own values)
                if (u >= nu) break;
                const int i = min(i0 + u * kBlock, n - 1);
                const int pl = i / per, rem = i - pl * per, r = rem / cpr, ch = rem - r * cpr;
                float2* d = reinterpret_cast<float2*>(dst + pl * lps + r * LW + kDwCol + 8 * ch);  // 8-B aligned
                float v[8];
                if constexpr (sizeof(T) == 2) {
                    unpack8(raw[u][0], v);
                } else {
                    const float4 a = __builtin_bit_cast(float4, raw[u][0]), b = __builtin_bit_cast(float4, raw[u][1]);
                    v[0] = a.x; v[1] = a.y; v[2] = a.z; v[3] = a.w; v[4] = b.x; v[5] = b.y; v[6] = b.z; v[7] = b.w;
                }
#pragma unroll
                for (int k = 0; k < 4; ++k) d[k] = make_float2(v[2 * k], v[2 * k + 1]);
            }
        }
        const int npad = LW - Wi;  // columns [0, kDwCol) and [kDwCol + Wi, LW)
        for (int i = threadIdx.x; i < np * LH * npad; i += kBlock) {
            const int pr = i / npad, k = i - pr * npad;
            const int pl = pr / LH, r = pr - pl * LH;
            dst[pl * lps + r * LW + (k < kDwCol ? k : Wi + k)] = 0.f;
        }
    } else {
        for (int i = threadIdx.x; i < np * LH * LW; i += kBlock) {
            const int pr = i / LW, c = i - pr * LW;
            const int pl = pr / LH, r = pr - pl * LH;
            const int ih = ih0 + r, iw = c - kDwCol;
            dst[pl * lps + r * LW + c] =
                (ih >= 0 && ih < Hi && iw >= 0 && iw < Wi) ? ld(xp + pl * gps + (size_t)ih * Wi + iw) : 0.f;
        }
    }
}

template <int SEG, typename T>
__device__ __forceinline__ void store_seg(T* __restrict__ p, const float* v, int n) {
    if (n == SEG) {
        if constexpr (sizeof(T) == 2 && SEG == 8) {
            *reinterpret_cast<uint4*>(p) = make_uint4(pack2(v[0], v[1]), pack2(v[2], v[3]), pack2(v[4], v[5]), pack2(v[6], v[7]));
            return;
        } else if constexpr (sizeof(T) == 2 && SEG == 4) {
            *reinterpret_cast<uint2*>(p) = make_uint2(pack2(v[0], v[1]), pack2(v[2], v[3]));
            return;
        } else if constexpr (sizeof(T) == 2 && SEG == 2) {
            *reinterpret_cast<unsigned*>(p) = pack2(v[0], v[1]);
            return;
        } else if constexpr (sizeof(T) == 4 && SEG % 4 == 0) {
#pragma unroll
            for (int k = 0; k < SEG; k += 4) *reinterpret_cast<float4*>(p + k) = make_float4(v[k], v[k + 1], v[k + 2], v[k + 3]);
            return;
        }
    }
#pragma unroll
    for (int k = 0; k < SEG; ++k)
        if (k < n) st(p + k, v[k]);
}

template <int SEG, typename T>
__device__ __forceinline__ void load_seg(const T* __restrict__ p, float* v, int n) {
    if (n == SEG) {
        if constexpr (sizeof(T) == 2 && SEG == 8) {
            unpack8(*reinterpret_cast<const uint4*>(p), v);
            return;
        } else if constexpr (sizeof(T) == 2 && SEG == 4) {
            const uint2 r = *reinterpret_cast<const uint2*>(p);
            v[0] = __uint_as_float(r.x << 16); v[1] = __uint_as_float(r.x & 0xFFFF0000u);
            v[2] = __uint_as_float(r.y << 16); v[3] = __uint_as_float(r.y & 0xFFFF0000u);
            return;
        } else if constexpr (sizeof(T) == 4 && SEG % 4 == 0) {
#pragma unroll
            for (int k = 0; k < SEG; k += 4) {
                const float4 a = *reinterpret_cast<const float4*>(p + k);
                v[k] = a.x; v[k + 1] = a.y; v[k + 2] = a.z; v[k + 3] = a.w;
            }
            return;
        }
    }
#pragma unroll
    for (int k = 0; k < SEG; ++k) v[k] = k < n ? ld(p + k) : 0.f;
}

template <typename T>
__device__ __forceinline__ void dw_stage_seg(const T* __restrict__ xp, int Hi, int Wi, int ih0, int LH, int LW, int pl,
                                         bool vec8, float* __restrict__ dst) {
    // LDS rows r = input rows ih0 + r, columns c = input columns c - pl; zero outside the input
    if (vec8) {  // Wi % 8 == 0: 8-element row chunks, 16-B (bf16) loads; the pad columns separately
        const int cpr = Wi / 8;
        for (int i = threadIdx.x; i < LH * cpr; i += kBlock) {
            const int r = i / cpr, ch = i - r * cpr;
            const int ih = ih0 + r;
            float v[8];
            if (ih >= 0 && ih < Hi) {
                const T* src = xp + (size_t)ih * Wi + 8 * ch;
                if constexpr (sizeof(T) == 2) {
                    unpack8(*reinterpret_cast<const uint4*>(src), v);
                } else {
                    const float4 a = *reinterpret_cast<const float4*>(src), b = *reinterpret_cast<const float4*>(src + 4);
                    v[0] = a.x; v[1] = a.y; v[2] = a.z; v[3] = a.w; v[4] = b.x; v[5] = b.y; v[6] = b.z; v[7] = b.w;
                }
            } else {
#pragma unroll
                for (int k = 0; k < 8; ++k) v[k] = 0.f;
            }
            float* d = dst + r * LW + pl + 8 * ch;
#pragma unroll
            for (int k = 0; k < 8; ++k) d[k] = v[k];
        }
        const int npad = LW - Wi;  // pl left + the rest right
        for (int i = threadIdx.x; i < LH * npad; i += kBlock) {
            const int r = i / npad, k = i - r * npad;
            dst[r * LW + (k < pl ? k : Wi + k)] = 0.f;
        }
    } else {
        for (int i = threadIdx.x; i < LH * LW; i += kBlock) {
            const int r = i / LW, c = i - r * LW;
            const int ih = ih0 + r, iw = c - pl;
            dst[i] = (ih >= 0 && ih < Hi && iw >= 0 && iw < Wi) ? ld(xp + (size_t)ih * Wi + iw) : 0.f;
        }
    }
}

// Round-5 segment kernel (the 5 x 5 and stride-2 forwards, where it measured faster than the tile
// mapping below): its own staging (column iw at iw + pl, row stride (Wo - 1) S + K) and SEG consecutive
// outputs of one row per thread. y (forward or stride-1 backward-data with flip): block = (PB
// consecutive planes, band of BHo output rows)
template <int K, int S, int SEG, typename T>
__global__ __launch_bounds__(kBlock) void k_dw_fwd_lds_seg(const T* __restrict__ x, const float* __restrict__ w, DwGeo g,
                                                       int flip, DwBand bd, T* __restrict__ y) {
    extern __shared__ float smem[];
    float* s_w = smem;                    // [PB][K*K]
    float* s_x = smem + bd.PB * K * K;    // [PB][LH][LW] (+ slack for the last segment's reads)
    const int band = blockIdx.x % bd.nbands, pg = blockIdx.x / bd.nbands;
    const int p0 = pg * bd.PB, np = min(bd.PB, g.nplanes - p0);
    const int oh0 = band * bd.BHo, nrow = min(bd.BHo, g.Ho - oh0);
    const int LH = (nrow - 1) * S + K;
    for (int i = threadIdx.x; i < np * K * K; i += kBlock) {
        const int pl = i / (K * K), t = i - pl * (K * K);
        s_w[i] = w[(size_t)((p0 + pl) % g.C) * K * K + (flip ? K * K - 1 - t : t)];
    }
    const bool vec8 = g.Wi % 8 == 0;
    for (int pl = 0; pl < np; ++pl)
        dw_stage_seg(x + (size_t)(p0 + pl) * g.Hi * g.Wi, g.Hi, g.Wi, oh0 * S - g.pt, LH, bd.LW, g.pl, vec8,
                 s_x + pl * bd.LHmax * bd.LW);
    __syncthreads();
    const int nseg = (g.Wo + SEG - 1) / SEG;
    const int items = np * nrow * nseg;
    constexpr int CW = (SEG - 1) * S + K;
    for (int it = threadIdx.x; it < items; it += kBlock) {
        const int pl = it / (nrow * nseg), rem = it - pl * (nrow * nseg);
        const int r = rem / nseg, sg = rem - r * nseg;
        const int ow0 = sg * SEG;
        const float* wk = s_w + pl * K * K;
        const float* xs = s_x + pl * bd.LHmax * bd.LW + (r * S) * bd.LW + ow0 * S;
        float acc[SEG];
#pragma unroll
        for (int j = 0; j < SEG; ++j) acc[j] = 0.f;
#pragma unroll
        for (int kh = 0; kh < K; ++kh) {
            float v[CW];
#pragma unroll
            for (int q = 0; q < CW; ++q) v[q] = xs[kh * bd.LW + q];
#pragma unroll
            for (int kw = 0; kw < K; ++kw) {
                const float wv = wk[kh * K + kw];
#pragma unroll
                for (int j = 0; j < SEG; ++j) acc[j] = fmaf(v[j * S + kw], wv, acc[j]);
            }
        }
        store_seg<SEG>(y + ((size_t)(p0 + pl) * g.Ho + oh0 + r) * g.Wo + ow0, acc, min(SEG, g.Wo - ow0));
    }
}

// Compute mapping of the LDS kernels: consecutive threads take consecutive output COLUMNS of a row
// group (TH output rows of one plane), so a wave's LDS reads of a tap are consecutive words (no bank
// conflicts; the round-5 mapping gave each thread SEG consecutive outputs, lanes 8 words apart: 8-way
// conflicts that made these kernels LDS-bound), and each staged input row a thread reads feeds every
// output row of its group it overlaps (vertical reuse: ((TH - 1) S + K) K reads for TH K^2 FMAs).
constexpr int kDwTH = 4;
// output columns per thread: TW consecutive outputs (one 4 * TW-byte store per row for bf16; the
// single-column form issued 8x the store instructions of the 16-B segment form and measured slower)
constexpr int kDwTW = 4;
// which LDS kernels take the TH x TW tile mapping (per-layer A/B, c3 step, profiles/r06/dw_tile_ab.txt):
// every weight gradient and the 3 x 3 stride-1 forward (27.9 vs 32.1 us at 64 x 176; weight gradients
// 33.6 vs 42.5, 46.3 vs 65.5); 5 x 5 and stride-2 forwards keep the segment mapping (57 vs 38 us: their
// threads' input columns 4 S words apart conflict in the LDS banks again)
__host__ __device__ constexpr bool dw_tile_map(int K, int S, bool fwd) { return !fwd || (K == 3 && S == 1); }

// y (forward or stride-1 backward-data with flip): block = (PB consecutive planes, band of BHo output rows)
template <int K, int S, int SEG, typename T>
__global__ __launch_bounds__(kBlock) void k_dw_fwd_lds(const T* __restrict__ x, const float* __restrict__ w, DwGeo g,
                                                       int flip, DwBand bd, T* __restrict__ y) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    constexpr int TH = kDwTH, TR = (TH - 1) * S + K;  // output rows per thread, input rows they read
    const int band = blockIdx.x % bd.nbands, pg = blockIdx.x / bd.nbands;
    const int p0 = pg * bd.PB, np = min(bd.PB, g.nplanes - p0);
    const int oh0 = band * bd.BHo, nrow = min(bd.BHo, g.Ho - oh0);
    const int LH = (nrow - 1) * S + K;
    const int lps = bd.LHmax * bd.LW;
    float* s_x = smem;                    // [PB][LHmax][LW] (8-B aligned rows)
    float* s_w = smem + bd.PB * lps;      // [PB][K*K]
    dw_stage(x + (size_t)p0 * g.Hi * g.Wi, (size_t)g.Hi * g.Wi, np, g.Hi, g.Wi, oh0 * S - g.pt, LH, bd.LW, lps, s_x);
    for (int i = threadIdx.x; i < np * K * K; i += kBlock) {
        const int pl = i / (K * K), t = i - pl * (K * K);
        s_w[i] = w[(size_t)((p0 + pl) % g.C) * K * K + (flip ? K * K - 1 - t : t)];
    }
    __syncthreads();
    const int col0 = kDwCol - g.pl;
    constexpr int TW = kDwTW, CW = (TW - 1) * S + K;  // output columns per thread, input columns they read
    const int nrg = (nrow + TH - 1) / TH, ncg = g.Wo / TW;  // (Wo % TW == 0: dw_lds_ok)
    const int items = np * nrg * ncg;
    for (int it = threadIdx.x; it < items; it += kBlock) {
        const int pr = it / ncg, ow = (it - pr * ncg) * TW;
        const int pl = pr / nrg, rg = pr - pl * nrg;
        const float* wk = s_w + pl * K * K;
        const float* xs = s_x + pl * lps + (rg * TH * S) * bd.LW + ow * S + col0;
        float acc[TH][TW];
#pragma unroll
        for (int j = 0; j < TH; ++j)
#pragma unroll
            for (int c = 0; c < TW; ++c) acc[j][c] = 0.f;
#pragma unroll
        for (int t = 0; t < TR; ++t) {  // input row t of the group (rows past the band's end: never stored)
            float v[CW];
#pragma unroll
            for (int q = 0; q < CW; ++q) v[q] = xs[min(t, LH - 1 - rg * TH * S) * bd.LW + q];
#pragma unroll
            for (int j = 0; j < TH; ++j) {
                const int kh = t - j * S;
                if (kh >= 0 && kh < K)
#pragma unroll
                    for (int kw = 0; kw < K; ++kw) {
                        const float wv = wk[kh * K + kw];
#pragma unroll
                        for (int c = 0; c < TW; ++c) acc[j][c] = fmaf(v[c * S + kw], wv, acc[j][c]);
                    }
            }
        }
        T* yp = y + ((size_t)(p0 + pl) * g.Ho + oh0 + rg * TH) * g.Wo + ow;
#pragma unroll
        for (int j = 0; j < TH; ++j)
            if (rg * TH + j < nrow) store_seg<TW>(yp + (size_t)j * g.Wo, acc[j], TW);
    }
}

// weight-gradient partials: block (channel c, image group q), PB images of the group staged at a time
template <int K, int S, int SEG, typename T>
__global__ __launch_bounds__(kBlock) void k_dw_wgt_lds(const T* __restrict__ x, const T* __restrict__ dy, DwGeo g,
                                                       int nimg, int ngroups, DwBand bd, float* __restrict__ partial,
                                                       DwFold fold) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    constexpr int TH = kDwTH, TR = (TH - 1) * S + K;
    float* s_x = smem;  // [PB][LHmax][LW]
    __shared__ float s_red[kBlock / kWave][K * K];
    const int c = blockIdx.x % g.C, q = blockIdx.x / g.C;
    const int n0 = (int)((long)nimg * q / ngroups), n1 = (int)((long)nimg * (q + 1) / ngroups);
    const int lps = bd.LHmax * bd.LW;
    const int col0 = kDwCol - g.pl;
    float acc[K * K];
#pragma unroll
    for (int i = 0; i < K * K; ++i) acc[i] = 0.f;
    for (int nb = n0; nb < n1; nb += bd.PB) {
        const int np = min(bd.PB, n1 - nb);
        for (int band = 0; band < bd.nbands; ++band) {
            const int oh0 = band * bd.BHo, nrow = min(bd.BHo, g.Ho - oh0);
            const int LH = (nrow - 1) * S + K;
            __syncthreads();  // the previous chunk's readers are done with s_x
            dw_stage(x + ((size_t)nb * g.C + c) * g.Hi * g.Wi, (size_t)g.C * g.Hi * g.Wi, np, g.Hi, g.Wi,
                     oh0 * S - g.pt, LH, bd.LW, lps, s_x);
            __syncthreads();
            constexpr int TW = kDwTW, CW = (TW - 1) * S + K;
            const int nrg = (nrow + TH - 1) / TH, ncg = g.Wo / TW;
            const int items = np * nrg * ncg;
            for (int it = threadIdx.x; it < items; it += kBlock) {
                const int pr = it / ncg, ow = (it - pr * ncg) * TW;
                const int pl = pr / nrg, rg = pr - pl * nrg;
                // the group's dy values (clamped rows, zeroed past the band: every load issued before the first use)
                const T* dp = dy + (((size_t)(nb + pl) * g.C + c) * g.Ho + oh0 + rg * TH) * g.Wo + ow;
                float d[TH][TW];
#pragma unroll
                for (int j = 0; j < TH; ++j) load_seg<TW>(dp + (size_t)min(j, nrow - 1 - rg * TH) * g.Wo, d[j], TW);
#pragma unroll
                for (int j = 0; j < TH; ++j)
                    if (rg * TH + j >= nrow)
#pragma unroll
                        for (int cc = 0; cc < TW; ++cc) d[j][cc] = 0.f;
                const float* xs = s_x + pl * lps + (rg * TH * S) * bd.LW + ow * S + col0;
#pragma unroll
                for (int t = 0; t < TR; ++t) {
                    float v[CW];
#pragma unroll
                    for (int qq = 0; qq < CW; ++qq) v[qq] = xs[min(t, LH - 1 - rg * TH * S) * bd.LW + qq];
#pragma unroll
                    for (int j = 0; j < TH; ++j) {
                        const int kh = t - j * S;
                        if (kh >= 0 && kh < K)
#pragma unroll
                            for (int kw = 0; kw < K; ++kw)
#pragma unroll
                                for (int cc = 0; cc < TW; ++cc)
                                    acc[kh * K + kw] = fmaf(d[j][cc], v[cc * S + kw], acc[kh * K + kw]);
                    }
                }
            }
        }
    }
    const int lane = threadIdx.x & (kWave - 1), wave = threadIdx.x / kWave;
#pragma unroll
    for (int i = 0; i < K * K; ++i) {
        float v = acc[i];
#pragma unroll
        for (int o = kWave / 2; o > 0; o >>= 1) v += __shfl_xor(v, o, kWave);
        if (lane == 0) s_red[wave][i] = v;
    }
    __syncthreads();
    float t = 0.f;
    if (threadIdx.x < K * K) {
#pragma unroll
        for (int jw = 0; jw < kBlock / kWave; ++jw) t += s_red[jw][threadIdx.x];
    }
    dw_finish<K * K>(partial, c, q, ngroups, t, fold);
}

// bands and planes per block for the LDS kernels: the whole plane when it fits, several planes per
// block while the block has fewer than ~2 output segments per thread
inline DwBand dw_band(int K, int S, const DwGeo& g, int seg, int max_planes, bool tile) {
    DwBand b;
    // row stride: the data at kDwCol, every compute read of the last (possibly partial) segment inside
    // the row; LW = 2 (mod 4): rows 8-B aligned for the staging writes, and consecutive rows start 2
    // banks apart (a stride of 0 mod 8 lined every row's segments up on the same banks: 32 -> 49 us at
    // block 0's 64 x 176 planes)
    (void)seg;
    b.LW = ((kDwCol - g.pl + (g.Wo - 1) * S + K + 1) & ~3) + 2;
    const int full = (g.Ho - 1) * S + K;
    if (full * b.LW <= kDwLdsFloats) {
        b.BHo = g.Ho;
        const int per_plane = tile ? ((g.Ho + kDwTH - 1) / kDwTH) * (g.Wo / kDwTW) : g.Ho * (g.Wo / seg);  // items
        int pb = std::max(1, kDwLdsFloats / (full * b.LW));
        pb = std::min(pb, std::max(1, (2 * kBlock + per_plane - 1) / per_plane));
        b.PB = std::max(1, std::min(pb, max_planes));
    } else {
        b.BHo = std::max(1, (kDwLdsFloats / b.LW - K) / S + 1);
        b.PB = 1;
    }
    b.LHmax = (b.BHo - 1) * S + K;
    b.nbands = (g.Ho + b.BHo - 1) / b.BHo;
    return b;
}

// the LDS kernels' vector accesses need 16-B aligned tensors (every lss_dwconv_* entry point refuses others,
// so the rule itself depends on the shape only); the staged row holds the whole input row
// (the right padding is not negative); and they run only where an output row splits into segments of
// 4 or 8 (Wo % 4 == 0): on the trunk's narrow planes (Wo = 22, 11) the register-tiled kernels are
// faster (c3 step, per layer: 15-55 vs 21-98 us), on the wide ones the LDS kernels (23-74 vs 50-181 us)
inline bool dw_lds_ok(int K, int S, const DwGeo& g) {
    return g.Wo % 4 == 0 && (g.Wo - 1) * S + K >= g.pl + g.Wi && (g.Ho - 1) * S + K >= g.pt + g.Hi;
}

inline int dw_seg(int Wo) { return Wo % 8 == 0 ? 8 : Wo % 4 == 0 ? 4 : Wo % 2 == 0 ? 2 : 1; }

// the round-5 band for the segment kernel: LDS rows of exactly (Wo - 1) S + K floats
inline DwBand dw_band_seg(int K, int S, const DwGeo& g, int seg, int max_planes) {
    DwBand b;
    b.LW = (g.Wo - 1) * S + K;
    const int full = (g.Ho - 1) * S + K;
    if (full * b.LW <= kDwLdsFloats) {
        b.BHo = g.Ho;
        const int per_plane = g.Ho * ((g.Wo + seg - 1) / seg);
        int pb = std::max(1, kDwLdsFloats / (full * b.LW));
        pb = std::min(pb, std::max(1, (2 * kBlock + per_plane - 1) / per_plane));
        b.PB = std::max(1, std::min(pb, max_planes));
    } else {
        b.BHo = std::max(1, (kDwLdsFloats / b.LW - K) / S + 1);
        b.PB = 1;
    }
    b.LHmax = (b.BHo - 1) * S + K;
    b.nbands = (g.Ho + b.BHo - 1) / b.BHo;
    return b;
}

template <int K, int S, typename T>
int dw_fwd_lds(const void* x, const float* w, DwGeo g, int flip, void* y, int seg, const DwBand& b, hipStream_t s) {
    if constexpr (!dw_tile_map(K, S, true)) {
        const long blocks = (long)b.nbands * ((g.nplanes + b.PB - 1) / b.PB);
        // slack past the staged rows: the last segment of a row reads up to (SEG - 1) * S columns past Wo
        const size_t lds = sizeof(float) * ((size_t)b.PB * K * K + (size_t)b.PB * b.LHmax * b.LW + 8 * S + K);
        if (blocks > INT_MAX) return LSS_CONV_EINVAL;
#define LSS_DW_FWD_SEG(SG) hipLaunchKernelGGL((k_dw_fwd_lds_seg<K, S, SG, T>), dim3((unsigned)blocks), dim3(kBlock), lds, \
                                              s, (const T*)x, w, g, flip, b, (T*)y)
        switch (seg) {
            case 8: LSS_DW_FWD_SEG(8); break;
            case 4: LSS_DW_FWD_SEG(4); break;
            case 2: LSS_DW_FWD_SEG(2); break;
            default: LSS_DW_FWD_SEG(1); break;
        }
#undef LSS_DW_FWD_SEG
        return launch_status();
    }
    const long blocks = (long)b.nbands * ((g.nplanes + b.PB - 1) / b.PB);
    const size_t lds = sizeof(float) * ((size_t)b.PB * b.LHmax * b.LW + (size_t)b.PB * K * K);
    if (blocks > INT_MAX) return LSS_CONV_EINVAL;
#define LSS_DW_FWD(SG) hipLaunchKernelGGL((k_dw_fwd_lds<K, S, SG, T>), dim3((unsigned)blocks), dim3(kBlock), lds, s, \
                                          (const T*)x, w, g, flip, b, (T*)y)
    switch (seg) {
        case 8: LSS_DW_FWD(8); break;
        case 4: LSS_DW_FWD(4); break;
        case 2: LSS_DW_FWD(2); break;
        default: LSS_DW_FWD(1); break;
    }
#undef LSS_DW_FWD
    return launch_status();
}

template <int K, int S, typename T>
int dw_wgt_lds(const void* x, const void* dy, DwGeo g, int nimg, int ngroups, float* partial, DwFold fold, int seg,
               const DwBand& b, hipStream_t s) {
    const size_t lds = sizeof(float) * ((size_t)b.PB * b.LHmax * b.LW);
#define LSS_DW_WGT(SG) hipLaunchKernelGGL((k_dw_wgt_lds<K, S, SG, T>), dim3(g.C * ngroups), dim3(kBlock), lds, s, \
                                          (const T*)x, (const T*)dy, g, nimg, ngroups, b, partial, fold)
    switch (seg) {
        case 8: LSS_DW_WGT(8); break;
        case 4: LSS_DW_WGT(4); break;
        case 2: LSS_DW_WGT(2); break;
        default: LSS_DW_WGT(1); break;
    }
#undef LSS_DW_WGT
    return launch_status();
}

// ---- narrow planes (the trunk's 8 x 22 and 4 x 11 maps: Wo in {22, 11}), whole planes per block. The
// register-tiled kernels above issue ~100 two-byte loads per thread on these (lanes 8 B apart; 0.6-1.4
// TB/s, profiles/r06/step_roofline.json), and their rows of 22 / 11 elements are not 16-B aligned,
// which kept them off the LDS kernels' vector staging. But a block's consecutive planes are ONE
// contiguous run of memory: staged here with flat 16-B loads into zero-padded fp32 LDS planes; a
// thread computes one output row (WO outputs; every staged value it reads feeds all the taps that
// reach it); the outputs go back through LDS as one contiguous run of 16-B stores.
// f(i, v) for the n elements of the run at src: 16-B loads when the run allows them (src 16-B aligned,
// n a multiple of the vector), else one element per load
template <typename T, typename F>
__device__ __forceinline__ void for_run(const T* __restrict__ src, int n, F&& f) {
    constexpr int V = 16 / sizeof(T);
    if ((reinterpret_cast<uintptr_t>(src) & 15) == 0 && n % V == 0) {
        for (int i = threadIdx.x; i < n / V; i += kBlock) {
            float v[V];
            ldv<16 / (int)sizeof(T)>(src + (size_t)i * V, v);
#pragma unroll
            for (int j = 0; j < V; ++j) f(i * V + j, v[j]);
        }
    } else {
        for (int i = threadIdx.x; i < n; i += kBlock) f(i, ld(src + i));
    }
}

// VW consecutive elements -> fp32, in loads of up to 16 B (the caller guarantees the alignment)
template <int VW, typename T>
__device__ __forceinline__ void ld_vec(const T* __restrict__ p, float* o) {
    constexpr int B = VW * (int)sizeof(T);
    if constexpr (B >= 16) {
        constexpr int E = 16 / (int)sizeof(T);
#pragma unroll
        for (int k = 0; k < VW; k += E) ldv<16 / (int)sizeof(T)>(p + k, o + k);
    } else if constexpr (B == 8 && sizeof(T) == 2) {
        const uint2 u = *reinterpret_cast<const uint2*>(p);
        o[0] = __uint_as_float(u.x << 16); o[1] = __uint_as_float(u.x & 0xFFFF0000u);
        o[2] = __uint_as_float(u.y << 16); o[3] = __uint_as_float(u.y & 0xFFFF0000u);
    } else if constexpr (B == 8) {
        const float2 a = *reinterpret_cast<const float2*>(p);
        o[0] = a.x; o[1] = a.y;
    } else if constexpr (B == 4 && sizeof(T) == 2) {
        const unsigned u = *reinterpret_cast<const unsigned*>(p);
        o[0] = __uint_as_float(u << 16); o[1] = __uint_as_float(u & 0xFFFF0000u);
    } else {
#pragma unroll
        for (int k = 0; k < VW; ++k) o[k] = ld(p + k);
    }
}

// f(pl, e, v) for element e of plane pl, over np planes of n elements each at x + (first + pl * step) * n:
// one flat loop over every plane's VW-element vectors, so all their loads are in flight together
template <int VW, typename T, typename F>
__device__ __forceinline__ void for_planes_v(const T* __restrict__ x, size_t first, size_t step, int np, int n, F&& f) {
    const int nv = n / VW;
    for (int i = threadIdx.x; i < np * nv; i += kBlock) {
        const int pl = i / nv, v = i - pl * nv;
        float vals[VW];
        ld_vec<VW, T>(x + (first + (size_t)pl * step) * n + (size_t)v * VW, vals);
#pragma unroll
        for (int j = 0; j < VW; ++j) f(pl, v * VW + j, vals[j]);
    }
}
template <typename T, typename F>
__device__ __forceinline__ void for_planes(const T* __restrict__ x, size_t first, size_t step, int np, int n, F&& f) {
    // (plane bases are n elements apart: n % VW == 0 keeps every vector aligned on an aligned tensor)
    if (n % 8 == 0) for_planes_v<8, T>(x, first, step, np, n, f);
    else if (n % 4 == 0) for_planes_v<4, T>(x, first, step, np, n, f);
    else if (n % 2 == 0) for_planes_v<2, T>(x, first, step, np, n, f);
    else for_planes_v<1, T>(x, first, step, np, n, f);
}

// the run [0, n) of s (T in LDS) to dst: 16-B stores when aligned
template <typename T>
__device__ __forceinline__ void store_run(T* __restrict__ dst, const T* __restrict__ s, int n) {
    constexpr int V = 16 / sizeof(T);
    if ((reinterpret_cast<uintptr_t>(dst) & 15) == 0 && n % V == 0) {
        for (int i = threadIdx.x; i < n / V; i += kBlock)
            *reinterpret_cast<uint4*>(dst + (size_t)i * V) = *reinterpret_cast<const uint4*>(s + (size_t)i * V);
    } else {
        for (int i = threadIdx.x; i < n; i += kBlock) dst[i] = s[i];
    }
}

// one input plane element (r, c) into its padded LDS slot (never read if it lies past the reach)
__device__ __forceinline__ void put_padded(float* __restrict__ plane, int r, int c, int pt, int pl, int LH, int LW,
                                          float v) {
    const int rr = r + pt, cc = c + pl;
    if (rr < LH && cc < LW) plane[rr * LW + cc] = v;
}

template <int K, int S, int WO>
struct PlaneGeo {
    static constexpr int LW = (WO - 1) * S + K;
    __host__ __device__ static int LH(int Ho) { return (Ho - 1) * S + K; }
};

// forward (and stride-1 backward-data with flip): block = PB consecutive planes
template <int K, int S, int WO, typename T>
__global__ __launch_bounds__(kBlock) void k_dw_fwd_planes(const T* __restrict__ x, const float* __restrict__ w,
                                                          DwGeo g, int flip, int PB, T* __restrict__ y) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    using PG = PlaneGeo<K, S, WO>;
    constexpr int LW = PG::LW;
    const int LH = PG::LH(g.Ho), plane_f = LH * LW;
    const int p0 = blockIdx.x * PB, np = min(PB, g.nplanes - p0);
    const int HiWi = g.Hi * g.Wi, HoWo = g.Ho * WO;
    float* s_w = smem;                                   // [PB][K*K]
    float* s_x = s_w + ((PB * K * K + 3) & ~3);          // [PB][LH][LW]
    T* s_y = reinterpret_cast<T*>(s_x + ((PB * plane_f + 3) & ~3));  // [PB][Ho][WO], 16-B aligned
    for (int i = threadIdx.x; i < np * plane_f; i += kBlock) s_x[i] = 0.f;
    for (int i = threadIdx.x; i < np * K * K; i += kBlock) {
        const int pl = i / (K * K), t = i - pl * (K * K);
        s_w[i] = w[(size_t)((p0 + pl) % g.C) * K * K + (flip ? K * K - 1 - t : t)];
    }
    __syncthreads();
    for_run(x + (size_t)p0 * HiWi, np * HiWi, [&](int f, float v) {
        const int pl = f / HiWi, rem = f - pl * HiWi;
        const int r = rem / g.Wi;
        put_padded(s_x + pl * plane_f, r, rem - r * g.Wi, g.pt, g.pl, LH, LW, v);
    });
    __syncthreads();
    for (int it = threadIdx.x; it < np * g.Ho; it += kBlock) {
        const int pl = it / g.Ho, oh = it - pl * g.Ho;
        const float* xs = s_x + pl * plane_f + oh * S * LW;
        const float* wk = s_w + pl * K * K;
        float acc[WO];
#pragma unroll
        for (int j = 0; j < WO; ++j) acc[j] = 0.f;
#pragma unroll
        for (int kh = 0; kh < K; ++kh) {
            float v[LW];
#pragma unroll
            for (int q = 0; q < LW; ++q) v[q] = xs[kh * LW + q];
#pragma unroll
            for (int kw = 0; kw < K; ++kw) {
                const float wv = wk[kh * K + kw];
#pragma unroll
                for (int j = 0; j < WO; ++j) acc[j] = fmaf(v[j * S + kw], wv, acc[j]);
            }
        }
        T* o = s_y + pl * HoWo + oh * WO;
#pragma unroll
        for (int j = 0; j < WO; ++j) st(o + j, acc[j]);
    }
    __syncthreads();
    store_run(y + (size_t)p0 * HoWo, s_y, np * HoWo);
}

// weight-gradient partials: block (channel c, image group q); PB images' planes of x and dy staged at
// a time; a thread takes output rows; fixed reduction order (the thread's rows in order, then wave
// shuffles, then waves in order)
template <int K, int S, int WO, typename T>
__global__ __launch_bounds__(kBlock) void k_dw_wgt_planes(const T* __restrict__ x, const T* __restrict__ dy, DwGeo g,
                                                          int nimg, int ngroups, int PB, float* __restrict__ partial,
                                                          DwFold fold) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    __shared__ float s_red[kBlock / kWave][K * K];
    using PG = PlaneGeo<K, S, WO>;
    constexpr int LW = PG::LW;
    const int LH = PG::LH(g.Ho), plane_f = LH * LW;
    const int c = blockIdx.x % g.C, q = blockIdx.x / g.C;
    const int n0 = (int)((long)nimg * q / ngroups), n1 = (int)((long)nimg * (q + 1) / ngroups);
    const int HiWi = g.Hi * g.Wi, HoWo = g.Ho * WO;
    float* s_x = smem;                                   // [PB][LH][LW]
    float* s_d = s_x + PB * plane_f;                     // [PB][Ho][WO]
    float acc[K * K];
#pragma unroll
    for (int i = 0; i < K * K; ++i) acc[i] = 0.f;
    for (int nb = n0; nb < n1; nb += PB) {
        const int np = min(PB, n1 - nb);
        __syncthreads();  // the previous chunk's readers are done
        for (int i = threadIdx.x; i < np * plane_f; i += kBlock) s_x[i] = 0.f;
        __syncthreads();
        const size_t first = (size_t)nb * g.C + c;  // plane (image nb, channel c); images g.C planes apart
        for_planes(x, first, (size_t)g.C, np, HiWi, [&](int pl, int f, float v) {
            const int r = f / g.Wi;
            put_padded(s_x + pl * plane_f, r, f - r * g.Wi, g.pt, g.pl, LH, LW, v);
        });
        for_planes(dy, first, (size_t)g.C, np, HoWo, [&](int pl, int f, float v) { s_d[pl * HoWo + f] = v; });
        __syncthreads();
        for (int it = threadIdx.x; it < np * g.Ho; it += kBlock) {
            const int pl = it / g.Ho, oh = it - pl * g.Ho;
            const float* xs = s_x + pl * plane_f + oh * S * LW;
            const float* ds = s_d + pl * HoWo + oh * WO;
            float d[WO];
#pragma unroll
            for (int j = 0; j < WO; ++j) d[j] = ds[j];
#pragma unroll
            for (int kh = 0; kh < K; ++kh) {
                float v[LW];
#pragma unroll
                for (int qq = 0; qq < LW; ++qq) v[qq] = xs[kh * LW + qq];
#pragma unroll
                for (int kw = 0; kw < K; ++kw) {
                    float a = acc[kh * K + kw];
#pragma unroll
                    for (int j = 0; j < WO; ++j) a = fmaf(d[j], v[j * S + kw], a);
                    acc[kh * K + kw] = a;
                }
            }
        }
    }
    const int lane = threadIdx.x & (kWave - 1), wave = threadIdx.x / kWave;
#pragma unroll
    for (int i = 0; i < K * K; ++i) {
        float v = acc[i];
#pragma unroll
        for (int o = kWave / 2; o > 0; o >>= 1) v += __shfl_xor(v, o, kWave);
        if (lane == 0) s_red[wave][i] = v;
    }
    __syncthreads();
    float t = 0.f;
    if (threadIdx.x < K * K) {
#pragma unroll
        for (int jw = 0; jw < kBlock / kWave; ++jw) t += s_red[jw][threadIdx.x];
    }
    dw_finish<K * K>(partial, c, q, ngroups, t, fold);
}

#ifndef LSS_DW_PLANES
#define LSS_DW_PLANES 1  // experiment switch: 0 = the register-tiled kernels on the narrow planes
#endif
constexpr int kDwPlanesLdsMax = 48 * 1024;  // bytes of LDS a planes block may use

// the planes kernels take Wo in {22, 11} (the trunk's narrow maps), a staged plane holding every input
// element a tap reaches; PB = planes per block: one output row per thread, within the LDS budget
inline int dw_planes_pb(int K, int S, const DwGeo& g, int extra_floats_per_plane, int elt) {
    if (!LSS_DW_PLANES || (g.Wo != 22 && g.Wo != 11)) return 0;
    const int WO = g.Wo, LW = (WO - 1) * S + K, LH = (g.Ho - 1) * S + K;  // PlaneGeo<K, S, WO>
    const int plane_bytes = 4 * (LH * LW + extra_floats_per_plane) + elt * g.Ho * WO;
    int pb = std::max(1, kBlock / g.Ho);
    while (pb > 1 && pb * plane_bytes + 4 * pb * K * K + 64 > kDwPlanesLdsMax) --pb;
    return pb * plane_bytes + 4 * pb * K * K + 64 <= kDwPlanesLdsMax ? pb : 0;
}

template <int K, int S, int WO, typename T>
int dw_fwd_planes(const void* x, const float* w, DwGeo g, int flip, void* y, int pb, hipStream_t s) {
    using PG = PlaneGeo<K, S, WO>;
    const size_t lds = 4 * ((((size_t)pb * K * K + 3) & ~(size_t)3) +
                            (((size_t)pb * PG::LH(g.Ho) * PG::LW + 3) & ~(size_t)3)) +
                       sizeof(T) * (size_t)pb * g.Ho * WO;
    const long blocks = ((long)g.nplanes + pb - 1) / pb;  // (<= nplanes < 2^31)
    hipLaunchKernelGGL((k_dw_fwd_planes<K, S, WO, T>), dim3((unsigned)blocks), dim3(kBlock), lds, s, (const T*)x, w, g,
                       flip, pb, (T*)y);
    return launch_status();
}

template <int K, int S, int WO, typename T>
int dw_wgt_planes(const void* x, const void* dy, DwGeo g, int nimg, int ngroups, float* partial, DwFold fold, int pb,
                  hipStream_t s) {
    using PG = PlaneGeo<K, S, WO>;
    const size_t lds = 4 * (size_t)pb * (PG::LH(g.Ho) * PG::LW + g.Ho * WO);
    hipLaunchKernelGGL((k_dw_wgt_planes<K, S, WO, T>), dim3(g.C * ngroups), dim3(kBlock), lds, s, (const T*)x,
                       (const T*)dy, g, nimg, ngroups, pb, partial, fold);
    return launch_status();
}

// ---- THE selection rule of the three passes: lss_dwconv_arm reports it, the launchers below switch on it.
// Forward and weight gradient: the LDS kernels where dw_lds_ok (the segment map for the forward of every
// (K, S) but (3, 1), the tile map otherwise), else the planes kernels (Wo 22 / 11 within the LDS budget;
// forward: stride 1 only -- stride 2 is slower than the register-tiled kernel, 21.9 / 21.0 vs 15.3 / 19.1 us
// in the c3 step), else the register-tiled kernels. Backward-data: stride 1 is the forward correlation with
// the kernel flipped and the padding mirrored (g and flip below); stride 2 has one kernel per parity of the
// paddings.
struct DwArm {
    int family, seg, banded, pb;
    DwBand band;  // the LDS families' bands
    DwGeo g;      // the geometry the kernel runs on (mirrored for stride-1 backward-data)
    int flip;
};

inline DwArm dw_arm(int pass, int K, int S, int elt, const DwGeo& g0, int nimg, int ngroups) {
    DwArm a{};
    a.g = g0;
    if (pass == LSS_DW_BWD_DATA) {
        if (S == 2) {
            a.family = LSS_DW_S2_PAR0 + (((g0.pt & 1) << 1) | (g0.pl & 1));
            return a;
        }
        a.g = DwGeo{g0.C, g0.Ho, g0.Wo, g0.Hi, g0.Wi, K - 1 - g0.pt, K - 1 - g0.pl, g0.nplanes};
        a.flip = 1;
    }
    const DwGeo& g = a.g;
    const bool wgt = pass == LSS_DW_BWD_WEIGHT;
    if (LSS_DW_LDS && dw_lds_ok(K, S, g)) {
        const bool tile = dw_tile_map(K, S, !wgt);
        a.family = tile ? LSS_DW_LDS_TILE : LSS_DW_LDS_SEG;
        a.seg = dw_seg(g.Wo);
        a.band = tile ? dw_band(K, S, g, a.seg, wgt ? (nimg + ngroups - 1) / ngroups : g.nplanes, true)
                      : dw_band_seg(K, S, g, a.seg, g.nplanes);
        a.banded = a.band.nbands > 1;
        a.pb = a.band.PB;
        return a;
    }
    const int pb = wgt ? dw_planes_pb(K, S, g, g.Ho * g.Wo, 0) : S == 1 ? dw_planes_pb(K, S, g, 0, elt) : 0;
    if (pb > 0) {
        a.family = g.Wo == 22 ? LSS_DW_PLANES22 : LSS_DW_PLANES11;
        a.pb = pb;
        return a;
    }
    a.family = LSS_DW_REG;
    return a;
}

// dispatch over (K, S, T)
template <template <int, int, typename> class F, typename... A>
int dispatch_kst(int K, int S, int dtype, A... a) {
    if (dtype == LSS_CONV_F32) {
        if (K == 3 && S == 1) return F<3, 1, float>::run(a...);
        if (K == 3 && S == 2) return F<3, 2, float>::run(a...);
        if (K == 5 && S == 1) return F<5, 1, float>::run(a...);
        if (K == 5 && S == 2) return F<5, 2, float>::run(a...);
    } else if (dtype == LSS_CONV_BF16) {
        if (K == 3 && S == 1) return F<3, 1, bf16>::run(a...);
        if (K == 3 && S == 2) return F<3, 2, bf16>::run(a...);
        if (K == 5 && S == 1) return F<5, 1, bf16>::run(a...);
        if (K == 5 && S == 2) return F<5, 2, bf16>::run(a...);
    }
    return LSS_CONV_EINVAL;
}

// the forward kernels on arm a (the forward itself, or stride-1 backward-data re-entering it)
template <int K, int S, typename T>
int dw_fwd_run(const void* x, const float* w, const DwArm& a, void* y, hipStream_t s) {
    const DwGeo& g = a.g;
    switch (a.family) {
        case LSS_DW_LDS_SEG:
        case LSS_DW_LDS_TILE: return dw_fwd_lds<K, S, T>(x, w, g, a.flip, y, a.seg, a.band, s);
        case LSS_DW_PLANES22: return dw_fwd_planes<K, S, 22, T>(x, w, g, a.flip, y, a.pb, s);
        case LSS_DW_PLANES11: return dw_fwd_planes<K, S, 11, T>(x, w, g, a.flip, y, a.pb, s);
        default: break;
    }
    constexpr int TH = Tile<S>::TH, TW = Tile<S>::TW;
    const long n = (long)g.nplanes * ((g.Ho + TH - 1) / TH) * ((g.Wo + TW - 1) / TW);
    hipLaunchKernelGGL((k_dw_fwd<K, S, TH, TW, T>), dim3(grid_blocks(n, kBlock)), dim3(kBlock), 0, s, (const T*)x, w, g,
                       a.flip, (T*)y);
    return launch_status();
}

template <int K, int S, typename T>
struct Fwd {
    static int run(const void* x, const float* w, DwGeo g, void* y, hipStream_t s) {
        return dw_fwd_run<K, S, T>(x, w, dw_arm(LSS_DW_FWD, K, S, (int)sizeof(T), g, 0, 1), y, s);
    }
};

template <int K, int S, typename T>
struct BwdData {
    static int run(const void* dy, const float* w, DwGeo g, void* dx, hipStream_t s) {
        const DwArm a = dw_arm(LSS_DW_BWD_DATA, K, S, (int)sizeof(T), g, 0, 1);
        const dim3 gr(grid_blocks((long)g.nplanes * ((g.Hi + 1) / 2) * ((g.Wi + 3) / 4), kBlock)), bl(kBlock);
        switch (a.family) {
            case LSS_DW_S2_PAR0: hipLaunchKernelGGL((k_dw_bwd_data_s2<K, 0, 0, T>), gr, bl, 0, s, (const T*)dy, w, g, (T*)dx); break;
            case LSS_DW_S2_PAR1: hipLaunchKernelGGL((k_dw_bwd_data_s2<K, 0, 1, T>), gr, bl, 0, s, (const T*)dy, w, g, (T*)dx); break;
            case LSS_DW_S2_PAR2: hipLaunchKernelGGL((k_dw_bwd_data_s2<K, 1, 0, T>), gr, bl, 0, s, (const T*)dy, w, g, (T*)dx); break;
            case LSS_DW_S2_PAR3: hipLaunchKernelGGL((k_dw_bwd_data_s2<K, 1, 1, T>), gr, bl, 0, s, (const T*)dy, w, g, (T*)dx); break;
            default: return dw_fwd_run<K, 1, T>(dy, w, a, dx, s);  // stride 1 (the rule gives stride 2 a parity)
        }
        return launch_status();
    }
};

template <int K, int S, typename T>
struct BwdWeight {
    static int run(const void* x, const void* dy, DwGeo g, int nimg, int ngroups, float* partial, DwFold fold,
                   hipStream_t s) {
        const DwArm a = dw_arm(LSS_DW_BWD_WEIGHT, K, S, (int)sizeof(T), g, nimg, ngroups);
        switch (a.family) {
            case LSS_DW_LDS_TILE: return dw_wgt_lds<K, S, T>(x, dy, g, nimg, ngroups, partial, fold, a.seg, a.band, s);
            case LSS_DW_PLANES22: return dw_wgt_planes<K, S, 22, T>(x, dy, g, nimg, ngroups, partial, fold, a.pb, s);
            case LSS_DW_PLANES11: return dw_wgt_planes<K, S, 11, T>(x, dy, g, nimg, ngroups, partial, fold, a.pb, s);
            default: break;
        }
        hipLaunchKernelGGL((k_dw_bwd_weight<K, S, 4, S == 1 ? 4 : 2, T>), dim3(g.C * ngroups), dim3(kBlock), 0, s,
                           (const T*)x, (const T*)dy, g, nimg, ngroups, partial, fold);
        return launch_status();
    }
};

}  // namespace

extern "C" {

int lss_dwconv_arm(int32_t pass, int32_t dtype, int32_t N, int32_t C, int32_t Hi, int32_t Wi, int32_t K, int32_t stride,
                   int32_t pad_top, int32_t pad_left, int32_t Ho, int32_t Wo, int32_t ngroups, lss_dw_arm_t* arm) {
    if (!arm || pass < LSS_DW_FWD || pass > LSS_DW_BWD_WEIGHT || (dtype != LSS_CONV_F32 && dtype != LSS_CONV_BF16) ||
        !geo_ok(N, C, Hi, Wi, K, stride, Ho, Wo))
        return LSS_CONV_EINVAL;
    if (pass == LSS_DW_BWD_WEIGHT && (ngroups <= 0 || ngroups > N)) return LSS_CONV_EINVAL;
    const DwGeo g{C, Hi, Wi, Ho, Wo, pad_top, pad_left, N * C};
    const DwArm a = dw_arm(pass, K, stride, dtype == LSS_CONV_BF16 ? 2 : 4, g, N, pass == LSS_DW_BWD_WEIGHT ? ngroups : 1);
    arm->family = a.family;
    arm->seg = a.seg;
    arm->banded = a.banded;
    arm->pb = a.pb;
    return 0;
}

int lss_dwconv_fwd(const void* x, int32_t dtype, const float* w, int32_t N, int32_t C, int32_t Hi, int32_t Wi,
                   int32_t K, int32_t stride, int32_t pad_top, int32_t pad_left, int32_t Ho, int32_t Wo, void* y,
                   void* stream) {
    if (!x || !w || !y || !geo_ok(N, C, Hi, Wi, K, stride, Ho, Wo) || !aligned16(x, y)) return LSS_CONV_EINVAL;
    const DwGeo g{C, Hi, Wi, Ho, Wo, pad_top, pad_left, N * C};
    return dispatch_kst<Fwd>(K, stride, dtype, x, w, g, y, (hipStream_t)stream);
}

int lss_dwconv_bwd_data(const void* dy, int32_t dtype, const float* w, int32_t N, int32_t C, int32_t Hi, int32_t Wi,
                        int32_t K, int32_t stride, int32_t pad_top, int32_t pad_left, int32_t Ho, int32_t Wo, void* dx,
                        void* stream) {
    if (!dy || !w || !dx || !geo_ok(N, C, Hi, Wi, K, stride, Ho, Wo) || !aligned16(dy, dx)) return LSS_CONV_EINVAL;
    const DwGeo g{C, Hi, Wi, Ho, Wo, pad_top, pad_left, N * C};
    return dispatch_kst<BwdData>(K, stride, dtype, dy, w, g, dx, (hipStream_t)stream);
}

int lss_dwconv_bwd_weight(const void* x, const void* dy, int32_t dtype, int32_t N, int32_t C, int32_t Hi, int32_t Wi,
                          int32_t K, int32_t stride, int32_t pad_top, int32_t pad_left, int32_t Ho, int32_t Wo,
                          int32_t ngroups, float* partial, void* stream) {
    if (!x || !dy || !partial || ngroups <= 0 || ngroups > N || !geo_ok(N, C, Hi, Wi, K, stride, Ho, Wo) ||
        !aligned16(x, dy))
        return LSS_CONV_EINVAL;
    const DwGeo g{C, Hi, Wi, Ho, Wo, pad_top, pad_left, N * C};
    return dispatch_kst<BwdWeight>(K, stride, dtype, x, dy, g, (int)N, (int)ngroups, partial, DwFold{nullptr, nullptr},
                                   (hipStream_t)stream);
}

int lss_dwconv_bwd_weight2(const void* x, const void* dy, int32_t dtype, int32_t N, int32_t C, int32_t Hi, int32_t Wi,
                           int32_t K, int32_t stride, int32_t pad_top, int32_t pad_left, int32_t Ho, int32_t Wo,
                           int32_t ngroups, float* partial, uint32_t* sync, float* dw, void* stream) {
    if (!x || !dy || !partial || !sync || !dw || ngroups <= 0 || ngroups > N || C > kDwSyncMaxC ||
        !geo_ok(N, C, Hi, Wi, K, stride, Ho, Wo) || !aligned16(x, dy))
        return LSS_CONV_EINVAL;
    const DwGeo g{C, Hi, Wi, Ho, Wo, pad_top, pad_left, N * C};
    return dispatch_kst<BwdWeight>(K, stride, dtype, x, dy, g, (int)N, (int)ngroups, partial, DwFold{sync, dw},
                                   (hipStream_t)stream);
}

}  // extern "C"
