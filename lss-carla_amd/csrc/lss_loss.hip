// lss_loss.hip -- the segmentation losses and their validation metrics. This half: the sigmoid losses (independent
// classes); the softmax half (exclusive classes) follows below.
//
// Partition, shared by every kernel here: thread = 8 consecutive elements of the (N, K, H, W) logits (fp32 or bf16; a
// bf16 input is the same as its exact fp32 cast), block = 256 threads, fp32 arithmetic. A thread loads its 8 logits and
// labels with 16-byte loads when the caller says all 8 are inside the bound and the bases are aligned, else one guarded
// element at a time (load8). Sums are folded in one fixed order: the lanes of a wave by a butterfly, then the block's 4
// waves in order (lanes_sum, fold_stage, fold_waves) into one record per block; a small second kernel folds the records in block
// order. An element that does not count (past the end, past n_valid, or masked out) is *selected* out, never multiplied
// by zero, so nothing of it reaches a sum, a count or a gradient, whatever its logit is.
//
// Training, k_sig_loss_fwd<T, P, MASKED>: the loss terms summed in fp32 into partial[block] and the input gradient
// (times 1 / n) written in the logits' type in the same pass. The term policy P says what an element of class k costs:
//   OneWeight     SimpleLoss (src/tools.py:222-230), BCEWithLogitsLoss(pos_weight): the weight travels as a kernel
//                 argument, and no class is walked;
//   ClassWeights  the same term with pos_weight[k] read from device memory;
//   FocalRows     focal_term with the row (w_pos, w_neg, gamma) of class k read from device memory.
// The per-class policies carry the device pointer, so a captured graph replays with the current weights. Element i
// belongs to class (i / plane) % K; 8 elements may cross a plane boundary (plane % 8 != 0), so the class is walked per
// element: one division per thread, then increments (ClassWalk). One body, so the variants agree bit for bit wherever
// their terms do: equal weights give OneWeight's bits, gamma = 0 with rows (pw, 1, 0) give ClassWeights' bits.
// MASKED (ABI 32) adds a uint8 mask `valid` (batch, plane), one plane shared by the K classes of a sample: a masked-out
// element adds nothing and its gradient is written as 0. The number of valid elements M is counted in the same pass
// (counts[block]), so the gradient cannot be divided by it there: it is stored times 1 / n as without a mask, and
// k_sig_loss_total<true> writes loss = sum / max(M, 1) and scale = n / max(M, 1) for k_sig_loss_bwd<T, true> -- exactly
// 1 when every element is valid, so an all-ones mask gives the unmasked gradient bit for bit.
//
// Validation (get_val_info, src/tools.py:243-270) over the first n_valid samples of a batch -- the leading
// limit = n_valid * per_sample elements -- in one pass: the loss terms summed in fp64, the counts in integers.
//   k_bce_iou       one weight, one threshold (x > 0): counts in registers, one struct record per block;
//   k_bce_iou_pc    per-class weights: a thread counts a run of one class and adds it to the block's LDS counters;
//   k_seg_metrics<T, MASKED>  focal rows and a ladder of thresholds: an LDS histogram per block, which the fold turns
//                   into the counts by suffix sums; MASKED adds the mask and one more count slot behind the histograms.

#include <limits.h>

#include <type_traits>

#include "lss_convs.h"
#include "lss_device.h"

// The library is built with -ffp-contract=off for the geometry's reference op order (lss_hip.hip);
// the conv-stack kernels here have no bit-exact contract, so they keep FMA contraction.
#pragma clang fp contract(fast)

namespace {

constexpr int kBlock = 256;
constexpr int kBceVpt = 8;
constexpr int kWaves = kBlock / kWave;

__device__ __forceinline__ long long first_element() {
    return ((long long)blockIdx.x * kBlock + threadIdx.x) * kBceVpt;
}

// ---- The per-element terms
struct LossTerm {
    float l, g;  // the loss term and dl/dx
};

// Torch's formula for pos_weight: lw = 1 + (pw - 1) t,  l = (1 - t) x + lw (log1p(exp(-|x|)) + max(-x, 0)),
// dl/dx = lw sigmoid(x) - pw t = (1 - t) sigmoid(x) - pw t sigmoid(-x): no cancellation for saturated x
__device__ __forceinline__ LossTerm bce_term(float xx, float tt, float pw) {
    const float lw = fmaf(pw - 1.f, tt, 1.f);
    const float e = expf(-fabsf(xx));
    const float l = (1.f - tt) * xx + lw * (log1pf(e) + fmaxf(-xx, 0.f));
    const float sp = 1.f / (1.f + e), sn = e / (1.f + e);  // sigmoid(|x|), sigmoid(-|x|)
    const float sx = xx >= 0.f ? sp : sn, smx = xx >= 0.f ? sn : sp;
    return {l, (1.f - tt) * sx - pw * tt * smx};
}

// Focal loss (ABI 29) for imbalanced classes: with q = (t != 0) (the IoU predicate's reading of a label), z = q ? x : -x
// (so p_t = sigmoid(z)) and the class's row (w_pos, w_neg, gamma),
//   l = exp(-gamma softplus(z)) w softplus(-z),   dl/dz = -exp(-gamma softplus(z)) w (gamma sigmoid(z) softplus(-z) + sigmoid(-z)),
// w = q ? w_pos : w_neg and dl/dx = q ? dl/dz : -dl/dz: (1 - p_t)^gamma times the weighted BCE with the power written
// as exp(gamma log(1 - p_t)), so the gradient has no division and no difference of near-equal terms (0 < gamma < 1
// at a saturated, correct element is 0, not inf * 0). softplus(z) = log1p(exp(-|x|)) + max(z, 0); the sigmoids are
// bce_term's.
__device__ __forceinline__ LossTerm focal_term(float xx, float tt, float wp, float wn, float gamma) {
    const bool q = tt != 0.f;
    const float z = q ? xx : -xx;
    const float e = expf(-fabsf(xx));
    const float lp = log1pf(e);
    const float spz = lp + fmaxf(z, 0.f), spm = lp + fmaxf(-z, 0.f);  // softplus(z), softplus(-z)
    const float sp = 1.f / (1.f + e), sn = e / (1.f + e);             // sigmoid(|x|), sigmoid(-|x|)
    const float sz = z >= 0.f ? sp : sn, sm = z >= 0.f ? sn : sp;     // sigmoid(z), sigmoid(-z)
    const float mw = expf(-gamma * spz) * (q ? wp : wn);
    const float gz = mw * (gamma * sz * spm + sm);  // -dl/dz
    return {mw * spm, q ? -gz : gz};
}

struct OneWeight {
    static constexpr bool kPerClass = false;
    float pw;
    __device__ __forceinline__ LossTerm term(float xx, float tt, int) const { return bce_term(xx, tt, pw); }
};
struct ClassWeights {
    static constexpr bool kPerClass = true;
    const float* __restrict__ pwc;
    __device__ __forceinline__ LossTerm term(float xx, float tt, int k) const { return bce_term(xx, tt, pwc[k]); }
};
struct FocalRows {
    static constexpr bool kPerClass = true;
    const float* __restrict__ params;
    __device__ __forceinline__ LossTerm term(float xx, float tt, int k) const {
        const float* pr = params + 3 * k;
        const float wp = pr[0], wn = pr[1], gamma = pr[2];
        return focal_term(xx, tt, wp, wn, gamma);
    }
};

// ---- Walks over a thread's elements
struct ClassWalk {
    long long rem, plane;  // position inside the plane
    int k, K;
    __device__ ClassWalk(long long i0, long long plane_, int K_) : plane(plane_), K(K_) {
        const long long p = i0 / plane_;
        rem = i0 - p * plane_;
        k = (int)(p % K_);
    }
    __device__ __forceinline__ void next() {
        if (++rem == plane) {
            rem = 0;
            k = k + 1 == K ? 0 : k + 1;
        }
    }
};
struct NoWalk {  // OneWeight's: every element is of class 0
    static constexpr int k = 0;
    __device__ NoWalk(long long, long long, int) {}
    __device__ __forceinline__ void next() {}
};

// Element i of the (batch, K, plane) logits reads valid[(i / (K plane)) plane + i % plane]. ClassWalk with that index
// walked beside it: inside a plane both advance by one, at the end of a class plane the mask index goes back to the
// plane's start, at the end of a sample it runs on into the next plane.
struct MaskWalk {
    long long rem, plane, vi;  // position inside the plane; index into valid
    int k, K;
    __device__ MaskWalk(long long i0, long long plane_, int K_) : plane(plane_), K(K_) {
        const long long p = i0 / plane_;
        rem = i0 - p * plane_;
        k = (int)(p % K_);
        vi = (p / K_) * plane_ + rem;
    }
    __device__ __forceinline__ void next() {
        ++vi;
        if (++rem == plane) {
            rem = 0;
            k = k + 1 == K ? 0 : k + 1;
            if (k != 0) vi -= plane;
        }
    }
};

// A thread's 8 mask bytes into bit j of the result: one 8-byte load when the 8 elements lie in one plane at an
// 8-byte aligned address (plane % 8 == 0: always), else a byte each, walked as the classes are. No bit is set at or
// past n.
__device__ __forceinline__ unsigned mask_bits(const uint8_t* __restrict__ valid, long long i0, long long n,
                                               long long plane, int K) {
    MaskWalk mw(i0, plane, K);
    unsigned bits = 0;
    if (i0 + kBceVpt <= n && mw.rem + kBceVpt <= plane && ((reinterpret_cast<uintptr_t>(valid) + mw.vi) & 7) == 0) {
        const uint2 w = *reinterpret_cast<const uint2*>(valid + mw.vi);
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            bits |= ((w.x >> (8 * j)) & 0xFFu) ? 1u << j : 0u;
            bits |= ((w.y >> (8 * j)) & 0xFFu) ? 1u << (4 + j) : 0u;
        }
        return bits;
    }
#pragma unroll
    for (int j = 0; j < kBceVpt; ++j) {
        if (i0 + j < n && valid[mw.vi]) bits |= 1u << j;
        mw.next();
    }
    return bits;
}

// ---- Loads, stores, folds
// A thread's 8 logits and labels: two or three 16-byte loads when `vec` (all 8 below `bound`, aligned bases), else
// element by element with 0 at and past `bound`.
template <typename T>
__device__ __forceinline__ void load8(const T* __restrict__ x, const float* __restrict__ t, long long i0, long long bound,
                                      bool vec, float (&xv)[kBceVpt], float (&tv)[kBceVpt]) {
    if (vec) {
        ldv<8>(x + i0, xv);
        const float4 a = *reinterpret_cast<const float4*>(t + i0), b = *reinterpret_cast<const float4*>(t + i0 + 4);
        tv[0] = a.x; tv[1] = a.y; tv[2] = a.z; tv[3] = a.w; tv[4] = b.x; tv[5] = b.y; tv[6] = b.z; tv[7] = b.w;
    } else {
#pragma unroll
        for (int j = 0; j < kBceVpt; ++j) {
            xv[j] = i0 + j < bound ? ld(x + i0 + j) : 0.f;
            tv[j] = i0 + j < bound ? t[i0 + j] : 0.f;
        }
    }
}

// The fold of a block, for float, double and integer sums alike: lanes_sum over all the sums of the kernel at once (their
// butterflies interleave; one after the other, three 64-bit sums are three times the dependent shuffles), fold_stage for
// each, one __syncthreads(), then thread 0 takes fold_waves of each.
template <typename... S> __device__ __forceinline__ void lanes_sum(S&... s) {
#pragma unroll
    for (int o = kWave / 2; o > 0; o >>= 1) ((s += __shfl_xor(s, o, kWave)), ...);
}
template <typename S> __device__ __forceinline__ void fold_stage(S s, S* s_w) {  // s: lanes_sum's
    if ((threadIdx.x & (kWave - 1)) == 0) s_w[threadIdx.x / kWave] = s;
}
template <typename S> __device__ __forceinline__ S fold_waves(const S* s_w) {
    S b = 0;
#pragma unroll
    for (int w = 0; w < kWaves; ++w) b += s_w[w];
    return b;
}

// n_valid (NULL: the whole batch) clamped to [0, batch]
__device__ __forceinline__ int clamp_valid(const int* __restrict__ n_valid, int batch) {
    const int nv = n_valid ? n_valid[0] : batch;
    return nv < 0 ? 0 : (nv > batch ? batch : nv);
}

// ---- Training
// (The second launch bound holds the masked instantiations to the 64 registers of 8 waves per SIMD: left alone the
// compiler stops at 65 for fp32, one past the step, and at 68 for bf16, whose unpacking it then schedules differently;
// 1 asks for nothing.)
template <typename T, typename P, bool MASKED>
__global__ __launch_bounds__(kBlock, MASKED ? 8 : 1) void k_sig_loss_fwd(const T* __restrict__ x, const float* __restrict__ t,
                                                         const uint8_t* __restrict__ valid, long long n, long long plane,
                                                         int K, P pol, float inv_n, float* __restrict__ partial,
                                                         int* __restrict__ counts, T* __restrict__ grad) {
    __shared__ float s_w[kWaves];
    __shared__ int s_m[kWaves];  // (MASKED only)
    const long long i0 = first_element();
    float xv[kBceVpt], tv[kBceVpt], gv[kBceVpt];
    const bool full = i0 + kBceVpt <= n;
    load8(x, t, i0, n, full, xv, tv);
    unsigned bits = 0;
    if constexpr (MASKED) {
        if (i0 < n) bits = mask_bits(valid, i0, n, plane, K);
    }
    std::conditional_t<P::kPerClass, ClassWalk, NoWalk> cw(i0, plane, K);
    float s = 0.f;
#pragma unroll
    for (int j = 0; j < kBceVpt; ++j) {
        const LossTerm f = pol.term(xv[j], tv[j], cw.k);
        cw.next();
        if constexpr (MASKED) {
            const bool on = (bits >> j) & 1u;
            gv[j] = on ? f.g * inv_n : 0.f;
            s += on ? f.l : 0.f;
        } else {
            gv[j] = f.g * inv_n;
            if (i0 + j < n) s += f.l;
        }
    }
    if (full) stv<8>(grad + i0, gv);
    else {
#pragma unroll
        for (int j = 0; j < kBceVpt; ++j)
            if (i0 + j < n) st(grad + i0 + j, gv[j]);
    }
    int m = __popc(bits);
    if constexpr (MASKED) lanes_sum(s, m);
    else lanes_sum(s);
    fold_stage(s, s_w);
    if constexpr (MASKED) fold_stage(m, s_m);
    __syncthreads();
    if (threadIdx.x == 0) {
        partial[blockIdx.x] = fold_waves(s_w);
        if constexpr (MASKED) counts[blockIdx.x] = fold_waves(s_m);
    }
}

// The block partials (lanes strided over blocks, then a butterfly) into loss = sum / n, or with the counts beside them
// (integers) into loss = sum / max(M, 1) and scale = n / max(M, 1). c = 1 / n, or n when MASKED.
template <bool MASKED>
__global__ __launch_bounds__(kWave) void k_sig_loss_total(const float* __restrict__ partial, const int* __restrict__ counts,
                                                          int nb, float c, float* __restrict__ loss,
                                                          float* __restrict__ scale) {
    float s = 0.f;
    long long m = 0;
    for (int b = threadIdx.x; b < nb; b += kWave) {
        s += partial[b];
        if constexpr (MASKED) m += counts[b];
    }
#pragma unroll
    for (int o = kWave / 2; o > 0; o >>= 1) {
        s += __shfl_xor(s, o, kWave);
        if constexpr (MASKED) m += __shfl_xor(m, o, kWave);
    }
    if (threadIdx.x == 0) {
        if constexpr (MASKED) {
            const float d = (float)(m > 0 ? m : 1);
            loss[0] = s / d;
            scale[0] = c / d;
        } else {
            loss[0] = s * c;
        }
    }
}

// dx = grad * gout[0] (the incoming gradient of the loss, read on the device), rounded once to T; SCALED: times
// scale[0] too, the normalisation a forward could not apply
template <typename T, bool SCALED>
__global__ __launch_bounds__(kBlock) void k_sig_loss_bwd(const T* __restrict__ grad, long long n,
                                                         const float* __restrict__ gout, const float* __restrict__ scale,
                                                         T* __restrict__ dx) {
    const long long i0 = first_element();
    float gs = gout[0];
    if constexpr (SCALED) gs = gout[0] * scale[0];
    float v[kBceVpt];
    if (i0 + kBceVpt <= n) {
        ldv<8>(grad + i0, v);
#pragma unroll
        for (int j = 0; j < kBceVpt; ++j) v[j] *= gs;
        stv<8>(dx + i0, v);
    } else {
        for (long long i = i0; i < n; ++i) st(dx + i, ld(grad + i) * gs);
    }
}

// ---- Validation
// The fp64 loss records of the blocks strided over the fold kernel's one block and staged for fold_waves.
__device__ __forceinline__ void loss_records_stage(const double* __restrict__ ploss, int nb, double* s_l) {
    double s = 0.0;
    for (int b = threadIdx.x; b < nb; b += kBlock) s += ploss[b];
    lanes_sum(s);
    fold_stage(s, s_l);
}

struct BceIouPartial {
    double loss;
    long long inter, uni;
};
template <typename T>
__global__ __launch_bounds__(kBlock) void k_bce_iou(const T* __restrict__ x, const float* __restrict__ t,
                                                    long long per_sample, int batch, const int* __restrict__ n_valid,
                                                    float pw, int vec, BceIouPartial* __restrict__ partial) {
    __shared__ double s_l[kWaves];
    __shared__ int s_i[kWaves], s_u[kWaves];
    const long long limit = (long long)clamp_valid(n_valid, batch) * per_sample;
    const long long i0 = first_element();
    double s = 0.0;
    int ni = 0, nu = 0;
    if (i0 < limit) {
        float xv[kBceVpt], tv[kBceVpt];
        load8(x, t, i0, limit, vec && i0 + kBceVpt <= limit, xv, tv);
#pragma unroll
        for (int j = 0; j < kBceVpt; ++j) {
            const float xx = xv[j], tt = tv[j];
            const float l = bce_term(xx, tt, pw).l;
            if (i0 + j < limit) {
                s += (double)l;
                const bool p = xx > 0.f, q = tt != 0.f;
                ni += (p && q) ? 1 : 0;
                nu += (p || q) ? 1 : 0;
            }
        }
    }
    lanes_sum(s, ni, nu);
    fold_stage(s, s_l);
    fold_stage(ni, s_i);
    fold_stage(nu, s_u);
    __syncthreads();
    if (threadIdx.x == 0) partial[blockIdx.x] = BceIouPartial{fold_waves(s_l), fold_waves(s_i), fold_waves(s_u)};
}

// totals[0] += (the loss records in block order) / per_sample, totals[1] += intersection, totals[2] += union
__global__ __launch_bounds__(kBlock) void k_bce_iou_fold(const BceIouPartial* __restrict__ partial, int nb,
                                                         double per_sample, double* __restrict__ totals) {
    __shared__ double s_l[kWaves];
    __shared__ long long s_i[kWaves], s_u[kWaves];
    double s = 0.0;
    long long ni = 0, nu = 0;
    for (int b = threadIdx.x; b < nb; b += kBlock) {  // (a record is read once: the loss and the counts together)
        const BceIouPartial r = partial[b];
        s += r.loss;
        ni += r.inter;
        nu += r.uni;
    }
    lanes_sum(s, ni, nu);
    fold_stage(s, s_l);
    fold_stage(ni, s_i);
    fold_stage(nu, s_u);
    __syncthreads();
    if (threadIdx.x == 0) {
        totals[0] += fold_waves(s_l) / per_sample;
        totals[1] += (double)fold_waves(s_i);
        totals[2] += (double)fold_waves(s_u);
    }
}

// Block record of the per-class metrics: partial = nb doubles (the loss terms), then nb x 2K int32 (intersection
// counts of the K classes, then union counts). A thread counts a run of one class in registers and adds it to the
// block's LDS counters when the class changes (integer adds: any order). K = 1 gives k_bce_iou's bits.
constexpr int kIouMaxClasses = 32;
template <typename T>
__global__ __launch_bounds__(kBlock) void k_bce_iou_pc(const T* __restrict__ x, const float* __restrict__ t,
                                                       long long per_sample, int batch, const int* __restrict__ n_valid,
                                                       long long plane, int K, const float* __restrict__ pwc, int vec,
                                                       double* __restrict__ ploss, int* __restrict__ pcount) {
    __shared__ double s_l[kWaves];
    __shared__ int s_c[2 * kIouMaxClasses];
    if (threadIdx.x < 2 * K) s_c[threadIdx.x] = 0;
    __syncthreads();
    const long long limit = (long long)clamp_valid(n_valid, batch) * per_sample;
    const long long i0 = first_element();
    double s = 0.0;
    if (i0 < limit) {
        float xv[kBceVpt], tv[kBceVpt];
        load8(x, t, i0, limit, vec && i0 + kBceVpt <= limit, xv, tv);
        ClassWalk cw(i0, plane, K);
        int ni = 0, nu = 0;
#pragma unroll
        for (int j = 0; j < kBceVpt; ++j) {
            const float xx = xv[j], tt = tv[j];
            const int k = cw.k;
            const float l = bce_term(xx, tt, pwc[k]).l;
            cw.next();
            if (i0 + j < limit) {
                s += (double)l;
                const bool p = xx > 0.f, q = tt != 0.f;
                ni += (p && q) ? 1 : 0;
                nu += (p || q) ? 1 : 0;
            }
            if (j == kBceVpt - 1 || cw.k != k) {  // the run of class k ends here
                if (ni) atomicAdd(&s_c[k], ni);
                if (nu) atomicAdd(&s_c[K + k], nu);
                ni = nu = 0;
            }
        }
    }
    lanes_sum(s);
    fold_stage(s, s_l);
    __syncthreads();
    if (threadIdx.x == 0) ploss[blockIdx.x] = fold_waves(s_l);
    if (threadIdx.x < 2 * K) pcount[(size_t)blockIdx.x * 2 * K + threadIdx.x] = s_c[threadIdx.x];
}

// totals[0] += (the loss records in block order) / per_sample; totals[1 + k] += intersection of class k,
// totals[1 + K + k] += its union (wave w sums the counters w, w + 4, ... over the blocks: integers).
__global__ __launch_bounds__(kBlock) void k_bce_iou_fold_pc(const double* __restrict__ ploss,
                                                            const int* __restrict__ pcount, int nb, int K,
                                                            double per_sample, double* __restrict__ totals) {
    __shared__ double s_l[kWaves];
    loss_records_stage(ploss, nb, s_l);
    __syncthreads();
    if (threadIdx.x == 0) totals[0] += fold_waves(s_l) / per_sample;
    const int lane = threadIdx.x & (kWave - 1);
    for (int c = threadIdx.x / kWave; c < 2 * K; c += kWaves) {
        long long a = 0;
        for (int b = lane; b < nb; b += kWave) a += pcount[(size_t)b * 2 * K + c];
#pragma unroll
        for (int o = kWave / 2; o > 0; o >>= 1) a += __shfl_xor(a, o, kWave);
        if (lane == 0) totals[1 + c] += (double)a;
    }
}

// Either loss and a ladder of T ascending logit thresholds (ABI 29). Since theta ascends, x > theta_j holds exactly for
// j < bin(x) = #(j: x > theta_j): an element adds one to the block's LDS histogram h[class][bin][q], q = (t != 0).
// Block record: partial = nb doubles (the loss terms of focal_term), then nb x nrec int32, nrec = K (T + 1) 2 histogram
// slots and, MASKED, the block's count of valid elements behind them.
constexpr int kSegMaxThresholds = 16;
constexpr int kSegMaxHist = kIouMaxClasses * (kSegMaxThresholds + 1) * 2;
template <typename T, bool MASKED>
__global__ __launch_bounds__(kBlock) void k_seg_metrics(const T* __restrict__ x, const float* __restrict__ t,
                                                        const uint8_t* __restrict__ valid, long long per_sample,
                                                        int batch, const int* __restrict__ n_valid, long long plane, int K,
                                                        FocalRows pol, const float* __restrict__ thetas, int nt, int vec,
                                                        double* __restrict__ ploss, int* __restrict__ pcount) {
    __shared__ double s_l[kWaves];
    __shared__ int s_h[kSegMaxHist + (MASKED ? 1 : 0)];
    __shared__ float s_th[kSegMaxThresholds];
    const int nh = K * (nt + 1) * 2, nrec = nh + (MASKED ? 1 : 0);
    for (int c = threadIdx.x; c < nrec; c += kBlock) s_h[c] = 0;
    if (threadIdx.x < nt) s_th[threadIdx.x] = thetas[threadIdx.x];
    __syncthreads();
    const long long limit = (long long)clamp_valid(n_valid, batch) * per_sample;
    const long long i0 = first_element();
    double s = 0.0;
    if (i0 < limit) {
        float xv[kBceVpt], tv[kBceVpt];
        load8(x, t, i0, limit, vec && i0 + kBceVpt <= limit, xv, tv);
        unsigned bits = 0;
        if constexpr (MASKED) bits = mask_bits(valid, i0, limit, plane, K);
        ClassWalk cw(i0, plane, K);
#pragma unroll
        for (int j = 0; j < kBceVpt; ++j) {
            const float xx = xv[j], tt = tv[j];
            const int k = cw.k;
            const LossTerm f = pol.term(xx, tt, k);
            cw.next();
            const bool on = MASKED ? ((bits >> j) & 1u) != 0 : i0 + j < limit;
            if (on) {
                s += (double)f.l;
                int bin = 0;
                for (int m = 0; m < nt; ++m) bin += xx > s_th[m] ? 1 : 0;
                atomicAdd(&s_h[(k * (nt + 1) + bin) * 2 + (tt != 0.f ? 1 : 0)], 1);
            }
        }
        if constexpr (MASKED) {
            if (bits) atomicAdd(&s_h[nh], __popc(bits));
        }
    }
    lanes_sum(s);
    fold_stage(s, s_l);
    __syncthreads();
    if (threadIdx.x == 0) ploss[blockIdx.x] = fold_waves(s_l);
    for (int c = threadIdx.x; c < nrec; c += kBlock) pcount[(size_t)blockIdx.x * nrec + c] = s_h[c];
}

// Count c of the totals from the batch's histogram h by suffix sums over the bins:
//   P_k = sum_b h[k][b][1],  TP_kj = sum_{b > j} h[k][b][1],  PP_kj = sum_{b > j} (h[k][b][0] + h[k][b][1]),
// c = k for P, K + k T + j for TP, K + K T + k T + j for PP.
__device__ __forceinline__ long long seg_count(const long long* h, int c, int K, int nt) {
    long long a = 0;
    if (c < K) {
        for (int b = 0; b <= nt; ++b) a += h[(c * (nt + 1) + b) * 2 + 1];
    } else {
        const int r = c - K, pp = r >= K * nt, kj = pp ? r - K * nt : r, k = kj / nt, j = kj - k * nt;
        for (int b = j + 1; b <= nt; ++b) a += h[(k * (nt + 1) + b) * 2 + 1] + (pp ? h[(k * (nt + 1) + b) * 2] : 0);
    }
    return a;
}

// The histograms summed over the blocks (integers) into LDS, then totals[1 + c] += seg_count(c). The loss records in
// block order: totals[0] += sum / per_sample, or, MASKED, with M the valid elements of the batch (K per valid cell) and
// nv the clamped n_valid, totals[0] += nv sum / max(M, 1) -- the masked batch mean times the batch size -- and
// valid_cells[0] += M / K (when not NULL).
template <bool MASKED>
__global__ __launch_bounds__(kBlock) void k_seg_metrics_fold(const double* __restrict__ ploss,
                                                             const int* __restrict__ pcount, int nb, int K, int nt,
                                                             double per_sample, int batch, const int* __restrict__ n_valid,
                                                             double* __restrict__ totals, double* __restrict__ valid_cells) {
    __shared__ double s_l[kWaves];
    __shared__ long long s_m[kWaves];  // (MASKED only)
    __shared__ long long s_h[kSegMaxHist];
    const int nh = K * (nt + 1) * 2, nrec = nh + (MASKED ? 1 : 0);
    loss_records_stage(ploss, nb, s_l);
    if constexpr (MASKED) {
        long long m = 0;
        for (int b = threadIdx.x; b < nb; b += kBlock) m += pcount[(size_t)b * nrec + nh];
        lanes_sum(m);
        fold_stage(m, s_m);
    }
    for (int c = threadIdx.x; c < nh; c += kBlock) {
        long long a = 0;
        for (int b = 0; b < nb; ++b) a += pcount[(size_t)b * nrec + c];
        s_h[c] = a;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        const double l = fold_waves(s_l);
        if constexpr (MASKED) {
            const long long M = fold_waves(s_m);
            totals[0] += (double)clamp_valid(n_valid, batch) * l / (double)(M > 0 ? M : 1);
            if (valid_cells) valid_cells[0] += (double)(M / K);
        } else {
            totals[0] += l / per_sample;
        }
    }
    for (int c = threadIdx.x; c < K + 2 * K * nt; c += kBlock) totals[1 + c] += (double)seg_count(s_h, c, K, nt);
}

// ---- host side
// The grid of n elements of dtype: blocks of kBlock threads x 8 elements. 0 refuses the call: an unknown dtype,
// n <= 0, or more blocks than a grid holds.
long long sig_blocks(int32_t dtype, long long n) {
    if ((dtype != LSS_CONV_BF16 && dtype != LSS_CONV_F32) || n <= 0) return 0;
    const long long nb = lss_bce_partials(n);
    return nb > INT_MAX ? 0 : nb;
}
// per_sample * batch, or 0 when either is not positive or the product overflows
long long batch_elements(int64_t per_sample, int32_t batch) {
    return per_sample > 0 && batch > 0 && per_sample <= LLONG_MAX / batch ? (long long)per_sample * batch : 0;
}
// some pointer has a bit of `mask` set (NULL passes)
template <typename... P> bool misaligned(uintptr_t mask, P... p) {
    return ((... | reinterpret_cast<uintptr_t>(p)) & mask) != 0;
}

// One launch of KERNEL, written with T for the element type, over nb blocks: T = bf16 or float by dtype
#define LSS_SIG_LAUNCH(dtype, nb, s, KERNEL, ...)                                                                    \
    do {                                                                                                             \
        const dim3 g_((unsigned)(nb)), b_(kBlock);                                                                   \
        if ((dtype) == LSS_CONV_BF16) {                                                                              \
            using T = bf16;                                                                                          \
            hipLaunchKernelGGL(KERNEL, g_, b_, 0, s, __VA_ARGS__);                                                   \
        } else {                                                                                                     \
            using T = float;                                                                                         \
            hipLaunchKernelGGL(KERNEL, g_, b_, 0, s, __VA_ARGS__);                                                   \
        }                                                                                                            \
    } while (0)

// k_sig_loss_fwd<T, P, MASKED> and its fold, behind the four training entries (which have checked their arguments)
template <typename P, bool MASKED>
int sig_loss_launch(const void* x, int32_t dtype, const float* target, const uint8_t* valid, int64_t n, int64_t plane,
                    int32_t K, P pol, long long nb, float* partial, float* loss, float* scale, void* grad, void* stream) {
    const float inv_n = 1.0f / (float)n;
    hipStream_t s = (hipStream_t)stream;
    int* counts = MASKED ? reinterpret_cast<int*>(partial + nb) : nullptr;
    LSS_SIG_LAUNCH(dtype, nb, s, (k_sig_loss_fwd<T, P, MASKED>), (const T*)x, target, valid, (long long)n, (long long)plane,
                   (int)K, pol, inv_n, partial, counts, (T*)grad);
    hipLaunchKernelGGL(k_sig_loss_total<MASKED>, dim3(1), dim3(kWave), 0, s, (const float*)partial, (const int*)counts,
                       (int)nb, MASKED ? (float)n : inv_n, loss, scale);
    return launch_status();
}

template <bool SCALED>
int sig_loss_bwd_launch(const void* grad, int32_t dtype, int64_t n, long long nb, const float* grad_loss,
                        const float* scale, void* dx, void* stream) {
    LSS_SIG_LAUNCH(dtype, nb, (hipStream_t)stream, (k_sig_loss_bwd<T, SCALED>), (const T*)grad, (long long)n, grad_loss,
                   scale, (T*)dx);
    return launch_status();
}

// k_seg_metrics<T, MASKED> and its fold, behind the two ladder entries (which have checked their arguments)
template <bool MASKED>
int seg_metrics_launch(const void* x, int32_t dtype, const float* target, const uint8_t* valid, int64_t per_sample,
                       int32_t batch, const int32_t* n_valid, int64_t plane, int32_t K, const float* params,
                       const float* thetas, int32_t nt, long long nb, double* totals, double* valid_cells, void* partial,
                       void* stream) {
    const int vec = !misaligned(15, x, target);
    hipStream_t s = (hipStream_t)stream;
    double* pl = (double*)partial;
    int* pc = (int*)(pl + nb);
    LSS_SIG_LAUNCH(dtype, nb, s, (k_seg_metrics<T, MASKED>), (const T*)x, target, valid, (long long)per_sample, (int)batch,
                   (const int*)n_valid, (long long)plane, (int)K, FocalRows{params}, thetas, (int)nt, vec, pl, pc);
    hipLaunchKernelGGL(k_seg_metrics_fold<MASKED>, dim3(1), dim3(kBlock), 0, s, (const double*)pl, (const int*)pc, (int)nb,
                       (int)K, (int)nt, (double)per_sample, (int)batch, (const int*)n_valid, totals, valid_cells);
    return launch_status();
}

}  // namespace

extern "C" {

int64_t lss_bce_partials(int64_t n) { return (n + (int64_t)kBlock * kBceVpt - 1) / ((int64_t)kBlock * kBceVpt); }

int lss_bce_logits(const void* x, int32_t dtype, const float* target, int64_t n, float pos_weight, float* partial,
                   float* loss, void* grad, void* stream) {
    const long long nb = sig_blocks(dtype, n);
    if (!x || !target || !partial || !loss || !grad || !nb || misaligned(15, x, grad, target)) return LSS_CONV_EINVAL;
    return sig_loss_launch<OneWeight, false>(x, dtype, target, nullptr, n, 1, 1, OneWeight{pos_weight}, nb, partial, loss,
                                             nullptr, grad, stream);
}

int lss_bce_logits_bwd(const void* grad, int32_t dtype, int64_t n, const float* grad_loss, void* dx, void* stream) {
    const long long nb = sig_blocks(dtype, n);
    if (!grad || !grad_loss || !dx || !nb || misaligned(15, grad, dx)) return LSS_CONV_EINVAL;
    return sig_loss_bwd_launch<false>(grad, dtype, n, nb, grad_loss, nullptr, dx, stream);
}

int lss_bce_logits_pc(const void* x, int32_t dtype, const float* target, int64_t n, int64_t plane, int32_t K,
                      const float* pos_weight, float* partial, float* loss, void* grad, void* stream) {
    const long long nb = sig_blocks(dtype, n);
    if (!x || !target || !pos_weight || !partial || !loss || !grad || !nb || plane <= 0 || K <= 0 ||
        misaligned(15, x, grad, target))
        return LSS_CONV_EINVAL;
    return sig_loss_launch<ClassWeights, false>(x, dtype, target, nullptr, n, plane, K, ClassWeights{pos_weight}, nb,
                                                partial, loss, nullptr, grad, stream);
}

int lss_focal_logits_pc(const void* x, int32_t dtype, const float* target, int64_t n, int64_t plane, int32_t K,
                        const float* params, float* partial, float* loss, void* grad, void* stream) {
    const long long nb = sig_blocks(dtype, n);
    if (!x || !target || !params || !partial || !loss || !grad || !nb || plane <= 0 || K <= 0 ||
        misaligned(15, x, grad, target) || misaligned(3, params))
        return LSS_CONV_EINVAL;
    return sig_loss_launch<FocalRows, false>(x, dtype, target, nullptr, n, plane, K, FocalRows{params}, nb, partial, loss,
                                             nullptr, grad, stream);
}

int lss_seg_loss_masked(const void* x, int32_t dtype, const float* target, const uint8_t* valid, int64_t n,
                        int64_t plane, int32_t K, const float* params, float* partial, float* loss, float* scale,
                        void* grad, void* stream) {
    const long long nb = sig_blocks(dtype, n);
    if (!x || !target || !valid || !params || !partial || !loss || !scale || !grad || !nb || plane <= 0 || K <= 0 ||
        plane > LLONG_MAX / K || n % (plane * K) != 0 || misaligned(15, x, grad, target) ||
        misaligned(3, params, partial, scale))
        return LSS_CONV_EINVAL;
    return sig_loss_launch<FocalRows, true>(x, dtype, target, valid, n, plane, K, FocalRows{params}, nb, partial, loss,
                                            scale, grad, stream);
}

int lss_seg_loss_masked_bwd(const void* grad, int32_t dtype, int64_t n, const float* grad_loss, const float* scale,
                            void* dx, void* stream) {
    const long long nb = sig_blocks(dtype, n);
    if (!grad || !grad_loss || !scale || !dx || !nb || misaligned(15, grad, dx) || misaligned(3, grad_loss, scale))
        return LSS_CONV_EINVAL;
    return sig_loss_bwd_launch<true>(grad, dtype, n, nb, grad_loss, scale, dx, stream);
}

int64_t lss_bce_iou_partial_bytes(int64_t n) {
    return n <= 0 ? 0 : lss_bce_partials(n) * (int64_t)sizeof(BceIouPartial);
}

// (the accumulate entries take 16-byte loads only from 16-byte aligned bases -- a thread's first element is a multiple
// of 8 -- and any alignment otherwise: vec)
int lss_bce_iou_accum(const void* x, int32_t dtype, const float* target, int64_t per_sample, int32_t batch,
                      const int32_t* n_valid, float pos_weight, double* totals, void* partial, void* stream) {
    const long long nb = sig_blocks(dtype, batch_elements(per_sample, batch));
    if (!x || !target || !totals || !partial || !nb || misaligned(7, partial, totals)) return LSS_CONV_EINVAL;
    const int vec = !misaligned(15, x, target);
    hipStream_t s = (hipStream_t)stream;
    BceIouPartial* pp = (BceIouPartial*)partial;
    LSS_SIG_LAUNCH(dtype, nb, s, k_bce_iou<T>, (const T*)x, target, (long long)per_sample, (int)batch,
                   (const int*)n_valid, pos_weight, vec, pp);
    hipLaunchKernelGGL(k_bce_iou_fold, dim3(1), dim3(kBlock), 0, s, (const BceIouPartial*)pp, (int)nb,
                       (double)per_sample, totals);
    return launch_status();
}

int64_t lss_bce_iou_pc_partial_bytes(int64_t n, int32_t K) {
    return n <= 0 || K <= 0 ? 0 : lss_bce_partials(n) * (int64_t)(sizeof(double) + 2 * (size_t)K * sizeof(int));
}

int lss_bce_iou_accum_pc(const void* x, int32_t dtype, const float* target, int64_t per_sample, int32_t batch,
                         const int32_t* n_valid, int64_t plane, int32_t K, const float* pos_weight, double* totals,
                         void* partial, void* stream) {
    const long long nb = sig_blocks(dtype, batch_elements(per_sample, batch));
    if (!x || !target || !pos_weight || !totals || !partial || !nb || plane <= 0 || K <= 0 || K > kIouMaxClasses ||
        per_sample != plane * K || misaligned(7, partial, totals))
        return LSS_CONV_EINVAL;
    const int vec = !misaligned(15, x, target);
    hipStream_t s = (hipStream_t)stream;
    double* pl = (double*)partial;
    int* pc = (int*)(pl + nb);
    LSS_SIG_LAUNCH(dtype, nb, s, k_bce_iou_pc<T>, (const T*)x, target, (long long)per_sample, (int)batch,
                   (const int*)n_valid, (long long)plane, (int)K, pos_weight, vec, pl, pc);
    hipLaunchKernelGGL(k_bce_iou_fold_pc, dim3(1), dim3(kBlock), 0, s, (const double*)pl, (const int*)pc, (int)nb, (int)K,
                       (double)per_sample, totals);
    return launch_status();
}

int64_t lss_seg_metrics_partial_bytes(int64_t n, int32_t K, int32_t T) {
    return n <= 0 || K <= 0 || K > kIouMaxClasses || T <= 0 || T > kSegMaxThresholds
               ? 0
               : lss_bce_partials(n) * (int64_t)(sizeof(double) + 2 * (size_t)K * (size_t)(T + 1) * sizeof(int));
}

int64_t lss_seg_metrics_masked_partial_bytes(int64_t n, int32_t K, int32_t T) {
    return n <= 0 || K <= 0 || K > kIouMaxClasses || T <= 0 || T > kSegMaxThresholds
               ? 0
               : lss_bce_partials(n) * (int64_t)(sizeof(double) + 2 * ((size_t)K * (size_t)(T + 1) + 1) * sizeof(int));
}

int lss_seg_metrics_accum(const void* x, int32_t dtype, const float* target, int64_t per_sample, int32_t batch,
                          const int32_t* n_valid, int64_t plane, int32_t K, const float* params, const float* thetas,
                          int32_t T, double* totals, void* partial, void* stream) {
    const long long nb = sig_blocks(dtype, batch_elements(per_sample, batch));
    if (!x || !target || !params || !thetas || !totals || !partial || !nb || plane <= 0 || K <= 0 ||
        K > kIouMaxClasses || T <= 0 || T > kSegMaxThresholds || per_sample != plane * K ||
        misaligned(7, partial, totals) || misaligned(3, params, thetas))
        return LSS_CONV_EINVAL;
    return seg_metrics_launch<false>(x, dtype, target, nullptr, per_sample, batch, n_valid, plane, K, params, thetas, T,
                                     nb, totals, nullptr, partial, stream);
}

int lss_seg_metrics_accum_masked(const void* x, int32_t dtype, const float* target, const uint8_t* valid,
                                 int64_t per_sample, int32_t batch, const int32_t* n_valid, int64_t plane, int32_t K,
                                 const float* params, const float* thetas, int32_t T, double* totals,
                                 double* valid_cells, void* partial, void* stream) {
    const long long nb = sig_blocks(dtype, batch_elements(per_sample, batch));
    if (!x || !target || !valid || !params || !thetas || !totals || !partial || !nb || plane <= 0 || K <= 0 ||
        K > kIouMaxClasses || T <= 0 || T > kSegMaxThresholds || per_sample != plane * K ||
        misaligned(7, partial, totals, valid_cells) || misaligned(3, params, thetas))
        return LSS_CONV_EINVAL;
    return seg_metrics_launch<true>(x, dtype, target, valid, per_sample, batch, n_valid, plane, K, params, thetas, T, nb,
                                    totals, valid_cells, partial, stream);
}

}  // extern "C"

// ---- Exclusive classes (ABI 34): softmax cross-entropy over (batch, C, plane) logits against a (batch, plane) uint8
// class map, the argmax class map and a C x C confusion matrix. A cell counts iff its label is < C and its mask byte
// (when there is a mask) is != 0; a cell that does not count is selected out -- nothing of it reaches a sum, a count
// or a gradient, whatever its logits are. Per counted cell, fp32, channel sums in ascending c:
//   m = max_c x_c,  e_c = exp(x_c - m),  S = sum_c e_c,  l = w_y ((m - x_y) + log S),
//   dl/dx_c = w_y e_c / S (c != y),  dl/dx_y = -w_y (sum_{c != y} e_c) / S
// -- p_y - 1 written as minus the other classes' share, so a confident, correct cell (p_y one ulp from 1) keeps a
// gradient with full relative precision. Two arms share every line of arithmetic:
//   vector  <T, C, 8>: plane % 8 == 0 and aligned bases. Thread = 8 consecutive cells of one sample: one 8-B label
//           load, one 8-B mask load (the labels again when there is no mask: the address is never conditional) and C
//           16-B (bf16) or 2 x 16-B (fp32) loads of the logits, all issued before the first use. Instantiated per C,
//           so no channel is guarded. A thread past the last group loads the last group's addresses and stores nothing.
//   scalar  <T, 8, 1>: thread = one cell, any plane and alignment. Channel c >= C reads channel C - 1 (a clamped
//           address, not a guarded load) and takes the value -inf: e_c = 0 leaves S, the sums and the argmax as they
//           are, bit for bit.
namespace {

constexpr int kCeMaxC = 8;

// pred = argmax_c x_c with a strict > scanning upwards from -inf: ties go to the lowest class, a NaN never wins,
// all-NaN (or all -inf) gives 0.
template <int C> __device__ __forceinline__ int argmax_class(const float (&x)[C]) {
    int best = 0;
    float bv = -INFINITY;
#pragma unroll
    for (int c = 0; c < C; ++c) {
        const bool gt = x[c] > bv;
        best = gt ? c : best;
        bv = gt ? x[c] : bv;
    }
    return best;
}

struct CeTerm {
    float l, w;  // the cell's loss term and its class weight w_y
};
// The label selects x_y and w_y through compare-and-select chains (no indexed register array: no scratch). A label
// >= C selects nothing (l = w = 0 from finite logits); the caller drops the term of a cell that does not count.
template <int C, bool GRAD>
__device__ __forceinline__ CeTerm ce_cell(const float (&x)[C], int y, const float (&w)[C], float inv_n, float (&g)[C]) {
    float m = x[0];
#pragma unroll
    for (int c = 1; c < C; ++c) m = fmaxf(m, x[c]);
    float e[C], S = 0.f, so = 0.f, xy = m, wy = 0.f;
#pragma unroll
    for (int c = 0; c < C; ++c) {
        e[c] = expf(x[c] - m);
        S += e[c];
        const bool is = c == y;
        so += is ? 0.f : e[c];
        xy = is ? x[c] : xy;
        wy = is ? w[c] : wy;
    }
    if constexpr (GRAD) {
        const float ws = wy * inv_n;
#pragma unroll
        for (int c = 0; c < C; ++c) g[c] = ws * (c == y ? -(so / S) : e[c] / S);
    }
    return {wy * ((m - xy) + logf(S)), wy};
}

// A thread's cells: `live` (inside the grid of cells), the sample b and the first cell's position r in its plane.
// Past the end everything is clamped to the last group, so every load below has an address inside the tensors.
template <int V> struct CeCoord {
    bool live;
    long long b, r;
    __device__ CeCoord(long long batch, long long plane) {
        const long long per = plane / V, total = batch * per;
        const long long g = (long long)blockIdx.x * kBlock + threadIdx.x;
        live = g < total;
        const long long gc = live ? g : total - 1;
        b = gc / per;
        r = (gc - b * per) * V;
    }
};

template <typename T, int C, int V>
__device__ __forceinline__ void ce_load_x(const T* __restrict__ x, const CeCoord<V>& at, long long plane, int nc,
                                          float (&xv)[V][C]) {
    float raw[C][V];
#pragma unroll
    for (int c = 0; c < C; ++c) {
        const int cc = V == 8 ? c : (c < nc ? c : nc - 1);
        ldv<V>(x + (at.b * nc + cc) * plane + at.r, raw[c]);
    }
#pragma unroll
    for (int c = 0; c < C; ++c)
#pragma unroll
        for (int j = 0; j < V; ++j) xv[j][c] = (V == 8 || c < nc) ? raw[c][j] : -INFINITY;
}

// the V label (or mask) bytes of a thread's cells
template <int V> __device__ __forceinline__ void ce_load_bytes(const uint8_t* __restrict__ p, const CeCoord<V>& at,
                                                               long long plane, int (&o)[V]) {
    if constexpr (V == 8) {
        const uint2 w = *reinterpret_cast<const uint2*>(p + at.b * plane + at.r);
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            o[j] = (int)((w.x >> (8 * j)) & 0xFFu);
            o[4 + j] = (int)((w.y >> (8 * j)) & 0xFFu);
        }
    } else {
        o[0] = p[at.b * plane + at.r];
    }
}

template <int C> __device__ __forceinline__ void ce_load_w(const float* __restrict__ weight, int nc, float (&wv)[C]) {
#pragma unroll
    for (int c = 0; c < C; ++c) wv[c] = weight[c < nc ? c : nc - 1];
}

// Loss terms and the stored gradient dl/dx / n_cells. Block record: partial[block] = sum of l, partial[nb + block] =
// sum of w_y, folded in k_sig_loss_fwd's order (lane, wave butterfly, the 4 waves in order).
template <typename T, int C, int V>
__global__ __launch_bounds__(kBlock) void k_softmax_ce(const T* __restrict__ x, const uint8_t* __restrict__ labels,
                                                       const uint8_t* __restrict__ valid, int use_valid, long long batch,
                                                       long long plane, int nc, const float* __restrict__ weight,
                                                       float inv_n, float* __restrict__ partial, T* __restrict__ grad) {
    __shared__ float s_l[kBlock / kWave], s_w[kBlock / kWave];
    const CeCoord<V> at(batch, plane);
    float xv[V][C], wv[C];
    int yv[V], mv[V];
    ce_load_x<T, C, V>(x, at, plane, nc, xv);
    ce_load_bytes<V>(labels, at, plane, yv);
    ce_load_bytes<V>(valid, at, plane, mv);  // (valid = labels when there is no mask: use_valid = 0)
    ce_load_w<C>(weight, nc, wv);
    float sl = 0.f, sw = 0.f;
#pragma unroll
    for (int j = 0; j < V; ++j) {
        float g[C];
        const CeTerm t = ce_cell<C, true>(xv[j], yv[j], wv, inv_n, g);
        const bool on = at.live && yv[j] < nc && (!use_valid || mv[j] != 0);
        sl += on ? t.l : 0.f;
        sw += on ? t.w : 0.f;
#pragma unroll
        for (int c = 0; c < C; ++c) xv[j][c] = on ? g[c] : 0.f;
    }
    if (at.live) {
#pragma unroll
        for (int c = 0; c < C; ++c) {
            if (V == 8 || c < nc) {
                float o[V];
#pragma unroll
                for (int j = 0; j < V; ++j) o[j] = xv[j][c];
                stv<V>(grad + (at.b * nc + c) * plane + at.r, o);
            }
        }
    }
#pragma unroll
    for (int o = kWave / 2; o > 0; o >>= 1) {
        sl += __shfl_xor(sl, o, kWave);
        sw += __shfl_xor(sw, o, kWave);
    }
    if ((threadIdx.x & (kWave - 1)) == 0) {
        s_l[threadIdx.x / kWave] = sl;
        s_w[threadIdx.x / kWave] = sw;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        float a = 0.f, b = 0.f;
#pragma unroll
        for (int w = 0; w < kBlock / kWave; ++w) {
            a += s_l[w];
            b += s_w[w];
        }
        partial[blockIdx.x] = a;
        partial[gridDim.x + blockIdx.x] = b;
    }
}

// k_sig_loss_total<true>'s fold, of both sums: loss = sum l / max(W, tiny), scale = n_cells / W (0 for W = 0)
__global__ __launch_bounds__(kWave) void k_softmax_ce_total(const float* __restrict__ partial, int nb, float nf,
                                                            float* __restrict__ loss, float* __restrict__ scale) {
    float s = 0.f, w = 0.f;
    for (int b = threadIdx.x; b < nb; b += kWave) {
        s += partial[b];
        w += partial[nb + b];
    }
#pragma unroll
    for (int o = kWave / 2; o > 0; o >>= 1) {
        s += __shfl_xor(s, o, kWave);
        w += __shfl_xor(w, o, kWave);
    }
    if (threadIdx.x == 0) {
        loss[0] = w > 0.f ? s / fmaxf(w, 1.17549435e-38f) : 0.f;
        scale[0] = w > 0.f ? nf / w : 0.f;
    }
}

// The class map of the prediction rule: one byte per cell, 8 bytes per store in the vector arm.
template <typename T, int C, int V>
__global__ __launch_bounds__(kBlock) void k_argmax_classes(const T* __restrict__ x, long long batch, long long plane,
                                                           int nc, uint8_t* __restrict__ out) {
    const CeCoord<V> at(batch, plane);
    float xv[V][C];
    ce_load_x<T, C, V>(x, at, plane, nc, xv);
    if (!at.live) return;
    if constexpr (V == 8) {
        uint2 w = make_uint2(0u, 0u);
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            w.x |= (unsigned)argmax_class<C>(xv[j]) << (8 * j);
            w.y |= (unsigned)argmax_class<C>(xv[4 + j]) << (8 * j);
        }
        *reinterpret_cast<uint2*>(out + at.b * plane + at.r) = w;
    } else {
        out[at.b * plane + at.r] = (uint8_t)argmax_class<C>(xv[0]);
    }
}

// Validation: the counted cells of the first n_valid samples add one to the block's LDS histogram h[y][pred] (integer
// adds: any order) and their loss terms and weights to fp64 sums folded in a fixed order. Block record: pl[block],
// pw[block] (doubles), ph[block][nc nc] (int32).
template <typename T, int C, int V>
__global__ __launch_bounds__(kBlock) void k_confusion(const T* __restrict__ x, const uint8_t* __restrict__ labels,
                                                      const uint8_t* __restrict__ valid, int use_valid, long long batch,
                                                      long long plane, int nc, const int* __restrict__ n_valid,
                                                      const float* __restrict__ weight, double* __restrict__ pl,
                                                      double* __restrict__ pw, int* __restrict__ ph) {
    __shared__ double s_l[kBlock / kWave], s_w[kBlock / kWave];
    __shared__ int s_h[kCeMaxC * kCeMaxC];
    if (threadIdx.x < nc * nc) s_h[threadIdx.x] = 0;
    __syncthreads();
    long long nv = n_valid ? n_valid[0] : batch;
    nv = nv < 0 ? 0 : (nv > batch ? batch : nv);
    const CeCoord<V> at(batch, plane);
    float xv[V][C], wv[C];
    int yv[V], mv[V];
    ce_load_x<T, C, V>(x, at, plane, nc, xv);
    ce_load_bytes<V>(labels, at, plane, yv);
    ce_load_bytes<V>(valid, at, plane, mv);
    ce_load_w<C>(weight, nc, wv);
    double sl = 0.0, sw = 0.0;
#pragma unroll
    for (int j = 0; j < V; ++j) {
        float g[C];
        const CeTerm t = ce_cell<C, false>(xv[j], yv[j], wv, 0.f, g);
        const int pred = argmax_class<C>(xv[j]);
        if (at.live && at.b < nv && yv[j] < nc && (!use_valid || mv[j] != 0)) {
            sl += (double)t.l;
            sw += (double)t.w;
            atomicAdd(&s_h[yv[j] * nc + pred], 1);
        }
    }
#pragma unroll
    for (int o = kWave / 2; o > 0; o >>= 1) {
        sl += __shfl_xor(sl, o, kWave);
        sw += __shfl_xor(sw, o, kWave);
    }
    if ((threadIdx.x & (kWave - 1)) == 0) {
        s_l[threadIdx.x / kWave] = sl;
        s_w[threadIdx.x / kWave] = sw;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        double a = 0.0, b = 0.0;
#pragma unroll
        for (int w = 0; w < kBlock / kWave; ++w) {
            a += s_l[w];
            b += s_w[w];
        }
        pl[blockIdx.x] = a;
        pw[blockIdx.x] = b;
    }
    if (threadIdx.x < nc * nc) ph[(size_t)blockIdx.x * nc * nc + threadIdx.x] = s_h[threadIdx.x];
}

// totals[0] += nv (sum l) / max(W, tiny), the records folded as k_seg_metrics_fold<true> folds its own;
// totals[1 + y nc + pred] += the counts summed over the blocks in block order.
__global__ __launch_bounds__(kBlock) void k_confusion_fold(const double* __restrict__ pl, const double* __restrict__ pw,
                                                           const int* __restrict__ ph, int nb, int nc, int batch,
                                                           const int* __restrict__ n_valid, double* __restrict__ totals) {
    __shared__ double s_l[kBlock / kWave], s_w[kBlock / kWave];
    double s = 0.0, w = 0.0;
    for (int b = threadIdx.x; b < nb; b += kBlock) {
        s += pl[b];
        w += pw[b];
    }
#pragma unroll
    for (int o = kWave / 2; o > 0; o >>= 1) {
        s += __shfl_xor(s, o, kWave);
        w += __shfl_xor(w, o, kWave);
    }
    if ((threadIdx.x & (kWave - 1)) == 0) {
        s_l[threadIdx.x / kWave] = s;
        s_w[threadIdx.x / kWave] = w;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        double l = 0.0, W = 0.0;
#pragma unroll
        for (int i = 0; i < kBlock / kWave; ++i) {
            l += s_l[i];
            W += s_w[i];
        }
        int nv = n_valid ? n_valid[0] : batch;
        nv = nv < 0 ? 0 : (nv > batch ? batch : nv);
        totals[0] += W > 0.0 ? (double)nv * l / fmax(W, 1.17549435e-38) : 0.0;
    }
    if (threadIdx.x < nc * nc) {
        long long a = 0;
        for (int b = 0; b < nb; ++b) a += ph[(size_t)b * nc * nc + threadIdx.x];
        totals[1 + threadIdx.x] += (double)a;
    }
}

// One launch of KERNEL's vector arm <T, C, 8> for the call's C, or of its scalar arm <T, 8, 1>
#define LSS_CE_LAUNCH(KERNEL, T, vec, nc, nb, s, ...)                                                                \
    do {                                                                                                             \
        const dim3 g_((unsigned)(nb)), b_(kBlock);                                                                   \
        if (!(vec)) hipLaunchKernelGGL((KERNEL<T, kCeMaxC, 1>), g_, b_, 0, s, __VA_ARGS__);                          \
        else switch (nc) {                                                                                           \
            case 2: hipLaunchKernelGGL((KERNEL<T, 2, 8>), g_, b_, 0, s, __VA_ARGS__); break;                         \
            case 3: hipLaunchKernelGGL((KERNEL<T, 3, 8>), g_, b_, 0, s, __VA_ARGS__); break;                         \
            case 4: hipLaunchKernelGGL((KERNEL<T, 4, 8>), g_, b_, 0, s, __VA_ARGS__); break;                         \
            case 5: hipLaunchKernelGGL((KERNEL<T, 5, 8>), g_, b_, 0, s, __VA_ARGS__); break;                         \
            case 6: hipLaunchKernelGGL((KERNEL<T, 6, 8>), g_, b_, 0, s, __VA_ARGS__); break;                         \
            case 7: hipLaunchKernelGGL((KERNEL<T, 7, 8>), g_, b_, 0, s, __VA_ARGS__); break;                         \
            default: hipLaunchKernelGGL((KERNEL<T, 8, 8>), g_, b_, 0, s, __VA_ARGS__); break;                        \
        }                                                                                                            \
    } while (0)

// What the three entries share: sizes in range (batch * C * plane elements addressable, a grid that fits), and the
// arm -- vector iff plane % 8 == 0, the logits-sized tensors 16-B and the byte maps 8-B aligned.
bool ce_sizes(int32_t batch, int64_t plane, int32_t C) {
    return batch > 0 && plane > 0 && C >= 2 && C <= kCeMaxC && plane <= LLONG_MAX / ((long long)batch * C) &&
           ((long long)batch * plane + kBlock - 1) / kBlock <= INT_MAX;
}
bool ce_vector(int64_t plane, const void* a16, const void* b16, const void* a8, const void* b8) {
    return plane % 8 == 0 && ((reinterpret_cast<uintptr_t>(a16) | reinterpret_cast<uintptr_t>(b16)) & 15) == 0 &&
           ((reinterpret_cast<uintptr_t>(a8) | reinterpret_cast<uintptr_t>(b8)) & 7) == 0;
}
long long ce_blocks(int32_t batch, int64_t plane, bool vec) {
    const long long units = (long long)batch * (vec ? plane / 8 : plane);
    return (units + kBlock - 1) / kBlock;
}

}  // namespace

extern "C" {

int64_t lss_softmax_ce_partials(int64_t n_cells) { return n_cells <= 0 ? 0 : 2 * ((n_cells + kBlock - 1) / kBlock); }

int lss_softmax_ce_arm(const void* x, int32_t dtype, const uint8_t* labels, const uint8_t* valid, int32_t batch,
                       int64_t plane, int32_t C, const void* grad) {
    const int esz = dtype == LSS_CONV_BF16 ? 2 : dtype == LSS_CONV_F32 ? 4 : 0;
    if (!x || !labels || !grad || !esz || !ce_sizes(batch, plane, C) ||
        ((reinterpret_cast<uintptr_t>(x) | reinterpret_cast<uintptr_t>(grad)) & (esz - 1)))
        return LSS_CONV_EINVAL;
    return ce_vector(plane, x, grad, labels, valid) ? LSS_CE_ARM_VECTOR : LSS_CE_ARM_SCALAR;
}

int lss_softmax_ce(const void* x, int32_t dtype, const uint8_t* labels, const uint8_t* valid, int32_t batch,
                   int64_t plane, int32_t C, const float* weight, float* partial, float* loss, float* scale, void* grad,
                   void* stream) {
    const int arm = lss_softmax_ce_arm(x, dtype, labels, valid, batch, plane, C, grad);
    if (arm < 0 || !weight || !partial || !loss || !scale ||
        ((reinterpret_cast<uintptr_t>(weight) | reinterpret_cast<uintptr_t>(partial) | reinterpret_cast<uintptr_t>(loss) |
          reinterpret_cast<uintptr_t>(scale)) & 3))
        return LSS_CONV_EINVAL;
    const bool vec = arm == LSS_CE_ARM_VECTOR;
    const long long nb = ce_blocks(batch, plane, vec);
    const float nf = (float)((long long)batch * plane);
    const uint8_t* mask = valid ? valid : labels;
    const int use_valid = valid != nullptr;
    hipStream_t s = (hipStream_t)stream;
    if (dtype == LSS_CONV_BF16)
        LSS_CE_LAUNCH(k_softmax_ce, bf16, vec, C, nb, s, (const bf16*)x, labels, mask, use_valid, (long long)batch,
                      (long long)plane, (int)C, weight, 1.0f / nf, partial, (bf16*)grad);
    else
        LSS_CE_LAUNCH(k_softmax_ce, float, vec, C, nb, s, (const float*)x, labels, mask, use_valid, (long long)batch,
                      (long long)plane, (int)C, weight, 1.0f / nf, partial, (float*)grad);
    hipLaunchKernelGGL(k_softmax_ce_total, dim3(1), dim3(kWave), 0, s, (const float*)partial, (int)nb, nf, loss, scale);
    return launch_status();
}

int lss_argmax_classes(const void* x, int32_t dtype, int32_t batch, int64_t plane, int32_t C, uint8_t* out,
                       void* stream) {
    const int esz = dtype == LSS_CONV_BF16 ? 2 : dtype == LSS_CONV_F32 ? 4 : 0;
    if (!x || !out || !esz || !ce_sizes(batch, plane, C) || (reinterpret_cast<uintptr_t>(x) & (esz - 1)))
        return LSS_CONV_EINVAL;
    const bool vec = ce_vector(plane, x, nullptr, out, nullptr);
    const long long nb = ce_blocks(batch, plane, vec);
    hipStream_t s = (hipStream_t)stream;
    if (dtype == LSS_CONV_BF16)
        LSS_CE_LAUNCH(k_argmax_classes, bf16, vec, C, nb, s, (const bf16*)x, (long long)batch, (long long)plane, (int)C,
                      out);
    else
        LSS_CE_LAUNCH(k_argmax_classes, float, vec, C, nb, s, (const float*)x, (long long)batch, (long long)plane,
                      (int)C, out);
    return launch_status();
}

int64_t lss_confusion_partial_bytes(int64_t n_cells, int32_t C) {
    return n_cells <= 0 || C < 2 || C > kCeMaxC
               ? 0
               : ((n_cells + kBlock - 1) / kBlock) * (int64_t)(2 * sizeof(double) + (size_t)C * C * sizeof(int));
}

int lss_confusion_accum(const void* x, int32_t dtype, const uint8_t* labels, const uint8_t* valid, int32_t batch,
                        int64_t plane, int32_t C, const int32_t* n_valid, const float* weight, double* totals,
                        void* partial, void* stream) {
    const int esz = dtype == LSS_CONV_BF16 ? 2 : dtype == LSS_CONV_F32 ? 4 : 0;
    if (!x || !labels || !weight || !totals || !partial || !esz || !ce_sizes(batch, plane, C) ||
        (reinterpret_cast<uintptr_t>(x) & (esz - 1)) ||
        ((reinterpret_cast<uintptr_t>(weight) | reinterpret_cast<uintptr_t>(n_valid)) & 3) ||
        ((reinterpret_cast<uintptr_t>(totals) | reinterpret_cast<uintptr_t>(partial)) & 7))
        return LSS_CONV_EINVAL;
    const bool vec = ce_vector(plane, x, nullptr, labels, valid);
    const long long nb = ce_blocks(batch, plane, vec);
    const uint8_t* mask = valid ? valid : labels;
    const int use_valid = valid != nullptr;
    double* pl = (double*)partial;
    double* pw = pl + nb;
    int* ph = (int*)(pw + nb);
    hipStream_t s = (hipStream_t)stream;
    if (dtype == LSS_CONV_BF16)
        LSS_CE_LAUNCH(k_confusion, bf16, vec, C, nb, s, (const bf16*)x, labels, mask, use_valid, (long long)batch,
                      (long long)plane, (int)C, (const int*)n_valid, weight, pl, pw, ph);
    else
        LSS_CE_LAUNCH(k_confusion, float, vec, C, nb, s, (const float*)x, labels, mask, use_valid, (long long)batch,
                      (long long)plane, (int)C, (const int*)n_valid, weight, pl, pw, ph);
    hipLaunchKernelGGL(k_confusion_fold, dim3(1), dim3(kBlock), 0, s, (const double*)pl, (const double*)pw,
                       (const int*)ph, (int)nb, (int)C, (int)batch, (const int*)n_valid, totals);
    return launch_status();
}

}  // extern "C"
