// lss_optim.hip -- gfx950 optimizer step of the training loop (train_simbev.py:245-248): gradient clipping
// (torch.nn.utils.clip_grad_norm_(params, max_norm)) fused with Adam (torch.optim.Adam, L2 weight decay,
// no amsgrad) over the flat fp32 master parameters, two launches for any number of parameter tensors:
//   1. sum of the squared gradients, one partial per block (fixed element ranges, fixed reduction order);
//      block 0 also advances every tensor's step counter (device-resident, as capturable Adam keeps it);
//   2. every block folds the partials in the same order (identical norm everywhere), clip factor
//      c = min(max_norm / (norm + 1e-6), 1), then for its elements: g = c grad + wd p,
//      m = b1 m + (1 - b1) g, v = b2 v + (1 - b2) g^2, p -= lr / (1 - b1^t) * m / (sqrt(v) / sqrt(1 - b2^t) + eps).
// torch's path runs a foreach norm, about eight scalar kernels, a foreach multiply of every gradient and the
// fused Adam kernel: the gradients are read three times and written once; here they are read twice.
// The clipped gradient itself is not written back (nothing reads it after the step).
// lss_clip_adam_guarded: the same update unless the norm is a NaN or an infinity; then pass 2 returns before
// writing anything and a third, one-block launch counts the skipped step instead of advancing the step counts
// (they cannot be advanced in pass 1, before the norm is known, nor in pass 2, whose blocks all read them).
// lss_clip_adam_sched: either form with the learning rate computed in pass 2 from each tensor's own step count
// (warm-up, then constant / linear / cosine decay: a captured update follows the schedule, a skipped step does
// not advance it) and, optionally, an exponential moving average of the updated parameters written in the same
// pass by the same thread (36 B per parameter instead of 28). A sibling kernel: the instantiations the two
// entries above launch are untouched.

#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "lss_convs.h"
#include "lss_device.h"

#pragma clang fp contract(fast)

namespace {

constexpr int kBlock = 256;
constexpr int kMaxBlocks = 1024;       // norm-pass blocks (partials)
constexpr int kMaxAdamBlocks = 16384;  // Adam-pass blocks
#ifndef LSS_ADAM_EMA_ELEMS
#define LSS_ADAM_EMA_ELEMS 4
#endif
constexpr int kEmaElems = LSS_ADAM_EMA_ELEMS;  // elements per thread of the Adam pass with the EMA (a multiple of 4)

struct Segs {
    float* p[LSS_ADAM_MAX_TENSORS];
    const float* g[LSS_ADAM_MAX_TENSORS];
    float* m[LSS_ADAM_MAX_TENSORS];
    float* v[LSS_ADAM_MAX_TENSORS];
    float* step[LSS_ADAM_MAX_TENSORS];
    long long start[LSS_ADAM_MAX_TENSORS + 1];  // prefix sums of the tensor sizes
    int count;
};

// the block's element range of the concatenated tensors, in multiples of 4 elements
__device__ __forceinline__ void block_range(long long total, long long& lo, long long& hi) {
    const long long per = ((total + gridDim.x - 1) / gridDim.x + 3) & ~3ll;
    lo = min((long long)blockIdx.x * per, total);
    hi = min(lo + per, total);
}

// f(segment, first, end) over the parts of [lo, hi) in each tensor
template <typename F>
__device__ __forceinline__ void for_segments(const Segs& s, long long lo, long long hi, F&& f) {
    for (int k = 0; k < s.count; ++k) {
        const long long a = max(lo, s.start[k]), b = min(hi, s.start[k + 1]);
        if (a < b) f(k, a - s.start[k], b - s.start[k]);
    }
}

__device__ __forceinline__ float block_sum(float x, float* s_w) {
#pragma unroll
    for (int o = kWave / 2; o > 0; o >>= 1) x += __shfl_xor(x, o, kWave);
    __syncthreads();
    if ((threadIdx.x & (kWave - 1)) == 0) s_w[threadIdx.x / kWave] = x;
    __syncthreads();
    float t = 0.f;
#pragma unroll
    for (int w = 0; w < kBlock / kWave; ++w) t += s_w[w];
    return t;  // every thread
}

// kGuard (lss_clip_adam_guarded): the step counts are not advanced here but by k_guard_commit, once the
// norm is known to be finite
template <bool kGuard>
__global__ __launch_bounds__(kBlock) void k_clip_sumsq(Segs s, float* __restrict__ partial) {
    __shared__ float s_w[kBlock / kWave];
    long long lo, hi;
    block_range(s.start[s.count], lo, hi);
    float acc = 0.f;
    for_segments(s, lo, hi, [&](int k, long long a, long long b) {
        const float* g = s.g[k];
        long long i = a + threadIdx.x * 4;
        // a segment's part starts on a 4-element boundary of the concatenation; its own alignment decides
        const bool vec = ((s.start[k] & 3) == 0) && ((reinterpret_cast<uintptr_t>(g) & 15) == 0);
        if (vec) {
            for (; i + 3 < b; i += kBlock * 4) {
                const float4 q = *reinterpret_cast<const float4*>(g + i);
                acc = fmaf(q.x, q.x, acc);
                acc = fmaf(q.y, q.y, acc);
                acc = fmaf(q.z, q.z, acc);
                acc = fmaf(q.w, q.w, acc);
            }
        }
        for (; i < b; i += kBlock * 4)
            for (long long j = i; j < min(i + 4, b); ++j) acc = fmaf(g[j], g[j], acc);
    });
    const float t = block_sum(acc, s_w);
    if (threadIdx.x == 0) partial[blockIdx.x] = t;
    if (!kGuard && blockIdx.x == 0 && (int)threadIdx.x < s.count) s.step[threadIdx.x][0] += 1.f;
}

// a NaN or an infinity (tested on the bits)
__device__ __forceinline__ bool non_finite(float x) { return (__float_as_uint(x) & 0x7f800000u) == 0x7f800000u; }

// the squared gradient norm from the partials; the same order in every block of every kernel that folds them
__device__ __forceinline__ float fold_partials(const float* __restrict__ partial, int npartial, float* s_w) {
    float acc = 0.f;
    for (int i = threadIdx.x; i < npartial; i += kBlock) acc += partial[i];
    return block_sum(acc, s_w);
}

__device__ __forceinline__ void adam_one(float& p, float g, float& m, float& v, float c, float wd, float b1, float b2,
                                         float step_size, float bc2_sqrt, float eps) {
    g = fmaf(wd, p, g * c);
    m = fmaf(b1, m, (1.f - b1) * g);
    v = fmaf(b2, v, (1.f - b2) * g * g);
    p -= step_size * m / (sqrtf(v) / bc2_sqrt + eps);
}

template <bool kGuard>
__global__ __launch_bounds__(kBlock) void k_clip_adam(Segs s, const float* __restrict__ partial, int npartial,
                                                      float max_norm, float lr, float b1, float b2, float eps,
                                                      float wd) {
    __shared__ float s_w[kBlock / kWave];
    const float norm = sqrtf(fold_partials(partial, npartial, s_w));
    if (kGuard && non_finite(norm)) return;  // uniform over the grid: no block writes anything
    // clip_coef.clamp(max=1) as torch computes it: a NaN / inf norm passes through (fminf would return
    // 1 for a NaN and leave the step unclipped), so every parameter goes non-finite as with torch
    const float q = max_norm / (norm + 1e-6f);
    const float c = q != q ? q : fminf(q, 1.f);
    long long lo, hi;
    block_range(s.start[s.count], lo, hi);
    for_segments(s, lo, hi, [&](int k, long long a, long long b) {
        const float t = kGuard ? s.step[k][0] + 1.f : s.step[k][0];  // (guarded: advanced after this kernel)
        const float step_size = lr / (1.f - powf(b1, t));
        const float bc2_sqrt = sqrtf(1.f - powf(b2, t));
        float* p = s.p[k];
        const float* g = s.g[k];
        float* m = s.m[k];
        float* v = s.v[k];
        long long i = a + threadIdx.x * 4;
        const bool vec = ((s.start[k] & 3) == 0) &&
                         (((reinterpret_cast<uintptr_t>(p) | reinterpret_cast<uintptr_t>(g) |
                            reinterpret_cast<uintptr_t>(m) | reinterpret_cast<uintptr_t>(v)) & 15) == 0);
        if (vec) {
            for (; i + 3 < b; i += kBlock * 4) {
                float4 pp = *reinterpret_cast<float4*>(p + i), mm = *reinterpret_cast<float4*>(m + i),
                       vv = *reinterpret_cast<float4*>(v + i);
                const float4 gg = *reinterpret_cast<const float4*>(g + i);
                adam_one(pp.x, gg.x, mm.x, vv.x, c, wd, b1, b2, step_size, bc2_sqrt, eps);
                adam_one(pp.y, gg.y, mm.y, vv.y, c, wd, b1, b2, step_size, bc2_sqrt, eps);
                adam_one(pp.z, gg.z, mm.z, vv.z, c, wd, b1, b2, step_size, bc2_sqrt, eps);
                adam_one(pp.w, gg.w, mm.w, vv.w, c, wd, b1, b2, step_size, bc2_sqrt, eps);
                *reinterpret_cast<float4*>(p + i) = pp;
                *reinterpret_cast<float4*>(m + i) = mm;
                *reinterpret_cast<float4*>(v + i) = vv;
            }
        }
        for (; i < b; i += kBlock * 4)
            for (long long j = i; j < min(i + 4, b); ++j)
                adam_one(p[j], g[j], m[j], v[j], c, wd, b1, b2, step_size, bc2_sqrt, eps);
    });
}

// ---- lss_clip_adam_sched: the learning-rate schedule and the EMA of the weights, inside pass 2
struct Sched {
    int kind;      // 0 constant, 1 linear, 2 cosine
    float W, wf;   // warm-up steps, the factor at s = 0
    float T, m;    // the decay ends at step T, at the factor m
    float ema_decay;
    int ema_warmup;
};

struct EmaSegs {
    float* e[LSS_ADAM_MAX_TENSORS];
};

// lr * warm(s) * decay(s), s = t - 1 (fp32). With y = 1 - x = clamp((T - s) / (T - W), 0, 1), one rounding of
// two exact integers: linear m + (1 - m) y; cosine 0.5 (1 + cos(pi x)) = sin^2(pi y / 2), which keeps its
// relative accuracy where 1 + cos(pi x) cancels (x -> 1). No warm-up: warm = 1 exactly; constant: decay = 1
// exactly, so a constant schedule without warm-up gives lr bit for bit.
__device__ __forceinline__ float sched_lr(const Sched& sc, float lr, float t) {
    const float s = t - 1.f;
    const float warm = sc.W > 0.f ? fmaf(1.f - sc.wf, fminf(s, sc.W) / sc.W, sc.wf) : 1.f;
    float decay = 1.f;
    if (sc.kind != 0) {
        const float y = fminf(fmaxf((sc.T - s) / (sc.T - sc.W), 0.f), 1.f);
        float shape = y;
        if (sc.kind == 2) {
            const float sn = sinpif(0.5f * y);
            shape = sn * sn;
        }
        decay = fmaf(1.f - sc.m, shape, sc.m);
    }
    return lr * warm * decay;
}

__device__ __forceinline__ void ema_one(float& e, float p, float omd) { e = fmaf(omd, p - e, e); }

template <bool kGuard, bool kEma>
__global__ __launch_bounds__(kBlock) void k_clip_adam_sched(Segs s, EmaSegs es, Sched sc,
                                                            const float* __restrict__ partial, int npartial,
                                                            float max_norm, float lr, float b1, float b2, float eps,
                                                            float wd, float* __restrict__ lr_out) {
    __shared__ float s_w[kBlock / kWave];
    const float norm = sqrtf(fold_partials(partial, npartial, s_w));
    if (kGuard && non_finite(norm)) return;  // uniform over the grid: no block writes anything, lr_out included
    const float q = max_norm / (norm + 1e-6f);
    const float c = q != q ? q : fminf(q, 1.f);  // (as k_clip_adam)
    if (lr_out && blockIdx.x == 0 && threadIdx.x == 0)
        lr_out[0] = sched_lr(sc, lr, kGuard ? s.step[0][0] + 1.f : s.step[0][0]);
    long long lo, hi;
    block_range(s.start[s.count], lo, hi);
    for_segments(s, lo, hi, [&](int k, long long a, long long b) {
        const float t = kGuard ? s.step[k][0] + 1.f : s.step[k][0];  // (guarded: advanced after this kernel)
        const float step_size = sched_lr(sc, lr, t) / (1.f - powf(b1, t));
        const float bc2_sqrt = sqrtf(1.f - powf(b2, t));
        const float omd = 1.f - (sc.ema_warmup ? fminf(sc.ema_decay, (1.f + t) / (10.f + t)) : sc.ema_decay);
        float* p = s.p[k];
        const float* g = s.g[k];
        float* m = s.m[k];
        float* v = s.v[k];
        float* e = kEma ? es.e[k] : nullptr;
        long long i = a + threadIdx.x * 4;
        const bool vec = ((s.start[k] & 3) == 0) &&
                         (((reinterpret_cast<uintptr_t>(p) | reinterpret_cast<uintptr_t>(g) |
                            reinterpret_cast<uintptr_t>(m) | reinterpret_cast<uintptr_t>(v) |
                            reinterpret_cast<uintptr_t>(e)) & 15) == 0);
        if (vec) {
            for (; i + 3 < b; i += kBlock * 4) {
                float4 pp = *reinterpret_cast<float4*>(p + i), mm = *reinterpret_cast<float4*>(m + i),
                       vv = *reinterpret_cast<float4*>(v + i);
                const float4 gg = *reinterpret_cast<const float4*>(g + i);
                float4 ee;
                if (kEma) ee = *reinterpret_cast<float4*>(e + i);
                adam_one(pp.x, gg.x, mm.x, vv.x, c, wd, b1, b2, step_size, bc2_sqrt, eps);
                adam_one(pp.y, gg.y, mm.y, vv.y, c, wd, b1, b2, step_size, bc2_sqrt, eps);
                adam_one(pp.z, gg.z, mm.z, vv.z, c, wd, b1, b2, step_size, bc2_sqrt, eps);
                adam_one(pp.w, gg.w, mm.w, vv.w, c, wd, b1, b2, step_size, bc2_sqrt, eps);
                *reinterpret_cast<float4*>(p + i) = pp;
                *reinterpret_cast<float4*>(m + i) = mm;
                *reinterpret_cast<float4*>(v + i) = vv;
                if (kEma) {
                    ema_one(ee.x, pp.x, omd);
                    ema_one(ee.y, pp.y, omd);
                    ema_one(ee.z, pp.z, omd);
                    ema_one(ee.w, pp.w, omd);
                    *reinterpret_cast<float4*>(e + i) = ee;
                }
            }
        }
        for (; i < b; i += kBlock * 4)
            for (long long j = i; j < min(i + 4, b); ++j) {
                adam_one(p[j], g[j], m[j], v[j], c, wd, b1, b2, step_size, bc2_sqrt, eps);
                if (kEma) ema_one(e[j], p[j], omd);
            }
    });
}

// After a guarded update (one block): advance every step count, or count the skipped step.
__global__ __launch_bounds__(kBlock) void k_guard_commit(Segs s, const float* __restrict__ partial, int npartial,
                                                         int* __restrict__ skipped) {
    __shared__ float s_w[kBlock / kWave];
    const float norm = sqrtf(fold_partials(partial, npartial, s_w));
    if (non_finite(norm)) {
        if (threadIdx.x == 0) skipped[0] += 1;
    } else if ((int)threadIdx.x < s.count) {
        s.step[threadIdx.x][0] += 1.f;
    }
}

int clip_adam(int32_t count, float* const* params, const float* const* grads, float* const* exp_avg,
              float* const* exp_avg_sq, float* const* step, const int64_t* numel, float max_norm, float lr,
              float beta1, float beta2, float eps, float weight_decay, float* partial, int32_t* skipped,
              void* stream, const Sched* sched = nullptr, float* lr_out = nullptr, float* const* ema = nullptr);

}  // namespace

extern "C" {

int lss_clip_adam_partials(void) { return kMaxBlocks; }

int lss_clip_adam(int32_t count, float* const* params, const float* const* grads, float* const* exp_avg,
                  float* const* exp_avg_sq, float* const* step, const int64_t* numel, float max_norm, float lr,
                  float beta1, float beta2, float eps, float weight_decay, float* partial, void* stream) {
    return clip_adam(count, params, grads, exp_avg, exp_avg_sq, step, numel, max_norm, lr, beta1, beta2, eps,
                     weight_decay, partial, nullptr, stream);
}

int lss_clip_adam_guarded(int32_t count, float* const* params, const float* const* grads, float* const* exp_avg,
                          float* const* exp_avg_sq, float* const* step, const int64_t* numel, float max_norm,
                          float lr, float beta1, float beta2, float eps, float weight_decay, float* partial,
                          int32_t* skipped, void* stream) {
    if (!skipped) return LSS_CONV_EINVAL;
    return clip_adam(count, params, grads, exp_avg, exp_avg_sq, step, numel, max_norm, lr, beta1, beta2, eps,
                     weight_decay, partial, skipped, stream);
}

int lss_clip_adam_sched(int32_t count, float* const* params, const float* const* grads, float* const* exp_avg,
                        float* const* exp_avg_sq, float* const* step, const int64_t* numel, float max_norm,
                        float lr, float beta1, float beta2, float eps, float weight_decay, float* partial,
                        int32_t* skipped, int32_t kind, int32_t warmup_steps, float warmup_factor,
                        int32_t total_steps, float min_factor, float* lr_out, float* const* ema, float ema_decay,
                        int32_t ema_warmup, void* stream) {
    if (kind < 0 || kind > 2 || warmup_steps < 0 || !(warmup_factor >= 0.f && warmup_factor <= 1.f) ||
        !(min_factor >= 0.f && min_factor <= 1.f) || (kind != 0 && total_steps <= warmup_steps) ||
        !(ema_decay >= 0.f && ema_decay < 1.f))
        return LSS_CONV_EINVAL;
    Sched sc{};
    sc.kind = kind;
    sc.W = (float)warmup_steps;
    sc.wf = warmup_factor;
    sc.T = (float)total_steps;
    sc.m = min_factor;
    sc.ema_decay = ema_decay;
    sc.ema_warmup = ema_warmup != 0;
    return clip_adam(count, params, grads, exp_avg, exp_avg_sq, step, numel, max_norm, lr, beta1, beta2, eps,
                     weight_decay, partial, skipped, stream, &sc, lr_out, ema);
}

}  // extern "C"

namespace {

// skipped: NULL = lss_clip_adam, else the guarded update; sched: NULL = those two entries' kernels, else
// lss_clip_adam_sched's (lr_out, ema: nullable)
int clip_adam(int32_t count, float* const* params, const float* const* grads, float* const* exp_avg,
              float* const* exp_avg_sq, float* const* step, const int64_t* numel, float max_norm, float lr,
              float beta1, float beta2, float eps, float weight_decay, float* partial, int32_t* skipped,
              void* stream, const Sched* sched, float* lr_out, float* const* ema) {
    if (count <= 0 || count > LSS_ADAM_MAX_TENSORS || !params || !grads || !exp_avg || !exp_avg_sq || !step ||
        !numel || !partial || !(max_norm > 0.f))
        return LSS_CONV_EINVAL;
    Segs s{};
    s.count = count;
    s.start[0] = 0;
    for (int k = 0; k < count; ++k) {
        if (!params[k] || !grads[k] || !exp_avg[k] || !exp_avg_sq[k] || !step[k] || numel[k] <= 0)
            return LSS_CONV_EINVAL;
        s.p[k] = params[k];
        s.g[k] = grads[k];
        s.m[k] = exp_avg[k];
        s.v[k] = exp_avg_sq[k];
        s.step[k] = step[k];
        for (int j = 0; j < k; ++j)  // each step counter is advanced once per call
            if (step[j] == step[k] || params[j] == params[k]) return LSS_CONV_EINVAL;
        s.start[k + 1] = s.start[k] + numel[k];
    }
    EmaSegs es{};
    if (ema) {
        for (int k = 0; k < count; ++k) {
            if (!ema[k]) return LSS_CONV_EINVAL;
            for (int j = 0; j < count; ++j)
                if (ema[k] == params[j] || ema[k] == exp_avg[j] || ema[k] == exp_avg_sq[j] || (j < k && ema[j] == ema[k]))
                    return LSS_CONV_EINVAL;
            es.e[k] = ema[k];
        }
    }
    const long long total = s.start[count];
    // the norm pass: at most kMaxBlocks partials (each Adam block folds them all); the Adam pass: ~8 elements
    // per thread, so the stream of 28 B per parameter has many blocks' loads in flight
    long long nb = (total + kBlock * 16 - 1) / (kBlock * 16);
    nb = nb < 1 ? 1 : (nb > kMaxBlocks ? kMaxBlocks : nb);
    long long nb2 = (total + kBlock * 8 - 1) / (kBlock * 8);
    nb2 = nb2 < 1 ? 1 : (nb2 > kMaxAdamBlocks ? kMaxAdamBlocks : nb2);
    hipStream_t st = (hipStream_t)stream;
    if (sched) {
        // the same three (two) launches with the sibling pass 2. The EMA arm streams 36 B per parameter; its
        // elements per thread are a tuning knob of their own (4 / 8 / 16 measured)
        if (ema) {
            nb2 = (total + kBlock * kEmaElems - 1) / (kBlock * kEmaElems);
            nb2 = nb2 < 1 ? 1 : (nb2 > kMaxAdamBlocks ? kMaxAdamBlocks : nb2);
        }
        const dim3 g2((unsigned)nb2), blk(kBlock);
        if (skipped) {
            hipLaunchKernelGGL(k_clip_sumsq<true>, dim3((unsigned)nb), blk, 0, st, s, partial);
            if (ema)
                hipLaunchKernelGGL((k_clip_adam_sched<true, true>), g2, blk, 0, st, s, es, *sched, (const float*)partial,
                                   (int)nb, max_norm, lr, beta1, beta2, eps, weight_decay, lr_out);
            else
                hipLaunchKernelGGL((k_clip_adam_sched<true, false>), g2, blk, 0, st, s, es, *sched, (const float*)partial,
                                   (int)nb, max_norm, lr, beta1, beta2, eps, weight_decay, lr_out);
            hipLaunchKernelGGL(k_guard_commit, dim3(1), blk, 0, st, s, (const float*)partial, (int)nb, (int*)skipped);
        } else {
            hipLaunchKernelGGL(k_clip_sumsq<false>, dim3((unsigned)nb), blk, 0, st, s, partial);
            if (ema)
                hipLaunchKernelGGL((k_clip_adam_sched<false, true>), g2, blk, 0, st, s, es, *sched, (const float*)partial,
                                   (int)nb, max_norm, lr, beta1, beta2, eps, weight_decay, lr_out);
            else
                hipLaunchKernelGGL((k_clip_adam_sched<false, false>), g2, blk, 0, st, s, es, *sched, (const float*)partial,
                                   (int)nb, max_norm, lr, beta1, beta2, eps, weight_decay, lr_out);
        }
        return launch_status();
    }
    if (skipped) {
        hipLaunchKernelGGL(k_clip_sumsq<true>, dim3((unsigned)nb), dim3(kBlock), 0, st, s, partial);
        hipLaunchKernelGGL(k_clip_adam<true>, dim3((unsigned)nb2), dim3(kBlock), 0, st, s, (const float*)partial,
                           (int)nb, max_norm, lr, beta1, beta2, eps, weight_decay);
        hipLaunchKernelGGL(k_guard_commit, dim3(1), dim3(kBlock), 0, st, s, (const float*)partial, (int)nb,
                           (int*)skipped);
    } else {
        hipLaunchKernelGGL(k_clip_sumsq<false>, dim3((unsigned)nb), dim3(kBlock), 0, st, s, partial);
        hipLaunchKernelGGL(k_clip_adam<false>, dim3((unsigned)nb2), dim3(kBlock), 0, st, s, (const float*)partial,
                           (int)nb, max_norm, lr, beta1, beta2, eps, weight_decay);
    }
    return launch_status();
}

}  // namespace
