// lss_device.h -- the device and host helpers the .hip files of this directory share: one definition of
// each. Internal: included by the .hip files only, not part of the C ABI (include/), and everything here
// is in an anonymous namespace, so the library's exported symbols do not depend on it.
//
// lss_hip.hip is compiled with FMA contraction off (the geometry's bit-exact op order) and the conv-stack
// files switch it on after their includes, so nothing here may round differently under either setting:
// no expression of the form a * b + c, and no fp contract pragma.
#pragma once

#include <hip/hip_runtime.h>
#include <hip/hip_bf16.h>
#include <stdint.h>

namespace {

using bf16 = __hip_bfloat16;
constexpr int kWave = 64;  // lanes per wave (gfx9)

// ---- one element <-> fp32 (bf16 -> fp32 is exact; fp32 -> bf16 rounds to nearest even)
__device__ __forceinline__ float ld(const float* p) { return *p; }
__device__ __forceinline__ float ld(const bf16* p) { return __bfloat162float(*p); }
__device__ __forceinline__ void st(float* p, float v) { *p = v; }
__device__ __forceinline__ void st(bf16* p, float v) { *p = __float2bfloat16(v); }
// The conversion of st as a value, for the stores lss_hip.hip writes as assignments (x = from_f32<T>(v)):
// st(&x, v) orders the address and the value the other way round, and k_splat_fwd_nhwc and k_splat_bwd_reg
// come out scheduled differently with it. Every other file stores through st.
template <typename T> __device__ __forceinline__ T from_f32(float v);
template <> __device__ __forceinline__ float from_f32<float>(float v) { return v; }
template <> __device__ __forceinline__ bf16 from_f32<bf16>(float v) { return __float2bfloat16(v); }

// ---- fp32 -> bf16, three forms that do not compile alike, so each kernel keeps the one it was built on:
//   __float2bfloat16 (st, stv, pack2 here): the compiler's conversion; every kernel but the two below.
//   bf16_bits_select: the squeeze-excite kernels (lss_se.hip). A select, not a branch: a branch per
//     element would put every load of an unrolled loop in a block of its own, each waited for before
//     the next is issued.
//   bf16_bits_branch: the upsample kernels (lss_resample.hip), c10::BFloat16's rounding as written there;
//     the select form schedules those kernels differently.
// All three round to nearest even and keep a NaN quiet.
__device__ __forceinline__ unsigned short bf16_bits_select(float x) {
    const unsigned u = __float_as_uint(x);
    const unsigned nan = (u >> 16) | 0x40u, rne = (u + 0x7fffu + ((u >> 16) & 1u)) >> 16;
    return (unsigned short)((u & 0x7fffffffu) > 0x7f800000u ? nan : rne);
}
__device__ __forceinline__ unsigned bf16_bits_branch(float x) {
    unsigned u = __float_as_uint(x);
    if ((u & 0x7fffffffu) > 0x7f800000u) return (u >> 16) | 0x40u;
    u += 0x7fffu + ((u >> 16) & 1u);
    return u >> 16;
}
__device__ __forceinline__ unsigned pack2(float a, float b) {
    const bf16 x = __float2bfloat16(a), y = __float2bfloat16(b);
    return (unsigned)*reinterpret_cast<const unsigned short*>(&x) |
           ((unsigned)*reinterpret_cast<const unsigned short*>(&y) << 16);
}

// ---- packed bf16 in registers -> fp32: 8 from a 16-B vector (uint4 or an ext_vector of 4 unsigned), 4 from a uint2
template <typename V4> __device__ __forceinline__ void unpack8(const V4& u, float* o) {
    const unsigned w[4] = {u.x, u.y, u.z, u.w};
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        o[2 * i] = __uint_as_float(w[i] << 16);
        o[2 * i + 1] = __uint_as_float(w[i] & 0xFFFF0000u);
    }
}
__device__ __forceinline__ void unpack4(uint2 u, float* o) {
    o[0] = __uint_as_float(u.x << 16); o[1] = __uint_as_float(u.x & 0xffff0000u);
    o[2] = __uint_as_float(u.y << 16); o[3] = __uint_as_float(u.y & 0xffff0000u);
}

// ---- V consecutive elements <-> fp32 (V in {1, 4, 8}), one 16-B access per 4 floats / 8 bf16; the caller
// guarantees the alignment
template <int V> __device__ __forceinline__ void ldv(const float* p, float* o) {
    if constexpr (V == 1) {
        o[0] = *p;
    } else {
#pragma unroll
        for (int i = 0; i < V; i += 4) {
            const float4 a = *reinterpret_cast<const float4*>(p + i);
            o[i] = a.x; o[i + 1] = a.y; o[i + 2] = a.z; o[i + 3] = a.w;
        }
    }
}
template <int V> __device__ __forceinline__ void ldv(const bf16* p, float* o) {
    if constexpr (V == 1) o[0] = __bfloat162float(*p);
    else if constexpr (V == 8) unpack8(*reinterpret_cast<const uint4*>(p), o);
    else unpack4(*reinterpret_cast<const uint2*>(p), o);
}
template <int V> __device__ __forceinline__ void stv(float* p, const float* v) {
    if constexpr (V == 1) {
        *p = v[0];
    } else {
#pragma unroll
        for (int i = 0; i < V; i += 4) *reinterpret_cast<float4*>(p + i) = make_float4(v[i], v[i + 1], v[i + 2], v[i + 3]);
    }
}
template <int V> __device__ __forceinline__ void stv(bf16* p, const float* v) {
    if constexpr (V == 1) {
        *p = __float2bfloat16(v[0]);
    } else {
        bf16 b[V];
#pragma unroll
        for (int i = 0; i < V; ++i) b[i] = __float2bfloat16(v[i]);
        if constexpr (V == 8) *reinterpret_cast<uint4*>(p) = *reinterpret_cast<const uint4*>(b);
        else *reinterpret_cast<uint2*>(p) = *reinterpret_cast<const uint2*>(b);
    }
}

__device__ __forceinline__ float sigmoid(float z) { return 1.f / (1.f + __expf(-z)); }

__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
    for (int o = kWave / 2; o > 0; o >>= 1) v += __shfl_xor(v, o, kWave);
    return v;
}

// "v if c else 0" without a branch: the mask goes through an empty asm, so the compiler cannot turn
// the AND back into a select and then into a branch around the load that produced v (it sinks such
// loads into conditional blocks, and the blocks serialise loads that should all be in flight).
__device__ __forceinline__ unsigned keep_mask(bool c) {
    unsigned m = c ? 0xFFFFFFFFu : 0u;
    asm("" : "+v"(m));
    return m;
}
__device__ __forceinline__ uint4 keep_if(bool c, uint4 v) {
    const unsigned m = keep_mask(c);
    return make_uint4(v.x & m, v.y & m, v.z & m, v.w & m);
}
__device__ __forceinline__ float keep_if(bool c, float v) { return __uint_as_float(__float_as_uint(v) & keep_mask(c)); }

// ---- Philox4x32-10 (Salmon et al., SC'11): 10 rounds of the two multiplies and key bumps; a pure function of
// (key, counter). Integer only: the same words under either contraction setting. The dropout kernels
// (lss_elementwise.hip) and the image kernel's sensor noise (lss_simbev.hip) share it.
__device__ __forceinline__ uint4 philox4x32(uint2 key, uint4 c) {
#pragma unroll
    for (int r = 0; r < 10; ++r) {
        const unsigned lo0 = 0xD2511F53u * c.x, hi0 = __umulhi(0xD2511F53u, c.x);
        const unsigned lo1 = 0xCD9E8D57u * c.z, hi1 = __umulhi(0xCD9E8D57u, c.z);
        c = make_uint4(hi1 ^ c.y ^ key.x, lo1, hi0 ^ c.w ^ key.y, lo0);
        key.x += 0x9E3779B9u;
        key.y += 0xBB67AE85u;
    }
    return c;
}

// values handed from block to block inside a launch: write-through stores, L1-bypassing loads
__device__ __forceinline__ unsigned long long ld_agent(const unsigned long long* p) {
    return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
__device__ __forceinline__ void st_agent(unsigned long long* p, unsigned long long v) {
    __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
__device__ __forceinline__ float ld_agent(const float* p) {
    return __uint_as_float(
        __hip_atomic_load(reinterpret_cast<const unsigned*>(p), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT));
}
__device__ __forceinline__ void st_agent(float* p, float v) {
    __hip_atomic_store(reinterpret_cast<unsigned*>(p), __float_as_uint(v), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
// two adjacent floats (8-B aligned) as one 8-B access
__device__ __forceinline__ float2 ld_pair_agent(const float* p) {
    const unsigned long long v = ld_agent(reinterpret_cast<const unsigned long long*>(p));
    return make_float2(__uint_as_float((unsigned)v), __uint_as_float((unsigned)(v >> 32)));
}
__device__ __forceinline__ void st_pair_agent(float* p, float a, float b) {
    st_agent(reinterpret_cast<unsigned long long*>(p), ((unsigned long long)__float_as_uint(b) << 32) | __float_as_uint(a));
}

// ---- host side
inline int launch_status() {
    const hipError_t e = hipGetLastError();
    return e == hipSuccess ? 0 : (int)e;
}

// every pointer 16-B aligned (NULL passes): the vector accesses of the kernels behind an entry point
template <typename... P> inline bool aligned16(P... p) {
    return ((... | reinterpret_cast<uintptr_t>(p)) & 15) == 0;
}

inline int grid_blocks(long n, int per) { return (int)((n + per - 1) / per); }

}  // namespace
