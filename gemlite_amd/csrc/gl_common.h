// gl_common.h — shared device/host definitions for libgemlite_hip.so (gfx950 only).
//
// Data layout facts every kernel relies on (reference: gemlite/core.py:384-398,419-420,478-485;
// gemlite/bitpack.py:36-60):
//   W_q packed   : int32 [K/e, N], N-contiguous; word (j, n) holds k = j*e .. j*e+e-1 of column n,
//                  element i at bits [b*i, b*i+b)  (e = 32 / W_nbits)
//   scales/zeros : [K/group, N], N-contiguous (or [N] channel-wise, or a scalar zero)
//   x            : [M, K] row-major,  out : [M, N] row-major
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include "../../include/gemlite_hip.h"

namespace gl {

typedef _Float16 h2_t __attribute__((ext_vector_type(2)));
typedef __bf16 b2_t __attribute__((ext_vector_type(2)));
typedef _Float16 h8_t __attribute__((ext_vector_type(8)));
typedef __bf16 b8_t __attribute__((ext_vector_type(8)));
typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
typedef uint32_t u32x2 __attribute__((ext_vector_type(2)));
typedef int i32x16 __attribute__((ext_vector_type(16)));

struct half_tag {};
struct bf16_tag {};

// ---------------------------------------------------------------------------------------------
// 16-bit float traits: the "magic number" unpack (q | MAGIC is the float OFF + q), packed dot2
// ---------------------------------------------------------------------------------------------
template <typename Tag>
struct F16Traits;

template <>
struct F16Traits<half_tag> {
    static constexpr uint32_t MAGIC2 = 0x64006400u;  // two fp16 1024.0
    static constexpr float OFF = 1024.0f;             // exact for q < 1024
    static constexpr int MAX_QBITS = 8;
    static constexpr uint32_t ONES2 = 0x3C003C00u;  // (1.0h, 1.0h)
    static constexpr int DT = GEMLITE_DT_FP16;
    typedef h8_t frag8;
    static __device__ __forceinline__ float dot2(uint32_t a, uint32_t b, float c) {
        return __builtin_amdgcn_fdot2(__builtin_bit_cast(h2_t, a), __builtin_bit_cast(h2_t, b), c, false);
    }
    static __device__ __forceinline__ float to_float(uint16_t v) {
        return (float)__builtin_bit_cast(_Float16, v);
    }
    static __device__ __forceinline__ uint16_t from_float(float f) {
        return __builtin_bit_cast(uint16_t, (_Float16)f);
    }
};

template <>
struct F16Traits<bf16_tag> {
    static constexpr uint32_t MAGIC2 = 0x43004300u;  // two bf16 128.0
    static constexpr float OFF = 128.0f;              // exact for q < 128
    static constexpr int MAX_QBITS = 4;
    static constexpr uint32_t ONES2 = 0x3F803F80u;
    static constexpr int DT = GEMLITE_DT_BF16;
    typedef b8_t frag8;
    static __device__ __forceinline__ float dot2(uint32_t a, uint32_t b, float c) {
        return __builtin_amdgcn_fdot2_f32_bf16(__builtin_bit_cast(b2_t, a), __builtin_bit_cast(b2_t, b), c, false);
    }
    static __device__ __forceinline__ float to_float(uint16_t v) {
        return __builtin_bit_cast(float, (uint32_t)v << 16);
    }
    static __device__ __forceinline__ uint16_t from_float(float f) {
        return __builtin_bit_cast(uint16_t, (__bf16)f);
    }
};

// ---------------------------------------------------------------------------------------------
// generic scalar load / store by dtype code (metadata, epilogue). Uniform branches only.
// ---------------------------------------------------------------------------------------------
#define GL_HD __host__ __device__ __forceinline__

GL_HD float fp8e4m3_to_float(uint8_t v) {
    // OCP e4m3fn: bias 7, no inf, NaN = S.1111.111
    const uint32_t s = (uint32_t)(v & 0x80) << 24;
    const uint32_t em = v & 0x7F;
    if (em == 0x7F) return __builtin_bit_cast(float, s | 0x7FC00000u);
    const uint32_t e = em >> 3, m = em & 7;
    if (e == 0) {  // subnormal: m * 2^-9
        const float f = (float)m * 0.001953125f;
        return s ? -f : f;
    }
    return __builtin_bit_cast(float, s | ((e + 120u) << 23) | (m << 20));
}

GL_HD float fp8e5m2_to_float(uint8_t v) {
    // e5m2 is the top byte of an fp16
    const uint16_t h = (uint16_t)v << 8;
    return (float)__builtin_bit_cast(_Float16, h);
}

// round-to-nearest-even, saturating to +-448 like torch's .to(float8_e4m3fn) for finite inputs
GL_HD uint8_t float_to_fp8e4m3(float f) {
    uint32_t u = __builtin_bit_cast(uint32_t, f);
    const uint8_t s = (u >> 24) & 0x80;
    u &= 0x7FFFFFFFu;
    if (u > 0x7F800000u) return s | 0x7F;  // NaN
    const float a = __builtin_bit_cast(float, u);
    if (a > 464.0f) return s | 0x7F;  // torch: overflow -> NaN pattern (no inf in e4m3fn)
    if (a < 0.015625f) {               // below 2^-6: subnormal grid of 2^-9
        const float r = __builtin_rintf(a * 512.0f);
        return s | (uint8_t)r;          // r in 0..8 (8 == smallest normal 0x08)
    }
    // normal: keep 3 mantissa bits with RNE
    const uint32_t lsb = (u >> 20) & 1u;
    u += 0x7FFFFu + lsb;
    const uint32_t e = (u >> 23) - 120u, m = (u >> 20) & 7u;
    return s | (uint8_t)((e << 3) | m);
}

GL_HD uint8_t float_to_fp8e5m2(float f) {
    // direct fp32 -> e5m2 RNE (bias 15, 2 mantissa bits); overflow -> inf like torch
    uint32_t u = __builtin_bit_cast(uint32_t, f);
    const uint8_t s = (u >> 24) & 0x80;
    u &= 0x7FFFFFFFu;
    if (u > 0x7F800000u) return s | 0x7F;  // NaN
    const float a = __builtin_bit_cast(float, u);
    if (a >= 61440.0f) return s | 0x7C;    // >= midpoint(57344, 65536) -> inf
    if (a < 6.103515625e-05f) {            // below 2^-14: subnormal grid of 2^-16
        const float r = __builtin_rintf(a * 65536.0f);
        return s | (uint8_t)r;
    }
    const uint32_t lsb = (u >> 21) & 1u;
    u += 0xFFFFFu + lsb;
    const uint32_t e = (u >> 23) - 112u, m = (u >> 21) & 3u;
    return s | (uint8_t)((e << 2) | m);
}

__device__ __forceinline__ float load_as_float(const void* p, int64_t i, int dt) {
    switch (dt) {
        case GEMLITE_DT_FP32: return ((const float*)p)[i];
        case GEMLITE_DT_FP16: return (float)((const _Float16*)p)[i];
        case GEMLITE_DT_BF16: return __builtin_bit_cast(float, (uint32_t)((const uint16_t*)p)[i] << 16);
        case GEMLITE_DT_INT8: return (float)((const int8_t*)p)[i];
        case GEMLITE_DT_UINT8: return (float)((const uint8_t*)p)[i];
        case GEMLITE_DT_INT32: return (float)((const int32_t*)p)[i];
        case GEMLITE_DT_FP8E4: return fp8e4m3_to_float(((const uint8_t*)p)[i]);
        case GEMLITE_DT_FP8E5: return fp8e5m2_to_float(((const uint8_t*)p)[i]);
        default: return 0.0f;
    }
}

__device__ __forceinline__ void store_from_float(void* p, int64_t i, int dt, float v) {
    switch (dt) {
        case GEMLITE_DT_FP32: ((float*)p)[i] = v; break;
        case GEMLITE_DT_FP16: ((_Float16*)p)[i] = (_Float16)v; break;
        case GEMLITE_DT_BF16: ((__bf16*)p)[i] = (__bf16)v; break;
        case GEMLITE_DT_INT32: ((int32_t*)p)[i] = (int32_t)__builtin_rintf(v); break;
        default: break;
    }
}

// 4 consecutive metadata values (one per owned column) as floats
__device__ __forceinline__ f32x4 load_meta4(const void* p, int64_t i, int dt) {
    f32x4 r;
    if (dt == GEMLITE_DT_FP16) {
        for (int j = 0; j < 4; ++j) r[j] = (float)((const _Float16*)p)[i + j];
    } else if (dt == GEMLITE_DT_BF16) {
        const u32x2 v = *(const u32x2*)((const uint16_t*)p + i);
        r[0] = __builtin_bit_cast(float, v[0] << 16); r[1] = __builtin_bit_cast(float, v[0] & 0xFFFF0000u);
        r[2] = __builtin_bit_cast(float, v[1] << 16); r[3] = __builtin_bit_cast(float, v[1] & 0xFFFF0000u);
    } else if (dt == GEMLITE_DT_FP32) {
        r = *(const f32x4*)((const float*)p + i);
    } else {
        for (int j = 0; j < 4; ++j) r[j] = load_as_float(p, i + j, dt);
    }
    return r;
}

// ---------------------------------------------------------------------------------------------
// activation quantisers: |x| max and scale that KEEP a NaN (every quantiser of the library goes through these).
// fmaxf / fminf return the operand that is not NaN, so max(amax, |v|) and max(amax / qmax, 1e-6) turn a NaN activation into an
// ordinary scale: a finite, wrong row.  The bits of a non-negative float order like unsigned integers — finite < Inf < NaN — in
// fp16 and bf16 as in fp32, so the first pass runs on the packed 16-bit words as they were loaded: `d & 0x7fff7fff`, one
// v_pk_max_u16 per two elements, no conversion; the running maximum stays a pair of 16-bit lanes through the shuffles and the LDS
// merge and becomes a float once per row (or block).  For finite rows that float is the number the fmaxf chain over the converted
// values gave, bit for bit (the conversions are exact and monotonic).
// ---------------------------------------------------------------------------------------------
typedef unsigned short u16x2_t __attribute__((ext_vector_type(2)));
__device__ __forceinline__ uint32_t pk_umax16(uint32_t a, uint32_t b) {
    return __builtin_bit_cast(uint32_t, __builtin_elementwise_max(__builtin_bit_cast(u16x2_t, a), __builtin_bit_cast(u16x2_t, b)));
}
// eight packed 16-bit floats into the running pair of lanes (a tree: one dependent step per 16 bytes)
__device__ __forceinline__ uint32_t absmax16_acc(uint32_t m, const u32x4& d) {
    constexpr uint32_t ABS = 0x7FFF7FFFu;
    return pk_umax16(m, pk_umax16(pk_umax16(d[0] & ABS, d[1] & ABS), pk_umax16(d[2] & ABS, d[3] & ABS)));
}
__device__ __forceinline__ uint32_t absmax16_shfl(uint32_t m, int off) { return pk_umax16(m, (uint32_t)__shfl_xor((int)m, off)); }
template <int N>
__device__ __forceinline__ uint32_t absmax16_merge(const uint32_t* w) {  // N partial maxima (LDS), as a tree
    if constexpr (N == 1) return w[0];
    else return pk_umax16(absmax16_merge<N / 2>(w), absmax16_merge<N - N / 2>(w + N / 2));
}
// the pair of lanes as the float |x| max: NaN if the row held one, else Inf if it held one
__device__ __forceinline__ float absmax16_value(uint32_t m, bool f16) {
    const uint32_t lo = m & 0xFFFFu, hi = m >> 16;
    const uint16_t h = (uint16_t)(lo > hi ? lo : hi);
    return f16 ? F16Traits<half_tag>::to_float(h) : F16Traits<bf16_tag>::to_float(h);
}
// the same on floats, for the paths that have no packed words (any input type, unaligned rows): max(a, |v|) for a >= 0
__device__ __forceinline__ float absmax_keep_nan(float a, float v) {
    const uint32_t x = __builtin_bit_cast(uint32_t, a), y = __builtin_bit_cast(uint32_t, v) & 0x7FFFFFFFu;
    return __builtin_bit_cast(float, x > y ? x : y);
}
// the per-token scale max(amax / qmax, 1e-6); NaN for a NaN amax, Inf for an Inf one (fmaxf would answer 1e-6 for NaN)
__device__ __forceinline__ float token_scale_keep_nan(float amax, float qmax) {
    const float s = __fdiv_rn(amax, qmax);
    return s < 1e-6f ? 1e-6f : s;
}
// a block whose |x| max is Inf or NaN: its scale byte becomes the format's NaN code (e8m0 0xFF, e4m3 0x7F)
__device__ __forceinline__ bool amax_not_finite(float amax) { return (__builtin_bit_cast(uint32_t, amax) & 0x7FFFFFFFu) >= 0x7F800000u; }

// ---------------------------------------------------------------------------------------------
// epilogue: channel scaling (gemm_kernels.py:392-404), cast, store
// ---------------------------------------------------------------------------------------------
struct Epilogue {
    void* out;
    const void* scales_w;   // [N] channel scales (channel_scale_mode 1/3)
    const float* scales_x;  // [M] per-token scales (channel_scale_mode 2/3)
    int64_t stride_om, stride_on, stride_sx_m;
    int out_dt, meta_dt, c_mode;
};

__device__ __forceinline__ float epilogue_scale(const Epilogue& e, float v, int64_t m, int64_t n) {
    if (e.c_mode == 1) {
        v *= load_as_float(e.scales_w, n, e.meta_dt);
    } else if (e.c_mode == 2) {
        v *= e.scales_x[m * e.stride_sx_m];
    } else if (e.c_mode == 3) {
        v *= e.scales_x[m * e.stride_sx_m] * load_as_float(e.scales_w, n, e.meta_dt);
    }
    return v;
}

__device__ __forceinline__ void epilogue_store(const Epilogue& e, float v, int64_t m, int64_t n) {
    store_from_float(e.out, m * e.stride_om + n * e.stride_on, e.out_dt, epilogue_scale(e, v, m, n));
}

// typed (compile-time dtype) variants used by the specialised kernels: no runtime dtype switches in hot loops
template <typename Tag>
__device__ __forceinline__ f32x4 load4_t(const void* p, int64_t i) {  // 4 consecutive 16-bit floats -> fp32
    const u32x2 v = *(const u32x2*)((const uint16_t*)p + i);
    f32x4 r;
    const uint32_t v0 = v[0], v1 = v[1];
    if constexpr (F16Traits<Tag>::DT == GEMLITE_DT_FP16) {
        // NOTE: going through bit_cast<h2_t>(v[1]) here was miscompiled by hipcc 7.2 (second dword dropped,
        // r[2], r[3] left undefined); extract the halves as integers instead.
        r[0] = (float)__builtin_bit_cast(_Float16, (uint16_t)(v0 & 0xFFFFu));
        r[1] = (float)__builtin_bit_cast(_Float16, (uint16_t)(v0 >> 16));
        r[2] = (float)__builtin_bit_cast(_Float16, (uint16_t)(v1 & 0xFFFFu));
        r[3] = (float)__builtin_bit_cast(_Float16, (uint16_t)(v1 >> 16));
    } else {
        r[0] = __builtin_bit_cast(float, v0 << 16); r[1] = __builtin_bit_cast(float, v0 & 0xFFFF0000u);
        r[2] = __builtin_bit_cast(float, v1 << 16); r[3] = __builtin_bit_cast(float, v1 & 0xFFFF0000u);
    }
    return r;
}

template <typename Tag>
__device__ __forceinline__ void store_out_t(const Epilogue& e, float v, int64_t m, int64_t n) {
    using TR = F16Traits<Tag>;
    // channel scales of the kernel's own 16-bit type, or (round 4: BitNet's fp32 scale, helper.py:173-208) any float type
    auto sw = [&]() -> float { return e.meta_dt == TR::DT ? TR::to_float(((const uint16_t*)e.scales_w)[n]) : load_as_float(e.scales_w, n, e.meta_dt); };
    if (e.c_mode == 1) {
        v *= sw();
    } else if (e.c_mode == 2) {
        v *= e.scales_x[m * e.stride_sx_m];
    } else if (e.c_mode == 3) {
        v *= e.scales_x[m * e.stride_sx_m] * sw();
    }
    ((uint16_t*)e.out)[m * e.stride_om + n] = TR::from_float(v);
}

// 4 consecutive outputs of one row: channel scaling, cast, one 8-byte store (n0 multiple of 4)
template <typename Tag>
__device__ __forceinline__ void store_out4_t(const Epilogue& e, f32x4 v, int64_t m, int64_t n0) {
    using TR = F16Traits<Tag>;
    if (e.c_mode == 1 || e.c_mode == 3) {
        const f32x4 sw = load4_t<Tag>(e.scales_w, n0);
        v *= sw;
    }
    if (e.c_mode == 2 || e.c_mode == 3) {
        const float sx = e.scales_x[m * e.stride_sx_m];
        v *= (f32x4){sx, sx, sx, sx};
    }
    u32x2 o;
    o[0] = (uint32_t)TR::from_float(v[0]) | ((uint32_t)TR::from_float(v[1]) << 16);
    o[1] = (uint32_t)TR::from_float(v[2]) | ((uint32_t)TR::from_float(v[3]) << 16);
    *(u32x2*)((uint16_t*)e.out + m * e.stride_om + n0) = o;
}

// 4 consecutive outputs of one row from fp32 values: channel scaling (scales of fp32 / fp16 / bf16: one uniform
// three-way branch, vector loads), cast, one vector store
__device__ __forceinline__ void store_out4_any(const Epilogue& e, f32x4 v, int64_t m, int64_t n0) {
    // same operation order as epilogue_scale(): mode 3 multiplies by the PRODUCT s_x[m] * s_w[n] (bit-identical outputs)
    f32x4 sw = {1.f, 1.f, 1.f, 1.f};
    if (e.c_mode == 1 || e.c_mode == 3) {
        if (e.meta_dt == GEMLITE_DT_FP32) sw = *(const f32x4*)((const float*)e.scales_w + n0);
        else if (e.meta_dt == GEMLITE_DT_FP16) sw = load4_t<half_tag>(e.scales_w, n0);
        else sw = load4_t<bf16_tag>(e.scales_w, n0);
    }
    if (e.c_mode == 2 || e.c_mode == 3) {
        const float sx = e.scales_x[m * e.stride_sx_m];
        sw = e.c_mode == 3 ? (f32x4){sx * sw[0], sx * sw[1], sx * sw[2], sx * sw[3]} : (f32x4){sx, sx, sx, sx};
    }
    if (e.c_mode != 0) v *= sw;
    if (e.out_dt == GEMLITE_DT_FP32) {
        *(f32x4*)((float*)e.out + m * e.stride_om + n0) = v;
        return;
    }
    u32x2 o;
    if (e.out_dt == GEMLITE_DT_FP16) {
        o[0] = (uint32_t)F16Traits<half_tag>::from_float(v[0]) | ((uint32_t)F16Traits<half_tag>::from_float(v[1]) << 16);
        o[1] = (uint32_t)F16Traits<half_tag>::from_float(v[2]) | ((uint32_t)F16Traits<half_tag>::from_float(v[3]) << 16);
    } else {
        o[0] = (uint32_t)F16Traits<bf16_tag>::from_float(v[0]) | ((uint32_t)F16Traits<bf16_tag>::from_float(v[1]) << 16);
        o[1] = (uint32_t)F16Traits<bf16_tag>::from_float(v[2]) | ((uint32_t)F16Traits<bf16_tag>::from_float(v[3]) << 16);
    }
    *(u32x2*)((uint16_t*)e.out + m * e.stride_om + n0) = o;
}


// dequant of an integer code q (as float) for W_group_mode (triton_kernels/utils.py:73-87),
// evaluated in fp32 on the stored scale / zero
__device__ __forceinline__ float dequant_f32(float q, float s, float z, int w_mode) {
    switch (w_mode) {
        case 1: return q - z;
        case 2: return q * s;
        case 3: return (q - z) * s;
        case 4: return __builtin_fmaf(q, s, z);
        default: return q;
    }
}

// (a, b) such that  sum_k x_k * dequant(q_k) = a * sum_k x_k q_k + b * sum_k x_k  inside one group
__device__ __forceinline__ void group_affine(float s, float z, int w_mode, float& a, float& b) {
    switch (w_mode) {
        case 1: a = 1.0f; b = -z; break;
        case 2: a = s; b = 0.0f; break;
        case 3: a = s; b = -z * s; break;
        case 4: a = s; b = z; break;
        default: a = 1.0f; b = 0.0f; break;
    }
}

// Workspace layout: [arrival counters: MAX_SPLITK_COUNTERS x u32 | slabs].  The counters sit at a FIXED
// place so that slab payload of one shape can never alias the counters of another; kernels leave them zero.
// The last 4096 words of the block belong to the opt-in timeline probes (GEMLITE_TF_TIMELINE): never used as tickets.
constexpr int COUNTER_WORDS = 65536;
constexpr int PROBE_WORDS = 4096;
constexpr int MAX_SPLITK_COUNTERS = COUNTER_WORDS - PROBE_WORDS;
constexpr uint64_t COUNTER_BYTES = (uint64_t)COUNTER_WORDS * 4;

// tuning[3] as the kernels see it (WnParams::flags / GenericParams::flags): the caller's public bits (GEMLITE_TF_*), then what the planner adds.
// The planner's own bits: K_ORDER_ON turns on the K order of the row tiles of a column tile (KOrder, gl_async.h); its group field is bits 24 .. 27,
// the same bits as the public GEMLITE_TF_K_ORDER_GROUP_MASK override: 1 + log2(steps per group), 0 = whole-K rotation.
constexpr int K_ORDER_ON = 1 << 30;
constexpr int K_ORDER_GROUP_SHIFT = 24;
constexpr int K_ORDER_GROUPS_OF_1 = 1 << K_ORDER_GROUP_SHIFT;  // group field value 1: groups of one K step
static inline int caller_flags(const gemlite_hip_forward_args& a) { return a.tuning[3] & GEMLITE_TF_PUBLIC_MASK; }
#if defined(GL_MMA_EXPERIMENTS) || defined(GL_TILED_EXPERIMENTS)  // development builds: the EXP of the K-loop ablation kernels
static inline int dev_ablation() { const char* s = getenv("GEMLITE_DEV_ABLATION"); return s ? atoi(s) : 0; }
#endif

// ---------------------------------------------------------------------------------------------
// split-K hand-off words: write-through (sc1) stores / loads at agent scope
// (MI355X: per-XCD L2s are not coherent; see DESIGN.md "split-K combine")
// ---------------------------------------------------------------------------------------------
__device__ __forceinline__ void slab_store(float* p, float v) {
    __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
__device__ __forceinline__ float slab_load(const float* p) {
    return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// Every storing wave drains its write-through stores, the block joins, one lane takes a ticket.
// Returns true in every thread of the LAST block to arrive for `counter`.
__device__ __forceinline__ bool splitk_arrive_is_last(unsigned* counter, unsigned nslices, unsigned* lds_flag) {
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    if (threadIdx.x == 0) {
        *lds_flag = __hip_atomic_fetch_add(counter, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    __syncthreads();
    return *lds_flag == nslices - 1u;
}
__device__ __forceinline__ void splitk_reset(unsigned* counter) {
    __hip_atomic_store(counter, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// ---------------------------------------------------------------------------------------------
// kernel parameter block shared by the packed-weight kernels
// ---------------------------------------------------------------------------------------------
struct WnParams {
    const void* x;
    const uint32_t* w;   // packed int32 words [K/e, N]
    const void* scales;
    const void* zeros;
    Epilogue epi;
    float* slabs;        // split-K partial sums (workspace)
    unsigned* counters;  // split-K arrival counters (workspace, zero between launches)
    int M, N, K;
    int group_size;      // K elements per metadata row; == K for channel-wise / none
    int w_mode;          // W_group_mode
    int meta_dt, zeros_dt;
    int zero_is_scalar;
    int splitk;          // K slices (gridDim.y)
    int rows_per_slice;  // packed rows per K slice
    int64_t stride_xm, stride_xk, stride_wk, stride_meta_g;
    int64_t stride_wn_b, stride_meta_n;  // block-scaled K-contiguous weights (gemm_wn_mma.hip MXW): bytes between weight rows / scale columns
    int combine;         // K-slice combine: 0 = slabs + arrival ticket (last block sums), 1 = reduce-scatter between co-resident
                         // slices (gemm_wn_mma.hip; needs every block of the launch resident at once)
    int flags;           // experiment switches forwarded from tuning[3] (kernel-specific)
    int gs_shift;        // log2(group_size); 31 when one metadata row spans all of K; -1 (not a power of two)
                         // sends the problem to the coverage kernel — an integer division per metadata load costs
                         // ~50 VALU instructions and a branch in kernels that have ~300 per chunk — except in the 8-wave tile kernel
                         // (round 6), whose metadata row index is wave-uniform: k / group = mulhi(k / 32, gs_magic) on the scalar unit
    uint32_t gs_magic;   // ceil(2^32 / (group_size / 32)) for a group size that is a multiple of 32 and not a power of two, else 0
};

__device__ __forceinline__ int group_of(int k, int gs_shift) { return k >> gs_shift; }
// the same for kernels that also take group sizes that are multiples of 32 and not a power of two (k a multiple of 32; gs_magic: see WnParams)
__device__ __forceinline__ int group_of(int k, int gs_shift, uint32_t gs_magic) {
    return gs_shift >= 0 ? (k >> gs_shift) : (int)__umulhi((uint32_t)k >> 5, gs_magic);
}

// Two-buffer software pipeline over n >= 1 units (chunks / pieces of K): unit i + 2 is requested as soon as unit i
// has been consumed, and nothing is requested twice — a clamped "re-request the last unit" tail would stream the
// whole weight matrix through L2 -> L1 up to three times when n == 2, which is the case for the 4096 x 4096 decode
// shape.  The steady-state loop has unconditional loads so the compiler's vmcnt bookkeeping stays exact; the
// last (up to three) units are peeled.
template <typename Buf, typename Load>
__device__ __forceinline__ void pipeline2_prime(int n, Buf& A, Buf& B, Load&& load) {
    load(A, 0);
    if (n > 1) load(B, 1);
}
template <typename Buf, typename Load, typename Compute>
__device__ __forceinline__ void pipeline2_run(int n, Buf& A, Buf& B, Load&& load, Compute&& compute) {
    int i = 0;
    for (; i + 4 <= n; i += 2) {
        // (round 3, scripts/isa_loops.py: hipcc 7.2 waits with s_waitcnt vmcnt(0) at the head of this loop in every gemv_wn_kernel
        // variant, i.e. both buffers are drained per iteration, and its scheduler makes up for it by hoisting the next requests above
        // the arithmetic.  Pinning the four phases with sched_barrier(0) and priming unconditionally removed neither the drain nor
        // its cause and took the hoisting away: 16384^2 M = 1 went 23.7 -> 27.9 us, 8192^2 10.4 -> 11.3 us.  Left to the compiler.)
        compute(A, i);
        load(A, i + 2);
        compute(B, i + 1);
        load(B, i + 3);
    }
    const int rem = n - i;  // 1, 2 or 3
    compute(A, i);
    if (rem >= 2) {
        if (rem == 3) load(A, i + 2);
        compute(B, i + 1);
        if (rem == 3) compute(A, i + 2);
    }
}

// parameter block of the coverage kernels (generic.hip)
struct GenericParams {
    const void* x;
    const void* w;
    const void* scales;
    const void* zeros;
    Epilogue epi;
    int M, N, K;
    int nbits, e, pack_bits;  // e == 1: unpacked
    int w_dt;                 // dtype of unpacked weights
    int x_dt;
    int group_size, w_mode, meta_dt, zeros_dt, zero_is_scalar;
    int int_acc;              // int8 x integer weights: exact int32 accumulation
    int64_t stride_xm, stride_xk, stride_wk, stride_wn, stride_meta_g, stride_meta_n;
    // split-K of the A8W8 MFMA kernel (workspace, same layout as WnParams)
    float* slabs;
    unsigned* counters;
    int splitk;
    int flags;
    // block-scaled (MX / NV) formats, gemm_mx.hip: element formats of x / w (MX_F16, MX_BF16, MX_FP8, MX_FP4), the
    // per-block scales of x (channel_scale_mode 4: e8m0 bytes [M_pad, K/32], or e4m3 bytes [M_pad, K/16] for NVFP4),
    // and the constant the accumulator is multiplied by at the end (NVFP4 meta scale squared, else 1)
    const void* sx_blocks;
    int64_t stride_sx_blk_m;
    int mx_x, mx_w, mx_scale_e4m3;
    float mx_post;
    // cooperative activation quantisation inside the launch (gl_coopquant.h): the caller's 16-bit activations, their row stride
    // (elements) and type.  `x` / `epi.scales_x` then point at the workspace copies (row stride K) that the blocks fill first;
    // `counters` [0, M) are the row flags, [M] the departure count.
    const void* cq_x;
    int64_t cq_stride_xm;
    int cq_xdt;
};
enum { MX_F16 = 1, MX_BF16 = 2, MX_FP8 = 3, MX_FP4 = 4 };

// 8 consecutive weights of row n from k (k % 8 == 0) of a float matrix w[.., ld_w] as fp32 — the load of the weight quantisers
// (quantize_groups.hip, quantize_mx.hip).  vec: w and the row pitch are 16-byte aligned (one 16-byte load of a 16-bit input, two for fp32)
__device__ __forceinline__ void load8_as_float(const void* w, int w_dt, int64_t ld_w, bool vec, int64_t n, int64_t k, float (&v)[8]) {
    const int64_t off = n * ld_w + k;
    if (w_dt == GEMLITE_DT_FP32) {
        const float* s = (const float*)w + off;
        if (vec) {
            const f32x4 a = *(const f32x4*)s, b = *(const f32x4*)(s + 4);
            v[0] = a[0]; v[1] = a[1]; v[2] = a[2]; v[3] = a[3];
            v[4] = b[0]; v[5] = b[1]; v[6] = b[2]; v[7] = b[3];
        } else {
#pragma unroll
            for (int e = 0; e < 8; ++e) v[e] = s[e];
        }
    } else {
        const uint16_t* s = (const uint16_t*)w + off;
        uint32_t d[4];
        if (vec) {
            const u32x4 a = *(const u32x4*)s;
            d[0] = a[0]; d[1] = a[1]; d[2] = a[2]; d[3] = a[3];
        } else {
#pragma unroll
            for (int e = 0; e < 4; ++e) d[e] = (uint32_t)s[2 * e] | ((uint32_t)s[2 * e + 1] << 16);
        }
        const bool f16 = w_dt == GEMLITE_DT_FP16;
#pragma unroll
        for (int e = 0; e < 8; ++e) {
            const uint16_t h = (uint16_t)(d[e >> 1] >> (16 * (e & 1)));
            v[e] = f16 ? F16Traits<half_tag>::to_float(h) : F16Traits<bf16_tag>::to_float(h);
        }
    }
}

// parameter block of the block-scaled weight quantiser (quantize_mx.hip)
struct QuantMxParams {
    const void* w;    // [N, ld_w] fp32 / fp16 / bf16
    uint8_t* q_out;   // bytes [N, ld_q]: e4m3 (K per row), e2m1 codes one per byte (K) or two per byte (K / 2)
    uint8_t* scales;  // one byte per block, (block j, row n) at j * stride_scale_g + n * stride_scale_n
    int64_t N, K, ld_w, ld_q, stride_scale_g, stride_scale_n;
    int w_dt, pack;
};

// parameter block of the channel-wise 8-bit weight quantiser (quantize_rows.hip)
struct QuantRowsParams {
    const void* w;    // [N, ld_w] fp32 / fp16 / bf16
    uint8_t* q_out;   // bytes [N, ld_q]: int8 / e4m3 / e5m2, K per row
    void* scales;     // row n at n * stride_s (elements of scale_dt)
    int64_t N, K, ld_w, ld_q, stride_s;
    int w_dt, scale_dt, rule;
};

// parameter block of the grouped weight quantiser (quantize_groups.hip)
struct QuantGroupsParams {
    const void* w;   // [N, ld_w] fp32 / fp16 / bf16
    void* q_out;     // pack32: uint32 [K/e, N]; else uint8 [N, ld_q]
    void* scales;    // 16-bit, element (g, n) at g * stride_meta_g + n * stride_meta_n
    void* zeros;
    int64_t N, K, ld_w, ld_q, stride_meta_g, stride_meta_n;
    int64_t span;    // k owned by one block: lcm(group, 256), whole groups only
    int w_dt, meta_dt, nbits, group, pack32, fold;
};

// the optimiser's constants for quantize_hqq_kernel (quantize_groups.hip), beside a QuantGroupsParams
struct QuantHqqParams {
    int iters;
    float lp_norm, beta, kappa;
};

// parameter block of the weight dequantiser (dequantize.hip)
enum { DQ_INT = 0, DQ_MXFP8 = 1, DQ_MXFP4 = 2, DQ_NVFP4 = 3 };
struct DequantParams {
    const void* w;       // packed words [K/e, N], or unpacked elements, at j * stride_wk + n * stride_wn (elements of the word / element type)
    const void* scales;  // element (g, n) at g * stride_meta_g + n * stride_meta_n; block-scaled formats: one byte per block
    const void* zeros;
    void* out;           // [N, ld_out] fp16 / bf16 / fp32
    int64_t N, K, stride_wk, stride_wn, stride_meta_g, stride_meta_n, ld_out;
    int nbits, e, pack_bits;  // e == 1: unpacked (fp4 codes: one per byte)
    int w_dt, meta_dt, zeros_dt, zero_is_scalar, group, w_mode;
    int chan;            // multiply by the channel scale scales[n * stride_meta_n]
    int fmt;             // DQ_*
    int out_dt;
    float post;          // one more multiply when != 1
};

// host-side launch description produced by the dispatcher
// How many blocks of a one-block-per-CU kernel are resident at once on the current device (its CU count; 256 until a device
// has been seen).  Kernels whose blocks WAIT for each other (reduce-scatter combine) are only planned within this limit.
int resident_block_limit();
// kernel label of a form for 8- / 16-bit packed words (pack_bits 8 / 16): `name` with ",b8" / ",b16" before its closing '>' (api.hip)
const char* pw_label(const char* name, int pack_bits);
// kernel label of a form that adds the bias in its epilogue: `name` with ",bias" before its closing '>' (api.hip)
const char* bias_label(const char* name);

// scalar kernel arguments of gemv_w4_decode3_kernel (gemv_decode.hip): 14 dwords the command processor preloads into SGPRs
struct Decode3Args {
    const char *w, *x, *s, *z;
    uint16_t* out;
    uint32_t sw4, mstride2;
    int nch_total;
    uint32_t modes;
    unsigned* counters;
};

// The grouped kernels (gemv_w4_decode3_group_kernel, gemv_decode.hip; gemm_w4_rows[_bias]_group_kernel, gemm_wn_rows_group.hip): the
// pointers of members 1 .. DECODE3_GMAX - 1 of a grouped launch, passed by value behind the scalar arguments (member 0's: Decode3Args
// without `counters`, Rows5Args).  sw4 / mstride2 / nch_total / modes are shared by the group; a decode group's member count and grid.y
// ride in bits 16..23 / 24..31 of `modes` (decode3_group_modes), which no single-layer launch sets; a rows group has grid.y = members.
constexpr int DECODE3_GMAX = 16;
struct GroupMember {
    const char *w, *x, *s, *z;
    uint16_t* out;
};
// The BIASED forms (out = from_float(to_float(from_float(acc)) + to_float(bias[n])): both roundings of "matmul, then out += bias" kept).  The
// bias pointer of a single-layer decode launch travels behind the 14 preloaded dwords like `counters` (a biased launch never carries the
// timeline probe); a biased group holds one bias pointer per member, member 0's included.  A group is all-biased or all-unbiased.
struct Decode3BiasTail {
    const uint16_t* bias;
};
// gemv_w4_decode3_experts_kernel (gemv_decode.hip; gemlite_hip_forward_experts): what travels behind the 14 preloaded dwords, which are
// expert 0's pointers, x row 0 and slot 0 of the output.  Slot s = blockIdx.y uses expert ids[s]: the strides are bytes, 64-bit
struct ExpertsTail {
    const void* ids;        // int32 or int64 (the kernel's IDS64), n_slots entries
    const uint16_t* bias;   // expert 0's (the BIASED forms)
    int64_t stride_w, stride_meta, stride_bias;  // between experts
    int64_t stride_x, stride_out;                // between x rows / output slots
    uint32_t n_experts, slots_per_x_row;
};
// gemv_w4_decode3_experts_fused_kernel (gemlite_hip_forward_experts_fused): the experts tail, then what the epilogue needs.  stride_out is
// between the output rows of the launch: slots (GLU) or tokens (COMBINE)
struct ExpertsFusedTail {
    ExpertsTail e;
    const void* weights;  // COMBINE: the routing weights, n_slots entries in the order of ids; fp32 (w_f32) or the output type
    uint32_t members;     // COMBINE: slots per token = members of a block, 1 .. DECODE3_GMAX
    uint32_t half_tiles;  // GLU: I / 16, the tiles between a block's gate tile and its up tile
    uint32_t w_f32;
};
// gemm_w4_rows_experts_kernel (gemm_wn_rows_experts.hip; gemlite_hip_forward_experts_rows): what travels behind the scalars of the rows
// kernel.  The work table is written by experts_route_kernel (experts_route.hip): [0] used blocks, [1..3] zero, block_expert[Bmax] at
// EXPERTS_ROWS_HEADER, block_rows[Bmax * R] behind it; Bmax = gridDim.y of the rows launch
constexpr int EXPERTS_ROWS_HEADER = 4;
struct ExpertsRowsTail {
    const int32_t* table;
    const uint16_t* bias;                        // expert 0's (the BIASED forms)
    int64_t stride_w, stride_meta, stride_bias;  // bytes between experts
    uint32_t n_experts, slots_per_x_row, n_slots;  // (an entry of the table that is no slot of this launch counts as -1: memory safety on a foreign table)
    uint32_t x_bytes;                            // extent of ALL of x (below 2^31): num_records of the gather's buffer descriptor
};
inline int64_t experts_rows_bmax(int64_t n_slots, int64_t n_experts, int64_t R) {
    return (n_slots + R - 1) / R + (n_experts + 1 < n_slots ? n_experts + 1 : n_slots);
}
// gemm_w4_rows_experts_glu_kernel (gemm_wn_rows_experts_glu.hip; gemlite_hip_forward_experts_rows_glu): the rows tail, then the distance
// between a block's gate tile and its up tile.  The launch's output rows are I = 16 half_tiles wide
struct ExpertsRowsGluTail {
    ExpertsRowsTail rows;
    uint32_t half_tiles;  // I / 16
};
// experts_combine_kernel (experts_combine.hip; gemlite_hip_experts_combine): out[t] = round(sum_k w[t spt + k] * y[t spt + k]) over the
// slots with a valid id.  Strides in elements, below 2^31 with the row behind them
struct ExpertsCombineArgs {
    const uint16_t* y;
    const void* ids;      // int32 or int64 (the kernel's IDS64)
    const void* weights;  // fp32 or the type of y (the kernel's W32)
    uint16_t* out;
    uint32_t n_experts, spt, N;
    uint32_t stride_y, stride_out;
};
// experts_topk_kernel (experts_topk.hip; gemlite_hip_experts_topk): one wave per token; the row stride in elements, 64-bit
struct ExpertsTopkArgs {
    const void* logits;
    const float* bias;  // sigmoid only; nullptr: the key is the logit
    void* ids;          // int32 or int64 (ids64)
    void* weights;      // fp32, fp16 or bf16 (w_dt)
    int64_t stride;
    uint32_t n_tokens, E, top_k;
    uint32_t sigmoid, renorm, ids64, w_dt;  // w_dt 0: fp16, 1: bf16, 2: fp32
    float scale;
};

// silu of the GLU epilogues (gemv_w4_decode3_experts_fused_kernel, gemm_w4_rows_experts_glu_kernel): v / (1 + exp(-v)) in fp32.  Below
// -88 exp(-v) leaves fp32 and the quotient is -0, while silu(v) = v exp(v) is a normal bf16 number down to about -92 and a subnormal
// one down to -97: there v exp(v / 2) exp(v / 2), whose factors stay normal.  v = -Inf gives -Inf * 0 = NaN, as the quotient does
__device__ __forceinline__ float silu_f32(float v) {
    float act = v / (1.f + expf(-v));
    if (v < -88.f) {
        const float hv = expf(0.5f * v);
        act = (v * hv) * hv;
    }
    return act;
}
template <bool BIASED>
struct GroupTable {
    GroupMember m[DECODE3_GMAX - 1];
    const uint16_t* bias[DECODE3_GMAX];
};
template <>
struct GroupTable<false> {
    GroupMember m[DECODE3_GMAX - 1];
};
// (capture_group.hip keeps ONE biased table per group and hands it to either kind of kernel: an unbiased kernel's argument is its prefix)
static_assert(offsetof(GroupTable<true>, m) == 0 && sizeof(GroupTable<false>) == offsetof(GroupTable<true>, bias), "the unbiased table is a prefix of the biased one");
static_assert(sizeof(GroupTable<false>) == 600 && sizeof(GroupTable<true>) == 728, "kernel-argument layout of the grouped kernels");
// ROUNDS.  A grouped DECODE node holds R >= 1 rounds of m <= DECODE3_GMAX members each, m * R <= DECODE3_NODE_MAX (capture_group.hip merges
// full neighbouring groups of a capture into one node): grid (grid_x, Y * R), block (x, yy) is block (x, yy % Y) of round yy / Y and does
// on the members m * round + ... of the table what block (x, y) of a one-round node does on its own.  The decode forms therefore take a
// table of their own, DECODE3_NODE_MAX - 1 members (and DECODE3_NODE_MAX bias pointers) by value; DECODE3_GMAX keeps meaning the members
// of one round, the slots of a block and its LDS regions.  The rows and experts kernels keep GroupTable.
constexpr int DECODE3_NODE_MAX = 64;
// rounds a node may hold: the hard limit of GEMLITE_HIP_CAPTURE_GROUP_ROUNDS, and the limit when nothing is set (capture_group.hip, ROUNDS)
constexpr int DECODE3_ROUNDS_LIMIT = 4, DECODE3_ROUNDS_DEFAULT = 4;
static_assert(DECODE3_ROUNDS_LIMIT * DECODE3_GMAX <= DECODE3_NODE_MAX, "a node of full rounds fits its table");
template <bool BIASED>
struct DecodeNodeTable {
    GroupMember m[DECODE3_NODE_MAX - 1];
    const uint16_t* bias[DECODE3_NODE_MAX];
};
template <>
struct DecodeNodeTable<false> {
    GroupMember m[DECODE3_NODE_MAX - 1];
};
static_assert(offsetof(DecodeNodeTable<true>, m) == 0 && sizeof(DecodeNodeTable<false>) == offsetof(DecodeNodeTable<true>, bias),
              "the unbiased node table is a prefix of the biased one");
// (the whole kernel-argument segment: the nine scalars in 56 bytes, the table, and the 256 bytes of hidden arguments a code object may add)
static_assert(56 + sizeof(DecodeNodeTable<true>) + 256 <= 4096, "kernel-argument segment of the grouped decode forms");
// The index rule, kernel and host: the member of the node's table that block row `block_y` of a node with m members per round and
// Y block rows per round holds as its block-local layer `li`.  One round (block_y < Y): y + li * Y, what it always was.
// (a block row is below 2^16 and Y below 2^8: the masks tell the compiler so, and the divide is the short one through the reciprocal)
GL_HD int decode3_round(int Y, int block_y) { return (int)((unsigned)(block_y & 0xFFFF) / (unsigned)(Y & 0xFF)); }
GL_HD int decode3_round_row(int Y, int block_y) { return (int)((unsigned)(block_y & 0xFFFF) % (unsigned)(Y & 0xFF)); }
GL_HD int decode3_round_member(int m, int Y, int block_y, int li) {
    return m * decode3_round(Y, block_y) + decode3_round_row(Y, block_y) + li * Y;
}
// LDS of a shared-x block: the 64 KiB of partial rows (DECODE3_GMAX layers x 4 KiB), then per 16-element unit of x (K / 16 = 16 per 32-row
// chunk) 32 bytes of pair dwords, then per unit its 4-byte sum: 64 KiB + 2.25 K bytes, dynamic.  The block's 1024 threads stage the
// units in trips of 1024.  0: the staging area does not fit beside the partial rows in the 160 KiB of a CU (K > 43520).
constexpr int64_t DECODE3_RED_BYTES = (int64_t)DECODE3_GMAX * 16 * 4 * 16 * 4, DECODE3_LDS_LIMIT = 160 * 1024;
constexpr int64_t DECODE3_SHARED_X_MAX_UNITS = ((DECODE3_LDS_LIMIT - DECODE3_RED_BYTES) / 36) & ~(int64_t)15;  // 2720, whole chunks
constexpr int64_t DECODE3_SHARED_X_MAX_LDS = DECODE3_RED_BYTES + DECODE3_SHARED_X_MAX_UNITS * 36;  // the cap api.hip raises once per kernel
// (two members: staging and its barrier cost more than they save, 4.11 us per layer against 3.82 — profiles/r15/decode_group_shared_x.log §5)
constexpr int DECODE3_SHARED_X_MIN_MEMBERS = 3;
inline int64_t decode3_shared_x_lds_bytes(int64_t nch_total) {
    return (nch_total > 0 && nch_total * 16 <= DECODE3_SHARED_X_MAX_UNITS) ? DECODE3_RED_BYTES + nch_total * 16 * 36 : 0;
}
// The form of a grouped node: 0 no group (one member), 1 per-wave x (every wave loads the x of its own layer), 2 shared x
inline int decode3_group_form(int members, bool same_x, int64_t nch_total, bool shared_x_enabled) {
    if (members < 2) return 0;
    return (shared_x_enabled && same_x && members >= DECODE3_SHARED_X_MIN_MEMBERS && decode3_shared_x_lds_bytes(nch_total) > 0) ? 2 : 1;
}
// `modes` of a grouped launch: members in bits 16..20, log2 of the tiles per block (TB) in 21..22, the span placement in 23, grid.y in
// 24..31.  TB = 1 without the span bit is the word the launch carried before tile groups existed.  (The tiles per wave, H, are not in
// the word: every H has kernel functions of its own.)
constexpr uint32_t DECODE3_M_MEMBERS = 31u, DECODE3_M_TB_SHIFT = 21u, DECODE3_M_SPAN = 1u << 23;
inline uint32_t decode3_group_modes(uint32_t modes, int members, int grid_y, int tb = 1, bool span = false) {
    return (modes & 0xFFFFu) | ((uint32_t)members << 16) | ((tb == 4 ? 2u : (tb == 2 ? 1u : 0u)) << DECODE3_M_TB_SHIFT) | (span ? DECODE3_M_SPAN : 0u) |
           ((uint32_t)grid_y << 24);
}
// grid.y of a grouped launch of `members` layers of `tiles` 16-column tiles each: block (tile, y) holds the layers y, y + grid.y, ...
// One block per CU is resident, so a wide layer (tiles >= resident) gets one block per tile that holds every member; a narrow one
// spreads its members over the CUs its tiles leave idle.
GL_HD int decode3_group_grid_y(int64_t tiles, int members, int64_t resident) {
    const int64_t y = tiles > 0 ? resident / tiles : 1;
    return (int)(y < 1 ? 1 : (y > members ? (members > 1 ? members : 1) : y));
}
// How the 16 waves of a grouped block share its `lb` layers (1 .. DECODE3_GMAX), all in flight at once: P = 16 / lb waves per layer,
// wave w works on block-local layer w / P (the waves past lb * P have no work) and, inside it, takes the place of the single-layer kernel's
// waves [v0, v1) — "virtual waves", a contiguous share of 16: virtual wave v is the chunks v, v + 16, ... of the layer.
struct Decode3WaveSplit {
    int layer;   // block-local layer, -1: the wave has no items
    int v0, v1;  // its virtual waves [v0, v1)
};
GL_HD Decode3WaveSplit decode3_wave_split(int lb, int wave) {
    const int P = 16 / lb, li = wave / P, wl = wave - li * P;
    if (li >= lb) return Decode3WaveSplit{-1, 0, 0};
    return Decode3WaveSplit{li, wl * 16 / P, (wl + 1) * 16 / P};
}
// TILE GROUPS.  A grouped block holds TB in {1, 2, 4} ADJACENT 16-column tiles x LB layers: grid (tiles / TB, Y) with
// Y = decode3_group_grid_y(tiles / TB, members, resident) and LB = ceil((members - y) / Y).  Its LB * TB (layer, tile) SLOTS (at most 16)
// take the place of the layers in decode3_wave_split(): slot s is block-local layer s / TB and tile s % TB of the block's tile group, so
// the waves that read the two (TB = 2) or four (TB = 4: two lines) 64-byte halves of a weight row's 128-byte lines are neighbours on one
// CU and walk the same item list.  Each slot owns one 4 KiB partial-row region, as each layer did.  (With LINES, below, a wave takes
// H adjacent slots of one layer at once — a WAVE-SLOT — in H passes, and decode3_wave_split() is called on LB * TB / H wave-slots.)
// The rule: the largest TB <= tb_want with tiles % TB == 0 and ceil(members / Y) * TB <= 16.
struct Decode3GroupGeometry {
    int tb, grid_x, grid_y;
    bool span;
};
GL_HD Decode3GroupGeometry decode3_group_geometry(int tiles, int members, int64_t resident, int tb_want, bool span) {
    for (int tb = tb_want >= 4 ? 4 : (tb_want >= 2 ? 2 : 1); tb > 1; tb >>= 1) {
        if (tiles % tb) continue;
        const int y = decode3_group_grid_y(tiles / tb, members, resident);
        if ((members + y - 1) / y * tb <= 16) return Decode3GroupGeometry{tb, tiles / tb, y, span};
    }
    return Decode3GroupGeometry{1, tiles, decode3_group_grid_y(tiles, members, resident), span};
}
// Block x of `groups` = tiles / TB -> the first tile of its tile group (speed only: any permutation is correct).  Blocks are dealt
// round-robin over the 8 XCDs, so block b runs on "XCD" b % 8.
//   interleaved (span = false): TB = 1 and `pair` (tiles % 16 == 0): the pair map — XCD x takes the tiles 16 m + 2 x, 16 m + 2 x + 1 (both
//       halves of the lines 8 m + x of a weight row); otherwise the identity (TB = 2: XCD x takes the lines 8 m + x as before, each
//       inside one block).
//   span (span = true): XCD x takes the contiguous tile groups [x groups / 8, (x + 1) groups / 8); the identity when groups % 8 != 0.
GL_HD int decode3_group_first_tile(int block, int groups, int tb, bool span, bool pair) {
    const int xcd = block & 7, idx = block >> 3;
    int grp = block;
    if (span) {
        if ((groups & 7) == 0) grp = xcd * (groups >> 3) + idx;
    } else if (pair && tb == 1) {
        grp = (((idx >> 1) << 3) + xcd) * 2 + (idx & 1);
    }
    return grp * tb;
}
// LINES.  A wave of a grouped block works on H in {1, 2, 4} adjacent tiles of the block's tile group at once: its 64 lanes are H sub-waves
// of 64 / H lanes, sub-wave h on tile run * H + h, lane l' of a sub-wave is (c = l' & 3, gl = l' >> 2) and in pass p = 0 .. H - 1 over a
// virtual wave takes the row pair g = p * 16 / H + gl.  One request instruction then covers one row of each of its 16 / H row pairs, in H tiles: 8 rows x 128
// contiguous bytes (H = 2) or 4 rows x 256 (H = 4) instead of 16 rows x 64, and every 128-byte line is asked for by ONE instruction.
// What the waves share is the block's LB * TB / H WAVE-SLOTS (a layer x a run of H tiles): decode3_wave_split() is called on that count,
// a wave's items are (virtual wave, pass, chunk) ascending, and sub-wave h of wave-slot ws fills slot ws * H + h — the same 4 KiB region,
// partial row v * 4 + r with r = p * 4 / H + (16-lane row inside the sub-wave), as the four row pairs 4 r .. 4 r + 3 always wrote.
// H must divide TB: a wanted H falls back 4 -> 2 -> 1.
GL_HD int decode3_group_lines(int tb, int h_want) {
    int h = h_want >= 4 ? 4 : (h_want >= 2 ? 2 : 1);
    while (h > tb) h >>= 1;
    return h;
}
// The H a launch carries when nothing is forced.  THE RULE (measured: profiles/r18/decode_group_lines.log §4 - §6): whole lines whenever the
// block holds them — H = 2 for every TB >= 2 — and H = 4 where TB = 4 and the fullest block holds four layers.  At 256 tiles on 256 CUs
// H = 2 beat H = 1 by 7 - 15 % at every member count measured under TB = 2 (2, 5, 6) and TB = 4 (4, 7, 8, 10, 12, 15, 16); H = 4 was
// 2 - 10 % SLOWER than H = 2 where the fullest block holds one to three layers (4 - 12 members: one to three wave-slots per block, every
// wave of the CU on the same 256-byte column strip) and level with it or ahead where it holds four (15, 16 members).
inline int decode3_group_lines_default(int tiles, int members, int64_t resident, int tb) {
    if (tb < 2) return 1;
    const Decode3GroupGeometry geo = decode3_group_geometry(tiles, members, resident, tb, false);
    const int lb = (members + geo.grid_y - 1) / geo.grid_y;  // layers of the fullest block
    return (geo.tb == 4 && lb >= 4) ? 4 : 2;
}
// POLICY.  Does a grouped launch ask for its weights non-temporally (the NT forms of gemv_w4_decode3_group_kernel)?  Only when
//   * H >= 2: one request instruction covers whole 128-byte lines.  With H = 1 the other half of a line belongs to another wave, which
//     asks later, when a non-temporal line has left the L2 (profiles/r13/decode_group_waves.log §2);
//   * the members' own launches are non-temporal (members_nt: the layer's tuning carries no GEMLITE_TF_GEMV_DEFAULT_POLICY_LOADS — the
//     switch for a model whose weights stay in the Infinity Cache from step to step);
//   * every member's weight base and the row pitch sw4 are multiples of 128 bytes (w_bases_or: the members' bases OR-ed together).
//     Otherwise a line straddles two waves' requests again: slower, never wrong.
// forced: -1 the rule; 0 / 1 GEMLITE_HIP_CAPTURE_GROUP_NT — a forced 1 overrides the last two conditions, never the first.
GL_HD bool decode3_group_nt(int h, bool members_nt, uint64_t w_bases_or, uint32_t sw4, int forced = -1) {
    if (h < 2 || forced == 0) return false;
    if (forced > 0) return true;
    return members_nt && ((w_bases_or | (uint64_t)sw4) & 127u) == 0;
}
// What capture_group.hip asks decode3_group_geometry() for when nothing is forced: {tb_want, span} from the group's shape.
// THE RULE (measured: profiles/r16/decode_group_tiles.log §4 - §6): the interleaved placement, and the largest TB whose busiest CU gets
// at most 5/4 of the work the busiest CU has with one tile per block.  Work of the busiest CU in (layer, tile) slots: rounds of blocks
// over the resident CUs x layers of the fullest block x TB.  16 members of 256 tiles on 256 CUs: 1 x 16 x 1 = 1 x 8 x 2 = 1 x 4 x 4, so
// TB = 4 (whole 256-byte runs of every weight row on one CU: 2.41 -> 2.01 us per layer); 4, 8 and 12 members likewise.  A member count
// that grid.y = 4 does not divide leaves the blocks unequal: 7, 10 and 15 members (8 / 7, 12 / 10, 16 / 15 of the work) were still 12,
// 10 and 13 % faster on TB = 4, six members (8 / 6) no faster than on TB = 2, five (8 / 5) and three (4 / 3, a quarter of the CUs idle)
// SLOWER than on TB = 1, two members on TB = 4 leave half the CUs idle.  The 5/4 bound gives every measured member count the TB that
// was fastest for it: 1 for 3; 2 for 2, 5 and 6; 4 for 4, 7, 8, 10, 12, 15 and 16.
// The span placement was slower than the interleaved one under every TB and is never chosen.
struct Decode3TilesWanted {
    int tb;
    bool span;
};
GL_HD int64_t decode3_group_busiest_cu(int tiles, int members, int64_t resident, int tb) {
    const Decode3GroupGeometry geo = decode3_group_geometry(tiles, members, resident, tb, false);
    if (geo.tb != tb) return -1;  // the shape does not admit this TB
    const int64_t blocks = (int64_t)geo.grid_x * geo.grid_y, cus = resident > 0 ? resident : 1;
    return (blocks + cus - 1) / cus * ((members + geo.grid_y - 1) / geo.grid_y) * tb;
}
inline Decode3TilesWanted decode3_group_tiles_default(int tiles, int members, int64_t resident) {
    const int64_t one = decode3_group_busiest_cu(tiles, members, resident, 1);
    for (int tb = 4; tb > 1; tb >>= 1) {
        const int64_t c = decode3_group_busiest_cu(tiles, members, resident, tb);
        if (c >= 0 && c * 4 <= one * 5) return Decode3TilesWanted{tb, false};
    }
    return Decode3TilesWanted{1, false};
}

// Waves per SIMD the compiler must keep resident for the grouped kernel (the second __launch_bounds__ argument of HIP).  One 1024-thread
// block is 4 waves per SIMD = 128 VGPRs per lane (two blocks per CU, 64 VGPRs, spill: profiles/r07/capture_groups.log)
#ifndef DECODE3_GROUP_WAVES_PER_SIMD
#define DECODE3_GROUP_WAVES_PER_SIMD 4
#endif

// scalar kernel arguments of gemm_w4_rows_kernel (gemm_wn_rows.hip): the same 14 preloaded dwords, then M and the row strides
struct Rows5Args {
    const char *w, *x, *s, *z;
    uint16_t* out;
    uint32_t sw4, mstride2;
    int nch_total;
    uint32_t modes;
    int M;
    uint32_t sxm2, som;
};

constexpr int ROWS5_GMAX = DECODE3_GMAX;  // members of a grouped rows launch (GroupTable, above)

struct LaunchPlan {
    const void* fn;
    const char* name;
    dim3 grid, block;
    size_t lds_bytes;
    uint64_t ws_bytes;    // total workspace needed (COUNTER_BYTES + slab_bytes when K is split, else 0)
    uint64_t slab_bytes;
    int arg_kind;         // 0: the kernel takes its parameter struct by value | 1: the scalar arguments of `d3` | 2: those of `r5`
    Decode3Args d3;
    Rows5Args r5;
    // the form of `bias_of` that adds a 16-bit bias[N] of the output's type in its epilogue (decode3 and rows kernels only; apply_bias, plan_forward.hip, swaps
    // it in when the caller's gemlite_hip_forward_ext qualifies and `fn` is still `bias_of`), and the bias pointer once it has
    const void* fn_bias = nullptr;
    const void* bias_of = nullptr;
    const uint16_t* bias = nullptr;
    // the grouped forms of `bias_of` and of `fn_bias` (rows kernels only: capture_group.hip rewrites a capture's node to one of them)
    const void* fn_group = nullptr;
    const void* fn_bias_group = nullptr;
    // decode3 launches: the dtype tag capture_group.hip asks gemv_w4_decode3_group_fn() with, at every join (H, shared x: the join's choice)
    int d3_group_tag = -1;  // 0 fp16 | 1 bf16 | -1: the launch has no grouped forms
    bool d3_nt = false;     // `fn` asks for its weights non-temporally (decode3_group_nt: a group follows its members)
};

}  // namespace gl
