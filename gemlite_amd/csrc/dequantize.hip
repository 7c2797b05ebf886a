// dequantize.hip — a layer's stored weights -> W[N, K] fp16 / bf16 / fp32, K-contiguous (DESIGN §2.3 has the contract; tests/dequant_spec.py
// restates it in torch).  q = the code of the packed word or the unpacked element as fp32 (exact); every step ONE fp32 IEEE operation
// (contraction is off for this file; the one multiply-add is the explicit fmaf of mode 4), then one round-to-nearest-even conversion:
//   W_group_mode 0: d = q | 1: d = q - z | 2: d = q * s | 3: d = (q - z) * s | 4: d = fmaf(q, s, z');   channel_scale_mode 1 / 3: d = d * c[n]
//   MXFP8 / MXFP4: d = elem * 2^(b - 127) (b = 0xFF: NaN);   NVFP4: d = elem * float(s8);   post != 1: d = d * post
// One launch per matrix, no workspace, no atomics.  The output is 4 - 16 x the input bytes: all three kernels are shaped by their stores.
//
// dequantize_words_kernel<NBITS>   32-bit words [K/e, N] with unit stride along n, group % 8 == 0, 16-byte aligned out rows.
//   A block owns 64 rows (n) x 256 k, the tile of both quantisers.  The tile's WORDS (256 / e word rows x 64 n) are read with consecutive
//   lanes along n — whole 256-byte row segments — and turned through LDS as words, not as expanded values; the metadata of the groups that
//   meet the tile (at most 33 of them: group >= 8, and a group that straddles two tiles is staged by both) and the channel scales are staged
//   once per block, lanes along n.  A thread then owns 8 consecutive k of one row: it unpacks them from its word (two words for 8-bit
//   codes), applies the contract and stores 16 bytes (16-bit out) or 2 x 16 bytes (fp32): consecutive lanes run along k, so a row of the tile
//   leaves as one contiguous 512- / 1024-byte run.
//   LDS pitch: 65 words per word row.  Banks are (byte address / 4) % 32 per 32-lane half.  Write: word row jl fixed per wave, lanes along n:
//   bank (65 jl + n) % 32 = (jl + n) % 32, 32 different banks per half: 0 conflicts.  Turned read: row r fixed per half, lane c reads word row
//   jl(c): 4-bit jl = c: bank (c + r) % 32, 0 conflicts; 2-bit jl = c / 2 and 1-bit jl = c / 4: lanes that share a word read the same
//   address (a broadcast), the others differ: 0 conflicts; 8-bit jl = 2c and 2c + 1: bank (2c + r) % 32, lanes c and c + 16 meet: 2-way on
//   each of the two reads (any pitch: 2 x pitch x c takes at most 16 values mod 32).  The metadata rows have the same pitch of 65 floats: the lanes of one group read
//   one address (a broadcast), different groups of a row sit in banks (gl + r) % 32: 0 conflicts.
// dequantize_rows_kernel<FMT>      K-contiguous bytes [N][K] (int8 / uint8 codes / e4m3 / e5m2 under any group mode with group % 8 == 0, MXFP8, one
//   fp4 code per byte) or [N][K / 2] (two fp4 codes per byte).  No turn: a thread loads 8 bytes (4 for packed fp4) of one row and stores 16 / 32,
//   lanes along k.  Only the tile's metadata goes through LDS, read with consecutive lanes along n: the block-scale bytes (64 n x 8 or 16
//   blocks), or the (s, z) of its groups and the 64 channel scales, staged as in the words kernel.
// dequantize_any_kernel            one thread per output element: 8- / 16-bit words, any strides, any group size, 16- / 32-bit float elements,
//   unaligned out.  Correct and slow.
// Lanes beyond N or K load nothing and store nothing (K % 8 == 0 in the two tiled kernels: a piece of 8 k is inside K or outside).
#include "gl_common.h"
#include "gl_host.h"

#pragma clang fp contract(off)

namespace gl {

typedef float f32x2 __attribute__((ext_vector_type(2)));

// e2m1 code -> value: magnitudes 0, 0.5, 1, 1.5, 2, 3, 4, 6 from the bits (no table in memory), bit 3 the sign (code 8 is -0.0)
__device__ __forceinline__ float dq_e2m1(uint32_t c) {
    const uint32_t m = c & 7u;
    const uint32_t mag = m >= 2u ? (((126u + (m >> 1)) << 23) | ((m & 1u) << 22)) : (m == 1u ? 0x3F000000u : 0u);
    return __builtin_bit_cast(float, mag | ((c & 8u) << 28));
}

// e8m0 byte -> 2^(b - 127): b = 0 is the subnormal 2^-127, b = 0xFF NaN
__device__ __forceinline__ float dq_e8m0(uint32_t b) {
    return __builtin_bit_cast(float, b == 0xFFu ? 0x7FC00000u : (b == 0u ? 0x00400000u : b << 23));
}

// 4 bytes of type dt -> fp32 (e4m3 / e5m2 by the hardware converters)
__device__ __forceinline__ void dq_bytes4(uint32_t v, int dt, float* o) {
    if (dt == GEMLITE_DT_FP8E4) {
        const f32x2 lo = __builtin_amdgcn_cvt_pk_f32_fp8((int)v, false), hi = __builtin_amdgcn_cvt_pk_f32_fp8((int)v, true);
        o[0] = lo[0]; o[1] = lo[1]; o[2] = hi[0]; o[3] = hi[1];
    } else if (dt == GEMLITE_DT_FP8E5) {
        const f32x2 lo = __builtin_amdgcn_cvt_pk_f32_bf8((int)v, false), hi = __builtin_amdgcn_cvt_pk_f32_bf8((int)v, true);
        o[0] = lo[0]; o[1] = lo[1]; o[2] = hi[0]; o[3] = hi[1];
    } else if (dt == GEMLITE_DT_INT8) {
#pragma unroll
        for (int i = 0; i < 4; ++i) o[i] = (float)(int)(int8_t)(v >> (8 * i));
    } else {
#pragma unroll
        for (int i = 0; i < 4; ++i) o[i] = (float)((v >> (8 * i)) & 0xFFu);
    }
}

__device__ __forceinline__ float dq_finish(float d, bool chan, float c, float post) {
    if (chan) d = d * c;
    if (post != 1.f) d = d * post;
    return d;
}

// 8 consecutive outputs of row n from k (16-byte aligned by the host's choice of kernel)
__device__ __forceinline__ void dq_store8(const DequantParams& p, int64_t n, int64_t k, const float (&d)[8]) {
    if (p.out_dt == GEMLITE_DT_FP32) {
        float* o = (float*)p.out + n * p.ld_out + k;
        *(f32x4*)o = (f32x4){d[0], d[1], d[2], d[3]};
        *(f32x4*)(o + 4) = (f32x4){d[4], d[5], d[6], d[7]};
        return;
    }
    u32x4 w;
    if (p.out_dt == GEMLITE_DT_FP16) {
#pragma unroll
        for (int i = 0; i < 4; ++i) w[i] = (uint32_t)F16Traits<half_tag>::from_float(d[2 * i]) | ((uint32_t)F16Traits<half_tag>::from_float(d[2 * i + 1]) << 16);
    } else {
#pragma unroll
        for (int i = 0; i < 4; ++i) w[i] = (uint32_t)F16Traits<bf16_tag>::from_float(d[2 * i]) | ((uint32_t)F16Traits<bf16_tag>::from_float(d[2 * i + 1]) << 16);
    }
    *(u32x4*)((uint16_t*)p.out + n * p.ld_out + k) = w;
}

// The metadata of a 64 n x 256 k tile into LDS, lanes along n: (s, z) of the groups that meet the tile — at most 255 / g + 2 <= 33 for
// g >= 8, rows of DQ_PITCH floats — and the channel scales of its rows.  Rows beyond N are left unwritten and are never read.
constexpr int DQ_TN = 64, DQ_TK = 256, DQ_PITCH = 65, DQ_MAXG = 33;
__device__ __forceinline__ void dq_stage_meta(const DequantParams& p, int64_t n0, int64_t k0, float* sS, float* sZ, float* sC) {
    const int tid = threadIdx.x;
    const bool need_s = p.w_mode >= 2, need_z = (p.w_mode == 1 || p.w_mode >= 3) && !p.zero_is_scalar;
    if (need_s || need_z) {
        const int64_t kend = (p.K - k0) < DQ_TK ? p.K : k0 + DQ_TK, g0 = k0 / p.group;
        const int ng = (int)((kend - 1) / p.group - g0) + 1;
        for (int o = tid; o < ng * DQ_TN; o += 256) {
            const int gl = o / DQ_TN, nl = o % DQ_TN;
            const int64_t n = n0 + nl;
            if (n >= p.N) continue;
            const int64_t idx = (g0 + gl) * p.stride_meta_g + n * p.stride_meta_n;
            if (need_s) sS[gl * DQ_PITCH + nl] = load_as_float(p.scales, idx, p.meta_dt);
            if (need_z) sZ[gl * DQ_PITCH + nl] = load_as_float(p.zeros, idx, p.zeros_dt);
        }
    }
    if (p.chan && tid < DQ_TN && n0 + tid < p.N) sC[tid] = load_as_float(p.scales, (n0 + tid) * p.stride_meta_n, p.meta_dt);
}

template <int NBITS>
__global__ __launch_bounds__(256) void dequantize_words_kernel(const DequantParams p) {
    constexpr int TN = DQ_TN, TK = DQ_TK, E = 32 / NBITS, WPT = TK / E, PITCH = DQ_PITCH, MAXG = DQ_MAXG;
    __shared__ uint32_t sW[WPT * PITCH];
    __shared__ float sS[MAXG * PITCH], sZ[MAXG * PITCH], sC[TN];
    const int tid = threadIdx.x;
    const int64_t n0 = (int64_t)blockIdx.x * TN, k0 = (int64_t)blockIdx.y * TK;
    const bool need_s = p.w_mode >= 2, need_z = (p.w_mode == 1 || p.w_mode >= 3) && !p.zero_is_scalar;
    const int64_t g = p.group, g0 = k0 / g;

    const int64_t j0 = k0 / E;
    for (int o = tid; o < WPT * TN; o += 256) {
        const int jl = o / TN, nl = o % TN;
        const int64_t n = n0 + nl, j = j0 + jl;
        uint32_t w = 0u;
        if (n < p.N && j * E < p.K) w = ((const uint32_t*)p.w)[j * p.stride_wk + n];
        sW[jl * PITCH + nl] = w;
    }
    dq_stage_meta(p, n0, k0, sS, sZ, sC);
    const float zs = ((p.w_mode == 1 || p.w_mode >= 3) && p.zero_is_scalar) ? load_as_float(p.zeros, 0, p.zeros_dt) : 0.f;
    __syncthreads();

    const int c = tid & 31;
    const int64_t k = k0 + c * 8;
    if (k >= p.K) return;
    const int jl = (c * 8) / E, sub = (c * 8) % E;
    const int gl = (int)(k / g - g0);
#pragma unroll 2
    for (int it = 0; it < 8; ++it) {
        const int r = it * 8 + (tid >> 5);
        const int64_t n = n0 + r;
        if (n >= p.N) break;
        const uint32_t w0 = sW[jl * PITCH + r];
        uint32_t w1 = 0u;
        if constexpr (NBITS == 8) w1 = sW[(jl + 1) * PITCH + r];
        const float s = need_s ? sS[gl * PITCH + r] : 1.f;
        const float z = need_z ? sZ[gl * PITCH + r] : zs;
        const float cs = p.chan ? sC[r] : 1.f;
        float d[8];
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            uint32_t q;
            if constexpr (NBITS == 8) q = ((i < 4 ? w0 : w1) >> (8 * (i & 3))) & 0xFFu;
            else q = (w0 >> ((sub + i) * NBITS)) & ((1u << NBITS) - 1u);
            d[i] = dq_finish(dequant_f32((float)q, s, z, p.w_mode), p.chan != 0, cs, p.post);
        }
        dq_store8(p, n, k, d);
    }
}

template <int FMT>
__global__ __launch_bounds__(256) void dequantize_rows_kernel(const DequantParams p) {
    constexpr int TN = DQ_TN, TK = DQ_TK, PITCH = DQ_PITCH, G = FMT == DQ_NVFP4 ? 16 : 32, NB = TK / G;
    constexpr int MW = FMT == DQ_INT ? DQ_MAXG * DQ_PITCH : 1, CW = FMT == DQ_INT ? TN : 1, BW = FMT == DQ_INT ? 1 : NB * TN;
    __shared__ uint8_t sB[BW];
    __shared__ float sS[MW], sZ[MW], sC[CW];
    const int tid = threadIdx.x;
    const int64_t n0 = (int64_t)blockIdx.x * TN, k0 = (int64_t)blockIdx.y * TK;
    const bool need_s = p.w_mode >= 2, need_z = (p.w_mode == 1 || p.w_mode >= 3) && !p.zero_is_scalar;
    float zs = 0.f;
    if constexpr (FMT == DQ_INT) {
        dq_stage_meta(p, n0, k0, sS, sZ, sC);
        if ((p.w_mode == 1 || p.w_mode >= 3) && p.zero_is_scalar) zs = load_as_float(p.zeros, 0, p.zeros_dt);
    } else {
        const int64_t b0 = k0 / G, nblk = p.K / G;
        for (int o = tid; o < NB * TN; o += 256) {
            const int jl = o / TN, nl = o % TN;
            const int64_t n = n0 + nl, j = b0 + jl;
            if (n >= p.N || j >= nblk) continue;
            sB[o] = ((const uint8_t*)p.scales)[j * p.stride_meta_g + n * p.stride_meta_n];
        }
    }
    __syncthreads();

    const int c = tid & 31;
    const int64_t k = k0 + c * 8;
    if (k >= p.K) return;
    const bool nibbles = FMT != DQ_INT && FMT != DQ_MXFP8 && p.e == 2;
    const int gl = FMT == DQ_INT ? (int)(k / p.group - k0 / p.group) : 0;
#pragma unroll 2
    for (int it = 0; it < 8; ++it) {
        const int r = it * 8 + (tid >> 5);
        const int64_t n = n0 + r;
        if (n >= p.N) break;
        const uint8_t* src = (const uint8_t*)p.w + n * p.stride_wn;
        float q[8];
        if (nibbles) {
            const uint32_t v = *(const uint32_t*)(src + (k >> 1));
#pragma unroll
            for (int i = 0; i < 8; ++i) q[i] = dq_e2m1(v >> (4 * i));
        } else {
            const u32x2 v = *(const u32x2*)(src + k);
            if constexpr (FMT == DQ_MXFP4 || FMT == DQ_NVFP4) {
#pragma unroll
                for (int i = 0; i < 8; ++i) q[i] = dq_e2m1(v[i >> 2] >> (8 * (i & 3)));
            } else {
                const int dt = FMT == DQ_MXFP8 ? (int)GEMLITE_DT_FP8E4 : p.w_dt;
                dq_bytes4(v[0], dt, q);
                dq_bytes4(v[1], dt, q + 4);
            }
        }
        float d[8];
        if constexpr (FMT == DQ_INT) {
            const float s = need_s ? sS[gl * PITCH + r] : 1.f;
            const float z = need_z ? sZ[gl * PITCH + r] : zs;
            const float cs = p.chan ? sC[r] : 1.f;
#pragma unroll
            for (int i = 0; i < 8; ++i) d[i] = dq_finish(dequant_f32(q[i], s, z, p.w_mode), p.chan != 0, cs, p.post);
        } else {
            const uint32_t b = sB[((c * 8) / G) * TN + r];
            const float s = FMT == DQ_NVFP4 ? fp8e4m3_to_float((uint8_t)b) : dq_e8m0(b);
#pragma unroll
            for (int i = 0; i < 8; ++i) d[i] = dq_finish(q[i] * s, false, 1.f, p.post);
        }
        dq_store8(p, n, k, d);
    }
}

__device__ __forceinline__ uint32_t dq_load_word(const void* w, int64_t idx, int pack_bits) {
    switch (pack_bits) {
        case 8: return ((const uint8_t*)w)[idx];
        case 16: return ((const uint16_t*)w)[idx];
        default: return ((const uint32_t*)w)[idx];
    }
}

__global__ __launch_bounds__(256) void dequantize_any_kernel(const DequantParams p) {
    const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (idx >= p.N * p.K) return;
    const int64_t n = idx / p.K, k = idx - n * p.K;
    float d;
    if (p.fmt != DQ_INT) {
        float q;
        if (p.fmt == DQ_MXFP8) {
            q = fp8e4m3_to_float(((const uint8_t*)p.w)[k * p.stride_wk + n * p.stride_wn]);
        } else if (p.e == 2) {
            q = dq_e2m1((uint32_t)((const uint8_t*)p.w)[(k >> 1) * p.stride_wk + n * p.stride_wn] >> (4 * (int)(k & 1)));
        } else {
            q = dq_e2m1(((const uint8_t*)p.w)[k * p.stride_wk + n * p.stride_wn]);
        }
        const uint8_t b = ((const uint8_t*)p.scales)[(k / p.group) * p.stride_meta_g + n * p.stride_meta_n];
        d = dq_finish(q * (p.fmt == DQ_NVFP4 ? fp8e4m3_to_float(b) : dq_e8m0(b)), false, 1.f, p.post);
    } else {
        float q;
        if (p.e > 1) {
            const int64_t j = k / p.e;
            const int sh = (int)(k - j * p.e) * p.nbits;
            q = (float)((dq_load_word(p.w, j * p.stride_wk + n * p.stride_wn, p.pack_bits) >> sh) & ((1u << p.nbits) - 1u));
        } else {
            q = load_as_float(p.w, k * p.stride_wk + n * p.stride_wn, p.w_dt);
        }
        const bool need_s = p.w_mode >= 2, need_z = p.w_mode == 1 || p.w_mode >= 3;
        const int64_t midx = (k / p.group) * p.stride_meta_g + n * p.stride_meta_n;
        const float s = need_s ? load_as_float(p.scales, midx, p.meta_dt) : 1.f;
        const float z = need_z ? load_as_float(p.zeros, p.zero_is_scalar ? 0 : midx, p.zeros_dt) : 0.f;
        const float cs = p.chan ? load_as_float(p.scales, n * p.stride_meta_n, p.meta_dt) : 1.f;
        d = dq_finish(dequant_f32(q, s, z, p.w_mode), p.chan != 0, cs, p.post);
    }
    store_from_float(p.out, n * p.ld_out + k, p.out_dt, d);
}

const void* dequantize_words_kernel_fn(int nbits) {
    switch (nbits) {
        case 8: return (const void*)dequantize_words_kernel<8>;
        case 4: return (const void*)dequantize_words_kernel<4>;
        case 2: return (const void*)dequantize_words_kernel<2>;
        default: return (const void*)dequantize_words_kernel<1>;
    }
}
const void* dequantize_rows_kernel_fn(int fmt) {
    switch (fmt) {
        case DQ_MXFP8: return (const void*)dequantize_rows_kernel<DQ_MXFP8>;
        case DQ_MXFP4: return (const void*)dequantize_rows_kernel<DQ_MXFP4>;
        case DQ_NVFP4: return (const void*)dequantize_rows_kernel<DQ_NVFP4>;
        default: return (const void*)dequantize_rows_kernel<DQ_INT>;
    }
}
const void* dequantize_any_kernel_fn() { return (const void*)dequantize_any_kernel; }

}  // namespace gl
