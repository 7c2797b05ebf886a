// quantize_mx.hip — float weights [N, K] -> block-scaled elements + one scale byte per block (DESIGN §2.2 has the contract;
// tests/quant_mx_spec.py restates it in torch).  FORMAT 0: MXFP8 (e4m3 elements, e8m0 scale per 32 k), 1: MXFP4 (e2m1 codes, e8m0 per 32 k),
// 2: NVFP4 (e2m1 codes, e4m3 scale per 16 k on top of the fixed meta scale 0.05).  amax = max |w| of the block; every step ONE fp32 IEEE
// operation (correctly rounded divisions, no multiply-add pair: nothing here can contract):
//   MX:  ideal = amax / qmax (448.f / 6.f);  ex = exponent_field(ideal) + (mantissa != 0), clamped to [97, 254];  byte = ex, s = 2^(ex - 127)
//        fp8:  e4m3_rne(clamp(w / s, -448, 448));   fp4:  q = w / s
//   NV:  t = (amax / 6.f) / 0.05f;  s8 = e4m3_rne(min(t, 448));  full = max(float(s8) * 0.05f, 1e-6f);  q = w / full
//   fp4 code: c = #{0.25, 0.75, 1.25, 1.75, 2.5, 3.5, 5.0 strictly below |q|}; c + 8 if q < 0 and c > 0, else c.  This is the WEIGHT rule
//        (the reference's round_to_closest_fp4 + to_index): seven thresholds, and a negative weight that rounds to zero is code 0 — not
//        mx_quant_block's activation rule (eight thresholds, sign kept on zero).
// A block that holds a NaN or an Inf gets the scale format's NaN code (e8m0 0xFF, e4m3 0x7F), like the activation quantisers; its element
// bytes are whatever the arithmetic above leaves.  One launch per matrix, no workspace, no atomics.
//
// A block owns 64 rows (n) x 256 k, as quantize_groups.hip does.  A thread takes 8 consecutive k (16 bytes of a 16-bit input), consecutive
// lanes along k; the 4 lanes of a block of 32 (2 lanes for NVFP4) are neighbours and join amax by xor shuffles (on the bits of |w|: a NaN
// survives the join).  The weights are read once and the elements leave straight from the registers, row-major: 8 bytes per lane (e4m3, or
// one code per byte) or 4 bytes (two codes per byte, even k in the low nibble).  Only the scale bytes are transposed: the tile's 64 x 8
// (64 x 16) bytes are staged in LDS and leave with consecutive lanes along n through the caller's strides: [K/g, N] (the layer) and
// [N * K/g, 1] (the quantiser's return) are the same code.  K % 32 == 0, so a piece of 8 k, and a whole block with it, is inside K or
// outside: lanes beyond N or K only ever shuffle with each other and store nothing.
#include "gl_common.h"
#include "gl_host.h"

namespace gl {

// weight rule (see above); NaN compares false everywhere: code 0
__device__ __forceinline__ uint32_t qmx_fp4_code(float q) {
    const float a = fabsf(q);
    const uint32_t c = (a > 0.25f) + (a > 0.75f) + (a > 1.25f) + (a > 1.75f) + (a > 2.5f) + (a > 3.5f) + (a > 5.0f);
    return (q < 0.f && c > 0u) ? c + 8u : c;
}

template <int FORMAT>
__global__ __launch_bounds__(256) void quantize_mx_kernel(const QuantMxParams p) {
    constexpr int TN = 64, TK = 256, G = FORMAT == 2 ? 16 : 32, NB = TK / G, LPB = G / 8;  // lanes per block of G k
    __shared__ uint8_t sS[NB * TN];  // scale bytes of the tile, [block][row]
    const int tid = threadIdx.x;
    const int64_t n0 = (int64_t)blockIdx.x * TN, k0 = (int64_t)blockIdx.y * TK;
    const int esz = p.w_dt == GEMLITE_DT_FP32 ? 4 : 2;
    const bool vec = (((uintptr_t)p.w) % 16 == 0) && ((p.ld_w * esz) % 16 == 0);
    const bool vec_q8 = (((uintptr_t)p.q_out) % 8 == 0) && (p.ld_q % 8 == 0);
    const bool vec_q4 = (((uintptr_t)p.q_out) % 4 == 0) && (p.ld_q % 4 == 0);
    const int c = tid & 31;
    const int64_t k = k0 + c * 8;

#pragma unroll 1
    for (int it2 = 0; it2 < 4; ++it2) {
        float v[2][8];
        bool valid[2];
#pragma unroll
        for (int h = 0; h < 2; ++h) {  // both loads in flight before either is used
            const int64_t n = n0 + (it2 * 2 + h) * 8 + (tid >> 5);
            valid[h] = n < p.N && k < p.K;
#pragma unroll
            for (int e = 0; e < 8; ++e) v[h][e] = 0.f;
            if (valid[h]) load8_as_float(p.w, p.w_dt, p.ld_w, vec, n, k, v[h]);
        }
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            const int r = (it2 * 2 + h) * 8 + (tid >> 5);
            const int64_t n = n0 + r;
            float amax = 0.f;
#pragma unroll
            for (int e = 0; e < 8; ++e) amax = absmax_keep_nan(amax, v[h][e]);
#pragma unroll
            for (int off = 1; off < LPB; off <<= 1) amax = absmax_keep_nan(amax, __shfl_xor(amax, off));

            uint8_t sb;
            float s, rinv = 1.f;
            bool use_mul = false;
            if constexpr (FORMAT == 2) {
                const float t = fminf(__fdiv_rn(__fdiv_rn(amax, 6.f), 0.05f), 448.f);
                sb = amax_not_finite(amax) ? (uint8_t)0x7F : float_to_fp8e4m3(t);
                s = fmaxf(fp8e4m3_to_float(sb) * 0.05f, 1e-6f);
            } else {
                const uint32_t xi = __builtin_bit_cast(uint32_t, __fdiv_rn(amax, FORMAT == 0 ? 448.f : 6.f));
                int ex = (int)((xi >> 23) & 0xFFu) + ((xi & 0x7FFFFFu) != 0u ? 1 : 0);
                ex = ex > 254 ? 254 : (ex < 97 ? 97 : ex);
                sb = amax_not_finite(amax) ? (uint8_t)0xFF : (uint8_t)ex;
                s = __builtin_bit_cast(float, (uint32_t)ex << 23);
                // w / 2^k == w * 2^-k bit for bit (one exact real value, one rounding) whenever 2^-k is a normal float: ex <= 253
                rinv = __builtin_bit_cast(float, (uint32_t)(254 - (ex > 253 ? 253 : ex)) << 23);
                use_mul = ex <= 253;
            }
            if (valid[h] && (c % LPB) == 0) sS[(c / LPB) * TN + r] = sb;

            uint32_t d[2] = {0u, 0u};
            if constexpr (FORMAT == 0) {
                float q[8];
#pragma unroll
                for (int e = 0; e < 8; ++e) q[e] = fminf(fmaxf(use_mul ? v[h][e] * rinv : __fdiv_rn(v[h][e], s), -448.f), 448.f);
#pragma unroll
                for (int w = 0; w < 2; ++w) {  // hardware e4m3 converter: round to nearest even, subnormals kept; the clamp keeps it from overflow
                    int pk = __builtin_amdgcn_cvt_pk_fp8_f32(q[4 * w], q[4 * w + 1], 0, false);
                    pk = __builtin_amdgcn_cvt_pk_fp8_f32(q[4 * w + 2], q[4 * w + 3], pk, true);
                    d[w] = (uint32_t)pk;
                }
            } else {
#pragma unroll
                for (int e = 0; e < 8; ++e) {
                    const uint32_t code = qmx_fp4_code(use_mul ? v[h][e] * rinv : __fdiv_rn(v[h][e], s));
                    d[e >> 2] |= code << (8 * (e & 3));
                }
            }
            if (!valid[h]) continue;
            if (FORMAT != 0 && p.pack) {  // two codes per byte: k even in the low nibble
                const uint32_t lo = d[0] | (d[0] >> 4), hi = d[1] | (d[1] >> 4);  // bytes 0 and 2 of each hold a packed pair
                const uint32_t word = (lo & 0xFFu) | ((lo >> 8) & 0xFF00u) | ((hi & 0xFFu) << 16) | ((hi << 8) & 0xFF000000u);
                uint8_t* dst = p.q_out + n * p.ld_q + (k >> 1);
                if (vec_q4) {
                    *(uint32_t*)dst = word;
                } else {
#pragma unroll
                    for (int i = 0; i < 4; ++i) dst[i] = (uint8_t)(word >> (8 * i));
                }
            } else {
                uint8_t* dst = p.q_out + n * p.ld_q + k;
                if (vec_q8) {
                    *(u32x2*)dst = (u32x2){d[0], d[1]};
                } else {
#pragma unroll
                    for (int i = 0; i < 8; ++i) dst[i] = (uint8_t)(d[i >> 2] >> (8 * (i & 3)));
                }
            }
        }
    }
    __syncthreads();

    // the tile's scale bytes: consecutive lanes along n
    const int64_t j0 = k0 / G, nblk = p.K / G;
    for (int o = tid; o < NB * TN; o += 256) {
        const int jl = o / TN, nl = o % TN;
        const int64_t n = n0 + nl, j = j0 + jl;
        if (n >= p.N || j >= nblk) continue;
        p.scales[j * p.stride_scale_g + n * p.stride_scale_n] = sS[o];
    }
}

const void* quantize_mx_kernel_fn(int format) {
    return format == 0 ? (const void*)quantize_mx_kernel<0> : (format == 1 ? (const void*)quantize_mx_kernel<1> : (const void*)quantize_mx_kernel<2>);
}

}  // namespace gl
