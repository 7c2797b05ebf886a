// quantize_groups.hip — float weights [N, K] -> grouped asymmetric INT codes + (scale, zero) per (row n, group of g k), round to nearest on
// the min / max of the group (DESIGN §2.1 has the contract; tests/quant_int_spec.py restates it in torch):
//     s = (hi - lo) / qmax, s < 2^-14 -> 1;  s_r = rT(s);  z_r = rT(-lo / s_r);  q = clamp(rint(w / s_r + z_r), 0, qmax)
// every step ONE fp32 IEEE operation (correctly rounded divisions, no multiply-add pair: nothing here can contract), rT = round to the 16-bit
// metadata type and back.  One launch per matrix, no workspace, no atomics.
//
// A block owns 64 rows (n) x one SPAN of k = lcm(g, 256): whole groups only, at most 8 of them per row.
//   g | 256   the span is one 64 x 256 tile.  A thread takes 8 consecutive k (16 bytes of a 16-bit input), consecutive lanes along k; the
//             g / 8 lanes of a group are neighbours inside half a wave and join their min / max by xor shuffles: the weights are read once.
//   else      (96, 192, 512, ..., channel-wise g = K): a wave per (row, group) first reduces the group over the span and leaves (s_r, z_r) in
//             LDS; the span is then walked tile by tile — a second read of the same bytes inside the launch, from L2 while 64 rows x span fit.
// Codes leave either as uint8 [N][K] straight from the registers (pack32 = 0: 8 bytes per lane along k) or, for pack32, through the LDS turn of
// pack_over_cols32_kernel (row pitch 260 bytes) as words [K / e][N] with consecutive lanes along n.  The metadata is staged in LDS and leaves
// with consecutive lanes along n through the caller's element strides: [K/g, N] (the layer) and [N * K/g, 1] (HQQ's meta) are the same code.
#include "gl_common.h"

namespace gl {

__device__ __forceinline__ float qg_round_meta(float v, bool f16) {
    return f16 ? F16Traits<half_tag>::to_float(F16Traits<half_tag>::from_float(v)) : F16Traits<bf16_tag>::to_float(F16Traits<bf16_tag>::from_float(v));
}

// 8 consecutive weights of row n from k (k % 8 == 0) as fp32
__device__ __forceinline__ void qg_load8(const QuantGroupsParams& p, bool vec, int64_t n, int64_t k, float (&v)[8]) {
    load8_as_float(p.w, p.w_dt, p.ld_w, vec, n, k, v);
}

// (lo, hi) of a group -> the rounded scale and zero the layer will dequantise with
__device__ __forceinline__ void qg_group_meta(float lo, float hi, float qmax, bool f16, float& s_r, float& z_r) {
    float s = __fdiv_rn(hi - lo, qmax);
    if (s < 6.103515625e-05f) s = 1.f;  // 2^-14: a constant group, or a range fp16 cannot carry
    s_r = qg_round_meta(s, f16);
    z_r = qg_round_meta(__fdiv_rn(-lo, s_r), f16);
}

template <bool ONEPASS>
__global__ __launch_bounds__(256) void quantize_groups_kernel(const QuantGroupsParams p) {
    constexpr int TN = 64, TK = 256, PITCH = 260, MAXG = 8;
    __shared__ __attribute__((aligned(16))) unsigned char tile[TN * PITCH];
    __shared__ float sS[MAXG * TN], sZ[MAXG * TN];  // (s_r, z_r) of the span's groups, [group][row]
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int64_t n0 = (int64_t)blockIdx.x * TN, ks0 = (int64_t)blockIdx.y * p.span;
    const int64_t klen = (p.K - ks0) < p.span ? (p.K - ks0) : p.span;  // K % g == 0: whole groups
    const int g = p.group, ng = (int)(klen / g);
    const bool f16 = p.meta_dt == GEMLITE_DT_FP16;
    const float qmax = (float)((1 << p.nbits) - 1);
    const int esz = p.w_dt == GEMLITE_DT_FP32 ? 4 : 2;
    const bool vec = (((uintptr_t)p.w) % 16 == 0) && ((p.ld_w * esz) % 16 == 0);

    if constexpr (!ONEPASS) {
        for (int pr = wave; pr < ng * TN; pr += 4) {
            const int gl = pr % ng, r = pr / ng;
            const int64_t n = n0 + r;
            float lo = 0.f, hi = 0.f;
            if (n < p.N) {
                lo = __builtin_inff();
                hi = -__builtin_inff();
                for (int kk = lane * 8; kk < g; kk += 512) {
                    float v[8];
                    qg_load8(p, vec, n, ks0 + (int64_t)gl * g + kk, v);
#pragma unroll
                    for (int e = 0; e < 8; ++e) {
                        lo = fminf(lo, v[e]);
                        hi = fmaxf(hi, v[e]);
                    }
                }
            }
#pragma unroll
            for (int off = 32; off >= 1; off >>= 1) {
                lo = fminf(lo, __shfl_xor(lo, off));
                hi = fmaxf(hi, __shfl_xor(hi, off));
            }
            if (lane == 0) {
                float s_r, z_r;
                qg_group_meta(lo, hi, qmax, f16, s_r, z_r);
                sS[gl * TN + r] = s_r;
                sZ[gl * TN + r] = z_r;
            }
        }
        __syncthreads();
    }

    const int ntiles = (int)((klen + TK - 1) / TK);
    const int e = 32 / p.nbits;
    for (int t = 0; t < ntiles; ++t) {
        const int64_t kt = (int64_t)t * TK;  // offset of the tile inside the span
#pragma unroll 1
        for (int it = 0; it < 8; ++it) {
            const int r = it * 8 + (tid >> 5), c = tid & 31;
            const int64_t n = n0 + r, kl = kt + c * 8;
            const bool valid = n < p.N && kl < klen;  // (K % 8 == 0: a piece of 8 is inside K or outside)
            float v[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
            if (valid) qg_load8(p, vec, n, ks0 + kl, v);
            float s_r, z_r;
            if constexpr (ONEPASS) {
                float lo = v[0], hi = v[0];
#pragma unroll
                for (int i = 1; i < 8; ++i) {
                    lo = fminf(lo, v[i]);
                    hi = fmaxf(hi, v[i]);
                }
                for (int off = 1; off < (g >> 3); off <<= 1) {  // the g / 8 lanes of a group: neighbours inside half a wave
                    lo = fminf(lo, __shfl_xor(lo, off));
                    hi = fmaxf(hi, __shfl_xor(hi, off));
                }
                qg_group_meta(lo, hi, qmax, f16, s_r, z_r);
                if (valid && (c * 8) % g == 0) {
                    sS[((c * 8) / g) * TN + r] = s_r;
                    sZ[((c * 8) / g) * TN + r] = z_r;
                }
            } else {
                const int gl = valid ? (int)(kl / g) : 0;
                s_r = sS[gl * TN + r];
                z_r = sZ[gl * TN + r];
            }
            uint32_t d[2] = {0u, 0u};
#pragma unroll
            for (int i = 0; i < 8; ++i) {
                const float q = fminf(fmaxf(rintf(__fdiv_rn(v[i], s_r) + z_r), 0.f), qmax);
                d[i >> 2] |= (uint32_t)q << (8 * (i & 3));
            }
            if (p.pack32) {
                uint32_t* dst = (uint32_t*)(tile + r * PITCH + c * 8);  // (PITCH % 4 == 0: dword stores)
                dst[0] = d[0];
                dst[1] = d[1];
            } else if (valid) {
                uint8_t* dst = (uint8_t*)p.q_out + n * p.ld_q + ks0 + kl;
                if ((((uintptr_t)p.q_out) % 8 == 0) && (p.ld_q % 8 == 0)) {
                    *(u32x2*)dst = (u32x2){d[0], d[1]};
                } else {
#pragma unroll
                    for (int i = 0; i < 8; ++i) dst[i] = (uint8_t)(d[i >> 2] >> (8 * (i & 3)));
                }
            }
        }
        __syncthreads();
        if (p.pack32) {
            const int wpt = TK / e;  // words per row in this tile
            for (int o = tid; o < wpt * TN; o += 256) {
                const int jl = o / TN, nl = o % TN;
                const int64_t n = n0 + nl, kl = kt + (int64_t)jl * e;
                if (n >= p.N || kl >= klen) continue;
                const unsigned char* src = tile + nl * PITCH + jl * e;
                uint32_t word = 0;
                for (int i = 0; i < e; i += 4) {
                    const uint32_t q = *(const uint32_t*)(src + i);
                    word |= ((q & 0xFFu) << (p.nbits * i)) | (((q >> 8) & 0xFFu) << (p.nbits * (i + 1))) |
                            (((q >> 16) & 0xFFu) << (p.nbits * (i + 2))) | ((q >> 24) << (p.nbits * (i + 3)));
                }
                ((uint32_t*)p.q_out)[((ks0 + kl) / e) * p.N + n] = word;
            }
            __syncthreads();
        }
    }

    // the span's metadata: consecutive lanes along n
    const int64_t g0 = ks0 / g;
    for (int o = tid; o < ng * TN; o += 256) {
        const int gl = o / TN, nl = o % TN;
        const int64_t n = n0 + nl;
        if (n >= p.N) continue;
        const float s_r = sS[gl * TN + nl], z_r = sZ[gl * TN + nl];
        const float zz = p.fold ? qg_round_meta(-z_r * s_r, f16) : z_r;  // what pack() stores for W_group_mode 4
        const int64_t idx = (g0 + gl) * p.stride_meta_g + n * p.stride_meta_n;
        ((uint16_t*)p.scales)[idx] = f16 ? F16Traits<half_tag>::from_float(s_r) : F16Traits<bf16_tag>::from_float(s_r);
        ((uint16_t*)p.zeros)[idx] = f16 ? F16Traits<half_tag>::from_float(zz) : F16Traits<bf16_tag>::from_float(zz);
    }
}

const void* quantize_groups_kernel_fn(bool onepass) {
    return onepass ? (const void*)quantize_groups_kernel<true> : (const void*)quantize_groups_kernel<false>;
}

}  // namespace gl
