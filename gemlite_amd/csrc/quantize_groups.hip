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
//
// quantize_hqq_kernel is the same block with one more step between a group's (s_r, z_r) and its codes: HQQ's proximal iteration on the ZERO
// (DESIGN §2.1a has the contract; tests/quant_hqq_spec.py restates it).  The scale stays s_r; every candidate zero is judged by the error of
// what the layer will compute with the ROUNDED zero, per group, and the best one seen is kept, so no group ends worse than round to nearest.
//   g | 256   a lane keeps its 8 weights and their quotients w / s_r in registers for the whole loop; the g / 8 lanes of a group join the two
//             sums of an iteration (the new zero, its error) by xor shuffles, all of them ending with the same bits.  Groups of a wave stop at
//             different iterations: state updates are masked per lane, the loop ends when no group of the wave is alive.
//   else      the wave that reduces a (row, group) also iterates on it: g <= 512 from 8 registers per lane, longer groups by walking the group
//             again per sum (L2 hits while 64 rows x span fit); the fp32 terms of a sum are added in fp64 here.
// The order of every sum is fixed by the lane layout alone: 8 values per lane in k order (per 512-k chunk in the wave form), then the butterfly.
#include "gl_common.h"
#include "gl_host.h"

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

// ------------------------------------------------------------------------------------------------ HQQ's iteration on the zero
// Every step below is ONE fp32 operation written so that it cannot contract, but the power (one v_log_f32 / v_exp_f32 pair).
// ws = w / s_r is the quotient the codes are taken from; E is compared as the SUM over the group (the mean times g, in one fixed order).
__device__ __forceinline__ float hqq_code(float ws, float z, float qmax) { return fminf(fmaxf(rintf(ws + z), 0.f), qmax); }

// |w - (Q(z_r) - z_r) s_r|: one term of E(z), z_r the rounded zero
__device__ __forceinline__ float hqq_err_term(float w, float ws, float z_r, float s_r, float qmax) {
    const float q = hqq_code(ws, z_r, qmax);
    return fabsf(__fsub_rn(w, __fmul_rn(__fsub_rn(q, z_r), s_r)));
}

// q - (w - e) / s_r, taken as (q - w / s_r) + e * (1 / s_r): one term of the next zero.  pm1 = lp_norm - 1, rb = 1 / beta_i.
// r == 0: log2 -> -inf, the power -> +inf, the shrunk magnitude -> max(-inf, 0) = 0, so e = 0 without a branch.
__device__ __forceinline__ float hqq_step_term(float w, float ws, float z, float s_r, float inv_s, float qmax, float pm1, float rb) {
    const float q = hqq_code(ws, z, qmax);
    const float r = __fsub_rn(w, __fmul_rn(__fsub_rn(q, z), s_r));
    const float a = fabsf(r);
    const float pw = pm1 == 0.f ? 1.f : __builtin_amdgcn_exp2f(__fmul_rn(pm1, __builtin_amdgcn_logf(a)));
    const float e = copysignf(fmaxf(__fsub_rn(a, __fmul_rn(pw, rb)), 0.f), r);
    return __fadd_rn(__fsub_rn(q, ws), __fmul_rn(e, inv_s));
}

// g | 256: the group's `lanes` = g / 8 neighbouring lanes each hold 8 weights.  Returns rT(best zero); h.iters == 0 returns z_r as it came.
__device__ __forceinline__ float hqq_refine_lanes(const QuantHqqParams& h, const float (&v)[8], int g, float lo, float s_r, float z_r, float qmax,
                                                  bool f16) {
    const int lanes = g >> 3;
    auto group_sum = [lanes](float x) {  // xor butterfly: a + b and b + a are the same bits, so every lane of the group ends with the same sum
#pragma unroll
        for (int off = 1; off < 32; off <<= 1)
            if (off < lanes) x = __fadd_rn(x, __shfl_xor(x, off));
        return x;
    };
    const float inv_s = __fdiv_rn(1.f, s_r), gf = (float)g, pm1 = h.lp_norm - 1.f;
    float ws[8], acc = 0.f;
#pragma unroll
    for (int e = 0; e < 8; ++e) {
        ws[e] = __fdiv_rn(v[e], s_r);
        acc = __fadd_rn(acc, hqq_err_term(v[e], ws[e], z_r, s_r, qmax));
    }
    float best_E = group_sum(acc), z = __fdiv_rn(-lo, s_r), best_z = z, b = h.beta;
    bool alive = true;
    for (int i = 0; i < h.iters; ++i) {
        if (!__any(alive)) break;  // the lanes of a stopped group go on computing (and exchanging among themselves); nothing of it is kept
        const float rb = __fdiv_rn(1.f, b);
        acc = 0.f;
#pragma unroll
        for (int e = 0; e < 8; ++e) acc = __fadd_rn(acc, hqq_step_term(v[e], ws[e], z, s_r, inv_s, qmax, pm1, rb));
        const float zn = __fdiv_rn(group_sum(acc), gf), zn_r = qg_round_meta(zn, f16);
        acc = 0.f;
#pragma unroll
        for (int e = 0; e < 8; ++e) acc = __fadd_rn(acc, hqq_err_term(v[e], ws[e], zn_r, s_r, qmax));
        const float E = group_sum(acc);
        if (alive) {
            if (E < best_E) {  // (false for NaN: a group with a non-finite weight stops here)
                best_E = E;
                best_z = z = zn;
            } else {
                alive = false;
            }
        }
        b = __fmul_rn(b, h.kappa);
    }
    return qg_round_meta(best_z, f16);
}

// one sum of the wave form over the group [k0, k0 + g) of row n: lane l takes k0 + 8 l + 512 j, j = 0, 1, ... in order, then the butterfly.
// STEP: terms of the next zero, else terms of E.  inreg (g <= 512): the lane's only chunk is vr (zeros where 8 l >= g: never read).
// The fp32 terms are ADDED in fp64: one step of a 16-bit zero moves the sum of thousands of terms by less than fp32 resolves, and a
// channel-wise group would stop on rounding noise.
template <bool STEP>
__device__ __forceinline__ double hqq_wave_sum(const QuantGroupsParams& p, bool vec, int64_t n, int64_t k0, int g, int lane, bool inreg,
                                              const float (&vr)[8], float z, float s_r, float inv_s, float qmax, float pm1, float rb) {
    double acc = 0.0;
    for (int kk = lane * 8; kk < g; kk += 512) {
        float v[8];
        if (inreg) {
#pragma unroll
            for (int e = 0; e < 8; ++e) v[e] = vr[e];
        } else {
            qg_load8(p, vec, n, k0 + kk, v);
        }
#pragma unroll
        for (int e = 0; e < 8; ++e) {
            const float ws = __fdiv_rn(v[e], s_r);
            acc += (double)(STEP ? hqq_step_term(v[e], ws, z, s_r, inv_s, qmax, pm1, rb) : hqq_err_term(v[e], ws, z, s_r, qmax));
        }
    }
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) acc += __shfl_xor(acc, off);
    return acc;
}

// every other group size: the whole wave owns the group (n < N: the caller checks, wave-uniform)
__device__ __forceinline__ float hqq_refine_wave(const QuantGroupsParams& p, const QuantHqqParams& h, bool vec, int64_t n, int64_t k0, int g, int lane,
                                                 float lo, float s_r, float z_r, float qmax, bool f16) {
    const bool inreg = g <= 512;
    float vr[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    if (inreg && lane * 8 < g) qg_load8(p, vec, n, k0 + lane * 8, vr);
    const float inv_s = __fdiv_rn(1.f, s_r), pm1 = h.lp_norm - 1.f;
    double best_E = hqq_wave_sum<false>(p, vec, n, k0, g, lane, inreg, vr, z_r, s_r, inv_s, qmax, pm1, 0.f);
    float z = __fdiv_rn(-lo, s_r), best_z = z, b = h.beta;
    for (int i = 0; i < h.iters; ++i) {
        const float rb = __fdiv_rn(1.f, b);
        const float zn = (float)(hqq_wave_sum<true>(p, vec, n, k0, g, lane, inreg, vr, z, s_r, inv_s, qmax, pm1, rb) / (double)g);
        const double E = hqq_wave_sum<false>(p, vec, n, k0, g, lane, inreg, vr, qg_round_meta(zn, f16), s_r, inv_s, qmax, pm1, 0.f);
        if (!(E < best_E)) break;  // the same bits in every lane: the wave stops as one
        best_E = E;
        best_z = z = zn;
        b = __fmul_rn(b, h.kappa);
    }
    return qg_round_meta(best_z, f16);
}

template <bool ONEPASS, bool HQQ>
__device__ __forceinline__ void quantize_groups_body(const QuantGroupsParams& p, const QuantHqqParams& h) {
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
            float s_r, z_r;
            qg_group_meta(lo, hi, qmax, f16, s_r, z_r);  // (every lane holds the same lo, hi)
            if constexpr (HQQ) {
                if (n < p.N) z_r = hqq_refine_wave(p, h, vec, n, ks0 + (int64_t)gl * g, g, lane, lo, s_r, z_r, qmax, f16);
            }
            if (lane == 0) {
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
                if constexpr (HQQ) z_r = hqq_refine_lanes(h, v, g, lo, s_r, z_r, qmax, f16);
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

template <bool ONEPASS>
__global__ __launch_bounds__(256) void quantize_groups_kernel(const QuantGroupsParams p) {
    quantize_groups_body<ONEPASS, false>(p, QuantHqqParams{});
}

template <bool ONEPASS>
__global__ __launch_bounds__(256) void quantize_hqq_kernel(const QuantGroupsParams p, const QuantHqqParams h) {
    quantize_groups_body<ONEPASS, true>(p, h);
}

const void* quantize_hqq_kernel_fn(bool onepass) {
    return onepass ? (const void*)quantize_hqq_kernel<true> : (const void*)quantize_hqq_kernel<false>;
}

const void* quantize_groups_kernel_fn(bool onepass) {
    return onepass ? (const void*)quantize_groups_kernel<true> : (const void*)quantize_groups_kernel<false>;
}

}  // namespace gl
