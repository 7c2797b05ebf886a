// quantize_rows.hip — float weights [N, K] -> channel-wise symmetric 8-bit codes (int8 / e4m3fn / e5m2) [N, K] + one scale per row: the
// tensors an A16W8 / A8W8 layer holds (DESIGN §2.4 has the contract; tests/quant_rows_spec.py restates it in torch).  Per row n, every
// step ONE fp32 IEEE operation (correctly rounded divisions, no multiply-add pair: nothing here can contract; denormals kept):
//   amax = max_k |w[n, k]|                                   (on the bits of |w|: a NaN survives, Inf < NaN)
//   rule 0: s = amax / qmax     rule 1: s = amax * (1.0f / qmax)            qmax = 127.f | 448.f | 57344.f
//   s = s < 1e-6f ? 1e-6f : s                                (a NaN or Inf scale stays what it is)
//   q = min(max(w / s, qmin), qmax)                          qmin = -128.f | -448.f | -57344.f
//   FORMAT 0: int8(rint(q)), half to even;  1 / 2: the hardware e4m3 / e5m2 converter (round to nearest even, subnormals kept, -0 -> 0x80)
//   scales[n * stride_s] = s as fp32, or rounded once to fp16 / bf16; the codes always use the fp32 s
// A row that holds a NaN or an Inf gets that non-finite scale; its codes are whatever the arithmetic above leaves (written, no fault).
// One launch per matrix, no workspace, no atomics, 64-bit addresses.
//
// Three forms, by K (the limits are GEMLITE_QUANT_ROWS_WAVE_MAX_K / _RESIDENT_MAX_K of the header, in elements, for every input type):
//   wave form      K <= 1024: one 64-lane wave per row, four rows per 256-thread block; the row sits in registers (R = 1 or 2 pieces of 8
//                  per lane), amax joins by xor shuffles, no LDS, no barrier.
//   resident form  K <= 16384: one 256-thread block per row; a thread loads R = 1 / 2 / 4 / 8 pieces of 8 consecutive k (16 bytes of a
//                  16-bit input, all in flight at once) and keeps them as floats across the reduction: lanes first, then the four wave
//                  partials through LDS.  The weight is read once.
//   re-read form   longer rows: one block per row, the same pieces in two passes; the second pass finds the row in L2.
// A piece leaves as one 8-byte store.  A `w` / row pitch that is not 16-byte aligned, a `q_out` / ld_q that is not 8-byte aligned and the
// last piece of a K that is no multiple of 8 take element loads / byte stores, each guarded by k < K: nothing outside the windows is touched.
#include "gl_common.h"
#include "gl_host.h"

namespace gl {

// 8 consecutive weights of a row from k as fp32; elements at or beyond K read as 0 (|0| never raises amax)
__device__ __forceinline__ void qr_load8(const QuantRowsParams& p, bool vec, int64_t n, int64_t k, float (&v)[8]) {
    if (k + 8 <= p.K) {
        load8_as_float(p.w, p.w_dt, p.ld_w, vec, n, k, v);
        return;
    }
#pragma unroll
    for (int e = 0; e < 8; ++e) v[e] = k + e < p.K ? load_as_float(p.w, n * p.ld_w + k + e, p.w_dt) : 0.f;
}

template <int FORMAT>
__device__ __forceinline__ float qr_scale(const QuantRowsParams& p, float amax) {
    constexpr float qmax = FORMAT == 0 ? 127.f : (FORMAT == 1 ? 448.f : 57344.f);
    constexpr float rq = 1.0f / qmax;  // the fp32 nearest to the reciprocal
    const float s = p.rule == 0 ? __fdiv_rn(amax, qmax) : amax * rq;
    return s < 1e-6f ? 1e-6f : s;  // false for NaN: a non-finite scale stays
}

// the 8 codes of a piece, and their store (8 bytes, or guarded bytes)
template <int FORMAT>
__device__ __forceinline__ void qr_store8(const QuantRowsParams& p, bool vec_q, int64_t n, int64_t k, const float (&v)[8], float s) {
    constexpr float qmin = FORMAT == 0 ? -128.f : (FORMAT == 1 ? -448.f : -57344.f);
    constexpr float qmax = FORMAT == 0 ? 127.f : (FORMAT == 1 ? 448.f : 57344.f);
    float q[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) q[e] = fminf(fmaxf(__fdiv_rn(v[e], s), qmin), qmax);  // (fmaxf drops a NaN: the converters below never see one)
    uint32_t d[2] = {0u, 0u};
    if constexpr (FORMAT == 0) {
#pragma unroll
        for (int e = 0; e < 8; ++e) d[e >> 2] |= (uint32_t)(uint8_t)(int8_t)(int)__builtin_rintf(q[e]) << (8 * (e & 3));
    } else {
#pragma unroll
        for (int h = 0; h < 2; ++h) {  // the clamp keeps the converters from overflow
            int w = 0;
            if constexpr (FORMAT == 1) {
                w = __builtin_amdgcn_cvt_pk_fp8_f32(q[4 * h], q[4 * h + 1], w, false);
                w = __builtin_amdgcn_cvt_pk_fp8_f32(q[4 * h + 2], q[4 * h + 3], w, true);
            } else {
                w = __builtin_amdgcn_cvt_pk_bf8_f32(q[4 * h], q[4 * h + 1], w, false);
                w = __builtin_amdgcn_cvt_pk_bf8_f32(q[4 * h + 2], q[4 * h + 3], w, true);
            }
            d[h] = (uint32_t)w;
        }
    }
    uint8_t* dst = p.q_out + n * p.ld_q + k;
    if (vec_q && k + 8 <= p.K) {
        *(u32x2*)dst = (u32x2){d[0], d[1]};
    } else {
#pragma unroll
        for (int e = 0; e < 8; ++e)
            if (k + e < p.K) dst[e] = (uint8_t)(d[e >> 2] >> (8 * (e & 3)));
    }
}

__device__ __forceinline__ float qr_wave_amax(float amax) {
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) amax = absmax_keep_nan(amax, __shfl_xor(amax, off));
    return amax;
}

// T = 64: wave form (row = 4 * block + wave);  T = 256: resident form (row = block).  The row is R pieces of 8 per thread, in registers.
template <int FORMAT, int T, int R>
__global__ __launch_bounds__(256) void quantize_rows_kernel(const QuantRowsParams p) {
    __shared__ float wmax[4];
    const int tid = threadIdx.x;
    const int lane = T == 64 ? (tid & 63) : tid;
    const int64_t n = T == 64 ? (int64_t)blockIdx.x * 4 + (tid >> 6) : (int64_t)blockIdx.x;
    if (T == 64 && n >= p.N) return;  // a whole wave: no barrier in this form
    const bool vec = (((uintptr_t)p.w) % 16 == 0) && ((p.ld_w * (p.w_dt == GEMLITE_DT_FP32 ? 4 : 2)) % 16 == 0);
    const bool vec_q = (((uintptr_t)p.q_out) % 8 == 0) && (p.ld_q % 8 == 0);

    float v[R][8];
#pragma unroll
    for (int r = 0; r < R; ++r) {  // every load in flight before the first is used
        const int64_t k = (int64_t)(r * T + lane) * 8;
#pragma unroll
        for (int e = 0; e < 8; ++e) v[r][e] = 0.f;
        if (k < p.K) qr_load8(p, vec, n, k, v[r]);
    }
    float amax = 0.f;
#pragma unroll
    for (int r = 0; r < R; ++r)
#pragma unroll
        for (int e = 0; e < 8; ++e) amax = absmax_keep_nan(amax, v[r][e]);
    amax = qr_wave_amax(amax);
    if constexpr (T == 256) {
        if ((tid & 63) == 0) wmax[tid >> 6] = amax;
        __syncthreads();
        amax = absmax_keep_nan(absmax_keep_nan(wmax[0], wmax[1]), absmax_keep_nan(wmax[2], wmax[3]));
    }
    const float s = qr_scale<FORMAT>(p, amax);
    if (lane == 0) store_from_float(p.scales, n * p.stride_s, p.scale_dt, s);
#pragma unroll
    for (int r = 0; r < R; ++r) {
        const int64_t k = (int64_t)(r * T + lane) * 8;
        if (k < p.K) qr_store8<FORMAT>(p, vec_q, n, k, v[r], s);
    }
}

// re-read form: any K, one block per row, four pieces in flight per thread
template <int FORMAT>
__global__ __launch_bounds__(256) void quantize_rows_reread_kernel(const QuantRowsParams p) {
    __shared__ float wmax[4];
    const int tid = threadIdx.x;
    const int64_t n = blockIdx.x;
    const bool vec = (((uintptr_t)p.w) % 16 == 0) && ((p.ld_w * (p.w_dt == GEMLITE_DT_FP32 ? 4 : 2)) % 16 == 0);
    const bool vec_q = (((uintptr_t)p.q_out) % 8 == 0) && (p.ld_q % 8 == 0);
    constexpr int U = 4;
    float amax = 0.f;
    for (int64_t k0 = (int64_t)tid * 8; k0 < p.K; k0 += (int64_t)U * 2048) {
        float v[U][8];
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const int64_t k = k0 + (int64_t)u * 2048;
#pragma unroll
            for (int e = 0; e < 8; ++e) v[u][e] = 0.f;
            if (k < p.K) qr_load8(p, vec, n, k, v[u]);
        }
#pragma unroll
        for (int u = 0; u < U; ++u)
#pragma unroll
            for (int e = 0; e < 8; ++e) amax = absmax_keep_nan(amax, v[u][e]);
    }
    amax = qr_wave_amax(amax);
    if ((tid & 63) == 0) wmax[tid >> 6] = amax;
    __syncthreads();
    amax = absmax_keep_nan(absmax_keep_nan(wmax[0], wmax[1]), absmax_keep_nan(wmax[2], wmax[3]));
    const float s = qr_scale<FORMAT>(p, amax);
    if (tid == 0) store_from_float(p.scales, n * p.stride_s, p.scale_dt, s);
    for (int64_t k0 = (int64_t)tid * 8; k0 < p.K; k0 += (int64_t)U * 2048) {
        float v[U][8];
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const int64_t k = k0 + (int64_t)u * 2048;
            if (k < p.K) qr_load8(p, vec, n, k, v[u]);
        }
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const int64_t k = k0 + (int64_t)u * 2048;
            if (k < p.K) qr_store8<FORMAT>(p, vec_q, n, k, v[u], s);
        }
    }
}

template <int FORMAT>
static const void* quantize_rows_pick(int64_t K) {
    if (K <= 512) return (const void*)quantize_rows_kernel<FORMAT, 64, 1>;
    if (K <= GEMLITE_QUANT_ROWS_WAVE_MAX_K) return (const void*)quantize_rows_kernel<FORMAT, 64, 2>;
    if (K <= 2048) return (const void*)quantize_rows_kernel<FORMAT, 256, 1>;
    if (K <= 4096) return (const void*)quantize_rows_kernel<FORMAT, 256, 2>;
    if (K <= 8192) return (const void*)quantize_rows_kernel<FORMAT, 256, 4>;
    if (K <= GEMLITE_QUANT_ROWS_RESIDENT_MAX_K) return (const void*)quantize_rows_kernel<FORMAT, 256, 8>;
    return (const void*)quantize_rows_reread_kernel<FORMAT>;
}
static_assert(GEMLITE_QUANT_ROWS_WAVE_MAX_K == 64 * 8 * 2 && GEMLITE_QUANT_ROWS_RESIDENT_MAX_K == 256 * 8 * 8, "form limits");

const void* quantize_rows_kernel_fn(int format, int64_t K) {
    return format == 0 ? quantize_rows_pick<0>(K) : (format == 1 ? quantize_rows_pick<1>(K) : quantize_rows_pick<2>(K));
}

}  // namespace gl
