// gemm_wn_mma_kernel.inc (included by gemm_wn_mma_f16.hip / _bf16.hip / gemm_wn_mma.hip) — fused unpack + dequant + tiled MFMA GEMM for packed low-bit weights (4 / 2 / 1 / 8-bit words),
// the large-M (prefill) kernel.  Replaces gemm_INT_kernel (gemlite/triton_kernels/gemm_kernels.py:248-413) and, for
// shapes the few-row kernels do not take, gemm_splitK_INT_kernel (gemm_splitK_kernels.py:277-450).
//
// Design (CDNA4; numbers in DESIGN.md §3.3):
//   * Block = 8 waves = two waves per SIMD, tile (32*MI) x 128, K step KSTEP (128 or 256).  Wave (cg = wave & 3,
//     kh = wave >> 2) owns ALL rows x columns [32cg, 32cg+32) x the kh-th HALF of every K step: the two waves of a SIMD
//     work on different halves of K, so one wave's MFMAs cover the other's unpack arithmetic, LDS reads and memory
//     requests, and a 256-row tile (the shape that needs the least dequant work per MFMA: 19 VALU per 8 MFMAs) no
//     longer leaves the SIMD with a single in-order wave.  The two K halves are added through LDS in the epilogue.
//   * B: one packed int32 word holds 8 (4-bit) / 16 / 32 / 4 consecutive k of ONE column, i.e. 1 / 2 / 4 / half of a
//     lane's B fragment of v_mfma_f32_32x32x16 (lane = column l & 31, k-octet l >> 5).  The wave loads its words
//     straight from HBM / L2 with buffer loads (voffset = column, soffset = packed row: no VALU per load),
//     dequantises them in registers in natural k order and feeds MI MFMAs with each fragment.  Weights never touch LDS.
//   * A (x): the (32*MI) x KSTEP tile of every step goes global -> LDS by LDS-DMA (buffer_load_dwordx4 ... lds), no
//     VGPR staging and no ds_write; the 16-byte slots of a row are XOR-swizzled with (row & 15) by permuting the
//     per-lane SOURCE address (the LDS image of a DMA is lane-linear), which makes the ds_read_b128 of 32 rows
//     conflict-free.  Two stages; everything a step needs is requested one step (x) / two steps (weights) ahead,
//     so ONE s_waitcnt vmcnt(0) + ONE s_barrier per step is all the synchronisation there is, and both sit a few
//     MFMA slots before the end of the step so that the first fragments of the next stage are read under MFMAs.
//   * K may be split over gridDim.y; slices are combined with the write-through slab + ticket protocol (gl_common.h).
#pragma once
#include <type_traits>

#include "gl_common.h"
#include "gl_async.h"

namespace gl {

namespace mma {

using namespace async;

constexpr int BN = 128;
constexpr int C_ROWS = 128;        // rows of the epilogue staging tile (one pass per 128 rows)
constexpr int C_PITCH = BN + 4;    // floats per row of that tile
constexpr int LOOKAHEAD = 4;       // A fragments requested ahead of their MFMA

template <typename Tag>
__device__ __forceinline__ f32x16 mfma32(u32x4 a, u32x4 b, f32x16 c);
template <>
__device__ __forceinline__ f32x16 mfma32<half_tag>(u32x4 a, u32x4 b, f32x16 c) {
    return __builtin_amdgcn_mfma_f32_32x32x16_f16(__builtin_bit_cast(h8_t, a), __builtin_bit_cast(h8_t, b), c, 0, 0, 0);
}
template <>
__device__ __forceinline__ f32x16 mfma32<bf16_tag>(u32x4 a, u32x4 b, f32x16 c) {
    return __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(b8_t, a), __builtin_bit_cast(b8_t, b), c, 0, 0, 0);
}

// ---- activation element type of the MFMA --------------------------------------------------------------------------------
// XDT = 0: x holds the 16-bit floats of Tag.  XDT = GEMLITE_DT_FP8E4 / GEMLITE_DT_INT8: 8-bit activations (the reference's
// A8Wn dynamic and BitNet-int8 processors, helper.py:502-615, 1006-1062): the dequantised weight is cast to the activation
// type, like the reference's `b.to(a.dtype)` before tl.dot (gemm_kernels.py:384), and the product runs on the fp8 / int8
// MFMA of the same 32x32x16 shape — a lane's fragment is still 8 consecutive k, now 8 bytes instead of 16.
template <typename Tag, int XDT>
struct XOps {
    static constexpr int ES = 2;
    typedef u32x4 frag_t;
    typedef f32x16 acc_t;
    static __device__ __forceinline__ f32x16 mfma(frag_t a, frag_t b, f32x16 c) { return mfma32<Tag>(a, b, c); }
};
template <typename Tag>
struct XOps<Tag, GEMLITE_DT_FP8E4> {
    static constexpr int ES = 1;
    typedef u32x2 frag_t;
    typedef f32x16 acc_t;
    static __device__ __forceinline__ f32x16 mfma(frag_t a, frag_t b, f32x16 c) {
        return __builtin_amdgcn_mfma_f32_32x32x16_fp8_fp8(__builtin_bit_cast(long, a), __builtin_bit_cast(long, b), c, 0, 0, 0);
    }
};
template <typename Tag>
struct XOps<Tag, GEMLITE_DT_INT8> {  // int32 accumulation (converted to fp32 once, after the K loop)
    static constexpr int ES = 1;
    typedef u32x2 frag_t;
    typedef i32x16 acc_t;
    static __device__ __forceinline__ i32x16 mfma(frag_t a, frag_t b, i32x16 c) {
        return __builtin_amdgcn_mfma_i32_32x32x16_i8(__builtin_bit_cast(long, a), __builtin_bit_cast(long, b), c, 0, 0, 0);
    }
};

// ---- geometry of one 64-k sub-block by bit width ------------------------------------------------------------------
// WPL words per lane, packed row of word i for lane half h: rb + RI(i) + HS * h, k offset (inside the sub-block) of
// MFMA slice u for lane half h: KO(u, h).
template <int NBITS>
struct Geo {
    static constexpr int E = 32 / NBITS;
    static constexpr int WPL = NBITS;                       // 4 -> 4 words, 2 -> 2, 1 -> 1, 8 -> 8
    static constexpr int ROWS = 64 / E;                     // packed rows per sub-block
    static constexpr int HS = NBITS == 8 ? 2 : 1;
    static __device__ __forceinline__ constexpr int row_of(int i) { return NBITS == 8 ? 4 * (i >> 1) + (i & 1) : (NBITS == 1 ? 0 : 2 * i); }
    static __device__ __forceinline__ constexpr int k_of(int u, int h) {
        return NBITS == 2 ? 16 * (2 * (u >> 1) + h) + 8 * (u & 1) : (NBITS == 1 ? 32 * h + 8 * u : 8 * (2 * u + h));
    }
};

// Block-scaled weights under 16-bit activations (A16W8 / A16W4 MXFP, helper.py:372-400): NBITS = 108 (fp8 e4m3) / 104 (e2m1
// codes, two per byte).  These rows are K-CONTIGUOUS per output column (core.py:363-398): lane half h owns the 32 k of ONE
// microscaling block of the 64-k sub-block — 32 / 16 consecutive bytes = WPL dwords, fetched as 16-byte pieces — and
// slice u is its k [8u, 8u + 8): k_of(u, h) = 32 h + 8 u (any k order works as long as A follows).  E = 1: "packed rows"
// are k itself.
constexpr int MXW8 = 108, MXW4 = 104;
// NVFP4 weights (round 4): the MXW4 bytes with an e4m3 scale per 16 k instead of an e8m0 per 32 k — a lane-half's 32 k are TWO
// blocks.  The converters take only a scale's exponent (scripts/ubench/probe_cvt_scale.hip), so a pair is converted at scale 1 and
// multiplied by the scale in fp16: e2m1 (2 significant bits) x e4m3 (4) is exact in fp16's 11, and |w s| stays within
// [2^-10, 2688].  fp16 only — the kernel's x is the fp16 expansion of the NVFP4 activations (exact as well), the epilogue is untyped.
constexpr int NVW4 = 204;
template <>
struct Geo<MXW8> {
    static constexpr int E = 1, WPL = 8, ROWS = 64, HS = 0, WBYTES64 = 64;
    static __device__ __forceinline__ constexpr int row_of(int) { return 0; }
    static __device__ __forceinline__ constexpr int k_of(int u, int h) { return 32 * h + 8 * u; }
};
template <>
struct Geo<MXW4> {
    static constexpr int E = 1, WPL = 4, ROWS = 64, HS = 0, WBYTES64 = 32;
    static __device__ __forceinline__ constexpr int row_of(int) { return 0; }
    static __device__ __forceinline__ constexpr int k_of(int u, int h) { return 32 * h + 8 * u; }
};
template <>
struct Geo<NVW4> : Geo<MXW4> {};
// Plain 8-bit weight-only layers (A16W8, helper.py:88-171; round 4): fp8 e4m3 / e5m2 / int8 weights, K-contiguous per output column like
// the MX fp8 rows but WITHOUT block scales — the same geometry, no scale request, the converters at scale 1 (int8: exact integer values);
// the layer's one scale per channel is applied in the epilogue.  Until round 4 these layers had no tile kernel: 68 us at 4096^2, M = 256
// (64-row tiles of the rows kernel), 506 us at M = 2048 — against 25 / 72 us for the block-scaled twin on this kernel.
constexpr int KW8F = 118, KW8B = 119, KW8I = 120;
template <> struct Geo<KW8F> : Geo<MXW8> {};
template <> struct Geo<KW8B> : Geo<MXW8> {};
template <> struct Geo<KW8I> : Geo<MXW8> {};
// pair j (k = 2j, 2j + 1 of the slice) of a block-scaled fragment: hardware converters with the block scale applied
// (v_cvt_scalef32_pk_{bf16,f16}_{fp8,fp4}; operand order measured with scripts/ubench/probe_mx.hip)
template <typename Tag, int NBITS, int J>
__device__ __forceinline__ uint32_t mx_pair_c(const uint32_t* w, int u, float sc) {  // the selectors are immediates
    if constexpr (NBITS == NVW4) {  // sc: the e4m3 block scale as an fp16 PAIR (bit pattern)
        static_assert(std::is_same<Tag, half_tag>::value, "NVFP4 weights: fp16 arithmetic");
        const h2_t v = __builtin_amdgcn_cvt_scalef32_pk_f16_fp4(w[u], 1.0f, J);
        return __builtin_bit_cast(uint32_t, v * __builtin_bit_cast(h2_t, sc));
    } else if constexpr (NBITS == KW8B) {  // e5m2 bytes
        const uint32_t src = w[2 * u + (J >> 1)];
        if constexpr (std::is_same<Tag, bf16_tag>::value) return __builtin_bit_cast(uint32_t, __builtin_amdgcn_cvt_scalef32_pk_bf16_bf8(src, sc, (J & 1) != 0));
        else return __builtin_bit_cast(uint32_t, __builtin_amdgcn_cvt_scalef32_pk_f16_bf8(src, sc, (J & 1) != 0));
    } else if constexpr (NBITS == KW8I) {  // int8 bytes: exact in fp16 and bf16
        const uint32_t src = w[2 * u + (J >> 1)];
        if constexpr (std::is_same<Tag, half_tag>::value) {
            // {0x64, u.b[2 r + 1], 0x64, u.b[2 r]} with u = b + 128: 1024 + (b + 128), minus 1152
            const uint32_t uu = src ^ 0x80808080u;
            const uint32_t pr = __builtin_amdgcn_perm(0x64646464u, uu, (J & 1) ? 0x04030402u : 0x04010400u);
            return __builtin_bit_cast(uint32_t, __builtin_bit_cast(h2_t, pr) - (h2_t){(_Float16)1152.0f, (_Float16)1152.0f});
        } else {
            const int sh = 16 * (J & 1);
            const b2_t v = {(__bf16)(float)(int8_t)(src >> sh), (__bf16)(float)(int8_t)(src >> (sh + 8))};
            return __builtin_bit_cast(uint32_t, v);
        }
    } else if constexpr (NBITS == MXW4) {
        if constexpr (std::is_same<Tag, bf16_tag>::value) return __builtin_bit_cast(uint32_t, __builtin_amdgcn_cvt_scalef32_pk_bf16_fp4(w[u], sc, J));
        else return __builtin_bit_cast(uint32_t, __builtin_amdgcn_cvt_scalef32_pk_f16_fp4(w[u], sc, J));
    } else {
        const uint32_t src = w[2 * u + (J >> 1)];
        if constexpr (std::is_same<Tag, bf16_tag>::value) return __builtin_bit_cast(uint32_t, __builtin_amdgcn_cvt_scalef32_pk_bf16_fp8(src, sc, (J & 1) != 0));
        else return __builtin_bit_cast(uint32_t, __builtin_amdgcn_cvt_scalef32_pk_f16_fp8(src, sc, (J & 1) != 0));
    }
}
template <typename Tag, int NBITS>
__device__ __forceinline__ uint32_t mx_pair(const uint32_t* w, int u, int j, float sc) {
    switch (j) {
        case 0: return mx_pair_c<Tag, NBITS, 0>(w, u, sc);
        case 1: return mx_pair_c<Tag, NBITS, 1>(w, u, sc);
        case 2: return mx_pair_c<Tag, NBITS, 2>(w, u, sc);
        default: return mx_pair_c<Tag, NBITS, 3>(w, u, sc);
    }
}

// ---- integer codes of slice u as bytes: byte j of `ev` = code 2j, byte j of `od` = code 2j + 1 (natural k order) -----
template <int NBITS>
struct Extract;
template <>
struct Extract<4> {
    __device__ __forceinline__ static void run(const uint32_t (&w)[4], int u, uint32_t& ev, uint32_t& od) {
        ev = w[u] & 0x0F0F0F0Fu;
        od = (w[u] >> 4) & 0x0F0F0F0Fu;
    }
};
template <>
struct Extract<8> {
    __device__ __forceinline__ static void run(const uint32_t (&w)[8], int u, uint32_t& ev, uint32_t& od) {
        ev = __builtin_amdgcn_perm(w[2 * u + 1], w[2 * u], 0x06040200u);  // bytes 0, 2 of each word
        od = __builtin_amdgcn_perm(w[2 * u + 1], w[2 * u], 0x07050301u);  // bytes 1, 3
    }
};
template <>
struct Extract<2> {
    // m_a = (w >> 2a) & 0x03030303: byte b of m_a = code 4b + a.  Slice t = u & 1 of word u >> 1 holds codes 8t .. 8t+7.
    __device__ __forceinline__ static void run(const uint32_t (&w)[2], int u, uint32_t& ev, uint32_t& od) {
        const uint32_t x = w[u >> 1];
        const uint32_t m0 = x & 0x03030303u, m1 = (x >> 2) & 0x03030303u, m2 = (x >> 4) & 0x03030303u, m3 = (x >> 6) & 0x03030303u;
        const uint32_t sel = (u & 1) ? 0x07030602u : 0x05010400u;  // {m0.b[2t], m2.b[2t], m0.b[2t+1], m2.b[2t+1]}
        ev = __builtin_amdgcn_perm(m2, m0, sel);
        od = __builtin_amdgcn_perm(m3, m1, sel);
    }
};
template <>
struct Extract<1> {
    // m_a = (w >> a) & 0x01010101: byte b of m_a = bit 8b + a, i.e. code a of slice b
    __device__ __forceinline__ static void run(const uint32_t (&w)[1], int u, uint32_t& ev, uint32_t& od) {
        const uint32_t x = w[0];
        uint32_t m[8];
#pragma unroll
        for (int a = 0; a < 8; ++a) m[a] = (x >> a) & 0x01010101u;
        const uint32_t s2 = 0x0C0C0400u + 0x00000101u * (uint32_t)u;  // {lo.b[u], hi.b[u], 0, 0}
        const uint32_t e01 = __builtin_amdgcn_perm(m[2], m[0], s2), e23 = __builtin_amdgcn_perm(m[6], m[4], s2);
        const uint32_t o01 = __builtin_amdgcn_perm(m[3], m[1], s2), o23 = __builtin_amdgcn_perm(m[7], m[5], s2);
        ev = e01 | (e23 << 16);
        od = o01 | (o23 << 16);
    }
};

// ---- codes -> one B fragment (8 dequantised 16-bit floats, natural k order) --------------------------------------------
template <typename Tag>
struct Convert;
// Integer codes 0 .. 15 read as e4m3 BYTES are linear (b < 8: subnormal b * 2^-9; 8 <= b < 16: (8 + (b - 8)) * 2^-9), so the
// block-scale converter of gfx950 turns two code bytes into two exact fp32 integers in ONE instruction (scale 2^9) where
// v_cvt_f32_ubyte<i> takes two.  HI selects bytes 2, 3 of the register (an immediate).
typedef float f2_t __attribute__((ext_vector_type(2)));
template <bool HI>
__device__ __forceinline__ f2_t codes_f32x2(uint32_t bytes) { return __builtin_amdgcn_cvt_scalef32_pk_f32_fp8(bytes, 512.0f, HI); }
// The affine map stays two SCALAR v_fma_f32 per converter result: v_pk_fma_f32 beside MFMAs is an anti-lever (guide: +22
// cycles per instruction; measured here on one box, scripts/ab_mma.sh: cfgB 47.6 us with v_cvt_f32_ubyte, 44.7 with the
// converter + scalar fmas, 47.6 with the converter + packed fmas; prefill 251 / 250 / 264 us)
#ifdef GL_MMA_PKFMA  // A/B builds only (scripts/ab_mma.sh): one v_pk_fma_f32 instead of two v_fma_f32
__device__ __forceinline__ f2_t affine2(f2_t q, float A, float B) { return __builtin_elementwise_fma(q, (f2_t){A, A}, (f2_t){B, B}); }
#else
__device__ __forceinline__ f2_t affine2(f2_t q, float A, float B) { return (f2_t){__builtin_fmaf(q.x, A, B), __builtin_fmaf(q.y, A, B)}; }
#endif

template <>
struct Convert<bf16_tag> {
    float A, B;  // v = fma(q, A, B) in fp32, rounded once to bf16
    f2_t te, to; // LIN: the fp32 values of codes (4h, 4h + 2) and (4h + 1, 4h + 3) of the half-slice in flight
    __device__ __forceinline__ void set(float s, float z, float u13, float u4) {
        A = s;
        B = z * __builtin_fmaf(-u13, s, u4);
    }
    // pair j = codes 2j, 2j+1 of the slice: two v_cvt_f32_ubyte<j>, two v_fma_f32, one v_cvt_pk_bf16_f32
    __device__ __forceinline__ uint32_t pair(uint32_t ev, uint32_t od, int j) const {
        const float lo = (float)((ev >> (8 * j)) & 0xFFu), hi = (float)((od >> (8 * j)) & 0xFFu);
        const b2_t v = {(__bf16)__builtin_fmaf(lo, A, B), (__bf16)__builtin_fmaf(hi, A, B)};
        return __builtin_bit_cast(uint32_t, v);
    }
    // LIN (codes < 16): per half-slice two converter ops + four v_fma_f32, then one v_cvt_pk_bf16_f32 per pair: 19 VALU per
    // fragment with the extraction instead of 23
    template <bool LIN>
    __device__ __forceinline__ uint32_t put(uint32_t ev, uint32_t od, int j) {
        if constexpr (!LIN) return pair(ev, od, j);
        else {
            if ((j & 1) == 0) {
                te = affine2((j >> 1) ? codes_f32x2<true>(ev) : codes_f32x2<false>(ev), A, B);
                to = affine2((j >> 1) ? codes_f32x2<true>(od) : codes_f32x2<false>(od), A, B);
            }
            const b2_t v = {(__bf16)((j & 1) ? te.y : te.x), (__bf16)((j & 1) ? to.y : to.x)};
            return __builtin_bit_cast(uint32_t, v);
        }
    }
};
template <>
struct Convert<half_tag> {
    h2_t zsub2, s2, zadd2;  // v = fma(q - zsub, s, zadd) in fp16: rounds where the reference rounds (utils.py:73-87)
    __device__ __forceinline__ void set(float s, float z, float u13, float u4) {
        const _Float16 zs = (_Float16)(z * u13), za = (_Float16)(z * u4), sc = (_Float16)s;
        zsub2 = (h2_t){zs, zs};
        zadd2 = (h2_t){za, za};
        s2 = (h2_t){sc, sc};
    }
    __device__ __forceinline__ uint32_t pair(uint32_t ev, uint32_t od, int j) const {
        // {0, od.b[j], 0, ev.b[j]} | (1024, 1024): 1024 + q exactly, then q = that - 1024
        const uint32_t sel = 0x0C040C00u + 0x00010001u * (uint32_t)j;
        const uint32_t h = __builtin_amdgcn_perm(od, ev, sel) | 0x64006400u;
        const h2_t q = __builtin_bit_cast(h2_t, h) - (h2_t){(_Float16)1024.0f, (_Float16)1024.0f};
        return __builtin_bit_cast(uint32_t, __builtin_elementwise_fma(q - zsub2, s2, zadd2));
    }
    template <bool LIN>
    __device__ __forceinline__ uint32_t put(uint32_t ev, uint32_t od, int j) { return pair(ev, od, j); }
};

// ---- codes -> one B fragment in the activation type ----------------------------------------------------------------------
template <typename Tag, int XDT>
struct ConvertX {  // 16-bit activations: the converters above, pair j -> register j
    Convert<Tag> c;
    __device__ __forceinline__ void set(float s, float z, float u13, float u4) { c.set(s, z, u13, u4); }
    __device__ __forceinline__ void prep(uint32_t&, uint32_t&) const {}
    template <bool LIN>
    __device__ __forceinline__ void put(u32x4& out, uint32_t ev, uint32_t od, int j) { out[j] = c.template put<LIN>(ev, od, j); }
};
template <typename Tag>
struct ConvertX<Tag, GEMLITE_DT_FP8E4> {  // fp32 fma, one rounding to e4m3 (v_cvt_pk_fp8_f32): pair j -> half j & 1 of register j >> 1
    float A, B;
    f2_t te, to;
    __device__ __forceinline__ void set(float s, float z, float u13, float u4) {
        A = s;
        B = z * __builtin_fmaf(-u13, s, u4);
    }
    __device__ __forceinline__ void prep(uint32_t&, uint32_t&) const {}
    template <bool LIN>
    __device__ __forceinline__ void put(u32x2& out, uint32_t ev, uint32_t od, int j) {
        float a, b;
        if constexpr (LIN) {  // see Convert<bf16_tag>::put
            if ((j & 1) == 0) {
                te = affine2((j >> 1) ? codes_f32x2<true>(ev) : codes_f32x2<false>(ev), A, B);
                to = affine2((j >> 1) ? codes_f32x2<true>(od) : codes_f32x2<false>(od), A, B);
            }
            a = (j & 1) ? te.y : te.x;
            b = (j & 1) ? to.y : to.x;
        } else {
            const float lo = (float)((ev >> (8 * j)) & 0xFFu), hi = (float)((od >> (8 * j)) & 0xFFu);
            a = __builtin_fmaf(lo, A, B), b = __builtin_fmaf(hi, A, B);
        }
        const uint32_t prev = out[j >> 1];
        out[j >> 1] = (j & 1) ? (uint32_t)__builtin_amdgcn_cvt_pk_fp8_f32(a, b, (int)prev, true)
                              : (uint32_t)__builtin_amdgcn_cvt_pk_fp8_f32(a, b, (int)prev, false);
    }
};
template <typename Tag>
struct ConvertX<Tag, GEMLITE_DT_INT8> {  // integer codes minus an integer zero (W_group_mode 0 / 1 with a scalar zero): exact int8
    uint32_t zz;  // the zero in every byte
    __device__ __forceinline__ void set(float, float z, float u13, float) { zz = 0x01010101u * ((uint32_t)(int)(z * u13) & 0xFFu); }
    // bytewise q - z without borrows between bytes: ((q | 0x80) - z) ^ 0x80  (q <= 127 + z, z <= 127)
    __device__ __forceinline__ void prep(uint32_t& ev, uint32_t& od) const {
        ev = ((ev | 0x80808080u) - zz) ^ 0x80808080u;
        od = ((od | 0x80808080u) - zz) ^ 0x80808080u;
    }
    template <bool LIN>
    __device__ __forceinline__ void put(u32x2& out, uint32_t ev, uint32_t od, int j) const {
        if (j & 1) out[j >> 1] = __builtin_amdgcn_perm(od, ev, j == 1 ? 0x05010400u : 0x07030602u);  // {ev[2r], od[2r], ev[2r+1], od[2r+1]}
    }
};

// (in a __device__ function: a "v" constraint inside a lambda of the kernel body silently drops the kernel's host stub)
__device__ __forceinline__ void opaque2(uint32_t& a, uint32_t& b) { asm volatile("" : "+v"(a), "+v"(b)); }

// 8- / 16-bit packed words (WB = 1 / 2 bytes per word).  The little-endian concatenation of byte rows 4R .. 4R+3 (short rows 2R, 2R+1)
// of a column IS that column's int32 word of packed row R (bitpack.py: element i of a word sits at bits [b i, b i + b)), so only the
// word source differs from WB = 4.  Lanes 4c .. 4c+3 own 4 adjacent columns: lane 4c + q loads byte row 4R + q of the quad's 4 columns
// (WB = 2: short row 2R + (q & 1), column pair q >> 1) as one dword, and a transpose across the quad — DPP quad_perm + v_perm, selectors
// per lane from quad_sel() — hands every lane its own column's word.  EXEC is all ones wherever this runs.
template <int WB>
__device__ __forceinline__ uint32_t quad_word(uint32_t v, uint32_t sel1, uint32_t sel2) {
    if constexpr (WB == 1) {
        const uint32_t t = (uint32_t)__builtin_amdgcn_mov_dpp((int)v, 0x4E, 0xF, 0xF, false);  // quad_perm(2, 3, 0, 1)
        const uint32_t y = __builtin_amdgcn_perm(t, v, sel1);  // q < 2: columns 0, 1 of rows q, q + 2; q >= 2: columns 2, 3 of rows q - 2, q
        const uint32_t u = (uint32_t)__builtin_amdgcn_mov_dpp((int)y, 0xB1, 0xF, 0xF, false);  // quad_perm(1, 0, 3, 2)
        return __builtin_amdgcn_perm(u, y, sel2);
    } else if constexpr (WB == 2) {
        const uint32_t t = (uint32_t)__builtin_amdgcn_mov_dpp((int)v, 0xB1, 0xF, 0xF, false);
        return __builtin_amdgcn_perm(t, v, sel1);
    } else {
        return v;
    }
}
template <int WB>
__device__ __forceinline__ void quad_sel(int q, uint32_t& sel1, uint32_t& sel2) {
    sel1 = WB == 1 ? (q < 2 ? 0x05040100u : 0x03020706u) : ((q & 1) ? 0x03020706u : 0x05040100u);
    sel2 = (q & 1) ? 0x03070105u : 0x06020400u;
}
// byte offset of lane q's dword inside packed row R of the quad at column c4 (a multiple of 4), with sw = the row stride in words
template <int WB>
__device__ __forceinline__ uint32_t quad_offset(int q, int c4, int sw) {
    if constexpr (WB == 1) return (uint32_t)(q * sw + c4);
    else if constexpr (WB == 2) return (uint32_t)((q & 1) * 2 * sw + c4 * 2 + (q >> 1) * 4);
    else return (uint32_t)(c4 + q) * 4u;
}
// the packed words slice u of a 64-k sub-block reads (Extract<NBITS>)
template <int NBITS>
__device__ __forceinline__ constexpr bool word_in_slice(int i, int u) {
    return NBITS == 4 ? i == u : (NBITS == 2 ? i == (u >> 1) : (NBITS == 1 ? i == 0 : (i >> 1) == u));
}

// One LDS-DMA piece: 64 lanes x 16 bytes from buffer offset (voff per lane + soff) to LDS [dst, dst + 1024), lane-linear.
// (A __device__ function: the address-space cast inside a kernel-body lambda silently drops the kernel's host stub.)
__device__ __forceinline__ void lds_dma16(__amdgpu_buffer_rsrc_t rs, unsigned char* dst, uint32_t voff, uint32_t soff) {
    __builtin_amdgcn_raw_ptr_buffer_load_lds(rs, (__attribute__((address_space(3))) void*)dst, 16, voff, soff, 0, 0);
}

}  // namespace mma

// MI 32-row blocks per wave (tile rows = 32 * MI), KSTEP k per step (each wave: KSTEP / 2).
// EXP (development builds only, -DGL_MMA_EXPERIMENTS + GEMLITE_DEV_ABLATION): drop parts of the K loop to see what each costs —
// 1 barrier + counted wait, 2 dequant VALU, 4 A-fragment reads, 8 x DMA requests, 16 weight requests, 32 the scalar address
// arithmetic of the requests (constant offsets).  Results are wrong.
// KH = 2 (default): tile 32 MI x 128, wave (cg = wave & 3, kh = wave >> 2) owns 32 columns x one HALF of every K step.
// KH = 4 ("narrow", round 4): tile 32 MI x 64, wave (cg = wave & 1, kh = wave >> 1) owns 32 columns x one QUARTER of every K step.
// Twice the tiles at the same rows: M = 256 over 4096^2 gives 4 x 64 = 256 tiles of 64 x 64 and 8192^2 gives 2 x 128 = 256 tiles of
// 128 x 64 — the chip is full WITHOUT K slices, so the whole slab + ticket combine (3.5-4.3 us of dependent memory round trips at
// the headline shapes, profiles/r03/timeline_mma3_v1.log) and its slab traffic disappear; what it costs is x traffic through the CU's
// vector-memory path (a 64-column tile moves (2 BM + 32) bytes per k for 128 BM flop) — the unsplit A8W8 tiles of this round
// (gemm_a8w8.hip: 21.7 -> 13.6 us) are the same trade.
// KH = 1 ("wide"): tile 32 MI x 256, wave cg = wave owns 32 columns x the whole step — every x byte DMA'd into LDS feeds twice
// the columns: the 128-column tiles move 576 B of operands per k for 2 * 256 * 128 flop, i.e. ~10 TB/s through the L2s at the
// prefill rate they reach, which is the measured ceiling of that path; the wide tile needs 640 B per k for twice the flop.
// XCH = 1: K slices are combined by reduce-scatter (see "epilogue 2x"); the slab + ticket code is not compiled into that variant
// (both epilogues in one kernel made the 256-row tiles shuffle their 128 accumulators through scratch at the branch).
// WL = 1 (round 6): the packed words of a K step travel global -> LDS by LDS-DMA next to the x tile — ONE 1-KiB request per wave and step
// instead of WPL four-byte register loads per lane and sub-block (64 lanes x 4 B: the CU's address path takes ~10 cycles per wave-level
// memory instruction WHATEVER its width, and the K-loop ablation of round 6 — profiles/r06/ablate_m256.log — put 4.1 of cfgA's 16.5 us on
// these requests, more than on the dequantisation arithmetic).  The words of step s + 1 are read back from LDS (one ds_read_b32 per word,
// conflict-free: 32 consecutive columns of one packed row) right behind the barrier of step s.  Metadata stays in the register ring.
// Tiles up to 128 rows (MI <= 4: the barrier slot must not come after the slot that dequantises the next step's first slice).
// NGS = 2 (round 6): quantisation groups of 32 — TWO (scale, zero) pairs per column and 64-k sub-block instead of one.  Slice u of a lane covers
// 8 k at k_of(u, h): its group inside the sub-block is k_of(u, h) / 32, which for 1-bit words depends on the lane half h (a per-lane select).
// 32-row tiles only (any M through the grid): it is what takes 1- / 2- / 8-bit words and 8-bit activations with groups of 32 off the
// coverage kernel at M >= 2 (VERDICT r5 #8); 4- / 2-bit words under 16-bit activations have the rows kernel up to 64 rows per block.
// WBY = 1 / 2: 8- / 16-bit packed words ([K / e8, N] uint8, [K / e16, N] int16) on the register path: the same requests (one dword per lane and
// word, voffset from quad_offset()), the words regrouped across the quad (quad_word()) where a slice is dequantised; everything else as WBY = 4.
template <typename Tag, int NBITS, int MI, int KSTEP, int RD, int NST, int EXP = 0, int XDT = 0, int KH = 2, int XCH = 0, int WL = 0, int NGS = 1, int WBY = 4>
__global__ __launch_bounds__(512, 2) void gemm_wn_mma_kernel(const WnParams p) {
    using namespace mma;
    using TR = F16Traits<Tag>;  // output / metadata type; also the activation type when XDT == 0
    using G = Geo<NBITS>;
    using XO = XOps<Tag, XDT>;
    typedef typename XO::frag_t frag_t;
    constexpr int ES = XO::ES;  // bytes per activation
    constexpr int BM = 32 * MI, KW = KSTEP / KH, SUB = KW / 64, WPL = G::WPL;
    constexpr int BN = 256 / KH, C_PITCH = BN + 4;  // (shadow the namespace's 128-column constants)
    static_assert(KH == 1 || KH == 2 || KH == 4, "one, two or four K parts per step");
    constexpr int NCG = 8 / KH;  // column groups of 32 = waves per K part
    constexpr bool NVW = NBITS == NVW4;                               // e4m3 scale per 16 k: two scale bytes per lane-half and sub-block
    constexpr bool NOSC = NBITS == KW8F || NBITS == KW8B || NBITS == KW8I;  // K-contiguous 8-bit weights without block scales (A16W8)
    constexpr bool MXW = NBITS == MXW8 || NBITS == MXW4 || NVW || NOSC;  // K-contiguous weights (16-bit activations only)
    static_assert(!MXW || XDT == 0, "block-scaled weights on this kernel: 16-bit activations");
    static_assert(NGS == 1 || (NGS == 2 && !MXW && !WL && MI == 1), "groups of 32: packed integer words, 32-row tiles");
    static_assert(WBY == 4 || ((WBY == 1 || WBY == 2) && !MXW && !WL && NGS == 1 && XDT == 0 && (NBITS != 8 || WBY == 2)),
                  "8- / 16-bit packed words: register path, 16-bit activations");
    constexpr int PITCH = KSTEP * ES, XSTAGE = BM * PITCH;  // bytes per row / per stage of x
    constexpr int WTILE = WL ? (KSTEP / G::E) * BN * 4 : 0;  // WL: the step's packed words [KSTEP / E rows][BN columns] behind the x tile
    constexpr int STAGE = XSTAGE + WTILE;
    constexpr int WPC = WL ? 1 : 0;                          // weight DMA pieces per wave and stage
    static_assert(!WL || (WTILE == 8 * 1024 && MI <= 4 && NBITS <= 8 && XDT == 0), "WL: 8 KiB of packed words per step = one piece per wave; 16-bit activations");
    constexpr int SWZ = (PITCH / 16 < 16 ? PITCH / 16 : 16) - 1;  // XOR swizzle of the 16-byte slots inside a row (8 or 16 slots)
    // the swizzle key of row r: r itself for rows of >= 256 B (one row spans all 64 banks); 128-byte rows alternate between
    // the two bank halves, so rows r and r + 8 of one ds_read_b128 lane group ({0-3, 12-15, 20-27}, {4-11, 16-19, 28-31})
    // would meet in the same slot AND the same half — key r >> 1 separates them (PMC on the first wide build:
    // SQ_LDS_BANK_CONFLICT = 49 % of SQ_LDS_IDX_ACTIVE with key r)
    constexpr int SWZ_SH = (PITCH == 128 && ES == 2) ? 1 : 0;
    constexpr int PIECES = XSTAGE / 1024 / 8;              // 1-KiB LDS-DMA pieces of x per wave and stage
    constexpr int PALL = PIECES + WPC;                     // ... of x and packed words
    constexpr int NS = SUB * 4;                            // MFMA slices (k16) per wave and step
    constexpr int NQ = NS * MI;                            // MFMA slots per wave and step
    constexpr int L = LOOKAHEAD;
    constexpr int PD = RD - 2;  // weights are requested PD steps ahead (ring of RD steps: short steps need a deep ring —
                                // an HBM round trip under load is 2-3k cycles, a step of the 32-row tile 512)
    // NST LDS stages of x: the tile of step s + NST - 1 is requested during step s.  With two stages the DMA is waited for
    // in the very step that issued it, which only a long step (256-row tile: ~2k cycles) covers; the shorter steps of the
    // smaller tiles spent ~40 % of their time in that wait (profiles/r02 PMC: SQ_WAIT_ANY 42 % of wave cycles).
    static_assert(SUB >= 1 && PIECES >= 1 && NQ >= 2 * L && RD % NST == 0 && RD >= 4 && NST >= 2, "tile too small for the slot schedule");
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];  // [NST][STAGE], later the epilogue tiles

    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int cg = KH == 1 ? wave : (wave & (NCG - 1)), kh = KH == 1 ? 0 : (KH == 2 ? (wave >> 2) : (wave >> 1));
    const int col = lane & 31, h = lane >> 5;
    const int mtiles = (p.M + BM - 1) / BM;
    // (tile, K slice) of this block.  Opt-in (GEMLITE_TF_XCD_SLICE_MAP): block b runs on XCD b % 8 and every XCD has its own L2, so
    // giving all blocks of one XCD the SAME K slice keeps that slice's x rows (re-read by every column tile) in one L2.
    // Measured SLOWER (cfgB 53 vs 46 us, cfgA 21.2 vs 19.1 us: 32 CUs asking for the same lines at once), so the default
    // is the plain (x = tile, y = slice) grid.  Speed only; any map is correct.
    int bid = blockIdx.x, slice = blockIdx.y;
    {
        const int T = gridDim.x, S = gridDim.y;
        if ((p.flags & GEMLITE_TF_XCD_SLICE_MAP) && S > 1 && (8 % S) == 0 && ((T * S) & 7) == 0) {
            const int lin = blockIdx.x + T * blockIdx.y, xcd = lin & 7, idx = lin >> 3;
            slice = xcd % S;
            bid = idx * (8 / S) + xcd / S;
        }
    }
    int mt = bid % mtiles, nt = bid / mtiles;  // M tiles fastest: neighbours share the weight tile in L2
    if constexpr (KH == 4) {
        // narrow tiles: the row tiles of one weight column tile on ONE XCD, back to back in its dispatch order (block b runs on XCD
        // b % 8 and every XCD has its own L2: mtiles - 1 of them read the weights from L2).  Speed only; any map is correct.
        const int ntiles = p.N / BN;
        if ((ntiles & 7) == 0 && gridDim.y == 1) {
            const int xcd = bid & 7, idx = bid >> 3;
            mt = idx % mtiles;
            nt = (idx / mtiles) * 8 + xcd;
        }
    }
    const int m0 = mt * BM;
    const int n = nt * BN + cg * 32 + col;  // this lane's column

    // K steps of this slice: the units are dealt as evenly as possible (rows_per_slice = ALL packed rows here), so any
    // step count works (K = 11008: 43 steps of 256)
    constexpr int STEP_ROWS = KSTEP / G::E;
    const int units = p.rows_per_slice / STEP_ROWS;
    const int s_begin = (int)((int64_t)slice * units / p.splitk), s_end = (int)((int64_t)(slice + 1) * units / p.splitk);
    const int nsteps = s_end - s_begin;
    const int row_s0 = s_begin * STEP_ROWS;  // first packed row of the slice
    const int k_s0 = row_s0 * G::E;

    // opt-in timeline (GEMLITE_TF_TIMELINE): wave 0 of EVERY block (the first 256) stores the 100 MHz global clock (s_memrealtime)
    // at 8 points behind the tickets, slot [block][i]: 0 start | 1 prologue barrier | 2 first step | 3 loop done | 4 K halves
    // added | 5 partial tile sent | 6 peers arrived / ticket taken | 7 output stored   (scripts/timeline_mma3.py)
    const int lin_block = blockIdx.x + gridDim.x * blockIdx.y;
    const bool probe = (p.flags & GEMLITE_TF_TIMELINE) && p.counters && wave == 0 && lane == 0 && lin_block < 256;
    unsigned long long* stamps = (unsigned long long*)(p.counters + MAX_SPLITK_COUNTERS) + lin_block * 8;
    auto stamp = [&](int i) __attribute__((always_inline)) {
        if (probe) stamps[i] = __builtin_amdgcn_s_memrealtime();
    };
    stamp(0);

    const bool need_s = p.w_mode >= 2, need_z = (p.w_mode == 1 || p.w_mode >= 3) && !p.zero_is_scalar;
    const float scalar_zero = p.zero_is_scalar ? (float)((const int32_t*)p.zeros)[0] : 0.f;
    const float u13 = (p.w_mode == 1 || p.w_mode == 3) ? 1.f : 0.f, u4 = p.w_mode == 4 ? 1.f : 0.f;
    const int sw = (int)p.stride_wk;
    const int ms = (need_s || need_z) ? (int)p.stride_meta_g : 0;
    const int meta_rows = p.gs_shift >= 31 ? 1 : ((NGS == 2 && p.gs_shift < 0) ? p.K / p.group_size : (p.K >> p.gs_shift));
    const int meta_bytes = ((meta_rows - 1) * ms + p.N) * 2;
    // buffer descriptors (rows >= M and absent metadata read zeros through the range check on the per-lane offset)
    const srd_t rsX = make_srd(p.x, (uint32_t)(((int64_t)(p.M - 1) * p.stride_xm + p.K) * ES));

    // ---- B stream --------------------------------------------------------------------------------------------------
    struct BStep { uint32_t w[SUB][WPL]; uint32_t s[SUB], z[SUB]; uint32_t s2[NGS == 2 ? SUB : 1], z2[NGS == 2 ? SUB : 1]; u128_t q[SUB][MXW ? WPL / 4 : 1]; };  // q: 16-byte pieces in flight (MX rows); s2 / z2: the second group of a sub-block (NGS = 2)
    const int wave_row0 = kh * (KW / G::E);  // first packed row of this wave's half inside a step
    constexpr int WREQ = WL ? 0 : WPL;                 // register requests of packed words per sub-block (WL: none, they come through LDS)
    constexpr int NREQ = MXW ? WPL / 4 + (NVW ? 2 : (NOSC ? 0 : 1)) : WREQ + 2 * NGS;  // requests per sub-block: MX = 16-byte pieces + one scale byte (NV: two, A16W8: none)
    constexpr int NLB = SUB * NREQ;                    // weight / metadata requests per step and wave
    // request `it` (0 .. NLB-1) of step `step` (slice-relative) into ring slot b
    // (the weight / metadata requests are ordinary buffer loads the compiler tracks: it retires them with its own COUNTED
    //  vmcnt — it cannot see the asm DMAs, so its count can only over-wait, never under-wait — and it never copies a
    //  register whose load is still in flight, which it is free to do with the output of an asm load)
    // Round 4: the weight / metadata requests are inline-asm loads like the DMAs, retired by hand with counted waits (wait_b below).
    // Rounds 2-3 left them to the compiler ("it retires them with its own COUNTED vmcnt"), which is only true while its waitcnt pass
    // keeps track across the unrolled ring: 77 of ~100 instantiations carried a full `s_waitcnt vmcnt(0)` per group of K steps
    // (scripts/isa_loops_known.txt), and WHICH ones did changed when a field was appended to WnParams.  An asm load's destination
    // is handed to the compiler with tie() right after the wait that covers it; scripts/isa_asmloads.py checks the generated code
    // for copies of a destination register between its load and that wait.
    uint32_t wvoff, mvoff;
    srd_t brW, brS, brZ;
    if constexpr (MXW) {
        constexpr int WB = G::WBYTES64;  // weight bytes per 64 k
        wvoff = (uint32_t)((int64_t)n * p.stride_wn_b + (int64_t)(k_s0 + kh * KW) * WB / 64 + h * (WB / 2));
        constexpr int SBK = NVW ? 16 : 32;  // k per scale byte
        mvoff = (uint32_t)((int64_t)n * p.stride_meta_n + (int64_t)((k_s0 + kh * KW) / SBK + h * (32 / SBK)) * p.stride_meta_g);
        brW = make_srd((const void*)p.w, (uint32_t)((int64_t)(p.N - 1) * p.stride_wn_b + (int64_t)p.K * WB / 64));
        brS = make_srd(p.scales, (uint32_t)((int64_t)(p.K / SBK - 1) * p.stride_meta_g + (int64_t)(p.N - 1) * p.stride_meta_n + 1));
        brZ = brS;
    } else {
        // (WBY < 4: bytes per packed row of the 32-bit layout = 4 sw whatever the word width, so every per-step / per-row offset below is the same)
        wvoff = (uint32_t)(G::HS * h * sw) * 4u + quad_offset<WBY>(lane & 3, n & ~3, sw);
        mvoff = (uint32_t)n * 2u;
        brW = make_srd((const void*)(p.w + (int64_t)row_s0 * sw), (uint32_t)(nsteps * STEP_ROWS * sw * 4));
        brS = make_srd(need_s ? p.scales : (const void*)p.w, (uint32_t)(need_s ? meta_bytes : 4));
        brZ = make_srd(need_z ? p.zeros : (const void*)p.w, (uint32_t)(need_z ? meta_bytes : 4));
    }
    // (scalar offsets of the packed-word requests = step * bytes-per-step + a loop-invariant per request: one s_mul per step and
    //  one s_add per request instead of add / mul / shift each — the SIMD issues scalar and vector instructions of its two
    //  waves one after the other, 36 SALU per step were ~8 % of the loop)
    uint32_t wconst[SUB][WPL > 8 ? 1 : WPL];
    const uint32_t step_wbytes = MXW ? 0u : (uint32_t)__builtin_amdgcn_readfirstlane(STEP_ROWS * sw * 4);
    if constexpr (!MXW) {
#pragma unroll
        for (int sb = 0; sb < SUB; ++sb)
#pragma unroll
            for (int i = 0; i < WPL; ++i)
                wconst[sb][i] = (uint32_t)__builtin_amdgcn_readfirstlane((wave_row0 + sb * G::ROWS + G::row_of(i)) * sw * 4);
    }
    const int kconst0 = k_s0 + kh * KW;
    const int ms2 = ms * 2;
    // K rotation (round 6; gemm_a8w8_sq_kernel has the reasoning): row tile mt of a weight column tile starts its K steps at mt nsteps / mtiles — every
    // request below maps its step through kof().  Bit 30 of flags, set by the planner for 8-BIT weights on the narrow tiles (same-XCD siblings) where
    // k_rotation_pays(): A16W8 4096^2 M = 256 / 192 23.4 / 23.3 -> 21.9 / 21.4 us, 2048 x 8192 M = 256 26.1 -> 24.6.  Packed 4-bit words gain nothing
    // (cfgA 16.75 vs 16.9 with it; the same row tiles on one XCD for the 128-row tiles + rotation: cfgB 43.7 -> 44.3) — their loops are not bound by
    // the weight stream: profiles/r06/probe_a16w8_tiles_rotation.log, probe_xcd_map_and_rotation_w4_tiles_no_gain.log.  The fp32 sums of a row
    // tile are added in rotated K order: last-bit differences between row tiles, none between runs.
    const int rot = (p.flags & K_ORDER_ON) && mtiles > 1 ? (mt * nsteps) / mtiles : 0;
    auto kof = [&](int step) __attribute__((always_inline)) { const int k = step + rot; return k >= nsteps ? k - nsteps : k; };
    auto req_b = [&](BStep& b, int step, int it) __attribute__((always_inline)) {
        if constexpr (MXW) step = kof(step);   // (only the K-contiguous geometries are ever rotated: the three scalar instructions per request cost cfgA 0.2 us)
        const int sb = it / NREQ, i = it % NREQ;
        if constexpr (MXW) {
            constexpr int WB = G::WBYTES64;
            if (i < WPL / 4) {
                req_u128(b.q[sb][i], brW, wvoff, (EXP & 32) ? 0u : (uint32_t)__builtin_amdgcn_readfirstlane((step * KSTEP + sb * 64) * WB / 64 + i * 16));
            } else if constexpr (NVW) {  // the scales of k [32 h, +16) and [32 h + 16, +16) of the sub-block: rows 2 r, 2 r + 1 of this lane-half
                const uint32_t so = (EXP & 32) ? 0u : (uint32_t)__builtin_amdgcn_readfirstlane(((step * KSTEP + sb * 64) / 16 + (i - WPL / 4)) * (int)p.stride_meta_g);
                if (i == WPL / 4) req_u8(b.s[sb], brS, mvoff, so);
                else req_u8(b.z[sb], brS, mvoff, so);
            } else {
                req_u8(b.s[sb], brS, mvoff, (EXP & 32) ? 0u : (uint32_t)__builtin_amdgcn_readfirstlane(((step * KSTEP + sb * 64) / 32) * (int)p.stride_meta_g));
            }
        } else {
            if (i < WREQ) {
                req_u32n(b.w[sb][i], brW, wvoff, (EXP & 32) ? 0u : (uint32_t)step * step_wbytes + wconst[sb][i]);
            } else {
                const int second = NGS == 2 ? ((i - WREQ) >> 1) : 0;  // NGS = 2: requests (s, z) of k [0, 32) then of k [32, 64) of the sub-block
                // (group sizes that are not a power of two — multiples of 32, round 6: k is wave-uniform and a multiple of 32, the quotient comes from one
                //  scalar multiply-high; tests/test_host_cpu.py checks the magic number over every k / group pair the planner admits)
                // ONLY in the NGS = 2 instantiations (the planner sends every group size that is not a power of two there): the select + multiply-high in
                // the power-of-two forms cost cfgA 0.6 us of 16.1 in a one-box A/B against the round-5 code, for a path those forms never take
                const int kq = kconst0 + sb * 64 + step * KSTEP + second * 32;
                int grow;
                if constexpr (NGS == 2) grow = p.gs_shift >= 0 ? (kq >> p.gs_shift) : (int)__umulhi((uint32_t)kq >> 5, p.gs_magic);
                else grow = kq >> p.gs_shift;
                const uint32_t mo = (EXP & 32) ? 0u : (uint32_t)__builtin_amdgcn_readfirstlane(grow * ms2);
                if (((i - WREQ) & 1) == 0) req_u16(second ? b.s2[sb] : b.s[sb], brS, mvoff, mo);
                else req_u16(second ? b.z2[sb] : b.z[sb], brZ, mvoff, mo);
            }
        }
    };
    // everything but the newest N requests of this wave has landed: the registers of ring slot `b` belong to the compiler from here
    auto tie_b = [&](BStep& b) __attribute__((always_inline)) {
#pragma unroll
        for (int sb = 0; sb < SUB; ++sb) {
            if constexpr (MXW) {
#pragma unroll
                for (int i = 0; i < WPL / 4; ++i) {
                    asm volatile("" : "+v"(b.q[sb][i]));
#pragma unroll
                    for (int t = 0; t < 4; ++t) b.w[sb][4 * i + t] = b.q[sb][i][t];
                }
                if constexpr (!NOSC) tie(b.s[sb]);
                if constexpr (NVW) tie(b.z[sb]);
            } else {
                if constexpr (!WL) {
#pragma unroll
                    for (int i = 0; i < WPL; ++i) tie(b.w[sb][i]);
                }
                tie(b.s[sb]);
                tie(b.z[sb]);
                if constexpr (NGS == 2) {
                    tie(b.s2[sb]);
                    tie(b.z2[sb]);
                }
            }
        }
    };
    // ---- A stream: LDS-DMA pieces.  Piece j of wave w covers LDS bytes [(w * PIECES + j) * 1024, +1024) of a stage;
    //      lane i's 16 bytes land at +16 i, i.e. row (byte / PITCH), physical slot (byte % PITCH) / 16, which holds the
    //      logical slot  phys ^ (row & SWZ)  of that row.
    uint32_t xvoff[PIECES];
#pragma unroll
    for (int j = 0; j < PIECES; ++j) {
        const int byte = (wave * PIECES + j) * 1024 + lane * 16;
        const int r = byte / PITCH, phys = (byte % PITCH) / 16;
        const int logical = phys ^ ((r >> SWZ_SH) & SWZ);
        xvoff[j] = m0 + r < p.M ? (uint32_t)(((int64_t)(m0 + r) * p.stride_xm + k_s0) * ES + logical * 16) : 0x80000000u;
    }
    const uint32_t lds0 = __builtin_amdgcn_readfirstlane(lds_addr_of(smem) + (uint32_t)(wave * PIECES) * 1024u);
    auto req_x = [&](int stage, int step, int j) __attribute__((always_inline)) {
        if constexpr (MXW) step = kof(step);
        req_lds16(rsX, lds0 + (uint32_t)(stage * STAGE + j * 1024), xvoff[j], (EXP & 32) ? 0u : (uint32_t)__builtin_amdgcn_readfirstlane(step * KSTEP * ES));
    };
    // WL: the wave's piece of the step's packed words — LDS bytes [wave * 1024, +1024) of the weight tile = RPP whole rows of BN words;
    // lane l fetches 16 bytes: row wave * RPP + l / CPR, chunk l % CPR.  Read side: word (packed row, column) at row * BN * 4 + column * 4.
    constexpr int CPR = BN / 4, RPP = WL ? 64 / CPR : 1;   // 16-byte chunks per row, rows per piece
    const uint32_t wl_voff = WL ? (uint32_t)(((wave * RPP + lane / CPR) * sw + nt * BN) * 4 + (lane % CPR) * 16) : 0u;
    const uint32_t wl_lds = __builtin_amdgcn_readfirstlane(lds_addr_of(smem) + (uint32_t)(XSTAGE + wave * 1024));
    auto req_wl = [&](int stage, int step) __attribute__((always_inline)) {
        if constexpr (MXW) step = kof(step);
        req_lds16(brW, wl_lds + (uint32_t)(stage * STAGE), wl_voff, (EXP & 32) ? 0u : (uint32_t)step * step_wbytes);
    };
    const int wl_rd = XSTAGE + (wave_row0 + G::HS * h) * (BN * 4) + (cg * 32 + col) * 4;  // this lane's word of packed row 0 of its K part
    auto read_wl = [&](BStep& b, int stage) __attribute__((always_inline)) {
#pragma unroll
        for (int sb = 0; sb < SUB; ++sb)
#pragma unroll
            for (int i = 0; i < WPL; ++i)
                b.w[sb][i] = *(const uint32_t*)(smem + stage * STAGE + wl_rd + (sb * G::ROWS + G::row_of(i)) * (BN * 4));
    };
    // A fragment of slot q = (slice g, row block mi): row mi*32 + col, k = kh*KW + (g/4)*64 + k_of(g%4, h)
    int fbase[NST][NS];
#pragma unroll
    for (int st = 0; st < NST; ++st)
#pragma unroll
        for (int g = 0; g < NS; ++g) {
            const int kb = (kh * KW + (g >> 2) * 64 + G::k_of(g & 3, h)) * ES;  // byte offset inside the row
            const int slot = kb >> 4;
            fbase[st][g] = st * STAGE + col * PITCH + (((slot & ~SWZ) | ((slot ^ (col >> SWZ_SH)) & SWZ)) << 4) + (kb & 15);
        }
    auto read_frag = [&](int stage, int q) __attribute__((always_inline)) -> frag_t {
        return *(const frag_t*)(smem + fbase[stage][q / MI] + (q % MI) * 32 * PITCH);
    };

    typename XO::acc_t accm[MI];  // fp32, or int32 for int8 activations
#pragma unroll
    for (int i = 0; i < MI; ++i)
#pragma unroll
        for (int e = 0; e < 16; ++e) accm[i][e] = 0;

    ConvertX<Tag, XDT> cv;
    uint32_t ev = 0, od = 0;  // codes of the slice being dequantised
    uint32_t qsel1 = 0, qsel2 = 0;  // WBY < 4: the quad transpose's byte selectors of this lane
    if constexpr (WBY != 4) quad_sel<WBY>(lane & 3, qsel1, qsel2);
    // Dequantisation of one slice (-> 4 registers of a B fragment) is cut into pieces that hide behind the MI MFMAs of
    // the slice before it: piece 0 = (scale, zero) of the sub-block + code extraction, then the 4 pairs.
    float mx_sc = 0.f;  // block scale of the sub-block being dequantised (MX)
    auto deq_piece = [&](const BStep& b, int g, int mi, frag_t& out) __attribute__((always_inline)) {
        const int sb = g >> 2, u = g & 3;
        if constexpr (MXW) {
            // e8m0 byte -> fp32 2^(b - 127): the byte IS the exponent field (0 -> 0.0 instead of 2^-127: the quantisers
            // floor the scale at 2^-30)
            if constexpr (NVW) {
                // e4m3 byte -> fp16 (exact: 4 significant bits, 2^-9 .. 448), both halves of a register: slices 0, 1 = the first block
                if (mi == 0 && (u & 1) == 0) {
                    const _Float16 hs = (_Float16)__builtin_amdgcn_cvt_f32_fp8((int)(u < 2 ? b.s[sb] : b.z[sb]), 0);
                    mx_sc = __builtin_bit_cast(float, (h2_t){hs, hs});
                }
            } else if constexpr (NOSC) {
                mx_sc = 1.0f;
            } else if (mi == 0 && u == 0) mx_sc = __builtin_bit_cast(float, b.s[sb] << 23);
#pragma unroll
            for (int j = 0; j < 4; ++j)
                if ((MI == 8 ? j + 1 : (j * MI) / 4) == mi) out[j] = mx_pair<Tag, NBITS>(b.w[sb], u, j, mx_sc);
        } else {
            if (mi == 0) {
                if constexpr (NGS == 1) {
                    if (u == 0) {  // (scale, zero) of the sub-block; slices 1..3 reuse them
                        const float sc = need_s ? TR::to_float((uint16_t)b.s[sb]) : 1.f;
                        const float zr = need_z ? TR::to_float((uint16_t)b.z[sb]) : scalar_zero;
                        cv.set(sc, zr, u13, u4);
                    }
                } else {  // groups of 32: the pair of the slice's group, re-set where it changes (every slice when it depends on the lane half)
                    const int g0 = G::k_of(u, 0) >> 5, g1 = G::k_of(u, 1) >> 5;
                    const int p0 = u == 0 ? -1 : (G::k_of(u - 1, 0) >> 5), p1 = u == 0 ? -1 : (G::k_of(u - 1, 1) >> 5);
                    if (g0 != p0 || g1 != p1) {
                        const uint32_t sraw = g0 == g1 ? (g0 ? b.s2[sb] : b.s[sb]) : (h ? (g1 ? b.s2[sb] : b.s[sb]) : (g0 ? b.s2[sb] : b.s[sb]));
                        const uint32_t zraw = g0 == g1 ? (g0 ? b.z2[sb] : b.z[sb]) : (h ? (g1 ? b.z2[sb] : b.z[sb]) : (g0 ? b.z2[sb] : b.z[sb]));
                        const float sc = need_s ? TR::to_float((uint16_t)sraw) : 1.f;
                        const float zr = need_z ? TR::to_float((uint16_t)zraw) : scalar_zero;
                        cv.set(sc, zr, u13, u4);
                    }
                }
                if constexpr (WBY == 4) {
                    Extract<NBITS>::run(b.w[sb], u, ev, od);
                } else {  // the words this slice reads, regrouped across the quad (a 2-bit word feeds two slices, a 1-bit word four: regrouped each time)
                    uint32_t wq[WPL];
#pragma unroll
                    for (int i = 0; i < WPL; ++i) wq[i] = word_in_slice<NBITS>(i, u) ? quad_word<WBY>(b.w[sb][i], qsel1, qsel2) : 0u;
                    Extract<NBITS>::run(wq, u, ev, od);
                }
                cv.prep(ev, od);
                // opaque to the optimiser: otherwise byte i becomes v_bfe_u32 + v_cvt_f32_ubyte0 instead of one v_cvt_f32_ubyte<i>
                opaque2(ev, od);
            }
#pragma unroll
            for (int j = 0; j < 4; ++j)
                if ((MI == 8 ? j + 1 : (j * MI) / 4) == mi) cv.template put<(NBITS <= 4)>(out, ev, od, j);
        }
    };

    BStep ring[RD];
    frag_t af[L];
    frag_t bfrag[2];

    // ---- prologue: x of step 0, weights of steps 0 .. PD-1 ------------------------------------------------------------
    // request order = the order things are needed: x and weights of step 0 first.  Only the x tile of step 0 is waited
    // for (counted: everything issued after it may still be in flight); the compiler waits for the weights of step 0 where
    // they are first used.
#pragma unroll
    for (int j = 0; j < PIECES; ++j) req_x(0, 0, j);
    if constexpr (WL) req_wl(0, 0);
#pragma unroll
    for (int it = 0; it < NLB; ++it) req_b(ring[0], 0, it);
#pragma unroll
    for (int st = 1; st < NST - 1; ++st) {
#pragma unroll
        for (int j = 0; j < PIECES; ++j) req_x(st, st < nsteps ? st : nsteps - 1, j);
        if constexpr (WL) req_wl(st, st < nsteps ? st : nsteps - 1);
    }
#pragma unroll
    for (int r = 1; r < PD; ++r)
#pragma unroll
        for (int it = 0; it < NLB; ++it) req_b(ring[r], r < nsteps ? r : nsteps - 1, it);
    {
        // requests issued after the weights of step 0 (which follow the x tile of step 0): both have landed behind this wait
        constexpr int AFTER = (NST - 2) * PALL + (PD - 1) * NLB;
        wait_vm<(AFTER < 63 ? AFTER : 63)>();  // (the counter holds 63: with more issued behind it, they have landed anyway)
        tie_b(ring[0]);
    }
    __builtin_amdgcn_s_barrier();
    stamp(1);
    if constexpr (WL) read_wl(ring[0], 0);
#pragma unroll
    for (int mi = 0; mi < MI; ++mi) deq_piece(ring[0], 0, mi, bfrag[0]);
#pragma unroll
    for (int q = 0; q < L; ++q) af[q] = read_frag(0, q);
    __builtin_amdgcn_sched_barrier(0);

    // One K step; J = step & 3 selects the ring slot / stage statically.  The step is written as NQ MFMA "slots"; slot q
    // issues MFMA q, one piece of the next slice's dequantisation, the A fragment needed L slots later and — in the first
    // slots — the step's memory requests: x of step + 1 FIRST (LDS-DMA), then the weights of step + 2.  The order is
    // pinned with sched_barrier (left alone, the machine scheduler pulls every ds_read back to just before its MFMA and
    // groups the requests).  Waits are counted: at slot NQ - L "all but the NLB newest requests" = this step's DMA has
    // landed (the weights just requested stay in flight for another step), then the block barrier: every wave's part of
    // the next stage is in LDS and every wave has finished reading the current stage.
    constexpr int NL = NLB + PALL;
    constexpr int NQI = NQ - L;                       // request slots
    constexpr int RPS = (NL + NQI - 1) / NQI;         // requests per slot
    static_assert((NST - 2) * PALL + (NST - 1) * NLB + NL <= 63, "vmcnt is a 6-bit counter");
    static_assert(!WL || NQI <= (NS - 1) * MI, "WL: the next step's words are read behind the barrier and needed in slot QW");
    auto do_step = [&](auto Jc, int step) __attribute__((always_inline)) {
        constexpr int J = decltype(Jc)::value;
        constexpr int stage = J % NST, stage_next = (J + 1) % NST, stage_fill = (J + NST - 1) % NST;
        const BStep& bc = ring[J];
        BStep& bn = ring[(J + 1) % RD];
        BStep& bl = ring[(J + PD) % RD];
        // The weights of step + 1 (requested PD steps ahead) are first touched in slot QW, by the dequantisation of the next step's
        // first slice.  Behind them in this wave's queue, in the steady state: (PD - 1) whole steps of requests, this step's included
        // (they go out in the slots before QW); in step 0, where they come from the prologue: the weights of steps 2 .. PD - 1 and
        // this step's requests.  The smaller count serves every step (it asks for a few requests of >= 1 step ago on top).
        constexpr int QW = (NS - 1) * MI;
        static_assert(QW * RPS >= NL || QW >= NQI, "the step's requests must be out before the weights of the next step are waited for");
        constexpr int WAITB = (PD - 2) * NLB + NL < 63 ? (PD - 2) * NLB + NL : 63;
        // Past the end of the slice the requests repeat the last step (never consumed): the SGPR offset of a buffer
        // access is not range-checked, so "out of range reads zeros" cannot be relied on; and the last step re-requests
        // its own x tile into the idle stage, which keeps the counted waits identical for every step.
        const int lstep = step + PD < nsteps ? step + PD : nsteps - 1;
        const int xstep = step + NST - 1 < nsteps ? step + NST - 1 : nsteps - 1;
#pragma unroll
        for (int q = 0; q < NQ; ++q) {
            const int g = q / MI, mi = q % MI;
            accm[mi] = XO::mfma(af[q % L], bfrag[g & 1], accm[mi]);
            if (q == NQI && !(EXP & 1)) {
                // everything but the requests issued after the DMA of step + 1: (NST - 2) later DMAs, (NST - 1) weight sets
                wait_vm<(NST - 2) * PALL + (NST - 1) * NLB>();
                __builtin_amdgcn_s_waitcnt(0xC07F);  // lgkmcnt(0): this wave's reads of the current stage are complete
                __builtin_amdgcn_s_barrier();
                asm volatile("" ::: "memory");
                if constexpr (WL) read_wl(bn, stage_next);  // the packed words of step + 1 (the last step reads its own again: never used)
            }
            if (q == QW) {
                wait_vm<WAITB>();
                tie_b(bn);
            }
            if (!(EXP & 2)) {
                if (g + 1 < NS) deq_piece(bc, g + 1, mi, bfrag[(g + 1) & 1]);
                else deq_piece(bn, 0, mi, bfrag[(g + 1) & 1]);  // the next step's first slice
            }
            if (!(EXP & 4)) {
                if (q + L < NQ) af[q % L] = read_frag(stage, q + L);
                else af[q % L] = read_frag(stage_next, q + L - NQ);
            }
#pragma unroll
            for (int it = q * RPS; it < (q + 1) * RPS && it < NL; ++it) {
                if (it < PIECES) { if (!(EXP & 8)) req_x(stage_fill, xstep, it); }
                else if (WL && it == PIECES) { if (!(EXP & 16)) req_wl(stage_fill, xstep); }
                else if (!(EXP & 16)) req_b(bl, lstep, it - PALL);
            }
            __builtin_amdgcn_sched_barrier(0);
        }
    };
    // unrolled by the ring depth: every ring / stage index is static.  Nested ifs, not breaks: the loop has ONE exit, so the
    // accumulators reach the epilogue through one set of registers (with a break per step the int32 accumulators of the
    // int8 variant got a copy per exit edge and spilled)
    auto chain = [&](auto self, auto Jc, int s0) -> void {
        constexpr int J = decltype(Jc)::value;
        do_step(std::integral_constant<int, J % RD>{}, s0 + J);
        if constexpr (J == 0) {
            if (s0 == 0) stamp(2);
        }
        if constexpr (J + 1 < RD) {
            if (s0 + J + 1 < nsteps) self(self, std::integral_constant<int, J + 1>{}, s0);
        }
    };
    // (A loop of whole RD-step groups without exits + a conditional tail was tried: hipcc's waitcnt pass then stops draining the
    //  request queue at the first step of every group — vmcnt(1..2) instead of vmcnt(18) — but the kernel time did not move:
    //  cfgB 44.36 vs 44.37 us, profiles/r02 lab notes.)
    for (int s0 = 0; s0 < nsteps; s0 += RD) chain(chain, std::integral_constant<int, 0>{}, s0);
    // retire every outstanding request (the last step's run-ahead DMA) before the LDS is reused
    wait_vm<0>();
    stamp(3);
    f32x16 acc[MI];  // int32 sums -> fp32 (exact below 2^24)
#pragma unroll
    for (int mi = 0; mi < MI; ++mi)
#pragma unroll
        for (int e = 0; e < 16; ++e) acc[mi][e] = (float)accm[mi][e];

    // ---- epilogue 0 (round 6; K not split over blocks, the K parts of the block fit LDS as [KH][BM][C_PITCH] fp32): EVERY wave drops its partial
    //      tile into LDS in output order, one barrier, and all 512 threads add the KH parts (in part order: the same additions as the path below,
    //      bit for bit) while they read their 16-byte row segments for the store.  The path below hands the partials of waves kh >= 1 to the
    //      NCG waves kh == 0 in fragment order (barrier), lets those 2 .. 4 waves add and transpose alone (barrier), and only then stores: one
    //      more LDS round trip and barrier with a quarter of the block working — ~0.4 of the 1.5 us tail of the unsplit 64 x 64 tiles.
    constexpr bool DIRECT_EPI = KH >= 2 && (KH * BM * C_PITCH * 4 <= 144 * 1024);
    if constexpr (DIRECT_EPI) {
        if (p.splitk == 1 && !(p.flags & GEMLITE_TF_ROUND5_TILE_EPILOGUE)) {  // (else the round-5 epilogue, A/B runs)
            __syncthreads();
            float* parts = (float*)smem;  // [KH][BM][C_PITCH]
#pragma unroll
            for (int mi = 0; mi < MI; ++mi)
#pragma unroll
                for (int e = 0; e < 16; ++e) {
                    const int r = mi * 32 + (e & 3) + 8 * (e >> 2) + 4 * h;
                    parts[(kh * BM + r) * C_PITCH + cg * 32 + col] = acc[mi][e];
                }
            __syncthreads();
            stamp(4);
            const bool typed_o = p.epi.out_dt == TR::DT && (p.epi.meta_dt == TR::DT || p.epi.c_mode == 0 || p.epi.c_mode == 2);
            const int64_t nc0 = (int64_t)nt * BN;
            constexpr int UN = (BM * BN / 4 + 511) / 512;
#pragma unroll
            for (int i = 0; i < UN; ++i) {
                const int u = tid + 512 * i, r = u / (BN / 4), c4 = (u % (BN / 4)) * 4;
                if (r < BM && m0 + r < p.M) {
                    f32x4 v = *(const f32x4*)(parts + r * C_PITCH + c4);
#pragma unroll
                    for (int part = 1; part < KH; ++part) {
                        const f32x4 w = *(const f32x4*)(parts + (part * BM + r) * C_PITCH + c4);
#pragma unroll
                        for (int t = 0; t < 4; ++t) v[t] += w[t];
                    }
                    if (typed_o) store_out4_t<Tag>(p.epi, v, m0 + r, nc0 + c4);
                    else store_out4_any(p.epi, v, m0 + r, nc0 + c4);
                }
            }
            stamp(7);
            return;
        }
    }

    // ---- epilogue 1: add the two K halves (waves 4..7 hand their accumulators to waves 0..3 through LDS) ------------
    __syncthreads();
    if constexpr (KH >= 2) {
        float* xch = (float*)smem;  // [kh - 1][cg][mi][e4][lane][4]
#pragma unroll
        for (int mi = 0; mi < MI; ++mi)
#pragma unroll
            for (int e4 = 0; e4 < 4; ++e4) {
                float* a = xch + (((((kh - 1) * NCG + cg) * MI + mi) * 4 + e4) * 64 + lane) * 4;
                if (kh >= 1) *(f32x4*)a = (f32x4){acc[mi][4 * e4], acc[mi][4 * e4 + 1], acc[mi][4 * e4 + 2], acc[mi][4 * e4 + 3]};
            }
        __syncthreads();
        if (kh == 0) {
#pragma unroll
            for (int part = 1; part < KH; ++part)  // K parts in order: deterministic
#pragma unroll
                for (int mi = 0; mi < MI; ++mi)
#pragma unroll
                    for (int e4 = 0; e4 < 4; ++e4) {
                        const f32x4 v = *(const f32x4*)(xch + (((((part - 1) * NCG + cg) * MI + mi) * 4 + e4) * 64 + lane) * 4);
#pragma unroll
                        for (int t = 0; t < 4; ++t) acc[mi][4 * e4 + t] += v[t];
                    }
        }
    }

    stamp(4);
    constexpr int NOUT = BM * BN;
    const int64_t ncol0 = (int64_t)nt * BN;
    constexpr int PASS_ROWS = BM < C_ROWS ? BM : C_ROWS;
    unsigned* flag = (unsigned*)(smem + PASS_ROWS * C_PITCH * 4);
    constexpr int MIH = (KH == 2 && MI >= 2) ? MI / 2 : MI;  // row blocks per wave in the combine
    bool split_rows = false;                    // combine done: the two K-half waves of a column group share the rows
    // ---- epilogue 2 (K split over blocks): the partial tile travels in FRAGMENT order — slabs are private to this
    //      kernel, so nothing is transposed: waves 0..3 store their registers as 16-byte write-through rows (1 KiB per
    //      wave instruction), and only the last block to arrive goes on: ALL 8 of its waves load the slices' words back
    //      into the same lanes (wave (cg, kh) takes row blocks [kh MIH, kh MIH + MIH)), add them in slice order (run-to-run
    //      deterministic) into the accumulator registers, and hand the sums to the output stage.
    // ---- epilogue 2x (K split over blocks, round 3): REDUCE-SCATTER between the co-resident slices of a tile.  With the slab +
    //      ticket protocol below every block writes its whole partial tile and the last block to arrive reads all of them back
    //      alone (cfgB, 256 x 128 x 4 slices: 4 us of slab stores + 1.5 us ticket + ~9 us of one CU reading 512 KB while its
    //      three peers have left).  Here slice s keeps the row blocks mi = s (mod S) and sends each of the others straight to
    //      its owner's inbox as write-through 16-byte rows in fragment order; every block bumps one arrival counter per peer,
    //      waits until its own counter shows S - 1, pulls the S - 1 partial copies of ITS row blocks into LDS with LDS-DMA (all
    //      pieces in flight at once, no registers), adds them in slice order (bit-identical to the ticket path) and writes its
    //      rows of the output.  (S - 1) / S of the tile leaves and enters every block, all blocks work in parallel, nobody
    //      waits for a ticket round trip.  The planner picks this mode when ALL blocks of the launch fit on the device at once
    //      (tiles x S <= CUs, one block per CU) — a speed rule, not a safety rule: the wait for the peers is bounded and a block
    //      whose peers are late hands its rows over instead of spinning (see the arrival word below), so two such launches
    //      sharing the device (streams, processes) cannot park each other's blocks.
    static_assert(!XCH || (KH == 2 && MI >= 2), "reduce-scatter: row blocks are dealt to the slices");
    if constexpr (XCH == 1) {
        if (p.splitk > 1) {
            const int S = p.splitk, LS = 31 - __builtin_clz((unsigned)S);  // S = 2^LS divides MI
            const int OWB = MI >> LS;                                      // row blocks this block owns
            float* inbox = p.slabs + (int64_t)bid * S * NOUT;             // [owner][from][j][cg][e4][lane] float4
            const __amdgpu_buffer_rsrc_t rs = __builtin_amdgcn_make_buffer_rsrc(inbox, (short)0, S * NOUT * 4, 0x00020000);
            if (kh == 0) {
#pragma unroll
                for (int mi = 0; mi < MI; ++mi) {
                    const int o = mi & (S - 1), j = mi >> LS;
                    if (o != slice) {
                        const int unit = (((o * S + slice) * OWB + j) * 4 + cg) * 4;  // in 1-KiB pieces
#pragma unroll
                        for (int e4 = 0; e4 < 4; ++e4) {
                            const f32x4 v = {acc[mi][4 * e4], acc[mi][4 * e4 + 1], acc[mi][4 * e4 + 2], acc[mi][4 * e4 + 3]};
                            __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(u32x4, v), rs, (unit + e4) * 1024 + lane * 16, 0, 16);  // sc1
                        }
                    }
                }
            }
            stamp(5);
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // the write-through stores have left
            __syncthreads();
            // Arrival word per owner: bits 0..15 = peers that have delivered, bit 16 = "the owner has left".  Nobody waits for a
            // block that may not be running: the owner polls its word for a bounded time only; if a peer is still missing then
            // (another kernel or process holds the CUs its peers need) it stores its OWN partial rows into its inbox, sets the
            // bit and leaves, and the peer that delivers last finds the bit set and finishes those rows on the owner's behalf
            // (`behalf` below) after its own.  The atomics on one word are totally ordered, so exactly one of the two does it.
            constexpr unsigned LEFT = 1u << 16;
            unsigned* cnt = p.counters + (int64_t)bid * S;    // one arrival word per owner
            unsigned* duty = flag;                            // LDS: bit o = finish owner o's rows; bit 31 = I left
            if (tid == 0) *duty = 0u;
            __syncthreads();
            // (the returned value of the arrival is looked at AFTER the own wait: consuming it here would put its round trip in
            //  front of the first poll — measured +2 us at cfgA)
            unsigned prev = 0u;
            if (tid < S && tid != slice) prev = __hip_atomic_fetch_add(cnt + tid, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            bool gave_up = false;
            {
                // ~0.3 us per poll: the usual skew between the slices of a tile is a few us; after ~100 us the peers are not coming soon
                const unsigned polls = (p.flags & GEMLITE_TF_COMBINE_HANDOVER_TEST) ? 1u : 384u;  // give up at once (tests of the hand-over)
                if (tid == 0) {
                    unsigned n = 0;
                    while ((__hip_atomic_load(cnt + slice, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) & 0xffffu) != (unsigned)(S - 1)) {
                        if (++n >= polls) { atomicOr(duty, 1u << 31); break; }
                        __builtin_amdgcn_s_sleep(4);
                    }
                }
                if (tid < S && tid != slice && (prev & LEFT) && (prev & 0xffffu) == (unsigned)(S - 2)) atomicOr(duty, 1u << tid);
                __syncthreads();
                gave_up = (*(volatile unsigned*)duty >> 31) != 0u;
            }
            if (gave_up) {
                // my own partial of MY rows joins the peers' copies in my inbox (slot `slice`), then the word gets the bit
                if (kh == 0) {
#pragma unroll
                    for (int mi = 0; mi < MI; ++mi) {
                        if ((mi & (S - 1)) != slice) continue;
                        const int unit = (((slice * S + slice) * OWB + (mi >> LS)) * 4 + cg) * 4;
#pragma unroll
                        for (int e4 = 0; e4 < 4; ++e4) {
                            const f32x4 v = {acc[mi][4 * e4], acc[mi][4 * e4 + 1], acc[mi][4 * e4 + 2], acc[mi][4 * e4 + 3]};
                            __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(u32x4, v), rs, (unit + e4) * 1024 + lane * 16, 0, 16);  // sc1
                        }
                    }
                }
                asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
                __syncthreads();
                if (tid == 0) {
                    const unsigned prev = __hip_atomic_fetch_or(cnt + slice, LEFT, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                    if ((prev & 0xffffu) == (unsigned)(S - 1)) atomicOr(duty, 1u << slice);  // the last peer came in meanwhile: mine after all
                }
                __syncthreads();
            }
            // rows of owner `ow` from the S copies in its inbox, summed in slice order (the same additions as everywhere else)
            auto behalf = [&](int ow) {
                float* ctb = (float*)smem;
                for (int j = 0; j < OWB; ++j) {
                    __syncthreads();
                    if (kh == 0) {
#pragma unroll
                        for (int e4 = 0; e4 < 4; ++e4) {
                            f32x4 sum = {0.f, 0.f, 0.f, 0.f};
                            for (int f = 0; f < S; ++f) {
                                const int unit = (((ow * S + f) * OWB + j) * 4 + cg) * 4 + e4;
                                const f32x4 v = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(rs, unit * 1024 + lane * 16, 0, 16));  // sc1
#pragma unroll
                                for (int t = 0; t < 4; ++t) sum[t] += v[t];
                            }
#pragma unroll
                            for (int t = 0; t < 4; ++t) {
                                const int e = 4 * e4 + t;
                                ctb[((e & 3) + 8 * (e >> 2) + 4 * h) * C_PITCH + cg * 32 + col] = sum[t];
                            }
                        }
                    }
                    __syncthreads();
                    const bool typed_b = p.epi.out_dt == TR::DT && (p.epi.meta_dt == TR::DT || p.epi.c_mode == 0 || p.epi.c_mode == 2);
                    for (int u = tid; u < 32 * (BN / 4); u += 512) {
                        const int r = u / (BN / 4), c4 = (u % (BN / 4)) * 4;
                        const int m = m0 + (((j << LS) + ow) << 5) + r;
                        if (m < p.M) {
                            const f32x4 v = *(const f32x4*)(ctb + r * C_PITCH + c4);
                            if (typed_b) store_out4_t<Tag>(p.epi, v, m, (int64_t)nt * BN + c4);
                            else store_out4_any(p.epi, v, m, (int64_t)nt * BN + c4);
                        }
                    }
                }
                __syncthreads();
                if (tid == 0) __hip_atomic_store(cnt + ow, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);  // leave it zero
            };
            // (read now: the gather below reuses this part of LDS)
            const unsigned dmask = (unsigned)__builtin_amdgcn_readfirstlane((int)(*(volatile unsigned*)duty & 0xffffu));
            auto duties = [&]() {
                for (int o = 0; o < S; ++o)
                    if ((dmask >> o) & 1u) behalf(o);
            };
            if (gave_up) {  // nothing of mine is left in registers that anybody needs: only duties remain
                duties();
                stamp(7);
                return;
            }
            if (tid == 0) __hip_atomic_store(cnt + slice, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);  // every peer has delivered: leave it zero
            __syncthreads();
            stamp(6);
            // the S - 1 partial copies of the owned row blocks -> LDS behind the output staging tile, as 1-KiB DMA pieces
            const int ct_bytes = (OWB * 32 * C_PITCH * 4 + 1023) & ~1023;
            const int per_from = OWB * 16;  // pieces one peer sent: [j][cg][e4]
            const int npieces = (S - 1) * per_from;
            const srd_t rsI = make_srd(inbox + (int64_t)slice * NOUT, (uint32_t)NOUT * 4u);
            const uint32_t gaddr = lds_addr_of(smem) + (uint32_t)ct_bytes;
            for (int q = wave; q < npieces; q += 8) {
                const int fi = q / per_from, rem = q - fi * per_from, f = fi + (fi >= slice ? 1 : 0);
                req_lds16_sc1(rsI, gaddr + (uint32_t)q * 1024u, (uint32_t)lane * 16u, (uint32_t)__builtin_amdgcn_readfirstlane((f * per_from + rem) * 1024));
            }
            wait_vm<0>();
            __syncthreads();
            float* ct = (float*)smem;  // [OWB * 32][C_PITCH]
            if (kh == 0) {
#pragma unroll
                for (int mi = 0; mi < MI; ++mi) {
                    if ((mi & (S - 1)) != slice) continue;
                    const int j = mi >> LS;
                    // four registers at a time (a 16-register running sum next to the 128 accumulators spilled the 256-row tiles)
#pragma unroll
                    for (int e4 = 0; e4 < 4; ++e4) {
                        f32x4 sum = {0.f, 0.f, 0.f, 0.f};
                        for (int f = 0; f < S; ++f) {  // slice order: bit-identical to the ticket path's sum
                            if (f == slice) {
#pragma unroll
                                for (int t = 0; t < 4; ++t) sum[t] += acc[mi][4 * e4 + t];
                            } else {
                                const int fi = f - (f > slice ? 1 : 0);
                                const f32x4 v = *(const f32x4*)(smem + ct_bytes + (((fi * OWB + j) * 4 + cg) * 4 + e4) * 1024 + lane * 16);
#pragma unroll
                                for (int t = 0; t < 4; ++t) sum[t] += v[t];
                            }
                        }
#pragma unroll
                        for (int t = 0; t < 4; ++t) {
                            const int e = 4 * e4 + t;
                            const int r = j * 32 + (e & 3) + 8 * (e >> 2) + 4 * h;
                            ct[r * C_PITCH + cg * 32 + col] = sum[t];
                        }
                    }
                }
            }
            __syncthreads();
            const bool typed_out_x = p.epi.out_dt == TR::DT && (p.epi.meta_dt == TR::DT || p.epi.c_mode == 0 || p.epi.c_mode == 2);
            const int64_t ncol0x = (int64_t)nt * BN;
            for (int u = tid; u < OWB * 32 * (BN / 4); u += 512) {
                const int r = u / (BN / 4), c4 = (u % (BN / 4)) * 4;
                const int m = m0 + ((((r >> 5) << LS) + slice) << 5) + (r & 31);
                if (m < p.M) {
                    const f32x4 v = *(const f32x4*)(ct + r * C_PITCH + c4);
                    if (typed_out_x) store_out4_t<Tag>(p.epi, v, m, ncol0x + c4);
                    else store_out4_any(p.epi, v, m, ncol0x + c4);
                }
            }
            duties();
            stamp(7);
            return;
        }
    }
    if (!XCH && p.splitk > 1) {
        float* slab = p.slabs + ((int64_t)bid * p.splitk) * NOUT;  // wave-uniform base of this tile's slabs
        const __amdgpu_buffer_rsrc_t rs = __builtin_amdgcn_make_buffer_rsrc(slab, (short)0, p.splitk * NOUT * 4, 0x00020000);
        const int frag0 = (cg * MI * 4 * 64 + lane) * 4;  // float index of (mi = 0, e4 = 0) of this lane inside a slab
        if (kh == 0) {
#pragma unroll
            for (int mi = 0; mi < MI; ++mi)
#pragma unroll
                for (int e4 = 0; e4 < 4; ++e4) {
                    const f32x4 v = {acc[mi][4 * e4], acc[mi][4 * e4 + 1], acc[mi][4 * e4 + 2], acc[mi][4 * e4 + 3]};
                    __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(u32x4, v), rs,
                                                            (slice * NOUT + frag0 + (mi * 4 + e4) * 256) * 4, 0, 16);  // sc1
                }
        }
        stamp(5);
        const bool last = splitk_arrive_is_last(p.counters + bid, p.splitk, flag);
        stamp(6);
        if (!last) return;
        auto gather = [&](auto BASEc) {  // row blocks [BASE, BASE + MIH): sum of all slices, in place
            constexpr int BASE = decltype(BASEc)::value;
#pragma unroll
            for (int j = 0; j < MIH; ++j)
#pragma unroll
                for (int e = 0; e < 16; ++e) acc[BASE + j][e] = 0.f;
            constexpr int CH = MIH > 2 ? 2 : MIH;  // row blocks per round trip (registers: 16 CH words in flight)
            for (int s = 0; s < p.splitk; ++s) {
#pragma unroll
                for (int c = 0; c < MIH; c += CH) {
                    u32x4 t[CH][4];
#pragma unroll
                    for (int j = 0; j < CH; ++j)
#pragma unroll
                        for (int e4 = 0; e4 < 4; ++e4)
                            t[j][e4] = __builtin_amdgcn_raw_buffer_load_b128(
                                rs, (s * NOUT + frag0 + ((BASE + c + j) * 4 + e4) * 256) * 4, 0, 16);
#pragma unroll
                    for (int j = 0; j < CH; ++j)
#pragma unroll
                        for (int e4 = 0; e4 < 4; ++e4) {
                            const f32x4 v = __builtin_bit_cast(f32x4, t[j][e4]);
#pragma unroll
                            for (int tt = 0; tt < 4; ++tt) acc[BASE + c + j][4 * e4 + tt] += v[tt];
                        }
                }
            }
        };
        if (KH == 2 && MI >= 2) {
            split_rows = true;
            if (kh == 0) gather(std::integral_constant<int, 0>{});
            else gather(std::integral_constant<int, ((KH == 2 && MI >= 2) ? MIH : 0)>{});
        } else if (kh == 0) {
            gather(std::integral_constant<int, 0>{});
        }
        if (tid == 0) splitk_reset(p.counters + bid);
    }

    // ---- epilogue 3: the complete tile is transposed through LDS, 128 rows per pass, so that the output moves as 16-byte
    //      row segments; C fragment of a 32x32 MFMA: col = lane & 31, row = (e & 3) + 8 (e >> 2) + 4 (lane >> 5)
    float* ct = (float*)smem;  // [PASS_ROWS][C_PITCH]
    const bool typed_out = p.epi.out_dt == TR::DT && (p.epi.meta_dt == TR::DT || p.epi.c_mode == 0 || p.epi.c_mode == 2);
    constexpr int NPASS = BM / PASS_ROWS, MIP = PASS_ROWS / 32;
    constexpr int UNITS = (PASS_ROWS * BN / 4 + 511) / 512;  // float4 units per thread and pass
#pragma unroll
    for (int ps = 0; ps < NPASS; ++ps) {
        __syncthreads();  // the exchange buffer / the previous pass is no longer read
#pragma unroll
        for (int mi = 0; mi < MIP; ++mi) {
            const int blk = ps * MIP + mi;  // row block of the tile (static)
            const bool mine = split_rows ? ((blk >= MIH) == (kh == 1)) : (kh == 0);
            if (mine) {
#pragma unroll
                for (int e = 0; e < 16; ++e) {
                    const int r = mi * 32 + (e & 3) + 8 * (e >> 2) + 4 * h;
                    ct[r * C_PITCH + cg * 32 + col] = acc[blk][e];
                }
            }
        }
        __syncthreads();
#pragma unroll
        for (int i = 0; i < UNITS; ++i) {
            const int u = tid + 512 * i, r = u / (BN / 4), c4 = (u % (BN / 4)) * 4;
            const int m = m0 + ps * PASS_ROWS + r;
            if (r < PASS_ROWS && m < p.M) {
                const f32x4 v = *(const f32x4*)(ct + r * C_PITCH + c4);
                if (typed_out) store_out4_t<Tag>(p.epi, v, m, ncol0 + c4);
                else store_out4_any(p.epi, v, m, ncol0 + c4);  // output / channel-scale dtype differs from Tag
            }
        }
    }
    stamp(7);
}

// ---------------------------------------------------------------------------------------------------------------
// host-side planning.  tuning[1]: 0 auto | n force split-K n;  tuning[2]: 0 auto | 1/2/4/8 force MI (tile rows / 32)
// ---------------------------------------------------------------------------------------------------------------
typedef void (*mma_kernel_fn)(const WnParams);
// register-path kernels with the reduce-scatter combine: 4- and 2-bit words under 16-bit activations
template <typename Tag, int NBITS>
static const void* mma_pick_xch(int mi) {
    mma_kernel_fn f = nullptr;
    switch (mi) {
        case 8: f = gemm_wn_mma_kernel<Tag, NBITS, 8, 128, 4, 2, 0, 0, 2, 1>; break;
        case 4: f = gemm_wn_mma_kernel<Tag, NBITS, 4, 128, 6, 3, 0, 0, 2, 1>; break;
        case 2: f = gemm_wn_mma_kernel<Tag, NBITS, 2, 256, 6, 3, 0, 0, 2, 1>; break;
        default: break;
    }
    return (const void*)f;
}
// narrow tiles (32 MI x 64, KH = 4): 16-bit activations x 4- / 2-bit words.  variant 0: 64 rows, 256-k steps, 3 stages | 1: 64 rows,
// 512-k steps, 2 stages | 2: 128 rows, 256-k steps, 2 stages, ring of 4 | 3: the same with a ring of 6 | 4: 256 rows, 256-k steps, 2 stages (64 KB each)
template <typename Tag, int NBITS>
static const void* mma_pick_narrow(int variant) {
    mma_kernel_fn f = nullptr;
    switch (variant) {
        case 0: f = gemm_wn_mma_kernel<Tag, NBITS, 2, 256, 6, 3, 0, 0, 4>; break;
        case 1: f = gemm_wn_mma_kernel<Tag, NBITS, 2, 512, 4, 2, 0, 0, 4>; break;
        case 2: f = gemm_wn_mma_kernel<Tag, NBITS, 4, 256, 4, 2, 0, 0, 4>; break;
        case 3: f = gemm_wn_mma_kernel<Tag, NBITS, 4, 256, 6, 2, 0, 0, 4>; break;
        case 4:  // variant 0 with the packed words through LDS (WL, round 6); 4-bit words: 8 KiB per step = one DMA piece per wave
            if constexpr (NBITS == 4) f = gemm_wn_mma_kernel<Tag, NBITS, 2, 256, 6, 3, 0, 0, 4, 0, 1>;
            break;
        default: break;
    }
    return (const void*)f;
}
// 128 x 128 tiles (MI = 4) with the packed words through LDS (WL, round 6): 4-bit words under 16-bit activations, slab + ticket combine
template <typename Tag>
static const void* mma_pick_wl128() {
    mma_kernel_fn f = gemm_wn_mma_kernel<Tag, 4, 4, 128, 6, 3, 0, 0, 2, 0, 1>;
    return (const void*)f;
}
// ... and variant 0 (64 x 64, 256-k steps) for the other geometries of the template (round 4, late): 8-bit activations x 4- / 2-bit
// words, block-scaled / NVFP4 / K-contiguous 8-bit weights under 16-bit activations (8 dwords per lane and sub-block: two stages)
template <typename Tag, int NBITS, int XDT>
static const void* mma_pick_narrow0() {
    mma_kernel_fn f = gemm_wn_mma_kernel<Tag, NBITS, 2, 256, 6, (mma::Geo<NBITS>::WPL == 8 ? 2 : 3), 0, XDT, 4>;
    return (const void*)f;
}
template <typename Tag, int NBITS, int XDT>
static const void* mma_pick_mi(int mi) {
    mma_kernel_fn f = nullptr;  // typed pointer first: a direct cast of the specialisation to void* does not instantiate the host stub
    switch (mi) {
        case 8: f = gemm_wn_mma_kernel<Tag, NBITS, 8, 128, 4, 2, 0, XDT>; break;
        case 4: f = gemm_wn_mma_kernel<Tag, NBITS, 4, 128, 6, 3, 0, XDT>; break;
        // 8 dwords per lane and sub-block (8-bit words, fp8 MX rows): a shallower ring keeps the registers in budget
        case 2: f = gemm_wn_mma_kernel<Tag, NBITS, 2, 256, 6, (mma::Geo<NBITS>::WPL == 8 ? 2 : 3), 0, XDT>; break;
        case 1: f = gemm_wn_mma_kernel<Tag, NBITS, 1, 256, (mma::Geo<NBITS>::WPL == 8 ? 6 : 8), (mma::Geo<NBITS>::WPL == 8 ? 2 : 4), 0, XDT>; break;
        default: break;
    }
    return (const void*)f;
}
// groups of 32 (NGS = 2): 32-row tiles, ring of 4 steps, two x stages (the doubled metadata requests keep the 8-step ring out of the registers)
template <typename Tag, int NBITS, int XDT>
static const void* mma_pick_g32() {
    mma_kernel_fn f = gemm_wn_mma_kernel<Tag, NBITS, 1, 256, 4, 2, 0, XDT, 2, 0, 0, 2>;
    return (const void*)f;
}
template <typename Tag>
static const void* mma_pick(int nbits, int mi, int xdt) {
    if (xdt == GEMLITE_DT_FP8E4) {  // 8-bit activations: the bit widths the reference's A8Wn / BitNet processors produce
        if (nbits == 4) return mma_pick_mi<Tag, 4, GEMLITE_DT_FP8E4>(mi);
        if (nbits == 2) return mma_pick_mi<Tag, 2, GEMLITE_DT_FP8E4>(mi);
        return nullptr;
    }
    if (xdt == GEMLITE_DT_INT8) {
        if (nbits == 4) return mma_pick_mi<Tag, 4, GEMLITE_DT_INT8>(mi);
        if (nbits == 2) return mma_pick_mi<Tag, 2, GEMLITE_DT_INT8>(mi);
        return nullptr;
    }
    switch (nbits) {
        case 4: return mma_pick_mi<Tag, 4, 0>(mi);
        case 2: return mma_pick_mi<Tag, 2, 0>(mi);
        case 1: return mma_pick_mi<Tag, 1, 0>(mi);
        case 8: return mma_pick_mi<Tag, 8, 0>(mi);
        default: return nullptr;
    }
}

// wide tiles (32 MI x 256, KH = 1, 64-k steps): 16-bit activations x 4- / 2-bit words, 128 or 256 rows
template <typename Tag>
static const void* mma_pick_wide(int nbits, int mi) {
    mma_kernel_fn f = nullptr;
    if (nbits == 4) f = mi == 8 ? gemm_wn_mma_kernel<Tag, 4, 8, 64, 4, 2, 0, 0, 1> : gemm_wn_mma_kernel<Tag, 4, 4, 64, 6, 3, 0, 0, 1>;
    else if (nbits == 2) f = mi == 8 ? gemm_wn_mma_kernel<Tag, 2, 8, 64, 4, 2, 0, 0, 1> : gemm_wn_mma_kernel<Tag, 2, 4, 64, 6, 3, 0, 0, 1>;
    return (const void*)f;
}

// 8- / 16-bit packed words (WB = 1 / 2) under 16-bit activations: the register-path forms of the 32-bit words with the same tile, ring and
// stage parameters — kind 0 (nbits 4 / 2 / 1, and 8 in 16-bit words; mi), 1 wide tiles, 4 reduce-scatter combine (nbits 4 / 2; mi), 6 narrow
// tiles variant 0 (nbits 4 / 2).  Compiled in gemm_wn_mma_pw_{f16,bf16}_b{8,16}.hip, one translation unit per (Tag, WB).
template <typename Tag, int NBITS, int WB>
static const void* mma_pick_mi_pw(int mi) {
    mma_kernel_fn f = nullptr;
    constexpr int W8 = mma::Geo<NBITS>::WPL == 8;
    switch (mi) {
        case 8: f = gemm_wn_mma_kernel<Tag, NBITS, 8, 128, 4, 2, 0, 0, 2, 0, 0, 1, WB>; break;
        case 4: f = gemm_wn_mma_kernel<Tag, NBITS, 4, 128, 6, 3, 0, 0, 2, 0, 0, 1, WB>; break;
        case 2: f = gemm_wn_mma_kernel<Tag, NBITS, 2, 256, 6, (W8 ? 2 : 3), 0, 0, 2, 0, 0, 1, WB>; break;
        case 1: f = gemm_wn_mma_kernel<Tag, NBITS, 1, 256, (W8 ? 6 : 8), (W8 ? 2 : 4), 0, 0, 2, 0, 0, 1, WB>; break;
        default: break;
    }
    return (const void*)f;
}
template <typename Tag, int NBITS, int WB>
static const void* mma_pick_xch_pw(int mi) {
    mma_kernel_fn f = nullptr;
    switch (mi) {
        case 8: f = gemm_wn_mma_kernel<Tag, NBITS, 8, 128, 4, 2, 0, 0, 2, 1, 0, 1, WB>; break;
        case 4: f = gemm_wn_mma_kernel<Tag, NBITS, 4, 128, 6, 3, 0, 0, 2, 1, 0, 1, WB>; break;
        case 2: f = gemm_wn_mma_kernel<Tag, NBITS, 2, 256, 6, 3, 0, 0, 2, 1, 0, 1, WB>; break;
        default: break;
    }
    return (const void*)f;
}
template <typename Tag, int NBITS, int WB>
static const void* mma_pick_wide_pw(int mi) {
    mma_kernel_fn f = mi == 8 ? gemm_wn_mma_kernel<Tag, NBITS, 8, 64, 4, 2, 0, 0, 1, 0, 0, 1, WB> : gemm_wn_mma_kernel<Tag, NBITS, 4, 64, 6, 3, 0, 0, 1, 0, 0, 1, WB>;
    return (const void*)f;
}
template <typename Tag, int WB>
static const void* mma_lookup_pw(int kind, int nbits, int mi) {
    switch (kind) {
        case 0:
            switch (nbits) {
                case 4: return mma_pick_mi_pw<Tag, 4, WB>(mi);
                case 2: return mma_pick_mi_pw<Tag, 2, WB>(mi);
                case 1: return mma_pick_mi_pw<Tag, 1, WB>(mi);
                case 8:
                    if constexpr (WB == 2) return mma_pick_mi_pw<Tag, 8, WB>(mi);
                    else return nullptr;
                default: return nullptr;
            }
        case 1:
            if (mi != 4 && mi != 8) return nullptr;
            return nbits == 4 ? mma_pick_wide_pw<Tag, 4, WB>(mi) : (nbits == 2 ? mma_pick_wide_pw<Tag, 2, WB>(mi) : nullptr);
        case 4: return nbits == 4 ? mma_pick_xch_pw<Tag, 4, WB>(mi) : (nbits == 2 ? mma_pick_xch_pw<Tag, 2, WB>(mi) : nullptr);
        case 6:  // mi = variant: 0 only
            if (mi != 0) return nullptr;
            if (nbits == 4) return (const void*)(mma_kernel_fn)gemm_wn_mma_kernel<Tag, 4, 2, 256, 6, 3, 0, 0, 4, 0, 0, 1, WB>;
            if (nbits == 2) return (const void*)(mma_kernel_fn)gemm_wn_mma_kernel<Tag, 2, 2, 256, 6, 3, 0, 0, 4, 0, 0, 1, WB>;
            return nullptr;
        default: return nullptr;
    }
}

// One entry point per Tag (each lives in its own translation unit: gemm_wn_mma_f16.hip / gemm_wn_mma_bf16.hip compile the
// kernel template for one 16-bit type each, in parallel).  kind: 0 register path (nbits, mi, xdt) | 1 wide tiles (nbits, mi) |
// 2 block-scaled weights (nbits = MXW8 / MXW4 / NVW4, mi) | 4 reduce-scatter combine (nbits, mi) | 6 narrow tiles (nbits, variant) | 7 128 x 128 tiles, words through LDS (nbits) | 8 groups of 32, 32-row tiles (nbits, xdt)
#ifdef GL_MMA_EXPERIMENTS
// development builds (make MMA_EXTRA=-DGL_MMA_EXPERIMENTS): the K-loop ablations of the two M = 256 headline kernels, selected by the
// environment variable GEMLITE_DEV_ABLATION: 4-bit words, 64 x 64 narrow tiles (kind 6) and 128 x 128 tiles (kind 0, mi 4; kind 7).  The ablation
// kernels fetch the packed words as register loads: they also stand in for the words-through-LDS variants (kind 6 variant 4, kind 7)
template <typename Tag, int EXP>
static const void* mma_exp_pick(int kind) {
    mma_kernel_fn f = kind == 6 ? gemm_wn_mma_kernel<Tag, 4, 2, 256, 6, 3, EXP, 0, 4> : gemm_wn_mma_kernel<Tag, 4, 4, 128, 6, 3, EXP, 0>;
    return (const void*)f;
}
template <typename Tag>
static const void* mma_exp_lookup(int kind, int exp) {
    switch (exp) {
        case 1: return mma_exp_pick<Tag, 1>(kind);
        case 2: return mma_exp_pick<Tag, 2>(kind);
        case 4: return mma_exp_pick<Tag, 4>(kind);
        case 6: return mma_exp_pick<Tag, 6>(kind);
        case 8: return mma_exp_pick<Tag, 8>(kind);
        case 18: return mma_exp_pick<Tag, 18>(kind);
        case 30: return mma_exp_pick<Tag, 30>(kind);
        case 31: return mma_exp_pick<Tag, 31>(kind);
        default: return nullptr;
    }
}
#endif

template <typename Tag>
static const void* mma_lookup(int kind, int nbits, int mi, int xdt) {
#ifdef GL_MMA_EXPERIMENTS
    if (const int e = dev_ablation(); e && nbits == 4 && xdt == 0 && ((kind == 6 && (mi == 0 || mi == 4)) || (kind == 0 && mi == 4) || kind == 7)) return mma_exp_lookup<Tag>(kind == 6 ? 6 : 0, e);
#endif
    switch (kind) {
        case 0: return mma_pick<Tag>(nbits, mi, xdt);
        case 1: return mma_pick_wide<Tag>(nbits, mi);
        case 2:
            if (nbits == mma::KW8F) return mma_pick_mi<Tag, mma::KW8F, 0>(mi);
            if (nbits == mma::KW8B) return mma_pick_mi<Tag, mma::KW8B, 0>(mi);
            if (nbits == mma::KW8I) return mma_pick_mi<Tag, mma::KW8I, 0>(mi);
            if (nbits == mma::NVW4) {  // NVFP4 weights: fp16 arithmetic only (both operands are exact there)
                if constexpr (std::is_same<Tag, half_tag>::value) return mma_pick_mi<Tag, mma::NVW4, 0>(mi);
                else return nullptr;
            }
            return nbits == mma::MXW8 ? mma_pick_mi<Tag, mma::MXW8, 0>(mi) : mma_pick_mi<Tag, mma::MXW4, 0>(mi);
        case 4: return nbits == 4 ? mma_pick_xch<Tag, 4>(mi) : mma_pick_xch<Tag, 2>(mi);
        case 7: return nbits == 4 ? mma_pick_wl128<Tag>() : nullptr;
        case 8:  // groups of 32
            if (xdt == GEMLITE_DT_FP8E4) return nbits == 4 ? mma_pick_g32<Tag, 4, GEMLITE_DT_FP8E4>() : (nbits == 2 ? mma_pick_g32<Tag, 2, GEMLITE_DT_FP8E4>() : nullptr);
            if (xdt != 0) return nullptr;
            switch (nbits) {
                case 4: return mma_pick_g32<Tag, 4, 0>();
                case 2: return mma_pick_g32<Tag, 2, 0>();
                case 1: return mma_pick_g32<Tag, 1, 0>();
                case 8: return mma_pick_g32<Tag, 8, 0>();
                default: return nullptr;
            }
        case 6:  // mi = variant
            if (xdt == GEMLITE_DT_FP8E4 && mi == 0) return nbits == 4 ? mma_pick_narrow0<Tag, 4, GEMLITE_DT_FP8E4>() : (nbits == 2 ? mma_pick_narrow0<Tag, 2, GEMLITE_DT_FP8E4>() : nullptr);
            if (xdt == GEMLITE_DT_INT8 && mi == 0) return nbits == 4 ? mma_pick_narrow0<Tag, 4, GEMLITE_DT_INT8>() : (nbits == 2 ? mma_pick_narrow0<Tag, 2, GEMLITE_DT_INT8>() : nullptr);
            if (xdt != 0) return nullptr;
            if (nbits == 4) return mma_pick_narrow<Tag, 4>(mi);
            if (nbits == 2) return mma_pick_narrow<Tag, 2>(mi);
            if (mi != 0) return nullptr;
            if (nbits == mma::MXW4) return mma_pick_narrow0<Tag, mma::MXW4, 0>();
            if (nbits == mma::MXW8) return mma_pick_narrow0<Tag, mma::MXW8, 0>();
            if (nbits == mma::KW8F) return mma_pick_narrow0<Tag, mma::KW8F, 0>();
            if (nbits == mma::KW8B) return mma_pick_narrow0<Tag, mma::KW8B, 0>();
            if (nbits == mma::KW8I) return mma_pick_narrow0<Tag, mma::KW8I, 0>();
            if (nbits == mma::NVW4) {
                if constexpr (std::is_same<Tag, half_tag>::value) return mma_pick_narrow0<Tag, mma::NVW4, 0>();
                else return nullptr;
            }
            return nullptr;
        default: return nullptr;
    }
}

}  // namespace gl
