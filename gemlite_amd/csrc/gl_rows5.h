// gl_rows5.h — what the translation units of gemm_w4_rows_kernel share (gemm_wn_rows.hip: the single-layer forms and the description;
// gemm_wn_rows_group.hip: the grouped forms): the MFMA wrappers, the `modes` bits, the LDS layout of a wave and the asm memory requests.
#pragma once
#include <type_traits>

#include "gl_common.h"
#include "gl_async.h"

namespace gl {

namespace rows5 {

template <typename Tag>
__device__ __forceinline__ f32x4 mfma16(u32x4 a, u32x4 b, f32x4 c);
template <>
__device__ __forceinline__ f32x4 mfma16<half_tag>(u32x4 a, u32x4 b, f32x4 c) {
    return __builtin_amdgcn_mfma_f32_16x16x32_f16(__builtin_bit_cast(h8_t, a), __builtin_bit_cast(h8_t, b), c, 0, 0, 0);
}
template <>
__device__ __forceinline__ f32x4 mfma16<bf16_tag>(u32x4 a, u32x4 b, f32x4 c) {
    return __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(b8_t, a), __builtin_bit_cast(b8_t, b), c, 0, 0, 0);
}

// modes: bits 0..3 W_group_mode | 4 zero_is_scalar | 5 pair the half-line tiles on one XCD | 7 channel scales (sp) in the epilogue | 8..15 log2(group)
constexpr uint32_t M_ZSCALAR = 16u, M_PAIR = 32u, M_POST32 = 64u, M_POST = 128u;  // (M_POST32: the epilogue's channel scales are fp32 — BitNet A16W158)
constexpr int NW = 8;                              // waves per block
constexpr int WSLOT_I1 = 272;                      // dword offset of the odd packed rows inside a wave's weight slot (16 dwords of padding: see below)
constexpr int WSLOT_BYTES = 2304;                  // >= (WSLOT_I1 + 256) * 4
constexpr int XBUF = 8192;                         // one x piece: 16 MT rows x 256 / 128 / 64 k
constexpr int WAVE_LDS = 2 * XBUF + WSLOT_BYTES;   // per wave: two x buffers + the weight slot

__device__ __forceinline__ void gld128_nt(u32x4& dst, const char* base, uint32_t voff) {
    asm volatile("global_load_dwordx4 %0, %1, %2 nt" : "=v"(dst) : "v"(voff), "s"(base) : "memory");
}
__device__ __forceinline__ void gld16(uint32_t& dst, const char* base, uint32_t voff) {
    asm volatile("global_load_ushort %0, %1, %2" : "=v"(dst) : "v"(voff), "s"(base) : "memory");
}
template <int N>
__device__ __forceinline__ void wait_vm() { asm volatile("s_waitcnt vmcnt(%0)" ::"n"(N) : "memory"); }
__device__ __forceinline__ void wait_lgkm0() { asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory"); }
__device__ __forceinline__ void tie4(u32x4& v) { asm volatile("" : "+v"(v)); }
__device__ __forceinline__ void tie1(uint32_t& v) { asm volatile("" : "+v"(v)); }

}  // namespace rows5

}  // namespace gl
