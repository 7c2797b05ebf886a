// gemm_wn_rows_experts.hip — the EXPERTS forms of gemm_w4_rows_kernel (gemm_wn_rows.hip has the description of the kernel): the experts of a
// mixture-of-experts layer on a BATCH of tokens, grid (N / 16, Bmax).  experts_route_kernel (experts_route.hip) has sorted the slots by
// expert into work blocks of at most R = 16 MT slots of one expert; block (tile, b) streams that expert's 16 columns ONCE for all its
// slots — the body is gemm_wn_rows_kernel.inc with GL_ROWS5_EXPERTS set: early exit beyond the used count, the expert's bases, gathered x
// rows, scattered output rows, zeros for the invalid bucket.  Nothing else differs and a row of the MFMA result depends on no other
// row, so every valid slot is bit-identical to its row of that expert's own gemm_w4_rows_kernel launch of the same (MT, SPG) form.
// Forms: 4-bit words, NT = 1, MT 1 .. 4 (groups of 32: MT <= 2, registers), biased and unbiased.  Only gemlite_hip_forward_experts_rows
// (api.hip) launches them.
//
// A translation unit of its own so that the build stays parallel.
#include "gl_rows5.h"
#include "gl_host.h"

namespace gl {

#define GL_ROWS5_EXPERTS 1
#define GL_ROWS5_KERNEL gemm_w4_rows_experts_kernel
#define GL_ROWS5_BIAS 0
#include "gemm_wn_rows_kernel.inc"
#undef GL_ROWS5_KERNEL
#undef GL_ROWS5_BIAS
#define GL_ROWS5_KERNEL gemm_w4_rows_bias_experts_kernel
#define GL_ROWS5_BIAS 1
#include "gemm_wn_rows_kernel.inc"
#undef GL_ROWS5_KERNEL
#undef GL_ROWS5_BIAS
#undef GL_ROWS5_EXPERTS

#define GL_ROWS5_EXPERTS_PICK(PICK, KERNEL)                                       \
    template <typename Tag, int MT>                                               \
    static const void* PICK##_spg(int spg) {                                      \
        switch (spg) {                                                            \
            case 4: return (const void*)KERNEL<Tag, MT, 4>;                       \
            case 2: return (const void*)KERNEL<Tag, MT, 2>;                       \
            case 1:                                                               \
                if constexpr (MT <= 2) return (const void*)KERNEL<Tag, MT, 1>;    \
                else return nullptr;                                              \
            default: return nullptr;                                              \
        }                                                                         \
    }                                                                             \
    template <typename Tag>                                                       \
    static const void* PICK(int mt, int spg) {                                    \
        switch (mt) {                                                             \
            case 1: return PICK##_spg<Tag, 1>(spg);                               \
            case 2: return PICK##_spg<Tag, 2>(spg);                               \
            case 3: return PICK##_spg<Tag, 3>(spg);                               \
            case 4: return PICK##_spg<Tag, 4>(spg);                               \
            default: return nullptr;                                              \
        }                                                                         \
    }
GL_ROWS5_EXPERTS_PICK(rows5_experts_pick, gemm_w4_rows_experts_kernel)
GL_ROWS5_EXPERTS_PICK(rows5_bias_experts_pick, gemm_w4_rows_bias_experts_kernel)
#undef GL_ROWS5_EXPERTS_PICK

// tag 0: fp16, 1: bf16; mt = R / 16; spg = 4 / 2 / 1 (groups of >= 128 / 64 / 32).  nullptr: no such form (groups of 32 above 32 rows)
const void* gemm_wn_rows_experts_fn(int tag, int mt, int spg, bool biased) {
    if (biased) return tag == 0 ? rows5_bias_experts_pick<half_tag>(mt, spg) : rows5_bias_experts_pick<bf16_tag>(mt, spg);
    return tag == 0 ? rows5_experts_pick<half_tag>(mt, spg) : rows5_experts_pick<bf16_tag>(mt, spg);
}
size_t gemm_wn_rows_experts_lds_bytes() { return (size_t)rows5::WAVE_LDS * rows5::NW; }

}  // namespace gl
