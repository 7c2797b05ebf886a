// gemm_wn_rows_group.hip — the GROUPED forms of gemm_w4_rows_kernel (gemm_wn_rows.hip has the description of the kernel): up to ROWS5_GMAX
// independent layers of identical shape, strides, modes, dtype and row count in ONE launch, grid (tiles, members).  Block (tile, y)
// computes member y's tile exactly as that member's own launch would — the body is gemm_wn_rows_kernel.inc with GL_ROWS5_GROUP set: the
// member's five pointers (and its bias) are chosen by blockIdx.y in front of the first memory request, nothing else differs, so every
// member's output is bit-identical to its own launch.  Blocks are dispatched x-fastest: all tiles of a member are placed before the next
// member's, so narrow layers (N / 16 < CUs) spread their members over the CUs a single launch leaves idle and full-width layers run their
// members in successive rounds with no launch boundary between them.  There are no row blocks (grid.y is the member): launches above
// 16 MT rows never group.  Only capture_group.hip launches these forms, by rewriting the kernel node of a stream capture.
//
// A translation unit of its own so that the build stays parallel: one grouped form per form rows5_pick / rows5_bias_pick can return.
#include "gl_rows5.h"
#include "gl_host.h"

namespace gl {

#define GL_ROWS5_GROUP 1
#define GL_ROWS5_KERNEL gemm_w4_rows_group_kernel
#define GL_ROWS5_BIAS 0
#include "gemm_wn_rows_kernel.inc"
#undef GL_ROWS5_KERNEL
#undef GL_ROWS5_BIAS
#define GL_ROWS5_KERNEL gemm_w4_rows_bias_group_kernel
#define GL_ROWS5_BIAS 1
#include "gemm_wn_rows_kernel.inc"
#undef GL_ROWS5_KERNEL
#undef GL_ROWS5_BIAS
#undef GL_ROWS5_GROUP

// The tables of gemm_wn_rows.hip (rows5_pick / rows5_bias_pick), form for form: nullptr where the single-layer table has none
#define GL_ROWS5_GROUP_PICK(PICK, KERNEL)                                                                    \
    template <typename Tag, int MT>                                                                          \
    static const void* PICK##_spg(int spg, int nt, int bits) {                                               \
        if (bits == 2) {                                                                                     \
            if (nt != 1) return nullptr;                                                                     \
            switch (spg) {                                                                                   \
                case 4: return (const void*)KERNEL<Tag, MT, 4, 1, 2>;                                        \
                case 2:                                                                                      \
                    if constexpr (MT <= 2) return (const void*)KERNEL<Tag, MT, 2, 1, 2>;                     \
                    else return nullptr;                                                                     \
                case 1:                                                                                      \
                    if constexpr (MT <= 1) return (const void*)KERNEL<Tag, MT, 1, 1, 2>;                     \
                    else return nullptr;                                                                     \
                default: return nullptr;                                                                     \
            }                                                                                                \
        }                                                                                                    \
        if (nt == 2) {                                                                                       \
            if (spg == 4) return (const void*)KERNEL<Tag, MT, 4, 2>;                                         \
            if constexpr (MT <= 2) {                                                                         \
                if (spg == 2) return (const void*)KERNEL<Tag, MT, 2, 2>;                                     \
            }                                                                                                \
            return nullptr;                                                                                  \
        }                                                                                                    \
        switch (spg) {                                                                                       \
            case 4: return (const void*)KERNEL<Tag, MT, 4>;                                                  \
            case 2: return (const void*)KERNEL<Tag, MT, 2>;                                                  \
            case 1:                                                                                          \
                if constexpr (MT <= 2) return (const void*)KERNEL<Tag, MT, 1>;                               \
                else return nullptr;                                                                         \
            default: return nullptr;                                                                         \
        }                                                                                                    \
    }                                                                                                        \
    template <typename Tag>                                                                                  \
    static const void* PICK(int mt, int spg, int nt, int bits) {                                             \
        switch (mt) {                                                                                        \
            case 1: return PICK##_spg<Tag, 1>(spg, nt, bits);                                                \
            case 2: return PICK##_spg<Tag, 2>(spg, nt, bits);                                                \
            case 3: return PICK##_spg<Tag, 3>(spg, nt, bits);                                                \
            case 4: return PICK##_spg<Tag, 4>(spg, nt, bits);                                                \
            default: return nullptr;                                                                         \
        }                                                                                                    \
    }
GL_ROWS5_GROUP_PICK(rows5_group_pick, gemm_w4_rows_group_kernel)
GL_ROWS5_GROUP_PICK(rows5_bias_group_pick, gemm_w4_rows_bias_group_kernel)
#undef GL_ROWS5_GROUP_PICK

// tag 0: fp16, 1: bf16 (plan_gemm_wn_rows asks once per plan; the answer goes into LaunchPlan::fn_group / fn_bias_group)
const void* gemm_wn_rows_group_fn(int tag, int mt, int spg, int nt, int bits, bool biased) {
    if (biased) return tag == 0 ? rows5_bias_group_pick<half_tag>(mt, spg, nt, bits) : rows5_bias_group_pick<bf16_tag>(mt, spg, nt, bits);
    return tag == 0 ? rows5_group_pick<half_tag>(mt, spg, nt, bits) : rows5_group_pick<bf16_tag>(mt, spg, nt, bits);
}

}  // namespace gl
