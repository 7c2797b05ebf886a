// gemm_wn_rows_experts_glu.hip — the GLU forms of gemm_w4_rows_experts_kernel (gemm_wn_rows_experts.hip; gemm_wn_rows.hip has the
// description of the kernel): the gate/up projection of a mixture-of-experts MLP on a BATCH of tokens with SwiGLU in the epilogue, grid
// (I / 16, Bmax), I = N / 2.  Block (t, b) computes tile t (gate) and tile t + I / 16 (up) of work block b of the routed table — the
// body is gemm_wn_rows_kernel.inc with GL_ROWS5_EXPERTS and GL_ROWS5_EXPERTS_GLU set and NT = 2: the expert's two tiles stream once for
// all slots of the block, every x piece read from LDS feeds both, and the thread that holds a (gate, up) pair behind the 8-wave sum
// rounds each as the experts form does and stores from_float(silu(g16) * u16) to the slot's I-wide row.  No [slots, 2 I] intermediate.
// Forms: exactly those of the NT = 2 body that stay free of scratch — groups >= 128 (SPG = 4) with MT 1 .. 4, groups of
// 64 (SPG = 2) with MT 1 .. 2; fp16 and bf16, biased and unbiased.  Groups of 32 have none.  Only gemlite_hip_forward_experts_rows_glu
// (api.hip) launches them.
//
// A translation unit of its own so that the build stays parallel.
#include "gl_rows5.h"
#include "gl_host.h"

namespace gl {

#define GL_ROWS5_EXPERTS 1
#define GL_ROWS5_EXPERTS_GLU 1
#define GL_ROWS5_KERNEL gemm_w4_rows_experts_glu_kernel
#define GL_ROWS5_BIAS 0
#include "gemm_wn_rows_kernel.inc"
#undef GL_ROWS5_KERNEL
#undef GL_ROWS5_BIAS
#define GL_ROWS5_KERNEL gemm_w4_rows_bias_experts_glu_kernel
#define GL_ROWS5_BIAS 1
#include "gemm_wn_rows_kernel.inc"
#undef GL_ROWS5_KERNEL
#undef GL_ROWS5_BIAS
#undef GL_ROWS5_EXPERTS_GLU
#undef GL_ROWS5_EXPERTS

#define GL_ROWS5_GLU_PICK(PICK, KERNEL)                                           \
    template <typename Tag>                                                       \
    static const void* PICK(int mt, int spg) {                                    \
        if (spg == 4) switch (mt) {                                               \
            case 1: return (const void*)KERNEL<Tag, 1, 4, 2>;                     \
            case 2: return (const void*)KERNEL<Tag, 2, 4, 2>;                     \
            case 3: return (const void*)KERNEL<Tag, 3, 4, 2>;                     \
            case 4: return (const void*)KERNEL<Tag, 4, 4, 2>;                     \
        }                                                                         \
        if (spg == 2) switch (mt) {                                               \
            case 1: return (const void*)KERNEL<Tag, 1, 2, 2>;                     \
            case 2: return (const void*)KERNEL<Tag, 2, 2, 2>;                     \
        }                                                                         \
        return nullptr;                                                           \
    }
GL_ROWS5_GLU_PICK(rows5_glu_pick, gemm_w4_rows_experts_glu_kernel)
GL_ROWS5_GLU_PICK(rows5_bias_glu_pick, gemm_w4_rows_bias_experts_glu_kernel)
#undef GL_ROWS5_GLU_PICK

// tag 0: fp16, 1: bf16; mt = R / 16; spg = 4 / 2 (groups of >= 128 / 64).  nullptr: no such form
const void* gemm_wn_rows_experts_glu_fn(int tag, int mt, int spg, bool biased) {
    if (biased) return tag == 0 ? rows5_bias_glu_pick<half_tag>(mt, spg) : rows5_bias_glu_pick<bf16_tag>(mt, spg);
    return tag == 0 ? rows5_glu_pick<half_tag>(mt, spg) : rows5_glu_pick<bf16_tag>(mt, spg);
}

}  // namespace gl
