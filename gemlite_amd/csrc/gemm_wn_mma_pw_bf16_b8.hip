// gemm_wn_mma_pw_bf16_b8.hip — the 8-wave MFMA tile kernel (gemm_wn_mma_kernel.inc) for 8-bit packed words, instantiated for bf16_tag: one
// translation unit per (16-bit type, word width) so that the packed-width forms compile in parallel with the 32-bit ones.
#include "gemm_wn_mma_kernel.inc"
#include "gl_host.h"

namespace gl {
const void* mma_lookup_pw_bf16_b8(int kind, int nbits, int mi) { return mma_lookup_pw<bf16_tag, 1>(kind, nbits, mi); }
}  // namespace gl
