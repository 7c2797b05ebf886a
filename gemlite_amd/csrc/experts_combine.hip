// experts_combine.hip — experts_combine_kernel: the routing-weight sum of a mixture-of-experts layer on a BATCH of tokens, in ONE launch
// (gemlite_hip_experts_combine, api.hip).  The rows launches sort the slots by expert, so the top_k slots of a token lie in different
// work blocks and the sum cannot live in the down launch without tickets or atomics; this kernel gathers instead:
//   out[t, n] = round(sum_k w[t spt + k] * float(y[t spt + k, n]))   over the slots k < spt whose id lies in [0, n_experts)
// Numerics — those of GEMLITE_EXPERTS_COMBINE of the decode kernel: every product is an fp32 multiply of its own, then an fp32 add, in
// ascending k from 0.f, one final rounding; nothing is contracted into a fused multiply-add.  A slot with an invalid id (the unsigned
// comparison of dec3::expert_valid: negative, too large, an int64 with a high dword) is skipped — neither its y row nor its weight is
// read; a token without a valid id gets N zeros (+0).
// Grid (ceil(N / (VEC 256)), tokens): a thread holds VEC adjacent columns of one token — 8 (16-byte requests: rows 16-byte aligned) or
// 2 (4-byte requests: what gemlite_hip_forward_experts_rows accepts for its output); the ids and weights of a block are uniform, so they
// are scalar loads.  Four slots are requested before the first is added: memory-bound, the requests of a token overlap.
#include "gl_common.h"
#include "gl_host.h"

namespace gl {

constexpr int COMBINE_THREADS = 256, COMBINE_AHEAD = 4;

// acc + w * y with two roundings (contraction off: the flag travels with the instructions through inlining)
__device__ __forceinline__ float combine_step(float acc, float w, float y) {
#pragma clang fp contract(off)
    const float p = w * y;
    return acc + p;
}

template <typename Tag, bool IDS64, bool W32, typename V>
__global__ __launch_bounds__(COMBINE_THREADS) void experts_combine_kernel(const ExpertsCombineArgs a) {
    using TR = F16Traits<Tag>;
    constexpr int WORDS = sizeof(V) / 4, VEC = WORDS * 2;
    const uint32_t tok = blockIdx.y;
    const uint32_t col = (blockIdx.x * COMBINE_THREADS + threadIdx.x) * VEC;
    if (col >= a.N) return;
    const uint32_t slot0 = tok * a.spt;
    float acc[VEC];
#pragma unroll
    for (int i = 0; i < VEC; ++i) acc[i] = 0.f;
    for (uint32_t k0 = 0; k0 < a.spt; k0 += COMBINE_AHEAD) {
        uint32_t v[COMBINE_AHEAD][WORDS];
        float w[COMBINE_AHEAD];
        bool ok[COMBINE_AHEAD];
#pragma unroll
        for (int i = 0; i < COMBINE_AHEAD; ++i) {
            const uint32_t slot = slot0 + k0 + i;
            ok[i] = false;
            if (k0 + i < a.spt) {
                uint64_t e;
                if constexpr (IDS64) e = (uint64_t)((const int64_t*)a.ids)[slot];
                else e = (uint64_t)(uint32_t)((const int32_t*)a.ids)[slot];
                ok[i] = e < (uint64_t)a.n_experts;
            }
            if (ok[i]) {
                w[i] = W32 ? ((const float*)a.weights)[slot] : TR::to_float(((const uint16_t*)a.weights)[slot]);
                const V row = *(const V*)(a.y + (size_t)slot * a.stride_y + col);
                __builtin_memcpy(v[i], &row, sizeof(V));
            }
        }
#pragma unroll
        for (int i = 0; i < COMBINE_AHEAD; ++i) {
            if (ok[i]) {
#pragma unroll
                for (int q = 0; q < WORDS; ++q) {
                    acc[2 * q] = combine_step(acc[2 * q], w[i], TR::to_float((uint16_t)(v[i][q] & 0xFFFFu)));
                    acc[2 * q + 1] = combine_step(acc[2 * q + 1], w[i], TR::to_float((uint16_t)(v[i][q] >> 16)));
                }
            }
        }
    }
    uint32_t r[WORDS];
#pragma unroll
    for (int q = 0; q < WORDS; ++q) r[q] = (uint32_t)TR::from_float(acc[2 * q]) | ((uint32_t)TR::from_float(acc[2 * q + 1]) << 16);
    V res;
    __builtin_memcpy(&res, r, sizeof(V));
    *(V*)(a.out + (size_t)tok * a.stride_out + col) = res;
}

template <typename Tag, bool IDS64, bool W32>
static const void* combine_pick_v(bool wide) {
    return wide ? (const void*)experts_combine_kernel<Tag, IDS64, W32, u32x4> : (const void*)experts_combine_kernel<Tag, IDS64, W32, uint32_t>;
}
template <typename Tag>
static const void* combine_pick(bool ids64, bool w32, bool wide) {
    if (ids64) return w32 ? combine_pick_v<Tag, true, true>(wide) : combine_pick_v<Tag, true, false>(wide);
    return w32 ? combine_pick_v<Tag, false, true>(wide) : combine_pick_v<Tag, false, false>(wide);
}

// tag 0: fp16, 1: bf16; wide: 16-byte requests (8 columns per thread), else 4-byte requests (2 columns)
const void* experts_combine_fn(int tag, bool ids64, bool w32, bool wide) {
    return tag == 0 ? combine_pick<half_tag>(ids64, w32, wide) : combine_pick<bf16_tag>(ids64, w32, wide);
}
int experts_combine_threads() { return COMBINE_THREADS; }

}  // namespace gl
