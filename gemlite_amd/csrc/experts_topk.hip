// experts_topk.hip — experts_topk_kernel: the router's top-k of a mixture-of-experts layer in ONE launch (gemlite_hip_experts_topk,
// api.hip): router logits [tokens, E] in, the top_k expert ids and routing weights [tokens, top_k] out, as the experts launches take them.
// One wave per token, four waves per 256-thread block; no LDS, no atomics, no barrier (a wave without a token leaves at once).
// Lane l holds the experts l, l + 64, ... in registers (PER of them: the kernel is instantiated on 1 / 2 / 4 / 8 / 16, E <= 64 PER).
// Selection — top_k rounds of a wave-wide arg-max over (key, index):
//   * a key is a float mapped to an unsigned word of the same order (order_key): NaN -> 0xFFFFFFFF (above every number, all NaNs equal),
//     -0 -> +0, a number -> its bits with the sign folded, which is >= 0x007FFFFF (-inf).  0 is left for "no candidate": a slot at or
//     past E and a slot whose expert has been selected.  The slot of a winner is retired in its owning lane.
//   * a round is two wave reductions: the greatest key (each lane offers its own greatest, the lower slot on a tie), then the lowest
//     index lane + 64 slot among the lanes that offer it: the greater key wins, among equal keys the lower index.  Both results are
//     wave-uniform (wave_reduce), so the winner's lane and slot are scalars and its value is one v_readlane away.
//   * top_k <= E, so every round has a candidate with a non-zero key: for EVERY bit pattern of logits and bias the ids of a token are
//     distinct and lie in [0, E).  Round r's winner stays in lane r, which stores it: ids come out in selection order.
// Weights (fp32 throughout; fp16 / bf16 logits convert exactly) — `val` is what a slot contributes:
//   softmax: key = val = the logit; m = the first winner's logit (the largest); p = exp(val - m); w = p / sum(p over the selected)
//            (renorm: top_k exponentials) or p / sum(p over all E).
//   sigmoid: val = 1 / (1 + exp(-logit)); key = the logit without a bias (sigmoid is monotone: exact), val + bias with one;
//            w = val, divided by sum(val over the selected) with renorm.  The bias never enters a weight.
//   then w * scale, a multiply of its own.  Sums run lane-local in ascending slot order, then through wave_reduce (one order, every lane
//   gets the same bits).  A 16-bit weight is the fp32 weight rounded once.
#include "gl_common.h"
#include "gl_host.h"

namespace gl {

constexpr int TOPK_THREADS = 256, TOPK_WAVES = TOPK_THREADS / 64;

__device__ __forceinline__ uint32_t order_key(float f) {
    uint32_t u = __builtin_bit_cast(uint32_t, f);
    if ((u & 0x7FFFFFFFu) > 0x7F800000u) return 0xFFFFFFFFu;  // NaN
    if (u == 0x80000000u) u = 0;                              // -0 == +0
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}

// Wave-wide reductions as an inclusive DPP scan whose total lands in lane 63 and is read into a scalar register: row_shr 1, 2, 4, 8 inside
// each row of 16 lanes, then row_bcast:15 into rows 1 and 3, row_bcast:31 into rows 2 and 3.  A lane without a source (the start of a
// row, a masked row) receives IDENTITY.  Six VALU instructions instead of six ds_bpermute round trips; the result is wave-uniform.
struct MaxU32 {
    static constexpr uint32_t IDENTITY = 0;
    static __device__ __forceinline__ uint32_t op(uint32_t a, uint32_t b) { return a > b ? a : b; }
};
struct MinU32 {
    static constexpr uint32_t IDENTITY = 0xFFFFFFFFu;
    static __device__ __forceinline__ uint32_t op(uint32_t a, uint32_t b) { return a < b ? a : b; }
};
struct SumF32 {
    static constexpr uint32_t IDENTITY = 0;  // +0.f
    static __device__ __forceinline__ uint32_t op(uint32_t a, uint32_t b) {
        return __builtin_bit_cast(uint32_t, __builtin_bit_cast(float, a) + __builtin_bit_cast(float, b));
    }
};
template <typename Op, int CTRL, int ROW_MASK>
__device__ __forceinline__ uint32_t dpp_step(uint32_t v) {
    return Op::op(v, (uint32_t)__builtin_amdgcn_update_dpp((int)Op::IDENTITY, (int)v, CTRL, ROW_MASK, 0xF, false));
}
template <typename Op>
__device__ __forceinline__ uint32_t wave_reduce(uint32_t v) {
    v = dpp_step<Op, 0x111, 0xF>(v);  // row_shr:1
    v = dpp_step<Op, 0x112, 0xF>(v);  // row_shr:2
    v = dpp_step<Op, 0x114, 0xF>(v);  // row_shr:4
    v = dpp_step<Op, 0x118, 0xF>(v);  // row_shr:8 — lane 15 of a row holds the row
    v = dpp_step<Op, 0x142, 0xA>(v);  // row_bcast:15 — rows 1 and 3 take in the row before them
    v = dpp_step<Op, 0x143, 0xC>(v);  // row_bcast:31 — rows 2 and 3 take in rows 0 and 1
    return (uint32_t)__builtin_amdgcn_readlane((int)v, 63);
}
__device__ __forceinline__ float wave_sum(float v) { return __builtin_bit_cast(float, wave_reduce<SumF32>(__builtin_bit_cast(uint32_t, v))); }
__device__ __forceinline__ float lane_value(float v, uint32_t lane) {  // (lane: wave-uniform)
    return __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, v), (int)lane));
}

__device__ __forceinline__ float topk_scaled(float w, float scale) {
#pragma clang fp contract(off)
    return w * scale;
}

template <int LDT>
__device__ __forceinline__ float topk_load(const void* row, uint32_t e) {
    if constexpr (LDT == 0) return F16Traits<half_tag>::to_float(((const uint16_t*)row)[e]);
    else if constexpr (LDT == 1) return F16Traits<bf16_tag>::to_float(((const uint16_t*)row)[e]);
    else return ((const float*)row)[e];
}

template <int LDT, int PER>
__global__ __launch_bounds__(TOPK_THREADS) void experts_topk_kernel(const ExpertsTopkArgs a) {
    const uint32_t lane = threadIdx.x & 63u;
    const uint64_t tok = (uint64_t)blockIdx.x * TOPK_WAVES + (threadIdx.x >> 6);
    if (tok >= a.n_tokens) return;
    const char* row = (const char*)a.logits + tok * (uint64_t)a.stride * (LDT == 2 ? 4 : 2);
    const bool sigmoid = a.sigmoid != 0, biased = a.bias != nullptr;

    uint32_t key[PER];
    float val[PER];
#pragma unroll
    for (int i = 0; i < PER; ++i) {
        const uint32_t e = lane + 64u * i;
        key[i] = 0;
        val[i] = 0.f;
        if (e < a.E) {
            const float l = topk_load<LDT>(row, e);
            float k = l;
            val[i] = l;
            if (sigmoid) {
                val[i] = 1.f / (1.f + expf(-l));
                if (biased) k = val[i] + a.bias[e];
            }
            key[i] = order_key(k);
        }
    }

    uint32_t my_id = 0;
    float my_val = 0.f;
    for (uint32_t r = 0; r < a.top_k; ++r) {
        uint32_t bk = key[0], bi = 0;
#pragma unroll
        for (int i = 1; i < PER; ++i)
            if (key[i] > bk) bk = key[i], bi = i;  // (strictly greater: the lower slot of a lane wins a tie)
        const uint32_t kmax = wave_reduce<MaxU32>(bk);  // >= 0x007FFFFF: a candidate is left
        const uint32_t id = wave_reduce<MinU32>(bk == kmax ? lane + 64u * bi : 0xFFFFFFFFu);  // the lowest index among the greatest keys
        const uint32_t owner = id & 63u, slot = id >> 6;  // (wave-uniform)
        float v = 0.f;
#pragma unroll
        for (int i = 0; i < PER; ++i) {
            if ((uint32_t)i == slot) {
                v = val[i];
                if (lane == owner) key[i] = 0;
            }
        }
        v = lane_value(v, owner);
        if (lane == r) my_id = id, my_val = v;
    }

    const bool mine = lane < a.top_k;
    float w;
    if (sigmoid) {
        w = my_val;
        if (a.renorm) w = w / wave_sum(mine ? my_val : 0.f);
    } else {
        const float m = lane_value(my_val, 0);
        const float p = expf(my_val - m);
        float sum;
        if (a.renorm) {
            sum = wave_sum(mine ? p : 0.f);
        } else {
            float s = 0.f;
#pragma unroll
            for (int i = 0; i < PER; ++i)
                if (lane + 64u * i < a.E) s += expf(val[i] - m);
            sum = wave_sum(s);
        }
        w = p / sum;
    }
    w = topk_scaled(w, a.scale);

    if (mine) {
        const uint64_t o = tok * a.top_k + lane;
        if (a.ids64) ((int64_t*)a.ids)[o] = (int64_t)my_id;
        else ((int32_t*)a.ids)[o] = (int32_t)my_id;
        if (a.w_dt == 2) ((float*)a.weights)[o] = w;
        else if (a.w_dt == 0) ((uint16_t*)a.weights)[o] = F16Traits<half_tag>::from_float(w);
        else ((uint16_t*)a.weights)[o] = F16Traits<bf16_tag>::from_float(w);
    }
}

template <int LDT>
static const void* topk_pick(int per_lane) {
    switch (per_lane) {
        case 1: return (const void*)experts_topk_kernel<LDT, 1>;
        case 2: return (const void*)experts_topk_kernel<LDT, 2>;
        case 4: return (const void*)experts_topk_kernel<LDT, 4>;
        case 8: return (const void*)experts_topk_kernel<LDT, 8>;
        case 16: return (const void*)experts_topk_kernel<LDT, 16>;
    }
    return nullptr;
}

// ldt 0: fp16, 1: bf16, 2: fp32 logits; per_lane: experts a lane holds (E <= 64 per_lane)
const void* experts_topk_fn(int ldt, int per_lane) {
    return ldt == 0 ? topk_pick<0>(per_lane) : ldt == 1 ? topk_pick<1>(per_lane) : topk_pick<2>(per_lane);
}
int experts_topk_threads() { return TOPK_THREADS; }

}  // namespace gl
