// gemv_mx_experts.hip — gemv_mxw4_experts_kernel: the experts of a mixture-of-experts layer with MXFP4 weights (e2m1 codes, one e8m0
// scale byte per 32 k) under fp16 / bf16 activations, as ONE decode launch whose expert ids are read on the GPU
// (gemlite_hip_forward_experts / _fused with layer.input_dtype MXFP16 / MXBF16).  The INT4 member of the family is
// gemv_w4_decode3_experts_kernel (gemv_decode.hip); nothing of its word layout, chunk deal or metadata path applies here: MX weights are
// K-contiguous per output column ([N][K / 2] bytes), their scales one byte per (32-k block, column), stored [K / 32][N].
//
// Grid (N / 16, slots) — GLU: (I / 16, slots), I = N / 2, a block holds gate tile t and up tile t + I / 16 of the slot's expert on the
// slot's x row — and NW = 4 / 8 / 16 waves per block (the planner rule and what it was measured against: api.hip, mx_experts_waves).
//
// Work unit: one 128-byte weight line = 256 k of one column, requested by 8 adjacent lanes, 16 bytes each; a lane's 16 bytes are ONE MX
// block (32 codes, one scale byte).  A wave holds 8 units: the same line of 8 adjacent columns.  The 8-lane group g = tid / 8 keeps
// column g % COLS (COLS = 16, GLU: 32) and is one of GPC = 8 NW / COLS groups of that column; it walks the lines part, part + GPC, ...
// (part = g / COLS, uniform per wave), so an accumulator never changes owner.
//
// The order of the sum is the same for every block size and both epilogues: a column's lines are dealt to PARTS = 8 VIRTUAL parts (line
// j belongs to part j % 8) and a group owns the V = 8 / GPC virtual parts congruent to its own, one fp32 accumulator per lane each.  A
// virtual part's accumulator takes its lines in ascending order, is reduced over its 8 lanes with three cross-lane steps and lands in
// LDS (red[part][column]); behind one barrier wave 0 adds the eight partials of a column in ascending part order.  So a slot's bits
// depend on K, x and the expert alone — not on its place in the grid, the block size, or whether the GLU form computed it.
//
// Requests: the group's first 8 lines (non-temporal: a group owns whole 128-byte lines, the rule of the grouped and experts decode
// launches) go out first, in front of the staging; while a batch of 8 is consumed the next 8 are in flight.
// LDS (dynamic), staged once per block with 16-byte requests:
//   red     [8][COLS] floats
//   x       the slot's row, 2 K bytes, as four REGIONS of K / 2 + 64 bytes: 16-byte piece d (8 k) of MX block b lies at
//           d * (K / 2 + 64) + 16 b.  A unit's 8 lanes hold 8 adjacent blocks, so each of a lane's four ds_read_b128 covers 128
//           contiguous bytes over the unit (conflict-free) and the other 7 units of the wave read the same addresses (broadcast).
//           The 64 bytes between regions spread the four pieces of one block over the banks for the staging WRITES, whose
//           lanes walk the row in memory order (piece p -> region p % 4): with K / 2 = 0 or 128 (mod 256) the regions begin
//           at 0 / 64 / 128 / 192 or 0 / 192 / 128 / 64 bytes (mod 256).
//   scales  [K / 32][COLS] bytes: row r is ONE 16-byte request (GLU: two), 16 adjacent columns of [K / 32][N].  A lane reads the byte
//           of (its block, its column): 8 rows x 8 bytes per wave, in 16 different banks.
// Arithmetic, the same for fp16 and bf16: codes -> pairs at scale 1.0 (v_cvt_scalef32_pk_{f16,bf16}_fp4; e2m1 is exact in both), 16
// v_dot2_f32_{f16,bf16} into a piece-local fp32 sum, acc = fma(2^e, piece_sum, acc) with 2^e = (byte << 23) as fp32 bits — the fp16 rule
// of mx_gemv_kernel (gemm_mx.hip), exact for every e8m0 byte.
// Finish: wave 0 rounds the 16 sums, adds the bias element of row ids[slot] (fetched in front of the barrier; fp32 add on the rounded
// value, rounded once more: "matmul, then out += bias") and stores 32 bytes.  GLU: from_float(silu_f32(g16) * u16) on the members
// rounded that way (gl_common.h: silu_f32).  An id outside [0, n_experts) takes a block-uniform branch in front of any address
// arithmetic: 16 zeros, no barrier.
#include <type_traits>

#include "gl_common.h"
#include "gl_host.h"

namespace gl {

namespace mxe {
constexpr int PARTS = 8;   // virtual parts of a column's lines
constexpr int BATCH = 8;   // lines of a group in flight per buffer
constexpr int XPAD = 64;   // bytes between the x regions

template <typename Tag>
__device__ __forceinline__ float block_dot(const u32x4& wv, const unsigned char* xs, uint32_t xregion) {
    using TR = F16Traits<Tag>;
    float part = 0.f;
#pragma unroll
    for (int d = 0; d < 4; ++d) {
        const u32x4 xv = *(const u32x4*)(xs + d * xregion);
        uint32_t wp[4];
        if constexpr (std::is_same<Tag, half_tag>::value) {
            wp[0] = __builtin_bit_cast(uint32_t, __builtin_amdgcn_cvt_scalef32_pk_f16_fp4(wv[d], 1.0f, 0));
            wp[1] = __builtin_bit_cast(uint32_t, __builtin_amdgcn_cvt_scalef32_pk_f16_fp4(wv[d], 1.0f, 1));
            wp[2] = __builtin_bit_cast(uint32_t, __builtin_amdgcn_cvt_scalef32_pk_f16_fp4(wv[d], 1.0f, 2));
            wp[3] = __builtin_bit_cast(uint32_t, __builtin_amdgcn_cvt_scalef32_pk_f16_fp4(wv[d], 1.0f, 3));
        } else {
            wp[0] = __builtin_bit_cast(uint32_t, __builtin_amdgcn_cvt_scalef32_pk_bf16_fp4(wv[d], 1.0f, 0));
            wp[1] = __builtin_bit_cast(uint32_t, __builtin_amdgcn_cvt_scalef32_pk_bf16_fp4(wv[d], 1.0f, 1));
            wp[2] = __builtin_bit_cast(uint32_t, __builtin_amdgcn_cvt_scalef32_pk_bf16_fp4(wv[d], 1.0f, 2));
            wp[3] = __builtin_bit_cast(uint32_t, __builtin_amdgcn_cvt_scalef32_pk_bf16_fp4(wv[d], 1.0f, 3));
        }
#pragma unroll
        for (int t = 0; t < 4; ++t) part = TR::dot2(wp[t], xv[t], part);
    }
    return part;
}
}  // namespace mxe

template <typename Tag, bool BIASED, bool IDS64, int EPI, int NW>
__global__ __launch_bounds__(NW * 64)
void gemv_mxw4_experts_kernel(const MxExpertsArgs a) {
    using namespace mxe;
    using TR = F16Traits<Tag>;
    constexpr bool GLU = EPI == GEMLITE_EXPERTS_GLU;
    constexpr int COLS = GLU ? 32 : 16, THREADS = NW * 64;
    constexpr int GPC = NW * 8 / COLS, V = PARTS / GPC;
    static_assert(GPC >= 1 && GPC <= PARTS && V * GPC == PARTS && BATCH % V == 0, "groups per column divide the virtual parts");
    extern __shared__ __attribute__((aligned(16))) unsigned char lds[];

    const int tid = threadIdx.x, lane = tid & 63, l8 = lane & 7;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const uint32_t tile = blockIdx.x, slot = blockIdx.y;
    const uint64_t e = dec3::expert_id<IDS64>(a.tail, slot);
    uint16_t* out = a.out + (uint64_t)slot * (uint64_t)a.tail.stride_out;
    if (!dec3::expert_valid(a.tail, e)) {
        if (tid < 16) out[tile * 16 + tid] = 0;
        return;
    }
    const char* wb = a.w + e * (uint64_t)a.tail.stride_w;
    const char* sb = a.s + e * (uint64_t)a.tail.stride_meta;
    const char* xb = a.x + (uint64_t)(slot / a.tail.slots_per_x_row) * (uint64_t)a.tail.stride_x;

    const uint32_t K = a.K, lines = K >> 8, xregion = (K >> 1) + XPAD;
    float* red = (float*)lds;
    unsigned char* xs = lds + PARTS * COLS * 4;
    unsigned char* sc = xs + 4 * xregion;

    // this group: its column of the block, its part, its column of the expert
    const int col = (wave * 8 + (lane >> 3)) % COLS, part = (wave * 8) / COLS;
    const uint32_t n = GLU && col >= 16 ? (tile + a.half_tiles) * 16 + (uint32_t)(col - 16) : tile * 16 + (uint32_t)col;
    const char* wcol = wb + n * a.stride_wn + l8 * 16;
    const int nl = (int)lines > part ? ((int)lines - part + GPC - 1) / GPC : 0;  // lines of this group

    auto request = [&](u32x4 (&w)[BATCH], int i0) {
#pragma unroll
        for (int i = 0; i < BATCH; ++i) {
            w[i] = (u32x4){0u, 0u, 0u, 0u};
            if (i0 + i < nl) w[i] = __builtin_nontemporal_load((const u32x4*)(wcol + (uint32_t)(part + (i0 + i) * GPC) * 128u));
        }
    };
    u32x4 cur[BATCH], nxt[BATCH];
    request(cur, 0);

    // the stage: scale rows, the x row
    for (uint32_t r = tid; r < (K >> 5); r += THREADS) {
        const char* srow = sb + r * a.stride_sg;
        *(u32x4*)(sc + r * COLS) = *(const u32x4*)(srow + tile * 16);
        if constexpr (GLU) *(u32x4*)(sc + r * COLS + 16) = *(const u32x4*)(srow + (tile + a.half_tiles) * 16);
    }
    for (uint32_t p = tid; p < (K >> 3); p += THREADS) *(u32x4*)(xs + (p & 3) * xregion + (p >> 2) * 16) = *(const u32x4*)(xb + p * 16);
    uint16_t bg = 0, bu = 0;
    if constexpr (BIASED) {
        if (wave == 0 && lane < 16) {
            const uint16_t* b = dec3::expert_bias(a.tail, e);
            bg = b[tile * 16 + lane];
            if constexpr (GLU) bu = b[(tile + a.half_tiles) * 16 + lane];
        }
    }
    __syncthreads();

    float acc[V];
#pragma unroll
    for (int v = 0; v < V; ++v) acc[v] = 0.f;
#pragma unroll 1
    for (int i0 = 0; i0 < nl; i0 += BATCH) {
        const bool more = i0 + BATCH < nl;
        if (more) request(nxt, i0 + BATCH);
#pragma unroll
        for (int i = 0; i < BATCH; ++i) {
            if (i0 + i < nl) {
                const uint32_t b = (uint32_t)(part + (i0 + i) * GPC) * 8u + (uint32_t)l8;  // the lane's MX block of this line
                const float sw = __builtin_bit_cast(float, (uint32_t)sc[b * COLS + col] << 23);
                acc[i % V] = __builtin_fmaf(sw, block_dot<Tag>(cur[i], xs + b * 16, xregion), acc[i % V]);
            }
        }
        if (more) {
#pragma unroll
            for (int i = 0; i < BATCH; ++i) cur[i] = nxt[i];
        }
    }
#pragma unroll
    for (int v = 0; v < V; ++v) {
        float s = acc[v];
        s += __shfl_xor(s, 1);
        s += __shfl_xor(s, 2);
        s += __shfl_xor(s, 4);
        if (l8 == 0) red[(part + v * GPC) * COLS + col] = s;
    }
    __syncthreads();
    if (wave == 0 && lane < 16) {
        auto member = [&](int c, uint16_t braw) -> uint16_t {
            float s = red[c];
#pragma unroll
            for (int p = 1; p < PARTS; ++p) s += red[p * COLS + c];
            uint16_t y = TR::from_float(s);
            if constexpr (BIASED) y = TR::from_float(TR::to_float(y) + TR::to_float(braw));
            return y;
        };
        const uint16_t g16 = member(lane, bg);
        if constexpr (GLU) {
            const uint16_t u16 = member(lane + 16, bu);
            out[tile * 16 + lane] = TR::from_float(silu_f32(TR::to_float(g16)) * TR::to_float(u16));
        } else {
            out[tile * 16 + lane] = g16;
        }
    }
}

size_t gemv_mxw4_experts_lds_bytes(int64_t K, bool glu) {
    const int64_t cols = glu ? 32 : 16;
    return (size_t)(mxe::PARTS * cols * 4 + 4 * (K / 2 + mxe::XPAD) + (K / 32) * cols);
}

template <typename F>
static const void* with_bool(bool b, F&& f) {
    return b ? f(std::true_type{}) : f(std::false_type{});
}
template <typename Tag, int EPI, int NW>
static const void* mx_experts_pick(bool biased, bool ids64) {
    return with_bool(biased, [&](auto B) {
        return with_bool(ids64, [&](auto I) { return (const void*)gemv_mxw4_experts_kernel<Tag, B(), I(), EPI, NW>; });
    });
}
template <typename Tag, int EPI>
static const void* mx_experts_pick_waves(int waves, bool biased, bool ids64) {
    return waves == 4 ? mx_experts_pick<Tag, EPI, 4>(biased, ids64)
                      : (waves == 8 ? mx_experts_pick<Tag, EPI, 8>(biased, ids64) : mx_experts_pick<Tag, EPI, 16>(biased, ids64));
}
// tag 0 fp16 | 1 bf16; epilogue 0 | GEMLITE_EXPERTS_GLU; waves 4 / 8 / 16
const void* gemv_mxw4_experts_fn(int tag, int epilogue, bool biased, bool ids64, int waves) {
    if (epilogue == GEMLITE_EXPERTS_GLU)
        return tag == 0 ? mx_experts_pick_waves<half_tag, GEMLITE_EXPERTS_GLU>(waves, biased, ids64)
                        : mx_experts_pick_waves<bf16_tag, GEMLITE_EXPERTS_GLU>(waves, biased, ids64);
    return tag == 0 ? mx_experts_pick_waves<half_tag, 0>(waves, biased, ids64) : mx_experts_pick_waves<bf16_tag, 0>(waves, biased, ids64);
}

}  // namespace gl
