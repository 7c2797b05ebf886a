// gemv_decode.hip — the M = 1 decode kernel for the short 4-bit shapes (4096 x 4096, 11008 x 4096 ...), round 4.
//
// Replaces gemv_INT_revsplitK_kernel / gemv_INT_kernel / gemv_INT_splitK_kernel (gemlite/triton_kernels/gemv_revsplitK_kernels.py:226-462,
// gemv_kernels.py:230-388, gemv_splitK_kernels.py:240-420) for the shapes gemv_w4_decode_kernel (gemv_wn.hip) took in round 3.  Same
// arithmetic (from the even / odd accumulator split on: without the fp16 pre-scale of x); what changed is everything between "the wave exists" and
// "its first weight request is out", because at 8.9 MB a launch is latency-bound (1.5 us launch boundary + 0.9 us to
// the first bytes + 1.3 us of streaming at the HBM rate + tail):
//   * SCALAR kernel arguments, 14 dwords, compiled with -amdgpu-kernarg-preload-count: the command processor writes them into
//     SGPRs before the wave starts, so address arithmetic begins at the first instruction instead of behind an s_load round trip
//     of the 200-byte parameter struct (the struct kernels wait ~1 HBM/L2 latency there before anything can be requested);
//   * the two weight rows are requested FIRST, then x, scales, zeros (3 % of the bytes; they used to head every wave's queue and the
//     CU's address path takes ~16 cycles per wave-level memory instruction whatever its width);
//   * x: ONE 8-byte load per lane (the wave's 32 packed rows are 512 contiguous bytes of x; quad g holds exactly rows 2g, 2g + 1)
//     instead of two 4-byte loads; the quad exchanges dwords with DPP broadcasts as before;
//   * grid size / tile pairing come in through the arguments: no implicit-argument loads at all.
// 16 waves x 64 lanes, lane (g = lane >> 2, c = lane & 3) owns columns 4c .. 4c + 3 of a 16-column tile and packed rows
// chunk * 512 + wave * 32 + 2 g + {0, 1}.
//
// Four kernels, the form of each spelled in its template parameters.  Three of them are a prologue (the tile, for an expert its id and
// bases, the member's 4 KiB of partial rows), dec3::run_member (one wave's share of one member: requests, Item::run, row sums, partial
// rows) and an epilogue (the bias request, the barrier, finish() or GLU or COMBINE); the grouped kernel has the same items in the same
// order behind its own counted-request ring.  All four share Item, row_sum and finish(), so a layer's, a group member's and an expert
// slot's output is bit-identical to the layer's own launch:
//   kernel                                               argument behind the 14 dwords    launched by
//   gemv_w4_decode3_kernel<Tag, NT, BIASED>              unsigned* counters (timeline) |  the planner: dependent chains, eager and profiled
//                                                        Decode3BiasTail (BIASED)         launches, a group of one.  Wave w runs virtual wave w
//   gemv_w4_decode3_group_kernel<Tag, BIASED, SX, HL,    DecodeNodeTable<BIASED> by value capture_group.hip, by rewriting a capture's node
//                                NT>
//   gemv_w4_decode3_experts_kernel<Tag, BIASED, IDS64>   ExpertsTail by value             gemlite_hip_forward_experts (api.hip): a block per
//                                                                                         (tile, slot), the expert id read on the GPU, then
//                                                                                         as the single-layer kernel
//   gemv_w4_decode3_experts_fused_kernel<Tag, BIASED,    ExpertsFusedTail by value        gemlite_hip_forward_experts_fused (api.hip): several
//                                        IDS64, EPI>                                      (expert, tile) members per block, a wave runs the
//                                                                                         virtual waves decode3_wave_split() gives it; SwiGLU
//                                                                                         or the routing-weight sum in the epilogue
//     BIASED  the bias add in the epilogue (gl_common.h has the arithmetic); the lanes that store ask for their bias element in front of
//             the barrier, so it arrives under the reduction
//     SX      SHARED X, for a group whose members all read the same x.  What a lane derives from x — the pair dwords (x0,x4)(x1,x5)(x2,x6)
//             (x3,x7) of its two rows and the sum of its 16 activations — depends on x alone, and the per-wave-x form derives it again in
//             every quad of every wave of every block: 8 DPP broadcasts, 8 v_perm, 8 dot products and one of five memory requests per
//             item.  Here thread u of a block does it ONCE for the units u, u + 1024, ... < K / 16 (x[16 u .. 16 u + 15], the rows 2 u,
//             2 u + 1), with the same instructions in the same order, and writes 36 bytes to LDS (dynamic: decode3_shared_x_lds_bytes);
//             an item is then four requests and three LDS reads.  The x loads go out first, the wave's first two items behind them, and
//             the counted wait in front of the one extra barrier covers the x loads only: the weight requests stay in flight across it.
//             The members' x pointers are not read.
//     HL      LINES (gl_common.h): H = 1 << HL = 1, 2 or 4 adjacent tiles per wave — its lanes are H sub-waves of 64 / H lanes, sub-wave h
//             on tile t0 + h, lane l' of a sub-wave is (c = l' & 3, gl = l' >> 2) — in H PASSES over each virtual wave, in pass p the row
//             pair g = p * 16 / H + gl.  One request instruction then asks for 8 rows x 128 contiguous bytes (H = 2) or 4 rows x 256
//             (H = 4) where it asked for 16 rows x 64: every 128-byte line of the weights is requested once, by one instruction, and
//             nothing depends on two waves staying in step.  A compile-time constant, so the H = 1 forms are the code they were and the
//             shifts of the others fold (profiles/r18/decode_group_lines.log §1).
// A group: up to DECODE3_GMAX independent layers of identical shape, strides, modes and dtype (capture_group.hip folds back-to-back
// independent launches of a stream capture into one launch).  Grid (N / 16 / TB, Y): block (tile group, y) holds the layers y, y + Y, ... of
// its tiles, all at once: each (layer, tile) slot gets its share of the 16 waves and its own 4 KB of LDS, and the block has ONE barrier (the
// comment at the kernel has the details).  Member count, TB and Y come in `modes`.  Layer 0's pointers are the preloaded scalars; the
// others come out of the by-value table with scalar loads, once per wave.  No timeline probe in a group.
// A NODE holds R >= 1 such groups as ROUNDS (capture_group.hip merges full neighbouring groups; gl_common.h: decode3_round_member): grid
// (N / 16 / TB, Y * R), block row yy is row yy % Y of round yy / Y and works on the members m * round + y + li * Y of the table, m the
// member count of ONE round from `modes`.  R is not in the kernel and gridDim.y is not read; blocks go out x-fastest and one block is
// resident per CU, so a CU takes its block of the next round as soon as its own block leaves.
#include <type_traits>

#include "gl_common.h"
#include "gl_host.h"
#include "gl_async.h"  // gvw: counted asm requests, ring2_run (the grouped kernel)

namespace gl {

namespace dec3 {

template <int CTRL>
__device__ __forceinline__ uint32_t dpp_mov(uint32_t v) {
    return (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, CTRL, 0xF, 0xF, true);
}
template <int CTRL>
__device__ __forceinline__ float dpp_movf(float v) {
    return __builtin_bit_cast(float, dpp_mov<CTRL>(__builtin_bit_cast(uint32_t, v)));
}

// modes: bits 0..3 W_group_mode | 4 zero_is_scalar | 5 pair the half-line tiles on one XCD | 6 timeline probe | 8..15 log2(group)
//        grouped launches only (capture_group.hip; gl_common.h: decode3_group_modes): 16..20 members | 21..22 log2(tiles per block) |
//        23 span placement of the tile groups | 24..31 grid.y of ONE round
constexpr uint32_t M_ZSCALAR = 16u, M_PAIR = 32u, M_PROBE = 64u;
constexpr int R = 2, NW = 16, CHUNK = 32, TC = 16;
constexpr int RED = NW * 4 * TC;  // floats of one partial-row region: [NW * 4 DPP rows][16 columns], 4 KiB

// What a lane holds of one item (a chunk of one virtual wave): its two weight rows, scales, zeros, its 8 bytes of x (per-wave x) ...
struct Chunk { u32x4 w[R]; u32x2 s, z, xq; };
// ... or, shared x, its unit as staged in LDS: the pair dwords of its two rows and the sum of its 16 activations
struct XStage { u32x4 p[R]; float sum; };
struct NoXStage {  // (what Item holds in its place in the per-wave-x forms)
    NoXStage() = default;
    __device__ NoXStage(const XStage&) {}
};
// The arithmetic of one item, added to tot[4] (the lane's four columns), and what it reads besides the item: references to the kernel's own
// variables, as a lambda would capture them.  (A closure, not a function of values: hipcc simplifies a callee before it inlines it, and
// this shape keeps every kernel's registers, LDS and occupancy what they were — profiles/r19/group_refactor.log.  After a compiler bump
// rerun scripts/compare_kernel_asm.py --by-body against the previous build: its "resources" line is the check.)
template <typename Tag, bool SX>
struct Item {
    using TR = F16Traits<Tag>;
    static constexpr bool SUBN = TR::DT == GEMLITE_DT_FP16;
    static constexpr int WP = SUBN ? 2 : 1;  // 4-bit fields per 16-bit window (Window<Tag, 4>::WP of gemv_wn.hip)
    static constexpr float QSCALE = SUBN ? 16777216.0f : 1.0f;
    std::conditional_t<SX, const XStage&, NoXStage> xs;
    const uint32_t (&wmask)[WP];   // (15u * 0x00010001u) << (4 * i)
    const bool &need_s, &need_z;
    const float &scalar_zero, &bz;  // bz: -1 / 1 / 0 by W_group_mode
    const bool& b_times_s;
    float (&tot)[4];

    // FULL: the caller knows need_s && need_z (the grouped loop's common case), the two selects are compiled out
    template <bool FULL>
    __device__ void run(const Chunk& ck) const {
        // fp16: the second field of a 16-bit window is read 4 bits up (16 q * 2^-24 as an fp16 subnormal).  Its products go to their
        // own accumulator and the 2^-4 is applied ONCE to the fp32 sum, so nothing is ever rounded: rounds 2-3 (and the first decode3)
        // scaled the matching x pairs by 2^-4 in fp16 instead, which lost mantissa bits for |x| < 2^-10 (1.8e-3 of mean |y|
        // at |x| ~ 1e-4, tests/test_gpu_parity.py::test_small_magnitude_fp16_activations_on_the_decode_kernels)
        float acc[WP][4];
#pragma unroll
        for (int wi = 0; wi < WP; ++wi)
#pragma unroll
            for (int j = 0; j < 4; ++j) acc[wi][j] = 0.f;
        float xsum = 0.f;
        // quad lane j holds dwords (2 (j & 1), 2 (j & 1) + 1) of row j >> 1: row i's dwords d0..d3 = (x0x1)(x2x3)(x4x5)(x6x7)
        uint32_t a0 = 0, a1 = 0, a2 = 0, a3 = 0, b0 = 0, b1 = 0, b2 = 0, b3 = 0;
        if constexpr (!SX) {
            a0 = dpp_mov<0x00>(ck.xq[0]), a1 = dpp_mov<0x00>(ck.xq[1]), a2 = dpp_mov<0x55>(ck.xq[0]), a3 = dpp_mov<0x55>(ck.xq[1]);
            b0 = dpp_mov<0xAA>(ck.xq[0]), b1 = dpp_mov<0xAA>(ck.xq[1]), b2 = dpp_mov<0xFF>(ck.xq[0]), b3 = dpp_mov<0xFF>(ck.xq[1]);
        }
#pragma unroll
        for (int i = 0; i < R; ++i) {
            const uint32_t d0 = i ? b0 : a0, d1 = i ? b1 : a1, d2 = i ? b2 : a2, d3 = i ? b3 : a3;
            uint32_t xr[4];  // pairs (x0,x4)(x1,x5)(x2,x6)(x3,x7)
            if constexpr (SX) {
#pragma unroll
                for (int dd = 0; dd < 4; ++dd) xr[dd] = xs.p[i][dd];
            } else {
                xr[0] = __builtin_amdgcn_perm(d2, d0, 0x05040100u);
                xr[1] = __builtin_amdgcn_perm(d2, d0, 0x07060302u);
                xr[2] = __builtin_amdgcn_perm(d3, d1, 0x05040100u);
                xr[3] = __builtin_amdgcn_perm(d3, d1, 0x07060302u);
#pragma unroll
                for (int dd = 0; dd < 4; ++dd) xsum = TR::dot2(xr[dd], TR::ONES2, xsum);
            }
#pragma unroll
            for (int dd = 0; dd < 4; ++dd) {
                const int win = dd / WP, wi = dd % WP;
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    uint32_t h = (ck.w[i][j] >> (4 * WP * win)) & wmask[wi];
                    if constexpr (!SUBN) h |= TR::MAGIC2;
                    acc[wi][j] = TR::dot2(h, xr[dd], acc[wi][j]);
                }
            }
        }
        if constexpr (SX) xsum = xs.sum;  // (the same chain of eight dot products from 0.f, run once per block)
        const uint32_t s0 = ck.s[0], s1 = ck.s[1], z0 = ck.z[0], z1 = ck.z[1];
        float s[4] = {TR::to_float((uint16_t)(s0 & 0xFFFFu)), TR::to_float((uint16_t)(s0 >> 16)), TR::to_float((uint16_t)(s1 & 0xFFFFu)), TR::to_float((uint16_t)(s1 >> 16))};
        float z[4] = {TR::to_float((uint16_t)(z0 & 0xFFFFu)), TR::to_float((uint16_t)(z0 >> 16)), TR::to_float((uint16_t)(z1 & 0xFFFFu)), TR::to_float((uint16_t)(z1 >> 16))};
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            if constexpr (!FULL) {
                if (!need_s) s[j] = 1.f;
                if (!need_z) z[j] = scalar_zero;
            }
            const float a = s[j] * QSCALE;
            const float b = bz * z[j] * (b_times_s ? s[j] : 1.f);
            float v = acc[0][j];
            if constexpr (WP > 1) v = __builtin_fmaf(acc[WP - 1][j], 1.0f / 16.0f, v);
            if constexpr (!SUBN) v -= TR::OFF * xsum;
            // (spelled out: left to -ffp-contract, hipcc chose fma(b, xsum, a v) in one instantiation and fma(a, v, b xsum) in another,
            // and a group's outputs must be bit-identical to the single-layer kernel's)
            tot[j] += __builtin_fmaf(b, xsum, a * v);
        }
    }
};

// The 4 row sub-groups of every 16-lane DPP row (lane bits 2, 3): two rotations, every lane ends with the row's sum
__device__ __forceinline__ float row_sum(float v) {
    v += dpp_movf<0x124>(v);  // row_ror:4
    v += dpp_movf<0x128>(v);  // row_ror:8
    return v;
}

// One wave sums the 64 partial rows of a 4 KiB region and stores the tile's 16 outputs (braw: the bias element of lane < 16).
// STORE = false: no store; -> the rounded 16-bit output of column lane & 15, in every lane, for an epilogue that goes on with it
// (Red: the region as the kernel names it — the kernel's own array, or a pointer into it)
template <typename Tag, bool BIASED, bool STORE = true, typename Red>
__device__ __forceinline__ auto finish(const Red& red, uint16_t braw, uint16_t* out, int tile) {
    using TR = F16Traits<Tag>;
    const int lane = threadIdx.x & 63;
    constexpr int PER = NW;  // partial rows per lane quarter: 4 NW rows over 4 quarters
    const int o = lane & 15, part = lane >> 4;
    float v = 0.f;
#pragma unroll
    for (int r = 0; r < PER; ++r) v += red[(part * PER + r) * TC + o];
    v += __shfl_xor(v, 16);
    v += __shfl_xor(v, 32);
    uint16_t h = TR::from_float(v);
    // (two roundings, as the matmul launch followed by torch's add has them; a sum of two converted values: nothing to contract)
    if constexpr (BIASED) h = TR::from_float(TR::to_float(h) + TR::to_float(braw));
    if constexpr (STORE) {
        if (lane < 16) out[tile * TC + o] = h;
    } else {
        return h;
    }
}
template <typename Tag, bool BIASED, typename Red>
__device__ __forceinline__ uint16_t finish_value(const Red& red, uint16_t braw) {
    return finish<Tag, BIASED, false>(red, braw, nullptr, 0);
}

// Block b's tile, one tile per block.  M_PAIR: adjacent half-line tiles on one XCD (speed only; any mapping is correct)
__device__ __forceinline__ int pair_tile(uint32_t modes, int b) {
    if (!(modes & M_PAIR)) return b;
    const int xcd = b & 7, idx = b >> 3;
    return (((idx >> 1) << 3) + xcd) * 2 + (idx & 1);
}

// One wave's share of one MEMBER — a layer, or an expert's tile: the member's virtual waves [v0, v1), where virtual wave v is the chunks
// v, v + 16, ... below nch_total (chunk gc: the packed rows gc * 32 .. gc * 32 + 31 and their 512 bytes of x).  The wave's items — its
// virtual waves in ascending order, each one's chunks in ascending order — are a flat list of known length, run through two chunk
// buffers: the first two requests, then per item the arithmetic (Item::run<false>) and the request of the item after the next.  `tot` adds a
// virtual wave's chunks in ascending order; at its end the two row_ror sums, the partial row v * 4 + (lane >> 4) of the member's 4 KiB
// region `rd`, `tot` back to zero; a virtual wave without a chunk writes zeros (K < 4096).  So a member's region, and what finish() makes
// of it, is the same bits whichever kernel ran it and however its virtual waves were dealt to the block's waves.
//   NT     non-temporal weight loads
//   ONE    v1 == v0 + 1: no cursors, no wrap test per item, one flush
//   probe  probe(1) behind the first two requests, probe(2) behind the last item (the single-layer kernel's timeline stamps)
// The four bases are the member's own (uniform: SGPR pairs); the offsets inside a member are 32-bit.
template <typename Tag, bool NT, bool ONE, typename Probe>
__device__ __forceinline__ void run_member(const char* wb, const char* xb, const char* sp, const char* zp, uint32_t sw4, uint32_t mstride2,
                                           int nch_total, uint32_t modes, int tile, int v0, int v1, float* rd, const Probe& probe) {
    const int lane = threadIdx.x & 63, c = lane & 3, g = lane >> 2;
    const uint32_t n0 = (uint32_t)(tile * TC + c * 4);
    const int w_mode = (int)(modes & 15u), gs_shift = (int)((modes >> 8) & 255u);
    const bool need_s = w_mode >= 2, need_z = (w_mode == 1 || w_mode >= 3) && !(modes & M_ZSCALAR);

    const uint32_t row0 = (uint32_t)(v0 * CHUNK + g * R);  // this lane's first row of chunk v0
    const uint32_t wo0 = row0 * sw4 + n0 * 4u;
    const uint32_t xo0 = (uint32_t)(v0 * CHUNK) * 16u + (uint32_t)lane * 8u;  // a chunk's 512 bytes of x, 8 per lane
    // chunk v0 + d of the member
    auto load_chunk = [&](Chunk& ck, int d) {
        const uint32_t wo = wo0 + (uint32_t)(d * CHUNK) * sw4;
#pragma unroll
        for (int i = 0; i < R; ++i) {
            const u32x4* src = (const u32x4*)(wb + (wo + (uint32_t)i * sw4));
            ck.w[i] = NT ? __builtin_nontemporal_load(src) : *src;
        }
        ck.xq = *(const u32x2*)(xb + (xo0 + (uint32_t)(d * CHUNK) * 16u));
        const uint32_t row = row0 + (uint32_t)(d * CHUNK);
        const uint32_t mo = (uint32_t)((row * 8u) >> gs_shift) * mstride2 + n0 * 2u;
        // (absent metadata is still "loaded" — from the member's weights, always in bounds — so the loop stays branch-free)
        ck.s = *(const u32x2*)((need_s ? sp : wb) + (need_s ? mo : 0u));
        ck.z = *(const u32x2*)((need_z ? zp : wb) + (need_z ? mo : 0u));
    };
    // items of this wave (a virtual wave >= nch_total has none)
    int n;
    if constexpr (ONE) {
        n = (nch_total - v0 + NW - 1) / NW;
    } else {
        const int nv = v1 - v0, rem = (nch_total & (NW - 1)) - v0;
        n = (nch_total / NW) * nv + (rem < 0 ? 0 : (rem > nv ? nv : rem));
    }
    int rv = v0, rgc = v0;  // request cursor: virtual wave, chunk (ONE: item i is chunk v0 + 16 i)
    auto request = [&](Chunk& ck, int i) {
        if constexpr (ONE) {
            load_chunk(ck, i * NW);
        } else {
            load_chunk(ck, rgc - v0);
            rgc += NW;
            if (rgc >= nch_total) rgc = ++rv;
        }
    };
    Chunk cur, nxt;
    if (n > 0) request(cur, 0);
    if (n > 1) request(nxt, 1);
    probe(1);

    float tot[4] = {0.f, 0.f, 0.f, 0.f};
    const float scalar_zero = (modes & M_ZSCALAR) ? (float)((const int32_t*)zp)[0] : 0.f;
    const float bz = (w_mode == 1 || w_mode == 3) ? -1.f : (w_mode == 4 ? 1.f : 0.f);
    const bool b_times_s = w_mode == 3;
    uint32_t wmask[Item<Tag, false>::WP];
#pragma unroll
    for (int i = 0; i < Item<Tag, false>::WP; ++i) wmask[i] = (15u * 0x00010001u) << (4 * i);
    const Item<Tag, false> item{{}, wmask, need_s, need_z, scalar_zero, bz, b_times_s, tot};
    // a virtual wave's end: DPP row sums, the partial row to the member's region
    auto flush = [&](int v) {
#pragma unroll
        for (int j = 0; j < 4; ++j) tot[j] = row_sum(tot[j]);
        if ((lane & 12) == 0) *(f32x4*)(rd + ((v * 4 + (lane >> 4)) * TC + c * 4)) = (f32x4){tot[0], tot[1], tot[2], tot[3]};
#pragma unroll
        for (int j = 0; j < 4; ++j) tot[j] = 0.f;
    };
    int cv = v0, cgc = v0;  // compute cursor
#pragma unroll 1
    for (int it = 0; it < n; ++it) {
        item.template run<false>(cur);
        if constexpr (!ONE) {
            cgc += NW;
            if (cgc >= nch_total) {
                flush(cv);
                cgc = ++cv;
            }
        }
        if (it + 1 < n) {
            cur = nxt;
            if (it + 2 < n) request(nxt, it + 2);
        }
    }
    probe(2);
    if constexpr (ONE) {
        flush(v0);
    } else {
#pragma unroll 1
        for (int v = cv; v < v1; ++v) flush(v);  // virtual waves without a chunk still write their rows
    }
}

// An experts launch, the prologue of a member.  The id of a slot is a SCALAR load (uniform per wave; int32 or int64 as the router wrote
// it); an id outside [0, n_experts) is never turned into an address
template <bool IDS64>
__device__ __forceinline__ uint64_t expert_id(const ExpertsTail& t, uint32_t slot) {
    // (int32: a negative id is >= 2^31 as unsigned and n_experts is below 2^31; int64: the high dword takes part in the comparison)
    if constexpr (IDS64) {
        return (uint64_t)((const int64_t*)t.ids)[slot];
    } else {
        return (uint64_t)(uint32_t)((const int32_t*)t.ids)[slot];
    }
}
__device__ __forceinline__ bool expert_valid(const ExpertsTail& t, uint64_t e) { return e < (uint64_t)t.n_experts; }
// Expert e's bases: base + e * stride in 64-bit scalar arithmetic (a stacked tensor is far beyond 4 GiB; the offsets inside an expert
// stay 32-bit), and the x row of the slot
__device__ __forceinline__ void expert_bases(const ExpertsTail& t, uint64_t e, uint32_t slot, uint32_t modes, const char*& wb,
                                             const char*& xb, const char*& sp, const char*& zp) {
    wb += e * (uint64_t)t.stride_w;
    sp += e * (uint64_t)t.stride_meta;
    if (!(modes & M_ZSCALAR)) zp += e * (uint64_t)t.stride_meta;  // (one scalar zero is shared by all experts)
    xb += (uint64_t)(slot / t.slots_per_x_row) * (uint64_t)t.stride_x;
}
__device__ __forceinline__ const uint16_t* expert_bias(const ExpertsTail& t, uint64_t e) {
    return (const uint16_t*)((const char*)t.bias + e * (uint64_t)t.stride_bias);
}

}  // namespace dec3

template <typename Tag, bool NT, bool BIASED = false>
__global__ __launch_bounds__(1024, 1)
void gemv_w4_decode3_kernel(const char* wb, const char* xb, const char* sp, const char* zp, uint16_t* out,
                            uint32_t sw4, uint32_t mstride2, int nch_total, uint32_t modes,
                            const std::conditional_t<BIASED, Decode3BiasTail, unsigned*> counters) {
    using namespace dec3;
    __shared__ __attribute__((aligned(16))) float red[RED];

    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int tile = pair_tile(modes, (int)blockIdx.x);
    // opt-in timeline (GEMLITE_TF_TIMELINE): the mode bit is a preloaded SGPR, so a normal launch never touches `counters` (the one
    // argument behind the preloaded 14 dwords) and never waits for a kernarg load
    auto stamp = [&](int i) {
        if constexpr (!BIASED) {
            if (__builtin_expect((modes & M_PROBE) != 0u, 0)) {
                if (counters && wave == 0 && lane == 0 && blockIdx.x < 1024)
                    ((unsigned long long*)(counters + MAX_SPLITK_COUNTERS))[blockIdx.x * 4 + i] = __builtin_amdgcn_s_memrealtime();
            }
        }
    };
    stamp(0);
    run_member<Tag, NT, true>(wb, xb, sp, zp, sw4, mstride2, nch_total, modes, tile, wave, wave + 1, red, stamp);
    uint16_t braw = 0;
    if constexpr (BIASED) {
        if (wave == 0 && lane < 16) braw = counters.bias[tile * TC + lane];
    }
    __syncthreads();
    if (wave == 0) finish<Tag, BIASED>(red, braw, out, tile);
    stamp(3);
}

// One block holds the layers y, y + Y, ... of its 16-column tile — LB of them, ALL in flight at once: decode3_wave_split()
// (gl_common.h) gives every layer 16 / LB waves, and a wave takes the place of a contiguous run of the single-layer kernel's waves
// ("virtual waves": virtual wave v is the chunks v, v + 16, ... below nch_total, each with the rows and x bytes the single-layer
// wave v reads).  Nothing orders the waves of a block before the one barrier at the end, so a CU's waves wait for memory and do
// arithmetic at different times.  A wave's items — its virtual waves in ascending order, each one's chunks in ascending order — are
// a flat list of known length: gvw::ring2_run (gl_async.h) with five counted asm requests per item (w, w, x, s, z).  Every base is
// a uniform SGPR pair moved by scalar arithmetic, every per-lane offset is set up once: the loop holds no vector address
// arithmetic and no select (the shared-x forms: four requests (w, w, s, z) and three LDS reads per item, whose two lane addresses
// move by one vector add each).  Bit-exact: `tot` accumulates a virtual wave's chunks in ascending order; at its end the two row_ror
// sums, the partial row v * 4 + (lane >> 4) of the LAYER'S OWN 4 KB of LDS, `tot` back to zero (a virtual wave without a chunk
// writes zeros: K < 4096); after the barrier waves 0 .. LB - 1 each run the single-layer epilogue on one layer's region.
// With tile groups (TB = 1 << tbl tiles per block) the block's LB * TB slots stand where the layers stand in this description:
// slot s is layer s / TB on tile s % TB of the block's group, with its own waves, virtual waves and 4 KB of LDS.
// With lines (H = 1 << HL tiles per wave) the waves share the block's slots / H wave-slots instead; a
// wave's items are (virtual wave, pass, chunk) ascending, H times as many on a 1 / H share of the waves, and sub-wave h of the
// lanes fills slot + h.  Per lane an item is the same item(); `tot` of a (virtual wave, pass) adds its chunks in ascending
// order; the four row pairs 4 r .. 4 r + 3 still meet in one 16-lane DPP row (r = p * 4 / H + the row inside the sub-wave) and
// land in partial row v * 4 + r of the slot's region: bit-exact under every H.  What depended on g depends on the pass through
// SCALAR adds to the uniform bases (weights, x, metadata row) and one constant inside the shared-x LDS offsets.
// NT: non-temporal weight requests, H = 2 and 4 only (gl_common.h: decode3_group_nt has the rule; x, scales and zeros keep the default
// policy — several waves of a block share those lines).  With whole lines per request no weight line is asked for twice and the L2 has
// nothing to keep: the bytes fetched are unchanged, a request is outstanding 11 % shorter (profiles/r24/decode_group_policy.log §c).
// H = 1 stays default-policy by construction: the two 16-column tiles of a 128-byte line are read by two different waves — with one
// tile per block (TB = 1) in two blocks on two CUs of one XCD, which meet in that XCD's L2 only; with tile groups by neighbouring waves of
// one block — and nothing keeps the two in step: the partner asks for its half some time later, and a non-temporal line has left the L2
// by then (11.6 MB fetched per layer against 9.5; profiles/r13/decode_group_waves.log §2).
template <typename Tag, bool BIASED, bool SX, int HL, bool NT>
__global__ __launch_bounds__(1024, DECODE3_GROUP_WAVES_PER_SIMD)
void gemv_w4_decode3_group_kernel(const char* wb, const char* xb, const char* sp, const char* zp, uint16_t* out,
                                  uint32_t sw4, uint32_t mstride2, int nch_total, uint32_t modes,
                                  const DecodeNodeTable<BIASED> tab) {
    using namespace dec3;
    using TR = F16Traits<Tag>;
    constexpr int hl = HL, H = 1 << hl;

    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int c = lane & 3;
    // the block's tile group and this wave's slot = (block-local layer, tile of the group); gl_common.h has the geometry
    // (rounds, gl_common.h: block row yy of the grid is row y of round yy / Y — one scalar divide in front of the first request; a node of
    // one round has yy < Y.  `members` are those of ONE round)
    const int members = (int)((modes >> 16) & DECODE3_M_MEMBERS), Y = (int)(modes >> 24), yy = (int)blockIdx.y;
    const int y = decode3_round_row(Y, yy);
    const int tbl = (int)((modes >> DECODE3_M_TB_SHIFT) & 3u);
    const int slots = ((members - y + Y - 1) / Y) << tbl;
    // lines: the block's slots / H wave-slots are what the waves share, sub-wave h of the lanes takes tile run * H + h
    const Decode3WaveSplit split = decode3_wave_split(slots >> hl, wave);
    // (the span placement alone needs the grid's width: one scalar load of the dispatch's block count, in front of the first request)
    const bool span = (modes & DECODE3_M_SPAN) != 0u;
    const int tile0 = decode3_group_first_tile((int)blockIdx.x, span ? (int)gridDim.x : 0, 1 << tbl, span, (modes & M_PAIR) != 0u);
    const int tile = tile0 + ((((split.layer < 0 ? 0 : split.layer) << hl) & ((1 << tbl) - 1)) + (lane >> (6 - hl)));
    const uint32_t n0 = (uint32_t)(tile * TC + c * 4);
    const int w_mode = (int)(modes & 15u), gs_shift = (int)((modes >> 8) & 255u);
    const bool need_s = w_mode >= 2, need_z = (w_mode == 1 || w_mode >= 3) && !(modes & M_ZSCALAR);
    float tot[4] = {0.f, 0.f, 0.f, 0.f};
    float scalar_zero = 0.f;  // (read once per wave, from its own layer)
    const float bz = (w_mode == 1 || w_mode == 3) ? -1.f : (w_mode == 4 ? 1.f : 0.f);
    const bool b_times_s = w_mode == 3;
    uint32_t wmask[Item<Tag, SX>::WP];
#pragma unroll
    for (int i = 0; i < Item<Tag, SX>::WP; ++i) wmask[i] = (15u * 0x00010001u) << (4 * i);
    XStage xs;
    const Item<Tag, SX> item{xs, wmask, need_s, need_z, scalar_zero, bz, b_times_s, tot};

    // (slot: the wave's first of H; lq: the lane inside its sub-wave, gl its row pair of a pass)
    const int lq = lane & ((64 >> hl) - 1), gl = lq >> 2;
    const int slot = (split.layer < 0 ? 0 : split.layer) << hl, li = slot >> tbl, v0 = split.v0, v1 = split.v1;
    // this wave's layer: the preloaded scalars (layer 0) or the by-value table, scalar loads either way, once per wave
    const int L = decode3_round_member(members, Y, yy, li);
    const char *w_ = wb, *x_ = xb, *s_ = sp, *z_ = zp;
    if (L > 0) {
        const GroupMember& m = tab.m[L - 1];
        w_ = m.w; x_ = m.x; s_ = m.s; z_ = m.z;
    }
    // (a scalar load, read ahead of the first request: a load hipcc tracks inside the counted ring would bring the full drain back)
    if (modes & M_ZSCALAR) scalar_zero = (float)((const int32_t*)z_)[0];
    // per-lane byte offsets, fixed for the whole launch.  Metadata row of chunk gc, row pair g: ((gc * 32 + 2 g) * 8) >> gs_shift
    // = (gc << 8 >> gs_shift) + (16 g >> gs_shift) for groups up to 256, gc >> (gs_shift - 8) for larger ones (16 g < 256).
    // In pass p the lane's row pair is g = p * 16 / H + gl: the lane keeps gl's share, the pass adds whole multiples to the uniform
    // bases — 32 / H weight rows, 512 / H bytes of x, (256 / H p) >> gs_shift metadata rows (16 g >> gs_shift splits exactly into the
    // pass's part and the lane's: 256 / H p is a multiple of the group, or the 16 gl < 256 / H behind it stay inside its group)
    const uint32_t vw0 = (uint32_t)(gl * R) * sw4 + n0 * 4u, vw1 = vw0 + sw4, vx = (uint32_t)lq * 8u;
    const uint32_t vm = (gs_shift < 8 ? (uint32_t)(gl * R * 8) >> gs_shift : 0u) * mstride2 + n0 * 2u;
    const uint32_t pass_w = (uint32_t)(CHUNK >> hl) * sw4, pass_x = (uint32_t)(CHUNK * 16) >> hl;
    const int pass_ms = gs_shift < 8 ? gs_shift : 31;  // (groups of 256 and more: no metadata row inside a chunk)
    // (absent metadata is still requested — the first bytes of the weight buffer — so every item is five requests)
    const uint32_t vs = need_s ? vm : 0u, vz = need_z ? vm : 0u, ms_s = need_s ? mstride2 : 0u, ms_z = need_z ? mstride2 : 0u;
    const char *sb = need_s ? s_ : w_, *zb = need_z ? z_ : w_;
    const int shl = gs_shift < 8 ? 8 - gs_shift : 0, shr = gs_shift > 8 ? gs_shift - 8 : 0;
    const uint32_t chunk_w = (uint32_t)CHUNK * sw4;
    const int nv = v1 - v0, rem = (nch_total & (NW - 1)) - v0;
    const int n = ((nch_total / NW) * nv + (rem < 0 ? 0 : (rem > nv ? nv : rem))) << hl;  // items of this wave: H passes per chunk (0: an idle wave, or K too short)
    // the partial rows: [slots the block can hold][RED], 64 KiB.  Shared x, dynamic LDS: [partial rows][units x 8 pair dwords][units x sum],
    // units = 16 per chunk (gl_common.h: decode3_shared_x_lds_bytes)
    float* redg;
    uint32_t* xpairs = nullptr;
    float* xsums = nullptr;
    const int units = nch_total * 16;
    if constexpr (SX) {
        extern __shared__ __attribute__((aligned(16))) float d3_lds[];
        redg = d3_lds;
        xpairs = (uint32_t*)(d3_lds + DECODE3_GMAX * RED);
        xsums = (float*)(xpairs + units * 8);
    } else {
        __shared__ __attribute__((aligned(16))) float red[DECODE3_GMAX * RED];
        redg = red;
    }
    // the lane's place in a partial row of ITS slot (sub-wave h: slot + h); row v * 4 + r with r = p * 4 / H + (DPP row inside the sub-wave)
    float* rd = redg + ((slot + (lane >> (6 - hl))) * RED + (lq >> 4) * TC + c * 4);

    constexpr int NLC = SX ? 4 : 5;
    int rv = v0, rp = 0, rgc = v0;  // request cursor: virtual wave, pass, chunk
    auto request = [&](Chunk& ck, int) __attribute__((always_inline)) {
        const char* wq = w_ + ((uint32_t)rgc * chunk_w + (uint32_t)rp * pass_w);
        gvw::gld128<NT>(ck.w[0], wq, vw0);
        gvw::gld128<NT>(ck.w[1], wq, vw1);
        if constexpr (!SX) gvw::gld64(ck.xq, x_ + ((uint32_t)rgc * (uint32_t)(CHUNK * 16) + (uint32_t)rp * pass_x), vx);
        const uint32_t grp = (((uint32_t)rgc << shl) >> shr) + (((uint32_t)rp << (8 - hl)) >> pass_ms);
        gvw::gld64(ck.s, sb + grp * ms_s, vs);
        gvw::gld64(ck.z, zb + grp * ms_z, vz);
        rgc += NW;
        if (rgc >= nch_total) {  // the next pass over this virtual wave, or the next virtual wave
            if (++rp == H) { rp = 0; ++rv; }
            rgc = rv;
        }
    };
    auto tie_chunk = [&](Chunk& ck) __attribute__((always_inline)) {
        gvw::tie(ck.w[0]);
        gvw::tie(ck.w[1]);
        if constexpr (!SX) gvw::tie(ck.xq);
        gvw::tie(ck.s);
        gvw::tie(ck.z);
    };
    // a virtual wave's end, the single-layer code: DPP row sums, the partial row to the layer's LDS region
    auto flush = [&](int v, int p) {
#pragma unroll
        for (int j = 0; j < 4; ++j) tot[j] = row_sum(tot[j]);
        if ((lane & 12) == 0) *(f32x4*)(rd + (v * 4 + (p << (2 - hl))) * TC) = (f32x4){tot[0], tot[1], tot[2], tot[3]};
#pragma unroll
        for (int j = 0; j < 4; ++j) tot[j] = 0.f;
    };
    int cv = v0, cp = 0, cgc = v0;  // compute cursor
    // (the first two requests belong to the variant that consumes them: requested ahead of the branch, their registers — still in
    // flight — were COPIED into each variant's own set in front of its loop)
    // shared x, staging: unit u's 32 bytes of x become its eight pair dwords and its sum with the instructions item() runs on them
    // (rows 2 u and 2 u + 1: dwords 0..3 and 4..7; the sum chain from 0.f over row 2 u's pairs, then row 2 u + 1's)
    auto stage_unit = [&](int u, const u32x4& lo, const u32x4& hi) __attribute__((always_inline)) {
        u32x4 pr[R];
        float xsum = 0.f;
#pragma unroll
        for (int i = 0; i < R; ++i) {
            const u32x4& d = i ? hi : lo;
            pr[i][0] = __builtin_amdgcn_perm(d[2], d[0], 0x05040100u);
            pr[i][1] = __builtin_amdgcn_perm(d[2], d[0], 0x07060302u);
            pr[i][2] = __builtin_amdgcn_perm(d[3], d[1], 0x05040100u);
            pr[i][3] = __builtin_amdgcn_perm(d[3], d[1], 0x07060302u);
#pragma unroll
            for (int dd = 0; dd < 4; ++dd) xsum = TR::dot2(pr[i][dd], TR::ONES2, xsum);
        }
        if (u < units) {
            *(u32x4*)(xpairs + u * 8) = pr[0];
            *(u32x4*)(xpairs + u * 8 + 4) = pr[1];
            xsums[u] = xsum;
        }
    };
    // (a lane past the last unit loads the last unit's bytes and writes nothing: units is a multiple of 16, not of 64)
    auto stage_off = [&](int u) { return (uint32_t)(u < units ? u : units - 1) * 32u; };
    constexpr int STRIPS = (int)((DECODE3_SHARED_X_MAX_UNITS + 1023) / 1024);  // staging trips of the 1024 threads: what fits in LDS
    // the lane's unit of chunk 0, pass 0; chunk gc is 128 dwords of pairs and 16 sums further, pass p 16 / H units: one vector add each per item
    const uint32_t* xp_lane = xpairs + gl * 8;
    const float* xs_lane = xsums + gl;
    auto run = [&](auto full) {
        Chunk A, B;
        if constexpr (SX) {
            // thread u loads the units u, u + 1024, ... (all trips' loads first), then the wave's first two items go out, then ONE wait
            // for the x loads alone: they are older than every item request
            u32x4 lo[STRIPS], hi[STRIPS];
#pragma unroll
            for (int t = 0; t < STRIPS; ++t) {
                if (wave * 64 + t * 1024 < units) {
                    const uint32_t so = stage_off(tid + t * 1024);
                    gvw::gld128<false>(lo[t], xb, so);
                    gvw::gld128<false>(hi[t], xb, so + 16u);
                }
            }
            if (n > 0) request(A, 0);
            if (n > 1) request(B, 1);
            if (wave * 64 < units) {
                if (n > 1) gvw::wait_vm<2 * NLC>(); else if (n > 0) gvw::wait_vm<NLC>(); else gvw::wait_vm<0>();
#pragma unroll
                for (int t = 0; t < STRIPS; ++t) {
                    if (wave * 64 + t * 1024 < units) {
                        gvw::tie(lo[t]);
                        gvw::tie(hi[t]);
                        stage_unit(tid + t * 1024, lo[t], hi[t]);
                    }
                }
            }
            __syncthreads();
        } else {
            if (n > 0) request(A, 0);
            if (n > 1) request(B, 1);
        }
        gvw::ring2_run_pre<NLC>(n, A, B, request, tie_chunk, [&](int) __attribute__((always_inline)) {
            if constexpr (SX) {
                const int unit = cgc * 16 + (cp << (4 - hl));
                const uint32_t* xp = xp_lane + unit * 8;
                xs.p[0] = *(const u32x4*)xp;
                xs.p[1] = *(const u32x4*)(xp + 4);
                xs.sum = xs_lane[unit];
            }
        }, [&](const Chunk& ck, int) __attribute__((always_inline)) {
            item.template run<decltype(full)::value>(ck);
            cgc += NW;
            if (cgc >= nch_total) {
                flush(cv, cp);
                if (++cp == H) { cp = 0; ++cv; }
                cgc = cv;
            }
        });
    };
    // (scales and zeros both present — every A16W4 layer quantised with a zero tensor: the selects are compiled out)
    if (need_s && need_z) run(std::true_type{}); else run(std::false_type{});
    if (split.layer >= 0) {
#pragma unroll 1
        for (int v = cv; v < v1; ++v)  // virtual waves without a chunk: every pass writes its rows (cp is 0 here: a virtual wave has all its passes or none)
            for (int p = 0; p < H; ++p) flush(v, p);
    }

    // waves 0 .. slots - 1 finish one slot each (layer wave / TB on tile wave % TB); they ask for its bias element in front of the barrier
    const bool fin = wave < slots;
    const int ftile = tile0 + (wave & ((1 << tbl) - 1));
    uint16_t* o_ = out;
    uint16_t braw = 0;
    if (fin) {
        const int Lf = decode3_round_member(members, Y, yy, wave >> tbl);
        if (Lf > 0) o_ = tab.m[Lf - 1].out;
        if constexpr (BIASED) {
            if (lane < 16) braw = tab.bias[Lf][ftile * TC + lane];
        }
    }
    __syncthreads();
    if (fin) finish<Tag, BIASED>(redg + wave * RED, braw, o_, ftile);
}

// The experts of a mixture-of-experts layer (gemlite_hip_forward_experts): grid (N / 16, slots), block (tile, s) is the single-layer block
// of expert ids[s] on x row s / slots_per_x_row: wave w runs virtual wave w of the member into the block's own 4 KiB of partial rows, so
// every slot is bit-identical to that expert's own launch.  What differs lies in front of the first request (dec3::expert_id, expert_bases): the
// first 14 dwords are the decode3 set (preloaded), the tail is read with scalar loads and the id load follows it: two dependent scalar
// round trips in front of the weight requests, where the single-layer kernel has none (no user SGPR is left to preload the ids pointer
// into).  A block with an invalid id writes its 16 zeros and leaves (a uniform branch).
template <typename Tag, bool BIASED, bool IDS64>
__global__ __launch_bounds__(1024, 1)
void gemv_w4_decode3_experts_kernel(const char* wb, const char* xb, const char* sp, const char* zp, uint16_t* out,
                                    uint32_t sw4, uint32_t mstride2, int nch_total, uint32_t modes, const ExpertsTail tail) {
    using namespace dec3;
    __shared__ __attribute__((aligned(16))) float red[RED];

    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int tile = pair_tile(modes, (int)blockIdx.x);
    const uint32_t slot = blockIdx.y;
    const uint64_t e = expert_id<IDS64>(tail, slot);
    out += (uint64_t)slot * (uint64_t)tail.stride_out;
    if (!expert_valid(tail, e)) {
        if (tid < TC) out[tile * TC + tid] = 0;
        return;
    }
    expert_bases(tail, e, slot, modes, wb, xb, sp, zp);
    run_member<Tag, true, true>(wb, xb, sp, zp, sw4, mstride2, nch_total, modes, tile, wave, wave + 1, red, [](int) {});
    uint16_t braw = 0;
    if constexpr (BIASED) {
        if (wave == 0 && lane < 16) braw = expert_bias(tail, e)[tile * TC + lane];
    }
    __syncthreads();
    if (wave == 0) finish<Tag, BIASED>(red, braw, out, tile);
}

// The fused epilogues of an expert MLP (gemlite_hip_forward_experts_fused): a block holds several MEMBERS — (expert, tile) pairs — that
// share its 16 waves the way the layers of a grouped block do with H = 1 and per-wave x: decode3_wave_split(members, wave) gives a wave
// its member and its virtual waves [v0, v1), the wave computes the member's bases from the id it loads itself (dec3::expert_id, expert_bases) and
// runs its share into the member's own 4 KiB of LDS; after one barrier a member's region is summed in finish()'s order.  So a member's
// rounded output is bit-identical to that expert's own gemv_w4_decode3_kernel launch, and to its slot of gemv_w4_decode3_experts_kernel.
//   EPI = GEMLITE_EXPERTS_GLU      grid (I / 16, slots), I = N / 2: block (t, s) holds tile t (gate, columns [0, I)) and tile t + I / 16
//                                  (up, columns [I, 2 I)) of expert ids[s] on x row s / slots_per_x_row, 8 waves each; with g16 / u16 the
//                                  members' rounded outputs (bias included) wave 0 stores from_float(silu(g16) * u16), silu(v) =
//                                  v / (1 + exp(-v)) in fp32 (v exp(v / 2) exp(v / 2) below -88, where exp(-v) overflows).  An invalid id: the block stores 16 zeros and leaves (block-uniform).
//   EPI = GEMLITE_EXPERTS_COMBINE  grid (N / 16, tokens): block (t, tok) holds tile t of the slots tok * spt + k, k < spt <= 16, each with
//                                  its own id, x row and bias row.  A member with an invalid id requests nothing (its waves go straight to
//                                  the barrier, uniform per wave) and contributes exactly 0.  Wave k rounds member k as finish() does and
//                                  leaves w[slot_k] * to_float(y16_k) in LDS; behind a second barrier wave 0 adds the products in
//                                  ascending k from 0.f and stores one rounded row per token.
template <typename Tag, bool BIASED, bool IDS64, int EPI>
__global__ __launch_bounds__(1024, 1)
void gemv_w4_decode3_experts_fused_kernel(const char* wb, const char* xb, const char* sp, const char* zp, uint16_t* out,
                                          uint32_t sw4, uint32_t mstride2, int nch_total, uint32_t modes, const ExpertsFusedTail tail) {
    using namespace dec3;
    using TR = F16Traits<Tag>;
    constexpr bool GLU = EPI == GEMLITE_EXPERTS_GLU;
    __shared__ __attribute__((aligned(16))) float red[(GLU ? 2 : DECODE3_GMAX) * RED];

    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int tile = pair_tile(modes, (int)blockIdx.x);  // GLU: of the I / 16 tiles of one half
    const int members = GLU ? 2 : (int)tail.members;
    const Decode3WaveSplit split = decode3_wave_split(members, wave);
    const int li = split.layer < 0 ? 0 : split.layer;
    // this wave's member: its slot (GLU: the block's), its tile (GLU: the up half lies I / 16 tiles further)
    const uint32_t slot = GLU ? blockIdx.y : blockIdx.y * (uint32_t)members + (uint32_t)li;
    const int mtile = GLU ? tile + li * (int)tail.half_tiles : tile;
    const uint64_t e = expert_id<IDS64>(tail.e, slot);
    out += (uint64_t)blockIdx.y * (uint64_t)tail.e.stride_out;
    if constexpr (GLU) {
        if (!expert_valid(tail.e, e)) {
            if (tid < TC) out[tile * TC + tid] = 0;
            return;
        }
    }
    if (split.layer >= 0 && expert_valid(tail.e, e)) {
        expert_bases(tail.e, e, slot, modes, wb, xb, sp, zp);
        run_member<Tag, true, false>(wb, xb, sp, zp, sw4, mstride2, nch_total, modes, mtile, split.v0, split.v1, red + li * RED, [](int) {});
    }

    if constexpr (GLU) {
        // wave 0 finishes both members; it asks for their bias elements in front of the barrier
        uint16_t bg = 0, bu = 0;
        if constexpr (BIASED) {
            if (wave == 0 && lane < 16) {
                const uint16_t* b = expert_bias(tail.e, e);
                bg = b[tile * TC + lane];
                bu = b[(tile + (int)tail.half_tiles) * TC + lane];
            }
        }
        __syncthreads();
        if (wave == 0) {
            const float gv = TR::to_float(finish_value<Tag, BIASED>(red, bg));
            const float uv = TR::to_float(finish_value<Tag, BIASED>(red + RED, bu));
            float act = gv / (1.f + expf(-gv));
            // (below -88 exp(-g) leaves fp32 and the quotient is -0, while silu(g) = g exp(g) is a normal bf16 number down to about -92 and
            // a subnormal one down to -97: there g exp(g / 2) exp(g / 2), whose factors stay normal.  g = -Inf gives -Inf * 0 = NaN, as the
            // quotient does; every g >= -88 takes the quotient, bit for bit what it was)
            if (gv < -88.f) {
                const float hv = expf(0.5f * gv);
                act = (gv * hv) * hv;
            }
            if (lane < 16) out[tile * TC + lane] = TR::from_float(act * uv);
        }
    } else {
        // waves 0 .. members - 1 finish one member each: the id again (a scalar load), the routing weight, the bias element
        const bool fin = wave < members;
        bool fvalid = false;
        float wk = 0.f;
        uint16_t braw = 0;
        if (fin) {
            const uint32_t fslot = blockIdx.y * (uint32_t)members + (uint32_t)wave;
            const uint64_t ef = expert_id<IDS64>(tail.e, fslot);
            fvalid = expert_valid(tail.e, ef);
            if (fvalid) {
                wk = tail.w_f32 ? ((const float*)tail.weights)[fslot] : TR::to_float(((const uint16_t*)tail.weights)[fslot]);
                if constexpr (BIASED) {
                    if (lane < 16) braw = expert_bias(tail.e, ef)[tile * TC + lane];
                }
            }
        }
        __syncthreads();
        if (fin) {
            // (the product is rounded on its own, in the wave that holds the weight; row 0 of the member's region carries it: the wave's
            // reads of the region are in front of this write in its own LDS queue, and no other wave touches the region)
            float p = 0.f;
            if (fvalid) p = wk * TR::to_float(finish_value<Tag, BIASED>(red + wave * RED, braw));
            if (lane < 16) red[wave * RED + lane] = p;
        }
        __syncthreads();
        if (wave == 0 && lane < 16) {
            float acc = 0.f;
#pragma unroll 1
            for (int k = 0; k < members; ++k) acc += red[k * RED + lane];
            out[tile * TC + lane] = TR::from_float(acc);
        }
    }
}

// The accessors: runtime arguments -> the kernel form.  with_tag (0 fp16 | 1 bf16) and with_bool hand their argument on as a TYPE
// (decltype(T); B() is a constant expression), so every form is spelled once
template <typename F>
static const void* with_tag(int tag, F&& f) {
    return tag == 0 ? f(half_tag{}) : f(bf16_tag{});
}
template <typename F>
static const void* with_bool(bool b, F&& f) {
    return b ? f(std::true_type{}) : f(std::false_type{});
}

const void* gemv_w4_decode3_fn(int tag, bool nt) {
    return with_tag(tag, [&](auto T) {
        return with_bool(nt, [&](auto NT) { return (const void*)gemv_w4_decode3_kernel<decltype(T), NT()>; });
    });
}
const void* gemv_w4_decode3_bias_fn(int tag, bool nt) {
    return with_tag(tag, [&](auto T) {
        return with_bool(nt, [&](auto NT) { return (const void*)gemv_w4_decode3_kernel<decltype(T), NT(), true>; });
    });
}
const void* gemv_w4_decode3_experts_fn(int tag, bool biased, bool ids64) {
    return with_tag(tag, [&](auto T) {
        return with_bool(biased, [&](auto B) {
            return with_bool(ids64, [&](auto I) { return (const void*)gemv_w4_decode3_experts_kernel<decltype(T), B(), I()>; });
        });
    });
}
const void* gemv_w4_decode3_experts_fused_fn(int tag, int epilogue, bool biased, bool ids64) {
    return with_tag(tag, [&](auto T) {
        return with_bool(biased, [&](auto B) {
            return with_bool(ids64, [&](auto I) {
                return with_bool(epilogue == GEMLITE_EXPERTS_GLU, [&](auto G) {
                    constexpr int EPI = G() ? GEMLITE_EXPERTS_GLU : GEMLITE_EXPERTS_COMBINE;
                    return (const void*)gemv_w4_decode3_experts_fused_kernel<decltype(T), B(), I(), EPI>;
                });
            });
        });
    });
}
// Every grouped form (h: the tiles per wave, 1 / 2 / 4; anything else: 1.  nt: non-temporal weight requests, H = 2 and 4 only — with one
// tile per wave the other half of a line belongs to another wave, and that form stays default-policy whatever is asked)
const void* gemv_w4_decode3_group_fn(int tag, bool biased, bool shared_x, int h, bool nt) {
    return with_tag(tag, [&](auto T) {
        return with_bool(biased, [&](auto B) {
            return with_bool(shared_x, [&](auto SX) {
                return with_bool(nt && (h == 2 || h == 4), [&](auto NT) {
                    if constexpr (NT()) {
                        return h == 4 ? (const void*)gemv_w4_decode3_group_kernel<decltype(T), B(), SX(), 2, true>
                                      : (const void*)gemv_w4_decode3_group_kernel<decltype(T), B(), SX(), 1, true>;
                    } else {
                        return h == 4 ? (const void*)gemv_w4_decode3_group_kernel<decltype(T), B(), SX(), 2, false>
                                      : (h == 2 ? (const void*)gemv_w4_decode3_group_kernel<decltype(T), B(), SX(), 1, false>
                                                : (const void*)gemv_w4_decode3_group_kernel<decltype(T), B(), SX(), 0, false>);
                    }
                });
            });
        });
    });
}

}  // namespace gl
