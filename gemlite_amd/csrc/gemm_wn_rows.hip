// gemm_wn_rows.hip — 2 .. 64 activation rows x packed 4-bit (and, late in the round, 2-bit) weights (round 5): the batched-decode regime,
// shaped like the M = 1 decode kernel of gemv_decode.hip instead of like a GEMM tile.  Template forms: MT = 1 .. 4 row tiles of 16, SPG = group
// size class (128+ / 64 / 32), NT = 1 / 2 column tiles per block (4096 < N <= 8192), BITS = 4 / 2; epilogue channel scales in the 16-bit
// type or fp32 (BitNet).  Experiments that did NOT ship are in profiles/r05/probe_rows5_*_slower.log.
//
// Replaces gemm_splitK_INT_kernel (gemlite/triton_kernels/gemm_splitK_kernels.py:277-450) for the decode-batch sizes where
// rounds 2-4 paid either a cross-block K-slice combine (gemm_wn_direct.hip: 32- / 64-column tiles x 2 slices, 7.4 us at 4096^2 M = 16)
// or an LDS-staged 64 x 64 tile (gemm_wn_mma_kernel.inc: 12.3 / 12.9 us at M = 32 / 64) for a weight stream that the M = 1 kernel
// finishes in 4.7 us.  Same numerics as gemm_wn_direct.hip (raw integer codes through the matrix core, scale / zero applied once per
// quantisation group to the fp32 accumulators, the group sums of x from a second MFMA against a constant B fragment).
//
// Shape of a launch: N / 16 blocks (256 at N = 4096: one per CU, K is NEVER split across blocks), 8 waves; wave w owns the 256-k chunks
// w, w + 8, ... of K and all MT row tiles of 16 rows.
//   * weights: requested FIRST, two chunks ahead, exactly like the decode kernel — lane (g = lane >> 2, c = lane & 3) asks for packed rows
//     2g, 2g + 1 of the chunk x columns 4c .. 4c + 3 as two 16-byte non-temporal loads (64-byte row segments; tiles 2p, 2p + 1 share an
//     XCD).  The matrix core wants lane (j = lane & 15, kb = lane >> 4) to hold the word of column j, packed row 4 s + kb for k-step s:
//     the wave turns its 2 KB around through a PRIVATE LDS slot (two ds_write_b128, eight ds_read_b32, conflict-free, no barrier: DS
//     operations of one wave execute in order).  Dword loads in MFMA layout (gemv_mfma.hip, V = 1) cost 4x the memory instructions.
//   * x: every block reads all of x (M K 2 bytes through the CU's L2 -> L1 path), so HOW it is requested decides the kernel.  The first
//     version loaded the A fragment of lane (j, kb) — 16 bytes of row j — straight into registers: one wave-level request = 16 rows x 64
//     bytes = sixteen HALF cache lines, and measured 37 GB/s per CU (4096^2: M = 32 11.3 us, M = 64 18.4).  A timing experiment with the
//     same bytes requested as 8 rows x 128 bytes per instruction (wrong results) ran M = 32 in 7.6 and M = 64 in 10.4 us
//     (profiles/r05/probe_rows5_xline.log).  The MFMA operand layout cannot give that from registers (a request covers 16 rows whatever
//     the k order), so x goes through LDS: LDS-DMA pieces of 1 KiB = whole 128-byte lines (2 / 4 / 8 rows per instruction), two
//     8-KiB buffers per wave (16 MT rows x 256 / 128 / 64 k), the 16-byte slot of (row r, piece p) XOR-swizzled with f(r) through the
//     SOURCE address so that the ds_read_b128 of an A fragment is conflict-free; piece i + 2 is requested when piece i has been consumed.
//     The B fragment is built in NATURAL k order — t_lo = w & 0x0F0F0F0F, t_hi = (w >> 4) & 0x0F0F0F0F, pair p = v_perm(t_hi, t_lo) |
//     MAGIC2 = (OFF + q_2p, OFF + q_2p+1), 11 VALU per word — so the A fragment is x as it lies in memory: nothing is permuted or
//     pre-scaled per row tile.  OFF = 1024 (fp16) / 128 (bf16): exact, and OFF * sum(x) leaves with the zero-point term.
//   * scale / zero: one 2-byte load each per lane and FOUR groups (lane (j, kb) fetches group 4 l + kb, column j), distributed with
//     ds_bpermute.
//   * the 8 partial tiles meet in LDS (the wave's own buffer again), one barrier, packed 4-byte stores.
// All memory requests are inline asm retired by hand-counted waits (gl_async.h has the reasoning; scripts/isa_asmloads.py audits the
// generated code).  Scalar kernel arguments, the first 14 dwords preloaded into SGPRs (-amdgpu-kernarg-preload-count, see gemv_decode.hip).
#include "gl_rows5.h"
#include "gl_host.h"

namespace gl {

// MT = row tiles of 16 (M <= 16 MT); SPG = 32-k steps per quantisation group (4: groups of >= 128, 2: 64, 1: 32); NT = 16-column tiles
// per block (2: layers with 4096 < N <= 8192 — N / 32 blocks stay resident in ONE round, and an x piece read from LDS feeds both tiles)
// BITS = 4 or 2 (late round 5: 2-bit words — A16W2, BitNet A16W158 — through the same kernel): a packed row holds E = 32 / BITS k-values, a chunk
// of 32 packed rows is 256 / 512 k = 8 / 16 MFMA k-steps.  2-bit: lane (j, kb) of k-step s needs k = 32 s + 8 kb .. + 7 = HALF (kb & 1) of the word
// of packed row 2 s + (kb >> 1): sixteen ds_read_b32 per chunk instead of eight (two lanes share an address: broadcast), the 16-bit half is
// spread to eight nibbles (three shift-or + and pairs) and then treated like a 4-bit word — natural k order again, so groups of 32 work
#define GL_ROWS5_KERNEL gemm_w4_rows_kernel
#define GL_ROWS5_BIAS 0
#include "gemm_wn_rows_kernel.inc"
#undef GL_ROWS5_KERNEL
#undef GL_ROWS5_BIAS
// the same kernel with the bias add in its epilogue (new instantiations: the forms above do not change)
#define GL_ROWS5_KERNEL gemm_w4_rows_bias_kernel
#define GL_ROWS5_BIAS 1
#include "gemm_wn_rows_kernel.inc"
#undef GL_ROWS5_KERNEL
#undef GL_ROWS5_BIAS

// ---------------------------------------------------------------------------------------------------------------------
// host-side planning.  tuning[0] = 9 forces this kernel (any M), GEMLITE_TF_NO_ROWS_KERNEL = never (the round-4 choice, A/B runs)
// ---------------------------------------------------------------------------------------------------------------------
typedef void (*rows5_fn)(const char*, const char*, const char*, const char*, uint16_t*, uint32_t, uint32_t, int, uint32_t, int, uint32_t, uint32_t);

template <typename Tag, int MT>
static rows5_fn rows5_pick_spg(int spg, int nt, int bits) {
    if (bits == 2) {  // 2-bit words: one column tile per block
        if (nt != 1) return nullptr;
        switch (spg) {  // (16 unrolled k-steps per chunk: groups of 64 fit 256 registers up to 32 rows, groups of 32 up to 16)
            case 4: return gemm_w4_rows_kernel<Tag, MT, 4, 1, 2>;
            case 2:
                if constexpr (MT <= 2) return gemm_w4_rows_kernel<Tag, MT, 2, 1, 2>;
                else return nullptr;
            case 1:
                if constexpr (MT <= 1) return gemm_w4_rows_kernel<Tag, MT, 1, 1, 2>;
                else return nullptr;
            default: return nullptr;
        }
    }
    if (nt == 2) {  // two column tiles per block: groups of >= 128 up to 64 rows, groups of 64 up to 32 rows (registers)
        if (spg == 4) return gemm_w4_rows_kernel<Tag, MT, 4, 2>;
        if constexpr (MT <= 2) {
            if (spg == 2) return gemm_w4_rows_kernel<Tag, MT, 2, 2>;
        }
        return nullptr;
    }
    switch (spg) {
        case 4: return gemm_w4_rows_kernel<Tag, MT, 4>;
        case 2: return gemm_w4_rows_kernel<Tag, MT, 2>;
        case 1:  // groups of 32: up to 32 rows per block (the 48- / 64-row forms need more than 256 registers); more rows go along grid.y
            if constexpr (MT <= 2) return gemm_w4_rows_kernel<Tag, MT, 1>;
            else return nullptr;
        default: return nullptr;
    }
}
template <typename Tag>
static rows5_fn rows5_pick(int mt, int spg, int nt, int bits) {
    switch (mt) {
        case 1: return rows5_pick_spg<Tag, 1>(spg, nt, bits);
        case 2: return rows5_pick_spg<Tag, 2>(spg, nt, bits);
        case 3: return rows5_pick_spg<Tag, 3>(spg, nt, bits);
        case 4: return rows5_pick_spg<Tag, 4>(spg, nt, bits);
        default: return nullptr;
    }
}

// the same table for the forms with the bias add
typedef void (*rows5_bias_fn)(const char*, const char*, const char*, const char*, uint16_t*, uint32_t, uint32_t, int, uint32_t, int, uint32_t, uint32_t, const uint16_t*);

template <typename Tag, int MT>
static rows5_bias_fn rows5_bias_pick_spg(int spg, int nt, int bits) {
    if (bits == 2) {  // 2-bit words: one column tile per block
        if (nt != 1) return nullptr;
        switch (spg) {  // (16 unrolled k-steps per chunk: groups of 64 fit 256 registers up to 32 rows, groups of 32 up to 16)
            case 4: return gemm_w4_rows_bias_kernel<Tag, MT, 4, 1, 2>;
            case 2:
                if constexpr (MT <= 2) return gemm_w4_rows_bias_kernel<Tag, MT, 2, 1, 2>;
                else return nullptr;
            case 1:
                if constexpr (MT <= 1) return gemm_w4_rows_bias_kernel<Tag, MT, 1, 1, 2>;
                else return nullptr;
            default: return nullptr;
        }
    }
    if (nt == 2) {  // two column tiles per block: groups of >= 128 up to 64 rows, groups of 64 up to 32 rows (registers)
        if (spg == 4) return gemm_w4_rows_bias_kernel<Tag, MT, 4, 2>;
        if constexpr (MT <= 2) {
            if (spg == 2) return gemm_w4_rows_bias_kernel<Tag, MT, 2, 2>;
        }
        return nullptr;
    }
    switch (spg) {
        case 4: return gemm_w4_rows_bias_kernel<Tag, MT, 4>;
        case 2: return gemm_w4_rows_bias_kernel<Tag, MT, 2>;
        case 1:  // groups of 32: up to 32 rows per block (the 48- / 64-row forms need more than 256 registers); more rows go along grid.y
            if constexpr (MT <= 2) return gemm_w4_rows_bias_kernel<Tag, MT, 1>;
            else return nullptr;
        default: return nullptr;
    }
}
template <typename Tag>
static rows5_bias_fn rows5_bias_pick(int mt, int spg, int nt, int bits) {
    switch (mt) {
        case 1: return rows5_bias_pick_spg<Tag, 1>(spg, nt, bits);
        case 2: return rows5_bias_pick_spg<Tag, 2>(spg, nt, bits);
        case 3: return rows5_bias_pick_spg<Tag, 3>(spg, nt, bits);
        case 4: return rows5_bias_pick_spg<Tag, 4>(spg, nt, bits);
        default: return nullptr;
    }
}

bool plan_gemm_wn_rows(const gemlite_hip_forward_args& a, WnParams& p, LaunchPlan& lp) {
    if ((a.W_nbits != 4 && a.W_nbits != 2) || a.w_pack_bits != 32) return false;
    const int bits = a.W_nbits, epr = 32 / bits;  // k-values per packed row
    if (a.M < 1 || a.M > 65535 * 64) return false;  // above 64 rows: 64-row blocks along grid.y (the weights stream once per block row)
    if (a.input_dtype != GEMLITE_DT_FP16 && a.input_dtype != GEMLITE_DT_BF16) return false;
    if (a.output_dtype != a.input_dtype || a.stride_on != 1 || a.stride_xk != 1 || a.stride_wn != 1) return false;
    // channel scales (mode 1) of the kernel's 16-bit type ride in the epilogue — then nothing in the K loop reads scales (W_group_mode 0 / 1)
    const bool post_s = a.channel_scale_mode == 1;
    if (a.channel_scale_mode != 0 && !post_s) return false;
    const bool post32 = post_s && a.meta_dtype == GEMLITE_DT_FP32;
    if (post_s && (a.W_group_mode >= 2 || (a.meta_dtype != a.input_dtype && !post32) || !a.scales || ((uintptr_t)a.scales % (post32 ? 8 : 4)) != 0)) return false;
    const bool loop_s = a.W_group_mode >= 2, has_z = (a.W_group_mode == 1 || a.W_group_mode >= 3);
    if (loop_s && a.meta_dtype != a.input_dtype) return false;
    if (has_z && !a.zero_is_scalar && a.zeros_dtype != a.input_dtype) return false;
    if (has_z && a.zero_is_scalar && a.zeros_dtype != GEMLITE_DT_INT32) return false;
    if ((a.stride_xm * 2) % 16 != 0 || ((uintptr_t)a.x % 16) != 0) return false;        // 16-byte A fragments
    if (((uintptr_t)a.w_q % 16) != 0 || (a.stride_wk % 4) != 0) return false;            // 16-byte weight loads
    if (((uintptr_t)a.out % 4) != 0 || a.stride_om % 2 != 0) return false;               // packed pairs of outputs
    if (a.N % 16 != 0 || a.K % (32 * epr) != 0) return false;   // whole chunks of 32 packed rows: K % 256 (4-bit) / % 512 (2-bit)
    if (p.gs_shift < 5 || (p.gs_shift > 30 && p.gs_shift != 31)) return false;            // groups of 32, 64, 128, ... k (31: one group spans K)
    const int spg = p.gs_shift >= 7 ? 4 : (p.gs_shift == 6 ? 2 : 1);
    const int64_t rows = a.K / epr;
    // 32-bit byte offsets in the kernel; the x extent of a row block stays below 2^31 so that the 0x80000000 offset of the padded rows (>= M) is
    // beyond the descriptor's num_records and reads zeros
    if (rows * a.stride_wk * 4 + a.N * 4 >= (1ll << 32) || (64 * a.stride_xm + a.K) * 2 >= (1ll << 31) || 64 * a.stride_om * 2 >= (1ll << 32)) return false;
    if (p.gs_shift < 31 && ((a.K >> p.gs_shift) * p.stride_meta_g + a.N) * 2 >= (1ll << 32)) return false;
    // two column tiles per block (tuning[1] = 2 forces, 1 = never): up to 32 rows of a layer whose 16-column tiles do not fit one round
    // of resident blocks but whose 32-column blocks do (4096 < N <= 8192 on 256 CUs)
    const int64_t resident = resident_block_limit();
    int nt = 1;
    if (a.tuning[1] == 2 || (a.tuning[1] == 0 && a.N / 16 > resident && a.N / 32 <= resident)) nt = 2;
    if (nt == 2 && (a.N % 32 != 0 || spg == 1 || bits != 4 || a.M > (spg == 4 ? 64 : 32))) {
        if (a.tuning[1] == 2) return false;
        nt = 1;
    }
    if (a.tuning[1] < 0 || a.tuning[1] > 2) return false;
    // row tiles per block (registers); more rows: blocks along grid.y (the weights stream once per block row)
    const int mt_cap = bits == 4 ? (spg == 1 ? 2 : 4) : (spg == 4 ? 4 : (spg == 2 ? 2 : 1));
    const int mt = a.M > 16 * mt_cap ? mt_cap : (int)((a.M + 15) / 16);
    if ((a.M + 16 * mt - 1) / (16 * mt) > 65535) return false;
    if (a.tuning[2] != 0 && a.tuning[2] != 8) return false;
    const bool f16 = a.input_dtype == GEMLITE_DT_FP16;
    const rows5_fn fn = f16 ? rows5_pick<half_tag>(mt, spg, nt, bits) : rows5_pick<bf16_tag>(mt, spg, nt, bits);
    if (!fn) return false;
    const int nw = rows5::NW;
    const int tiles = (int)(a.N / (16 * nt));
    const bool need_s = loop_s, need_z = has_z && !a.zero_is_scalar;
    p.splitk = 1;
    p.rows_per_slice = (int)rows;
    lp.fn = (const void*)fn;
    lp.bias_of = lp.fn;
    lp.fn_bias = (const void*)(f16 ? rows5_bias_pick<half_tag>(mt, spg, nt, bits) : rows5_bias_pick<bf16_tag>(mt, spg, nt, bits));
    lp.fn_group = gemm_wn_rows_group_fn(f16 ? 0 : 1, mt, spg, nt, bits, false);
    lp.fn_bias_group = gemm_wn_rows_group_fn(f16 ? 0 : 1, mt, spg, nt, bits, true);
    static const char* names[4] = {"gemm_w4_rows_kernel<16x16>", "gemm_w4_rows_kernel<32x16>", "gemm_w4_rows_kernel<48x16>", "gemm_w4_rows_kernel<64x16>"};
    static const char* names2[4] = {"gemm_w4_rows_kernel<16x32>", "gemm_w4_rows_kernel<32x32>", "gemm_w4_rows_kernel<48x32>", "gemm_w4_rows_kernel<64x32>"};
    static const char* names_w2[4] = {"gemm_w2_rows_kernel<16x16>", "gemm_w2_rows_kernel<32x16>", "gemm_w2_rows_kernel<48x16>", "gemm_w2_rows_kernel<64x16>"};
    lp.name = bits == 2 ? names_w2[mt - 1] : (nt == 2 ? names2[mt - 1] : names[mt - 1]);
    lp.grid = dim3((unsigned)tiles, (unsigned)((a.M + 16 * mt - 1) / (16 * mt)), 1);
    lp.block = dim3(64 * nw, 1, 1);
    lp.lds_bytes = (size_t)rows5::WAVE_LDS * nw;
    lp.slab_bytes = 0;
    lp.ws_bytes = 0;
    lp.arg_kind = 2;
    lp.r5.w = (const char*)p.w;
    lp.r5.x = (const char*)p.x;
    lp.r5.s = (need_s || post_s) ? (const char*)p.scales : (const char*)p.w;
    lp.r5.z = (need_z || (has_z && a.zero_is_scalar)) ? (const char*)p.zeros : (const char*)p.w;
    lp.r5.out = (uint16_t*)p.epi.out;
    lp.r5.sw4 = (uint32_t)a.stride_wk * 4u;
    lp.r5.mstride2 = ((need_s || need_z) && p.gs_shift < 31) ? (uint32_t)p.stride_meta_g * 2u : 0u;
    lp.r5.nch_total = (int)(rows / 32);
    lp.r5.modes = (uint32_t)a.W_group_mode | ((has_z && a.zero_is_scalar) ? 16u : 0u) | ((nt == 1 && (tiles & 15) == 0) ? 32u : 0u) | (post_s ? 128u : 0u) | (post32 ? 64u : 0u) | ((uint32_t)p.gs_shift << 8);
    lp.r5.M = (int)a.M;
    lp.r5.sxm2 = (uint32_t)a.stride_xm * 2u;
    lp.r5.som = (uint32_t)a.stride_om;
    return true;
}

}  // namespace gl
