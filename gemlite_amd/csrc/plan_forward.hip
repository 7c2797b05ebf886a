// plan_forward.hip — the forward planner of libgemlite_hip.so (gl_plan.h): validation and kernel selection.  Host code only: nothing is
// launched and no device is touched, so the host queries of the C ABI (api.hip) plan exactly like gemlite_hip_forward.
//
// Selection mirrors get_matmul_type() (gemlite/core.py:100-114) in spirit: the caller's matmul_type names
// a kernel FAMILY; inside a family the library picks the CDNA4 kernel that covers the configuration, and
// everything else goes to the generic coverage kernel — never to a CPU path.
//
// resolve() at the end of the file is a dispatcher over one routine per layer family; each routine returns whether it answered the
// request (a kernel, or a final status).  The planners it asks are defined next to their kernels (gl_host.h).
#include "gl_common.h"
#include "gl_coopquant.h"
#include "gl_host.h"
#include "gl_plan.h"

namespace gl {

static int dtype_size(int dt) {
    switch (dt) {
        case GEMLITE_DT_FP32: case GEMLITE_DT_INT32: case GEMLITE_DT_UINT32: return 4;
        case GEMLITE_DT_FP16: case GEMLITE_DT_BF16: case GEMLITE_DT_INT16: case GEMLITE_DT_UINT16: return 2;
        case GEMLITE_DT_INT64: return 8;
        case GEMLITE_DT_FP8E4: case GEMLITE_DT_FP8E5: case GEMLITE_DT_INT8: case GEMLITE_DT_UINT8: return 1;
        default: return 0;
    }
}

// ---- small predicates and builders the families share ----------------------------------------------------------------------------------
// tuning[0 .. 2] force nothing: the measured rules decide (tuning[3] carries flag bits, never a kernel choice)
static bool tuning_default(const gemlite_hip_forward_args& a) { return a.tuning[0] == 0 && a.tuning[1] == 0 && a.tuning[2] == 0; }

// matmul_type names none of the three GEMV kinds: AUTO or one of the GEMM kinds
static bool gemm_kind(const gemlite_hip_forward_args& a) {
    return a.matmul_type != GEMLITE_MATMUL_GEMV && a.matmul_type != GEMLITE_MATMUL_GEMV_SPLITK && a.matmul_type != GEMLITE_MATMUL_GEMV_REVSPLITK;
}

// The plan is made: a parameter block and launch that were planned aside ...
static bool take(Resolved& r, Kind kind, const WnParams& p, const LaunchPlan& lp) { r.kind = kind; r.wn = p; r.lp = lp; return true; }
static bool take(Resolved& r, Kind kind, const GenericParams& g, const LaunchPlan& lp) { r.kind = kind; r.gp = g; r.lp = lp; return true; }
// ... or one that the planner wrote into r.gp / r.lp itself
static bool take(Resolved& r, Kind kind) { r.kind = kind; return true; }
// ... or a kernel that has no planner of its own: its launch goes into r.lp here (lds_bytes 0: untouched, whatever a planner asked before left there stays)
static bool take_kernel(Resolved& r, Kind kind, const void* fn, const char* name, dim3 grid, dim3 block, size_t lds_bytes = 0) {
    r.lp.fn = fn; r.lp.name = name; r.lp.grid = grid; r.lp.block = block;
    if (lds_bytes) r.lp.lds_bytes = lds_bytes;
    return take(r, kind);
}

static Epilogue make_epilogue(const gemlite_hip_forward_args& a) {
    Epilogue e{};
    e.out = a.out;
    e.scales_w = a.scales;
    e.scales_x = (const float*)a.scales_x;
    e.stride_om = a.stride_om;
    e.stride_on = a.stride_on;
    e.stride_sx_m = a.stride_sx_m;
    e.out_dt = a.output_dtype;
    e.meta_dt = a.meta_dtype;
    e.c_mode = a.channel_scale_mode;
    return e;
}

// A request with the activation quantiser inside the launch is planned on the arguments the matmul will see: x of the quantised type
// x_dt with row stride stride_xm, and its scales with row stride stride_sx_m.  (The pointers serve alignment checks only: the workspace
// copies are 256-byte aligned, and a kernel that quantises in registers gets the caller's x back after planning.)
static gemlite_hip_forward_args quantised_proxy(const gemlite_hip_forward_args& a, int x_dt, int64_t stride_xm, int64_t stride_sx_m) {
    gemlite_hip_forward_args b = a;
    b.input_dtype = x_dt;
    b.x = (const void*)(uintptr_t)0x1000;
    b.scales_x = (const void*)(uintptr_t)0x1000;
    b.stride_xm = stride_xm;
    b.stride_sx_m = stride_sx_m;
    return b;
}

// WnParams of a packed-word layer.  eff_group: the K elements per metadata row; per_group_meta: those rows are indexed by K (the callers
// differ in both: see resolve_fused_quant_packed_row).  stride_xm: the row stride of x as the kernel reads it.
static WnParams packed_wn_params(const gemlite_hip_forward_args& a, int64_t stride_xm, bool per_group_meta, int eff_group) {
    WnParams p{};
    p.x = a.x; p.w = (const uint32_t*)a.w_q; p.scales = a.scales; p.zeros = a.zeros;
    p.epi = make_epilogue(a);
    p.M = (int)a.M; p.N = (int)a.N; p.K = (int)a.K;
    p.group_size = eff_group;
    p.w_mode = a.W_group_mode;
    p.meta_dt = a.meta_dtype; p.zeros_dt = a.zeros_dtype; p.zero_is_scalar = a.zero_is_scalar;
    p.stride_xm = stride_xm; p.stride_xk = a.stride_xk; p.stride_wk = a.stride_wk;
    // one metadata row spanning all of K ([1, N] scales of a K-long group): the row stride is never used, and views of a
    // [N, 1] tensor carry arbitrary values there (1 for `.t()`), which the planners' alignment checks would reject
    p.stride_meta_g = (per_group_meta && eff_group < a.K) ? a.stride_meta_g : 0;
    p.flags = caller_flags(a);
    p.gs_shift = eff_group >= a.K ? 31
                 : ((eff_group > 0 && (eff_group & (eff_group - 1)) == 0) ? __builtin_ctz((unsigned)eff_group) : -1);
    return p;
}

// WnParams of plan_gemm_wn_mma_mx: 16-bit x at `x` (row stride stride_xm) over K-contiguous 8-bit or block-scaled weights, whose scale
// blocks hold group_size k.  The callers set the epilogue's modes afterwards.  (stride_xk: every caller has checked that it is 1.)
static WnParams kcontig_wn_params(const gemlite_hip_forward_args& a, const void* x, int64_t stride_xm, const Epilogue& epi, int group_size) {
    WnParams p{};
    p.x = x; p.w = (const uint32_t*)a.w_q; p.scales = a.scales; p.zeros = nullptr;
    p.epi = epi;
    p.M = (int)a.M; p.N = (int)a.N; p.K = (int)a.K;
    p.group_size = group_size;
    p.stride_xm = stride_xm; p.stride_xk = a.stride_xk; p.stride_wk = 1;
    p.flags = caller_flags(a);
    return p;
}

// GenericParams: what the block-scaled kernels and the coverage kernels fill the same way (zeros, the groups and the metadata strides
// are the callers')
static GenericParams generic_head(const gemlite_hip_forward_args& a) {
    GenericParams g{};
    g.x = a.x; g.w = a.w_q; g.scales = a.scales;
    g.epi = make_epilogue(a);
    g.M = (int)a.M; g.N = (int)a.N; g.K = (int)a.K;
    g.nbits = a.W_nbits; g.e = a.elements_per_sample; g.pack_bits = a.w_pack_bits;
    g.w_dt = a.w_dtype; g.x_dt = a.input_dtype;
    g.stride_xm = a.stride_xm; g.stride_xk = a.stride_xk; g.stride_wk = a.stride_wk; g.stride_wn = a.stride_wn;
    return g;
}

// ---- which requests ask for the activation quantiser inside the launch -----------------------------------------------------------------
// Dynamic activation quantisation fused into the matmul: the caller passes the UNQUANTISED 16-bit x, no scales_x, and the 8-bit
// unpacked weights of a dynamically quantised layer (channel_scale_mode 2 / 3).  M = 1: every block quantises the row itself
// (kmajor_fused_quant_kernel); 2 <= M: the blocks of the A8W8 kernels deal the rows among themselves (gl_coopquant.h).
static bool wants_fused_quant(const gemlite_hip_forward_args* a) {
    if (is_mx_input(a->type_id / 100)) return false;  // a block-scaled layer (its weights carry e8m0 block scales): not this kernel family
    return a->M >= 1 && a->elements_per_sample == 1 && !a->scales_x &&
           (a->channel_scale_mode == 2 || a->channel_scale_mode == 3) && a->W_group_mode == 0 &&
           (a->input_dtype == GEMLITE_DT_FP16 || a->input_dtype == GEMLITE_DT_BF16) &&
           (a->w_dtype == GEMLITE_DT_INT8 || a->w_dtype == GEMLITE_DT_FP8E4 || a->w_dtype == GEMLITE_DT_FP8E5);
}

// The same request for PACKED weights (A8Wn fp8 dynamic, BitNet int8 dynamic; round 4, M = 1): the layer's activation type rides in
// type_id (= input_dtype * 100 + W_nbits, core.py:141-145), x is the unquantised 16-bit row.
static int fused_quant_packed_dtype(const gemlite_hip_forward_args* a) {
    if (a->M != 1 || a->elements_per_sample <= 1 || a->scales_x) return 0;
    if (!(a->channel_scale_mode == 2 || a->channel_scale_mode == 3)) return 0;
    if (!(a->input_dtype == GEMLITE_DT_FP16 || a->input_dtype == GEMLITE_DT_BF16)) return 0;
    const int layer_dt = a->type_id / 100;
    return (layer_dt == GEMLITE_DT_FP8E4 || layer_dt == GEMLITE_DT_INT8) && a->type_id % 100 == a->W_nbits ? layer_dt : 0;
}

// ... and for the block-scaled dynamic layers (round 4, M = 1, MXFP8 / MXFP4 activations with block scales): x is the unquantised 16-bit
// row, input_dtype names ITS type, the layer's format rides in type_id like above, scales_x is NULL, channel_scale_mode 4 (block
// scales) or 2 (MXFP8 with one scale per token)
static int fused_quant_mx_dtype(const gemlite_hip_forward_args* a) {
    if (a->M != 1 || a->scales_x || !(a->channel_scale_mode == 4 || a->channel_scale_mode == 2)) return 0;
    if (!(a->input_dtype == GEMLITE_DT_FP16 || a->input_dtype == GEMLITE_DT_BF16)) return 0;
    const int layer_dt = a->type_id / 100;
    if (a->channel_scale_mode == 2 && layer_dt != GEMLITE_DT_MXFP8) return 0;  // one fp32 scale per token: fp8 activations
    return (layer_dt == GEMLITE_DT_MXFP8 || layer_dt == GEMLITE_DT_MXFP4 || layer_dt == GEMLITE_DT_NVFP4) && a->type_id % 100 == a->W_nbits ? layer_dt : 0;
}

// ---- validation ------------------------------------------------------------------------------------------------------------------------
// block-scaled formats (see the header): what must hold before any kernel is chosen
static int validate_mx(const gemlite_hip_forward_args* a) {
    const bool nv = a->input_dtype == GEMLITE_DT_NVFP4;
    if (a->group_size != (nv ? 16 : 32)) return GEMLITE_ERR_UNSUPPORTED;
    if (a->K % 32 != 0) return GEMLITE_ERR_BAD_SHAPE;
    if (!a->scales) return GEMLITE_ERR_BAD_ARGUMENT;
    if (!(a->output_dtype == GEMLITE_DT_FP32 || a->output_dtype == GEMLITE_DT_FP16 || a->output_dtype == GEMLITE_DT_BF16))
        return GEMLITE_ERR_UNSUPPORTED;
    const bool w8 = a->W_nbits == 8 && a->elements_per_sample == 1 && a->w_dtype == GEMLITE_DT_FP8E4;
    const bool w4 = a->W_nbits == 4 && a->elements_per_sample == 2 && a->w_pack_bits == 8;
    if (!w8 && !w4) return GEMLITE_ERR_UNSUPPORTED;
    const bool x16 = a->input_dtype == GEMLITE_DT_MXFP16 || a->input_dtype == GEMLITE_DT_MXBF16;
    if ((a->input_dtype == GEMLITE_DT_MXFP4 || nv) && !w4) return GEMLITE_ERR_UNSUPPORTED;
    if (x16 ? a->channel_scale_mode != 0 : !(a->channel_scale_mode == 4 || (a->channel_scale_mode == 2 && !nv))) return GEMLITE_ERR_UNSUPPORTED;
    if (!x16 && !a->scales_x) return GEMLITE_ERR_BAD_ARGUMENT;
    if (a->stride_xk != 1) return GEMLITE_ERR_UNSUPPORTED;
    if (a->M > 65535 && a->M > 0x7FFFFFFF) return GEMLITE_ERR_BAD_SHAPE;
    return GEMLITE_OK;
}

int validate(const gemlite_hip_forward_args* a) {
    if (!a || a->struct_size != sizeof(gemlite_hip_forward_args)) return GEMLITE_ERR_BAD_ARGUMENT;
    if (!a->x || !a->w_q || !a->out) return GEMLITE_ERR_BAD_ARGUMENT;
    if (a->M <= 0 || a->N <= 0 || a->K <= 0) return GEMLITE_ERR_BAD_ARGUMENT;
    if (a->M > 0x7FFFFFFF || a->N > 0x7FFFFFFF || a->K > 0x7FFFFFFF) return GEMLITE_ERR_BAD_SHAPE;
    if (is_mx_input(a->input_dtype)) return validate_mx(a);
    if (const int mxdt = fused_quant_mx_dtype(a)) {  // validated as the block-scaled call it stands for
        // (validate_mx reads neither x nor the row strides: the caller's stand)
        const gemlite_hip_forward_args b = quantised_proxy(*a, mxdt, a->stride_xm, a->stride_sx_m);
        return validate_mx(&b);
    }
    if (a->W_group_mode < 0 || a->W_group_mode > 4) return GEMLITE_ERR_UNSUPPORTED;
    if (a->channel_scale_mode < 0 || a->channel_scale_mode > 3) return GEMLITE_ERR_UNSUPPORTED;  // 4: block-scaled inputs only
    if (a->elements_per_sample < 1) return GEMLITE_ERR_BAD_ARGUMENT;
    if (a->K % a->elements_per_sample != 0) return GEMLITE_ERR_BAD_SHAPE;
    if (a->input_dtype == GEMLITE_DT_FP8E4NUZ || a->input_dtype == GEMLITE_DT_FP8E5NUZ) return GEMLITE_ERR_UNSUPPORTED;
    if (a->input_dtype > GEMLITE_DT_FP8E5NUZ) return GEMLITE_ERR_UNSUPPORTED;
    if (dtype_size(a->input_dtype) == 0) return GEMLITE_ERR_UNSUPPORTED;
    if (!(a->output_dtype == GEMLITE_DT_FP32 || a->output_dtype == GEMLITE_DT_FP16 || a->output_dtype == GEMLITE_DT_BF16))
        return GEMLITE_ERR_UNSUPPORTED;
    const bool need_s = a->W_group_mode >= 2 || a->channel_scale_mode == 1 || a->channel_scale_mode == 3;
    const bool need_z = a->W_group_mode == 1 || a->W_group_mode >= 3;
    if (need_s && !a->scales) return GEMLITE_ERR_BAD_ARGUMENT;
    if (need_z && !a->zeros) return GEMLITE_ERR_BAD_ARGUMENT;
    if ((a->channel_scale_mode == 2 || a->channel_scale_mode == 3) && !a->scales_x && !wants_fused_quant(a) && !fused_quant_packed_dtype(a)) return GEMLITE_ERR_BAD_ARGUMENT;
    if (a->elements_per_sample > 1) {
        if (a->w_pack_bits != 8 && a->w_pack_bits != 16 && a->w_pack_bits != 32 && a->w_pack_bits != 64)
            return GEMLITE_ERR_BAD_ARGUMENT;
        if (a->W_nbits * a->elements_per_sample != a->w_pack_bits) return GEMLITE_ERR_BAD_ARGUMENT;
    } else if (dtype_size(a->w_dtype) == 0) {
        return GEMLITE_ERR_UNSUPPORTED;
    }
    const bool grouped = a->W_group_mode >= 2 || (need_z && !a->zero_is_scalar);
    if (grouped && a->group_size <= 0) return GEMLITE_ERR_BAD_SHAPE;
    if (a->input_dtype == GEMLITE_DT_INT8 && a->W_group_mode >= 2) return GEMLITE_ERR_UNSUPPORTED;
    return GEMLITE_OK;
}

// ---- family: block-scaled formats ------------------------------------------------------------------------------------------------------
// Block-scaled formats: the scaled-MFMA kernel for 8 / 4-bit activations, the coverage kernel for everything else
// (16-bit activations x MX weights, NVFP4, layouts that are not K-contiguous).  tuning[0] = 1 forces the coverage kernel.
static GenericParams mx_params(const gemlite_hip_forward_args& a) {
    GenericParams g = generic_head(a);  // (zeros stay NULL)
    if (a.channel_scale_mode == 4) g.epi.c_mode = 0;  // block scales are applied inside the contraction
    g.group_size = a.group_size;
    g.stride_meta_g = a.stride_meta_g; g.stride_meta_n = a.stride_meta_n;
    g.mx_x = a.input_dtype == GEMLITE_DT_MXFP16 ? MX_F16 : (a.input_dtype == GEMLITE_DT_MXBF16 ? MX_BF16 : (a.input_dtype == GEMLITE_DT_MXFP8 ? MX_FP8 : MX_FP4));
    g.mx_w = a.W_nbits == 8 ? MX_FP8 : MX_FP4;
    g.mx_scale_e4m3 = a.input_dtype == GEMLITE_DT_NVFP4 ? 1 : 0;
    g.sx_blocks = a.channel_scale_mode == 4 ? a.scales_x : nullptr;
    g.stride_sx_blk_m = a.stride_sx_m;
    g.mx_post = a.input_dtype == GEMLITE_DT_NVFP4 ? 0.0025f : 1.0f;  // meta_scale_norm = 0.05 ** 2 (gemm_kernels.py:461, 530-531)
    g.splitk = 1;
    return g;
}
static void resolve_mx_plan(const gemlite_hip_forward_args& a, Resolved& r, const GenericParams& g) {
    // 1 .. 64 rows of fp8 / fp4 activations (round 4): 16-column blocks, one 16-row scaled MFMA per 128-k chunk straight from memory.
    // Faster than the streaming kernel below from ONE row (4096^2 fp4 x fp4: 5.4 vs 6.3 us at M = 1, 5.6 vs 9.9 at M = 4) and than the
    // 32-row tile up to 64 rows (M = 16: 5.8 vs 17.3 us) — profiles/r04/probe_mx_rows.log.  tuning[0] = 4 forces it past its
    // x re-read budget, 5 = the streaming kernel, 2 = the tile kernels.
    if ((a.tuning[0] == 4 || tuning_default(a)) && plan_mx_rows(a, r.gp, r.lp)) { r.kind = K_KMAJOR; return; }
    // 16-bit activations x block-scaled weights, 1 .. 64 rows (round 4): the A16W8 rows kernel with the scaled converters — while every
    // block's re-read of x (M K 2 bytes x N / 16 blocks) stays in budget.  tuning[0] = 4 forces it, 5 / 2 keep the streaming / tile kernels
    // (round 4, profiles/r04/probe_rows_vs_tiles*.log: against the tile kernel the crossover sits at M N K ~ 570 M for 4096^2-sized layers
    //  — M = 34; M = 64: 19.0 vs 13.0 us — and ~ 250 M for the larger ones: 8192^2 and 14336 x 4096 from 4 rows, M = 16: 25.4 vs 17.7)
    const bool mx16 = a.input_dtype == GEMLITE_DT_MXFP16 || a.input_dtype == GEMLITE_DT_MXBF16;
    const bool a16_over = mx16 && a.M >= 2 && a.M <= 64 && a.N % 128 == 0 && a.K % 128 == 0 &&
                          (int64_t)a.M * a.N * a.K > ((int64_t)a.N * a.K <= (32ll << 20) ? 570000000ll : 250000000ll);
    if (mx16 && a.M <= 64 && (a.tuning[0] == 4 || (tuning_default(a) && !a16_over)) &&
        plan_a16w8_rows(a, r.lp)) { r.kind = K_KMAJOR; return; }
    // 65 .. 384 (512) rows (round 4): 64 x 64 tiles, K unsplit; tuning[0] = 6 forces them, 2 keeps the 128-column kernel with its K slices
    // (profiles/r04/probe_mx_sq.log, `layer(x)` at 4096^2 / 8192^2 / 4096 x 14336 / 14336 x 4096: ahead or within 5 % everywhere up to 384
    //  rows — 4096^2 M = 256: fp8 27.2 -> 17.4 us, fp4 29.7 -> 13.7; at 512 rows for fp4 x fp4 and for one-round shapes)
    // Up to 64 rows they take what the few-row kernel's budget refuses (plan_mx_rows): fp4 x fp4 anywhere, fp8 activations from 128 column tiles.
    const bool sq_few = a.M >= 2 && a.M <= 64 && ((g.mx_x == MX_FP4 && g.mx_w == MX_FP4) || a.N / 64 >= 128);
    // Late round 6 (the tiles walk K in the rotated / grouped order now and are 10 - 25 % faster: profiles/r06/probe_mx_forms*.log): up to 1024 rows — MXFP8 4096^2 M = 768 / 1024
    // 62.5 / 52.2 (128-column tiles) -> 34.8 / 35.2 us, 8192^2 M = 512 / 1024 94.0 / 134.8 -> 82.7 / 127.3, 4096 x 14336 M = 512 87.1 -> 84.2; MXFP4 4096^2 M = 1024 37.9 -> 22.4, but
    // 8192^2 M = 1024 75.0 (256 x 256 tiles) vs 87.5.  2048 rows: the 256 x 256 tiles (59.3 vs 73.5, fp4 43.0 vs 46.3).
    // fp4 WEIGHTS (fp4 x fp4 and fp8 x fp4: 8192^2 M = 1024 111.9 (256 x 256) vs 119.7) above 512 rows only up to N K = 4096^2 (M = 1024: 38.9 -> 33.0).
    const bool mx_w4 = g.mx_w == MX_FP4;
    // ... and a long K (> 8192) under 320 .. 640 of these tiles goes back to the 128-row tiles, whose slice count now minimises rounds x slice length (plan_gemm_mx_mma;
    // profiles/r06/scan_mx_*.log, 20 LLM layer shapes x M = 128 .. 512): MXFP8 5120 x 13824 M = 256 / 512 62.0 / 134.0 -> 55.9 / 104.4 us, 2560 x 9728 M = 448 / 512 48.5 / 47.7 -> 40.3 / 43.4
    // (4096 x 11008 / x 14336 M = 448 / 512 stay although the slices are 7 - 14 % ahead there); fp4 weights only on the largest of them (fp8 x fp4 5120 x 13824: 49.1 / 86.8 -> 40.7 / 76.1; 2560 x 9728 M = 512 the other way, 29.8 vs 32.6)
    const int64_t sq_tiles = (a.N / 64) * ((a.M + 63) / 64);
    // Two of these tiles share a CU, so 257 .. 512 of them cost what 512 do: the hand-over only where they fill less than 0.7 of their last round (320 / 640 tiles: 0.625;
    // at 384 / 480 they win by 1.3 - 1.5x — M = 384 on the same layers, scan_mx_a8w8_long_k_*.log)
    const int64_t sq_slots = (sq_tiles + 511) / 512 * 512;
    // ... and only where one to three slices of the 128-row tiles fill >= 0.9 of one or two rounds of CUs (4096 x 14336 M = 320: 96 tiles x 2 = 0.75 -> 76.8 us vs 55.8 here)
    bool slices_fill = false;
    for (int64_t sk = 1, t128 = (a.N / 128) * ((a.M + 127) / 128), cus = gl::resident_block_limit(); sk <= 3 && sk * 1024 <= a.K && !slices_fill; ++sk) {
        const int64_t rounds = (t128 * sk + cus - 1) / cus;
        slices_fill = rounds <= 2 && t128 * sk * 10 >= rounds * cus * 9;
    }
    const bool long_k_slices = a.M > 128 && a.K > 8192 && a.N % 128 == 0 && sq_tiles > 256 && sq_tiles <= 720 && sq_tiles * 10 < sq_slots * 7 && slices_fill &&
                               (!mx_w4 || ((int64_t)a.N * a.K > (1ll << 26) && g.mx_x == MX_FP8));
    const bool sq_auto = sq_few || (a.M > 64 && !long_k_slices && (a.M <= 512 || (a.M <= 1024 && (!mx_w4 || (int64_t)a.N * a.K <= (1ll << 24)))));
    if ((a.tuning[0] == 6 || (tuning_default(a) && sq_auto)) && plan_gemm_mx_sq(a, r.gp, r.lp)) { r.kind = K_A8_MMA; return; }
    // decode sizes of what is left (K % 64 != 0 ...): the streaming kernel
    if ((a.tuning[0] == 5 || (a.tuning[0] == 0 && !a16_over)) && a.tuning[1] == 0 && a.tuning[2] == 0 && plan_mx_gemv(a, r.gp, r.lp)) { r.kind = K_KMAJOR; return; }
    // prefill sizes of the same-format pairs: 256 x 256 tiles, both operands through LDS (tuning[0] = 3 forces it at any M)
    if (plan_gemm_mx_tile(a, r.gp, r.lp)) { r.kind = K_A8_MMA; return; }
    if ((a.tuning[0] == 0 || a.tuning[0] == 2) && plan_gemm_mx_mma(a, r.gp, r.lp)) { r.kind = K_A8_MMA; return; }
    if ((a.tuning[0] == 0 || a.tuning[0] == 2) && (a.input_dtype == GEMLITE_DT_MXFP16 || a.input_dtype == GEMLITE_DT_MXBF16)) {
        // 16-bit activations: the tiled MFMA kernel of the integer formats with the block-scaled weight geometry
        WnParams p = kcontig_wn_params(a, a.x, a.stride_xm, g.epi, 32);
        p.epi.meta_dt = p.epi.out_dt;  // no channel scales: keeps the typed epilogue
        if (plan_gemm_wn_mma_mx(a, p, r.lp)) { r.kind = K_TILED_WN; r.wn = p; return; }
    }
    // fp8 / fp4 activations that no tile kernel took (K % 512 != 0 with fp4 activations ...): the few-row kernel over 64-row tiles
    if (a.tuning[0] == 0 && plan_mx_rows(a, r.gp, r.lp, true)) { r.kind = K_KMAJOR; return; }
    // NVFP4, 1 .. 64 rows (round 4): 16-column blocks, both operands expanded to fp16 in registers (tuning[0] = 2 keeps the tile kernel)
    if ((a.tuning[0] == 0 || a.tuning[0] == 4) && a.tuning[1] == 0 && a.tuning[2] == 0 && plan_nvfp4_rows(a, r.gp, r.lp)) { r.kind = K_KMAJOR; return; }
    // NVFP4 (round 4): both operands are exact in fp16 — x is expanded into the workspace by a small kernel in front, the weights in
    // the K loop of the fp16 MFMA tile kernel (Geo<NVW4>), the layer's constant output factor rides as a per-row scale.  Two launches
    // inside this call.  tuning[0] = 1 keeps the coverage kernel.
    if (a.input_dtype == GEMLITE_DT_NVFP4 && a.channel_scale_mode == 4 && (a.tuning[0] == 0 || a.tuning[0] == 2) &&
        ((uintptr_t)a.x % 8) == 0 && a.stride_xm % 8 == 0 && a.K % 128 == 0 && (int64_t)a.M * a.K < (1ll << 30)) {
        // planned on the fp16 expansion of x (scales_x stays the caller's: the expansion kernel reads it)
        gemlite_hip_forward_args b = a;
        b.input_dtype = GEMLITE_DT_MXFP16;
        b.x = (const void*)(uintptr_t)0x1000;  // (alignment checks only: the workspace copy is 256-byte aligned)
        b.stride_xm = a.K;
        WnParams p = kcontig_wn_params(a, nullptr, a.K, g.epi, 16);
        p.epi.c_mode = 2;  // out = acc * post[m]
        p.epi.scales_x = nullptr;
        p.epi.stride_sx_m = 1;
        p.epi.meta_dt = p.epi.out_dt;
        if (plan_gemm_wn_mma_mx(b, p, r.lp, 1)) {
            r.kind = K_NV_MMA;
            r.wn = p;
            r.nv_x16_bytes = (uint64_t)(((int64_t)a.M * a.K * 2 + 255) & ~(int64_t)255);
            r.lp.ws_bytes = COUNTER_BYTES + r.lp.slab_bytes + r.nv_x16_bytes + (uint64_t)((a.M * 4 + 255) & ~(int64_t)255);
            return;
        }
    }
    // past their budgets but no tile kernel took the shape (an alignment the tile kernels need ...): the few-row kernels after all,
    // before the coverage kernel
    if (tuning_default(a)) {
        gemlite_hip_forward_args f = a;
        f.tuning[0] = 4;
        if (a16_over && plan_a16w8_rows(f, r.lp)) { r.kind = K_KMAJOR; return; }
        if (a.input_dtype == GEMLITE_DT_NVFP4 && plan_nvfp4_rows(f, r.gp, r.lp)) { r.kind = K_KMAJOR; return; }
    }
    if (a.M > 65535) { r.status = GEMLITE_ERR_BAD_SHAPE; return; }
    take_kernel(r, K_GENERIC, mx_generic_kernel_fn(), "mx_generic_kernel", dim3((unsigned)((a.N + 255) / 256), (unsigned)a.M, 1), dim3(256, 1, 1));
}
static void resolve_mx(const gemlite_hip_forward_args& a, Resolved& r) {
    const GenericParams g = mx_params(a);  // (a copy of its own: the planners write into r.gp)
    r.gp = g;
    resolve_mx_plan(a, r, g);
}

// ---- family: one row of a block-scaled dynamic layer, quantiser inside the launch (mx_rows_kernel<..., FQ>) ----------------------------
static bool resolve_fused_quant_mx_row(const gemlite_hip_forward_args& a, Resolved& r) {
    const int mxdt = fused_quant_mx_dtype(&a);
    if (!mxdt) return false;
    r.status = GEMLITE_ERR_NO_FUSED_QUANT;
    if (!tuning_default(a) || a.matmul_type != GEMLITE_MATMUL_AUTO) return true;
    if (a.stride_xk != 1 || ((uintptr_t)a.x % 16) != 0) return true;
    const gemlite_hip_forward_args b = quantised_proxy(a, mxdt, mxdt == GEMLITE_DT_MXFP8 ? a.K : a.K / 2, mxdt == GEMLITE_DT_NVFP4 ? a.K / 16 : a.K / 32);
    GenericParams g = mx_params(b);
    LaunchPlan lp{};
    if (!(mxdt == GEMLITE_DT_NVFP4 ? plan_nvfp4_rows(b, g, lp, true) : plan_mx_rows(b, g, lp, false, true))) return true;
    g.x = a.x;                 // the raw row
    g.x_dt = a.input_dtype;    // ... and its type
    g.sx_blocks = a.channel_scale_mode == 4 ? a.x : nullptr;  // (non-null: block-scaled activations)
    r.status = GEMLITE_OK;
    return take(r, K_KMAJOR, g, lp);
}

// ---- family: M = 1 of a dynamically quantised PACKED layer with the activation quantiser inside the launch (gemv_a8wn.hip) ---------------
static bool resolve_fused_quant_packed_row(const gemlite_hip_forward_args& a, Resolved& r) {
    const int qdt = fused_quant_packed_dtype(&a);
    if (!qdt) return false;
    r.status = GEMLITE_ERR_NO_FUSED_QUANT;
    if (!tuning_default(a) || a.matmul_type != GEMLITE_MATMUL_AUTO) return true;
    if (a.stride_xk != 1 || ((uintptr_t)a.x % 16) != 0 || a.output_dtype != a.input_dtype || a.w_pack_bits != 32 || a.stride_wn != 1 || a.stride_on != 1) return true;
    // Unlike the metadata rule of resolve(), this one does not exclude zeros beside channel scales (W_group_mode 1 under channel_scale_mode 3
    // keeps per-group rows here).  The code gives no reason for the difference: it is kept as it was.
    const bool pgm = a.W_group_mode >= 2 || ((a.W_group_mode == 1) && !a.zero_is_scalar);
    const int eg = pgm ? a.group_size : (int)a.K;
    if (eg <= 0 || a.K % eg != 0 || (a.stride_meta_n != 1 && pgm)) return true;
    const gemlite_hip_forward_args b = quantised_proxy(a, qdt, a.K, a.stride_sx_m);
    // M = 1 and stride_xk = 1 were checked above; the row stride of the one row is the proxy's
    WnParams p = packed_wn_params(a, a.K, pgm, eg);
    LaunchPlan lp{};
    if (p.gs_shift < 0 || !plan_gemv_a8wn(b, p, lp, true)) return true;
    r.status = GEMLITE_OK;
    return take(r, K_GEMV_WN, p, lp);
}

// When gemm_w4_rows_kernel (gemm_wn_rows.hip, round 5) is the default for A16W4 (profiles/r05/probe_rows5_v2*.log: 14 layer shapes x
// M = 2 .. 64 against the round-4 choice, graph-replayed layer(x) in us):
//   * its 16-column blocks hold 146 KB of LDS, so one block per CU: it pays while ONE round of blocks covers N (N / 16 <= CUs: N <= 4096 —
//     4096^2 M = 16 / 32 / 64: 7.4 / 12.2 / 12.9 -> 6.8 / 8.5 / 11.0, 3584 x 4096: 9.0 / 12.0 / 14.8 -> 6.7 / 8.5 / 11.1; at N = 5120 ..
//     14336 two or three rounds lose 1.3 - 2.2x).  From 192 column tiles at any row count below, from 128 (N = 2048) with 16 .. 32 rows;
//   * every block re-reads all of x through L2 -> LDS: past ~176 MB per launch the tile kernels win (4096 x 11008: M = 32 17.7 -> 17.2,
//     M = 48 19.9 -> 21.5; 4096 x 8192 M = 64, 256 MB: 18.3 -> 19.0);
//   * weights are requested two chunks (2 KB per wave) ahead: enough for K <= 12288, not for K = 14336 (M = 16: 14.6 -> 16.3);
//   * from how many rows: K <= 2048 from 2 (4096 x 1024 / x 2048, M = 2: 5.0 / 5.1 -> 3.7 / 4.4); K <= 4096 from 8 (2 .. 7 rows are a
//     draw with the MFMA GEMV / the registers-only kernel: 6.2 - 6.9 vs 6.1 - 6.5); longer K from 2 again since the x pieces are requested
//     ahead of the weights (probe_rows5_v2b*.log: 4096 x 8192 M = 2 / 8 / 16 / 32: 10.1 / 9.3 / 10.5 / 15.6 -> 8.8 / 9.4 / 10.2 / 13.0;
//     4096 x 11008: 12.8 / 17.0 / 17.1 / 17.8 -> 10.5 / 11.4 / 12.3 / 16.7; 3072 x 8192: 9.0 / 11.2 / 14.0 / 15.3 -> 8.7 / 9.4 / 10.1 / 12.8).
//   * 4096 < N <= 8192 (N % 32 = 0, groups of >= 64): TWO column tiles per block (N / 32 resident blocks, an x piece read from LDS feeds both;
//     probe_rows5_nt2*.log) — each CU then streams twice the weights through the same 8 waves, which loses below 17 rows against the
//     registers-only kernel (8192^2 M = 16: 12.5 -> 16.0) and wins where that kernel's K-slice combine or the 32-row tile kernel took over:
//     17 .. 32 rows (8192^2 19.5 -> 18.5, 8192 x 4096 13.6 -> 11.9, 6144 x 4096 13.4 -> 11.4, 5120^2 15.5 -> 13.4; groups of 64 in bf16 at
//     6144 x 4096: 33.5 -> 12.1 — the round-4 planner fell to the LDS-staged streaming kernel there), and 8 .. 64 rows over K <= 2048
//     (8192 x 2048: 6.6 / 7.4 / 9.0 / 11.0 -> 6.2 / 6.3 / 7.3 / 9.4).  Groups of 64 over K > 4096 stay (8192^2 M = 32: 19.0 -> 20.3).
//   * 2-bit words (A16W2, BitNet A16W158; late round 5, probe_rows5_w2*.log): the same kernel, 512 k per chunk.  4096^2 M = 16 / 32 / 48 / 64:
//     6.8 / 11.6 / 12.2 / 12.3 -> 6.1 / 7.6 / 8.8 / 10.1; 3584 x 4096: 7.9 / 11.6 / 13.8 / 14.0 -> 6.0 / 7.5 / 8.7 / 10.1; 4096 x 2048 from 8 rows
//     (5.4 / 6.4 / 8.9 / 9.8 -> 4.4 / 4.5 / 5.5 / 7.1; 2 - 4 rows lose 0.1 - 0.3); 4096 x 14336 up to 32 rows (M = 32: 21.4 -> 17.8; 48 / 64 lose);
//     2048 x 8192 16 .. 32 rows (9.9 / 13.7 -> 9.0 / 11.5); groups of 64 hold 32 rows per block (M = 64 along grid.y loses: 11.6 -> 13.7);
//     one column tile per block only (N <= 4096).
//   * narrow layers (64 <= N / 16 < 192 tiles: the k / v projections of grouped-query models; probe_rows5_narrow_layers.log, 4-bit / 2-bit):
//     K <= 4096 from 8 rows (1024 x 4096 M = 16 / 32 / 64: 7.2 / 10.7 / 12.7 -> 6.3 / 7.7 / 10.6; 2-bit 6.8 / 10.4 / 12.7 -> 5.7 / 6.8 / 9.6;
//     1536 x 4096 the same), K <= 2048 from 4 (1024 x 2048 M = 32 / 64: 8.8 / 10.6 -> 5.0 / 6.7); a longer K only where the registers-only
//     kernel's K-slice combine ends: 16 (128 tiles) / 17 .. 32 rows (1024 x 8192 M = 32: 15.4 -> 12.3; M = 8 / 16 / 64 lose 0.6 - 0.8 us)
static bool rows5_narrow_layer_pays(int64_t M, int64_t tiles, int64_t K) {
    if (tiles < 64) return false;
    if (K <= 4096) return M >= (K <= 2048 ? 4 : 8);
    return M >= (tiles >= 128 ? 16 : 17) && M <= 32;
}
static bool rows5_pays_w2(int64_t M, int64_t N, int64_t K, int gs_shift) {
    if (M < 2 || M > 64 || N % 16 != 0 || K % 512 != 0 || K > 16384) return false;
    const int64_t tiles = N / 16;
    if (tiles > gl::resident_block_limit()) return false;
    const bool g64_two_tiles = gs_shift == 6 && M >= 17 && M <= 32;
    if (tiles < 192 && !(g64_two_tiles && tiles >= 32) && !rows5_narrow_layer_pays(M, tiles, K)) return false;
    if (gs_shift == 6 && M > 32) return false;
    if (gs_shift < 6) return false;  // (groups of 32: 16 rows per block — only where nothing else applies)
    if (M < (K <= 2048 ? 8 : 2)) return false;
    const int64_t bytes = tiles * ((M + 15) / 16 * 16) * K * 2;
    return bytes <= (192ll << 20) || (M <= 32 && bytes <= (256ll << 20));  // (4096 x 8192 M = 48, 192 MiB: 17.6 -> 14.4 us)
}
static bool rows5_pays(int64_t M, int64_t N, int64_t K, int gs_shift) {
    if (M < 2 || M > 64 || N % 16 != 0 || K > 12288) return false;
    const int64_t tiles = N / 16, resident = gl::resident_block_limit();
    if (tiles > resident) {
        if (N % 32 != 0 || tiles / 2 > resident || gs_shift < 6) return false;
        if (K <= 2048 ? M < 8 : (M < 17 || M > 32)) return false;
        if (gs_shift == 6 && (K > 4096 || M > 32)) return false;
        return (tiles / 2) * ((M + 15) / 16 * 16) * K * 2 <= (176ll << 20);
    }
    // groups of 64 at 17 .. 32 rows have no registers-only kernel behind them (only the 32-row MFMA tiles: 1024 x 4096 11.8 vs 7.8 us here)
    const bool g64_two_tiles = gs_shift == 6 && M >= 17 && M <= 32;
    if (tiles < 192 && !(g64_two_tiles && tiles >= 32) && !rows5_narrow_layer_pays(M, tiles, K)) return false;
    const int64_t min_m = (K > 2048 && K <= 4096) ? 8 : 2;
    if (M < min_m) return false;
    return tiles * ((M + 15) / 16 * 16) * K * 2 <= (176ll << 20);
}

// ---- family: specialised packed-weight kernels -----------------------------------------------------------------------------------------
// Group size not a power of two.  Multiples of 32 (round 6, VERDICT r5 #8: the reference only asks for K % group == 0, core.py:253-271) run on
// the 8-wave tile kernel at every M — its metadata row index is wave-uniform, so k / group is one scalar multiply-high (gs_magic); 32-row tiles
// carry two (scale, zero) pairs per 64-k sub-block when the group is an odd multiple of 32.  Everything else: the coverage kernel.
static bool resolve_packed_odd_group(const gemlite_hip_forward_args& a, WnParams& p, bool want_gemv, Resolved& r) {
    const int mt = a.matmul_type, eff_group = p.group_size;
    LaunchPlan lp{};
    if (eff_group % 32 == 0 && eff_group > 32 && a.K % eff_group == 0 && (int64_t)a.K * eff_group < (1ll << 40) &&
        a.tuning[0] == 0 && (mt == GEMLITE_MATMUL_AUTO || mt == GEMLITE_MATMUL_GEMM || mt == GEMLITE_MATMUL_GEMM_SPLITK)) {
        const uint32_t d = (uint32_t)(eff_group / 32);
        p.gs_magic = (uint32_t)(((1ull << 32) + d - 1) / d);
        // one row: the dot-product GEMV (a lane's 32-k span lies inside one group; the same multiply-high per lane and chunk) — the reference's
        // GEMV runs a group of 96 at 4096 x 3072 in 7.9 us, the 32-row tile below needs 12.4 (profiles/r06/reference_triton_mi355x_r6.json)
        if (want_gemv && a.tuning[1] == 0 && a.tuning[2] == 0 && plan_gemv_wn(a, p, lp)) return take(r, K_GEMV_WN, p, lp);
        if (plan_gemm_wn_mma(a, p, lp)) return take(r, K_TILED_WN, p, lp);
    }
    return false;
}

static bool resolve_packed_words(const gemlite_hip_forward_args& a, bool per_group_meta, int eff_group, Resolved& r) {
    const bool x16 = a.input_dtype == GEMLITE_DT_FP16 || a.input_dtype == GEMLITE_DT_BF16;
    const bool x8 = a.input_dtype == GEMLITE_DT_FP8E4 || a.input_dtype == GEMLITE_DT_INT8;  // A8Wn dynamic / BitNet int8
    // (8- / 16-bit packed words, round 7: every planner below declines the widths it has no word source for — only gemm_wn_mma.hip and
    //  gemv_wn.hip take them — so the order of the calls cannot send them to an int32-only kernel; what none takes falls to the coverage kernel)
    if (!(a.elements_per_sample > 1 && (a.w_pack_bits == 32 || a.w_pack_bits == 16 || a.w_pack_bits == 8) && (x16 || x8) && a.stride_wn == 1 && a.stride_xk == 1 && a.stride_on == 1 &&
          (a.stride_meta_n == 1 || !per_group_meta) && (a.K % eff_group == 0))) return false;
    WnParams p = packed_wn_params(a, a.stride_xm, per_group_meta, eff_group);
    const int mt = a.matmul_type;
    const bool want_gemv = (mt == GEMLITE_MATMUL_GEMV || mt == GEMLITE_MATMUL_GEMV_REVSPLITK ||
                            mt == GEMLITE_MATMUL_GEMV_SPLITK || (mt == GEMLITE_MATMUL_AUTO && a.M <= 1));
    if (p.gs_shift < 0) return resolve_packed_odd_group(a, p, want_gemv, r);
    LaunchPlan lp{};
    // 2 .. 64 rows of 8-bit activations x packed weights (round 4): 16-column blocks on the 16-row fp8 / int8 MFMA.  (From 2 rows, not 5:
    // the streaming GEMV below re-reads the weights per row pair — 4096^2 M = 4 `layer(x)` 14.1 vs 9.5 us, 2-bit 14336 x 4096 M = 3 74.7 vs
    // 16.0, profiles/r04/probe_a8wn_fewrows.log.)  tuning[0] = 4 forces it at one row, 7 keeps the GEMV up to 4 rows.
    if (x8 && (want_gemv || mt == GEMLITE_MATMUL_AUTO) && a.tuning[1] == 0 && a.tuning[2] == 0 &&
        (a.tuning[0] == 4 || (a.tuning[0] == 0 && a.M >= 2)) && plan_a8wn_rows(a, p, lp)) {
        return take(r, K_GEMV_WN, p, lp);
    }
    // decode sizes of 8-bit activations x packed weights (A8Wn fp8 dynamic, BitNet int8): per-weight cast to the activation type
    // (one row by default; 2 .. 4 rows only as the A/B switch tuning[0] = 7: past the rows kernel's budget the tile kernel is the faster one)
    if (x8 && a.M <= (a.tuning[0] == 7 ? 4 : 1) && (want_gemv || mt == GEMLITE_MATMUL_AUTO) && (a.tuning[0] == 0 || a.tuning[0] == 7) && a.tuning[1] == 0 && a.tuning[2] == 0 &&
        plan_gemv_a8wn(a, p, lp)) {
        return take(r, K_GEMV_WN, p, lp);
    }
    // round 5: 2 .. 64 rows of 16-bit activations x 4- / 2-bit words on the decode-shaped MFMA rows kernel (gemm_wn_rows.hip): 16-column
    // blocks, K unsplit, weights requested first, x through LDS in whole cache lines.  Every block re-reads all of x (M K 2 bytes through
    // the CU's L2 -> LDS path), so the default stops at a budget on that traffic; groups of 32 and N % 64 != 0 — which no other
    // specialised kernel takes at M >= 2 — always come here (any M: row blocks along grid.y).  tuning[0] = 9 forces the kernel
    // (tuning[1] = 1 / 2 column tiles per block), GEMLITE_TF_NO_ROWS_KERNEL keeps the round-4 choice (A/B runs).
    if (x16 && (a.W_nbits == 4 || a.W_nbits == 2) && (mt == GEMLITE_MATMUL_AUTO || mt == GEMLITE_MATMUL_GEMM_SPLITK || (mt == GEMLITE_MATMUL_GEMM && a.tuning[0] == 9)) &&
        !(caller_flags(a) & GEMLITE_TF_NO_ROWS_KERNEL) && (a.tuning[0] == 9 || (tuning_default(a) && a.M >= 2))) {
        // nothing FASTER behind this one.  2-bit groups of 32 and N % 64 != 0: only the coverage kernel.  4-bit groups of 32 over N % 64 == 0 do have
        // gemm_wn_stream_kernel behind them (round 4's choice) and ADVICE r5 asked to hand M > 64 back to it, because the rows kernel re-streams
        // the weights once per 32-row block there — measured (round 6, profiles/r06/probe_g32_rows_vs_stream.log, layer(x) in us, rows / stream):
        // 4096^2 M = 64 17.0 / 114, M = 128 31.9 / 184, M = 256 61.5 / 324, M = 1024 242 / 1242; 8192^2 M = 256 208 / 1244; 11008 x 4096 M = 256
        // 172 / 926 — the rows kernel is 5 - 7 x faster at every M, so it keeps every group-32 layer.  (What these layers lack at M > 64 is a
        // group-32 form of the MFMA tile kernel: 61.5 us against 16.8 for groups of 128 at 4096^2 M = 256.)
        // Round 6, later: groups of 32 also have the 32-row tiles of the 8-wave kernel (template parameter NGS = 2, gemm_wn_mma.hip) — for M > 32
        // over N % 128 == 0, K % 256 == 0 they win (4096^2, rows / tiles: M = 128 31.4 / 17.6, M = 256 61.6 / 25.4, M = 1024 244 / 89.9 us;
        // profiles/r06/probe_g32_w4.log), so the rows kernel keeps groups of 32 up to its 32 rows per block and wherever the tiles do not apply.
        // (profiles/r06/probe_g32_w4_m33_64.log, rows / tiles: 4096^2 M = 40 .. 64 16.8 .. 17.3 / 13.2; 8192^2 M = 40 .. 64 52 / 27 and M = 24 / 32
        //  27.5 / 18.3; 11008 x 4096 M = 40 .. 64 47.5 / 30 — from 17 rows where the rows kernel's N / 16 blocks need more than one round)
        const bool g32_tiles = p.gs_shift == 5 && a.N % 128 == 0 && a.K % 256 == 0 &&
                               (a.M > 32 || (a.M > 16 && a.K >= 2048 && a.N / 16 > gl::resident_block_limit()));
        const bool only_here = (p.gs_shift == 5 && !g32_tiles) || a.N % 64 != 0;
        const bool in_budget = a.W_nbits == 4 ? rows5_pays(a.M, a.N, a.K, p.gs_shift) : rows5_pays_w2(a.M, a.N, a.K, p.gs_shift);
        // the group-32 tiles take the layer only if their planner accepts this request (an output or x alignment it declines would
        // otherwise drop the layer to the streaming kernel, 5 - 7 x behind the rows kernel): ask it first, keep the rows kernel if not
        bool tiles_take = false;
        if (g32_tiles) {
            WnParams pt = p;
            LaunchPlan lt{};
            tiles_take = plan_gemm_wn_mma(a, pt, lt);
        }
        if (a.tuning[0] == 9 || only_here || (in_budget && !g32_tiles) || (g32_tiles && !tiles_take)) {
            WnParams pr = p;
            LaunchPlan lr{};
            if (plan_gemm_wn_rows(a, pr, lr)) return take(r, K_STREAM_WN, pr, lr);
        }
    }
    // Decode on the matrix core (gemv_mfma.hip, round 3) where it measured faster than the dot-product family
    // (profiles/r03/probe_gemv3_*.log, us per launch in a replayed graph):
    //   4-bit, M = 1: 32-column tiles over a long K (8192^2: 9.9 vs 10.4).  Not the 16-column shapes (4096^2: 5.8 vs 4.8 for the
    //     dot-product decode kernel), not 64-column tiles (16384^2: 25.3 vs 23.7), not 32-column tiles over K = 4096 (9.3 vs 8.9);
    //   2-bit, M = 1: 16- and 32-column tiles (4096^2 4.4 vs 4.9, 8192^2 7.4 vs 8.6, 11008 x 4096 6.1 vs 8.2; 16384^2 18.0 vs 17.4: no);
    //   4-bit, 2..4 rows: N < 12288 (4096^2: 5.8 - 6.2 vs 6.4 - 7.5 for gemm_wn_direct, 6144 x 4096 5.9 vs 7.4, 5120 x 13824 17.1 vs 21.2,
    //     1536 x 8960 10.7 vs 14.9) except a long K over a narrow N, which takes the registers-only kernel with 64-column tiles and
    //     K slices (4096 x 14336 11.7 vs 16.5, 8192 x 28672 22.2 vs 28.5); N >= 12288: the registers-only kernel's 64-column tiles
    //     unsplit (13824 x 5120 10.9 vs 11.6 .. 17.6, 28672 x 8192 21.9 vs 30.5) — profiles/r03/probe_m4_llm_shapes_*.log.
    // GEMLITE_TF_NO_MFMA_GEMV = never, GEMLITE_TF_FORCE_MFMA_GEMV = wherever it applies (A/B runs).
    if (x16 && a.W_nbits == 4 && a.M >= 2 && a.M <= 4 && mt == GEMLITE_MATMUL_AUTO && tuning_default(a) &&
        !(caller_flags(a) & GEMLITE_TF_FORCE_MFMA_GEMV) && a.K >= 12288 && a.N <= 8192 && a.N % 64 == 0 && a.N / 64 >= 40) {
        gemlite_hip_forward_args a2 = a;
        a2.tuning[0] = 4;
        a2.tuning[1] = a.N / 64 >= 128 ? 2 : 4;
        WnParams pd = p;
        LaunchPlan ld{};
        if (plan_gemm_wn_direct(a2, pd, ld)) return take(r, K_STREAM_WN, pd, ld);
    }
    if (x16 && !(caller_flags(a) & GEMLITE_TF_NO_MFMA_GEMV) && a.tuning[1] == 0 &&
        ((want_gemv && a.M == 1 && mt != GEMLITE_MATMUL_GEMV_SPLITK) || (a.M >= 2 && a.M <= 4 && mt == GEMLITE_MATMUL_AUTO))) {
        WnParams pm = p;
        LaunchPlan lm{};
        if (plan_gemv_mfma(a, pm, lm)) {
            const int cols = (int)(a.N / lm.grid.x);
            // (round 3 sweep over 22 LLM shapes: 4-bit M = 1 also wins on every 6144 <= N <= 12288 with K <= 8192 — 6144 x 4096 5.6
            //  vs 7.0 us, 8192 x 3072 5.6 vs 6.2, 8960 x 1536 5.1 vs 5.5, 11008 x 4096 7.9 vs 8.5 — and loses on narrow N, K > 8192
            //  under 64-column tiles, and N >= 13824)
            // Round 6: with gemv_wn_kernel on counted asm loads (no drain at the head of its chunk loop) the dot-product family is ahead at ONE row
            // on 20 of 22 LLM shapes for 4-bit words (8192^2 9.14 vs 9.86 us, 12288 x 4096 7.76 vs 8.56, 11008 x 4096 7.70 vs 7.98; 6144 x 4096
            // 5.73 vs 5.49 the other way) and on 16 of 22 for 2-bit words (5120^2 5.65 vs 7.17, 13824 x 5120 7.26 vs 9.00, 28672 x 8192 16.2 vs 20.6,
            // 8192^2 7.07 vs 7.87) — profiles/r06/probe_m1_shapes_w{4,2}.log.  The matrix-core GEMV keeps one row only for 2-bit words over a K that
            // is not a multiple of 1024 (K = 8960 / 9728 / 11008: 7.26 vs 8.04, 7.84 vs 8.22, 8.29 vs 9.16), and 2 .. 4 rows as before.
            (void)cols;
            const bool wins = a.M >= 2 ? (a.W_nbits != 4 || a.N < 12288) : (a.W_nbits == 2 && a.K % 1024 != 0);
            if ((caller_flags(a) & GEMLITE_TF_FORCE_MFMA_GEMV) || a.tuning[0] != 0 || wins) return take(r, K_GEMV_WN, pm, lm);
        }
    }
    if (want_gemv && plan_gemv_wn(a, p, lp)) return take(r, K_GEMV_WN, p, lp);
    if (!want_gemv) {
        // Many rows: the 8-wave MFMA kernel (all bit widths) from 33 rows.  tuning[0]: 1 = LDS-staged streaming kernel,
        // 2 = the 4-wave tiled kernel of round 1 (4-bit only; kept for A/B runs)
        const bool want_tiled = (mt == GEMLITE_MATMUL_GEMM || (mt == GEMLITE_MATMUL_AUTO && a.M > 32));
        if (want_tiled && a.tuning[0] == 0 && plan_gemm_wn_mma(a, p, lp)) return take(r, K_TILED_WN, p, lp);
        if (want_tiled && a.tuning[0] != 1 && plan_gemm_wn_tiled(a, p, lp)) return take(r, K_TILED_WN, p, lp);
        // 17..32 rows over a long K: the 8-wave kernel's LDS-staged x beats the
        // registers-only kernel, whose blocks each re-read their K range of every row from L2 (M = 32: N 5120 x K 13824
        // 25.3 vs 39.8 us, 8192 x 28672 51 vs 72, 28672 x 8192 49.5 vs 60; K <= 5120 the other way round —
        // profiles/r02/autotune_report.json)
        const bool long_k = mt == GEMLITE_MATMUL_AUTO && a.W_nbits == 4 && a.tuning[0] == 0 && a.tuning[2] == 0 &&
                            a.M > 16 && a.K >= 8192;
        if (long_k && plan_gemm_wn_mma(a, p, lp)) return take(r, K_TILED_WN, p, lp);
        // few rows: registers-only MFMA path (tuning[2] == 1 keeps the LDS-staged streaming kernel)
        if (a.M <= 32 && a.tuning[2] != 1 && a.tuning[0] != 3 && plan_gemm_wn_direct(a, p, lp)) return take(r, K_STREAM_WN, p, lp);
        // 17 .. 32 rows the registers-only kernel refuses (groups of 64 — hqq's default — need one row tile there): rounds 2-4 fell to the
        // LDS-staged streaming kernel, 1.3 - 2.2x behind the 32-row MFMA tiles (profiles/r05/probe_g64_m17_32_w{4,2}.log, 4-bit / 2-bit:
        // 4096^2 16.3 / 15.7 -> 12.9 / 11.9 us, 6144 x 4096 2-bit 23.1 -> 12.2, 11008 x 4096 31.4 / 31.0 -> 16.5 / 22.6, 8192^2 2-bit 25.3 -> 17.2);
        // a short K keeps the streaming kernel (8960 x 1536: 10.6 vs 11.1)
        if (mt == GEMLITE_MATMUL_AUTO && a.M > 16 && a.K >= 2048 && tuning_default(a) && !(caller_flags(a) & GEMLITE_TF_NO_ROWS_KERNEL) &&
            plan_gemm_wn_mma(a, p, lp)) return take(r, K_TILED_WN, p, lp);
        if (a.tuning[0] != 3 && plan_gemm_wn_stream(a, p, lp)) return take(r, K_STREAM_WN, p, lp);
        // shapes the few-row kernels do not take (K = 11008, 8960, ...): small tiles of the MFMA kernel, never the
        // coverage kernel (tuning[0] == 3 forces this path for A/B runs)
        if (plan_gemm_wn_mma(a, p, lp)) return take(r, K_TILED_WN, p, lp);
    }
    // AUTO with small M that the GEMV planner rejected may still fit the streaming kernel
    if (want_gemv && mt == GEMLITE_MATMUL_AUTO && plan_gemm_wn_stream(a, p, lp)) return take(r, K_STREAM_WN, p, lp);
    // what none of the above takes at M = 1 — 8-bit activations x packed weights (A8Wn dynamic, BitNet int8), an output
    // or channel-scale type that differs from the activations' — still has the 8-wave MFMA kernel (32-row tiles)
    if (want_gemv && plan_gemm_wn_mma(a, p, lp)) return take(r, K_TILED_WN, p, lp);
    return false;
}

// ---- the unpacked families (elements_per_sample == 1).  They plan into r.gp, which holds the coverage kernels' parameters, and r.lp ------
static GenericParams coverage_params(const gemlite_hip_forward_args& a, bool per_group_meta, int eff_group) {
    GenericParams g = generic_head(a);
    g.zeros = a.zeros;
    g.group_size = eff_group; g.w_mode = a.W_group_mode;
    g.meta_dt = a.meta_dtype; g.zeros_dt = a.zeros_dtype; g.zero_is_scalar = a.zero_is_scalar;
    g.int_acc = (a.input_dtype == GEMLITE_DT_INT8 && (a.elements_per_sample > 1 || a.w_dtype == GEMLITE_DT_INT8)) ? 1 : 0;
    g.stride_meta_g = per_group_meta ? a.stride_meta_g : 0;
    g.stride_meta_n = per_group_meta ? a.stride_meta_n : ((a.W_group_mode == 1 && !a.zero_is_scalar) ? 1 : 0);
    return g;
}

// family: a dynamically quantised 8-bit layer with the activation quantiser inside the launch
static bool resolve_fused_quant_unpacked(const gemlite_hip_forward_args& a, Resolved& r) {
    if (!wants_fused_quant(&a)) return false;
    // 2 <= M <= 64 of a dynamically quantised layer: the rows kernel with producer blocks in front that quantise x (gl_coopquant.h).
    // Planned on the arguments the matmul will see — 8-bit x [M, K] (row stride K) and fp32 scales in the workspace; the pointers
    // are filled in at launch.  GEMLITE_ERR_NO_FUSED_QUANT: ask again with quantised x and scales_x (two launches).
    if (a.M >= 2) {
        r.status = GEMLITE_ERR_NO_FUSED_QUANT;
        if (!tuning_default(a) || a.matmul_type != GEMLITE_MATMUL_AUTO) return true;
        if (a.M > cq::MAX_ROWS || a.stride_xk != 1 || a.K % 16 != 0 || a.stride_xm % 8 != 0 || ((uintptr_t)a.x % 16) != 0) return true;
        const gemlite_hip_forward_args b = quantised_proxy(a, a.w_dtype, a.K, 1);
        LaunchPlan lp{};
        GenericParams gq = r.gp;
        if (a.M > 64 || !plan_a8w8_rows(b, lp, true)) return true;
        gq.x = nullptr; gq.x_dt = a.w_dtype; gq.stride_xm = a.K; gq.stride_xk = 1;
        gq.int_acc = a.w_dtype == GEMLITE_DT_INT8 ? 1 : 0;
        gq.epi.scales_x = nullptr; gq.epi.stride_sx_m = 1;
        gq.cq_x = a.x; gq.cq_stride_xm = a.stride_xm; gq.cq_xdt = a.input_dtype;
        gq.flags = caller_flags(a);
        r.status = GEMLITE_OK;
        return take(r, K_A8_FQ, gq, lp);
    }
    // M = 1 of a dynamically quantised layer with the activation quantisation fused into the prologue
    if (a.stride_wk != 1 || a.stride_xk != 1 || a.K % 16 != 0 || a.stride_wn % 16 != 0 || a.K > 65536 ||
        (((uintptr_t)a.w_q | (uintptr_t)a.x) % 16) != 0) { r.status = GEMLITE_ERR_NO_FUSED_QUANT; return true; }
    // round 4: one wave per column with the whole weight row requested BEFORE the block quantises x (a8w8_decode_kernel);
    // tuning[0] = 7 keeps the round-2 kernel, which quantises first
    // (profiles/r04/probe_a8w8_decode.log: int8 faster on all 8 shapes tried, 4096^2 7.27 -> 6.18 us, 4096 x 14336 18.9 -> 14.5; fp8 —
    //  8 converter + 16 fma instructions per 16 bytes — only while the tiles are one round of blocks: 4096^2 7.80 -> 6.62, but
    //  8192^2 17.3 -> 18.9, 16384^2 54.5 -> 58.7)
    const bool dec_ok = a.tuning[0] != 7 && a.K % 1024 == 0 && a.N % 16 == 0 && (a.w_dtype == GEMLITE_DT_INT8 || a.N <= 4096 || a.tuning[0] == 8);
    if (dec_ok && a.stride_on == 1 && a.K <= 61440)
        return take_kernel(r, K_KMAJOR, a8w8_decode_kernel_fn(a.w_dtype, true), "a8w8_decode_fused_quant_kernel<tile16,16w>", dim3((unsigned)(a.N / 16), 1, 1),
                           dim3(1024, 1, 1), (size_t)a.K + 64);
    return take_kernel(r, K_KMAJOR, kmajor_fused_quant_kernel_fn(a.w_dtype), "kmajor_fused_quant_kernel", dim3((unsigned)((a.N + 7) / 8), 1, 1), dim3(512, 1, 1),
                       (size_t)((a.K + 15) & ~15) + 64);
}

// When the unsplit 64 x 64 A8W8 tiles are the default (profiles/r04/probe_a8w8_sq*.log; everything else keeps the round-3 kernels):
// more than 64 rows and at most one round of tiles over the CUs (4096^2 int8: M = 65 .. 256 17.0 .. 21.7 -> 11.2 .. 13.6 us, 8192^2 M = 128
// 28.4 -> 24.2), or up to two rounds of a short K with two blocks per CU (4096^2 M = 384 / 512: 31.5 / 23.9 -> 19.3 / 21.5 us; at
// K = 8192 two rounds lose: 8192^2 M = 256 39.4 vs 34.4)
// Up to 64 rows (one row tile) they take what the rows kernel's budget refuses from 128 column tiles (plan_a8w8_rows).
static bool a8w8_sq_pays(const gemlite_hip_forward_args& a) {
    if (a.N % 64 != 0) return false;
    if (a.M <= 64) return a.M >= 2 && a.N / 64 >= 128 && a.N / 64 <= 512;
    const int64_t tiles = (a.N / 64) * ((a.M + 63) / 64);
    // late round 6 (profiles/r06/scan_a8w8_*.log, 20 LLM layer shapes x M = 96 .. 512): two rounds hold up to K = 8192 since the requests sit between
    // the MFMAs and the row tiles rotate their K order (8192^2 M = 256: 35.4 -> 32.7 us, 13824 x 5120 M = 128: 37.9 -> 25.0, 3072 x 8192 M = 512:
    // 43.4 -> 27.2; K = 11008 / 13824 still lose: 4096 x 11008 M = 512 58.8 vs 43.7); a very long K under few tiles goes to the K slices of the
    // 128 x 128 tiles (4096 x 14336 M = 96 / 128: 28.2 / 30.6 -> 26.4 / 27.5; M = 256 stays: 30.4 vs 38.2)
    if (a.K >= 14336 && a.M <= 128 && tiles <= 128 && a.N % 128 == 0) return false;
    return tiles <= 256 || (tiles <= 512 && a.K <= 8192);
}

// When the unsplit 128 x 128 A8W8 tiles are the default (profiles/r05/probe_a8w8_sq128.log): more than 64 rows, and the 128 x 128 tiles
// number 192 .. 256 — one round with most CUs busy (FP8 16384^2 M = 256: 95.8 vs 98.5 us; int8 8192^2 M = 512: 47.0 vs 52.7;
// 4096^2 M = 1024: 27.5 vs 32.2; 14336 x 4096 M = 256: 29.0 vs 31.1).  Fewer tiles (8192^2 M = 256: 44.5 vs 36.1 us) and several rounds
// (8192^2 M = 1024: 89.8 vs 76.3) stay on the 128- / 256-row tiles with K slices.  Late round 6: from 160 tiles (11008 x 4096 M = 256, 172 tiles: 38.4 -> 28.1 us;
// 128 tiles still lose: 8192^2 M = 256 44.6 vs 34.2 — profiles/r06/probe_a8w8_forms.log).
static bool a8w8_sq128_pays(const gemlite_hip_forward_args& a) {
    // From 144 tiles (6144 x 4096 M = 384: 36.2 -> 26.1 us); a short K (< 4096) only where the 64 x 64 tiles would need more than two rounds
    // (8192 x 2048 / x 3072 M = 384: 30.0 / 33.5 -> 17.9 / 23.1; 8960 x 1536 M = 256, 140 tiles: 28.5 -> 16.4) — profiles/r06/scan_a8w8_*.log.
    if (a.M <= 64 || a.N % 128 != 0) return false;
    const int64_t tiles = (a.N / 128) * ((a.M + 127) / 128);
    if (a.K < 4096) return tiles >= 136 && tiles <= gl::resident_block_limit() && (a.N / 64) * ((a.M + 63) / 64) > 512;
    return tiles >= 144 && tiles <= gl::resident_block_limit();
}

// family: A8W8 (int8 / fp8) rows and tiles.  A GEMV matmul_type skips them all
static bool resolve_a8w8(const gemlite_hip_forward_args& a, Resolved& r) {
    if (!gemm_kind(a)) return false;
    // A8W8 (int8 / fp8), 2..16 rows: 16-column blocks, one 16-row MFMA per 64-k chunk (tuning[0] = 4 forces it at M = 1 too,
    // any other non-zero tuning[0] skips it)
    if ((a.tuning[0] == 4 || (tuning_default(a) && a.M >= 2)) && plan_a8w8_rows(a, r.lp)) return take(r, K_KMAJOR);  // GenericParams, no workspace
    // A8W8 (int8 / fp8), round 5: 128 x 128 tiles with K unsplit where THEY number about one per CU (FP8 x FP8 16384^2 at M = 256: 256 tiles) —
    // tuning[0] = 10 forces them, tuning[0] = 6 keeps the round-3 choice
    if ((a.tuning[0] == 10 || (tuning_default(a) && !(caller_flags(a) & GEMLITE_TF_A8W8_WEIGHTS_FROM_MEMORY) && a8w8_sq128_pays(a))) &&
        plan_gemm_a8w8_sq128(a, r.gp, r.lp)) return take(r, K_A8_MMA);
    // A8W8 (int8 / fp8), round 4: 64 x 64 tiles with K unsplit where they fill the chip about once (config 4 at M = 256: 256 tiles) —
    // tuning[0] = 5 forces them, tuning[0] = 6 keeps the round-3 choice
    if ((a.tuning[0] == 5 || (tuning_default(a) && !(caller_flags(a) & GEMLITE_TF_A8W8_WEIGHTS_FROM_MEMORY) && a8w8_sq_pays(a))) &&
        plan_gemm_a8w8_sq(a, r.gp, r.lp)) return take(r, K_A8_MMA);
    // A8W8 (int8 / fp8) from 2 rows: the 8-wave MFMA kernel.  tuning[0]: 1 = streaming kernel (one wave per column),
    // 2 = the 4-wave MFMA kernel of round 1 (M >= 32)
    if ((a.tuning[0] == 0 || a.tuning[0] == 6) && plan_gemm_a8w8_mma(a, r.gp, r.lp)) return take(r, K_A8_MMA);
    if (a.tuning[0] != 1 && plan_gemm_a8w8(a, r.lp)) return take(r, K_KMAJOR);  // same launch path: GenericParams, no workspace
    return false;
}

// family: A16W8: 8-bit unpacked weights under 16-bit activations, no metadata or one pre-scale per channel
static bool resolve_a16w8(const gemlite_hip_forward_args& a, int eff_group, Resolved& r) {
    if (!((a.W_group_mode == 0 || (a.W_group_mode == 2 && eff_group >= a.K && a.scales)) && a.stride_wk == 1 &&
          a.stride_xk == 1 && (a.input_dtype == GEMLITE_DT_FP16 || a.input_dtype == GEMLITE_DT_BF16) &&
          (a.w_dtype == GEMLITE_DT_INT8 || a.w_dtype == GEMLITE_DT_FP8E4 || a.w_dtype == GEMLITE_DT_FP8E5) &&
          a.K % 16 == 0 && a.stride_wn % 16 == 0 && (a.stride_xm * 2) % 16 == 0 && (((uintptr_t)a.w_q | (uintptr_t)a.x) % 16 == 0))) return false;
    r.kind = K_KMAJOR;
    // round 4, one row: a wave per column, the weight row in flight before x is staged (tuning[0] = 4 keeps the rows kernel)
    if (a.M == 1 && a.tuning[0] == 0 && a.K % 1024 == 0 && a.K <= 30720 && a.N % 16 == 0)
        return take_kernel(r, K_KMAJOR, a16w8_decode_kernel_fn(a.input_dtype, a.w_dtype), "a16w8_decode_kernel<tile16,16w>", dim3((unsigned)(a.N / 16), 1, 1),
                           dim3(1024, 1, 1), (size_t)a.K * 2);
    // round 4, more than 64 rows: the 8-wave MFMA tile kernel with the K-contiguous 8-bit geometry (x through LDS, weights converted
    // in registers); the per-channel pre-scale becomes the epilogue's channel scale.  tuning[0] = 4 keeps the rows kernel.
    // (rows vs tile, profiles/r04/probe_rows_vs_tiles*.log: the crossover sits at M N K ~ 850 M — 4096^2: M = 52, 8192^2: 13 (M = 64 there:
    //  67.6 vs 29.1 us), 14336 x 4096: 12, 4096 x 14336: 19)
    //  round 6: the rows kernel with x through LDS first where IT is the faster one — a16w8_rows_lds_pays(), gemm_a8w8.hip)
    if (a.tuning[0] == 0 && a16w8_rows_lds_pays(a) && plan_a16w8_rows(a, r.lp)) return true;
    if ((a.tuning[0] == 2 || ((a.M > 64 || (a.M >= 2 && (int64_t)a.M * a.N * a.K > 850000000ll)) && a.tuning[0] == 0)) &&
        !(a.W_group_mode == 2 && a.channel_scale_mode != 0)) {
        WnParams p = kcontig_wn_params(a, a.x, a.stride_xm, make_epilogue(a), 32);
        if (a.W_group_mode == 2) { p.epi.c_mode = 1; p.epi.scales_w = a.scales; }
        if (plan_gemm_wn_mma_mx(a, p, r.lp, 2)) { r.kind = K_TILED_WN; r.wn = p; return true; }
    }
    // round 4: 16-column blocks, weights converted in registers, MFMA (tuning[0] = 7 keeps the streaming kernel of rounds 1-3)
    if (a.tuning[0] != 7 && plan_a16w8_rows(a, r.lp)) return true;
    const int mb = a.M == 1 ? 1 : 4;
    return take_kernel(r, K_KMAJOR, kmajor_w8a16_kernel_fn(mb), "kmajor_w8a16_kernel", dim3((unsigned)((a.N + 3) / 4), (unsigned)((a.M + mb - 1) / mb), 1), dim3(256, 1, 1));
}

// family: weights of the activations' own type, K-contiguous, no metadata
static bool resolve_same_type_kmajor(const gemlite_hip_forward_args& a, Resolved& r) {
    const int esz = dtype_size(a.w_dtype);
    if (!(a.W_group_mode == 0 && a.stride_wk == 1 && a.stride_xk == 1 && a.w_dtype == a.input_dtype &&
          esz > 0 && (a.K % (16 / esz) == 0) && ((a.stride_wn * esz) % 16 == 0) && ((a.stride_xm * esz) % 16 == 0) &&
          (((uintptr_t)a.w_q | (uintptr_t)a.x) % 16 == 0) &&
          !(a.M > 1 && (a.w_dtype == GEMLITE_DT_FP8E4 || a.w_dtype == GEMLITE_DT_FP8E5)))) return false;  // fp8 rows > 1: MFMA kernels / coverage
    const int mb = a.M == 1 ? 1 : 4;
    // round 4: the 8-bit decode kernel (one wave per column, the whole row in flight at once); tuning[0] = 7 keeps kmajor_matmul_kernel
    if (a.M == 1 && esz == 1 && a.tuning[0] != 7 && a.K % 1024 == 0 && a.N % 16 == 0 &&
        (a.w_dtype == GEMLITE_DT_INT8 || ((a.w_dtype == GEMLITE_DT_FP8E4 || a.w_dtype == GEMLITE_DT_FP8E5) && (a.N <= 4096 || a.tuning[0] == 8))))
        return take_kernel(r, K_KMAJOR, a8w8_decode_kernel_fn(a.w_dtype, false), "a8w8_decode_kernel<tile16,16w>", dim3((unsigned)(a.N / 16), 1, 1), dim3(1024, 1, 1));
    return take_kernel(r, K_KMAJOR, kmajor_kernel_fn(mb), "kmajor_matmul_kernel", dim3((unsigned)((a.N + 3) / 4), (unsigned)((a.M + mb - 1) / mb), 1), dim3(256, 1, 1));
}

// ---- coverage kernels ------------------------------------------------------------------------------------------------------------------
static void resolve_coverage(const gemlite_hip_forward_args& a, Resolved& r) {
    if (a.M > 65535) { r.status = GEMLITE_ERR_BAD_SHAPE; return; }
    take_kernel(r, K_GENERIC, generic_kernel_fn(), "generic_matmul_kernel", dim3((unsigned)((a.N + 255) / 256), (unsigned)a.M, 1), dim3(256, 1, 1));
}

void resolve(const gemlite_hip_forward_args& a, Resolved& r) {
    r.status = validate(&a);
    if (r.status != GEMLITE_OK) return;
    if (is_mx_input(a.input_dtype)) { resolve_mx(a, r); return; }
    if (resolve_fused_quant_mx_row(a, r)) return;
    if (resolve_fused_quant_packed_row(a, r)) return;
    const bool packed = a.elements_per_sample > 1;
    // metadata rows actually indexed by K: channel-wise / scalar metadata behaves like one K-long group
    const bool per_group_meta = a.W_group_mode >= 2 || ((a.W_group_mode == 1) && !a.zero_is_scalar &&
                                                        !(a.channel_scale_mode == 1 || a.channel_scale_mode == 3));
    const int eff_group = per_group_meta ? a.group_size : (int)a.K;
    if (packed && resolve_packed_words(a, per_group_meta, eff_group, r)) return;
    r.gp = coverage_params(a, per_group_meta, eff_group);
    if (!packed && (resolve_fused_quant_unpacked(a, r) || resolve_a8w8(a, r) || resolve_a16w8(a, eff_group, r) || resolve_same_type_kmajor(a, r))) return;
    resolve_coverage(a, r);
}

// The ONE place that decides whether the planned launch adds the caller's bias itself: the planner chose a kernel that has a biased form
// (gemv_w4_decode3_kernel, gemm_w{4,2}_rows_kernel: LaunchPlan::fn_bias) and still runs it, the bias has the output's 16-bit type and is
// 2-byte aligned (the kernels load single elements), and the launch is not a timeline probe (the biased decode form has no `counters`).
// Then the plan is rewritten to the biased form: kernel, label, bias pointer.  Nothing is dereferenced.
bool apply_bias(const gemlite_hip_forward_args& a, const gemlite_hip_forward_ext* e, Resolved& r) {
    if (!e || !e->bias || r.status != GEMLITE_OK) return false;
    LaunchPlan& lp = r.lp;
    if ((lp.arg_kind != 1 && lp.arg_kind != 2) || !lp.fn_bias || lp.fn != lp.bias_of) return false;
    if (e->bias_dtype != a.output_dtype || (a.output_dtype != GEMLITE_DT_FP16 && a.output_dtype != GEMLITE_DT_BF16)) return false;
    if (((uintptr_t)e->bias & 1u) != 0) return false;
    if (lp.arg_kind == 1 && (lp.d3.modes & 64u)) return false;
    lp.fn = lp.fn_bias;
    lp.name = bias_label(lp.name);
    lp.bias = (const uint16_t*)e->bias;
    return true;
}

}  // namespace gl
