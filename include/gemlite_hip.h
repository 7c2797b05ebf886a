/*
 * gemlite_hip.h — C ABI of libgemlite_hip.so (MI355X / gfx950 only).
 *
 * This is the drop-in boundary for the fused unpack + dequant + matmul hot path of
 * mobiusml/gemlite.  Each entry point replaces one seam of the reference (paths relative
 * to the reference tree):
 *
 *   gemlite_hip_forward            <- GEMLITE_TRITON_MAPPING[matmul_type].forward(...)
 *                                     gemlite/core.py:184-190; the identical 17-argument
 *                                     launchers gemv_kernels.py:553-638,
 *                                     gemv_revsplitK_kernels.py:391-462,
 *                                     gemv_splitK_kernels.py:423-476,
 *                                     gemm_splitK_kernels.py:595-652, gemm_kernels.py:549-601
 *   gemlite_hip_workspace_bytes    <- the reference has no workspace: it zero-fills the
 *                                     output and uses atomics (gemv_revsplitK_kernels.py:422,
 *                                     gemm_splitK_kernels.py:141); we use caller-owned scratch
 *   gemlite_hip_scale_activations_per_token
 *                                  <- scale_activations_per_token_triton,
 *                                     gemlite/quant_utils.py:268-347 (spec: :231-253)
 *   gemlite_hip_scale_activations_mxfp8 / _mxfp4 / _nvfp4
 *                                  <- scale_activations_mxfp8 / mxfp4 / nvfp4 (= the *_triton_v2 launchers),
 *                                     gemlite/quant_utils.py:546-590, 820-855, 917-954
 *   gemlite_hip_pack_over_cols     <- pack_weights_over_cols_triton, gemlite/bitpack.py:77-144
 *                                     (bit layout spec: pack_weights_over_cols_torch :36-60)
 *   gemlite_hip_unpack_over_cols   <- unpack_over_cols_triton, gemlite/bitpack.py:175-241
 *   gemlite_hip_quantize_groups    <- (no counterpart: the reference leaves float -> grouped INT to the third-party hqq package)
 *   gemlite_hip_quantize_groups_hqq <- (hqq's optimize_weights_proximal, restated per group: see the declaration)
 *   gemlite_hip_quantize_mx        <- gemlite/quant_utils.py  WeightQuantizerMXFP (torch ops there; one kernel here)
 *   gemlite_hip_dequantize         <- (no counterpart for a packed layer; WeightQuantizerMXFP.dequantize is torch ops on the quantiser's return)
 *   gemlite_hip_quantize_rows      <- gemlite/helper.py  A16W8.from_weights / A8W8_dynamic.from_weights (torch ops there; one kernel here)
 *
 * Conventions
 *   - plain pointers and sizes only; every pointer is a DEVICE pointer unless stated;
 *   - all launches are asynchronous on `stream` (a hipStream_t passed as void*); the library
 *     never allocates, frees or synchronises, so every call is hipGraph-capturable;
 *   - return value: 0 on success, a negative gemlite_status_t otherwise;
 *     gemlite_hip_status_string() maps it to text.  Nothing is launched on error;
 *   - dtype arguments are the integer codes of gemlite/dtypes.py:8-29 (gemlite_dtype_t);
 *   - strides are in ELEMENTS of the tensor's own dtype (what torch's .stride() returns);
 *   - strides are 64-bit: an operand whose addressed extent reaches what a kernel's 32-bit offsets cover (2 GiB or 4 GiB, by
 *     kernel) is routed to a kernel with 64-bit addresses (the planner's side of this is tested: tests/test_addressing_limits_cpu.py).
 */
#ifndef GEMLITE_HIP_H
#define GEMLITE_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define GEMLITE_HIP_ABI_VERSION 1

/* integer dtype codes — wire format shared with gemlite/dtypes.py:8-29 */
typedef enum gemlite_dtype_t {
    GEMLITE_DT_FP32 = 0,
    GEMLITE_DT_FP16 = 1,
    GEMLITE_DT_BF16 = 2,
    GEMLITE_DT_FP8E4 = 3, /* OCP e4m3fn: the gfx950 MFMA flavour */
    GEMLITE_DT_INT8 = 4,
    GEMLITE_DT_UINT8 = 5,
    GEMLITE_DT_INT32 = 6,
    GEMLITE_DT_UINT32 = 7,
    GEMLITE_DT_FP8E5 = 8, /* OCP e5m2 */
    GEMLITE_DT_INT16 = 9,
    GEMLITE_DT_UINT16 = 10,
    GEMLITE_DT_INT64 = 11,
    GEMLITE_DT_FP8E4NUZ = 12, /* MI300X flavour: rejected on gfx950 */
    GEMLITE_DT_FP8E5NUZ = 13,
    /* block-scaled ("microscaling") input formats, dtypes.py:24-29.  As input_dtype they name the FORMAT PAIR of a layer:
     * what x holds and how w_q / scales are laid out (see "Block-scaled formats" below) */
    GEMLITE_DT_MXFP16 = 14, /* x fp16,             w fp8 / fp4 + e8m0 scale per 32 k            */
    GEMLITE_DT_MXBF16 = 15, /* x bf16,             w fp8 / fp4 + e8m0 scale per 32 k            */
    GEMLITE_DT_MXFP8 = 16,  /* x fp8 e4m3,         w fp8 / fp4 + e8m0 scale per 32 k            */
    GEMLITE_DT_MXFP4 = 17,  /* x fp4 e2m1 (2/byte), w fp4 + e8m0 scale per 32 k                  */
    GEMLITE_DT_NVFP4 = 18,  /* x fp4 e2m1 (2/byte), w fp4 + e4m3 scale per 16 k, result * 0.05^2 */
    GEMLITE_DT_E8M0 = 19
} gemlite_dtype_t;

/* index into GEMLITE_MATMUL_TYPES (gemlite/core.py:56-66) */
typedef enum gemlite_matmul_type_t {
    GEMLITE_MATMUL_AUTO = -1, /* pick by M like get_matmul_type(), core.py:100-114 */
    GEMLITE_MATMUL_GEMV = 0,
    GEMLITE_MATMUL_GEMV_REVSPLITK = 1,
    GEMLITE_MATMUL_GEMV_SPLITK = 2,
    GEMLITE_MATMUL_GEMM_SPLITK = 3,
    GEMLITE_MATMUL_GEMM = 4
} gemlite_matmul_type_t;

typedef enum gemlite_status_t {
    GEMLITE_OK = 0,
    GEMLITE_ERR_BAD_ARGUMENT = -1, /* null pointer, non-positive size, bad struct_size  */
    GEMLITE_ERR_UNSUPPORTED = -2,  /* dtype / bit-width / mode combination not built     */
    GEMLITE_ERR_BAD_SHAPE = -3,    /* K not a multiple of elements_per_sample / group    */
    GEMLITE_ERR_WORKSPACE = -4,    /* workspace missing or smaller than required         */
    GEMLITE_ERR_LAUNCH = -5,       /* hipLaunchKernel failed; see gemlite_hip_last_hip_error */
    GEMLITE_ERR_NO_DEVICE = -6,    /* current device is not gfx950                       */
    GEMLITE_ERR_NO_FUSED_QUANT = -7 /* scales_x == NULL with 16-bit x asked for the in-launch activation quantisation, which this
                                    * shape / M has no kernel for: quantise x (gemlite_hip_scale_activations_per_token) and call
                                    * again with scales_x.  Not an error of the layer. */
} gemlite_status_t;

/* W_group_mode / channel_scale_mode follow gemlite/triton_kernels/utils.py:73-87 and
 * gemm_kernels.py:392-404:
 *   W_group_mode        0 none | 1 (q - z) | 2 q*s | 3 (q - z)*s | 4 fma(q, s, z')
 *   channel_scale_mode  0 none | 1 acc*s_w[n] | 2 acc*s_x[m] | 3 acc*s_x[m]*s_w[n]
 *                       4 block scales on the activations (MX / NV input formats only, gemm_kernels.py:508-509)
 *
 * Block-scaled formats (input_dtype GEMLITE_DT_MXFP16 .. GEMLITE_DT_NVFP4; gemm_MX_kernel, gemm_kernels.py:422-547;
 * layout produced by pack(), core.py:363-398, 489-497):
 *   w_q     W_nbits 8: fp8 e4m3 [K, N] view of an [N, K] tensor (elements_per_sample 1, w_dtype FP8E4);
 *           W_nbits 4: e2m1 codes, two per byte, k even in the low nibble: uint8 [K/2, N] (elements_per_sample 2,
 *           w_pack_bits 8).  Either way stride_wk / stride_wn are torch's strides of that tensor; the MFMA kernels take
 *           the K-contiguous layout pack() produces (stride_wk == 1), anything else runs on the coverage kernel
 *   scales  one byte per (32-k block, n): e8m0 (value 2^(b-127)); NVFP4: e4m3 per 16-k block; strides stride_meta_g
 *           (between blocks) / stride_meta_n;  W_group_mode is ignored, zeros unused
 *   x       MXFP16 / MXBF16: 16-bit floats, channel_scale_mode 0;  MXFP8: fp8 e4m3;  MXFP4 / NVFP4: uint8 [M, K/2]
 *   scales_x  channel_scale_mode 4: the block scales of x, uint8 [M_pad, K/32] (NVFP4: e4m3 [M_pad, K/16]), rows
 *           contiguous, row stride stride_sx_m, M_pad = M rounded up to 32 (16) — what
 *           gemlite_hip_scale_activations_mxfp8 / _mxfp4 / _nvfp4 write;  channel_scale_mode 2: fp32 [M] per token     */
typedef struct gemlite_hip_forward_args {
    uint32_t struct_size; /* = sizeof(gemlite_hip_forward_args), ABI guard */
    int32_t matmul_type;  /* gemlite_matmul_type_t */

    const void* x;        /* [M, K] activations, dtype input_dtype, row stride stride_xm   */
    const void* w_q;      /* packed: [K/e, N] words of w_pack_bits; unpacked: [K, N] view  */
    const void* scales;   /* [K/group, N] meta_dtype, or [N] channel scales, or NULL       */
    const void* zeros;    /* [K/group, N] meta_dtype, 1-elem int32 (scalar), or NULL       */
    const void* scales_x; /* [M] fp32 per-token activation scales, or NULL.  NULL together with
                           * channel_scale_mode 2/3, 16-bit float x and unpacked int8 / fp8 weights asks for
                           * the FUSED dynamic quantisation: x is quantised per token inside the matmul launch
                           * (same arithmetic as gemlite_hip_scale_activations_per_token, one launch instead of two).
                           * M == 1: always available.  2 <= M <= 64: producer blocks of the launch quantise the rows
                           * (needs the workspace: flags + M*K bytes + M floats; measured slower than two launches, the
                           * Python host does not use it by default); GEMLITE_ERR_NO_FUSED_QUANT where no such kernel
                           * applies (gemlite_hip_query() answers without launching).
                           * The same request exists at M == 1 for the layers whose activation format cannot be read off
                           * the weights — PACKED weights under fp8 / int8 activations (A8Wn dynamic, BitNet) and the
                           * block-scaled MXFP8 / MXFP4 layers (channel_scale_mode 4: block scales; 2: one scale per
                           * token): input_dtype names the type of the 16-bit x that is passed, the layer's activation
                           * format rides in type_id (= its DType code * 100 + W_nbits), scales_x is NULL. */
    void* out;            /* [M, N] output_dtype                                           */
    void* workspace;      /* >= gemlite_hip_workspace_bytes(); zero-filled ONCE by the owner */
    uint64_t workspace_bytes;

    int64_t M, N, K;

    int32_t W_nbits;             /* 1,2,4,8 packed; 8/16/32 unpacked                        */
    int32_t group_size;          /* K elements per scale/zero row (1 when there is none)    */
    int32_t unpack_mask;         /* 2^W_nbits - 1 (carried for signature parity; rederived) */
    int32_t elements_per_sample; /* e = w_pack_bits / W_nbits; 1 for unpacked weights       */
    int32_t w_pack_bits;         /* 8/16/32 for packed words; 0 when elements_per_sample==1 */
    int32_t w_dtype;             /* gemlite_dtype_t of w_q when unpacked (int8/fp8/fp16...) */

    int32_t input_dtype;  /* dtype of x as the kernel sees it (after activation quant)     */
    int32_t output_dtype;
    int32_t acc_dtype;    /* carried for parity; the HIP kernels accumulate fp32 / int32   */
    int32_t meta_dtype;   /* dtype of scales / tensor zeros                                */
    int32_t zeros_dtype;  /* meta_dtype for tensor zeros, GEMLITE_DT_INT32 for a scalar    */

    int32_t channel_scale_mode;
    int32_t W_group_mode;
    int32_t zero_is_scalar; /* zeros holds exactly one element (gemm_kernels.py:597)       */
    int32_t data_contiguous;
    int32_t type_id;        /* input_dtype*100 + W_nbits (core.py:141-145); tuning key only */

    int64_t stride_xm, stride_xk;
    int64_t stride_wk, stride_wn;       /* of w_q as given (packed rows or K)               */
    int64_t stride_om, stride_on;
    int64_t stride_meta_g, stride_meta_n;
    int64_t stride_sx_m;

    /* Planner overrides — the named values are the enums GEMLITE_T0_* / GEMLITE_T2_* / GEMLITE_TF_* below this struct (round 6, VERDICT r5 #9:
     * the numbers of rounds 1-5 stay valid, the names are what new callers should write).
     * (0 = library default everywhere; what helper.autotune_layer() searches and the tuning table
     * stores — the counterpart of the reference's per-shape Triton autotune configs).  Meaning per kernel family:
     *   packed GEMV (M = 1)        [0] 2/3/4 = 16-/32-/64-column tiles   [1] K slices   [2] 4/8/16 waves per block
     *                              (82 = 8 waves, 2 rows per lane; 48 = 4 waves, 8 rows per lane)   [3] & 3: 1 = x through LDS,
     *                              2 = x direct; & 16 = the round-2 kernel instead of the 16-column decode kernel,
     *                              & 32 = default-policy (not non-temporal) weight loads in the decode kernel (single-layer launches; a grouped launch under
     *                              capture always uses the default policy),
     *                              & 4096 = the round-3 decode kernel (struct arguments) instead of gemv_w4_decode3_kernel
     *   MFMA GEMV (M = 1..4, 4- and 2-bit words under 16-bit activations; default where it measured faster)
     *                              [0] 21/22/24 = 16-/32-/64-column tiles   [2] 4/8/16 waves per block
     *                              [3] & 512 = never, & 1024 = wherever it applies
     *   few rows (2..32, MFMA)     [0] 1/2/4 = 16-/32-/64-column tiles, 3 = the 8-wave tiled kernel instead
     *                              [1] K slices   [2] 1 = LDS-staged streaming kernel, 4 / 8 = waves per block of the registers-only
     *                              kernel (8: one row tile, >= 32-column tiles; default with two K slices)
     *   decode batch (2..64 rows, 4- and 2-bit words under 16-bit activations; round 5: gemm_w{4,2}_rows_kernel, 16-column blocks, K unsplit,
     *                              raw integer codes through the MFMA)   [0] 9 = at any M >= 2 the kernel takes (row blocks along
     *                              grid.y above 16 MT rows; [2] must be 0 or 8; [1] = 1 / 2 column tiles per block, 4-bit); default for 2..64 rows where N / 16 blocks are
     *                              resident in one round and the x re-reads stay <= 176 MiB, and ALWAYS for group size 32 and
     *                              N % 64 != 0 (no other MFMA kernel takes them)   [3] & 65536 = never (the round-4 choice, A/B runs)
     *   tiled (M > 32, MFMA)       [0] 1 = streaming kernel, 2 = the 4-wave tiled kernel of round 1 (4-bit only; the planner's
     *                              fallback for K = 64 * odd)
     *                              [1] K slices (any count <= K steps; slices may be uneven)
     *                              [2] tile rows / 32: 1/2/4/8 (8-wave kernel, 128-column tiles); 20 / 24 = 128 / 256 rows x 256
     *                              columns (4- and 2-bit, 16-bit activations); 32 .. 35 = the narrow 64-COLUMN tiles of round 4 (32 also
     *                              for 8-bit activations, block-scaled / NVFP4 / K-contiguous 8-bit weights)
     *                              (32: 64 x 64, 256-k steps — the default where they fill the chip without K slices, e.g.
     *                              4096^2 at M = 256; 33: 64 x 64, 512-k steps; 34 / 35: 128 x 64); with [0] = 2: 4 = one-step-ahead,
     *                              8 = 256 rows (both only in a library built with `make AB=1`)
     *                              [3] K-slice combine: & 128 = slabs + ticket always, & 2048 = reduce-scatter with 2 slices too
     *                              (default: from 4 slices), & 256 = reduce-scatter with immediate hand-over (test switch);
     *                              & 16384 = never the narrow tiles (the round-3 choice, A/B runs)
     *   unpacked 8-bit (A8W8)      [0] 1 = streaming (one wave per column), 2 = the 4-wave MFMA kernel of round 1 (the planner's
     *                              fallback for K % 256 != 0), 4 = the 16-column few-row kernel (default for 2..64 rows while
     *                              M K N / 16 <= 88 MiB and, from 128 column tiles of 64, M N K <= 800 M) at any M <= 64 and at M = 1, 5 = the unsplit 64 x 64 tiles of round 4
     *                              (default from 65 rows where they fill the chip once or twice, and from 2 rows past the few-row budget; [2] = 2/3/4 LDS stages),
     *                              6 = the round-3 kernels instead; M = 1: 7 = the round-2 streaming kernels instead of
     *                              a8w8_decode_kernel, 8 = a8w8_decode_kernel also for fp8 with N > 4096;
     *                              10 = the unsplit 128 x 128 tiles of round 5 (default above 64 rows where they number 192 .. 256 and
     *                              K >= 4096; [2] = 4 / 5 LDS stages of 128-byte K steps)
     *                              [1] K slices   [2] tile rows / 32 (forces the 8-wave kernels at any M)
     *                              [3] & 64: 128- / 256-row tiles with the weights straight from memory (default: through LDS)
     *                              [3] & 32768: test switch of the in-launch activation quantisation (no producer block runs)
     *   block-scaled (MX / NVFP4)  [0] 1 = coverage kernel, 2 = the 8-wave scaled-MFMA tile kernels at any M, 3 = the 256 x 256 tile
     *                              kernel at any M, 4 = the few-row kernel (default for 1..64 rows of fp8 / fp4 activations) past
     *                              its x re-read budget, 5 = the streaming kernel of rounds 2-3 (M <= 4), 6 = the unsplit 64 x 64
     *                              tiles of round 4 at any M (default for 65..384 rows, to 512 for fp4 x fp4 and one-round
     *                              shapes; [2] = 2/3/4 LDS stages)
     *                              [1] K slices   [2] tile rows / 32   (NVFP4: [0] = 1 coverage kernel, else the fp16 tile kernel)
     *   8-bit x packed (A8Wn, BitNet int8)   [0] 4 = the 16-column few-row kernel also at one row (default for 2..64 rows),
     *                              7 = the streaming GEMV of rounds 2-3 up to 4 rows
     *   unpacked 8-bit under 16-bit x (A16W8)   [0] 4 = the 16-column rows kernel at any M (default for 2..64 rows; above: the 8-wave
     *                              tile kernel, [1] K slices, [2] tile rows / 32), 7 = the streaming kernel of rounds 1-3
     *   tiled, round 6             [3] & 131072 = the packed words of the 64 x 64 / 128 x 128 4-bit tiles as register loads (the round-5 path; default:
     *                              through LDS-DMA, one request per wave and step); groups of 32 run on 32-row tiles with two metadata pairs per
     *                              sub-block ("<32x128,g32>": [1] K slices, [0] and [2] must be 0)
     *   [3] & 4: development timeline stamps (needs a workspace)   [3] & 8: XCD-aware (tile, K slice) map (opt-in).
     *   A value that does not apply to the shape makes the planner fall through to its own choice or to another family;
     *   it never produces a wrong result. */
    int32_t tuning[4];
} gemlite_hip_forward_args;

/* ---- names for the tuning[] values (per kernel family; the comment inside the struct has what each one selects) ------------------------- */
enum gemlite_hip_tuning0 {                 /* tuning[0]: which kernel of the family */
    GEMLITE_T0_AUTO = 0,
    /* packed words, one row (dot-product GEMV family): tile width */
    GEMLITE_T0_GEMV_TILE16 = 2, GEMLITE_T0_GEMV_TILE32 = 3, GEMLITE_T0_GEMV_TILE64 = 4,
    /* packed words, matrix-core GEMV (1 .. 4 rows): tile width */
    GEMLITE_T0_MFMA_GEMV_TILE16 = 21, GEMLITE_T0_MFMA_GEMV_TILE32 = 22, GEMLITE_T0_MFMA_GEMV_TILE64 = 24,
    /* packed words, 2 .. 32 rows (registers-only MFMA kernel): tile width; 3 = the 8-wave tile kernel instead */
    GEMLITE_T0_FEWROWS_TILE16 = 1, GEMLITE_T0_FEWROWS_TILE32 = 2, GEMLITE_T0_FEWROWS_TILE64 = 4, GEMLITE_T0_FEWROWS_USE_TILES = 3,
    /* packed 4- / 2-bit words, 2 .. 64 rows: the decode-shaped rows kernel at any M it takes */
    GEMLITE_T0_ROWS_KERNEL = 9,
    /* packed words, many rows: 1 = LDS-staged streaming kernel, 2 = the 4-wave tile kernel of round 1 */
    GEMLITE_T0_TILED_STREAM = 1, GEMLITE_T0_TILED_ROUND1 = 2,
    /* unpacked 8-bit (A8W8) */
    GEMLITE_T0_A8W8_STREAM = 1, GEMLITE_T0_A8W8_ROUND1 = 2, GEMLITE_T0_A8W8_ROWS = 4, GEMLITE_T0_A8W8_SQ64 = 5, GEMLITE_T0_A8W8_ROUND3 = 6,
    GEMLITE_T0_A8W8_M1_ROUND2 = 7, GEMLITE_T0_A8W8_M1_DECODE_FP8_WIDE = 8, GEMLITE_T0_A8W8_SQ128 = 10,
    /* block-scaled (MX / NVFP4) */
    GEMLITE_T0_MX_COVERAGE = 1, GEMLITE_T0_MX_TILES = 2, GEMLITE_T0_MX_TILES_256 = 3, GEMLITE_T0_MX_ROWS = 4, GEMLITE_T0_MX_STREAM = 5, GEMLITE_T0_MX_SQ64 = 6,
    /* 8-bit activations x packed words (A8Wn, BitNet int8); unpacked 8-bit weights under 16-bit activations (A16W8) */
    GEMLITE_T0_A8WN_ROWS = 4, GEMLITE_T0_A8WN_GEMV = 7, GEMLITE_T0_A16W8_ROWS = 4, GEMLITE_T0_A16W8_STREAM = 7
};
enum gemlite_hip_tuning2 {                 /* tuning[2]: tile geometry of the 8-wave tile kernel (other families: waves per block, see the struct) */
    GEMLITE_T2_AUTO = 0,
    GEMLITE_T2_ROWS32 = 1, GEMLITE_T2_ROWS64 = 2, GEMLITE_T2_ROWS128 = 4, GEMLITE_T2_ROWS256 = 8,        /* x 128 columns */
    GEMLITE_T2_WIDE_128x256 = 20, GEMLITE_T2_WIDE_256x256 = 24,                                              /* 256-column tiles */
    GEMLITE_T2_NARROW_64x64 = 32, GEMLITE_T2_NARROW_64x64_K512 = 33, GEMLITE_T2_NARROW_128x64 = 34, GEMLITE_T2_NARROW_128x64_RING6 = 35,
    GEMLITE_T2_GEMV_8WAVES_2ROWS = 82, GEMLITE_T2_GEMV_4WAVES_8ROWS = 48
};
enum gemlite_hip_tuning_flags {            /* tuning[3]: bit flags (A/B switches and test hooks; 0 = the shipped defaults) */
    GEMLITE_TF_GEMV_X_THROUGH_LDS = 1, GEMLITE_TF_GEMV_X_DIRECT = 2,
    GEMLITE_TF_GEMV_X_MODE_MASK = 3,             /* field: 0 = auto, else one of the two values above */
    /* the same two bits in other families: the wave count of the block-scaled decode kernel (a field, & 3: 1 = 4 waves, 2 = 16 waves,
     * 0 = auto) and s_setprio around the MFMAs of the round-1 4-wave tiled kernel (bit 0) */
    GEMLITE_TF_MX_GEMV_WAVES_MASK = 3, GEMLITE_TF_MX_GEMV_4_WAVES = 1, GEMLITE_TF_MX_GEMV_16_WAVES = 2,
    GEMLITE_TF_TILED_SETPRIO = 1,
    GEMLITE_TF_TIMELINE = 4,                     /* development stamps (needs a workspace) */
    GEMLITE_TF_XCD_SLICE_MAP = 8,                /* XCD-aware (tile, K slice) map of the tile kernel */
    GEMLITE_TF_GEMV_ROUND2_KERNEL = 16, GEMLITE_TF_GEMV_DEFAULT_POLICY_LOADS = 32,
    GEMLITE_TF_MX_PLAIN_TILE_ORDER = 16,         /* same bit: plain M-fastest tile order of the block-scaled 256 x 256 tiles */
    GEMLITE_TF_A8W8_WEIGHTS_FROM_MEMORY = 64,
    GEMLITE_TF_COMBINE_TICKET = 128, GEMLITE_TF_COMBINE_HANDOVER_TEST = 256,
    GEMLITE_TF_NO_MFMA_GEMV = 512, GEMLITE_TF_FORCE_MFMA_GEMV = 1024,
    GEMLITE_TF_COMBINE_REDUCE_SCATTER_2 = 2048,
    GEMLITE_TF_GEMV_ROUND3_DECODE = 4096,
    GEMLITE_TF_NO_NARROW_TILES = 16384,
    GEMLITE_TF_MX_NO_SLICE_RULE = 16384,         /* same bit: the block-scaled 128-row tiles keep the fill-the-chip K slice count */
    GEMLITE_TF_QUANT_NO_PRODUCER_TEST = 32768,
    GEMLITE_TF_NO_ROWS_KERNEL = 65536,           /* the round-4 choice for 2 .. 64 rows */
    GEMLITE_TF_WORDS_AS_REGISTER_LOADS = 131072, /* round 6: the round-5 weight path of the 64 x 64 / 128 x 128 4-bit tiles */
    GEMLITE_TF_ROUND5_TILE_EPILOGUE = 262144,    /* round 6: the two-barrier K-part join of the unsplit tiles instead of the direct one */
    GEMLITE_TF_W8_ROWS_X_FROM_REGISTERS = 524288, /* round 6: the round-3 / round-4 few-row kernels of unpacked 8-bit weights (a8w8_rows_kernel / a16w8_rows_kernel)
                                                    instead of w8_rows_lds_kernel (x through LDS in whole cache lines) */
    GEMLITE_TF_W8_ROWS_LDS_BELOW_4_ROWS = 1048576, /* A16W8: take w8_rows_lds_kernel at 1 .. 3 rows too (default: from 4) */
    GEMLITE_TF_A8W8_TILE_REQUESTS_FIRST = 2097152, /* round 6: the round-4 order of a K step of the 64 x 64 A8W8 tile (DMA requests in front of the LDS reads) */
    GEMLITE_TF_NO_K_ROTATION = 4194304,            /* round 6: every row tile of the unsplit tiles of 8-bit weights walks K in the plain order */
    GEMLITE_TF_K_ORDER_GROUP_MASK = 0x0F000000,    /* round 6: bits 24 .. 27 = 1 + log2(steps per group) of the grouped K order between the row tiles of a column tile (0 = the planner's choice) */
    GEMLITE_TF_PUBLIC_MASK = 0x0FFFDFFF            /* every bit named above (0 .. 12, 14 .. 27).  The library ignores the others: bits 28 .. 31 are its own */
};

/* Library / ABI identification (host only, no device access). */
int gemlite_hip_abi_version(void);
const char* gemlite_hip_build_info(void);
const char* gemlite_hip_status_string(int status);
/* hipError_t of the last failed HIP runtime call made by this library on this thread. */
int gemlite_hip_last_hip_error(void);

/* 0 if the configuration has a native kernel, GEMLITE_ERR_* otherwise. Never launches. */
int gemlite_hip_query(const gemlite_hip_forward_args* args);

/* Scratch bytes gemlite_hip_forward needs for this configuration (split-K slabs + arrival
 * counters).  The caller allocates it once, zero-fills it once, and then only passes it in:
 * every launch leaves the counters at zero again.  One workspace per concurrently used stream. */
uint64_t gemlite_hip_workspace_bytes(const gemlite_hip_forward_args* args);

/* out[M,N] = epilogue( x[M,K] @ dequant(w_q, scales, zeros) ) — one fused launch. */
int gemlite_hip_forward(const gemlite_hip_forward_args* args, void* stream);

/* Name of the kernel gemlite_hip_forward would launch for `args` (for profiles/tests). */
const char* gemlite_hip_kernel_name(const gemlite_hip_forward_args* args);

/* Optional: the NEXT gemlite_hip_forward on this thread is launched with
 * hipExtLaunchKernel(start, stop) so that hipEventElapsedTime(start, stop) is that kernel's
 * own device duration.  Pass NULL, NULL to clear.  Events are hipEvent_t passed as void*. */
void gemlite_hip_set_profile_events(void* start_event, void* stop_event);

/* Measurement aid: launches an EMPTY kernel of `blocks` x `threads` on `stream` (honours
 * gemlite_hip_set_profile_events).  bench.py uses it to report the floor of the per-launch event clock next
 * to every kernel duration it quotes (on MI355X an empty kernel already reads ~4 us). */
int gemlite_hip_launch_noop(int32_t blocks, int32_t threads, void* stream);

/* Capture-time grouping of the M = 1 decode kernel and of the few-row (2 .. 64 rows) 4- / 2-bit rows kernel.  While `stream` is being captured into a graph, a gemlite_hip_forward call that runs
 * gemv_w4_decode3_kernel and is INDEPENDENT of the decode launches captured directly before it (nothing else captured on the stream in
 * between; same kernel, shape, strides and modes; its output overlaps none of their inputs or outputs, their outputs none of its inputs)
 * adds no node: the node before it becomes one grouped launch of up to gemlite_hip_capture_group_max layers.  Every layer's result is
 * bit-identical to its own launch, the graph stays linear, and a dependent chain is captured node for node as before.  Eager launches,
 * launches with profile events and GEMLITE_TF_TIMELINE launches never group.  The environment variable GEMLITE_HIP_NO_CAPTURE_GROUPS=1
 * (read once per process) turns grouping off.
 * The SECOND family: a call that runs gemm_w4_rows_kernel / gemm_w2_rows_kernel (2 .. 64 rows in one row block) joins the rows launches
 * captured directly before it under the same rule — same kernel form, tiles, strides, modes and M, the same independence — and the node
 * becomes gemm_w4_rows_group_kernel, grid (tiles, members): block (tile, y) computes member y's tile as its own launch would, bit for
 * bit.  The families never mix: a launch of one family behind an open group of the other closes it and opens its own.  Launches with
 * row blocks (grid.y > 1) never group.  GEMLITE_HIP_CAPTURE_GROUP_ROWS=0 (read once per process) keeps only this family ungrouped.
 *   _max         layers per grouped launch (1 = grouping is off)
 *   _stats       process-wide counts: decode and rows launches seen under capture, and how many of them joined a node instead of adding one
 *   _compatible  host only, nothing is dereferenced: 1 if launch `b` captured directly behind launch `a` would join it, else 0
 *   _grid_y      host only: the grid.y rule for a grouped launch of `members` layers of `tiles` 16-column tiles (N / 16), answered for
 *                a full 256-CU part: clamp(256 / tiles, 1, members) (a launch uses its own device's CU count in place of 256); block (tile, y) holds the layers y, y + grid.y, ...  0 for a non-positive argument
 *   _wave_split  host only: how the 16 waves of a grouped block share its `layers_in_block` layers (1 .. 16), which are all in flight at
 *                once: out = {block-local layer of `wave` (-1: the wave has no work), v0, v1} — the wave does what the single-layer
 *                kernel's waves v0 .. v1 - 1 do for that layer (wave v there: the 32-row chunks v, v + 16, ... of K / 8 packed rows).
 *                16 / layers_in_block waves per layer.  {-1, 0, 0} for an argument out of range
 *   _last_form   host only: the form of the grouped node the calling thread rewrote last: 0 none (no join since the thread's last group
 *                opened), 1 per-wave x (every wave loads the x of its own layer), 2 shared x (three or more members that all read the same x pointer: a
 *                block stages x in LDS once; GEMLITE_HIP_CAPTURE_GROUP_SHARED_X=0, read once, keeps every group on form 1), 3 a group of
 *                the rows kernel (grid (tiles, members))
 *   _form, _shared_x_lds_bytes   DEVELOPMENT / TEST exports (tests/test_decode_group_shared_x_cpu.py restates them in Python); not part of
 *                what a caller needs, and free to change with the kernel:
 *   _form        host only: the rule behind it for `members` layers (1 .. 16) of reduction length K (a multiple of 256) whose x pointers
 *                all agree (same_x != 0) or not: 0 / 1 / 2 as above, -1 for an argument out of range
 *   _shared_x_lds_bytes  host only: dynamic LDS of a shared-x block, 64 KiB of partial rows + 2.25 K bytes of staged x; 0 when that is
 *                past the 160 KiB of a CU (K > 43520: such a K keeps form 1) or K is no positive multiple of 256
 *   _geometry    host only, DEVELOPMENT / TEST: the tile-group geometry of a grouped launch of `members` layers of `tiles` tiles on a
 *                device with `resident` CUs: out = {TB, grid.x, grid.y, placement}.  A block holds TB (1, 2 or 4) adjacent tiles x
 *                ceil((members - y) / grid.y) layers, grid.x = tiles / TB, grid.y = the _grid_y rule for tiles / TB tile groups; its
 *                (layer, tile) slots — slot s = layer s / TB, tile s % TB, at most 16 — are what _wave_split calls layers.  TB is the
 *                largest one <= tb_want (1, 2, 4) with tiles % TB == 0 and ceil(members / grid.y) * TB <= 16; placement 0 interleaved,
 *                1 span (span_want).  tb_want = 0: what a capture picks (GEMLITE_HIP_CAPTURE_GROUP_TILES=<TB>[s|i], read once, or the
 *                default rule).  Returns 0, or -1 for an argument out of range
 *   _tile_of     host only, DEVELOPMENT / TEST: the first tile of the tile group that block `block` (0 .. tiles / tb - 1) of a grouped
 *                launch works on, a permutation of the groups under either placement (span = 0 / 1); -1 for an argument out of range
 *   _lines       host only, DEVELOPMENT / TEST: the tiles per wave H (1, 2 or 4) that a grouped launch of `members` layers of `tiles`
 *                tiles with `tb` tiles per block carries: a wave's lanes are H sub-waves on H adjacent tiles and take H passes over each
 *                virtual wave, so one request instruction asks for whole 128-byte (H = 2) or 256-byte (H = 4) runs of a weight row; the
 *                block's slots / H wave-slots are what _wave_split calls layers.  H divides TB: h_want = 4 falls back to 2, then 1.
 *                h_want = 0: what a capture picks (GEMLITE_HIP_CAPTURE_GROUP_LINES=1|2|4, read once, or the default rule).  -1 for an
 *                argument out of range
 *   _last_lines  host only: the H of the grouped decode node the calling thread rewrote last (0: none)
 *   _policy      host only, DEVELOPMENT / TEST: does a grouped decode launch of H = `h` (1, 2, 4) tiles per wave ask for its weights
 *                non-temporally?  1 only when h >= 2, the members' own launches are non-temporal (default_policy_loads = 0: the layers'
 *                tuning[3] carries no GEMLITE_TF_GEMV_DEFAULT_POLICY_LOADS) and every member's weight base (w_bases_or: the bases OR-ed
 *                together) and the row pitch in bytes are multiples of 128: one request then covers whole lines that nobody asks for again.
 *                forced = 0 / 1 overrides the last two conditions (never h >= 2), -1 is the rule alone, -2 what a capture picks
 *                (GEMLITE_HIP_CAPTURE_GROUP_NT=0|1, read once, or the rule).  0 / 1, or -1 for an argument out of range.
 *                Weights that stay in the 256 MiB Infinity Cache from step to step are read 3 - 6 % faster with the default
 *                policy (the crossover lies between 286 and 572 MB of weights per step): set GEMLITE_TF_GEMV_DEFAULT_POLICY_LOADS in
 *                such a model's tuning[3]
 *   _last_policy host only: the weight-load policy of the grouped decode node the calling thread rewrote last: 0 default, 1
 *                non-temporal, -1 none
 * ROUNDS.  When a grouped DECODE node fills up (_max members) directly behind another full one of the same capture, with nothing else on
 * either node, and every member of the one is independent of every member of the other, the two become ONE node of two rounds: grid
 * (grid.x, grid.y x rounds), a CU takes its block of the next round when its own block leaves, no launch boundary in between; up to
 * _rounds_max rounds (at most 64 members per node).  A partial trailing group keeps its own node.  _stats counts as before.
 * GEMLITE_HIP_CAPTURE_GROUP_ROUNDS=1..4 (development, read once per process) sets the round limit, 1 = no merging.  Rows groups do not merge.
 *   _merge_stats   process-wide count of groups merged into the node in front of them
 *   _rounds_max    rounds a decode node may hold (1 = merging is off)
 *   _last_rounds   host only: rounds of the grouped decode node the calling thread rewrote or merged last (0: none)
 *   _round_member  host only, DEVELOPMENT / TEST: the index rule of the kernel.  In a node of `m` members per round (1 .. 16) and `Y`
 *                  block rows per round (1 .. m), the member of the node's table that block row `block_y` holds as its block-local layer
 *                  `local_layer`: m x (block_y / Y) + block_y % Y + local_layer x Y.  -1 for an argument out of range (a round past
 *                  64 members, a layer the block does not hold) */
int gemlite_hip_capture_group_max(void);
void gemlite_hip_capture_group_stats(uint64_t* seen, uint64_t* joined);
int gemlite_hip_capture_group_compatible(const gemlite_hip_forward_args* a, const gemlite_hip_forward_args* b);
int gemlite_hip_capture_group_grid_y(int32_t tiles, int32_t members);
void gemlite_hip_capture_group_wave_split(int32_t layers_in_block, int32_t wave, int32_t out[3]);
int gemlite_hip_capture_group_last_form(void);
int gemlite_hip_capture_group_form(int32_t members, int32_t same_x, int64_t K);
int64_t gemlite_hip_capture_group_shared_x_lds_bytes(int64_t K);
int gemlite_hip_capture_group_geometry(int32_t tiles, int32_t members, int32_t resident, int32_t tb_want, int32_t span_want, int32_t out[4]);
int gemlite_hip_capture_group_tile_of(int32_t tiles, int32_t tb, int32_t span, int32_t block);
int gemlite_hip_capture_group_lines(int32_t tiles, int32_t members, int32_t resident, int32_t tb, int32_t h_want);
int gemlite_hip_capture_group_last_lines(void);
int gemlite_hip_capture_group_policy(int32_t h, int32_t default_policy_loads, uint64_t w_bases_or, uint32_t pitch_bytes, int32_t forced);
int gemlite_hip_capture_group_last_policy(void);
void gemlite_hip_capture_group_merge_stats(uint64_t* merged);
int gemlite_hip_capture_group_rounds_max(void);
int gemlite_hip_capture_group_last_rounds(void);
int gemlite_hip_capture_group_round_member(int32_t m, int32_t Y, int32_t block_y, int32_t local_layer);

/* K order of the unsplit 8-bit tiles (host only, DEVELOPMENT / TEST: nothing is launched, no device is touched).  The row tiles of a weight
 * column tile of gemm_a8w8_sq_kernel<64x64> / <128x128> and gemm_mx_*_sq_kernel<64x64> may walk their K steps in different orders (an L2
 * matter; every order visits every step once).  `mode`: -1 = plain order, 0 = whole-K rotation (row tile mt starts at step
 * mt nsteps / mtiles), 1 .. 15 = the group field of GEMLITE_TF_K_ORDER_GROUP_MASK (groups of 2^(mode - 1) steps, rotated by mt inside every
 * full run of mtiles groups; a tail of fewer than mtiles groups, a partial last group and a group larger than nsteps are plain).
 *   _step   the step of K that row tile `mt` of `mtiles` takes as its `step`-th of `nsteps`: evaluates the struct the kernels compile.
 *           -1 for an argument out of range (step outside [0, nsteps), mt outside [0, mtiles), mode outside [-1, 15])
 *   _mode   the mode the kernel planned for `args` is launched with; -1 when that kernel has no K order or walks K plain (one row tile,
 *           GEMLITE_TF_NO_K_ROTATION, a split K, any other kernel, a request without a kernel).  The narrow 64 x 64 tiles of the weight-only
 *           8-bit layers (gemm_a16w8_kernel<64x64>, gemm_a16w8_mxfp_kernel<64x64>) have the whole rotation only: they IGNORE the group
 *           field, so 0 or -1 is reported for them whatever GEMLITE_TF_K_ORDER_GROUP_MASK holds.
 * A forced group (GEMLITE_TF_K_ORDER_GROUP_MASK != 0) turns the order on for the three sq kernels wherever they have two or more row tiles —
 * also where the column tiles are NOT a multiple of 8 and the kernel maps its blocks plainly (row tiles fastest) instead of keeping a column
 * tile's row tiles on one XCD: the order is then of no use to the L2, and the result is the same as ever. */
int gemlite_hip_k_order_step(int32_t step, int32_t mt, int32_t mtiles, int32_t nsteps, int32_t mode);
int gemlite_hip_k_order_mode(const gemlite_hip_forward_args* args);

/* Bias in the launch (optional extension; gemlite_hip_forward_args and every entry point above are unchanged).  The M = 1 decode kernel
 * (gemv_w4_decode3_kernel, single and grouped) and the few-row kernels (gemm_w4_rows_kernel / gemm_w2_rows_kernel) have forms that add a
 * bias[N] in their epilogue:   out[m, n] = round16( float(round16(acc[m, n])) + float(bias[n]) )   — both roundings of "matmul, then
 * out += bias", so the result is bit-identical to the two launches.  The bias is fused when it is a contiguous [N] vector of the OUTPUT's
 * dtype (fp16 / bf16), at least 2-byte aligned, and the planner chose one of those kernels for `args` (not a GEMLITE_TF_TIMELINE launch).
 *   gemlite_hip_forward_ex    with ext == NULL or ext->bias == NULL exactly gemlite_hip_forward.  Otherwise it NEVER fails because of
 *                             the bias: it returns GEMLITE_OK when the launch added it, and GEMLITE_BIAS_NOT_ADDED (a positive status)
 *                             when the launch ran WITHOUT it and the caller has to add it (out += bias); negative statuses as ever.
 *   gemlite_hip_bias_fused    host only, launches and dereferences nothing: 1 = the launch planned for (args, ext) adds the bias itself,
 *                             0 = the caller must add it (also for ext == NULL / no bias), negative = bad arguments / no kernel
 *   gemlite_hip_kernel_name_ex   the kernel of (args, ext); a biased form carries ",bias" before the closing '>' of its label
 *   gemlite_hip_capture_group_compatible_ex   the capture-group rule for two (args, ext) pairs: a fused bias is one more READ span of
 *                             its launch (an output that overlaps another member's bias does not join, in either order), and a biased
 *                             and an unbiased launch never share a group.  gemlite_hip_capture_group_compatible(a, b) = both ext NULL. */
typedef struct gemlite_hip_forward_ext {
    uint32_t struct_size; /* sizeof(gemlite_hip_forward_ext), ABI guard */
    int32_t bias_dtype;   /* gemlite_hip_dtype code of bias                */
    const void* bias;     /* [N] contiguous, device memory, or NULL        */
} gemlite_hip_forward_ext;
#define GEMLITE_BIAS_NOT_ADDED 1
int gemlite_hip_forward_ex(const gemlite_hip_forward_args* args, const gemlite_hip_forward_ext* ext, void* stream);
int gemlite_hip_bias_fused(const gemlite_hip_forward_args* args, const gemlite_hip_forward_ext* ext);
const char* gemlite_hip_kernel_name_ex(const gemlite_hip_forward_args* args, const gemlite_hip_forward_ext* ext);
int gemlite_hip_capture_group_compatible_ex(const gemlite_hip_forward_args* a, const gemlite_hip_forward_ext* ea,
                                             const gemlite_hip_forward_args* b, const gemlite_hip_forward_ext* eb);

/* Experts of a mixture-of-experts layer: ONE launch of n_slots M = 1 GEMVs whose expert ids are read ON THE GPU, so the call can be
 * captured in a graph once and replayed with other ids.  The E experts are identical layers stacked at fixed byte strides; slot s
 *   reads x row s / slots_per_x_row (layer.x + row * stride_x_row elements), uses expert e = ids[s] (weights layer.w_q + e * stride_expert_w
 *   bytes, scales / zero tensor + e * stride_expert_meta, bias + e * stride_expert_bias; a scalar zero is shared by all experts), and
 *   writes its N outputs at layer.out + s * stride_out_slot elements — bit-identical to the M = 1 decode launch (gemv_w4_decode3_kernel)
 *   of expert e on that row, with the bias added as gemlite_hip_forward_ex adds it.
 * An id outside [0, n_experts) — negative, too large, an int64 with a high dword — is never dereferenced: that slot's N outputs are
 * zeros (no bias) and nothing else is touched (expert-parallel serving marks "not on this rank" with -1).
 * Domain: W_nbits 4 in 32-bit words; fp16 / bf16 with input = output = scale (= zero tensor) dtype, a scalar zero as INT32;
 * channel_scale_mode 0; W_group_mode 1..4; group_size a power of two >= 32 that divides K; M = 1; N % 16 == 0; K % 256 == 0; unit inner
 * strides; 16-byte aligned w_q and x rows, 8-byte aligned metadata, expert strides in multiples of 16 / 8 / 2 bytes (weights / metadata /
 * bias); 1 <= n_slots <= 65535; inside one expert the 2^32 / 2^31 byte-offset limits of the decode kernel (expert strides are 64-bit).
 * Everything is validated before the launch: GEMLITE_ERR_BAD_ARGUMENT (null pointers, struct_size, non-positive counts, misaligned
 * or negative strides), GEMLITE_ERR_UNSUPPORTED (dtypes, bit width, modes, ids dtype, inner strides), GEMLITE_ERR_BAD_SHAPE (M, N, K, group
 * size, slot count, offset limits).  layer.matmul_type / tuning / workspace are not read.
 *   gemlite_hip_experts_query   validates and never launches or dereferences; works without a GPU */
typedef struct gemlite_hip_experts_args {
    uint32_t struct_size;           /* sizeof(gemlite_hip_experts_args), ABI guard */
    int32_t ids_dtype;              /* GEMLITE_DT_INT32 | GEMLITE_DT_INT64 */
    gemlite_hip_forward_args layer; /* expert 0: w_q / scales / zeros / shapes / strides / modes; x = row 0, out = slot 0; M must be 1 */
    const void* ids;                /* device, n_slots entries */
    const void* bias;               /* expert 0's bias[N] of the output type, or NULL */
    int64_t n_slots, n_experts, slots_per_x_row;
    int64_t stride_expert_w, stride_expert_meta, stride_expert_bias; /* bytes between experts */
    int64_t stride_x_row, stride_out_slot;                           /* elements */
    int64_t reserved[2];
} gemlite_hip_experts_args;
int gemlite_hip_forward_experts(const gemlite_hip_experts_args* args, void* stream);
int gemlite_hip_experts_query(const gemlite_hip_experts_args* args);

/* The same launch with the rest of an expert MLP fused into its epilogue: an expert MLP is two launches, gate/up (GLU) and down (COMBINE).
 * `experts` is a complete gemlite_hip_forward_experts request (its own struct_size set) and is validated by the same rules first; every
 * member (slot, 16-column tile) is computed and rounded exactly as gemlite_hip_forward_experts computes it, bias included.
 *   GEMLITE_EXPERTS_GLU      the N columns of an expert are [gate; up] halves of I = N / 2 columns (the w13 layout of HF / vLLM
 *                            checkpoints).  With g, u the rounded gate / up outputs of slot s, its I outputs at experts.layer.out +
 *                            s * stride_out_slot are round(silu(g) * u), silu(v) = v / (1 + exp(-v)) in fp32, one rounding; for v < -88, where
 *                            exp(-v) leaves fp32, silu(v) = v exp(v / 2) exp(v / 2), so the result stays within one ulp of the output
 *                            type down to its smallest subnormal.  g = +Inf gives sign(u) Inf (NaN for u = 0), g = -Inf gives NaN
 *                            (-Inf / (1 + Inf); torch's silu gives the same).  A slot whose id is outside [0, n_experts) gets I zeros.
 *   GEMLITE_EXPERTS_COMBINE  token t = the slots t * slots_per_token + k, k < slots_per_token, each with its own id, x row
 *                            (slot / slots_per_x_row) and bias row.  With y_k the rounded output of slot k its N outputs at experts.layer.out
 *                            + t * stride_out_slot are round(sum_k weights[slot_k] * y_k): fp32, ascending k from 0, one rounding.  A slot
 *                            with an invalid id is never dereferenced and contributes exactly 0; a token without a valid id gets N zeros.
 * Refusals beyond those of the nested request: GEMLITE_ERR_BAD_ARGUMENT (null struct, struct_size, COMBINE: null or misaligned weights,
 * slots_per_token <= 0), GEMLITE_ERR_UNSUPPORTED (epilogue, activation, weights_dtype), GEMLITE_ERR_BAD_SHAPE (GLU: N % 32 != 0; COMBINE:
 * slots_per_token > 16 or not a divisor of n_slots).  Fields of the other epilogue are not read.
 *   gemlite_hip_experts_fused_query   validates and never launches or dereferences; works without a GPU */
#define GEMLITE_EXPERTS_GLU 1
#define GEMLITE_EXPERTS_COMBINE 2
#define GEMLITE_ACT_SILU 1
typedef struct gemlite_hip_experts_fused_args {
    uint32_t struct_size;             /* sizeof(gemlite_hip_experts_fused_args), ABI guard */
    int32_t epilogue;                 /* GEMLITE_EXPERTS_GLU | GEMLITE_EXPERTS_COMBINE */
    gemlite_hip_experts_args experts; /* exactly as for gemlite_hip_forward_experts */
    int32_t activation;               /* GLU: GEMLITE_ACT_SILU */
    int32_t weights_dtype;            /* COMBINE: GEMLITE_DT_FP32 or the output dtype */
    const void* weights;              /* COMBINE: device, n_slots entries in the order of ids */
    int64_t slots_per_token;          /* COMBINE: 1..16, divides n_slots */
    int64_t reserved[3];
} gemlite_hip_experts_fused_args;
int gemlite_hip_forward_experts_fused(const gemlite_hip_experts_fused_args* args, void* stream);
int gemlite_hip_experts_fused_query(const gemlite_hip_experts_fused_args* args);

/* Experts for BATCHES (more than one token): the slots are sorted by expert ON THE GPU and every expert's weights stream once per work
 * block of up to R = rows_per_block slots through the matrix core (gemm_w4_rows_experts_kernel, gemm_wn_rows_experts.hip: the body of
 * gemm_w4_rows_kernel with gathered x rows and scattered output rows).  Two launches, no host synchronisation, both graph-capturable:
 *   gemlite_hip_experts_route         reads experts.ids (experts.n_slots entries of experts.ids_dtype) and writes the work table into
 *                                     `workspace`; it reads experts.ids / ids_dtype / n_slots / n_experts and nothing else of `experts`'
 *                                     pointers, and validates the whole request as gemlite_hip_forward_experts_rows does.
 *   gemlite_hip_forward_experts_rows  consumes a routed workspace: grid (N / 16, Bmax), block (tile, b) computes the 16 columns of tile for
 *                                     the slots of work block b.  Slot s reads x row s / slots_per_x_row and writes layer.out +
 *                                     s * stride_out_slot, as in gemlite_hip_forward_experts.
 * Work table (int32): [0] the number of work blocks used, [1..3] zero, then block_expert[Bmax], then block_rows[Bmax * R] — the slot
 * indices of each work block, padded with -1.  A work block holds at most R slots of ONE expert; an expert with c slots has ceil(c / R)
 * blocks; ids outside [0, n_experts) (the test of gemlite_hip_forward_experts) form bucket n_experts, whose slots get N zeros.
 * Bmax = ceil(n_slots / R) + min(n_experts + 1, n_slots); entries beyond the used count are unspecified and never read.  The order of
 * the slots inside an expert's blocks is unspecified: no output depends on it.
 * Numerics: every valid slot is bit-identical to gemm_w4_rows_kernel (tuning[0] = 9) of that expert with R / 16 row tiles on a matrix that
 * holds the slot's x row, bias added as gemlite_hip_forward_ex adds it.  (The decode launches above sum K in another order.)
 * rows_per_block: 0 = the library's default (the smallest of 16 / 32 / 48 / 64 that holds the mean slots per expert, m = n_slots /
 * min(n_experts, n_slots), plus a quarter: m + m / 4 in integers), else 16 / 32 / 48 / 64; groups of 32 allow 16 / 32 only (registers).
 * Domain: that of gemlite_hip_forward_experts, then the rows kernel's: 16-byte aligned x rows (stride_x_row % 8), 4-byte aligned out and
 * an even stride_out_slot, n_experts <= GEMLITE_EXPERTS_ROWS_MAX_EXPERTS, n_slots <= 65535, the extent of x — (ceil(n_slots /
 * slots_per_x_row) - 1) * stride_x_row * 2 + K * 2 bytes — below 2^31.  The workspace is non-null, 4-byte aligned and at least
 * gemlite_hip_experts_rows_workspace_bytes long (GEMLITE_ERR_WORKSPACE otherwise).
 *   gemlite_hip_experts_rows_workspace_bytes  bytes of the work table for (n_slots, n_experts, R = 16 / 32 / 48 / 64); 0 for arguments
 *                                             outside the domain
 *   gemlite_hip_experts_rows_per_block        the R the library resolves for `args` (workspace fields not read), or a negative status
 *   gemlite_hip_experts_rows_query            validates and never launches or dereferences; works without a GPU */
#define GEMLITE_EXPERTS_ROWS_MAX_EXPERTS 4096
typedef struct gemlite_hip_experts_rows_args {
    uint32_t struct_size;             /* sizeof(gemlite_hip_experts_rows_args), ABI guard */
    int32_t rows_per_block;           /* 0 (default) | 16 | 32 | 48 | 64 */
    gemlite_hip_experts_args experts; /* exactly as for gemlite_hip_forward_experts */
    void* workspace;                  /* device, the work table */
    uint64_t workspace_bytes;
    int64_t reserved[2];
} gemlite_hip_experts_rows_args;
uint64_t gemlite_hip_experts_rows_workspace_bytes(int64_t n_slots, int64_t n_experts, int32_t rows_per_block);
int gemlite_hip_experts_rows_per_block(const gemlite_hip_experts_rows_args* args);
int gemlite_hip_experts_route(const gemlite_hip_experts_rows_args* args, void* stream);
int gemlite_hip_forward_experts_rows(const gemlite_hip_experts_rows_args* args, void* stream);
int gemlite_hip_experts_rows_query(const gemlite_hip_experts_rows_args* args);

/* The batched expert MLP without an fp32 intermediate in memory: route, gate/up with SwiGLU inside, down, combine — four launches.
 *   gemlite_hip_forward_experts_rows_glu  gemlite_hip_forward_experts_rows on experts whose N columns are [gate; up] halves of I = N / 2
 *                                         columns (the layout of GEMLITE_EXPERTS_GLU), with the GLU epilogue of that call: grid (I / 16,
 *                                         Bmax), block (t, b) computes tile t and tile t + I / 16 of work block b.  With g, u the outputs
 *                                         of slot s as gemlite_hip_forward_experts_rows rounds them at the same R (bias included), its I
 *                                         outputs at rows.experts.layer.out + s * stride_out_slot are round(silu(g) * u): fp32, one
 *                                         rounding, silu exactly as GEMLITE_EXPERTS_GLU states it.  A slot of the invalid bucket gets I zeros.
 *                                         `rows` is a complete gemlite_hip_forward_experts_rows request (its own struct_size set) and is
 *                                         validated by the same rules first, stride_out_slot being the stride of the I-wide output rows;
 *                                         the work table is the one gemlite_hip_experts_route writes for the same R.
 *     Refusals beyond those of `rows`: GEMLITE_ERR_BAD_ARGUMENT (null struct, struct_size), GEMLITE_ERR_UNSUPPORTED (activation; groups
 *     of 32: the two-tile body has no form that fits the registers), GEMLITE_ERR_BAD_SHAPE (N % 32 != 0; rows_per_block above the GLU cap:
 *     64 for groups >= 128, 32 for groups of 64).  rows_per_block 0: the default rule of gemlite_hip_experts_rows_per_block under that cap.
 *   gemlite_hip_experts_rows_glu_per_block the R the library resolves for `args` (workspace fields not read), or a negative status
 *   gemlite_hip_experts_rows_glu_query     validates and never launches or dereferences; works without a GPU */
typedef struct gemlite_hip_experts_rows_glu_args {
    uint32_t struct_size;               /* sizeof(gemlite_hip_experts_rows_glu_args), ABI guard */
    int32_t activation;                 /* GEMLITE_ACT_SILU */
    gemlite_hip_experts_rows_args rows; /* exactly as for gemlite_hip_forward_experts_rows; out rows are I = N / 2 wide */
    int64_t reserved[2];
} gemlite_hip_experts_rows_glu_args;
int gemlite_hip_forward_experts_rows_glu(const gemlite_hip_experts_rows_glu_args* args, void* stream);
int gemlite_hip_experts_rows_glu_query(const gemlite_hip_experts_rows_glu_args* args);
int gemlite_hip_experts_rows_glu_per_block(const gemlite_hip_experts_rows_glu_args* args);

/*   gemlite_hip_experts_combine  the routing-weight sum over a token's slots in ONE launch (experts_combine_kernel): token t = the slots
 *                                t * slots_per_token + k, k < slots_per_token; with y_k the row of slot k at y + slot * stride_y_slot,
 *                                out + t * stride_out_token gets round(sum_k weights[slot_k] * float(y_k)) over the slots whose id lies in
 *                                [0, n_experts): each product an fp32 multiply of its own, then an fp32 add, ascending k from 0, one
 *                                rounding, no fused multiply-add — the numerics of GEMLITE_EXPERTS_COMBINE, so the same y gives the same
 *                                bits.  A slot with an invalid id (negative, too large, an int64 with a high dword) is skipped: neither
 *                                its y row nor its weight is read; a token without a valid id gets N zeros (+0).
 *     (The rows launches sort the slots by expert, so a token's slots lie in different work blocks: the sum is a launch of its own.)
 *     Domain: y and out fp16 or bf16 of the same type (`dtype`); ids int32 or int64; weights fp32 or `dtype`; N % 16 == 0;
 *     1 <= slots_per_token <= 64, a divisor of n_slots; n_slots <= 65535; y and out 4-byte aligned with even, non-negative row strides
 *     (what gemlite_hip_forward_experts_rows accepts for its output); every row offset plus N below 2^31 elements.  Rows that are
 *     16-byte aligned (pointers % 16, strides % 8) are moved in 16-byte requests, others in 4-byte requests: the same bits.
 *     GEMLITE_ERR_BAD_ARGUMENT (null or misaligned pointers, struct_size, non-positive counts, odd or negative strides),
 *     GEMLITE_ERR_UNSUPPORTED (dtypes), GEMLITE_ERR_BAD_SHAPE (N, slots_per_token, n_slots, the offset limit).
 *   gemlite_hip_experts_combine_query  validates and never launches or dereferences; works without a GPU */
#define GEMLITE_EXPERTS_COMBINE_MAX_SLOTS_PER_TOKEN 64
typedef struct gemlite_hip_experts_combine_args {
    uint32_t struct_size;           /* sizeof(gemlite_hip_experts_combine_args), ABI guard */
    int32_t dtype;                  /* of y and out: GEMLITE_DT_FP16 | GEMLITE_DT_BF16 */
    int32_t ids_dtype;              /* GEMLITE_DT_INT32 | GEMLITE_DT_INT64 */
    int32_t weights_dtype;          /* GEMLITE_DT_FP32 or dtype */
    const void* y;                  /* device, n_slots rows of N */
    const void* ids;                /* device, n_slots entries */
    const void* weights;            /* device, n_slots entries in the order of ids */
    void* out;                      /* device, n_slots / slots_per_token rows of N */
    int64_t n_slots, n_experts, slots_per_token, N;
    int64_t stride_y_slot, stride_out_token; /* elements */
    int64_t reserved[2];
} gemlite_hip_experts_combine_args;
int gemlite_hip_experts_combine(const gemlite_hip_experts_combine_args* args, void* stream);
int gemlite_hip_experts_combine_query(const gemlite_hip_experts_combine_args* args);

/*   gemlite_hip_experts_topk  the router's top-k in ONE launch (experts_topk_kernel): token t reads its n_experts logits at
 *                             logits + t * stride_logits_token and writes top_k ids and top_k routing weights at ids / weights + t * top_k —
 *                             what the experts launches above take as ids and weights.
 *     Selection: top_k rounds of an arg-max over (key, index): the greater key wins, among equal keys (-0 == +0) the lower index, a NaN
 *     key ranks above every number and NaNs tie among themselves by index.  Ids come out in selection order (descending key, like a
 *     sorted top-k).  For EVERY bit pattern of logits and bias the top_k ids of a token are distinct and lie in [0, n_experts).
 *     Arithmetic in fp32 (fp16 / bf16 logits convert exactly); a 16-bit weight is the fp32 weight rounded once.
 *       GEMLITE_EXPERTS_TOPK_SOFTMAX  key = the logit (softmax is monotone: the selection is exact).  With m the largest logit and
 *                                     p_j = exp(l_j - m): w_j = p_j / sum of p over the SELECTED (renormalize) or over ALL experts.
 *       GEMLITE_EXPERTS_TOPK_SIGMOID  key = the logit without bias (exact), sigmoid(l_j) + bias_j with it (bias fp32 [n_experts], the
 *                                     selection bias of DeepSeek-V3-style routers); w_j = sigmoid(l_j) = 1 / (1 + exp(-l_j)) never
 *                                     includes the bias, and is divided by the sum of w over the selected when renormalize is set.
 *     Both then multiply by `scale` (a multiply of its own).
 *     Domain: 1 <= n_experts <= GEMLITE_EXPERTS_TOPK_MAX_EXPERTS; 1 <= top_k <= min(n_experts,
 *     GEMLITE_EXPERTS_COMBINE_MAX_SLOTS_PER_TOKEN); logits fp16 / bf16 / fp32 with a unit inner stride, stride_logits_token >= n_experts,
 *     element-aligned; ids int32 / int64; weights fp32 / fp16 / bf16; bias fp32, contiguous, SIGMOID only; n_tokens >= 1 and
 *     n_tokens * top_k < 2^32.
 *     GEMLITE_ERR_BAD_ARGUMENT (null or misaligned pointers, struct_size, non-positive counts, renormalize not 0 / 1),
 *     GEMLITE_ERR_UNSUPPORTED (dtypes, scoring, a bias with SOFTMAX), GEMLITE_ERR_BAD_SHAPE (n_experts, top_k, the row stride, the
 *     n_tokens * top_k limit).
 *   gemlite_hip_experts_topk_query  validates and never launches or dereferences; works without a GPU */
#define GEMLITE_EXPERTS_TOPK_MAX_EXPERTS 1024
#define GEMLITE_EXPERTS_TOPK_SOFTMAX 0
#define GEMLITE_EXPERTS_TOPK_SIGMOID 1
typedef struct gemlite_hip_experts_topk_args {
    uint32_t struct_size;           /* sizeof(gemlite_hip_experts_topk_args), ABI guard */
    int32_t logits_dtype;           /* GEMLITE_DT_FP16 | GEMLITE_DT_BF16 | GEMLITE_DT_FP32 */
    int32_t ids_dtype;              /* GEMLITE_DT_INT32 | GEMLITE_DT_INT64 */
    int32_t weights_dtype;          /* GEMLITE_DT_FP32 | GEMLITE_DT_FP16 | GEMLITE_DT_BF16 */
    int32_t scoring;                /* GEMLITE_EXPERTS_TOPK_SOFTMAX | GEMLITE_EXPERTS_TOPK_SIGMOID */
    int32_t renormalize;            /* 0 | 1 */
    float scale;                    /* the weights' last factor (1.f: none) */
    int32_t reserved0;
    const void* logits;             /* device, n_tokens rows of n_experts */
    const void* bias;               /* device, n_experts fp32 entries, or NULL */
    void* ids;                      /* device, n_tokens * top_k entries */
    void* weights;                  /* device, n_tokens * top_k entries */
    int64_t n_tokens, n_experts, top_k;
    int64_t stride_logits_token;    /* elements */
    int64_t reserved[2];
} gemlite_hip_experts_topk_args;
int gemlite_hip_experts_topk(const gemlite_hip_experts_topk_args* args, void* stream);
int gemlite_hip_experts_topk_query(const gemlite_hip_experts_topk_args* args);

/* Per-token dynamic activation quantisation: for each row m of x[M,K] (fp16/bf16/fp32)
 *   s[m] = max(amax(|x[m,:]|) / qmax, 1e-6) (fp32);  y = clamp(x / s, qmin, qmax);
 *   int8: round half away from zero;  fp8: round-to-nearest-even cast.
 * out_dtype: GEMLITE_DT_INT8, GEMLITE_DT_FP8E4 or GEMLITE_DT_FP8E5. */
int gemlite_hip_scale_activations_per_token(const void* x, void* y, float* scales, int64_t M,
                                            int64_t K, int64_t stride_xm, int32_t in_dtype,
                                            int32_t out_dtype, void* stream);

/* Block-scaled activation quantisers (scale_activations_mxfp8 / mxfp4 / nvfp4_triton_v2, gemlite/quant_utils.py:
 * 502-590, 769-855, 859-954).  x [M, K] fp16 / bf16 / fp32, row stride stride_xm, K % 32 == 0 (nvfp4: % 16).
 *   mxfp8: y fp8 e4m3 [M, K];       scales e8m0 [M_pad, K/32], M_pad = M rounded up to a multiple of 32
 *   mxfp4: y uint8 [M, K/2] (e2m1 codes, k even in the low nibble); scales e8m0 [M_pad, K/32]
 *   nvfp4: y uint8 [M, K/2];        scales fp8 e4m3 [M_pad, K/16], M_pad = M rounded up to a multiple of 16
 * The block scale is the next power of two of amax / qmax (exponent clamped to [-30, 127]); nvfp4: e4m3(amax / 0.3).
 * Rows M .. M_pad-1 of `scales` receive the scale of an all-zero block, like the reference's padded programs. */
int gemlite_hip_scale_activations_mxfp8(const void* x, void* y, uint8_t* scales, int64_t M, int64_t K,
                                        int64_t stride_xm, int32_t in_dtype, void* stream);
int gemlite_hip_scale_activations_mxfp4(const void* x, uint8_t* y, uint8_t* scales, int64_t M, int64_t K,
                                        int64_t stride_xm, int32_t in_dtype, void* stream);
int gemlite_hip_scale_activations_nvfp4(const void* x, uint8_t* y, uint8_t* scales, int64_t M, int64_t K,
                                        int64_t stride_xm, int32_t in_dtype, void* stream);

/* Bit-pack W_q[N, K] (uint8 values < 2^W_nbits, row stride ld_in) along K into words of
 * pack_bits: word(n, j) = OR_i W_q[n, j*e+i] << (W_nbits*i), e = pack_bits/W_nbits, stored
 * TRANSPOSED and contiguous: out[j*N + n]  (shape [K/e, N]) — the layout GemLiteLinear.pack()
 * produces with transpose=True + .contiguous() (core.py:384-398,478-480). */
int gemlite_hip_pack_over_cols(const uint8_t* w_q, void* out, int64_t N, int64_t K, int64_t ld_in,
                               int32_t W_nbits, int32_t pack_bits, void* stream);
/* Inverse: out[N, K] uint8 from packed [K/e, N]. */
int gemlite_hip_unpack_over_cols(const void* packed, uint8_t* out, int64_t N, int64_t K,
                                 int32_t W_nbits, int32_t pack_bits, void* stream);

/* Quantise float weights W[N, K] (fp32 / fp16 / bf16, row stride ld_w) to grouped asymmetric INT: round to nearest on the min / max of
 * every group of group_size consecutive k of a row — one (scale, zero) pair per (n, group), T = meta_dtype (fp16 / bf16), rT = round to
 * T and back, every step a single fp32 IEEE operation:
 *     s = (hi - lo) / (2^W_nbits - 1), s < 2^-14 -> 1;   s_r = rT(s);   z_r = rT(-lo / s_r);
 *     q = clamp(rint(w / s_r + z_r), 0, 2^W_nbits - 1)          (rint: half to even; the layer computes (q - z_r) * s_r)
 *   pack_bits 32: q_out = the packed words [K/e, N] of gemlite_hip_pack_over_cols (ld_q unused);
 *   pack_bits 0 : q_out = uint8 codes [N, K] with row stride ld_q.
 *   scales / zeros: element (group j, row n) at j * stride_meta_g + n * stride_meta_n (elements): (N, 1) is the layer's [K/g, N],
 *   (1, K/g) is [N * K/g, 1].  fold_zeros != 0 stores rT(-z_r * s_r) instead of z_r (what pack() keeps for W_group_mode 4).
 * group_size % 32 == 0, K % group_size == 0; one launch, no workspace.  Non-finite weights give unspecified codes (and no fault). */
typedef struct gemlite_hip_quantize_args {
    uint32_t struct_size; /* = sizeof(gemlite_hip_quantize_args), ABI guard */
    int32_t w_dtype;      /* GEMLITE_DT_FP32 / FP16 / BF16 */
    const void* w;
    int64_t N, K, ld_w;
    int32_t W_nbits;      /* 1, 2, 4, 8 */
    int32_t group_size;
    int32_t pack_bits;    /* 0 or 32 */
    int32_t meta_dtype;   /* GEMLITE_DT_FP16 / BF16 */
    void* q_out;
    int64_t ld_q;
    void* scales;
    void* zeros;
    int64_t stride_meta_g, stride_meta_n;
    int32_t fold_zeros;
    int32_t reserved;     /* 0 */
} gemlite_hip_quantize_args;
int gemlite_hip_quantize_groups(const gemlite_hip_quantize_args* args, void* stream);

/* The same launch with HQQ's proximal optimiser on the ZERO of every group between the metadata and the codes (the scale stays s_r).
 * `q` is the struct above, read exactly as there (outputs, layouts, fold_zeros, limits).  Per group of g = group_size weights, fp32:
 *     Q(z) = clamp(rint(w / s_r + z), 0, qmax);   E(z) = mean_k |w - (Q(rT(z)) - rT(z)) * s_r|     (the error of what the layer computes)
 *     z = z0 = -lo / s_r;  best_z = z0, best_E = E(z0)                     (rT(z0) is z_r above: iteration 0 is round to nearest)
 *     for i in 0 .. iters-1, while the group is alive:   beta_i = beta * kappa^i
 *         q = Q(z);  r = w - (q - z) * s_r;  e = sign(r) * max(|r| - |r|^(lp_norm - 1) / beta_i, 0)      (e = 0 where r == 0)
 *         z = mean_k(q - (w - e) / s_r);   E(z) < best_E ? best_z, best_E = z, E(z) : the group stops
 *     stored: s_r, z_r = rT(best_z), codes Q(z_r)
 * Unlike HQQ's optimize_weights_proximal the stop is per group, the best zero seen is kept (not the last), and the error is taken against
 * the rounded zero: no group ends worse than round to nearest.  The order of the sums inside a group is fixed by the kernel: the same
 * input gives the same bits on every run, in both output forms, wherever the group sits.  The last bit of the power is not part of the
 * contract.  0 <= iters <= 100 (0: byte for byte the launch above), 0 < lp_norm <= 1, beta > 0, kappa > 0 (finite): anything else is
 * GEMLITE_ERR_BAD_ARGUMENT; a bad `q` returns what the launch above returns for it; nothing is launched then.  HQQ's defaults: 20, 0.7,
 * 10, 1.01.  Non-finite weights: unspecified codes for their group, no fault, the loop ends (a comparison with NaN stops the group). */
typedef struct gemlite_hip_quantize_hqq_args {
    uint32_t struct_size; /* = sizeof(gemlite_hip_quantize_hqq_args), ABI guard */
    int32_t iters;
    gemlite_hip_quantize_args q; /* q.struct_size = sizeof(gemlite_hip_quantize_args) */
    float lp_norm, beta, kappa;
    int32_t reserved;     /* 0 */
} gemlite_hip_quantize_hqq_args;
int gemlite_hip_quantize_groups_hqq(const gemlite_hip_quantize_hqq_args* args, void* stream);

/* Quantise float weights W[N, K] (fp32 / fp16 / bf16, unit inner stride, row stride ld_w >= K) to a block-scaled format in one launch
 * on `stream`: no workspace, no atomics, 64-bit indices.  K % 32 == 0.  Every step is ONE fp32 IEEE operation (correctly rounded
 * divisions, nothing contracts); amax = max |w| over the block:
 *   format 0 MXFP8 / 1 MXFP4, block = 32 consecutive k of a row:  ideal = amax / qmax (448.f / 6.f);
 *       ex = exponent_field(ideal) + (mantissa(ideal) != 0), clamped to [97, 254];  scale byte (e8m0) = ex, s = 2^(ex - 127)
 *       (= the reference's 2^ceil(log2(ideal)) floored at 2^-30, taken from the bits: the bit form is the contract)
 *     MXFP8 element: e4m3fn_rne(clamp(w / s, -448, 448))
 *     MXFP4 element: q = w / s, c = #{0.25, 0.75, 1.25, 1.75, 2.5, 3.5, 5.0 strictly below |q|} (a midpoint takes the lower value),
 *       code = c + 8 if q < 0 and c > 0, else c.  (NOT the activation quantiser's rule: no eighth threshold, and a negative weight
 *       that rounds to zero is code 0, not 8.)
 *   format 2 NVFP4, block = 16 k:  t = (amax / 6.f) / 0.05f (two divisions);  scale byte s8 = e4m3fn_rne(min(t, 448));
 *       full = max(float(s8) * 0.05f, 1e-6f);  codes from q = w / full by the rule above (|q| > 7 under a clamped scale stays 7 / 15).
 *   A block that holds a NaN or an Inf gets the scale format's NaN code (e8m0 0xFF, e4m3 0x7F); its element bytes are unspecified
 *   (written, no fault); every other block is unaffected.
 * q_out: MXFP8 e4m3 bytes [N][K]; fp4 formats: pack_nibbles 0 = one code per byte [N][K], 1 = two per byte [N][K/2], even k in the
 * low nibble (what a packed layer stores); row stride ld_q bytes.  scales: one byte per block j of row n at
 * j * stride_scale_g + n * stride_scale_n: (N, 1) is the layer's [K/g, N], (1, K/g) is [N * K/g, 1].
 * Checked on the host before the launch: BAD_ARGUMENT (null pointers, struct_size, N / K <= 0, ld_w < K, ld_q below a row),
 * UNSUPPORTED (format, dtype, pack_nibbles with MXFP8), BAD_SHAPE (K % 32 != 0, more than 65535 * 256 k). */
typedef struct gemlite_hip_quantize_mx_args {
    uint32_t struct_size; /* = sizeof(gemlite_hip_quantize_mx_args), ABI guard */
    int32_t w_dtype;      /* GEMLITE_DT_FP32 / FP16 / BF16 */
    const void* w;
    int64_t N, K, ld_w;
    int32_t format;       /* 0 MXFP8, 1 MXFP4, 2 NVFP4 */
    int32_t pack_nibbles; /* 0 or 1 (fp4 formats only) */
    void* q_out;
    int64_t ld_q;
    void* scales;
    int64_t stride_scale_g, stride_scale_n;
    int64_t reserved;     /* 0 */
} gemlite_hip_quantize_mx_args;
int gemlite_hip_quantize_mx(const gemlite_hip_quantize_mx_args* args, void* stream);

/* Dequantise a layer's weights: out[n, k] (fp16 / bf16 / fp32, K-contiguous, row stride ld_out >= K elements) = the weight the layer
 * multiplies x[:, k] by for output n, from the layer's stored tensors only.  The weight fields mean what they mean in
 * gemlite_hip_forward_args, so a caller fills both structs from one layer.  Every step is ONE fp32 IEEE operation (nothing contracts),
 * then one round-to-nearest-even conversion to out_dtype (overflow gives Inf, NaN stays NaN):
 *   integer / plain layers (q = the code of the packed word, or the int8 / uint8 / fp8 e4m3fn / fp8 e5m2 / 16- / 32-bit float element, exact)
 *     W_group_mode 0: d = q | 1: d = q - z | 2: d = q * s | 3: d = (q - z) * s | 4: d = fmaf(q, s, z') (z' = the stored folded zero)
 *       s, z: element (k / group_size, n) of scales / zeros at g * stride_meta_g + n * stride_meta_n; zero_is_scalar: z = zeros[0]
 *     channel_scale_mode 1 or 3: d = d * c[n], c[n] = scales[n * stride_meta_n] (the layer's [1, N] weight scale); 0 and 2: nothing
 *   block-scaled layers (input_dtype GEMLITE_DT_MXFP16 .. GEMLITE_DT_NVFP4; W_group_mode / channel_scale_mode / zeros ignored)
 *     MXFP8 (W_nbits 8, w_dtype FP8E4, group 32) / MXFP4 (W_nbits 4, group 32):  d = elem * 2^(b - 127), b = the e8m0 byte, 0xFF -> NaN
 *     NVFP4 (input_dtype NVFP4, W_nbits 4, group 16):  d = elem * float(s8), s8 = the e4m3 byte (exact product; a NaN byte -> NaN)
 *     fp4 codes: elements_per_sample 2 = two per byte, even k in the low nibble (the layer); 1 = one code per byte (the quantiser's return)
 *   post_scale != 1.0f: d = d * post_scale, one more multiply (0.05f for an NVFP4 layer; 1.0f keeps the quantiser-level value)
 * Non-finite metadata propagates to the elements it belongs to and nowhere else.  One launch on `stream`, no workspace, no atomics,
 * 64-bit addresses.  32-bit words with stride_wn == 1, group_size % 8 == 0 and a 16-byte aligned out / row pitch take the tiled
 * kernel; K-contiguous (stride_wk == 1) 8-bit elements and block-scaled bytes without a zero take the streaming kernel; every other
 * layout (8- / 16-bit words, any strides, any group size that divides K, 16- / 32-bit float elements, unaligned out) takes a plain
 * per-element kernel.  Checked on the host before the launch: BAD_ARGUMENT (null pointers, struct_size, N / K / group_size /
 * elements_per_sample <= 0, ld_out < K, missing scales / zeros for the mode, words that do not hold elements_per_sample codes),
 * UNSUPPORTED (dtypes, bit width, modes, a *NUZ fp8, 64-bit words, a block-scaled combination that is no format),
 * BAD_SHAPE (K not a multiple of elements_per_sample / group_size / the block size, grid limits). */
typedef struct gemlite_hip_dequantize_args {
    uint32_t struct_size; /* = sizeof(gemlite_hip_dequantize_args), ABI guard */
    int32_t out_dtype;    /* GEMLITE_DT_FP16 / BF16 / FP32 */
    const void* w_q;
    const void* scales;
    const void* zeros;
    void* out;
    int64_t N, K;
    int64_t stride_wk, stride_wn;
    int64_t stride_meta_g, stride_meta_n;
    int64_t ld_out;
    int32_t W_nbits, group_size, elements_per_sample, w_pack_bits, w_dtype;
    int32_t input_dtype;  /* selects the block-scaled formats, as for forward; anything else: an integer / plain layer */
    int32_t meta_dtype, zeros_dtype, zero_is_scalar;
    int32_t W_group_mode, channel_scale_mode;
    float post_scale;
    int64_t reserved;     /* 0 */
} gemlite_hip_dequantize_args;
int gemlite_hip_dequantize(const gemlite_hip_dequantize_args* args, void* stream);

/* Quantise float weights W[N, K] (fp32 / fp16 / bf16, unit inner stride, row stride ld_w >= K elements) to channel-wise symmetric 8-bit
 * codes and one scale per row — the tensors an A16W8 / A8W8 layer holds — in one launch on `stream`: no workspace, no atomics, 64-bit
 * addresses, capturable.  Per row n, every step ONE fp32 IEEE operation (correctly rounded divisions, nothing contracts, denormals kept):
 *     amax = max_k |w[n, k]|                       (exact: widening to fp32 is exact)
 *     scale_rule 0: s = amax / qmax      scale_rule 1: s = amax * (1.0f / qmax)        qmax = 127.f | 448.f | 57344.f
 *     s = max(s, 1e-6f)                            (the fp32 nearest to 1e-6)
 *     q = min(max(w / s, qmin), qmax)              qmin = -128.f | -448.f | -57344.f
 *     format 0 int8: rint(q), half to even, stored as int8
 *     format 1 e4m3fn, 2 e5m2: one round-to-nearest-even conversion (subnormal results kept, -0 keeps its sign)
 *     scales[n * stride_s] = s as fp32, or rounded once (RNE) to fp16 / bf16 (scale_dtype); the codes always use the fp32 s
 * Rule 0 is a true division by the format's maximum (what torch computes for `amax / max` on a CPU tensor), rule 1 the multiplication
 * by its fp32 reciprocal; they differ in the last bit of s for some amax.
 * A row that holds a NaN or an Inf gets a non-finite scale; its codes are unspecified (written, no fault); every other row is unaffected.
 * q_out: bytes [N][K], row stride ld_q >= K bytes.  Rows of at most GEMLITE_QUANT_ROWS_WAVE_MAX_K elements take one wave each, rows of
 * at most GEMLITE_QUANT_ROWS_RESIDENT_MAX_K one block that reads the weight once, longer rows one block that reads it twice; any
 * alignment of w / q_out / ld_w / ld_q and any K are correct (narrower accesses).
 * Checked on the host before the launch: BAD_ARGUMENT (null pointers, struct_size, N / K <= 0, ld_w < K, ld_q < K, stride_s <= 0),
 * UNSUPPORTED (dtypes, format, scale_rule), BAD_SHAPE (N beyond the grid limit 2^31 - 1). */
#define GEMLITE_QUANT_ROWS_WAVE_MAX_K 1024
#define GEMLITE_QUANT_ROWS_RESIDENT_MAX_K 16384
typedef struct gemlite_hip_quantize_rows_args {
    uint32_t struct_size; /* = sizeof(gemlite_hip_quantize_rows_args), ABI guard */
    int32_t w_dtype;      /* GEMLITE_DT_FP32 / FP16 / BF16 */
    const void* w;
    int64_t N, K, ld_w;
    int32_t format;       /* 0 int8, 1 fp8 e4m3fn, 2 fp8 e5m2 */
    int32_t scale_rule;   /* 0 divide by qmax, 1 multiply by 1.0f / qmax */
    void* q_out;
    int64_t ld_q;
    void* scales;
    int64_t stride_s;     /* elements of scale_dtype between the scales of consecutive rows */
    int32_t scale_dtype;  /* GEMLITE_DT_FP32 / FP16 / BF16 */
    int32_t reserved;     /* 0 */
} gemlite_hip_quantize_rows_args;
int gemlite_hip_quantize_rows(const gemlite_hip_quantize_rows_args* args, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* GEMLITE_HIP_H */
