// gl_host.h — every host function of libgemlite_hip.so that one translation unit defines and another calls: the planners and kernel
// getters (defined next to their kernels), the capture groups, ensure_lds.  The file that defines one of these includes this header too,
// so a definition always sees its declaration; default arguments are written here and nowhere else.
#pragma once
#include "gl_common.h"

namespace gl {

// ---- planners of the forward kernels: true = the kernel takes the request, the launch is described in lp (and p / g) -----------------
bool plan_gemv_wn(const gemlite_hip_forward_args& a, WnParams& p, LaunchPlan& lp);         // gemv_wn.hip
bool plan_gemv_mfma(const gemlite_hip_forward_args& a, WnParams& p, LaunchPlan& lp);       // gemv_mfma.hip
bool plan_gemv_a8wn(const gemlite_hip_forward_args& a, WnParams& p, LaunchPlan& lp, bool fq = false);  // gemv_a8wn.hip
bool plan_a8wn_rows(const gemlite_hip_forward_args& a, WnParams& p, LaunchPlan& lp);
bool plan_gemm_wn_stream(const gemlite_hip_forward_args& a, WnParams& p, LaunchPlan& lp);  // gemm_wn_stream.hip
bool plan_gemm_wn_direct(const gemlite_hip_forward_args& a, WnParams& p, LaunchPlan& lp);  // gemm_wn_direct.hip
bool plan_gemm_wn_rows(const gemlite_hip_forward_args& a, WnParams& p, LaunchPlan& lp);    // gemm_wn_rows.hip
bool plan_gemm_wn_tiled(const gemlite_hip_forward_args& a, WnParams& p, LaunchPlan& lp);   // gemm_wn_tiled.hip
bool plan_gemm_wn_mma(const gemlite_hip_forward_args& a, WnParams& p, LaunchPlan& lp);     // gemm_wn_mma.hip
bool plan_gemm_wn_mma_mx(const gemlite_hip_forward_args& a, WnParams& p, LaunchPlan& lp, int mode = 0);
bool plan_gemm_a8w8(const gemlite_hip_forward_args& a, LaunchPlan& lp);                    // gemm_a8w8.hip
bool plan_gemm_a8w8_mma(const gemlite_hip_forward_args& a, GenericParams& g, LaunchPlan& lp);
bool plan_gemm_a8w8_sq(const gemlite_hip_forward_args& a, GenericParams& g, LaunchPlan& lp);
bool plan_gemm_a8w8_sq128(const gemlite_hip_forward_args& a, GenericParams& g, LaunchPlan& lp);
bool plan_a8w8_rows(const gemlite_hip_forward_args& a, LaunchPlan& lp, bool fq = false);
bool plan_a16w8_rows(const gemlite_hip_forward_args& a, LaunchPlan& lp);
bool a16w8_rows_lds_pays(const gemlite_hip_forward_args& a);
bool k_rotation_pays(const gemlite_hip_forward_args& a, int64_t tile_bytes);
int k_order_flags(const gemlite_hip_forward_args& a, int64_t tile_bytes);
bool plan_w8_rows_lds(const gemlite_hip_forward_args& a, LaunchPlan& lp, int mt, bool two);  // gemm_w8_rows.hip
bool plan_gemm_mx_mma(const gemlite_hip_forward_args& a, GenericParams& g, LaunchPlan& lp);  // gemm_mx.hip
bool plan_gemm_mx_sq(const gemlite_hip_forward_args& a, GenericParams& g, LaunchPlan& lp);
bool plan_gemm_mx_tile(const gemlite_hip_forward_args& a, GenericParams& g, LaunchPlan& lp);
bool plan_mx_gemv(const gemlite_hip_forward_args& a, GenericParams& g, LaunchPlan& lp);
bool plan_mx_rows(const gemlite_hip_forward_args& a, GenericParams& g, LaunchPlan& lp, bool any_m = false, bool fq = false);
bool plan_nvfp4_rows(const gemlite_hip_forward_args& a, GenericParams& g, LaunchPlan& lp, bool fq = false);

// ---- kernel getters ------------------------------------------------------------------------------------------------------------------
const void* mx_generic_kernel_fn();  // gemm_mx.hip
const void* act_quant_mx_kernel_fn(int mode);
const void* nvfp4_expand_f16_kernel_fn();
const void* generic_kernel_fn();  // generic.hip
const void* kmajor_kernel_fn(int mb);
const void* kmajor_w8a16_kernel_fn(int mb);
const void* kmajor_fused_quant_kernel_fn(int qdt);
const void* a8w8_decode_kernel_fn(int qdt, bool fused);
const void* a16w8_decode_kernel_fn(int x_dt, int w_dt);
const void* act_quant_kernel_fn();
const void* act_quant_vec_kernel_fn(int in_dt, int out_dt, int64_t K, int64_t stride_xm, const void* x, const void* y);
const void* pack_kernel_fn();
const void* pack32_kernel_fn();
const void* unpack_kernel_fn();
const void* quantize_groups_kernel_fn(bool onepass);  // quantize_groups.hip
const void* quantize_hqq_kernel_fn(bool onepass);
const void* quantize_mx_kernel_fn(int format);              // quantize_mx.hip
const void* quantize_rows_kernel_fn(int format, int64_t K);  // quantize_rows.hip
const void* dequantize_words_kernel_fn(int nbits);          // dequantize.hip
const void* dequantize_rows_kernel_fn(int fmt);
const void* dequantize_any_kernel_fn();
const void* gemv_w4_decode3_fn(int tag, bool nt);  // gemv_decode.hip
const void* gemv_w4_decode3_bias_fn(int tag, bool nt);
// the grouped forms (h: tiles per wave; nt: non-temporal weight requests, H >= 2 only).  A group holds biased launches
// or unbiased ones, never both, and launches of one load policy: their kernel functions differ, so same_launch() keeps them apart
const void* gemv_w4_decode3_group_fn(int tag, bool biased, bool shared_x, int h, bool nt);
const void* gemv_w4_decode3_experts_fn(int tag, bool biased, bool ids64);
const void* gemv_w4_decode3_experts_fused_fn(int tag, int epilogue, bool biased, bool ids64);
const void* gemm_wn_rows_group_fn(int tag, int mt, int spg, int nt, int bits, bool biased);  // gemm_wn_rows_group.hip: the grouped forms
const void* gemm_wn_rows_experts_fn(int tag, int mt, int spg, bool biased);  // gemm_wn_rows_experts.hip
size_t gemm_wn_rows_experts_lds_bytes();
const void* gemm_wn_rows_experts_glu_fn(int tag, int mt, int spg, bool biased);  // gemm_wn_rows_experts_glu.hip (nullptr: no such form)
const void* experts_route_fn(bool ids64);  // experts_route.hip
const void* experts_combine_fn(int tag, bool ids64, bool w32, bool wide);  // experts_combine.hip
int experts_combine_threads();
const void* experts_topk_fn(int ldt, int per_lane);  // experts_topk.hip; ldt 0: fp16, 1: bf16, 2: fp32; per_lane 1 / 2 / 4 / 8 / 16
int experts_topk_threads();
// the instantiations of gemm_wn_mma_kernel.inc, one translation unit per activation type and word width (gemm_wn_mma_*.hip)
const void* mma_lookup_f16(int kind, int nbits, int mi, int xdt);
const void* mma_lookup_bf16(int kind, int nbits, int mi, int xdt);
const void* mma_lookup_pw_f16_b8(int kind, int nbits, int mi);
const void* mma_lookup_pw_f16_b16(int kind, int nbits, int mi);
const void* mma_lookup_pw_bf16_b8(int kind, int nbits, int mi);
const void* mma_lookup_pw_bf16_b16(int kind, int nbits, int mi);

// ---- capture_group.hip: independent decode3 (or rows) launches of one stream capture folded into one grouped launch -------------------
int capture_group_limit();
void capture_group_stats(uint64_t* seen, uint64_t* joined);
bool capture_group_compatible(const gemlite_hip_forward_args& a, const LaunchPlan& la, const gemlite_hip_forward_args& b, const LaunchPlan& lb);
bool capture_group_try_join(const gemlite_hip_forward_args& a, const LaunchPlan& lp, hipStream_t st, int resident, int dev);
void capture_group_note_launch(const gemlite_hip_forward_args& a, const LaunchPlan& lp, hipStream_t st);
bool capture_group_shared_x_enabled();
int capture_group_last_form();
int capture_group_last_lines();
int capture_group_last_rounds();
int capture_group_rounds_max();
void capture_group_merge_stats(uint64_t* merged);
int capture_group_last_policy();
int capture_group_policy_forced();
int capture_group_lines_wanted(int tiles, int members, int resident, int tb);
Decode3TilesWanted capture_group_tiles_wanted(int tiles, int members, int resident);

// ---- api.hip ---------------------------------------------------------------------------------------------------------------------------
// Raise the dynamic-LDS cap of a kernel above 64 KiB: once per (device, kernel)
int ensure_lds(const void* fn, size_t lds, int dev);

}  // namespace gl
