// gl_plan.h — what api.hip (the C ABI, the launch code) sees of the forward planner (plan_forward.hip): a request is validated, then
// resolved to ONE kernel with its launch geometry and parameter block.  Host code only; nothing here touches a device.
#pragma once
#include "gl_common.h"

namespace gl {

enum Kind { K_NONE = 0, K_GEMV_WN, K_STREAM_WN, K_TILED_WN, K_KMAJOR, K_A8_MMA, K_A8_FQ, K_NV_MMA, K_GENERIC };

struct Resolved {
    Kind kind = K_NONE;
    LaunchPlan lp{};
    WnParams wn{};
    GenericParams gp{};
    int status = GEMLITE_OK;
    uint64_t nv_x16_bytes = 0;  // K_NV_MMA: bytes of the fp16 expansion of x in the workspace (behind the split-K slabs)
};

inline bool is_mx_input(int dt) { return dt >= GEMLITE_DT_MXFP16 && dt <= GEMLITE_DT_NVFP4; }

// what must hold before any kernel is chosen: GEMLITE_OK or the status the call returns
int validate(const gemlite_hip_forward_args* a);
// kernel selection: r.status, and for GEMLITE_OK the kind, the launch plan and the parameter block of the kind.  Plans for the device
// resident_block_limit() answers for.
void resolve(const gemlite_hip_forward_args& a, Resolved& r);
// rewrites a resolved plan to the form of its kernel that adds the caller's bias; false: the bias is left to the caller
bool apply_bias(const gemlite_hip_forward_args& a, const gemlite_hip_forward_ext* e, Resolved& r);

}  // namespace gl
