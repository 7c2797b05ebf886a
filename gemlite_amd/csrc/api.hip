// api.hip — the C ABI of libgemlite_hip.so (include/gemlite_hip.h): the device check, workspace carving and launch of a planned
// forward, the experts and quantise entry points.  Host code only; validation and kernel selection are the planner's (plan_forward.hip,
// asked through gl_plan.h), the kernels live next to their own planners (gl_host.h).
#include <hip/hip_runtime.h>
#include <stdio.h>
#include <string.h>

#include <atomic>
#include <mutex>
#include <set>
#include <string>

#include "gl_common.h"
#include "gl_async.h"
#include "gl_coopquant.h"
#include "gl_host.h"
#include "gl_plan.h"

using namespace gl;

// kernel label of a form for 8- / 16-bit packed words: the 32-bit label with ",b8" / ",b16" before the closing '>' (interned: labels are C strings
// that live as long as the library)
const char* gl::pw_label(const char* name, int pack_bits) {
    if (pack_bits == 32) return name;
    static std::mutex mu;
    static std::set<std::string>* names = new std::set<std::string>();
    std::string s(name);
    s.insert(s.size() - 1, pack_bits == 8 ? ",b8" : ",b16");
    std::lock_guard<std::mutex> lock(mu);
    return names->insert(s).first->c_str();
}

// kernel label of a form that adds the bias in its epilogue: ",bias" before the closing '>' (interned like the labels above)
const char* gl::bias_label(const char* name) {
    static std::mutex mu;
    static std::set<std::string>* names = new std::set<std::string>();
    std::string s(name);
    s.insert(s.size() - 1, ",bias");
    std::lock_guard<std::mutex> lock(mu);
    return names->insert(s).first->c_str();
}

static thread_local int tl_last_hip_error = 0;
static thread_local void* tl_evt_start = nullptr;
static thread_local void* tl_evt_stop = nullptr;

static int launch(const void* fn, dim3 grid, dim3 block, void** kargs, size_t lds, hipStream_t stream) {
    hipError_t err;
    if (tl_evt_start || tl_evt_stop) {
        err = hipExtLaunchKernel(fn, grid, block, kargs, lds, stream, (hipEvent_t)tl_evt_start, (hipEvent_t)tl_evt_stop, 0);
        tl_evt_start = tl_evt_stop = nullptr;
    } else {
        err = hipLaunchKernel(fn, grid, block, kargs, lds, stream);
    }
    if (err != hipSuccess) {
        tl_last_hip_error = (int)err;
        (void)hipGetLastError();
        return GEMLITE_ERR_LAUNCH;
    }
    return GEMLITE_OK;
}

// CU count PER DEVICE (one process-global minimum made the planners' choices depend on which other devices the process had
// touched).  gemlite_hip_forward names the device it plans for (tl_plan_dev); the host-only queries (gemlite_hip_kernel_name,
// gemlite_hip_query, gemlite_hip_workspace_bytes) plan for a full 256-CU part, whatever was launched before.
static std::atomic<int> g_cu_by_dev[64];
static thread_local int tl_plan_dev = -1;
int gl::resident_block_limit() {
    if (tl_plan_dev < 0) return 256;
    const int n = g_cu_by_dev[tl_plan_dev & 63].load(std::memory_order_relaxed);
    return n > 0 ? n : 256;
}

// The current device must be a gfx950 part: the code object holds no other ISA.  Checked once per device id.
static int check_device(int* dev_out) {
    int dev = -1;
    if (hipGetDevice(&dev) != hipSuccess || dev < 0) { (void)hipGetLastError(); return GEMLITE_ERR_NO_DEVICE; }
    *dev_out = dev;
    static std::atomic<int> state[64];  // 0 unknown | 1 gfx950 | 2 something else
    const int slot = dev & 63;
    int st = state[slot].load(std::memory_order_relaxed);
    if (st == 0) {
        hipDeviceProp_t prop;
        st = (hipGetDeviceProperties(&prop, dev) == hipSuccess && strncmp(prop.gcnArchName, "gfx950", 6) == 0) ? 1 : 2;
        // what the planners may assume co-resident on THIS device (partitioned devices report fewer CUs)
        if (st == 1 && prop.multiProcessorCount > 0) g_cu_by_dev[slot].store(prop.multiProcessorCount, std::memory_order_relaxed);
        state[slot].store(st, std::memory_order_relaxed);
    }
    return st == 1 ? GEMLITE_OK : GEMLITE_ERR_NO_DEVICE;
}

// Raise the dynamic-LDS cap of a kernel above 64 KiB: once per (device, kernel) — the attribute is per device.
int gl::ensure_lds(const void* fn, size_t lds, int dev) {
    if (lds <= 65536) return GEMLITE_OK;
    struct Done { const void* fn; int dev; };
    static thread_local Done done[32] = {};
    for (const Done& d : done) if (d.fn == fn && d.dev == dev) return GEMLITE_OK;
    hipError_t err = hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    if (err != hipSuccess) { tl_last_hip_error = (int)err; (void)hipGetLastError(); return GEMLITE_ERR_LAUNCH; }
    static thread_local int next = 0;
    done[next] = Done{fn, dev};
    next = (next + 1) & 31;
    return GEMLITE_OK;
}

__global__ void gemlite_noop_kernel() {}

// gemlite_hip_forward_ext: 0 = usable (NULL: no extension), else a negative status
static int validate_ext(const gemlite_hip_forward_ext* e) {
    if (e && e->struct_size != sizeof(gemlite_hip_forward_ext)) return GEMLITE_ERR_BAD_ARGUMENT;
    return GEMLITE_OK;
}

extern "C" {

int gemlite_hip_abi_version(void) { return GEMLITE_HIP_ABI_VERSION; }

const char* gemlite_hip_build_info(void) {
    return "libgemlite_hip gfx950 (CDNA4) abi=1 kernels: gemv_wn, gemv_decode, gemv_mfma, gemv_a8wn, gemm_wn_rows, gemm_wn_direct, gemm_wn_stream, gemm_wn_mma, gemm_wn_tiled, gemm_a8w8, "
           "gemm_mx, mx_rows, nvfp4_f16, kmajor, generic, act_quant_per_token, act_quant_mx, pack/unpack_over_cols, quantize_groups, quantize_mx, dequantize, quantize_hqq, quantize_rows"
#ifdef GL_AB_KERNELS
           " +ab_kernels"
#endif
        ;
}

const char* gemlite_hip_status_string(int status) {
    switch (status) {
        case GEMLITE_OK: return "ok";
        case GEMLITE_ERR_BAD_ARGUMENT: return "bad argument (null pointer, non-positive size or ABI struct_size mismatch)";
        case GEMLITE_ERR_UNSUPPORTED: return "unsupported dtype / bit-width / mode combination";
        case GEMLITE_ERR_BAD_SHAPE: return "bad shape (K not divisible by elements_per_sample / group_size, or too large)";
        case GEMLITE_ERR_WORKSPACE: return "workspace missing or too small";
        case GEMLITE_ERR_LAUNCH: return "HIP launch failed (see gemlite_hip_last_hip_error)";
        case GEMLITE_ERR_NO_DEVICE: return "current device is not gfx950";
        case GEMLITE_ERR_NO_FUSED_QUANT: return "no kernel with in-launch activation quantisation for this shape: quantise x first and pass scales_x";
        default: return "unknown status";
    }
}

int gemlite_hip_last_hip_error(void) { return tl_last_hip_error; }

int gemlite_hip_query(const gemlite_hip_forward_args* args) {
    const int v = validate(args);
    if (v != GEMLITE_OK) return v;
    Resolved r;
    resolve(*args, r);
    return r.status;
}

uint64_t gemlite_hip_workspace_bytes(const gemlite_hip_forward_args* args) {
    if (validate(args) != GEMLITE_OK) return 0;
    Resolved r;
    resolve(*args, r);
    return r.status == GEMLITE_OK ? r.lp.ws_bytes : 0;
}

const char* gemlite_hip_kernel_name(const gemlite_hip_forward_args* args) {
    if (validate(args) != GEMLITE_OK) return "invalid";
    Resolved r;
    resolve(*args, r);
    return r.status == GEMLITE_OK ? r.lp.name : "unsupported";
}

void gemlite_hip_set_profile_events(void* start_event, void* stop_event) {
    tl_evt_start = start_event;
    tl_evt_stop = stop_event;
}

int gemlite_hip_capture_group_max(void) { return capture_group_limit(); }

void gemlite_hip_capture_group_stats(uint64_t* seen, uint64_t* joined) { capture_group_stats(seen, joined); }

int gemlite_hip_capture_group_grid_y(int32_t tiles, int32_t members) {
    return (tiles > 0 && members > 0) ? decode3_group_grid_y(tiles, members, 256) : 0;
}

void gemlite_hip_capture_group_wave_split(int32_t layers_in_block, int32_t wave, int32_t out[3]) {
    if (!out) return;
    Decode3WaveSplit s{-1, 0, 0};
    if (layers_in_block >= 1 && layers_in_block <= DECODE3_GMAX && wave >= 0 && wave < 16) s = decode3_wave_split(layers_in_block, wave);
    out[0] = s.layer; out[1] = s.v0; out[2] = s.v1;
}

int gemlite_hip_capture_group_last_form(void) { return capture_group_last_form(); }

int gemlite_hip_capture_group_geometry(int32_t tiles, int32_t members, int32_t resident, int32_t tb_want, int32_t span_want, int32_t out[4]) {
    if (!out || tiles < 1 || members < 1 || members > DECODE3_GMAX || resident < 1 || tb_want < 0 || tb_want > 4 || tb_want == 3) return -1;
    Decode3TilesWanted want{tb_want, span_want != 0};
    if (tb_want == 0) want = capture_group_tiles_wanted(tiles, members, resident);
    const Decode3GroupGeometry geo = decode3_group_geometry(tiles, members, resident, want.tb, want.span);
    out[0] = geo.tb; out[1] = geo.grid_x; out[2] = geo.grid_y; out[3] = geo.span ? 1 : 0;
    return 0;
}

int gemlite_hip_capture_group_last_lines(void) { return capture_group_last_lines(); }

void gemlite_hip_capture_group_merge_stats(uint64_t* merged) { capture_group_merge_stats(merged); }

int gemlite_hip_capture_group_rounds_max(void) { return capture_group_rounds_max(); }

int gemlite_hip_capture_group_last_rounds(void) { return capture_group_last_rounds(); }

int gemlite_hip_capture_group_round_member(int32_t m, int32_t Y, int32_t block_y, int32_t local_layer) {
    if (m < 1 || m > DECODE3_GMAX || Y < 1 || Y > m || block_y < 0 || local_layer < 0) return -1;
    const int r = block_y / Y, y = block_y % Y;
    if ((int64_t)m * (r + 1) > DECODE3_NODE_MAX || (int64_t)y + (int64_t)local_layer * Y >= m) return -1;
    return decode3_round_member(m, Y, block_y, local_layer);
}

int gemlite_hip_capture_group_last_policy(void) { return capture_group_last_policy(); }

int gemlite_hip_capture_group_policy(int32_t h, int32_t default_policy_loads, uint64_t w_bases_or, uint32_t pitch_bytes, int32_t forced) {
    if ((h != 1 && h != 2 && h != 4) || forced < -2 || forced > 1) return -1;
    return decode3_group_nt(h, default_policy_loads == 0, w_bases_or, pitch_bytes, forced == -2 ? capture_group_policy_forced() : forced) ? 1 : 0;
}

// The K order of the unsplit 8-bit tiles, host only (nothing is launched, no device is touched).  _step evaluates the struct the kernels compile
// (KOrder, gl_async.h: its host spelling); _mode plans like gemlite_hip_kernel_name and reads the order bits the planned kernel will be launched with.
int gemlite_hip_k_order_step(int32_t step, int32_t mt, int32_t mtiles, int32_t nsteps, int32_t mode) {
    if (nsteps < 1 || step < 0 || step >= nsteps || mtiles < 1 || mt < 0 || mt >= mtiles || mode < -1 || mode > 15) return -1;
    async::KOrder k;
    k.init(mt, mtiles, nsteps, mode < 0 ? 0 : (K_ORDER_ON | (mode << K_ORDER_GROUP_SHIFT)));
    return k.at(step);
}

int gemlite_hip_k_order_mode(const gemlite_hip_forward_args* args) {
    if (validate(args) != GEMLITE_OK) return -1;
    Resolved r;
    resolve(*args, r);
    if (r.status != GEMLITE_OK || !r.lp.name) return -1;
    const char* n = r.lp.name;
    const size_t len = strlen(n);
    const bool narrow = len > 7 && strcmp(n + len - 7, "<64x64>") == 0;
    if (r.kind == K_A8_MMA && (strncmp(n, "gemm_a8w8_sq_kernel<", 20) == 0 || (strncmp(n, "gemm_mx_a", 9) == 0 && strstr(n, "_sq_kernel<")))) {
        const int bm = strstr(n, "<128x128>") ? 128 : 64;
        if (!(r.gp.flags & K_ORDER_ON) || (args->M + bm - 1) / bm < 2) return -1;
        return (r.gp.flags >> K_ORDER_GROUP_SHIFT) & 15;
    }
    // the narrow 64 x 64 tiles of gemm_wn_mma_kernel: their own whole-K rotation, the group field is ignored
    if (r.kind == K_TILED_WN && narrow && (r.wn.flags & K_ORDER_ON) && (args->M + 63) / 64 >= 2) return 0;
    return -1;
}

int gemlite_hip_capture_group_lines(int32_t tiles, int32_t members, int32_t resident, int32_t tb, int32_t h_want) {
    if (tiles < 1 || members < 1 || members > DECODE3_GMAX || resident < 1 || (tb != 1 && tb != 2 && tb != 4) || tiles % tb || h_want < 0 ||
        h_want > 4 || h_want == 3)
        return -1;
    return decode3_group_lines(tb, h_want == 0 ? capture_group_lines_wanted(tiles, members, resident, tb) : h_want);
}

int gemlite_hip_capture_group_tile_of(int32_t tiles, int32_t tb, int32_t span, int32_t block) {
    if (tiles < 1 || (tb != 1 && tb != 2 && tb != 4) || tiles % tb || block < 0 || block >= tiles / tb) return -1;
    return decode3_group_first_tile(block, tiles / tb, tb, span != 0, (tiles & 15) == 0);
}

int gemlite_hip_capture_group_form(int32_t members, int32_t same_x, int64_t K) {
    if (members < 1 || members > DECODE3_GMAX || K <= 0 || (K & 255)) return -1;
    return decode3_group_form(members, same_x != 0, K / 256, capture_group_shared_x_enabled());
}

int64_t gemlite_hip_capture_group_shared_x_lds_bytes(int64_t K) {
    return (K > 0 && !(K & 255)) ? decode3_shared_x_lds_bytes(K / 256) : 0;
}

int gemlite_hip_capture_group_compatible(const gemlite_hip_forward_args* a, const gemlite_hip_forward_args* b) {
    if (validate(a) != GEMLITE_OK || validate(b) != GEMLITE_OK) return 0;
    Resolved ra, rb;
    resolve(*a, ra);
    resolve(*b, rb);
    if (ra.status != GEMLITE_OK || rb.status != GEMLITE_OK) return 0;
    return capture_group_compatible(*a, ra.lp, *b, rb.lp) ? 1 : 0;
}

int gemlite_hip_bias_fused(const gemlite_hip_forward_args* args, const gemlite_hip_forward_ext* ext) {
    const int v = validate(args);
    if (v != GEMLITE_OK) return v;
    if (validate_ext(ext) != GEMLITE_OK) return GEMLITE_ERR_BAD_ARGUMENT;
    Resolved r;
    resolve(*args, r);
    if (r.status != GEMLITE_OK) return r.status;
    return apply_bias(*args, ext, r) ? 1 : 0;
}

const char* gemlite_hip_kernel_name_ex(const gemlite_hip_forward_args* args, const gemlite_hip_forward_ext* ext) {
    if (validate(args) != GEMLITE_OK || validate_ext(ext) != GEMLITE_OK) return "invalid";
    Resolved r;
    resolve(*args, r);
    (void)apply_bias(*args, ext, r);
    return r.status == GEMLITE_OK ? r.lp.name : "unsupported";
}

int gemlite_hip_capture_group_compatible_ex(const gemlite_hip_forward_args* a, const gemlite_hip_forward_ext* ea,
                                             const gemlite_hip_forward_args* b, const gemlite_hip_forward_ext* eb) {
    if (validate(a) != GEMLITE_OK || validate(b) != GEMLITE_OK || validate_ext(ea) != GEMLITE_OK || validate_ext(eb) != GEMLITE_OK) return 0;
    Resolved ra, rb;
    resolve(*a, ra);
    resolve(*b, rb);
    if (ra.status != GEMLITE_OK || rb.status != GEMLITE_OK) return 0;
    (void)apply_bias(*a, ea, ra);
    (void)apply_bias(*b, eb, rb);
    return capture_group_compatible(*a, ra.lp, *b, rb.lp) ? 1 : 0;
}

int gemlite_hip_launch_noop(int32_t blocks, int32_t threads, void* stream) {
    if (blocks <= 0 || threads <= 0 || threads > 1024) return GEMLITE_ERR_BAD_ARGUMENT;
    void* none[1] = {nullptr};
    return launch((const void*)gemlite_noop_kernel, dim3((unsigned)blocks, 1, 1), dim3((unsigned)threads, 1, 1), none, 0,
                  (hipStream_t)stream);
}

static int launch_resolved(const gemlite_hip_forward_args* args, Resolved& r, int dev, int resident, hipStream_t st);

int gemlite_hip_forward(const gemlite_hip_forward_args* args, void* stream) { return gemlite_hip_forward_ex(args, nullptr, stream); }

int gemlite_hip_forward_ex(const gemlite_hip_forward_args* args, const gemlite_hip_forward_ext* ext, void* stream) {
    const int v = validate(args);
    if (v != GEMLITE_OK) return v;
    if (validate_ext(ext) != GEMLITE_OK) return GEMLITE_ERR_BAD_ARGUMENT;
    int dev = 0;
    const int dv = check_device(&dev);  // (before planning: the planners ask for the device's CU count)
    Resolved r;
    tl_plan_dev = dv == GEMLITE_OK ? dev : -1;
    resolve(*args, r);
    const int resident = gl::resident_block_limit();  // of the device planned for: a capture-group join sizes its grid.y by it
    tl_plan_dev = -1;
    if (r.status != GEMLITE_OK) return r.status;
    if (dv != GEMLITE_OK) return dv;
    // a bias the launch does not add itself is left to the caller: the launch runs as without it and says so
    const bool bias_left = ext && ext->bias && !apply_bias(*args, ext, r);
    const int rc = launch_resolved(args, r, dev, resident, (hipStream_t)stream);
    return (rc == GEMLITE_OK && bias_left) ? GEMLITE_BIAS_NOT_ADDED : rc;
}

// the tail of a planned launch whose kernel takes ONE parameter struct by value
static int launch_struct(const LaunchPlan& lp, void* params, int dev, hipStream_t st) {
    const int e = ensure_lds(lp.fn, lp.lds_bytes, dev);
    if (e != GEMLITE_OK) return e;
    void* kargs[] = {params};
    return launch(lp.fn, lp.grid, lp.block, kargs, lp.lds_bytes, st);
}

// ... and of one with scalar arguments: the two families of capture_group.hip (decode3, rows), the same two calls around the launch
static int launch_scalars(const gemlite_hip_forward_args& a, const LaunchPlan& lp, void** dargs, size_t lds, int dev, int resident, hipStream_t st) {
    const int e = ensure_lds(lp.fn, lp.lds_bytes, dev);
    if (e != GEMLITE_OK) return e;
    // under stream capture an independent neighbour joins the node of the launch before it (capture_group.hip); a launch with
    // profile events or the timeline probe is always its own
    const bool plain = tl_evt_start || tl_evt_stop;
    if (!plain && capture_group_try_join(a, lp, st, resident, dev)) return GEMLITE_OK;
    const int rc = launch(lp.fn, lp.grid, lp.block, dargs, lds, st);
    if (!plain && rc == GEMLITE_OK) capture_group_note_launch(a, lp, st);
    return rc;
}

static int launch_resolved(const gemlite_hip_forward_args* args, Resolved& r, int dev, int resident, hipStream_t st) {
    if (r.kind == K_GEMV_WN || r.kind == K_STREAM_WN || r.kind == K_TILED_WN) {
        if (r.lp.ws_bytes > 0) {
            if (!args->workspace || args->workspace_bytes < r.lp.ws_bytes) return GEMLITE_ERR_WORKSPACE;
            r.wn.counters = (unsigned*)args->workspace;
            r.wn.slabs = (float*)((char*)args->workspace + COUNTER_BYTES);
        } else if (args->workspace && args->workspace_bytes >= COUNTER_BYTES) {
            r.wn.counters = (unsigned*)args->workspace;  // lets the opt-in timeline probes (GEMLITE_TF_TIMELINE) find a buffer
        }
        if (r.lp.arg_kind == 1) {  // scalar (SGPR-preloaded) arguments: gemv_decode.hip
            Decode3Args& d = r.lp.d3;
            d.counters = r.wn.counters;
            Decode3BiasTail btail{r.lp.bias};  // (the biased form: the bias pointer in the place of `counters`)
            void* dargs[] = {(void*)&d.w, (void*)&d.x, (void*)&d.s, (void*)&d.z, (void*)&d.out, (void*)&d.sw4, (void*)&d.mstride2,
                             (void*)&d.nch_total, (void*)&d.modes, r.lp.bias ? (void*)&btail : (void*)&d.counters};
            return launch_scalars(*args, r.lp, dargs, 0, dev, resident, st);
        }
        if (r.lp.arg_kind == 2) {  // gemm_wn_rows.hip
            Rows5Args& d = r.lp.r5;
            void* dargs[] = {(void*)&d.w, (void*)&d.x, (void*)&d.s, (void*)&d.z, (void*)&d.out, (void*)&d.sw4, (void*)&d.mstride2,
                             (void*)&d.nch_total, (void*)&d.modes, (void*)&d.M, (void*)&d.sxm2, (void*)&d.som, (void*)&r.lp.bias};  // (bias: the biased form only)
            return launch_scalars(*args, r.lp, dargs, r.lp.lds_bytes, dev, resident, st);
        }
        return launch_struct(r.lp, &r.wn, dev, st);
    }
    if (r.kind == K_A8_MMA) {
        if (r.lp.ws_bytes > 0) {
            if (!args->workspace || args->workspace_bytes < r.lp.ws_bytes) return GEMLITE_ERR_WORKSPACE;
            r.gp.counters = (unsigned*)args->workspace;
            r.gp.slabs = (float*)((char*)args->workspace + COUNTER_BYTES);
        }
        return launch_struct(r.lp, &r.gp, dev, st);
    }
    if (r.kind == K_NV_MMA) {  // NVFP4: [tickets | split-K slabs | fp16 expansion of x | per-row output factor]
        if (!args->workspace || args->workspace_bytes < r.lp.ws_bytes) return GEMLITE_ERR_WORKSPACE;
        char* base = (char*)args->workspace;
        uint16_t* x16 = (uint16_t*)(base + COUNTER_BYTES + r.lp.slab_bytes);
        float* post = (float*)((char*)x16 + r.nv_x16_bytes);
        r.wn.counters = (unsigned*)base;
        r.wn.slabs = (float*)(base + COUNTER_BYTES);
        r.wn.x = x16;
        r.wn.epi.scales_x = post;
        const uint8_t* xq = (const uint8_t*)args->x;
        const uint8_t* sx = (const uint8_t*)args->scales_x;
        int M = (int)args->M, K = (int)args->K;
        int64_t sxm = args->stride_xm, ssm = args->stride_sx_m;
        float post_v = r.gp.mx_post;
        void* eargs[] = {(void*)&xq, (void*)&sx, (void*)&x16, (void*)&post, (void*)&M, (void*)&K, (void*)&sxm, (void*)&ssm, (void*)&post_v};
        const int64_t nblk = ((int64_t)M * (K / 16) + 255) / 256;
        void* es = tl_evt_start; void* ee = tl_evt_stop;  // (profile events, if any, bracket BOTH launches)
        tl_evt_stop = nullptr;
        int rc = launch(nvfp4_expand_f16_kernel_fn(), dim3((unsigned)nblk, 1, 1), dim3(256, 1, 1), eargs, 0, st);
        if (rc != GEMLITE_OK) return rc;
        (void)es;
        tl_evt_start = nullptr; tl_evt_stop = ee;
        return launch_struct(r.lp, &r.wn, dev, st);
    }
    if (r.kind == K_A8_FQ) {  // cooperative activation quantisation: the workspace holds the flags, the quantised rows and their scales
        if (!args->workspace || args->workspace_bytes < r.lp.ws_bytes) return GEMLITE_ERR_WORKSPACE;
        char* payload = (char*)args->workspace + COUNTER_BYTES;
        r.gp.counters = (unsigned*)args->workspace;
        r.gp.x = payload;
        r.gp.epi.scales_x = (const float*)(payload + cq::xq_bytes(args->M, args->K));
        return launch_struct(r.lp, &r.gp, dev, st);
    }
    return launch_struct(r.lp, &r.gp, dev, st);  // (round 6: w8_rows_lds_kernel stages x in up to 128 KB)
}

// ---- experts: n_slots M = 1 GEMVs in one launch, the expert of each read on the GPU (gemv_decode.hip: gemv_w4_decode3_experts_kernel) ----
// Not a planned launch: resolve(), the planners and capture_group.hip never see it.  The 14 scalars are derived here exactly as
// plan_gemv_wn derives them for the single-layer kernel (Decode3Args), from expert 0's layer; the domain is checked in full first.
struct ExpertsLaunch {
    Decode3Args d3;
    ExpertsTail tail;
    const void* fn;
    dim3 grid;
};

static int experts_plan(const gemlite_hip_experts_args* e, ExpertsLaunch& L) {
    if (!e || e->struct_size != sizeof(gemlite_hip_experts_args)) return GEMLITE_ERR_BAD_ARGUMENT;
    const gemlite_hip_forward_args& a = e->layer;
    const int v = validate(&a);
    if (v != GEMLITE_OK) return v;
    if (!e->ids || e->n_slots <= 0 || e->n_experts <= 0 || e->slots_per_x_row <= 0) return GEMLITE_ERR_BAD_ARGUMENT;
    if (e->ids_dtype != GEMLITE_DT_INT32 && e->ids_dtype != GEMLITE_DT_INT64) return GEMLITE_ERR_UNSUPPORTED;
    const bool f16 = a.input_dtype == GEMLITE_DT_FP16;
    if ((!f16 && a.input_dtype != GEMLITE_DT_BF16) || a.output_dtype != a.input_dtype) return GEMLITE_ERR_UNSUPPORTED;
    if (a.W_nbits != 4 || a.elements_per_sample != 8 || a.w_pack_bits != 32) return GEMLITE_ERR_UNSUPPORTED;
    if (a.channel_scale_mode != 0 || a.W_group_mode < 1) return GEMLITE_ERR_UNSUPPORTED;
    const bool need_s = a.W_group_mode >= 2, has_z = a.W_group_mode == 1 || a.W_group_mode >= 3;
    const bool z_scalar = has_z && a.zero_is_scalar != 0, need_z = has_z && !z_scalar;
    if ((need_s && a.meta_dtype != a.input_dtype) || (need_z && a.zeros_dtype != a.input_dtype) || (z_scalar && a.zeros_dtype != GEMLITE_DT_INT32))
        return GEMLITE_ERR_UNSUPPORTED;
    if (a.stride_xk != 1 || a.stride_wn != 1 || a.stride_on != 1 || ((need_s || need_z) && a.stride_meta_n != 1)) return GEMLITE_ERR_UNSUPPORTED;
    const int64_t gs = a.group_size;
    if (a.M != 1 || a.N % 16 != 0 || a.K % 256 != 0 || gs < 32 || (gs & (gs - 1)) != 0 || a.K % gs != 0) return GEMLITE_ERR_BAD_SHAPE;
    if (e->n_slots > 65535 || e->n_experts > 0x7FFFFFFF) return GEMLITE_ERR_BAD_SHAPE;
    // every base a slot can produce keeps the alignment of the kernel's loads: 16-byte weights and x rows, 8-byte metadata, 2-byte bias
    const bool per_group = (need_s || need_z) && gs < a.K;  // (one K-long group: the row stride is never used)
    if (e->stride_expert_w < 0 || e->stride_expert_meta < 0 || e->stride_expert_bias < 0 || e->stride_x_row < 0 || e->stride_out_slot < 0 ||
        a.stride_wk <= 0 || (per_group && a.stride_meta_g <= 0))
        return GEMLITE_ERR_BAD_ARGUMENT;
    if (((uintptr_t)a.w_q % 16) != 0 || (a.stride_wk % 4) != 0 || (e->stride_expert_w % 16) != 0) return GEMLITE_ERR_BAD_ARGUMENT;
    if (((uintptr_t)a.x % 16) != 0 || (e->stride_x_row % 8) != 0) return GEMLITE_ERR_BAD_ARGUMENT;
    if ((need_s && ((uintptr_t)a.scales % 8) != 0) || (need_z && ((uintptr_t)a.zeros % 8) != 0) || (z_scalar && ((uintptr_t)a.zeros % 4) != 0) ||
        (per_group && (a.stride_meta_g % 4) != 0) || ((need_s || need_z) && (e->stride_expert_meta % 8) != 0))
        return GEMLITE_ERR_BAD_ARGUMENT;
    if (((uintptr_t)a.out % 2) != 0 || (e->bias && (((uintptr_t)e->bias % 2) != 0 || (e->stride_expert_bias % 2) != 0))) return GEMLITE_ERR_BAD_ARGUMENT;
    // 32-bit byte offsets inside one expert, as the single-layer kernel has them
    const int64_t rows = a.K / 8, meta_g = per_group ? a.stride_meta_g : 0;
    if (rows * a.stride_wk * 4 >= (1ll << 32) || (a.K / gs) * meta_g * 2 + a.N * 2 >= (1ll << 32) || rows * 16 >= (1ll << 31)) return GEMLITE_ERR_BAD_SHAPE;

    const int64_t tiles = a.N / 16;
    const uint32_t gs_shift = per_group ? (uint32_t)__builtin_ctzll((unsigned long long)gs) : 31u;
    L.d3.w = (const char*)a.w_q;
    L.d3.x = (const char*)a.x;
    L.d3.s = need_s ? (const char*)a.scales : (const char*)a.w_q;
    L.d3.z = has_z ? (const char*)a.zeros : (const char*)a.w_q;
    L.d3.out = (uint16_t*)a.out;
    L.d3.sw4 = (uint32_t)a.stride_wk * 4u;
    L.d3.mstride2 = (uint32_t)meta_g * 2u;
    L.d3.nch_total = (int)(rows / 32);
    L.d3.modes = (uint32_t)a.W_group_mode | (z_scalar ? 16u : 0u) | (((tiles & 15) == 0) ? 32u : 0u) | (gs_shift << 8);
    L.d3.counters = nullptr;
    L.tail.ids = e->ids;
    L.tail.bias = (const uint16_t*)e->bias;
    L.tail.stride_w = e->stride_expert_w;
    L.tail.stride_meta = e->stride_expert_meta;
    L.tail.stride_bias = e->stride_expert_bias;
    L.tail.stride_x = e->stride_x_row * 2;
    L.tail.stride_out = e->stride_out_slot;
    L.tail.n_experts = (uint32_t)e->n_experts;
    L.tail.slots_per_x_row = (uint32_t)(e->slots_per_x_row > 65536 ? 65536 : e->slots_per_x_row);  // (slot < 65535: row 0 either way)
    L.fn = gemv_w4_decode3_experts_fn(f16 ? 0 : 1, e->bias != nullptr, e->ids_dtype == GEMLITE_DT_INT64);
    L.grid = dim3((unsigned)tiles, (unsigned)e->n_slots, 1);
    return GEMLITE_OK;
}

int gemlite_hip_experts_query(const gemlite_hip_experts_args* args) {
    ExpertsLaunch L;
    return experts_plan(args, L);
}

int gemlite_hip_forward_experts(const gemlite_hip_experts_args* args, void* stream) {
    ExpertsLaunch L;
    const int v = experts_plan(args, L);
    if (v != GEMLITE_OK) return v;
    int dev = 0;
    const int dv = check_device(&dev);
    if (dv != GEMLITE_OK) return dv;
    Decode3Args& d = L.d3;
    void* kargs[] = {(void*)&d.w, (void*)&d.x, (void*)&d.s, (void*)&d.z, (void*)&d.out, (void*)&d.sw4, (void*)&d.mstride2,
                     (void*)&d.nch_total, (void*)&d.modes, (void*)&L.tail};
    return launch(L.fn, L.grid, dim3(1024, 1, 1), kargs, 0, (hipStream_t)stream);
}

// ---- experts with a fused epilogue (gemv_decode.hip: gemv_w4_decode3_experts_fused_kernel): the nested request by experts_plan's rules,
// unchanged, then the epilogue's own.  GLU: grid (I / 16, slots), a block holds a slot's gate tile and up tile; COMBINE: grid (N / 16,
// tokens), a block holds one tile of a token's slots_per_token slots.
struct ExpertsFusedLaunch {
    ExpertsLaunch base;
    ExpertsFusedTail tail;
    const void* fn;
    dim3 grid;
};

static int experts_fused_plan(const gemlite_hip_experts_fused_args* f, ExpertsFusedLaunch& L) {
    if (!f || f->struct_size != sizeof(gemlite_hip_experts_fused_args)) return GEMLITE_ERR_BAD_ARGUMENT;
    const int v = experts_plan(&f->experts, L.base);
    if (v != GEMLITE_OK) return v;
    const gemlite_hip_experts_args& e = f->experts;
    const int64_t tiles = e.layer.N / 16;
    L.tail.e = L.base.tail;
    L.tail.weights = nullptr;
    L.tail.members = 2;
    L.tail.half_tiles = 0;
    L.tail.w_f32 = 0;
    uint32_t modes = L.base.d3.modes & ~32u;  // (the tile pairing is decided on the tiles of THIS grid)
    if (f->epilogue == GEMLITE_EXPERTS_GLU) {
        if (f->activation != GEMLITE_ACT_SILU) return GEMLITE_ERR_UNSUPPORTED;
        if (e.layer.N % 32 != 0) return GEMLITE_ERR_BAD_SHAPE;
        const int64_t half = tiles / 2;
        L.tail.half_tiles = (uint32_t)half;
        if ((half & 15) == 0) modes |= 32u;
        L.grid = dim3((unsigned)half, (unsigned)e.n_slots, 1);
    } else if (f->epilogue == GEMLITE_EXPERTS_COMBINE) {
        const bool w32 = f->weights_dtype == GEMLITE_DT_FP32;
        if (!w32 && f->weights_dtype != e.layer.output_dtype) return GEMLITE_ERR_UNSUPPORTED;
        if (!f->weights || ((uintptr_t)f->weights % (w32 ? 4 : 2)) != 0 || f->slots_per_token <= 0) return GEMLITE_ERR_BAD_ARGUMENT;
        if (f->slots_per_token > DECODE3_GMAX || e.n_slots % f->slots_per_token != 0) return GEMLITE_ERR_BAD_SHAPE;
        L.tail.weights = f->weights;
        L.tail.members = (uint32_t)f->slots_per_token;
        L.tail.w_f32 = w32 ? 1u : 0u;
        if ((tiles & 15) == 0) modes |= 32u;
        L.grid = dim3((unsigned)tiles, (unsigned)(e.n_slots / f->slots_per_token), 1);
    } else {
        return GEMLITE_ERR_UNSUPPORTED;
    }
    L.base.d3.modes = modes;
    L.fn = gemv_w4_decode3_experts_fused_fn(e.layer.input_dtype == GEMLITE_DT_FP16 ? 0 : 1, f->epilogue, e.bias != nullptr, e.ids_dtype == GEMLITE_DT_INT64);
    return GEMLITE_OK;
}

int gemlite_hip_experts_fused_query(const gemlite_hip_experts_fused_args* args) {
    ExpertsFusedLaunch L;
    return experts_fused_plan(args, L);
}

int gemlite_hip_forward_experts_fused(const gemlite_hip_experts_fused_args* args, void* stream) {
    ExpertsFusedLaunch L;
    const int v = experts_fused_plan(args, L);
    if (v != GEMLITE_OK) return v;
    int dev = 0;
    const int dv = check_device(&dev);
    if (dv != GEMLITE_OK) return dv;
    Decode3Args& d = L.base.d3;
    void* kargs[] = {(void*)&d.w, (void*)&d.x, (void*)&d.s, (void*)&d.z, (void*)&d.out, (void*)&d.sw4, (void*)&d.mstride2,
                     (void*)&d.nch_total, (void*)&d.modes, (void*)&L.tail};
    return launch(L.fn, L.grid, dim3(1024, 1, 1), kargs, 0, (hipStream_t)stream);
}

// ---- experts on a batch (gemm_wn_rows_experts.hip: gemm_w4_rows_experts_kernel; experts_route.hip: experts_route_kernel): the nested
// request by experts_plan's rules, unchanged, then the rows kernel's own (plan_gemm_wn_rows), then the workspace.  Two launches: the route
// writes the work table, the rows launch — grid (N / 16, Bmax) — consumes it; neither reads anything on the host.
struct ExpertsRowsLaunch {
    ExpertsLaunch base;
    ExpertsRowsTail tail;
    const void *fn, *route_fn;
    dim3 grid;
    int R;
    uint32_t sxm2, som;
};

static bool experts_rows_r_ok(int64_t r) { return r == 16 || r == 32 || r == 48 || r == 64; }

uint64_t gemlite_hip_experts_rows_workspace_bytes(int64_t n_slots, int64_t n_experts, int32_t rows_per_block) {
    if (n_slots <= 0 || n_slots > 65535 || n_experts <= 0 || n_experts > GEMLITE_EXPERTS_ROWS_MAX_EXPERTS || !experts_rows_r_ok(rows_per_block)) return 0;
    const int64_t bmax = experts_rows_bmax(n_slots, n_experts, rows_per_block);
    return (uint64_t)(EXPERTS_ROWS_HEADER + bmax + bmax * rows_per_block) * 4u;
}

// Default R: the smallest block that holds the mean slot count per expert, n_slots / min(E, n_slots), PLUS A QUARTER; capped by the
// registers of the group size (groups of 32: 32 rows).  The first rule was the mean itself; profiles/r23/probe_experts_rows*.log replaced
// it: a work block of 32 / 64 rows costs 1.2 / 1.6 blocks of 16 (4096^2, 16 blocks: 101.7 / 121.1 / 162.8 us), a second block of the same
// expert costs a whole one, and under random routing about half the experts lie above the mean — at a mean of exactly 16 (Mixtral, 64
// tokens) R = 16 needed 13 / 12 blocks for 8 experts and ran 277.7 / 170.6 us (gate/up / down) against 218.4 / 151.4 with R = 32.  Far
// below 16 slots per expert (Qwen3-30B-A3B up to 128 tokens) R = 16 stays 1.2 x ahead of 32.
static int experts_rows_default_r(int64_t n_slots, int64_t n_experts, int cap) {
    const int64_t mean = n_slots / (n_experts < n_slots ? n_experts : n_slots), want = mean + mean / 4;
    const int r = want <= 16 ? 16 : (want <= 32 ? 32 : (want <= 48 ? 48 : 64));
    return r < cap ? r : cap;
}

static int experts_rows_plan(const gemlite_hip_experts_rows_args* r, ExpertsRowsLaunch& L, bool with_workspace) {
    if (!r || r->struct_size != sizeof(gemlite_hip_experts_rows_args)) return GEMLITE_ERR_BAD_ARGUMENT;
    const int v = experts_plan(&r->experts, L.base);
    if (v != GEMLITE_OK) return v;
    const gemlite_hip_experts_args& e = r->experts;
    const gemlite_hip_forward_args& a = e.layer;
    // the rows kernel's own rules (plan_gemm_wn_rows): packed pairs of outputs, 32-bit offsets inside an expert, an x extent below 2^31
    // (the 0x80000000 offset of an empty row must lie beyond the descriptor of ALL of x)
    if (((uintptr_t)a.out % 4) != 0 || (e.stride_out_slot % 2) != 0) return GEMLITE_ERR_BAD_ARGUMENT;
    if (e.n_experts > GEMLITE_EXPERTS_ROWS_MAX_EXPERTS) return GEMLITE_ERR_BAD_SHAPE;
    const Decode3Args& d = L.base.d3;
    const int64_t rows = a.K / 8, x_rows = (e.n_slots + e.slots_per_x_row - 1) / e.slots_per_x_row;
    const int64_t x_bytes = (x_rows - 1) * e.stride_x_row * 2 + a.K * 2;
    if (rows * a.stride_wk * 4 + a.N * 4 >= (1ll << 32) || x_bytes >= (1ll << 31) || e.stride_out_slot >= (1ll << 31)) return GEMLITE_ERR_BAD_SHAPE;
    const uint32_t gs_shift = (d.modes >> 8) & 255u;
    if (gs_shift < 31 && ((a.K >> gs_shift) * (int64_t)(d.mstride2 / 2) + a.N) * 2 >= (1ll << 32)) return GEMLITE_ERR_BAD_SHAPE;
    const int spg = gs_shift >= 7 ? 4 : (gs_shift == 6 ? 2 : 1), cap = spg == 1 ? 32 : 64;
    if (r->rows_per_block != 0 && !experts_rows_r_ok(r->rows_per_block)) return GEMLITE_ERR_BAD_ARGUMENT;
    if (r->rows_per_block > cap) return GEMLITE_ERR_BAD_SHAPE;  // (groups of 32: the 48- / 64-row forms need more than 256 registers)
    L.R = r->rows_per_block ? r->rows_per_block : experts_rows_default_r(e.n_slots, e.n_experts, cap);
    const int64_t bmax = experts_rows_bmax(e.n_slots, e.n_experts, L.R);
    if (with_workspace) {
        if (!r->workspace || ((uintptr_t)r->workspace % 4) != 0 ||
            r->workspace_bytes < gemlite_hip_experts_rows_workspace_bytes(e.n_slots, e.n_experts, L.R))
            return GEMLITE_ERR_WORKSPACE;
    }
    const bool f16 = a.input_dtype == GEMLITE_DT_FP16;
    L.fn = gemm_wn_rows_experts_fn(f16 ? 0 : 1, L.R / 16, spg, e.bias != nullptr);
    if (!L.fn) return GEMLITE_ERR_UNSUPPORTED;
    L.route_fn = experts_route_fn(e.ids_dtype == GEMLITE_DT_INT64);
    L.tail.table = (const int32_t*)r->workspace;
    L.tail.bias = (const uint16_t*)e.bias;
    L.tail.stride_w = e.stride_expert_w;
    L.tail.stride_meta = e.stride_expert_meta;
    L.tail.stride_bias = e.stride_expert_bias;
    L.tail.n_experts = (uint32_t)e.n_experts;
    L.tail.slots_per_x_row = L.base.tail.slots_per_x_row;
    L.tail.n_slots = (uint32_t)e.n_slots;
    L.tail.x_bytes = (uint32_t)x_bytes;
    L.sxm2 = (uint32_t)(e.stride_x_row * 2);
    L.som = (uint32_t)e.stride_out_slot;
    L.grid = dim3((unsigned)(a.N / 16), (unsigned)bmax, 1);
    return GEMLITE_OK;
}

int gemlite_hip_experts_rows_query(const gemlite_hip_experts_rows_args* args) {
    ExpertsRowsLaunch L;
    return experts_rows_plan(args, L, true);
}

int gemlite_hip_experts_rows_per_block(const gemlite_hip_experts_rows_args* args) {
    ExpertsRowsLaunch L;
    const int v = experts_rows_plan(args, L, false);
    return v != GEMLITE_OK ? v : L.R;
}

int gemlite_hip_experts_route(const gemlite_hip_experts_rows_args* args, void* stream) {
    ExpertsRowsLaunch L;
    const int v = experts_rows_plan(args, L, true);
    if (v != GEMLITE_OK) return v;
    int dev = 0;
    const int dv = check_device(&dev);
    if (dv != GEMLITE_OK) return dv;
    const void* ids = args->experts.ids;
    int32_t* table = (int32_t*)args->workspace;
    uint32_t n_slots = (uint32_t)args->experts.n_slots, n_experts = L.tail.n_experts, R = (uint32_t)L.R, bmax = L.grid.y;
    void* kargs[] = {(void*)&ids, (void*)&table, (void*)&n_slots, (void*)&n_experts, (void*)&R, (void*)&bmax};
    return launch(L.route_fn, dim3(1, 1, 1), dim3(1024, 1, 1), kargs, 0, (hipStream_t)stream);
}

int gemlite_hip_forward_experts_rows(const gemlite_hip_experts_rows_args* args, void* stream) {
    ExpertsRowsLaunch L;
    const int v = experts_rows_plan(args, L, true);
    if (v != GEMLITE_OK) return v;
    int dev = 0;
    const int dv = check_device(&dev);
    if (dv != GEMLITE_OK) return dv;
    const size_t lds = gemm_wn_rows_experts_lds_bytes();
    const int le = ensure_lds(L.fn, lds, dev);
    if (le != GEMLITE_OK) return le;
    Decode3Args& d = L.base.d3;
    int M = L.R;
    void* kargs[] = {(void*)&d.w, (void*)&d.x, (void*)&d.s, (void*)&d.z, (void*)&d.out, (void*)&d.sw4, (void*)&d.mstride2,
                     (void*)&d.nch_total, (void*)&d.modes, (void*)&M, (void*)&L.sxm2, (void*)&L.som, (void*)&L.tail};
    return launch(L.fn, L.grid, dim3(64 * 8, 1, 1), kargs, lds, (hipStream_t)stream);
}

// ---- the batched gate/up launch with SwiGLU inside (gemm_wn_rows_experts_glu.hip: gemm_w4_rows_experts_glu_kernel): the nested request by
// experts_rows_plan's rules, unchanged, then the GLU forms' own.  Grid (I / 16, Bmax); the table is the one the route launch wrote.
struct ExpertsRowsGluLaunch {
    ExpertsRowsLaunch base;
    ExpertsRowsGluTail tail;
    const void* fn;
    dim3 grid;
};

static int experts_rows_glu_plan(const gemlite_hip_experts_rows_glu_args* g, ExpertsRowsGluLaunch& L, bool with_workspace) {
    if (!g || g->struct_size != sizeof(gemlite_hip_experts_rows_glu_args)) return GEMLITE_ERR_BAD_ARGUMENT;
    // the nested request first, without its workspace: the table's size depends on R, and the default R on the GLU cap
    const int v = experts_rows_plan(&g->rows, L.base, false);
    if (v != GEMLITE_OK) return v;
    if (g->activation != GEMLITE_ACT_SILU) return GEMLITE_ERR_UNSUPPORTED;
    const gemlite_hip_experts_args& e = g->rows.experts;
    if (e.layer.N % 32 != 0) return GEMLITE_ERR_BAD_SHAPE;
    const uint32_t gs_shift = (L.base.base.d3.modes >> 8) & 255u;
    if (gs_shift < 6) return GEMLITE_ERR_UNSUPPORTED;  // groups of 32: the two-tile body spills
    const int spg = gs_shift >= 7 ? 4 : 2, cap = spg == 4 ? 64 : 32;
    if (g->rows.rows_per_block > cap) return GEMLITE_ERR_BAD_SHAPE;
    gemlite_hip_experts_rows_args rows = g->rows;
    if (!rows.rows_per_block) rows.rows_per_block = experts_rows_default_r(e.n_slots, e.n_experts, cap);
    const int vw = experts_rows_plan(&rows, L.base, with_workspace);  // (again at the resolved R: the workspace rule, the tail)
    if (vw != GEMLITE_OK) return vw;
    L.fn = gemm_wn_rows_experts_glu_fn(e.layer.input_dtype == GEMLITE_DT_FP16 ? 0 : 1, L.base.R / 16, spg, e.bias != nullptr);
    if (!L.fn) return GEMLITE_ERR_UNSUPPORTED;
    L.tail.rows = L.base.tail;
    L.tail.half_tiles = (uint32_t)(e.layer.N / 32);
    L.grid = dim3((unsigned)(e.layer.N / 32), (unsigned)experts_rows_bmax(e.n_slots, e.n_experts, L.base.R), 1);
    return GEMLITE_OK;
}

int gemlite_hip_experts_rows_glu_query(const gemlite_hip_experts_rows_glu_args* args) {
    ExpertsRowsGluLaunch L;
    return experts_rows_glu_plan(args, L, true);
}

int gemlite_hip_experts_rows_glu_per_block(const gemlite_hip_experts_rows_glu_args* args) {
    ExpertsRowsGluLaunch L;
    const int v = experts_rows_glu_plan(args, L, false);
    return v != GEMLITE_OK ? v : L.base.R;
}

int gemlite_hip_forward_experts_rows_glu(const gemlite_hip_experts_rows_glu_args* args, void* stream) {
    ExpertsRowsGluLaunch L;
    const int v = experts_rows_glu_plan(args, L, true);
    if (v != GEMLITE_OK) return v;
    int dev = 0;
    const int dv = check_device(&dev);
    if (dv != GEMLITE_OK) return dv;
    const size_t lds = gemm_wn_rows_experts_lds_bytes();
    const int le = ensure_lds(L.fn, lds, dev);
    if (le != GEMLITE_OK) return le;
    Decode3Args& d = L.base.base.d3;
    int M = L.base.R;
    void* kargs[] = {(void*)&d.w, (void*)&d.x, (void*)&d.s, (void*)&d.z, (void*)&d.out, (void*)&d.sw4, (void*)&d.mstride2,
                     (void*)&d.nch_total, (void*)&d.modes, (void*)&M, (void*)&L.base.sxm2, (void*)&L.base.som, (void*)&L.tail};
    return launch(L.fn, L.grid, dim3(64 * 8, 1, 1), kargs, lds, (hipStream_t)stream);
}

// ---- the routing-weight sum of a batch (experts_combine.hip: experts_combine_kernel): one memory-bound launch, grid (column groups, tokens) ----
struct ExpertsCombineLaunch {
    ExpertsCombineArgs a;
    const void* fn;
    dim3 grid, block;
};

static int experts_combine_plan(const gemlite_hip_experts_combine_args* c, ExpertsCombineLaunch& L) {
    if (!c || c->struct_size != sizeof(gemlite_hip_experts_combine_args)) return GEMLITE_ERR_BAD_ARGUMENT;
    if (!c->y || !c->ids || !c->weights || !c->out) return GEMLITE_ERR_BAD_ARGUMENT;
    if (c->n_slots <= 0 || c->n_experts <= 0 || c->slots_per_token <= 0 || c->N <= 0) return GEMLITE_ERR_BAD_ARGUMENT;
    const bool f16 = c->dtype == GEMLITE_DT_FP16, ids64 = c->ids_dtype == GEMLITE_DT_INT64, w32 = c->weights_dtype == GEMLITE_DT_FP32;
    if (!f16 && c->dtype != GEMLITE_DT_BF16) return GEMLITE_ERR_UNSUPPORTED;
    if (!ids64 && c->ids_dtype != GEMLITE_DT_INT32) return GEMLITE_ERR_UNSUPPORTED;
    if (!w32 && c->weights_dtype != c->dtype) return GEMLITE_ERR_UNSUPPORTED;
    if (((uintptr_t)c->y % 4) != 0 || ((uintptr_t)c->out % 4) != 0 || ((uintptr_t)c->ids % (ids64 ? 8 : 4)) != 0 ||
        ((uintptr_t)c->weights % (w32 ? 4 : 2)) != 0)
        return GEMLITE_ERR_BAD_ARGUMENT;
    if (c->stride_y_slot < 0 || c->stride_out_token < 0 || (c->stride_y_slot % 2) != 0 || (c->stride_out_token % 2) != 0) return GEMLITE_ERR_BAD_ARGUMENT;
    if (c->N % 16 != 0 || c->slots_per_token > GEMLITE_EXPERTS_COMBINE_MAX_SLOTS_PER_TOKEN || c->n_slots % c->slots_per_token != 0 ||
        c->n_slots > 65535 || c->n_experts > 0x7FFFFFFF)
        return GEMLITE_ERR_BAD_SHAPE;
    const int64_t tokens = c->n_slots / c->slots_per_token;
    if (c->N >= (1ll << 31) || c->stride_y_slot >= (1ll << 31) || c->stride_out_token >= (1ll << 31) ||
        (c->n_slots - 1) * c->stride_y_slot + c->N >= (1ll << 31) || (tokens - 1) * c->stride_out_token + c->N >= (1ll << 31))
        return GEMLITE_ERR_BAD_SHAPE;
    const bool wide = ((uintptr_t)c->y % 16) == 0 && ((uintptr_t)c->out % 16) == 0 && (c->stride_y_slot % 8) == 0 && (c->stride_out_token % 8) == 0;
    L.a.y = (const uint16_t*)c->y;
    L.a.ids = c->ids;
    L.a.weights = c->weights;
    L.a.out = (uint16_t*)c->out;
    L.a.n_experts = (uint32_t)c->n_experts;
    L.a.spt = (uint32_t)c->slots_per_token;
    L.a.N = (uint32_t)c->N;
    L.a.stride_y = (uint32_t)c->stride_y_slot;
    L.a.stride_out = (uint32_t)c->stride_out_token;
    L.fn = experts_combine_fn(f16 ? 0 : 1, ids64, w32, wide);
    const int64_t threads = experts_combine_threads(), per_block = threads * (wide ? 8 : 2);
    L.block = dim3((unsigned)threads, 1, 1);
    L.grid = dim3((unsigned)((c->N + per_block - 1) / per_block), (unsigned)tokens, 1);
    return GEMLITE_OK;
}

int gemlite_hip_experts_combine_query(const gemlite_hip_experts_combine_args* args) {
    ExpertsCombineLaunch L;
    return experts_combine_plan(args, L);
}

int gemlite_hip_experts_combine(const gemlite_hip_experts_combine_args* args, void* stream) {
    ExpertsCombineLaunch L;
    const int v = experts_combine_plan(args, L);
    if (v != GEMLITE_OK) return v;
    int dev = 0;
    const int dv = check_device(&dev);
    if (dv != GEMLITE_OK) return dv;
    void* kargs[] = {(void*)&L.a};
    return launch(L.fn, L.grid, L.block, kargs, 0, (hipStream_t)stream);
}

// ---- the router's top-k (experts_topk.hip: experts_topk_kernel): one wave per token, four tokens per block ----
struct ExpertsTopkLaunch {
    ExpertsTopkArgs a;
    const void* fn;
    dim3 grid, block;
};

static int experts_topk_plan(const gemlite_hip_experts_topk_args* t, ExpertsTopkLaunch& L) {
    if (!t || t->struct_size != sizeof(gemlite_hip_experts_topk_args)) return GEMLITE_ERR_BAD_ARGUMENT;
    if (!t->logits || !t->ids || !t->weights) return GEMLITE_ERR_BAD_ARGUMENT;
    if (t->n_tokens <= 0 || t->n_experts <= 0 || t->top_k <= 0) return GEMLITE_ERR_BAD_ARGUMENT;
    if (t->renormalize != 0 && t->renormalize != 1) return GEMLITE_ERR_BAD_ARGUMENT;
    const int ldt = t->logits_dtype == GEMLITE_DT_FP16 ? 0 : t->logits_dtype == GEMLITE_DT_BF16 ? 1 : t->logits_dtype == GEMLITE_DT_FP32 ? 2 : -1;
    const int wdt = t->weights_dtype == GEMLITE_DT_FP16 ? 0 : t->weights_dtype == GEMLITE_DT_BF16 ? 1 : t->weights_dtype == GEMLITE_DT_FP32 ? 2 : -1;
    const bool ids64 = t->ids_dtype == GEMLITE_DT_INT64;
    if (ldt < 0 || wdt < 0 || (!ids64 && t->ids_dtype != GEMLITE_DT_INT32)) return GEMLITE_ERR_UNSUPPORTED;
    if (t->scoring != GEMLITE_EXPERTS_TOPK_SOFTMAX && t->scoring != GEMLITE_EXPERTS_TOPK_SIGMOID) return GEMLITE_ERR_UNSUPPORTED;
    if (t->bias && t->scoring != GEMLITE_EXPERTS_TOPK_SIGMOID) return GEMLITE_ERR_UNSUPPORTED;
    if (((uintptr_t)t->logits % (ldt == 2 ? 4 : 2)) != 0 || ((uintptr_t)t->ids % (ids64 ? 8 : 4)) != 0 ||
        ((uintptr_t)t->weights % (wdt == 2 ? 4 : 2)) != 0 || ((uintptr_t)t->bias % 4) != 0)
        return GEMLITE_ERR_BAD_ARGUMENT;
    const int64_t k_max = t->n_experts < GEMLITE_EXPERTS_COMBINE_MAX_SLOTS_PER_TOKEN ? t->n_experts : GEMLITE_EXPERTS_COMBINE_MAX_SLOTS_PER_TOKEN;
    if (t->n_experts > GEMLITE_EXPERTS_TOPK_MAX_EXPERTS || t->top_k > k_max || t->stride_logits_token < t->n_experts) return GEMLITE_ERR_BAD_SHAPE;
    if (t->n_tokens > 0xFFFFFFFFll / t->top_k) return GEMLITE_ERR_BAD_SHAPE;             // n_tokens top_k < 2^32
    if (t->stride_logits_token > (1ll << 62) / t->n_tokens) return GEMLITE_ERR_BAD_SHAPE;  // (byte offsets stay in 64 bits)
    L.a.logits = t->logits;
    L.a.bias = (const float*)t->bias;
    L.a.ids = t->ids;
    L.a.weights = t->weights;
    L.a.stride = t->stride_logits_token;
    L.a.n_tokens = (uint32_t)t->n_tokens;
    L.a.E = (uint32_t)t->n_experts;
    L.a.top_k = (uint32_t)t->top_k;
    L.a.sigmoid = t->scoring == GEMLITE_EXPERTS_TOPK_SIGMOID;
    L.a.renorm = (uint32_t)t->renormalize;
    L.a.ids64 = ids64;
    L.a.w_dt = (uint32_t)wdt;
    L.a.scale = t->scale;
    int per = 1;
    while (64 * per < t->n_experts) per *= 2;
    L.fn = experts_topk_fn(ldt, per);
    if (!L.fn) return GEMLITE_ERR_UNSUPPORTED;
    const int64_t threads = experts_topk_threads(), waves = threads / 64;
    L.block = dim3((unsigned)threads, 1, 1);
    L.grid = dim3((unsigned)((t->n_tokens + waves - 1) / waves), 1, 1);
    return GEMLITE_OK;
}

int gemlite_hip_experts_topk_query(const gemlite_hip_experts_topk_args* args) {
    ExpertsTopkLaunch L;
    return experts_topk_plan(args, L);
}

int gemlite_hip_experts_topk(const gemlite_hip_experts_topk_args* args, void* stream) {
    ExpertsTopkLaunch L;
    const int v = experts_topk_plan(args, L);
    if (v != GEMLITE_OK) return v;
    int dev = 0;
    const int dv = check_device(&dev);
    if (dv != GEMLITE_OK) return dv;
    void* kargs[] = {(void*)&L.a};
    return launch(L.fn, L.grid, L.block, kargs, 0, (hipStream_t)stream);
}

int gemlite_hip_scale_activations_per_token(const void* x, void* y, float* scales, int64_t M, int64_t K,
                                            int64_t stride_xm, int32_t in_dtype, int32_t out_dtype, void* stream) {
    if (!x || !y || !scales || M <= 0 || K <= 0) return GEMLITE_ERR_BAD_ARGUMENT;
    if (!(in_dtype == GEMLITE_DT_FP16 || in_dtype == GEMLITE_DT_BF16 || in_dtype == GEMLITE_DT_FP32)) return GEMLITE_ERR_UNSUPPORTED;
    if (!(out_dtype == GEMLITE_DT_INT8 || out_dtype == GEMLITE_DT_FP8E4 || out_dtype == GEMLITE_DT_FP8E5)) return GEMLITE_ERR_UNSUPPORTED;
    if (M > 0x7FFFFFFF) return GEMLITE_ERR_BAD_SHAPE;
    int in_dt = in_dtype, out_dt = out_dtype;
    if (const void* vec = act_quant_vec_kernel_fn(in_dt, out_dt, K, stride_xm, x, y)) {  // row in registers: one memory round trip
        int k32 = (int)K;
        void* vargs[] = {(void*)&x, (void*)&y, (void*)&scales, (void*)&k32, (void*)&stride_xm};
        return launch(vec, dim3((unsigned)M, 1, 1), dim3(256, 1, 1), vargs, 0, (hipStream_t)stream);
    }
    void* kargs[] = {(void*)&x, (void*)&y, (void*)&scales, (void*)&K, (void*)&stride_xm, (void*)&in_dt, (void*)&out_dt};
    return launch(act_quant_kernel_fn(), dim3((unsigned)M, 1, 1), dim3(256, 1, 1), kargs, 0, (hipStream_t)stream);
}

static int scale_activations_mx(int mode, const void* x, void* y, uint8_t* scales, int64_t M, int64_t K, int64_t stride_xm,
                                int32_t in_dtype, void* stream) {
    const int64_t G = mode == 2 ? 16 : 32;
    if (!x || !y || !scales || M <= 0 || K <= 0) return GEMLITE_ERR_BAD_ARGUMENT;
    if (!(in_dtype == GEMLITE_DT_FP16 || in_dtype == GEMLITE_DT_BF16 || in_dtype == GEMLITE_DT_FP32)) return GEMLITE_ERR_UNSUPPORTED;
    if (K % 32 != 0) return GEMLITE_ERR_BAD_SHAPE;  // 16-byte output pieces; the formats' own block is 32 (16) k
    if (((uintptr_t)y % 16) != 0) return GEMLITE_ERR_BAD_ARGUMENT;
    int64_t m_pad = (M + G - 1) / G * G;
    const int64_t total = m_pad * (K / G);
    if (total > 0x7FFFFFFFll * 256) return GEMLITE_ERR_BAD_SHAPE;
    int in_dt = in_dtype;
    void* kargs[] = {(void*)&x, (void*)&y, (void*)&scales, (void*)&M, (void*)&m_pad, (void*)&K, (void*)&stride_xm, (void*)&in_dt};
    return launch(act_quant_mx_kernel_fn(mode), dim3((unsigned)((total + 255) / 256), 1, 1), dim3(256, 1, 1), kargs, 0, (hipStream_t)stream);
}

int gemlite_hip_scale_activations_mxfp8(const void* x, void* y, uint8_t* scales, int64_t M, int64_t K, int64_t stride_xm,
                                        int32_t in_dtype, void* stream) {
    return scale_activations_mx(0, x, y, scales, M, K, stride_xm, in_dtype, stream);
}
int gemlite_hip_scale_activations_mxfp4(const void* x, uint8_t* y, uint8_t* scales, int64_t M, int64_t K, int64_t stride_xm,
                                        int32_t in_dtype, void* stream) {
    return scale_activations_mx(1, x, y, scales, M, K, stride_xm, in_dtype, stream);
}
int gemlite_hip_scale_activations_nvfp4(const void* x, uint8_t* y, uint8_t* scales, int64_t M, int64_t K, int64_t stride_xm,
                                        int32_t in_dtype, void* stream) {
    return scale_activations_mx(2, x, y, scales, M, K, stride_xm, in_dtype, stream);
}

static int check_pack(int64_t N, int64_t K, int32_t nbits, int32_t pack_bits) {
    if (N <= 0 || K <= 0) return GEMLITE_ERR_BAD_ARGUMENT;
    if (!(nbits == 1 || nbits == 2 || nbits == 4 || nbits == 8)) return GEMLITE_ERR_UNSUPPORTED;
    if (!(pack_bits == 8 || pack_bits == 16 || pack_bits == 32 || pack_bits == 64) || pack_bits < nbits) return GEMLITE_ERR_UNSUPPORTED;
    if (K % (pack_bits / nbits) != 0) return GEMLITE_ERR_BAD_SHAPE;
    if ((K / (pack_bits / nbits)) * N > 0x7FFFFFFFll * 256) return GEMLITE_ERR_BAD_SHAPE;
    return GEMLITE_OK;
}

int gemlite_hip_pack_over_cols(const uint8_t* w_q, void* out, int64_t N, int64_t K, int64_t ld_in, int32_t W_nbits,
                               int32_t pack_bits, void* stream) {
    if (!w_q || !out) return GEMLITE_ERR_BAD_ARGUMENT;
    const int c = check_pack(N, K, W_nbits, pack_bits);
    if (c != GEMLITE_OK) return c;
    const int64_t total = (K / (pack_bits / W_nbits)) * N;
    int nb = W_nbits, pb = pack_bits;
    if (pack_bits == 32 && K % (32 / W_nbits) == 0 && (N + 63) / 64 <= 0x7FFFFFFF && (K + 255) / 256 <= 65535) {  // tiled through LDS: coalesced both ways
        void* targs[] = {(void*)&w_q, (void*)&out, (void*)&N, (void*)&K, (void*)&ld_in, (void*)&nb};
        return launch(pack32_kernel_fn(), dim3((unsigned)((N + 63) / 64), (unsigned)((K + 255) / 256), 1), dim3(256, 1, 1), targs, 0, (hipStream_t)stream);
    }
    void* kargs[] = {(void*)&w_q, (void*)&out, (void*)&N, (void*)&K, (void*)&ld_in, (void*)&nb, (void*)&pb};
    return launch(pack_kernel_fn(), dim3((unsigned)((total + 255) / 256), 1, 1), dim3(256, 1, 1), kargs, 0, (hipStream_t)stream);
}

int gemlite_hip_unpack_over_cols(const void* packed, uint8_t* out, int64_t N, int64_t K, int32_t W_nbits,
                                 int32_t pack_bits, void* stream) {
    if (!packed || !out) return GEMLITE_ERR_BAD_ARGUMENT;
    const int c = check_pack(N, K, W_nbits, pack_bits);
    if (c != GEMLITE_OK) return c;
    const int64_t total = (K / (pack_bits / W_nbits)) * N;
    int nb = W_nbits, pb = pack_bits;
    void* kargs[] = {(void*)&packed, (void*)&out, (void*)&N, (void*)&K, (void*)&nb, (void*)&pb};
    return launch(unpack_kernel_fn(), dim3((unsigned)((total + 255) / 256), 1, 1), dim3(256, 1, 1), kargs, 0, (hipStream_t)stream);
}

// everything is checked before the launch (host only: testable without a device).  h: the optimiser's constants (quantize_hqq_kernel), or null
static int quantize_groups_launch(const gemlite_hip_quantize_args* a, const QuantHqqParams* h, void* stream) {
    if (!a || a->struct_size != sizeof(gemlite_hip_quantize_args)) return GEMLITE_ERR_BAD_ARGUMENT;
    if (!a->w || !a->q_out || !a->scales || !a->zeros) return GEMLITE_ERR_BAD_ARGUMENT;
    if (a->N <= 0 || a->K <= 0 || a->group_size <= 0 || a->ld_w < a->K) return GEMLITE_ERR_BAD_ARGUMENT;
    const int nb = a->W_nbits;
    if (!(nb == 1 || nb == 2 || nb == 4 || nb == 8)) return GEMLITE_ERR_UNSUPPORTED;
    if (!(a->pack_bits == 0 || a->pack_bits == 32)) return GEMLITE_ERR_UNSUPPORTED;
    if (!(a->w_dtype == GEMLITE_DT_FP32 || a->w_dtype == GEMLITE_DT_FP16 || a->w_dtype == GEMLITE_DT_BF16)) return GEMLITE_ERR_UNSUPPORTED;
    if (!(a->meta_dtype == GEMLITE_DT_FP16 || a->meta_dtype == GEMLITE_DT_BF16)) return GEMLITE_ERR_UNSUPPORTED;
    if (a->pack_bits == 0 && a->ld_q < a->K) return GEMLITE_ERR_BAD_ARGUMENT;
    const int64_t g = a->group_size;
    if (g % 32 != 0 || a->K % g != 0) return GEMLITE_ERR_BAD_SHAPE;
    if (a->pack_bits == 32 && a->K % (32 / nb) != 0) return GEMLITE_ERR_BAD_SHAPE;
    int64_t gcd = g, t = 256;
    while (t) { const int64_t r = gcd % t; gcd = t; t = r; }
    QuantGroupsParams p;
    p.w = a->w; p.q_out = a->q_out; p.scales = a->scales; p.zeros = a->zeros;
    p.N = a->N; p.K = a->K; p.ld_w = a->ld_w; p.ld_q = a->ld_q;
    p.stride_meta_g = a->stride_meta_g; p.stride_meta_n = a->stride_meta_n;
    p.span = g / gcd * 256;  // lcm(g, 256): whole groups, at most 8 per row
    p.w_dt = a->w_dtype; p.meta_dt = a->meta_dtype; p.nbits = nb; p.group = (int)g;
    p.pack32 = a->pack_bits == 32; p.fold = a->fold_zeros != 0;
    const int64_t gx = (a->N + 63) / 64, gy = (a->K + p.span - 1) / p.span;
    if (gx > 0x7FFFFFFF || gy > 65535) return GEMLITE_ERR_BAD_SHAPE;
    if (h) {
        void* hargs[] = {(void*)&p, (void*)h};
        return launch(quantize_hqq_kernel_fn(p.span == 256), dim3((unsigned)gx, (unsigned)gy, 1), dim3(256, 1, 1), hargs, 0, (hipStream_t)stream);
    }
    void* kargs[] = {(void*)&p};
    return launch(quantize_groups_kernel_fn(p.span == 256), dim3((unsigned)gx, (unsigned)gy, 1), dim3(256, 1, 1), kargs, 0, (hipStream_t)stream);
}

int gemlite_hip_quantize_groups(const gemlite_hip_quantize_args* a, void* stream) { return quantize_groups_launch(a, nullptr, stream); }

int gemlite_hip_quantize_groups_hqq(const gemlite_hip_quantize_hqq_args* a, void* stream) {
    if (!a || a->struct_size != sizeof(gemlite_hip_quantize_hqq_args)) return GEMLITE_ERR_BAD_ARGUMENT;
    if (a->iters < 0 || a->iters > 100) return GEMLITE_ERR_BAD_ARGUMENT;
    const float inf = __builtin_inff();  // (every comparison below is false for NaN)
    if (!(a->lp_norm > 0.f && a->lp_norm <= 1.f) || !(a->beta > 0.f && a->beta < inf) || !(a->kappa > 0.f && a->kappa < inf)) return GEMLITE_ERR_BAD_ARGUMENT;
    const QuantHqqParams h{a->iters, a->lp_norm, a->beta, a->kappa};
    return quantize_groups_launch(&a->q, &h, stream);
}

// everything is checked before the launch (host only: testable without a device)
int gemlite_hip_quantize_mx(const gemlite_hip_quantize_mx_args* a, void* stream) {
    if (!a || a->struct_size != sizeof(gemlite_hip_quantize_mx_args)) return GEMLITE_ERR_BAD_ARGUMENT;
    if (!a->w || !a->q_out || !a->scales) return GEMLITE_ERR_BAD_ARGUMENT;
    if (a->N <= 0 || a->K <= 0 || a->ld_w < a->K) return GEMLITE_ERR_BAD_ARGUMENT;
    if (a->format < 0 || a->format > 2) return GEMLITE_ERR_UNSUPPORTED;
    if (!(a->w_dtype == GEMLITE_DT_FP32 || a->w_dtype == GEMLITE_DT_FP16 || a->w_dtype == GEMLITE_DT_BF16)) return GEMLITE_ERR_UNSUPPORTED;
    if (!(a->pack_nibbles == 0 || a->pack_nibbles == 1) || (a->pack_nibbles == 1 && a->format == 0)) return GEMLITE_ERR_UNSUPPORTED;
    if (a->ld_q < (a->pack_nibbles ? a->K / 2 : a->K)) return GEMLITE_ERR_BAD_ARGUMENT;
    if (a->K % 32 != 0) return GEMLITE_ERR_BAD_SHAPE;
    QuantMxParams p;
    p.w = a->w; p.q_out = (uint8_t*)a->q_out; p.scales = (uint8_t*)a->scales;
    p.N = a->N; p.K = a->K; p.ld_w = a->ld_w; p.ld_q = a->ld_q;
    p.stride_scale_g = a->stride_scale_g; p.stride_scale_n = a->stride_scale_n;
    p.w_dt = a->w_dtype; p.pack = a->pack_nibbles;
    const int64_t gx = (a->N + 63) / 64, gy = (a->K + 255) / 256;
    if (gx > 0x7FFFFFFF || gy > 65535) return GEMLITE_ERR_BAD_SHAPE;
    void* kargs[] = {(void*)&p};
    return launch(quantize_mx_kernel_fn(a->format), dim3((unsigned)gx, (unsigned)gy, 1), dim3(256, 1, 1), kargs, 0, (hipStream_t)stream);
}

// everything is checked before the launch (host only: testable without a device)
int gemlite_hip_quantize_rows(const gemlite_hip_quantize_rows_args* a, void* stream) {
    if (!a || a->struct_size != sizeof(gemlite_hip_quantize_rows_args)) return GEMLITE_ERR_BAD_ARGUMENT;
    if (!a->w || !a->q_out || !a->scales) return GEMLITE_ERR_BAD_ARGUMENT;
    if (a->N <= 0 || a->K <= 0 || a->ld_w < a->K || a->ld_q < a->K || a->stride_s <= 0) return GEMLITE_ERR_BAD_ARGUMENT;
    if (a->format < 0 || a->format > 2 || !(a->scale_rule == 0 || a->scale_rule == 1)) return GEMLITE_ERR_UNSUPPORTED;
    if (!(a->w_dtype == GEMLITE_DT_FP32 || a->w_dtype == GEMLITE_DT_FP16 || a->w_dtype == GEMLITE_DT_BF16)) return GEMLITE_ERR_UNSUPPORTED;
    if (!(a->scale_dtype == GEMLITE_DT_FP32 || a->scale_dtype == GEMLITE_DT_FP16 || a->scale_dtype == GEMLITE_DT_BF16)) return GEMLITE_ERR_UNSUPPORTED;
    if (a->N > 0x7FFFFFFF) return GEMLITE_ERR_BAD_SHAPE;
    QuantRowsParams p;
    p.w = a->w; p.q_out = (uint8_t*)a->q_out; p.scales = a->scales;
    p.N = a->N; p.K = a->K; p.ld_w = a->ld_w; p.ld_q = a->ld_q; p.stride_s = a->stride_s;
    p.w_dt = a->w_dtype; p.scale_dt = a->scale_dtype; p.rule = a->scale_rule;
    const int64_t gx = a->K <= GEMLITE_QUANT_ROWS_WAVE_MAX_K ? (a->N + 3) / 4 : a->N;  // wave form: four rows per block
    void* kargs[] = {(void*)&p};
    return launch(quantize_rows_kernel_fn(a->format, a->K), dim3((unsigned)gx, 1, 1), dim3(256, 1, 1), kargs, 0, (hipStream_t)stream);
}

// everything is checked before the launch (host only: testable without a device)
int gemlite_hip_dequantize(const gemlite_hip_dequantize_args* a, void* stream) {
    if (!a || a->struct_size != sizeof(gemlite_hip_dequantize_args)) return GEMLITE_ERR_BAD_ARGUMENT;
    if (!a->w_q || !a->out) return GEMLITE_ERR_BAD_ARGUMENT;
    if (a->N <= 0 || a->K <= 0 || a->group_size <= 0 || a->elements_per_sample <= 0 || a->ld_out < a->K) return GEMLITE_ERR_BAD_ARGUMENT;
    if (!(a->out_dtype == GEMLITE_DT_FP16 || a->out_dtype == GEMLITE_DT_BF16 || a->out_dtype == GEMLITE_DT_FP32)) return GEMLITE_ERR_UNSUPPORTED;
    const int e = a->elements_per_sample, nb = a->W_nbits;
    DequantParams p{};
    bool grouped = false;
    if (is_mx_input(a->input_dtype)) {
        const bool nv = a->input_dtype == GEMLITE_DT_NVFP4;
        if (!a->scales) return GEMLITE_ERR_BAD_ARGUMENT;
        if (nb == 8) {
            if (nv || a->input_dtype == GEMLITE_DT_MXFP4 || e != 1 || a->w_dtype != GEMLITE_DT_FP8E4) return GEMLITE_ERR_UNSUPPORTED;
            p.fmt = DQ_MXFP8;
        } else if (nb == 4) {
            if (!(e == 1 || (e == 2 && a->w_pack_bits == 8))) return GEMLITE_ERR_UNSUPPORTED;
            p.fmt = nv ? DQ_NVFP4 : DQ_MXFP4;
        } else {
            return GEMLITE_ERR_UNSUPPORTED;
        }
        if (a->group_size != (nv ? 16 : 32)) return GEMLITE_ERR_UNSUPPORTED;
        if (a->K % 32 != 0) return GEMLITE_ERR_BAD_SHAPE;
        p.w_dt = e == 1 && nb == 8 ? GEMLITE_DT_FP8E4 : GEMLITE_DT_UINT8;
        p.pack_bits = e == 2 ? 8 : 0;
        p.group = a->group_size;
    } else {
        if (a->W_group_mode < 0 || a->W_group_mode > 4) return GEMLITE_ERR_UNSUPPORTED;
        if (a->channel_scale_mode < 0 || a->channel_scale_mode > 3) return GEMLITE_ERR_UNSUPPORTED;
        p.w_mode = a->W_group_mode;
        p.chan = a->channel_scale_mode == 1 || a->channel_scale_mode == 3;
        const bool need_s = p.w_mode >= 2 || p.chan, need_z = p.w_mode == 1 || p.w_mode >= 3;
        if ((need_s && !a->scales) || (need_z && !a->zeros)) return GEMLITE_ERR_BAD_ARGUMENT;
        if (e > 1) {
            if (a->w_pack_bits == 64) return GEMLITE_ERR_UNSUPPORTED;
            if (!(nb == 1 || nb == 2 || nb == 4 || nb == 8)) return GEMLITE_ERR_UNSUPPORTED;
            if (!(a->w_pack_bits == 8 || a->w_pack_bits == 16 || a->w_pack_bits == 32) || nb * e != a->w_pack_bits) return GEMLITE_ERR_BAD_ARGUMENT;
        } else {
            const int dt = a->w_dtype;
            if (!(dt == GEMLITE_DT_INT8 || dt == GEMLITE_DT_UINT8 || dt == GEMLITE_DT_FP8E4 || dt == GEMLITE_DT_FP8E5 || dt == GEMLITE_DT_FP16 ||
                  dt == GEMLITE_DT_BF16 || dt == GEMLITE_DT_FP32))
                return GEMLITE_ERR_UNSUPPORTED;  // (the *NUZ fp8 types are the MI300X formats)
        }
        const auto meta_ok = [](int dt) { return dt == GEMLITE_DT_FP16 || dt == GEMLITE_DT_BF16 || dt == GEMLITE_DT_FP32; };
        if (need_s && !meta_ok(a->meta_dtype)) return GEMLITE_ERR_UNSUPPORTED;
        if (need_z && !(a->zero_is_scalar ? (a->zeros_dtype == GEMLITE_DT_INT32 || meta_ok(a->zeros_dtype)) : meta_ok(a->zeros_dtype))) return GEMLITE_ERR_UNSUPPORTED;
        if (a->K % e != 0) return GEMLITE_ERR_BAD_SHAPE;
        grouped = p.w_mode >= 2 || (need_z && !a->zero_is_scalar);
        if (grouped && a->K % a->group_size != 0) return GEMLITE_ERR_BAD_SHAPE;
        p.fmt = DQ_INT;
        p.w_dt = a->w_dtype;
        p.pack_bits = e > 1 ? a->w_pack_bits : 0;
        p.group = grouped ? a->group_size : (int)(a->K > 0x7FFFFFFF ? 0x7FFFFFFF : a->K);  // no group metadata: one group, never indexed
    }
    if (a->N > 0x7FFFFFFFll * 64 || a->K > 65535ll * 256) return GEMLITE_ERR_BAD_SHAPE;
    p.w = a->w_q; p.scales = a->scales; p.zeros = a->zeros; p.out = a->out;
    p.N = a->N; p.K = a->K; p.stride_wk = a->stride_wk; p.stride_wn = a->stride_wn;
    p.stride_meta_g = a->stride_meta_g; p.stride_meta_n = a->stride_meta_n; p.ld_out = a->ld_out;
    p.nbits = nb; p.e = e;
    p.meta_dt = a->meta_dtype; p.zeros_dt = a->zeros_dtype; p.zero_is_scalar = a->zero_is_scalar != 0;
    p.out_dt = a->out_dtype; p.post = a->post_scale;

    const int osz = a->out_dtype == GEMLITE_DT_FP32 ? 4 : 2;
    const bool out_vec = ((uintptr_t)a->out % 16 == 0) && ((a->ld_out * osz) % 16 == 0) && a->K % 8 == 0;
    const void* fn = nullptr;
    if (out_vec && p.fmt == DQ_INT && e > 1 && a->w_pack_bits == 32 && a->stride_wn == 1 && a->stride_wk >= a->N && (uintptr_t)a->w_q % 4 == 0 &&
        (!grouped || a->group_size % 8 == 0)) {
        fn = dequantize_words_kernel_fn(nb);
    } else if (out_vec && a->stride_wk == 1) {
        const bool bytes8 = (uintptr_t)a->w_q % 8 == 0 && a->stride_wn % 8 == 0, bytes4 = (uintptr_t)a->w_q % 4 == 0 && a->stride_wn % 4 == 0;
        if (p.fmt == DQ_INT) {
            const int dt = a->w_dtype;
            const bool one_byte = e == 1 && (dt == GEMLITE_DT_INT8 || dt == GEMLITE_DT_UINT8 || dt == GEMLITE_DT_FP8E4 || dt == GEMLITE_DT_FP8E5);
            if (one_byte && bytes8 && a->stride_wn >= a->K && (!grouped || a->group_size % 8 == 0)) fn = dequantize_rows_kernel_fn(DQ_INT);
        } else if (e == 2 ? (bytes4 && a->stride_wn >= a->K / 2) : (bytes8 && a->stride_wn >= a->K)) {
            fn = dequantize_rows_kernel_fn(p.fmt);
        }
    }
    void* kargs[] = {(void*)&p};
    if (fn) return launch(fn, dim3((unsigned)((a->N + 63) / 64), (unsigned)((a->K + 255) / 256), 1), dim3(256, 1, 1), kargs, 0, (hipStream_t)stream);
    const int64_t blocks = (a->N * a->K + 255) / 256;
    if (blocks > 0x7FFFFFFF) return GEMLITE_ERR_BAD_SHAPE;
    return launch(dequantize_any_kernel_fn(), dim3((unsigned)blocks, 1, 1), dim3(256, 1, 1), kargs, 0, (hipStream_t)stream);
}

}  // extern "C"
