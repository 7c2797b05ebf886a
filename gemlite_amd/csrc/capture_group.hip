// capture_group.hip — host only: back-to-back INDEPENDENT launches of one stream capture become one grouped launch.  Two kernel families
// group, each with its own kind: the M = 1 decode kernel (described first) and the few-row rows kernel (ROWS GROUPS, below).
//
// At 8.9 MB a gemv_w4_decode3_kernel launch is latency-bound: of ~4.75 us per layer in a replayed graph, ~1.7 us is the dependent-launch
// boundary and ~1.6 us ramp, first-byte latency and tail, all paid again by the next launch.  Real decode graphs hold runs
// of launches that do not depend on each other (q / k / v, gate / up, experts; the benchmark step: one x, 64 weights, 64 outputs); they are
// serialised only because `layer(x)` is a per-layer call.  A stream capture can be looked back into while it is in progress
// (hipStreamGetCaptureInfo_v2 names the node the next launch would depend on) and its nodes can be edited (hipGraphKernelNodeSetParams), so:
//
//   * a decode3 launch under capture that cannot join is launched as always, and the node it became opens a group of one;
//   * the next decode3 launch joins the open group when NOTHING else was captured on the stream since (the stream's only dependency is the
//     group's node), kernel / shape / strides / modes agree, and its output overlaps no member's inputs or output and no member's output
//     overlaps its inputs (a bias the kernel adds itself — gemlite_hip_forward_ext — is one more input).  Joining rewrites the node to gemv_w4_decode3_group_kernel, grid (tiles, Y) with
//     Y = clamp(resident blocks / tiles, 1, members): one resident block per tile holds its members ALL AT ONCE — each member gets
//     16 / (members of the block) of the block's waves and its own 4 KB of LDS, and the block has one barrier (decode3_wave_split,
//     gl_common.h; gemv_decode.hip) — and narrow layers spread their members over the CUs their tiles leave idle.  No node is added and
//     the stream's dependency set stays as it is.
//
// The graph stays LINEAR on one queue.  Sound because nothing foreign lies between A and B on the stream: B's stream-order dependencies are
// A plus A's own, and independence from A makes A's own sufficient; everything captured later depends on the group node and so on every
// member.  A dependent chain (x_B overlaps out_A) never groups and gets the graph it always got, node for node.  Any HIP error on this path
// drops the group and the call is launched the plain way: grouping never turns a working capture into a failing one.
//
// A group whose members all read the SAME x (q / k / v, gate / up, the experts of one token) takes the shared-x form of the grouped kernel
// (gemv_decode.hip: x is staged in LDS once per block): the form is chosen again at every join (decode3_group_form, gl_common.h), so the
// first member with another x puts the group back on the per-wave-x form for good.
//
// GEMLITE_HIP_NO_CAPTURE_GROUPS=1 (read once) turns it off; GEMLITE_HIP_CAPTURE_GROUP_MAX=n (development, read once) lowers the member limit;
// GEMLITE_HIP_CAPTURE_GROUP_SHARED_X=0 (read once) keeps every group on the per-wave-x form (A/B runs in separate processes).
//
// TILE GROUPS (gl_common.h: decode3_group_geometry): a grouped block may hold TB = 1, 2 or 4 adjacent tiles x its layers, grid
// (tiles / TB, Y), and its tile groups are placed on the XCDs interleaved or in contiguous spans.  (TB, placement) is chosen again at every
// join from members, tiles and resident blocks (decode3_group_tiles_default); GEMLITE_HIP_CAPTURE_GROUP_TILES=<TB>[s|i] (development, read
// once) forces the TB asked for and the span ("s") or interleaved ("i", the default) placement for A/B runs — a TB that does not fit the
// shape still falls back to the next smaller one.
//
// LINES (gl_common.h: decode3_group_lines): a wave of a grouped block may work on H = 1, 2 or 4 adjacent tiles of its block's tile group at once,
// in H passes over each virtual wave, so that one request instruction asks for whole 128-byte (H = 2) or 256-byte (H = 4) runs of 8 or 4 weight
// rows.  H divides TB; it is chosen at every join (decode3_group_lines_default), and every H has kernel functions of its own.
// GEMLITE_HIP_CAPTURE_GROUP_LINES=1|2|4 (development, read once) forces the H asked for; one that TB does not admit falls back 4 -> 2 -> 1.
//
// POLICY (gl_common.h: decode3_group_nt): a grouped node asks for its weights non-temporally when its waves ask for whole lines (H >= 2), its
// members' own launches are non-temporal (no GEMLITE_TF_GEMV_DEFAULT_POLICY_LOADS in the layer's tuning) and every member's weight base and
// the row pitch are multiples of 128 bytes; evaluated at every join, so one member 64 bytes into a line puts the group back on the
// default-policy form.  GEMLITE_HIP_CAPTURE_GROUP_NT=0|1 (development, read once) forces the policy; a forced 1 still falls back where H = 1.
//
// ROUNDS (gl_common.h: decode3_round_member).  A node holds at most DECODE3_GMAX members because a block holds at most 16 slots, so a run of
// 64 independent layers used to become four nodes and pay the dependent-launch boundary, the ramp and the tail four times.  When a join
// makes the open decode group B FULL (members == the limit), B is merged into its predecessor A — the group that was open and full when
// B's first launch was declined for the member limit, kept as this thread's "previous group" — if A is of the same capture and graph,
// holds a whole number of full rounds below the round limit, same_launch(A, B) holds with both biased or both not, every member of B is
// independent() of every member of A, and the RUNTIME says that the graph is the chain it should be: B's node has exactly one dependency,
// A's node, and no dependent; A's node has exactly one dependent, B's node; the stream's only capture dependency is B's node (a fork
// from another stream onto B, or anything foreign between A and B, rules the merge out).  A's node then becomes a node of R + 1 rounds:
// grid (grid_x, Y (R + 1)), the table A's members followed by B's, form / H / policy by the rules above on all members (both nodes were
// full: TB, Y and H agree); the stream's capture dependency is set back to A's node; B's node is destroyed; the open group is A, full,
// so the next launch opens C, which merges when it fills, up to DECODE3_NODE_MAX / limit rounds.  Members of B are independent of A's
// and of each other, so every intermediate state — B's members in both nodes — computes the right outputs; a step that fails undoes the
// ones before it (A gets its parameters back), the runtime's error is swallowed and the capture is what it was without merging.  A
// trailing partial group keeps its own node: its best (TB, H, form) is another.  Blocks go out x-fastest, one block is resident per CU, so
// a CU takes its block of the next round as soon as its own block leaves.  GEMLITE_HIP_CAPTURE_GROUP_ROUNDS=1..4 (development, read once)
// is the round limit, 1: no merging (the A/B switch inside one build); GEMLITE_HIP_NO_CAPTURE_GROUPS=1 turns merging off with the rest.
// The rows family does not merge: its table stays at DECODE3_GMAX and its node already runs full-width members as rounds.
//
// ROWS GROUPS (family 2).  A serving engine captures one graph per batch size; with two or more requests in a step every 4- / 2-bit layer runs
// gemm_w4_rows_kernel / gemm_w2_rows_kernel (gemm_wn_rows.hip, LaunchPlan::arg_kind == 2), and q / k / v, gate / up and the experts of a step
// pay the launch boundary each.  They group under the same look-back, independence rule, member limit and counters: a rows launch joins
// the open rows group when same_launch() holds — the same kernel function (dtype, MT, SPG, NT, bits, biased or not), grid.x, block, LDS
// bytes and the seven shared scalars sw4 / mstride2 / nch_total / modes / M / sxm2 / som, and ONE row block (grid.y == 1: the grouped
// kernel has none).  The node becomes gemm_w4_rows[_bias]_group_kernel (gemm_wn_rows_group.hip), grid (tiles, members): block (tile, y)
// computes member y's tile exactly as its own launch would; blocks go out x-fastest, so narrow layers spread their members over idle CUs
// and full-width ones run their members in successive rounds without a launch boundary.  The dynamic-LDS cap of the grouped function is
// raised once per device (ensure_lds) before the node is rewritten.  The families never mix: a launch of one family behind an open group
// of the other fails same_launch(), is launched the plain way and opens its own group.  gemlite_hip_capture_group_last_form() == 3.
// GEMLITE_HIP_CAPTURE_GROUP_ROWS=0 (read once) keeps only this family ungrouped (A/B runs in separate processes).
#include <atomic>
#include <cstdlib>
#include <cstring>

#include "gl_host.h"

namespace gl {

namespace {

struct Span {  // bytes [lo, hi); empty when lo == hi
    uintptr_t lo, hi;
};
struct Footprint {
    Span rd[5];  // x, W_q, scales, zeros, bias (empty unless the launch adds one)
    Span wr;     // out
};

bool overlap(const Span& a, const Span& b) { return a.lo < b.hi && b.lo < a.hi && a.lo != a.hi && b.lo != b.hi; }

int elt_bytes(int dt) {  // (unknown codes: the widest, the footprint only has to be large enough)
    switch (dt) {
        case GEMLITE_DT_FP16: case GEMLITE_DT_BF16: case GEMLITE_DT_INT16: case GEMLITE_DT_UINT16: return 2;
        case GEMLITE_DT_FP32: case GEMLITE_DT_INT32: case GEMLITE_DT_UINT32: return 4;
        default: return 8;
    }
}

// A 2-d view of n0 x n1 elements of `esz` bytes at strides s0 / s1 (elements, either sign): from its lowest byte to the end of its last element
Span span2d(const void* p, int64_t esz, int64_t n0, int64_t s0, int64_t n1, int64_t s1) {
    if (!p || n0 <= 0 || n1 <= 0) return Span{0, 0};
    const int64_t e0 = (n0 - 1) * s0, e1 = (n1 - 1) * s1;
    const int64_t lo = (e0 < 0 ? e0 : 0) + (e1 < 0 ? e1 : 0), hi = (e0 > 0 ? e0 : 0) + (e1 > 0 ? e1 : 0) + 1;
    return Span{(uintptr_t)p + (uintptr_t)(lo * esz), (uintptr_t)p + (uintptr_t)(hi * esz)};
}

// Everything one decode3 launch may touch, from the caller's pointers, shapes and strides (never less than the kernel reads or writes:
// metadata pointers count whenever they are given, whether the mode reads them or not)
Footprint footprint(const gemlite_hip_forward_args& a, const LaunchPlan& lp) {
    Footprint f;
    const int64_t e = a.elements_per_sample > 0 ? a.elements_per_sample : 1, gs = a.group_size > 0 ? a.group_size : 1;
    f.rd[0] = span2d(a.x, elt_bytes(a.input_dtype), a.M, a.stride_xm, a.K, a.stride_xk);
    f.rd[1] = span2d(a.w_q, a.w_pack_bits > 0 ? a.w_pack_bits / 8 : elt_bytes(a.w_dtype), (a.K + e - 1) / e, a.stride_wk, a.N, a.stride_wn);
    f.rd[2] = span2d(a.scales, elt_bytes(a.meta_dtype), (a.K + gs - 1) / gs, a.stride_meta_g, a.N, a.stride_meta_n);
    f.rd[3] = a.zero_is_scalar ? span2d(a.zeros, 8, 1, 0, 1, 0)
                               : span2d(a.zeros, elt_bytes(a.zeros_dtype), (a.K + gs - 1) / gs, a.stride_meta_g, a.N, a.stride_meta_n);
    f.rd[4] = span2d(lp.bias, 2, 1, 0, a.N, 1);
    f.wr = span2d(a.out, elt_bytes(a.output_dtype), a.M, a.stride_om, a.N, a.stride_on);
    return f;
}

bool independent(const Footprint& a, const Footprint& b) {
    if (overlap(a.wr, b.wr)) return false;
    for (int i = 0; i < 5; ++i)
        if (overlap(b.wr, a.rd[i]) || overlap(a.wr, b.rd[i])) return false;
    return true;
}

// What a group shares: the kernel, its grid and the four scalars behind the five pointers.  (The timeline probe never groups.)
// Rows launches (arg_kind 2): the kernel, grid.x with ONE row block, block, LDS bytes and the seven scalars behind the five pointers.
// No shape, M or member count is kept out: every measured cell — 2, 4 and 16 members, 64 and 256 tiles, K = 4096 and 11008, M = 8 .. 64 —
// was faster grouped by more than the run-to-run spread (profiles/r17/rows_groups.log §2: smallest gain 0.76 us per layer, spread 0.18).
bool same_launch(const LaunchPlan& a, const LaunchPlan& b) {
    if (a.arg_kind == 2 && b.arg_kind == 2)
        return a.fn == b.fn && a.grid.x == b.grid.x && a.grid.y == 1 && b.grid.y == 1 && a.grid.z == 1 && b.grid.z == 1 &&
               a.block.x == b.block.x && a.lds_bytes == b.lds_bytes && a.r5.sw4 == b.r5.sw4 && a.r5.mstride2 == b.r5.mstride2 &&
               a.r5.nch_total == b.r5.nch_total && a.r5.modes == b.r5.modes && a.r5.M == b.r5.M && a.r5.sxm2 == b.r5.sxm2 &&
               a.r5.som == b.r5.som;
    return a.arg_kind == 1 && b.arg_kind == 1 && a.fn == b.fn && a.grid.x == b.grid.x && a.grid.y == 1 && b.grid.y == 1 && a.grid.z == 1 &&
           b.grid.z == 1 && a.block.x == b.block.x && a.d3.sw4 == b.d3.sw4 && a.d3.mstride2 == b.d3.mstride2 &&
           a.d3.nch_total == b.d3.nch_total && a.d3.modes == b.d3.modes && !(a.d3.modes & 64u);
}

// Does the launch have grouped forms?  The planner says so — rows: LaunchPlan::fn_group / fn_bias_group, decode3: d3_group_tag — and `fn`
// is still the planner's choice (the biased form exactly when the launch carries a bias)
bool has_group_form(const LaunchPlan& lp) {
    if (lp.fn != (lp.bias ? lp.fn_bias : lp.bias_of)) return false;
    if (lp.arg_kind == 2) return (lp.bias ? lp.fn_bias_group : lp.fn_group) != nullptr;
    return lp.arg_kind == 1 && lp.d3_group_tag >= 0;
}

int env_int(const char* name, int absent) {
    const char* v = getenv(name);
    return (v && *v) ? atoi(v) : absent;
}

std::atomic<uint64_t> g_seen{0}, g_joined{0}, g_merged{0};

struct Group {
    bool open = false;
    bool capturing = false;  // the last try_join() of this thread saw an active capture: note_launch() has a node to pick up
    unsigned long long cap_id = 0;
    hipGraph_t graph = nullptr;
    hipGraphNode_t node = nullptr;
    LaunchPlan lp{};  // member 0: kernel, grid, block, scalars
    bool same_x = true;  // every member so far reads member 0's x
    uintptr_t w_or = 0;  // every member's weight base, OR-ed: the alignment decode3_group_nt() asks about
    // members 1 .. and every member's bias; an unbiased kernel's argument is its prefix (gl_common.h).  A decode group keeps the node
    // table (room for the rounds it may absorb), a rows group the table of its kernels
    DecodeNodeTable<true> tab{};
    GroupTable<true> rtab{};
    Footprint fp[DECODE3_NODE_MAX];
    int members = 0;
    int rounds = 1;         // decode: full rounds in the node once it has merged (members == rounds * limit then)
    bool mergeable = true;  // false once a rewrite for a merge failed on this node
    // the node as the last rewrite left it (decode groups): what a failed merge puts back
    const void* node_fn = nullptr;
    dim3 node_grid{1, 1, 1};
    size_t node_lds = 0;
    uint32_t node_modes = 0;
    int node_form = 0, node_lines = 0, node_policy = -1;
};
thread_local Group tl_group;
// The previous group: the one that was open and full when the launch that opened tl_group was declined for the member limit
thread_local Group tl_prev;
thread_local bool tl_prev_valid = false;
thread_local int tl_last_rounds = 0;  // rounds of the last decode node this thread rewrote or merged (0: none yet)
thread_local int tl_last_form = 0;  // of the last group node this thread rewrote: decode3_group_form()
thread_local int tl_last_lines = 0;  // and its H (0: no grouped decode node yet)
thread_local int tl_last_policy = -1;  // and its weight-load policy: 0 default, 1 non-temporal (-1: no grouped decode node yet)

bool capture_state(hipStream_t st, unsigned long long* id, hipGraph_t* graph, hipGraphNode_t* only_dep) {
    hipStreamCaptureStatus status = hipStreamCaptureStatusNone;
    const hipGraphNode_t* deps = nullptr;
    size_t ndeps = 0;
    *graph = nullptr;
    if (hipStreamGetCaptureInfo_v2(st, &status, id, graph, &deps, &ndeps) != hipSuccess) {
        (void)hipGetLastError();
        return false;
    }
    if (status != hipStreamCaptureStatusActive || !*graph) return false;
    *only_dep = (ndeps == 1 && deps) ? deps[0] : nullptr;
    return true;
}

}  // namespace

int capture_group_limit() {
    static const int limit = [] {
        if (env_int("GEMLITE_HIP_NO_CAPTURE_GROUPS", 0) != 0) return 1;
        const int n = env_int("GEMLITE_HIP_CAPTURE_GROUP_MAX", DECODE3_GMAX);
        return n < 1 ? 1 : (n > DECODE3_GMAX ? DECODE3_GMAX : n);
    }();
    return limit;
}

bool capture_group_rows_enabled() {
    static const bool on = env_int("GEMLITE_HIP_CAPTURE_GROUP_ROWS", 1) != 0;
    return on;
}

bool capture_group_shared_x_enabled() {
    static const bool on = env_int("GEMLITE_HIP_CAPTURE_GROUP_SHARED_X", 1) != 0;
    return on;
}

// What try_join() asks decode3_group_geometry() for: the forced pair of GEMLITE_HIP_CAPTURE_GROUP_TILES, or the rule of gl_common.h
Decode3TilesWanted capture_group_tiles_wanted(int tiles, int members, int resident) {
    static const Decode3TilesWanted forced = [] {
        const char* v = getenv("GEMLITE_HIP_CAPTURE_GROUP_TILES");
        if (!v || !*v) return Decode3TilesWanted{0, false};
        const int tb = atoi(v);
        return Decode3TilesWanted{tb >= 4 ? 4 : (tb >= 2 ? 2 : 1), strchr(v, 's') != nullptr};
    }();
    return forced.tb ? forced : decode3_group_tiles_default(tiles, members, resident);
}

// The H try_join() asks decode3_group_lines() for: the forced one of GEMLITE_HIP_CAPTURE_GROUP_LINES, or the rule of gl_common.h
int capture_group_lines_wanted(int tiles, int members, int resident, int tb) {
    static const int forced = [] {
        const int h = env_int("GEMLITE_HIP_CAPTURE_GROUP_LINES", 0);
        return h >= 4 ? 4 : (h >= 2 ? 2 : (h == 1 ? 1 : 0));
    }();
    return forced ? forced : decode3_group_lines_default(tiles, members, resident, tb);
}

// The policy try_join() hands decode3_group_nt(): what GEMLITE_HIP_CAPTURE_GROUP_NT forces (0 / 1), or -1: the rule
int capture_group_policy_forced() {
    static const int forced = [] {
        const int v = env_int("GEMLITE_HIP_CAPTURE_GROUP_NT", -1);
        return v < 0 ? -1 : (v ? 1 : 0);
    }();
    return forced;
}

int capture_group_last_form() { return tl_last_form; }
int capture_group_last_policy() { return tl_last_policy; }
int capture_group_last_lines() { return tl_last_lines; }
int capture_group_last_rounds() { return tl_last_rounds; }

// Rounds a decode node may hold: GEMLITE_HIP_CAPTURE_GROUP_ROUNDS (1 .. 4, read once), within what the node table holds at this member limit
int capture_group_rounds_max() {
    static const int rounds = [] {
        if (capture_group_limit() < 2) return 1;
        const int n = env_int("GEMLITE_HIP_CAPTURE_GROUP_ROUNDS", DECODE3_ROUNDS_DEFAULT), cap = DECODE3_NODE_MAX / capture_group_limit();
        const int r = n < 1 ? 1 : (n > DECODE3_ROUNDS_LIMIT ? DECODE3_ROUNDS_LIMIT : n);
        return r > cap ? cap : r;
    }();
    return rounds;
}

void capture_group_merge_stats(uint64_t* merged) {
    if (merged) *merged = g_merged.load(std::memory_order_relaxed);
}

void capture_group_stats(uint64_t* seen, uint64_t* joined) {
    if (seen) *seen = g_seen.load(std::memory_order_relaxed);
    if (joined) *joined = g_joined.load(std::memory_order_relaxed);
}

// The host-only rule: may launch B (args b, plan lb) run in the same grouped launch as A?
bool capture_group_compatible(const gemlite_hip_forward_args& a, const LaunchPlan& la, const gemlite_hip_forward_args& b, const LaunchPlan& lb) {
    if (!same_launch(la, lb)) return false;
    if (!has_group_form(la)) return false;
    return independent(footprint(a, la), footprint(b, lb));
}

// What a join of either family does once its kernel, grid, LDS bytes and argument list are chosen: member g.members goes into the table
// (its pointers behind the scalars of member 0), the node becomes `fn`, the bookkeeping.  A failed rewrite leaves the node what it was: the
// group is dropped and this call runs on its own.
static bool set_node(const Group& g, const void* fn, dim3 grid, size_t lds, void** kargs) {
    hipKernelNodeParams np;
    memset(&np, 0, sizeof(np));
    np.func = (void*)fn;
    np.gridDim = grid;
    np.blockDim = g.lp.block;
    np.sharedMemBytes = (unsigned)lds;
    np.kernelParams = kargs;
    np.extra = nullptr;
    if (hipGraphKernelNodeSetParams(g.node, &np) != hipSuccess) {
        (void)hipGetLastError();
        return false;
    }
    return true;
}
template <typename Table>
static bool rewrite_node(Group& g, Table& tab, const GroupMember& mb, const uint16_t* bias, const Footprint& fb, const void* fn, dim3 grid,
                         size_t lds, void** kargs) {
    tab.m[g.members - 1] = mb;
    tab.bias[g.members] = bias;
    if (!set_node(g, fn, grid, lds, kargs)) {
        g.open = false;
        return false;
    }
    g.fp[g.members++] = fb;
    g_joined.fetch_add(1, std::memory_order_relaxed);
    return true;
}

// ROUNDS: the open decode group `b` has just become full and tl_prev is the full group in front of it.  Merge b into it when every
// condition of the header holds; whatever happens, the capture computes what it computed without this call.  dep: the stream's only
// capture dependency, as asked at the top of this join (b's node: the join added nothing).
static size_t node_count(hipGraphNode_t node, bool dependents, hipGraphNode_t* only) {
    size_t n = 0;
    *only = nullptr;
    if ((dependents ? hipGraphNodeGetDependentNodes(node, nullptr, &n) : hipGraphNodeGetDependencies(node, nullptr, &n)) != hipSuccess) {
        (void)hipGetLastError();
        return (size_t)-1;
    }
    if (n != 1) return n;
    if ((dependents ? hipGraphNodeGetDependentNodes(node, only, &n) : hipGraphNodeGetDependencies(node, only, &n)) != hipSuccess) {
        (void)hipGetLastError();
        return (size_t)-1;
    }
    return n;
}
static void try_merge(Group& b, hipGraphNode_t dep, hipStream_t st, int resident, int dev) {
    Group& a = tl_prev;
    tl_prev_valid = false;  // one attempt: merged, a is the open group; not merged, b's successor has b (or nothing) in front of it
    const int limit = capture_group_limit();
    if (!a.mergeable || a.cap_id != b.cap_id || a.graph != b.graph || a.node == b.node || dep != b.node) return;
    if (a.members != a.rounds * limit || b.members != limit || a.rounds >= capture_group_rounds_max() || a.members + b.members > DECODE3_NODE_MAX) return;
    if (!same_launch(a.lp, b.lp) || (a.lp.bias != nullptr) != (b.lp.bias != nullptr) || !a.node_fn || !b.node_fn) return;
    // the graph, as the runtime has it: ... -> A -> B, nothing else on either, and the stream waits for B alone (dep, above)
    hipGraphNode_t only = nullptr;
    if (node_count(b.node, false, &only) != 1 || only != a.node) return;
    if (node_count(b.node, true, &only) != 0) return;
    if (node_count(a.node, true, &only) != 1 || only != b.node) return;
    for (int i = 0; i < a.members; ++i)
        for (int j = 0; j < b.members; ++j)
            if (!independent(a.fp[i], b.fp[j])) return;
    // 1. A's node: one more round.  Both nodes are full, so (TB, Y, H) of a round are b's; form and policy over all members
    Decode3Args& d = a.lp.d3;
    const int tiles = (int)a.lp.grid.x, rounds = a.rounds + 1;
    const Decode3TilesWanted want = capture_group_tiles_wanted(tiles, limit, resident);
    const Decode3GroupGeometry geo = decode3_group_geometry(tiles, limit, resident, want.tb, want.span);
    const int lines = decode3_group_lines(geo.tb, capture_group_lines_wanted(tiles, limit, resident, geo.tb));
    uint32_t modes = decode3_group_modes(d.modes, limit, geo.grid_y, geo.tb, geo.span);
    const dim3 grid((unsigned)geo.grid_x, (unsigned)(geo.grid_y * rounds), 1);
    if (modes != b.node_modes || modes != a.node_modes || a.node_grid.x != grid.x || a.node_grid.y != (unsigned)(geo.grid_y * a.rounds) ||
        lines != a.node_lines || lines != b.node_lines)
        return;  // (a round of A and B's are not the same blocks: cannot happen with both full, and is not merged if it does)
    const bool same_x = a.same_x && b.same_x && b.lp.d3.x == d.x;
    int form = decode3_group_form(limit, same_x, d.nch_total, capture_group_shared_x_enabled());
    const uintptr_t w_or = a.w_or | b.w_or;
    const bool nt = decode3_group_nt(lines, a.lp.d3_nt && b.lp.d3_nt, (uint64_t)w_or, d.sw4, capture_group_policy_forced());
    const bool biased = a.lp.bias != nullptr;
    const void* fn = gemv_w4_decode3_group_fn(a.lp.d3_group_tag, biased, form == 2, lines, nt);
    if (form == 2 && ensure_lds(fn, (size_t)DECODE3_SHARED_X_MAX_LDS, dev) != GEMLITE_OK) {
        form = 1;
        fn = gemv_w4_decode3_group_fn(a.lp.d3_group_tag, biased, false, lines, nt);
    }
    const size_t lds = form == 2 ? (size_t)decode3_shared_x_lds_bytes(d.nch_total) : 0;
    // the table: A's members, then B's (B's member 0 travelled in B's scalars).  Entries past a.members are read by no block of A's
    // present grid, so a failed step leaves A exactly what it was
    const int m0 = a.members;
    a.tab.m[m0 - 1] = GroupMember{b.lp.d3.w, b.lp.d3.x, b.lp.d3.s, b.lp.d3.z, b.lp.d3.out};
    for (int j = 1; j < b.members; ++j) a.tab.m[m0 + j - 1] = b.tab.m[j - 1];
    for (int j = 0; j < b.members; ++j) a.tab.bias[m0 + j] = b.tab.bias[j];
    void* kargs[] = {(void*)&d.w, (void*)&d.x, (void*)&d.s, (void*)&d.z, (void*)&d.out, (void*)&d.sw4, (void*)&d.mstride2,
                     (void*)&d.nch_total, (void*)&modes, (void*)&a.tab};
    if (!set_node(a, fn, grid, lds, kargs)) {
        a.mergeable = false;
        return;
    }
    auto restore_a = [&] {
        void* old[] = {(void*)&d.w, (void*)&d.x, (void*)&d.s, (void*)&d.z, (void*)&d.out, (void*)&d.sw4, (void*)&d.mstride2,
                       (void*)&d.nch_total, (void*)&a.node_modes, (void*)&a.tab};
        (void)set_node(a, a.node_fn, a.node_grid, a.node_lds, old);
    };
    // 2. the stream waits for A's node instead of B's
    hipGraphNode_t na = a.node;
    if (hipStreamUpdateCaptureDependencies(st, &na, 1, hipStreamSetCaptureDependencies) != hipSuccess) {
        (void)hipGetLastError();
        restore_a();
        return;
    }
    // 3. B's node leaves the graph
    if (hipGraphDestroyNode(b.node) != hipSuccess) {
        (void)hipGetLastError();
        hipGraphNode_t nb = b.node;
        if (hipStreamUpdateCaptureDependencies(st, &nb, 1, hipStreamSetCaptureDependencies) != hipSuccess) (void)hipGetLastError();
        restore_a();
        return;
    }
    // 4. the open group is A, full: the next launch is declined for the member limit and finds A in front of it
    for (int j = 0; j < b.members; ++j) a.fp[m0 + j] = b.fp[j];
    a.members = m0 + b.members;
    a.rounds = rounds;
    a.same_x = same_x;
    a.w_or = w_or;
    a.lp.d3_nt = a.lp.d3_nt && b.lp.d3_nt;
    a.node_fn = fn;
    a.node_grid = grid;
    a.node_lds = lds;
    a.node_modes = modes;
    a.node_form = tl_last_form = form;
    a.node_lines = tl_last_lines = lines;
    a.node_policy = tl_last_policy = nt ? 1 : 0;
    tl_last_rounds = rounds;
    a.open = true;
    a.capturing = b.capturing;
    b = a;
    g_merged.fetch_add(1, std::memory_order_relaxed);
}

// Called in front of every decode3 and every rows launch that carries no profile events.  true: the call was folded into the open group's node, nothing
// is left to launch.  false: launch as always, then call capture_group_note_launch().  resident: blocks of a one-block-per-CU kernel
// the stream's device holds at once (its CU count).
bool capture_group_try_join(const gemlite_hip_forward_args& a, const LaunchPlan& lp, hipStream_t st, int resident, int dev) {
    Group& g = tl_group;
    g.capturing = false;
    const bool rows = lp.arg_kind == 2;
    if (capture_group_limit() < 2 || (rows ? !capture_group_rows_enabled() : (lp.d3.modes & 64u) != 0)) {
        tl_prev_valid = false;
        return false;
    }
    unsigned long long id = 0;
    hipGraph_t graph = nullptr;
    hipGraphNode_t dep = nullptr;
    if (!capture_state(st, &id, &graph, &dep)) {
        g.open = false;
        tl_prev_valid = false;
        return false;
    }
    g.capturing = true;
    g_seen.fetch_add(1, std::memory_order_relaxed);
    const bool follows = g.open && g.cap_id == id && g.graph == graph && dep && dep == g.node && same_launch(g.lp, lp);
    if (!follows || g.members >= capture_group_limit()) {
        // declined: the launch opens a group of its own (note_launch).  Declined for the member limit ALONE, behind a decode node of whole
        // rounds that may take one more: the open group is that group's predecessor, and is kept for the merge
        tl_prev_valid = follows && !rows && g.mergeable && g.rounds < capture_group_rounds_max() && g.members == g.rounds * capture_group_limit();
        if (tl_prev_valid) tl_prev = g;
        return false;
    }
    const Footprint fb = footprint(a, lp);
    for (int i = 0; i < g.members; ++i)
        if (!independent(g.fp[i], fb)) {
            tl_prev_valid = false;  // (this launch opens a group that does not follow the open one)
            return false;
        }
    const bool biased = g.lp.bias != nullptr;  // (lp.bias too: same_launch() compared the kernel functions)
    if (rows) {
        // grid.y one more.  The cap on dynamic LDS first (a rows block takes 146 KiB): once per grouped function and device
        const void* fn = biased ? g.lp.fn_bias_group : g.lp.fn_group;
        if (ensure_lds(fn, g.lp.lds_bytes, dev) != GEMLITE_OK) {
            g.open = false;
            return false;
        }
        Rows5Args& r = g.lp.r5;
        void* kargs[] = {(void*)&r.w, (void*)&r.x, (void*)&r.s, (void*)&r.z, (void*)&r.out, (void*)&r.sw4, (void*)&r.mstride2, (void*)&r.nch_total,
                         (void*)&r.modes, (void*)&r.M, (void*)&r.sxm2, (void*)&r.som, (void*)&g.rtab};
        if (!rewrite_node(g, g.rtab, GroupMember{lp.r5.w, lp.r5.x, lp.r5.s, lp.r5.z, lp.r5.out}, lp.bias, fb, fn, dim3(g.lp.grid.x, (unsigned)(g.members + 1), 1),
                          g.lp.lds_bytes, kargs))
            return false;
        tl_last_form = 3;
        tl_last_lines = 0;
        tl_last_policy = -1;
        return true;
    }
    Decode3Args& d = g.lp.d3;
    // the node as it is after this join: members and grid.y are recomputed every time and travel in `modes` (no implicit grid arguments)
    const int members = g.members + 1, tiles = (int)g.lp.grid.x;
    const Decode3TilesWanted want = capture_group_tiles_wanted(tiles, members, resident);
    const Decode3GroupGeometry geo = decode3_group_geometry(tiles, members, resident, want.tb, want.span);
    const int lines = decode3_group_lines(geo.tb, capture_group_lines_wanted(tiles, members, resident, geo.tb));
    uint32_t modes = decode3_group_modes(d.modes, members, geo.grid_y, geo.tb, geo.span);
    void* kargs[] = {(void*)&d.w, (void*)&d.x, (void*)&d.s, (void*)&d.z, (void*)&d.out, (void*)&d.sw4, (void*)&d.mstride2,
                     (void*)&d.nch_total, (void*)&modes, (void*)&g.tab};
    const bool same_x = g.same_x && lp.d3.x == d.x;
    int form = decode3_group_form(members, same_x, d.nch_total, capture_group_shared_x_enabled());
    const uintptr_t w_or = g.w_or | (uintptr_t)lp.d3.w;
    const bool nt = decode3_group_nt(lines, g.lp.d3_nt, (uint64_t)w_or, d.sw4, capture_group_policy_forced());
    // (every H and either policy has kernel functions of its own.  The cap is raised once per kernel and device, to the form's maximum: the size of a launch depends on its K)
    const void* fn = gemv_w4_decode3_group_fn(g.lp.d3_group_tag, biased, form == 2, lines, nt);
    if (form == 2 && ensure_lds(fn, (size_t)DECODE3_SHARED_X_MAX_LDS, dev) != GEMLITE_OK) {
        form = 1;
        fn = gemv_w4_decode3_group_fn(g.lp.d3_group_tag, biased, false, lines, nt);
    }
    const size_t lds = form == 2 ? (size_t)decode3_shared_x_lds_bytes(d.nch_total) : 0;
    const dim3 grid((unsigned)geo.grid_x, (unsigned)geo.grid_y, 1);
    if (!rewrite_node(g, g.tab, GroupMember{lp.d3.w, lp.d3.x, lp.d3.s, lp.d3.z, lp.d3.out}, lp.bias, fb, fn, grid, lds, kargs)) return false;
    g.same_x = same_x;
    g.w_or = w_or;
    g.node_fn = fn;
    g.node_grid = grid;
    g.node_lds = lds;
    g.node_modes = modes;
    g.node_form = tl_last_form = form;
    g.node_lines = tl_last_lines = lines;
    g.node_policy = tl_last_policy = nt ? 1 : 0;
    tl_last_rounds = 1;
    if (g.members == capture_group_limit() && tl_prev_valid) try_merge(g, dep, st, resident, dev);
    return true;
}

// After a plain decode3 / rows launch that try_join() declined under capture: the node it became is the stream's single dependency now,
// and opens a new group of one (which keeps the single-layer kernel until somebody joins).
void capture_group_note_launch(const gemlite_hip_forward_args& a, const LaunchPlan& lp, hipStream_t st) {
    Group& g = tl_group;
    if (!g.capturing) return;
    g.capturing = false;
    g.open = false;
    if (!has_group_form(lp) || lp.grid.y != 1 || lp.grid.z != 1) return;
    unsigned long long id = 0;
    hipGraph_t graph = nullptr;
    hipGraphNode_t dep = nullptr;
    if (!capture_state(st, &id, &graph, &dep) || !dep) return;
    hipGraphNodeType type = hipGraphNodeTypeEmpty;
    if (hipGraphNodeGetType(dep, &type) != hipSuccess) { (void)hipGetLastError(); return; }
    if (type != hipGraphNodeTypeKernel) return;
    g.cap_id = id;
    g.graph = graph;
    g.node = dep;
    g.lp = lp;
    g.same_x = true;
    g.w_or = (uintptr_t)lp.d3.w;
    tl_last_form = 0;  // (a group of one: no grouped node yet)
    tl_last_lines = 0;
    tl_last_policy = -1;
    tl_last_rounds = 0;
    g.rounds = 1;
    g.mergeable = true;
    g.node_fn = nullptr;
    // (only the one-round part of the node table: the rest is written before a kernel indexes it)
    memset(&g.rtab, 0, sizeof(g.rtab));
    memset(g.tab.m, 0, sizeof(GroupMember) * (DECODE3_GMAX - 1));
    memset(g.tab.bias, 0, sizeof(g.tab.bias[0]) * DECODE3_GMAX);
    g.tab.bias[0] = g.rtab.bias[0] = lp.bias;
    g.fp[0] = footprint(a, lp);
    g.members = 1;
    g.open = true;
}

}  // namespace gl
