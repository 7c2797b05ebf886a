// experts_route.hip — experts_route_kernel: the router's ids -> the work table of gemm_w4_rows_experts_kernel (gemm_wn_rows_experts.hip), in
// ONE launch of ONE block, with no host synchronisation (gemlite_hip_experts_route, api.hip).  The slots are counted per expert in LDS,
// the block counts ceil(c_e / R) are prefix-summed, and every slot takes the next free row of its expert's blocks (an LDS atomic: the
// order inside an expert is whatever the atomics give, and no output depends on it).  Table (int32, gl_common.h: EXPERTS_ROWS_HEADER):
//   [0] blocks used, [1..3] 0 | block_expert[Bmax] | block_rows[Bmax * R], -1 = no slot
// An id outside [0, E) — the unsigned comparison of dec3::expert_valid: negative, too large, an int64 with a high dword — goes to bucket
// E.  Entries beyond the used count are not written.  Limits: E <= ROUTE_MAX_EXPERTS (the three LDS arrays), n_slots <= 65535 — at most
// 64 slots per thread and pass; the launch costs a few microseconds and is off the weight stream.
#include "gl_common.h"
#include "gl_host.h"

namespace gl {

constexpr int ROUTE_THREADS = 1024, ROUTE_MAX_EXPERTS = GEMLITE_EXPERTS_ROWS_MAX_EXPERTS, ROUTE_BUCKETS = ROUTE_MAX_EXPERTS + 1;
constexpr int ROUTE_PER_THREAD = (ROUTE_BUCKETS + ROUTE_THREADS - 1) / ROUTE_THREADS;

template <bool IDS64>
__device__ __forceinline__ uint32_t route_bucket(const void* ids, uint32_t slot, uint32_t n_experts) {
    uint64_t e;
    if constexpr (IDS64) e = (uint64_t)((const int64_t*)ids)[slot];
    else e = (uint64_t)(uint32_t)((const int32_t*)ids)[slot];
    return e < (uint64_t)n_experts ? (uint32_t)e : n_experts;
}

template <bool IDS64>
__global__ __launch_bounds__(ROUTE_THREADS, 1) void experts_route_kernel(const void* ids, int32_t* table, uint32_t n_slots, uint32_t n_experts,
                                                                          uint32_t R, uint32_t bmax) {
    __shared__ uint32_t cnt[ROUTE_BUCKETS], first[ROUTE_BUCKETS], cur[ROUTE_BUCKETS];  // slots of a bucket, its first block, its next free row
    __shared__ uint32_t wave_sum[ROUTE_THREADS / 64];
    const uint32_t tid = threadIdx.x, nb = n_experts + 1;
    for (uint32_t e = tid; e < nb; e += ROUTE_THREADS) cnt[e] = cur[e] = 0u;
    __syncthreads();
    for (uint32_t s = tid; s < n_slots; s += ROUTE_THREADS) atomicAdd(&cnt[route_bucket<IDS64>(ids, s, n_experts)], 1u);
    __syncthreads();
    // exclusive prefix sum of the block counts: thread t owns the buckets t PER .. t PER + PER - 1
    uint32_t mine = 0;
    for (int i = 0; i < ROUTE_PER_THREAD; ++i) {
        const uint32_t e = tid * ROUTE_PER_THREAD + i;
        if (e < nb) mine += (cnt[e] + R - 1) / R;
    }
    uint32_t incl = mine;
    for (int d = 1; d < 64; d <<= 1) {
        const uint32_t up = __shfl_up(incl, d, 64);
        if ((int)(tid & 63) >= d) incl += up;
    }
    if ((tid & 63) == 63) wave_sum[tid >> 6] = incl;
    __syncthreads();
    uint32_t before = incl - mine, used = 0;
    for (uint32_t w = 0; w < ROUTE_THREADS / 64; ++w) {
        if (w < (tid >> 6)) before += wave_sum[w];
        used += wave_sum[w];
    }
    for (int i = 0; i < ROUTE_PER_THREAD; ++i) {
        const uint32_t e = tid * ROUTE_PER_THREAD + i;
        if (e < nb) {
            first[e] = before;
            before += (cnt[e] + R - 1) / R;
        }
    }
    if (tid < (uint32_t)EXPERTS_ROWS_HEADER) table[tid] = tid == 0 ? (int32_t)used : 0;
    __syncthreads();
    int32_t* const block_expert = table + EXPERTS_ROWS_HEADER;
    int32_t* const block_rows = block_expert + bmax;
    // (used <= bmax by arithmetic — ceil(n / R) + the non-empty buckets; the comparisons keep a wrong call inside the table all the same)
    for (uint32_t s = tid; s < n_slots; s += ROUTE_THREADS) {
        const uint32_t e = route_bucket<IDS64>(ids, s, n_experts);
        const uint32_t pos = atomicAdd(&cur[e], 1u);
        const uint32_t b = first[e] + pos / R;
        if (b < bmax) block_rows[(size_t)b * R + pos % R] = (int32_t)s;
    }
    for (uint32_t e = tid; e < nb; e += ROUTE_THREADS) {
        const uint32_t c = cnt[e], blocks = (c + R - 1) / R;
        for (uint32_t k = 0; k < blocks; ++k)
            if (first[e] + k < bmax) block_expert[first[e] + k] = (int32_t)e;
        if (c % R != 0 && first[e] + blocks - 1 < bmax)  // the rows of the last block that hold no slot
            for (uint32_t r = c % R; r < R; ++r) block_rows[(size_t)(first[e] + blocks - 1) * R + r] = -1;
    }
}

const void* experts_route_fn(bool ids64) {
    return ids64 ? (const void*)experts_route_kernel<true> : (const void*)experts_route_kernel<false>;
}

}  // namespace gl
