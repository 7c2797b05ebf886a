// gl_async.h — memory requests that the compiler must not wait for, and the counted waits that retire them.
#pragma once
#include "gl_common.h"

namespace gl {
namespace async {

// ---- memory requests the compiler must NOT wait for.  hipcc answers any use of a tracked load with vmcnt(0) while an
// LDS-DMA is outstanding, which would drain the x / weight pipeline every step; these requests are therefore issued from
// inline asm and retired by hand with COUNTED s_waitcnt (cdna_hip_programming.md §5.7): loads return in issue order, so
// "vmcnt(n)" = everything but the newest n requests of this wave has landed.  A loaded register is handed to the compiler
// with tie() right after the wait that covers it.  s_nop 4: SALU-written SGPR / M0 -> VMEM wait states (nothing inside an
// asm string is padded by the compiler).
typedef uint32_t srd_t __attribute__((ext_vector_type(4)));
__device__ __forceinline__ srd_t make_srd(const void* base, uint32_t bytes) {
    const uint64_t b = (uint64_t)base;
    srd_t r;
    r[0] = __builtin_amdgcn_readfirstlane((uint32_t)b);
    r[1] = __builtin_amdgcn_readfirstlane((uint32_t)(b >> 32) & 0xFFFFu);
    r[2] = __builtin_amdgcn_readfirstlane(bytes);
    r[3] = 0x00020000u;
    return r;
}
__device__ __forceinline__ void req_u32(uint32_t& dst, srd_t rs, uint32_t voff, uint32_t soff) {
    asm volatile("s_nop 4\n\tbuffer_load_dword %0, %1, %2, %3 offen" : "=v"(dst) : "v"(voff), "s"(rs), "s"(soff) : "memory");
}
__device__ __forceinline__ void req_u16(uint32_t& dst, srd_t rs, uint32_t voff, uint32_t soff) {
    asm volatile("s_nop 4\n\tbuffer_load_ushort %0, %1, %2, %3 offen" : "=v"(dst) : "v"(voff), "s"(rs), "s"(soff) : "memory");
}
// the same without the nop: soffset computed by SALU instructions (s_mul / s_add / s_mov) is interlocked; only a VALU-written SGPR
// (v_readfirstlane) needs the 5 wait states
__device__ __forceinline__ void req_u32n(uint32_t& dst, srd_t rs, uint32_t voff, uint32_t soff) {
    asm volatile("buffer_load_dword %0, %1, %2, %3 offen" : "=v"(dst) : "v"(voff), "s"(rs), "s"(soff) : "memory");
}
__device__ __forceinline__ void req_u8(uint32_t& dst, srd_t rs, uint32_t voff, uint32_t soff) {
    asm volatile("s_nop 4\n\tbuffer_load_ubyte %0, %1, %2, %3 offen" : "=v"(dst) : "v"(voff), "s"(rs), "s"(soff) : "memory");
}
typedef uint32_t u128_t __attribute__((ext_vector_type(4)));
__device__ __forceinline__ void req_u128(u128_t& dst, srd_t rs, uint32_t voff, uint32_t soff) {
    asm volatile("s_nop 4\n\tbuffer_load_dwordx4 %0, %1, %2, %3 offen" : "=v"(dst) : "v"(voff), "s"(rs), "s"(soff) : "memory");
}
// one LDS-DMA piece: 64 lanes x 16 bytes from buffer offset (voff per lane + soff) to LDS [lds_addr, +1024), lane-linear
// (m0 is a RESERVED register of the AMDGPU backend: hipcc never keeps a value in it across statements, it writes m0 right
//  before the few instructions that read it — none of which these kernels contain; `grep m0` on the generated code of the
//  three files that use this helper shows only the moves below.  The clobber is declared anyway; clang warns that clobbers of
//  reserved registers are advisory, hence the pragma.)
#pragma clang diagnostic push
#pragma clang diagnostic ignored "-Winline-asm"
__device__ __forceinline__ void req_lds16(srd_t rs, uint32_t lds_addr, uint32_t voff, uint32_t soff) {
    // m0 is declared clobbered, not saved / restored (two SALU + a 5-cycle nop per piece in the round-2 loops); one wait state
    // between the SALU write of M0 and the LDS-DMA that reads it
    asm volatile("s_mov_b32 m0, %3\n\ts_nop 0\n\tbuffer_load_dwordx4 %0, %1, %2 offen lds"
                 : : "v"(voff), "s"(rs), "s"(soff), "s"(lds_addr) : "memory", "m0");
}
// the same reading around the (non-coherent) L1 / XCD L2: the consumer side of a write-through (sc1) hand-off
__device__ __forceinline__ void req_lds16_sc1(srd_t rs, uint32_t lds_addr, uint32_t voff, uint32_t soff) {
    asm volatile("s_mov_b32 m0, %3\n\ts_nop 0\n\tbuffer_load_dwordx4 %0, %1, %2 offen sc1 lds"
                 : : "v"(voff), "s"(rs), "s"(soff), "s"(lds_addr) : "memory", "m0");
}
// the same with 4 bytes per lane: 64 lanes x 4 bytes to LDS [lds_addr, +256)
__device__ __forceinline__ void req_lds4(srd_t rs, uint32_t lds_addr, uint32_t voff, uint32_t soff) {
    asm volatile("s_mov_b32 m0, %3\n\ts_nop 0\n\tbuffer_load_dword %0, %1, %2 offen lds"
                 : : "v"(voff), "s"(rs), "s"(soff), "s"(lds_addr) : "memory", "m0");
}
#pragma clang diagnostic pop
// K order of the row tiles that share a weight column tile (round 6; gemm_a8w8_sq_kernel has the reasoning).  flags & K_ORDER_ON = on (gl_common.h); group field = 0: row tile
// mt starts at step mt nsteps / mtiles (whole-K rotation); = 1 + log2(G): the K steps form groups of G, and inside every run of mtiles groups row tile mt takes
// them in the order mt, mt + 1, ... — each tile LEADS (pulls HBM-cold lines) on one group of the run and follows its siblings on the others, so the lines only have
// to survive mtiles - 1 groups in L2 instead of a whole rotation.  A tail of fewer than mtiles groups keeps the plain order.
// Everything per step is SCALAR arithmetic (the quotient by mtiles through a multiply-high with a constant set up once): the step offset feeds the soffset operand
// of inline-asm requests, and an SGPR written by v_readfirstlane right in front of them would need wait states nothing inserts.
// The struct also compiles for the HOST (gemlite_hip_k_order_step, api.hip: the tests evaluate the rule the kernels compile, not a restatement of it): the two
// device builtins have host spellings below, chosen by __HIP_DEVICE_COMPILE__ — the device pass sees the same tokens as before.
#if defined(__HIP_DEVICE_COMPILE__)
#define GL_KORDER_UNIFORM(v) __builtin_amdgcn_readfirstlane(v)
#define GL_KORDER_UMULHI(a, b) __umulhi(a, b)
#else
#define GL_KORDER_UNIFORM(v) (v)
#define GL_KORDER_UMULHI(a, b) ((uint32_t)(((uint64_t)(a) * (uint64_t)(b)) >> 32))
#endif
struct KOrder {
    int mode;        // 0 plain, 1 whole-K rotation, 2 grouped
    int rot, nsteps; // whole rotation
    int gsh, P, mt, ngroups;
    uint32_t magic;  // ceil(2^32 / P)
    __host__ __device__ __forceinline__ void init(int mt_, int mtiles, int nsteps_, int flags) {
        mode = 0; rot = 0; nsteps = nsteps_; gsh = 0; P = mtiles; mt = mt_; ngroups = 0; magic = 0u;
        if (!(flags & K_ORDER_ON) || mtiles < 2) return;
        const int gm = (flags >> K_ORDER_GROUP_SHIFT) & 15;
        if (gm == 0) {
            mode = 1;
            rot = GL_KORDER_UNIFORM((mt_ * nsteps_) / mtiles);
        } else {
            mode = 2;
            gsh = gm - 1;
            ngroups = nsteps_ >> gsh;
            magic = (uint32_t)GL_KORDER_UNIFORM((int)(uint32_t)(((1ull << 32) + (uint64_t)mtiles - 1ull) / (uint64_t)mtiles));
        }
    }
    __host__ __device__ __forceinline__ int at(int step) const {
        if (mode == 0) return step;
        if (mode == 1) {
            const int k = step + rot;
            return k >= nsteps ? k - nsteps : k;
        }
        int g = step >> gsh;
        const int i = step & ((1 << gsh) - 1);
        const int base = (int)GL_KORDER_UMULHI((uint32_t)g, magic) * P;  // (g / P) * P: exact while g P < 2^32
        if (base + P <= ngroups) {
            int r = g - base + mt;
            if (r >= P) r -= P;
            g = base + r;
        }
        return (g << gsh) + i;
    }
};
#undef GL_KORDER_UNIFORM
#undef GL_KORDER_UMULHI
template <int N>
__device__ __forceinline__ void wait_vm() { asm volatile("s_waitcnt vmcnt(%0)" ::"n"(N) : "memory"); }
__device__ __forceinline__ void tie(uint32_t& v) { asm volatile("" : "+v"(v)); }
__device__ __forceinline__ uint32_t lds_addr_of(const unsigned char* p) {
    return (uint32_t)(uintptr_t)(const __attribute__((address_space(3))) unsigned char*)p;
}

}  // namespace async

// Round 6 ("GEMV family onto counted asm loads"): the chunk requests of gemv_wn_kernel (and, round 13, of the grouped gemv_w4_decode3_kernel) are inline-asm global loads
// retired with hand-counted s_waitcnt (the head of this file has the reasoning; scripts/isa_asmloads.py replays the generated code).  With the loads
// left to hipcc, every instantiation carried a full `s_waitcnt vmcnt(0)` at the head of its two-chunk loop: the chunk requested a moment
// before was waited for in full before the arithmetic on the OLDER chunk could start — one memory latency per loop iteration with nothing
// overlapped.  Uniform base + 32-bit byte offset per lane, as before.
namespace gvw {
template <bool NT>
__device__ __forceinline__ void gld128(u32x4& d, const char* base, uint32_t voff) {
    if constexpr (NT) asm volatile("global_load_dwordx4 %0, %1, %2 nt" : "=v"(d) : "v"(voff), "s"(base) : "memory");
    else asm volatile("global_load_dwordx4 %0, %1, %2" : "=v"(d) : "v"(voff), "s"(base) : "memory");
}
__device__ __forceinline__ void gld64(u32x2& d, const char* base, uint32_t voff) {
    asm volatile("global_load_dwordx2 %0, %1, %2" : "=v"(d) : "v"(voff), "s"(base) : "memory");
}
__device__ __forceinline__ void gld32(uint32_t& d, const char* base, uint32_t voff) {
    asm volatile("global_load_dword %0, %1, %2" : "=v"(d) : "v"(voff), "s"(base) : "memory");
}
template <int N>
__device__ __forceinline__ void wait_vm() { asm volatile("s_waitcnt vmcnt(%0)" ::"n"(N) : "memory"); }
template <typename T>
__device__ __forceinline__ void tie(T& v) { asm volatile("" : "+v"(v)); }

// Two chunk buffers A / B, one chunk in flight while the other is computed on.  NLC = requests per chunk.  On entry A holds chunk 0 and B
// chunk 1 (requested by the caller, those that exist).  Steady state: unconditional requests, ONE wait value ("everything but the newest
// chunk has landed": loads return in order); the last one to three chunks are peeled, their waits picked by uniform branches.
// `pre(i)` runs in front of the wait for chunk i: what chunk i needs from elsewhere (the shared-x grouped decode kernel: its LDS reads of x)
// is asked for before the wave goes to sleep on the counter.
template <int NLC, typename Buf, typename Issue, typename Tie, typename Pre, typename Compute>
__device__ __forceinline__ void ring2_run_pre(int n, Buf& A, Buf& B, Issue&& issue, Tie&& tie_buf, Pre&& pre, Compute&& compute) {
    int i = 0;
#pragma unroll 1
    for (; i + 4 <= n; i += 2) {
        pre(i);
        wait_vm<NLC>();
        tie_buf(A);
        compute(A, i);
        issue(A, i + 2);
        pre(i + 1);
        wait_vm<NLC>();
        tie_buf(B);
        compute(B, i + 1);
        issue(B, i + 3);
    }
    const int rem = n - i;  // 0 (no chunk at all), 1, 2 or 3
    if (rem >= 1) {
        pre(i);
        if (rem >= 2) wait_vm<NLC>(); else wait_vm<0>();
        tie_buf(A);
        compute(A, i);
        if (rem >= 2) {
            pre(i + 1);
            if (rem == 3) { issue(A, i + 2); wait_vm<NLC>(); } else wait_vm<0>();
            tie_buf(B);
            compute(B, i + 1);
            if (rem == 3) {
                pre(i + 2);
                wait_vm<0>();
                tie_buf(A);
                compute(A, i + 2);
            }
        }
    }
}
template <int NLC, typename Buf, typename Issue, typename Tie, typename Compute>
__device__ __forceinline__ void ring2_run(int n, Buf& A, Buf& B, Issue&& issue, Tie&& tie_buf, Compute&& compute) {
    ring2_run_pre<NLC>(n, A, B, issue, tie_buf, [](int) {}, compute);
}
}  // namespace gvw

}  // namespace gl
