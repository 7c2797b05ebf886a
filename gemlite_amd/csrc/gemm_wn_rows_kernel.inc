// gemm_wn_rows_kernel.inc — the body of gemm_w4_rows_kernel (gemm_wn_rows.hip has the description), included once per form:
//   GL_ROWS5_KERNEL = gemm_w4_rows_kernel,      GL_ROWS5_BIAS = 0: the kernel as it always was, token for token
//   GL_ROWS5_KERNEL = gemm_w4_rows_bias_kernel, GL_ROWS5_BIAS = 1: one more argument (behind the preloaded dwords) and the bias add in the epilogue
//   GL_ROWS5_GROUP = 1 (gemm_wn_rows_group.hip: gemm_w4_rows_group_kernel / gemm_w4_rows_bias_group_kernel): the GROUPED forms — grid (tiles,
//       members), block (tile, y) computes member y's tile.  Member 0's pointers are the preloaded dwords, members 1 .. come from the by-value
//       table behind the scalars (gl_common.h: GroupTable<biased>), selected by blockIdx.y — uniform, so scalar loads, once
//       per wave and in front of the first request.  Everything behind the selection is the single-layer body; the row blocks along grid.y
//       are compiled out (launches with row blocks never group).  GL_ROWS5_GROUP undefined or 0: the two forms above, token for token.
//   GL_ROWS5_EXPERTS = 1 (gemm_wn_rows_experts.hip: gemm_w4_rows_experts_kernel / gemm_w4_rows_bias_experts_kernel): the EXPERTS forms — grid
//       (tiles, Bmax), block (tile, b) computes work block b of the table experts_route_kernel wrote (gl_common.h: ExpertsRowsTail): up to
//       16 MT slots of ONE expert.  The block leaves at once if b is beyond the used count; the expert's bases are 64-bit scalar arithmetic
//       (as dec3::expert_bases); row r of the block is the x row of slot block_rows[b][r] (GATHER: the source offset of the LDS-DMA
//       request; a -1 entry takes the out-of-range offset and reads zeros like the rows >= M of the other forms) and is stored at that
//       slot's output row (SCATTER); a block of the invalid bucket stores zeros.  Everything between is the single-layer body, and a row
//       of the MFMA result depends on no other row: a slot is bit-identical to its row of the single-layer form.  Undefined or 0: the
//       forms above, token for token.
//   GL_ROWS5_EXPERTS_GLU = 1 on top of GL_ROWS5_EXPERTS (gemm_wn_rows_experts_glu.hip: gemm_w4_rows_experts_glu_kernel /
//       gemm_w4_rows_bias_experts_glu_kernel), instantiated with NT = 2: the experts form with SwiGLU in its epilogue — grid (I / 16, Bmax),
//       I = N / 2; block (t, b) computes tile t (gate, columns [0, I)) and tile t + I / 16 (up) of work block b.  The body is the NT = 2 body
//       whose second tile lies half_tiles tiles further instead of adjacent (GL_ROWS5_COL0 / _W_NEXT / _M_NEXT below, and + I elements
//       in the bias); requests per chunk, wait counts, LDS layout and the x gather are those of NT = 2, a piece of x read from LDS feeds
//       both tiles, and the MFMA / fold sequence of a tile is that of NT = 1.  Behind the 8-wave sum one thread holds the gate pair and
//       the up pair of (row, column pair): each is rounded as the experts form rounds it (bias included), then from_float(silu(g16) *
//       u16) — fp32, one rounding — goes to the slot's I-wide row; a block of the invalid bucket stores I zeros per slot.  Undefined
//       or 0: the forms above, token for token (the three macros expand to what stood in their place).
#if defined(GL_ROWS5_GROUP) && GL_ROWS5_GROUP
#define GL_ROWS5_GROUPED 1
#else
#define GL_ROWS5_GROUPED 0
#endif
#if defined(GL_ROWS5_EXPERTS) && GL_ROWS5_EXPERTS
#define GL_ROWS5_EXP 1
#else
#define GL_ROWS5_EXP 0
#endif
#if defined(GL_ROWS5_EXPERTS_GLU) && GL_ROWS5_EXPERTS_GLU
#if !GL_ROWS5_EXP
#error "GL_ROWS5_EXPERTS_GLU is a form of GL_ROWS5_EXPERTS"
#endif
#define GL_ROWS5_GLU 1
#define GL_ROWS5_OUT_COLS TC                         // output columns of a block
#define GL_ROWS5_COL0 (tile * TC)                    // first column of the block's first tile (weights, metadata, bias, output)
#define GL_ROWS5_W_NEXT(n) ((uint32_t)(n) * glu_w4)  // bytes from the first tile to tile n inside a packed row
#define GL_ROWS5_M_NEXT(n) ((uint32_t)(n) * glu_m2)  // ... inside a metadata row
#else
#define GL_ROWS5_GLU 0
#define GL_ROWS5_OUT_COLS TCN
#define GL_ROWS5_COL0 (tile * TCN)
#define GL_ROWS5_W_NEXT(n) ((uint32_t)(n * 64))
#define GL_ROWS5_M_NEXT(n) ((uint32_t)(n * 32))
#endif
#if GL_ROWS5_GLU
#define GL_ROWS5_BIAS_PARAM , const ExpertsRowsGluTail gtail
#elif GL_ROWS5_EXP
#define GL_ROWS5_BIAS_PARAM , const ExpertsRowsTail tail
#elif GL_ROWS5_GROUPED
#define GL_ROWS5_BIAS_PARAM , const GroupTable<GL_ROWS5_BIAS != 0> tab
#elif GL_ROWS5_BIAS
#define GL_ROWS5_BIAS_PARAM , const uint16_t* bias
#else
#define GL_ROWS5_BIAS_PARAM
#endif

template <typename Tag, int MT, int SPG, int NT = 1, int BITS = 4>
__global__ __launch_bounds__(rows5::NW * 64, 1) void GL_ROWS5_KERNEL(const char* wb, const char* xb, const char* sp, const char* zp, uint16_t* out,
                                                                      uint32_t sw4, uint32_t mstride2, int nch_total, uint32_t modes,
                                                                      int M, uint32_t sxm2, uint32_t som GL_ROWS5_BIAS_PARAM) {
    using namespace rows5;
    using TR = F16Traits<Tag>;
    constexpr int CHUNK = 32, TC = 16, TCN = TC * NT, CSTRIDE = NW * CHUNK;  // packed rows per chunk (256 k), tile columns, block columns
    constexpr int E = 32 / BITS, KS = E;                      // k-values per packed row; MFMA k-steps (32 k) per chunk
    constexpr int KCH = 32 * E;                               // k per chunk: 256 (4-bit) / 512 (2-bit)
    constexpr int NG = KS / SPG;                              // quantisation groups per chunk (group sizes above the chunk repeat their row)
    constexpr int NML = (NG + 3) / 4;                         // metadata loads per chunk and kind (scales / zeros), each 4 groups x 16 columns
    constexpr int XK = MT == 1 ? 256 : (MT == 2 ? 128 : 64);  // k per x piece
    constexpr int NP = KCH / XK;                              // x pieces per chunk
    constexpr int SPP = XK / 32;                              // MFMA k-steps per piece
    constexpr int PPR = XK / 8;                               // 16-byte slots per row of a piece
    constexpr int RPI = 64 / PPR;                             // rows per LDS-DMA instruction (1 KiB)
    constexpr int DPI = 16 * MT / RPI;                        // LDS-DMA instructions per piece
    constexpr int NWM = NT * (2 + 2 * NML);                   // requests of one chunk's weights + metadata
    constexpr int NS = 2;                                     // weight register sets = chunks the weight requests run ahead.  (4 sets — 64 KB per CU in
                                                              // flight like the decode kernel — measured SLOWER: a wave's requests return in order, so every
                                                              // x piece then waits behind more HBM round trips; 4096 x 8192 M = 8: 9.4 -> 10.7 us)
    static_assert((BITS == 4 || BITS == 2) && NG >= 2 && DPI * 1024 <= XBUF && (WSLOT_I1 + 256) * 4 <= WSLOT_BYTES && MT * NT * 1024 <= XBUF, "LDS layout");
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];

    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    int tile = blockIdx.x;
    if (NT == 1 && (modes & M_PAIR)) {  // adjacent half-line tiles on one XCD (speed only; any mapping is correct)
        const int xcd = tile & 7, idx = tile >> 3;
        tile = (((idx >> 1) << 3) + xcd) * 2 + (idx & 1);
    }
#if GL_ROWS5_GLU
    static_assert(NT == 2, "a gate tile and an up tile");
    const ExpertsRowsTail& tail = gtail.rows;
    const uint32_t glu_w4 = gtail.half_tiles * 64u, glu_m2 = gtail.half_tiles * 32u;
#endif
#if GL_ROWS5_EXP
    // this block's work block: beyond the used count -> nothing to do (uniform, in front of any address arithmetic)
    const int32_t* const wtab = tail.table;
    if ((int)blockIdx.y >= wtab[0]) return;
    const uint32_t expert = (uint32_t)wtab[EXPERTS_ROWS_HEADER + blockIdx.y];
    const int32_t* const brow = wtab + EXPERTS_ROWS_HEADER + gridDim.y + (size_t)blockIdx.y * (16 * MT);  // the block's 16 MT slots, -1 = none
    M = 16 * MT;
    if (expert >= tail.n_experts) {  // the invalid bucket: zeros to this tile of its slots, nothing is dereferenced
        for (int o = tid; o < MT * 16 * (GL_ROWS5_OUT_COLS / 2); o += NW * 64) {
            const int m = o / (GL_ROWS5_OUT_COLS / 2), cp = o % (GL_ROWS5_OUT_COLS / 2);
            const int slot = brow[m];
            if ((uint32_t)slot < tail.n_slots) *(uint32_t*)(out + (size_t)slot * som + (size_t)(GL_ROWS5_COL0 + cp * 2)) = 0u;
        }
        return;
    }
    // the expert's bases: 64-bit scalar arithmetic, the offsets inside an expert stay 32-bit (one scalar zero is shared by all experts)
    wb += (uint64_t)expert * (uint64_t)tail.stride_w;
    sp += (uint64_t)expert * (uint64_t)tail.stride_meta;
    if (!(modes & M_ZSCALAR)) zp += (uint64_t)expert * (uint64_t)tail.stride_meta;
#if GL_ROWS5_BIAS
    const uint16_t* bias = (const uint16_t*)((const char*)tail.bias + (uint64_t)expert * (uint64_t)tail.stride_bias);
#endif
#elif GL_ROWS5_GROUPED
    // this block's member: the preloaded scalars (member 0) or the by-value table — blockIdx.y is uniform, so these are scalar loads
    const int member = (int)blockIdx.y;
    if (member > 0) {
        const GroupMember& mb = tab.m[member - 1];
        wb = mb.w; xb = mb.x; sp = mb.s; zp = mb.z; out = mb.out;
    }
#if GL_ROWS5_BIAS
    const uint16_t* bias = tab.bias[member];
#endif
#else
    // more than 16 MT rows (shapes no tile kernel takes — groups of 32, N % 64 != 0 — at prefill sizes): blocks along grid.y, 16 MT rows each
    if (gridDim.y > 1) {
        const uint32_t m0 = blockIdx.y * (uint32_t)(16 * MT);
        xb += (size_t)m0 * sxm2;
        out += (size_t)m0 * som;
        M -= (int)m0;
    }
#endif
    if (M > 16 * MT) M = 16 * MT;
    const int c = lane & 3, g = lane >> 2;    // role in the weight request
    const int j = lane & 15, kb = lane >> 4;  // role in the MFMA: column j / row j of a tile, 8-k block kb of the 32-k step
    const int nchunks = (nch_total - wave + NW - 1) / NW;
    const int npieces = nchunks * NP;
    const int w_mode = (int)(modes & 15u), gs_shift = (int)((modes >> 8) & 255u);
    const bool need_s = w_mode >= 2, need_z = (w_mode == 1 || w_mode >= 3) && !(modes & M_ZSCALAR);

    unsigned char* wl = smem + (size_t)wave * WAVE_LDS;  // this wave's LDS: [x buffer 0][x buffer 1][weight slot]
    uint32_t* wslot = (uint32_t*)(wl + 2 * XBUF);
    // weight slot, write side: packed row 2g + i of the chunk at dword (i ? WSLOT_I1 : 0) + 16 g + 4 c (a fixed i makes 8 lanes = 128 contiguous
    // bytes); read side: row 4 s + kb = 2 (2 s + (kb >> 1)) + (kb & 1) -> dword (kb & 1) WSLOT_I1 + 32 s + 16 (kb >> 1) + j: the 32 lanes of a
    // ds_read_b32 half (kb = 0, 1 or 2, 3) land on banks j and 16 + j
    const int wr_off = g * 16 + c * 4;
    const int rd_off = BITS == 4 ? (kb & 1) * WSLOT_I1 + (kb >> 1) * 16 + j   // row 4 s + kb: + 32 s
                                 : (kb >> 1) * WSLOT_I1 + j;                  // 2-bit: row 2 s + (kb >> 1): + 16 s (kb = 2 m, 2 m + 1 read the same dword)
    const uint32_t half_sh = (uint32_t)(kb & 1) * 16u;                        // 2-bit: which half of that word
    const uint32_t wo0 = (uint32_t)(wave * CHUNK + g * 2) * sw4 + (uint32_t)(GL_ROWS5_COL0 + c * 4) * 4u;  // (+ 64 bytes per further column tile)

    // ---- x pieces: LDS slot (row r, 16-byte slot p') of a buffer holds piece p = p' ^ f(r) of the row; DMA instruction q fills rows
    //      q RPI .. q RPI + RPI - 1 lane-linearly.  f: the low bits of r that separate the rows one ds_read_b128 lane group touches
    auto fswz = [](int r) { return PPR >= 16 ? (r & 15) : ((r >> 1) & 7); };
    uint32_t xvo[DPI];  // per-lane source byte offset of DMA instruction q (k offset of the piece added per request); rows >= M: out of range -> zeros
#pragma unroll
    for (int q = 0; q < DPI; ++q) {
        const int r = q * RPI + lane / PPR, pp = lane % PPR;
#if GL_ROWS5_EXP
        const int slot = brow[r];  // gather: the x row of the slot (the descriptor covers all of x, its extent is below 2^31)
        xvo[q] = (uint32_t)slot < tail.n_slots ? ((uint32_t)slot / tail.slots_per_x_row) * sxm2 + (uint32_t)((pp ^ fswz(r)) * 16) : 0x80000000u;
#else
        xvo[q] = r < M ? (uint32_t)r * sxm2 + (uint32_t)((pp ^ fswz(r)) * 16) : 0x80000000u;
#endif
    }
#if GL_ROWS5_EXP
    const async::srd_t rsX = async::make_srd(xb, tail.x_bytes);
#else
    const async::srd_t rsX = async::make_srd(xb, (uint32_t)(M - 1) * sxm2 + (uint32_t)nch_total * (uint32_t)(KCH * 2));
#endif
    const uint32_t xlds = async::lds_addr_of(wl);
    uint32_t abase[MT];  // byte offset of this lane's A fragment (k-step 0 of a piece) inside a buffer; k-step s' = abase ^ (s' << 6)
#pragma unroll
    for (int t = 0; t < MT; ++t) {
        const int r = t * 16 + j;
        abase[t] = (uint32_t)(r * PPR * 16 + ((kb ^ fswz(r)) << 4));
    }
    // piece i of the wave = (chunk i / NP, part i % NP): its first k as a byte offset inside a row of x
    auto issue_x = [&](int i, int par) {
        const uint32_t koff = (uint32_t)(((i / NP) * CSTRIDE + wave * CHUNK) * E + (i % NP) * XK) * 2u;
#pragma unroll
        for (int q = 0; q < DPI; ++q) async::req_lds16(rsX, xlds + (uint32_t)(par * XBUF + q * 1024), xvo[q] + koff, 0u);
    };

    // ---- weights + metadata of a chunk: lane (j, kb) loads the scale and the zero of group 4 l + kb of the chunk, column j (uniform base +
    //      32-bit lane offset: no 64-bit address arithmetic between the requests; absent metadata is still "loaded" — from the weight buffer,
    //      always in bounds — so the loop stays branch-free)
    const char* sbase = need_s ? sp : wb;
    const char* zbase = need_z ? zp : wb;
    const uint32_t mcol = (uint32_t)(GL_ROWS5_COL0 + j) * 2u;  // (+ 32 bytes per further column tile)
    struct WSet { u32x4 w0[NT], w1[NT]; uint32_t s[NT][NML], z[NT][NML]; };
    auto issue_w = [&](WSet& S, int ch) {
        const uint32_t wo = wo0 + (uint32_t)(ch * CSTRIDE) * sw4;
#pragma unroll
        for (int n = 0; n < NT; ++n) {
            gld128_nt(S.w0[n], wb, wo + GL_ROWS5_W_NEXT(n));
            gld128_nt(S.w1[n], wb, wo + sw4 + GL_ROWS5_W_NEXT(n));
        }
        const uint32_t k0 = (uint32_t)(ch * CSTRIDE + wave * CHUNK) * (uint32_t)E;
#pragma unroll
        for (int n = 0; n < NT; ++n)
#pragma unroll
            for (int l = 0; l < NML; ++l) {
                const int gq = 4 * l + kb < NG ? 4 * l + kb : NG - 1;
                const uint32_t mo = ((k0 + (uint32_t)(gq * 32 * SPG)) >> gs_shift) * mstride2 + mcol + GL_ROWS5_M_NEXT(n);
                gld16(S.s[n][l], sbase, need_s ? mo : 0u);
                gld16(S.z[n][l], zbase, need_z ? mo : 0u);
            }
    };
    // everything but the newest `newer` requests of this wave has landed; newer is wave-uniform and one of four values
    auto wait_newer = [&](bool w_behind, bool x_behind) {
        if (w_behind) { if (x_behind) wait_vm<NWM + DPI>(); else wait_vm<NWM>(); }
        else          { if (x_behind) wait_vm<DPI>(); else wait_vm<0>(); }
    };

    f32x4 tot[MT][NT];
#pragma unroll
    for (int t = 0; t < MT; ++t)
#pragma unroll
        for (int n = 0; n < NT; ++n) tot[t][n] = (f32x4){0.f, 0.f, 0.f, 0.f};
    const float scalar_zero = (modes & M_ZSCALAR) ? (float)((const int32_t*)zp)[0] : 0.f;
    const float bz = (w_mode == 1 || w_mode == 3) ? -1.f : (w_mode == 4 ? 1.f : 0.f);
    const bool b_times_s = w_mode == 3;
    const u32x4 onesb = {TR::ONES2, TR::ONES2, TR::ONES2, TR::ONES2};

    // One chunk.  CPAR = chunk parity (which of the two register sets and — for one piece per chunk — which x buffer).  Request queue of the
    // wave, oldest first:
    //     W(0) X(0) W(1) X(1) | end of piece i:  X(i + 2)  [W(c + 2) if i closed chunk c]            (each only if it exists)
    // so behind X(i) sit [X(i + 1)] and [W(c + 1) if i opens chunk c] — x first: a wave's requests return in order, and a piece
    // must not wait behind the HBM round trip of the weights requested with it (4096 x 11008, M = 8: 12.7 -> 11.4 us).
    auto chunk = [&](WSet& S, int ch, auto cpar) {
        constexpr int CPAR = decltype(cpar)::value;
        uint32_t bw[NT][KS];
        f32x4 acc[MT][NT], ones[MT];
#pragma unroll
        for (int pi = 0; pi < NP; ++pi) {
            const int i = ch * NP + pi;
            const int par = ((NP & 1) ? CPAR : 0) ^ (pi & 1);
            wait_newer(pi == 0 && ch + 1 < nchunks, i + 1 < npieces);
            if (pi == 0) {  // the wave's 2 KB of weights: registers -> own LDS slot -> MFMA layout
#pragma unroll
                for (int n = 0; n < NT; ++n) {
                    tie4(S.w0[n]);
                    tie4(S.w1[n]);
#pragma unroll
                    for (int l = 0; l < NML; ++l) {
                        tie1(S.s[n][l]);
                        tie1(S.z[n][l]);
                    }
                }
#pragma unroll
                for (int n = 0; n < NT; ++n) {  // (one slot, tile after tile: the DS operations of a wave execute in order)
                    *(u32x4*)(wslot + wr_off) = S.w0[n];
                    *(u32x4*)(wslot + WSLOT_I1 + wr_off) = S.w1[n];
#pragma unroll
                    for (int s = 0; s < KS; ++s) bw[n][s] = wslot[rd_off + s * (BITS == 4 ? 32 : 16)];
                }
            }
            const unsigned char* xbuf = wl + par * XBUF;
#pragma unroll
            for (int sq = 0; sq < SPP; ++sq) {
                const int s = pi * SPP + sq;
                u32x4 bf[NT];
#pragma unroll
                for (int n = 0; n < NT; ++n) {
                    uint32_t wv = bw[n][s];
                    if constexpr (BITS == 2) {  // this lane's 16-bit half -> eight nibbles (q0 .. q7 in the low two bits of each)
                        wv = (wv >> half_sh) & 0xFFFFu;
                        wv = (wv | (wv << 8)) & 0x00FF00FFu;
                        wv = (wv | (wv << 4)) & 0x0F0F0F0Fu;
                        wv = (wv | (wv << 2)) & 0x33333333u;
                    }
                    const uint32_t t_lo = wv & 0x0F0F0F0Fu, t_hi = (wv >> 4) & 0x0F0F0F0Fu;
#pragma unroll
                    for (int pq = 0; pq < 4; ++pq) bf[n][pq] = __builtin_amdgcn_perm(t_hi, t_lo, 0x0C040C00u + (uint32_t)pq * 0x00010001u) | TR::MAGIC2;
                }
                const bool first = s % SPG == 0;
#pragma unroll
                for (int t = 0; t < MT; ++t) {
                    const u32x4 a = *(const u32x4*)(xbuf + (abase[t] ^ (uint32_t)(sq << 6)));
#pragma unroll
                    for (int n = 0; n < NT; ++n) acc[t][n] = mfma16<Tag>(a, bf[n], first ? (f32x4){0.f, 0.f, 0.f, 0.f} : acc[t][n]);
                    ones[t] = mfma16<Tag>(a, onesb, first ? (f32x4){0.f, 0.f, 0.f, 0.f} : ones[t]);
                }
                if ((s + 1) % SPG == 0) {  // end of a quantisation group: fold scale / zero into the totals
                    const int q = s / SPG, l = q >> 2, gq = q & 3;  // group q of the chunk: loaded by the lanes kb = gq of load l
#pragma unroll
                    for (int n = 0; n < NT; ++n) {
                        const uint32_t sraw = (uint32_t)__builtin_amdgcn_ds_bpermute((j + 16 * gq) * 4, (int)S.s[n][l]);
                        const uint32_t zraw = (uint32_t)__builtin_amdgcn_ds_bpermute((j + 16 * gq) * 4, (int)S.z[n][l]);
                        const float sv = need_s ? TR::to_float((uint16_t)sraw) : 1.f;
                        const float zv = need_z ? TR::to_float((uint16_t)zraw) : scalar_zero;
                        const float a = sv;
                        const float b = bz * zv * (b_times_s ? sv : 1.f) - a * TR::OFF;
#pragma unroll
                        for (int t = 0; t < MT; ++t)
#pragma unroll
                            for (int r = 0; r < 4; ++r) tot[t][n][r] += a * acc[t][n][r] + b * ones[t][r];
                    }
                }
            }
            // the buffer is free once this wave's reads of it have returned; then the requests two pieces / two chunks ahead
            wait_lgkm0();
            if (i + 2 < npieces) issue_x(i + 2, par);
            if (pi == NP - 1 && ch + NS < nchunks) issue_w(S, ch + NS);
        }
    };

    WSet W[NS];
    if (nchunks > 0) issue_w(W[0], 0);
    if (npieces > 0) issue_x(0, 0);
    if (nchunks > 1) issue_w(W[1], 1);
    if (npieces > 1) issue_x(1, 1);
#pragma unroll 1
    for (int ch = 0; ch < nchunks; ch += NS) {
        chunk(W[0], ch, std::integral_constant<int, 0>{});
        if (ch + 1 < nchunks) chunk(W[1], ch + 1, std::integral_constant<int, 1>{});
        if constexpr (NS == 4) {
            if (ch + 2 < nchunks) chunk(W[2], ch + 2, std::integral_constant<int, 0>{});
            if (ch + 3 < nchunks) chunk(W[3], ch + 3, std::integral_constant<int, 1>{});
        }
    }

    // ---- the 8 waves (disjoint K) meet in LDS: [MT x 16 rows][16 NT columns] fp32 at the start of each wave's region; C layout: column j,
    //      rows 4 kb + r ------------------------------------------------------------------------------------------------------------------
    float* part = (float*)wl;
#pragma unroll
    for (int t = 0; t < MT; ++t)
#pragma unroll
        for (int n = 0; n < NT; ++n)
#pragma unroll
            for (int r = 0; r < 4; ++r) part[(t * 16 + 4 * kb + r) * TCN + n * TC + j] = tot[t][n][r];
    __syncthreads();
#if GL_ROWS5_GLU
    constexpr int CPR = TC / 2;                // pairs of adjacent OUTPUT columns per row of the block
    constexpr int NPAIR = MT * 16 * CPR;
    for (int o = tid; o < NPAIR; o += NW * 64) {
        const int m = o / CPR, cp = o % CPR;
        float g0 = 0.f, g1 = 0.f, u0 = 0.f, u1 = 0.f;  // the sums of the experts form, pair by pair: gate at column cp * 2, up TC further
#pragma unroll
        for (int w = 0; w < NW; ++w) {
            const float2 pg = *(const float2*)(smem + (size_t)w * WAVE_LDS + (size_t)(m * TCN + cp * 2) * 4);
            const float2 pu = *(const float2*)(smem + (size_t)w * WAVE_LDS + (size_t)(m * TCN + TC + cp * 2) * 4);
            g0 += pg.x;
            g1 += pg.y;
            u0 += pu.x;
            u1 += pu.y;
        }
        uint16_t hg0 = TR::from_float(g0), hg1 = TR::from_float(g1), hu0 = TR::from_float(u0), hu1 = TR::from_float(u1);
#if GL_ROWS5_BIAS
        // (the two roundings of "matmul, then out += bias", as the experts form has them)
        const uint16_t* bp = bias + (size_t)(GL_ROWS5_COL0 + cp * 2);
        const uint32_t glu_i = gtail.half_tiles * 16u;  // the up half of the bias lies I elements further
        hg0 = TR::from_float(TR::to_float(hg0) + TR::to_float(bp[0]));
        hg1 = TR::from_float(TR::to_float(hg1) + TR::to_float(bp[1]));
        hu0 = TR::from_float(TR::to_float(hu0) + TR::to_float(bp[glu_i]));
        hu1 = TR::from_float(TR::to_float(hu1) + TR::to_float(bp[glu_i + 1]));
#endif
        const uint16_t h0 = TR::from_float(silu_f32(TR::to_float(hg0)) * TR::to_float(hu0));
        const uint16_t h1 = TR::from_float(silu_f32(TR::to_float(hg1)) * TR::to_float(hu1));
        const int oslot = brow[m];  // scatter: the row's slot; nothing is stored for a -1 entry
        if ((uint32_t)oslot < tail.n_slots)
            *(uint32_t*)(out + (size_t)(uint32_t)oslot * som + (size_t)(GL_ROWS5_COL0 + cp * 2)) = (uint32_t)h0 | ((uint32_t)h1 << 16);
    }
#else
    constexpr int CPR = TCN / 2;               // pairs of adjacent columns per row of the block
    constexpr int NPAIR = MT * 16 * CPR;
    for (int o = tid; o < NPAIR; o += NW * 64) {
        const int m = o / CPR, cp = o % CPR;
        float v0 = 0.f, v1 = 0.f;
#pragma unroll
        for (int w = 0; w < NW; ++w) {
            const float2 pv = *(const float2*)(smem + (size_t)w * WAVE_LDS + (size_t)(m * TCN + cp * 2) * 4);
            v0 += pv.x;
            v1 += pv.y;
        }
        if (modes & M_POST) {  // channel scales (channel_scale_mode 1): the kernel's 16-bit type, or fp32 (the BitNet processors' default)
            if (modes & M_POST32) {
                const float2 sw = *(const float2*)(sp + (size_t)(tile * TCN + cp * 2) * 4);
                v0 *= sw.x;
                v1 *= sw.y;
            } else {
                const uint32_t sw = *(const uint32_t*)(sp + (size_t)(tile * TCN + cp * 2) * 2);
                v0 *= TR::to_float((uint16_t)(sw & 0xFFFFu));
                v1 *= TR::to_float((uint16_t)(sw >> 16));
            }
        }
#if GL_ROWS5_EXP
        const int oslot = brow[m];  // scatter: the row's slot; nothing is stored for a -1 entry
        uint16_t* const orow = out + (size_t)(uint32_t)oslot * som;
#define GL_ROWS5_STORE_IF ((uint32_t)oslot < tail.n_slots)
#define GL_ROWS5_OUT_ROW orow
#else
#define GL_ROWS5_STORE_IF (m < M)
#define GL_ROWS5_OUT_ROW (out + (size_t)m * som)
#endif
#if GL_ROWS5_BIAS
        // the ROUNDED result plus bias[n] (the output's 16-bit type, broadcast over the rows), rounded again: the two roundings of "matmul, then
        // out += bias", bit for bit (a sum of two converted values: nothing to contract).  Two 2-byte loads: the bias needs 2-byte alignment only
        const uint16_t* bp = bias + (size_t)(tile * TCN + cp * 2);
        const uint16_t h0 = TR::from_float(TR::to_float(TR::from_float(v0)) + TR::to_float(bp[0]));
        const uint16_t h1 = TR::from_float(TR::to_float(TR::from_float(v1)) + TR::to_float(bp[1]));
        if (GL_ROWS5_STORE_IF) *(uint32_t*)(GL_ROWS5_OUT_ROW + (size_t)(tile * TCN + cp * 2)) = (uint32_t)h0 | ((uint32_t)h1 << 16);
#else
        if (GL_ROWS5_STORE_IF) *(uint32_t*)(GL_ROWS5_OUT_ROW + (size_t)(tile * TCN + cp * 2)) = (uint32_t)TR::from_float(v0) | ((uint32_t)TR::from_float(v1) << 16);
#endif
#undef GL_ROWS5_STORE_IF
#undef GL_ROWS5_OUT_ROW
    }
#endif
}

#undef GL_ROWS5_BIAS_PARAM
#undef GL_ROWS5_GROUPED
#undef GL_ROWS5_EXP
#undef GL_ROWS5_GLU
#undef GL_ROWS5_OUT_COLS
#undef GL_ROWS5_COL0
#undef GL_ROWS5_W_NEXT
#undef GL_ROWS5_M_NEXT
