// Body of the SGEMM kernel (see gemm.hip): everything one workgroup does for one output tile / K-slice.  Included as the
// body of the __global__ kernel sgemm_mfma (LG_TILE_OWNS_LDS = 1, LG_TILE_BID = blockIdx.x) and, once per product, inside
// the two-product kernel sgemm_pair_wgrad_xgrad (LDS declared by the includer, workgroup index relative to the product).
// Textual inclusion, not a call: with the body behind a __device__ function the compiler schedules the K loop differently
// and the N-contiguous-B layouts lose 7 % (measured: 1024^3 NN 79 -> 73 TFLOP/s, the dx GEMM of the MLP 14.9 -> 16.2 us,
// the two-product launch 27.3 -> 25.3 us with the text).
// In scope at the point of inclusion: BM, BN, BK, WM, WN, AKC, BKC, VA, VB, PD, KG, XT (compile-time constants) and `g` (GemmArgs).
// LG_TILE_SIGNAL = 1 (sgemm_bias_head_fwd): the tile's stores are write-through and every storing wavefront, once they are drained,
// adds 1 to the ticket of its ROW of tiles (signal_tickets[tm * signal_stride]); the signal_per_row-th raises the row's flag (16 ints
// further) - workgroups at the end of the same launch wait for it and carry on with the row.
#ifndef LG_TILE_SIGNAL
#define LG_TILE_SIGNAL 0
#endif
// LG_TILE_WAVE_PRIVATE (sgemm_mfma's WP; one wave per K-group, both operands K-contiguous): the K-groups share no operand, so each
// wave runs a K loop of its own on its own BK columns of every K-step - it fetches, stages (a region of LDS nobody else
// touches) and multiplies them, and the loop has no barrier: a wave's LDS operations complete in order, so the
// write of tile kt+2 behind the fragment reads of tile kt+1 needs neither a second buffer nor a wait.  Everything below that
// says "staged together" (NTS threads, BKS k-values) then means one wave and its own BK columns.
#ifndef LG_TILE_WAVE_PRIVATE
#define LG_TILE_WAVE_PRIVATE false
#endif
    constexpr bool WPK = LG_TILE_WAVE_PRIVATE;
    static_assert(!WPK || (KG > 1 && WM * WN == 1 && BM == 32 && BN == 32 && AKC && BKC && VA && VB && XT != 2 && !LG_TILE_SIGNAL), "wave-private K loop: one wave per K-group, NT form");
    constexpr int NT = WM * WN * KG * 64;
    constexpr int NTS = WPK ? 64 : NT;                   // threads that stage one K-tile together
    constexpr int BKS = WPK ? BK : BK * KG;              // k-values staged per K-step
    constexpr int TM = BM / WM / 32, TN = BN / WN / 32;
    static_assert(TM >= 1 && TN >= 1 && BK % 16 == 0 && (KG == 1 || KG == 2 || KG == 4), "tile config");
    // "Gather" staging (round 4, the 256 x 256 tile): an M- / N-contiguous operand is fetched as FOUR single dwords along k per
    // (row, k-quad) - lanes along the row index, so every load instruction still covers 256 contiguous bytes - and written to
    // LDS as ONE 16-byte store into the K-contiguous [row][BK+4] layout.  The transposition happens in the register file for
    // free, and the operand then leaves LDS as ds_read_b128 like a K-contiguous one: the TN product (both operands of this
    // kind, 138 TFLOP/s at 4096^3 with ds_read_b32 fragments) runs the NT product's inner loop (146).
    constexpr bool AG = kGatherStaging<BM, BN, AKC>, BG = kGatherStaging<BM, BN, BKC>;
    static_assert((!AG || VA) && (!BG || VB), "gather staging replaces the float4 form");
    constexpr bool ALK = AKC || AG, BLK = BKC || BG;     // K-contiguous in LDS
    constexpr int A_PITCH = ALK ? BKS + 4 : BM;          // floats per LDS row
    constexpr int B_PITCH = BLK ? BKS + 4 : BN;
    constexpr int A_TILE = ALK ? BM * A_PITCH : BKS * A_PITCH;
    constexpr int B_TILE = BLK ? BN * B_PITCH : BKS * B_PITCH;
    constexpr int A_ELEMS = BM * BKS / NTS, B_ELEMS = BN * BKS / NTS;   // floats staged per thread
    static_assert(A_ELEMS % 4 == 0 && B_ELEMS % 4 == 0, "staging must divide into float4");

    static_assert(WPK || 2 * (A_TILE + B_TILE) == gemm_lds_floats<BM, BN, BK, AKC, BKC, KG>(), "LDS size");
    static_assert(!(AG || BG) || TM * TN > 1, "gather staging: the multi-accumulator loop only");
#if LG_TILE_OWNS_LDS
    __shared__ __attribute__((aligned(16))) float lds[gemm_lds_floats<BM, BN, BK, AKC, BKC, KG>()];
#endif
    // buffer b: A tile at lds + b*(A_TILE+B_TILE), B tile right behind it
    constexpr int BUF = A_TILE + B_TILE;

    const int tid = threadIdx.x;
    const int lane = tid & 63, wave = tid >> 6;
    // (wave-private loop: the K-group picks the wave's K range, descriptors and trip count - scalar values)
    const int kg = WPK ? __builtin_amdgcn_readfirstlane(wave) : wave / (WM * WN), wl = wave % (WM * WN);          // K-group of this wave, wave inside the group
    const int wm = wl / WN, wn = wl % WN;
    const int kofs = WPK ? 0 : kg * BK;                              // its k offset inside a staged K-step
    const int stid = WPK ? lane : tid;                               // index among the threads that stage a tile together
    float* const ldsw = WPK ? lds + kg * BUF : lds;                  // wave-private loop: ONE buffer per wave, its own
    const int r = lane & 31, h = lane >> 5;
    LG_TL(0);                                        // workgroup entered

    // tile coordinates
    const int id = xcd_remap(LG_TILE_BID, g.nwg);
    const int per_batch = g.tiles_m * g.tiles_n;
    const int bs = g.div_per_batch.div(id);        // (batch, k-slice) pair
    const int batch = g.div_slices.div(bs), slice = bs - batch * g.k_slices;
    const int t = id - bs * per_batch;
    // grouped order: consecutive ids walk GROUP_M tile rows before moving to the next tile column, so the
    // ~64 workgroups resident on one XCD at a time cover a near-square patch of C and share both their
    // A row-panels and their B column-panels in that XCD's 4 MiB L2
    const int GROUP_M = g.group_m;
    const int gspan = GROUP_M * g.tiles_n;
    const int group = g.div_gspan.div(t);
    const int first_m = group * GROUP_M, in_group = t - group * gspan;
    const bool last_group = g.tiles_m - first_m < GROUP_M;
    const int gsize = last_group ? g.tiles_m - first_m : GROUP_M;
    const int tn = last_group ? g.div_last_group.div(in_group) : g.div_group.div(in_group);
    const int tm = first_m + (in_group - tn * gsize);
    const int64_t m0 = int64_t(tm) * BM, n0 = int64_t(tn) * BN;
    const int b_outer = g.div_batch_inner.div(batch), b_inner = batch - b_outer * g.batch_inner;
    const float* __restrict__ A = g.A + int64_t(b_outer) * g.sA + int64_t(b_inner) * g.sA2;
    const float* Bp = g.B + int64_t(b_outer) * g.sB + int64_t(b_inner) * g.sB2;
    float* Cp = g.C + int64_t(b_outer) * g.sC + int64_t(b_inner) * g.sC2;
    const float* biasp = g.bias;
    if constexpr (XT == 1) {
        {
            // three products on one op(A) (lg_gemm_multi3_f32): operand offsets by product
            Bp += batch == 0 ? g.boff[0] : batch == 1 ? g.boff[1] : g.boff[2];
            Cp += batch == 0 ? g.coff[0] : batch == 1 ? g.coff[1] : g.coff[2];
            if (biasp) biasp += batch == 0 ? g.biasoff[0] : batch == 1 ? g.biasoff[1] : g.biasoff[2];
        }
    }
    const float* __restrict__ B = Bp;
    float* __restrict__ C = Cp;
    const int64_t ldc = g.ldc;
    const int accumulate = g.accumulate;
    const float* __restrict__ bias = biasp;
    const int64_t k_begin = int64_t(slice) * g.k_per_slice;
    const int64_t k_end = (k_begin + g.k_per_slice < g.K) ? k_begin + g.k_per_slice : g.K;
    // the virtual ones-column (row sums of A) lives in column N of this workgroup's tile, if at all
    const bool has_virtual = kHasExtras<BM, BN> && g.rowsum != nullptr && n0 <= g.N && g.N < n0 + BN;

    // staging registers: a ring of PD K-tiles in flight between global memory and LDS (PD = 1: the tile fetched at the
    // top of an iteration is written to LDS in its middle; small tiles have too few MFMAs per K-tile to cover the
    // load latency that way and run PD = 2..3)
    using StageA = std::conditional_t<VA, f32x4, float>;
    using StageB = std::conditional_t<VB, f32x4, float>;
    constexpr int A_CHUNKS = VA ? A_ELEMS / 4 : A_ELEMS, B_CHUNKS = VB ? B_ELEMS / 4 : B_ELEMS;
    constexpr int NL = (kGatherStaging<BM, BN, AKC> ? 4 : 1) * A_CHUNKS + (kGatherStaging<BM, BN, BKC> ? 4 : 1) * B_CHUNKS;      // loads per thread and K-tile
    static_assert((PD - 1) * NL + NL <= 63, "vmcnt is a 6-bit counter");
    StageA ra_ring[PD][A_CHUNKS];
    StageB rb_ring[PD][B_CHUNKS];
    // gather staging: four separately loaded dwords per chunk (an inline-asm load cannot target one element of a vector)
    [[maybe_unused]] float ga_ring[PD][AG ? A_CHUNKS : 1][4];
    [[maybe_unused]] float gb_ring[PD][BG ? B_CHUNKS : 1][4];

    // Global -> register staging through buffer loads: the descriptor starts at the K-tile's first element (wave-uniform),
    // the per-thread byte offsets are loop invariant, and every predicate (row / column beyond the matrix, k beyond the
    // slice) turns the offset into one past the descriptor's range, for which the hardware returns 0 - no branches and
    // no zero-fill moves in the K loop.
    constexpr unsigned OOB = 0x80000000u;            // == num_records
    // Chunk i of a thread is chunk 0 moved by a COMPILE-TIME number of tile rows (K-contiguous staging) or k-rows (the other
    // kind): flat index f = tid + i * NT, and NT is a multiple of the chunks per row.  Written out that way - `(tid + i * NT) / D`
    // is not folded by the compiler - so that the per-chunk LDS addresses are one register + an immediate and the k coordinate
    // needs one register per operand: the 256 x 256 tile (128 registers per lane, 64 of them accumulators) kept four LDS
    // addresses and four k coordinates apart and spilled 9-11 registers into its K loop (VERDICT r3).
    constexpr int A_W = VA ? 4 : 1, B_W = VB ? 4 : 1;
    constexpr int A_DIV = AG ? BM : (AKC ? BKS : BM) / A_W, B_DIV = BG ? BN : (BKC ? BKS : BN) / B_W;   // chunks per staged row (gather: per k-quad)
    static_assert(NTS % A_DIV == 0 && NTS % B_DIV == 0, "a thread's chunks must differ by whole rows");
    constexpr int A_STEP = NTS / A_DIV, B_STEP = NTS / B_DIV;                               // rows (k-rows, k-quads) between a thread's chunks
    const int a_q = stid / A_DIV, a_r = AG ? stid % A_DIV : (stid % A_DIV) * A_W;            // AKC: (row, k)   gather: (k-quad, row)   else: (k, row)
    const int b_q = stid / B_DIV, b_r = BG ? stid % B_DIV : (stid % B_DIV) * B_W;            // BKC: (col, k)   gather: (k-quad, col)   else: (k, col)
    auto kcA = [&](int i) { return AG ? 4 * (a_q + i * A_STEP) : (AKC ? a_r : a_q + i * A_STEP); };   // k coordinate of chunk i inside its K-tile
    auto kcB = [&](int i) { return BG ? 4 * (b_q + i * B_STEP) : (BKC ? b_r : b_q + i * B_STEP); };
    // LDS position of chunk 0 and the (compile-time) distance to the thread's next chunk
    const int a_lds0 = AG ? a_r * A_PITCH + 4 * a_q : a_q * A_PITCH + a_r, b_lds0 = BG ? b_r * B_PITCH + 4 * b_q : b_q * B_PITCH + b_r;
    constexpr int A_LDS_STEP = AG ? 4 * A_STEP : A_STEP * A_PITCH, B_LDS_STEP = BG ? 4 * B_STEP : B_STEP * B_PITCH;
    unsigned offA[A_CHUNKS], offB[B_CHUNKS];
    unsigned virt_mask = 0;                          // B chunks of this thread that start at the virtual column
    int krem_ring[PD];                               // k extent of the tile waiting in each ring slot
#pragma unroll
    for (int i = 0; i < A_CHUNKS; ++i) {
        const int row = AKC ? a_q + i * A_STEP : a_r, kk = kcA(i);     // row: index along M inside the tile, kk: index along K
        // 32-bit on purpose: the host guarantees that a tile's farthest byte offset is below 2^31
        const unsigned bytes = AKC ? (unsigned(row) * unsigned(g.lda) + unsigned(kk)) * 4u : (unsigned(kk) * unsigned(g.lda) + unsigned(row)) * 4u;
        offA[i] = (m0 + row < g.M) ? bytes : OOB;
    }
#pragma unroll
    for (int i = 0; i < B_CHUNKS; ++i) {
        const int col = BKC ? b_q + i * B_STEP : b_r, kk = kcB(i);
        const unsigned bytes = BKC ? (unsigned(col) * unsigned(g.ldb) + unsigned(kk)) * 4u : (unsigned(kk) * unsigned(g.ldb) + unsigned(col)) * 4u;
        offB[i] = (n0 + col < g.N) ? bytes : OOB;
        if (has_virtual && n0 + col == g.N) virt_mask |= 1u << i;
    }
    const float* const Atile0 = AKC ? A + m0 * g.lda : A + m0;      // + k0 (AKC) / + k0 * lda per K-tile
    const float* const Btile0 = BKC ? B + n0 * g.ldb : B + n0;

    // The loads are inline asm so that the K loop can keep PD tiles in flight: hipcc's own wait insertion is
    // conservative across the loop back-edge (it drains every outstanding load before the first LDS write).  The
    // destination registers are NOT protected until wait_tile() below has run for that ring slot.
    auto descriptor = [](const float* base) {
        const unsigned long long p = reinterpret_cast<unsigned long long>(base);
        u32x4 d;
        d[0] = unsigned(p); d[1] = unsigned(p >> 32) & 0xffffu; d[2] = OOB; d[3] = 0x00020000u;
        return d;
    };
    // tiles are requested strictly in order: running pointers instead of index arithmetic (every scalar instruction in
    // the K loop of a lone small-tile workgroup shows up in its time)
    // wave-private loop: wave kg owns the k-columns kg * BK .. kg * BK + BK - 1 of every BK * KG - wide step of the slice, the columns it
    // multiplies in the cooperative loop - so every accumulator, and with it the result, is bit for bit what that loop gives.  A wave
    // whose columns lie beyond the slice's end in the last step skips it (the cooperative loop multiplies zeros there); one with
    // no column at all contributes zeros to the exchange.
    constexpr int KSTEP = BK * KG;                                   // k distance between a wave's (a workgroup's) consecutive tiles
    int64_t wk_begin = k_begin, wk_len = k_end - k_begin;
    if constexpr (WPK) {
        wk_begin = k_begin + kg * BK;
        wk_len = wk_len - kg * BK;
        wk_len = wk_len < 0 ? 0 : wk_len;
    }
    const float* nextA = AKC ? Atile0 + wk_begin : Atile0 + wk_begin * g.lda;
    const float* nextB = BKC ? Btile0 + wk_begin : Btile0 + wk_begin * g.ldb;
    const int64_t stepA = AKC ? int64_t(KSTEP) : int64_t(KSTEP) * g.lda, stepB = BKC ? int64_t(KSTEP) : int64_t(KSTEP) * g.ldb;
    [[maybe_unused]] const unsigned gatherA = unsigned(g.lda) * 4u, gatherB = unsigned(g.ldb) * 4u;    // bytes between k-rows (gather staging)
    const int nkt = int((wk_len + KSTEP - 1) / KSTEP);              // K-steps of this slice (32-bit: scalar compares in the loop)
    const int last_left = int(wk_len) - (nkt - 1) * KSTEP;
    const int last_krem = last_left < BKS ? last_left : BKS;         // k values of the last one
    int requested = 0;
    int seg_left = 0, seg_idx = 0;                                   // K through several B operands (lg_gemm_kseg3_f32)
    if constexpr (XT == 2) seg_left = g.seg_steps;
    auto load_tile = [&](int slot) {
        const int krem = requested == nkt - 1 ? last_krem : BKS;     // k values of this tile inside the slice
        ++requested;
        krem_ring[slot] = krem;
        const u32x4 da = descriptor(nextA);
        const u32x4 db = descriptor(nextB);
        nextA += stepA;
        nextB += stepB;
        if constexpr (XT == 2) {
            if (--seg_left == 0) {                                   // the next K-step starts in the next operand
                nextB += seg_idx ? g.seg_jump[1] : g.seg_jump[0];           // (no dynamic index: g may live in registers)
                seg_idx = 1;
                seg_left = g.seg_steps;
            }
        }
#pragma unroll
        for (int i = 0; i < A_CHUNKS; ++i) {
            if constexpr (AG) {
                // k-rows kk .. kk+3 of this lane's row: the k-row distance rides in the instruction's scalar offset.  A full
                // tile needs no k predicate (uniform branch: the offsets are used as they are, no temporaries)
                if (krem == BKS) {
#pragma unroll
                    for (int e = 0; e < 4; ++e)
                        asm volatile("buffer_load_dword %0, %1, %2, %3 offen" : "=v"(ga_ring[slot][i][e]) : "v"(offA[i]), "s"(da), "s"(unsigned(e) * gatherA));
                } else {
#pragma unroll
                    for (int e = 0; e < 4; ++e) {
                        const unsigned off = kcA(i) + e < krem ? offA[i] : OOB;
                        asm volatile("buffer_load_dword %0, %1, %2, %3 offen" : "=v"(ga_ring[slot][i][e]) : "v"(off), "s"(da), "s"(unsigned(e) * gatherA));
                    }
                }
            } else {
                const unsigned off = kcA(i) < krem ? offA[i] : OOB;
                if constexpr (VA) asm volatile("buffer_load_dwordx4 %0, %1, %2, 0 offen" : "=v"(ra_ring[slot][i]) : "v"(off), "s"(da));
                else              asm volatile("buffer_load_dword %0, %1, %2, 0 offen" : "=v"(ra_ring[slot][i]) : "v"(off), "s"(da));
            }
        }
#pragma unroll
        for (int i = 0; i < B_CHUNKS; ++i) {
            if constexpr (BG) {
                if (krem == BKS) {
#pragma unroll
                    for (int e = 0; e < 4; ++e)
                        asm volatile("buffer_load_dword %0, %1, %2, %3 offen" : "=v"(gb_ring[slot][i][e]) : "v"(offB[i]), "s"(db), "s"(unsigned(e) * gatherB));
                } else {
#pragma unroll
                    for (int e = 0; e < 4; ++e) {
                        const unsigned off = kcB(i) + e < krem ? offB[i] : OOB;
                        asm volatile("buffer_load_dword %0, %1, %2, %3 offen" : "=v"(gb_ring[slot][i][e]) : "v"(off), "s"(db), "s"(unsigned(e) * gatherB));
                    }
                }
            } else {
                const unsigned off = kcB(i) < krem ? offB[i] : OOB;
                if constexpr (VB) asm volatile("buffer_load_dwordx4 %0, %1, %2, 0 offen" : "=v"(rb_ring[slot][i]) : "v"(off), "s"(db));
                else              asm volatile("buffer_load_dword %0, %1, %2, 0 offen" : "=v"(rb_ring[slot][i]) : "v"(off), "s"(db));
            }
        }
    };
    // wait until the loads of ring slot `slot` have landed, given that `younger` tiles were requested after it
    auto wait_tile = [&](int slot, int younger) {
        if (PD >= 3 && younger >= 2)      asm volatile("s_waitcnt vmcnt(%0)" :: "n"(PD >= 3 ? 2 * NL : 0) : "memory");
        else if (PD >= 2 && younger == 1) asm volatile("s_waitcnt vmcnt(%0)" :: "n"(PD >= 2 ? NL : 0) : "memory");
        else                              asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
#pragma unroll
        for (int i = 0; i < A_CHUNKS; ++i) {
            if constexpr (AG) { asm volatile("" : "+v"(ga_ring[slot][i][0]), "+v"(ga_ring[slot][i][1]), "+v"(ga_ring[slot][i][2]), "+v"(ga_ring[slot][i][3])); }
            else              asm volatile("" : "+v"(ra_ring[slot][i]));
        }
#pragma unroll
        for (int i = 0; i < B_CHUNKS; ++i) {
            if constexpr (BG) { asm volatile("" : "+v"(gb_ring[slot][i][0]), "+v"(gb_ring[slot][i][1]), "+v"(gb_ring[slot][i][2]), "+v"(gb_ring[slot][i][3])); }
            else              asm volatile("" : "+v"(rb_ring[slot][i]));
        }
    };

    auto store_tile = [&](int buf, int slot) {
        float* a = ldsw + buf * BUF;
        float* b = ldsw + buf * BUF + A_TILE;
        // K not a multiple of 4: the last float4 of a K-contiguous row runs into the next row - zero what lies beyond the
        // slice (only the slice's last tile can be short)
        if (g.k_tail && krem_ring[slot] < BKS) {
            asm volatile("; short K tail" ::: "memory");        // keeps this rare fix-up a branch, not selects in every iteration
            if constexpr (VA && AKC) {
#pragma unroll
                for (int i = 0; i < A_CHUNKS; ++i)
#pragma unroll
                    for (int e = 1; e < 4; ++e)
                        if (kcA(i) + e >= krem_ring[slot]) ra_ring[slot][i][e] = 0.f;
            }
            if constexpr (VB && BKC) {
#pragma unroll
                for (int i = 0; i < B_CHUNKS; ++i)
#pragma unroll
                    for (int e = 1; e < 4; ++e)
                        if (kcB(i) + e >= krem_ring[slot]) rb_ring[slot][i][e] = 0.f;
            }
        }
        if constexpr (kHasExtras<BM, BN>) if (g.relu_a) {
            asm volatile("; relu(A) on the way to LDS" ::: "memory");
#pragma unroll
            for (int i = 0; i < A_CHUNKS; ++i) {
                if constexpr (VA) {
#pragma unroll
                    for (int e = 0; e < 4; ++e) { const float x = ra_ring[slot][i][e]; ra_ring[slot][i][e] = (x != x) ? x : (x > 0.0f ? x : 0.0f); }
                } else {
                    const float x = ra_ring[slot][i]; ra_ring[slot][i] = (x != x) ? x : (x > 0.0f ? x : 0.0f);
                }
            }
        }
#pragma unroll
        for (int i = 0; i < A_CHUNKS; ++i) {
            if constexpr (AG)      *reinterpret_cast<f32x4*>(a + a_lds0 + i * A_LDS_STEP) = f32x4{ga_ring[slot][i][0], ga_ring[slot][i][1], ga_ring[slot][i][2], ga_ring[slot][i][3]};
            else if constexpr (VA) *reinterpret_cast<f32x4*>(a + a_lds0 + i * A_LDS_STEP) = ra_ring[slot][i];
            else                   a[a_lds0 + i * A_LDS_STEP] = ra_ring[slot][i];
        }
        if constexpr (kHasExtras<BM, BN>) if (g.relu_b) {
            asm volatile("; relu(B) on the way to LDS" ::: "memory");
#pragma unroll
            for (int i = 0; i < B_CHUNKS; ++i) {
                if constexpr (VB) {
#pragma unroll
                    for (int e = 0; e < 4; ++e) { const float x = rb_ring[slot][i][e]; rb_ring[slot][i][e] = (x != x) ? x : (x > 0.0f ? x : 0.0f); }
                } else {
                    const float x = rb_ring[slot][i]; rb_ring[slot][i] = (x != x) ? x : (x > 0.0f ? x : 0.0f);
                }
            }
        }
        if constexpr (kHasExtras<BM, BN>) if (has_virtual) {
            // the loads returned zeros for the virtual column (beyond N): put the ones in, for the k values that exist
#pragma unroll
            for (int i = 0; i < B_CHUNKS; ++i) {
                const bool virt = (virt_mask >> i) & 1u, kv = kcB(i) < krem_ring[slot];
                const float one = kv ? 1.0f : 0.0f;
                if constexpr (VB) {
                    if constexpr (BKC) {                                                           // row N of B^T: ones along k
                        if (virt) {
                            const int kr = krem_ring[slot] - kcB(i);
                            rb_ring[slot][i] = f32x4{kr > 0 ? 1.f : 0.f, kr > 1 ? 1.f : 0.f, kr > 2 ? 1.f : 0.f, kr > 3 ? 1.f : 0.f};
                        }
                    }
                    else               { if (virt) rb_ring[slot][i] = f32x4{one, 0.f, 0.f, 0.f}; }     // k-row of B: column N, then beyond
                } else {
                    if (virt) rb_ring[slot][i] = one;
                }
            }
        }
#pragma unroll
        for (int i = 0; i < B_CHUNKS; ++i) {
            if constexpr (BG)      *reinterpret_cast<f32x4*>(b + b_lds0 + i * B_LDS_STEP) = f32x4{gb_ring[slot][i][0], gb_ring[slot][i][1], gb_ring[slot][i][2], gb_ring[slot][i][3]};
            else if constexpr (VB) *reinterpret_cast<f32x4*>(b + b_lds0 + i * B_LDS_STEP) = rb_ring[slot][i];
            else                   b[b_lds0 + i * B_LDS_STEP] = rb_ring[slot][i];
        }
    };

    f32x16 acc[TM][TN];
    // the bias values of this lane's columns, requested before the K loop: in the epilogue their load would be one more
    // memory round trip behind the last MFMA
    // (small tiles only: the 256 x 256 tile has 128 MFMAs per K-tile to hide one more load behind, and no register to park it in)
    [[maybe_unused]] float bias_ahead[TN];
    if constexpr (kHasExtras<BM, BN>) {
#pragma unroll
        for (int j = 0; j < TN; ++j) {
            const int64_t col = n0 + (wn * TN + j) * 32 + r;
            bias_ahead[j] = (bias && col < g.N) ? bias[col] : 0.f;
        }
    }
#pragma unroll
    for (int i = 0; i < TM; ++i)
#pragma unroll
        for (int j = 0; j < TN; ++j)
#pragma unroll
            for (int e = 0; e < 16; ++e) acc[i][j][e] = 0.f;

    auto compute_tile = [&](int buf, int kb_begin, int kb_end) {
        const float* a = lds + buf * BUF + (ALK ? (wm * TM * 32 + r) * A_PITCH + 4 * h + kofs : (4 * h + kofs) * A_PITCH + wm * TM * 32 + r);
        const float* b = lds + buf * BUF + A_TILE + (BLK ? (wn * TN * 32 + r) * B_PITCH + 4 * h + kofs : (4 * h + kofs) * B_PITCH + wn * TN * 32 + r);
#pragma unroll
        for (int kb = kb_begin; kb < kb_end; kb += 8) {
            float fa[TM][4], fb[TN][4];
#pragma unroll
            for (int i = 0; i < TM; ++i) {
                if constexpr (ALK) {
                    const float4 v = *reinterpret_cast<const float4*>(a + i * 32 * A_PITCH + kb);
                    fa[i][0] = v.x; fa[i][1] = v.y; fa[i][2] = v.z; fa[i][3] = v.w;
                } else {
#pragma unroll
                    for (int s = 0; s < 4; ++s) fa[i][s] = a[(kb + s) * A_PITCH + i * 32];
                }
            }
#pragma unroll
            for (int j = 0; j < TN; ++j) {
                if constexpr (BLK) {
                    const float4 v = *reinterpret_cast<const float4*>(b + j * 32 * B_PITCH + kb);
                    fb[j][0] = v.x; fb[j][1] = v.y; fb[j][2] = v.z; fb[j][3] = v.w;
                } else {
#pragma unroll
                    for (int s = 0; s < 4; ++s) fb[j][s] = b[(kb + s) * B_PITCH + j * 32];
                }
            }
#pragma unroll
            for (int s = 0; s < 4; ++s)
#pragma unroll
                for (int i = 0; i < TM; ++i)
#pragma unroll
                    for (int j = 0; j < TN; ++j)
                        acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x2f32(fa[i][s], fb[j][s], acc[i][j], 0, 0, 0);
        }
    };

    // tile j waits in ring slot j % PD; tiles 0 .. PD-1 are requested up front
#pragma unroll
    for (int u = 0; u < PD; ++u)
        if (u < nkt) load_tile(u);
    if constexpr (!WPK) {
        const int younger = nkt - 1 < PD - 1 ? nkt - 1 : PD - 1;
        wait_tile(0, younger);
        store_tile(0, 0);
        __syncthreads();
    }
    LG_TL(1);                                        // first K-tile in LDS
    if constexpr (WPK) {
        // The wave's own pipeline: during iteration kt its LDS region holds tile kt, and tile kt+1 moves from the ring into the
        // same region in the MIDDLE of the dependent MFMA chain - behind the reads of tile kt's second half in program order, which
        // is all a single buffer needs; the first half of tile kt+1 follows it out of LDS under the second half's MFMAs.  A ring
        // slot is refilled as soon as its tile is in LDS: before the wait for tile t the tiles up to t + PD - 1 have been requested.
        static_assert(BK == 16, "one K-step is two k-blocks of 8");
        float fa[2][4], fb[2][4];
        auto read_half = [&](int half, int set) {
            const float4 va = *reinterpret_cast<const float4*>(ldsw + r * A_PITCH + 4 * h + half * 8);
            const float4 vb = *reinterpret_cast<const float4*>(ldsw + A_TILE + r * B_PITCH + 4 * h + half * 8);
            fa[set][0] = va.x; fa[set][1] = va.y; fa[set][2] = va.z; fa[set][3] = va.w;
            fb[set][0] = vb.x; fb[set][1] = vb.y; fb[set][2] = vb.z; fb[set][3] = vb.w;
        };
        auto mfma_part = [&](int set, int e0, int e1) {
#pragma unroll
            for (int e = e0; e < e1; ++e)
                acc[0][0] = __builtin_amdgcn_mfma_f32_32x32x2f32(fa[set][e], fb[set][e], acc[0][0], 0, 0, 0);
        };
        // tile t: ring -> LDS, and its ring slot is asked for tile t + PD
        auto advance = [&](int t, int slot) {
            const int younger = (nkt < t + PD ? nkt : t + PD) - (t + 1);
            wait_tile(slot, younger);
            store_tile(0, slot);
            if (t + PD < nkt) load_tile(slot);
        };
        if (nkt > 0) {
            advance(0, 0);
            read_half(0, 0);
        }
        for (int kt0 = 0; kt0 < nkt; kt0 += PD) {
#pragma unroll
            for (int u = 0; u < PD; ++u) {
                const int kt = kt0 + u;
                if (kt < nkt) {
                    read_half(1, 1);
                    mfma_part(0, 0, 4);
                    __builtin_amdgcn_sched_barrier(0);
                    if (kt + 1 < nkt) advance(kt + 1, (u + 1) % PD);
                    __builtin_amdgcn_sched_barrier(0);
                    // the next tile's first half leaves LDS behind the first MFMA of this half: the wait in front of that MFMA
                    // then covers the second-half fragments alone, and three MFMAs run over the read
                    mfma_part(1, 0, 1);
                    __builtin_amdgcn_sched_barrier(0);
                    if (kt + 1 < nkt) read_half(0, 0);
                    mfma_part(1, 1, 4);
                }
            }
        }
    } else if constexpr (TM * TN == 1) {
        // One accumulator per wave (small tiles: often ONE such wave per SIMD, nothing else to hide latency behind):
        // the fragments of the next half K-tile are fetched from LDS while the MFMAs of the current half run.  The
        // barrier sits between the halves: before it every wave has read ALL of tile kt and written its share of tile
        // kt+1, after it the first-half fragments of tile kt+1 are fetched under the second half's MFMAs.
        constexpr int HG = BK / 16;                  // k-groups of 8 per half tile
        float fa[2][HG][4], fb[2][HG][4];
        auto read_half = [&](int buf, int half, int slot) {
            const float* a = lds + buf * BUF + (AKC ? (wm * 32 + r) * A_PITCH + 4 * h + kofs : (4 * h + kofs) * A_PITCH + wm * 32 + r);
            const float* b = lds + buf * BUF + A_TILE + (BKC ? (wn * 32 + r) * B_PITCH + 4 * h + kofs : (4 * h + kofs) * B_PITCH + wn * 32 + r);
#pragma unroll
            for (int q = 0; q < HG; ++q) {
                const int kb = half * (BK / 2) + q * 8;
                if constexpr (AKC) {
                    const float4 v = *reinterpret_cast<const float4*>(a + kb);
                    fa[slot][q][0] = v.x; fa[slot][q][1] = v.y; fa[slot][q][2] = v.z; fa[slot][q][3] = v.w;
                } else {
#pragma unroll
                    for (int e = 0; e < 4; ++e) fa[slot][q][e] = a[(kb + e) * A_PITCH];
                }
                if constexpr (BKC) {
                    const float4 v = *reinterpret_cast<const float4*>(b + kb);
                    fb[slot][q][0] = v.x; fb[slot][q][1] = v.y; fb[slot][q][2] = v.z; fb[slot][q][3] = v.w;
                } else {
#pragma unroll
                    for (int e = 0; e < 4; ++e) fb[slot][q][e] = b[(kb + e) * B_PITCH];
                }
            }
        };
        auto mfma_part = [&](int slot, int q0, int q1) {
#pragma unroll
            for (int q = q0; q < q1; ++q)
#pragma unroll
                for (int e = 0; e < 4; ++e)
                    acc[0][0] = __builtin_amdgcn_mfma_f32_32x32x2f32(fa[slot][q][e], fb[slot][q][e], acc[0][0], 0, 0, 0);
        };
        auto mfma_half = [&](int slot) { mfma_part(slot, 0, HG); };
        constexpr int HQ = HG > 1 ? HG / 2 : HG;     // MFMA groups issued before the LDS write of the next tile
        read_half(0, 0, 0);
        for (int kt0 = 0; kt0 < nkt; kt0 += PD) {
#pragma unroll
            for (int u = 0; u < PD; ++u) {
                const int kt = kt0 + u;
                if (kt < nkt) {
                    const int cur = kt & 1;
                    if (PD == 1 && kt + 1 < nkt) load_tile(0);
                    read_half(cur, 1, 1);
                    // the LDS write of tile kt+1 goes in the MIDDLE of the dependent MFMA chain: its latency, and the
                    // barrier's, then run under the MFMAs still queued instead of after the last one
                    mfma_part(0, 0, HQ);
                    __builtin_amdgcn_sched_barrier(0);
                    if (kt + 1 < nkt) {
                        int younger = nkt - (kt + 2);
                        if (younger > PD - 2) younger = PD - 2;
                        wait_tile((u + 1) % PD, PD == 1 ? 0 : (younger < 0 ? 0 : younger));
                        store_tile(cur ^ 1, (u + 1) % PD);
                    }
                    if (PD > 1 && kt + PD < nkt) load_tile(u);
                    __builtin_amdgcn_sched_barrier(0);
                    mfma_part(0, HQ, HG);
                    __syncthreads();
                    if (kt + 1 < nkt) read_half(cur ^ 1, 0, 0);
                    mfma_half(1);
                }
            }
        }
    } else {
        for (int kt0 = 0; kt0 < nkt; kt0 += PD) {
    #pragma unroll
            for (int u = 0; u < PD; ++u) {
                const int kt = kt0 + u;
                if (kt < nkt) {
                    const int cur = kt & 1;
                    // PD == 1: tile kt+1 is requested here and written to LDS in the middle of this iteration.
                    // PD  > 1: slot u (tile kt, in LDS since the last iteration) is refilled with tile kt + PD below, after
                    //          the LDS write of tile kt+1 - whose loads were requested PD-1 iterations ago.
                    if (PD == 1 && kt + 1 < nkt) load_tile(0);
                    compute_tile(cur, 0, BK / 2);
                    if (kt + 1 < nkt) {
                        int younger = nkt - (kt + 2);                 // tiles kt+2 .. kt+PD-1 requested after tile kt+1
                        if (younger > PD - 2) younger = PD - 2;
                        wait_tile((u + 1) % PD, PD == 1 ? 0 : (younger < 0 ? 0 : younger));
                        store_tile(cur ^ 1, (u + 1) % PD);                // ds_writes issue in the shadow of the second half's MFMAs
                    }
                    if (PD > 1 && kt + PD < nkt) load_tile(u);
                    compute_tile(cur, BK / 2, BK);
                    __syncthreads();
                }
            }
        }
    }

    LG_TL(2);                                        // K loop done
    if constexpr (KG > 1) {
        // K-groups 1 .. KG-1 hand their accumulators to group 0 through LDS (the staging buffers are free after the loop's last
        // barrier): slot (group - 1, wave-in-group, accumulator, register) holds one value per lane, so both sides move 256 B per
        // wave instruction without bank conflicts; group 0 adds them in group order.  The other groups are done after that.
        constexpr int GROUP_FLOATS = WM * WN * TM * TN * 16 * 64;
        static_assert(WPK || (KG - 1) * GROUP_FLOATS <= 2 * (A_TILE + B_TILE), "the K-group exchange must fit the staging buffers");
        // (wave-private loop: no barrier says that the other waves have left their loops - the exchange lies behind their regions)
        static_assert(!WPK || KG * BUF + (KG - 1) * GROUP_FLOATS <= gemm_lds_floats<BM, BN, BK, AKC, BKC, KG>(), "staging regions + exchange");
        float* x = lds + (WPK ? KG * BUF : 0) + (wl * TM * TN * 16) * 64 + lane;
        if (kg >= 1) {
#pragma unroll
            for (int i = 0; i < TM; ++i)
#pragma unroll
                for (int j = 0; j < TN; ++j)
#pragma unroll
                    for (int e = 0; e < 16; ++e) x[(kg - 1) * GROUP_FLOATS + ((i * TN + j) * 16 + e) * 64] = acc[i][j][e];
        }
        __syncthreads();
        if (kg >= 1) return;
#pragma unroll
        for (int gq = 0; gq < KG - 1; ++gq)
#pragma unroll
            for (int i = 0; i < TM; ++i)
#pragma unroll
                for (int j = 0; j < TN; ++j)
#pragma unroll
                    for (int e = 0; e < 16; ++e) acc[i][j][e] += x[gq * GROUP_FLOATS + ((i * TN + j) * 16 + e) * 64];
    }
    // The optimizer's update of the parameter whose gradient this tile holds (lg_adam_epilogue_arm): this step's scalars once per
    // wave - a chain of three dependent scalar loads (plan -> step number -> table of bias corrections), started ahead of the
    // split-K hand-off (at the top of the kernel they cost the prologue of EVERY workgroup: the MLP step 64.0 -> 65.4 us).  Uniform branches on kernel arguments that are NULL in every other launch.
    // (Measured and not kept: requesting the parameter and its moments here too - 48 more live VGPRs take the two-product
    // launch from 128 to 172 registers and from four to two waves per SIMD: 24.9 -> 37.9 us, profiles/r4/README.)
    [[maybe_unused]] AdamScalars adam_cs_c, adam_cs_r;
    [[maybe_unused]] int64_t adam_done_c = 0, adam_done_r = 0;
    if constexpr (kCanAdam<BM, BN, KG>) {
        if (g.adam_c) adam_cs_c = adam_plan_scalars(g.adam_c, adam_done_c);
        if (g.adam_r) adam_cs_r = adam_plan_scalars(g.adam_r, adam_done_r);
    }
    if constexpr (kCanSplitK<BM, BN, KG>) if (g.k_slices > 1) {
        // split-K, folded inside the launch (cdna_hip_programming.md, in-launch split-K recipe, write-through form).
        // Partial tiles go to the workspace in ACCUMULATOR layout - 16-byte piece ((i*TN + j)*4 + q) of thread tid at
        // byte (((i*TN + j)*4 + q)*NT + tid)*16 of the (batch, slice, tile) slab - so stores and the fold move 1 KiB per
        // wave instruction.  The slices of a tile run on different XCDs whose L2s are not coherent: slabs are stored
        // write-through (sc1) and drained, ONE lane takes an agent-scope ticket, and the workgroup that arrives last
        // reads every slab with sc1 loads (never served from a stale line), sums them in slice order - the same
        // order in every run, so results are bit-reproducible - and runs the epilogue.  The ticket is reset for the
        // next launch by that workgroup.
        constexpr int SC1 = 16;                                   // aux bit of the raw buffer builtins
        constexpr int TILE_BYTES = BM * BN * 4;
        char* slab0 = reinterpret_cast<char*>(g.W) + (int64_t(batch) * g.k_slices * per_batch + t) * int64_t(TILE_BYTES);
        const int64_t slice_stride = int64_t(per_batch) * TILE_BYTES;
        {
            const auto mine = __builtin_amdgcn_make_buffer_rsrc(slab0 + slice * slice_stride, 0, TILE_BYTES, 0x00020000);
#pragma unroll
            for (int i = 0; i < TM; ++i)
#pragma unroll
                for (int j = 0; j < TN; ++j)
#pragma unroll
                    for (int q = 0; q < 4; ++q) {
                        u32x4 v;
#pragma unroll
                        for (int e = 0; e < 4; ++e) v[e] = __float_as_uint(acc[i][j][4 * q + e]);
                        __builtin_amdgcn_raw_buffer_store_b128(v, mine, (((i * TN + j) * 4 + q) * NT + tid) * 16, 0, SC1);
                    }
        }
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");          // every storing wave drains its write-through stores
        __syncthreads();
        LG_TL(3);                                                 // slab written and drained
        int* arrived_last = reinterpret_cast<int*>(lds);          // the staging buffers are free after the K loop's last barrier
        if (tid == 0) {
            int* ticket = g.tickets + batch * per_batch + t;
            const int order = __hip_atomic_fetch_add(ticket, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            const int last = order == g.k_slices - 1;
            if (last) __hip_atomic_store(ticket, 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            *arrived_last = last;
        }
        __syncthreads();
        LG_TL(4);                                                 // ticket drawn
        if (!*arrived_last) return;
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");    // no instruction: keeps the slab loads below the ticket
        constexpr int CH = TM * TN >= 4 ? 1 : (TM * TN == 2 ? 2 : 4);     // slices whose loads are in flight together
        for (int s0 = 0; s0 < g.k_slices; s0 += CH) {
            u32x4 v[CH][TM * TN * 4];
#pragma unroll
            for (int c = 0; c < CH; ++c) {
                const int sl = s0 + c < g.k_slices ? s0 + c : s0;
                const auto src = __builtin_amdgcn_make_buffer_rsrc(slab0 + sl * slice_stride, 0, TILE_BYTES, 0x00020000);
#pragma unroll
                for (int f = 0; f < TM * TN * 4; ++f) v[c][f] = __builtin_amdgcn_raw_buffer_load_b128(src, (f * NT + tid) * 16, 0, SC1);
            }
#pragma unroll
            for (int c = 0; c < CH; ++c) {
                const bool live = s0 + c < g.k_slices, first = s0 + c == 0;
#pragma unroll
                for (int i = 0; i < TM; ++i)
#pragma unroll
                    for (int j = 0; j < TN; ++j)
#pragma unroll
                        for (int e = 0; e < 16; ++e) {
                            const float w = __uint_as_float(v[c][(i * TN + j) * 4 + e / 4][e % 4]);
                            acc[i][j][e] = first ? w : (live ? acc[i][j][e] + w : acc[i][j][e]);
                        }
            }
        }
    }

    LG_TL(5);                                        // slabs folded (or nothing to fold)
    // epilogue: C/D layout of the 32x32 MFMA: col = lane & 31, row = (reg & 3) + 8 * (reg >> 2) + 4 * (lane >> 5).
    // The lane's coordinates are formed AGAIN from the thread index (opaque to the compiler): carried through the K loop from
    // the prologue they cost the 256 x 256 tile two registers it does not have.
    int etid = threadIdx.x;
    asm volatile("" : "+v"(etid));
    const int ewl = (etid >> 6) % (WM * WN), er = etid & 31, eh = (etid >> 5) & 1;
    const int ewm = ewl / WN, ewn = ewl % WN;
#pragma unroll
    for (int i = 0; i < TM; ++i) {
#pragma unroll
        for (int j = 0; j < TN; ++j) {
            const int64_t col = n0 + (ewn * TN + j) * 32 + er;
            const int64_t row0 = m0 + (ewm * TM + i) * 32 + 4 * eh;
            const bool vcol = has_virtual && col == g.N;             // this lane holds row sums, not a column of C
            if (col < g.N || vcol) {
                float bv = 0.f;
                if constexpr (kHasExtras<BM, BN>) bv = (bias && !vcol) ? bias_ahead[j] : 0.f;
                else                              bv = bias ? bias[col] : 0.f;
                float* const dst = vcol ? g.rowsum : C + col;
                const int64_t dstride = vcol ? 1 : ldc;
                const float* const addend = vcol ? nullptr : g.addend;        // C = value + addend[row][col] (never with accumulate)
                const bool acc_flag = vcol ? g.rowsum_accumulate != 0 : (accumulate != 0 || addend != nullptr);
                const float* const old_src = addend ? addend + col : dst;
                const int64_t old_stride = addend ? g.ldadd : dstride;
                // The values first, the stores last, and the read-modify-write of `C += ...` in a block of its own:
                // on gfx9-family hardware stores count in vmcnt like loads, so when the old-value loads sat in the same
                // straight-line code as the stores, the wait in front of every add also drained the PREVIOUS store -
                // 16 serialised store round trips, 2.0 of a 15.6 us launch (tools/gemm_timeline.py).
                float val[16];
#pragma unroll
                for (int e = 0; e < 16; ++e) val[e] = bias ? acc[i][j][e] + bv : acc[i][j][e];
                if (acc_flag) {
                    float old[16];
#pragma unroll
                    for (int e = 0; e < 16; ++e) {
                        const int64_t row = row0 + (e & 3) + 8 * (e >> 2);
                        old[e] = row < g.M ? old_src[row * old_stride] : 0.f;
                    }
#pragma unroll
                    for (int e = 0; e < 16; ++e) val[e] = old[e] + val[e];
                }
                if constexpr (kHasExtras<BM, BN>) {
                    if (g.act == 2 && !vcol) {                        // gelu backward: the product times gelu'(aux)
                        float x[16];
#pragma unroll
                        for (int e = 0; e < 16; ++e) {
                            const int64_t row = row0 + (e & 3) + 8 * (e >> 2);
                            x[e] = row < g.M ? g.aux[row * g.ldadd + col] : 0.f;
                        }
#pragma unroll
                        for (int e = 0; e < 16; ++e) val[e] = gelu_grad(x[e], val[e]);
                    }
                }
                float* p = dst + row0 * dstride;
#pragma unroll
                for (int e = 0; e < 16; ++e) {
                    const int64_t row = row0 + (e & 3) + 8 * (e >> 2);
#if LG_TILE_SIGNAL
                    if (row < g.M) __hip_atomic_store(p + ((e & 3) + 8 * (e >> 2)) * dstride, val[e], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
#else
                    if (row < g.M) p[((e & 3) + 8 * (e >> 2)) * dstride] = val[e];
#endif
                }
                if constexpr (kCanAdam<BM, BN, KG>) {
                    const AdamPlan* const pl = vcol ? g.adam_r : g.adam_c;
                    if (pl) {
                        // the parameter has the gradient's layout: element (row, col) of C sits at row * ldc + col (ldc == N),
                        // row sum `row` at `row`.  New values go to the plan's second buffer: dx = g @ W of the same launch
                        // (sgemm_pair_wgrad_xgrad) still reads the old ones.  Eight values at a time (registers).
                        const AdamScalars& cs = vcol ? adam_cs_r : adam_cs_c;
                        const int64_t base = vcol ? row0 : row0 * ldc + col;
                        const float* const pin = pl->p_in + base;
                        float* const pout = pl->p_out + base;
                        float* const pm = pl->m + base;
                        float* const pv = pl->v + base;
#pragma unroll
                        for (int half = 0; half < 2; ++half) {
                            float P[8], Mo[8], Vo[8];
#pragma unroll
                            for (int q = 0; q < 8; ++q) {
                                const int e = half * 8 + q;
                                const int64_t row = row0 + (e & 3) + 8 * (e >> 2);
                                const int64_t o = ((e & 3) + 8 * (e >> 2)) * dstride;
                                const bool in = row < g.M;
                                P[q] = in ? pin[o] : 0.f;
                                Mo[q] = in ? pm[o] : 0.f;
                                Vo[q] = in ? pv[o] : 0.f;
                            }
#pragma unroll
                            for (int q = 0; q < 8; ++q) adam_elem(P[q], val[half * 8 + q], Mo[q], Vo[q], cs);
#pragma unroll
                            for (int q = 0; q < 8; ++q) {
                                const int e = half * 8 + q;
                                const int64_t row = row0 + (e & 3) + 8 * (e >> 2);
                                const int64_t o = ((e & 3) + 8 * (e >> 2)) * dstride;
                                if (row < g.M) { pout[o] = P[q]; pm[o] = Mo[q]; pv[o] = Vo[q]; }
                            }
                        }
                    }
                }
                if constexpr (kHasExtras<BM, BN>) {
                    if (g.act == 1 && !vcol) {                        // gelu forward: C holds the pre-activation, aux its gelu
                        float* q = g.aux + row0 * g.ldadd + col;
#pragma unroll
                        for (int e = 0; e < 16; ++e) {
                            const int64_t row = row0 + (e & 3) + 8 * (e >> 2);
                            if (row < g.M) q[((e & 3) + 8 * (e >> 2)) * g.ldadd] = gelu_value(val[e]);
                        }
                    }
                }
            }
        }
    }
    if constexpr (kCanAdam<BM, BN, KG>) {
        // the one workgroup per step that advances the optimizer's step number: the tile holding element 0 of the plan that
        // carries step_out (every reader of this step reads step_in, which nobody writes now)
        if (tid == 0 && tm == 0) {
            if (g.adam_c && tn == 0 && g.adam_c->step_out)
                __hip_atomic_store(g.adam_c->step_out, adam_done_c + 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            if (g.adam_r && has_virtual && g.adam_r->step_out)
                __hip_atomic_store(g.adam_r->step_out, adam_done_r + 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
    }
    LG_TL(6);                                        // epilogue stores issued
#if LG_TILE_SIGNAL
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // this wavefront's part of the tile has reached memory
    if (lane == 0) {
        // the wavefront that completes the row of tiles raises the row's FLAG (a word of its own: the waiting workgroups poll it
        // with plain loads, which do not queue up with the atomics on the ticket) and leaves the ticket at zero for the next launch
        int* const ticket = signal_tickets + tm * signal_stride;
        if (__hip_atomic_fetch_add(ticket, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == signal_per_row - 1) {
            __hip_atomic_store(ticket, 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            __hip_atomic_store(ticket + 16, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
    }
#endif
