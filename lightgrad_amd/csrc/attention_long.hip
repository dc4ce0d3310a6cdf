// Self-attention of a sequence of 129 .. 512 tokens in one launch each way (gfx950, fp32 MFMA): the long forms of attention.hip.
//
//   forward    P = softmax((Q K^T) * scale + bias)   O = P V          per (batch, head), reference examples/bert.py:78-88
//   backward   dV = P^T dO   dP = dO V^T   dS = P o (dP - shift) * scale   dQ = dS K   dK = dS^T Q
//
// attention.hip keeps all of K and V (forward) or of dO and Q (backward, key role) of one (batch, head) pair in LDS: at
// S = 512, D = 64 that is about 290 KB against the 160 KiB of a CU.  Here only what is one ROW BLOCK wide stays for the whole
// launch - the 32 x (Sp + 4) tile of scores / probabilities (forward) or dP / dS (backward, query role), 66 KB at 512 - and
// everything that is S long streams through ONE chunk buffer of 128 rows: K, then V forward; V, then K in the query role; dO and
// Q side by side in the key role.  The next chunk's global loads are issued into registers before the MFMAs of the chunk in
// LDS, so they fly behind the matrix cores.  With the whole row in LDS the softmax is the three passes of attention.hip: no
// online rescaling.  Accumulators (context, dQ, dK, dV) live in registers across the chunks and fold through LDS once, in wave
// order, at the end: no float atomics, the same bits every run.
//
// Everything else is attention.hip's TAIL form: work split (one workgroup per (batch, head, block of 32 queries) forward; query
// role and key role backward with the in-launch hand-off of the row shifts and its bounded wait), MFMA operand layouts and
// pitches (mfma_lds.h), Sp = S rounded up to 32 with LDS operand rows [S, Sp) ZERO, keys >= S taken out of the softmax by
// selection, global rows >= S neither read nor written, the per-key bias (1 - mask) * -10000 in fp32, and the probabilities
// (row pitch S, 16-byte aligned only when S % 4 == 0) written once by the forward and read by the backward.  Both roles of the
// backward form dP by the same MFMA sequence over the same operands (wave_mma over D), so their dP - and dS - agree bit for bit.
//
// LDS at D = 64, S = 512: forward 126 KB, query role 124 KB, key role 132 KB: one workgroup per CU.  The argument for the
// hand-off - query-role workgroups fill the front of the grid, so a key-role workgroup only ever waits for workgroups that are
// already running and wait for nothing - does not depend on occupancy.
//
// Layout.  The argument structs and device helpers are attention.hip's own (attention_common.h).  This file holds the long kernels,
// one launcher per direction (attn_long_launch_fwd / _bwd, called by the shared host path of attention.hip - for the long
// entries below and, beyond 128 positions, for the dropout entries and the causal forward entry) and the two
// lg_attention_long_* entries.
#include "attention_common.h"

namespace lg {

constexpr int kLongChunk = 128;        // rows of a streamed operand in LDS at a time
constexpr int kLongMaxBlocks = 16;     // 32-column blocks of the longest row (512 / 32)

// rows [c0, c0 + 128) of an operand of S rows: global -> registers (only rows < S are addressed; c0 < S) ...
template <int D, int N>
__device__ __forceinline__ void chunk_load(af32x4 (&v)[N], const float* x, int64_t ld, int c0, int S) {
    const int rows = S - c0 < kLongChunk ? S - c0 : kLongChunk;
    load_rows<D, N>(v, x + int64_t(c0) * ld, ld, rows);
}
// ... and registers -> LDS, rows [S, Sp) of the chunk zero
template <int D, int N>
__device__ __forceinline__ void chunk_store(const af32x4 (&v)[N], float* dst, int pitch, int c0, int S, int Sp) {
    const int rows = S - c0 < kLongChunk ? S - c0 : kLongChunk;
    const int padded = Sp - c0 < kLongChunk ? Sp - c0 : kLongChunk;
    store_rows_padded<D, N>(v, dst, pitch, rows, padded);
}

template <int D>
constexpr int attn_long_fwd_lds_floats(int Sp) { return 32 * (D + 4) + 32 * (Sp + 4) + kLongChunk * (D + 8) + 3 * 1024 + Sp; }

// DROP: dropout of the probabilities between the softmax and the context, from the stream of dropout.hip (one call per launch:
// read `draws`, take a ticket, the last arriver advances).  P goes to HBM undropped; what feeds the context MFMAs is Pd.
// CAUSAL: query i sees keys j <= i (attention.hip: the selection of the softmax, +0.0 stored to P above the diagonal).  No key
// beyond column q0 + 31 is anyone's in this block, so the K chunks and the V chunks end at the chunk that holds that column -
// Sc = q0 + 32 stands where Sp stood: the same bound for the whole workgroup, about half the MFMAs over the grid.
template <int D, bool DROP = false, bool CAUSAL = false>
__global__ void __launch_bounds__(256) attn_long_fwd(std::conditional_t<DROP, AttnDropArgs, AttnTailArgs> a) {
    extern __shared__ __attribute__((aligned(16))) float lds[];
    const int S = a.S, Sp = round32(S), PP = Sp + 4;
    constexpr int PQ = D + 4, PV = D + 8;
    constexpr int NB = 32 * (D / 4) / 256 > 0 ? 32 * (D / 4) / 256 : 1, NA = kLongChunk * (D / 4) / 256;
    float* Qs = lds;                      // Q rows of the block                    32 x PQ
    float* Ps = Qs + 32 * PQ;             // scores, then probabilities             32 x PP
    float* Buf = Ps + 32 * PP;            // a chunk of K (pitch PQ), then of V (pitch PV)
    float* Red = Buf + kLongChunk * PV;
    float* Bias = Red + 3 * 1024;         // what key j adds to every score of its column
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, r = lane & 31, h = lane >> 5;
    const int q0 = blockIdx.x * 32, head = blockIdx.y, b = blockIdx.z;
    const int qrows = S - q0 < 32 ? S - q0 : 32;                      // rows of this block that exist: a row past them is never read
    const int Sc = CAUSAL ? q0 + 32 : Sp;                             // the key columns the chunk loops cover (q0 + 32 <= Sp)
    const float* kg = a.k + int64_t(b) * a.sbk + head * D;
    const float* vg = a.v + int64_t(b) * a.sbv + head * D;
    [[maybe_unused]] unsigned long long* const call = rng_call_slot<DROP>();
    [[maybe_unused]] int order = 0, grp = 0, groups = 0;
    [[maybe_unused]] int* tickets = nullptr;
    [[maybe_unused]] int* mine = nullptr;
    if constexpr (DROP) {
        tickets = rng_tickets(a.drop.state);
        grp = grid_linear_block() / a.drop.group;
        groups = (grid_blocks() + a.drop.group - 1) / a.drop.group;
        mine = tickets + (1 + grp) * kRngLine;
        if (tid == 0) {
            rng_read_call(a.drop.state, call);                        // `draws` is in a register before the ticket is taken
            if (grid_linear_block() == 0) a.drop.base[0] = call[1];
            order = rng_take_ticket(mine);
        }
    }

    af32x4 rc[NA];
    {
        af32x4 rq[NB];
        load_rows<D, NB>(rq, a.q + int64_t(b) * a.sbq + int64_t(q0) * a.ldq + head * D, a.ldq, qrows);
        chunk_load<D, NA>(rc, kg, a.ldk, 0, S);
        store_rows_padded<D, NB>(rq, Qs, PQ, qrows, 32);
        // (1.0 - mask) * -10000.0 in fp32, the composite's own arithmetic (bert.py:82); -0.0f where the mask is 1 or absent:
        // adding it changes no bit of a score
        for (int j = tid; j < Sp; j += 256) Bias[j] = (j < S && a.mask) ? (1.0f - a.mask[int64_t(b) * a.sbm + j]) * -10000.0f : -0.0f;
    }

    // scores: the keys arrive in chunks of 128; wave w takes keys [c0 + 32 w, c0 + 32 w + 32) of the chunk, scaled (the product
    // rounded to fp32 first, like `scores * c`)
    // (CAUSAL: columns [Sc, Sp) of the tile are never written: the softmax below deselects them before it looks at them)
    for (int c0 = 0; c0 < Sc; c0 += kLongChunk) {
        chunk_store<D, NA>(rc, Buf, PQ, c0, S, Sc);
        __syncthreads();
        if (c0 + kLongChunk < Sc) chunk_load<D, NA>(rc, kg, a.ldk, c0 + kLongChunk, S);
        else                      chunk_load<D, NA>(rc, vg, a.ldv, 0, S);                 // the first chunk of V flies behind the softmax
        const int rows = Sc - c0 < kLongChunk ? Sc - c0 : kLongChunk;
        if (32 * wave < rows) {
            af32x16 acc = zero16();
            wave_mma<true, true>(acc, Qs, PQ, Buf + 32 * wave * PQ, PQ, D, r, h);
            const int col = c0 + 32 * wave + r;
            const float bias = Bias[col];
#pragma unroll
            for (int e = 0; e < 16; ++e) Ps[acc_row(e, h) * PP + col] = acc[e] * a.scale + bias;
        }
        __syncthreads();
    }

    // softmax of each row: 8 threads per row, float4 columns sub, sub + 8, ... held in registers between the three passes;
    // exp(x - max) * (1 / sum) (autograd/ops.py:62-66) over the keys that exist: a key >= S is no part of the max or the sum,
    // its column of the LDS tile becomes 0 (it is an MFMA operand of the context) and nothing of it is stored
    {
        // (the barriers of the score chunks lie between thread 0's write of the call and these reads)
        [[maybe_unused]] unsigned long long seed = 0, base = 0;
        if constexpr (DROP) { seed = rng_uniform64(call[0]); base = rng_uniform64(call[1]); }
        const int row = tid >> 3, sub = tid & 7;
        // the keys of this row: [0, S), CAUSAL [0, min(S, q0 + row + 1)) - key 0 is always one of them
        const int vis = CAUSAL ? (q0 + row + 1 < S ? q0 + row + 1 : S) : S;
        float* pr = Ps + row * PP;
        af32x4 t[kLongMaxBlocks];
        float m = -INFINITY;
#pragma unroll
        for (int i = 0; i < kLongMaxBlocks; ++i) {
            const int c = sub * 4 + 32 * i;
            if (c < Sp) {
                t[i] = *reinterpret_cast<const af32x4*>(pr + c);
#pragma unroll
                for (int e = 0; e < 4; ++e)
                    if (c + e < vis) m = (t[i][e] > m || t[i][e] != t[i][e]) ? t[i][e] : m;
            }
        }
#pragma unroll
        for (int off = 1; off < 8; off <<= 1) { const float o = __shfl_xor(m, off, 64); m = (o > m || o != o) ? o : m; }
        float s = 0.f;
#pragma unroll
        for (int i = 0; i < kLongMaxBlocks; ++i) {
            const int c = sub * 4 + 32 * i;
            if (c < Sp) {
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    if (c + e < vis) { t[i][e] = expf(t[i][e] + (-m)); s += t[i][e]; }
                    else t[i][e] = 0.f;
                }
            }
        }
#pragma unroll
        for (int off = 1; off < 8; off <<= 1) s += __shfl_xor(s, off, 64);
        const float inv = 1.0f / s;
        const bool row_exists = row < qrows;
        float* pg = a.p + ((int64_t(b) * a.heads + head) * S + q0 + row) * S;
#pragma unroll
        for (int i = 0; i < kLongMaxBlocks; ++i) {
            const int c = sub * 4 + 32 * i;
            if (c < Sp) {
#pragma unroll
                for (int e = 0; e < 4; ++e) t[i][e] *= inv;
                // (DROP: a key >= S holds 0 and stays 0 whatever word it meets; a row >= S is never stored)
                if constexpr (DROP) *reinterpret_cast<af32x4*>(pr + c) = drop4<false>(t[i], (pg - a.p) + c, seed, base, a.drop.threshold, a.drop.s);
                else                *reinterpret_cast<af32x4*>(pr + c) = t[i];
                if (row_exists) {
                    if ((S & 3) == 0) {
                        if (c < S) *reinterpret_cast<af32x4*>(pg + c) = t[i];
                    } else {
#pragma unroll
                        for (int e = 0; e < 4; ++e)
                            if (c + e < S) pg[c + e] = t[i][e];
                    }
                }
            }
        }
    }

    // context = P @ V: D / 32 column tiles, the keys of every chunk split over the remaining waves; the partial sums stay in
    // registers across the chunks and fold in wave order at the end
    constexpr int NT = D / 32, KP = 4 / NT;
    const int n = wave % NT, kp = wave / NT;
    af32x16 acc = zero16();
    for (int c0 = 0; c0 < Sc; c0 += kLongChunk) {
        chunk_store<D, NA>(rc, Buf, PV, c0, S, Sc);
        __syncthreads();                                              // (the first one also publishes the probabilities in LDS)
        if (c0 + kLongChunk < Sc) chunk_load<D, NA>(rc, vg, a.ldv, c0 + kLongChunk, S);
        const int rows = Sc - c0 < kLongChunk ? Sc - c0 : kLongChunk, kspan = rows / KP;
        wave_mma<true, false>(acc, Ps + c0 + kp * kspan, PP, Buf + kp * kspan * PV + 32 * n, PV, kspan, r, h);
        __syncthreads();
    }
    if (kp > 0) {
#pragma unroll
        for (int e = 0; e < 16; ++e) Red[((kp - 1) * NT + n) * 1024 + e * 64 + lane] = acc[e];
    }
    __syncthreads();
    if (kp == 0) {
        for (int q = 1; q < KP; ++q) {
#pragma unroll
            for (int e = 0; e < 16; ++e) acc[e] += Red[((q - 1) * NT + n) * 1024 + e * 64 + lane];
        }
        float* og = a.o + int64_t(b) * a.sbo + int64_t(q0) * a.ldo + head * D + 32 * n + r;
#pragma unroll
        for (int e = 0; e < 16; ++e)
            if (acc_row(e, h) < qrows) og[int64_t(acc_row(e, h)) * a.ldo] = acc[e];
    }
    if constexpr (DROP) {
        if (tid == 0)
            rng_last_arriver_advances(a.drop.state, tickets, mine, order, grp, groups, a.drop.group, grid_blocks(), rng_uniform64(call[1]));
    }
}

// floats of LDS: the larger of the two roles
template <int D>
constexpr int attn_long_bwd_lds_floats(int Sp) {
    const int query = 32 * (D + 4) + 32 * (Sp + 4) + kLongChunk * (D + 8) + 3 * 1024;
    const int key = 2 * kLongChunk * (D + 8) + 32 * (D + 4) + 2 * kLongChunk * 40 + 2048;
    return query > key ? query : key;
}

// DROP: the mask of the forward again, from the seed in the generator's state and the call number the forward wrote; nothing
// is drawn.  dP is masked in both roles after the same MFMA sequence (one multiply, the same bits); the key role forms dS from
// the undropped P[chunk, block] in registers and stores that tile under the mask for dV: no second tile.
template <int D, bool DROP = false>
__global__ void __launch_bounds__(256) attn_long_bwd(std::conditional_t<DROP, AttnBwdDropArgs, AttnBwdArgs> a) {
    extern __shared__ __attribute__((aligned(16))) float lds[];
    const int S = a.S, Sp = round32(S);           // the sequence / what the tiles, the shift slab and the hand-off counter cover
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, r = lane & 31, h = lane >> 5;
    // the query-role workgroups of the whole grid are dispatched before any key-role one (role in the slowest grid index): a
    // key-role workgroup that waits, waits for workgroups that are already running and wait for nothing
    const int role = int(blockIdx.z) >= a.batch ? 1 : 0;
    const int blk = blockIdx.x, head = blockIdx.y, b = int(blockIdx.z) - role * a.batch;
    const int j0 = blk * 32, nblk = Sp / 32;
    const int brows = S - j0 < 32 ? S - j0 : 32;     // rows of this block that exist
    const int bh = b * a.heads + head;
    const float* pg = a.p + int64_t(bh) * S * S;
    double* shifts = a.shift + int64_t(bh) * Sp;
    int* flags = a.flags + 2 * bh;
    constexpr int NT = D / 32;
    constexpr int NB = 32 * (D / 4) / 256 > 0 ? 32 * (D / 4) / 256 : 1, NA = kLongChunk * (D / 4) / 256;
    const float* qg = a.q + int64_t(b) * a.sbq + head * D;
    const float* kg = a.k + int64_t(b) * a.sbk + head * D;
    const float* vg = a.v + int64_t(b) * a.sbv + head * D;
    const float* gg = a.g + int64_t(b) * a.sbg + head * D;
    [[maybe_unused]] unsigned long long seed = 0, base = 0;
    if constexpr (DROP) { seed = a.drop.state[0]; base = a.drop.base[0]; }

    if (role == 0) {
        // ---- query role: dQ of queries [j0, j0 + 32), and the shift of their rows for the key role ------------------
        constexpr int PG = D + 4, PVK = D + 4, PK = D + 8;
        const int PP = Sp + 4;
        float* Gs = lds;                  // dO rows of the block                        32 x PG
        float* Ss = Gs + 32 * PG;         // dP, then dS                                 32 x PP
        float* Buf = Ss + 32 * PP;        // a chunk of V (K-contiguous B of dP, pitch PVK), then of K (N-contiguous B of dQ, pitch PK)
        float* Red = Buf + kLongChunk * PK;
        af32x4 rc[NA];
        {
            af32x4 rg[NB];
            load_rows<D, NB>(rg, gg + int64_t(j0) * a.ldg, a.ldg, brows);
            chunk_load<D, NA>(rc, vg, a.ldv, 0, S);
            store_rows_padded<D, NB>(rg, Gs, PG, brows, 32);
        }
        // the probabilities of this thread's row (tid >> 3), float4 columns (tid & 7) + 8 i, fetched ahead of the MFMAs whose
        // result they meet.  A key >= S has no probability: 0, so the row pass adds nothing for it and its dS is 0.  A row
        // >= brows takes row 0's values: with its dP = 0 the shift it forms is 0 / 1, not 0 / 0.
        af32x4 y[kLongMaxBlocks];
        {
            const int sub = tid & 7, row0 = tid >> 3, row = row0 < brows ? row0 : 0;
            const float* yr = pg + int64_t(j0 + row) * S;
#pragma unroll
            for (int i = 0; i < kLongMaxBlocks; ++i) {
                const int c = sub * 4 + 32 * i;
                y[i] = af32x4{0.f, 0.f, 0.f, 0.f};
                if ((S & 3) == 0) {
                    if (c < S) y[i] = *reinterpret_cast<const af32x4*>(yr + c);
                } else {
#pragma unroll
                    for (int e = 0; e < 4; ++e)
                        if (c + e < S) y[i][e] = yr[c + e];
                }
            }
        }
        for (int c0 = 0; c0 < Sp; c0 += kLongChunk) {
            chunk_store<D, NA>(rc, Buf, PVK, c0, S, Sp);
            __syncthreads();
            if (c0 + kLongChunk < Sp) chunk_load<D, NA>(rc, vg, a.ldv, c0 + kLongChunk, S);
            else                      chunk_load<D, NA>(rc, kg, a.ldk, 0, S);             // the first chunk of K flies behind the row pass
            const int rows = Sp - c0 < kLongChunk ? Sp - c0 : kLongChunk;
            if (32 * wave < rows) {
                af32x16 acc = zero16();
                wave_mma<true, true>(acc, Gs, PG, Buf + 32 * wave * PVK, PVK, D, r, h);
                const int col = c0 + 32 * wave + r;
#pragma unroll
                for (int e = 0; e < 16; ++e) Ss[acc_row(e, h) * PP + col] = acc[e];
            }
            __syncthreads();
        }
        // dS = float(double(y) * (double(dP) - shift)) * scale, shift = sum(dP * y) / sum(y) over the row in double (rowwise.hip:
        // softmax_bwd explains why), in place; 8 threads per row.  The shift of every row that exists is published
        // (write-through: workgroups on other XCDs read it).
        {
            const int sub = tid & 7, row = tid >> 3;
            float* gr = Ss + row * PP;
            double dot = 0.0, norm = 0.0;
#pragma unroll
            for (int i = 0; i < kLongMaxBlocks; ++i) {
                const int c = sub * 4 + 32 * i;
                if (c < Sp) {
                    af32x4 g4 = *reinterpret_cast<const af32x4*>(gr + c);
                    if constexpr (DROP) {
                        // what the MFMAs left is dO V^T: dP is that under the forward's mask, kept for the pass below (this
                        // thread's own float4: no barrier); the shift is formed from the masked dP
                        g4 = drop4<false>(g4, (int64_t(bh) * S + j0 + row) * S + c, seed, base, a.drop.threshold, a.drop.s);
                        *reinterpret_cast<af32x4*>(gr + c) = g4;
                    }
#pragma unroll
                    for (int e = 0; e < 4; ++e) { const double yc = double(y[i][e]); dot += double(g4[e]) * yc; norm += yc; }
                }
            }
#pragma unroll
            for (int off = 1; off < 8; off <<= 1) { dot += __shfl_xor(dot, off, 64); norm += __shfl_xor(norm, off, 64); }
            const double shift = dot / norm;
            if (sub == 0 && row < brows) __hip_atomic_store(shifts + j0 + row, shift, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
#pragma unroll
            for (int i = 0; i < kLongMaxBlocks; ++i) {
                const int c = sub * 4 + 32 * i;
                if (c < Sp) {
                    af32x4 g4 = *reinterpret_cast<const af32x4*>(gr + c);
#pragma unroll
                    for (int e = 0; e < 4; ++e) g4[e] = float(double(y[i][e]) * (double(g4[e]) - shift)) * a.scale;
                    *reinterpret_cast<af32x4*>(gr + c) = g4;
                }
            }
        }
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");             // the shifts have left this CU
        __syncthreads();
        if (tid == 0) __hip_atomic_fetch_add(flags, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);      // 32 more rows are published
        constexpr int KP = 4 / NT;
        const int n = wave % NT, kp = wave / NT;
        af32x16 acc = zero16();
        for (int c0 = 0; c0 < Sp; c0 += kLongChunk) {
            chunk_store<D, NA>(rc, Buf, PK, c0, S, Sp);
            __syncthreads();
            if (c0 + kLongChunk < Sp) chunk_load<D, NA>(rc, kg, a.ldk, c0 + kLongChunk, S);
            const int rows = Sp - c0 < kLongChunk ? Sp - c0 : kLongChunk, kspan = rows / KP;
            wave_mma<true, false>(acc, Ss + c0 + kp * kspan, PP, Buf + kp * kspan * PK + 32 * n, PK, kspan, r, h);
            __syncthreads();
        }
        if (kp > 0) {
#pragma unroll
            for (int e = 0; e < 16; ++e) Red[((kp - 1) * NT + n) * 1024 + e * 64 + lane] = acc[e];
        }
        __syncthreads();
        if (kp == 0) {
            for (int q = 1; q < KP; ++q) {
#pragma unroll
                for (int e = 0; e < 16; ++e) acc[e] += Red[((q - 1) * NT + n) * 1024 + e * 64 + lane];
            }
            float* dst = a.dq + int64_t(b) * a.sbdq + int64_t(j0) * a.lddq + head * D + 32 * n + r;
#pragma unroll
            for (int e = 0; e < 16; ++e)
                if (acc_row(e, h) < brows) dst[int64_t(acc_row(e, h)) * a.lddq] = acc[e];
        }
        return;
    }

    // ---- key role: dK and dV of keys [j0, j0 + 32) --------------------------------------------------------------
    // dS[:, block] = P[:, block] o (dP[:, block] - shift) * scale needs dP only for the block's own keys - and the shift of EVERY
    // row, which the query-role workgroups of this (batch, head) publish; a counter says how many of them have.  The queries
    // arrive in chunks of 128: per chunk dO and Q rows, P[chunk, block] and dS[chunk, block]; wave w forms dP of queries
    // [c0 + 32 w, c0 + 32 w + 32) against the block's V rows.  dV and dK accumulate in registers across the chunks.
    constexpr int PG = D + 8;             // dO: K-contiguous A of dP (two-way conflicts there) and N-contiguous B of dV
    constexpr int PVK = D + 4, PQN = D + 8, PC = 40;
    float* Gs = lds;                      // dO rows of the chunk          128 x PG
    float* Qs = Gs + kLongChunk * PG;     // Q, N-contiguous B of dK       128 x PQN
    float* Vj = Qs + kLongChunk * PQN;    // V rows of the block           32 x PVK
    float* Pc = Vj + 32 * PVK;            // P[chunk, block]               128 x PC
    float* Dc = Pc + kLongChunk * PC;     // dS[chunk, block]              128 x PC
    float* Red = Dc + kLongChunk * PC;
    af32x4 rg[NA], rq[NA];
    {
        af32x4 rv[NB];
        load_rows<D, NB>(rv, vg + int64_t(j0) * a.ldv, a.ldv, brows);
        chunk_load<D, NA>(rg, gg, a.ldg, 0, S);
        chunk_load<D, NA>(rq, qg, a.ldq, 0, S);
        store_rows_padded<D, NB>(rv, Vj, PVK, brows, 32);
    }
    // dV = P[:, block]^T @ dO and dK = dS[:, block]^T @ Q: 2 * NT output tiles of 32 x 32 over four waves
    constexpr int TILES = 2 * NT, KP = 4 / TILES > 0 ? 4 / TILES : 1;
    const int tile = wave % TILES, kp = wave / TILES;
    const bool is_dk = tile >= NT;
    const int n = tile % NT;
    af32x16 acc = zero16();
    for (int c0 = 0; c0 < Sp; c0 += kLongChunk) {
        chunk_store<D, NA>(rg, Gs, PG, c0, S, Sp);
        chunk_store<D, NA>(rq, Qs, PQN, c0, S, Sp);
        __syncthreads();
        if (c0 + kLongChunk < Sp) {
            chunk_load<D, NA>(rg, gg, a.ldg, c0 + kLongChunk, S);
            chunk_load<D, NA>(rq, qg, a.ldq, c0 + kLongChunk, S);
        }
        const int rows = Sp - c0 < kLongChunk ? Sp - c0 : kLongChunk;
        const bool active = 32 * wave < rows;
        // the probabilities that meet this wave's block of dP: element e of the accumulator is (row c0 + 32 w + acc_row(e, h), key
        // j0 + r); a (row, key) pair past the sequence has no probability: 0, so its dS and its share of dK / dV are 0
        float y[16];
        af32x16 dp = zero16();
        if (active) {
#pragma unroll
            for (int e = 0; e < 16; ++e) {
                const int row = c0 + 32 * wave + acc_row(e, h);
                const bool in = row < S && r < brows;
                const float t = pg[in ? int64_t(row) * S + j0 + r : 0];
                y[e] = in ? t : 0.f;
            }
            wave_mma<true, true>(dp, Gs + 32 * wave * PG, PG, Vj, PVK, D, r, h);
        }
        if (c0 == 0) {
            // wait for the shifts of all S rows
            if (tid == 0) {
                // (bounded: 2 s of the 100 MHz wall clock, then the device status flag is raised and the launch runs to its end)
                const unsigned long long t0 = wall_clock64();
                while (__hip_atomic_load(flags, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) < nblk) {
                    __builtin_amdgcn_s_sleep(1);
                    if (wall_clock64() - t0 > 200000000ull) {
                        __hip_atomic_fetch_or(a.status, LG_STATUS_HANDOFF_TIMEOUT, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
                        break;
                    }
                }
            }
            __syncthreads();
            __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
        }
        if (active) {
            double sh[16];
#pragma unroll
            for (int e = 0; e < 16; ++e) {
                const int row = c0 + 32 * wave + acc_row(e, h);
                sh[e] = __hip_atomic_load(shifts + row, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                sh[e] = row < S ? sh[e] : 0.0;                       // no row, nothing published: not read as a number
            }
#pragma unroll
            for (int e = 0; e < 16; ++e) {
                const int row = 32 * wave + acc_row(e, h);
                if constexpr (DROP) {
                    // element (c0 + row, j0 + r); a pair past the sequence has y = 0: 0 either way
                    const uint32_t word = rng_word((int64_t(bh) * S + c0 + row) * S + j0 + r, seed, base);
                    Dc[row * PC + r] = float(double(y[e]) * (double(rng_keep(dp[e], word, a.drop.threshold, a.drop.s)) - sh[e])) * a.scale;
                    Pc[row * PC + r] = rng_keep(y[e], word, a.drop.threshold, a.drop.s);
                } else {
                    Dc[row * PC + r] = float(double(y[e]) * (double(dp[e]) - sh[e])) * a.scale;
                    Pc[row * PC + r] = y[e];
                }
            }
        }
        __syncthreads();
        const int kspan = rows / KP;
        if (is_dk) wave_mma<false, false>(acc, Dc + kp * kspan * PC, PC, Qs + kp * kspan * PQN + 32 * n, PQN, kspan, r, h);
        else       wave_mma<false, false>(acc, Pc + kp * kspan * PC, PC, Gs + kp * kspan * PG + 32 * n, PG, kspan, r, h);
        __syncthreads();
    }
    // every wave has read all its shifts: this workgroup is served; the last one of the (batch, head) pair clears the counters
    if (tid == 0) {
        const int served = __hip_atomic_fetch_add(flags + 1, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (served == nblk - 1) {
            __hip_atomic_store(flags, 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            __hip_atomic_store(flags + 1, 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
    }
    if constexpr (KP > 1) {
        if (kp > 0) {
#pragma unroll
            for (int e = 0; e < 16; ++e) Red[(kp - 1) * TILES * 1024 + tile * 1024 + e * 64 + lane] = acc[e];
        }
        __syncthreads();
        if (kp > 0) return;
        for (int q = 1; q < KP; ++q) {
#pragma unroll
            for (int e = 0; e < 16; ++e) acc[e] += Red[(q - 1) * TILES * 1024 + tile * 1024 + e * 64 + lane];
        }
    }
    float* dst = is_dk ? a.dk + int64_t(b) * a.sbdk + int64_t(j0) * a.lddk + head * D + 32 * n + r
                       : a.dv + int64_t(b) * a.sbdv + int64_t(j0) * a.lddv + head * D + 32 * n + r;
    const int64_t ldd = is_dk ? a.lddk : a.lddv;
#pragma unroll
    for (int e = 0; e < 16; ++e)
        if (acc_row(e, h) < brows) dst[int64_t(acc_row(e, h)) * ldd] = acc[e];
}

// ---- the launchers behind attn_forward / attn_backward (attention.hip): LDS size, allow_lds, launch -----------------------------
template <int D, bool DROP, bool CAUSAL = false>
static int launch_long_fwd_as(const AttnDropArgs& a, dim3 grid) {
    const size_t bytes = size_t(attn_long_fwd_lds_floats<D>(round32(a.S))) * 4;
    int rc = allow_lds(&attn_long_fwd<D, DROP, CAUSAL>, bytes);
    if (rc != LG_OK) return rc;
    hipLaunchKernelGGL((attn_long_fwd<D, DROP, CAUSAL>), grid, dim3(256), bytes, rt().stream, a);
    return LG_OK;
}

template <int D, bool DROP>
static int launch_long_bwd_as(const AttnBwdDropArgs& a, dim3 grid) {
    const size_t bytes = size_t(attn_long_bwd_lds_floats<D>(round32(a.S))) * 4;
    int rc = allow_lds(&attn_long_bwd<D, DROP>, bytes);
    if (rc != LG_OK) return rc;
    hipLaunchKernelGGL((attn_long_bwd<D, DROP>), grid, dim3(256), bytes, rt().stream, a);
    return LG_OK;
}

int attn_long_launch_fwd(const AttnDropArgs& a, dim3 grid, int64_t D, bool drop, bool causal) {
    static int (*const table[2][2][2])(const AttnDropArgs&, dim3) = {          // [causal][D == 64][drop]
        {{launch_long_fwd_as<32, false>, launch_long_fwd_as<32, true>}, {launch_long_fwd_as<64, false>, launch_long_fwd_as<64, true>}},
        {{launch_long_fwd_as<32, false, true>, launch_long_fwd_as<32, true, true>},
         {launch_long_fwd_as<64, false, true>, launch_long_fwd_as<64, true, true>}}};
    return table[causal][D == 64][drop](a, grid);
}

int attn_long_launch_bwd(const AttnBwdDropArgs& a, dim3 grid, int64_t D, bool drop) {
    static int (*const table[2][2])(const AttnBwdDropArgs&, dim3) = {          // [D == 64][drop]
        {launch_long_bwd_as<32, false>, launch_long_bwd_as<32, true>}, {launch_long_bwd_as<64, false>, launch_long_bwd_as<64, true>}};
    return table[D == 64][drop](a, grid);
}

}  // namespace lg

using namespace lg;

extern "C" int lg_attention_long_supported(int64_t S, int64_t D) {
    return (D == 64 || D == 32) && S >= 129 && S <= 512;
}

static const AttnFamily kLong{"lg_attention_long_fwd_f32", "lg_attention_long_bwd_f32", lg_attention_long_supported, "129..512", AttnForm::Long};

extern "C" int lg_attention_long_fwd_f32(const float* q, int64_t ldq, int64_t sbq, const float* k, int64_t ldk, int64_t sbk,
                                         const float* v, int64_t ldv, int64_t sbv, float* o, int64_t ldo, int64_t sbo, float* p,
                                         int64_t batch, int64_t heads, int64_t S, int64_t D, float scale,
                                         const float* mask, int64_t sbm) {
    LG_REQUIRE_INIT();
    return attn_forward(kLong, {{q, ldq, sbq}, {k, ldk, sbk}, {v, ldv, sbv}, {o, ldo, sbo}, p, batch, heads, S, D, scale, mask, sbm, 0.0, nullptr});
}

extern "C" int lg_attention_long_bwd_f32(const float* q, int64_t ldq, int64_t sbq, const float* k, int64_t ldk, int64_t sbk,
                                         const float* v, int64_t ldv, int64_t sbv, const float* g, int64_t ldg, int64_t sbg,
                                         const float* p, float* dq, int64_t lddq, int64_t sbdq, float* dk, int64_t lddk, int64_t sbdk,
                                         float* dv, int64_t lddv, int64_t sbdv, int64_t batch, int64_t heads, int64_t S, int64_t D,
                                         float scale) {
    LG_REQUIRE_INIT();
    return attn_backward(kLong, {{q, ldq, sbq}, {k, ldk, sbk}, {v, ldv, sbv}, {g, ldg, sbg}, p, {dq, lddq, sbdq}, {dk, lddk, sbdk},
                                 {dv, lddv, sbdv}, batch, heads, S, D, scale, 0.0, nullptr});
}
