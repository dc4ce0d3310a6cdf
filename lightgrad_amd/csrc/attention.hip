// Self-attention of a short sequence in one launch each way (gfx950, fp32 MFMA).
//
//   forward    P = softmax((Q K^T) * scale)   O = P V          per (batch, head), reference examples/bert.py:78-88
//   backward   dV = P^T dO   dP = dO V^T   dS = P o (dP - shift) * scale   dQ = dS K   dK = dS^T Q
//
// The composite form is five launches forward (three Linear products apart: scores GEMM, scaled softmax, context GEMM) and
// three backward (two two-product launches and the softmax backward), each a few microseconds of work behind a launch
// floor of its own; at tiny-BERT's size (S = 128, D = 64, 16 (batch, head) pairs) everything one (batch, head) pair needs
// fits the LDS of one CU.  The scores never reach HBM; the probabilities do, once: the model returns them
// (bert.py:88) and the backward reads them instead of recomputing the softmax.
//
// Work split.  Forward: one workgroup per (batch, head, block of 32 queries).  Backward: two roles, one workgroup each per
// (batch, head, block of 32): the QUERY role makes dQ of its 32 queries, the KEY role dK and dV of its 32 keys.  The key role
// needs dS[:, block] for ALL queries: dP only for its own keys (32 MFMAs per wave) but the softmax shift of every row, a sum
// over the whole row of dP.  The query-role workgroups form those sums anyway and hand them over inside the launch: each
// publishes its 32 shifts (write-through doubles) and raises a counter of its (batch, head) pair; a key-role workgroup waits
// for the counter to reach S / 32.  The query-role workgroups fill the front of the grid, so whoever waits, waits for
// workgroups that are already running and wait for nothing; the wait is bounded (2 s, then the device status flag).  The
// first version recomputed dP for all queries in the key role instead (128 MFMAs per wave and a row pass over S rows:
// 14.8 us for the role against 11.6 us with the hand-off, tools/attn_timeline.py).  Both roles run the same MFMA sequence on the
// same operands, so their dP - and dS - agree bit for bit.  The shift is formed in double exactly like the separate softmax
// backward (rowwise.hip: softmax_bwd explains why).
//
// MFMA operands come from LDS.  v_mfma_f32_32x32x2f32 takes one float per lane: lane (r, h) = (lane & 31, lane >> 5) holds
// A[r][k + h] and B[k + h][r].  Any order of the k values will do as long as A and B agree, so a wave walks K in groups of
// 8 with lane half h on k = 8j + 4h .. 8j + 4h + 3: an operand that is contiguous along K is then ONE ds_read_b128 per
// four MFMAs, the others four ds_read_b32 of 32 consecutive floats.  Row pitches: K-contiguous rows + 4 floats (16 lanes of a
// b128 read hit 16 different 16-byte slots), M/N-contiguous rows = 8 mod 16 floats (the two lane halves, 4 rows apart, land
// on different halves of the 64 banks).
//
// TAIL instantiations (lg_attention_masked_*): any S in 1 .. 128 and an additive per-key bias from a padding mask (reference
// examples/bert.py:80-83: scores + (1 - mask) * -10000).  Everything above runs on Sp = S rounded up to 32 - grid, LDS, MFMA K
// spans, hand-off counter - with the LDS operand rows [S, Sp) ZERO (not whatever the LDS held: NaN * 0 would reach the sums);
// the softmax takes keys >= S out by selection, global rows >= S are neither read nor written, and the probabilities
// (row pitch S, not 16-byte aligned unless S % 4 == 0) go out and come in as scalars.  The TAIL = false instantiations are
// the kernels as they were.
//
// Layout.  attention_common.h has what this file and attention_long.hip share: the argument structs, the small device helpers, and
// the host interface.  This file has the short kernels (attn_fwd: <D, TAIL, DROP, CAUSAL>, attn_bwd: <D, TAIL, DROP>), their
// launchers, and the ONE host path of all nine lg_attention_*_f32 launch entries - attn_forward / attn_backward: the checks in one
// order, the selection of the kernels (pick_form), the `shift` slab allocated and freed in one place - plus the plain, masked,
// dropout and causal entries, which only fill a call struct and name their family.  attention_long.hip adds the long kernels,
// their launchers and entries.
#include "attention_common.h"

namespace lg {

template <int D>
constexpr int attn_fwd_lds_floats(int S) { return 32 * (D + 4) + S * (D + 4) + S * (D + 8) + 32 * (S + 4) + 3 * 1024; }
// TAIL: the same layout over Sp rows and the per-key bias behind it
template <int D>
constexpr int attn_fwd_tail_lds_floats(int S) { return attn_fwd_lds_floats<D>(round32(S)) + 128; }

// DROP: dropout of the probabilities between the softmax and the context, from the stream of dropout.hip (one call per launch:
// read `draws`, take a ticket, the last arriver advances).  P goes to HBM undropped; what feeds the context MFMAs is Pd.
// CAUSAL (TAIL only): query i sees keys j <= i.  The selection that takes keys >= S out of the softmax also takes out keys
// j > q0 + row: no part of the max or the sum, 0 in the LDS tile, +0.0 stored to P (the backward reads the whole dense tensor).
// A wave whose 32 keys all lie above the block's diagonal leaves its score MFMAs out: what it would have written is deselected.
template <int D, bool TAIL = false, bool DROP = false, bool CAUSAL = false>
__global__ void __launch_bounds__(256) attn_fwd(std::conditional_t<DROP, AttnDropArgs, std::conditional_t<TAIL, AttnTailArgs, AttnArgs>> a) {
    static_assert(TAIL || !CAUSAL, "the causal selection lives in the TAIL softmax");
    extern __shared__ __attribute__((aligned(16))) float lds[];
    const int S = a.S;                               // the sequence
    const int Sp = TAIL ? round32(S) : S;            // what the tiles cover
    constexpr int PQ = D + 4, PV = D + 8;
    const int PP = Sp + 4;
    float* Qs = lds;
    float* Ks = Qs + 32 * PQ;
    float* Vs = Ks + Sp * PQ;
    float* Ps = Vs + Sp * PV;
    float* Red = Ps + 32 * PP;
    [[maybe_unused]] float* Bias = Red + 3 * 1024;   // TAIL: what key j adds to every score of its column
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, r = lane & 31, h = lane >> 5;
    const int q0 = blockIdx.x * 32, head = blockIdx.y, b = blockIdx.z;
    LG_ATL(0);
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

    {
        constexpr int NB = 32 * (D / 4) / 256 > 0 ? 32 * (D / 4) / 256 : 1, NA = 128 * (D / 4) / 256;   // float4 per thread: 32 rows / all rows
        af32x4 rq[NB], rk[NA], rv[NA];
        if constexpr (!TAIL) {
            load_rows<D, NB>(rq, a.q + int64_t(b) * a.sbq + int64_t(q0) * a.ldq + head * D, a.ldq, 32);
            load_rows<D, NA>(rk, a.k + int64_t(b) * a.sbk + head * D, a.ldk, S);
            load_rows<D, NA>(rv, a.v + int64_t(b) * a.sbv + head * D, a.ldv, S);
            store_rows<D, NB>(rq, Qs, PQ, 32);
            store_rows<D, NA>(rk, Ks, PQ, S);
            store_rows<D, NA>(rv, Vs, PV, S);
        } else {
            const int qrows = S - q0 < 32 ? S - q0 : 32;                  // rows of this block that exist: a row past them is never read
            load_rows<D, NB>(rq, a.q + int64_t(b) * a.sbq + int64_t(q0) * a.ldq + head * D, a.ldq, qrows);
            load_rows<D, NA>(rk, a.k + int64_t(b) * a.sbk + head * D, a.ldk, S);
            load_rows<D, NA>(rv, a.v + int64_t(b) * a.sbv + head * D, a.ldv, S);
            store_rows_padded<D, NB>(rq, Qs, PQ, qrows, 32);
            store_rows_padded<D, NA>(rk, Ks, PQ, S, Sp);
            store_rows_padded<D, NA>(rv, Vs, PV, S, Sp);
            // (1.0 - mask) * -10000.0 in fp32, the composite's own arithmetic (bert.py:82); -0.0f where the mask is 1 or absent:
            // adding it changes no bit of a score
            if (tid < Sp) Bias[tid] = (tid < S && a.mask) ? (1.0f - a.mask[int64_t(b) * a.sbm + tid]) * -10000.0f : -0.0f;
        }
    }
    __syncthreads();
    LG_ATL(1);
    [[maybe_unused]] unsigned long long seed = 0, base = 0;
    if constexpr (DROP) { seed = rng_uniform64(call[0]); base = rng_uniform64(call[1]); }

    // scores of 32 queries against keys [32 wave, 32 wave + 32), scaled (the product rounded to fp32 first, like `scores * c`)
    bool has_scores = 32 * wave < Sp;
    // (CAUSAL: keys wholly above the diagonal of the block are no one's: their columns of the tile stay stale, loaded by the
    // softmax and never used - the bound is the same for the whole wave)
    if constexpr (CAUSAL) has_scores = has_scores && 32 * wave <= q0 + 31;
    if (has_scores) {
        af32x16 acc = zero16();
        wave_mma<true, true>(acc, Qs, PQ, Ks + 32 * wave * PQ, PQ, D, r, h);
        if constexpr (TAIL) {
            const float bias = Bias[32 * wave + r];
#pragma unroll
            for (int e = 0; e < 16; ++e) Ps[acc_row(e, h) * PP + 32 * wave + r] = acc[e] * a.scale + bias;
        } else {
#pragma unroll
            for (int e = 0; e < 16; ++e) Ps[acc_row(e, h) * PP + 32 * wave + r] = acc[e] * a.scale;
        }
    }
    __syncthreads();
    LG_ATL(2);

    // softmax of each row: 8 threads per row, float4 columns sub, sub + 8, ... held in registers between the three passes;
    // exp(x - max) * (1 / sum) (autograd/ops.py:62-66)
    if constexpr (TAIL) {
        // the same three passes in the same order over the keys that exist: a key >= S is no part of the max or the sum, its
        // column of the LDS tile becomes 0 (it is an MFMA operand of the context) and nothing of it is stored
        const int row = tid >> 3, sub = tid & 7;
        // the keys of this row: [0, S), CAUSAL [0, min(S, q0 + row + 1)) - key 0 is always one of them
        const int vis = CAUSAL ? (q0 + row + 1 < S ? q0 + row + 1 : S) : S;
        float* pr = Ps + row * PP;
        af32x4 t[4];
        float m = -INFINITY;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
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
        for (int i = 0; i < 4; ++i) {
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
        const bool row_exists = q0 + row < S;
        float* pg = a.p + ((int64_t(b) * a.heads + head) * S + q0 + row) * S;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
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
    } else {
        const int row = tid >> 3, sub = tid & 7;
        float* pr = Ps + row * PP;
        af32x4 t[4];
        float m = -INFINITY;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int c = sub * 4 + 32 * i;
            if (c < S) {
                t[i] = *reinterpret_cast<const af32x4*>(pr + c);
#pragma unroll
                for (int e = 0; e < 4; ++e) m = (t[i][e] > m || t[i][e] != t[i][e]) ? t[i][e] : m;
            }
        }
#pragma unroll
        for (int off = 1; off < 8; off <<= 1) { const float o = __shfl_xor(m, off, 64); m = (o > m || o != o) ? o : m; }
        float s = 0.f;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            if (sub * 4 + 32 * i < S) {
#pragma unroll
                for (int e = 0; e < 4; ++e) { t[i][e] = expf(t[i][e] + (-m)); s += t[i][e]; }
            }
        }
#pragma unroll
        for (int off = 1; off < 8; off <<= 1) s += __shfl_xor(s, off, 64);
        const float inv = 1.0f / s;
        float* pg = a.p + ((int64_t(b) * a.heads + head) * S + q0 + row) * S;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int c = sub * 4 + 32 * i;
            if (c < S) {
#pragma unroll
                for (int e = 0; e < 4; ++e) t[i][e] *= inv;
                // (DROP: S % 32 == 0 here, so a float4 of a row is one group of the stream)
                if constexpr (DROP) *reinterpret_cast<af32x4*>(pr + c) = drop4<true>(t[i], (pg - a.p) + c, seed, base, a.drop.threshold, a.drop.s);
                else                *reinterpret_cast<af32x4*>(pr + c) = t[i];
                *reinterpret_cast<af32x4*>(pg + c) = t[i];
            }
        }
    }
    __syncthreads();
    LG_ATL(3);

    // context = P @ V: D / 32 column tiles, the keys split over the remaining waves, partial sums folded in wave order
    constexpr int NT = D / 32, KP = 4 / NT;
    const int n = wave % NT, kp = wave / NT;
    const int kspan = Sp / KP;
    af32x16 acc = zero16();
    wave_mma<true, false>(acc, Ps + kp * kspan, PP, Vs + kp * kspan * PV + 32 * n, PV, kspan, r, h);
    LG_ATL(4);
    if (kp > 0) {
#pragma unroll
        for (int e = 0; e < 16; ++e) Red[((kp - 1) * NT + n) * 1024 + e * 64 + lane] = acc[e];
    }
    __syncthreads();
    LG_ATL(5);
    if (kp == 0) {
        for (int q = 1; q < KP; ++q) {
#pragma unroll
            for (int e = 0; e < 16; ++e) acc[e] += Red[((q - 1) * NT + n) * 1024 + e * 64 + lane];
        }
        float* og = a.o + int64_t(b) * a.sbo + int64_t(q0) * a.ldo + head * D + 32 * n + r;
#pragma unroll
        for (int e = 0; e < 16; ++e)
            if (!TAIL || q0 + acc_row(e, h) < S) og[int64_t(acc_row(e, h)) * a.ldo] = acc[e];
    }
    if constexpr (DROP) {
        if (tid == 0) rng_last_arriver_advances(a.drop.state, tickets, mine, order, grp, groups, a.drop.group, grid_blocks(), base);
    }
    LG_ATL(6);
}

// The probabilities a thread needs for its rows: row = (tid >> 3) + 32 * pass, float4 columns (tid & 7) + 8 * i.  Fetched into
// registers ahead of the MFMAs whose result they meet, so the row pass below never waits for HBM.
template <int PASSES>
struct ProbRows { af32x4 y[PASSES][4]; };

template <int PASSES>
__device__ __forceinline__ void load_probs(ProbRows<PASSES>& pr, const float* y, int S, int rows) {
    const int sub = threadIdx.x & 7;
#pragma unroll
    for (int p = 0; p < PASSES; ++p) {
        const int row0 = (threadIdx.x >> 3) + 32 * p, row = row0 < rows ? row0 : 0;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int c0 = sub * 4 + 32 * i, c = c0 < S ? c0 : 0;
            pr.y[p][i] = *reinterpret_cast<const af32x4*>(y + int64_t(row) * S + c);
        }
    }
}

// TAIL form: rows of pitch S are not 16-byte aligned, and a key >= S has no probability: scalars, 0 where there is none (so the
// row pass below adds nothing for it and its dS is 0).  A row >= rows takes row 0's values like above: with its dP = 0 the
// shift it forms is 0 / 1, not 0 / 0.
template <int PASSES>
__device__ __forceinline__ void load_probs_tail(ProbRows<PASSES>& pr, const float* y, int S, int rows) {
    const int sub = threadIdx.x & 7;
#pragma unroll
    for (int p = 0; p < PASSES; ++p) {
        const int row0 = (threadIdx.x >> 3) + 32 * p, row = row0 < rows ? row0 : 0;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const int c0 = sub * 4 + 32 * i + e, c = c0 < S ? c0 : 0;
                const float t = y[int64_t(row) * S + c];
                pr.y[p][i][e] = c0 < S ? t : 0.f;
            }
        }
    }
}

// dS = float(double(y) * (double(g) - shift)) * scale, shift = sum(g * y) / sum(y) over the row in double, in place, for 32 rows of
// dP held in LDS (pitch pp) against their probabilities y (load_probs); 8 threads per row.  The shift of every row is also
// stored to `shift_out` (write-through: workgroups on other XCDs read it).
// TAIL: only the first `rows` of the 32 rows exist; the others are computed on zeros and publish nothing.
// DROP: what the MFMAs left in LDS is dO V^T; dP is that under the mask of the forward, fl(x * s) or +0.0 (element (row, c) of the
// block is element first + row * pitch + c of the call), and the shift is formed from the masked dP.
struct DropRows {
    unsigned long long seed, base;
    uint32_t threshold;
    float s;
    int64_t first;                   // flat index of (first row of the block, key 0) in the dense (batch, heads, S, S) tensor
    int pitch;                       // S
};

template <bool TAIL, bool DROP = false>
__device__ __forceinline__ void softmax_bwd_rows(float* dp, int pp, const ProbRows<1>& pr, int S, float scale, double* shift_out, int rows,
                                                 [[maybe_unused]] const DropRows& dr = DropRows{}) {
    const int sub = threadIdx.x & 7, row = threadIdx.x >> 3;
    float* gr = dp + row * pp;
    af32x4 g4[4];
    double dot = 0.0, norm = 0.0;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int c = sub * 4 + 32 * i;
        if (c < S) {
            g4[i] = *reinterpret_cast<const af32x4*>(gr + c);
            if constexpr (DROP) g4[i] = drop4<!TAIL>(g4[i], dr.first + int64_t(row) * dr.pitch + c, dr.seed, dr.base, dr.threshold, dr.s);
#pragma unroll
            for (int e = 0; e < 4; ++e) { const double yc = double(pr.y[0][i][e]); dot += double(g4[i][e]) * yc; norm += yc; }
        }
    }
#pragma unroll
    for (int off = 1; off < 8; off <<= 1) { dot += __shfl_xor(dot, off, 64); norm += __shfl_xor(norm, off, 64); }
    const double shift = dot / norm;
    if (sub == 0 && (!TAIL || row < rows)) __hip_atomic_store(shift_out + row, shift, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int c = sub * 4 + 32 * i;
        if (c < S) {
#pragma unroll
            for (int e = 0; e < 4; ++e) g4[i][e] = float(double(pr.y[0][i][e]) * (double(g4[i][e]) - shift)) * scale;
            *reinterpret_cast<af32x4*>(gr + c) = g4[i];
        }
    }
}

// floats of LDS: the larger of the two roles
template <int D>
constexpr int attn_bwd_lds_floats(int S) {
    const int query = 32 * (D + 4) + S * (D + 4) + S * (D + 8) + 32 * (S + 4) + 3 * 1024;
    const int key = 2 * S * (D + 8) + 32 * (D + 4) + 2 * S * 40 + 2048;
    return query > key ? query : key;
}

// DROP: the mask of the forward again, from the seed in the generator's state and the call number the forward wrote; nothing
// is drawn.  dP is masked in both roles after the same MFMA sequence (one multiply, the same bits), dV takes P under the mask.
template <int D, bool TAIL = false, bool DROP = false>
__global__ void __launch_bounds__(256) attn_bwd(std::conditional_t<DROP, AttnBwdDropArgs, AttnBwdArgs> a) {
    extern __shared__ __attribute__((aligned(16))) float lds[];
    const int S = a.S;                               // the sequence
    const int Sp = TAIL ? round32(S) : S;            // what the tiles, the shift slab and the hand-off counter cover
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, r = lane & 31, h = lane >> 5;
    // the query-role workgroups of the whole grid are dispatched before any key-role one (role in the slowest grid index): a
    // key-role workgroup that waits, waits for workgroups that are already running and wait for nothing
    const int role = int(blockIdx.z) >= a.batch ? 1 : 0;
    const int blk = blockIdx.x, head = blockIdx.y, b = int(blockIdx.z) - role * a.batch;
    const int j0 = blk * 32, nblk = Sp / 32;
    constexpr int kBlock = 32;
    const int brows = TAIL ? (S - j0 < kBlock ? S - j0 : kBlock) : kBlock;        // rows of this block that exist
    const int bh = b * a.heads + head;
    const float* pg = a.p + int64_t(bh) * S * S;
    double* shifts = a.shift + int64_t(bh) * Sp;
    int* flags = a.flags + 2 * bh;
    constexpr int NT = D / 32;
    constexpr int NB = 32 * (D / 4) / 256 > 0 ? 32 * (D / 4) / 256 : 1, NA = 128 * (D / 4) / 256;       // float4 per thread: 32 rows / all rows
    [[maybe_unused]] DropRows dr{};
    if constexpr (DROP) dr = DropRows{a.drop.state[0], a.drop.base[0], a.drop.threshold, a.drop.s, (int64_t(bh) * S + j0) * S, S};

    LG_ATL(0);
    if (role == 0) {
        // ---- query role: dQ of queries [j0, j0 + 32), and the shift of their rows for the key role ------------------
        constexpr int PG = D + 4, PVK = D + 4, PK = D + 8;
        const int PP = Sp + 4;
        float* Gs = lds;                 // dO rows of the block          32 x PG
        float* Vs = Gs + 32 * PG;        // V, K-contiguous B of dP       Sp x PVK
        float* Ks = Vs + Sp * PVK;       // K, N-contiguous B of dQ       Sp x PK
        float* Ss = Ks + Sp * PK;        // dP, then dS                   32 x PP
        float* Red = Ss + 32 * PP;
        {
            af32x4 rg[NB], rv[NA], rk[NA];
            load_rows<D, NB>(rg, a.g + int64_t(b) * a.sbg + int64_t(j0) * a.ldg + head * D, a.ldg, brows);
            load_rows<D, NA>(rv, a.v + int64_t(b) * a.sbv + head * D, a.ldv, S);
            load_rows<D, NA>(rk, a.k + int64_t(b) * a.sbk + head * D, a.ldk, S);
            if constexpr (!TAIL) {
                store_rows<D, NB>(rg, Gs, PG, 32);
                store_rows<D, NA>(rv, Vs, PVK, S);
                store_rows<D, NA>(rk, Ks, PK, S);
            } else {
                store_rows_padded<D, NB>(rg, Gs, PG, brows, 32);
                store_rows_padded<D, NA>(rv, Vs, PVK, S, Sp);
                store_rows_padded<D, NA>(rk, Ks, PK, S, Sp);
            }
        }
        ProbRows<1> probs;
        if constexpr (TAIL) load_probs_tail<1>(probs, pg + int64_t(j0) * S, S, brows);
        else                load_probs<1>(probs, pg + int64_t(j0) * S, S, 32);
        __syncthreads();
        LG_ATL(1);
        if (32 * wave < Sp) {
            af32x16 acc = zero16();
            wave_mma<true, true>(acc, Gs, PG, Vs + 32 * wave * PVK, PVK, D, r, h);
#pragma unroll
            for (int e = 0; e < 16; ++e) Ss[acc_row(e, h) * PP + 32 * wave + r] = acc[e];
        }
        __syncthreads();
        LG_ATL(2);
        // (TAIL: over the Sp columns of the tile - a key >= S has probability 0 and dP 0, so it adds nothing and its dS is 0)
        softmax_bwd_rows<TAIL, DROP>(Ss, PP, probs, Sp, a.scale, shifts + j0, brows, dr);
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");             // the shifts have left this CU
        __syncthreads();
        if (tid == 0) __hip_atomic_fetch_add(flags, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);      // 32 more rows are published
        LG_ATL(3);
        constexpr int KP = 4 / NT;
        const int n = wave % NT, kp = wave / NT;
        const int kspan = Sp / KP;
        af32x16 acc = zero16();
        wave_mma<true, false>(acc, Ss + kp * kspan, PP, Ks + kp * kspan * PK + 32 * n, PK, kspan, r, h);
        LG_ATL(4);
        if (kp > 0) {
#pragma unroll
            for (int e = 0; e < 16; ++e) Red[((kp - 1) * NT + n) * 1024 + e * 64 + lane] = acc[e];
        }
        __syncthreads();
        LG_ATL(5);
        if (kp == 0) {
            for (int q = 1; q < KP; ++q) {
#pragma unroll
                for (int e = 0; e < 16; ++e) acc[e] += Red[((q - 1) * NT + n) * 1024 + e * 64 + lane];
            }
            float* dst = a.dq + int64_t(b) * a.sbdq + int64_t(j0) * a.lddq + head * D + 32 * n + r;
#pragma unroll
            for (int e = 0; e < 16; ++e)
                if (!TAIL || acc_row(e, h) < brows) dst[int64_t(acc_row(e, h)) * a.lddq] = acc[e];
        }
        LG_ATL(6);
        return;
    }

    // ---- key role: dK and dV of keys [j0, j0 + 32) --------------------------------------------------------------
    // dS[:, block] = P[:, block] o (dP[:, block] - shift) * scale needs dP only for the block's own keys (32 MFMAs per wave, query
    // rows [32 w, 32 w + 32) each) - and the shift of EVERY row, a sum over the whole row of dP that the query-role workgroups of
    // this (batch, head) have formed: they publish it, a counter says how many of them have.  The values of dP agree bit for bit
    // between the roles (the same MFMA sequence over the same operands), so dS does too.
    constexpr int PG = D + 8;            // dO: K-contiguous A of dP (two-way conflicts there) and N-contiguous B of dV
    constexpr int PVK = D + 4, PQN = D + 8, PC = 40;
    float* Gs = lds;                     // dO, all queries               Sp x PG
    float* Qs = Gs + Sp * PG;            // Q, N-contiguous B of dK       Sp x PQN
    float* Vj = Qs + Sp * PQN;           // V rows of the block           32 x PVK
    float* Pc = Vj + 32 * PVK;           // P[:, block]                   Sp x PC
    float* Dc = Pc + Sp * PC;            // dS[:, block]                  Sp x PC
    float* Red = Dc + Sp * PC;
    {
        af32x4 rg[NA], rq[NA], rv[NB];
        load_rows<D, NA>(rg, a.g + int64_t(b) * a.sbg + head * D, a.ldg, S);
        load_rows<D, NA>(rq, a.q + int64_t(b) * a.sbq + head * D, a.ldq, S);
        load_rows<D, NB>(rv, a.v + int64_t(b) * a.sbv + int64_t(j0) * a.ldv + head * D, a.ldv, brows);
        if constexpr (!TAIL) {
            store_rows<D, NA>(rg, Gs, PG, S);
            store_rows<D, NA>(rq, Qs, PQN, S);
            store_rows<D, NB>(rv, Vj, PVK, 32);
        } else {
            store_rows_padded<D, NA>(rg, Gs, PG, S, Sp);
            store_rows_padded<D, NA>(rq, Qs, PQN, S, Sp);
            store_rows_padded<D, NB>(rv, Vj, PVK, brows, 32);
        }
    }
    const bool active = 32 * wave < Sp;
    // the probabilities that meet this wave's block of dP: element e of the accumulator is (row 32 w + acc_row(e, h), key j0 + r)
    float y[16];
    if (active) {
#pragma unroll
        for (int e = 0; e < 16; ++e) {
            if constexpr (TAIL) {
                // a (row, key) pair past the sequence has no probability: 0, so its dS and its share of dK / dV are 0
                const int row = 32 * wave + acc_row(e, h);
                const bool in = row < S && r < brows;
                const float t = pg[in ? int64_t(row) * S + j0 + r : 0];
                y[e] = in ? t : 0.f;
            } else {
                y[e] = pg[int64_t(32 * wave + acc_row(e, h)) * S + j0 + r];
            }
        }
    }
    __syncthreads();
    LG_ATL(1);
    af32x16 dp = zero16();
    if (active) wave_mma<true, true>(dp, Gs + 32 * wave * PG, PG, Vj, PVK, D, r, h);
    LG_ATL(2);
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
    LG_ATL(3);
    if (active) {
        double sh[16];
#pragma unroll
        for (int e = 0; e < 16; ++e) {
            sh[e] = __hip_atomic_load(shifts + 32 * wave + acc_row(e, h), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            if constexpr (TAIL) sh[e] = 32 * wave + acc_row(e, h) < S ? sh[e] : 0.0;        // no row, nothing published: not read as a number
        }
#pragma unroll
        for (int e = 0; e < 16; ++e) {
            const int row = 32 * wave + acc_row(e, h);
            if constexpr (DROP) {
                // element (row, j0 + r); a pair past the sequence has y = 0: 0 either way
                const uint32_t word = rng_word((int64_t(bh) * S + row) * S + j0 + r, dr.seed, dr.base);
                Dc[row * PC + r] = float(double(y[e]) * (double(rng_keep(dp[e], word, dr.threshold, dr.s)) - sh[e])) * a.scale;
                Pc[row * PC + r] = rng_keep(y[e], word, dr.threshold, dr.s);
            } else {
                Dc[row * PC + r] = float(double(y[e]) * (double(dp[e]) - sh[e])) * a.scale;
                Pc[row * PC + r] = y[e];
            }
        }
    }
    __syncthreads();
    // every wave has read its shifts: this workgroup is served; the last one of the (batch, head) pair clears the counters
    if (tid == 0) {
        const int served = __hip_atomic_fetch_add(flags + 1, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (served == nblk - 1) {
            __hip_atomic_store(flags, 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            __hip_atomic_store(flags + 1, 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
    }
    LG_ATL(4);
    // dV = P[:, block]^T @ dO and dK = dS[:, block]^T @ Q: 2 * NT output tiles of 32 x 32 over four waves
    constexpr int TILES = 2 * NT, KP = 4 / TILES > 0 ? 4 / TILES : 1;
    const int tile = wave % TILES, kp = wave / TILES;
    const bool is_dk = tile >= NT;
    const int n = tile % NT;
    const int kspan = Sp / KP;
    af32x16 acc = zero16();
    if (is_dk) wave_mma<false, false>(acc, Dc + kp * kspan * PC, PC, Qs + kp * kspan * PQN + 32 * n, PQN, kspan, r, h);
    else       wave_mma<false, false>(acc, Pc + kp * kspan * PC, PC, Gs + kp * kspan * PG + 32 * n, PG, kspan, r, h);
    LG_ATL(5);
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
        if (!TAIL || acc_row(e, h) < brows) dst[int64_t(acc_row(e, h)) * ldd] = acc[e];
    LG_ATL(6);
}

#ifdef LG_GEMM_TIMELINE
static unsigned long long* g_atl = nullptr;
static int g_atl_wgs = 0;
static unsigned long long* timeline_buffer(int wgs) {
    constexpr int kMax = 4096;
    if (!g_atl && hipMalloc(reinterpret_cast<void**>(&g_atl), size_t(kMax) * 16 * 8) != hipSuccess) return nullptr;
    if (wgs > kMax) return nullptr;
    (void)hipMemsetAsync(g_atl, 0, size_t(wgs) * 16 * 8, rt().stream);
    g_atl_wgs = wgs;
    return g_atl;
}
#endif

// ---- the launchers: LDS size, allow_lds, launch.  `a` is sliced to the struct the instantiation takes ---------------------------
template <int D, bool TAIL, bool DROP, bool CAUSAL = false>
static int launch_fwd_as(const AttnDropArgs& a, dim3 grid) {
    const size_t bytes = size_t(TAIL ? attn_fwd_tail_lds_floats<D>(a.S) : attn_fwd_lds_floats<D>(a.S)) * 4;
    int rc = allow_lds(&attn_fwd<D, TAIL, DROP, CAUSAL>, bytes);
    if (rc != LG_OK) return rc;
    hipLaunchKernelGGL((attn_fwd<D, TAIL, DROP, CAUSAL>), grid, dim3(256), bytes, rt().stream, a);
    return LG_OK;
}

template <int D, bool TAIL, bool DROP>
static int launch_bwd_as(const AttnBwdDropArgs& a, dim3 grid) {
    const size_t bytes = size_t(attn_bwd_lds_floats<D>(round32(a.S))) * 4;
    int rc = allow_lds(&attn_bwd<D, TAIL, DROP>, bytes);
    if (rc != LG_OK) return rc;
    hipLaunchKernelGGL((attn_bwd<D, TAIL, DROP>), grid, dim3(256), bytes, rt().stream, a);
    return LG_OK;
}

static int launch_fwd(const AttnDropArgs& a, dim3 grid, int64_t D, bool tail, bool drop) {
    static int (*const table[2][2][2])(const AttnDropArgs&, dim3) = {          // [D == 64][tail][drop]
        {{launch_fwd_as<32, false, false>, launch_fwd_as<32, false, true>}, {launch_fwd_as<32, true, false>, launch_fwd_as<32, true, true>}},
        {{launch_fwd_as<64, false, false>, launch_fwd_as<64, false, true>}, {launch_fwd_as<64, true, false>, launch_fwd_as<64, true, true>}}};
    return table[D == 64][tail][drop](a, grid);
}

// the causal family's short form: the TAIL kernels at every length 1 .. 128
static int launch_causal_fwd(const AttnDropArgs& a, dim3 grid, int64_t D, bool drop) {
    static int (*const table[2][2])(const AttnDropArgs&, dim3) = {             // [D == 64][drop]
        {launch_fwd_as<32, true, false, true>, launch_fwd_as<32, true, true, true>},
        {launch_fwd_as<64, true, false, true>, launch_fwd_as<64, true, true, true>}};
    return table[D == 64][drop](a, grid);
}

static int launch_bwd(const AttnBwdDropArgs& a, dim3 grid, int64_t D, bool tail, bool drop) {
    static int (*const table[2][2][2])(const AttnBwdDropArgs&, dim3) = {       // [D == 64][tail][drop]
        {{launch_bwd_as<32, false, false>, launch_bwd_as<32, false, true>}, {launch_bwd_as<32, true, false>, launch_bwd_as<32, true, true>}},
        {{launch_bwd_as<64, false, false>, launch_bwd_as<64, false, true>}, {launch_bwd_as<64, true, false>, launch_bwd_as<64, true, true>}}};
    return table[D == 64][tail][drop](a, grid);
}

// ---- the one host path ---------------------------------------------------------------------------------------------------------
static bool ok_operand(const void* p, int64_t ld, int64_t sb) { return p && aligned16(p) && ld % 4 == 0 && sb % 4 == 0; }

static int check_rows_write(const AttnOut& x, int64_t batch, int64_t S, int64_t width) {
    const int64_t shape[3] = {batch, S, width}, strides[3] = {x.sb, x.ld, 1};
    return adam_epilogue_check_strided(x.x, 4, 3, shape, strides);
}

static int check_launch(const char* name) {
    const hipError_t e = hipGetLastError();
    if (e == hipSuccess) return LG_OK;
    set_error("%s: kernel launch failed: %s", name, hipGetErrorString(e));
    return LG_EHIP;
}

// The selection rule.  A family with a form of its own runs that form for every call it accepts - the masked entries the TAIL
// kernels also at S % 32 == 0 and with mask == NULL.  The dropout family goes by length: the long kernels beyond 128, else
// the plain kernels where `plain_fits` (forward: no mask and S % 32 == 0; backward: S % 32 == 0 - which forward ran makes no
// difference to the backward's bits), else the TAIL ones.  The causal family goes by length too and has no plain form.
static AttnForm pick_form(const AttnFamily& f, int64_t S, bool plain_fits) {
    if (f.form != AttnForm::ByLength) return f.form;
    return S > 128 ? AttnForm::Long : plain_fits ? AttnForm::Plain : AttnForm::Tail;
}

int attn_forward(const AttnFamily& f, const AttnFwdCall& c) {
    const char* name = f.fwd;
    const bool drops = f.causal ? c.base != nullptr : f.dropout();       // the causal entry draws where it is given a base_out
    const int64_t batch = c.batch, heads = c.heads, S = c.S, D = c.D, w = heads * D;
    LG_ARG(f.supported(S, D), "%s: S = %lld (%s), D = %lld (32 or 64) unsupported", name, (long long)S, f.range, (long long)D);
    if (drops) {
        LG_ARG(c.prob >= 0.0 && c.prob < 1.0, "%s: p = %g outside [0, 1)", name, c.prob);
        LG_ARG(c.base != nullptr, "%s: base_out is NULL", name);
    } else if (f.causal) {
        LG_ARG(c.prob == 0.0, "%s: p = %g with a NULL base_out (dropout writes the call's number there)", name, c.prob);
    }
    LG_ARG(batch >= 0 && heads >= 1 && batch <= 65535 && heads <= 65535, "%s: bad batch / heads", name);
    if (drops) LG_ARG(batch > 0, "%s: an empty batch draws nothing (batch must be >= 1)", name);
    if (batch == 0) return LG_OK;
    LG_ARG(ok_operand(c.q.x, c.q.ld, c.q.sb) && ok_operand(c.k.x, c.k.ld, c.k.sb) && ok_operand(c.v.x, c.v.ld, c.v.sb) &&
               ok_operand(c.o.x, c.o.ld, c.o.sb) && c.p && aligned16(c.p),
           "%s: operands must be %s16-byte aligned with pitches that are multiples of 4", name, drops ? "non-NULL and " : "");
    LG_ARG(c.q.ld >= w && c.k.ld >= w && c.v.ld >= w && c.o.ld >= w, "%s: row pitch below heads * D", name);
    LG_ARG(!c.mask || c.sbm == 0 || c.sbm >= S, "%s: mask batch pitch %lld is neither 0 (one row for the batch) nor >= S", name, (long long)c.sbm);
    const int Sp = round32(int(S));                  // what the grid and the tiles cover; S itself where the plain form runs
    const int64_t wgs = int64_t(Sp / 32) * heads * batch;
    AttnDrop drop{};
    if (drops) {
        LG_ARG(wgs <= int64_t(kRngMaxGroup) * kRngMaxGroup, "%s: %lld workgroups, more than the stream's tickets count", name, (long long)wgs);
        { int rc = check_rows_write(c.o, batch, S, w); if (rc != LG_OK) return rc; }
        { int rc = adam_epilogue_check_write(c.p, batch * heads * S * S * 4); if (rc != LG_OK) return rc; }
        { int rc = adam_epilogue_check_write(c.base, 8); if (rc != LG_OK) return rc; }
        drop = AttnDrop{rt().rng_state, reinterpret_cast<unsigned long long*>(c.base), 0u, 0.f, rng_group(unsigned(wgs))};
        rng_threshold(c.prob, drop.threshold, drop.s);
    }
    const AttnForm form = pick_form(f, S, !f.causal && !c.mask && S % 32 == 0);
    AttnDropArgs a{{{
#ifdef LG_GEMM_TIMELINE
        form == AttnForm::Long ? nullptr : timeline_buffer(int(wgs)),        // the long kernels take no timestamps
#endif
        c.q.x, c.k.x, c.v.x, c.q.ld, c.q.sb, c.k.ld, c.k.sb, c.v.ld, c.v.sb, c.o.x, c.o.ld, c.o.sb, c.p, int(S), int(heads), c.scale},
        c.mask, c.sbm}, drop};
    const dim3 grid(unsigned(Sp / 32), unsigned(heads), unsigned(batch));
    const int rc = form == AttnForm::Long ? attn_long_launch_fwd(a, grid, D, drops, f.causal)
                   : f.causal             ? launch_causal_fwd(a, grid, D, drops)
                                          : launch_fwd(a, grid, D, form == AttnForm::Tail, drops);
    return rc != LG_OK ? rc : check_launch(name);
}

int attn_backward(const AttnFamily& f, const AttnBwdCall& c) {
    const char* name = f.bwd;
    const bool drops = f.dropout();
    const int64_t batch = c.batch, heads = c.heads, S = c.S, D = c.D, w = heads * D;
    LG_ARG(f.supported(S, D), "%s: S = %lld (%s), D = %lld (32 or 64) unsupported", name, (long long)S, f.range, (long long)D);
    if (drops) {
        LG_ARG(c.prob >= 0.0 && c.prob < 1.0, "%s: p = %g outside [0, 1)", name, c.prob);
        LG_ARG(c.base != nullptr, "%s: base is NULL", name);
    }
    LG_ARG(batch >= 0 && heads >= 1 && batch <= 65535 && heads <= 65535, "%s: bad batch / heads", name);
    if (batch == 0) return LG_OK;
    LG_ARG(ok_operand(c.q.x, c.q.ld, c.q.sb) && ok_operand(c.k.x, c.k.ld, c.k.sb) && ok_operand(c.v.x, c.v.ld, c.v.sb) &&
               ok_operand(c.g.x, c.g.ld, c.g.sb) && ok_operand(c.dq.x, c.dq.ld, c.dq.sb) && ok_operand(c.dk.x, c.dk.ld, c.dk.sb) &&
               ok_operand(c.dv.x, c.dv.ld, c.dv.sb) && c.p && aligned16(c.p),
           "%s: operands must be %s16-byte aligned with pitches that are multiples of 4", name, drops ? "non-NULL and " : "");
    LG_ARG(c.q.ld >= w && c.k.ld >= w && c.v.ld >= w && c.g.ld >= w && c.dq.ld >= w && c.dk.ld >= w && c.dv.ld >= w,
           "%s: row pitch below heads * D", name);
    LG_ARG(batch * heads <= rt().n_attn_pairs && 2 * batch <= 65535, "%s: more than %d (batch, head) pairs in one launch", name, rt().n_attn_pairs);
    AttnDrop drop{};
    if (drops) {
        { int rc = check_rows_write(c.dq, batch, S, w); if (rc != LG_OK) return rc; }
        { int rc = check_rows_write(c.dk, batch, S, w); if (rc != LG_OK) return rc; }
        { int rc = check_rows_write(c.dv, batch, S, w); if (rc != LG_OK) return rc; }
        drop = AttnDrop{rt().rng_state, const_cast<unsigned long long*>(reinterpret_cast<const unsigned long long*>(c.base)), 0u, 0.f, 0};
        rng_threshold(c.prob, drop.threshold, drop.s);
    }
    const int Sp = round32(int(S));                  // what the grid, the tiles and the shift slab cover; S itself where the plain form runs
    const AttnForm form = pick_form(f, S, S % 32 == 0);
    double* shift = nullptr;
    {
        const int mrc = lg_malloc(reinterpret_cast<void**>(&shift), size_t(batch * heads * Sp) * sizeof(double));
        if (mrc != LG_OK) return mrc;
    }
    AttnBwdDropArgs a{{
#ifdef LG_GEMM_TIMELINE
        form == AttnForm::Long ? nullptr : timeline_buffer(int(2 * (Sp / 32) * heads * batch)),
#endif
        c.q.x, c.k.x, c.v.x, c.g.x, c.q.ld, c.q.sb, c.k.ld, c.k.sb, c.v.ld, c.v.sb, c.g.ld, c.g.sb, c.p, c.dq.x, c.dk.x, c.dv.x,
        c.dq.ld, c.dq.sb, c.dk.ld, c.dk.sb, c.dv.ld, c.dv.sb, int(S), int(heads), int(batch), c.scale, shift, rt().attn_flags, rt().status_dev},
        drop};
    const dim3 grid(unsigned(Sp / 32), unsigned(heads), unsigned(2 * batch));
    int rc = form == AttnForm::Long ? attn_long_launch_bwd(a, grid, D, drops) : launch_bwd(a, grid, D, form == AttnForm::Tail, drops);
    if (rc == LG_OK) rc = check_launch(name);
    const int frc = lg_free(shift);                  // on every path out; stream-ordered: the block is only reused by later launches
    return rc != LG_OK ? rc : frc;
}

}  // namespace lg

using namespace lg;

// ---- the entries: each fills the call, names its family and takes the path above ---------------------------------------------
extern "C" int lg_attention_supported(int64_t S, int64_t D) {
    return (D == 64 || D == 32) && S >= 32 && S <= 128 && S % 32 == 0;
}
extern "C" int lg_attention_masked_supported(int64_t S, int64_t D) {
    return (D == 64 || D == 32) && S >= 1 && S <= 128;
}
extern "C" int lg_attention_dropout_supported(int64_t S, int64_t D) {
    return (D == 64 || D == 32) && S >= 1 && S <= 512;
}
extern "C" int lg_attention_causal_supported(int64_t S, int64_t D) {
    return (D == 64 || D == 32) && S >= 1 && S <= 512;
}

static const AttnFamily kPlain{"lg_attention_fwd_f32", "lg_attention_bwd_f32", lg_attention_supported, "32..128, multiple of 32", AttnForm::Plain};
static const AttnFamily kMasked{"lg_attention_masked_fwd_f32", "lg_attention_masked_bwd_f32", lg_attention_masked_supported, "1..128", AttnForm::Tail};
// one pair for every length, with dropout of the probabilities inside the launches
static const AttnFamily kDropout{"lg_attention_dropout_fwd_f32", "lg_attention_dropout_bwd_f32", lg_attention_dropout_supported, "1..512",
                                 AttnForm::ByLength};
// the forward with a causal mask at every length; dropout where the call brings a base_out.  No backward of its own: P is zero
// above the diagonal, and the backward entry of the form reads P.
static const AttnFamily kCausal{"lg_attention_causal_fwd_f32", nullptr, lg_attention_causal_supported, "1..512", AttnForm::ByLength, true};

extern "C" int lg_attention_fwd_f32(const float* q, int64_t ldq, int64_t sbq, const float* k, int64_t ldk, int64_t sbk,
                                    const float* v, int64_t ldv, int64_t sbv, float* o, int64_t ldo, int64_t sbo, float* p,
                                    int64_t batch, int64_t heads, int64_t S, int64_t D, float scale) {
    LG_REQUIRE_INIT();
    return attn_forward(kPlain, {{q, ldq, sbq}, {k, ldk, sbk}, {v, ldv, sbv}, {o, ldo, sbo}, p, batch, heads, S, D, scale, nullptr, 0, 0.0, nullptr});
}

extern "C" int lg_attention_bwd_f32(const float* q, int64_t ldq, int64_t sbq, const float* k, int64_t ldk, int64_t sbk,
                                    const float* v, int64_t ldv, int64_t sbv, const float* g, int64_t ldg, int64_t sbg,
                                    const float* p, float* dq, int64_t lddq, int64_t sbdq, float* dk, int64_t lddk, int64_t sbdk,
                                    float* dv, int64_t lddv, int64_t sbdv, int64_t batch, int64_t heads, int64_t S, int64_t D,
                                    float scale) {
    LG_REQUIRE_INIT();
    return attn_backward(kPlain, {{q, ldq, sbq}, {k, ldk, sbk}, {v, ldv, sbv}, {g, ldg, sbg}, p, {dq, lddq, sbdq}, {dk, lddk, sbdk},
                                  {dv, lddv, sbdv}, batch, heads, S, D, scale, 0.0, nullptr});
}

extern "C" int lg_attention_masked_fwd_f32(const float* q, int64_t ldq, int64_t sbq, const float* k, int64_t ldk, int64_t sbk,
                                           const float* v, int64_t ldv, int64_t sbv, float* o, int64_t ldo, int64_t sbo, float* p,
                                           int64_t batch, int64_t heads, int64_t S, int64_t D, float scale,
                                           const float* mask, int64_t sbm) {
    LG_REQUIRE_INIT();
    return attn_forward(kMasked, {{q, ldq, sbq}, {k, ldk, sbk}, {v, ldv, sbv}, {o, ldo, sbo}, p, batch, heads, S, D, scale, mask, sbm, 0.0, nullptr});
}

extern "C" int lg_attention_masked_bwd_f32(const float* q, int64_t ldq, int64_t sbq, const float* k, int64_t ldk, int64_t sbk,
                                           const float* v, int64_t ldv, int64_t sbv, const float* g, int64_t ldg, int64_t sbg,
                                           const float* p, float* dq, int64_t lddq, int64_t sbdq, float* dk, int64_t lddk, int64_t sbdk,
                                           float* dv, int64_t lddv, int64_t sbdv, int64_t batch, int64_t heads, int64_t S, int64_t D,
                                           float scale) {
    LG_REQUIRE_INIT();
    return attn_backward(kMasked, {{q, ldq, sbq}, {k, ldk, sbk}, {v, ldv, sbv}, {g, ldg, sbg}, p, {dq, lddq, sbdq}, {dk, lddk, sbdk},
                                   {dv, lddv, sbdv}, batch, heads, S, D, scale, 0.0, nullptr});
}

extern "C" int lg_attention_dropout_fwd_f32(const float* q, int64_t ldq, int64_t sbq, const float* k, int64_t ldk, int64_t sbk,
                                            const float* v, int64_t ldv, int64_t sbv, float* o, int64_t ldo, int64_t sbo, float* p,
                                            int64_t batch, int64_t heads, int64_t S, int64_t D, float scale,
                                            const float* mask, int64_t sbm, double prob, uint64_t* base_out) {
    LG_REQUIRE_INIT();
    return attn_forward(kDropout, {{q, ldq, sbq}, {k, ldk, sbk}, {v, ldv, sbv}, {o, ldo, sbo}, p, batch, heads, S, D, scale, mask, sbm, prob, base_out});
}

extern "C" int lg_attention_dropout_bwd_f32(const float* q, int64_t ldq, int64_t sbq, const float* k, int64_t ldk, int64_t sbk,
                                            const float* v, int64_t ldv, int64_t sbv, const float* g, int64_t ldg, int64_t sbg,
                                            const float* p, float* dq, int64_t lddq, int64_t sbdq, float* dk, int64_t lddk, int64_t sbdk,
                                            float* dv, int64_t lddv, int64_t sbdv, int64_t batch, int64_t heads, int64_t S, int64_t D,
                                            float scale, double prob, const uint64_t* base) {
    LG_REQUIRE_INIT();
    return attn_backward(kDropout, {{q, ldq, sbq}, {k, ldk, sbk}, {v, ldv, sbv}, {g, ldg, sbg}, p, {dq, lddq, sbdq}, {dk, lddk, sbdk},
                                    {dv, lddv, sbdv}, batch, heads, S, D, scale, prob, base});
}

extern "C" int lg_attention_causal_fwd_f32(const float* q, int64_t ldq, int64_t sbq, const float* k, int64_t ldk, int64_t sbk,
                                           const float* v, int64_t ldv, int64_t sbv, float* o, int64_t ldo, int64_t sbo, float* p,
                                           int64_t batch, int64_t heads, int64_t S, int64_t D, float scale,
                                           const float* mask, int64_t sbm, double prob, uint64_t* base_out) {
    LG_REQUIRE_INIT();
    return attn_forward(kCausal, {{q, ldq, sbq}, {k, ldk, sbk}, {v, ldv, sbv}, {o, ldo, sbo}, p, batch, heads, S, D, scale, mask, sbm, prob, base_out});
}

#ifdef LG_GEMM_TIMELINE
// experiments build only: the 16 timestamps per workgroup of the LAST attention launch; returns the workgroup count
extern "C" int lg_debug_attn_timeline(unsigned long long* host_out, int max_wgs) {
    if (!g_atl || g_atl_wgs > max_wgs) return -1;
    if (hipStreamSynchronize(rt().stream) != hipSuccess) return -1;
    if (hipMemcpy(host_out, g_atl, size_t(g_atl_wgs) * 16 * 8, hipMemcpyDeviceToHost) != hipSuccess) return -1;
    return g_atl_wgs;
}
#endif
