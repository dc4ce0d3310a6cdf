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
#include "common.h"
#include "mfma_lds.h"
#include "rng_common.h"
#include <cmath>
#include <type_traits>

namespace lg {

#ifdef LG_GEMM_TIMELINE
// experiments build only (make timeline; tools/attn_timeline.py): 16 timestamps of the 100 MHz wall clock per workgroup
#define LG_ATL(slot) do { if (a.tl && threadIdx.x == 0) a.tl[size_t((blockIdx.z * gridDim.y + blockIdx.y) * gridDim.x + blockIdx.x) * 16 + (slot)] = wall_clock64(); } while (0)
#define LG_ATL_FIELD unsigned long long* tl;
#else
#define LG_ATL(slot) do { } while (0)
#define LG_ATL_FIELD
#endif

struct AttnArgs {
    LG_ATL_FIELD
    const float *q, *k, *v;          // element (b, s, head, d) of X at X + b * sbX + s * ldX + head * D + d
    int64_t ldq, sbq, ldk, sbk, ldv, sbv;
    float* o;                        // context, same addressing
    int64_t ldo, sbo;
    float* p;                        // probabilities (batch, heads, S, S), dense
    int S, heads;
    float scale;
};

struct AttnTailArgs : AttnArgs {
    const float* mask;               // key-padding mask, element (b, j) at mask + b * sbm + j (sbm = 0: one row for the batch); NULL = none
    int64_t sbm;
};

// DROP instantiations: the tail arguments (mask NULL for none) and the call of the random stream
struct AttnDropArgs : AttnTailArgs {
    AttnDrop drop;
};

// the two 64-bit words of a call in LDS (DROP instantiations only: 16 bytes of static LDS next to the dynamic tiles)
template <bool DROP>
__device__ __forceinline__ unsigned long long* rng_call_slot() {
    if constexpr (DROP) {
        __shared__ unsigned long long call[2];
        return call;
    } else {
        return nullptr;
    }
}

// linear index of this workgroup over the 3-D grid / workgroups of the launch: what the tickets of the random stream count
__device__ __forceinline__ int grid_linear_block() { return int((blockIdx.z * gridDim.y + blockIdx.y) * gridDim.x + blockIdx.x); }
__device__ __forceinline__ int grid_blocks() { return int(gridDim.x * gridDim.y * gridDim.z); }

// the float4 of probabilities at flat element index i of the dense (batch, heads, S, S) tensor as the context's MFMA operand:
// P * s where the stream keeps the element, +0.0 where it drops it
template <bool ALIGNED>
__device__ __forceinline__ af32x4 drop4(af32x4 t, int64_t i, unsigned long long seed, unsigned long long base, uint32_t threshold, float s) {
    uint32_t w[4];
    rng_words4<ALIGNED>(i, seed, base, w);
    return af32x4{rng_keep(t[0], w[0], threshold, s), rng_keep(t[1], w[1], threshold, s), rng_keep(t[2], w[2], threshold, s),
                  rng_keep(t[3], w[3], threshold, s)};
}

__host__ __device__ constexpr int round32(int S) { return (S + 31) & ~31; }

template <int D>
constexpr int attn_fwd_lds_floats(int S) { return 32 * (D + 4) + S * (D + 4) + S * (D + 8) + 32 * (S + 4) + 3 * 1024; }
// TAIL: the same layout over Sp rows and the per-key bias behind it
template <int D>
constexpr int attn_fwd_tail_lds_floats(int S) { return attn_fwd_lds_floats<D>(round32(S)) + 128; }

// store_rows that also clears rows [rows, padded): an MFMA operand row past the sequence must be zero, not stale LDS
template <int D, int N>
__device__ __forceinline__ void store_rows_padded(const af32x4 (&v)[N], float* dst, int pitch, int rows, int padded) {
    constexpr int Q = D / 4;
#pragma unroll
    for (int i = 0; i < N; ++i) {
        const int f = threadIdx.x + i * 256;
        if (f < padded * Q) {
            af32x4 t = v[i];
            if (f >= rows * Q) t = af32x4{0.f, 0.f, 0.f, 0.f};
            *reinterpret_cast<af32x4*>(dst + (f / Q) * pitch + (f % Q) * 4) = t;
        }
    }
}

// DROP: dropout of the probabilities between the softmax and the context, from the stream of dropout.hip (one call per launch:
// read `draws`, take a ticket, the last arriver advances).  P goes to HBM undropped; what feeds the context MFMAs is Pd.
template <int D, bool TAIL = false, bool DROP = false>
__global__ void __launch_bounds__(256) attn_fwd(std::conditional_t<DROP, AttnDropArgs, std::conditional_t<TAIL, AttnTailArgs, AttnArgs>> a) {
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
    if (32 * wave < Sp) {
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
                    if (c + e < S) m = (t[i][e] > m || t[i][e] != t[i][e]) ? t[i][e] : m;
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
                    if (c + e < S) { t[i][e] = expf(t[i][e] + (-m)); s += t[i][e]; }
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

struct AttnBwdArgs {
    LG_ATL_FIELD
    const float *q, *k, *v, *g;      // g = gradient of the context; addressing as in AttnArgs
    int64_t ldq, sbq, ldk, sbk, ldv, sbv, ldg, sbg;
    const float* p;                  // probabilities saved by the forward
    float *dq, *dk, *dv;
    int64_t lddq, sbdq, lddk, sbdk, lddv, sbdv;
    int S, heads, batch;
    float scale;
    double* shift;                   // [batch, heads, S]: the softmax shift of every query row, query role -> key role
    int*    flags;                   // [batch * heads][2]: rows published / key-role workgroups served; zero between launches
    int*    status;                  // device status flag (a wait that gives up raises it)
};

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

struct AttnBwdDropArgs : AttnBwdArgs {
    AttnDrop drop;
};

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

template <class K>
static int allow_lds(K kernel, size_t bytes) {
    hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize, int(bytes));
    if (e != hipSuccess) { set_error("attention: %zu bytes of LDS refused: %s", bytes, hipGetErrorString(e)); return LG_EHIP; }
    return LG_OK;
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

static bool ok_operand(const void* p, int64_t ld, int64_t sb) { return p && aligned16(p) && ld % 4 == 0 && sb % 4 == 0; }

}  // namespace lg

using namespace lg;

extern "C" int lg_attention_supported(int64_t S, int64_t D) {
    return (D == 64 || D == 32) && S >= 32 && S <= 128 && S % 32 == 0;
}

extern "C" int lg_attention_fwd_f32(const float* q, int64_t ldq, int64_t sbq, const float* k, int64_t ldk, int64_t sbk,
                                    const float* v, int64_t ldv, int64_t sbv, float* o, int64_t ldo, int64_t sbo, float* p,
                                    int64_t batch, int64_t heads, int64_t S, int64_t D, float scale) {
    LG_REQUIRE_INIT();
    LG_ARG(lg_attention_supported(S, D), "lg_attention_fwd_f32: S = %lld (32..128, multiple of 32), D = %lld (32 or 64) unsupported",
           (long long)S, (long long)D);
    LG_ARG(batch >= 0 && heads >= 1 && batch <= 65535 && heads <= 65535, "lg_attention_fwd_f32: bad batch / heads");
    if (batch == 0) return LG_OK;
    LG_ARG(ok_operand(q, ldq, sbq) && ok_operand(k, ldk, sbk) && ok_operand(v, ldv, sbv) && ok_operand(o, ldo, sbo) && p && aligned16(p),
           "lg_attention_fwd_f32: operands must be 16-byte aligned with pitches that are multiples of 4");
    LG_ARG(ldq >= heads * D && ldk >= heads * D && ldv >= heads * D && ldo >= heads * D, "lg_attention_fwd_f32: row pitch below heads * D");
    AttnArgs a{
#ifdef LG_GEMM_TIMELINE
        timeline_buffer(int(S / 32 * heads * batch)),
#endif
        q, k, v, ldq, sbq, ldk, sbk, ldv, sbv, o, ldo, sbo, p, int(S), int(heads), scale};
    const dim3 grid(unsigned(S / 32), unsigned(heads), unsigned(batch));
    if (D == 64) {
        const size_t bytes = size_t(attn_fwd_lds_floats<64>(int(S))) * 4;
        int rc = allow_lds(&attn_fwd<64>, bytes);
        if (rc != LG_OK) return rc;
        hipLaunchKernelGGL(attn_fwd<64>, grid, dim3(256), bytes, rt().stream, a);
    } else {
        const size_t bytes = size_t(attn_fwd_lds_floats<32>(int(S))) * 4;
        int rc = allow_lds(&attn_fwd<32>, bytes);
        if (rc != LG_OK) return rc;
        hipLaunchKernelGGL(attn_fwd<32>, grid, dim3(256), bytes, rt().stream, a);
    }
    LG_CHECK_LAUNCH();
    return LG_OK;
}

extern "C" int lg_attention_bwd_f32(const float* q, int64_t ldq, int64_t sbq, const float* k, int64_t ldk, int64_t sbk,
                                    const float* v, int64_t ldv, int64_t sbv, const float* g, int64_t ldg, int64_t sbg,
                                    const float* p, float* dq, int64_t lddq, int64_t sbdq, float* dk, int64_t lddk, int64_t sbdk,
                                    float* dv, int64_t lddv, int64_t sbdv, int64_t batch, int64_t heads, int64_t S, int64_t D,
                                    float scale) {
    LG_REQUIRE_INIT();
    LG_ARG(lg_attention_supported(S, D), "lg_attention_bwd_f32: S = %lld (32..128, multiple of 32), D = %lld (32 or 64) unsupported",
           (long long)S, (long long)D);
    LG_ARG(batch >= 0 && heads >= 1 && batch <= 65535 && heads <= 65535, "lg_attention_bwd_f32: bad batch / heads");
    if (batch == 0) return LG_OK;
    LG_ARG(ok_operand(q, ldq, sbq) && ok_operand(k, ldk, sbk) && ok_operand(v, ldv, sbv) && ok_operand(g, ldg, sbg) &&
               ok_operand(dq, lddq, sbdq) && ok_operand(dk, lddk, sbdk) && ok_operand(dv, lddv, sbdv) && p && aligned16(p),
           "lg_attention_bwd_f32: operands must be 16-byte aligned with pitches that are multiples of 4");
    const int64_t w = heads * D;
    LG_ARG(ldq >= w && ldk >= w && ldv >= w && ldg >= w && lddq >= w && lddk >= w && lddv >= w, "lg_attention_bwd_f32: row pitch below heads * D");
    LG_ARG(batch * heads <= rt().n_attn_pairs && 2 * batch <= 65535, "lg_attention_bwd_f32: more than %d (batch, head) pairs in one launch",
           rt().n_attn_pairs);
    int* flags = rt().attn_flags;
    double* shift = nullptr;
    {
        const int mrc = lg_malloc(reinterpret_cast<void**>(&shift), size_t(batch * heads * S) * sizeof(double));
        if (mrc != LG_OK) return mrc;
    }
    AttnBwdArgs a{
#ifdef LG_GEMM_TIMELINE
        timeline_buffer(int(2 * (S / 32) * heads * batch)),
#endif
        q, k, v, g, ldq, sbq, ldk, sbk, ldv, sbv, ldg, sbg, p, dq, dk, dv, lddq, sbdq, lddk, sbdk, lddv, sbdv, int(S), int(heads), int(batch), scale,
        shift, flags, rt().status_dev};
    const dim3 grid(unsigned(S / 32), unsigned(heads), unsigned(2 * batch));
    if (D == 64) {
        const size_t bytes = size_t(attn_bwd_lds_floats<64>(int(S))) * 4;
        int rc = allow_lds(&attn_bwd<64>, bytes);
        if (rc != LG_OK) return rc;
        hipLaunchKernelGGL(attn_bwd<64>, grid, dim3(256), bytes, rt().stream, a);
    } else {
        const size_t bytes = size_t(attn_bwd_lds_floats<32>(int(S))) * 4;
        int rc = allow_lds(&attn_bwd<32>, bytes);
        if (rc != LG_OK) return rc;
        hipLaunchKernelGGL(attn_bwd<32>, grid, dim3(256), bytes, rt().stream, a);
    }
    LG_CHECK_LAUNCH();
    return lg_free(shift);          // stream-ordered: the block is only reused by later launches
}

extern "C" int lg_attention_masked_supported(int64_t S, int64_t D) {
    return (D == 64 || D == 32) && S >= 1 && S <= 128;
}

extern "C" int lg_attention_masked_fwd_f32(const float* q, int64_t ldq, int64_t sbq, const float* k, int64_t ldk, int64_t sbk,
                                           const float* v, int64_t ldv, int64_t sbv, float* o, int64_t ldo, int64_t sbo, float* p,
                                           int64_t batch, int64_t heads, int64_t S, int64_t D, float scale,
                                           const float* mask, int64_t sbm) {
    LG_REQUIRE_INIT();
    LG_ARG(lg_attention_masked_supported(S, D), "lg_attention_masked_fwd_f32: S = %lld (1..128), D = %lld (32 or 64) unsupported",
           (long long)S, (long long)D);
    LG_ARG(batch >= 0 && heads >= 1 && batch <= 65535 && heads <= 65535, "lg_attention_masked_fwd_f32: bad batch / heads");
    if (batch == 0) return LG_OK;
    LG_ARG(ok_operand(q, ldq, sbq) && ok_operand(k, ldk, sbk) && ok_operand(v, ldv, sbv) && ok_operand(o, ldo, sbo) && p && aligned16(p),
           "lg_attention_masked_fwd_f32: operands must be 16-byte aligned with pitches that are multiples of 4");
    LG_ARG(ldq >= heads * D && ldk >= heads * D && ldv >= heads * D && ldo >= heads * D, "lg_attention_masked_fwd_f32: row pitch below heads * D");
    LG_ARG(!mask || sbm == 0 || sbm >= S, "lg_attention_masked_fwd_f32: mask batch pitch %lld is neither 0 (one row for the batch) nor >= S",
           (long long)sbm);
    const int Sp = round32(int(S));
    AttnTailArgs a{{
#ifdef LG_GEMM_TIMELINE
        timeline_buffer(int(Sp / 32 * heads * batch)),
#endif
        q, k, v, ldq, sbq, ldk, sbk, ldv, sbv, o, ldo, sbo, p, int(S), int(heads), scale}, mask, sbm};
    const dim3 grid(unsigned(Sp / 32), unsigned(heads), unsigned(batch));
    if (D == 64) {
        const size_t bytes = size_t(attn_fwd_tail_lds_floats<64>(int(S))) * 4;
        int rc = allow_lds(&attn_fwd<64, true>, bytes);
        if (rc != LG_OK) return rc;
        hipLaunchKernelGGL((attn_fwd<64, true>), grid, dim3(256), bytes, rt().stream, a);
    } else {
        const size_t bytes = size_t(attn_fwd_tail_lds_floats<32>(int(S))) * 4;
        int rc = allow_lds(&attn_fwd<32, true>, bytes);
        if (rc != LG_OK) return rc;
        hipLaunchKernelGGL((attn_fwd<32, true>), grid, dim3(256), bytes, rt().stream, a);
    }
    LG_CHECK_LAUNCH();
    return LG_OK;
}

extern "C" int lg_attention_masked_bwd_f32(const float* q, int64_t ldq, int64_t sbq, const float* k, int64_t ldk, int64_t sbk,
                                           const float* v, int64_t ldv, int64_t sbv, const float* g, int64_t ldg, int64_t sbg,
                                           const float* p, float* dq, int64_t lddq, int64_t sbdq, float* dk, int64_t lddk, int64_t sbdk,
                                           float* dv, int64_t lddv, int64_t sbdv, int64_t batch, int64_t heads, int64_t S, int64_t D,
                                           float scale) {
    LG_REQUIRE_INIT();
    LG_ARG(lg_attention_masked_supported(S, D), "lg_attention_masked_bwd_f32: S = %lld (1..128), D = %lld (32 or 64) unsupported",
           (long long)S, (long long)D);
    LG_ARG(batch >= 0 && heads >= 1 && batch <= 65535 && heads <= 65535, "lg_attention_masked_bwd_f32: bad batch / heads");
    if (batch == 0) return LG_OK;
    LG_ARG(ok_operand(q, ldq, sbq) && ok_operand(k, ldk, sbk) && ok_operand(v, ldv, sbv) && ok_operand(g, ldg, sbg) &&
               ok_operand(dq, lddq, sbdq) && ok_operand(dk, lddk, sbdk) && ok_operand(dv, lddv, sbdv) && p && aligned16(p),
           "lg_attention_masked_bwd_f32: operands must be 16-byte aligned with pitches that are multiples of 4");
    const int64_t w = heads * D;
    LG_ARG(ldq >= w && ldk >= w && ldv >= w && ldg >= w && lddq >= w && lddk >= w && lddv >= w, "lg_attention_masked_bwd_f32: row pitch below heads * D");
    LG_ARG(batch * heads <= rt().n_attn_pairs && 2 * batch <= 65535, "lg_attention_masked_bwd_f32: more than %d (batch, head) pairs in one launch",
           rt().n_attn_pairs);
    const int Sp = round32(int(S));
    int* flags = rt().attn_flags;
    double* shift = nullptr;
    {
        const int mrc = lg_malloc(reinterpret_cast<void**>(&shift), size_t(batch * heads * Sp) * sizeof(double));
        if (mrc != LG_OK) return mrc;
    }
    AttnBwdArgs a{
#ifdef LG_GEMM_TIMELINE
        timeline_buffer(int(2 * (Sp / 32) * heads * batch)),
#endif
        q, k, v, g, ldq, sbq, ldk, sbk, ldv, sbv, ldg, sbg, p, dq, dk, dv, lddq, sbdq, lddk, sbdk, lddv, sbdv, int(S), int(heads), int(batch), scale,
        shift, flags, rt().status_dev};
    const dim3 grid(unsigned(Sp / 32), unsigned(heads), unsigned(2 * batch));
    if (D == 64) {
        const size_t bytes = size_t(attn_bwd_lds_floats<64>(Sp)) * 4;
        int rc = allow_lds(&attn_bwd<64, true>, bytes);
        if (rc != LG_OK) return rc;
        hipLaunchKernelGGL((attn_bwd<64, true>), grid, dim3(256), bytes, rt().stream, a);
    } else {
        const size_t bytes = size_t(attn_bwd_lds_floats<32>(Sp)) * 4;
        int rc = allow_lds(&attn_bwd<32, true>, bytes);
        if (rc != LG_OK) return rc;
        hipLaunchKernelGGL((attn_bwd<32, true>), grid, dim3(256), bytes, rt().stream, a);
    }
    LG_CHECK_LAUNCH();
    return lg_free(shift);          // stream-ordered: the block is only reused by later launches
}

// ---- attention with dropout of the probabilities: one pair for every length ------------------------------------------------
namespace lg {
// attention_long.hip: the launches of its DROP instantiations (129 <= S <= 512; arguments already checked)
int attn_long_drop_fwd(const float* q, int64_t ldq, int64_t sbq, const float* k, int64_t ldk, int64_t sbk, const float* v, int64_t ldv,
                       int64_t sbv, float* o, int64_t ldo, int64_t sbo, float* p, int64_t batch, int64_t heads, int64_t S, int64_t D,
                       float scale, const float* mask, int64_t sbm, const AttnDrop& drop);
int attn_long_drop_bwd(const float* q, int64_t ldq, int64_t sbq, const float* k, int64_t ldk, int64_t sbk, const float* v, int64_t ldv,
                       int64_t sbv, const float* g, int64_t ldg, int64_t sbg, const float* p, float* dq, int64_t lddq, int64_t sbdq,
                       float* dk, int64_t lddk, int64_t sbdk, float* dv, int64_t lddv, int64_t sbdv, int64_t batch, int64_t heads,
                       int64_t S, int64_t D, float scale, const AttnDrop& drop);

static int check_rows_write(const float* x, int64_t ld, int64_t sb, int64_t batch, int64_t S, int64_t width) {
    const int64_t shape[3] = {batch, S, width}, strides[3] = {sb, ld, 1};
    return adam_epilogue_check_strided(x, 4, 3, shape, strides);
}

template <int D, bool TAIL>
static int launch_drop_fwd(const AttnDropArgs& a, dim3 grid, int Sp) {
    const size_t bytes = size_t(TAIL ? attn_fwd_tail_lds_floats<D>(a.S) : attn_fwd_lds_floats<D>(a.S)) * 4;
    (void)Sp;
    int rc = allow_lds(&attn_fwd<D, TAIL, true>, bytes);
    if (rc != LG_OK) return rc;
    hipLaunchKernelGGL((attn_fwd<D, TAIL, true>), grid, dim3(256), bytes, rt().stream, a);
    return LG_OK;
}

template <int D, bool TAIL>
static int launch_drop_bwd(const AttnBwdDropArgs& a, dim3 grid, int Sp) {
    const size_t bytes = size_t(attn_bwd_lds_floats<D>(Sp)) * 4;
    int rc = allow_lds(&attn_bwd<D, TAIL, true>, bytes);
    if (rc != LG_OK) return rc;
    hipLaunchKernelGGL((attn_bwd<D, TAIL, true>), grid, dim3(256), bytes, rt().stream, a);
    return LG_OK;
}
}  // namespace lg

extern "C" int lg_attention_dropout_supported(int64_t S, int64_t D) {
    return (D == 64 || D == 32) && S >= 1 && S <= 512;
}

extern "C" int lg_attention_dropout_fwd_f32(const float* q, int64_t ldq, int64_t sbq, const float* k, int64_t ldk, int64_t sbk,
                                            const float* v, int64_t ldv, int64_t sbv, float* o, int64_t ldo, int64_t sbo, float* p,
                                            int64_t batch, int64_t heads, int64_t S, int64_t D, float scale,
                                            const float* mask, int64_t sbm, double prob, uint64_t* base_out) {
    LG_REQUIRE_INIT();
    LG_ARG(lg_attention_dropout_supported(S, D), "lg_attention_dropout_fwd_f32: S = %lld (1..512), D = %lld (32 or 64) unsupported",
           (long long)S, (long long)D);
    LG_ARG(prob >= 0.0 && prob < 1.0, "lg_attention_dropout_fwd_f32: p = %g outside [0, 1)", prob);
    LG_ARG(base_out != nullptr, "lg_attention_dropout_fwd_f32: base_out is NULL");
    LG_ARG(batch >= 0 && heads >= 1 && batch <= 65535 && heads <= 65535, "lg_attention_dropout_fwd_f32: bad batch / heads");
    LG_ARG(batch > 0, "lg_attention_dropout_fwd_f32: an empty batch draws nothing (batch must be >= 1)");
    LG_ARG(ok_operand(q, ldq, sbq) && ok_operand(k, ldk, sbk) && ok_operand(v, ldv, sbv) && ok_operand(o, ldo, sbo) && p && aligned16(p),
           "lg_attention_dropout_fwd_f32: operands must be non-NULL and 16-byte aligned with pitches that are multiples of 4");
    LG_ARG(ldq >= heads * D && ldk >= heads * D && ldv >= heads * D && ldo >= heads * D, "lg_attention_dropout_fwd_f32: row pitch below heads * D");
    LG_ARG(!mask || sbm == 0 || sbm >= S, "lg_attention_dropout_fwd_f32: mask batch pitch %lld is neither 0 (one row for the batch) nor >= S",
           (long long)sbm);
    const int Sp = round32(int(S));
    const int64_t wgs = int64_t(Sp / 32) * heads * batch;
    LG_ARG(wgs <= int64_t(kRngMaxGroup) * kRngMaxGroup, "lg_attention_dropout_fwd_f32: %lld workgroups, more than the stream's tickets count", (long long)wgs);
    { int rc = check_rows_write(o, ldo, sbo, batch, S, heads * D); if (rc != LG_OK) return rc; }
    { int rc = adam_epilogue_check_write(p, batch * heads * S * S * 4); if (rc != LG_OK) return rc; }
    { int rc = adam_epilogue_check_write(base_out, 8); if (rc != LG_OK) return rc; }
    AttnDrop drop{rt().rng_state, reinterpret_cast<unsigned long long*>(base_out), 0u, 0.f, rng_group(unsigned(wgs))};
    rng_threshold(prob, drop.threshold, drop.s);
    if (S > 128) {
        const int rc = attn_long_drop_fwd(q, ldq, sbq, k, ldk, sbk, v, ldv, sbv, o, ldo, sbo, p, batch, heads, S, D, scale, mask, sbm, drop);
        if (rc != LG_OK) return rc;
        LG_CHECK_LAUNCH();
        return LG_OK;
    }
    AttnDropArgs a{{{
#ifdef LG_GEMM_TIMELINE
        timeline_buffer(int(wgs)),
#endif
        q, k, v, ldq, sbq, ldk, sbk, ldv, sbv, o, ldo, sbo, p, int(S), int(heads), scale}, mask, sbm}, drop};
    const dim3 grid(unsigned(Sp / 32), unsigned(heads), unsigned(batch));
    const bool plain = !mask && S % 32 == 0;
    const int rc = D == 64 ? (plain ? launch_drop_fwd<64, false>(a, grid, Sp) : launch_drop_fwd<64, true>(a, grid, Sp))
                           : (plain ? launch_drop_fwd<32, false>(a, grid, Sp) : launch_drop_fwd<32, true>(a, grid, Sp));
    if (rc != LG_OK) return rc;
    LG_CHECK_LAUNCH();
    return LG_OK;
}

extern "C" int lg_attention_dropout_bwd_f32(const float* q, int64_t ldq, int64_t sbq, const float* k, int64_t ldk, int64_t sbk,
                                            const float* v, int64_t ldv, int64_t sbv, const float* g, int64_t ldg, int64_t sbg,
                                            const float* p, float* dq, int64_t lddq, int64_t sbdq, float* dk, int64_t lddk, int64_t sbdk,
                                            float* dv, int64_t lddv, int64_t sbdv, int64_t batch, int64_t heads, int64_t S, int64_t D,
                                            float scale, double prob, const uint64_t* base) {
    LG_REQUIRE_INIT();
    LG_ARG(lg_attention_dropout_supported(S, D), "lg_attention_dropout_bwd_f32: S = %lld (1..512), D = %lld (32 or 64) unsupported",
           (long long)S, (long long)D);
    LG_ARG(prob >= 0.0 && prob < 1.0, "lg_attention_dropout_bwd_f32: p = %g outside [0, 1)", prob);
    LG_ARG(base != nullptr, "lg_attention_dropout_bwd_f32: base is NULL");
    LG_ARG(batch >= 0 && heads >= 1 && batch <= 65535 && heads <= 65535, "lg_attention_dropout_bwd_f32: bad batch / heads");
    if (batch == 0) return LG_OK;
    LG_ARG(ok_operand(q, ldq, sbq) && ok_operand(k, ldk, sbk) && ok_operand(v, ldv, sbv) && ok_operand(g, ldg, sbg) &&
               ok_operand(dq, lddq, sbdq) && ok_operand(dk, lddk, sbdk) && ok_operand(dv, lddv, sbdv) && p && aligned16(p),
           "lg_attention_dropout_bwd_f32: operands must be non-NULL and 16-byte aligned with pitches that are multiples of 4");
    const int64_t w = heads * D;
    LG_ARG(ldq >= w && ldk >= w && ldv >= w && ldg >= w && lddq >= w && lddk >= w && lddv >= w, "lg_attention_dropout_bwd_f32: row pitch below heads * D");
    LG_ARG(batch * heads <= rt().n_attn_pairs && 2 * batch <= 65535, "lg_attention_dropout_bwd_f32: more than %d (batch, head) pairs in one launch",
           rt().n_attn_pairs);
    { int rc = check_rows_write(dq, lddq, sbdq, batch, S, w); if (rc != LG_OK) return rc; }
    { int rc = check_rows_write(dk, lddk, sbdk, batch, S, w); if (rc != LG_OK) return rc; }
    { int rc = check_rows_write(dv, lddv, sbdv, batch, S, w); if (rc != LG_OK) return rc; }
    AttnDrop drop{rt().rng_state, const_cast<unsigned long long*>(reinterpret_cast<const unsigned long long*>(base)), 0u, 0.f, 0};
    rng_threshold(prob, drop.threshold, drop.s);
    if (S > 128)
        return attn_long_drop_bwd(q, ldq, sbq, k, ldk, sbk, v, ldv, sbv, g, ldg, sbg, p, dq, lddq, sbdq, dk, lddk, sbdk, dv, lddv, sbdv,
                                  batch, heads, S, D, scale, drop);
    const int Sp = round32(int(S));
    double* shift = nullptr;
    {
        const int mrc = lg_malloc(reinterpret_cast<void**>(&shift), size_t(batch * heads * Sp) * sizeof(double));
        if (mrc != LG_OK) return mrc;
    }
    AttnBwdDropArgs a{{
#ifdef LG_GEMM_TIMELINE
        timeline_buffer(int(2 * (Sp / 32) * heads * batch)),
#endif
        q, k, v, g, ldq, sbq, ldk, sbk, ldv, sbv, ldg, sbg, p, dq, dk, dv, lddq, sbdq, lddk, sbdk, lddv, sbdv, int(S), int(heads), int(batch), scale,
        shift, rt().attn_flags, rt().status_dev}, drop};
    const dim3 grid(unsigned(Sp / 32), unsigned(heads), unsigned(2 * batch));
    // (which forward ran - plain or tail - makes no difference to the backward's bits; the plain kernels take what they can)
    const bool plain = S % 32 == 0;
    const int rc = D == 64 ? (plain ? launch_drop_bwd<64, false>(a, grid, Sp) : launch_drop_bwd<64, true>(a, grid, Sp))
                           : (plain ? launch_drop_bwd<32, false>(a, grid, Sp) : launch_drop_bwd<32, true>(a, grid, Sp));
    if (rc != LG_OK) { lg_free(shift); return rc; }
    LG_CHECK_LAUNCH();
    return lg_free(shift);          // stream-ordered: the block is only reused by later launches
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
