// Streaming self-attention: any length, no stored probabilities, forward and backward (gfx950, fp32 MFMA).
//
//   forward    O = softmax((Q K^T) * scale + bias) V,   lse = log sum exp of every row         per (batch, head)
//   backward   P = exp(S - lse)   delta = rowsum(dO o O) (+ the row residual, see attn_stream_bwd_q)
//              dS = P o (dO V^T - delta) * scale   dQ = dS K   dK = dS^T Q   dV = P^T dO
//
// attention.hip and attention_long.hip keep a whole score row per query in LDS and write the (batch, heads, S, S) probabilities to
// HBM for the backward; that bounds them at 512 positions and makes P the largest tensor of the step.  Here no row is resident:
// the softmax is ONLINE (a running maximum m and sum l per query, the context rescaled by exp(m_old - m_new) when the maximum
// moves), the forward leaves one float per row (lse = m + log l) and the backward forms P again from it.  LDS holds two chunks of
// 128 rows whatever S is.
//
// Work split.  Forward and query role: one workgroup of 4 waves per 128 queries of a (batch, head); wave w owns queries
// [32 w, 32 w + 32) for the whole launch, its Q (and dO) fragment in registers, and walks ALL keys, which stream through LDS in
// chunks of 128 shared by the four waves (the next chunk's global loads are issued into registers ahead of the MFMAs, as in
// attention_long.hip).  Key role: the same with keys and queries exchanged - 128 keys per workgroup, K and V fragments in
// registers, Q and dO streaming.  The backward is the two launches in stream order: the query role writes delta, the key role
// reads it.  No float atomics, no in-launch hand-off, every fold in a fixed order: the same bits every run.
//
// Operand orientation.  v_mfma_f32_32x32x2f32 leaves lane (r, h) = (lane & 31, lane >> 5) with rows acc_row(e, h) =
// 4 h + (e & 3) + 8 (e >> 2) of column r.  mfma_lds.h feeds the B operand in exactly that k-order: the MFMA number e = 4 g + i of
// a 32-deep product takes k = 8 g + 4 h + i from lane half h.  So a 32 x 32 tile in an accumulator IS the B operand of the next
// product over its rows: element e goes into MFMA e, no LDS round trip, no shuffle.  Every kernel is oriented for that:
//   forward      S^T = K Q^T  (keys x queries)    ->  O^T  += V^T P^T          query role   ->  dQ^T += K^T dS^T
//   key role     S   = Q K^T  (queries x keys)    ->  dV^T += dO^T P,  dK^T += Q^T dS
// With S^T, lane (r, h) holds 16 keys of ONE query r: max and sum of a row are an in-lane fold plus one exchange between the lane
// halves, and m, l, lse, delta and the rescale factor are per-lane scalars.  The outputs come out transposed with four
// consecutive d per lane: 16-byte stores.
//
// Both backward roles form S from the same products in the same k-order (a * b commutes, the two roles swap A and B), add the
// same bias and take the same expf: their P agree bit for bit.
//
// LDS: forward 128 x (D + 4) K rows + 128 x (D + 8) V rows + 128 bias; backward roles 2 x 128 x (D + 4) + 256.  At D = 64: 72 192
// and 70 656 bytes.  K in the query role, Q and dO in the key role are read both K-contiguous (ds_read_b128) and with d along the
// lanes (ds_read_b32); the pitch D + 4 is the b128 reads' one, the b32 reads take a two-way conflict.
#include "attention_common.h"
#include "stream_tiles.h"

namespace lg {

constexpr int kStreamChunk = 128;      // rows of a streamed operand in LDS at a time = rows a workgroup owns
constexpr int64_t kStreamMaxS = 16384; // see lg_attention_stream_supported

struct AttnStreamFwdArgs {
    const float *q, *k, *v;            // element (b, s, head, d) of X at X + b * sbX + s * ldX + head * D + d
    int64_t ldq, sbq, ldk, sbk, ldv, sbv;
    float* o;
    int64_t ldo, sbo;
    float* lse;                        // (batch, heads, S), dense
    const float* mask;                 // key-padding mask as in AttnTailArgs; NULL = none
    int64_t sbm;
    int S, heads;
    float scale;
};

struct AttnStreamBwdArgs {
    const float *q, *k, *v, *o, *g;    // g = gradient of the context
    int64_t ldq, sbq, ldk, sbk, ldv, sbv, ldo, sbo, ldg, sbg;
    const float* lse;
    float* delta;                      // (batch, heads, S): written by the query role, read by the key role
    float *dq, *dk, *dv;
    int64_t lddq, sbdq, lddk, sbdk, lddv, sbdv;
    const float* mask;
    int64_t sbm;
    int S, heads;
    float scale;
};

// DROP instantiations: the same arguments and the call of the random stream (rng_common.h), as attention_long.hip has them
struct AttnStreamFwdDropArgs : AttnStreamFwdArgs {
    AttnDrop drop;
};
struct AttnStreamBwdDropArgs : AttnStreamBwdArgs {
    AttnDrop drop;
};

// frag_load, tile_product, tile_accumulate, halves_sum and store_transposed - the wave-level tiles of the orientation above - are
// stream_tiles.h's: extend_split.hip takes them too.

// ---- DROP: dropout of the probabilities between the softmax and the second product ------------------------------------------------
// D = keep * s is the composite's `probs.dropout(p)`: one call of the stream per attention, element ((b * heads + head) * S + i) * S + j.
//   forward    m, l and lse from the undropped scores; O^T += V^T (D o P)^T
//   backward   dV = (D o P)^T dO   dP = D o (dO V^T)   dS = P o (dP - delta) * scale with the undropped P; delta = rowsum(dO o O)
//              holds as it stands (O contains D), and so does the row residual: sum_j dS_ij is still 0
// No probability is stored, so all three kernels draw the words of every tile they visit again - 40 integer multiplies a Philox
// call next to the tile's MFMAs.  What a lane keeps of them is ONE register: the 16 verdicts word >= threshold of its 16 elements,
// bit e for accumulator element e, formed right behind the tile's first product so that the integer pipe works under the matrix
// cores, and met by the values (rng_keep_bit) once the softmax arithmetic has them.  A4 (S % 4 == 0) picks how few calls that takes:
//   S^T tiles (forward, query role): lane (r, h) holds keys kb + 8 g + 4 h + i, i = 0 .. 3, of ITS query - four consecutive elements
//     of a row.  A4: they are one group of the stream, one call per g; otherwise they straddle two groups, two calls per g.
//   S tiles (key role): lane (r, h) holds ONE key and rows qb + 8 g + 4 h + i - elements S apart, a call per element (16 a tile)
//     when S % 4 != 0.  A4: the four lanes of a quad (keys ki & ~3 .. ki | 3) need, for each row, the four words of ONE group.
//     Lane j = r & 3 calls for row i = j only (4 calls a tile) and the quad exchanges the verdicts: four DPP quad broadcasts of the
//     packed register, lane j picks bit j of every nibble of lane i's - a 4 x 4 transpose per g without LDS.
// Tiles the causal bounds skip draw nothing: the stream is counter-based.  A row or key past the sequence meets words of indices
// that belong to nobody; its probability is deselected to 0 and 0 stays 0 under either verdict.

// S^T tile: bit 4 g + i is element first + 8 g + i of the call (first: this lane's key 4 h of the block, in its query's row)
template <bool A4>
__device__ __forceinline__ uint32_t stream_keep_row(int64_t first, unsigned long long seed, unsigned long long base, uint32_t threshold) {
    uint32_t keep = 0;
#pragma unroll
    for (int g = 0; g < 4; ++g) keep |= rng_keep_bits4<A4>(first + 8 * g, seed, base, threshold) << (4 * g);
    return keep;
}

// every lane of a quad gets the value of its lane I (DPP quad_perm [I, I, I, I]; the four lanes are active together)
template <int I>
__device__ __forceinline__ uint32_t quad_lane(uint32_t x) {
    return uint32_t(__builtin_amdgcn_update_dpp(0, int(x), I * 0x55, 0xf, 0xf, false));
}

// S tile: bit 4 g + i is element (row0 + 8 g + i) * S + key of the call (row0: row 4 h of the block, counted over the whole
// (batch, heads, S) rows; key < S or, with its whole quad, past the sequence)
template <bool A4>
__device__ __forceinline__ uint32_t stream_keep_column(int64_t row0, int key, int S, unsigned long long seed, unsigned long long base,
                                                       uint32_t threshold) {
    uint32_t keep = 0;
    if constexpr (A4) {
        const int j = key & 3;
        uint32_t mine = 0;                                            // bit 4 g + k: (row row0 + 8 g + j, key (key & ~3) + k)
#pragma unroll
        for (int g = 0; g < 4; ++g) mine |= rng_keep_bits4<true>((row0 + 8 * g + j) * S + (key & ~3), seed, base, threshold) << (4 * g);
        keep = ((quad_lane<0>(mine) >> j) & 0x1111u) | ((quad_lane<1>(mine) >> j) & 0x1111u) << 1 |
               ((quad_lane<2>(mine) >> j) & 0x1111u) << 2 | ((quad_lane<3>(mine) >> j) & 0x1111u) << 3;
    } else {
#pragma unroll
        for (int e = 0; e < 16; ++e)
            keep |= uint32_t(rng_word((row0 + 8 * (e >> 2) + (e & 3)) * S + key, seed, base) >= threshold) << e;
    }
    return keep;
}

// rows [c0, c0 + 128) of an operand of S rows: global -> registers (c0 < S; only rows < S are addressed) and registers -> LDS, the
// rows past S ZERO: they are MFMA operands
template <int D, int N>
__device__ __forceinline__ void stream_load(af32x4 (&v)[N], const float* x, int64_t ld, int c0, int S) {
    load_rows<D, N>(v, x + int64_t(c0) * ld, ld, S - c0 < kStreamChunk ? S - c0 : kStreamChunk);
}
template <int D, int N>
__device__ __forceinline__ void stream_store(const af32x4 (&v)[N], float* dst, int pitch, int c0, int S) {
    store_rows_padded<D, N>(v, dst, pitch, S - c0 < kStreamChunk ? S - c0 : kStreamChunk, kStreamChunk);
}

// what key j adds to every score of its column: (1.0 - mask) * -10000.0 in fp32, the composite's own arithmetic; -0.0f where there
// is no mask or no key (adding it changes no bit)
__device__ __forceinline__ float key_bias(const float* mask, int64_t sbm, int b, int j, int S) {
    return (mask && j < S) ? (1.0f - mask[int64_t(b) * sbm + j]) * -10000.0f : -0.0f;
}

template <int D> constexpr int attn_stream_fwd_lds_floats() { return kStreamChunk * (D + 4) + kStreamChunk * (D + 8) + kStreamChunk; }
template <int D> constexpr int attn_stream_bwd_lds_floats() { return 2 * kStreamChunk * (D + 4) + 2 * kStreamChunk; }

// CAUSAL: query i sees keys j <= i.  The workgroup visits the key chunks up to the one that holds its last query, a wave the
// 32-key blocks up to the one that holds ITS last query: nothing wholly above the diagonal costs an MFMA.
// DROP: this launch IS the call of the stream - thread 0 of every workgroup reads seed and `draws`, takes its group's ticket and,
// after its last use, lets the last arriver advance `draws` (the order of attn_long_fwd); workgroup 0 leaves the call's number for
// the backward.
template <int D, bool CAUSAL, bool DROP = false, bool A4 = false>
__global__ void __launch_bounds__(256, DROP ? 2 : 1) attn_stream_fwd(std::conditional_t<DROP, AttnStreamFwdDropArgs, AttnStreamFwdArgs> a) {
    extern __shared__ __attribute__((aligned(16))) float lds[];
    constexpr int PK = D + 4, PV = D + 8, NA = kStreamChunk * (D / 4) / 256, NT = D / 32;
    float* Ks = lds;                      // a chunk of K, K-contiguous A of S^T            128 x PK
    float* Vs = Ks + kStreamChunk * PK;   // the same chunk of V, d along the lanes          128 x PV
    float* Bias = Vs + kStreamChunk * PV; // the bias of the chunk's keys                    128
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, r = lane & 31, h = lane >> 5;
    const int S = a.S, q0 = blockIdx.x * kStreamChunk, head = blockIdx.y, b = blockIdx.z;
    const int qw = q0 + 32 * wave, qi = qw + r;                       // the wave's first query, this lane's query
    const float* kg = a.k + int64_t(b) * a.sbk + head * D;
    const float* vg = a.v + int64_t(b) * a.sbv + head * D;
    const int kend = CAUSAL ? (q0 + kStreamChunk < S ? q0 + kStreamChunk : S) : S;        // the keys this workgroup visits
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

    float qf[D / 2];
    frag_load<D>(qf, qi < S ? a.q + int64_t(b) * a.sbq + int64_t(qi) * a.ldq + head * D : nullptr, h);
    af32x4 rk[NA], rv[NA];
    float rb = 0.f;
    stream_load<D, NA>(rk, kg, a.ldk, 0, S);
    stream_load<D, NA>(rv, vg, a.ldv, 0, S);
    if (tid < kStreamChunk) rb = key_bias(a.mask, a.sbm, b, tid, S);
    // element 0 of this lane's query row in the call, plus the lane half's 4 h
    [[maybe_unused]] unsigned long long seed = 0, base = 0;
    [[maybe_unused]] int64_t drow = 0;
    if constexpr (DROP) {
        __syncthreads();                                              // thread 0's call words are in LDS
        seed = rng_uniform64(call[0]);
        base = rng_uniform64(call[1]);
        drow = ((int64_t(b) * a.heads + head) * S + qi) * S + 4 * h;
    }

    // Key 0 is visible to every row (0 < S, 0 <= i) and lies in the first block a wave visits: m is finite from the first block
    // on, so m - m_new and s - m_new never meet inf - inf (a block with no visible key of some row leaves that row's m as it was)
    float m = -INFINITY, l = 0.f;
    af32x16 ot[NT];
#pragma unroll
    for (int n = 0; n < NT; ++n) ot[n] = zero16();

    for (int c0 = 0; c0 < kend; c0 += kStreamChunk) {
        stream_store<D, NA>(rk, Ks, PK, c0, S);
        stream_store<D, NA>(rv, Vs, PV, c0, S);
        if (tid < kStreamChunk) Bias[tid] = rb;
        __syncthreads();
        if (c0 + kStreamChunk < kend) {
            stream_load<D, NA>(rk, kg, a.ldk, c0 + kStreamChunk, S);
            stream_load<D, NA>(rv, vg, a.ldv, c0 + kStreamChunk, S);
            if (tid < kStreamChunk) rb = key_bias(a.mask, a.sbm, b, c0 + kStreamChunk + tid, S);
        }
        for (int blk = 0; blk < 4; ++blk) {
            const int kb = c0 + 32 * blk;
            if (kb >= kend || (CAUSAL && kb > qw + 31)) break;        // wave-uniform
            af32x16 st = tile_product<D>(Ks, 32 * blk, qf, r, h);     // S^T: element e is (key kb + acc_row(e, h), query qi)
            [[maybe_unused]] uint32_t keep = 0;
            if constexpr (DROP) keep = stream_keep_row<A4>(drow + kb, seed, base, a.drop.threshold);
            // the product rounded to fp32 first, then * scale, then + bias; a key >= S, CAUSAL a key > qi: deselected
            float bm = -INFINITY;
#pragma unroll
            for (int g = 0; g < 4; ++g) {
                const af32x4 bias = *reinterpret_cast<const af32x4*>(Bias + 32 * blk + 8 * g + 4 * h);
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    const int key = kb + 8 * g + 4 * h + i;
                    float x = st[4 * g + i] * a.scale + bias[i];
                    if (key >= S || (CAUSAL && key > qi)) x = -INFINITY;
                    st[4 * g + i] = x;
                    bm = x > bm ? x : bm;
                }
            }
            { const float other = __shfl_xor(bm, 32, 64); bm = other > bm ? other : bm; }
            const float mn = bm > m ? bm : m;
            const float alpha = expf(m - mn);                         // 0 at the first block (m = -inf, mn finite)
            float ps = 0.f;
#pragma unroll
            for (int e = 0; e < 16; ++e) { st[e] = expf(st[e] - mn); ps += st[e]; }       // P^T, unnormalised; 0 where deselected
            l = l * alpha + halves_sum(ps, h);
            m = mn;
            if constexpr (DROP) {                                     // (D o P)^T: l has the undropped sum
#pragma unroll
                for (int e = 0; e < 16; ++e) st[e] = rng_keep_bit(st[e], (keep >> e) & 1u, a.drop.s);
            }
#pragma unroll
            for (int n = 0; n < NT; ++n)
#pragma unroll
                for (int e = 0; e < 16; ++e) ot[n][e] *= alpha;
            tile_accumulate<D>(ot, Vs, PV, 32 * blk, st, r, h);       // O^T += V^T P^T
        }
        __syncthreads();
    }
    if (qi < S) {
        store_transposed<D>(a.o + int64_t(b) * a.sbo + int64_t(qi) * a.ldo + head * D, ot, 1.0f / l, h);
        if (h == 0) a.lse[(int64_t(b) * a.heads + head) * S + qi] = m + logf(l);
    }
    if constexpr (DROP) {
        if (tid == 0) rng_last_arriver_advances(a.drop.state, tickets, mine, order, grp, groups, a.drop.group, grid_blocks(), base);
    }
}

// P^T (or P) of one element from its accumulator value: the forward's score arithmetic, then exp(s - lse); 0 where deselected
__device__ __forceinline__ float stream_prob(float acc, float scale, float bias, float lse, bool gone) {
    return gone ? 0.f : expf((acc * scale + bias) - lse);
}

// query role: dQ of 128 queries, and delta of their rows for the key role.  Work split, chunk loop and CAUSAL bounds: the forward's.
// The row residual.  Mathematically sum_j dS_ij = 0; with delta = rowsum(dO o O) from the ROUNDED context and P from the rounded
// lse the sum is some rho_i ~ 1e-7 |delta_i| instead, the same sign along the whole row - and dQ_i = sum_j dS_ij K_j picks up
// rho_i times the mean key, which is all of the error when the keys of a row are alike and the true dQ is small (rowwise.hip:
// softmax_bwd forms its shift in double for this reason).  Here the row is never resident, so the wave measures the residual
// instead: it sums u_ij = P_ij (dP_ij - delta_i) and P_ij per lane, accumulates (P K)^T next to dQ^T, and at the end takes
// c_i = sum_j u_ij / sum_j P_ij out: dQ_i -= c_i * scale * (P K)_i - exactly dQ under the shift delta_i + c_i, whose row sum is 0.
// That corrected shift is what it writes for the key role.
// DROP (both roles): the forward's mask again from the seed in the generator's state and the call number the forward wrote;
// nothing is drawn.
template <int D, bool CAUSAL, bool DROP = false, bool A4 = false>
__global__ void __launch_bounds__(256) attn_stream_bwd_q(std::conditional_t<DROP, AttnStreamBwdDropArgs, AttnStreamBwdArgs> a) {
    extern __shared__ __attribute__((aligned(16))) float lds[];
    constexpr int PK = D + 4, NA = kStreamChunk * (D / 4) / 256, NT = D / 32;
    float* Ks = lds;                      // a chunk of K: K-contiguous A of S^T, d along the lanes for dQ^T    128 x PK
    float* Vs = Ks + kStreamChunk * PK;   // the same chunk of V, K-contiguous A of dP^T                        128 x PK
    float* Bias = Vs + kStreamChunk * PK;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, r = lane & 31, h = lane >> 5;
    const int S = a.S, q0 = blockIdx.x * kStreamChunk, head = blockIdx.y, b = blockIdx.z;
    const int qw = q0 + 32 * wave, qi = qw + r;
    const float* kg = a.k + int64_t(b) * a.sbk + head * D;
    const float* vg = a.v + int64_t(b) * a.sbv + head * D;
    const int kend = CAUSAL ? (q0 + kStreamChunk < S ? q0 + kStreamChunk : S) : S;
    const int64_t row = (int64_t(b) * a.heads + head) * S + qi;

    // a query past the sequence: zeros and lse = 0 - finite values in its own column of every tile, never stored
    float qf[D / 2], gf[D / 2];
    frag_load<D>(qf, qi < S ? a.q + int64_t(b) * a.sbq + int64_t(qi) * a.ldq + head * D : nullptr, h);
    frag_load<D>(gf, qi < S ? a.g + int64_t(b) * a.sbg + int64_t(qi) * a.ldg + head * D : nullptr, h);
    float delta;
    {
        float of[D / 2], part = 0.f;
        frag_load<D>(of, qi < S ? a.o + int64_t(b) * a.sbo + int64_t(qi) * a.ldo + head * D : nullptr, h);
#pragma unroll
        for (int j = 0; j < D / 2; ++j) part += gf[j] * of[j];
        delta = halves_sum(part, h);
    }
    const float lse = qi < S ? a.lse[row] : 0.f;
    [[maybe_unused]] unsigned long long seed = 0, base = 0;
    if constexpr (DROP) { seed = a.drop.state[0]; base = a.drop.base[0]; }
    af32x4 rk[NA], rv[NA];
    float rb = 0.f;
    stream_load<D, NA>(rk, kg, a.ldk, 0, S);
    stream_load<D, NA>(rv, vg, a.ldv, 0, S);
    if (tid < kStreamChunk) rb = key_bias(a.mask, a.sbm, b, tid, S);
    af32x16 dqt[NT], pkt[NT];
#pragma unroll
    for (int n = 0; n < NT; ++n) { dqt[n] = zero16(); pkt[n] = zero16(); }
    float usum = 0.f, psum = 0.f;                                     // this lane's share of the row sums of u and P

    for (int c0 = 0; c0 < kend; c0 += kStreamChunk) {
        stream_store<D, NA>(rk, Ks, PK, c0, S);
        stream_store<D, NA>(rv, Vs, PK, c0, S);
        if (tid < kStreamChunk) Bias[tid] = rb;
        __syncthreads();
        if (c0 + kStreamChunk < kend) {
            stream_load<D, NA>(rk, kg, a.ldk, c0 + kStreamChunk, S);
            stream_load<D, NA>(rv, vg, a.ldv, c0 + kStreamChunk, S);
            if (tid < kStreamChunk) rb = key_bias(a.mask, a.sbm, b, c0 + kStreamChunk + tid, S);
        }
        for (int blk = 0; blk < 4; ++blk) {
            const int kb = c0 + 32 * blk;
            if (kb >= kend || (CAUSAL && kb > qw + 31)) break;
            af32x16 st = tile_product<D>(Ks, 32 * blk, qf, r, h);             // S^T = K Q^T, then P^T
            af32x16 dpt = tile_product<D>(Vs, 32 * blk, gf, r, h);            // dP^T = V dO^T, then dS^T
            [[maybe_unused]] uint32_t keep = 0;
            if constexpr (DROP) keep = stream_keep_row<A4>(row * S + 4 * h + kb, seed, base, a.drop.threshold);
#pragma unroll
            for (int g = 0; g < 4; ++g) {
                const af32x4 bias = *reinterpret_cast<const af32x4*>(Bias + 32 * blk + 8 * g + 4 * h);
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    const int key = kb + 8 * g + 4 * h + i, e = 4 * g + i;
                    const float p = stream_prob(st[e], a.scale, bias[i], lse, key >= S || (CAUSAL && key > qi));
                    if constexpr (DROP) dpt[e] = rng_keep_bit(dpt[e], (keep >> e) & 1u, a.drop.s);       // dP = D o (dO V^T)
                    const float u = p * (dpt[e] - delta);
                    st[e] = p;
                    dpt[e] = u * a.scale;
                    psum += p;
                    usum += u;
                }
            }
            tile_accumulate<D>(dqt, Ks, PK, 32 * blk, dpt, r, h);             // dQ^T += K^T dS^T
            tile_accumulate<D>(pkt, Ks, PK, 32 * blk, st, r, h);              // (P K)^T += K^T P^T
        }
        __syncthreads();
    }
    // psum > 0: key 0 is visible to every row and P of the row maximum is about 1 / l
    const float c = halves_sum(usum, h) / halves_sum(psum, h);
    if (qi < S) {
        const float cs = c * a.scale;
#pragma unroll
        for (int n = 0; n < NT; ++n)
#pragma unroll
            for (int e = 0; e < 16; ++e) dqt[n][e] -= cs * pkt[n][e];
        store_transposed<D>(a.dq + int64_t(b) * a.sbdq + int64_t(qi) * a.lddq + head * D, dqt, 1.0f, h);
        if (h == 0) a.delta[row] = delta + c;
    }
}

// key role: dK and dV of 128 keys.  CAUSAL: key j is seen by queries i >= j - the query chunks start at the one that holds the
// workgroup's first key, and a wave skips the 32-query blocks that end before ITS first key.
template <int D, bool CAUSAL, bool DROP = false, bool A4 = false>
__global__ void __launch_bounds__(256) attn_stream_bwd_kv(std::conditional_t<DROP, AttnStreamBwdDropArgs, AttnStreamBwdArgs> a) {
    extern __shared__ __attribute__((aligned(16))) float lds[];
    constexpr int PQ = D + 4, NA = kStreamChunk * (D / 4) / 256, NT = D / 32;
    float* Qs = lds;                      // a chunk of Q: K-contiguous A of S, d along the lanes for dK^T      128 x PQ
    float* Gs = Qs + kStreamChunk * PQ;   // the same chunk of dO: K-contiguous A of dP, d along the lanes for dV^T
    float* Lse = Gs + kStreamChunk * PQ;  // lse and delta of the chunk's queries                               2 x 128
    float* Del = Lse + kStreamChunk;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, r = lane & 31, h = lane >> 5;
    const int S = a.S, k0 = blockIdx.x * kStreamChunk, head = blockIdx.y, b = blockIdx.z;
    const int kw = k0 + 32 * wave, ki = kw + r;                       // the wave's first key, this lane's key
    const float* qg = a.q + int64_t(b) * a.sbq + head * D;
    const float* gg = a.g + int64_t(b) * a.sbg + head * D;
    const float* lrow = a.lse + (int64_t(b) * a.heads + head) * S;
    const float* drow = a.delta + (int64_t(b) * a.heads + head) * S;
    const int cbeg = CAUSAL ? k0 : 0;                                 // k0 < S: the grid covers no more

    float kf[D / 2], vf[D / 2];
    frag_load<D>(kf, ki < S ? a.k + int64_t(b) * a.sbk + int64_t(ki) * a.ldk + head * D : nullptr, h);
    frag_load<D>(vf, ki < S ? a.v + int64_t(b) * a.sbv + int64_t(ki) * a.ldv + head * D : nullptr, h);
    const float bias = key_bias(a.mask, a.sbm, b, ki, S);
    [[maybe_unused]] unsigned long long seed = 0, base = 0;
    if constexpr (DROP) { seed = a.drop.state[0]; base = a.drop.base[0]; }
    af32x4 rq[NA], rg[NA];
    float rl = 0.f, rd = 0.f;
    stream_load<D, NA>(rq, qg, a.ldq, cbeg, S);
    stream_load<D, NA>(rg, gg, a.ldg, cbeg, S);
    if (tid < kStreamChunk && cbeg + tid < S) { rl = lrow[cbeg + tid]; rd = drow[cbeg + tid]; }
    af32x16 dkt[NT], dvt[NT];
#pragma unroll
    for (int n = 0; n < NT; ++n) { dkt[n] = zero16(); dvt[n] = zero16(); }

    for (int c0 = cbeg; c0 < S; c0 += kStreamChunk) {
        stream_store<D, NA>(rq, Qs, PQ, c0, S);
        stream_store<D, NA>(rg, Gs, PQ, c0, S);
        if (tid < kStreamChunk) { Lse[tid] = rl; Del[tid] = rd; }     // (0 for a query past the sequence: its P is deselected)
        __syncthreads();
        if (c0 + kStreamChunk < S) {
            const int c1 = c0 + kStreamChunk;
            stream_load<D, NA>(rq, qg, a.ldq, c1, S);
            stream_load<D, NA>(rg, gg, a.ldg, c1, S);
            rl = rd = 0.f;
            if (tid < kStreamChunk && c1 + tid < S) { rl = lrow[c1 + tid]; rd = drow[c1 + tid]; }
        }
        for (int blk = 0; blk < 4 && kw < S; ++blk) {
            const int qb = c0 + 32 * blk;
            if (qb >= S) break;
            if (CAUSAL && qb + 31 < kw) continue;                     // wave-uniform
            af32x16 p = tile_product<D>(Qs, 32 * blk, kf, r, h);      // S = Q K^T: element e is (query qb + acc_row(e, h), key ki)
            af32x16 ds = tile_product<D>(Gs, 32 * blk, vf, r, h);     // dP = dO V^T
            [[maybe_unused]] uint32_t keep = 0;
            if constexpr (DROP)
                keep = stream_keep_column<A4>((int64_t(b) * a.heads + head) * S + qb + 4 * h, ki, S, seed, base, a.drop.threshold);
#pragma unroll
            for (int g = 0; g < 4; ++g) {
                const af32x4 l4 = *reinterpret_cast<const af32x4*>(Lse + 32 * blk + 8 * g + 4 * h);
                const af32x4 d4 = *reinterpret_cast<const af32x4*>(Del + 32 * blk + 8 * g + 4 * h);
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    const int qrow = qb + 8 * g + 4 * h + i, e = 4 * g + i;
                    p[e] = stream_prob(p[e], a.scale, bias, l4[i], qrow >= S || ki >= S || (CAUSAL && ki > qrow));
                    if constexpr (DROP) ds[e] = rng_keep_bit(ds[e], (keep >> e) & 1u, a.drop.s);         // dP = D o (dO V^T)
                    ds[e] = p[e] * (ds[e] - d4[i]) * a.scale;
                    if constexpr (DROP) p[e] = rng_keep_bit(p[e], (keep >> e) & 1u, a.drop.s);           // D o P, for dV
                }
            }
            tile_accumulate<D>(dvt, Gs, PQ, 32 * blk, p, r, h);       // dV^T += dO^T P (DROP: D o P)
            tile_accumulate<D>(dkt, Qs, PQ, 32 * blk, ds, r, h);      // dK^T += Q^T dS
        }
        __syncthreads();
    }
    if (ki < S) {
        store_transposed<D>(a.dk + int64_t(b) * a.sbdk + int64_t(ki) * a.lddk + head * D, dkt, 1.0f, h);
        store_transposed<D>(a.dv + int64_t(b) * a.sbdv + int64_t(ki) * a.lddv + head * D, dvt, 1.0f, h);
    }
}

// ---- host side -------------------------------------------------------------------------------------------------------------
template <class K, class A>
static int stream_launch(K kernel, const A& a, dim3 grid, size_t bytes) {
    int rc = allow_lds(kernel, bytes);
    if (rc != LG_OK) return rc;
    hipLaunchKernelGGL(kernel, grid, dim3(256), bytes, rt().stream, a);
    return LG_OK;
}

// [causal][drop ? 1 + (S % 4 == 0) : 0]: the kernel of a call; the DROP = false instantiations take the base of the argument struct
template <int D>
static int stream_fwd_as(const AttnStreamFwdDropArgs& a, dim3 grid, bool causal, bool drop) {
    const size_t bytes = size_t(attn_stream_fwd_lds_floats<D>()) * 4;
    const AttnStreamFwdArgs& plain = a;
    if (!drop) return causal ? stream_launch(&attn_stream_fwd<D, true>, plain, grid, bytes) : stream_launch(&attn_stream_fwd<D, false>, plain, grid, bytes);
    if (a.S % 4 == 0)
        return causal ? stream_launch(&attn_stream_fwd<D, true, true, true>, a, grid, bytes) : stream_launch(&attn_stream_fwd<D, false, true, true>, a, grid, bytes);
    return causal ? stream_launch(&attn_stream_fwd<D, true, true, false>, a, grid, bytes) : stream_launch(&attn_stream_fwd<D, false, true, false>, a, grid, bytes);
}

template <int D, bool CAUSAL>
static int stream_bwd_roles(const AttnStreamBwdDropArgs& a, dim3 grid, bool drop) {
    const size_t bytes = size_t(attn_stream_bwd_lds_floats<D>()) * 4;
    const AttnStreamBwdArgs& plain = a;
    int rc;
    if (!drop) {
        rc = stream_launch(&attn_stream_bwd_q<D, CAUSAL>, plain, grid, bytes);
        return rc != LG_OK ? rc : stream_launch(&attn_stream_bwd_kv<D, CAUSAL>, plain, grid, bytes);
    }
#ifdef LG_STREAM_DROP_KEY_ROLE_PER_ELEMENT              // experiments only: the key role's per-element form also at S % 4 == 0
    constexpr bool QUAD = false;
#else
    constexpr bool QUAD = true;
#endif
    if (a.S % 4 == 0) {
        rc = stream_launch(&attn_stream_bwd_q<D, CAUSAL, true, true>, a, grid, bytes);
        return rc != LG_OK ? rc : stream_launch(&attn_stream_bwd_kv<D, CAUSAL, true, QUAD>, a, grid, bytes);
    }
    rc = stream_launch(&attn_stream_bwd_q<D, CAUSAL, true, false>, a, grid, bytes);
    return rc != LG_OK ? rc : stream_launch(&attn_stream_bwd_kv<D, CAUSAL, true, false>, a, grid, bytes);
}

template <int D>
static int stream_bwd_as(const AttnStreamBwdDropArgs& a, dim3 grid, bool causal, bool drop) {
    return causal ? stream_bwd_roles<D, true>(a, grid, drop) : stream_bwd_roles<D, false>(a, grid, drop);
}

static bool stream_operand(const void* p, int64_t ld, int64_t sb) { return p && aligned16(p) && ld % 4 == 0 && sb % 4 == 0; }

// the checks every stream entry starts with, in the order of attn_forward (attention.hip); 1: an empty batch, nothing to do
static int stream_check(const char* name, int64_t batch, int64_t heads, int64_t S, int64_t D) {
    LG_ARG(lg_attention_stream_supported(S, D), "%s: S = %lld (1..%lld), D = %lld (32 or 64) unsupported", name, (long long)S,
           (long long)kStreamMaxS, (long long)D);
    LG_ARG(batch >= 0 && heads >= 1 && batch <= 65535 && heads <= 65535, "%s: bad batch / heads", name);
    return batch == 0 ? 1 : LG_OK;
}

// what the dropout entries check on top: the probability, the word of the call's number, and what one call of the stream covers
// (lightgrad_amd/random.py: kRngMaxElements elements, kRngMaxGroup^2 workgroups); then threshold and s as attn_forward derives them
static int stream_drop(const char* name, double p, const unsigned long long* base, int64_t batch, int64_t heads, int64_t S, AttnDrop& drop) {
    LG_ARG(p >= 0.0 && p < 1.0, "%s: p = %g outside [0, 1)", name, p);
    LG_ARG(base != nullptr, "%s: base is NULL", name);
    LG_ARG(batch * heads * S * S <= kRngMaxElements, "%s: %lld x %lld x %lld x %lld probabilities, more than the kRngMaxElements = %lld of one call of the stream",
           name, (long long)batch, (long long)heads, (long long)S, (long long)S, (long long)kRngMaxElements);
    const int64_t wgs = (S + kStreamChunk - 1) / kStreamChunk * heads * batch;
    LG_ARG(wgs <= int64_t(kRngMaxGroup) * kRngMaxGroup, "%s: %lld workgroups, more than the stream's tickets count", name, (long long)wgs);
    drop = AttnDrop{rt().rng_state, const_cast<unsigned long long*>(base), 0u, 0.f, rng_group(unsigned(wgs))};
    rng_threshold(p, drop.threshold, drop.s);
    return LG_OK;
}

// the one path behind the two forward entries; base != NULL: the dropout entry
static int stream_forward(const char* name, const float* q, int64_t ldq, int64_t sbq, const float* k, int64_t ldk, int64_t sbk,
                          const float* v, int64_t ldv, int64_t sbv, float* o, int64_t ldo, int64_t sbo, float* lse,
                          int64_t batch, int64_t heads, int64_t S, int64_t D, float scale, const float* mask, int64_t sbm, int causal,
                          bool drops, double p, unsigned long long* base) {
    { const int rc = stream_check(name, batch, heads, S, D); if (rc < 0) return rc; if (rc != LG_OK && !drops) return LG_OK; }
    AttnDrop drop{};
    if (drops) {
        LG_ARG(batch > 0, "%s: an empty batch draws nothing (batch must be >= 1)", name);
        const int rc = stream_drop(name, p, base, batch, heads, S, drop);
        if (rc != LG_OK) return rc;
    }
    const int64_t w = heads * D;
    LG_ARG(stream_operand(q, ldq, sbq) && stream_operand(k, ldk, sbk) && stream_operand(v, ldv, sbv) && stream_operand(o, ldo, sbo) && lse,
           "%s: operands must be non-NULL and 16-byte aligned with pitches that are multiples of 4 (lse: non-NULL)", name);
    LG_ARG(ldq >= w && ldk >= w && ldv >= w && ldo >= w, "%s: row pitch below heads * D", name);
    LG_ARG(!mask || sbm == 0 || sbm >= S, "%s: mask batch pitch %lld is neither 0 (one row for the batch) nor >= S", name, (long long)sbm);
    const AttnStreamFwdDropArgs a{{q, k, v, ldq, sbq, ldk, sbk, ldv, sbv, o, ldo, sbo, lse, mask, sbm, int(S), int(heads), scale}, drop};
    const dim3 grid(unsigned((S + kStreamChunk - 1) / kStreamChunk), unsigned(heads), unsigned(batch));
    const int rc = D == 64 ? stream_fwd_as<64>(a, grid, causal != 0, drops) : stream_fwd_as<32>(a, grid, causal != 0, drops);
    if (rc != LG_OK) return rc;
    LG_CHECK_LAUNCH();
    return LG_OK;
}

static int stream_backward(const char* name, const float* q, int64_t ldq, int64_t sbq, const float* k, int64_t ldk, int64_t sbk,
                           const float* v, int64_t ldv, int64_t sbv, const float* o, int64_t ldo, int64_t sbo,
                           const float* g, int64_t ldg, int64_t sbg, const float* lse, float* delta,
                           float* dq, int64_t lddq, int64_t sbdq, float* dk, int64_t lddk, int64_t sbdk,
                           float* dv, int64_t lddv, int64_t sbdv, int64_t batch, int64_t heads, int64_t S, int64_t D,
                           float scale, const float* mask, int64_t sbm, int causal, bool drops, double p, const unsigned long long* base) {
    { const int rc = stream_check(name, batch, heads, S, D); if (rc < 0) return rc; if (rc != LG_OK && !drops) return LG_OK; }
    AttnDrop drop{};
    if (drops) {
        const int rc = stream_drop(name, p, base, batch, heads, S, drop);
        if (rc != LG_OK) return rc;
        if (batch == 0) return LG_OK;
    }
    const int64_t w = heads * D;
    LG_ARG(stream_operand(q, ldq, sbq) && stream_operand(k, ldk, sbk) && stream_operand(v, ldv, sbv) && stream_operand(o, ldo, sbo) &&
               stream_operand(g, ldg, sbg) && stream_operand(dq, lddq, sbdq) && stream_operand(dk, lddk, sbdk) &&
               stream_operand(dv, lddv, sbdv) && lse && delta,
           "%s: operands must be non-NULL and 16-byte aligned with pitches that are multiples of 4 (lse, delta: non-NULL)", name);
    LG_ARG(ldq >= w && ldk >= w && ldv >= w && ldo >= w && ldg >= w && lddq >= w && lddk >= w && lddv >= w, "%s: row pitch below heads * D", name);
    LG_ARG(!mask || sbm == 0 || sbm >= S, "%s: mask batch pitch %lld is neither 0 (one row for the batch) nor >= S", name, (long long)sbm);
    const AttnStreamBwdDropArgs a{{q, k, v, o, g, ldq, sbq, ldk, sbk, ldv, sbv, ldo, sbo, ldg, sbg, lse, delta, dq, dk, dv,
                                   lddq, sbdq, lddk, sbdk, lddv, sbdv, mask, sbm, int(S), int(heads), scale}, drop};
    const dim3 grid(unsigned((S + kStreamChunk - 1) / kStreamChunk), unsigned(heads), unsigned(batch));
    const int rc = D == 64 ? stream_bwd_as<64>(a, grid, causal != 0, drops) : stream_bwd_as<32>(a, grid, causal != 0, drops);
    if (rc != LG_OK) return rc;
    LG_CHECK_LAUNCH();
    return LG_OK;
}

}  // namespace lg

using namespace lg;

// The bound is the largest length the index arithmetic has been checked for: every position (q0 + 127, c0 + 128 + tid, a key or
// query index) is an int below 2^15, every global offset is formed in int64_t, the grid's x is S / 128 <= 128.  LDS and registers do
// not depend on S.
extern "C" int lg_attention_stream_supported(int64_t S, int64_t D) {
    return (D == 64 || D == 32) && S >= 1 && S <= kStreamMaxS;
}

extern "C" int lg_attention_stream_fwd_f32(const float* q, int64_t ldq, int64_t sbq, const float* k, int64_t ldk, int64_t sbk,
                                           const float* v, int64_t ldv, int64_t sbv, float* o, int64_t ldo, int64_t sbo, float* lse,
                                           int64_t batch, int64_t heads, int64_t S, int64_t D, float scale,
                                           const float* mask, int64_t sbm, int causal) {
    LG_REQUIRE_INIT();
    return stream_forward("lg_attention_stream_fwd_f32", q, ldq, sbq, k, ldk, sbk, v, ldv, sbv, o, ldo, sbo, lse, batch, heads, S, D, scale,
                          mask, sbm, causal, false, 0.0, nullptr);
}

extern "C" int lg_attention_stream_bwd_f32(const float* q, int64_t ldq, int64_t sbq, const float* k, int64_t ldk, int64_t sbk,
                                           const float* v, int64_t ldv, int64_t sbv, const float* o, int64_t ldo, int64_t sbo,
                                           const float* g, int64_t ldg, int64_t sbg, const float* lse, float* delta,
                                           float* dq, int64_t lddq, int64_t sbdq, float* dk, int64_t lddk, int64_t sbdk,
                                           float* dv, int64_t lddv, int64_t sbdv, int64_t batch, int64_t heads, int64_t S, int64_t D,
                                           float scale, const float* mask, int64_t sbm, int causal) {
    LG_REQUIRE_INIT();
    return stream_backward("lg_attention_stream_bwd_f32", q, ldq, sbq, k, ldk, sbk, v, ldv, sbv, o, ldo, sbo, g, ldg, sbg, lse, delta,
                           dq, lddq, sbdq, dk, lddk, sbdk, dv, lddv, sbdv, batch, heads, S, D, scale, mask, sbm, causal, false, 0.0, nullptr);
}

extern "C" int lg_attention_stream_dropout_fwd_f32(const float* q, int64_t ldq, int64_t sbq, const float* k, int64_t ldk, int64_t sbk,
                                                   const float* v, int64_t ldv, int64_t sbv, float* o, int64_t ldo, int64_t sbo, float* lse,
                                                   int64_t batch, int64_t heads, int64_t S, int64_t D, float scale,
                                                   const float* mask, int64_t sbm, int causal, double p, unsigned long long* base) {
    LG_REQUIRE_INIT();
    return stream_forward("lg_attention_stream_dropout_fwd_f32", q, ldq, sbq, k, ldk, sbk, v, ldv, sbv, o, ldo, sbo, lse, batch, heads, S, D,
                          scale, mask, sbm, causal, true, p, base);
}

extern "C" int lg_attention_stream_dropout_bwd_f32(const float* q, int64_t ldq, int64_t sbq, const float* k, int64_t ldk, int64_t sbk,
                                                   const float* v, int64_t ldv, int64_t sbv, const float* o, int64_t ldo, int64_t sbo,
                                                   const float* g, int64_t ldg, int64_t sbg, const float* lse, float* delta,
                                                   float* dq, int64_t lddq, int64_t sbdq, float* dk, int64_t lddk, int64_t sbdk,
                                                   float* dv, int64_t lddv, int64_t sbdv, int64_t batch, int64_t heads, int64_t S, int64_t D,
                                                   float scale, const float* mask, int64_t sbm, int causal, double p,
                                                   const unsigned long long* base) {
    LG_REQUIRE_INIT();
    return stream_backward("lg_attention_stream_dropout_bwd_f32", q, ldq, sbq, k, ldk, sbk, v, ldv, sbv, o, ldo, sbo, g, ldg, sbg, lse, delta,
                           dq, lddq, sbdq, dk, lddk, sbdk, dv, lddv, sbdv, batch, heads, S, D, scale, mask, sbm, causal, true, p, base);
}
