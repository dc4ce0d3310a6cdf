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

// frag_load, tile_product, tile_accumulate, halves_sum and store_transposed - the wave-level tiles of the orientation above - are
// stream_tiles.h's: extend_split.hip takes them too.

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
template <int D, bool CAUSAL>
__global__ void __launch_bounds__(256) attn_stream_fwd(AttnStreamFwdArgs a) {
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

    float qf[D / 2];
    frag_load<D>(qf, qi < S ? a.q + int64_t(b) * a.sbq + int64_t(qi) * a.ldq + head * D : nullptr, h);
    af32x4 rk[NA], rv[NA];
    float rb = 0.f;
    stream_load<D, NA>(rk, kg, a.ldk, 0, S);
    stream_load<D, NA>(rv, vg, a.ldv, 0, S);
    if (tid < kStreamChunk) rb = key_bias(a.mask, a.sbm, b, tid, S);

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
template <int D, bool CAUSAL>
__global__ void __launch_bounds__(256) attn_stream_bwd_q(AttnStreamBwdArgs a) {
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
#pragma unroll
            for (int g = 0; g < 4; ++g) {
                const af32x4 bias = *reinterpret_cast<const af32x4*>(Bias + 32 * blk + 8 * g + 4 * h);
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    const int key = kb + 8 * g + 4 * h + i, e = 4 * g + i;
                    const float p = stream_prob(st[e], a.scale, bias[i], lse, key >= S || (CAUSAL && key > qi));
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
template <int D, bool CAUSAL>
__global__ void __launch_bounds__(256) attn_stream_bwd_kv(AttnStreamBwdArgs a) {
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
#pragma unroll
            for (int g = 0; g < 4; ++g) {
                const af32x4 l4 = *reinterpret_cast<const af32x4*>(Lse + 32 * blk + 8 * g + 4 * h);
                const af32x4 d4 = *reinterpret_cast<const af32x4*>(Del + 32 * blk + 8 * g + 4 * h);
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    const int qrow = qb + 8 * g + 4 * h + i, e = 4 * g + i;
                    p[e] = stream_prob(p[e], a.scale, bias, l4[i], qrow >= S || ki >= S || (CAUSAL && ki > qrow));
                    ds[e] = p[e] * (ds[e] - d4[i]) * a.scale;
                }
            }
            tile_accumulate<D>(dvt, Gs, PQ, 32 * blk, p, r, h);       // dV^T += dO^T P
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

template <int D>
static int stream_fwd_as(const AttnStreamFwdArgs& a, dim3 grid, bool causal) {
    const size_t bytes = size_t(attn_stream_fwd_lds_floats<D>()) * 4;
    return causal ? stream_launch(&attn_stream_fwd<D, true>, a, grid, bytes) : stream_launch(&attn_stream_fwd<D, false>, a, grid, bytes);
}

template <int D>
static int stream_bwd_as(const AttnStreamBwdArgs& a, dim3 grid, bool causal) {
    const size_t bytes = size_t(attn_stream_bwd_lds_floats<D>()) * 4;
    int rc = causal ? stream_launch(&attn_stream_bwd_q<D, true>, a, grid, bytes) : stream_launch(&attn_stream_bwd_q<D, false>, a, grid, bytes);
    if (rc != LG_OK) return rc;
    return causal ? stream_launch(&attn_stream_bwd_kv<D, true>, a, grid, bytes) : stream_launch(&attn_stream_bwd_kv<D, false>, a, grid, bytes);
}

static bool stream_operand(const void* p, int64_t ld, int64_t sb) { return p && aligned16(p) && ld % 4 == 0 && sb % 4 == 0; }

// the checks every stream entry starts with, in the order of attn_forward (attention.hip); 1: an empty batch, nothing to do
static int stream_check(const char* name, int64_t batch, int64_t heads, int64_t S, int64_t D) {
    LG_ARG(lg_attention_stream_supported(S, D), "%s: S = %lld (1..%lld), D = %lld (32 or 64) unsupported", name, (long long)S,
           (long long)kStreamMaxS, (long long)D);
    LG_ARG(batch >= 0 && heads >= 1 && batch <= 65535 && heads <= 65535, "%s: bad batch / heads", name);
    return batch == 0 ? 1 : LG_OK;
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
    const char* name = "lg_attention_stream_fwd_f32";
    { const int rc = stream_check(name, batch, heads, S, D); if (rc != LG_OK) return rc < 0 ? rc : LG_OK; }
    const int64_t w = heads * D;
    LG_ARG(stream_operand(q, ldq, sbq) && stream_operand(k, ldk, sbk) && stream_operand(v, ldv, sbv) && stream_operand(o, ldo, sbo) && lse,
           "%s: operands must be non-NULL and 16-byte aligned with pitches that are multiples of 4 (lse: non-NULL)", name);
    LG_ARG(ldq >= w && ldk >= w && ldv >= w && ldo >= w, "%s: row pitch below heads * D", name);
    LG_ARG(!mask || sbm == 0 || sbm >= S, "%s: mask batch pitch %lld is neither 0 (one row for the batch) nor >= S", name, (long long)sbm);
    const AttnStreamFwdArgs a{q, k, v, ldq, sbq, ldk, sbk, ldv, sbv, o, ldo, sbo, lse, mask, sbm, int(S), int(heads), scale};
    const dim3 grid(unsigned((S + kStreamChunk - 1) / kStreamChunk), unsigned(heads), unsigned(batch));
    const int rc = D == 64 ? stream_fwd_as<64>(a, grid, causal != 0) : stream_fwd_as<32>(a, grid, causal != 0);
    if (rc != LG_OK) return rc;
    LG_CHECK_LAUNCH();
    return LG_OK;
}

extern "C" int lg_attention_stream_bwd_f32(const float* q, int64_t ldq, int64_t sbq, const float* k, int64_t ldk, int64_t sbk,
                                           const float* v, int64_t ldv, int64_t sbv, const float* o, int64_t ldo, int64_t sbo,
                                           const float* g, int64_t ldg, int64_t sbg, const float* lse, float* delta,
                                           float* dq, int64_t lddq, int64_t sbdq, float* dk, int64_t lddk, int64_t sbdk,
                                           float* dv, int64_t lddv, int64_t sbdv, int64_t batch, int64_t heads, int64_t S, int64_t D,
                                           float scale, const float* mask, int64_t sbm, int causal) {
    LG_REQUIRE_INIT();
    const char* name = "lg_attention_stream_bwd_f32";
    { const int rc = stream_check(name, batch, heads, S, D); if (rc != LG_OK) return rc < 0 ? rc : LG_OK; }
    const int64_t w = heads * D;
    LG_ARG(stream_operand(q, ldq, sbq) && stream_operand(k, ldk, sbk) && stream_operand(v, ldv, sbv) && stream_operand(o, ldo, sbo) &&
               stream_operand(g, ldg, sbg) && stream_operand(dq, lddq, sbdq) && stream_operand(dk, lddk, sbdk) &&
               stream_operand(dv, lddv, sbdv) && lse && delta,
           "%s: operands must be non-NULL and 16-byte aligned with pitches that are multiples of 4 (lse, delta: non-NULL)", name);
    LG_ARG(ldq >= w && ldk >= w && ldv >= w && ldo >= w && ldg >= w && lddq >= w && lddk >= w && lddv >= w, "%s: row pitch below heads * D", name);
    LG_ARG(!mask || sbm == 0 || sbm >= S, "%s: mask batch pitch %lld is neither 0 (one row for the batch) nor >= S", name, (long long)sbm);
    const AttnStreamBwdArgs a{q, k, v, o, g, ldq, sbq, ldk, sbk, ldv, sbv, ldo, sbo, ldg, sbg, lse, delta, dq, dk, dv,
                              lddq, sbdq, lddk, sbdk, lddv, sbdv, mask, sbm, int(S), int(heads), scale};
    const dim3 grid(unsigned((S + kStreamChunk - 1) / kStreamChunk), unsigned(heads), unsigned(batch));
    const int rc = D == 64 ? stream_bwd_as<64>(a, grid, causal != 0) : stream_bwd_as<32>(a, grid, causal != 0);
    if (rc != LG_OK) return rc;
    LG_CHECK_LAUNCH();
    return LG_OK;
}
