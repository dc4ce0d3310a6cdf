// Attention of m NEW tokens against a filled key / value cache in one launch (gfx950, fp32 MFMA): lg_attention_extend_f32.
//
// Between the causal forward (the whole prompt, an empty cache: attention.hip / attention_long.hip) and the decode kernel (one
// token, a filled cache: decode.hip).  lg_attention_extend_rows_f32 is the same kernel with a position word per batch element
// (ExtendArgs::pos_pitch = 1 in place of 0): everything below holds per element with its own t.  With t = the word `pos` holds on the device, query row i sits at position t + i and
// sees keys 0 .. t + i: the cache's rows 0 .. t - 1, then rows 0 .. i of k_new / v_new - which this launch also writes to rows
// t .. t + m - 1 of the caches, and which it always takes from the new-token buffers, never back from the cache (other
// workgroups of the same launch write those rows).  m query rows against up to 512 keys is a matrix-matrix problem: the
// kernel is attn_long_fwd<D, false, CAUSAL = true> (attention_long.hip) with four differences.
//
//   partition   one workgroup of 256 threads (4 waves) per (block of 32 query rows, head, batch)
//   bound       the chunk loops end at Kend = round32(t + q0 + rows of the block): formed on the device from t; LDS is sized on
//               the host by round32(capacity), which Kend never exceeds (t + m <= capacity)
//   seam        key j of a streamed chunk comes from the cache (j < t), from k_new / v_new (t <= j < t + m) or is ZERO in LDS
//               (j >= t + m): the address is selected per float4, so the seam can fall anywhere inside a chunk; a row that does
//               not exist is never multiplied - cache rows >= t may hold NaN
//   diagonal    row i of the block sees the columns [0, t + q0 + i]: the softmax selects, nothing is multiplied by a mask
//   cache rows  the workgroup stores the 32 new K / V rows of its own block and head to rows t + q0 .. of the caches
//
// Everything else is the model's: Q rows of the block (pitch D + 4), the 32 x (Cp + 4) tile of scores / probabilities, ONE chunk
// buffer of 128 rows through which K (pitch D + 4), then V (pitch D + 8) stream with the next chunk's global loads issued ahead
// of the MFMAs, wave w on keys [32 w, 32 w + 32) of a chunk for the scores, the three-pass softmax with 8 threads per row,
// context tiles split over the waves with the partial sums in registers across the chunks and ONE fold through LDS in wave
// order: the same bits every run, and a (batch, head, block) triple's bits depend on its own data and t only.
// lg_attention_extend_counts_f32 is the per-element kernel once more with a word count[b] per batch element (ExtendArgs::count, NULL
// for the other two entries): of the m rows given, the first n = count[b] are tokens.  The element is computed as by a launch of
// its own with m = n (keys = t + n, Kend and the seam from n, cache rows t .. t + n - 1 written), only t + n must fit the capacity,
// rows >= n of the context and of p become +0.0, and a block that starts at q0 >= n returns after clearing its rows.
// lg_attention_extend_packed_f32 is the body once more for a token-packed step (attn_packed<D>): the tokens of ALL cache slots lie in
// flat (T, .) operands and `cu` (slots + 1 words) says whose they are - slot z owns rows cu[z] .. cu[z + 1] - 1 and is computed as by a
// `_rows` launch of its own at batch 1 on those rows, against cache rows, position and mask of slot z; one more slice of the grid
// clears the rows behind cu[slots], which belong to nobody.
// LDS at D = 64, capacity = 512: 32 * 68 + 32 * 516 + 128 * 72 + 3072 + 512 floats = 126 KB - one workgroup per CU.
#include "attention_common.h"

namespace lg {

constexpr int kExtChunk = 128;         // rows of a streamed operand in LDS at a time
constexpr int kExtMaxBlocks = 16;      // 32-column blocks of the longest row (512 / 32)
constexpr int kExtMaxKeys = 512;

struct ExtendArgs {
    const float *q, *k_new, *v_new;      // element (b, i, head, d) at x + b * sbX + i * ldX + head * D + d
    int64_t ldq, sbq, ldk, sbk, ldv, sbv;
    float *k_cache, *v_cache;            // element (b, j, head, d) at x + b * sbc + j * ldc + head * D + d
    int64_t ldc, sbc;
    const int32_t* pos;                  // batch element b reads pos[b * pos_pitch]: pitch 0 = one word for the batch, 1 = a word per row
    int64_t pos_pitch;
    const int32_t* count;                // NULL: each of the m rows is a new token; else batch element b has count[b] real ones (0 .. m)
    float* o;                            // context, addressed like q
    int64_t ldo, sbo;
    float* p;                            // NULL, or (batch, heads, m, capacity) dense
    int heads, capacity, m;
    float scale;
    const float* mask;                   // element (b, j) at mask + b * sbm + j; NULL = none
    int64_t sbm;
    int* status;
    const int32_t* cu;                   // NULL for the three (b, m) entries; lg_attention_extend_packed_f32: slots + 1 words, slot z owns rows cu[z] .. cu[z + 1] - 1
    int tokens;                          // ... of the `tokens` rows of the flat (tokens, .) operands: no batch pitch, p is (heads, tokens, capacity)
};

template <int D>
constexpr int attn_extend_lds_floats(int Cp) { return 32 * (D + 4) + 32 * (Cp + 4) + kExtChunk * (D + 8) + 3 * 1024 + Cp; }

// keys [c0, c0 + 128) of the stream: global -> registers.  Key j < t is the cache's row j, key j >= t row j - t of the new
// tokens (clamped to a row that exists: what a key >= t + m loads is dropped by seam_store); no branch, all loads in flight
template <int D, int N>
__device__ __forceinline__ void seam_load(af32x4 (&v)[N], const float* cache, int64_t ldc, const float* fresh, int64_t ldn, int c0, int t, int m) {
    constexpr int Q = D / 4;
#pragma unroll
    for (int i = 0; i < N; ++i) {
        const int f = threadIdx.x + i * 256, j = c0 + f / Q;
        const int jn = j - t < 0 ? 0 : (j - t < m ? j - t : m - 1);
        const float* src = j < t ? cache + int64_t(j) * ldc : fresh + int64_t(jn) * ldn;
        v[i] = *reinterpret_cast<const af32x4*>(src + (f % Q) * 4);
    }
}
// ... and registers -> LDS: keys [t + m, Kend) of the chunk ZERO
template <int D, int N>
__device__ __forceinline__ void seam_store(const af32x4 (&v)[N], float* dst, int pitch, int c0, int keys, int Kend) {
    const int left = keys - c0, rows = left < 0 ? 0 : (left < kExtChunk ? left : kExtChunk);
    const int padded = Kend - c0 < kExtChunk ? Kend - c0 : kExtChunk;
    store_rows_padded<D, N>(v, dst, pitch, rows, padded);
}

// the slice behind the last slot of a packed launch: token rows cu[slots] .. tokens - 1 belong to nobody and become +0.0 in the
// context and in p, so that what the launch returns is determined whatever the projection buffer holds there.  The (x, head)
// workgroups of the slice share the rows in runs of 32
template <int D>
__device__ __forceinline__ void packed_clear(const ExtendArgs& a, int slots) {
    constexpr int Q4 = D / 4;
    const int tid = threadIdx.x, head = blockIdx.y, C = a.capacity, T = a.tokens;
    const int used = a.cu[slots];
    if (used < 0 || used > T) {
        if (tid == 0) __hip_atomic_fetch_or(a.status, LG_STATUS_BAD_INDEX, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
        return;
    }
    const af32x4 zero{0.f, 0.f, 0.f, 0.f};
    for (int lo = used + 32 * int(blockIdx.x); lo < T; lo += 32 * int(gridDim.x)) {
        const int hi = lo + 32 < T ? lo + 32 : T;
        float* oz = a.o + head * D;
        for (int f = tid; f < (hi - lo) * Q4; f += 256) *reinterpret_cast<af32x4*>(oz + int64_t(lo + f / Q4) * a.ldo + (f % Q4) * 4) = zero;
        if (a.p != nullptr) {
            float* pz = a.p + (int64_t(head) * T + lo) * C;              // rows lo .. hi - 1 of p are one dense run of floats
            const int total = (hi - lo) * C;
            const int ahead = int((4 - ((reinterpret_cast<uintptr_t>(pz) >> 2) & 3)) & 3);
            const int lead = ahead < total ? ahead : total, quads = (total - lead) / 4;
            for (int f = tid; f < lead; f += 256) pz[f] = 0.f;
            for (int f = tid; f < quads; f += 256) *reinterpret_cast<af32x4*>(pz + lead + 4 * f) = zero;
            for (int f = lead + 4 * quads + tid; f < total; f += 256) pz[f] = 0.f;
        }
    }
}

// PACKED (attn_packed<D>, lg_attention_extend_packed_f32): blockIdx.z is a cache SLOT whose token rows are rows cu[z] .. cu[z + 1] - 1
// of flat (tokens, .) operands; the caches, the positions and the mask are addressed by the slot as by a batch element, and the
// first row of the slot's tokens is a scalar like t and count.  A flag of the template and not a branch on a kernel argument:
// attn_extend<D>, the kernel of the three (b, m) entries, keeps the code, the registers and the time it had (the branch at run
// time compiled to 4 VGPRs fewer and a launch 5 % slower: profiles/serve_packed.md)
template <int D, bool PACKED>
__device__ __forceinline__ void attn_extend_body(const ExtendArgs& a) {
    extern __shared__ __attribute__((aligned(16))) float lds[];
    const int m = a.m, C = a.capacity, Cp = round32(C), PP = Cp + 4;
    constexpr int PQ = D + 4, PV = D + 8, Q4 = D / 4;
    constexpr int NB = 32 * Q4 / 256, NA = kExtChunk * Q4 / 256;
    if constexpr (PACKED) {
        if (blockIdx.z + 1 == gridDim.z) { packed_clear<D>(a, int(gridDim.z) - 1); return; }
    }
    const int t = a.pos[int64_t(blockIdx.z) * a.pos_pitch];       // uniform over the workgroup either way: a scalar load
    const int tid = threadIdx.x;
    // the element's real new tokens: each of the launch's m rows, or - lg_attention_extend_counts_f32 - the first count[b] of them.
    // From here on the element is computed as by a launch of its own with m = real; `m` stays the pitch of `p` and the rows to clear
    // (packed: the slot's rows cu[z + 1] - cu[z], at most m = m_max of them; its first row is workgroup-uniform like t)
    int real, row0 = 0;
    bool bad;
    if constexpr (PACKED) {
        row0 = a.cu[blockIdx.z];
        const int64_t n = int64_t(a.cu[blockIdx.z + 1]) - row0;
        bad = row0 < 0 || n < 0 || n > m || n + row0 > a.tokens || t < 0 || t > C - n;
        real = int(n);
    } else {
        real = a.count ? a.count[blockIdx.z] : m;
        bad = t < 0 || real < 0 || real > m || t > C - real;
    }
    if (bad) {
        // a bounds check, never a fault: nothing is written for this batch element (the others of a per-row launch are computed
        // as usual), the next synchronising call reports LG_EINDEX
        if (tid == 0) __hip_atomic_fetch_or(a.status, LG_STATUS_BAD_INDEX, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
        return;
    }
    float* Qs = lds;                      // Q rows of the block                    32 x PQ
    float* Ps = Qs + 32 * PQ;             // scores, then probabilities             32 x PP
    float* Buf = Ps + 32 * PP;            // a chunk of K (pitch PQ), then of V (pitch PV)
    float* Red = Buf + kExtChunk * PV;
    float* Bias = Red + 3 * 1024;         // what key j adds to every score of its column
    const int lane = tid & 63, wave = tid >> 6, r = lane & 31, h = lane >> 5;
    const int q0 = blockIdx.x * 32, head = blockIdx.y, b = blockIdx.z;
    if constexpr (PACKED) {
        // a block without a row of the slot is done: uniform over the workgroup, before any load, MFMA or barrier
        if (q0 >= real) return;
    } else if (real < m) {
        // rows of the block that are given but hold no token: +0.0 in the context and in p, so that what the launch returns is
        // determined.  A block without a real row is done then: uniform over the workgroup, before any load, MFMA or barrier
        const int lo = q0 > real ? q0 : real, hi = q0 + 32 < m ? q0 + 32 : m;
        const af32x4 zero{0.f, 0.f, 0.f, 0.f};
        float* oz = a.o + int64_t(b) * a.sbo + head * D;
        for (int f = tid; f < (hi - lo) * Q4; f += 256) *reinterpret_cast<af32x4*>(oz + int64_t(lo + f / Q4) * a.ldo + (f % Q4) * 4) = zero;
        if (a.p != nullptr && hi > lo) {
            float* pz = a.p + ((int64_t(b) * a.heads + head) * m + lo) * C;       // rows lo .. hi - 1 of p are one dense run of floats
            const int total = (hi - lo) * C;
            const int ahead = int((4 - ((reinterpret_cast<uintptr_t>(pz) >> 2) & 3)) & 3);       // floats in front of the first aligned float4
            const int lead = ahead < total ? ahead : total, quads = (total - lead) / 4;
            for (int f = tid; f < lead; f += 256) pz[f] = 0.f;
            for (int f = tid; f < quads; f += 256) *reinterpret_cast<af32x4*>(pz + lead + 4 * f) = zero;
            for (int f = lead + 4 * quads + tid; f < total; f += 256) pz[f] = 0.f;
        }
        if (q0 >= real) return;
    }
    const int qrows = real - q0 < 32 ? real - q0 : 32;                // rows of this block that exist
    const int keys = t + real;                                        // keys that exist in this launch
    const int Kend = round32(t + q0 + qrows);                         // the key columns the chunk loops cover (<= Cp)
    const float* kc = a.k_cache + int64_t(b) * a.sbc + head * D;
    const float* vc = a.v_cache + int64_t(b) * a.sbc + head * D;
    // the element's token rows: a batch pitch, or - packed - the slot's first row of the flat operands
    const float* kn = a.k_new + (PACKED ? int64_t(row0) * a.ldk : int64_t(b) * a.sbk) + head * D;
    const float* vn = a.v_new + (PACKED ? int64_t(row0) * a.ldv : int64_t(b) * a.sbv) + head * D;
    const float* qn = a.q + (PACKED ? int64_t(row0) * a.ldq : int64_t(b) * a.sbq) + head * D;
    float* on = a.o + (PACKED ? int64_t(row0) * a.ldo : int64_t(b) * a.sbo) + head * D;
    // row 0 of the element in p: (batch, heads, m, capacity), or - packed - (heads, tokens, capacity)
    const int64_t prow = PACKED ? int64_t(head) * a.tokens + row0 : (int64_t(b) * a.heads + head) * m;

    af32x4 rc[NA];
    {
        af32x4 rq[NB], rk[NB], rv[NB];
        load_rows<D, NB>(rq, qn + int64_t(q0) * a.ldq, a.ldq, qrows);
        load_rows<D, NB>(rk, kn + int64_t(q0) * a.ldk, a.ldk, qrows);
        load_rows<D, NB>(rv, vn + int64_t(q0) * a.ldv, a.ldv, qrows);
        seam_load<D, NA>(rc, kc, a.ldc, kn, a.ldk, 0, t, real);
        store_rows_padded<D, NB>(rq, Qs, PQ, qrows, 32);
        // the block's own new rows become rows t + q0 .. of the caches, bit for bit; nothing in this launch reads them there
        float* kd = a.k_cache + int64_t(b) * a.sbc + int64_t(t + q0) * a.ldc + head * D;
        float* vd = a.v_cache + int64_t(b) * a.sbc + int64_t(t + q0) * a.ldc + head * D;
#pragma unroll
        for (int i = 0; i < NB; ++i) {
            const int f = tid + i * 256;
            if (f < qrows * Q4) {
                *reinterpret_cast<af32x4*>(kd + int64_t(f / Q4) * a.ldc + (f % Q4) * 4) = rk[i];
                *reinterpret_cast<af32x4*>(vd + int64_t(f / Q4) * a.ldc + (f % Q4) * 4) = rv[i];
            }
        }
        // (1.0 - mask) * -10000.0 in fp32, the composite's own arithmetic; -0.0f where the mask is 1 or absent or the key does
        // not exist: adding it changes no bit of a score
        for (int j = tid; j < Kend; j += 256) Bias[j] = (j < keys && a.mask) ? (1.0f - a.mask[int64_t(b) * a.sbm + j]) * -10000.0f : -0.0f;
    }

    // scores: the keys arrive in chunks of 128; wave w takes keys [c0 + 32 w, c0 + 32 w + 32) of the chunk, scaled (the product
    // rounded to fp32 first, like `scores * c`).  Columns [Kend, Cp) of the tile are never written and never read
    for (int c0 = 0; c0 < Kend; c0 += kExtChunk) {
        seam_store<D, NA>(rc, Buf, PQ, c0, keys, Kend);
        __syncthreads();
        if (c0 + kExtChunk < Kend) seam_load<D, NA>(rc, kc, a.ldc, kn, a.ldk, c0 + kExtChunk, t, real);
        else                       seam_load<D, NA>(rc, vc, a.ldc, vn, a.ldv, 0, t, real);      // the first chunk of V flies behind the softmax
        const int rows = Kend - c0 < kExtChunk ? Kend - c0 : kExtChunk;
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
    // exp(x - max) * (1 / sum) over the keys the row sees, [0, t + q0 + row]: a key beyond is no part of the max or the sum, its
    // column of the LDS tile becomes 0 (it is an MFMA operand of the context) and +0.0 is what `p` holds for it up to the capacity
    {
        const int row = tid >> 3, sub = tid & 7;
        const int vis = t + q0 + row + 1 < keys ? t + q0 + row + 1 : keys;       // key 0 is always one of them
        float* pr = Ps + row * PP;
        af32x4 x[kExtMaxBlocks];
        float mx = -INFINITY;
#pragma unroll
        for (int i = 0; i < kExtMaxBlocks; ++i) {
            const int c = sub * 4 + 32 * i;
            x[i] = af32x4{0.f, 0.f, 0.f, 0.f};
            if (c < Kend) {
                x[i] = *reinterpret_cast<const af32x4*>(pr + c);
#pragma unroll
                for (int e = 0; e < 4; ++e)
                    if (c + e < vis) mx = (x[i][e] > mx || x[i][e] != x[i][e]) ? x[i][e] : mx;
            }
        }
#pragma unroll
        for (int off = 1; off < 8; off <<= 1) { const float o = __shfl_xor(mx, off, 64); mx = (o > mx || o != o) ? o : mx; }
        float s = 0.f;
#pragma unroll
        for (int i = 0; i < kExtMaxBlocks; ++i) {
            const int c = sub * 4 + 32 * i;
            if (c < Kend) {
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    if (c + e < vis) { x[i][e] = expf(x[i][e] + (-mx)); s += x[i][e]; }
                    else x[i][e] = 0.f;
                }
            }
        }
#pragma unroll
        for (int off = 1; off < 8; off <<= 1) s += __shfl_xor(s, off, 64);
        const float inv = 1.0f / s;
        const bool stored = a.p != nullptr && row < qrows;
        float* pg = a.p + (prow + q0 + (row < qrows ? row : 0)) * C;
#pragma unroll
        for (int i = 0; i < kExtMaxBlocks; ++i) {
            const int c = sub * 4 + 32 * i;
            if (c < Cp) {
                if (c < Kend) {
#pragma unroll
                    for (int e = 0; e < 4; ++e) x[i][e] *= inv;
                    *reinterpret_cast<af32x4*>(pr + c) = x[i];
                }
                if (stored) {
                    if ((C & 3) == 0) {
                        if (c < C) *reinterpret_cast<af32x4*>(pg + c) = x[i];
                    } else {
#pragma unroll
                        for (int e = 0; e < 4; ++e)
                            if (c + e < C) pg[c + e] = x[i][e];
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
    for (int c0 = 0; c0 < Kend; c0 += kExtChunk) {
        seam_store<D, NA>(rc, Buf, PV, c0, keys, Kend);
        __syncthreads();                                              // (the first one also publishes the probabilities in LDS)
        if (c0 + kExtChunk < Kend) seam_load<D, NA>(rc, vc, a.ldc, vn, a.ldv, c0 + kExtChunk, t, real);
        const int rows = Kend - c0 < kExtChunk ? Kend - c0 : kExtChunk, kspan = rows / KP;
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
        float* og = on + int64_t(q0) * a.ldo + 32 * n + r;
#pragma unroll
        for (int e = 0; e < 16; ++e)
            if (acc_row(e, h) < qrows) og[int64_t(acc_row(e, h)) * a.ldo] = acc[e];
    }
}

template <int D>
__global__ void __launch_bounds__(256) attn_extend(const ExtendArgs a) { attn_extend_body<D, false>(a); }

template <int D>
__global__ void __launch_bounds__(256) attn_packed(const ExtendArgs a) { attn_extend_body<D, true>(a); }

static bool extend_operand(const void* p, int64_t ld, int64_t sb) { return p && aligned16(p) && ld >= 0 && sb >= 0 && ld % 4 == 0 && sb % 4 == 0; }

// do the floats [x, x + (batch - 1) sb + (rows - 1) ld + w) and [y, ...) share an address?
static bool extend_overlap(const float* x, int64_t ldx, int64_t sbx, int64_t rowsx, const float* y, int64_t ldy, int64_t sby, int64_t rowsy,
                           int64_t batch, int64_t w) {
    const float* xe = x + (batch - 1) * sbx + (rowsx - 1) * ldx + w;
    const float* ye = y + (batch - 1) * sby + (rowsy - 1) * ldy + w;
    return x < ye && y < xe;
}

// do the `words` position words share an address with the floats [c, c + (batch - 1) sbc + (capacity - 1) ldc + w) of a cache?
static bool positions_overlap(const int32_t* pos, int64_t words, const float* c, int64_t ldc, int64_t sbc, int64_t capacity, int64_t batch, int64_t w) {
    const char *x = reinterpret_cast<const char*>(pos), *xe = x + 4 * words;
    const char *y = reinterpret_cast<const char*>(c), *ye = reinterpret_cast<const char*>(c + (batch - 1) * sbc + (capacity - 1) * ldc + w);
    return x < ye && y < xe;
}

template <int D>
static int launch_extend(const ExtendArgs& a, dim3 grid) {
    const size_t bytes = size_t(attn_extend_lds_floats<D>(round32(a.capacity))) * 4;
    int rc = allow_lds(&attn_extend<D>, bytes);
    if (rc != LG_OK) return rc;
    hipLaunchKernelGGL(attn_extend<D>, grid, dim3(256), bytes, rt().stream, a);
    return LG_OK;
}

template <int D>
static int launch_packed(const ExtendArgs& a, dim3 grid) {
    const size_t bytes = size_t(attn_extend_lds_floats<D>(round32(a.capacity))) * 4;
    int rc = allow_lds(&attn_packed<D>, bytes);
    if (rc != LG_OK) return rc;
    hipLaunchKernelGGL(attn_packed<D>, grid, dim3(256), bytes, rt().stream, a);
    return LG_OK;
}

}  // namespace lg

using namespace lg;

extern "C" int lg_attention_extend_supported(int64_t m, int64_t capacity, int64_t D) {
    return (D == 32 || D == 64) && m >= 1 && m <= capacity && capacity <= kExtMaxKeys;
}

// every entry: `pos_pitch` words between the positions of neighbouring batch elements (0: one word for the batch); `counts`: the
// entry takes a word per batch element in `count` (NULL for the others)
static int extend_entry(const char* name, int64_t pos_pitch, bool counts, const int32_t* count, const float* q, int64_t ldq, int64_t sbq, const float* k_new, int64_t ldk, int64_t sbk,
                        const float* v_new, int64_t ldv, int64_t sbv, float* k_cache, float* v_cache, int64_t ldc, int64_t sbc,
                        const int32_t* pos, float* o, int64_t ldo, int64_t sbo, float* p, int64_t batch, int64_t heads, int64_t m,
                        int64_t capacity, int64_t D, float scale, const float* mask, int64_t sbm) {
    LG_ARG(lg_attention_extend_supported(m, capacity, D), "%s: m = %lld (1 .. capacity), capacity = %lld (1 .. 512), D = %lld (32 or 64) unsupported",
           name, (long long)m, (long long)capacity, (long long)D);
    LG_ARG(batch >= 0 && heads >= 1 && batch <= 65535 && heads <= 65535, "%s: bad batch / heads", name);
    if (batch == 0) return LG_OK;
    LG_ARG(extend_operand(q, ldq, sbq) && extend_operand(k_new, ldk, sbk) && extend_operand(v_new, ldv, sbv) && extend_operand(k_cache, ldc, sbc) &&
               extend_operand(v_cache, ldc, sbc) && extend_operand(o, ldo, sbo) && pos && (reinterpret_cast<uintptr_t>(pos) & 3u) == 0 && aligned16(p),
           "%s: operands must be non-NULL and 16-byte aligned with pitches that are non-negative multiples of 4", name);
    const int64_t w = heads * D;
    LG_ARG(ldc >= w, "%s: cache row pitch %lld below heads * D = %lld", name, (long long)ldc, (long long)w);
    LG_ARG(!mask || sbm == 0 || sbm >= capacity, "%s: mask batch pitch %lld is neither 0 (one row for the batch) nor >= capacity", name,
           (long long)sbm);
    LG_ARG(!extend_overlap(k_new, ldk, sbk, m, k_cache, ldc, sbc, capacity, batch, w) && !extend_overlap(k_new, ldk, sbk, m, v_cache, ldc, sbc, capacity, batch, w) &&
               !extend_overlap(v_new, ldv, sbv, m, k_cache, ldc, sbc, capacity, batch, w) && !extend_overlap(v_new, ldv, sbv, m, v_cache, ldc, sbc, capacity, batch, w),
           "%s: k_new / v_new overlap a cache: the launch writes the caches while other workgroups read the new rows", name);
    LG_ARG(!positions_overlap(pos, pos_pitch ? batch : 1, k_cache, ldc, sbc, capacity, batch, w) &&
               !positions_overlap(pos, pos_pitch ? batch : 1, v_cache, ldc, sbc, capacity, batch, w),
           "%s: pos overlaps a cache: the launch writes the caches while other workgroups read their positions", name);
    if (counts) {
        LG_ARG(count && (reinterpret_cast<uintptr_t>(count) & 3u) == 0, "%s: count must be non-NULL and 4-byte aligned", name);
        LG_ARG(!positions_overlap(count, batch, k_cache, ldc, sbc, capacity, batch, w) && !positions_overlap(count, batch, v_cache, ldc, sbc, capacity, batch, w),
               "%s: count overlaps a cache: the launch writes the caches while other workgroups read their counts", name);
        LG_ARG(!(count < pos + (pos_pitch ? batch : 1) && pos < count + batch), "%s: count overlaps pos", name);
    }
    {
        const int64_t rows[3] = {batch, m, w}, row_strides[3] = {sbo, ldo, 1};
        int rc = adam_epilogue_check_strided(o, 4, 3, rows, row_strides);
        if (rc != LG_OK) return rc;
        const int64_t crows[3] = {batch, capacity, w}, strides[3] = {sbc, ldc, 1};
        rc = adam_epilogue_check_strided(k_cache, 4, 3, crows, strides);
        if (rc != LG_OK) return rc;
        rc = adam_epilogue_check_strided(v_cache, 4, 3, crows, strides);
        if (rc != LG_OK) return rc;
        if (p) { rc = adam_epilogue_check_write(p, batch * heads * m * capacity * 4); if (rc != LG_OK) return rc; }
    }
    const ExtendArgs a{q, k_new, v_new, ldq, sbq, ldk, sbk, ldv, sbv, k_cache, v_cache, ldc, sbc, pos, pos_pitch, counts ? count : nullptr, o, ldo, sbo, p,
                       int(heads), int(capacity), int(m), scale, mask, sbm, rt().status_dev, nullptr, 0};
    const dim3 grid{unsigned((m + 31) / 32), unsigned(heads), unsigned(batch)};
    const int rc = D == 64 ? launch_extend<64>(a, grid) : launch_extend<32>(a, grid);
    return rc;
}

extern "C" int lg_attention_extend_f32(const float* q, int64_t ldq, int64_t sbq, const float* k_new, int64_t ldk, int64_t sbk,
                                       const float* v_new, int64_t ldv, int64_t sbv, float* k_cache, float* v_cache, int64_t ldc,
                                       int64_t sbc, const int32_t* pos, float* o, int64_t ldo, int64_t sbo, float* p, int64_t batch,
                                       int64_t heads, int64_t m, int64_t capacity, int64_t D, float scale, const float* mask, int64_t sbm) {
    LG_REQUIRE_INIT();
    const int rc = extend_entry("lg_attention_extend_f32", 0, false, nullptr, q, ldq, sbq, k_new, ldk, sbk, v_new, ldv, sbv, k_cache, v_cache, ldc, sbc, pos, o, ldo, sbo,
                        p, batch, heads, m, capacity, D, scale, mask, sbm);
    if (rc != LG_OK || batch == 0) return rc;
    LG_CHECK_LAUNCH();
    return LG_OK;
}

// the same launch with a position per batch element: pos holds `batch` contiguous words, element b uses t = pos[b]
extern "C" int lg_attention_extend_rows_f32(const float* q, int64_t ldq, int64_t sbq, const float* k_new, int64_t ldk, int64_t sbk,
                                            const float* v_new, int64_t ldv, int64_t sbv, float* k_cache, float* v_cache, int64_t ldc,
                                            int64_t sbc, const int32_t* pos, float* o, int64_t ldo, int64_t sbo, float* p, int64_t batch,
                                            int64_t heads, int64_t m, int64_t capacity, int64_t D, float scale, const float* mask, int64_t sbm) {
    LG_REQUIRE_INIT();
    const int rc = extend_entry("lg_attention_extend_rows_f32", 1, false, nullptr, q, ldq, sbq, k_new, ldk, sbk, v_new, ldv, sbv, k_cache, v_cache, ldc, sbc, pos, o, ldo,
                        sbo, p, batch, heads, m, capacity, D, scale, mask, sbm);
    if (rc != LG_OK || batch == 0) return rc;
    LG_CHECK_LAUNCH();
    return LG_OK;
}

// the `_rows` entry with a token count per batch element: count holds `batch` contiguous words, element b has n = count[b] real new
// tokens among the m rows it is given and is computed as by the `_rows` entry on it alone with m = n; rows >= n of o and p are +0.0
extern "C" int lg_attention_extend_counts_f32(const float* q, int64_t ldq, int64_t sbq, const float* k_new, int64_t ldk, int64_t sbk,
                                              const float* v_new, int64_t ldv, int64_t sbv, float* k_cache, float* v_cache, int64_t ldc,
                                              int64_t sbc, const int32_t* pos, const int32_t* count, float* o, int64_t ldo, int64_t sbo, float* p,
                                              int64_t batch, int64_t heads, int64_t m, int64_t capacity, int64_t D, float scale, const float* mask,
                                              int64_t sbm) {
    LG_REQUIRE_INIT();
    const int rc = extend_entry("lg_attention_extend_counts_f32", 1, true, count, q, ldq, sbq, k_new, ldk, sbk, v_new, ldv, sbv, k_cache, v_cache, ldc, sbc,
                                pos, o, ldo, sbo, p, batch, heads, m, capacity, D, scale, mask, sbm);
    if (rc != LG_OK || batch == 0) return rc;
    LG_CHECK_LAUNCH();
    return LG_OK;
}

// do the `words` int32 words at x share an address with the `bytes` bytes at y?
static bool words_overlap(const int32_t* x, int64_t words, const void* y, int64_t bytes) {
    const char *a = reinterpret_cast<const char*>(x), *ae = a + 4 * words, *b = static_cast<const char*>(y);
    return y != nullptr && a < b + bytes && b < ae;
}

// the token-packed launch: the step's tokens of ALL slots in flat (T, .) operands, slot z owning rows cu[z] .. cu[z + 1] - 1 (at
// most m_max of them) behind its own position pos[z] of its own cache rows.  The `_rows` kernel per slot, with the slot's first
// row in place of a batch pitch; one more slice of the grid clears the rows behind cu[slots]
extern "C" int lg_attention_extend_packed_f32(const float* q, int64_t ldq, const float* k_new, int64_t ldk, const float* v_new, int64_t ldv,
                                              float* k_cache, float* v_cache, int64_t ldc, int64_t sbc, const int32_t* pos, const int32_t* cu,
                                              float* o, int64_t ldo, float* p, int64_t slots, int64_t heads, int64_t T, int64_t m_max,
                                              int64_t capacity, int64_t D, float scale, const float* mask, int64_t sbm) {
    LG_REQUIRE_INIT();
    const char* name = "lg_attention_extend_packed_f32";
    LG_ARG(lg_attention_extend_supported(m_max, capacity, D), "%s: m_max = %lld (1 .. capacity), capacity = %lld (1 .. 512), D = %lld (32 or 64) unsupported",
           name, (long long)m_max, (long long)capacity, (long long)D);
    LG_ARG(T >= 1 && T < (int64_t(1) << 30), "%s: T = %lld token rows (1 .. 2^30 - 1) unsupported", name, (long long)T);
    LG_ARG(slots >= 0 && heads >= 1 && slots <= 65534 && heads <= 65535, "%s: bad slots / heads", name);
    if (slots == 0) return LG_OK;
    LG_ARG(extend_operand(q, ldq, 0) && extend_operand(k_new, ldk, 0) && extend_operand(v_new, ldv, 0) && extend_operand(k_cache, ldc, sbc) &&
               extend_operand(v_cache, ldc, sbc) && extend_operand(o, ldo, 0) && pos && (reinterpret_cast<uintptr_t>(pos) & 3u) == 0 && aligned16(p),
           "%s: operands must be non-NULL and 16-byte aligned with pitches that are non-negative multiples of 4", name);
    const int64_t w = heads * D;
    LG_ARG(ldc >= w, "%s: cache row pitch %lld below heads * D = %lld", name, (long long)ldc, (long long)w);
    LG_ARG(!mask || sbm == 0 || sbm >= capacity, "%s: mask slot pitch %lld is neither 0 (one row for every slot) nor >= capacity", name, (long long)sbm);
    // (extend_overlap spans `slots` elements of both operands: the flat ones have no batch pitch)
    LG_ARG(!extend_overlap(k_new, ldk, 0, T, k_cache, ldc, sbc, capacity, slots, w) && !extend_overlap(k_new, ldk, 0, T, v_cache, ldc, sbc, capacity, slots, w) &&
               !extend_overlap(v_new, ldv, 0, T, k_cache, ldc, sbc, capacity, slots, w) && !extend_overlap(v_new, ldv, 0, T, v_cache, ldc, sbc, capacity, slots, w),
           "%s: k_new / v_new overlap a cache: the launch writes the caches while other workgroups read the new rows", name);
    LG_ARG(!positions_overlap(pos, slots, k_cache, ldc, sbc, capacity, slots, w) && !positions_overlap(pos, slots, v_cache, ldc, sbc, capacity, slots, w),
           "%s: pos overlaps a cache: the launch writes the caches while other workgroups read their positions", name);
    LG_ARG(cu && (reinterpret_cast<uintptr_t>(cu) & 3u) == 0, "%s: cu must be non-NULL and 4-byte aligned", name);
    LG_ARG(!positions_overlap(cu, slots + 1, k_cache, ldc, sbc, capacity, slots, w) && !positions_overlap(cu, slots + 1, v_cache, ldc, sbc, capacity, slots, w),
           "%s: cu overlaps a cache: the launch writes the caches while other workgroups read their rows' bounds", name);
    LG_ARG(!(cu < pos + slots && pos < cu + slots + 1), "%s: cu overlaps pos", name);
    {
        const int64_t span[4] = {((T - 1) * ldq + w) * 4, ((T - 1) * ldk + w) * 4, ((T - 1) * ldv + w) * 4, ((T - 1) * ldo + w) * 4};
        LG_ARG(!words_overlap(cu, slots + 1, q, span[0]) && !words_overlap(cu, slots + 1, k_new, span[1]) && !words_overlap(cu, slots + 1, v_new, span[2]) &&
                   !words_overlap(cu, slots + 1, o, span[3]) && !words_overlap(cu, slots + 1, p, heads * T * capacity * 4),
               "%s: cu overlaps an operand (q, k_new, v_new, o or p)", name);
    }
    {
        const int64_t rows[2] = {T, w}, row_strides[2] = {ldo, 1};
        int rc = adam_epilogue_check_strided(o, 4, 2, rows, row_strides);
        if (rc != LG_OK) return rc;
        const int64_t crows[3] = {slots, capacity, w}, strides[3] = {sbc, ldc, 1};
        rc = adam_epilogue_check_strided(k_cache, 4, 3, crows, strides);
        if (rc != LG_OK) return rc;
        rc = adam_epilogue_check_strided(v_cache, 4, 3, crows, strides);
        if (rc != LG_OK) return rc;
        if (p) { rc = adam_epilogue_check_write(p, heads * T * capacity * 4); if (rc != LG_OK) return rc; }
    }
    const ExtendArgs a{q, k_new, v_new, ldq, 0, ldk, 0, ldv, 0, k_cache, v_cache, ldc, sbc, pos, 1, nullptr, o, ldo, 0, p,
                       int(heads), int(capacity), int(m_max), scale, mask, sbm, rt().status_dev, cu, int(T)};
    const dim3 grid{unsigned((m_max + 31) / 32), unsigned(heads), unsigned(slots + 1)};
    const int rc = D == 64 ? launch_packed<64>(a, grid) : launch_packed<32>(a, grid);
    if (rc != LG_OK) return rc;
    LG_CHECK_LAUNCH();
    return LG_OK;
}
