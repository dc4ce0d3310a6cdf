// The kernel body of the split-key extend launches, attn_extend_split_body<D, PAGED, KV16>, and the one launch of its kernels
// (ext_split_launch): included by extend_split.hip (the three contiguous entries, PAGED = false: the text they had) and by
// paged_split.hip (lg_attention_extend_paged_split_f32 and, KV16 = true, lg_attention_extend_paged_split_bf16_f32: the caches
// are pools reached through a block table).  What the kernel does is the comment of extend_split.hip; what PAGED adds stands
// above the body.  The host checks of the entries are cache_entry.h's
#pragma once
#include "extend_body.h"
#include "handoff.h"
#include "stream_tiles.h"

namespace lg {

constexpr int kExtSplitMaxKeys = 16384;          // the range of lg_attention_stream_supported
constexpr int kExtSplitMaxRows = 128;            // m of one launch: four query blocks, which bounds the workspace
constexpr int kExtSplitMinSlice = 256;           // 64 slices at the most: what the merge's LDS rows are sized for
constexpr int kExtSplitMaxSlice = 1024;
constexpr int kExtSplitSlice = 256;              // L, chosen by profiles/extend_split.md
constexpr int kSplitTabWords = kExtSplitMaxSlice / 4;       // PAGED: the table words of one slice, blocks of 4 rows at the least
constexpr int kSplitScanWords = kExtSplitMaxKeys / 4;       // ... and of a whole row of the table: 16 a thread

struct ExtSplitArgs {
    const float *q, *k_new, *v_new;      // element (b, i, head, d) at x + b * sbX + i * ldX + head * D + d
    int64_t ldq, sbq, ldk, sbk, ldv, sbv;
    float *k_cache, *v_cache;            // element (b, j, head, d) at x + b * sbc + j * ldc + head * D + d
    int64_t ldc, sbc;
    const int32_t* pos;                  // batch element b reads pos[b * pos_pitch]
    int64_t pos_pitch;
    const int32_t* count;                // NULL: each of the m rows is a new token
    float* o;
    int64_t ldo, sbo;
    float* lse;                          // NULL, or (batch, heads, m) dense
    int heads, capacity, m, L, slices, blocks;
    float scale;
    const float* mask;                   // element (b, j) at mask + b * sbm + j; NULL = none
    int64_t sbm;
    float* ws;                           // slot (b, head, block, slice): 32 * (D + 2) floats {O[32][D], m[32], l[32]}; NULL when slices == 1
    int* tickets;                        // one per (b, head, block), tstride ints apart
    int tstride;
    int* status;
    // the paged entries (NULL / 0 for the contiguous ones): the caches are POOLS of num_blocks blocks of 1 << log2_block rows (row r at
    // x + r * ldc, no batch pitch), position j of element b is row block_table[b * max_blocks + (j >> log2_block)] << log2_block |
    // (j & ((1 << log2_block) - 1)), capacity = max_blocks << log2_block; KV16: the pools hold bfloat16 words, ldc counts them
    const int32_t* block_table;
    int max_blocks, num_blocks, log2_block;
};

template <int D> constexpr int attn_extend_split_lds_floats() { return kExtChunk * (D + 4) + kExtChunk * (D + 8) + kExtChunk; }
// the paged kernels keep the table words of their slice behind it
template <int D> constexpr int attn_paged_split_lds_floats() { return attn_extend_split_lds_floats<D>() + kSplitTabWords; }

// exp(x - m) with m = -inf read as 0: x = -inf gives +0, and -inf - -inf is never formed
__device__ __forceinline__ float exp_below(float x, float m) { return expf(x - (m == -INFINITY ? 0.f : m)); }

// seam_load_paged / seam_load_paged16 (extend_body.h) for a slice: `tab` holds the words of keys [j_lo, j_lo + L) only, word
// (j - j_lo) >> lb that of key j - each of them checked, the words behind the element's reach 0 -, and every key of a chunk of the
// slice lies in that range.  A key j >= t takes the new-token buffer (fp32) or has its pool words dropped by seam_settle16 (KV16):
// what its word names is a row inside the pool either way
template <int D, int N>
__device__ __forceinline__ void seam_load_slice(af32x4 (&v)[N], const float* pool, int64_t ldc, const int* tab, int lb, int j_lo, const float* fresh,
                                                int64_t ldn, int c0, int t, int m) {
    constexpr int Q = D / 4;
#pragma unroll
    for (int i = 0; i < N; ++i) {
        const int f = threadIdx.x + i * 256, j = c0 + f / Q;
        const int jn = j - t < 0 ? 0 : (j - t < m ? j - t : m - 1);
        const int row = (tab[((j - j_lo) >> lb) & (kSplitTabWords - 1)] << lb) | (j & ((1 << lb) - 1));
        const float* src = j < t ? pool + int64_t(row) * ldc : fresh + int64_t(jn) * ldn;
        v[i] = *reinterpret_cast<const af32x4*>(src + (f % Q) * 4);
    }
}
template <int D, int N>
__device__ __forceinline__ void seam_load_slice16(af32x4 (&v)[N], au32x2 (&w)[N], const uint16_t* pool, int64_t ldc, const int* tab, int lb, int j_lo,
                                                  const float* fresh, int64_t ldn, int c0, int t, int m) {
    constexpr int Q = D / 4;
#pragma unroll
    for (int i = 0; i < N; ++i) {
        const int f = threadIdx.x + i * 256, j = c0 + f / Q;
        const int jn = j - t < 0 ? 0 : (j - t < m ? j - t : m - 1);
        const int row = (tab[((j - j_lo) >> lb) & (kSplitTabWords - 1)] << lb) | (j & ((1 << lb) - 1));
        w[i] = *reinterpret_cast<const au32x2*>(pool + int64_t(row) * ldc + (f % Q) * 4);
        v[i] = *reinterpret_cast<const af32x4*>(fresh + int64_t(jn) * ldn + (f % Q) * 4);
    }
}

// PAGED (attn_paged_split<D>, paged_split.hip): the counts form with the caches reached through a block table of up to 4096 words.
//   verdict   different slices see different parts of the table, and an element with a bad word writes NOTHING - so every
//             workgroup that would write or arrive reaches the verdict on its own: it scans words 0 .. ceil((t + n) / B) - 1 of its
//             row with coalesced loads (at most 16 a thread) and votes across the workgroup, before its first store and before
//             it touches a ticket.  All of them leave then; slice 0 of block 0 of head 0 - which always gets here - raises the flag
//   table     only the L >> lb words of the slice's own keys are staged in LDS, checked once more on their way, the words behind
//             the reach 0: LDS does not depend on the capacity, and no address is formed from an unchecked word
//   rows      key j < t is pool row tab << lb | (j & (B - 1)); the slice that owns position t + q0 + i stores new row i through
//             the same words.  Nothing below t is written
// KV16 (attn_paged_split_bf16<D>): pools of bfloat16 words by the rule of paged_bf16.hip - 8-byte pool loads, widened in registers
// (seam_settle16), the launch's own keys attended to as r(.) of them and stored as that word.  Tiles, MFMAs, softmax, folds: fp32
template <int D, bool PAGED, bool KV16>
__device__ __forceinline__ void attn_extend_split_body(const ExtSplitArgs& a) {
    static_assert(PAGED || !KV16, "the bfloat16 pools are a form of the paged launch");
    using CacheT = std::conditional_t<KV16, uint16_t, float>;
    extern __shared__ __attribute__((aligned(16))) float lds[];
    __shared__ int s_last;
    constexpr int PK = D + 4, PV = D + 8, Q4 = D / 4, NA = kExtChunk * Q4 / 256, NB = 32 * Q4 / 256, NT = D / 32, SW = 32 * (D + 2);
    float* Ks = lds;                      // a chunk of K, K-contiguous A of S^T            128 x PK
    float* Vs = Ks + kExtChunk * PK;      // the same chunk of V, d along the lanes          128 x PV
    float* Bias = Vs + kExtChunk * PV;    // the bias of the chunk's keys                    128
    [[maybe_unused]] int* Tab = reinterpret_cast<int*>(Bias + kExtChunk);       // PAGED: the table words of the slice's keys
    [[maybe_unused]] const int lb = a.log2_block;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, r = lane & 31, h = lane >> 5;
    const int slice = blockIdx.x, qb = blockIdx.y / a.heads, head = blockIdx.y % a.heads, b = blockIdx.z;
    const int m = a.m, L = a.L;
    const int t = a.pos[int64_t(b) * a.pos_pitch];                    // uniform over the workgroup: scalar loads
    const int n = a.count ? a.count[b] : m;
    if (t < 0 || n < 0 || n > m || t > a.capacity - n) {
        // a bounds check, never a fault: nothing is written for this batch element, the others are computed as usual
        if (slice == 0 && blockIdx.y == 0 && tid == 0) __hip_atomic_fetch_or(a.status, LG_STATUS_BAD_INDEX, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
        return;
    }
    const int q0 = 32 * qb;
    if constexpr (PAGED) {
        const int rows = n - q0 < 32 ? n - q0 : 32;
        const bool clears = n < m && slice == 0, works = q0 < n && slice * L < t + q0 + rows;
        if (!clears && !works) return;                                // beyond the block's reach: before any other load
        const int words = (t + n + (1 << lb) - 1) >> lb;              // <= max_blocks, since t + n <= capacity
        const int32_t* const row = a.block_table + int64_t(b) * a.max_blocks;
        int wrong = 0;
#pragma unroll
        for (int i = 0; i < kSplitScanWords / 256; ++i) {
            if (256 * i >= words) break;                              // uniform over the workgroup
            const int w = tid + 256 * i;
            if (w < words) { const int e = row[w]; wrong |= e < 0 || e >= a.num_blocks; }
        }
        if (tid < kSplitTabWords) {
            const int w = ((slice * L) >> lb) + tid;
            int e = 0;
            if (works && tid < (L >> lb) && w < words) {
                e = row[w];
                if (e < 0 || e >= a.num_blocks) { wrong = 1; e = 0; }
            }
            Tab[tid] = e;
        }
        if (__syncthreads_or(wrong)) {
            // a bad word makes the element bad like a bad position: every workgroup of it leaves here, none has stored or arrived
            if (slice == 0 && blockIdx.y == 0 && tid == 0) __hip_atomic_fetch_or(a.status, LG_STATUS_BAD_INDEX, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
            return;
        }
    }
    float* const on = a.o + int64_t(b) * a.sbo + head * D;
    float* const ln = a.lse ? a.lse + (int64_t(b) * a.heads + head) * m : nullptr;
    if (n < m && slice == 0) {
        // rows of the block that are given but hold no token: +0.0, so that what the launch returns is determined
        const int lo = q0 > n ? q0 : n, hi = q0 + 32 < m ? q0 + 32 : m;
        for (int f = tid; f < (hi - lo) * Q4; f += 256)
            *reinterpret_cast<af32x4*>(on + int64_t(lo + f / Q4) * a.ldo + (f % Q4) * 4) = af32x4{0.f, 0.f, 0.f, 0.f};
        if (ln && lo + tid < hi) ln[lo + tid] = 0.f;
    }
    if (q0 >= n) return;
    const int qrows = n - q0 < 32 ? n - q0 : 32;                      // rows of this block that exist
    const int keys = t + n, reach = t + q0 + qrows;                   // keys that exist in this launch; keys this block sees
    const int j_lo = slice * L;
    if (j_lo >= reach) return;                                        // no key of this slice is visible: before any load, without a ticket
    const int live = (reach + L - 1) / L;
    const int j_hi = j_lo + L < reach ? j_lo + L : reach, Kend = round32(j_hi);

    const CacheT* kc = reinterpret_cast<const CacheT*>(a.k_cache) + (PAGED ? 0 : int64_t(b) * a.sbc) + head * D;
    const CacheT* vc = reinterpret_cast<const CacheT*>(a.v_cache) + (PAGED ? 0 : int64_t(b) * a.sbc) + head * D;
    [[maybe_unused]] au32x2 wk[KV16 ? NA : 1], wv[KV16 ? NA : 1];     // KV16: the pool side of the streamed chunk, 4 bfloat16 words a lane
    // the streamed keys / values of a chunk: the contiguous rows of the element, or the pool through the slice's words
    auto stream = [&](af32x4 (&v)[NA], au32x2 (&w)[KV16 ? NA : 1], const CacheT* cache, const float* fresh, int64_t ldn, int c0) {
        if constexpr (KV16)       seam_load_slice16<D, NA>(v, w, cache, a.ldc, Tab, lb, j_lo, fresh, ldn, c0, t, n);
        else if constexpr (PAGED) seam_load_slice<D, NA>(v, cache, a.ldc, Tab, lb, j_lo, fresh, ldn, c0, t, n);
        else                      seam_load<D, NA>(v, cache, a.ldc, fresh, ldn, c0, t, n);
    };
    const float* kn = a.k_new + int64_t(b) * a.sbk + head * D;
    const float* vn = a.v_new + int64_t(b) * a.sbv + head * D;
    const float* mrow = a.mask ? a.mask + int64_t(b) * a.sbm : nullptr;
    // what key j adds to every score of its column: (1.0 - mask) * -10000.0 in fp32, the composite's own arithmetic; -0.0f where
    // there is no mask or no key
    auto key_bias = [&](int j) { return (mrow && j < keys) ? (1.0f - mrow[j]) * -10000.0f : -0.0f; };

    af32x4 rk[NA], rv[NA];
    float rb = -0.0f;
    stream(rk, wk, kc, kn, a.ldk, j_lo);
    stream(rv, wv, vc, vn, a.ldv, j_lo);
    if (tid < kExtChunk) rb = key_bias(j_lo + tid);
    float qf[D / 2];
    frag_load<D>(qf, r < qrows ? a.q + int64_t(b) * a.sbq + int64_t(q0 + r) * a.ldq + head * D : nullptr, h);

    // the block's new rows whose positions this slice owns become rows of the caches, bit for bit; nothing in this launch reads
    // them there
#pragma unroll
    for (int i = 0; i < NB; ++i) {
        const int f = tid + i * 256, row = f / Q4, at = t + q0 + row;
        if (row < qrows && at >= j_lo && at < j_lo + L) {
            const af32x4 xk = *reinterpret_cast<const af32x4*>(kn + int64_t(q0 + row) * a.ldk + (f % Q4) * 4);
            const af32x4 xv = *reinterpret_cast<const af32x4*>(vn + int64_t(q0 + row) * a.ldv + (f % Q4) * 4);
            if constexpr (PAGED) {
                // ... of the pool: the word of position `at` is one of the slice's, inside the element's reach and checked
                const int64_t dst = int64_t((Tab[(at - j_lo) >> lb] << lb) | (at & ((1 << lb) - 1))) * a.ldc + head * D + (f % Q4) * 4;
                if constexpr (KV16) {
                    // each value as the word r leaves of it, one 8-byte store per lane and pool
                    *reinterpret_cast<au32x2*>(reinterpret_cast<uint16_t*>(a.k_cache) + dst) =
                        au32x2{bf16_word(xk[0]) | (bf16_word(xk[1]) << 16), bf16_word(xk[2]) | (bf16_word(xk[3]) << 16)};
                    *reinterpret_cast<au32x2*>(reinterpret_cast<uint16_t*>(a.v_cache) + dst) =
                        au32x2{bf16_word(xv[0]) | (bf16_word(xv[1]) << 16), bf16_word(xv[2]) | (bf16_word(xv[3]) << 16)};
                } else {
                    *reinterpret_cast<af32x4*>(a.k_cache + dst) = xk;
                    *reinterpret_cast<af32x4*>(a.v_cache + dst) = xv;
                }
            } else {
                const int64_t dst = int64_t(b) * a.sbc + int64_t(at) * a.ldc + head * D + (f % Q4) * 4;
                *reinterpret_cast<af32x4*>(a.k_cache + dst) = xk;
                *reinterpret_cast<af32x4*>(a.v_cache + dst) = xv;
            }
        }
    }

    // ---- the slice: wave w on the 32-key block w of every chunk, an online softmax per query ----------------------------------------
    float mx = -INFINITY, l = 0.f;
    af32x16 ot[NT];
#pragma unroll
    for (int nn = 0; nn < NT; ++nn) ot[nn] = zero16();
    const int last_key = t + q0 + r;                                  // the last key this lane's query sees
    for (int c0 = j_lo; c0 < j_hi; c0 += kExtChunk) {
        if constexpr (KV16) {
            seam_settle16<D, NA>(rk, wk, c0, t, keys);
            seam_settle16<D, NA>(rv, wv, c0, t, keys);
        }
        seam_store<D, NA>(rk, Ks, PK, c0, keys, Kend);
        seam_store<D, NA>(rv, Vs, PV, c0, keys, Kend);
        if (tid < kExtChunk) Bias[tid] = rb;
        __syncthreads();
        if (c0 + kExtChunk < j_hi) {
            stream(rk, wk, kc, kn, a.ldk, c0 + kExtChunk);
            stream(rv, wv, vc, vn, a.ldv, c0 + kExtChunk);
            if (tid < kExtChunk) rb = key_bias(c0 + kExtChunk + tid);
        }
        const int kb = c0 + 32 * wave;
        if (kb < j_hi) {                                              // wave-uniform; key kb is visible to the block's last row
            af32x16 st = tile_product<D>(Ks, 32 * wave, qf, r, h);    // S^T: element e is (key kb + acc_row(e, h), query q0 + r)
            // the product rounded to fp32 first, then * scale, then + bias; a key beyond the row's reach: deselected
            float bm = -INFINITY;
#pragma unroll
            for (int g = 0; g < 4; ++g) {
                const af32x4 bias = *reinterpret_cast<const af32x4*>(Bias + 32 * wave + 8 * g + 4 * h);
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    float x = st[4 * g + i] * a.scale + bias[i];
                    if (kb + 8 * g + 4 * h + i > last_key) x = -INFINITY;
                    st[4 * g + i] = x;
                    bm = x > bm ? x : bm;
                }
            }
            { const float other = __shfl_xor(bm, 32, 64); bm = other > bm ? other : bm; }
            const float mn = bm > mx ? bm : mx;
            const float alpha = exp_below(mx, mn);                    // +0 while the row has seen no key
            float ps = 0.f;
#pragma unroll
            for (int e = 0; e < 16; ++e) { st[e] = exp_below(st[e], mn); ps += st[e]; }       // P^T, unnormalised; 0 where deselected
            l = l * alpha + halves_sum(ps, h);
            mx = mn;
#pragma unroll
            for (int nn = 0; nn < NT; ++nn)
#pragma unroll
                for (int e = 0; e < 16; ++e) ot[nn][e] *= alpha;
            tile_accumulate<D>(ot, Vs, PV, 32 * wave, st, r, h);      // O^T += V^T P^T
        }
        __syncthreads();
    }

    // ---- level 1: the four waves in wave order; thread (wave, r, h) ends with d = 32 nn + 8 wave + 4 h .. + 3 of query r ----------
    float* Red = lds;                     // [wave][nn][e][lane]                            4 * NT * 16 * 64
    float* Mw = Red + 4 * NT * 1024;      // [wave][r], then Lw                             2 * 4 * 32
    float* Lw = Mw + 128;
#pragma unroll
    for (int nn = 0; nn < NT; ++nn)
#pragma unroll
        for (int e = 0; e < 16; ++e) Red[((wave * NT + nn) * 16 + e) * 64 + lane] = ot[nn][e];
    if (h == 0) { Mw[wave * 32 + r] = mx; Lw[wave * 32 + r] = l; }
    __syncthreads();
    float M = -INFINITY, lsum = 0.f;
#pragma unroll
    for (int w = 0; w < 4; ++w) { const float o = Mw[w * 32 + r]; M = o > M ? o : M; }
    af32x4 acc[NT];
#pragma unroll
    for (int nn = 0; nn < NT; ++nn) acc[nn] = af32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int w = 0; w < 4; ++w) {
        const float wgt = exp_below(Mw[w * 32 + r], M);
        lsum += wgt * Lw[w * 32 + r];
#pragma unroll
        for (int nn = 0; nn < NT; ++nn)
#pragma unroll
            for (int i = 0; i < 4; ++i) acc[nn][i] += wgt * Red[((w * NT + nn) * 16 + 4 * wave + i) * 64 + lane];
    }
    const int dcol = 8 * wave + 4 * h;                                // this thread's columns: 32 nn + dcol .. + 3
    float* const orow = on + int64_t(q0 + (r < qrows ? r : 0)) * a.ldo + dcol;

    if (live == 1) {
        // every row of the block has a visible key here (its own at the least): lsum > 0
        if (r < qrows) {
            const float inv = 1.0f / lsum;
#pragma unroll
            for (int nn = 0; nn < NT; ++nn)
                *reinterpret_cast<af32x4*>(orow + 32 * nn) = af32x4{acc[nn][0] * inv, acc[nn][1] * inv, acc[nn][2] * inv, acc[nn][3] * inv};
            if (ln && wave == 0 && h == 0) ln[q0 + r] = M + logf(lsum);
        }
        return;
    }

    // ---- level 2: publish, arrive, the last arriver merges the live slices in ascending order ---------------------------------------
    float* const slots = a.ws + ((int64_t(b) * a.heads + head) * a.blocks + qb) * a.slices * SW;
    {
        float* const slot = slots + int64_t(slice) * SW;
#pragma unroll
        for (int nn = 0; nn < NT; ++nn) handoff::publish<unsigned long long>(reinterpret_cast<af32x4*>(slot + r * D + 32 * nn + dcol), acc[nn]);
        if (wave == 0 && h == 0) {
            handoff::publish<float>(slot + 32 * D + r, M);
            handoff::publish<float>(slot + 32 * D + 32 + r, lsum);
        }
    }
    int* const ticket = a.tickets + ((int64_t(b) * a.heads + head) * a.blocks + qb) * a.tstride;
    if (!handoff::arrive_workgroup(ticket, live, &s_last)) return;

    float* Ms = lds;                      // [slice][r] of the live slices (at most 64), then Ls
    float* Ls = Ms + 64 * 32;
    for (int idx = tid; idx < live * 32; idx += 256) {
        const float* ml = slots + int64_t(idx >> 5) * SW + 32 * D + (idx & 31);
        Ms[idx] = handoff::fetch<float>(ml);
        Ls[idx] = handoff::fetch<float>(ml + 32);
    }
    __syncthreads();
    M = -INFINITY;
    for (int s = 0; s < live; ++s) { const float o = Ms[s * 32 + r]; M = o > M ? o : M; }
    lsum = 0.f;
#pragma unroll
    for (int nn = 0; nn < NT; ++nn) acc[nn] = af32x4{0.f, 0.f, 0.f, 0.f};
    for (int s0 = 0; s0 < live; s0 += 8) {
        af32x4 part[8][NT];
#pragma unroll
        for (int u = 0; u < 8; ++u)
#pragma unroll
            for (int nn = 0; nn < NT; ++nn) {
                part[u][nn] = af32x4{0.f, 0.f, 0.f, 0.f};
                if (s0 + u < live)
                    part[u][nn] = handoff::fetch<af32x4, unsigned long long>(reinterpret_cast<const af32x4*>(slots + int64_t(s0 + u) * SW + r * D + 32 * nn + dcol));
            }
#pragma unroll
        for (int u = 0; u < 8; ++u) {
            if (s0 + u < live) {
                const float wgt = exp_below(Ms[(s0 + u) * 32 + r], M);       // a slice whose keys are all masked next to a visible one: +0
                lsum += wgt * Ls[(s0 + u) * 32 + r];
#pragma unroll
                for (int nn = 0; nn < NT; ++nn)
#pragma unroll
                    for (int i = 0; i < 4; ++i) acc[nn][i] += wgt * part[u][nn][i];
            }
        }
    }
    if (r < qrows) {
        const float inv = 1.0f / lsum;
#pragma unroll
        for (int nn = 0; nn < NT; ++nn)
            *reinterpret_cast<af32x4*>(orow + 32 * nn) = af32x4{acc[nn][0] * inv, acc[nn][1] * inv, acc[nn][2] * inv, acc[nn][3] * inv};
        if (ln && wave == 0 && h == 0) ln[q0 + r] = M + logf(lsum);
    }
}

// attn_extend_split<D>, attn_paged_split<D> or attn_paged_split_bf16<D> with lds_bytes of dynamic LDS
template <class K>
static int ext_split_launch(K kernel, size_t lds_bytes, const ExtSplitArgs& a, dim3 grid) {
    const int rc = allow_lds(kernel, lds_bytes);
    if (rc != LG_OK) return rc;
    hipLaunchKernelGGL(kernel, grid, dim3(256), lds_bytes, rt().stream, a);
    return LG_OK;
}

}  // namespace lg
