// Attention of m NEW tokens against a key / value cache of up to 16384 rows, the keys SPLIT over workgroups and the partial
// softmaxes merged inside the same launch (gfx950, fp32 MFMA): lg_attention_extend_split_f32 / _rows_f32 / _counts_f32.
//
// lg_attention_extend_f32 (extend.hip) keeps the 32 x capacity score tile of a query block in LDS and stops at 512 keys;
// attn_stream_fwd (attention_stream.hip) has no LDS bound but gives ALL keys to the workgroup of 128 queries: 4 .. 128 new rows
// behind 16384 keys would be a handful of workgroups walking 128 chunks each; attn_decode_split (decode_split.hip) splits the keys
// but has one query and no matrix cores.  This kernel is the online softmax of the first in the partition of the second.
//
//   partition   grid (slices of L keys, query blocks of 32 rows x heads, batch), 256 threads.  Every workgroup reads t (and
//               n = count[b]) itself.  Block q0 of an element reaches keys [0, t + q0 + rows); slice s owns [sL, sL + L): it returns
//               before any load when sL is beyond the reach, and knows that live = ceil(reach / L) slices of its block work.
//   slice       keys stream through LDS in chunks of 128 - K rows at pitch D + 4, V rows at pitch D + 8, the bias of the keys -
//               with the next chunk's global loads issued ahead of the MFMAs.  Wave w takes the 32-key block w of every chunk; Q is
//               not split: each wave holds the block's Q fragment (D / 2 floats a lane), forms S^T = K Q^T, keeps a running
//               maximum and sum per query as per-lane scalars and feeds P^T from the accumulator to O^T += V^T P^T in registers
//               (stream_tiles.h).  LDS does not depend on the capacity.
//   seam        extend.hip's: key j < t from the cache, t <= j < t + n from k_new / v_new, j >= t + n ZERO in LDS (seam_load /
//               seam_store); row i sees columns [0, t + q0 + i] by selection, nothing is multiplied by a mask; cache rows >= t may
//               hold NaN.  The chunk loop covers keys up to round32(min(sL + L, reach)): what lies between the reach and that
//               bound is >= t, so it is a new row or zero, never a cache row.
//   cache rows  the slice that owns position t + q0 + i stores new row i of its head: every new row once, no other row.
//   merge       (1) the four waves' {m, l, O^T} fold through LDS in wave order, thread (wave w, lane (r, h)) taking d =
//               32 n + 8 w + 4 h .. + 3 of query r; (2) live == 1: that thread normalises and stores, no workspace, no ticket;
//               (3) else the workgroup publishes 32 x {O[D], m, l} (handoff.h) into slot (b, head, block, slice) and arrives at
//               the ticket of (b, head, block) with expected = live; the last arriver fetches m and l of every live slice into
//               LDS, takes M = max m_s, and sums w_s l_s and w_s O_s with w_s = exp(m_s - M) in ascending slice order, eight
//               slices' fetches in flight at a time; o = sum * (1 / Lsum), lse = M + log(Lsum).  Nothing depends on who is last.
// A wave or a slice without a visible key of some row carries m = -inf, l = 0 for it: its weight is exp(-inf - M) = +0 and it
// adds exact zeros; a maximum of -inf is replaced by 0 before it is subtracted, so -inf - -inf is never formed.
// Errors: t < 0 or t + n > capacity - nothing is written for the element, ONE workgroup (slice 0 of block 0 of head 0) raises
// LG_STATUS_BAD_INDEX.  Counts: rows >= n of o and lse are +0.0, cleared by slice 0 of their block; a block with q0 >= n ends there.
#include "extend_body.h"
#include "handoff.h"
#include "stream_tiles.h"

namespace lg {

constexpr int kExtSplitMaxKeys = 16384;          // the range of lg_attention_stream_supported
constexpr int kExtSplitMaxRows = 128;            // m of one launch: four query blocks, which bounds the workspace
constexpr int kExtSplitMinSlice = 256;           // 64 slices at the most: what the merge's LDS rows are sized for
constexpr int kExtSplitSlice = 256;              // L, chosen by profiles/extend_split.md
static int g_ext_split_slice = kExtSplitSlice;   // (tools/extend_split_time.py compares 256, 512 and 1024 in one process)

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
};

template <int D> constexpr int attn_extend_split_lds_floats() { return kExtChunk * (D + 4) + kExtChunk * (D + 8) + kExtChunk; }

// exp(x - m) with m = -inf read as 0: x = -inf gives +0, and -inf - -inf is never formed
__device__ __forceinline__ float exp_below(float x, float m) { return expf(x - (m == -INFINITY ? 0.f : m)); }

template <int D>
__global__ void __launch_bounds__(256) attn_extend_split(const ExtSplitArgs a) {
    extern __shared__ __attribute__((aligned(16))) float lds[];
    __shared__ int s_last;
    constexpr int PK = D + 4, PV = D + 8, Q4 = D / 4, NA = kExtChunk * Q4 / 256, NB = 32 * Q4 / 256, NT = D / 32, SW = 32 * (D + 2);
    float* Ks = lds;                      // a chunk of K, K-contiguous A of S^T            128 x PK
    float* Vs = Ks + kExtChunk * PK;      // the same chunk of V, d along the lanes          128 x PV
    float* Bias = Vs + kExtChunk * PV;    // the bias of the chunk's keys                    128
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

    const float* kc = a.k_cache + int64_t(b) * a.sbc + head * D;
    const float* vc = a.v_cache + int64_t(b) * a.sbc + head * D;
    const float* kn = a.k_new + int64_t(b) * a.sbk + head * D;
    const float* vn = a.v_new + int64_t(b) * a.sbv + head * D;
    const float* mrow = a.mask ? a.mask + int64_t(b) * a.sbm : nullptr;
    // what key j adds to every score of its column: (1.0 - mask) * -10000.0 in fp32, the composite's own arithmetic; -0.0f where
    // there is no mask or no key
    auto key_bias = [&](int j) { return (mrow && j < keys) ? (1.0f - mrow[j]) * -10000.0f : -0.0f; };

    af32x4 rk[NA], rv[NA];
    float rb = -0.0f;
    seam_load<D, NA>(rk, kc, a.ldc, kn, a.ldk, j_lo, t, n);
    seam_load<D, NA>(rv, vc, a.ldc, vn, a.ldv, j_lo, t, n);
    if (tid < kExtChunk) rb = key_bias(j_lo + tid);
    float qf[D / 2];
    frag_load<D>(qf, r < qrows ? a.q + int64_t(b) * a.sbq + int64_t(q0 + r) * a.ldq + head * D : nullptr, h);

    // the block's new rows whose positions this slice owns become rows of the caches, bit for bit; nothing in this launch reads
    // them there
#pragma unroll
    for (int i = 0; i < NB; ++i) {
        const int f = tid + i * 256, row = f / Q4, at = t + q0 + row;
        if (row < qrows && at >= j_lo && at < j_lo + L) {
            const int64_t dst = int64_t(b) * a.sbc + int64_t(at) * a.ldc + head * D + (f % Q4) * 4;
            *reinterpret_cast<af32x4*>(a.k_cache + dst) = *reinterpret_cast<const af32x4*>(kn + int64_t(q0 + row) * a.ldk + (f % Q4) * 4);
            *reinterpret_cast<af32x4*>(a.v_cache + dst) = *reinterpret_cast<const af32x4*>(vn + int64_t(q0 + row) * a.ldv + (f % Q4) * 4);
        }
    }

    // ---- the slice: wave w on the 32-key block w of every chunk, an online softmax per query ----------------------------------------
    float mx = -INFINITY, l = 0.f;
    af32x16 ot[NT];
#pragma unroll
    for (int nn = 0; nn < NT; ++nn) ot[nn] = zero16();
    const int last_key = t + q0 + r;                                  // the last key this lane's query sees
    for (int c0 = j_lo; c0 < j_hi; c0 += kExtChunk) {
        seam_store<D, NA>(rk, Ks, PK, c0, keys, Kend);
        seam_store<D, NA>(rv, Vs, PV, c0, keys, Kend);
        if (tid < kExtChunk) Bias[tid] = rb;
        __syncthreads();
        if (c0 + kExtChunk < j_hi) {
            seam_load<D, NA>(rk, kc, a.ldc, kn, a.ldk, c0 + kExtChunk, t, n);
            seam_load<D, NA>(rv, vc, a.ldc, vn, a.ldv, c0 + kExtChunk, t, n);
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

}  // namespace lg

using namespace lg;

// Every index of the kernel (t + q0 + 31, c0 + 128 + tid, slice * L) is an int below 2^15, every global offset is formed in
// int64_t.  LDS and registers do not depend on the capacity.  m <= 128 bounds the workspace of a launch:
// batch * heads * 4 blocks * slices * 32 * (D + 2) floats.
extern "C" int lg_attention_extend_split_supported(int64_t m, int64_t capacity, int64_t D) {
    return cache_head_dim(D) && capacity >= 1 && capacity <= kExtSplitMaxKeys && m >= 1 && m <= capacity && m <= kExtSplitMaxRows;
}

extern "C" int lg_attention_extend_split_slice(void) { return g_ext_split_slice; }

// experiments only (tools/extend_split_time.py): the candidates of L side by side in one process
extern "C" int lg_attention_extend_split_set_slice(int64_t L) {
    LG_ARG(L == 256 || L == 512 || L == 1024, "lg_attention_extend_split_set_slice: L = %lld is none of 256, 512, 1024", (long long)L);
    static_assert(kExtSplitMaxKeys / kExtSplitMinSlice <= 64, "the merge keeps m and l of 64 slices in LDS");
    g_ext_split_slice = int(L);
    return LG_OK;
}

template <class K>
static int ext_split_launch(K kernel, size_t lds_bytes, const ExtSplitArgs& a, dim3 grid) {
    const int rc = allow_lds(kernel, lds_bytes);
    if (rc != LG_OK) return rc;
    hipLaunchKernelGGL(kernel, grid, dim3(256), lds_bytes, rt().stream, a);
    return LG_OK;
}

// every entry: `pos_pitch` words between the positions of neighbouring batch elements (0: one word for the batch); `counts`: the
// entry takes a word per batch element in `count` (NULL for the others)
static int ext_split_entry(const char* name, int64_t pos_pitch, bool counts, const int32_t* count, const float* q, int64_t ldq, int64_t sbq,
                           const float* k_new, int64_t ldk, int64_t sbk, const float* v_new, int64_t ldv, int64_t sbv, float* k_cache, float* v_cache,
                           int64_t ldc, int64_t sbc, const int32_t* pos, float* o, int64_t ldo, int64_t sbo, float* lse, int64_t batch, int64_t heads,
                           int64_t m, int64_t capacity, int64_t D, float scale, const float* mask, int64_t sbm) {
    LG_ARG(lg_attention_extend_split_supported(m, capacity, D),
           "%s: m = %lld (1 .. min(capacity, %d)), capacity = %lld (1 .. %d), D = %lld (32 or 64) unsupported", name, (long long)m, kExtSplitMaxRows,
           (long long)capacity, kExtSplitMaxKeys, (long long)D);
    int rc = cache_check_grid(name, "batch", batch, 65535, heads);
    if (rc != LG_OK) return rc;
    const int64_t blocks = (m + 31) / 32, slices = (capacity + g_ext_split_slice - 1) / g_ext_split_slice;
    LG_ARG(heads * blocks <= 65535, "%s: %lld heads x %lld query blocks exceed a grid dimension of 65535", name, (long long)heads, (long long)blocks);
    if (batch == 0) return LG_OK;
    const int64_t w = heads * D, pos_words = pos_pitch ? batch : 1, triples = batch * heads * blocks, lse_bytes = batch * heads * m * 4;
    rc = extend_check_caches(name, q, k_new, v_new, o, {ldq, ldk, ldv, ldo}, {sbq, sbk, sbv, sbo}, k_cache, v_cache, ldc, sbc, pos, pos_words, nullptr, batch,
                             m, capacity, w, mask, sbm, "batch", "the batch");
    if (rc != LG_OK) return rc;
    const int64_t cache_bytes = 4 * cache_span(batch, sbc, capacity, ldc, w);
    if (counts) {
        LG_ARG(cache_words(count), "%s: count must be non-NULL and 4-byte aligned", name);
        LG_ARG(!words_overlap_caches(count, batch, k_cache, v_cache, cache_bytes),
               "%s: count overlaps a cache: the launch writes the caches while other workgroups read their counts", name);
        LG_ARG(!bytes_overlap(count, 4 * batch, pos, 4 * pos_words), "%s: count overlaps pos", name);
    }
    LG_ARG((reinterpret_cast<uintptr_t>(lse) & 3u) == 0, "%s: lse must be 4-byte aligned (or NULL)", name);
    LG_ARG(!bytes_overlap(lse, lse_bytes, o, 4 * cache_span(batch, sbo, m, ldo, w)) && !bytes_overlap(lse, lse_bytes, k_cache, cache_bytes) &&
               !bytes_overlap(lse, lse_bytes, v_cache, cache_bytes),
           "%s: lse overlaps o or a cache: the launch writes all of them", name);
    LG_ARG(triples <= rt().n_tickets, "%s: the ticket pool holds %d counters, %lld (batch, head, query block) triples need one each", name,
           rt().n_tickets, (long long)triples);
    rc = cache_check_writes(o, batch, sbo, m, ldo, k_cache, v_cache, 4, batch, sbc, capacity, ldc, w, lse, lse_bytes);
    if (rc != LG_OK) return rc;
    float* ws = nullptr;                             // a cache of one slice never hands anything over
    if (slices > 1) {
        rc = lg_malloc(reinterpret_cast<void**>(&ws), size_t(triples * slices * 32 * (D + 2)) * sizeof(float));
        if (rc != LG_OK) return rc;
    }
    const ExtSplitArgs a{q, k_new, v_new, ldq, sbq, ldk, sbk, ldv, sbv, k_cache, v_cache, ldc, sbc, pos, pos_pitch, counts ? count : nullptr, o, ldo, sbo, lse,
                         int(heads), int(capacity), int(m), g_ext_split_slice, int(slices), int(blocks), scale, mask, sbm, ws, rt().tickets,
                         ticket_stride(triples), rt().status_dev};
    const dim3 grid{unsigned(slices), unsigned(heads * blocks), unsigned(batch)};
    rc = D == 64 ? ext_split_launch(&attn_extend_split<64>, size_t(attn_extend_split_lds_floats<64>()) * 4, a, grid)
                 : ext_split_launch(&attn_extend_split<32>, size_t(attn_extend_split_lds_floats<32>()) * 4, a, grid);
    if (ws) { const int rf = lg_free(ws); if (rc == LG_OK) rc = rf; }      // stream-ordered: the block is only reused by later launches
    return rc;
}

extern "C" int lg_attention_extend_split_f32(const float* q, int64_t ldq, int64_t sbq, const float* k_new, int64_t ldk, int64_t sbk,
                                             const float* v_new, int64_t ldv, int64_t sbv, float* k_cache, float* v_cache, int64_t ldc,
                                             int64_t sbc, const int32_t* pos, float* o, int64_t ldo, int64_t sbo, float* lse, int64_t batch,
                                             int64_t heads, int64_t m, int64_t capacity, int64_t D, float scale, const float* mask, int64_t sbm) {
    LG_REQUIRE_INIT();
    const int rc = ext_split_entry("lg_attention_extend_split_f32", 0, false, nullptr, q, ldq, sbq, k_new, ldk, sbk, v_new, ldv, sbv, k_cache, v_cache, ldc,
                                   sbc, pos, o, ldo, sbo, lse, batch, heads, m, capacity, D, scale, mask, sbm);
    if (rc != LG_OK || batch == 0) return rc;
    LG_CHECK_LAUNCH();
    return LG_OK;
}

// the same launch with a position per batch element: pos holds `batch` contiguous words, element b uses t = pos[b]
extern "C" int lg_attention_extend_split_rows_f32(const float* q, int64_t ldq, int64_t sbq, const float* k_new, int64_t ldk, int64_t sbk,
                                                  const float* v_new, int64_t ldv, int64_t sbv, float* k_cache, float* v_cache, int64_t ldc,
                                                  int64_t sbc, const int32_t* pos, float* o, int64_t ldo, int64_t sbo, float* lse, int64_t batch,
                                                  int64_t heads, int64_t m, int64_t capacity, int64_t D, float scale, const float* mask,
                                                  int64_t sbm) {
    LG_REQUIRE_INIT();
    const int rc = ext_split_entry("lg_attention_extend_split_rows_f32", 1, false, nullptr, q, ldq, sbq, k_new, ldk, sbk, v_new, ldv, sbv, k_cache, v_cache,
                                   ldc, sbc, pos, o, ldo, sbo, lse, batch, heads, m, capacity, D, scale, mask, sbm);
    if (rc != LG_OK || batch == 0) return rc;
    LG_CHECK_LAUNCH();
    return LG_OK;
}

// the `_rows` entry with a token count per batch element: element b has n = count[b] real new tokens among its m rows and is
// computed as by the one-word entry on it alone with m = n; rows >= n of o and lse are +0.0
extern "C" int lg_attention_extend_split_counts_f32(const float* q, int64_t ldq, int64_t sbq, const float* k_new, int64_t ldk, int64_t sbk,
                                                    const float* v_new, int64_t ldv, int64_t sbv, float* k_cache, float* v_cache, int64_t ldc,
                                                    int64_t sbc, const int32_t* pos, const int32_t* count, float* o, int64_t ldo, int64_t sbo,
                                                    float* lse, int64_t batch, int64_t heads, int64_t m, int64_t capacity, int64_t D, float scale,
                                                    const float* mask, int64_t sbm) {
    LG_REQUIRE_INIT();
    const int rc = ext_split_entry("lg_attention_extend_split_counts_f32", 1, true, count, q, ldq, sbq, k_new, ldk, sbk, v_new, ldv, sbv, k_cache, v_cache,
                                   ldc, sbc, pos, o, ldo, sbo, lse, batch, heads, m, capacity, D, scale, mask, sbm);
    if (rc != LG_OK || batch == 0) return rc;
    LG_CHECK_LAUNCH();
    return LG_OK;
}
