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
// The kernel's text is attn_extend_split_body<D, false, false> (extend_split_body.h), shared with the paged launches of
// paged_split.hip.
#include "extend_split_body.h"

namespace lg {

static int g_ext_split_slice = kExtSplitSlice;   // (tools/extend_split_time.py compares 256, 512 and 1024 in one process)

template <int D>
__global__ void __launch_bounds__(256) attn_extend_split(const ExtSplitArgs a) { attn_extend_split_body<D, false, false>(a); }

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
