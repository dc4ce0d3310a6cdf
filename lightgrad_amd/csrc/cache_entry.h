// The host checks of the KV-cache attention entries: lg_attention_decode{,_rows}_f32 (decode.hip), lg_attention_decode_split{,_rows}_f32
// (decode_split.hip), lg_attention_extend{,_rows,_counts,_packed}_f32 (extend.hip), lg_attention_extend_split{,_rows,_counts}_f32
// (extend_split.hip), lg_attention_extend_paged{,_bf16}_f32 (paged.hip, paged_bf16.hip) and lg_attention_extend_paged_split{,_bf16}_f32
// (paged_split.hip).  Host only; each entry calls these in its own order of refusal - shape, batch / heads, an empty
// batch, operands, row pitch, mask pitch, overlaps, applied updates - and every message starts with the entry's own name.
#pragma once
#include "common.h"

namespace lg {

// the head sizes the kernels of the family are instantiated for
inline bool cache_head_dim(int64_t D) { return D == 32 || D == 64; }

// `n` batch elements (or cache slots: `what`) and `heads` are dimensions of the grid
inline int cache_check_grid(const char* name, const char* what, int64_t n, int64_t most, int64_t heads) {
    LG_ARG(n >= 0 && heads >= 1 && n <= most && heads <= 65535, "%s: bad %s / heads", name, what);
    return LG_OK;
}

// a float operand that lanes reach 16 bytes at a time, rows `ld` and batch elements `sb` floats apart.  The decode kernels take a
// negative batch pitch; the extend body does not (cache_rows_operand)
inline bool cache_operand(const void* p, int64_t ld, int64_t sb) { return p && aligned16(p) && ld % 4 == 0 && sb % 4 == 0; }
inline bool cache_rows_operand(const void* p, int64_t ld, int64_t sb) { return cache_operand(p, ld, sb) && ld >= 0 && sb >= 0; }
// pos, count, cu, block_table: int32 words
inline bool cache_words(const void* p) { return p && (reinterpret_cast<uintptr_t>(p) & 3u) == 0; }

// the elements from the first to behind the last of a strided operand: `batch` elements sb apart, `rows` rows ld apart, w a row
inline int64_t cache_span(int64_t batch, int64_t sb, int64_t rows, int64_t ld, int64_t w) { return (batch - 1) * sb + (rows - 1) * ld + w; }

inline int cache_check_row_pitch(const char* name, const char* what, int64_t ldc, int64_t w) {
    LG_ARG(ldc >= w, "%s: %s row pitch %lld below heads * D = %lld", name, what, (long long)ldc, (long long)w);
    return LG_OK;
}

// `what` / `all`: "batch" / "the batch", or "slot" / "every slot" for the token-packed entry
inline int cache_check_mask(const char* name, const float* mask, int64_t sbm, int64_t capacity, const char* what, const char* all) {
    LG_ARG(!mask || sbm == 0 || sbm >= capacity, "%s: mask %s pitch %lld is neither 0 (one row for %s) nor >= capacity", name, what, (long long)sbm, all);
    return LG_OK;
}

// do `words` int32 words (pos, count, cu) share a byte with either cache?  `bytes`: 4 (or 2) * cache_span of a cache
inline bool words_overlap_caches(const int32_t* x, int64_t words, const void* k_cache, const void* v_cache, int64_t bytes) {
    return bytes_overlap(x, 4 * words, k_cache, bytes) || bytes_overlap(x, 4 * words, v_cache, bytes);
}

inline int cache_check_pos(const char* name, const int32_t* pos, int64_t words, const void* k_cache, const void* v_cache, int64_t bytes) {
    LG_ARG(!words_overlap_caches(pos, words, k_cache, v_cache, bytes),
           "%s: pos overlaps a cache: the launch writes the caches while other workgroups read their positions", name);
    return LG_OK;
}

// a write into a gradient whose update has been applied (common.h) is refused: o as (batch, rows, w) floats, both caches or pools
// as (cbatch, crows, w) elements of `item` bytes, and the dense optional output (p or lse, NULL = none)
inline int cache_check_writes(const float* o, int64_t batch, int64_t sbo, int64_t rows, int64_t ldo, const void* k_cache, const void* v_cache, int item,
                              int64_t cbatch, int64_t sbc, int64_t crows, int64_t ldc, int64_t w, const float* extra, int64_t extra_bytes) {
    const int64_t oshape[3] = {batch, rows, w}, ostrides[3] = {sbo, ldo, 1}, cshape[3] = {cbatch, crows, w}, cstrides[3] = {sbc, ldc, 1};
    int rc = adam_epilogue_check_strided(o, 4, 3, oshape, ostrides);
    if (rc != LG_OK) return rc;
    rc = adam_epilogue_check_strided(k_cache, item, 3, cshape, cstrides);
    if (rc != LG_OK) return rc;
    rc = adam_epilogue_check_strided(v_cache, item, 3, cshape, cstrides);
    if (rc != LG_OK) return rc;
    return extra ? adam_epilogue_check_write(extra, extra_bytes) : LG_OK;
}

// The one-token entries up to their overlap check (a cache of at most max_keys rows; `extra`: p or lse, 4-byte aligned).  The
// caller returns when this does not return LG_OK, or when batch == 0: nothing is launched then
inline int decode_check_operands(const char* name, int max_keys, int64_t pos_pitch, const float* q, int64_t sbq, const float* k_new, int64_t sbk,
                                 const float* v_new, int64_t sbv, const float* k_cache, const float* v_cache, int64_t ldc, int64_t sbc,
                                 const int32_t* pos, const float* o, int64_t sbo, const float* extra, int64_t batch, int64_t heads, int64_t capacity,
                                 int64_t D, const float* mask, int64_t sbm) {
    LG_ARG(cache_head_dim(D) && capacity >= 1 && capacity <= max_keys, "%s: capacity = %lld (1 .. %d), D = %lld (32 or 64) unsupported", name,
           (long long)capacity, max_keys, (long long)D);
    int rc = cache_check_grid(name, "batch", batch, 65535, heads);
    if (rc != LG_OK || batch == 0) return rc;
    LG_ARG(cache_operand(q, 0, sbq) && cache_operand(k_new, 0, sbk) && cache_operand(v_new, 0, sbv) && cache_operand(k_cache, ldc, sbc) &&
               cache_operand(v_cache, ldc, sbc) && cache_operand(o, 0, sbo) && cache_words(pos) && (reinterpret_cast<uintptr_t>(extra) & 3u) == 0,
           "%s: operands must be non-NULL and 16-byte aligned with pitches that are multiples of 4", name);
    const int64_t w = heads * D;
    rc = cache_check_row_pitch(name, "cache", ldc, w);
    if (rc != LG_OK) return rc;
    rc = cache_check_mask(name, mask, sbm, capacity, "batch", "the batch");
    if (rc != LG_OK) return rc;
    return cache_check_pos(name, pos, pos_pitch ? batch : 1, k_cache, v_cache, 4 * cache_span(batch, sbc, capacity, ldc, w));
}

// `m_name`: "m" new rows a batch element, or "m_max" a slot of the token-packed entry
inline int extend_check_shape(const char* name, const char* m_name, int64_t m, int64_t capacity, int64_t D) {
    LG_ARG(lg_attention_extend_supported(m, capacity, D), "%s: %s = %lld (1 .. capacity), capacity = %lld (1 .. 512), D = %lld (32 or 64) unsupported",
           name, m_name, (long long)m, (long long)capacity, (long long)D);
    return LG_OK;
}

// q, k_new, v_new and o of an extend entry (ld / sb in that order), pos and p under one message; `caches`: the entry's own
// cache_rows_operand of its two caches or pools - true where the bfloat16 entry refuses its pools under a message of its own
inline int extend_check_operands(const char* name, const float* q, const float* k_new, const float* v_new, const float* o, const int64_t (&ld)[4],
                                 const int64_t (&sb)[4], bool caches, const int32_t* pos, const float* p) {
    LG_ARG(cache_rows_operand(q, ld[0], sb[0]) && cache_rows_operand(k_new, ld[1], sb[1]) && cache_rows_operand(v_new, ld[2], sb[2]) && caches &&
               cache_rows_operand(o, ld[3], sb[3]) && cache_words(pos) && aligned16(p),
           "%s: operands must be non-NULL and 16-byte aligned with pitches that are non-negative multiples of 4", name);
    return LG_OK;
}

// The middle of lg_attention_extend{,_rows,_counts}_f32 (n batch elements with rows = m new rows each) and of the token-packed
// entry (n slots; its flat operands have rows = T rows and no batch pitch): operands, row pitch, mask pitch, then the new rows and
// the positions against the caches.  Every span covers n elements, the flat operands' at batch pitch 0
inline int extend_check_caches(const char* name, const float* q, const float* k_new, const float* v_new, const float* o, const int64_t (&ld)[4],
                               const int64_t (&sb)[4], const float* k_cache, const float* v_cache, int64_t ldc, int64_t sbc, const int32_t* pos,
                               int64_t pos_words, const float* p, int64_t n, int64_t rows, int64_t capacity, int64_t w, const float* mask, int64_t sbm,
                               const char* mask_what, const char* mask_all) {
    int rc = extend_check_operands(name, q, k_new, v_new, o, ld, sb, cache_rows_operand(k_cache, ldc, sbc) && cache_rows_operand(v_cache, ldc, sbc), pos, p);
    if (rc != LG_OK) return rc;
    rc = cache_check_row_pitch(name, "cache", ldc, w);
    if (rc != LG_OK) return rc;
    rc = cache_check_mask(name, mask, sbm, capacity, mask_what, mask_all);
    if (rc != LG_OK) return rc;
    const int64_t bytes = 4 * cache_span(n, sbc, capacity, ldc, w), k_bytes = 4 * cache_span(n, sb[1], rows, ld[1], w),
                  v_bytes = 4 * cache_span(n, sb[2], rows, ld[2], w);
    LG_ARG(!bytes_overlap(k_new, k_bytes, k_cache, bytes) && !bytes_overlap(k_new, k_bytes, v_cache, bytes) &&
               !bytes_overlap(v_new, v_bytes, k_cache, bytes) && !bytes_overlap(v_new, v_bytes, v_cache, bytes),
           "%s: k_new / v_new overlap a cache: the launch writes the caches while other workgroups read the new rows", name);
    return cache_check_pos(name, pos, pos_words, k_cache, v_cache, bytes);
}

// The paged entries behind their shape checks (batch >= 1): operands, row pitch, mask pitch, overlaps, the ticket pool, applied
// updates.  `item` / `align`: bytes of a pool element and the alignment of the pools; `extra`: the dense optional output - "p" of
// the 512-row launches, 16-byte aligned, or "lse" of the split-key ones, 4-byte aligned -, `extra_bytes` of it; `other`: the entry
// that takes float32 pools where this one takes bfloat16 words; `triples`: the tickets the launch counts on (0: none)
inline int paged_check_operands(const char* name, int item, int align, const char* other, const float* q, int64_t ldq, int64_t sbq, const float* k_new,
                                int64_t ldk, int64_t sbk, const float* v_new, int64_t ldv, int64_t sbv, const void* k_pool, const void* v_pool,
                                int64_t ldc, const int32_t* pos, const int32_t* count, const int32_t* block_table, const float* o, int64_t ldo,
                                int64_t sbo, const float* extra, const char* extra_what, int64_t extra_bytes, int64_t batch, int64_t heads, int64_t m,
                                int64_t max_blocks, int64_t num_blocks, int64_t log2_block, int64_t D, const float* mask, int64_t sbm, int64_t triples) {
    const int64_t B = int64_t(1) << log2_block, capacity = max_blocks * B;
    const bool is_p = extra_what[0] == 'p';
    const bool pools = k_pool && v_pool && ((reinterpret_cast<uintptr_t>(k_pool) | reinterpret_cast<uintptr_t>(v_pool)) & uintptr_t(align - 1)) == 0 &&
                       ldc >= 0 && ldc % 4 == 0;
    int rc = extend_check_operands(name, q, k_new, v_new, o, {ldq, ldk, ldv, ldo}, {sbq, sbk, sbv, sbo}, item == 2 || pools, pos, is_p ? extra : nullptr);
    if (rc != LG_OK) return rc;
    // (float32 pools were refused with the operands above)
    LG_ARG(pools, "%s: the bfloat16 pools must be non-NULL and 8-byte aligned with a row pitch that is a non-negative multiple of 4 elements (the float32 pools "
           "go to %s)", name, other);
    LG_ARG(cache_words(count) && cache_words(block_table), "%s: count and block_table must be non-NULL and 4-byte aligned", name);
    LG_ARG(is_p || (reinterpret_cast<uintptr_t>(extra) & 3u) == 0, "%s: lse must be 4-byte aligned (or NULL)", name);
    const int64_t w = heads * D, rows = num_blocks * B;
    rc = cache_check_row_pitch(name, "pool", ldc, w);
    if (rc != LG_OK) return rc;
    rc = cache_check_mask(name, mask, sbm, capacity, "batch", "the batch");
    if (rc != LG_OK) return rc;
    {
        // what the launch writes - the pools (`item` bytes an element), o, p or lse - shares no byte with any other operand it reads or
        // writes: other workgroups of the launch read the new rows, the positions, the counts and the tables while the pools are written
        const void* ptr[9] = {k_pool, v_pool, o, extra, k_new, v_new, pos, count, block_table};
        const char* what[9] = {"k_pool", "v_pool", "o", extra_what, "k_new", "v_new", "pos", "count", "block_table"};
        const int64_t pool_bytes = cache_span(1, 0, rows, ldc, w) * item;
        const int64_t bytes[9] = {pool_bytes, pool_bytes, cache_span(batch, sbo, m, ldo, w) * 4, extra_bytes,
                                  cache_span(batch, sbk, m, ldk, w) * 4, cache_span(batch, sbv, m, ldv, w) * 4, batch * 4, batch * 4, batch * max_blocks * 4};
        for (int i = 0; i < 4; ++i)
            for (int j = i + 1; j < 9; ++j)
                LG_ARG(!bytes_overlap(ptr[i], bytes[i], ptr[j], bytes[j]), "%s: %s overlaps %s: the launch writes the one while other workgroups use the other",
                       name, what[i], what[j]);
        LG_ARG(!bytes_overlap(pos, bytes[6], count, bytes[7]), "%s: count overlaps pos", name);
    }
    LG_ARG(triples <= rt().n_tickets, "%s: the ticket pool holds %d counters, %lld (batch, head, query block) triples need one each", name,
           rt().n_tickets, (long long)triples);
    return cache_check_writes(o, batch, sbo, m, ldo, k_pool, v_pool, item, 1, 0, rows, ldc, w, extra, extra_bytes);
}

// Everything lg_attention_extend_paged_f32 (item = 4 bytes a pool element, pools aligned to align = 16) and
// lg_attention_extend_paged_bf16_f32 (2, 8: a lane loads and stores 4 pool words = 8 bytes at once) refuse, in their order.
// max_table / max_keys: kPagedMaxTable / kExtMaxKeys of extend_body.h.  *capacity = max_blocks << log2_block.  The caller returns
// when this does not return LG_OK, or when batch == 0
inline int paged_check(const char* name, int item, int align, int max_table, int max_keys, const float* q, int64_t ldq, int64_t sbq,
                       const float* k_new, int64_t ldk, int64_t sbk, const float* v_new, int64_t ldv, int64_t sbv, const void* k_pool, const void* v_pool,
                       int64_t ldc, const int32_t* pos, const int32_t* count, const int32_t* block_table, const float* o, int64_t ldo, int64_t sbo,
                       const float* p, int64_t batch, int64_t heads, int64_t m, int64_t max_blocks, int64_t num_blocks, int64_t log2_block, int64_t D,
                       const float* mask, int64_t sbm, int64_t* capacity_out) {
    LG_ARG(log2_block >= 2 && log2_block <= 7 && max_blocks >= 1 && max_blocks <= max_table && (max_blocks << log2_block) <= max_keys,
           "%s: blocks of 1 << %lld rows (4 .. 128) and %lld of them per table (capacity 1 .. 512) unsupported", name, (long long)log2_block,
           (long long)max_blocks);
    const int64_t B = int64_t(1) << log2_block, capacity = *capacity_out = max_blocks * B;
    int rc = extend_check_shape(name, "m", m, capacity, D);
    if (rc != LG_OK) return rc;
    LG_ARG(num_blocks >= 1 && num_blocks * B < (int64_t(1) << 31), "%s: a pool of %lld blocks of %lld rows (1 .. 2^31 - 1 rows) unsupported", name,
           (long long)num_blocks, (long long)B);
    rc = cache_check_grid(name, "batch", batch, 65535, heads);
    if (rc != LG_OK || batch == 0) return rc;
    return paged_check_operands(name, item, align, "lg_attention_extend_paged_f32", q, ldq, sbq, k_new, ldk, sbk, v_new, ldv, sbv, k_pool, v_pool, ldc, pos,
                                count, block_table, o, ldo, sbo, p, "p", batch * heads * m * capacity * 4, batch, heads, m, max_blocks, num_blocks,
                                log2_block, D, mask, sbm, 0);
}

// ... and lg_attention_extend_paged_split_f32 / _bf16_f32 (paged_split.hip): tables of up to 16384 positions, m <= 128 rows, lse
// (NULL, or (batch, heads, m)) in place of p, a ticket per (batch, head, query block) triple.  *capacity and the return as above
inline int paged_split_check(const char* name, int item, int align, const float* q, int64_t ldq, int64_t sbq, const float* k_new, int64_t ldk, int64_t sbk,
                             const float* v_new, int64_t ldv, int64_t sbv, const void* k_pool, const void* v_pool, int64_t ldc, const int32_t* pos,
                             const int32_t* count, const int32_t* block_table, const float* o, int64_t ldo, int64_t sbo, const float* lse, int64_t batch,
                             int64_t heads, int64_t m, int64_t max_blocks, int64_t num_blocks, int64_t log2_block, int64_t D, const float* mask,
                             int64_t sbm, int64_t* capacity_out) {
    LG_ARG(lg_attention_extend_paged_split_supported(m, max_blocks, log2_block, D),
           "%s: m = %lld (1 .. min(capacity, 128)), blocks of 1 << %lld rows (4 .. 128), %lld of them per table (capacity 1 .. 16384), D = %lld (32 or 64) "
           "unsupported", name, (long long)m, (long long)log2_block, (long long)max_blocks, (long long)D);
    const int64_t B = int64_t(1) << log2_block, blocks = (m + 31) / 32;
    *capacity_out = max_blocks * B;
    LG_ARG(num_blocks >= 1 && num_blocks * B < (int64_t(1) << 31), "%s: a pool of %lld blocks of %lld rows (1 .. 2^31 - 1 rows) unsupported", name,
           (long long)num_blocks, (long long)B);
    const int rc = cache_check_grid(name, "batch", batch, 65535, heads);
    if (rc != LG_OK) return rc;
    LG_ARG(heads * blocks <= 65535, "%s: %lld heads x %lld query blocks exceed a grid dimension of 65535", name, (long long)heads, (long long)blocks);
    if (batch == 0) return LG_OK;
    return paged_check_operands(name, item, align, "lg_attention_extend_paged_split_f32", q, ldq, sbq, k_new, ldk, sbk, v_new, ldv, sbv, k_pool, v_pool, ldc,
                                pos, count, block_table, o, ldo, sbo, lse, "lse", batch * heads * m * 4, batch, heads, m, max_blocks, num_blocks, log2_block,
                                D, mask, sbm, batch * heads * blocks);
}

}  // namespace lg
