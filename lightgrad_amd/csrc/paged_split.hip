// The split-key extend launch against a PAGED key / value cache of up to 16384 positions (gfx950, fp32 MFMA):
// lg_attention_extend_paged_split_f32 and, over pools of bfloat16 words, lg_attention_extend_paged_split_bf16_f32.
//
// lg_attention_extend_paged_f32 (paged.hip) keeps the 32 x capacity score tile and the whole table of an element in LDS and stops
// at 512 positions; lg_attention_extend_split_counts_f32 (extend_split.hip) reaches 16384 rows of a contiguous cache.  This launch
// is both at once: the partition, the online softmax over chunks of 128 keys and the in-launch merge of the second, with key
// j < t read from pool row block_table[b, j >> log2_block] * B + (j & (B - 1)) and the new rows written through the same words.
// The kernel is the same text (extend_split_body.h, attn_extend_split_body<D, PAGED = true, KV16>), so element b is computed bit
// for bit as the contiguous counts entry computes it on a (capacity, width) cache that holds the same rows.
//
//   grid      (slices of L keys, query blocks of 32 rows x heads, batch), 256 threads; L = lg_attention_extend_split_slice() is
//             256, 512 or 1024 and B = 4 .. 128, so a slice covers L >> log2_block WHOLE blocks: its table words are words
//             (sL >> log2_block) .. of the row, at most L / 4 of them, staged in LDS once and indexed by (j - sL) >> log2_block
//   verdict   an element with a word outside 0 .. num_blocks - 1 among words 0 .. ceil((t + n) / B) - 1 writes nothing at all - no
//             row of o, no lse, no pool row, no +0.0 row - and slices see different parts of the table: every workgroup of the
//             element that would store or arrive scans ALL live words of the row itself (coalesced, at most 16 loads a thread)
//             and votes across the workgroup before its first store and before it touches a ticket.  They all leave then, the
//             tickets stay zero, ONE workgroup raises LG_STATUS_BAD_INDEX; the other elements are computed
//   rows      only positions t .. t + n - 1 of an element are written, each once, by the slice that owns it: blocks that lie
//             wholly below the positions of the elements that name them may be shared; a block no table names is not touched
//   bf16      the rule of paged_bf16.hip: 8-byte pool loads widened in registers, a key of the launch's own attended to as r(.)
//             of it and stored as that word; tiles, MFMAs, softmax and fold order are fp32.  The launch returns o and lse bit for
//             bit as the fp32 one on (q, r(k_new), r(v_new), the widened pools)
// LDS (the chunk buffers, the bias row, L / 4 table words at the most) and registers do not depend on the capacity.  The host
// checks are paged_split_check (cache_entry.h); workspace and tickets are handled as by the contiguous entries.
#include "extend_split_body.h"

namespace lg {

template <int D>
__global__ void __launch_bounds__(256) attn_paged_split(const ExtSplitArgs a) { attn_extend_split_body<D, true, false>(a); }
template <int D>
__global__ void __launch_bounds__(256) attn_paged_split_bf16(const ExtSplitArgs a) { attn_extend_split_body<D, true, true>(a); }

}  // namespace lg

using namespace lg;

// Every key index of the kernel is an int below 2^15, a pool row an int below 2^31 (num_blocks << log2_block is checked), every
// global offset is formed in int64_t
extern "C" int lg_attention_extend_paged_split_supported(int64_t m, int64_t max_blocks, int64_t log2_block, int64_t D) {
    if (!cache_head_dim(D) || log2_block < 2 || log2_block > 7 || max_blocks < 1 || max_blocks > (kExtSplitMaxKeys >> log2_block)) return 0;
    return m >= 1 && m <= (max_blocks << log2_block) && m <= kExtSplitMaxRows;
}

// both entries: `item` bytes a pool element, the pools aligned to `align`
template <bool KV16>
static int paged_split_entry(const char* name, int item, int align, const float* q, int64_t ldq, int64_t sbq, const float* k_new, int64_t ldk, int64_t sbk,
                             const float* v_new, int64_t ldv, int64_t sbv, void* k_pool, void* v_pool, int64_t ldc, const int32_t* pos,
                             const int32_t* count, const int32_t* block_table, float* o, int64_t ldo, int64_t sbo, float* lse, int64_t batch,
                             int64_t heads, int64_t m, int64_t max_blocks, int64_t num_blocks, int64_t log2_block, int64_t D, float scale,
                             const float* mask, int64_t sbm) {
    int64_t capacity = 0;
    int rc = paged_split_check(name, item, align, q, ldq, sbq, k_new, ldk, sbk, v_new, ldv, sbv, k_pool, v_pool, ldc, pos, count, block_table, o, ldo, sbo,
                               lse, batch, heads, m, max_blocks, num_blocks, log2_block, D, mask, sbm, &capacity);
    if (rc != LG_OK || batch == 0) return rc;
    const int L = lg_attention_extend_split_slice();
    const int64_t blocks = (m + 31) / 32, slices = (capacity + L - 1) / L, triples = batch * heads * blocks;
    float* ws = nullptr;                             // a table of one slice never hands anything over
    if (slices > 1) {
        rc = lg_malloc(reinterpret_cast<void**>(&ws), size_t(triples * slices * 32 * (D + 2)) * sizeof(float));
        if (rc != LG_OK) return rc;
    }
    // the body addresses the pools through the argument block's cache pointers: with KV16 they are read as uint16_t again
    const ExtSplitArgs a{q, k_new, v_new, ldq, sbq, ldk, sbk, ldv, sbv, static_cast<float*>(k_pool), static_cast<float*>(v_pool), ldc, 0, pos, 1, count,
                         o, ldo, sbo, lse, int(heads), int(capacity), int(m), L, int(slices), int(blocks), scale, mask, sbm, ws, rt().tickets,
                         ticket_stride(triples), rt().status_dev, block_table, int(max_blocks), int(num_blocks), int(log2_block)};
    const dim3 grid{unsigned(slices), unsigned(heads * blocks), unsigned(batch)};
    if constexpr (KV16)
        rc = D == 64 ? ext_split_launch(&attn_paged_split_bf16<64>, size_t(attn_paged_split_lds_floats<64>()) * 4, a, grid)
                     : ext_split_launch(&attn_paged_split_bf16<32>, size_t(attn_paged_split_lds_floats<32>()) * 4, a, grid);
    else
        rc = D == 64 ? ext_split_launch(&attn_paged_split<64>, size_t(attn_paged_split_lds_floats<64>()) * 4, a, grid)
                     : ext_split_launch(&attn_paged_split<32>, size_t(attn_paged_split_lds_floats<32>()) * 4, a, grid);
    if (ws) { const int rf = lg_free(ws); if (rc == LG_OK) rc = rf; }      // stream-ordered: the block is only reused by later launches
    return rc;
}

extern "C" int lg_attention_extend_paged_split_f32(const float* q, int64_t ldq, int64_t sbq, const float* k_new, int64_t ldk, int64_t sbk,
                                                   const float* v_new, int64_t ldv, int64_t sbv, float* k_pool, float* v_pool, int64_t ldc,
                                                   const int32_t* pos, const int32_t* count, const int32_t* block_table, float* o, int64_t ldo,
                                                   int64_t sbo, float* lse, int64_t batch, int64_t heads, int64_t m, int64_t max_blocks,
                                                   int64_t num_blocks, int64_t log2_block, int64_t D, float scale, const float* mask, int64_t sbm) {
    LG_REQUIRE_INIT();
    const int rc = paged_split_entry<false>("lg_attention_extend_paged_split_f32", 4, 16, q, ldq, sbq, k_new, ldk, sbk, v_new, ldv, sbv, k_pool, v_pool, ldc,
                                            pos, count, block_table, o, ldo, sbo, lse, batch, heads, m, max_blocks, num_blocks, log2_block, D, scale, mask, sbm);
    if (rc != LG_OK || batch == 0) return rc;
    LG_CHECK_LAUNCH();
    return LG_OK;
}

// the same over pools of bfloat16 words, 2 bytes an element (ldc counts them); a lane loads and stores 4 pool words = 8 bytes at once
extern "C" int lg_attention_extend_paged_split_bf16_f32(const float* q, int64_t ldq, int64_t sbq, const float* k_new, int64_t ldk, int64_t sbk,
                                                        const float* v_new, int64_t ldv, int64_t sbv, uint16_t* k_pool, uint16_t* v_pool, int64_t ldc,
                                                        const int32_t* pos, const int32_t* count, const int32_t* block_table, float* o, int64_t ldo,
                                                        int64_t sbo, float* lse, int64_t batch, int64_t heads, int64_t m, int64_t max_blocks,
                                                        int64_t num_blocks, int64_t log2_block, int64_t D, float scale, const float* mask, int64_t sbm) {
    LG_REQUIRE_INIT();
    const int rc = paged_split_entry<true>("lg_attention_extend_paged_split_bf16_f32", 2, 8, q, ldq, sbq, k_new, ldk, sbk, v_new, ldv, sbv, k_pool, v_pool,
                                           ldc, pos, count, block_table, o, ldo, sbo, lse, batch, heads, m, max_blocks, num_blocks, log2_block, D, scale, mask,
                                           sbm);
    if (rc != LG_OK || batch == 0) return rc;
    LG_CHECK_LAUNCH();
    return LG_OK;
}
