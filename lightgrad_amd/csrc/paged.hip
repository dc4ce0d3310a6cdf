// The extend launch against a PAGED key / value cache (gfx950, fp32 MFMA): lg_attention_extend_paged_f32.
//
// lg_attention_extend_counts_f32 (extend.hip) with the caches reached through a table of fixed-size blocks: the keys and values of
// every layer lie in a POOL of num_blocks blocks of B = 1 << log2_block rows, and word n of row b of `block_table` (batch,
// max_blocks) names the block that holds positions n * B .. n * B + B - 1 of batch element b.  Position j of element b is pool
// row block_table[b, j >> log2_block] * B + (j & (B - 1)): for the streamed keys j < t and for the count[b] new rows the launch
// writes at t ..; capacity = max_blocks * B.  Everything else is the counts entry - the kernel body is the same text
// (extend_body.h, attn_extend_body<D, false, PAGED = true>): grid, LDS tile, chunks of 128 keys, fold order, softmax, the +0.0
// rows, p, the mask over logical positions, the status flag.  So element b is computed bit for bit as the counts entry computes
// it on a contiguous (capacity, width) cache that holds the same rows.  What the entry refuses on the host is paged_check
// (cache_entry.h), shared with the bfloat16 pools of paged_bf16.hip.
//
// No address is ever formed from an unchecked word: the workgroup reads its element's table ONCE, into LDS, checks words
// 0 .. ceil((t + count) / B) - 1 against 0 .. num_blocks - 1 on the way (a barrier with a vote: uniform over the workgroup) and
// replaces the words behind by 0; a bad word makes the element bad - nothing of it is written, LG_STATUS_BAD_INDEX is raised, the
// other elements are computed.  The launch writes rows t .. t + count - 1 of an element only: blocks that lie wholly below the
// positions of the elements that name them may be shared, and a block no table names is never touched.
#include "extend_body.h"

namespace lg {

template <int D>
__global__ void __launch_bounds__(256) attn_paged(const ExtendArgs a) { attn_extend_body<D, false, true>(a); }

}  // namespace lg

using namespace lg;

extern "C" int lg_attention_extend_paged_f32(const float* q, int64_t ldq, int64_t sbq, const float* k_new, int64_t ldk, int64_t sbk,
                                             const float* v_new, int64_t ldv, int64_t sbv, float* k_pool, float* v_pool, int64_t ldc,
                                             const int32_t* pos, const int32_t* count, const int32_t* block_table, float* o, int64_t ldo,
                                             int64_t sbo, float* p, int64_t batch, int64_t heads, int64_t m, int64_t max_blocks,
                                             int64_t num_blocks, int64_t log2_block, int64_t D, float scale, const float* mask, int64_t sbm) {
    LG_REQUIRE_INIT();
    int64_t capacity = 0;
    int rc = paged_check("lg_attention_extend_paged_f32", 4, 16, kPagedMaxTable, kExtMaxKeys, q, ldq, sbq, k_new, ldk, sbk, v_new, ldv, sbv, k_pool, v_pool,
                         ldc, pos, count, block_table, o, ldo, sbo, p, batch, heads, m, max_blocks, num_blocks, log2_block, D, mask, sbm, &capacity);
    if (rc != LG_OK || batch == 0) return rc;
    const ExtendArgs a{q, k_new, v_new, ldq, sbq, ldk, sbk, ldv, sbv, k_pool, v_pool, ldc, 0, pos, 1, count, o, ldo, sbo, p,
                       int(heads), int(capacity), int(m), scale, mask, sbm, rt().status_dev, nullptr, 0,
                       block_table, int(max_blocks), int(num_blocks), int(log2_block)};
    const dim3 grid{unsigned((m + 31) / 32), unsigned(heads), unsigned(batch)};
    const int Cp = round32(a.capacity);
    rc = D == 64 ? launch_extend_body(&attn_paged<64>, size_t(attn_paged_lds_floats<64>(Cp)) * 4, a, grid)
                 : launch_extend_body(&attn_paged<32>, size_t(attn_paged_lds_floats<32>(Cp)) * 4, a, grid);
    if (rc != LG_OK) return rc;
    LG_CHECK_LAUNCH();
    return LG_OK;
}
