// The paged extend launch over key / value pools of bfloat16 words (gfx950, fp32 MFMA): lg_attention_extend_paged_bf16_f32.
//
// lg_attention_extend_paged_f32 (paged.hip) with 2 bytes per pool element: a pool row holds the upper 16 bits of r(x), r = round
// to bfloat16 (nearest, ties to even: `bf16_round_array`), of every key / value the projection produced.  The kernel body is the
// same text once more (extend_body.h, attn_extend_body<D, false, true, KV16 = true>).  It widens the pool's words while it stages
// them (w << 16 IS the fp32 value), passes the launch's own new rows through r where they are read as keys and values, and packs
// them with the same r where they are written; tiles, MFMAs, softmax, bias row and fold order are fp32 as they were.  So the
// launch returns o and p bit for bit as lg_attention_extend_paged_f32 returns them on (q, r(k_new), r(v_new), the widened pools),
// and a key is attended to as r of it whether this launch or an earlier one brought it in.  Queries are not rounded.
//
// A file of its own: paged.hip holds exactly its two kernels with the code they had (tests/test_paged_registers.py).  The host
// checks are the paged entry's too: paged_check (cache_entry.h) with the pool element's size and the pools' alignment.
// The bounds behaviour is the paged entry's: every table word of the reach checked in LDS before an address is formed, a bad
// position, count or word -> nothing of the element written, LG_STATUS_BAD_INDEX raised, the other elements computed.
#include "extend_body.h"

namespace lg {

template <int D>
__global__ void __launch_bounds__(256) attn_paged_bf16(const ExtendArgs a) { attn_extend_body<D, false, true, true>(a); }

}  // namespace lg

using namespace lg;

extern "C" int lg_attention_extend_paged_bf16_f32(const float* q, int64_t ldq, int64_t sbq, const float* k_new, int64_t ldk, int64_t sbk,
                                                  const float* v_new, int64_t ldv, int64_t sbv, uint16_t* k_pool, uint16_t* v_pool, int64_t ldc,
                                                  const int32_t* pos, const int32_t* count, const int32_t* block_table, float* o, int64_t ldo,
                                                  int64_t sbo, float* p, int64_t batch, int64_t heads, int64_t m, int64_t max_blocks,
                                                  int64_t num_blocks, int64_t log2_block, int64_t D, float scale, const float* mask, int64_t sbm) {
    LG_REQUIRE_INIT();
    int64_t capacity = 0;
    // the paged entry's refusals at 2 bytes a pool element; a lane loads and stores 4 pool words = 8 bytes at once
    int rc = paged_check("lg_attention_extend_paged_bf16_f32", 2, 8, kPagedMaxTable, kExtMaxKeys, q, ldq, sbq, k_new, ldk, sbk, v_new, ldv, sbv, k_pool,
                         v_pool, ldc, pos, count, block_table, o, ldo, sbo, p, batch, heads, m, max_blocks, num_blocks, log2_block, D, mask, sbm, &capacity);
    if (rc != LG_OK || batch == 0) return rc;
    // the body addresses the pools through the argument block's cache pointers: with KV16 they are read as uint16_t again
    const ExtendArgs a{q, k_new, v_new, ldq, sbq, ldk, sbk, ldv, sbv, reinterpret_cast<float*>(k_pool), reinterpret_cast<float*>(v_pool), ldc, 0,
                       pos, 1, count, o, ldo, sbo, p, int(heads), int(capacity), int(m), scale, mask, sbm, rt().status_dev, nullptr, 0,
                       block_table, int(max_blocks), int(num_blocks), int(log2_block)};
    const dim3 grid{unsigned((m + 31) / 32), unsigned(heads), unsigned(batch)};
    const int Cp = round32(a.capacity);
    rc = D == 64 ? launch_extend_body(&attn_paged_bf16<64>, size_t(attn_paged_lds_floats<64>(Cp)) * 4, a, grid)
                 : launch_extend_body(&attn_paged_bf16<32>, size_t(attn_paged_lds_floats<32>(Cp)) * 4, a, grid);
    if (rc != LG_OK) return rc;
    LG_CHECK_LAUNCH();
    return LG_OK;
}
