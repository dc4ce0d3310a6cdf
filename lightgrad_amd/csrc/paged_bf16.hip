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
// A file of its own: paged.hip holds exactly its two kernels with the code they had (tests/test_paged_registers.py).
// The bounds behaviour is the paged entry's: every table word of the reach checked in LDS before an address is formed, a bad
// position, count or word -> nothing of the element written, LG_STATUS_BAD_INDEX raised, the other elements computed.
#include "extend_body.h"

namespace lg {

template <int D>
__global__ void __launch_bounds__(256) attn_paged_bf16(const ExtendArgs a) { attn_extend_body<D, false, true, true>(a); }

template <int D>
static int launch_paged_bf16(const ExtendArgs& a, dim3 grid) {
    const size_t bytes = size_t(attn_paged_lds_floats<D>(round32(a.capacity))) * 4;
    int rc = allow_lds(&attn_paged_bf16<D>, bytes);
    if (rc != LG_OK) return rc;
    hipLaunchKernelGGL(attn_paged_bf16<D>, grid, dim3(256), bytes, rt().stream, a);
    return LG_OK;
}

}  // namespace lg

using namespace lg;

extern "C" int lg_attention_extend_paged_bf16_f32(const float* q, int64_t ldq, int64_t sbq, const float* k_new, int64_t ldk, int64_t sbk,
                                                  const float* v_new, int64_t ldv, int64_t sbv, uint16_t* k_pool, uint16_t* v_pool, int64_t ldc,
                                                  const int32_t* pos, const int32_t* count, const int32_t* block_table, float* o, int64_t ldo,
                                                  int64_t sbo, float* p, int64_t batch, int64_t heads, int64_t m, int64_t max_blocks,
                                                  int64_t num_blocks, int64_t log2_block, int64_t D, float scale, const float* mask, int64_t sbm) {
    LG_REQUIRE_INIT();
    const char* name = "lg_attention_extend_paged_bf16_f32";
    LG_ARG(log2_block >= 2 && log2_block <= 7 && max_blocks >= 1 && max_blocks <= kPagedMaxTable && (max_blocks << log2_block) <= kExtMaxKeys,
           "%s: blocks of 1 << %lld rows (4 .. 128) and %lld of them per table (capacity 1 .. 512) unsupported", name, (long long)log2_block,
           (long long)max_blocks);
    const int64_t B = int64_t(1) << log2_block, capacity = max_blocks * B;
    LG_ARG(lg_attention_extend_supported(m, capacity, D), "%s: m = %lld (1 .. capacity), capacity = %lld (1 .. 512), D = %lld (32 or 64) unsupported",
           name, (long long)m, (long long)capacity, (long long)D);
    LG_ARG(num_blocks >= 1 && num_blocks * B < (int64_t(1) << 31), "%s: a pool of %lld blocks of %lld rows (1 .. 2^31 - 1 rows) unsupported", name,
           (long long)num_blocks, (long long)B);
    LG_ARG(batch >= 0 && heads >= 1 && batch <= 65535 && heads <= 65535, "%s: bad batch / heads", name);
    if (batch == 0) return LG_OK;
    LG_ARG(extend_operand(q, ldq, sbq) && extend_operand(k_new, ldk, sbk) && extend_operand(v_new, ldv, sbv) && extend_operand(o, ldo, sbo) && pos &&
               (reinterpret_cast<uintptr_t>(pos) & 3u) == 0 && aligned16(p),
           "%s: operands must be non-NULL and 16-byte aligned with pitches that are non-negative multiples of 4", name);
    // a lane loads and stores 4 pool words = 8 bytes at once
    LG_ARG(k_pool && v_pool && (reinterpret_cast<uintptr_t>(k_pool) & 7u) == 0 && (reinterpret_cast<uintptr_t>(v_pool) & 7u) == 0 && ldc >= 0 && ldc % 4 == 0,
           "%s: the bfloat16 pools must be non-NULL and 8-byte aligned with a row pitch that is a non-negative multiple of 4 elements (the float32 pools "
           "go to lg_attention_extend_paged_f32)", name);
    LG_ARG(count && (reinterpret_cast<uintptr_t>(count) & 3u) == 0 && block_table && (reinterpret_cast<uintptr_t>(block_table) & 3u) == 0,
           "%s: count and block_table must be non-NULL and 4-byte aligned", name);
    const int64_t w = heads * D, rows = num_blocks * B;
    LG_ARG(ldc >= w, "%s: pool row pitch %lld below heads * D = %lld", name, (long long)ldc, (long long)w);
    LG_ARG(!mask || sbm == 0 || sbm >= capacity, "%s: mask batch pitch %lld is neither 0 (one row for the batch) nor >= capacity", name,
           (long long)sbm);
    {
        // what the launch writes - the pools (2 bytes an element), o, p - shares no byte with any other operand it reads or writes
        const void* ptr[9] = {k_pool, v_pool, o, p, k_new, v_new, pos, count, block_table};
        const char* what[9] = {"k_pool", "v_pool", "o", "p", "k_new", "v_new", "pos", "count", "block_table"};
        const int64_t bytes[9] = {((rows - 1) * ldc + w) * 2, ((rows - 1) * ldc + w) * 2, ((batch - 1) * sbo + (m - 1) * ldo + w) * 4,
                                  batch * heads * m * capacity * 4, ((batch - 1) * sbk + (m - 1) * ldk + w) * 4,
                                  ((batch - 1) * sbv + (m - 1) * ldv + w) * 4, batch * 4, batch * 4, batch * max_blocks * 4};
        for (int i = 0; i < 4; ++i)
            for (int j = i + 1; j < 9; ++j)
                LG_ARG(!bytes_overlap(ptr[i], bytes[i], ptr[j], bytes[j]), "%s: %s overlaps %s: the launch writes the one while other workgroups use the other",
                       name, what[i], what[j]);
        LG_ARG(!bytes_overlap(pos, bytes[6], count, bytes[7]), "%s: count overlaps pos", name);
    }
    {
        const int64_t orows[3] = {batch, m, w}, row_strides[3] = {sbo, ldo, 1};
        int rc = adam_epilogue_check_strided(o, 4, 3, orows, row_strides);
        if (rc != LG_OK) return rc;
        const int64_t crows[2] = {rows, w}, strides[2] = {ldc, 1};
        rc = adam_epilogue_check_strided(k_pool, 2, 2, crows, strides);
        if (rc != LG_OK) return rc;
        rc = adam_epilogue_check_strided(v_pool, 2, 2, crows, strides);
        if (rc != LG_OK) return rc;
        if (p) { rc = adam_epilogue_check_write(p, batch * heads * m * capacity * 4); if (rc != LG_OK) return rc; }
    }
    // the body addresses the pools through the argument block's cache pointers: with KV16 they are read as uint16_t again
    const ExtendArgs a{q, k_new, v_new, ldq, sbq, ldk, sbk, ldv, sbv, reinterpret_cast<float*>(k_pool), reinterpret_cast<float*>(v_pool), ldc, 0,
                       pos, 1, count, o, ldo, sbo, p, int(heads), int(capacity), int(m), scale, mask, sbm, rt().status_dev, nullptr, 0,
                       block_table, int(max_blocks), int(num_blocks), int(log2_block)};
    const dim3 grid{unsigned((m + 31) / 32), unsigned(heads), unsigned(batch)};
    const int rc = D == 64 ? launch_paged_bf16<64>(a, grid) : launch_paged_bf16<32>(a, grid);
    if (rc != LG_OK) return rc;
    LG_CHECK_LAUNCH();
    return LG_OK;
}
