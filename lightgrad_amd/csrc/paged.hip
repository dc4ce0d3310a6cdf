// The extend launch against a PAGED key / value cache (gfx950, fp32 MFMA): lg_attention_extend_paged_f32.
//
// lg_attention_extend_counts_f32 (extend.hip) with the caches reached through a table of fixed-size blocks: the keys and values of
// every layer lie in a POOL of num_blocks blocks of B = 1 << log2_block rows, and word n of row b of `block_table` (batch,
// max_blocks) names the block that holds positions n * B .. n * B + B - 1 of batch element b.  Position j of element b is pool
// row block_table[b, j >> log2_block] * B + (j & (B - 1)): for the streamed keys j < t and for the count[b] new rows the launch
// writes at t ..; capacity = max_blocks * B.  Everything else is the counts entry - the kernel body is the same text
// (extend_body.h, attn_extend_body<D, false, PAGED = true>): grid, LDS tile, chunks of 128 keys, fold order, softmax, the +0.0
// rows, p, the mask over logical positions, the status flag.  So element b is computed bit for bit as the counts entry computes
// it on a contiguous (capacity, width) cache that holds the same rows.
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

template <int D>
static int launch_paged(const ExtendArgs& a, dim3 grid) {
    const size_t bytes = size_t(attn_paged_lds_floats<D>(round32(a.capacity))) * 4;
    int rc = allow_lds(&attn_paged<D>, bytes);
    if (rc != LG_OK) return rc;
    hipLaunchKernelGGL(attn_paged<D>, grid, dim3(256), bytes, rt().stream, a);
    return LG_OK;
}

}  // namespace lg

using namespace lg;

extern "C" int lg_attention_extend_paged_f32(const float* q, int64_t ldq, int64_t sbq, const float* k_new, int64_t ldk, int64_t sbk,
                                             const float* v_new, int64_t ldv, int64_t sbv, float* k_pool, float* v_pool, int64_t ldc,
                                             const int32_t* pos, const int32_t* count, const int32_t* block_table, float* o, int64_t ldo,
                                             int64_t sbo, float* p, int64_t batch, int64_t heads, int64_t m, int64_t max_blocks,
                                             int64_t num_blocks, int64_t log2_block, int64_t D, float scale, const float* mask, int64_t sbm) {
    LG_REQUIRE_INIT();
    const char* name = "lg_attention_extend_paged_f32";
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
    LG_ARG(extend_operand(q, ldq, sbq) && extend_operand(k_new, ldk, sbk) && extend_operand(v_new, ldv, sbv) && extend_operand(k_pool, ldc, 0) &&
               extend_operand(v_pool, ldc, 0) && extend_operand(o, ldo, sbo) && pos && (reinterpret_cast<uintptr_t>(pos) & 3u) == 0 && aligned16(p),
           "%s: operands must be non-NULL and 16-byte aligned with pitches that are non-negative multiples of 4", name);
    LG_ARG(count && (reinterpret_cast<uintptr_t>(count) & 3u) == 0 && block_table && (reinterpret_cast<uintptr_t>(block_table) & 3u) == 0,
           "%s: count and block_table must be non-NULL and 4-byte aligned", name);
    const int64_t w = heads * D, rows = num_blocks * B;
    LG_ARG(ldc >= w, "%s: pool row pitch %lld below heads * D = %lld", name, (long long)ldc, (long long)w);
    LG_ARG(!mask || sbm == 0 || sbm >= capacity, "%s: mask batch pitch %lld is neither 0 (one row for the batch) nor >= capacity", name,
           (long long)sbm);
    {
        // what the launch writes - the pools, o, p - shares no byte with any other operand it reads or writes: other workgroups of
        // the launch read the new rows, the positions, the counts and the tables while the pools are written
        const void* ptr[9] = {k_pool, v_pool, o, p, k_new, v_new, pos, count, block_table};
        const char* what[9] = {"k_pool", "v_pool", "o", "p", "k_new", "v_new", "pos", "count", "block_table"};
        const int64_t bytes[9] = {((rows - 1) * ldc + w) * 4, ((rows - 1) * ldc + w) * 4, ((batch - 1) * sbo + (m - 1) * ldo + w) * 4,
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
        rc = adam_epilogue_check_strided(k_pool, 4, 2, crows, strides);
        if (rc != LG_OK) return rc;
        rc = adam_epilogue_check_strided(v_pool, 4, 2, crows, strides);
        if (rc != LG_OK) return rc;
        if (p) { rc = adam_epilogue_check_write(p, batch * heads * m * capacity * 4); if (rc != LG_OK) return rc; }
    }
    const ExtendArgs a{q, k_new, v_new, ldq, sbq, ldk, sbk, ldv, sbv, k_pool, v_pool, ldc, 0, pos, 1, count, o, ldo, sbo, p,
                       int(heads), int(capacity), int(m), scale, mask, sbm, rt().status_dev, nullptr, 0,
                       block_table, int(max_blocks), int(num_blocks), int(log2_block)};
    const dim3 grid{unsigned((m + 31) / 32), unsigned(heads), unsigned(batch)};
    const int rc = D == 64 ? launch_paged<64>(a, grid) : launch_paged<32>(a, grid);
    if (rc != LG_OK) return rc;
    LG_CHECK_LAUNCH();
    return LG_OK;
}
