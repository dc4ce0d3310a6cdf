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
// The body, attn_extend_body<D, PACKED, PAGED>, and the host checks live in extend_body.h: paged.hip instantiates the body once
// more with the caches reached through a block table (lg_attention_extend_paged_f32); this file keeps its four kernels.
#include "extend_body.h"

namespace lg {

template <int D>
__global__ void __launch_bounds__(256) attn_extend(const ExtendArgs a) { attn_extend_body<D, false>(a); }

template <int D>
__global__ void __launch_bounds__(256) attn_packed(const ExtendArgs a) { attn_extend_body<D, true>(a); }

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
