// Per-request sampling: one token per row of fp32 logits, every row with the temperature, top-k, top-p, SEED and COUNTER of a table
// row of its own (C ABI and definition: include/lghip.h, lightgrad_amd/random.py `sample_tokens_rows`).  The row body
// is sample.hip's (sample_body.h): for equal (inv_T, top_k, top_p, u) the token is that launch's bit for bit.
//
// One workgroup per row.  Thread 0 reads index[row], then - for 0 <= i < n - the 8 words of table row i (two 16-byte loads) and
// counter[i], checks them and leaves them in SampleShared; the workgroup branches uniformly behind the one barrier:
//   * i < 0 (a free slot) answers 0, a BAD row (i >= n, a negative counter, top_k < 0, top_p outside (0, 1], inv_T with its sign
//     set, NaN or infinite) answers 0 and raises LG_STATUS_BAD_INDEX - both before any load of the logits;
//   * inv_T == +0.0 is GREEDY: the body returns the argmax where a degenerate row returns it;
//   * otherwise the row draws u from word 0 of philox4x32_10((lo32(g), hi32(g), 0, 0), key(seed)), g = counter[i].
// The global (seed, draws) state is neither read nor advanced: no ticket protocol, no rng_state.  What a row answers depends on
// its logits and its table row alone - not on its position in the launch, nor on the other rows.
#include "sample_body.h"

namespace lg {

constexpr int kSampleRowDraw = 0, kSampleRowFree = 1, kSampleRowBad = 2;

template <bool LDS, typename OutT>
__global__ void __launch_bounds__(1024) sample_rows_kernel(const float* __restrict__ logits, int64_t cols, int64_t pitch,
                                                           const int32_t* __restrict__ table, int64_t n, const int32_t* __restrict__ index,
                                                           const int32_t* __restrict__ counter, float scale, OutT* __restrict__ out, int* status) {
    extern __shared__ __align__(16) unsigned char sample_dyn[];
    SampleShared& sh = *reinterpret_cast<SampleShared*>(sample_dyn);
    const int tid = threadIdx.x;
    const int64_t row = blockIdx.x;                                      // the grid is the rows

    if (tid == 0) {
        const int32_t i = index[row];
        int kind = i < 0 ? kSampleRowFree : i >= n ? kSampleRowBad : kSampleRowDraw;
        if (kind == kSampleRowDraw) {
            const int4* const t4 = reinterpret_cast<const int4*>(table) + 2 * int64_t(i);
            const int4 a = t4[0], b = t4[1];
            const int32_t g = counter[i];
            const float inv_t = __int_as_float(a.x);
            const double top_p = __longlong_as_double((long long)((u64(uint32_t(a.w)) << 32) | uint32_t(a.z)));
            const bool ok = g >= 0 && a.y >= 0 && top_p > 0.0 && top_p <= 1.0 && a.x >= 0 && inv_t == inv_t && inv_t != INFINITY;
            kind = ok ? kSampleRowDraw : kSampleRowBad;
            sh.row_words[0] = a.x; sh.row_words[1] = a.y; sh.row_words[2] = a.z; sh.row_words[3] = a.w;
            sh.row_words[4] = b.x; sh.row_words[5] = b.y; sh.row_words[6] = b.z; sh.row_words[7] = b.w;
            sh.row_counter = g;
        }
        sh.row_kind = kind;
        if (kind != kSampleRowDraw) out[row] = OutT(0);
        if (kind == kSampleRowBad) __hip_atomic_fetch_or(status, LG_STATUS_BAD_INDEX, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
    }
    __syncthreads();
    if (sh.row_kind != kSampleRowDraw) return;                           // uniform: nothing of the logits is read

    // uniform values out of LDS into scalar registers
    const auto word = [&](int k) { return uint32_t(__builtin_amdgcn_readfirstlane(sh.row_words[k])); };
    const float inv_t = __uint_as_float(word(0));
    const int64_t top_k = int64_t(int32_t(word(1)));
    const double top_p = __longlong_as_double((long long)((u64(word(3)) << 32) | word(2)));
    const uint32_t g = uint32_t(__builtin_amdgcn_readfirstlane(sh.row_counter));       // >= 0: its high half is 0
    sample_row_body<LDS, true, OutT>(sample_dyn, logits + row * pitch, row, cols, inv_t, top_k, top_p, scale, out, g, 0u, 0u, 0u, word(4), word(5));
}

template <bool LDS, typename OutT>
static int launch_sample_rows(dim3 grid, dim3 block, size_t lds, const float* logits, int64_t cols, int64_t pitch, const int32_t* table, int64_t n,
                              const int32_t* index, const int32_t* counter, float scale, void* out) {
    const hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(&sample_rows_kernel<LDS, OutT>),
                                             hipFuncAttributeMaxDynamicSharedMemorySize, int(lds));
    if (e != hipSuccess) { set_error("lg_sample_rows_f32: %zu bytes of LDS refused: %s", lds, hipGetErrorString(e)); return LG_EHIP; }
    hipLaunchKernelGGL((sample_rows_kernel<LDS, OutT>), grid, block, lds, rt().stream, logits, cols, pitch, table, n, index, counter, scale,
                       static_cast<OutT*>(out), rt().status_dev);
    return LG_OK;
}

}  // namespace lg

using namespace lg;

extern "C" int lg_sample_rows_f32(const float* logits, int64_t rows, int64_t cols, int64_t row_pitch, const int32_t* table, int64_t n,
                                  const int32_t* index, const int32_t* counter, void* out, int out_itemsize) {
    LG_REQUIRE_INIT();
    note_sample_plan(-1, 0, 0, 0);                       // until a kernel is launched: refused calls
    LG_ARG(out_itemsize == 4 || out_itemsize == 8, "lg_sample_rows_f32: the tokens are int32 or int64 (itemsize %d)", out_itemsize);
    LG_ARG(rows >= 0 && rows <= (int64_t(1) << 24), "lg_sample_rows_f32: rows = %lld outside [0, 2^24]", (long long)rows);
    LG_ARG(cols >= 1 && cols < (int64_t(1) << 31), "lg_sample_rows_f32: cols = %lld outside [1, 2^31)", (long long)cols);
    LG_ARG(row_pitch >= cols, "lg_sample_rows_f32: row_pitch = %lld below cols = %lld", (long long)row_pitch, (long long)cols);
    LG_ARG(n >= 1 && n < (int64_t(1) << 31), "lg_sample_rows_f32: a table of n = %lld rows, outside [1, 2^31)", (long long)n);
    LG_ARG(logits != nullptr && table != nullptr && index != nullptr && counter != nullptr && out != nullptr, "lg_sample_rows_f32: NULL pointer");
    LG_ARG((reinterpret_cast<uintptr_t>(logits) & 3u) == 0 && aligned16(table) && (reinterpret_cast<uintptr_t>(index) & 3u) == 0 &&
               (reinterpret_cast<uintptr_t>(counter) & 3u) == 0 && (reinterpret_cast<uintptr_t>(out) & uintptr_t(out_itemsize - 1)) == 0,
           "lg_sample_rows_f32: a misaligned operand (the table: 16 bytes; logits, index, counter: 4; the tokens: their size)");
    const int64_t out_bytes = rows * out_itemsize;
    if (rows > 0) {
        const int64_t logit_bytes = ((rows - 1) * row_pitch + cols) * 4;
        LG_ARG(!bytes_overlap(out, out_bytes, logits, logit_bytes) && !bytes_overlap(out, out_bytes, table, n * 32) &&
                   !bytes_overlap(out, out_bytes, index, rows * 4) && !bytes_overlap(out, out_bytes, counter, n * 4),
               "lg_sample_rows_f32: the tokens overlap an operand");
    }
    { const int rc = adam_epilogue_check_write(out, out_bytes); if (rc != LG_OK) return rc; }
    if (rows == 0) return LG_OK;                         // nothing to draw and no stream to advance: nothing is launched
    const SampleShape shape = sample_shape(cols);
    const dim3 grid{unsigned(rows)}, block(shape.threads);
    int rc;
    if (shape.lds_row)
        rc = out_itemsize == 4 ? launch_sample_rows<true, int32_t>(grid, block, shape.lds, logits, cols, row_pitch, table, n, index, counter, shape.scale, out)
                               : launch_sample_rows<true, int64_t>(grid, block, shape.lds, logits, cols, row_pitch, table, n, index, counter, shape.scale, out);
    else
        rc = out_itemsize == 4 ? launch_sample_rows<false, int32_t>(grid, block, shape.lds, logits, cols, row_pitch, table, n, index, counter, shape.scale, out)
                               : launch_sample_rows<false, int64_t>(grid, block, shape.lds, logits, cols, row_pitch, table, n, index, counter, shape.scale, out);
    if (rc != LG_OK) return rc;
    // the passes of a sampled row with every filter the table COULD turn on (max, top-k, W + top-p, the scan); none is added for a greedy row
    note_sample_plan(shape.lds_row ? 0 : 1, shape.threads, 1 + 3 + 4 + 2, shape.vec);
    LG_CHECK_LAUNCH();
    return LG_OK;
}
