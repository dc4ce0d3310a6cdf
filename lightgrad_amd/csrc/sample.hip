// Sampled decoding: one token per row of fp32 logits with temperature, top-k and top-p, in ONE launch, from the counter-based
// random stream of dropout.hip (C ABI and definition: include/lghip.h, lightgrad_amd/random.py `sample_tokens`).
//
// One workgroup per row.  The row is staged once into LDS with 16-byte loads from its first aligned element (kernel 0: every
// row of at most kSampleMaxLdsCols floats - a 30522-wide vocabulary is 122 KB of the CU's 160 KiB), as order-preserving 32-bit
// KEYS of its values (-0.0 canonicalised to +0.0), and every later pass reads the keys from there; a wider row takes the same
// passes from memory (kernel 1).  The passes:
//   1. max and argmax with the combine of argreduce.hip (`beats`), on the values in flight while the row is staged (a pass of
//      its own in kernel 1): a row with a NaN, +inf or an all -inf row answers that argmax and is done;
//   2. top-k: the k-th largest value by a radix select on the keys - three passes of 11, 11 and 10 bits from the top down, 2048
//      bins holding COUNTS;
//   3. W, the sum of the weights q over K;
//   4. top-p: the same three-pass select with the bins holding MASS, which gives the largest value whose mass at or above it
//      reaches top_p * W;
//   5. a blocked scan in index order over N: each thread sums a contiguous run, the runs are scanned over the wave and the
//      workgroup, and the one thread whose run holds the target walks it to the token.
// A pass costs what its instructions per element cost on ONE CU (about 0.2 us per instruction and element at 30522 columns), which
// is why the keys are staged, the row is read four elements at a time without a test per element, and members of K are told by
// one integer compare.
//
// FIXED POINT.  A weight is q_j = floor(2^shift * __expf((x_j - m) * inv_T)), a 64-bit integer (shift = 40 for every row of
// fewer than 2^22 elements: each q is exact to 2^-40 of the largest weight, which is exactly 2^shift).  Counts, W, the bins'
// masses and the running sums are then INTEGER sums: exact in any order, so the LDS atomics that fill the bins and every fold
// give the same bits on every run without any fixed order, and the scan compares C_i * 2^25 >= (2h + 1) * W' exactly (u = (2h +
// 1) / 2^25 with h the top 24 bits of the row's word), which always has a solution.  No running fp32 sum exists anywhere.
//
// Seed and `draws` are read by the kernel with dropout_fwd's protocol (read, two-level tickets, the last arriver advances): a
// captured decode step draws fresh numbers at every replay, and no host scalar depends on the data.
//
// The row body and what it stands on live in sample_body.h, which sample_rows.hip (a set of parameters and a stream per row)
// instantiates as well; this file keeps the launch that draws from the global stream: its two kernels and the ticket protocol.
#include "sample_body.h"

namespace lg {

template <bool LDS, typename OutT>
__global__ void __launch_bounds__(1024) sample_kernel(const float* __restrict__ logits, int64_t rows, int64_t cols, int64_t pitch, float inv_t,
                                                      int64_t top_k, double top_p, float scale, OutT* __restrict__ out, u64* state,
                                                      u64* base_out, int group) {
    extern __shared__ __align__(16) unsigned char sample_dyn[];
    SampleShared& sh = *reinterpret_cast<SampleShared*>(sample_dyn);
    const int tid = threadIdx.x;

    // the stream: thread 0 reads the call, takes its ticket and - as the last arriver - advances `draws`
    int* const tickets = rng_tickets(state);
    if (tid == 0) {
        rng_read_call(state, sh.call);                                   // `draws` is in a register before the ticket below is taken
        if (blockIdx.x == 0) base_out[0] = sh.call[1];
    }
    __syncthreads();
    const u64 seed = rng_uniform64(sh.call[0]), base = rng_uniform64(sh.call[1]);
    if (tid == 0) {
        const int grp = blockIdx.x / group, groups = (gridDim.x + group - 1) / group;
        int* const mine = tickets + (1 + grp) * kRngLine;
        const int order = rng_take_ticket(mine);
        rng_last_arriver_advances(state, tickets, mine, order, grp, groups, group, int(gridDim.x), base);
    }
    const int64_t row = blockIdx.x;
    if (row >= rows) return;                                             // rows == 0: the one workgroup only advances `draws`
    // row r of the call with draws == base: the block of counter (r, base) under the key `seed`
    sample_row_body<LDS, false, OutT>(sample_dyn, logits + row * pitch, row, cols, inv_t, top_k, top_p, scale, out, uint32_t(row),
                                      uint32_t(u64(row) >> 32), uint32_t(base), uint32_t(base >> 32), uint32_t(seed), uint32_t(seed >> 32));
}

// ---- host --------------------------------------------------------------------------------------------------------------------------
static thread_local int32_t g_sample_plan[4] = {-1, 0, 0, 0};

void note_sample_plan(int kernel, int threads, int passes, int vec) {
    g_sample_plan[0] = kernel; g_sample_plan[1] = threads; g_sample_plan[2] = passes; g_sample_plan[3] = vec;
}

template <bool LDS, typename OutT>
static int launch_sample(dim3 grid, dim3 block, size_t lds, const float* logits, int64_t rows, int64_t cols, int64_t pitch, float inv_t,
                         int64_t top_k, double top_p, float scale, void* out, u64* base_out) {
    const hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(&sample_kernel<LDS, OutT>), hipFuncAttributeMaxDynamicSharedMemorySize,
                                             int(lds));
    if (e != hipSuccess) { set_error("lg_sample_f32: %zu bytes of LDS refused: %s", lds, hipGetErrorString(e)); return LG_EHIP; }
    hipLaunchKernelGGL((sample_kernel<LDS, OutT>), grid, block, lds, rt().stream, logits, rows, cols, pitch, inv_t, top_k, top_p, scale,
                       static_cast<OutT*>(out), rt().rng_state, base_out, rng_group(grid.x));
    return LG_OK;
}

}  // namespace lg

using namespace lg;

extern "C" int lg_sample_f32(const float* logits, int64_t rows, int64_t cols, int64_t row_pitch, double temperature, int64_t top_k,
                             double top_p, void* out, int out_itemsize, uint64_t* base_out) {
    LG_REQUIRE_INIT();
    note_sample_plan(-1, 0, 0, 0);                       // until a kernel is launched: refused calls
    LG_ARG(out_itemsize == 4 || out_itemsize == 8, "lg_sample_f32: the tokens are int32 or int64 (itemsize %d)", out_itemsize);
    LG_ARG(rows >= 0 && rows <= (int64_t(1) << 24), "lg_sample_f32: rows = %lld outside [0, 2^24]", (long long)rows);
    LG_ARG(cols >= 1 && cols < (int64_t(1) << 31), "lg_sample_f32: cols = %lld outside [1, 2^31)", (long long)cols);
    LG_ARG(row_pitch >= cols, "lg_sample_f32: row_pitch = %lld below cols = %lld", (long long)row_pitch, (long long)cols);
    LG_ARG(base_out != nullptr && (rows == 0 || (logits != nullptr && out != nullptr)), "lg_sample_f32: NULL pointer");
    LG_ARG(temperature > 0.0 && std::isfinite(temperature) && std::isfinite(float(1.0 / temperature)),
           "lg_sample_f32: temperature = %g must be positive and finite, with 1 / temperature finite in float", temperature);
    LG_ARG(top_k >= 0, "lg_sample_f32: top_k = %lld is negative (0: off)", (long long)top_k);
    LG_ARG(top_p > 0.0 && top_p <= 1.0, "lg_sample_f32: top_p = %g outside (0, 1] (1: off)", top_p);
    { const int rc = adam_epilogue_check_write(out, rows * out_itemsize); if (rc != LG_OK) return rc; }
    const float inv_t = float(1.0 / temperature);
    const SampleShape shape = sample_shape(cols);
    const float scale = shape.scale;
    const bool lds_row = shape.lds_row;
    const int threads = shape.threads, vec = shape.vec;
    const size_t lds = shape.lds;
    const bool select_k = top_k >= 1 && top_k < cols, select_p = top_p < 1.0;
    const int passes = 1 + (select_k ? 3 : 0) + (select_p ? 4 : 0) + 2;  // (kernel 0 finds the maximum while it stages the row)
    const dim3 grid(unsigned(rows < 1 ? 1 : rows)), block(threads);      // no rows: one workgroup, which advances `draws`
    u64* const base = reinterpret_cast<u64*>(base_out);
    int rc;
    if (lds_row)
        rc = out_itemsize == 4 ? launch_sample<true, int32_t>(grid, block, lds, logits, rows, cols, row_pitch, inv_t, top_k, top_p, scale, out, base)
                               : launch_sample<true, int64_t>(grid, block, lds, logits, rows, cols, row_pitch, inv_t, top_k, top_p, scale, out, base);
    else
        rc = out_itemsize == 4 ? launch_sample<false, int32_t>(grid, block, lds, logits, rows, cols, row_pitch, inv_t, top_k, top_p, scale, out, base)
                               : launch_sample<false, int64_t>(grid, block, lds, logits, rows, cols, row_pitch, inv_t, top_k, top_p, scale, out, base);
    if (rc != LG_OK) return rc;
    note_sample_plan(lds_row ? 0 : 1, threads, passes, vec);
    LG_CHECK_LAUNCH();
    return LG_OK;
}

extern "C" int lg_sample_last_plan(int32_t out[4]) {
    LG_ARG(out != nullptr, "lg_sample_last_plan: NULL pointer");
    for (int k = 0; k < 4; ++k) out[k] = g_sample_plan[k];
    return LG_OK;
}
