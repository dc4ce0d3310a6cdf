// Per-request repetition, presence and frequency penalties and the minimum of new tokens, IN PLACE on fp32 logits (C ABI and
// definition: include/lghip.h, lightgrad_amd/random.py `penalize_logits`).  ONE launch for all rows, between the head
// and the draw; every operand is device state, so a captured step replays it as it stands.
//
// One workgroup of 256 threads per row of logits.  Every thread reads the row's request i = index[row], the 4 table words,
// prompt_len[i] and out_len[i] from the same addresses - uniform values, no barrier - and the workgroup branches uniformly: a free
// row (i < 0) and a row whose request, lengths or parameters are bad return before anything else is read.  Then
//   1. the history - prompts[i, :len] and out[i, :g], at most P + G <= 4096 ids - goes ONCE through a range check into an
//      open-addressing table in LDS: 2^k >= 2 (P + G) slots of (key, count), linear probing, the key claimed with an integer
//      compare-and-swap, the count (occurrences in `out` only) with an integer add.  Counts are integers: the arrival order cannot
//      change them.  Nothing has been stored to memory yet;
//   2. ONE barrier with a vote (__syncthreads_or) makes an id outside 0 .. V - 1 uniform: such a row writes nothing at all;
//   3. the threads walk the slots.  A key sits in exactly one slot, so exactly ONE thread reads logits[row, key], applies
//      x = x < 0 ? x * rho : x / rho, then (x - beta * float(c)) - alpha where c > 0, then -inf if the key is `eos` and g < min_new,
//      and stores it.  Thread 0 looks `eos` up in the table (read-only by now) and stores -inf itself only if it is in no slot: one
//      writer per address, no ordering between stores needed.
// The row of V logits is NOT streamed: the launch touches at most P + G + 1 floats of it, whatever the vocabulary.  -ffp-contract=off
// (Makefile) keeps x - beta * c unfused and `/` is the correctly rounded division: the results are the definition's bit for bit.
#include "common.h"

namespace lg {

constexpr int kPenalizeThreads = 256;
constexpr int kPenalizeMaxHistory = 4096;         // P + G: speculate.hip's bound for a sequence in LDS
constexpr int kPenalizeMinSlots = 64;

__device__ __forceinline__ uint32_t penalize_hash(int32_t id, int log_slots) { return (uint32_t(id) * 2654435761u) >> (32 - log_slots); }

__global__ void __launch_bounds__(kPenalizeThreads) penalize_rows_kernel(float* __restrict__ logits, int64_t cols, int64_t pitch,
                                                                         const int32_t* __restrict__ table, int64_t n, const int32_t* __restrict__ index,
                                                                         const int32_t* __restrict__ prompts, int64_t ldp, int P,
                                                                         const int32_t* __restrict__ prompt_len, const int32_t* __restrict__ out, int64_t ldo,
                                                                         int G, const int32_t* __restrict__ out_len, int eos, int log_slots, int* status) {
    extern __shared__ __align__(16) int32_t penalize_dyn[];
    const int slots = 1 << log_slots, mask = slots - 1;
    int32_t* const keys = penalize_dyn;                                   // -1: an empty slot
    int32_t* const counts = penalize_dyn + slots;
    const int tid = threadIdx.x;
    const int64_t row = blockIdx.x;                                      // the grid is the rows

    const int32_t i = index[row];
    if (i < 0) return;                                                   // a free slot: its logits are not read
    bool bad = i >= n;
    int len = 0, g = 0, min_new = 0;
    float rho = 1.0f, alpha = 0.0f, beta = 0.0f;
    if (!bad) {
        const int4 w = reinterpret_cast<const int4*>(table)[i];
        len = prompt_len[i];
        g = out_len[i];
        rho = __int_as_float(w.x); alpha = __int_as_float(w.y); beta = __int_as_float(w.z); min_new = w.w;
        // rho finite, > 0, its sign clear: its bits as an int lie in (0, the bits of +inf); alpha and beta finite
        bad = len < 0 || len > P || g < 0 || g > G || w.x <= 0 || w.x >= 0x7F800000 || (w.y & 0x7FFFFFFF) >= 0x7F800000 ||
              (w.z & 0x7FFFFFFF) >= 0x7F800000 || min_new < 0;
    }
    if (bad) {                                                           // uniform: nothing of the row or its history is read
        if (tid == 0) __hip_atomic_fetch_or(status, LG_STATUS_BAD_INDEX, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
        return;
    }

    for (int s = tid; s < slots; s += kPenalizeThreads) { keys[s] = -1; counts[s] = 0; }
    __syncthreads();

    const int32_t* const own_prompt = prompts + int64_t(i) * ldp;
    const int32_t* const own_out = out + int64_t(i) * ldo;
    int bad_id = 0;
    for (int t = tid; t < len + g; t += kPenalizeThreads) {              // words behind len and behind g are never read
        const bool drawn = t >= len;
        const int32_t id = drawn ? own_out[t - len] : own_prompt[t];
        if (id < 0 || int64_t(id) >= cols) { bad_id = 1; continue; }
        uint32_t h = penalize_hash(id, log_slots);
        for (;;) {                                                       // at most P + G distinct keys in >= 2 (P + G) slots: it ends
            const int32_t before = atomicCAS(&keys[h], -1, id);
            if (before == -1 || before == id) break;
            h = (h + 1) & uint32_t(mask);
        }
        if (drawn) atomicAdd(&counts[h], 1);
    }
    if (__syncthreads_or(bad_id)) {                                      // uniform, and before the first store: a bad row writes nothing
        if (tid == 0) __hip_atomic_fetch_or(status, LG_STATUS_BAD_INDEX, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
        return;
    }

    float* const x_row = logits + row * pitch;
    const bool no_eos_yet = eos >= 0 && g < min_new;
    for (int s = tid; s < slots; s += kPenalizeThreads) {
        const int32_t key = keys[s];
        if (key < 0) continue;
        const int32_t c = counts[s];
        float x = x_row[key];
        x = x < 0.0f ? x * rho : x / rho;
        if (c > 0) x = (x - beta * float(c)) - alpha;
        if (no_eos_yet && key == eos) x = -INFINITY;
        x_row[key] = x;
    }
    if (no_eos_yet && tid == 0) {                                        // `eos` outside the history: nobody above wrote it
        uint32_t h = penalize_hash(eos, log_slots);
        int32_t key = keys[h];
        while (key != -1 && key != eos) { h = (h + 1) & uint32_t(mask); key = keys[h]; }
        if (key == -1) x_row[eos] = -INFINITY;
    }
}

}  // namespace lg

using namespace lg;

extern "C" int lg_penalize_rows_f32(float* logits, int64_t rows, int64_t cols, int64_t row_pitch, const int32_t* table, int64_t n,
                                    const int32_t* index, const int32_t* prompts, int64_t prompt_pitch, int64_t P, const int32_t* prompt_len,
                                    const int32_t* out, int64_t out_pitch, int64_t G, const int32_t* out_len, int32_t eos) {
    LG_REQUIRE_INIT();
    if (rows == 0) return LG_OK;                         // nothing to penalise: nothing is checked, nothing is launched
    LG_ARG(rows >= 1 && rows <= 65535, "lg_penalize_rows_f32: rows = %lld outside [0, 65535]", (long long)rows);
    LG_ARG(cols >= 1 && cols < (int64_t(1) << 31), "lg_penalize_rows_f32: cols = %lld outside [1, 2^31)", (long long)cols);
    LG_ARG(row_pitch >= cols, "lg_penalize_rows_f32: row_pitch = %lld below cols = %lld", (long long)row_pitch, (long long)cols);
    LG_ARG(n >= 1 && n < (int64_t(1) << 31), "lg_penalize_rows_f32: a table of n = %lld rows, outside [1, 2^31)", (long long)n);
    LG_ARG(P >= 1 && G >= 1, "lg_penalize_rows_f32: prompts of P = %lld and out of G = %lld columns, each at least 1", (long long)P, (long long)G);
    LG_ARG(P + G <= kPenalizeMaxHistory, "lg_penalize_rows_f32: a history of P + G = %lld + %lld ids exceeds the %d the launch keeps in LDS",
           (long long)P, (long long)G, kPenalizeMaxHistory);
    LG_ARG(prompt_pitch >= P && out_pitch >= G, "lg_penalize_rows_f32: prompt_pitch = %lld below P = %lld, or out_pitch = %lld below G = %lld",
           (long long)prompt_pitch, (long long)P, (long long)out_pitch, (long long)G);
    LG_ARG(eos >= -1 && int64_t(eos) < cols, "lg_penalize_rows_f32: eos = %d is neither -1 (none) nor an id below cols = %lld", int(eos), (long long)cols);
    LG_ARG(logits != nullptr && table != nullptr && index != nullptr && prompts != nullptr && prompt_len != nullptr && out != nullptr && out_len != nullptr,
           "lg_penalize_rows_f32: NULL pointer");
    const auto word_aligned = [](const void* p) { return (reinterpret_cast<uintptr_t>(p) & 3u) == 0; };
    LG_ARG(word_aligned(logits) && aligned16(table) && word_aligned(index) && word_aligned(prompts) && word_aligned(prompt_len) && word_aligned(out) &&
               word_aligned(out_len),
           "lg_penalize_rows_f32: a misaligned operand (the table: 16 bytes; everything else: 4)");
    const int64_t logit_bytes = ((rows - 1) * row_pitch + cols) * 4;
    const void* const words[6] = {table, index, prompts, prompt_len, out, out_len};
    const int64_t bytes[6] = {n * 16, rows * 4, ((n - 1) * prompt_pitch + P) * 4, n * 4, ((n - 1) * out_pitch + G) * 4, n * 4};
    for (int k = 0; k < 6; ++k)
        LG_ARG(!bytes_overlap(logits, logit_bytes, words[k], bytes[k]),
               "lg_penalize_rows_f32: the logits overlap operand %d (of table, index, prompts, prompt_len, out, out_len)", k);
    { const int rc = adam_epilogue_check_write(logits, logit_bytes); if (rc != LG_OK) return rc; }
    int log_slots = 6;                                   // 2^k >= 2 (P + G), at least kPenalizeMinSlots: at most 8192 slots, 64 KiB
    while ((int64_t(1) << log_slots) < 2 * (P + G)) ++log_slots;
    static_assert(kPenalizeMinSlots == 64, "log_slots starts at 6");
    const size_t lds = size_t(2) * sizeof(int32_t) << log_slots;
    const hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(&penalize_rows_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, int(lds));
    if (e != hipSuccess) { set_error("lg_penalize_rows_f32: %zu bytes of LDS refused: %s", lds, hipGetErrorString(e)); return LG_EHIP; }
    hipLaunchKernelGGL(penalize_rows_kernel, dim3{unsigned(rows)}, dim3(kPenalizeThreads), lds, rt().stream, logits, cols, row_pitch, table, n, index, prompts,
                       prompt_pitch, int(P), prompt_len, out, out_pitch, int(G), out_len, int(eos), log_slots, rt().status_dev);
    LG_CHECK_LAUNCH();
    return LG_OK;
}
