// Per-token log-probabilities and the top-n alternatives of a serving step (C ABI and definition: include/lghip.h,
// lightgrad_amd/random.py `token_logprobs_rows`).  ONE launch for all rows, behind the draw and in front of the commit;
// every operand is device state, so a captured step replays it as it stands.
//
// One workgroup per row of logits.  Every thread reads the row's request i = index[row], want[i], counter[i] and token[row] from the
// same addresses - uniform values, no barrier - and the workgroup branches uniformly: a free row (i < 0), a request that wants
// nothing (want[i] == -1) and a bad row return before anything of the row is read.  Then
//   1. the row goes ONCE through memory: as order-preserving 32-bit KEYS of its values (sample_body.h: -0.0 canonicalised to +0.0;
//      here a NaN takes the key above +inf's) into LDS where it fits (kLogprobMaxLdsCols floats), and the later passes read the keys
//      from there; a wider row is read again from memory by every pass.  The largest key is found on the way: it tells a
//      degenerate row (a NaN, +inf, or nothing but -inf), which writes NaN and -1 and is done;
//   2. W = sum_j floor(2^shift * __expf(x_j - m)) as 64-bit INTEGERS (sample_body.h's weights with inv_T = 1): exact in any order, so
//      the wave shuffles and the fold over the waves give the same bits on every run without a fixed order.  The maximum's own weight
//      is exactly 2^shift: W >= 2^shift and log S = logf(float(W) * 2^-shift) >= 0;
//   3. a log-probability is (x - m) - log S in fp32, two subtractions with both terms of one sign: no cancellation however large the
//      logits are.  ONE expression for the token's and for the alternatives': where the token is an alternative the bits are equal;
//   4. top-n, only where want[i] >= 1: 64-bit keys (the value's key, the INVERTED index), so that the larger key is the larger value
//      and, among equal values, the lower index, and no two elements share a key.  Every thread keeps the 8 best of its elements in
//      registers (a branch-free insertion into a sorted list, on the 32-bit keys alone: it meets its elements in index order); then want[i] rounds of a workgroup maximum over the threads' heads -
//      one barrier a round, the waves' slots double-buffered - in which the one thread that owns the winner stores it and pops it.
//      A round that finds nothing (cols < want[i]) ends the loop: the entries left keep their fill.
// Every index is checked before it is used; a bad row raises the status flag and writes nothing.
#include "sample_body.h"

namespace lg {

constexpr int kLogprobMaxTop = 8;
constexpr int kLogprobMaxWaves = 16;
constexpr int kLogprobStaticBytes = 512;                                 // LogprobShared, in front of the staged row
constexpr int64_t kLogprobMaxLdsCols = 36864;                            // 144 KiB of keys: with the 512 bytes in front, within the CU's 160 KiB
constexpr uint32_t kLogprobKeyNan = 0xFFFFFFFFu;                         // above the key of +inf, 0xFF800000
constexpr uint32_t kLogprobKeyPosInf = 0xFF800000u;
constexpr uint32_t kLogprobKeyNegInf = 0x007FFFFFu;

struct LogprobShared {
    u64      wave_sum[kLogprobMaxWaves];
    u64      wave_best[2][kLogprobMaxWaves];
    uint32_t wave_key[kLogprobMaxWaves];
};
static_assert(sizeof(LogprobShared) <= kLogprobStaticBytes, "LogprobShared outgrew its share of the LDS");
static_assert(kLogprobStaticBytes + kLogprobMaxLdsCols * 4 <= kSampleLdsBytes, "the staged row exceeds the CU's LDS");

__device__ __forceinline__ uint32_t logprob_key(float x) { return x != x ? kLogprobKeyNan : sample_key(x); }

__global__ void __launch_bounds__(1024) logprob_rows_kernel(const float* __restrict__ logits, int64_t cols, int64_t pitch,
                                                            const int32_t* __restrict__ token, const int32_t* __restrict__ want, int64_t n,
                                                            const int32_t* __restrict__ index, const int32_t* __restrict__ counter,
                                                            float* __restrict__ logprob, int64_t G, int32_t* __restrict__ top_ids,
                                                            float* __restrict__ top_logprob, int n_max, int lds_row, float scale, float inv_scale,
                                                            int* status) {
    extern __shared__ __align__(16) unsigned char logprob_dyn[];
    LogprobShared& sh = *reinterpret_cast<LogprobShared*>(logprob_dyn);
    uint32_t* const buf = reinterpret_cast<uint32_t*>(logprob_dyn + kLogprobStaticBytes);
    const int tid = threadIdx.x, T = blockDim.x, lane = tid & 63, wave = tid >> 6, nw = T >> 6;
    const int64_t row = blockIdx.x;                                      // the grid is the rows

    const int32_t i = index[row];
    if (i < 0) return;                                                   // a free slot: its logits are not read
    bool bad = i >= n;
    int k = 0, g = 0;
    int32_t tok = 0;
    if (!bad) {
        k = want[i];
        if (k == -1) return;                                             // a request that wants nothing: neither read nor written
        g = counter[i];
        tok = token[row];
        bad = k < -1 || k > n_max || g < 0 || g >= G || tok < 0 || int64_t(tok) >= cols;
    }
    if (bad) {                                                           // uniform: nothing of the row is read, nothing written
        if (tid == 0) __hip_atomic_fetch_or(status, LG_STATUS_BAD_INDEX, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
        return;
    }
    const float* const x = logits + row * pitch;
    const int64_t cell = int64_t(i) * G + g;                             // i < n, g < G: inside logprob; cell * n_max + r, r < k <= n_max, inside the others
    const auto key_at = [&](int64_t j) { return lds_row ? buf[j] : logprob_key(x[j]); };

    // 1. the row once through memory, its largest key on the way
    uint32_t kmax = 0;
#pragma unroll 4
    for (int64_t j = tid; j < cols; j += T) {
        const uint32_t key = logprob_key(x[j]);
        if (lds_row) buf[j] = key;
        kmax = key > kmax ? key : kmax;
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const uint32_t other = __shfl_xor(kmax, o, 64);
        kmax = other > kmax ? other : kmax;
    }
    if (lane == 0) sh.wave_key[wave] = kmax;
    __syncthreads();                                                     // (the staged row is complete, too)
    for (int w = 0; w < nw; ++w) kmax = sh.wave_key[w] > kmax ? sh.wave_key[w] : kmax;
    if (kmax >= kLogprobKeyPosInf || kmax == kLogprobKeyNegInf) {        // a NaN, +inf, or nothing but -inf: a degenerate row
        if (tid == 0) logprob[cell] = NAN;
        if (tid < k) { top_ids[cell * n_max + tid] = -1; top_logprob[cell * n_max + tid] = NAN; }
        return;
    }
    const float m = sample_value(kmax);

    // 2. the sum of the weights, integers
    u64 mine = 0;
#pragma unroll 4
    for (int64_t j = tid; j < cols; j += T) mine += sample_q(key_at(j), m, 1.0f, scale);
    mine = sample_wave_sum(mine);
    if (lane == 0) sh.wave_sum[wave] = mine;
    __syncthreads();
    u64 W = 0;
    for (int w = 0; w < nw; ++w) W += sh.wave_sum[w];
    const float log_s = logf(__fmul_rn(float(W), inv_scale));

    // 3. the token's own
    const auto logprob_of = [&](uint32_t key) { return __fsub_rn(__fsub_rn(sample_value(key), m), log_s); };
    if (tid == 0) logprob[cell] = logprob_of(key_at(tok));
    if (k == 0) return;

    // 4. the k most likely ids: the 8 best of this thread as (key, index) pairs, sorted, slot 0 the largest; 0 is no element's key.
    // A thread meets its elements by increasing index, so a STRICT 32-bit compare of the keys keeps equal values in index order:
    // no 64-bit compare in the pass over the row
    uint32_t bkey[kLogprobMaxTop], bidx[kLogprobMaxTop];
#pragma unroll
    for (int s = 0; s < kLogprobMaxTop; ++s) { bkey[s] = 0; bidx[s] = 0; }
    for (int64_t j = tid; j < cols; j += T) {
        const uint32_t c = key_at(j), at = uint32_t(j);
        if (c > bkey[kLogprobMaxTop - 1]) {
#pragma unroll
            for (int s = kLogprobMaxTop - 1; s > 0; --s) {
                const bool up = c > bkey[s - 1], here = c > bkey[s];
                bidx[s] = up ? bidx[s - 1] : (here ? at : bidx[s]);
                bkey[s] = up ? bkey[s - 1] : (here ? c : bkey[s]);
            }
            const bool here = c > bkey[0];
            bidx[0] = here ? at : bidx[0];
            bkey[0] = here ? c : bkey[0];
        }
    }
    for (int r = 0; r < k; ++r) {
        const u64 head = bkey[0] != 0 ? (u64(bkey[0]) << 32) | u64(0xFFFFFFFFu - bidx[0]) : u64(0);
        u64 top = head;
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            const u64 other = __shfl_xor(top, o, 64);
            top = other > top ? other : top;
        }
        if (lane == 0) sh.wave_best[r & 1][wave] = top;
        __syncthreads();                                                 // round r + 1 writes the other slots; round r + 2 these, two barriers on
        for (int w = 0; w < nw; ++w) top = sh.wave_best[r & 1][w] > top ? sh.wave_best[r & 1][w] : top;
        if (top == 0) break;                                             // uniform: the row has fewer than k elements
        if (head == top) {                                               // exactly one thread: keys are distinct
            top_ids[cell * n_max + r] = int32_t(bidx[0]);
            top_logprob[cell * n_max + r] = logprob_of(bkey[0]);
#pragma unroll
            for (int s = 0; s < kLogprobMaxTop - 1; ++s) { bkey[s] = bkey[s + 1]; bidx[s] = bidx[s + 1]; }
            bkey[kLogprobMaxTop - 1] = 0;
        }
    }
}

}  // namespace lg

using namespace lg;

extern "C" int lg_logprob_rows_f32(const float* logits, int64_t rows, int64_t cols, int64_t row_pitch, const int32_t* token, const int32_t* want,
                                   int64_t n, const int32_t* index, const int32_t* counter, float* logprob, int64_t G, int32_t* top_ids,
                                   float* top_logprob, int64_t n_max) {
    LG_REQUIRE_INIT();
    if (rows == 0) return LG_OK;                         // no rows: nothing is checked, nothing is launched
    LG_ARG(rows >= 1 && rows <= 65535, "lg_logprob_rows_f32: rows = %lld outside [0, 65535]", (long long)rows);
    LG_ARG(cols >= 1 && cols < (int64_t(1) << 31), "lg_logprob_rows_f32: cols = %lld outside [1, 2^31)", (long long)cols);
    LG_ARG(row_pitch >= cols, "lg_logprob_rows_f32: row_pitch = %lld below cols = %lld", (long long)row_pitch, (long long)cols);
    LG_ARG(n >= 1 && n < (int64_t(1) << 31), "lg_logprob_rows_f32: n = %lld requests, outside [1, 2^31)", (long long)n);
    LG_ARG(G >= 1 && G < (int64_t(1) << 31), "lg_logprob_rows_f32: G = %lld columns, outside [1, 2^31)", (long long)G);
    LG_ARG(n_max >= 1 && n_max <= kLogprobMaxTop, "lg_logprob_rows_f32: n_max = %lld alternatives outside [1, %d]", (long long)n_max, kLogprobMaxTop);
    LG_ARG(n * G <= (int64_t(1) << 40), "lg_logprob_rows_f32: n * G = %lld * %lld cells exceed 2^40", (long long)n, (long long)G);
    LG_ARG(logits != nullptr && token != nullptr && want != nullptr && index != nullptr && counter != nullptr && logprob != nullptr && top_ids != nullptr &&
               top_logprob != nullptr,
           "lg_logprob_rows_f32: NULL pointer");
    const void* const words[8] = {logits, token, want, index, counter, logprob, top_ids, top_logprob};
    const int64_t bytes[8] = {((rows - 1) * row_pitch + cols) * 4, rows * 4, n * 4, rows * 4, n * 4, n * G * 4, n * G * n_max * 4, n * G * n_max * 4};
    static const char* const names[8] = {"logits", "token", "want", "index", "counter", "logprob", "top_ids", "top_logprob"};
    for (int a = 0; a < 8; ++a)
        LG_ARG((reinterpret_cast<uintptr_t>(words[a]) & 3u) == 0, "lg_logprob_rows_f32: %s is not aligned to 4 bytes", names[a]);
    for (int a = 5; a < 8; ++a)                          // what the launch writes shares no byte with anything else
        for (int b = 0; b < a; ++b)
            LG_ARG(!bytes_overlap(words[a], bytes[a], words[b], bytes[b]), "lg_logprob_rows_f32: %s overlaps %s", names[a], names[b]);
    for (int a = 5; a < 8; ++a) { const int rc = adam_epilogue_check_write(words[a], bytes[a]); if (rc != LG_OK) return rc; }
    const SampleShape shape = sample_shape(cols);        // the scale of the integer weights and the threads, as the sampling launches choose them
    const bool lds_row = cols <= kLogprobMaxLdsCols;
    const size_t lds = size_t(kLogprobStaticBytes) + (lds_row ? size_t(cols) * 4 : 0);
    const hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(&logprob_rows_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, int(lds));
    if (e != hipSuccess) { set_error("lg_logprob_rows_f32: %zu bytes of LDS refused: %s", lds, hipGetErrorString(e)); return LG_EHIP; }
    hipLaunchKernelGGL(logprob_rows_kernel, dim3{unsigned(rows)}, dim3(shape.threads), lds, rt().stream, logits, cols, row_pitch, token, want, n, index,
                       counter, logprob, G, top_ids, top_logprob, int(n_max), int(lds_row), shape.scale, 1.0f / shape.scale, rt().status_dev);
    LG_CHECK_LAUNCH();
    return LG_OK;
}

extern "C" int lg_logprob_lds_cols(void) { return int(kLogprobMaxLdsCols); }
