// The bookkeeping of one step of speculative decoding by prompt lookup in ONE launch: lg_speculate_commit_i32.
//
// A speculative step runs b sequences through the model, m token rows each: row 0 of a sequence is its last committed token, the
// rows behind it are guesses ("drafts") at the tokens that follow, and the model scores all of them at once.  Between two steps
// every sequence keeps the longest prefix of its drafts that the model agrees with plus one token of the model's own, stops at the
// end-of-sequence id or at its last column, and guesses again: the continuation of the most recent earlier occurrence of its last
// n-gram in its own ids (prompt lookup).  The definition is the sequential loop of `CpuTensor.speculate_commit`
// (autograd/cpu/ops.py); as tensor expressions it is dozens of launches and a search, in a step that is bound by its launch
// boundaries.
//
// One workgroup of 256 threads per sequence; nothing is shared between sequences but the three words of `stats`, which take
// integer atomic adds (the sums do not depend on their order).  Inside a workgroup every decision is a fold over the threads with
// a fixed shape - shuffles inside a wave, then the waves' words in LDS in wave order - of integers under max: the accepted length
// (the first draft that differs, the first end-of-sequence id) and, per n-gram length, the LARGEST start q of a match, the
// candidate starts being split over the threads.  The sequence - the row's ids up to its new position - is staged in LDS when the
// ids have at most kSpecLdsColumns columns (the model has 512 positions); wider rows are served too, by the same code reading the
// row from memory.
//
// Every index is checked before it is used: a row whose count, position or end is out of bounds (see the definition) raises the
// status flag - LG_EINDEX at the next synchronisation -, gets count = 0 and nothing else of it is written: a bounds check, never a
// fault.
#include "common.h"

namespace lg {

constexpr int kSpecThreads = 256;
constexpr int kSpecLdsColumns = 4096;           // 16 KiB of LDS per workgroup

struct SpecArgs {
    const int32_t* tgt;                         // (b, m) dense
    int32_t *ids, *count, *position_ids;        // (b, m), (b), (b, m) dense
    int32_t* out_ids;                           // row r at out_ids + r * out_pitch
    int64_t out_pitch;
    int32_t *pos, *done, *stats;
    const int32_t* end;
    int m, columns, draft, max_ngram, min_ngram;
    int32_t eos_id;
    int* status;
};

// the largest v of the workgroup, in every thread: a fold of fixed shape (xor shuffles, then the waves' words in wave order)
__device__ __forceinline__ int spec_block_max(int v, int* s_wave) {
    for (int off = 32; off >= 1; off >>= 1) {
        const int o = __shfl_xor(v, off, 64);
        v = o > v ? o : v;
    }
    __syncthreads();                            // whoever still reads s_wave from the fold before is through
    if ((threadIdx.x & 63) == 0) s_wave[threadIdx.x >> 6] = v;
    __syncthreads();
    int best = s_wave[0];
    for (int w = 1; w < kSpecThreads / 64; ++w) best = s_wave[w] > best ? s_wave[w] : best;
    return best;
}

__global__ __launch_bounds__(kSpecThreads) void speculate_commit(const SpecArgs a) {
    __shared__ int32_t s_seq[kSpecLdsColumns];
    __shared__ int s_wave[kSpecThreads / 64];
    const int r = blockIdx.x, tid = threadIdx.x, m = a.m;
    const int big = 0x7fffffff;
    // the row's words, read by every thread before thread 0 writes any of them (behind the barriers of the folds below)
    const int was_done = a.done[r], c = a.count[r], p0 = a.pos[r], last = a.end[r];
    __syncthreads();
    if (was_done != 0) {
        if (tid == 0) a.count[r] = 0;
        return;
    }
    if (!(c >= 1 && c <= m && p0 >= 0 && int64_t(p0) + c <= last && last <= a.columns - 1)) {
        if (tid == 0) {
            __hip_atomic_fetch_or(a.status, LG_STATUS_BAD_INDEX, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
            a.count[r] = 0;
        }
        return;
    }
    const int32_t* tgt = a.tgt + int64_t(r) * m;
    int32_t *ids = a.ids + int64_t(r) * m, *position_ids = a.position_ids + int64_t(r) * m, *row = a.out_ids + int64_t(r) * a.out_pitch;

    // step 3: the first draft the model disagrees with, the first end-of-sequence id (as minima: max of big - j)
    int differs = 0, stops = 0;
    for (int j = tid; j < c; j += kSpecThreads) {
        const int32_t t = tgt[j];
        if (j < c - 1 && ids[j + 1] != t && big - j > differs) differs = big - j;
        if (a.eos_id >= 0 && t == a.eos_id && big - j > stops) stops = big - j;
    }
    differs = spec_block_max(differs, s_wave);
    stops = spec_block_max(stops, s_wave);
    const int accepted = differs ? big - differs : c - 1;
    const int eos_at = stops ? big - stops : big;
    const bool stopped = eos_at <= accepted;
    const int e = stopped ? eos_at + 1 : accepted + 1;            // 1 <= e <= c, so p0 + e <= end <= columns - 1
    const int p = p0 + e;
    const bool finished = stopped || p == last;

    // step 4: the tokens kept
    for (int j = tid; j < e; j += kSpecThreads) row[p0 + 1 + j] = tgt[j];
    if (finished) {
        if (tid == 0) {
            a.pos[r] = p;
            a.done[r] = 1;
            a.count[r] = 0;
            atomicAdd(a.stats + 0, 1);
            atomicAdd(a.stats + 1, c - 1);
            atomicAdd(a.stats + 2, accepted);
        }
        return;
    }

    // step 6: the sequence 0 .. p, from LDS where the ids are narrow enough (the row's old columns from memory, the new ones from tgt)
    const int L = p + 1;
    const bool staged = a.columns <= kSpecLdsColumns;
    if (staged) {
        for (int j = tid; j < L; j += kSpecThreads) s_seq[j] = j <= p0 ? row[j] : tgt[j - p0 - 1];
    }
    __syncthreads();                            // s_seq is complete; the stores to `row` above are visible to the workgroup
    const int32_t* seq = staged ? s_seq : row;
    const int cap = a.draft < last - p - 1 ? a.draft : last - p - 1;
    int q = -1, n = 0;
    if (cap > 0) {
        for (n = a.max_ngram < L - 1 ? a.max_ngram : L - 1; n >= a.min_ngram; --n) {
            int mine = -1;
            for (int s = tid; s <= L - n - 1; s += kSpecThreads) {
                int i = 0;
                while (i < n && seq[s + i] == seq[L - n + i]) ++i;
                if (i == n) mine = s;           // the thread's starts ascend: the last match is its largest
            }
            q = spec_block_max(mine, s_wave);
            if (q >= 0) break;
        }
    }
    int drafts = 0;
    if (q >= 0) drafts = cap < L - (q + n) ? cap : L - (q + n);  // q + n <= L - 1: at least one
    for (int i = tid; i < m; i += kSpecThreads) {
        ids[i] = i == 0 ? seq[p] : (i <= drafts ? seq[q + n + i - 1] : 0);
        position_ids[i] = i <= drafts ? p + i : 0;
    }
    if (tid == 0) {
        a.pos[r] = p;
        a.count[r] = 1 + drafts;
        atomicAdd(a.stats + 1, c - 1);
        atomicAdd(a.stats + 2, accepted);
    }
}

}  // namespace lg

using namespace lg;

extern "C" int lg_speculate_commit_i32(const int32_t* tgt, int32_t* ids, int32_t* count, int32_t* position_ids, int32_t* out_ids, int64_t out_pitch,
                                       int64_t columns, int32_t* pos, const int32_t* end, int32_t* done, int32_t* stats, int64_t batch, int64_t m,
                                       int64_t draft, int64_t max_ngram, int64_t min_ngram, int32_t eos_id) {
    LG_REQUIRE_INIT();
    const char* name = "lg_speculate_commit_i32";
    const int64_t lim = int64_t(1) << 31;
    LG_ARG(batch >= 0 && batch < (int64_t(1) << 24) && m >= 1 && m < lim && batch * m < lim && columns >= 1 && columns < lim,
           "%s: batch = %lld (0 .. 2^24 - 1: a workgroup each), m = %lld, columns = %lld (each 1 .. 2^31 - 1, batch * m too) unsupported", name,
           (long long)batch, (long long)m, (long long)columns);
    LG_ARG(draft >= 0 && draft <= m - 1 && min_ngram >= 1 && min_ngram <= max_ngram && max_ngram < lim,
           "%s: draft = %lld (0 .. m - 1 = %lld), n-grams of %lld .. %lld tokens (1 <= min <= max < 2^31) unsupported", name, (long long)draft,
           (long long)(m - 1), (long long)min_ngram, (long long)max_ngram);
    if (batch == 0) return LG_OK;
    const void* ptr[9] = {tgt, ids, count, position_ids, out_ids, pos, end, done, stats};
    for (int i = 0; i < 9; ++i) LG_ARG(ptr[i], "%s: NULL operand %d (of tgt, ids, count, position_ids, out_ids, pos, end, done, stats)", name, i);
    for (int i = 0; i < 9; ++i) LG_ARG((reinterpret_cast<uintptr_t>(ptr[i]) & 3u) == 0, "%s: operand %d must be 4-byte aligned", name, i);
    LG_ARG(out_pitch >= columns && (batch - 1) * out_pitch + columns < (int64_t(1) << 60), "%s: row pitch %lld (out_ids, >= columns = %lld)", name,
           (long long)out_pitch, (long long)columns);
    {
        // a workgroup writes its row's words: bytes shared by two operands would make the result depend on which workgroup ran first
        const int64_t bytes[9] = {batch * m * 4, batch * m * 4, batch * 4, batch * m * 4, ((batch - 1) * out_pitch + columns) * 4, batch * 4, batch * 4,
                                  batch * 4, 12};
        for (int i = 0; i < 9; ++i)
            for (int j = i + 1; j < 9; ++j)
                LG_ARG(!bytes_overlap(ptr[i], bytes[i], ptr[j], bytes[j]), "%s: operands %d and %d (of tgt, ids, count, position_ids, out_ids, pos, end, done, stats) overlap", name, i, j);
        for (int i = 1; i < 9; ++i) {
            if (i == 6) continue;               // `end` is read only
            const int rc = adam_epilogue_check_write(ptr[i], bytes[i]);
            if (rc != LG_OK) return rc;
        }
    }
    const SpecArgs a{tgt, ids, count, position_ids, out_ids, out_pitch, pos, done, stats, end, int(m), int(columns), int(draft), int(max_ngram),
                     int(min_ngram), eos_id, rt().status_dev};
    hipLaunchKernelGGL(speculate_commit, dim3(unsigned(batch)), dim3(kSpecThreads), 0, rt().stream, a);
    LG_CHECK_LAUNCH();
    return LG_OK;
}
