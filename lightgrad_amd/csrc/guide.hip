// Guided decoding: per-request token automata on fp32 logits, IN PLACE (C ABI and definition: include/lghip.h,
// lightgrad_amd/guide.py `guide_logits`).  ONE launch for all rows, behind the penalties and in front of the draw; every
// operand is device state, so a captured step replays it as it stands.
//
// The grid is (slices, rows): a row of logits is cut into `slices` runs of 16-byte groups, one workgroup of 256 threads each (slices = 1
// is a workgroup per row, like the siblings).  Every thread of every workgroup of a row reads the row's request i = index[row], the pair
// (q, k) = state[i] - ONE 8-byte load - and g = out_len[i] from the same addresses: uniform values, no barrier, and the workgroup
// branches uniformly.  A free row (i < 0), an unguided one (q == -1) and a bad one return before the row of logits is addressed.
//   1. catch-up: for j = k .. g - 1 the state absorbs out[i, j] - its range and its bit in q's bitset checked, its exception found by
//      binary search in the state's run of `edges`, else the default.  Every index and every table word is checked before it forms an
//      address.  This runs before the first store, so a bad row writes nothing.  Every slice computes the same (q', g): the automaton
//      is deterministic, and whichever pair a slice sees - (q, k), or the (q', g) that slice 0 has already stored - leads there;
//   2. slice 0, thread 0 alone stores state[i] = (q', g) as one 8-byte word and +0.0 at the forced id (whose bit is set: no thread
//      masks it);
//   3. the pass is STORE-ONLY: the slice stages its words of q's bitset in LDS (while they fit, else reads them from memory) and
//      walks the 16-byte groups of the row's ADDRESSES - a row start off 16 bytes shifts the groups, not the path: four masked ids
//      inside the row take one 16-byte store of -inf, a group with some bits set or cut by a row end takes single stores, a group of
//      allowed ids is not touched.  No logit is read; each has one writer.
#include "common.h"

namespace lg {

constexpr int kGuideThreads = 256;
constexpr int kGuideLdsWords = 4096;              // 16 KiB: the bitset words of 131072 ids per slice
constexpr int kGuideGroupsPerThread = 4;          // the automatic grid gives a thread about this many 16-byte groups
constexpr int kGuideMaxSlices = 64;

static int guide_slices_override = 0;             // 0: automatic

__global__ void __launch_bounds__(kGuideThreads) guide_rows_kernel(float* __restrict__ logits, int64_t cols, int64_t pitch,
                                                                   const uint32_t* __restrict__ allow, const int32_t* __restrict__ states, int64_t S,
                                                                   const int32_t* __restrict__ edges, int64_t E, const int32_t* __restrict__ index,
                                                                   const int32_t* __restrict__ out, int64_t ldo, int G,
                                                                   const int32_t* __restrict__ out_len, int32_t* state, int64_t N, int* status) {
    __shared__ uint32_t staged[kGuideLdsWords];
    const int tid = threadIdx.x;
    const int64_t row = blockIdx.y;
    const int slice = blockIdx.x, slices = gridDim.x;
    const int64_t W = (cols + 31) >> 5;

    const int32_t i = index[row];
    if (i < 0) return;                                                   // a free slot: its logits are not read
    const bool reporter = tid == 0 && slice == 0;
    if (i >= N) {
        if (reporter) __hip_atomic_fetch_or(status, LG_STATUS_BAD_INDEX, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
        return;
    }
    unsigned long long* const pair = reinterpret_cast<unsigned long long*>(state) + i;
    const unsigned long long qk = __hip_atomic_load(pair, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);      // (q, k) as one word
    int64_t q = int32_t(uint32_t(qk));
    const int k = int32_t(uint32_t(qk >> 32));
    if (q == -1) return;                                                 // an unguided request
    const int g = out_len[i];
    bool bad = g < 0 || g > G || q < 0 || q >= S || k < 0 || k > g;
    if (!bad) {
        const int32_t* const own_out = out + int64_t(i) * ldo;
        for (int j = k; j < g; ++j) {                                    // uniform: every thread walks the same tokens
            const int32_t tok = own_out[j];
            if (tok < 0 || int64_t(tok) >= cols) { bad = true; break; }
            if (!((allow[q * W + (tok >> 5)] >> (tok & 31)) & 1u)) { bad = true; break; }
            const int4 w = reinterpret_cast<const int4*>(states)[q];
            if (w.y < 0 || w.z < 0 || int64_t(w.y) + int64_t(w.z) > E) { bad = true; break; }
            int64_t lo = w.y, hi = int64_t(w.y) + w.z;                   // the first entry whose id is >= tok
            while (lo < hi) {
                const int64_t mid = (lo + hi) >> 1;
                if (edges[2 * mid] < tok) lo = mid + 1; else hi = mid;
            }
            q = (lo < int64_t(w.y) + w.z && edges[2 * lo] == tok) ? edges[2 * lo + 1] : w.x;
            if (q < 0 || q >= S) { bad = true; break; }
        }
    }
    int32_t forced = -1;
    if (!bad) {
        forced = states[4 * q + 3];
        bad = forced < -1 || int64_t(forced) >= cols || (forced >= 0 && !((allow[q * W + (forced >> 5)] >> (forced & 31)) & 1u));
    }
    if (bad) {                                                           // uniform, and before the first store: a bad row writes nothing
        if (reporter) __hip_atomic_fetch_or(status, LG_STATUS_BAD_INDEX, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
        return;
    }

    float* const x_row = logits + row * pitch;
    if (reporter) {
        __hip_atomic_store(pair, (unsigned long long)(uint32_t(q)) | ((unsigned long long)(uint32_t(g)) << 32), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (forced >= 0) x_row[forced] = 0.0f;
    }

    // the 16-byte groups of the row's addresses: group j holds the columns 4 j - a .. 4 j - a + 3, a = the row start's words off 16 bytes
    const int64_t a = int64_t((reinterpret_cast<uintptr_t>(x_row) >> 2) & 3u);
    const int64_t groups = (a + cols + 3) >> 2;
    const int64_t j0 = groups * slice / slices, j1 = groups * (slice + 1) / slices;
    if (j0 >= j1) return;
    const int64_t c_lo = 4 * j0 - a < 0 ? 0 : 4 * j0 - a, c_hi = 4 * j1 - a > cols ? cols : 4 * j1 - a;      // the slice's columns [c_lo, c_hi)
    const int64_t w_lo = c_lo >> 5, w_n = ((c_hi - 1) >> 5) - w_lo + 1;
    const uint32_t* const bits = allow + q * W + w_lo;
    const bool in_lds = w_n <= kGuideLdsWords;                           // uniform
    if (in_lds) {
        for (int64_t w = tid; w < w_n; w += kGuideThreads) staged[w] = bits[w];
        __syncthreads();
    }
    const float4 minus = {-INFINITY, -INFINITY, -INFINITY, -INFINITY};
    for (int64_t j = j0 + tid; j < j1; j += kGuideThreads) {
        const int64_t c0 = 4 * j - a;
        unsigned set = 0;                                                // bit t: column c0 + t is allowed, or outside the row
#pragma unroll
        for (int t = 0; t < 4; ++t) {
            const int64_t c = c0 + t;
            unsigned b = 1u;
            if (c >= 0 && c < cols) {
                const int64_t w = (c >> 5) - w_lo;
                b = ((in_lds ? staged[w] : bits[w]) >> (c & 31)) & 1u;
            }
            set |= b << t;
        }
        if (set == 0u) {
            *reinterpret_cast<float4*>(x_row + c0) = minus;              // four masked ids inside the row, 16-byte aligned
        } else if (set != 15u) {
#pragma unroll
            for (int t = 0; t < 4; ++t)
                if (!((set >> t) & 1u)) x_row[c0 + t] = -INFINITY;
        }
    }
}

}  // namespace lg

using namespace lg;

extern "C" int lg_guide_rows_slices(int slices) {
    const int before = guide_slices_override;
    if (slices >= 0 && slices <= kGuideMaxSlices) guide_slices_override = slices;
    return before;
}

extern "C" int lg_guide_rows_f32(float* logits, int64_t rows, int64_t cols, int64_t row_pitch, const int32_t* allow, const int32_t* states, int64_t S,
                                 const int32_t* edges, int64_t E, const int32_t* index, const int32_t* out, int64_t out_pitch, int64_t G,
                                 const int32_t* out_len, int32_t* state, int64_t N) {
    LG_REQUIRE_INIT();
    if (rows == 0) return LG_OK;                         // nothing to guide: nothing is checked, nothing is launched
    LG_ARG(rows >= 1 && rows <= 65535, "lg_guide_rows_f32: rows = %lld outside [0, 65535]", (long long)rows);
    LG_ARG(cols >= 1 && cols < (int64_t(1) << 31), "lg_guide_rows_f32: cols = %lld outside [1, 2^31)", (long long)cols);
    LG_ARG(row_pitch >= cols, "lg_guide_rows_f32: row_pitch = %lld below cols = %lld", (long long)row_pitch, (long long)cols);
    LG_ARG(S >= 1 && S < (int64_t(1) << 31) && E >= 1 && E < (int64_t(1) << 31), "lg_guide_rows_f32: S = %lld states and E = %lld edges, each in [1, 2^31)",
           (long long)S, (long long)E);
    LG_ARG(N >= 1 && N < (int64_t(1) << 31) && G >= 1 && G < (int64_t(1) << 31), "lg_guide_rows_f32: N = %lld requests and G = %lld columns of out, each in [1, 2^31)",
           (long long)N, (long long)G);
    LG_ARG(out_pitch >= G, "lg_guide_rows_f32: out_pitch = %lld below G = %lld", (long long)out_pitch, (long long)G);
    LG_ARG(logits != nullptr && allow != nullptr && states != nullptr && edges != nullptr && index != nullptr && out != nullptr && out_len != nullptr &&
               state != nullptr,
           "lg_guide_rows_f32: NULL pointer");
    const auto aligned = [](const void* p, uintptr_t to) { return (reinterpret_cast<uintptr_t>(p) & (to - 1)) == 0; };
    LG_ARG(aligned(logits, 4) && aligned(allow, 4) && aligned16(states) && aligned(edges, 4) && aligned(index, 4) && aligned(out, 4) && aligned(out_len, 4) &&
               aligned(state, 8),
           "lg_guide_rows_f32: a misaligned operand (states: 16 bytes; state: 8; everything else: 4)");
    const int64_t W = (cols + 31) / 32;
    const int64_t logit_bytes = ((rows - 1) * row_pitch + cols) * 4;
    const void* const words[7] = {allow, states, edges, index, out, out_len, state};
    const int64_t bytes[7] = {S * W * 4, S * 16, E * 8, rows * 4, ((N - 1) * out_pitch + G) * 4, N * 4, N * 8};
    for (int k = 0; k < 7; ++k)
        LG_ARG(!bytes_overlap(logits, logit_bytes, words[k], bytes[k]),
               "lg_guide_rows_f32: the logits overlap operand %d (of allow, states, edges, index, out, out_len, state)", k);
    for (int k = 0; k < 6; ++k)
        LG_ARG(!bytes_overlap(state, bytes[6], words[k], bytes[k]),
               "lg_guide_rows_f32: state overlaps operand %d (of allow, states, edges, index, out, out_len)", k);
    { const int rc = adam_epilogue_check_write(logits, logit_bytes); if (rc != LG_OK) return rc; }
    { const int rc = adam_epilogue_check_write(state, bytes[6]); if (rc != LG_OK) return rc; }
    int64_t slices = guide_slices_override;
    if (slices == 0) {                                   // about kGuideGroupsPerThread 16-byte groups a thread
        const int64_t groups = (cols + 3) / 4, per = int64_t(kGuideThreads) * kGuideGroupsPerThread;
        slices = (groups + per - 1) / per;
        if (slices > kGuideMaxSlices) slices = kGuideMaxSlices;
    }
    hipLaunchKernelGGL(guide_rows_kernel, dim3(unsigned(slices), unsigned(rows)), dim3(kGuideThreads), 0, rt().stream, logits, cols, row_pitch,
                       reinterpret_cast<const uint32_t*>(allow), states, S, edges, E, index, out, out_pitch, int(G), out_len, state, N, rt().status_dev);
    LG_CHECK_LAUNCH();
    return LG_OK;
}
