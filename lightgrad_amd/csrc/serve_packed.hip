// The slot bookkeeping of one TOKEN-PACKED step of continuous batching in ONE launch: lg_serve_commit_packed_i32.
//
// lg_serve_commit_i32 (serve.hip) lays a step out as (slots, m) rows: a slot that decodes one token still carries m rows through
// the model.  Here the step is T token rows for all slots together - the token budget, T >= slots - and slot s owns rows
// cu[s] .. cu[s + 1] - 1 of them.  What a slot WANTS is decided as in serve.hip with m = chunk (steps 1 and 2 of the definition: the
// next piece of its prompt, the token just drawn, a waiting request admitted to a free slot in slot order); what it GETS is the
// budget's: every decoding slot its one token, and the R = T - (decoding slots) rows left go to the prefilling slots in slot
// order, n = min(want, what is left).  A prefilling slot granted 0 keeps its request and its position and asks again in the next
// step.  The definition is the sequential loop of `CpuTensor.serve_commit_packed` (autograd/cpu/ops.py).
//
// One workgroup, one thread per slot (slots <= 1024).  A slot depends on the others through three exclusive sums in slot order,
// each taken inside a wave (a ballot for the flags, a shuffle scan for the numbers) and across the waves through per-wave totals
// in LDS: its rank among the free slots (the admission order), the wants of the prefilling slots in front of it
// (grant = clamp(R - prefix, 0, want)), and the rows granted in front of it (cu).  The step's T ids and position ids are then
// written by all threads together, coalesced; a row finds its slot by bisection of cu in LDS.
//
// A slot that would leave its bounds (see the definition) raises the status flag - LG_EINDEX at the next synchronisation -, gets
// count = 0, takes no rows and nothing else of it is written: a bounds check, never a fault.
#include "common.h"

namespace lg {

constexpr int kPackedMaxSlots = 1024;
constexpr int kPackedWaves = kPackedMaxSlots / 64;

struct ServePackedArgs {
    const int32_t* nxt;                  // slot s reads nxt[s * nxt_pitch]
    int64_t nxt_pitch;
    const int32_t *prompts, *prompt_len, *budget;        // prompts: request r, token i at prompts + r * prompt_pitch + i
    int64_t prompt_pitch;
    int32_t *out, *out_len;              // out: request r, token g at out + r * out_pitch + g
    int64_t out_pitch;
    int32_t *queue, *req, *pos, *count, *cu, *ids, *position_ids, *last;
    int P, G, N, b, T, chunk, capacity;
    int32_t eos_id;
    int* status;
};

// the sum of `v` over the lanes in front of this one, and - in `total` - over the wave
__device__ __forceinline__ int wave_exclusive_sum(int v, int lane, int& total) {
    int inc = v;
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
        const int o = __shfl_up(inc, off, 64);
        if (lane >= off) inc += o;
    }
    total = __shfl(inc, 63, 64);
    return inc - v;
}

__global__ __launch_bounds__(kPackedMaxSlots) void serve_commit_packed(const ServePackedArgs a) {
    __shared__ int s_cu[kPackedMaxSlots + 1];    // the first row of the slot; [b]: the rows in use
    __shared__ int s_t[kPackedMaxSlots];         // position of its token 0
    __shared__ int s_row[kPackedMaxSlots];       // the request whose prompt the tokens come from, -1: the one token s_tok
    __shared__ int s_tok[kPackedMaxSlots];
    __shared__ int s_free[kPackedWaves], s_done[kPackedWaves], s_dec[kPackedWaves], s_want[kPackedWaves], s_grant[kPackedWaves];
    const int s = threadIdx.x, lane = s & 63, wave = s >> 6, waves = blockDim.x >> 6;
    const int chunk = a.chunk, N = a.N, T = a.T;
    const int first = a.queue[0];                // read by every thread before thread 0 writes it (behind the barrier below)

    // step 1: the slot's own request (serve.hip's, with m = chunk)
    int r = -1, t = 0, n = 0, row = -1, tok = 0;
    bool fault = false, finished = false;
    if (s < a.b) {
        r = a.req[s];
        if (r >= 0) {
            const int64_t tt = int64_t(a.pos[s]) + a.count[s];
            if (r >= N || tt < 0 || tt > a.capacity) {
                fault = true;
            } else {
                t = int(tt);
                const int len = a.prompt_len[r];
                if (t < len) {
                    n = len - t < chunk ? len - t : chunk;
                    row = r;
                    fault = t + n > a.P;
                } else {
                    const int g = a.out_len[r];
                    if (g < 0 || g >= a.G) {
                        fault = true;
                    } else {
                        tok = a.nxt[int64_t(s) * a.nxt_pitch];
                        a.out[int64_t(r) * a.out_pitch + g] = tok;
                        a.out_len[r] = g + 1;
                        if ((a.eos_id >= 0 && tok == a.eos_id) || g + 1 == a.budget[r]) {
                            finished = true;
                            r = -1;
                        } else {
                            n = 1;
                        }
                    }
                }
            }
        }
    }
    // step 2: the admission order - free slots in slot order
    const bool is_free = s < a.b && !fault && r < 0;
    const unsigned long long free_mask = __ballot(is_free), done_mask = __ballot(finished);
    if (lane == 0) { s_free[wave] = __popcll(free_mask); s_done[wave] = __popcll(done_mask); }
    __syncthreads();
    int rank = __popcll(free_mask & ((1ull << lane) - 1ull)), all_free = 0, all_done = 0;
    for (int w = 0; w < waves; ++w) {
        if (w < wave) rank += s_free[w];
        all_free += s_free[w];
        all_done += s_done[w];
    }
    if (is_free) {
        t = 0;
        if (int64_t(first) + rank < N && first >= 0) {
            r = first + rank;
            const int len = a.prompt_len[r];
            n = len < chunk ? len : chunk;
            row = r;
            fault = n < 0 || n > a.P;
        }
    }
    if (s == 0) {
        const int64_t waiting = first < 0 ? 0 : int64_t(N) - first;
        a.queue[0] = first + int(waiting < all_free ? (waiting < 0 ? 0 : waiting) : all_free);
        a.queue[1] += all_done;
    }
    // a slot whose want would leave the cache takes no rows, whatever the budget would grant it
    fault = fault || int64_t(t) + n > a.capacity;
    if (fault) n = 0;
    // step 3: the budget.  Every decoding slot its token; the prefilling slots share the R rows left, in slot order
    const bool decoding = s < a.b && !fault && row < 0 && n == 1;
    const int want = (s < a.b && !fault && row >= 0) ? n : 0;
    const unsigned long long dec_mask = __ballot(decoding);
    int want_wave;
    int before = wave_exclusive_sum(want, lane, want_wave);
    if (lane == 0) { s_dec[wave] = __popcll(dec_mask); s_want[wave] = want_wave; }
    __syncthreads();
    int all_dec = 0;
    for (int w = 0; w < waves; ++w) {
        all_dec += s_dec[w];
        if (w < wave) before += s_want[w];
    }
    const int R = T - all_dec, left = R - before;                 // (R >= 1 whenever a slot prefills: T >= slots)
    if (!decoding) n = left < 0 ? 0 : (left < want ? left : want);
    // step 4: the slot's rows - the exclusive sum of the grants
    int grant_wave;
    int start = wave_exclusive_sum(n, lane, grant_wave);
    if (lane == 0) s_grant[wave] = grant_wave;
    __syncthreads();
    int used = 0;
    for (int w = 0; w < waves; ++w) {
        if (w < wave) start += s_grant[w];
        used += s_grant[w];
    }
    if (s < a.b) {
        if (fault) {
            __hip_atomic_fetch_or(a.status, LG_STATUS_BAD_INDEX, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
            a.count[s] = 0;
        } else {
            const int end = start + (n > 0 ? n - 1 : 0);
            a.req[s] = r;
            a.pos[s] = t;
            a.count[s] = n;
            a.last[s] = end < T - 1 ? end : T - 1;                // an idle slot behind a full buffer must not name row T
        }
        a.cu[s] = start;
        if (s == 0) a.cu[a.b] = used;
        s_cu[s] = start;
        if (s == 0) s_cu[a.b] = used;
        s_t[s] = t;
        s_row[s] = row;
        s_tok[s] = tok;
    }
    __syncthreads();
    // the step's inputs: T words each, consecutive threads on consecutive words.  Row e < used belongs to the LAST slot whose
    // first row is <= e (the slots in front of it that start there own no row)
    for (int e = s; e < T; e += blockDim.x) {
        int id = 0, position = 0;
        if (e < used) {
            int lo = 0, hi = a.b;                                 // s_cu[lo] <= e < s_cu[hi]
            while (hi - lo > 1) {
                const int mid = (lo + hi) >> 1;
                if (s_cu[mid] <= e) lo = mid; else hi = mid;
            }
            const int i = e - s_cu[lo];
            id = s_row[lo] >= 0 ? a.prompts[int64_t(s_row[lo]) * a.prompt_pitch + s_t[lo] + i] : s_tok[lo];
            position = s_t[lo] + i;
        }
        a.ids[e] = id;
        a.position_ids[e] = position;
    }
}

// do the bytes [x, x + nx) and [y, y + ny) share an address?
static bool packed_overlap(const void* x, int64_t nx, const void* y, int64_t ny) {
    const char *a = static_cast<const char*>(x), *b = static_cast<const char*>(y);
    return a < b + ny && b < a + nx;
}

}  // namespace lg

using namespace lg;

extern "C" int lg_serve_commit_packed_i32(const int32_t* nxt, int64_t nxt_pitch, const int32_t* prompts, int64_t prompt_pitch, int64_t P,
                                          const int32_t* prompt_len, const int32_t* budget, int32_t* out, int64_t out_pitch, int64_t G,
                                          int32_t* out_len, int32_t* queue, int64_t N, int32_t* req, int32_t* pos, int32_t* count, int32_t* cu,
                                          int32_t* ids, int32_t* position_ids, int32_t* last, int64_t slots, int64_t T, int64_t chunk,
                                          int64_t capacity, int32_t eos_id) {
    LG_REQUIRE_INIT();
    const char* name = "lg_serve_commit_packed_i32";
    const int64_t lim = int64_t(1) << 31;
    LG_ARG(slots >= 0 && slots <= kPackedMaxSlots && chunk >= 1 && chunk < lim && slots * chunk < lim && T >= 1 && T >= slots && T < lim && N >= 1 && N < lim &&
               P >= 1 && P < lim && G >= 1 && G < lim && capacity >= 1 && capacity < lim,
           "%s: slots = %lld (0 .. 1024), T = %lld (>= slots), chunk = %lld, N = %lld, P = %lld, G = %lld, capacity = %lld (each 1 .. 2^31 - 1, slots * chunk too) unsupported",
           name, (long long)slots, (long long)T, (long long)chunk, (long long)N, (long long)P, (long long)G, (long long)capacity);
    if (slots == 0) return LG_OK;
    const char* operands = "nxt, prompts, prompt_len, budget, out, out_len, queue, req, pos, count, cu, ids, position_ids, last";
    const void* ptr[14] = {nxt, prompts, prompt_len, budget, out, out_len, queue, req, pos, count, cu, ids, position_ids, last};
    for (int i = 0; i < 14; ++i) LG_ARG(ptr[i], "%s: NULL operand %d (of %s)", name, i, operands);
    for (int i = 0; i < 14; ++i) LG_ARG((reinterpret_cast<uintptr_t>(ptr[i]) & 3u) == 0, "%s: operand %d must be 4-byte aligned", name, i);
    LG_ARG(nxt_pitch >= 1 && prompt_pitch >= P && out_pitch >= G, "%s: row pitches %lld (nxt, >= 1) / %lld (prompts, >= P = %lld) / %lld (out, >= G = %lld)",
           name, (long long)nxt_pitch, (long long)prompt_pitch, (long long)P, (long long)out_pitch, (long long)G);
    {
        // a thread writes its slot's words and its request's words: bytes shared by two operands would make the result depend on
        // which thread ran first
        const int64_t bytes[14] = {((slots - 1) * nxt_pitch + 1) * 4, ((N - 1) * prompt_pitch + P) * 4, N * 4, N * 4, ((N - 1) * out_pitch + G) * 4, N * 4, 8,
                                   slots * 4, slots * 4, slots * 4, (slots + 1) * 4, T * 4, T * 4, slots * 4};
        for (int i = 0; i < 14; ++i)
            for (int j = i + 1; j < 14; ++j)
                LG_ARG(!packed_overlap(ptr[i], bytes[i], ptr[j], bytes[j]), "%s: operands %d and %d (of %s) overlap", name, i, j, operands);
        for (int i = 4; i < 14; ++i) { const int rc = adam_epilogue_check_write(ptr[i], bytes[i]); if (rc != LG_OK) return rc; }
    }
    const ServePackedArgs a{nxt, nxt_pitch, prompts, prompt_len, budget, prompt_pitch, out, out_len, out_pitch, queue, req, pos, count, cu, ids, position_ids,
                            last, int(P), int(G), int(N), int(slots), int(T), int(chunk), int(capacity), eos_id, rt().status_dev};
    hipLaunchKernelGGL(serve_commit_packed, dim3(1), dim3(unsigned((slots + 63) / 64 * 64)), 0, rt().stream, a);
    LG_CHECK_LAUNCH();
    return LG_OK;
}
