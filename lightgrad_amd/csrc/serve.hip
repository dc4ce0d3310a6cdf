// The slot bookkeeping of one step of continuous batching in ONE launch: lg_serve_commit_i32.
//
// A serving step runs b cache slots through the model, m token rows each: a slot decodes (one real token), prefills a piece of
// its prompt (up to m), or idles (none).  Between two steps every slot moves on: the tokens of the step are in the cache now
// (pos += count); a prefilling slot takes the next piece of its prompt; a decoding slot stores the token just drawn, and either
// feeds it back or - end-of-sequence id, budget used up - finishes its request and becomes free; a free slot takes the next
// waiting request, in slot order, and starts on its prompt in the same launch.  The definition is the sequential loop of
// `CpuTensor.serve_commit` (autograd/cpu/ops.py); as tensor expressions it is a dozen launches in a step that is bound by its
// launch boundaries.
//
// One workgroup, one thread per slot (b <= 1024).  What a slot decides depends on the other slots through ONE number only: how
// many free slots stand in front of it - its rank in the admission order.  So: every thread settles its own slot (step 1 of the
// definition), the free flags are counted per wave with a ballot and summed over the waves in front through LDS (an exclusive
// scan in slot order), slot s takes request queue[0] + rank if that is < N, and thread 0 moves the two queue words.  A request is
// held by at most one slot, so no two threads write the same word of out / out_len.  The step's ids and position ids, b * m
// words each, are then written by all threads together, coalesced, from what the slots left in LDS.
//
// A slot that would leave its bounds (see the definition) raises the status flag - LG_EINDEX at the next synchronisation -, gets
// count = 0 and nothing else of it is written: a bounds check, never a fault.
#include "common.h"

namespace lg {

constexpr int kServeMaxSlots = 1024;

struct ServeArgs {
    const int32_t* nxt;                  // slot s reads nxt[s * nxt_pitch]
    int64_t nxt_pitch;
    const int32_t *prompts, *prompt_len, *budget;        // prompts: request r, token i at prompts + r * prompt_pitch + i
    int64_t prompt_pitch;
    int32_t *out, *out_len;              // out: request r, token g at out + r * out_pitch + g
    int64_t out_pitch;
    int32_t *queue, *req, *pos, *count, *ids, *position_ids, *last;
    int P, G, N, b, m, capacity;
    int32_t eos_id;
    int* status;
};

__global__ __launch_bounds__(kServeMaxSlots) void serve_commit(const ServeArgs a) {
    __shared__ int s_n[kServeMaxSlots];          // real tokens of the slot; -1: the slot keeps its bytes
    __shared__ int s_t[kServeMaxSlots];          // position of its token 0
    __shared__ int s_row[kServeMaxSlots];        // the request whose prompt the tokens come from, -1: the one token s_tok
    __shared__ int s_tok[kServeMaxSlots];
    __shared__ int s_free[kServeMaxSlots / 64], s_done[kServeMaxSlots / 64];
    const int s = threadIdx.x, lane = s & 63, wave = s >> 6, waves = blockDim.x >> 6;
    const int m = a.m, N = a.N;
    const int first = a.queue[0];                // read by every thread before thread 0 writes it (behind the barrier below)

    // step 1: the slot's own request
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
                    n = len - t < m ? len - t : m;
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
            n = len < m ? len : m;
            row = r;
            fault = n < 0 || n > a.P;
        }
    }
    if (s == 0) {
        const int64_t waiting = first < 0 ? 0 : int64_t(N) - first;
        a.queue[0] = first + int(waiting < all_free ? (waiting < 0 ? 0 : waiting) : all_free);
        a.queue[1] += all_done;
    }
    // steps 3 and 4: the slot's words
    if (s < a.b) {
        if (fault || int64_t(t) + n > a.capacity) {
            __hip_atomic_fetch_or(a.status, LG_STATUS_BAD_INDEX, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
            a.count[s] = 0;
            n = -1;
        } else {
            a.req[s] = r;
            a.pos[s] = t;
            a.count[s] = n;
            a.last[s] = s * m + (n > 0 ? n - 1 : 0);
        }
        s_n[s] = n;
        s_t[s] = t;
        s_row[s] = row;
        s_tok[s] = tok;
    }
    __syncthreads();
    // the step's inputs: b * m words each, consecutive threads on consecutive words
    for (int e = s; e < a.b * m; e += blockDim.x) {
        const int slot = e / m, i = e - slot * m, k = s_n[slot];
        if (k < 0) continue;
        int id = 0;
        if (i < k) id = s_row[slot] >= 0 ? a.prompts[int64_t(s_row[slot]) * a.prompt_pitch + s_t[slot] + i] : s_tok[slot];
        a.ids[e] = id;
        a.position_ids[e] = i < k ? s_t[slot] + i : 0;
    }
}

// do the bytes [x, x + nx) and [y, y + ny) share an address?
static bool serve_overlap(const void* x, int64_t nx, const void* y, int64_t ny) {
    const char *a = static_cast<const char*>(x), *b = static_cast<const char*>(y);
    return a < b + ny && b < a + nx;
}

}  // namespace lg

using namespace lg;

extern "C" int lg_serve_commit_i32(const int32_t* nxt, int64_t nxt_pitch, const int32_t* prompts, int64_t prompt_pitch, int64_t P,
                                   const int32_t* prompt_len, const int32_t* budget, int32_t* out, int64_t out_pitch, int64_t G,
                                   int32_t* out_len, int32_t* queue, int64_t N, int32_t* req, int32_t* pos, int32_t* count, int32_t* ids,
                                   int32_t* position_ids, int32_t* last, int64_t slots, int64_t m, int64_t capacity, int32_t eos_id) {
    LG_REQUIRE_INIT();
    const char* name = "lg_serve_commit_i32";
    const int64_t lim = int64_t(1) << 31;
    LG_ARG(slots >= 0 && slots <= kServeMaxSlots && m >= 1 && slots * m < lim && N >= 1 && N < lim && P >= 1 && P < lim && G >= 1 && G < lim &&
               capacity >= 1 && capacity < lim,
           "%s: slots = %lld (0 .. 1024), m = %lld, N = %lld, P = %lld, G = %lld, capacity = %lld (each 1 .. 2^31 - 1, slots * m too) unsupported", name,
           (long long)slots, (long long)m, (long long)N, (long long)P, (long long)G, (long long)capacity);
    if (slots == 0) return LG_OK;
    const void* ptr[13] = {nxt, prompts, prompt_len, budget, out, out_len, queue, req, pos, count, ids, position_ids, last};
    for (int i = 0; i < 13; ++i) LG_ARG(ptr[i], "%s: NULL operand %d (of nxt, prompts, prompt_len, budget, out, out_len, queue, req, pos, count, ids, position_ids, last)", name, i);
    for (int i = 0; i < 13; ++i) LG_ARG((reinterpret_cast<uintptr_t>(ptr[i]) & 3u) == 0, "%s: operand %d must be 4-byte aligned", name, i);
    LG_ARG(nxt_pitch >= 1 && prompt_pitch >= P && out_pitch >= G, "%s: row pitches %lld (nxt, >= 1) / %lld (prompts, >= P = %lld) / %lld (out, >= G = %lld)",
           name, (long long)nxt_pitch, (long long)prompt_pitch, (long long)P, (long long)out_pitch, (long long)G);
    {
        // a thread writes its slot's words and its request's words: bytes shared by two operands would make the result depend on
        // which thread ran first
        const int64_t bytes[13] = {((slots - 1) * nxt_pitch + 1) * 4, ((N - 1) * prompt_pitch + P) * 4, N * 4, N * 4, ((N - 1) * out_pitch + G) * 4, N * 4, 8,
                                   slots * 4, slots * 4, slots * 4, slots * m * 4, slots * m * 4, slots * 4};
        for (int i = 0; i < 13; ++i)
            for (int j = i + 1; j < 13; ++j)
                LG_ARG(!serve_overlap(ptr[i], bytes[i], ptr[j], bytes[j]), "%s: operands %d and %d (of nxt, prompts, prompt_len, budget, out, out_len, queue, req, pos, count, ids, position_ids, last) overlap", name, i, j);
        for (int i = 4; i < 13; ++i) { const int rc = adam_epilogue_check_write(ptr[i], bytes[i]); if (rc != LG_OK) return rc; }
    }
    const ServeArgs a{nxt, nxt_pitch, prompts, prompt_len, budget, prompt_pitch, out, out_len, out_pitch, queue, req, pos, count, ids, position_ids, last,
                      int(P), int(G), int(N), int(slots), int(m), int(capacity), eos_id, rt().status_dev};
    hipLaunchKernelGGL(serve_commit, dim3(1), dim3(unsigned((slots + 63) / 64 * 64)), 0, rt().stream, a);
    LG_CHECK_LAUNCH();
    return LG_OK;
}
