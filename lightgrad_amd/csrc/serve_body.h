// What the three commit kernels of a serving step share: serve_commit (serve.hip), serve_commit_packed (serve_packed.hip) and
// serve_commit_paged (serve_paged.hip).  Each is one workgroup with a thread per slot; each lays the step out differently
// ((slots, m) rows, T packed rows, rows behind a block table), and each does the same with a slot's own request.  Here, once:
//   ServeOperands          the operands every commit takes
//   serve_slot_request     step 1 of the definition (`CpuTensor.serve_commit`, autograd/cpu/ops.py): the slot's own request
//   serve_admit            step 2, plain and packed: a free slot takes request queue[0] + its rank among the free slots
//   serve_write_slots      steps 3 and 4, plain and paged: the slot's words and the (b, m) rows of ids / position_ids
//   wave_inclusive_sum     the shuffle scan inside a wave, packed and paged
//   serve_check_operands   the host's refusals: NULL, alignment, pitches, operands that share bytes
// The helpers declare no LDS of their own: the arrays are the calling kernel's, which sizes them.
#pragma once
#include "common.h"

namespace lg {

constexpr int kServeMaxSlots = 1024;
constexpr int kServeWaves = kServeMaxSlots / 64;

struct ServeOperands {
    const int32_t* nxt;                  // slot s reads nxt[s * nxt_pitch]
    int64_t nxt_pitch;
    const int32_t *prompts, *prompt_len, *budget;        // prompts: request r, token i at prompts + r * prompt_pitch + i
    int64_t prompt_pitch;
    int32_t *out, *out_len;              // out: request r, token g at out + r * out_pitch + g
    int64_t out_pitch;
    int32_t *queue, *req, *pos, *count, *ids, *position_ids, *last;
    int P, G, N, b;
    int32_t eos_id;
    int* status;
};

// what a slot does in the coming step: n tokens from position t on - of the prompt of request `row`, or (row < 0) the one token tok
struct ServeSlot {
    int r, t, n, row, tok;
    bool fault, finished;
};

// the sum of v over the lanes in front of and including this one
__device__ __forceinline__ int wave_inclusive_sum(int v, int lane) {
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
        const int o = __shfl_up(v, off, 64);
        if (lane >= off) v += o;
    }
    return v;
}

// step 1: the slot's own request.  `m`: the most token rows a slot takes in a step
__device__ __forceinline__ ServeSlot serve_slot_request(const ServeOperands& a, int s, int m, int capacity) {
    ServeSlot x{-1, 0, 0, -1, 0, false, false};
    if (s >= a.b) return x;
    x.r = a.req[s];
    if (x.r < 0) return x;
    const int r = x.r;
    const int64_t tt = int64_t(a.pos[s]) + a.count[s];
    if (r >= a.N || tt < 0 || tt > capacity) {
        x.fault = true;
        return x;
    }
    x.t = int(tt);
    const int len = a.prompt_len[r];
    if (x.t < len) {
        x.n = len - x.t < m ? len - x.t : m;
        x.row = r;
        x.fault = x.t + x.n > a.P;
        return x;
    }
    const int g = a.out_len[r];
    if (g < 0 || g >= a.G) {
        x.fault = true;
        return x;
    }
    x.tok = a.nxt[int64_t(s) * a.nxt_pitch];
    a.out[int64_t(r) * a.out_pitch + g] = x.tok;
    a.out_len[r] = g + 1;
    if ((a.eos_id >= 0 && x.tok == a.eos_id) || g + 1 == a.budget[r]) {
        x.finished = true;
        x.r = -1;
    } else {
        x.n = 1;
    }
    return x;
}

// step 2: the admission order - free slots in slot order.  The free flags are counted per wave with a ballot and summed over the
// waves in front through s_free (kServeWaves words, as s_done): slot s takes request first + rank if that is < N and starts on
// its prompt; thread 0 moves the two queue words.  `first` is queue[0] as every thread read it before this call.  Every thread
// calls; one barrier.
__device__ __forceinline__ void serve_admit(const ServeOperands& a, ServeSlot& x, int s, int m, int first, int* s_free, int* s_done) {
    const int lane = s & 63, wave = s >> 6, waves = blockDim.x >> 6;
    const bool is_free = s < a.b && !x.fault && x.r < 0;
    const unsigned long long free_mask = __ballot(is_free), done_mask = __ballot(x.finished);
    if (lane == 0) { s_free[wave] = __popcll(free_mask); s_done[wave] = __popcll(done_mask); }
    __syncthreads();
    int rank = __popcll(free_mask & ((1ull << lane) - 1ull)), all_free = 0, all_done = 0;
    for (int w = 0; w < waves; ++w) {
        if (w < wave) rank += s_free[w];
        all_free += s_free[w];
        all_done += s_done[w];
    }
    if (is_free) {
        x.t = 0;
        if (int64_t(first) + rank < a.N && first >= 0) {
            x.r = first + rank;
            const int len = a.prompt_len[x.r];
            x.n = len < m ? len : m;
            x.row = x.r;
            x.fault = x.n < 0 || x.n > a.P;
        }
    }
    if (s == 0) {
        const int64_t waiting = first < 0 ? 0 : int64_t(a.N) - first;
        a.queue[0] = first + int(waiting < all_free ? (waiting < 0 ? 0 : waiting) : all_free);
        a.queue[1] += all_done;
    }
}

// steps 3 and 4 for a step of (b, m) rows: the slot's words, then - all threads together, consecutive threads on consecutive
// words - the b * m words of ids and of position_ids from what the slots left in the four LDS arrays (kServeMaxSlots words each).
// A slot that would leave its bounds raises the status flag, gets count = 0 and keeps its other bytes.  Every thread calls; one
// barrier.
__device__ __forceinline__ void serve_write_slots(const ServeOperands& a, const ServeSlot& x, int s, int m, int capacity, int* s_n, int* s_t,
                                                  int* s_row, int* s_tok) {
    if (s < a.b) {
        int n = x.n;
        if (x.fault || int64_t(x.t) + n > capacity) {
            __hip_atomic_fetch_or(a.status, LG_STATUS_BAD_INDEX, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
            a.count[s] = 0;
            n = -1;
        } else {
            a.req[s] = x.r;
            a.pos[s] = x.t;
            a.count[s] = n;
            a.last[s] = s * m + (n > 0 ? n - 1 : 0);
        }
        s_n[s] = n;                              // real tokens of the slot; -1: the slot keeps its bytes
        s_t[s] = x.t;                            // position of its token 0
        s_row[s] = x.row;                        // the request whose prompt the tokens come from, -1: the one token s_tok
        s_tok[s] = x.tok;
    }
    __syncthreads();
    for (int e = s; e < a.b * m; e += blockDim.x) {
        const int slot = e / m, i = e - slot * m, k = s_n[slot];
        if (k < 0) continue;
        int id = 0;
        if (i < k) id = s_row[slot] >= 0 ? a.prompts[int64_t(s_row[slot]) * a.prompt_pitch + s_t[slot] + i] : s_tok[slot];
        a.ids[e] = id;
        a.position_ids[e] = i < k ? s_t[slot] + i : 0;
    }
}

// The refusals every commit entry shares, in this order: a NULL operand, one that is not 4-byte aligned, a row pitch below its
// row, two operands that share bytes - a thread writes its slot's words and its request's words, so shared bytes would make the
// result depend on which thread ran first - and a write into a gradient whose update has been applied.  `operands` names the n
// of them in the order of ptr / bytes; those from `first_written` on are written.
static int serve_check_operands(const char* name, const char* operands, const ServeOperands& a, const void* const* ptr, const int64_t* bytes, int n,
                                int first_written) {
    for (int i = 0; i < n; ++i) LG_ARG(ptr[i], "%s: NULL operand %d (of %s)", name, i, operands);
    for (int i = 0; i < n; ++i) LG_ARG((reinterpret_cast<uintptr_t>(ptr[i]) & 3u) == 0, "%s: operand %d must be 4-byte aligned", name, i);
    LG_ARG(a.nxt_pitch >= 1 && a.prompt_pitch >= a.P && a.out_pitch >= a.G, "%s: row pitches %lld (nxt, >= 1) / %lld (prompts, >= P = %d) / %lld (out, >= G = %d)",
           name, (long long)a.nxt_pitch, (long long)a.prompt_pitch, a.P, (long long)a.out_pitch, a.G);
    for (int i = 0; i < n; ++i)
        for (int j = i + 1; j < n; ++j)
            LG_ARG(!bytes_overlap(ptr[i], bytes[i], ptr[j], bytes[j]), "%s: operands %d and %d (of %s) overlap", name, i, j, operands);
    for (int i = first_written; i < n; ++i) { const int rc = adam_epilogue_check_write(ptr[i], bytes[i]); if (rc != LG_OK) return rc; }
    return LG_OK;
}

}  // namespace lg
