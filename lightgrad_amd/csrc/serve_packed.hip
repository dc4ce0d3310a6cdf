// The slot bookkeeping of one TOKEN-PACKED step of continuous batching in ONE launch: lg_serve_commit_packed_i32.
//
// lg_serve_commit_i32 (serve.hip) lays a step out as (slots, m) rows: a slot that decodes one token still carries m rows through
// the model.  Here the step is T token rows for all slots together - the token budget, T >= slots - and slot s owns rows
// cu[s] .. cu[s + 1] - 1 of them.  What a slot WANTS is decided as there, by serve_body.h's serve_slot_request and serve_admit
// with m = chunk (steps 1 and 2 of the definition: the next piece of its prompt, the token just drawn, a waiting request admitted
// to a free slot in slot order); what it GETS is the budget's: every decoding slot its one token, and the R = T - (decoding
// slots) rows left go to the prefilling slots in slot order, n = min(want, what is left).  A prefilling slot granted 0 keeps its
// request and its position and asks again in the next step.  The definition is the sequential loop of
// `CpuTensor.serve_commit_packed` (autograd/cpu/ops.py).
//
// One workgroup, one thread per slot (slots <= 1024).  A slot depends on the others through three exclusive sums in slot order,
// each taken inside a wave (a ballot for the flags, a shuffle scan for the numbers) and across the waves through per-wave totals
// in LDS: its rank among the free slots (the admission order), the wants of the prefilling slots in front of it
// (grant = clamp(R - prefix, 0, want)), and the rows granted in front of it (cu).  The step's T ids and position ids are then
// written by all threads together, coalesced; a row finds its slot by bisection of cu in LDS.
//
// A slot that would leave its bounds (see the definition) raises the status flag - LG_EINDEX at the next synchronisation -, gets
// count = 0, takes no rows and nothing else of it is written: a bounds check, never a fault.
#include "serve_body.h"

namespace lg {

struct ServePackedArgs {
    ServeOperands o;
    int32_t* cu;
    int T, chunk, capacity;
};

__global__ __launch_bounds__(kServeMaxSlots) void serve_commit_packed(const ServePackedArgs a) {
    __shared__ int s_cu[kServeMaxSlots + 1];     // the first row of the slot; [b]: the rows in use
    __shared__ int s_t[kServeMaxSlots];          // position of its token 0
    __shared__ int s_row[kServeMaxSlots];        // the request whose prompt the tokens come from, -1: the one token s_tok
    __shared__ int s_tok[kServeMaxSlots];
    __shared__ int s_free[kServeWaves], s_done[kServeWaves], s_dec[kServeWaves], s_want[kServeWaves], s_grant[kServeWaves];
    const ServeOperands& o = a.o;
    const int s = threadIdx.x, lane = s & 63, wave = s >> 6, waves = blockDim.x >> 6;
    const int T = a.T;
    const int first = o.queue[0];                // read by every thread before thread 0 writes it (behind the barrier of serve_admit)

    // steps 1 and 2: what the slot wants
    ServeSlot x = serve_slot_request(o, s, a.chunk, a.capacity);
    serve_admit(o, x, s, a.chunk, first, s_free, s_done);
    // a slot whose want would leave the cache takes no rows, whatever the budget would grant it
    const bool fault = x.fault || int64_t(x.t) + x.n > a.capacity;
    int n = fault ? 0 : x.n;
    // step 3: the budget.  Every decoding slot its token; the prefilling slots share the R rows left, in slot order
    const bool decoding = s < o.b && !fault && x.row < 0 && n == 1;
    const int want = (s < o.b && !fault && x.row >= 0) ? n : 0;
    const unsigned long long dec_mask = __ballot(decoding);
    const int want_upto = wave_inclusive_sum(want, lane);
    if (lane == 63) { s_dec[wave] = __popcll(dec_mask); s_want[wave] = want_upto; }
    __syncthreads();
    int all_dec = 0, before = want_upto - want;
    for (int w = 0; w < waves; ++w) {
        all_dec += s_dec[w];
        if (w < wave) before += s_want[w];
    }
    const int R = T - all_dec, left = R - before;                 // (R >= 1 whenever a slot prefills: T >= slots)
    if (!decoding) n = left < 0 ? 0 : (left < want ? left : want);
    // step 4: the slot's rows - the exclusive sum of the grants
    const int grant_upto = wave_inclusive_sum(n, lane);
    if (lane == 63) s_grant[wave] = grant_upto;
    __syncthreads();
    int used = 0, start = grant_upto - n;
    for (int w = 0; w < waves; ++w) {
        if (w < wave) start += s_grant[w];
        used += s_grant[w];
    }
    if (s < o.b) {
        if (fault) {
            __hip_atomic_fetch_or(o.status, LG_STATUS_BAD_INDEX, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
            o.count[s] = 0;
        } else {
            const int end = start + (n > 0 ? n - 1 : 0);
            o.req[s] = x.r;
            o.pos[s] = x.t;
            o.count[s] = n;
            o.last[s] = end < T - 1 ? end : T - 1;                // an idle slot behind a full buffer must not name row T
        }
        a.cu[s] = start;
        if (s == 0) a.cu[o.b] = used;
        s_cu[s] = start;
        if (s == 0) s_cu[o.b] = used;
        s_t[s] = x.t;
        s_row[s] = x.row;
        s_tok[s] = x.tok;
    }
    __syncthreads();
    // the step's inputs: T words each, consecutive threads on consecutive words.  Row e < used belongs to the LAST slot whose
    // first row is <= e (the slots in front of it that start there own no row)
    for (int e = s; e < T; e += blockDim.x) {
        int id = 0, position = 0;
        if (e < used) {
            int lo = 0, hi = o.b;                                 // s_cu[lo] <= e < s_cu[hi]
            while (hi - lo > 1) {
                const int mid = (lo + hi) >> 1;
                if (s_cu[mid] <= e) lo = mid; else hi = mid;
            }
            const int i = e - s_cu[lo];
            id = s_row[lo] >= 0 ? o.prompts[int64_t(s_row[lo]) * o.prompt_pitch + s_t[lo] + i] : s_tok[lo];
            position = s_t[lo] + i;
        }
        o.ids[e] = id;
        o.position_ids[e] = position;
    }
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
    LG_ARG(slots >= 0 && slots <= kServeMaxSlots && chunk >= 1 && chunk < lim && slots * chunk < lim && T >= 1 && T >= slots && T < lim && N >= 1 && N < lim &&
               P >= 1 && P < lim && G >= 1 && G < lim && capacity >= 1 && capacity < lim,
           "%s: slots = %lld (0 .. 1024), T = %lld (>= slots), chunk = %lld, N = %lld, P = %lld, G = %lld, capacity = %lld (each 1 .. 2^31 - 1, slots * chunk too) unsupported",
           name, (long long)slots, (long long)T, (long long)chunk, (long long)N, (long long)P, (long long)G, (long long)capacity);
    if (slots == 0) return LG_OK;
    const ServeOperands o{nxt, nxt_pitch, prompts, prompt_len, budget, prompt_pitch, out, out_len, out_pitch, queue, req, pos, count, ids, position_ids, last,
                          int(P), int(G), int(N), int(slots), eos_id, rt().status_dev};
    const void* ptr[14] = {nxt, prompts, prompt_len, budget, out, out_len, queue, req, pos, count, cu, ids, position_ids, last};
    const int64_t bytes[14] = {((slots - 1) * nxt_pitch + 1) * 4, ((N - 1) * prompt_pitch + P) * 4, N * 4, N * 4, ((N - 1) * out_pitch + G) * 4, N * 4, 8,
                               slots * 4, slots * 4, slots * 4, (slots + 1) * 4, T * 4, T * 4, slots * 4};
    const int rc = serve_check_operands(name, "nxt, prompts, prompt_len, budget, out, out_len, queue, req, pos, count, cu, ids, position_ids, last", o, ptr, bytes, 14, 4);
    if (rc != LG_OK) return rc;
    const ServePackedArgs a{o, cu, int(T), int(chunk), int(capacity)};
    hipLaunchKernelGGL(serve_commit_packed, dim3(1), dim3(unsigned((slots + 63) / 64 * 64)), 0, rt().stream, a);
    LG_CHECK_LAUNCH();
    return LG_OK;
}
