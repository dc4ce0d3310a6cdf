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
// words each, are then written by all threads together, coalesced, from what the slots left in LDS.  The three pieces are
// serve_body.h's, which the packed and the paged commit (serve_packed.hip, serve_paged.hip) share; the LDS is this kernel's.
//
// A slot that would leave its bounds (see the definition) raises the status flag - LG_EINDEX at the next synchronisation -, gets
// count = 0 and nothing else of it is written: a bounds check, never a fault.
#include "serve_body.h"

namespace lg {

struct ServeArgs {
    ServeOperands o;
    int m, capacity;
};

__global__ __launch_bounds__(kServeMaxSlots) void serve_commit(const ServeArgs a) {
    __shared__ int s_n[kServeMaxSlots], s_t[kServeMaxSlots], s_row[kServeMaxSlots], s_tok[kServeMaxSlots];       // serve_write_slots'
    __shared__ int s_free[kServeWaves], s_done[kServeWaves];
    const int s = threadIdx.x;
    const int first = a.o.queue[0];              // read by every thread before thread 0 writes it (behind the barrier of serve_admit)
    ServeSlot x = serve_slot_request(a.o, s, a.m, a.capacity);
    serve_admit(a.o, x, s, a.m, first, s_free, s_done);
    serve_write_slots(a.o, x, s, a.m, a.capacity, s_n, s_t, s_row, s_tok);
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
    const ServeOperands o{nxt, nxt_pitch, prompts, prompt_len, budget, prompt_pitch, out, out_len, out_pitch, queue, req, pos, count, ids, position_ids, last,
                          int(P), int(G), int(N), int(slots), eos_id, rt().status_dev};
    const void* ptr[13] = {nxt, prompts, prompt_len, budget, out, out_len, queue, req, pos, count, ids, position_ids, last};
    const int64_t bytes[13] = {((slots - 1) * nxt_pitch + 1) * 4, ((N - 1) * prompt_pitch + P) * 4, N * 4, N * 4, ((N - 1) * out_pitch + G) * 4, N * 4, 8,
                               slots * 4, slots * 4, slots * 4, slots * m * 4, slots * m * 4, slots * 4};
    const int rc = serve_check_operands(name, "nxt, prompts, prompt_len, budget, out, out_len, queue, req, pos, count, ids, position_ids, last", o, ptr, bytes, 13, 4);
    if (rc != LG_OK) return rc;
    const ServeArgs a{o, int(m), int(capacity)};
    hipLaunchKernelGGL(serve_commit, dim3(1), dim3(unsigned((slots + 63) / 64 * 64)), 0, rt().stream, a);
    LG_CHECK_LAUNCH();
    return LG_OK;
}
