// The slot bookkeeping of one serving step over a PAGED key / value cache in ONE launch: lg_serve_commit_paged_i32.
//
// lg_serve_commit_i32 (serve.hip) with the cache rows of a slot reached through a table of blocks (nn.PagedKVCache): block_table
// (slots, max_blocks), held (slots,) the blocks a slot's table names, and `free` (num_blocks + 1,), a stack - word 0 the number n
// of free blocks, words 1 .. n their indices, the top at word n.  Blocks 0 .. F - 1 (F = prefix_blocks) hold a prefix every
// request shares: they are in every table and never on the stack.  The definition is the loop of `CpuTensor.serve_commit_paged`
// (autograd/cpu/ops.py); it is serve_commit with
//   release    a slot whose request has just finished pushes block_table[s, F .. held[s] - 1] onto the stack, slots in slot
//              order and each slot's blocks in table order; its table row becomes -1, held[s] = 0
//   admission  free slots, those just released included, are offered the waiting requests in slot and queue order; request r
//              needs ceil((prompt_len[r] + budget[r] - 1) / B) - F blocks for its whole life.  The first request that needs more
//              than the stack holds stops the admission of this commit: its slot and every later free slot stay free (no
//              overtaking).  Otherwise the slot pops its blocks into table words F .., takes 0 .. F - 1 in front, and starts at
//              position F * B with prompt tokens F * B ..
// One workgroup, a thread per slot, as serve_commit; step 1 of the definition, the slot's words and the rows of ids /
// position_ids are serve_body.h's serve_slot_request and serve_write_slots, which the two kernels share.  The slots depend on each other through three exclusive scans in slot
// order: the blocks pushed in front of a slot (where its own go on the stack), the free slots in front of it (which request it is
// offered), and the blocks needed in front of it (which stack words it pops; the cumulative needs are monotone, so "stop at the
// first that does not fit" is a prefix of the free slots).  A barrier stands between the pushes and the pops.  Which block a slot
// gets is fixed by the definition: the tables, not only the tokens, are those of the numpy backend.
//
// A slot or request that would leave its bounds raises the status flag - LG_EINDEX at the next synchronisation -, gets count = 0
// and nothing else of it is written: a bounds check, never a fault.
#include "serve_body.h"

namespace lg {

struct PagedServeArgs {
    ServeOperands o;
    int32_t *block_table, *held, *free;
    int m, max_blocks, num_blocks, log2_block, prefix_blocks;
};

// inclusive sum of v over the threads in front of and including this one, and the sum over the workgroup; every thread calls
__device__ __forceinline__ int block_scan(int v, int* s_wave, int& total) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, waves = blockDim.x >> 6;
    int x = wave_inclusive_sum(v, lane);
    __syncthreads();                             // (the words may still be read from the scan before)
    if (lane == 63) s_wave[wave] = x;
    __syncthreads();
    total = 0;
    for (int w = 0; w < waves; ++w) {
        if (w < wave) x += s_wave[w];
        total += s_wave[w];
    }
    return x;
}

__global__ __launch_bounds__(kServeMaxSlots) void serve_commit_paged(const PagedServeArgs a) {
    __shared__ int s_n[kServeMaxSlots], s_t[kServeMaxSlots], s_row[kServeMaxSlots], s_tok[kServeMaxSlots];       // serve_write_slots'
    __shared__ int s_wave[kServeWaves];
    const ServeOperands& o = a.o;
    const int s = threadIdx.x;
    const int m = a.m, N = o.N, F = a.prefix_blocks, lb = a.log2_block, MB = a.max_blocks;
    const int capacity = MB << lb, start = F << lb;
    const int first = o.queue[0], n0 = a.free[0];        // read by every thread before thread 0 writes them (behind the barriers below)
    const bool stack_ok = n0 >= 0 && n0 <= a.num_blocks;
    int32_t* table = a.block_table + int64_t(s < o.b ? s : 0) * MB;

    // step 1: the slot's own request
    ServeSlot x = serve_slot_request(o, s, m, capacity);
    const bool finished = x.finished;
    // release: the blocks behind the shared prefix go back on the stack, slots in slot order
    int push = 0, all_done = 0;
    if (finished) {
        const int h = a.held[s];
        bool ok = stack_ok && h >= 0 && h <= MB;
        if (ok)
            for (int i = F; i < h; ++i) ok = ok && table[i] >= 0 && table[i] < a.num_blocks;
        if (ok) push = h > F ? h - F : 0;
        else x.fault = true;
    }
    block_scan(finished ? 1 : 0, s_wave, all_done);
    int pushed = 0;
    const int behind = block_scan(push, s_wave, pushed);
    const bool overflow = stack_ok && int64_t(n0) + pushed > a.num_blocks;
    if (finished && !x.fault) {
        if (overflow) {
            x.fault = true;
        } else {
            for (int i = 0; i < push; ++i) a.free[1 + n0 + (behind - push) + i] = table[F + i];
            for (int i = 0; i < MB; ++i) table[i] = -1;
            a.held[s] = 0;
        }
    }
    const int avail = !stack_ok ? 0 : (overflow ? n0 : n0 + pushed);
    __syncthreads();                             // the pushes are on the stack before anybody pops

    // admission: free slots in slot order take the waiting requests in queue order while their blocks fit
    const bool is_free = s < o.b && !x.fault && x.r < 0;
    int all_free = 0;
    const int rank = block_scan(is_free ? 1 : 0, s_wave, all_free) - (is_free ? 1 : 0);
    bool offered = false, refused = false;
    int need = 0, rr = -1, nn = 0;
    if (is_free && first >= 0 && int64_t(first) + rank < N) {
        offered = true;
        rr = first + rank;
        const int len = o.prompt_len[rr];
        const int64_t rows = int64_t(len) + o.budget[rr] - 1;
        const int64_t want = ((rows + (int64_t(1) << lb) - 1) >> lb) - F;
        const int64_t tokens = int64_t(len) - start < m ? int64_t(len) - start : m;
        refused = !stack_ok || want < 0 || F + want > MB || tokens < 1 || start + tokens > o.P;
        need = refused ? 0 : int(want);
        nn = int(tokens);
    }
    int needed = 0, admitted_all = 0, popped = 0;
    const int upto = block_scan(need, s_wave, needed);
    const bool admitted = offered && upto <= avail;
    block_scan(admitted ? 1 : 0, s_wave, admitted_all);
    block_scan(admitted ? need : 0, s_wave, popped);
    if (is_free) x.t = 0;
    if (admitted) {
        if (refused) {
            x.fault = true;
        } else {
            x.r = rr;
            x.t = start;
            x.n = nn;
            x.row = rr;
            const int top = avail - (upto - need);           // the stack's top when this slot's turn comes
            for (int i = 0; i < need; ++i) table[F + i] = a.free[top - i];
            for (int i = 0; i < F; ++i) table[i] = i;
            a.held[s] = F + need;
        }
    }
    if (s == 0) {
        o.queue[0] = first + admitted_all;
        o.queue[1] += all_done;
        if (stack_ok) a.free[0] = avail - popped;
    }
    // steps 3 and 4: the slot's words and the step's inputs
    serve_write_slots(o, x, s, m, capacity, s_n, s_t, s_row, s_tok);
}

}  // namespace lg

using namespace lg;

extern "C" int lg_serve_commit_paged_i32(const int32_t* nxt, int64_t nxt_pitch, const int32_t* prompts, int64_t prompt_pitch, int64_t P,
                                         const int32_t* prompt_len, const int32_t* budget, int32_t* out, int64_t out_pitch, int64_t G,
                                         int32_t* out_len, int32_t* queue, int64_t N, int32_t* req, int32_t* pos, int32_t* count, int32_t* ids,
                                         int32_t* position_ids, int32_t* last, int32_t* block_table, int32_t* held, int32_t* free_stack,
                                         int64_t slots, int64_t m, int64_t max_blocks, int64_t num_blocks, int64_t log2_block,
                                         int64_t prefix_blocks, int32_t eos_id) {
    LG_REQUIRE_INIT();
    const char* name = "lg_serve_commit_paged_i32";
    const int64_t lim = int64_t(1) << 31;
    LG_ARG(slots >= 0 && slots <= kServeMaxSlots && m >= 1 && slots * m < lim && N >= 1 && N < lim && P >= 1 && P < lim && G >= 1 && G < lim,
           "%s: slots = %lld (0 .. 1024), m = %lld, N = %lld, P = %lld, G = %lld (each 1 .. 2^31 - 1, slots * m too) unsupported", name,
           (long long)slots, (long long)m, (long long)N, (long long)P, (long long)G);
    LG_ARG(log2_block >= 2 && log2_block <= 7 && max_blocks >= 1 && (max_blocks << log2_block) <= 512 && num_blocks >= 1 &&
               (num_blocks << log2_block) < lim && prefix_blocks >= 0 && prefix_blocks <= max_blocks && prefix_blocks <= num_blocks,
           "%s: blocks of 1 << %lld rows (4 .. 128), %lld per table (capacity 1 .. 512), %lld in the pool, %lld of them a shared prefix unsupported", name,
           (long long)log2_block, (long long)max_blocks, (long long)num_blocks, (long long)prefix_blocks);
    if (slots == 0) return LG_OK;
    const ServeOperands o{nxt, nxt_pitch, prompts, prompt_len, budget, prompt_pitch, out, out_len, out_pitch, queue, req, pos, count, ids, position_ids, last,
                          int(P), int(G), int(N), int(slots), eos_id, rt().status_dev};
    const void* ptr[16] = {nxt, prompts, prompt_len, budget, out, out_len, queue, req, pos, count, ids, position_ids, last, block_table, held, free_stack};
    const int64_t bytes[16] = {((slots - 1) * nxt_pitch + 1) * 4, ((N - 1) * prompt_pitch + P) * 4, N * 4, N * 4, ((N - 1) * out_pitch + G) * 4, N * 4, 8,
                               slots * 4, slots * 4, slots * 4, slots * m * 4, slots * m * 4, slots * 4, slots * max_blocks * 4, slots * 4,
                               (num_blocks + 1) * 4};
    const int rc = serve_check_operands(name, "nxt, prompts, prompt_len, budget, out, out_len, queue, req, pos, count, ids, position_ids, last, block_table, held, free",
                                        o, ptr, bytes, 16, 4);
    if (rc != LG_OK) return rc;
    const PagedServeArgs a{o, block_table, held, free_stack, int(m), int(max_blocks), int(num_blocks), int(log2_block), int(prefix_blocks)};
    hipLaunchKernelGGL(serve_commit_paged, dim3(1), dim3(unsigned((slots + 63) / 64 * 64)), 0, rt().stream, a);
    LG_CHECK_LAUNCH();
    return LG_OK;
}
