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
// One workgroup, a thread per slot, as serve_commit.  The slots depend on each other through three exclusive scans in slot
// order: the blocks pushed in front of a slot (where its own go on the stack), the free slots in front of it (which request it is
// offered), and the blocks needed in front of it (which stack words it pops; the cumulative needs are monotone, so "stop at the
// first that does not fit" is a prefix of the free slots).  A barrier stands between the pushes and the pops.  Which block a slot
// gets is fixed by the definition: the tables, not only the tokens, are those of the numpy backend.
//
// A slot or request that would leave its bounds raises the status flag - LG_EINDEX at the next synchronisation -, gets count = 0
// and nothing else of it is written: a bounds check, never a fault.
#include "common.h"

namespace lg {

constexpr int kPagedServeMaxSlots = 1024;

struct PagedServeArgs {
    const int32_t* nxt;                  // slot s reads nxt[s * nxt_pitch]
    int64_t nxt_pitch;
    const int32_t *prompts, *prompt_len, *budget;        // prompts: request r, token i at prompts + r * prompt_pitch + i
    int64_t prompt_pitch;
    int32_t *out, *out_len;              // out: request r, token g at out + r * out_pitch + g
    int64_t out_pitch;
    int32_t *queue, *req, *pos, *count, *ids, *position_ids, *last;
    int32_t *block_table, *held, *free;
    int P, G, N, b, m, max_blocks, num_blocks, log2_block, prefix_blocks;
    int32_t eos_id;
    int* status;
};

// inclusive sum of v over the threads in front of and including this one, and the sum over the workgroup; every thread calls
__device__ __forceinline__ int block_scan(int v, int* s_wave, int& total) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, waves = blockDim.x >> 6;
    int x = v;
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
        const int y = __shfl_up(x, off, 64);
        if (lane >= off) x += y;
    }
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

__global__ __launch_bounds__(kPagedServeMaxSlots) void serve_commit_paged(const PagedServeArgs a) {
    __shared__ int s_n[kPagedServeMaxSlots];     // real tokens of the slot; -1: the slot keeps its bytes
    __shared__ int s_t[kPagedServeMaxSlots];     // position of its token 0
    __shared__ int s_row[kPagedServeMaxSlots];   // the request whose prompt the tokens come from, -1: the one token s_tok
    __shared__ int s_tok[kPagedServeMaxSlots];
    __shared__ int s_wave[kPagedServeMaxSlots / 64];
    const int s = threadIdx.x;
    const int m = a.m, N = a.N, F = a.prefix_blocks, lb = a.log2_block, MB = a.max_blocks;
    const int capacity = MB << lb, start = F << lb;
    const int first = a.queue[0], n0 = a.free[0];        // read by every thread before thread 0 writes them (behind the barriers below)
    const bool stack_ok = n0 >= 0 && n0 <= a.num_blocks;
    int32_t* table = a.block_table + int64_t(s < a.b ? s : 0) * MB;

    // step 1: the slot's own request
    int r = -1, t = 0, n = 0, row = -1, tok = 0;
    bool fault = false, finished = false;
    if (s < a.b) {
        r = a.req[s];
        if (r >= 0) {
            const int64_t tt = int64_t(a.pos[s]) + a.count[s];
            if (r >= N || tt < 0 || tt > capacity) {
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
    // release: the blocks behind the shared prefix go back on the stack, slots in slot order
    int push = 0, all_done = 0;
    if (finished) {
        const int h = a.held[s];
        bool ok = stack_ok && h >= 0 && h <= MB;
        if (ok)
            for (int i = F; i < h; ++i) ok = ok && table[i] >= 0 && table[i] < a.num_blocks;
        if (ok) push = h > F ? h - F : 0;
        else fault = true;
    }
    block_scan(finished ? 1 : 0, s_wave, all_done);
    int pushed = 0;
    const int behind = block_scan(push, s_wave, pushed);
    const bool overflow = stack_ok && int64_t(n0) + pushed > a.num_blocks;
    if (finished && !fault) {
        if (overflow) {
            fault = true;
        } else {
            for (int i = 0; i < push; ++i) a.free[1 + n0 + (behind - push) + i] = table[F + i];
            for (int i = 0; i < MB; ++i) table[i] = -1;
            a.held[s] = 0;
        }
    }
    const int avail = !stack_ok ? 0 : (overflow ? n0 : n0 + pushed);
    __syncthreads();                             // the pushes are on the stack before anybody pops

    // admission: free slots in slot order take the waiting requests in queue order while their blocks fit
    const bool is_free = s < a.b && !fault && r < 0;
    int all_free = 0;
    const int rank = block_scan(is_free ? 1 : 0, s_wave, all_free) - (is_free ? 1 : 0);
    bool offered = false, refused = false;
    int need = 0, rr = -1, nn = 0;
    if (is_free && first >= 0 && int64_t(first) + rank < N) {
        offered = true;
        rr = first + rank;
        const int len = a.prompt_len[rr];
        const int64_t rows = int64_t(len) + a.budget[rr] - 1;
        const int64_t want = ((rows + (int64_t(1) << lb) - 1) >> lb) - F;
        const int64_t tokens = int64_t(len) - start < m ? int64_t(len) - start : m;
        refused = !stack_ok || want < 0 || F + want > MB || tokens < 1 || start + tokens > a.P;
        need = refused ? 0 : int(want);
        nn = int(tokens);
    }
    int needed = 0, admitted_all = 0, popped = 0;
    const int upto = block_scan(need, s_wave, needed);
    const bool admitted = offered && upto <= avail;
    block_scan(admitted ? 1 : 0, s_wave, admitted_all);
    block_scan(admitted ? need : 0, s_wave, popped);
    if (is_free) t = 0;
    if (admitted) {
        if (refused) {
            fault = true;
        } else {
            r = rr;
            t = start;
            n = nn;
            row = rr;
            const int top = avail - (upto - need);           // the stack's top when this slot's turn comes
            for (int i = 0; i < need; ++i) table[F + i] = a.free[top - i];
            for (int i = 0; i < F; ++i) table[i] = i;
            a.held[s] = F + need;
        }
    }
    if (s == 0) {
        a.queue[0] = first + admitted_all;
        a.queue[1] += all_done;
        if (stack_ok) a.free[0] = avail - popped;
    }
    // steps 3 and 4: the slot's words
    if (s < a.b) {
        if (fault || int64_t(t) + n > capacity) {
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
static bool paged_serve_overlap(const void* x, int64_t nx, const void* y, int64_t ny) {
    const char *a = static_cast<const char*>(x), *b = static_cast<const char*>(y);
    return a < b + ny && b < a + nx;
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
    LG_ARG(slots >= 0 && slots <= kPagedServeMaxSlots && m >= 1 && slots * m < lim && N >= 1 && N < lim && P >= 1 && P < lim && G >= 1 && G < lim,
           "%s: slots = %lld (0 .. 1024), m = %lld, N = %lld, P = %lld, G = %lld (each 1 .. 2^31 - 1, slots * m too) unsupported", name,
           (long long)slots, (long long)m, (long long)N, (long long)P, (long long)G);
    LG_ARG(log2_block >= 2 && log2_block <= 7 && max_blocks >= 1 && (max_blocks << log2_block) <= 512 && num_blocks >= 1 &&
               (num_blocks << log2_block) < lim && prefix_blocks >= 0 && prefix_blocks <= max_blocks && prefix_blocks <= num_blocks,
           "%s: blocks of 1 << %lld rows (4 .. 128), %lld per table (capacity 1 .. 512), %lld in the pool, %lld of them a shared prefix unsupported", name,
           (long long)log2_block, (long long)max_blocks, (long long)num_blocks, (long long)prefix_blocks);
    if (slots == 0) return LG_OK;
    const void* ptr[16] = {nxt, prompts, prompt_len, budget, out, out_len, queue, req, pos, count, ids, position_ids, last, block_table, held, free_stack};
    const char* names = "nxt, prompts, prompt_len, budget, out, out_len, queue, req, pos, count, ids, position_ids, last, block_table, held, free";
    for (int i = 0; i < 16; ++i) LG_ARG(ptr[i], "%s: NULL operand %d (of %s)", name, i, names);
    for (int i = 0; i < 16; ++i) LG_ARG((reinterpret_cast<uintptr_t>(ptr[i]) & 3u) == 0, "%s: operand %d must be 4-byte aligned", name, i);
    LG_ARG(nxt_pitch >= 1 && prompt_pitch >= P && out_pitch >= G, "%s: row pitches %lld (nxt, >= 1) / %lld (prompts, >= P = %lld) / %lld (out, >= G = %lld)",
           name, (long long)nxt_pitch, (long long)prompt_pitch, (long long)P, (long long)out_pitch, (long long)G);
    {
        // a thread writes its slot's words and its request's words: bytes shared by two operands would make the result depend on
        // which thread ran first
        const int64_t bytes[16] = {((slots - 1) * nxt_pitch + 1) * 4, ((N - 1) * prompt_pitch + P) * 4, N * 4, N * 4, ((N - 1) * out_pitch + G) * 4, N * 4, 8,
                                   slots * 4, slots * 4, slots * 4, slots * m * 4, slots * m * 4, slots * 4, slots * max_blocks * 4, slots * 4,
                                   (num_blocks + 1) * 4};
        for (int i = 0; i < 16; ++i)
            for (int j = i + 1; j < 16; ++j)
                LG_ARG(!paged_serve_overlap(ptr[i], bytes[i], ptr[j], bytes[j]), "%s: operands %d and %d (of %s) overlap", name, i, j, names);
        for (int i = 4; i < 16; ++i) { const int rc = adam_epilogue_check_write(ptr[i], bytes[i]); if (rc != LG_OK) return rc; }
    }
    const PagedServeArgs a{nxt, nxt_pitch, prompts, prompt_len, budget, prompt_pitch, out, out_len, out_pitch, queue, req, pos, count, ids, position_ids, last,
                           block_table, held, free_stack, int(P), int(G), int(N), int(slots), int(m), int(max_blocks), int(num_blocks), int(log2_block),
                           int(prefix_blocks), eos_id, rt().status_dev};
    hipLaunchKernelGGL(serve_commit_paged, dim3(1), dim3(unsigned((slots + 63) / 64 * 64)), 0, rt().stream, a);
    LG_CHECK_LAUNCH();
    return LG_OK;
}
