// Beam search between two decode forwards in TWO launches: lg_beam_step_f32 picks the best w of the w * V continuations of every
// group of w beams and commits them, lg_beam_reorder_f32 makes the rows of the key / value cache follow the surviving beams.
// Beams are rows of the batch: group g is rows g * w .. g * w + w - 1, best first, 1 <= w <= 8.  The definitions are the loops
// `CpuTensor.beam_step` and `CpuTensor.kv_reorder` (autograd/cpu/ops.py).
//
// lg_beam_step_f32.  Grid (w, b): one workgroup per beam row.
//   * Every workgroup first reads the w positions and done words of its group and decides, as every other workgroup of the group
//     does from the same words, whether the group is out of bounds (flag, identity, every byte kept) or finished (identity, every
//     byte kept): workgroup 0 of the group writes the identity and nobody takes a ticket.
//   * A live row is read once with 16-byte loads from its first aligned element.  A thread keeps the W largest of its elements
//     (W = 1, 2, 4 or 8 >= w) as 64-bit KEYS - the order-preserving key of the value (sample.hip) above the complement of the
//     index - so that one integer compare is "larger value, or equal value and smaller index", a total order over all bit
//     patterns: degenerate logits select something, they never fault.  w rounds of a workgroup-wide integer max (xor shuffles,
//     then the waves' words in wave order) take the row's top w from the threads' lists; overall winners can only come from there.
//   * m is the value of the row's largest key.  The sum of exponentials is a sum of 64-bit INTEGERS floor(2^40 exp(x - m)), as in
//     sample.hip: exact in any order, so the 16-byte phase of a row (which decides the thread an element goes to) cannot change a
//     bit, and two beams with identical rows and scores get identical constants.  c_i = score_i - m - log(sum) is the beam's one
//     constant, a DOUBLE (one thread per row forms it: an fp32 constant would cost half an ulp of |m| + |score|, more than the
//     scores' bound allows where the logits are larger than the score); a candidate is fp32(x_j + c_i), one rounding: inside a
//     beam the order is the order of x, which is exact.
//   * The row's w keys and c_i are published (handoff.h) and the workgroup takes the group's ticket.  The last arriver ranks the
//     at most w * w candidates (a done beam offers one: itself, at flat index i * V) by integer compares on (key of the fp32
//     candidate, flat index) - a permutation, whatever the values - and commits: a thread owns a column of out_ids across the w
//     rows of the group, reads all w words, then writes them (in place, no scratch buffer, no cross-thread hazard); threads
//     0 .. w - 1 write the slots' words; thread 0 adds the statistics.
// Nothing depends on which workgroup arrives last, nothing is shared between groups but the two words of `stats`, which take
// integer atomic adds.
//
// lg_beam_reorder_f32.  One launch for all cache tensors, whose pointers travel by value in the argument struct (up to 64).  A
// thread owns one (tensor, group, cache position j, 16-byte column chunk): it reads the chunk from all w rows into registers, then
// writes the slots with parent[n] != n - in place and safe for any parent inside the group.  Every workgroup first reads the
// group's w parents and positions and returns before any cache load when the group is the identity or its j >= L = max pos.  A
// parent outside its group writes nothing for that group and raises the status flag: a bounds check, never a fault.
#include "common.h"
#include "handoff.h"
#include <climits>

namespace lg {

typedef unsigned long long u64;

constexpr int kBeamMax = 8;                      // beams per group
constexpr int kBeamMaxTensors = 64;              // cache tensors per reorder launch
constexpr int kBeamMaxWaves = 16;
constexpr float kBeamScale = 1099511627776.0f;   // 2^40: the fixed point of the sum of exponentials (V < 2^22: no overflow)

struct BeamSlot {                                // what a live row hands to the last arriver
    u64 key[kBeamMax];
    u64 c;                                       // the bits of c_i, a double
};

struct BeamArgs {
    const float* logits;                         // row r at logits + r * pitch
    int64_t pitch;
    float* scores;
    int32_t *parent, *token, *out_ids;
    int64_t out_pitch;
    int32_t *pos, *done, *stats;
    int V, w, columns;
    int32_t eos_id;
    BeamSlot* slots;                             // one per row
    int* tickets;                                // one per group, tstride ints apart
    int tstride;
    int* status;
};

// larger value <=> larger key; -0.0 and +0.0 share one key (sample.hip)
__device__ __forceinline__ uint32_t beam_key(float x) {
    uint32_t b = __float_as_uint(x);
    if (b == 0x80000000u) b = 0u;
    return b ^ ((b >> 31) ? 0xFFFFFFFFu : 0x80000000u);
}

__device__ __forceinline__ float beam_value(uint32_t k) {
    return __uint_as_float(k ^ ((k >> 31) ? 0x80000000u : 0xFFFFFFFFu));
}

// element j of value x: larger key <=> larger value, or the same value at a smaller index.  Never 0 (j < 2^31)
__device__ __forceinline__ u64 beam_pack(float x, int j) { return (u64(beam_key(x)) << 32) | u64(0xFFFFFFFFu - uint32_t(j)); }

__device__ __forceinline__ u64 beam_shfl_xor(u64 v, int off) {
    const uint32_t lo = __shfl_xor(uint32_t(v), off, 64), hi = __shfl_xor(uint32_t(v >> 32), off, 64);
    return (u64(hi) << 32) | lo;
}

// the largest / the sum of one word per thread, in every thread: xor shuffles, then the waves' words in wave order
template <bool SUM>
__device__ __forceinline__ u64 beam_block_fold(u64 v, u64* s_wave) {
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) {
        const u64 o = beam_shfl_xor(v, off);
        v = SUM ? v + o : (o > v ? o : v);
    }
    __syncthreads();                             // whoever still reads s_wave from the fold before is through
    if ((threadIdx.x & 63) == 0) s_wave[threadIdx.x >> 6] = v;
    __syncthreads();
    u64 r = s_wave[0];
    for (int k = 1; k < int(blockDim.x >> 6); ++k) r = SUM ? r + s_wave[k] : (s_wave[k] > r ? s_wave[k] : r);
    return r;
}

// f(j, x) over this thread's share of the row g[0 .. V): 16-byte loads from the first aligned element, scalars in front and behind
template <class F>
__device__ __forceinline__ void beam_each(const float* __restrict__ g, int V, F f) {
    const int tid = threadIdx.x, T = blockDim.x;
    int head = int((4 - ((reinterpret_cast<uintptr_t>(g) >> 2) & 3)) & 3);
    if (head > V) head = V;
    if (tid < head) f(tid, g[tid]);
    const int nv = (V - head) >> 2;
    const float4* const g4 = reinterpret_cast<const float4*>(g + head);
    int v = tid;
    for (; v + T < nv; v += 2 * T) {             // two loads in flight per thread
        const float4 a = g4[v], b = g4[v + T];
        const int ja = head + 4 * v, jb = head + 4 * (v + T);
        f(ja, a.x); f(ja + 1, a.y); f(ja + 2, a.z); f(ja + 3, a.w);
        f(jb, b.x); f(jb + 1, b.y); f(jb + 2, b.z); f(jb + 3, b.w);
    }
    for (; v < nv; v += T) {
        const float4 a = g4[v];
        const int ja = head + 4 * v;
        f(ja, a.x); f(ja + 1, a.y); f(ja + 2, a.z); f(ja + 3, a.w);
    }
    const int t0 = head + 4 * nv;
    if (t0 + tid < V) f(t0 + tid, g[t0 + tid]);
}

template <int W>
__global__ __launch_bounds__(1024) void beam_step(const BeamArgs a) {
    __shared__ u64 s_wave[kBeamMaxWaves];
    __shared__ int s_last;
    __shared__ int s_pos[kBeamMax], s_done[kBeamMax], s_token[kBeamMax];
    __shared__ float s_score[kBeamMax];
    __shared__ uint32_t s_ckey[kBeamMax * kBeamMax], s_flat[kBeamMax * kBeamMax];      // the candidates: key of the value, flat index
    __shared__ int s_sel[kBeamMax];                                                  // the candidate output slot n takes
    const int tid = threadIdx.x, w = a.w, V = a.V, beam = blockIdx.x, lo = blockIdx.y * w;

    // the group's words, the same in every workgroup of the group: nothing of them is written before all w have arrived
    bool bad = false, all_done = true;
    int longest = 0;
#pragma unroll
    for (int i = 0; i < W; ++i) {
        if (i < w) {
            const int p = a.pos[lo + i], d = a.done[lo + i];
            bad = bad || p < 0 || (d == 0 && int64_t(p) + 1 >= a.columns);
            all_done = all_done && d != 0;
            longest = p > longest ? p : longest;
        }
    }
    if (bad || all_done) {
        if (beam == 0 && tid < w) a.parent[lo + tid] = lo + tid;
        if (bad && beam == 0 && tid == 0) __hip_atomic_fetch_or(a.status, LG_STATUS_BAD_INDEX, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
        return;
    }

    const int row = lo + beam;
    if (a.done[row] == 0) {
        const float* const g = a.logits + int64_t(row) * a.pitch;
        // the thread's W largest keys, descending, in registers (every index below is a constant after unrolling)
        u64 top[W];
#pragma unroll
        for (int k = 0; k < W; ++k) top[k] = 0;
        beam_each(g, V, [&](int j, float x) {
            const u64 key = beam_pack(x, j);
            if (key > top[W - 1]) {
                top[W - 1] = key;
#pragma unroll
                for (int k = W - 1; k > 0; --k) {
                    const u64 hi = top[k - 1], lw = top[k];
                    const bool swap = lw > hi;
                    top[k - 1] = swap ? lw : hi;
                    top[k] = swap ? hi : lw;
                }
            }
        });
        // the row's top w: w rounds of the workgroup's largest head; the one thread that holds it moves its list up
        u64 best[W];
#pragma unroll
        for (int n = 0; n < W; ++n) {
            best[n] = 0;
            if (n < w) {
                best[n] = beam_block_fold<false>(top[0], s_wave);
                if (top[0] == best[n]) {
#pragma unroll
                    for (int k = 0; k + 1 < W; ++k) top[k] = top[k + 1];
                    top[W - 1] = 0;
                }
            }
        }
        const float m = beam_value(uint32_t(best[0] >> 32));
        u64 mine = 0;
        beam_each(g, V, [&](int, float x) { mine += u64(__fmul_rn(expf(__fsub_rn(x, m)), kBeamScale)); });
        const u64 total = beam_block_fold<true>(mine, s_wave);
        if (tid == 0) {
            const double c = double(a.scores[row]) - double(m) - log(double(total) * 0x1p-40);
            BeamSlot s;
#pragma unroll
            for (int n = 0; n < kBeamMax; ++n) s.key[n] = n < W ? best[n] : 0;
            s.c = u64(__double_as_longlong(c));
            handoff::publish<u64>(a.slots + row, s);
        }
    }
    if (!handoff::arrive_thread0(a.tickets + int64_t(blockIdx.y) * a.tstride, w, &s_last)) return;

    // ---- the last arriver of the group: rank the candidates, commit --------------------------------------------------------------
    if (tid < w) {
        s_pos[tid] = a.pos[lo + tid];
        s_done[tid] = a.done[lo + tid];
        s_token[tid] = a.token[lo + tid];
        s_score[tid] = a.scores[lo + tid];
        s_sel[tid] = tid * W;                                                         // (every slot is ranked below: never read as it stands)
    }
    if (tid < W * W) {
        const int i = tid / W, k = tid % W;
        uint32_t ckey = 0, flat = 0xFFFFFFFFu;                                    // no candidate: behind every real one
        if (i < w && k < w) {
            if (a.done[lo + i] != 0) {
                if (k == 0) { ckey = beam_key(a.scores[lo + i]); flat = uint32_t(i) * uint32_t(V); }
            } else {
                const u64 key = handoff::fetch<u64>(&a.slots[lo + i].key[k]);
                const double c = __longlong_as_double((long long)handoff::fetch<u64>(&a.slots[lo + i].c));
                uint32_t j = 0xFFFFFFFFu - uint32_t(key);
                if (j >= uint32_t(V)) j = 0;                                      // (a key is an element of the row: never taken)
                ckey = beam_key(float(double(beam_value(uint32_t(key >> 32))) + c));
                flat = uint32_t(i) * uint32_t(V) + j;
            }
        }
        s_ckey[tid] = ckey;
        s_flat[tid] = flat;
    }
    __syncthreads();
    if (tid < W * W && s_flat[tid] != 0xFFFFFFFFu) {
        // (key, flat) is unique per candidate: the ranks are a permutation, and at least w candidates exist
        const uint32_t ck = s_ckey[tid], fl = s_flat[tid];
        int rank = 0;
        for (int o = 0; o < W * W; ++o) {
            const uint32_t ok = s_ckey[o], of = s_flat[o];
            rank += (of != 0xFFFFFFFFu && (ok > ck || (ok == ck && of < fl))) ? 1 : 0;
        }
        if (rank < w) s_sel[rank] = tid;
    }
    __syncthreads();

    // out_ids: a thread owns column `col` of the w rows - reads them all, then writes the slots
    int src[W], tok[W], keep[W];                                                  // per slot: its beam, its new token (-1: a copy), the columns it copies
#pragma unroll
    for (int n = 0; n < W; ++n) {
        src[n] = 0; tok[n] = -1; keep[n] = -1;
        if (n < w) {
            const int c = s_sel[n];
            src[n] = c / W;
            keep[n] = s_pos[src[n]];
            if (s_done[src[n]] == 0) tok[n] = int(s_flat[c] - uint32_t(src[n]) * uint32_t(V));
        }
    }
    const int cols = longest + 2 < a.columns ? longest + 2 : a.columns;
    for (int col = tid; col < cols; col += blockDim.x) {
        int32_t old[W];
#pragma unroll
        for (int i = 0; i < W; ++i) old[i] = i < w ? a.out_ids[int64_t(lo + i) * a.out_pitch + col] : 0;
#pragma unroll
        for (int n = 0; n < W; ++n) {
            if (n < w) {
                int32_t v = old[0];
#pragma unroll
                for (int i = 1; i < W; ++i) v = src[n] == i ? old[i] : v;
                if (col <= keep[n]) {
                    if (src[n] != n) a.out_ids[int64_t(lo + n) * a.out_pitch + col] = v;
                } else if (col == keep[n] + 1 && tok[n] >= 0) {
                    a.out_ids[int64_t(lo + n) * a.out_pitch + col] = tok[n];
                }
            }
        }
    }
    if (tid < w) {
        const int c = s_sel[tid], i = c / W;
        const bool copy = s_done[i] != 0;
        const int j = copy ? s_token[i] : int(s_flat[c] - uint32_t(i) * uint32_t(V));
        const int now_done = copy || (a.eos_id >= 0 && j == a.eos_id) ? 1 : 0;
        a.parent[lo + tid] = lo + i;
        a.scores[lo + tid] = copy ? s_score[i] : beam_value(s_ckey[c]);
        a.token[lo + tid] = j;
        a.pos[lo + tid] = copy ? s_pos[i] : s_pos[i] + 1;
        a.done[lo + tid] = now_done;
        // the statistics: every slot's words over the wave (w <= 8 lanes of wave 0)
        const u64 done_mask = __ballot(now_done != 0), moved_mask = __ballot(i != tid);
        if (tid == 0) {
            if (int(__popcll(done_mask)) == w) atomicAdd(a.stats + 0, 1);
            const int moved = int(__popcll(moved_mask));
            if (moved) atomicAdd(a.stats + 1, moved);
        }
    }
}

// ---- the cache follows the beams ---------------------------------------------------------------------------------------------------
struct ReorderArgs {
    float* tensor[kBeamMaxTensors];              // element (r, j, c) at tensor[t] + r * sbc + j * ldc + c
    int64_t ldc, sbc;
    const int32_t *parent, *pos;
    int w, capacity, chunks;                     // chunks: 16-byte pieces of a cache row (width / 4)
    int* status;
};

template <int W>
__global__ __launch_bounds__(256) void beam_reorder(const ReorderArgs a) {
    const int w = a.w, lo = blockIdx.y * w;
    // the group's words first: identity, out of bounds or beyond the group's longest row - return before any cache load
    int src[W];
    int longest = 0;
    bool identity = true, bad = false;
#pragma unroll
    for (int n = 0; n < W; ++n) {
        src[n] = n;
        if (n < w) {
            const int p = a.parent[lo + n] - lo, q = a.pos[lo + n];
            bad = bad || p < 0 || p >= w;
            identity = identity && p == n;
            longest = q > longest ? q : longest;
            src[n] = p;
        }
    }
    if (bad) {
        if (blockIdx.x == 0 && blockIdx.z == 0 && threadIdx.x == 0)
            __hip_atomic_fetch_or(a.status, LG_STATUS_BAD_INDEX, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
        return;
    }
    if (longest > a.capacity) longest = a.capacity;
    const int64_t first = int64_t(blockIdx.x) * 256, work = int64_t(longest) * a.chunks;
    if (identity || first >= work) return;
    const int64_t item = first + threadIdx.x;
    if (item >= work) return;
    const int64_t j = item / a.chunks, c = item % a.chunks;
    float* const base = a.tensor[blockIdx.z] + int64_t(lo) * a.sbc + j * a.ldc + c * 4;
    float4 old[W];                               // (a row beyond w reads row 0 again: every element is set, nothing is indexed at run time)
#pragma unroll
    for (int i = 0; i < W; ++i) old[i] = *reinterpret_cast<const float4*>(base + int64_t(i < w ? i : 0) * a.sbc);
#pragma unroll
    for (int n = 0; n < W; ++n) {
        if (n < w && src[n] != n) {
            float4 v = old[0];
#pragma unroll
            for (int i = 1; i < W; ++i) {
                const bool s = src[n] == i;
                v.x = s ? old[i].x : v.x; v.y = s ? old[i].y : v.y; v.z = s ? old[i].z : v.z; v.w = s ? old[i].w : v.w;
            }
            *reinterpret_cast<float4*>(base + int64_t(n) * a.sbc) = v;
        }
    }
}

template <int W>
static void launch_beam_step(const BeamArgs& a, int64_t groups, int threads) {
    hipLaunchKernelGGL(beam_step<W>, dim3(unsigned(a.w), unsigned(groups)), dim3(threads), 0, rt().stream, a);
}

template <int W>
static void launch_beam_reorder(const ReorderArgs& a, int64_t blocks, int64_t groups, int64_t tensors) {
    hipLaunchKernelGGL(beam_reorder<W>, dim3(unsigned(blocks), unsigned(groups), unsigned(tensors)), dim3(256), 0, rt().stream, a);
}

}  // namespace lg

using namespace lg;

extern "C" int lg_beam_step_f32(const float* logits, int64_t logits_pitch, float* scores, int32_t* parent, int32_t* token, int32_t* out_ids,
                                int64_t out_pitch, int64_t columns, int32_t* pos, int32_t* done, int32_t* stats, int64_t rows, int64_t vocab,
                                int64_t num_beams, int32_t eos_id) {
    LG_REQUIRE_INIT();
    const char* name = "lg_beam_step_f32";
    const int64_t w = num_beams;
    LG_ARG(w >= 1 && w <= kBeamMax, "%s: num_beams = %lld outside 1 .. %d", name, (long long)w, kBeamMax);
    LG_ARG(rows >= 0 && rows < (int64_t(1) << 24) && rows % w == 0 && rows / w < 65536,
           "%s: rows = %lld (0 .. 2^24 - 1, a multiple of num_beams = %lld, fewer than 65536 groups) unsupported", name, (long long)rows, (long long)w);
    LG_ARG(vocab >= w && vocab < (int64_t(1) << 22) && rows * vocab < (int64_t(1) << 32) && columns >= 1 && columns < (int64_t(1) << 31),
           "%s: vocab = %lld (num_beams = %lld .. 2^22 - 1, rows * vocab < 2^32), columns = %lld (1 .. 2^31 - 1) unsupported", name, (long long)vocab,
           (long long)w, (long long)columns);
    if (rows == 0) return LG_OK;
    const void* ptr[8] = {logits, scores, parent, token, out_ids, pos, done, stats};
    for (int i = 0; i < 8; ++i) LG_ARG(ptr[i], "%s: NULL operand %d (of logits, scores, parent, token, out_ids, pos, done, stats)", name, i);
    for (int i = 0; i < 8; ++i) LG_ARG((reinterpret_cast<uintptr_t>(ptr[i]) & 3u) == 0, "%s: operand %d must be 4-byte aligned", name, i);
    LG_ARG(logits_pitch >= vocab && out_pitch >= columns && (rows - 1) * out_pitch + columns < (int64_t(1) << 60) &&
               (rows - 1) * logits_pitch + vocab < (int64_t(1) << 60),
           "%s: row pitches %lld (logits, >= vocab = %lld) / %lld (out_ids, >= columns = %lld)", name, (long long)logits_pitch, (long long)vocab,
           (long long)out_pitch, (long long)columns);
    const int64_t groups = rows / w;
    LG_ARG(groups <= rt().n_tickets, "%s: the ticket pool holds %d counters, %lld groups need one each", name, rt().n_tickets, (long long)groups);
    {
        // the last arriver of a group writes the group's words: bytes shared by two operands would make the result depend on who it was
        const int64_t bytes[8] = {((rows - 1) * logits_pitch + vocab) * 4, rows * 4, rows * 4, rows * 4, ((rows - 1) * out_pitch + columns) * 4,
                                  rows * 4, rows * 4, 8};
        for (int i = 0; i < 8; ++i)
            for (int j = i + 1; j < 8; ++j)
                LG_ARG(!bytes_overlap(ptr[i], bytes[i], ptr[j], bytes[j]),
                       "%s: operands %d and %d (of logits, scores, parent, token, out_ids, pos, done, stats) overlap", name, i, j);
        for (int i = 1; i < 8; ++i) {
            const int rc = adam_epilogue_check_write(ptr[i], bytes[i]);
            if (rc != LG_OK) return rc;
        }
    }
    BeamSlot* slots = nullptr;
    { const int rc = lg_malloc(reinterpret_cast<void**>(&slots), size_t(rows) * sizeof(BeamSlot)); if (rc != LG_OK) return rc; }
    const BeamArgs a{logits, logits_pitch, scores, parent, token, out_ids, out_pitch, pos, done, stats, int(vocab), int(w), int(columns), eos_id,
                     slots, rt().tickets, ticket_stride(groups), rt().status_dev};
    const int threads = vocab <= 8192 ? 256 : 1024;
    if (w == 1) launch_beam_step<1>(a, groups, threads);
    else if (w == 2) launch_beam_step<2>(a, groups, threads);
    else if (w <= 4) launch_beam_step<4>(a, groups, threads);
    else launch_beam_step<8>(a, groups, threads);
    const int rc = lg_free(slots);                       // stream-ordered: the block is only reused by later launches
    if (rc != LG_OK) return rc;
    LG_CHECK_LAUNCH();
    return LG_OK;
}

extern "C" int lg_beam_reorder_f32(float* const* tensors, int64_t n_tensors, int64_t ldc, int64_t sbc, int64_t capacity, int64_t width,
                                   const int32_t* parent, const int32_t* pos, int64_t rows, int64_t num_beams) {
    LG_REQUIRE_INIT();
    const char* name = "lg_beam_reorder_f32";
    const int64_t w = num_beams;
    LG_ARG(w >= 1 && w <= kBeamMax, "%s: num_beams = %lld outside 1 .. %d", name, (long long)w, kBeamMax);
    LG_ARG(n_tensors >= 0 && n_tensors <= kBeamMaxTensors, "%s: %lld cache tensors in one launch (0 .. %d) unsupported", name, (long long)n_tensors,
           kBeamMaxTensors);
    LG_ARG(rows >= 0 && rows % w == 0 && rows / w < 65536 && capacity >= 1 && capacity < (int64_t(1) << 24) && width >= 4 && width % 4 == 0 &&
               width < (int64_t(1) << 24),
           "%s: rows = %lld (a multiple of num_beams = %lld, fewer than 65536 groups), capacity = %lld (1 .. 2^24 - 1), width = %lld (a multiple of 4 "
           "below 2^24) unsupported", name, (long long)rows, (long long)w, (long long)capacity, (long long)width);
    if (rows == 0 || n_tensors == 0) return LG_OK;
    LG_ARG(tensors && parent && pos, "%s: NULL operand", name);
    LG_ARG(((reinterpret_cast<uintptr_t>(parent) | reinterpret_cast<uintptr_t>(pos)) & 3u) == 0, "%s: parent and pos must be 4-byte aligned", name);
    LG_ARG(ldc >= width && ldc % 4 == 0 && sbc % 4 == 0 && sbc >= (capacity - 1) * ldc + width && (rows - 1) * sbc < (int64_t(1) << 58),
           "%s: pitches %lld (a cache row, >= width = %lld) / %lld (a sequence, >= (capacity - 1) * ldc + width), multiples of 4", name, (long long)ldc,
           (long long)width, (long long)sbc);
    const int64_t span = ((rows - 1) * sbc + (capacity - 1) * ldc + width) * 4;
    LG_ARG(!bytes_overlap(parent, rows * 4, pos, rows * 4), "%s: parent and pos overlap", name);
    for (int64_t t = 0; t < n_tensors; ++t) {
        LG_ARG(tensors[t] && aligned16(tensors[t]), "%s: cache tensor %lld is NULL or not 16-byte aligned", name, (long long)t);
        // a thread reads and writes its chunk of one tensor only: a tensor that shares bytes with another, or with the words every
        // workgroup reads first, would make the result depend on the order of the workgroups
        LG_ARG(!bytes_overlap(parent, rows * 4, tensors[t], span) && !bytes_overlap(pos, rows * 4, tensors[t], span),
               "%s: parent / pos overlap cache tensor %lld", name, (long long)t);
        for (int64_t u = t + 1; u < n_tensors; ++u)
            LG_ARG(!bytes_overlap(tensors[t], span, tensors[u], span), "%s: cache tensors %lld and %lld overlap", name, (long long)t, (long long)u);
        const int rc = adam_epilogue_check_write(tensors[t], span);
        if (rc != LG_OK) return rc;
    }
    ReorderArgs a;
    for (int t = 0; t < kBeamMaxTensors; ++t) a.tensor[t] = t < n_tensors ? tensors[t] : nullptr;
    a.ldc = ldc; a.sbc = sbc; a.parent = parent; a.pos = pos; a.w = int(w); a.capacity = int(capacity); a.chunks = int(width / 4);
    a.status = rt().status_dev;
    const int64_t blocks = (capacity * (width / 4) + 255) / 256;
    LG_ARG(blocks < (int64_t(1) << 31), "%s: capacity * width = %lld too large for one launch", name, (long long)(capacity * width));
    if (w == 1) launch_beam_reorder<1>(a, blocks, rows / w, n_tensors);
    else if (w == 2) launch_beam_reorder<2>(a, blocks, rows / w, n_tensors);
    else if (w <= 4) launch_beam_reorder<4>(a, blocks, rows / w, n_tensors);
    else launch_beam_reorder<8>(a, blocks, rows / w, n_tensors);
    LG_CHECK_LAUNCH();
    return LG_OK;
}
