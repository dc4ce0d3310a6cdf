// Attention of ONE new token against a key / value cache of up to 16384 rows, the keys SPLIT over workgroups and the partial
// softmaxes merged inside the same launch: lg_attention_decode_split_f32 / lg_attention_decode_split_rows_f32.
//
// lg_attention_decode_f32 (decode.hip) runs one workgroup per (batch, head) pair and stops at 512 keys: a pair's workgroup walks
// its keys in groups of dependent loads, and 16 workgroups cannot fill the memory system.  Here the grid is
// (ceil(capacity / L), heads, batch) with L = kSplitSlice = 256 keys: workgroup s of a pair owns keys [sL, sL + L).  It reads
// the position t of the new token from device memory (one word, or a word per batch element for `_rows`), returns before any
// load when sL > t, and knows without communication that live = t / L + 1 workgroups of its pair work.
//
// Inside a slice the lanes are partitioned as in decode.hip: a key row of D floats is read by G = D / 4 neighbouring lanes, one
// 16-byte load each; a wave covers KW = 64 / G rows per load instruction, the workgroup KP = 4 KW rows per pass (D = 64: 16,
// D = 32: 32), and a slice is U = L / KP passes (16 / 8):
//     key sL + i  ->  pass i / KP, wave (i % KP) / KW, lane group i % KW, lane chunk c = lane % G holds floats [4c, 4c + 4)
// All U rows of K, all U rows of V and the U mask words of a lane are issued before the first of them is used: a lane waits for
// memory ONCE, whatever t is.  Row t is never loaded: the lanes that own it in the slice t / L take k_new / v_new from registers
// and store them to the caches; no other slice touches row t; rows beyond t are neither read nor written.
//
// Per slice: scores (fixed-order partial dot, DPP row sum over the G lanes) * scale + (1 - mask) * -10000 to LDS; thread i owns
// key sL + i: m_s = max, e = exp(x + (-m_s)), l_s = sum of e - each folded over the wave by xor shuffles and over the 4 waves in
// wave order through LDS; a_s = sum of e[j] V[j], UNNORMALISED, per lane in pass order, over the lane groups by xor shuffles
// G .. 32, over the waves in wave order.
//
// live == 1: the slice divides by l_s and stores o and lse = m_s + log(l_s) itself; no workspace, no ticket.
// live > 1 (handoff.h): the slice publishes {a_s[D], m_s, l_s} into its workspace slot (b, head, s) and arrives at the pair's
// ticket with expected = live.  The last arriver fetches every live slot - all its fetches are issued together: thread (col,
// grp) takes column col of the PER slices grp * PER .. (D = 64: 4 groups of 16 slices, D = 32: 8 groups of 8), lane s of wave
// 0 takes m_s and l_s - and folds
//     M = max m_s,  w_s = exp(m_s + (-M)),  Lsum = sum w_s l_s,  o = (sum w_s a_s) * (1 / Lsum),  lse = M + log(Lsum)
// with fixed trees: Lsum by the xor butterfly over the lanes (slices) of wave 0, a column's sum in ascending slice order inside a
// group and the groups in ascending order.  Nothing depends on which workgroup arrived last; the ticket is zero again afterwards.
// A slice whose keys are all masked has m_s near -10000 and w_s = +0: it adds exact zeros.  m_s is the maximum over at least one
// key with a finite score, so m_s + (-M) is never -inf - -inf for finite operands.
//
// Registers: q, k_new, v_new chunks, U float4 of K and U of V in flight, U mask words, one float4 accumulator.  LDS: 256 + 256 +
// 8 floats and the hand-off word, static.
// The lane folds (wave_max, wave_sum, row_sum) are decode_lanes.h's, the host checks cache_entry.h's: both shared with decode.hip;
// the ticket pool's bound and the workspace around the launch are this file's own.
#include "cache_entry.h"
#include "decode_lanes.h"
#include "handoff.h"
#include <cmath>

namespace lg {

constexpr int kSplitSlice = 256;                 // L: keys per workgroup, one load group for both head sizes
constexpr int kSplitMaxKeys = 16384;             // the range of lg_attention_stream_supported
constexpr int kSplitMaxSlices = kSplitMaxKeys / kSplitSlice;      // 64: one lane of a wave per slice in the merge

struct SplitArgs {
    const float *q, *k_new, *v_new;      // element (b, head, d) at x + b * sb + head * D + d
    int64_t sbq, sbk, sbv;
    float *k_cache, *v_cache;            // element (b, j, head, d) at x + b * sbc + j * ldc + head * D + d
    int64_t ldc, sbc;
    const int32_t* pos;                  // batch element b reads pos[b * pos_pitch]: pitch 0 = one word for the batch, 1 = a word per row
    int64_t pos_pitch;
    float* o;
    int64_t sbo;
    float* lse;                          // NULL, or (batch, heads) dense
    int heads, capacity, slices;
    float scale;
    const float* mask;                   // element (b, j) at mask + b * sbm + j; NULL = none
    int64_t sbm;
    float* ws;                           // slot (b, head, s): D + 2 floats {a[D], m, l}; NULL when slices == 1
    int* tickets;                        // one per (b, head) pair, tstride ints apart
    int tstride;
    int* status;
};

template <int D>
__global__ __launch_bounds__(256) void attn_decode_split(const SplitArgs a) {
    constexpr int L = kSplitSlice, G = D / 4, KW = 64 / G, KP = 4 * KW, U = L / KP;
    constexpr int SW = D + 2;                // floats of a workspace slot
    constexpr int GR = 256 / D, PER = kSplitMaxSlices / GR;      // the merge: GR groups of PER slices per column
    __shared__ float Sc[L];                  // scores, then exponentials; in the merge: w_s
    __shared__ __attribute__((aligned(16))) float Part[256];     // per-wave partial contexts [4][64]; in the merge: per-group [GR][D]
    __shared__ float Red[8];                 // per-wave maxima [0, 4), sums [4, 8); in the merge: M, Lsum
    __shared__ int s_last;

    const int tid = threadIdx.x, slice = blockIdx.x, head = blockIdx.y, b = blockIdx.z;
    const int t = a.pos[int64_t(b) * a.pos_pitch];       // uniform over the workgroup either way: a scalar load
    if (t < 0 || t >= a.capacity) {
        // a bounds check, never a fault: nothing is written for this batch element, the others are computed as usual
        if (slice == 0 && tid == 0) __hip_atomic_fetch_or(a.status, LG_STATUS_BAD_INDEX, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
        return;
    }
    const int j_lo = slice * L;
    if (j_lo > t) return;                    // no key of this slice is visible: before any load, without a ticket
    const int live = t / L + 1;

    const int wave = tid >> 6, lane = tid & 63, g = lane / G, c = lane % G;
    const int col = head * D + 4 * c;
    const df32x4 q4 = *reinterpret_cast<const df32x4*>(a.q + int64_t(b) * a.sbq + col);
    const df32x4 kn = *reinterpret_cast<const df32x4*>(a.k_new + int64_t(b) * a.sbk + col);
    const df32x4 vn = *reinterpret_cast<const df32x4*>(a.v_new + int64_t(b) * a.sbv + col);
    float* kc = a.k_cache + int64_t(b) * a.sbc + col;
    float* vc = a.v_cache + int64_t(b) * a.sbc + col;
    const float* mrow = a.mask ? a.mask + int64_t(b) * a.sbm : nullptr;
    const int first = wave * KW + g;         // this lane's key of pass 0 inside the slice; pass u: first + u * KP

    // row t of the caches, in the slice that holds it (L is a multiple of KP): the lanes that own key t hold its chunks already
    if (slice == live - 1 && first % KP == t % KP) {
        *reinterpret_cast<df32x4*>(kc + int64_t(t) * a.ldc) = kn;
        *reinterpret_cast<df32x4*>(vc + int64_t(t) * a.ldc) = vn;
    }

    // ---- the slice's K rows, mask words and V rows: everything in flight before the first use ------------------------------------
    df32x4 k4[U], v4[U];
    float mk[U];
#pragma unroll
    for (int u = 0; u < U; ++u) {
        const int j = j_lo + first + u * KP;
        k4[u] = kn;
        if (j < t) k4[u] = *reinterpret_cast<const df32x4*>(kc + int64_t(j) * a.ldc);
    }
#pragma unroll
    for (int u = 0; u < U; ++u) {
        const int j = j_lo + first + u * KP;
        mk[u] = 1.0f;                        // where there is no mask or no key
        if (mrow && j <= t) mk[u] = mrow[j];
    }
#pragma unroll
    for (int u = 0; u < U; ++u) {
        const int j = j_lo + first + u * KP;
        v4[u] = vn;
        if (j < t) v4[u] = *reinterpret_cast<const df32x4*>(vc + int64_t(j) * a.ldc);
    }

    // ---- scores ------------------------------------------------------------------------------------------------------------------
#pragma unroll
    for (int u = 0; u < U; ++u) {
        const int i = first + u * KP;
        const float s = row_sum<G>(((q4[0] * k4[u][0] + q4[1] * k4[u][1]) + q4[2] * k4[u][2]) + q4[3] * k4[u][3]);
        // (1.0 - mask) * -10000.0 in fp32, the composite's own arithmetic; -0.0f for a mask of 1 or none: it changes no bit
        if (c == 0 && j_lo + i <= t) Sc[i] = s * a.scale + (1.0f - mk[u]) * -10000.0f;
    }
    __syncthreads();

    // ---- the slice's softmax pieces: thread i owns key j_lo + i ------------------------------------------------------------------
    const bool mine = j_lo + tid <= t;
    const float x = mine ? Sc[tid] : -INFINITY;
    float m = wave_max(x);
    if (lane == 0) Red[wave] = m;
    __syncthreads();
    m = Red[0];
#pragma unroll
    for (int w = 1; w < 4; ++w) { const float o = Red[w]; m = (o > m || o != o) ? o : m; }
    const float e = mine ? expf(x + (-m)) : 0.f;
    Sc[tid] = e;                             // (the thread's own word: nobody else reads it before the barrier)
    float l = wave_sum(e);
    if (lane == 0) Red[4 + wave] = l;
    __syncthreads();
    l = ((Red[4] + Red[5]) + Red[6]) + Red[7];

    // ---- the unnormalised context of the slice -----------------------------------------------------------------------------------
    df32x4 acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int u = 0; u < U; ++u) {
        const int i = first + u * KP;
        if (j_lo + i <= t) {
            const float ej = Sc[i];
#pragma unroll
            for (int k = 0; k < 4; ++k) acc[k] += ej * v4[u][k];
        }
    }
#pragma unroll
    for (int off = G; off < 64; off <<= 1) {
#pragma unroll
        for (int k = 0; k < 4; ++k) acc[k] += __shfl_xor(acc[k], off, 64);
    }
    if (g == 0) *reinterpret_cast<df32x4*>(&Part[wave * 64 + 4 * c]) = acc;
    __syncthreads();
    float mine_a = 0.f;                      // thread d < D: column d of a_s, the waves in wave order
    if (tid < D) mine_a = ((Part[tid] + Part[64 + tid]) + Part[128 + tid]) + Part[192 + tid];
    float* const og = a.o + int64_t(b) * a.sbo + head * D;
    float* const lse_out = a.lse ? a.lse + int64_t(b) * a.heads + head : nullptr;

    if (live == 1) {
        if (tid < D) og[tid] = mine_a * (1.0f / l);
        if (tid == 0 && lse_out) *lse_out = m + logf(l);
        return;
    }

    // ---- the hand-off: publish, arrive, the last arriver merges ------------------------------------------------------------------
    float* const slots = a.ws + (int64_t(b) * a.heads + head) * a.slices * SW;
    {
        float* const slot = slots + int64_t(slice) * SW;
        if (tid < D) handoff::publish<float>(slot + tid, mine_a);
        else if (tid == D) handoff::publish<float>(slot + D, m);
        else if (tid == D + 1) handoff::publish<float>(slot + D + 1, l);
    }
    int* const ticket = a.tickets + (int64_t(b) * a.heads + head) * a.tstride;
    if (!handoff::arrive_workgroup(ticket, live, &s_last)) return;

    // every fetch of the merge is issued here, before anything waits for one: column mcol of the slices grp * PER ..
    const int mcol = tid % D, grp = tid / D;
    float av[PER];
#pragma unroll
    for (int u = 0; u < PER; ++u) {
        const int s = grp * PER + u;
        av[u] = 0.f;
        if (s < live) av[u] = handoff::fetch<float>(slots + int64_t(s) * SW + mcol);
    }
    if (wave == 0) {
        float ms = -INFINITY, ls = 0.f;
        if (lane < live) { ms = handoff::fetch<float>(slots + int64_t(lane) * SW + D); ls = handoff::fetch<float>(slots + int64_t(lane) * SW + D + 1); }
        const float M = wave_max(ms);
        const float w = lane < live ? expf(ms + (-M)) : 0.f;     // a fully masked slice next to a visible one: +0
        Sc[lane] = w;
        const float Lsum = wave_sum(w * ls);
        if (lane == 0) { Red[0] = M; Red[1] = Lsum; }
    }
    __syncthreads();
    float part = 0.f;
#pragma unroll
    for (int u = 0; u < PER; ++u) {
        const int s = grp * PER + u;
        if (s < live) part += Sc[s] * av[u];
    }
    Part[grp * D + mcol] = part;
    __syncthreads();
    if (tid < D) {
        float r = Part[tid];
#pragma unroll
        for (int k = 1; k < GR; ++k) r += Part[k * D + tid];
        og[tid] = r * (1.0f / Red[1]);
    }
    if (tid == 0 && lse_out) *lse_out = Red[0] + logf(Red[1]);
}

}  // namespace lg

using namespace lg;

extern "C" int lg_attention_decode_split_supported(int64_t capacity, int64_t D) {
    return cache_head_dim(D) && capacity >= 1 && capacity <= kSplitMaxKeys;
}

extern "C" int lg_attention_decode_split_slice(void) { return kSplitSlice; }

// both entries: `pos_pitch` words between the positions of neighbouring batch elements (0: one word for the batch)
static int split_entry(const char* name, int64_t pos_pitch, const float* q, int64_t sbq, const float* k_new, int64_t sbk, const float* v_new,
                       int64_t sbv, float* k_cache, float* v_cache, int64_t ldc, int64_t sbc, const int32_t* pos, float* o, int64_t sbo,
                       float* lse, int64_t batch, int64_t heads, int64_t capacity, int64_t D, float scale, const float* mask, int64_t sbm) {
    int rc = decode_check_operands(name, kSplitMaxKeys, pos_pitch, q, sbq, k_new, sbk, v_new, sbv, k_cache, v_cache, ldc, sbc, pos, o, sbo, lse, batch,
                                   heads, capacity, D, mask, sbm);
    if (rc != LG_OK || batch == 0) return rc;
    const int64_t pairs = batch * heads, slices = (capacity + kSplitSlice - 1) / kSplitSlice;
    LG_ARG(pairs <= rt().n_tickets, "%s: the ticket pool holds %d counters, %lld (batch, head) pairs need one each", name, rt().n_tickets,
           (long long)pairs);
    rc = cache_check_writes(o, batch, sbo, 1, 0, k_cache, v_cache, 4, batch, sbc, capacity, ldc, heads * D, lse, pairs * 4);
    if (rc != LG_OK) return rc;
    float* ws = nullptr;                             // a cache of one slice never hands anything over
    if (slices > 1) {
        rc = lg_malloc(reinterpret_cast<void**>(&ws), size_t(pairs * slices * (D + 2)) * sizeof(float));
        if (rc != LG_OK) return rc;
    }
    const SplitArgs a{q, k_new, v_new, sbq, sbk, sbv, k_cache, v_cache, ldc, sbc, pos, pos_pitch, o, sbo, lse, int(heads), int(capacity), int(slices),
                      scale, mask, sbm, ws, rt().tickets, ticket_stride(pairs), rt().status_dev};
    const dim3 grid{unsigned(slices), unsigned(heads), unsigned(batch)};
    if (D == 64) hipLaunchKernelGGL(attn_decode_split<64>, grid, dim3(256), 0, rt().stream, a);
    else         hipLaunchKernelGGL(attn_decode_split<32>, grid, dim3(256), 0, rt().stream, a);
    if (ws) { rc = lg_free(ws); if (rc != LG_OK) return rc; }      // stream-ordered: the block is only reused by later launches
    return LG_OK;
}

extern "C" int lg_attention_decode_split_f32(const float* q, int64_t sbq, const float* k_new, int64_t sbk, const float* v_new, int64_t sbv,
                                             float* k_cache, float* v_cache, int64_t ldc, int64_t sbc, const int32_t* pos, float* o, int64_t sbo,
                                             float* lse, int64_t batch, int64_t heads, int64_t capacity, int64_t D, float scale,
                                             const float* mask, int64_t sbm) {
    LG_REQUIRE_INIT();
    const int rc = split_entry("lg_attention_decode_split_f32", 0, q, sbq, k_new, sbk, v_new, sbv, k_cache, v_cache, ldc, sbc, pos, o, sbo, lse, batch,
                               heads, capacity, D, scale, mask, sbm);
    if (rc != LG_OK || batch == 0) return rc;
    LG_CHECK_LAUNCH();
    return LG_OK;
}

// the same launch with a position per batch element: pos holds `batch` contiguous words, element b uses t = pos[b]
extern "C" int lg_attention_decode_split_rows_f32(const float* q, int64_t sbq, const float* k_new, int64_t sbk, const float* v_new, int64_t sbv,
                                                  float* k_cache, float* v_cache, int64_t ldc, int64_t sbc, const int32_t* pos, float* o,
                                                  int64_t sbo, float* lse, int64_t batch, int64_t heads, int64_t capacity, int64_t D, float scale,
                                                  const float* mask, int64_t sbm) {
    LG_REQUIRE_INIT();
    const int rc = split_entry("lg_attention_decode_split_rows_f32", 1, q, sbq, k_new, sbk, v_new, sbv, k_cache, v_cache, ldc, sbc, pos, o, sbo, lse,
                               batch, heads, capacity, D, scale, mask, sbm);
    if (rc != LG_OK || batch == 0) return rc;
    LG_CHECK_LAUNCH();
    return LG_OK;
}
