// Grouped-query attention of ONE new token against a key / value cache of up to 16384 rows whose K / V heads are SHARED by
// R = heads / kv_heads query heads each: lg_attention_decode_gqa_f32 / lg_attention_decode_gqa_rows_f32.
//
// The launch of decode_split.hip carried to R query heads per workgroup.  There a workgroup holds its slice of L = 256 K rows and
// 256 V rows in registers before the first use and spends them on one query head.  Here the grid is (ceil(capacity / L),
// kv_heads, batch): workgroup s of a (batch, K/V head) pair owns keys [sL, sL + L) of that K/V head, loads them ONCE - the same
// lane layout, G = D / 4 lanes per key row with a 16-byte load each, U passes, every K row, mask word and V row of a lane issued
// before the first of them is used - and serves the R query heads kvh * R .. kvh * R + R - 1 from those registers: 1 / R of the
// split launch's bytes, workgroups and cache rows.  Row t is written to the caches once per K/V head, from registers, by the
// lanes that own it; rows beyond t are neither read nor written; a slice beyond t returns before any load.
//
// The heads are a compile-time loop (template <int D, int R>) over the K / V registers:
//   - the R query chunks of a lane are loaded up front, with k_new / v_new;
//   - per head the scores are decode_split.hip's fixed-order partial dot and DPP row sum, written to Sc[r][256] in LDS;
//   - max, exp and sum of all R heads pass through the SAME three barriers the split kernel has: thread i owns key sL + i of every
//     head, the wave folds run a butterfly step of all R heads at a time, and the per-wave pieces cross the waves through Red,
//     [R][4] maxima and [R][4] sums;
//   - R float4 accumulators take the unnormalised contexts from the one set of V registers, in pass order; they are folded over
//     the lane groups by xor shuffles G .. 32 and over the waves in wave order through Part[R][256].
// Per (batch, head) every operation and every fold is the one attn_decode_split performs, in its order: o and lse are bit for
// bit what the split launch computes on caches whose K / V heads were repeated R times, and R = 1 IS the split launch.
//
// No matrix cores: with at most R = 8 query rows in fp32 an MFMA tile would run at most a quarter full, and the design spends its
// registers on ONE wait for memory per lane.  Measured (profiles/decode_gqa.md): a further head costs a workgroup about 2.3 us of
// dependent work behind that wait, so on a grid below one workgroup per CU the R = 8 launch is slower than the split launch on
// repeated heads (25.0 against 9.0 us at 1024 keys, batch 8) and faster only where the bytes decide (38.9 against 98.1 us at 16384).
//
// Hand-off (handoff.h): live = t / L + 1 workgroups of a (batch, K/V head) pair work.  live == 1: the slice divides by l and
// stores o and lse of its R heads itself; no workspace, no ticket.  live > 1: the slice publishes R workspace slots {a[D], m, l},
// slot (b, head, s) as in the split launch, and arrives at the ONE ticket of its (batch, K/V head) pair with expected = live.  The
// last arriver merges the R heads with the split kernel's fixed trees - thread (col, grp) takes column col of the PER slices grp *
// PER .. of every head, R * PER fetches all issued before the first wait (the K / V registers are dead by then); lane s of wave
// r % 4 takes m_s and l_s of head r - and leaves the ticket zero.
//
// Registers at D = 64, R = 8: 64 + 64 of K / V in flight, 16 mask words, 32 of q, 32 of accumulators, 8 of k_new / v_new; no
// scratch in any instantiation (profiles/decode_gqa.md).  LDS: Sc and Part R KiB each, Red 32 R bytes, the hand-off word; static.
// The lane folds are decode_lanes.h's, the host checks cache_entry.h's with a cache width of kv_heads * D.
#include "cache_entry.h"
#include "decode_lanes.h"
#include "handoff.h"
#include <cmath>

namespace lg {

constexpr int kGqaSlice = 256;                   // L: keys per workgroup, as in decode_split.hip
constexpr int kGqaMaxKeys = 16384;
constexpr int kGqaMaxSlices = kGqaMaxKeys / kGqaSlice;            // 64: one lane of a wave per slice in the merge

struct GqaArgs {
    const float *q, *k_new, *v_new;      // q: element (b, head, d) at q + b * sbq + head * D + d; k_new / v_new: (b, kvh, d) likewise
    int64_t sbq, sbk, sbv;
    float *k_cache, *v_cache;            // element (b, j, kvh, d) at x + b * sbc + j * ldc + kvh * D + d
    int64_t ldc, sbc;
    const int32_t* pos;                  // batch element b reads pos[b * pos_pitch]
    int64_t pos_pitch;
    float* o;                            // (b, heads * D)
    int64_t sbo;
    float* lse;                          // NULL, or (batch, heads) dense
    int heads, capacity, slices;
    float scale;
    const float* mask;                   // element (b, j) at mask + b * sbm + j; NULL = none; shared by all heads
    int64_t sbm;
    float* ws;                           // slot (b, head, s): D + 2 floats {a[D], m, l}; NULL when slices == 1
    int* tickets;                        // one per (b, kvh) pair, tstride ints apart
    int tstride;
    int* status;
};

// wave_max / wave_sum of decode_lanes.h for the R heads at once: the same pairs in the same order per head - the same bits -, with
// the R exchanges of a butterfly step in flight together instead of R dependent chains of six one after the other
template <int R>
__device__ __forceinline__ void wave_max_heads(float (&m)[R]) {
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
        float o[R];
#pragma unroll
        for (int r = 0; r < R; ++r) o[r] = __shfl_xor(m[r], off, 64);
#pragma unroll
        for (int r = 0; r < R; ++r) m[r] = (o[r] > m[r] || o[r] != o[r]) ? o[r] : m[r];
    }
}

template <int R>
__device__ __forceinline__ void wave_sum_heads(float (&s)[R]) {
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
        float o[R];
#pragma unroll
        for (int r = 0; r < R; ++r) o[r] = __shfl_xor(s[r], off, 64);
#pragma unroll
        for (int r = 0; r < R; ++r) s[r] += o[r];
    }
}

template <int D, int R>
__global__ __launch_bounds__(256) void attn_decode_gqa(const GqaArgs a) {
    constexpr int L = kGqaSlice, G = D / 4, KW = 64 / G, KP = 4 * KW, U = L / KP;
    constexpr int SW = D + 2;                // floats of a workspace slot
    constexpr int GR = 256 / D, PER = kGqaMaxSlices / GR;        // the merge: GR groups of PER slices per column
    constexpr int NA = (R * D + 255) / 256;  // context columns (head, d) a thread finishes: column tid + 256 n
    __shared__ float Sc[R][L];               // scores, then exponentials; in the merge: w_s of head r in Sc[r][s]
    __shared__ __attribute__((aligned(16))) float Part[R][256];   // per-wave partial contexts [4][64]; in the merge: per-group [GR][D]
    __shared__ float Red[8 * R];             // per-wave maxima [r][4], then sums [R + r][4]; in the merge: {M, Lsum} of head r at 2 r
    __shared__ int s_last;

    const int tid = threadIdx.x, slice = blockIdx.x, kvh = blockIdx.y, b = blockIdx.z;
    const int t = a.pos[int64_t(b) * a.pos_pitch];       // uniform over the workgroup: a scalar load
    if (t < 0 || t >= a.capacity) {
        // a bounds check, never a fault: nothing is written for this batch element, the others are computed as usual
        if (slice == 0 && kvh == 0 && tid == 0) __hip_atomic_fetch_or(a.status, LG_STATUS_BAD_INDEX, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
        return;
    }
    const int j_lo = slice * L;
    if (j_lo > t) return;                    // no key of this slice is visible: before any load, without a ticket
    const int live = t / L + 1;

    const int wave = tid >> 6, lane = tid & 63, g = lane / G, c = lane % G;
    const int col = kvh * D + 4 * c, head0 = kvh * R;
    df32x4 q4[R];
#pragma unroll
    for (int r = 0; r < R; ++r) q4[r] = *reinterpret_cast<const df32x4*>(a.q + int64_t(b) * a.sbq + (head0 + r) * D + 4 * c);
    const df32x4 kn = *reinterpret_cast<const df32x4*>(a.k_new + int64_t(b) * a.sbk + col);
    const df32x4 vn = *reinterpret_cast<const df32x4*>(a.v_new + int64_t(b) * a.sbv + col);
    float* kc = a.k_cache + int64_t(b) * a.sbc + col;
    float* vc = a.v_cache + int64_t(b) * a.sbc + col;
    const float* mrow = a.mask ? a.mask + int64_t(b) * a.sbm : nullptr;
    const int first = wave * KW + g;         // this lane's key of pass 0 inside the slice; pass u: first + u * KP

    // row t of the caches, once per K/V head, in the slice that holds it: the lanes that own key t hold its chunks already
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

    // ---- scores of the R heads from the one set of K registers -------------------------------------------------------------------
#pragma unroll
    for (int u = 0; u < U; ++u) {
        const int i = first + u * KP;
        const float bias = (1.0f - mk[u]) * -10000.0f;           // the composite's own arithmetic; -0.0f for a mask of 1 or none
#pragma unroll
        for (int r = 0; r < R; ++r) {
            const float s = row_sum<G>(((q4[r][0] * k4[u][0] + q4[r][1] * k4[u][1]) + q4[r][2] * k4[u][2]) + q4[r][3] * k4[u][3]);
            if (c == 0 && j_lo + i <= t) Sc[r][i] = s * a.scale + bias;
        }
    }
    __syncthreads();

    // ---- the slice's softmax pieces: thread i owns key j_lo + i of every head; three barriers for all R heads ------------------------
    const bool mine = j_lo + tid <= t;
    float x[R], m[R], l[R];
#pragma unroll
    for (int r = 0; r < R; ++r) m[r] = x[r] = mine ? Sc[r][tid] : -INFINITY;
    wave_max_heads<R>(m);
    if (lane == 0) {
#pragma unroll
        for (int r = 0; r < R; ++r) Red[4 * r + wave] = m[r];
    }
    __syncthreads();
#pragma unroll
    for (int r = 0; r < R; ++r) {
        m[r] = Red[4 * r];
#pragma unroll
        for (int w = 1; w < 4; ++w) { const float o = Red[4 * r + w]; m[r] = (o > m[r] || o != o) ? o : m[r]; }
        l[r] = mine ? expf(x[r] + (-m[r])) : 0.f;
        Sc[r][tid] = l[r];                   // (the thread's own word: nobody else reads it before the barrier)
    }
    wave_sum_heads<R>(l);
    if (lane == 0) {
#pragma unroll
        for (int r = 0; r < R; ++r) Red[4 * (R + r) + wave] = l[r];
    }
    __syncthreads();

    // ---- the R unnormalised contexts of the slice from the one set of V registers ------------------------------------------------
    df32x4 acc[R];
#pragma unroll
    for (int r = 0; r < R; ++r) acc[r] = df32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int u = 0; u < U; ++u) {
        const int i = first + u * KP;
        if (j_lo + i <= t) {
#pragma unroll
            for (int r = 0; r < R; ++r) {
                const float ej = Sc[r][i];
#pragma unroll
                for (int k = 0; k < 4; ++k) acc[r][k] += ej * v4[u][k];
            }
        }
    }
#pragma unroll
    for (int off = G; off < 64; off <<= 1) {                     // the split kernel's fold per head, the R heads' exchanges of a step together
        df32x4 o[R];
#pragma unroll
        for (int r = 0; r < R; ++r) {
#pragma unroll
            for (int k = 0; k < 4; ++k) o[r][k] = __shfl_xor(acc[r][k], off, 64);
        }
#pragma unroll
        for (int r = 0; r < R; ++r) acc[r] += o[r];
    }
    if (g == 0) {
#pragma unroll
        for (int r = 0; r < R; ++r) *reinterpret_cast<df32x4*>(&Part[r][wave * 64 + 4 * c]) = acc[r];
    }
    __syncthreads();

    // thread tid finishes the columns idx = tid + 256 n < R * D: head idx / D, element idx % D - the waves in wave order; m and l of
    // that head come back from Red (a head index that depends on the thread never indexes a register array)
    float mine_a[NA], m_a[NA], l_a[NA];
#pragma unroll
    for (int n = 0; n < NA; ++n) {
        const int idx = tid + 256 * n, r = idx / D, d = idx % D;
        mine_a[n] = m_a[n] = l_a[n] = 0.f;
        if (idx < R * D) {
            mine_a[n] = ((Part[r][d] + Part[r][64 + d]) + Part[r][128 + d]) + Part[r][192 + d];
            float mm = Red[4 * r];
#pragma unroll
            for (int w = 1; w < 4; ++w) { const float o = Red[4 * r + w]; mm = (o > mm || o != o) ? o : mm; }
            m_a[n] = mm;
            l_a[n] = ((Red[4 * (R + r)] + Red[4 * (R + r) + 1]) + Red[4 * (R + r) + 2]) + Red[4 * (R + r) + 3];
        }
    }
    float* const og = a.o + int64_t(b) * a.sbo + head0 * D;      // the R heads of a K/V head are neighbours: column idx of them
    float* const lse_out = a.lse ? a.lse + int64_t(b) * a.heads + head0 : nullptr;

    if (live == 1) {
#pragma unroll
        for (int n = 0; n < NA; ++n) {
            const int idx = tid + 256 * n;
            if (idx < R * D) {
                og[idx] = mine_a[n] * (1.0f / l_a[n]);
                if (idx % D == 0 && lse_out) lse_out[idx / D] = m_a[n] + logf(l_a[n]);
            }
        }
        return;
    }

    // ---- the hand-off: publish R slots, arrive at the pair's one ticket, the last arriver merges the R heads ----------------------
    float* const slots = a.ws + (int64_t(b) * a.heads + head0) * a.slices * SW;          // head r: + r * slices * SW
#pragma unroll
    for (int n = 0; n < NA; ++n) {
        const int idx = tid + 256 * n, r = idx / D, d = idx % D;
        if (idx < R * D) {
            float* const slot = slots + (int64_t(r) * a.slices + slice) * SW;
            handoff::publish<float>(slot + d, mine_a[n]);
            if (d == 0) { handoff::publish<float>(slot + D, m_a[n]); handoff::publish<float>(slot + D + 1, l_a[n]); }
        }
    }
    int* const ticket = a.tickets + (int64_t(b) * gridDim.y + kvh) * a.tstride;
    if (!handoff::arrive_workgroup(ticket, live, &s_last)) return;

    // every fetch of the merge is issued here, before anything waits for one: column mcol of the slices grp * PER .. of every head
    const int mcol = tid % D, grp = tid / D;
    float av[R][PER];
#pragma unroll
    for (int r = 0; r < R; ++r) {
#pragma unroll
        for (int u = 0; u < PER; ++u) {
            const int s = grp * PER + u;
            av[r][u] = 0.f;
            if (s < live) av[r][u] = handoff::fetch<float>(slots + (int64_t(r) * a.slices + s) * SW + mcol);
        }
    }
#pragma unroll
    for (int r = 0; r < R; ++r) {
        if (wave == r % 4) {                 // (wave-uniform; any wave folds the same butterfly to the same bits)
            const float* const sl = slots + (int64_t(r) * a.slices + lane) * SW;
            float ms = -INFINITY, ls = 0.f;
            if (lane < live) { ms = handoff::fetch<float>(sl + D); ls = handoff::fetch<float>(sl + D + 1); }
            const float M = wave_max(ms);
            const float w = lane < live ? expf(ms + (-M)) : 0.f;     // a fully masked slice next to a visible one: +0
            Sc[r][lane] = w;
            const float Lsum = wave_sum(w * ls);
            if (lane == 0) { Red[2 * r] = M; Red[2 * r + 1] = Lsum; }
        }
    }
    __syncthreads();
#pragma unroll
    for (int r = 0; r < R; ++r) {
        float part = 0.f;
#pragma unroll
        for (int u = 0; u < PER; ++u) {
            const int s = grp * PER + u;
            if (s < live) part += Sc[r][s] * av[r][u];
        }
        Part[r][grp * D + mcol] = part;
    }
    __syncthreads();
#pragma unroll
    for (int n = 0; n < NA; ++n) {
        const int idx = tid + 256 * n, r = idx / D, d = idx % D;
        if (idx < R * D) {
            float s = Part[r][d];
#pragma unroll
            for (int k = 1; k < GR; ++k) s += Part[r][k * D + d];
            og[idx] = s * (1.0f / Red[2 * r + 1]);
            if (d == 0 && lse_out) lse_out[r] = Red[2 * r] + logf(Red[2 * r + 1]);
        }
    }
}

inline bool gqa_group(int64_t heads, int64_t kv_heads) {
    if (heads < 1 || kv_heads < 1 || heads % kv_heads) return false;
    const int64_t r = heads / kv_heads;
    return r == 1 || r == 2 || r == 4 || r == 8;
}

template <int D>
static void gqa_launch(int R, dim3 grid, const GqaArgs& a) {
    switch (R) {
        case 1: hipLaunchKernelGGL((attn_decode_gqa<D, 1>), grid, dim3(256), 0, rt().stream, a); break;
        case 2: hipLaunchKernelGGL((attn_decode_gqa<D, 2>), grid, dim3(256), 0, rt().stream, a); break;
        case 4: hipLaunchKernelGGL((attn_decode_gqa<D, 4>), grid, dim3(256), 0, rt().stream, a); break;
        default: hipLaunchKernelGGL((attn_decode_gqa<D, 8>), grid, dim3(256), 0, rt().stream, a); break;
    }
}

}  // namespace lg

using namespace lg;

extern "C" int lg_attention_decode_gqa_supported(int64_t capacity, int64_t D, int64_t heads, int64_t kv_heads) {
    return cache_head_dim(D) && capacity >= 1 && capacity <= kGqaMaxKeys && gqa_group(heads, kv_heads);
}

// both entries: `pos_pitch` words between the positions of neighbouring batch elements (0: one word for the batch)
static int gqa_entry(const char* name, int64_t pos_pitch, const float* q, int64_t sbq, const float* k_new, int64_t sbk, const float* v_new, int64_t sbv,
                     float* k_cache, float* v_cache, int64_t ldc, int64_t sbc, const int32_t* pos, float* o, int64_t sbo, float* lse, int64_t batch,
                     int64_t heads, int64_t kv_heads, int64_t capacity, int64_t D, float scale, const float* mask, int64_t sbm) {
    LG_ARG(gqa_group(heads, kv_heads) && heads <= 65535, "%s: heads = %lld over kv_heads = %lld (a group of 1, 2, 4 or 8 query heads per K/V head) unsupported",
           name, (long long)heads, (long long)kv_heads);
    // the caches, k_new and v_new are kv_heads * D wide: the shared checks see that width
    int rc = decode_check_operands(name, kGqaMaxKeys, pos_pitch, q, sbq, k_new, sbk, v_new, sbv, k_cache, v_cache, ldc, sbc, pos, o, sbo, lse, batch,
                                   kv_heads, capacity, D, mask, sbm);
    if (rc != LG_OK || batch == 0) return rc;
    const int64_t pairs = batch * kv_heads, slices = (capacity + kGqaSlice - 1) / kGqaSlice;
    LG_ARG(pairs <= rt().n_tickets, "%s: the ticket pool holds %d counters, %lld (batch, K/V head) pairs need one each", name, rt().n_tickets,
           (long long)pairs);
    rc = cache_check_writes(o, batch, sbo, 1, 0, k_cache, v_cache, 4, batch, sbc, capacity, ldc, kv_heads * D, lse, batch * heads * 4);
    if (rc != LG_OK) return rc;
    {
        const int64_t oshape[2] = {batch, heads * D}, ostrides[2] = {sbo, 1};            // o is heads * D wide
        rc = adam_epilogue_check_strided(o, 4, 2, oshape, ostrides);
        if (rc != LG_OK) return rc;
    }
    float* ws = nullptr;                             // a cache of one slice never hands anything over
    if (slices > 1) {
        rc = lg_malloc(reinterpret_cast<void**>(&ws), size_t(batch * heads * slices * (D + 2)) * sizeof(float));
        if (rc != LG_OK) return rc;
    }
    const GqaArgs a{q, k_new, v_new, sbq, sbk, sbv, k_cache, v_cache, ldc, sbc, pos, pos_pitch, o, sbo, lse, int(heads), int(capacity), int(slices),
                    scale, mask, sbm, ws, rt().tickets, ticket_stride(pairs), rt().status_dev};
    const dim3 grid{unsigned(slices), unsigned(kv_heads), unsigned(batch)};
    if (D == 64) gqa_launch<64>(int(heads / kv_heads), grid, a);
    else         gqa_launch<32>(int(heads / kv_heads), grid, a);
    if (ws) { rc = lg_free(ws); if (rc != LG_OK) return rc; }      // stream-ordered: the block is only reused by later launches
    return LG_OK;
}

extern "C" int lg_attention_decode_gqa_f32(const float* q, int64_t sbq, const float* k_new, int64_t sbk, const float* v_new, int64_t sbv,
                                           float* k_cache, float* v_cache, int64_t ldc, int64_t sbc, const int32_t* pos, float* o, int64_t sbo,
                                           float* lse, int64_t batch, int64_t heads, int64_t kv_heads, int64_t capacity, int64_t D, float scale,
                                           const float* mask, int64_t sbm) {
    LG_REQUIRE_INIT();
    const int rc = gqa_entry("lg_attention_decode_gqa_f32", 0, q, sbq, k_new, sbk, v_new, sbv, k_cache, v_cache, ldc, sbc, pos, o, sbo, lse, batch,
                             heads, kv_heads, capacity, D, scale, mask, sbm);
    if (rc != LG_OK || batch == 0) return rc;
    LG_CHECK_LAUNCH();
    return LG_OK;
}

// the same launch with a position per batch element: pos holds `batch` contiguous words, element b uses t = pos[b]
extern "C" int lg_attention_decode_gqa_rows_f32(const float* q, int64_t sbq, const float* k_new, int64_t sbk, const float* v_new, int64_t sbv,
                                                float* k_cache, float* v_cache, int64_t ldc, int64_t sbc, const int32_t* pos, float* o,
                                                int64_t sbo, float* lse, int64_t batch, int64_t heads, int64_t kv_heads, int64_t capacity, int64_t D,
                                                float scale, const float* mask, int64_t sbm) {
    LG_REQUIRE_INIT();
    const int rc = gqa_entry("lg_attention_decode_gqa_rows_f32", 1, q, sbq, k_new, sbk, v_new, sbv, k_cache, v_cache, ldc, sbc, pos, o, sbo, lse,
                             batch, heads, kv_heads, capacity, D, scale, mask, sbm);
    if (rc != LG_OK || batch == 0) return rc;
    LG_CHECK_LAUNCH();
    return LG_OK;
}
