// Attention of ONE new token against a key / value cache (incremental decoding of the causal LM): lg_attention_decode_f32.
//
// A single query row is a matrix-vector problem bound by the read of K and V, so nothing here is shared with the MFMA prefill
// kernels of attention.hip / attention_long.hip: no matrix cores, no LDS staging of K or V.  One workgroup of 256 threads (4
// waves) per (batch, head) pair.  The position t of the new token is ONE word in device memory that the kernel reads - a
// captured step replays with whatever the word holds then.  lg_attention_decode_rows_f32 is the same kernel with a word per batch
// element (DecodeArgs::pos_pitch = 1 in place of 0): everything below holds per element with its own t.
//
// Partition of the keys 0 .. t.  A key row of D floats is read by G = D / 4 neighbouring lanes, one 16-byte load each, so a
// wave covers KW = 64 / G rows per load instruction (D = 64: 4, D = 32: 8) and the workgroup KP = 4 KW rows per PASS (16 / 32):
//     key j  ->  pass j / KP, wave (j % KP) / KW, lane group (j % KW), lane chunk c = lane % G holds floats [4c, 4c + 4)
// kUnroll = 16 passes (256 / 512 keys) are loaded before the first is used - 16 independent 16-byte loads in flight per lane: the
// launch is bound by the latency of its loads (16 workgroups at batch 8 x 2 heads cannot fill the memory system), so what counts is
// how many dependent round trips a lane makes, not bytes.  For the same reason the first group of V rows is loaded BEFORE the
// scores: it needs nothing from the softmax and is in flight across it; up to 256 keys at D = 64 (every length at D = 32) a lane
// waits for memory once.  Row t itself is never loaded from the cache: its lanes take k_new / v_new, which the same lanes also
// store to row t of the caches - no in-kernel visibility question.  Rows j > t are neither read nor written.
//
//   scores    partial dot of the lane's 4 floats (fixed order), folded over the G lanes of the row by the xor butterfly 1 .. G/2 (row_sum);
//             score * scale + (1 - mask[j]) * -10000 goes to LDS (at most 512 floats)
//   softmax   thread i owns scores i and i + 256: max, exp(x + (-max)), sum - each folded over the wave by xor shuffles and
//             over the 4 waves in wave order through LDS; p = e * (1 / sum) back to LDS (and to `p`, +0.0 beyond t)
//   context   acc += p[j] * V[j] in pass order per lane, folded over the lane groups of the wave by xor shuffles G .. 32, the
//             4 per-wave partial contexts (4 x D floats in LDS) folded in wave order
// Every fold has a fixed order and depends on t, D and the (batch, head) pair's own data only: the same bits from run to run
// and whatever else the launch computes.  Registers: q, k_new, v_new chunks (3 float4), kUnroll float4 of K and kUnroll of V in
// flight, one float4 accumulator.  LDS: 512 + 4 * 64 + 8 floats, static.
// The lane folds (wave_max, wave_sum, row_sum) are decode_lanes.h's, the host checks cache_entry.h's: both shared with decode_split.hip.
#include "cache_entry.h"
#include "decode_lanes.h"
#include <cmath>

namespace lg {

constexpr int kDecodeMaxKeys = 512;
constexpr int kDecodeUnroll = 16;

struct DecodeArgs {
    const float *q, *k_new, *v_new;      // element (b, head, d) at x + b * sb + head * D + d
    int64_t sbq, sbk, sbv;
    float *k_cache, *v_cache;            // element (b, j, head, d) at x + b * sbc + j * ldc + head * D + d
    int64_t ldc, sbc;
    const int32_t* pos;                  // batch element b reads pos[b * pos_pitch]: pitch 0 = one word for the batch, 1 = a word per row
    int64_t pos_pitch;
    float* o;
    int64_t sbo;
    float* p;                            // NULL, or (batch, heads, capacity) dense
    int heads, capacity;
    float scale;
    const float* mask;                   // element (b, j) at mask + b * sbm + j; NULL = none
    int64_t sbm;
    int* status;
};

// rows j0, j0 + KP, ... of a cache (this lane's chunk) for one group of passes: below t from the cache, at t the new token's
template <int KP>
__device__ __forceinline__ void load_group(df32x4 (&r)[kDecodeUnroll], const float* rows, int64_t ld, const df32x4& fresh, int j0, int t) {
#pragma unroll
    for (int u = 0; u < kDecodeUnroll; ++u) {
        const int j = j0 + u * KP;
        r[u] = fresh;
        if (j < t) r[u] = *reinterpret_cast<const df32x4*>(rows + int64_t(j) * ld);
    }
}

template <int D>
__global__ __launch_bounds__(256) void attn_decode(const DecodeArgs a) {
    constexpr int G = D / 4, KW = 64 / G, KP = 4 * KW;
    __shared__ float Sc[kDecodeMaxKeys];     // scores, then probabilities
    __shared__ __attribute__((aligned(16))) float Part[4][64];            // per-wave partial contexts
    __shared__ float Red[8];                 // per-wave maxima [0, 4), sums [4, 8)

    const int tid = threadIdx.x, head = blockIdx.x, b = blockIdx.y;
    const int t = a.pos[int64_t(b) * a.pos_pitch];       // uniform over the workgroup either way: a scalar load
    if (t < 0 || t >= a.capacity) {
        // a bounds check, never a fault: nothing is written for this batch element (the others of a per-row launch are computed
        // as usual), the next synchronising call reports LG_EINDEX
        if (tid == 0) __hip_atomic_fetch_or(a.status, LG_STATUS_BAD_INDEX, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
        return;
    }
    const int wave = tid >> 6, lane = tid & 63, g = lane / G, c = lane % G;
    const int col = head * D + 4 * c;
    const df32x4 q4 = *reinterpret_cast<const df32x4*>(a.q + int64_t(b) * a.sbq + col);
    const df32x4 kn = *reinterpret_cast<const df32x4*>(a.k_new + int64_t(b) * a.sbk + col);
    const df32x4 vn = *reinterpret_cast<const df32x4*>(a.v_new + int64_t(b) * a.sbv + col);
    float* kc = a.k_cache + int64_t(b) * a.sbc + col;
    float* vc = a.v_cache + int64_t(b) * a.sbc + col;
    const float* mrow = a.mask ? a.mask + int64_t(b) * a.sbm : nullptr;
    const int first = wave * KW + g;         // this lane's key of pass 0; pass n: first + n * KP (the loops' bounds are the wave's)

    // row t of the caches: the lanes that own key t hold its chunks already
    if (first % KP == t % KP) {
        *reinterpret_cast<df32x4*>(kc + int64_t(t) * a.ldc) = kn;
        *reinterpret_cast<df32x4*>(vc + int64_t(t) * a.ldc) = vn;
    }

    // the first group of V rows: in flight across the scores and the softmax
    df32x4 v4[kDecodeUnroll];
    load_group<KP>(v4, vc, a.ldc, vn, first, t);

    // ---- scores ------------------------------------------------------------------------------------------------------------
    for (int jw = wave * KW; jw <= t; jw += kDecodeUnroll * KP) {
        const int j0 = jw + g;
        df32x4 k4[kDecodeUnroll];
        load_group<KP>(k4, kc, a.ldc, kn, j0, t);
        // the keys' mask entries ride with the rows (one wait for all of them); 1.0f where there is no mask or no key
        float mk[kDecodeUnroll];
#pragma unroll
        for (int u = 0; u < kDecodeUnroll; ++u) {
            const int j = j0 + u * KP;
            mk[u] = 1.0f;
            if (mrow && j <= t) mk[u] = mrow[j];
        }
#pragma unroll
        for (int u = 0; u < kDecodeUnroll; ++u) {
            const int j = j0 + u * KP;
            const float s = row_sum<G>(((q4[0] * k4[u][0] + q4[1] * k4[u][1]) + q4[2] * k4[u][2]) + q4[3] * k4[u][3]);
            // (1.0 - mask) * -10000.0 in fp32, the composite's own arithmetic; -0.0f for a mask of 1 or none: it changes no bit
            if (c == 0 && j <= t) Sc[j] = s * a.scale + (1.0f - mk[u]) * -10000.0f;
        }
    }
    __syncthreads();

    // ---- softmax over the keys 0 .. t: exp(x + (-max)) * (1 / sum), as the tail kernels of attention.hip ---------------------
    const int i0 = tid, i1 = tid + 256;
    const float x0 = i0 <= t ? Sc[i0] : -INFINITY, x1 = i1 <= t ? Sc[i1] : -INFINITY;
    float m = (x1 > x0 || x1 != x1) ? x1 : x0;
    m = wave_max(m);
    if (lane == 0) Red[wave] = m;
    __syncthreads();
    m = Red[0];
#pragma unroll
    for (int w = 1; w < 4; ++w) { const float o = Red[w]; m = (o > m || o != o) ? o : m; }
    const float e0 = i0 <= t ? expf(x0 + (-m)) : 0.f, e1 = i1 <= t ? expf(x1 + (-m)) : 0.f;
    float s = wave_sum(e0 + e1);
    if (lane == 0) Red[4 + wave] = s;
    __syncthreads();
    s = ((Red[4] + Red[5]) + Red[6]) + Red[7];
    const float inv = 1.0f / s;
    const float p0 = e0 * inv, p1 = e1 * inv;
    if (i0 <= t) Sc[i0] = p0;
    if (i1 <= t) Sc[i1] = p1;
    if (a.p) {
        float* pg = a.p + (int64_t(b) * a.heads + head) * a.capacity;
        if (i0 < a.capacity) pg[i0] = p0;            // e = 0 beyond t: exact +0.0
        if (i1 < a.capacity) pg[i1] = p1;
    }
    __syncthreads();

    // ---- context -------------------------------------------------------------------------------------------------------------
    df32x4 acc = {0.f, 0.f, 0.f, 0.f};
    for (int jw = wave * KW; jw <= t; jw += kDecodeUnroll * KP) {
        const int j0 = jw + g;
        if (jw != wave * KW) load_group<KP>(v4, vc, a.ldc, vn, j0, t);
#pragma unroll
        for (int u = 0; u < kDecodeUnroll; ++u) {
            const int j = j0 + u * KP;
            if (j <= t) {
                const float pj = Sc[j];
#pragma unroll
                for (int e = 0; e < 4; ++e) acc[e] += pj * v4[u][e];
            }
        }
    }
#pragma unroll
    for (int off = G; off < 64; off <<= 1) {
#pragma unroll
        for (int e = 0; e < 4; ++e) acc[e] += __shfl_xor(acc[e], off, 64);
    }
    if (g == 0) *reinterpret_cast<df32x4*>(&Part[wave][4 * c]) = acc;
    __syncthreads();
    if (tid < G) {
        df32x4 r;
#pragma unroll
        for (int e = 0; e < 4; ++e) r[e] = ((Part[0][4 * tid + e] + Part[1][4 * tid + e]) + Part[2][4 * tid + e]) + Part[3][4 * tid + e];
        *reinterpret_cast<df32x4*>(a.o + int64_t(b) * a.sbo + head * D + 4 * tid) = r;
    }
}

}  // namespace lg

using namespace lg;

extern "C" int lg_attention_decode_supported(int64_t capacity, int64_t D) {
    return cache_head_dim(D) && capacity >= 1 && capacity <= kDecodeMaxKeys;
}

// both entries: `pos_pitch` words between the positions of neighbouring batch elements (0: one word for the batch)
static int decode_entry(const char* name, int64_t pos_pitch, const float* q, int64_t sbq, const float* k_new, int64_t sbk, const float* v_new,
                        int64_t sbv, float* k_cache, float* v_cache, int64_t ldc, int64_t sbc, const int32_t* pos, float* o, int64_t sbo,
                        float* p, int64_t batch, int64_t heads, int64_t capacity, int64_t D, float scale, const float* mask, int64_t sbm) {
    int rc = decode_check_operands(name, kDecodeMaxKeys, pos_pitch, q, sbq, k_new, sbk, v_new, sbv, k_cache, v_cache, ldc, sbc, pos, o, sbo, p, batch,
                                   heads, capacity, D, mask, sbm);
    if (rc != LG_OK || batch == 0) return rc;
    rc = cache_check_writes(o, batch, sbo, 1, 0, k_cache, v_cache, 4, batch, sbc, capacity, ldc, heads * D, p, batch * heads * capacity * 4);
    if (rc != LG_OK) return rc;
    const DecodeArgs a{q, k_new, v_new, sbq, sbk, sbv, k_cache, v_cache, ldc, sbc, pos, pos_pitch, o, sbo, p, int(heads), int(capacity), scale,
                       mask, sbm, rt().status_dev};
    const dim3 grid{unsigned(heads), unsigned(batch)};
    if (D == 64) hipLaunchKernelGGL(attn_decode<64>, grid, dim3(256), 0, rt().stream, a);
    else         hipLaunchKernelGGL(attn_decode<32>, grid, dim3(256), 0, rt().stream, a);
    return LG_OK;
}

extern "C" int lg_attention_decode_f32(const float* q, int64_t sbq, const float* k_new, int64_t sbk, const float* v_new, int64_t sbv,
                                       float* k_cache, float* v_cache, int64_t ldc, int64_t sbc, const int32_t* pos, float* o, int64_t sbo,
                                       float* p, int64_t batch, int64_t heads, int64_t capacity, int64_t D, float scale,
                                       const float* mask, int64_t sbm) {
    LG_REQUIRE_INIT();
    const int rc = decode_entry("lg_attention_decode_f32", 0, q, sbq, k_new, sbk, v_new, sbv, k_cache, v_cache, ldc, sbc, pos, o, sbo, p, batch, heads,
                        capacity, D, scale, mask, sbm);
    if (rc != LG_OK || batch == 0) return rc;
    LG_CHECK_LAUNCH();
    return LG_OK;
}

// the same launch with a position per batch element: pos holds `batch` contiguous words, element b uses t = pos[b]
extern "C" int lg_attention_decode_rows_f32(const float* q, int64_t sbq, const float* k_new, int64_t sbk, const float* v_new, int64_t sbv,
                                            float* k_cache, float* v_cache, int64_t ldc, int64_t sbc, const int32_t* pos, float* o, int64_t sbo,
                                            float* p, int64_t batch, int64_t heads, int64_t capacity, int64_t D, float scale,
                                            const float* mask, int64_t sbm) {
    LG_REQUIRE_INIT();
    const int rc = decode_entry("lg_attention_decode_rows_f32", 1, q, sbq, k_new, sbk, v_new, sbv, k_cache, v_cache, ldc, sbc, pos, o, sbo, p, batch,
                        heads, capacity, D, scale, mask, sbm);
    if (rc != LG_OK || batch == 0) return rc;
    LG_CHECK_LAUNCH();
    return LG_OK;
}
