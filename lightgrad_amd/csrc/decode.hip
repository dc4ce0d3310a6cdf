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
#include "common.h"
#include <cmath>

namespace lg {

typedef float df32x4 __attribute__((ext_vector_type(4)));

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

__device__ __forceinline__ float wave_max(float m) {
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) { const float o = __shfl_xor(m, off, 64); m = (o > m || o != o) ? o : m; }
    return m;
}

__device__ __forceinline__ float wave_sum(float s) {
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) s += __shfl_xor(s, off, 64);
    return s;
}

// the sum over the G = 8 or 16 neighbouring lanes of a key row, in every one of them: the xor butterfly 1, 2, 4 (, 8) as data-parallel
// moves inside a row of 16 lanes - after the two quad steps the lanes of a quad agree, so mirroring 8 (then 16) lanes brings each
// the other quad's (then the other half's) sum.  Same pairs, same order, same bits as __shfl_xor, without its trips through LDS:
// with one key per lane group and pass, these folds - not the loads - were what a lane waited for
template <int CTRL>
__device__ __forceinline__ float lane_move(float x) {
    return __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, x), CTRL, 0xf, 0xf, false));
}

template <int G>
__device__ __forceinline__ float row_sum(float s) {
    s += lane_move<0xB1>(s);                 // quad_perm [1, 0, 3, 2]: lane ^ 1
    s += lane_move<0x4E>(s);                 // quad_perm [2, 3, 0, 1]: lane ^ 2
    s += lane_move<0x141>(s);                // row_half_mirror: the other quad of 8 lanes
    if constexpr (G == 16) s += lane_move<0x140>(s);      // row_mirror: the other half of 16 lanes
    return s;
}

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

static bool decode_operand(const void* p, int64_t sb) { return p && aligned16(p) && sb % 4 == 0; }

// do the `words` position words share an address with the floats [c, c + (batch - 1) sbc + (capacity - 1) ldc + w) of a cache?
static bool positions_overlap(const int32_t* pos, int64_t words, const float* c, int64_t ldc, int64_t sbc, int64_t capacity, int64_t batch, int64_t w) {
    const char *x = reinterpret_cast<const char*>(pos), *xe = x + 4 * words;
    const char *y = reinterpret_cast<const char*>(c), *ye = reinterpret_cast<const char*>(c + (batch - 1) * sbc + (capacity - 1) * ldc + w);
    return x < ye && y < xe;
}

}  // namespace lg

using namespace lg;

extern "C" int lg_attention_decode_supported(int64_t capacity, int64_t D) {
    return (D == 32 || D == 64) && capacity >= 1 && capacity <= kDecodeMaxKeys;
}

// both entries: `pos_pitch` words between the positions of neighbouring batch elements (0: one word for the batch)
static int decode_entry(const char* name, int64_t pos_pitch, const float* q, int64_t sbq, const float* k_new, int64_t sbk, const float* v_new,
                        int64_t sbv, float* k_cache, float* v_cache, int64_t ldc, int64_t sbc, const int32_t* pos, float* o, int64_t sbo,
                        float* p, int64_t batch, int64_t heads, int64_t capacity, int64_t D, float scale, const float* mask, int64_t sbm) {
    LG_ARG(lg_attention_decode_supported(capacity, D), "%s: capacity = %lld (1 .. 512), D = %lld (32 or 64) unsupported", name,
           (long long)capacity, (long long)D);
    LG_ARG(batch >= 0 && heads >= 1 && batch <= 65535 && heads <= 65535, "%s: bad batch / heads", name);
    if (batch == 0) return LG_OK;
    LG_ARG(decode_operand(q, sbq) && decode_operand(k_new, sbk) && decode_operand(v_new, sbv) && decode_operand(k_cache, sbc) &&
               decode_operand(v_cache, sbc) && decode_operand(o, sbo) && ldc % 4 == 0 && pos && (reinterpret_cast<uintptr_t>(pos) & 3u) == 0 &&
               (reinterpret_cast<uintptr_t>(p) & 3u) == 0,
           "%s: operands must be non-NULL and 16-byte aligned with pitches that are multiples of 4", name);
    const int64_t w = heads * D;
    LG_ARG(ldc >= w, "%s: cache row pitch %lld below heads * D = %lld", name, (long long)ldc, (long long)w);
    LG_ARG(!mask || sbm == 0 || sbm >= capacity, "%s: mask batch pitch %lld is neither 0 (one row for the batch) nor >= capacity", name,
           (long long)sbm);
    LG_ARG(!positions_overlap(pos, pos_pitch ? batch : 1, k_cache, ldc, sbc, capacity, batch, w) &&
               !positions_overlap(pos, pos_pitch ? batch : 1, v_cache, ldc, sbc, capacity, batch, w),
           "%s: pos overlaps a cache: the launch writes the caches while other workgroups read their positions", name);
    {
        const int64_t row[2] = {batch, w}, row_strides[2] = {sbo, 1};
        int rc = adam_epilogue_check_strided(o, 4, 2, row, row_strides);
        if (rc != LG_OK) return rc;
        const int64_t rows[3] = {batch, capacity, w}, strides[3] = {sbc, ldc, 1};
        rc = adam_epilogue_check_strided(k_cache, 4, 3, rows, strides);
        if (rc != LG_OK) return rc;
        rc = adam_epilogue_check_strided(v_cache, 4, 3, rows, strides);
        if (rc != LG_OK) return rc;
        if (p) { rc = adam_epilogue_check_write(p, batch * heads * capacity * 4); if (rc != LG_OK) return rc; }
    }
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
