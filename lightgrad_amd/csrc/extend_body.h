// The kernel body of the extend launches, attn_extend_body<D, PACKED, PAGED, KV16>, and the host checks their entries share: included
// by extend.hip (the (b, m) entries and the token-packed one, PAGED = false), by paged.hip (lg_attention_extend_paged_f32) and by
// paged_bf16.hip (lg_attention_extend_paged_bf16_f32, KV16 = true: pools of bfloat16 words)
#pragma once
#include <type_traits>
#include "attention_common.h"

namespace lg {

constexpr int kExtChunk = 128;         // rows of a streamed operand in LDS at a time
constexpr int kExtMaxBlocks = 16;      // 32-column blocks of the longest row (512 / 32)
constexpr int kExtMaxKeys = 512;

struct ExtendArgs {
    const float *q, *k_new, *v_new;      // element (b, i, head, d) at x + b * sbX + i * ldX + head * D + d
    int64_t ldq, sbq, ldk, sbk, ldv, sbv;
    float *k_cache, *v_cache;            // element (b, j, head, d) at x + b * sbc + j * ldc + head * D + d
    int64_t ldc, sbc;
    const int32_t* pos;                  // batch element b reads pos[b * pos_pitch]: pitch 0 = one word for the batch, 1 = a word per row
    int64_t pos_pitch;
    const int32_t* count;                // NULL: each of the m rows is a new token; else batch element b has count[b] real ones (0 .. m)
    float* o;                            // context, addressed like q
    int64_t ldo, sbo;
    float* p;                            // NULL, or (batch, heads, m, capacity) dense
    int heads, capacity, m;
    float scale;
    const float* mask;                   // element (b, j) at mask + b * sbm + j; NULL = none
    int64_t sbm;
    int* status;
    const int32_t* cu;                   // NULL for the three (b, m) entries; lg_attention_extend_packed_f32: slots + 1 words, slot z owns rows cu[z] .. cu[z + 1] - 1
    int tokens;                          // ... of the `tokens` rows of the flat (tokens, .) operands: no batch pitch, p is (heads, tokens, capacity)
    // lg_attention_extend_paged_f32 (NULL / 0 for every other entry): the caches are POOLS of num_blocks blocks of 1 << log2_block rows
    // (row r at x + r * ldc, no batch pitch); position j of batch element b is row block_table[b * max_blocks + (j >> log2_block)]
    // * (1 << log2_block) + (j & ((1 << log2_block) - 1)), and capacity = max_blocks << log2_block
    const int32_t* block_table;
    int max_blocks, num_blocks, log2_block;
};

constexpr int kPagedMaxTable = 128;    // words of a slot's block table: 512 positions in blocks of 4 at the least

template <int D>
constexpr int attn_extend_lds_floats(int Cp) { return 32 * (D + 4) + 32 * (Cp + 4) + kExtChunk * (D + 8) + 3 * 1024 + Cp; }
// the paged kernels keep the slot's block table behind it
template <int D>
constexpr int attn_paged_lds_floats(int Cp) { return attn_extend_lds_floats<D>(Cp) + kPagedMaxTable; }

// keys [c0, c0 + 128) of the stream: global -> registers.  Key j < t is the cache's row j, key j >= t row j - t of the new
// tokens (clamped to a row that exists: what a key >= t + m loads is dropped by seam_store); no branch, all loads in flight
template <int D, int N>
__device__ __forceinline__ void seam_load(af32x4 (&v)[N], const float* cache, int64_t ldc, const float* fresh, int64_t ldn, int c0, int t, int m) {
    constexpr int Q = D / 4;
#pragma unroll
    for (int i = 0; i < N; ++i) {
        const int f = threadIdx.x + i * 256, j = c0 + f / Q;
        const int jn = j - t < 0 ? 0 : (j - t < m ? j - t : m - 1);
        const float* src = j < t ? cache + int64_t(j) * ldc : fresh + int64_t(jn) * ldn;
        v[i] = *reinterpret_cast<const af32x4*>(src + (f % Q) * 4);
    }
}
// the same with the cache a pool: key j < t is pool row tab[j >> lb] << lb | (j & mask) with `tab` the slot's table in LDS - every
// word of it checked, the words behind the slot's reach 0 -, so a key j >= t looks up a word that is in range and never becomes an
// address: the new-token buffer is selected as above.  One LDS read in front of each global load, no memory round trip
template <int D, int N>
__device__ __forceinline__ void seam_load_paged(af32x4 (&v)[N], const float* pool, int64_t ldc, const int* tab, int lb, const float* fresh, int64_t ldn,
                                                int c0, int t, int m) {
    constexpr int Q = D / 4;
#pragma unroll
    for (int i = 0; i < N; ++i) {
        const int f = threadIdx.x + i * 256, j = c0 + f / Q;
        const int jn = j - t < 0 ? 0 : (j - t < m ? j - t : m - 1);
        const int row = (tab[(j >> lb) & (kPagedMaxTable - 1)] << lb) | (j & ((1 << lb) - 1));
        const float* src = j < t ? pool + int64_t(row) * ldc : fresh + int64_t(jn) * ldn;
        v[i] = *reinterpret_cast<const af32x4*>(src + (f % Q) * 4);
    }
}
// KV16: the pools hold bfloat16 words, the upper halves of fp32 values.  r(x) = `bf16_round_array` of autograd/cpu/ops.py as the
// 16-bit word it keeps: nearest, ties to even, +-0 and +-Inf kept, a finite value beyond the largest bfloat16 -> +-Inf (the carry
// runs into the exponent), a NaN -> (u >> 16) | 0x0040, a NaN whatever its low half held.  The one function of the seam load (a
// key of the same launch is attended to as r of it) and of the row store (what a later launch reads is that very word, widened)
__device__ __forceinline__ uint32_t bf16_word(float x) {
    const uint32_t u = __float_as_uint(x);
    return (u & 0x7FFFFFFFu) > 0x7F800000u ? (u >> 16) | 0x0040u : (u + 0x7FFFu + ((u >> 16) & 1u)) >> 16;
}
typedef uint32_t au32x2 __attribute__((ext_vector_type(2)));
// seam_load_paged with a pool of bfloat16 words (ldc counts them): the two sources take loads of different sizes, so a lane issues
// BOTH, each from an address that is always valid, and seam_settle16 selects.  The pool side is ONE 8-byte load of 4 words from
// row tab[j >> lb] << lb | (j & mask) (8-byte aligned: the entry checks the pools and ldc % 4) - for a key j >= t that is a row of a
// checked word, or of block 0 behind the reach: inside the pool, its words dropped; the new-token side is the 16-byte fp32 load
// from row j - t clamped to 0 .. m - 1 as in seam_load.  No branch, nothing converted here: all 2 N loads are in flight behind the
// MFMAs of the chunk before.  (A branch per lane around the two loads made the compiler wait for every load in flight in front
// of each pool load - the two sides shared destination registers -: profiles/paged_bf16.md)
template <int D, int N>
__device__ __forceinline__ void seam_load_paged16(af32x4 (&v)[N], au32x2 (&w)[N], const uint16_t* pool, int64_t ldc, const int* tab, int lb,
                                                  const float* fresh, int64_t ldn, int c0, int t, int m) {
    constexpr int Q = D / 4;
#pragma unroll
    for (int i = 0; i < N; ++i) {
        const int f = threadIdx.x + i * 256, j = c0 + f / Q;
        const int jn = j - t < 0 ? 0 : (j - t < m ? j - t : m - 1);
        const int row = (tab[(j >> lb) & (kPagedMaxTable - 1)] << lb) | (j & ((1 << lb) - 1));
        w[i] = *reinterpret_cast<const au32x2*>(pool + int64_t(row) * ldc + (f % Q) * 4);
        v[i] = *reinterpret_cast<const af32x4*>(fresh + int64_t(jn) * ldn + (f % Q) * 4);
    }
}
// ... and what it left in the registers -> the fp32 values the tiles take: for a key j < t the 4 pool words widened (w << 16),
// for a key t <= j < keys = t + m the 4 floats passed through r.  In registers, in front of seam_store with the c0 the load had
template <int D, int N>
__device__ __forceinline__ void seam_settle16(af32x4 (&v)[N], const au32x2 (&w)[N], int c0, int t, int keys) {
    constexpr int Q = D / 4;
#pragma unroll
    for (int i = 0; i < N; ++i) {
        const int f = threadIdx.x + i * 256, j = c0 + f / Q;
        // branches, not a select: the 64 lanes of a wave hold 64 / Q neighbouring keys, so only the waves that hold one of the
        // launch's own keys run the rounding (some 40 VALU instructions a register quad) - one wave in a decoding step
        if (j < t) {
            v[i] = af32x4{__uint_as_float(w[i][0] << 16), __uint_as_float(w[i][0] & 0xFFFF0000u), __uint_as_float(w[i][1] << 16),
                          __uint_as_float(w[i][1] & 0xFFFF0000u)};
        } else if (j < keys) {                                        // (a key >= t + m does not exist: seam_store writes 0 for it)
            v[i] = af32x4{__uint_as_float(bf16_word(v[i][0]) << 16), __uint_as_float(bf16_word(v[i][1]) << 16),
                          __uint_as_float(bf16_word(v[i][2]) << 16), __uint_as_float(bf16_word(v[i][3]) << 16)};
        }
    }
}
// ... and registers -> LDS: keys [t + m, Kend) of the chunk ZERO
template <int D, int N>
__device__ __forceinline__ void seam_store(const af32x4 (&v)[N], float* dst, int pitch, int c0, int keys, int Kend) {
    const int left = keys - c0, rows = left < 0 ? 0 : (left < kExtChunk ? left : kExtChunk);
    const int padded = Kend - c0 < kExtChunk ? Kend - c0 : kExtChunk;
    store_rows_padded<D, N>(v, dst, pitch, rows, padded);
}

// the slice behind the last slot of a packed launch: token rows cu[slots] .. tokens - 1 belong to nobody and become +0.0 in the
// context and in p, so that what the launch returns is determined whatever the projection buffer holds there.  The (x, head)
// workgroups of the slice share the rows in runs of 32
template <int D>
__device__ __forceinline__ void packed_clear(const ExtendArgs& a, int slots) {
    constexpr int Q4 = D / 4;
    const int tid = threadIdx.x, head = blockIdx.y, C = a.capacity, T = a.tokens;
    const int used = a.cu[slots];
    if (used < 0 || used > T) {
        if (tid == 0) __hip_atomic_fetch_or(a.status, LG_STATUS_BAD_INDEX, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
        return;
    }
    const af32x4 zero{0.f, 0.f, 0.f, 0.f};
    for (int lo = used + 32 * int(blockIdx.x); lo < T; lo += 32 * int(gridDim.x)) {
        const int hi = lo + 32 < T ? lo + 32 : T;
        float* oz = a.o + head * D;
        for (int f = tid; f < (hi - lo) * Q4; f += 256) *reinterpret_cast<af32x4*>(oz + int64_t(lo + f / Q4) * a.ldo + (f % Q4) * 4) = zero;
        if (a.p != nullptr) {
            float* pz = a.p + (int64_t(head) * T + lo) * C;              // rows lo .. hi - 1 of p are one dense run of floats
            const int total = (hi - lo) * C;
            const int ahead = int((4 - ((reinterpret_cast<uintptr_t>(pz) >> 2) & 3)) & 3);
            const int lead = ahead < total ? ahead : total, quads = (total - lead) / 4;
            for (int f = tid; f < lead; f += 256) pz[f] = 0.f;
            for (int f = tid; f < quads; f += 256) *reinterpret_cast<af32x4*>(pz + lead + 4 * f) = zero;
            for (int f = lead + 4 * quads + tid; f < total; f += 256) pz[f] = 0.f;
        }
    }
}

// PACKED (attn_packed<D>, lg_attention_extend_packed_f32): blockIdx.z is a cache SLOT whose token rows are rows cu[z] .. cu[z + 1] - 1
// of flat (tokens, .) operands; the caches, the positions and the mask are addressed by the slot as by a batch element, and the
// first row of the slot's tokens is a scalar like t and count.  A flag of the template and not a branch on a kernel argument:
// attn_extend<D>, the kernel of the three (b, m) entries, keeps the code, the registers and the time it had (the branch at run
// time compiled to 4 VGPRs fewer and a launch 5 % slower: profiles/serve_packed.md)
// PAGED (attn_paged<D>, lg_attention_extend_paged_f32, csrc/paged.hip): the counts form with the caches reached through a block
// table.  The slot's table (at most 128 words) is read ONCE into LDS by the first two waves, each word of the slot's reach
// 0 .. ceil((t + count) / B) - 1 checked against the pool on its way (one barrier with a vote, uniform over the workgroup: a bad
// word makes the slot bad like a bad position), the words behind the reach replaced by 0; every row address is formed from LDS
// KV16 (attn_paged_bf16<D>, lg_attention_extend_paged_bf16_f32, csrc/paged_bf16.hip): the paged form over pools of bfloat16 words -
// `k_cache` / `v_cache` of the arguments point to uint16_t then and ldc counts them.  Three places differ: the streamed keys
// (seam_load_paged16: 8 bytes per lane from the pool), their way into LDS (seam_settle16: widened, the launch's own keys rounded),
// and the store of the block's new rows (packed by the same r, 8 bytes per lane).  The tiles, the MFMAs, the softmax, the bias
// row, the fold order and the +0.0 rows are the text below, in fp32: the launch computes bit for bit what the paged one computes
// on the rounded new rows and the widened pools.  With KV16 = false nothing of it is compiled
template <int D, bool PACKED, bool PAGED = false, bool KV16 = false>
__device__ __forceinline__ void attn_extend_body(const ExtendArgs& a) {
    static_assert(!(PACKED && PAGED), "the paged launch is the counts form");
    static_assert(PAGED || !KV16, "the bfloat16 pools are a form of the paged launch");
    using CacheT = std::conditional_t<KV16, uint16_t, float>;
    extern __shared__ __attribute__((aligned(16))) float lds[];
    const int m = a.m, C = a.capacity, Cp = round32(C), PP = Cp + 4;
    constexpr int PQ = D + 4, PV = D + 8, Q4 = D / 4;
    constexpr int NB = 32 * Q4 / 256, NA = kExtChunk * Q4 / 256;
    if constexpr (PACKED) {
        if (blockIdx.z + 1 == gridDim.z) { packed_clear<D>(a, int(gridDim.z) - 1); return; }
    }
    const int t = a.pos[int64_t(blockIdx.z) * a.pos_pitch];       // uniform over the workgroup either way: a scalar load
    const int tid = threadIdx.x;
    // the element's real new tokens: each of the launch's m rows, or - lg_attention_extend_counts_f32 - the first count[b] of them.
    // From here on the element is computed as by a launch of its own with m = real; `m` stays the pitch of `p` and the rows to clear
    // (packed: the slot's rows cu[z + 1] - cu[z], at most m = m_max of them; its first row is workgroup-uniform like t)
    int real, row0 = 0;
    bool bad;
    if constexpr (PACKED) {
        row0 = a.cu[blockIdx.z];
        const int64_t n = int64_t(a.cu[blockIdx.z + 1]) - row0;
        bad = row0 < 0 || n < 0 || n > m || n + row0 > a.tokens || t < 0 || t > C - n;
        real = int(n);
    } else {
        real = a.count ? a.count[blockIdx.z] : m;
        bad = t < 0 || real < 0 || real > m || t > C - real;
    }
    if (bad) {
        // a bounds check, never a fault: nothing is written for this batch element (the others of a per-row launch are computed
        // as usual), the next synchronising call reports LG_EINDEX
        if (tid == 0) __hip_atomic_fetch_or(a.status, LG_STATUS_BAD_INDEX, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
        return;
    }
    float* Qs = lds;                      // Q rows of the block                    32 x PQ
    float* Ps = Qs + 32 * PQ;             // scores, then probabilities             32 x PP
    float* Buf = Ps + 32 * PP;            // a chunk of K (pitch PQ), then of V (pitch PV)
    float* Red = Buf + kExtChunk * PV;
    float* Bias = Red + 3 * 1024;         // what key j adds to every score of its column
    [[maybe_unused]] int* Tab = reinterpret_cast<int*>(Bias + Cp);       // PAGED: the slot's block table
    [[maybe_unused]] const int lb = a.log2_block;
    if constexpr (PAGED) {
        const int reach = (t + real + (1 << lb) - 1) >> lb;       // <= max_blocks, since t + real <= capacity
        int wrong = 0;
        if (tid < kPagedMaxTable) {
            int e = 0;
            if (tid < reach) {
                e = a.block_table[int64_t(blockIdx.z) * a.max_blocks + tid];
                wrong = e < 0 || e >= a.num_blocks;
            }
            Tab[tid] = wrong ? 0 : e;
        }
        if (__syncthreads_or(wrong)) {
            if (tid == 0) __hip_atomic_fetch_or(a.status, LG_STATUS_BAD_INDEX, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
            return;
        }
    }
    const int lane = tid & 63, wave = tid >> 6, r = lane & 31, h = lane >> 5;
    const int q0 = blockIdx.x * 32, head = blockIdx.y, b = blockIdx.z;
    if constexpr (PACKED) {
        // a block without a row of the slot is done: uniform over the workgroup, before any load, MFMA or barrier
        if (q0 >= real) return;
    } else if (real < m) {
        // rows of the block that are given but hold no token: +0.0 in the context and in p, so that what the launch returns is
        // determined.  A block without a real row is done then: uniform over the workgroup, before any load, MFMA or barrier
        const int lo = q0 > real ? q0 : real, hi = q0 + 32 < m ? q0 + 32 : m;
        const af32x4 zero{0.f, 0.f, 0.f, 0.f};
        float* oz = a.o + int64_t(b) * a.sbo + head * D;
        for (int f = tid; f < (hi - lo) * Q4; f += 256) *reinterpret_cast<af32x4*>(oz + int64_t(lo + f / Q4) * a.ldo + (f % Q4) * 4) = zero;
        if (a.p != nullptr && hi > lo) {
            float* pz = a.p + ((int64_t(b) * a.heads + head) * m + lo) * C;       // rows lo .. hi - 1 of p are one dense run of floats
            const int total = (hi - lo) * C;
            const int ahead = int((4 - ((reinterpret_cast<uintptr_t>(pz) >> 2) & 3)) & 3);       // floats in front of the first aligned float4
            const int lead = ahead < total ? ahead : total, quads = (total - lead) / 4;
            for (int f = tid; f < lead; f += 256) pz[f] = 0.f;
            for (int f = tid; f < quads; f += 256) *reinterpret_cast<af32x4*>(pz + lead + 4 * f) = zero;
            for (int f = lead + 4 * quads + tid; f < total; f += 256) pz[f] = 0.f;
        }
        if (q0 >= real) return;
    }
    const int qrows = real - q0 < 32 ? real - q0 : 32;                // rows of this block that exist
    const int keys = t + real;                                        // keys that exist in this launch
    const int Kend = round32(t + q0 + qrows);                         // the key columns the chunk loops cover (<= Cp)
    const CacheT* kc = reinterpret_cast<const CacheT*>(a.k_cache) + (PAGED ? 0 : int64_t(b) * a.sbc) + head * D;
    const CacheT* vc = reinterpret_cast<const CacheT*>(a.v_cache) + (PAGED ? 0 : int64_t(b) * a.sbc) + head * D;
    [[maybe_unused]] au32x2 rw[KV16 ? NA : 1];                        // KV16: the pool side of the streamed chunk, 4 bfloat16 words a lane
    // the streamed keys / values of a chunk: the contiguous rows of the element, or the pool through the table
    auto stream = [&](af32x4 (&v)[NA], const CacheT* cache, const float* fresh, int64_t ldn, int c0) {
        if constexpr (KV16)       seam_load_paged16<D, NA>(v, rw, cache, a.ldc, Tab, lb, fresh, ldn, c0, t, real);
        else if constexpr (PAGED) seam_load_paged<D, NA>(v, cache, a.ldc, Tab, lb, fresh, ldn, c0, t, real);
        else                      seam_load<D, NA>(v, cache, a.ldc, fresh, ldn, c0, t, real);
    };
    // the element's token rows: a batch pitch, or - packed - the slot's first row of the flat operands
    const float* kn = a.k_new + (PACKED ? int64_t(row0) * a.ldk : int64_t(b) * a.sbk) + head * D;
    const float* vn = a.v_new + (PACKED ? int64_t(row0) * a.ldv : int64_t(b) * a.sbv) + head * D;
    const float* qn = a.q + (PACKED ? int64_t(row0) * a.ldq : int64_t(b) * a.sbq) + head * D;
    float* on = a.o + (PACKED ? int64_t(row0) * a.ldo : int64_t(b) * a.sbo) + head * D;
    // row 0 of the element in p: (batch, heads, m, capacity), or - packed - (heads, tokens, capacity)
    const int64_t prow = PACKED ? int64_t(head) * a.tokens + row0 : (int64_t(b) * a.heads + head) * m;

    af32x4 rc[NA];
    {
        af32x4 rq[NB], rk[NB], rv[NB];
        load_rows<D, NB>(rq, qn + int64_t(q0) * a.ldq, a.ldq, qrows);
        load_rows<D, NB>(rk, kn + int64_t(q0) * a.ldk, a.ldk, qrows);
        load_rows<D, NB>(rv, vn + int64_t(q0) * a.ldv, a.ldv, qrows);
        stream(rc, kc, kn, a.ldk, 0);
        store_rows_padded<D, NB>(rq, Qs, PQ, qrows, 32);
        // the block's own new rows become rows t + q0 .. of the caches, bit for bit; nothing in this launch reads them there
        if constexpr (KV16) {
            // ... of the bfloat16 pool: the same rows, each value as the word r leaves of it, one 8-byte store per lane and pool
            uint16_t *k16 = reinterpret_cast<uint16_t*>(a.k_cache), *v16 = reinterpret_cast<uint16_t*>(a.v_cache);
#pragma unroll
            for (int i = 0; i < NB; ++i) {
                const int f = tid + i * 256;
                if (f < qrows * Q4) {
                    const int j = t + q0 + f / Q4;
                    const int64_t at = int64_t((Tab[j >> lb] << lb) | (j & ((1 << lb) - 1))) * a.ldc + head * D + (f % Q4) * 4;
                    *reinterpret_cast<au32x2*>(k16 + at) = au32x2{bf16_word(rk[i][0]) | (bf16_word(rk[i][1]) << 16), bf16_word(rk[i][2]) | (bf16_word(rk[i][3]) << 16)};
                    *reinterpret_cast<au32x2*>(v16 + at) = au32x2{bf16_word(rv[i][0]) | (bf16_word(rv[i][1]) << 16), bf16_word(rv[i][2]) | (bf16_word(rv[i][3]) << 16)};
                }
            }
        } else if constexpr (PAGED) {
            // ... of the pool: position t + q0 + i through the table (its words up to the reach are checked), a row of its own block
#pragma unroll
            for (int i = 0; i < NB; ++i) {
                const int f = tid + i * 256;
                if (f < qrows * Q4) {
                    const int j = t + q0 + f / Q4;
                    const int64_t at = int64_t((Tab[j >> lb] << lb) | (j & ((1 << lb) - 1))) * a.ldc + head * D + (f % Q4) * 4;
                    *reinterpret_cast<af32x4*>(a.k_cache + at) = rk[i];
                    *reinterpret_cast<af32x4*>(a.v_cache + at) = rv[i];
                }
            }
        } else {
            float* kd = a.k_cache + int64_t(b) * a.sbc + int64_t(t + q0) * a.ldc + head * D;
            float* vd = a.v_cache + int64_t(b) * a.sbc + int64_t(t + q0) * a.ldc + head * D;
#pragma unroll
            for (int i = 0; i < NB; ++i) {
                const int f = tid + i * 256;
                if (f < qrows * Q4) {
                    *reinterpret_cast<af32x4*>(kd + int64_t(f / Q4) * a.ldc + (f % Q4) * 4) = rk[i];
                    *reinterpret_cast<af32x4*>(vd + int64_t(f / Q4) * a.ldc + (f % Q4) * 4) = rv[i];
                }
            }
        }
        // (1.0 - mask) * -10000.0 in fp32, the composite's own arithmetic; -0.0f where the mask is 1 or absent or the key does
        // not exist: adding it changes no bit of a score
        for (int j = tid; j < Kend; j += 256) Bias[j] = (j < keys && a.mask) ? (1.0f - a.mask[int64_t(b) * a.sbm + j]) * -10000.0f : -0.0f;
    }

    // scores: the keys arrive in chunks of 128; wave w takes keys [c0 + 32 w, c0 + 32 w + 32) of the chunk, scaled (the product
    // rounded to fp32 first, like `scores * c`).  Columns [Kend, Cp) of the tile are never written and never read
    for (int c0 = 0; c0 < Kend; c0 += kExtChunk) {
        if constexpr (KV16) seam_settle16<D, NA>(rc, rw, c0, t, keys);
        seam_store<D, NA>(rc, Buf, PQ, c0, keys, Kend);
        __syncthreads();
        if (c0 + kExtChunk < Kend) stream(rc, kc, kn, a.ldk, c0 + kExtChunk);
        else                       stream(rc, vc, vn, a.ldv, 0);      // the first chunk of V flies behind the softmax
        const int rows = Kend - c0 < kExtChunk ? Kend - c0 : kExtChunk;
        if (32 * wave < rows) {
            af32x16 acc = zero16();
            wave_mma<true, true>(acc, Qs, PQ, Buf + 32 * wave * PQ, PQ, D, r, h);
            const int col = c0 + 32 * wave + r;
            const float bias = Bias[col];
#pragma unroll
            for (int e = 0; e < 16; ++e) Ps[acc_row(e, h) * PP + col] = acc[e] * a.scale + bias;
        }
        __syncthreads();
    }

    // softmax of each row: 8 threads per row, float4 columns sub, sub + 8, ... held in registers between the three passes;
    // exp(x - max) * (1 / sum) over the keys the row sees, [0, t + q0 + row]: a key beyond is no part of the max or the sum, its
    // column of the LDS tile becomes 0 (it is an MFMA operand of the context) and +0.0 is what `p` holds for it up to the capacity
    {
        const int row = tid >> 3, sub = tid & 7;
        const int vis = t + q0 + row + 1 < keys ? t + q0 + row + 1 : keys;       // key 0 is always one of them
        float* pr = Ps + row * PP;
        af32x4 x[kExtMaxBlocks];
        float mx = -INFINITY;
#pragma unroll
        for (int i = 0; i < kExtMaxBlocks; ++i) {
            const int c = sub * 4 + 32 * i;
            x[i] = af32x4{0.f, 0.f, 0.f, 0.f};
            if (c < Kend) {
                x[i] = *reinterpret_cast<const af32x4*>(pr + c);
#pragma unroll
                for (int e = 0; e < 4; ++e)
                    if (c + e < vis) mx = (x[i][e] > mx || x[i][e] != x[i][e]) ? x[i][e] : mx;
            }
        }
#pragma unroll
        for (int off = 1; off < 8; off <<= 1) { const float o = __shfl_xor(mx, off, 64); mx = (o > mx || o != o) ? o : mx; }
        float s = 0.f;
#pragma unroll
        for (int i = 0; i < kExtMaxBlocks; ++i) {
            const int c = sub * 4 + 32 * i;
            if (c < Kend) {
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    if (c + e < vis) { x[i][e] = expf(x[i][e] + (-mx)); s += x[i][e]; }
                    else x[i][e] = 0.f;
                }
            }
        }
#pragma unroll
        for (int off = 1; off < 8; off <<= 1) s += __shfl_xor(s, off, 64);
        const float inv = 1.0f / s;
        const bool stored = a.p != nullptr && row < qrows;
        float* pg = a.p + (prow + q0 + (row < qrows ? row : 0)) * C;
#pragma unroll
        for (int i = 0; i < kExtMaxBlocks; ++i) {
            const int c = sub * 4 + 32 * i;
            if (c < Cp) {
                if (c < Kend) {
#pragma unroll
                    for (int e = 0; e < 4; ++e) x[i][e] *= inv;
                    *reinterpret_cast<af32x4*>(pr + c) = x[i];
                }
                if (stored) {
                    if ((C & 3) == 0) {
                        if (c < C) *reinterpret_cast<af32x4*>(pg + c) = x[i];
                    } else {
#pragma unroll
                        for (int e = 0; e < 4; ++e)
                            if (c + e < C) pg[c + e] = x[i][e];
                    }
                }
            }
        }
    }

    // context = P @ V: D / 32 column tiles, the keys of every chunk split over the remaining waves; the partial sums stay in
    // registers across the chunks and fold in wave order at the end
    constexpr int NT = D / 32, KP = 4 / NT;
    const int n = wave % NT, kp = wave / NT;
    af32x16 acc = zero16();
    for (int c0 = 0; c0 < Kend; c0 += kExtChunk) {
        if constexpr (KV16) seam_settle16<D, NA>(rc, rw, c0, t, keys);
        seam_store<D, NA>(rc, Buf, PV, c0, keys, Kend);
        __syncthreads();                                              // (the first one also publishes the probabilities in LDS)
        if (c0 + kExtChunk < Kend) stream(rc, vc, vn, a.ldv, c0 + kExtChunk);
        const int rows = Kend - c0 < kExtChunk ? Kend - c0 : kExtChunk, kspan = rows / KP;
        wave_mma<true, false>(acc, Ps + c0 + kp * kspan, PP, Buf + kp * kspan * PV + 32 * n, PV, kspan, r, h);
        __syncthreads();
    }
    if (kp > 0) {
#pragma unroll
        for (int e = 0; e < 16; ++e) Red[((kp - 1) * NT + n) * 1024 + e * 64 + lane] = acc[e];
    }
    __syncthreads();
    if (kp == 0) {
        for (int q = 1; q < KP; ++q) {
#pragma unroll
            for (int e = 0; e < 16; ++e) acc[e] += Red[((q - 1) * NT + n) * 1024 + e * 64 + lane];
        }
        float* og = on + int64_t(q0) * a.ldo + 32 * n + r;
#pragma unroll
        for (int e = 0; e < 16; ++e)
            if (acc_row(e, h) < qrows) og[int64_t(acc_row(e, h)) * a.ldo] = acc[e];
    }
}

static bool extend_operand(const void* p, int64_t ld, int64_t sb) { return p && aligned16(p) && ld >= 0 && sb >= 0 && ld % 4 == 0 && sb % 4 == 0; }

// do the floats [x, x + (batch - 1) sb + (rows - 1) ld + w) and [y, ...) share an address?
static bool extend_overlap(const float* x, int64_t ldx, int64_t sbx, int64_t rowsx, const float* y, int64_t ldy, int64_t sby, int64_t rowsy,
                           int64_t batch, int64_t w) {
    const float* xe = x + (batch - 1) * sbx + (rowsx - 1) * ldx + w;
    const float* ye = y + (batch - 1) * sby + (rowsy - 1) * ldy + w;
    return x < ye && y < xe;
}

// do the `words` position words share an address with the floats [c, c + (batch - 1) sbc + (capacity - 1) ldc + w) of a cache?
static bool positions_overlap(const int32_t* pos, int64_t words, const float* c, int64_t ldc, int64_t sbc, int64_t capacity, int64_t batch, int64_t w) {
    const char *x = reinterpret_cast<const char*>(pos), *xe = x + 4 * words;
    const char *y = reinterpret_cast<const char*>(c), *ye = reinterpret_cast<const char*>(c + (batch - 1) * sbc + (capacity - 1) * ldc + w);
    return x < ye && y < xe;
}

// do the `words` int32 words at x share an address with the `bytes` bytes at y?
static bool words_overlap(const int32_t* x, int64_t words, const void* y, int64_t bytes) {
    const char *a = reinterpret_cast<const char*>(x), *ae = a + 4 * words, *b = static_cast<const char*>(y);
    return y != nullptr && a < b + bytes && b < ae;
}

}  // namespace lg
