// The row body of the sampling launches, sample_row_body<LDS, GREEDY, OutT>, with what it stands on (the row as keys, the radix
// select, the integer weights), and the host's choice of kernel, threads and LDS: included by sample.hip (lg_sample_f32: one set
// of parameters and one call of the global stream for all rows, GREEDY = false) and by sample_rows.hip (lg_sample_rows_f32: every
// row with the parameters, the seed and the counter of its own table row, GREEDY = true: inv_t == +0.0 answers the argmax).
// What differs between the two arrives as arguments: inv_t, top_k, top_p and the Philox counter and key of the row.
//
// One workgroup per row.  The row is staged once into LDS with 16-byte loads from its first aligned element (kernel 0: every
// row of at most kSampleMaxLdsCols floats - a 30522-wide vocabulary is 122 KB of the CU's 160 KiB), as order-preserving 32-bit
// KEYS of its values (-0.0 canonicalised to +0.0), and every later pass reads the keys from there; a wider row takes the same
// passes from memory (kernel 1).  The passes:
//   1. max and argmax with the combine of argreduce.hip (`beats`), on the values in flight while the row is staged (a pass of
//      its own in kernel 1): a row with a NaN, +inf or an all -inf row answers that argmax and is done;
//   2. top-k: the k-th largest value by a radix select on the keys - three passes of 11, 11 and 10 bits from the top down, 2048
//      bins holding COUNTS;
//   3. W, the sum of the weights q over K;
//   4. top-p: the same three-pass select with the bins holding MASS, which gives the largest value whose mass at or above it
//      reaches top_p * W;
//   5. a blocked scan in index order over N: each thread sums a contiguous run, the runs are scanned over the wave and the
//      workgroup, and the one thread whose run holds the target walks it to the token.
// A pass costs what its instructions per element cost on ONE CU (about 0.2 us per instruction and element at 30522 columns), which
// is why the keys are staged, the row is read four elements at a time without a test per element, and members of K are told by
// one integer compare.
//
// FIXED POINT.  A weight is q_j = floor(2^shift * __expf((x_j - m) * inv_T)), a 64-bit integer (shift = 40 for every row of
// fewer than 2^22 elements: each q is exact to 2^-40 of the largest weight, which is exactly 2^shift).  Counts, W, the bins'
// masses and the running sums are then INTEGER sums: exact in any order, so the LDS atomics that fill the bins and every fold
// give the same bits on every run without any fixed order, and the scan compares C_i * 2^25 >= (2h + 1) * W' exactly (u = (2h +
// 1) / 2^25 with h the top 24 bits of the row's word), which always has a solution.  No running fp32 sum exists anywhere.
//
// The token depends on (the row, inv_t, top_k, top_p, the 24 bits of the Philox word) alone: two launches that hand the body equal
// values give equal bits.
#pragma once
#include "common.h"
#include "rng_common.h"
#include <cmath>
#include <climits>

namespace lg {

typedef unsigned long long u64;
typedef unsigned __int128 u128;

constexpr int kSampleBins = 2048;                                        // 11 bits of the key a pass (the last one: 10)
constexpr int kSampleHistBytes = kSampleBins * 8;                        // 16 KiB
constexpr int kSampleLdsBytes = 160 * 1024;                              // the CU's LDS: what one workgroup may declare
constexpr int kSampleStaticBytes = 1024;                                 // SampleShared below, in front of the bins: all of the LDS is
                                                                         // dynamic, so its base - and the staged row - is 16-byte aligned
constexpr int64_t kSampleRowFloats = (kSampleLdsBytes - kSampleHistBytes - kSampleStaticBytes) / 4;
constexpr int64_t kSampleMaxLdsCols = kSampleRowFloats - 4;              // up to three floats in front keep the row's 16-byte phase
constexpr int kSampleMaxWaves = 16;
constexpr int64_t kSampleNone = INT64_MAX;

struct SampleShared {
    u64       call[2];                                                   // seed, draws
    u64       wave_total[kSampleMaxWaves];
    long long wave_i[kSampleMaxWaves];
    float     wave_v[kSampleMaxWaves];
    u64       sel_rem;
    uint32_t  sel_digit;
    // sample_rows.hip only: what thread 0 read for the row - the 8 words of its table row, its counter, and what to do with it
    int32_t   row_words[8];
    int32_t   row_counter;
    int32_t   row_kind;                                                  // kSampleRowDraw / Free / Bad
};
static_assert(sizeof(SampleShared) <= kSampleStaticBytes, "SampleShared outgrew its share of the LDS");

// the combine of argreduce.hip: does (v, i) beat (w, j) for argmax?
__device__ __forceinline__ bool sample_beats(float v, long long i, float w, long long j) {
    const bool vn = v != v, wn = w != w;
    if (vn || wn) return vn && (!wn || i < j);
    return v > w || (!(w > v) && i < j);
}

// larger value <=> larger key; -0.0 and +0.0 share one key.  (No NaN reaches a key: such a row is degenerate.)
__device__ __forceinline__ uint32_t sample_key(float x) {
    uint32_t b = __float_as_uint(x);
    if (b == 0x80000000u) b = 0u;
    return b ^ ((b >> 31) ? 0xFFFFFFFFu : 0x80000000u);
}

// the value whose key is k (no value has the key 0)
__device__ __forceinline__ float sample_value(uint32_t k) {
    return __uint_as_float(k ^ ((k >> 31) ? 0x80000000u : 0xFFFFFFFFu));
}

// the weight of the value x with key k as an integer: floor(scale * exp((x - m) * inv_t)); -inf gives 0.  One expression for
// every pass.
__device__ __forceinline__ u64 sample_q(uint32_t k, float m, float inv_t, float scale) {
    return u64(__fmul_rn(__expf(__fmul_rn(__fsub_rn(sample_value(k), m), inv_t)), scale));
}

__device__ __forceinline__ u64 sample_wave_sum(u64 v) {                  // every lane ends with the wave's sum
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
    return v;
}

__device__ __forceinline__ u64 sample_wave_scan(u64 v, int lane) {      // inclusive, by increasing lane
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
        const u64 t = __shfl_up(v, off, 64);
        if (lane >= off) v += t;
    }
    return v;
}

// the sum of one value per thread over the workgroup (ends with a barrier passed; sh.wave_total is free again after the next one)
__device__ __forceinline__ u64 sample_block_sum(u64 v, SampleShared& sh, int lane, int wave, int nw) {
    v = sample_wave_sum(v);
    __syncthreads();                                                     // the previous user of wave_total is done
    if (lane == 0) sh.wave_total[wave] = v;
    __syncthreads();
    u64 total = 0;
    for (int w = 0; w < nw; ++w) total += sh.wave_total[w];
    return total;
}

// The row as the passes read it: KEYS.  LDS: `p` is the 16-byte aligned buffer and the key of element i is its word off + i (the
// staging converts once; the value comes back from the key where a weight is needed) - the passes walk it with 16-byte reads, four
// elements each, with no test per element: the up to three words in front of element 0 and behind the last hold the key of -inf,
// which every pass may see (weight 0; counted by the top-k select only where the k-th largest value is -inf itself and the
// answer is "everything" either way; never returned, because the scan stops at a positive weight).  Memory: `p` is the row
// itself, off == 0, scalar reads, the key computed on the way.
template <bool LDS>
struct SampleRow {
    const void* p;
    int off;
    int64_t cols;

    template <class F>
    __device__ __forceinline__ void vector(int v, F& f) const {          // the four words of vector v (i < 0 or >= cols: -inf)
        const uint4 k = reinterpret_cast<const uint4*>(p)[v];
        const int i = 4 * v - off;
        f(int64_t(i), k.x); f(int64_t(i + 1), k.y); f(int64_t(i + 2), k.z); f(int64_t(i + 3), k.w);
    }

    // f(i, key) over this thread's share of the row, by increasing i: the threads interleave
    template <class F>
    __device__ __forceinline__ void each(F f) const {
        const int tid = threadIdx.x, T = blockDim.x;
        if constexpr (LDS) {
            const int nvec = (off + int(cols) + 3) >> 2;
#pragma unroll 2
            for (int v = tid; v < nvec; v += T) vector(v, f);
        } else {
            for (int64_t i = tid; i < cols; i += T) f(i, sample_key(static_cast<const float*>(p)[i]));
        }
    }

    // f(i, key) over the contiguous run of this thread, by increasing i: thread t's run lies in front of thread t + 1's.  An odd
    // number of vectors (elements) per run: the threads of a wave start on different LDS banks
    template <class F>
    __device__ __forceinline__ void run(F f) const {
        const int tid = threadIdx.x, T = blockDim.x;
        if constexpr (LDS) {
            const int nvec = (off + int(cols) + 3) >> 2, per = ((nvec + T - 1) / T) | 1;
            const int v0 = tid * per < nvec ? tid * per : nvec, v1 = v0 + per < nvec ? v0 + per : nvec;
#pragma unroll 2
            for (int v = v0; v < v1; ++v) vector(v, f);
        } else {
            const int64_t per = ((cols + T - 1) / T) | 1;
            const int64_t i0 = int64_t(tid) * per < cols ? int64_t(tid) * per : cols, i1 = i0 + per < cols ? i0 + per : cols;
            for (int64_t i = i0; i < i1; ++i) f(i, sample_key(static_cast<const float*>(p)[i]));
        }
    }
};

// The largest key v occurring in the row with sum{weight_j : key_j >= v} >= target, 1 <= target <= the sum of all weights
// (integers: exact).  Three passes over the key's bits 31 .. 21, 20 .. 10 and 9 .. 0; a pass counts only the elements that match
// the bits chosen so far.  (Eleven bits - sign, exponent and two bits of the mantissa - spread logits over enough bins that
// the atomics of a wave rarely meet.)  blockDim.x divides kSampleBins.
template <class Row, class WF>
__device__ __forceinline__ uint32_t sample_select(const Row& row, u64 target, WF weight, u64* hist, SampleShared& sh) {
    const int tid = threadIdx.x, T = blockDim.x, lane = tid & 63, wave = tid >> 6;
    uint32_t prefix = 0;
    u64 rem = target;
#pragma unroll 1
    for (int pass = 0; pass < 3; ++pass) {
        const int low = pass == 0 ? 21 : pass == 1 ? 10 : 0;
        const uint32_t digit = pass == 2 ? 1023u : 2047u, above = pass == 0 ? 0u : 0xFFFFFFFFu << (pass == 1 ? 21 : 10);
        __syncthreads();                                                 // the bins' previous readers are done
        for (int b = tid; b < kSampleBins; b += T) hist[b] = 0;
        __syncthreads();
        row.each([&](int64_t, uint32_t k) {
            if ((k & above) == prefix) {
                const u64 w = weight(k);
                if (w != 0) atomicAdd(hist + ((k >> low) & digit), w);
            }
        });
        __syncthreads();
        // thread t holds the bins 2047 - t * per - j, j < per: an inclusive scan over the threads runs from the top bin down
        const int per = kSampleBins / T;
        const u64* const h = hist + (kSampleBins - 1 - tid * per);
        u64 val = 0;
        for (int j = 0; j < per; ++j) val += h[-j];
        u64 incl = sample_wave_scan(val, lane);
        if (lane == 63) sh.wave_total[wave] = incl;
        __syncthreads();
        for (int w = 0; w < wave; ++w) incl += sh.wave_total[w];
        if (incl >= rem && incl - val < rem) {                           // exactly one thread: the target is reached in one of its bins
            u64 c = incl - val;
            for (int j = 0; j < per; ++j) {
                const u64 b = h[-j];
                if (c + b >= rem) {
                    sh.sel_digit = uint32_t(kSampleBins - 1 - tid * per - j);
                    sh.sel_rem = rem - c;
                    break;
                }
                c += b;
            }
        }
        __syncthreads();
        prefix |= sh.sel_digit << low;
        rem = sh.sel_rem;
    }
    return prefix;
}

// One row: `g` its logits, `sample_dyn` the workgroup's dynamic LDS (SampleShared, the bins, the staged row), (c0 .. c3), (k0, k1)
// the Philox counter and key whose word 0 gives u.  Every argument is uniform over the workgroup, and every thread of it calls.
// GREEDY: inv_t == +0.0 answers the argmax where a degenerate row answers it, in front of every other pass.
template <bool LDS, bool GREEDY, typename OutT>
__device__ __forceinline__ void sample_row_body(unsigned char* sample_dyn, const float* __restrict__ g, int64_t row, int64_t cols, float inv_t,
                                                int64_t top_k, double top_p, float scale, OutT* __restrict__ out, uint32_t c0, uint32_t c1,
                                                uint32_t c2, uint32_t c3, uint32_t k0, uint32_t k1) {
    SampleShared& sh = *reinterpret_cast<SampleShared*>(sample_dyn);
    u64* const hist = reinterpret_cast<u64*>(sample_dyn + kSampleStaticBytes);
    const int tid = threadIdx.x, T = blockDim.x, lane = tid & 63, wave = tid >> 6, nw = T >> 6;
    SampleRow<LDS> r{g, 0, cols};                                        // (kernel 1: as it stands; kernel 0: the buffer, below)

    // 0. and 1. stage the row (LDS) and find max and argmax.  A thread visits its elements by increasing index: the running
    // update is rules 1 and 2 of the combine
    float bv = -INFINITY;
    long long bi = kSampleNone;
    const auto absorb = [&](int64_t i, float x) {
        const bool take = !(bv >= x) && bv == bv;
        bv = take ? x : bv;
        bi = take ? i : bi;
    };
    const auto absorb4 = [&](int64_t i, const float4& x) { absorb(i, x.x); absorb(i + 1, x.y); absorb(i + 2, x.z); absorb(i + 3, x.w); };
    if constexpr (LDS) {
        // global element i goes to word off + i of the buffer, off = the row's phase within 16 bytes
        uint32_t* const buf = reinterpret_cast<uint32_t*>(sample_dyn + kSampleStaticBytes + kSampleHistBytes);
        const auto keys = [](const float4& x) { return uint4{sample_key(x.x), sample_key(x.y), sample_key(x.z), sample_key(x.w)}; };
        const int off = int((reinterpret_cast<uintptr_t>(g) >> 2) & 3);
        int64_t head = (4 - off) & 3;
        if (head > cols) head = cols;
        if (tid < head) { const float x = g[tid]; buf[off + tid] = sample_key(x); absorb(tid, x); }
        const int64_t nv = (cols - head) >> 2;
        const float4* const g4 = reinterpret_cast<const float4*>(g + head);
        uint4* const b4 = reinterpret_cast<uint4*>(buf + off + head);
        int64_t v = tid;
        for (; v + 3 * int64_t(T) < nv; v += 4 * int64_t(T)) {           // four loads in flight per thread
            const float4 a0 = g4[v], a1 = g4[v + T], a2 = g4[v + 2 * int64_t(T)], a3 = g4[v + 3 * int64_t(T)];
            b4[v] = keys(a0); b4[v + T] = keys(a1); b4[v + 2 * int64_t(T)] = keys(a2); b4[v + 3 * int64_t(T)] = keys(a3);
            absorb4(head + 4 * v, a0); absorb4(head + 4 * (v + T), a1);
            absorb4(head + 4 * (v + 2 * int64_t(T)), a2); absorb4(head + 4 * (v + 3 * int64_t(T)), a3);
        }
        for (; v < nv; v += T) { const float4 a = g4[v]; b4[v] = keys(a); absorb4(head + 4 * v, a); }
        const int64_t t0 = head + 4 * nv;
        if (t0 + tid < cols) { const float x = g[t0 + tid]; buf[off + t0 + tid] = sample_key(x); absorb(t0 + tid, x); }
        if (tid < off) buf[tid] = sample_key(-INFINITY);                 // the words around the row that the 16-byte reads see
        if (tid < 4 * ((off + int(cols) + 3) >> 2) - off - int(cols)) buf[off + cols + tid] = sample_key(-INFINITY);
        r.p = buf;
        r.off = off;
    } else {
        for (int64_t i = tid; i < cols; i += T) absorb(i, g[i]);
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const float ov = __shfl_xor(bv, o, 64);
        const long long oi = __shfl_xor(bi, o, 64);
        if (sample_beats(ov, oi, bv, bi)) { bv = ov; bi = oi; }
    }
    if (lane == 0) { sh.wave_v[wave] = bv; sh.wave_i[wave] = bi; }
    __syncthreads();                                                     // (the staged row is complete, too)
    bv = sh.wave_v[0]; bi = sh.wave_i[0];
    for (int w = 1; w < nw; ++w)
        if (sample_beats(sh.wave_v[w], sh.wave_i[w], bv, bi)) { bv = sh.wave_v[w]; bi = sh.wave_i[w]; }
    if (bi == kSampleNone) bi = 0;                                       // nothing but -inf: the first index
    if (bv != bv || bv == INFINITY || bv == -INFINITY || (GREEDY && inv_t == 0.0f)) {    // a degenerate row answers its argmax, a greedy one too
        if (tid == 0) out[row] = OutT(bi);
        return;
    }
    const float m = bv;

    // 2. top-k: K = {key >= kkey}
    uint32_t nkey = 0;                                                   // N = {key >= nkey}; 0: everything
    if (top_k >= 1 && top_k < cols)
        nkey = sample_select(r, u64(top_k), [](uint32_t) { return u64(1); }, hist, sh);

    // 3. and 4. top-p: the largest value whose mass at or above it reaches top_p * W
    if (top_p < 1.0) {
        u64 mine = 0;
        const uint32_t kkey = nkey;
        r.each([&](int64_t, uint32_t k) {
            if (k >= kkey) mine += sample_q(k, m, inv_t, scale);
        });
        const u64 W = sample_block_sum(mine, sh, lane, wave, nw);
        u64 target = u64(double(W) * top_p);
        if (double(target) < double(W) * top_p) target += 1;             // the ceiling
        if (target > W) target = W;
        if (target < 1) target = 1;
        nkey = sample_select(r, target, [=](uint32_t k) { return k >= kkey ? sample_q(k, m, inv_t, scale) : u64(0); }, hist, sh);
    }

    // 5. the blocked scan over N in index order: every thread sums its contiguous run
    u64 s = 0;
    r.run([&](int64_t, uint32_t k) {
        if (k >= nkey) s += sample_q(k, m, inv_t, scale);
    });
    const u64 incl = sample_wave_scan(s, lane);
    __syncthreads();                                                     // the previous user of wave_total is done
    if (lane == 63) sh.wave_total[wave] = incl;
    __syncthreads();
    u64 before = 0, total = 0;
    for (int w = 0; w < nw; ++w) {
        const u64 t = sh.wave_total[w];
        before += w < wave ? t : 0;
        total += t;
    }
    uint32_t word[4];
    philox4x32_10(c0, c1, c2, c3, k0, k1, word);
    const u128 aim = u128(total) * u128(2u * (word[0] >> 8) + 1u);       // C_i * 2^25 >= aim  <=>  C_i >= u * W'
    u64 c = before + incl - s;                                           // the running sum in front of this thread's run
    if ((u128(c) << 25) < aim && aim <= (u128(c + s) << 25)) {           // exactly one thread: the target lies in its run
        bool found = false;
        r.run([&](int64_t i, uint32_t k) {
            if (found) return;
            if (k >= nkey) c += sample_q(k, m, inv_t, scale);
            if ((u128(c) << 25) >= aim) { out[row] = OutT(i); found = true; }
        });
    }
}

// ---- host: what both entries choose from the width of a row ---------------------------------------------------------------------
struct SampleShape {
    float  scale;                                        // 2^shift: the weight of the row's maximum
    bool   lds_row;                                      // kernel 0 (the row staged in LDS) or kernel 1
    int    threads;
    size_t lds;                                          // dynamic LDS in bytes
    int    vec;                                          // 1 when the row is staged with 16-byte loads
};

inline SampleShape sample_shape(int64_t cols) {
    // 2^shift * cols < 2^63: the integer sums cannot overflow; 40 for every row of fewer than 2^22 elements
    int bits = 0;
    while ((int64_t(1) << bits) <= cols) ++bits;
    const int shift = bits <= 22 ? 40 : 62 - bits;
    SampleShape s;
    s.scale = float(double(uint64_t(1) << shift));
    s.lds_row = cols <= kSampleMaxLdsCols;
    s.threads = cols <= 8192 ? 256 : 1024;
    s.lds = size_t(kSampleStaticBytes + kSampleHistBytes) + (s.lds_row ? size_t((cols + 4 + 3) & ~int64_t(3)) * 4 : 0);
    s.vec = s.lds_row && cols >= 7 ? 1 : 0;              // (a row of seven floats holds an aligned float4 wherever it starts)
    return s;
}

// sample.hip: what lg_sample_last_plan reports of the calling thread's most recent sampling launch
void note_sample_plan(int kernel, int threads, int passes, int vec);

}  // namespace lg
