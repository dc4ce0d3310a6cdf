// The counter-based random stream on the device: Philox4x32-10, the layout of Runtime::rng_state, and the protocol by which ONE
// launch both uses `draws` and advances it (dropout.hip explains it; the dropout inside the attention kernels takes the same
// steps from here).  Stream definition: lightgrad_amd/random.py, include/lghip.h.
#pragma once
#include "common.h"

namespace lg {

constexpr int kRngMaxGroup = 4096;                 // workgroups per first-level ticket, at most: 2^24 workgroups, 2^34 elements a call
constexpr int64_t kRngMaxElements = int64_t(kRngMaxGroup) * kRngMaxGroup * 1024;
constexpr int kRngGroups = kRngMaxGroup;           // first-level tickets
constexpr int kRngLine = 16;                       // ints per ticket line (64 bytes: what one memory-side atomic request covers)
// layout of Runtime::rng_state (64-bit words): [0] seed, [1] draws; from byte 128 on the ticket lines: the top one, then the groups'
constexpr size_t kRngTicketByte = 128;
constexpr size_t kRngStateBytes = kRngTicketByte + size_t(kRngGroups + 1) * kRngLine * sizeof(int);

__device__ __forceinline__ void philox4x32_10(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t k0, uint32_t k1,
                                               uint32_t (&out)[4]) {
#pragma unroll
    for (int round = 0; round < 10; ++round) {
        const uint64_t p0 = uint64_t(0xD2511F53u) * c0, p1 = uint64_t(0xCD9E8D57u) * c2;     // (one 32 x 32 -> 64 multiply each)
        const uint32_t n0 = uint32_t(p1 >> 32) ^ c1 ^ k0, n2 = uint32_t(p0 >> 32) ^ c3 ^ k1;
        c0 = n0; c1 = uint32_t(p1); c2 = n2; c3 = uint32_t(p0);
        k0 += 0x9E3779B9u; k1 += 0xBB67AE85u;
    }
    out[0] = c0; out[1] = c1; out[2] = c2; out[3] = c3;
}

// ---- the protocol of a launch that draws: every step is thread 0's of a workgroup ---------------------------------------------
// 1. seed and `draws` (agent scope) into call[0], call[1] (LDS); `draws` is in a register before a ticket is taken
__device__ __forceinline__ void rng_read_call(unsigned long long* state, unsigned long long* call) {
    call[0] = state[0];
    call[1] = __hip_atomic_load(state + 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
}

__device__ __forceinline__ int* rng_tickets(unsigned long long* state) {
    return reinterpret_cast<int*>(reinterpret_cast<char*>(state) + kRngTicketByte);
}

// 2. the ticket of group `grp` (workgroup index / group): the order of arrival within the group
__device__ __forceinline__ int rng_take_ticket(int* mine) {
    return __hip_atomic_fetch_add(mine, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// (uniform values out of LDS: in scalar registers the ten key additions of a Philox call cost no vector instruction)
__device__ __forceinline__ unsigned long long rng_uniform64(unsigned long long v) {
    const uint32_t lo = __builtin_amdgcn_readfirstlane(uint32_t(v)), hi = __builtin_amdgcn_readfirstlane(uint32_t(v >> 32));
    return (static_cast<unsigned long long>(hi) << 32) | lo;
}

// 3. the last of its group resets the group's ticket and takes the top one; the last group (every workgroup of the launch has
//    read `draws` by then) resets that and stores draws + 1.  wg / wgs: this workgroup's linear index / the launch's workgroups
__device__ __forceinline__ void rng_last_arriver_advances(unsigned long long* state, int* tickets, int* mine, int order, int grp, int groups,
                                                          int group, int wgs, unsigned long long base) {
    const int in_group = grp == groups - 1 ? wgs - grp * group : group;
    if (order == in_group - 1) {                               // last of its group: every workgroup of the group has read `draws`
        __hip_atomic_store(mine, 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        int* const top = tickets;
        if (__hip_atomic_fetch_add(top, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == groups - 1) {     // last group: so has every workgroup
            __hip_atomic_store(top, 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            __hip_atomic_store(state + 1, base + 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
    }
}

// workgroups per first-level ticket: the power of two g with g * g >= workgroups (and (g / 2)^2 < workgroups)
inline int rng_group(unsigned blocks) {
    int g = 1;
    while (int64_t(g) * g < int64_t(blocks)) g *= 2;
    return g;
}

// T and s as the stream's definition gives them: both computed in double on the host, s rounded to float32 once
inline void rng_threshold(double p, uint32_t& threshold, float& s) {
    const double t = p * 4294967296.0;
    threshold = t >= 4294967295.0 ? 4294967295u : uint32_t(t);
    s = float(1.0 / (1.0 - p));
}

// ---- the stream's words for elements that are not one aligned group of four (the attention kernels) ----------------------------
// words of elements i .. i + 3 of the call, i any 64-bit element index: one Philox call when i % 4 == 0 (ALIGNED: known), two
// when the four straddle two groups.  Selections only, no indexed array: nothing goes to scratch.
template <bool ALIGNED>
__device__ __forceinline__ void rng_words4(int64_t i, unsigned long long seed, unsigned long long base, uint32_t (&w)[4]) {
    const uint64_t grp = uint64_t(i) >> 2;
    philox4x32_10(uint32_t(grp), uint32_t(grp >> 32), uint32_t(base), uint32_t(base >> 32), uint32_t(seed), uint32_t(seed >> 32), w);
    if constexpr (!ALIGNED) {
        const int o = int(i & 3);
        if (o != 0) {
            uint32_t n[4];
            philox4x32_10(uint32_t(grp + 1), uint32_t((grp + 1) >> 32), uint32_t(base), uint32_t(base >> 32), uint32_t(seed), uint32_t(seed >> 32), n);
            const uint32_t a0 = w[0], a1 = w[1], a2 = w[2], a3 = w[3];
            (void)a0;
            w[0] = o == 1 ? a1 : o == 2 ? a2 : a3;
            w[1] = o == 1 ? a2 : o == 2 ? a3 : n[0];
            w[2] = o == 1 ? a3 : o == 2 ? n[0] : n[1];
            w[3] = o == 1 ? n[0] : o == 2 ? n[1] : n[2];
        }
    }
}

// the word of the single element i
__device__ __forceinline__ uint32_t rng_word(int64_t i, unsigned long long seed, unsigned long long base) {
    uint32_t w[4];
    const uint64_t grp = uint64_t(i) >> 2;
    philox4x32_10(uint32_t(grp), uint32_t(grp >> 32), uint32_t(base), uint32_t(base >> 32), uint32_t(seed), uint32_t(seed >> 32), w);
    const int o = int(i & 3);
    return o == 0 ? w[0] : o == 1 ? w[1] : o == 2 ? w[2] : w[3];
}

// x * s for a kept element, +0.0 for a dropped one (a select: a dropped NaN or infinity becomes +0.0 too)
__device__ __forceinline__ float rng_keep(float x, uint32_t word, uint32_t threshold, float s) {
    return word >= threshold ? __fmul_rn(x, s) : 0.0f;
}

// What the attention kernels get of a call.  Forward: `state` is Runtime::rng_state (read, ticket, advance) and `base` the word
// workgroup 0 writes; backward: `state` gives the seed, `base` is what the forward wrote, nothing is drawn.
struct AttnDrop {
    unsigned long long* state;
    unsigned long long* base;
    uint32_t threshold;
    float s;
    int group;                       // workgroups per first-level ticket (forward)
};

}  // namespace lg
