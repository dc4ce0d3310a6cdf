// The cross-workgroup hand-off of every kernel that splits a reduction over workgroups and folds it inside the same launch
// (the write-through form of the in-launch split-K recipe, cdna_hip_programming.md § split-K item 2, Guideline 16 R1).
//
// THE PROTOCOL.  Each workgroup publishes its partial, arrives at a ticket that `expected` workgroups take, and the one that
// draws the last ticket reads every partial and folds them in an order that does not depend on who it is.  Nobody waits.
//
//   1. Published means: stored by publish() below (or a relaxed agent-scope __hip_atomic_store of at most 8 bytes).  These
//      stores write through to memory; a plain store does not count, whatever drains behind it.
//   2. EVERY wave that published drains its own stores (s_waitcnt vmcnt(0)) before the ticket is taken.  Where several waves
//      published, they meet at the workgroup's barrier after their drains and before the one lane that takes the ticket
//      (arrive_workgroup).  A drain in the ticket lane alone leaves the other waves' stores in flight (Pitfall 14).
//   3. The ticket is a relaxed agent-scope fetch_add.  The last arriver stores zero into it: EVERY TICKET IS ZERO AGAIN WHEN
//      THE LAUNCH ENDS.  All users share one pool (Runtime::tickets, below), so a ticket left non-zero corrupts the next,
//      unrelated kernel, not the one that left it.
//   4. The last arriver reads the partials with fetch() (relaxed agent-scope atomic loads) ONLY.  They pass the caches of its
//      CU, which may hold stale copies of those lines; that is why the acquire behind the ticket is
//      fence(acquire, "wavefront"), which emits no instruction and only keeps the compiler from moving the loads above the
//      ticket.  One plain load of a partial breaks this silently.
//   5. One ticket per 64-byte line while the pool allows (ticket_stride): atomics on one line are served one after the other.
//   6. One ticket serves a few dozen arrivals.  An arrival costs 13 ns because atomics on one address serialise (768
//      workgroups on one ticket: a 64 MiB sum goes from 14.2 to 23.9 us, profiles/r4/hbm_sum_single_ticket.txt), so hundreds
//      of workgroups that finish together fold in two levels (fold_two_level): groups of kFoldGroup with a ticket each, then
//      one ticket for the groups.
//
// Nothing here declares LDS: the caller owns the words that broadcast "this workgroup is last" and passes them in.
#pragma once
#include "common.h"

namespace lg {
namespace handoff {

// ---- the payload: word-wise, T is any struct of words of type W (float, {u64, u64}, {float, float, float}) ---------------------
template <typename W, typename T> struct Words { W w[sizeof(T) / sizeof(W)]; };

template <typename W, typename S, typename T>
__device__ __forceinline__ void publish(S* slot, const T& x) {           // the first sizeof(T) bytes of *slot
    static_assert(sizeof(T) % sizeof(W) == 0 && sizeof(T) <= sizeof(S) && sizeof(W) <= 8, "a payload of whole words inside its slot");
    const Words<W, T> s = __builtin_bit_cast(Words<W, T>, x);
    W* p = reinterpret_cast<W*>(slot);
#pragma unroll
    for (unsigned k = 0; k < sizeof(T) / sizeof(W); ++k) __hip_atomic_store(p + k, s.w[k], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

template <typename T, typename W = T, typename S>
__device__ __forceinline__ T fetch(const S* slot) {
    static_assert(sizeof(T) % sizeof(W) == 0 && sizeof(T) <= sizeof(S) && sizeof(W) <= 8, "a payload of whole words inside its slot");
    Words<W, T> s;
    const W* p = reinterpret_cast<const W*>(slot);
#pragma unroll
    for (unsigned k = 0; k < sizeof(T) / sizeof(W); ++k) s.w[k] = __hip_atomic_load(p + k, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    return __builtin_bit_cast(T, s);
}

// ---- arrivals ----------------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ bool take_ticket(int* ticket, int expected) {  // true for the last of `expected`, who leaves zero behind
    const bool last = __hip_atomic_fetch_add(ticket, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == expected - 1;
    if (last) __hip_atomic_store(ticket, 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    return last;
}

// ONE lane, which published everything its workgroup hands over: drain, take the ticket
__device__ __forceinline__ bool arrive(int* ticket, int expected) {
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    return take_ticket(ticket, expected);
}

// every thread after a barrier behind the write of *lds_last: was this workgroup last?  The last one may fetch() from here on.
__device__ __forceinline__ bool told_last(const int* lds_last) {
    __syncthreads();
    const bool last = *lds_last != 0;
    if (last) __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    return last;
}

// a whole workgroup of which thread 0 alone published: true in every thread of the last arriver
__device__ __forceinline__ bool arrive_thread0(int* ticket, int expected, int* lds_last) {
    if (threadIdx.x == 0) *lds_last = arrive(ticket, expected);
    return told_last(lds_last);
}

// a whole workgroup of which any thread may have published: true in every thread of the last arriver
__device__ __forceinline__ bool arrive_workgroup(int* ticket, int expected, int* lds_last) {
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    if (threadIdx.x == 0) *lds_last = take_ticket(ticket, expected);
    return told_last(lds_last);
}

// ---- two levels, for `n` workgroups of 256 threads that finish together and hold one T each ------------------------------------------
// This workgroup is number `idx` and has its T in `mine` (thread 0).  Level 1: groups of kFoldGroup consecutive slots, ticket
// `tickets[g * tstride]` for group g; a group's last arriver folds it - one slot per lane of wave 0, then `wave_tree`.  Level 2:
// ticket `tickets[groups * tstride]`; the last of the groups' folders folds slots2 lane-strided in ascending order, then `wave_tree`.
// Fixed trees at both levels: the same bits whoever folds.  True in wave 0 of the ONE workgroup that arrived last of all, with the
// total in `mine` (where wave_tree leaves it: lane 0 at least).  slots: n, slots2: ceil(n / kFoldGroup); lds_last: two words, one
// per level (slower waves still read the first when wave 0 writes the second).
constexpr int kFoldGroup = 32;                       // <= 64: one wave folds a group

template <class F, typename W, typename T, class WaveTree>
__device__ __forceinline__ bool fold_two_level(T& mine, T* slots, T* slots2, int* tickets, int64_t tstride, int64_t idx, int64_t n,
                                               int* lds_last, WaveTree&& wave_tree) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int64_t groups = (n + kFoldGroup - 1) / kFoldGroup, grp = idx / kFoldGroup;
    const int64_t in_group = (grp == groups - 1) ? n - grp * kFoldGroup : kFoldGroup;
    if (threadIdx.x == 0) publish<W>(slots + idx, mine);
    if (!arrive_thread0(tickets + grp * tstride, int(in_group), lds_last)) return false;
    if (wave == 0) {
        const T g = wave_tree(lane < in_group ? fetch<T, W>(slots + grp * kFoldGroup + lane) : F::identity());
        if (lane == 0) {
            publish<W>(slots2 + grp, g);
            lds_last[1] = arrive(tickets + groups * tstride, int(groups));
        }
    }
    if (!told_last(lds_last + 1) || wave != 0) return false;
    T f = F::identity();
    for (int64_t r = lane; r < groups; r += 64) f = F::comb(f, fetch<T, W>(slots2 + r));
    mine = wave_tree(f);
    return true;
}

}  // namespace handoff

// ---- the ticket pool on the host: Runtime::tickets, n_tickets ints, all zero between launches ------------------------------------
// Every launch goes to one stream, so two launches never count at the same time; tickets must be disjoint only INSIDE a launch.

// ints between two tickets of a launch that needs `needed` of them: a 64-byte line each while the pool allows (invariant 5)
inline int ticket_stride(int64_t needed) {
    const int64_t t = rt().n_tickets / needed;
    return int(t > 32 ? 32 : t);
}

// [0, tickets_group_end()): where the products queued into the gradient-group launch (lg_gemm_group_*) count, from index 0 like
// every launch that is alone on the stream.  It ends where the tail jobs begin because both are in flight in that one launch.
inline int tickets_group_end() { return rt().n_tickets / 2; }

// [tail, tail + tickets_tail_count()): the jobs queued into that same launch behind the products - LayerNorm parameter gradients,
// the scatter tail (tail_jobs.h) - so that they never share a ticket with a product's K-slices.
inline int* tickets_tail() { return rt().tickets + rt().n_tickets / 2; }
inline int tickets_tail_count() { return rt().n_tickets / 2 - 1; }

// the loss kernel's word (cross_entropy with the mean inside the launch): the last one, which no other user counts up to, so the
// loss launch needs no share of anybody's region.
inline int* ticket_of_loss() { return rt().tickets + rt().n_tickets - 1; }

}  // namespace lg
