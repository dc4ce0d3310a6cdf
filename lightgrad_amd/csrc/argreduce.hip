// fp32 argmax / argmin over one axis (or the whole flattened view) and top-1 counting for gfx950 (C ABI: include/lghip.h).
// The output is int64 and the semantics are numpy's, bit for bit: the lowest index among equal extrema, -0.0 == +0.0, and the
// index of the FIRST NaN when the reduced run holds one (argmax and argmin alike).
//
// THE COMBINE.  A candidate (v, i) beats (w, j) when
//   1. v is NaN and w is not, or
//   2. neither is NaN and v > w (v < w for argmin), or
//   3. neither 1 nor 2 holds in either direction and i < j.
// This is a total order on candidates with distinct indices, so every fold order - lanes, waves, workgroups, splits - gives the
// same answer: the result is deterministic without any fixed order (`beats` below is this text; nothing else compares
// candidates across threads).
//
// Inside ONE thread the elements are visited by increasing index, so the new candidate always carries the larger index and
// rule 3 never lets it win: the running update is rules 1 and 2 alone, `!(best >= x) && best == best`.  A thread starts from
// (identity, kNone) with kNone above every index.  An element EQUAL to the identity (-inf for argmax) does not replace that start,
// so a run left at kNone after the fold held nothing but the identity - all its elements are equal and the answer is the run's
// first index (`settle`).  This is the all -inf row that an accumulator with a sentinel index gets wrong.
//
// After collapsing, the problem is [outer][axis][inner] with one stride each:
//   arg_rows_wave   inner == 1, axis contiguous, many or short rows: one wave per row.  The row is walked with 16-byte loads from
//                   its first 16-byte aligned element on (rows of 30522 floats start aligned only every other time), eight loads
//                   in flight per lane and the next eight issued before the current are compared: one wave per SIMD has to keep
//                   the memory system busy by itself.  With COUNT the wave compares the index with the row's label instead of
//                   storing it (lg_top1_count_f32): ignored rows are not read, workgroups publish their integer counts and the last
//                   arriver folds them.
//   arg_rows_split  few long rows (axis = all of a big tensor): a row is split over many workgroups, each publishes one candidate,
//                   and the two-level fold of handoff.h (groups of 32 segments with a ticket each, then one ticket per row) folds
//                   them inside the launch.
//   arg_cols        the axis is strided: one thread per output element, lanes along the output (coalesced when the kept axis is
//                   contiguous); a long axis is split over blockIdx.y with the same publish-and-fold, one ticket per 256 outputs.
// Views that do not collapse to one stride each are refused (LG_EINVAL); the tensor layer makes them dense first.
#include "common.h"
#include "handoff.h"
#include <cmath>
#include <climits>

namespace lg {

constexpr int64_t kNone = INT64_MAX;                    // the index of "no candidate yet"
typedef unsigned long long u64;

template <int OP> __device__ __forceinline__ float arg_identity() { return OP == LG_RED_MAX ? -INFINITY : INFINITY; }

// the combine: does (v, i) beat (w, j)?
template <int OP>
__device__ __forceinline__ bool beats(float v, int64_t i, float w, int64_t j) {
    const bool vn = v != v, wn = w != w;
    if (vn || wn) return vn && (!wn || i < j);
    const bool ahead = OP == LG_RED_MAX ? v > w : v < w, behind = OP == LG_RED_MAX ? w > v : w < v;
    return ahead || (!behind && i < j);
}

// a candidate as two 64-bit words (what workgroups hand to each other): {bits of the value, index}
struct Pair { u64 a, b; };

template <int OP> struct ArgFold {
    __device__ static Pair identity() { return Pair{u64(__float_as_uint(arg_identity<OP>())), u64(kNone)}; }
    __device__ static Pair comb(Pair x, Pair y) {
        return beats<OP>(__uint_as_float(uint32_t(x.a)), int64_t(x.b), __uint_as_float(uint32_t(y.a)), int64_t(y.b)) ? x : y;
    }
};
struct CountFold {                                      // {correct, counted}: integers, any order is exact
    __device__ static Pair identity() { return Pair{0, 0}; }
    __device__ static Pair comb(Pair x, Pair y) { return Pair{x.a + y.a, x.b + y.b}; }
};

template <class F>
__device__ __forceinline__ Pair wave_fold(Pair x) {     // butterfly: every lane ends with the wave's result
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        Pair y;
        y.a = __shfl_xor(x.a, off, 64);
        y.b = __shfl_xor(x.b, off, 64);
        x = F::comb(x, y);
    }
    return x;
}

using handoff::kFoldGroup;                              // workgroups that hold one Pair each fold them in two levels (handoff.h)

// ---- walking a contiguous run ------------------------------------------------------------------------------------------------

// the running update of one thread: `i` is larger than every index this thread has seen (rules 1 and 2 of the combine)
template <int OP>
__device__ __forceinline__ void absorb(float x, int64_t i, float& bv, int64_t& bi) {
    const bool take = (OP == LG_RED_MAX ? !(bv >= x) : !(bv <= x)) && bv == bv;
    bv = take ? x : bv;
    bi = take ? i : bi;
}
template <int OP>
__device__ __forceinline__ void absorb4(const float4& x, int64_t i, float& bv, int64_t& bi) {
    absorb<OP>(x.x, i, bv, bi); absorb<OP>(x.y, i + 1, bv, bi); absorb<OP>(x.z, i + 2, bv, bi); absorb<OP>(x.w, i + 3, bv, bi);
}

// elements [begin, end) of the run at `p`, shared by T threads (this one is `tid`), by increasing index in every thread: the
// elements in front of the first 16-byte aligned one, float4 loads, the rest.  T >= 4.
template <int OP, int T>
__device__ __forceinline__ void scan_run(const float* __restrict__ p, int64_t begin, int64_t end, int tid, float& bv, int64_t& bi) {
    constexpr int U = 8;                                 // 16-byte loads in flight per thread
    int64_t a = begin + ((4 - int64_t((reinterpret_cast<uintptr_t>(p + begin) >> 2) & 3)) & 3);
    if (a > end) a = end;
    if (begin + tid < a) absorb<OP>(p[begin + tid], begin + tid, bv, bi);
    const int64_t nv = (end - a) >> 2;
    const float4* p4 = reinterpret_cast<const float4*>(p + a);
    int64_t v = tid;
    if (v + int64_t(U - 1) * T < nv) {
        float4 x[U];
#pragma unroll
        for (int u = 0; u < U; ++u) x[u] = p4[v + u * T];
        for (;;) {
            const int64_t vn = v + int64_t(U) * T;
            const bool more = vn + int64_t(U - 1) * T < nv;
            float4 y[U];
            if (more) {
#pragma unroll
                for (int u = 0; u < U; ++u) y[u] = p4[vn + u * T];
            }
#pragma unroll
            for (int u = 0; u < U; ++u) absorb4<OP>(x[u], a + 4 * (v + u * T), bv, bi);
            v = vn;
            if (!more) break;
#pragma unroll
            for (int u = 0; u < U; ++u) x[u] = y[u];
        }
    }
    for (; v < nv; v += T) absorb4<OP>(p4[v], a + 4 * v, bv, bi);
    const int64_t t0 = a + 4 * nv;
    if (t0 + tid < end) absorb<OP>(p[t0 + tid], t0 + tid, bv, bi);
}

// a run that nothing but the identity was found in: every element equals it, the first one is the answer
__device__ __forceinline__ Pair settle(Pair c, int64_t first) {
    if (int64_t(c.b) == kNone) c.b = u64(first);
    return c;
}

__device__ __forceinline__ Pair as_pair(float v, int64_t i) { return Pair{u64(__float_as_uint(v)), u64(i)}; }

// ---- rows: one wave per row ------------------------------------------------------------------------------------------------------
struct CountArgs {
    const void* labels;
    int64_t     ignore;
    int         has_ignore, accumulate;
    int64_t*    counts;                                  // {correct, counted}
    Pair*       slots;                                   // gridDim.x + groups
    int*        tickets;
    int64_t     tstride;
    int*        status;
};

constexpr int kRowsWaveMaxBlocks = 1 << 20;              // beyond: the waves stride over the rows

template <int OP, bool COUNT, typename LabelT>
__global__ void __launch_bounds__(256) arg_rows_wave(const float* __restrict__ in, int64_t* __restrict__ out, int64_t n_rows, int64_t rlen,
                                                     int64_t row_stride, CountArgs c) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    u64 correct = 0, counted = 0;
    for (int64_t row = int64_t(blockIdx.x) * 4 + wave; row < n_rows; row += int64_t(gridDim.x) * 4) {
        int64_t label = 0;
        if constexpr (COUNT) {
            label = int64_t(static_cast<const LabelT*>(c.labels)[row]);
            if (c.has_ignore && label == c.ignore) continue;            // (the whole wave: nothing of the row is read)
            if (label < 0) label += rlen;
            if (label < 0 || label >= rlen) {                           // numpy raises IndexError; a kernel raises the status flag
                if (lane == 0) __hip_atomic_fetch_or(c.status, LG_STATUS_BAD_INDEX, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
                continue;
            }
        }
        float bv = arg_identity<OP>();
        int64_t bi = kNone;
        scan_run<OP, 64>(in + row * row_stride, 0, rlen, lane, bv, bi);
        const Pair best = settle(wave_fold<ArgFold<OP>>(as_pair(bv, bi)), 0);
        if constexpr (COUNT) {
            counted += 1;
            correct += int64_t(best.b) == label ? 1 : 0;
        } else {
            if (lane == 0) out[row] = int64_t(best.b);
        }
    }
    if constexpr (COUNT) {
        __shared__ u64 wc[4][2];
        __shared__ int last[2];
        if (lane == 0) { wc[wave][0] = correct; wc[wave][1] = counted; }
        __syncthreads();
        Pair total{wc[0][0] + wc[1][0] + wc[2][0] + wc[3][0], wc[0][1] + wc[1][1] + wc[2][1] + wc[3][1]};
        if (gridDim.x > 1 && !handoff::fold_two_level<CountFold, u64>(total, c.slots, c.slots + gridDim.x, c.tickets, c.tstride, blockIdx.x,
                                                                      gridDim.x, last, wave_fold<CountFold>))
            return;
        if (threadIdx.x == 0) {
            c.counts[0] = int64_t(total.a) + (c.accumulate ? c.counts[0] : 0);
            c.counts[1] = int64_t(total.b) + (c.accumulate ? c.counts[1] : 0);
        }
    }
}

// ---- rows split over workgroups: grid = (splits, rows), a workgroup per segment of `seg` elements ------------------------------------
template <int OP>
__global__ void __launch_bounds__(256) arg_rows_split(const float* __restrict__ in, int64_t* __restrict__ out, Pair* slots, int* tickets,
                                                      int64_t rlen, int64_t row_stride, int64_t seg, int64_t tstride) {
    __shared__ Pair wbest[4];
    __shared__ int last[2];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int64_t row = blockIdx.y, split = blockIdx.x, splits = gridDim.x;
    const int64_t begin = split * seg;
    int64_t end = begin + seg;
    if (end > rlen) end = rlen;
    float bv = arg_identity<OP>();
    int64_t bi = kNone;
    scan_run<OP, 256>(in + row * row_stride, begin, end, threadIdx.x, bv, bi);
    const Pair w = wave_fold<ArgFold<OP>>(as_pair(bv, bi));
    if (lane == 0) wbest[wave] = w;
    __syncthreads();
    Pair best = settle(ArgFold<OP>::comb(ArgFold<OP>::comb(wbest[0], wbest[1]), ArgFold<OP>::comb(wbest[2], wbest[3])), begin);
    if (splits > 1) {
        const int64_t groups = (splits + kFoldGroup - 1) / kFoldGroup;
        Pair* const mine = slots + row * (splits + groups);                      // [row]: splits, then groups
        if (!handoff::fold_two_level<ArgFold<OP>, u64>(best, mine, mine + splits, tickets + row * (groups + 1) * tstride, tstride, split, splits,
                                                       last, wave_fold<ArgFold<OP>>))
            return;
    }
    if (threadIdx.x == 0) out[row] = int64_t(best.b);
}

// ---- columns: one thread per output element, the axis strided --------------------------------------------------------------------
// output o = oo * n_inner + ii reads in[oo * so + ii * si + r * sa], r in [0, rlen); gridDim.y > 1 splits r into chunks
template <int OP>
__global__ void __launch_bounds__(256) arg_cols(const float* __restrict__ in, int64_t* __restrict__ out, Pair* slots, int* tickets,
                                                int64_t n_out, int64_t n_inner, int64_t so, int64_t si, int64_t sa, int64_t rlen, int64_t chunk) {
    const int64_t o_raw = int64_t(blockIdx.x) * 256 + threadIdx.x;
    const bool live = o_raw < n_out;
    const int64_t o = live ? o_raw : n_out - 1;          // idle lanes of the last block recompute a valid output
    const int64_t split = blockIdx.y, begin = split * chunk;
    int64_t end = begin + chunk;
    if (end > rlen) end = rlen;
    const float* p = in + (o / n_inner) * so + (o % n_inner) * si;
    float bv = arg_identity<OP>();
    int64_t bi = kNone;
    int64_t r = begin;
    for (; r + 3 < end; r += 4) {
        const float x0 = p[r * sa], x1 = p[(r + 1) * sa], x2 = p[(r + 2) * sa], x3 = p[(r + 3) * sa];
        absorb<OP>(x0, r, bv, bi); absorb<OP>(x1, r + 1, bv, bi); absorb<OP>(x2, r + 2, bv, bi); absorb<OP>(x3, r + 3, bv, bi);
    }
    for (; r < end; ++r) absorb<OP>(p[r * sa], r, bv, bi);
    Pair best = settle(as_pair(bv, bi), begin);
    const int splits = gridDim.y;
    if (splits > 1) {
        __shared__ int arrived_last;
        handoff::publish<u64>(slots + split * n_out + o, best);
        if (!handoff::arrive_workgroup(tickets + blockIdx.x, splits, &arrived_last)) return;
        best = ArgFold<OP>::identity();
        int s = 0;
        for (; s + 3 < splits; s += 4) {                 // four candidates in flight: their loads cross XCDs
            Pair x[4];
#pragma unroll
            for (int e = 0; e < 4; ++e) x[e] = handoff::fetch<Pair, u64>(slots + int64_t(s + e) * n_out + o);
#pragma unroll
            for (int e = 0; e < 4; ++e) best = ArgFold<OP>::comb(best, x[e]);
        }
        for (; s < splits; ++s) best = ArgFold<OP>::comb(best, handoff::fetch<Pair, u64>(slots + int64_t(s) * n_out + o));
    }
    if (live) out[o] = int64_t(best.b);
}

// ---- host --------------------------------------------------------------------------------------------------------------------------
enum { ARG_NONE = -1, ARG_ROWS_WAVE = 0, ARG_ROWS_SPLIT = 1, ARG_COLS = 2 };
static thread_local int32_t g_arg_plan[4] = {ARG_NONE, 0, 0, 0};

static void note_arg_plan(int kernel, int64_t splits, int merged, int vec) {
    g_arg_plan[0] = kernel; g_arg_plan[1] = int32_t(splits); g_arg_plan[2] = merged; g_arg_plan[3] = vec;
}

// merge neighbouring dimensions that one stride walks; returns how many are left (0: a single element)
static int merge_dims(int n, int64_t* shp, int64_t* st) {
    int m = 0;
    for (int d = 0; d < n; ++d) {
        if (shp[d] == 1) continue;
        if (m > 0 && st[m - 1] == st[d] * shp[d]) {
            shp[m - 1] *= shp[d];
            st[m - 1] = st[d];
        } else {
            shp[m] = shp[d];
            st[m] = st[d];
            ++m;
        }
    }
    return m;
}

// does a run of `n` floats at `p` hold a 16-byte aligned float4?
static bool run_has_vector(const float* p, int64_t n) {
    const int64_t head = (4 - int64_t((reinterpret_cast<uintptr_t>(p) >> 2) & 3)) & 3;
    return n - head >= 4;
}

template <int OP>
static int run_argreduce(const float* in, int64_t* out, int64_t n_outer, int64_t so, int64_t rlen, int64_t sa, int64_t n_inner, int64_t si) {
    hipStream_t s = rt().stream;
    const int64_t n_out = n_outer * n_inner;
    const CountArgs none{};
    // a contiguous axis with nothing in front of it (axis 0 of a transposed matrix): the dimension behind it numbers the rows
    if (n_outer == 1 && sa == 1) { n_outer = n_inner; so = si; n_inner = 1; si = 0; }
    if (n_inner == 1 && sa == 1 && rlen > 1) {
        const auto wave_per_row = [&]() {
            int64_t blocks = (n_out + 3) / 4;
            if (blocks > kRowsWaveMaxBlocks) blocks = kRowsWaveMaxBlocks;
            note_arg_plan(ARG_ROWS_WAVE, 1, 1, run_has_vector(in, rlen));
            hipLaunchKernelGGL((arg_rows_wave<OP, false, int32_t>), dim3(unsigned(blocks)), dim3(256), 0, s, in, out, n_out, rlen, so, none);
            return LG_OK;
        };
        // many rows, or short rows: a wave per row (the thresholds of reduce.hip: the same reads, the same trade)
        if (n_out >= 256 || rlen <= 8192) return wave_per_row();
        // few long rows: enough segments to fill the chip, at least 16 KiB each
        int64_t splits = (768 + n_out - 1) / n_out;
        const int64_t min_seg = 4096;
        if (splits * min_seg > rlen) splits = (rlen + min_seg - 1) / min_seg;
        const int64_t seg = ((rlen + splits - 1) / splits + 3) & ~int64_t(3);
        splits = (rlen + seg - 1) / seg;
        const int64_t groups = (splits + kFoldGroup - 1) / kFoldGroup, n_tickets = n_out * (groups + 1);
        if (splits == 1) {
            note_arg_plan(ARG_ROWS_SPLIT, 1, 1, run_has_vector(in, rlen));
            hipLaunchKernelGGL((arg_rows_split<OP>), dim3(1, unsigned(n_out)), dim3(256), 0, s, in, out, nullptr, nullptr, rlen, so, seg, int64_t(1));
            return LG_OK;
        }
        if (n_tickets > rt().n_tickets) return wave_per_row();     // (fewer than 256 rows, a few dozen groups: the pool is far larger)
        Pair* slots = nullptr;
        const int rc = lg_malloc(reinterpret_cast<void**>(&slots), size_t(n_out * (splits + groups)) * sizeof(Pair));
        if (rc != LG_OK) return rc;
        note_arg_plan(ARG_ROWS_SPLIT, splits, 1, run_has_vector(in, seg));
        hipLaunchKernelGGL((arg_rows_split<OP>), dim3(unsigned(splits), unsigned(n_out)), dim3(256), 0, s, in, out, slots, rt().tickets,
                           rlen, so, seg, int64_t(ticket_stride(n_tickets)));
        return lg_free(slots);                           // stream-ordered: the block is only reused by later launches
    }

    // the axis is strided.  Outer and inner become ONE output dimension when one stride walks both.
    int merged = 0;
    if (n_outer == 1) { merged = 1; }
    else if (n_inner == 1) { merged = 1; n_inner = n_outer; si = so; }
    else if (so == n_inner * si) { merged = 1; n_inner = n_out; }
    if (merged) so = 0;                                  // o / n_inner is then 0 for every output
    const int64_t blocks_x = (n_out + 255) / 256;
    if (blocks_x >= (int64_t(1) << 31)) { set_error("lg_argreduce_f32: output too large"); return LG_EINVAL; }
    // few output blocks and a long axis: split the axis (red_cols' numbers: 1536 workgroups, at least 16 elements per thread, and
    // no more candidates than the last workgroup folds quickly)
    int64_t splits = 1;
    if (blocks_x < 1536 && rlen >= 64) {
        splits = 1536 / blocks_x;
        if (splits * 16 > rlen) splits = rlen / 16;
        const int64_t cap = rlen >= 8192 ? 64 : 32;
        if (splits > cap) splits = cap;
        if (splits < 1) splits = 1;
    }
    int64_t chunk = (rlen + splits - 1) / splits;
    splits = (rlen + chunk - 1) / chunk;
    if (splits > 1 && blocks_x > rt().n_tickets) { splits = 1; chunk = rlen; }
    Pair* slots = nullptr;
    if (splits > 1) {
        const int rc = lg_malloc(reinterpret_cast<void**>(&slots), size_t(n_out * splits) * sizeof(Pair));
        if (rc != LG_OK) return rc;
    }
    note_arg_plan(ARG_COLS, splits, merged, 0);
    hipLaunchKernelGGL((arg_cols<OP>), dim3(unsigned(blocks_x), unsigned(splits)), dim3(256), 0, s, in, out, slots, rt().tickets, n_out,
                       n_inner, so, si, sa, rlen, chunk);
    return splits > 1 ? lg_free(slots) : LG_OK;
}

template <typename LabelT>
static void launch_top1(const float* logits, int64_t rows, int64_t cols, unsigned blocks, const CountArgs& c) {
    hipLaunchKernelGGL((arg_rows_wave<LG_RED_MAX, true, LabelT>), dim3(blocks), dim3(256), 0, rt().stream, logits, static_cast<int64_t*>(nullptr),
                       rows, cols, cols, c);
}

}  // namespace lg

using namespace lg;

extern "C" int lg_argreduce_f32(int op, int ndim, const int64_t* shape, const float* in, const int64_t* in_strides, int axis, int64_t* out) {
    LG_REQUIRE_INIT();
    note_arg_plan(ARG_NONE, 0, 0, 0);                    // until a kernel is launched: refused calls, no output elements
    LG_ARG(op == LG_RED_MAX || op == LG_RED_MIN, "lg_argreduce_f32: op %d is neither LG_RED_MAX nor LG_RED_MIN", op);
    LG_ARG(ndim >= 0 && ndim <= LG_MAX_DIMS, "lg_argreduce_f32: ndim %d out of range [0, %d]", ndim, LG_MAX_DIMS);
    LG_ARG(ndim == 0 || (shape != nullptr && in_strides != nullptr), "lg_argreduce_f32: NULL shape/strides");
    LG_ARG(axis == -1 || (axis >= 0 && axis < ndim), "lg_argreduce_f32: axis %d of %d dimensions (-1: all, flattened)", axis, ndim);
    int64_t oshape[LG_MAX_DIMS], ostride[LG_MAX_DIMS], ishape[LG_MAX_DIMS], istride[LG_MAX_DIMS], ashape[LG_MAX_DIMS], astride[LG_MAX_DIMS];
    int no = 0, ni = 0, na = 0;
    int64_t n_outer = 1, n_inner = 1, rlen = 1;
    for (int k = 0; k < ndim; ++k) {
        LG_ARG(shape[k] >= 0, "lg_argreduce_f32: negative extent");
        if (axis == -1 || k == axis) { ashape[na] = shape[k]; astride[na] = in_strides[k]; ++na; rlen *= shape[k]; }
        else if (k < axis)           { oshape[no] = shape[k]; ostride[no] = in_strides[k]; ++no; n_outer *= shape[k]; }
        else                         { ishape[ni] = shape[k]; istride[ni] = in_strides[k]; ++ni; n_inner *= shape[k]; }
    }
    LG_ARG(rlen > 0, "lg_argreduce_f32: attempt to get the arg%s of an empty sequence", op == LG_RED_MAX ? "max" : "min");
    if (n_outer * n_inner == 0) return LG_OK;
    LG_ARG(in != nullptr && out != nullptr, "lg_argreduce_f32: NULL pointer");
    no = merge_dims(no, oshape, ostride);
    ni = merge_dims(ni, ishape, istride);
    na = merge_dims(na, ashape, astride);
    LG_ARG(no <= 1 && ni <= 1 && na <= 1, "lg_argreduce_f32: the view does not collapse to one stride each for outer / axis / inner "
           "(%d / %d / %d dimensions left): make it dense first", no, na, ni);
    { const int rc = adam_epilogue_check_write(out, n_outer * n_inner * int64_t(sizeof(int64_t))); if (rc != LG_OK) return rc; }
    const int64_t so = no ? ostride[0] : 0, si = ni ? istride[0] : 0, sa = na ? astride[0] : 0;
    const int rc = op == LG_RED_MAX ? run_argreduce<LG_RED_MAX>(in, out, n_outer, so, rlen, sa, n_inner, si)
                                    : run_argreduce<LG_RED_MIN>(in, out, n_outer, so, rlen, sa, n_inner, si);
    if (rc != LG_OK) return rc;
    LG_CHECK_LAUNCH();
    return LG_OK;
}

extern "C" int lg_argreduce_last_plan(int32_t out[4]) {
    LG_ARG(out != nullptr, "lg_argreduce_last_plan: NULL pointer");
    for (int k = 0; k < 4; ++k) out[k] = g_arg_plan[k];
    return LG_OK;
}

extern "C" int lg_top1_count_f32(const float* logits, int64_t rows, int64_t cols, const void* labels, int label_itemsize, int has_ignore,
                                 int64_t ignore_index, int accumulate, int64_t* counts) {
    LG_REQUIRE_INIT();
    LG_ARG(label_itemsize == 2 || label_itemsize == 4 || label_itemsize == 8, "lg_top1_count_f32: labels must be int16/int32/int64");
    LG_ARG(rows >= 0 && cols >= 0, "lg_top1_count_f32: negative extent");
    LG_ARG(rows == 0 || cols > 0, "lg_top1_count_f32: attempt to get the argmax of an empty sequence");
    LG_ARG(counts != nullptr && (rows == 0 || (logits != nullptr && labels != nullptr)), "lg_top1_count_f32: NULL pointer");
    { const int rc = adam_epilogue_check_write(counts, 2 * int64_t(sizeof(int64_t))); if (rc != LG_OK) return rc; }
    // one workgroup per four rows up to a grid whose fold stays inside the ticket pool; beyond, the waves stride over the rows.
    // No rows: one workgroup, which writes {0, 0} (or adds nothing).
    int64_t blocks = (rows + 3) / 4;
    if (blocks < 1) blocks = 1;
    if (blocks > 8192) blocks = 8192;
    const int64_t groups = (blocks + kFoldGroup - 1) / kFoldGroup;
    CountArgs c{};
    c.labels = labels; c.ignore = ignore_index; c.has_ignore = has_ignore ? 1 : 0; c.accumulate = accumulate ? 1 : 0;
    c.counts = counts; c.tickets = rt().tickets; c.tstride = ticket_stride(groups + 1); c.status = rt().status_dev;
    LG_ARG(groups + 1 <= rt().n_tickets, "lg_top1_count_f32: the ticket pool holds %d counters, %lld are needed", rt().n_tickets,
           (long long)(groups + 1));
    if (blocks > 1) {
        const int rc = lg_malloc(reinterpret_cast<void**>(&c.slots), size_t(blocks + groups) * sizeof(Pair));
        if (rc != LG_OK) return rc;
    }
    if (label_itemsize == 2)      launch_top1<int16_t>(logits, rows, cols, unsigned(blocks), c);
    else if (label_itemsize == 4) launch_top1<int32_t>(logits, rows, cols, unsigned(blocks), c);
    else                          launch_top1<int64_t>(logits, rows, cols, unsigned(blocks), c);
    if (blocks > 1) { const int rc = lg_free(c.slots); if (rc != LG_OK) return rc; }
    LG_CHECK_LAUNCH();
    return LG_OK;
}
