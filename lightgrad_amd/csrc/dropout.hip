// Dropout for gfx950 from a counter-based random stream (C ABI and stream definition: include/lghip.h).
//
// Philox4x32-10 is arithmetic on the element index, the call number and the seed, so nothing is stored: one Philox call per
// lane yields the four words for one float4, the backward kernel makes the same words again, and the numpy backend
// (autograd/rng.py) makes them on the host - the two backends agree bit for bit.
//
// The generator's state (Runtime::rng_state) lives in device memory and is READ BY THE KERNEL, not baked into its arguments: a
// captured graph draws a new mask at every replay.  One launch both uses `draws` and advances it:
//   1. lane 0 of every workgroup reads `draws` (agent scope), waits for the value, and only then
//   2. takes a ticket.  The workgroup that arrives last resets the ticket and adds 1 to `draws`.
// The add therefore comes after the read of every workgroup; the next launch on the stream sees it.  Tickets have two levels
// (groups of consecutive workgroups, then one ticket for the groups), each on a 64-byte line of its own: atomics on one address
// are served one after the other, 13 ns each (csrc/reduce.hip), which a single ticket would turn into 3.4 ms for the 262144
// workgroups of 2^28 elements.  A group holds g workgroups, g the power of two with g * g >= workgroups: the longest chain is
// g + g adds (2^28 elements: 13 us, under the time the data takes), and no size takes another path.
#include "common.h"
#include "rng_common.h"

namespace lg {

// x * s for a kept element, +0.0 for a dropped one (a select: a dropped NaN or infinity becomes +0.0 too); with a residual the
// sum is a second rounding, and a dropped element is +0.0 + r like the numpy expression
template <bool RES>
__device__ __forceinline__ float drop_value(float x, float r, uint32_t word, uint32_t threshold, float s) {
    const float v = word >= threshold ? __fmul_rn(x, s) : 0.0f;
    return RES ? __fadd_rn(v, r) : v;
}

// Work item v covers elements 4v .. 4v+3: a float4 when all four exist and VEC (every pointer 16-byte aligned), else scalars.
template <bool RES, bool VEC>
__device__ __forceinline__ void drop_items(const float* x, const float* res, float* y, int64_t n, uint32_t threshold, float s,
                                           uint64_t seed, uint64_t base) {
    const int64_t items = (n + 3) / 4, v = int64_t(blockIdx.x) * blockDim.x + threadIdx.x;
    if (v < items) {
        uint32_t w[4];
        philox4x32_10(uint32_t(v), uint32_t(uint64_t(v) >> 32), uint32_t(base), uint32_t(base >> 32), uint32_t(seed),
                      uint32_t(seed >> 32), w);
        const int64_t e = v * 4;
        if (VEC && e + 4 <= n) {
            const float4 a = *reinterpret_cast<const float4*>(x + e);
            float4 r = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
            if (RES) r = *reinterpret_cast<const float4*>(res + e);
            *reinterpret_cast<float4*>(y + e) = make_float4(drop_value<RES>(a.x, r.x, w[0], threshold, s), drop_value<RES>(a.y, r.y, w[1], threshold, s),
                                                            drop_value<RES>(a.z, r.z, w[2], threshold, s), drop_value<RES>(a.w, r.w, w[3], threshold, s));
        } else {
            float a[4], r[4];
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                a[k] = e + k < n ? x[e + k] : 0.0f;
                r[k] = RES && e + k < n ? res[e + k] : 0.0f;
            }
#pragma unroll
            for (int k = 0; k < 4; ++k)
                if (e + k < n) y[e + k] = drop_value<RES>(a[k], r[k], w[k], threshold, s);
        }
    }
}

template <bool RES, bool VEC>
__global__ void __launch_bounds__(256) dropout_fwd(const float* x, const float* res, float* y, int64_t n, uint32_t threshold, float s,
                                                   unsigned long long* state, unsigned long long* base_out, int group) {
    __shared__ unsigned long long call[2];
    int* const tickets = rng_tickets(state);
    if (threadIdx.x == 0) {
        rng_read_call(state, call);                                // `draws` is in a register before the ticket below is taken
        if (blockIdx.x == 0) base_out[0] = call[1];
    }
    __syncthreads();
    int order = 0;
    const int grp = blockIdx.x / group, groups = (gridDim.x + group - 1) / group;
    int* const mine = tickets + (1 + grp) * kRngLine;
    if (threadIdx.x == 0) order = rng_take_ticket(mine);
    const unsigned long long seed = rng_uniform64(call[0]), base = rng_uniform64(call[1]);

    drop_items<RES, VEC>(x, res, y, n, threshold, s, seed, base);

    if (threadIdx.x == 0) rng_last_arriver_advances(state, tickets, mine, order, grp, groups, group, int(gridDim.x), base);
}

template <bool VEC>
__global__ void __launch_bounds__(256) dropout_bwd(const float* g, float* dx, int64_t n, uint32_t threshold, float s,
                                                   const unsigned long long* state, const unsigned long long* base) {
    drop_items<false, VEC>(g, nullptr, dx, n, threshold, s, state[0], base[0]);
}

__global__ void rng_seed_kernel(unsigned long long* state, unsigned long long seed) {
    state[0] = seed;
    state[1] = 0;
}

int rng_init() {
    Runtime& R = rt();
    LG_HIP(hipMalloc(reinterpret_cast<void**>(&R.rng_state), kRngStateBytes));
    LG_HIP(hipMemset(R.rng_state, 0, kRngStateBytes));           // synchronous: seed 0, draws 0, tickets at zero before any launch
    return LG_OK;
}

// one work item (four elements) per thread; an empty call still launches one workgroup, which advances `draws`
static unsigned rng_grid(int64_t n) {
    const int64_t need = ((n + 3) / 4 + 255) / 256;
    return unsigned(need < 1 ? 1 : need);
}

}  // namespace lg

using namespace lg;

extern "C" int lg_rng_seed(uint64_t seed) {
    LG_REQUIRE_INIT();
    LG_ARG(!capturing(), "lg_rng_seed: not allowed while capturing a graph (a replay reads the seed from device memory: seed between replays)");
    hipLaunchKernelGGL(rng_seed_kernel, dim3(1), dim3(1), 0, rt().stream, rt().rng_state, static_cast<unsigned long long>(seed));
    LG_CHECK_LAUNCH();
    return LG_OK;
}

extern "C" int lg_rng_state(uint64_t* seed, uint64_t* draws) {
    LG_REQUIRE_INIT();
    LG_ARG(seed != nullptr && draws != nullptr, "lg_rng_state: NULL pointer");
    LG_ARG(!capturing(), "lg_rng_state: not allowed while capturing a graph");
    unsigned long long host[2] = {0, 0};
    LG_HIP(hipMemcpyAsync(host, rt().rng_state, sizeof(host), hipMemcpyDeviceToHost, rt().stream));
    LG_HIP(hipStreamSynchronize(rt().stream));
    *seed = host[0];
    *draws = host[1];
    return LG_OK;
}

extern "C" int lg_dropout_fwd_f32(const float* x, const float* residual, float* y, int64_t n, double p, uint64_t* base_out) {
    LG_REQUIRE_INIT();
    LG_ARG(x != nullptr && y != nullptr && base_out != nullptr, "lg_dropout_fwd_f32: NULL pointer");
    LG_ARG(n >= 0 && n <= kRngMaxElements, "lg_dropout_fwd_f32: n = %lld outside [0, 2^34]", (long long)n);
    LG_ARG(p >= 0.0 && p < 1.0, "lg_dropout_fwd_f32: p = %g outside [0, 1)", p);
    { const int rc = adam_epilogue_check_write(y, n * 4); if (rc != LG_OK) return rc; }
    uint32_t threshold;
    float s;
    rng_threshold(p, threshold, s);
    const bool vec = aligned16(x) && aligned16(y) && (residual == nullptr || aligned16(residual));
    const dim3 grid(rng_grid(n)), block(256);
    unsigned long long* const state = rt().rng_state;
    unsigned long long* const out = reinterpret_cast<unsigned long long*>(base_out);
    hipStream_t st = rt().stream;
    const int group = rng_group(grid.x);
    if (residual != nullptr) {
        if (vec) hipLaunchKernelGGL((dropout_fwd<true, true>), grid, block, 0, st, x, residual, y, n, threshold, s, state, out, group);
        else hipLaunchKernelGGL((dropout_fwd<true, false>), grid, block, 0, st, x, residual, y, n, threshold, s, state, out, group);
    } else {
        if (vec) hipLaunchKernelGGL((dropout_fwd<false, true>), grid, block, 0, st, x, residual, y, n, threshold, s, state, out, group);
        else hipLaunchKernelGGL((dropout_fwd<false, false>), grid, block, 0, st, x, residual, y, n, threshold, s, state, out, group);
    }
    LG_CHECK_LAUNCH();
    return LG_OK;
}

extern "C" int lg_dropout_bwd_f32(const float* g, float* dx, int64_t n, double p, const uint64_t* base) {
    LG_REQUIRE_INIT();
    LG_ARG(g != nullptr && dx != nullptr && base != nullptr, "lg_dropout_bwd_f32: NULL pointer");
    LG_ARG(n >= 0 && n <= kRngMaxElements, "lg_dropout_bwd_f32: n = %lld outside [0, 2^34]", (long long)n);
    LG_ARG(p >= 0.0 && p < 1.0, "lg_dropout_bwd_f32: p = %g outside [0, 1)", p);
    if (n == 0) return LG_OK;
    { const int rc = adam_epilogue_check_write(dx, n * 4); if (rc != LG_OK) return rc; }
    uint32_t threshold;
    float s;
    rng_threshold(p, threshold, s);
    const dim3 grid(rng_grid(n)), block(256);
    const unsigned long long* const b = reinterpret_cast<const unsigned long long*>(base);
    if (aligned16(g) && aligned16(dx)) hipLaunchKernelGGL((dropout_bwd<true>), grid, block, 0, rt().stream, g, dx, n, threshold, s, rt().rng_state, b);
    else hipLaunchKernelGGL((dropout_bwd<false>), grid, block, 0, rt().stream, g, dx, n, threshold, s, rt().rng_state, b);
    LG_CHECK_LAUNCH();
    return LG_OK;
}
