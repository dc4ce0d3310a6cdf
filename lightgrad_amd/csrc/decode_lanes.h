// The lane folds of the one-token decode kernels: included by decode.hip (attn_decode) and decode_split.hip (attn_decode_split),
// each under its own compile flags.  (rowwise.hip, reduce.hip and sample_body.h fold in other orders and keep their own helpers.)
#pragma once
#include <hip/hip_runtime.h>

namespace lg {

typedef float df32x4 __attribute__((ext_vector_type(4)));

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

}  // namespace lg
