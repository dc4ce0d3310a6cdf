// The wave-level tiles of the kernels that keep S^T = K Q^T in an accumulator and feed it to the next product from registers:
// included by attention_stream.hip (forward and both backward roles) and extend_split.hip.  The orientation is described at the
// head of attention_stream.hip: v_mfma_f32_32x32x2f32 leaves lane (r, h) = (lane & 31, lane >> 5) with rows acc_row(e, h) of
// column r, and mfma_lds.h feeds the B operand in exactly that k-order, so element e of a 32 x 32 tile in an accumulator IS the B
// operand of MFMA e of the next product over its rows.
#pragma once
#include "mfma_lds.h"

namespace lg {

// the fragment of row `row` that lane half h feeds a product over d: x[4 g + i] = row[8 g + 4 h + i]; NULL: a row past the
// sequence, zeros
template <int D>
__device__ __forceinline__ void frag_load(float (&x)[D / 2], const float* row, int h) {
#pragma unroll
    for (int g = 0; g < D / 8; ++g) {
        const af32x4 t = row ? *reinterpret_cast<const af32x4*>(row + 8 * g + 4 * h) : af32x4{0.f, 0.f, 0.f, 0.f};
        x[4 * g] = t[0]; x[4 * g + 1] = t[1]; x[4 * g + 2] = t[2]; x[4 * g + 3] = t[3];
    }
}

// acc (32 x 32) = L F^T: rows [row0, row0 + 32) of an LDS chunk (K-contiguous, pitch D + 4) against the register fragment
template <int D>
__device__ __forceinline__ af32x16 tile_product(const float* Ls, int row0, const float (&f)[D / 2], int r, int h) {
    af32x4 t[D / 8];
#pragma unroll
    for (int g = 0; g < D / 8; ++g) t[g] = *reinterpret_cast<const af32x4*>(Ls + (row0 + r) * (D + 4) + 8 * g + 4 * h);
    af32x16 acc = zero16();
#pragma unroll
    for (int g = 0; g < D / 8; ++g)
#pragma unroll
        for (int i = 0; i < 4; ++i) acc = __builtin_amdgcn_mfma_f32_32x32x2f32(t[g][i], f[4 * g + i], acc, 0, 0, 0);
    return acc;
}

// out[n] (32 d x 32) += L^T T: rows [row0, row0 + 32) of an LDS chunk read with d along the lanes, against the tile T that sits
// in an accumulator (element e is the B operand of MFMA e: see the head of the file)
template <int D>
__device__ __forceinline__ void tile_accumulate(af32x16 (&out)[D / 32], const float* Ls, int pitch, int row0, const af32x16& t, int r, int h) {
#pragma unroll
    for (int n = 0; n < D / 32; ++n) {
        float a[16];
#pragma unroll
        for (int e = 0; e < 16; ++e) a[e] = Ls[(row0 + acc_row(e, h)) * pitch + 32 * n + r];
#pragma unroll
        for (int e = 0; e < 16; ++e) out[n] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[e], t[e], out[n], 0, 0, 0);
    }
}

// the sum of both lane halves' x in a fixed order (half 0's first): the same bits in both lanes
__device__ __forceinline__ float halves_sum(float x, int h) {
    const float y = __shfl_xor(x, 32, 64);
    return h ? y + x : x + y;
}

// x^T (d x rows) of an accumulator pair -> row `dst` of a (rows, D) global operand, scaled: lane (r, h) holds d = 32 n +
// acc_row(e, h) of ITS row r, four consecutive d per e >> 2
template <int D>
__device__ __forceinline__ void store_transposed(float* dst, const af32x16 (&x)[D / 32], float s, int h) {
#pragma unroll
    for (int n = 0; n < D / 32; ++n)
#pragma unroll
        for (int g = 0; g < 4; ++g)
            *reinterpret_cast<af32x4*>(dst + 32 * n + 8 * g + 4 * h) =
                af32x4{x[n][4 * g] * s, x[n][4 * g + 1] * s, x[n][4 * g + 2] * s, x[n][4 * g + 3] * s};
}

}  // namespace lg
