// Matrix product of fp32 tensors on the bf16 matrix cores (gfx950): C (+)= r(op(A)) @ r(op(B)) [+ bias], r = round to bfloat16
// (nearest, ties to even), products exact, sums in fp32 (v_mfma_f32_32x32x16_bf16).  The C ABI is in include/lghip.h.
//
//   global --16-byte loads along the contiguous index--> registers --v_cvt_pk_bf16_f32--> LDS (bf16, two buffers) --> fragments --> MFMA
//
// One workgroup (4 waves as 2 x 2, 64 x 64 of C each = 2 x 2 MFMA tiles) owns a 128 x 128 tile of C and walks K in steps of 32.
// Both operands sit in LDS K-CONTIGUOUS, [row or column of C][k], 32 bf16 = 64 bytes of data per line on an 80-byte pitch: a
// fragment (lane (r, h) = (lane & 31, lane >> 5): line r, k = 8h .. 8h+7 of a 16-deep MFMA step) is one ds_read_b128, and the
// 16 lanes of one b128 group land on 16 different 16-byte slots (20 r mod 64 dwords: all distinct multiples of 4).
// Staging is in registers because the values are converted on the way (the LDS-DMA copies bytes).  Thread (p, q) =
// (tid / 8, tid % 8) holds a 4 x 4 block of the tile, four float4 along the operand's contiguous index:
//   k contiguous   (A[m*lda + k], B[n*ldb + k]): lines p, p+32, p+64, p+96, k = 4q .. 4q+3 - written as they come;
//   m/n contiguous (A[k*lda + m], B[k*ldb + n]): k = 4q .. 4q+3, lines 4p .. 4p+3          - transposed in the write pass
//     (a register renaming: line 4p+e takes element e of the four loads).
// Either way a write is 8 bytes (4 bf16) at [line][4q]: the 8 lanes of one p cover 16 consecutive dwords and the four p of a
// 32-lane group start 20 (or 80) dwords apart = 0 / 16 / 0 / 16 mod 32 banks after wrapping: two dwords per bank, the minimum.
// Edges: a float4 whose line or first k lies outside the operand is fetched from the operand's first element instead (no
// branch) and replaced by zeros; elements beyond K inside a float4 are zeroed; lines beyond M / N are never stored.  A float4
// that starts inside the last line may read up to 12 bytes behind the operand (see lghip.h, lg_gemm_f32).
//
// Few output tiles and a long K (an input gradient against a wide layer: 1024 x 128 with K = 30522): K is cut into equal
// chunks, one workgroup per (tile, chunk) writes its partial tile into a workspace and a second kernel adds the chunks in
// ascending order.  The cut depends on the shape alone, so results are the same bits from run to run; there are no atomics.
#include "common.h"

namespace lg {

namespace {

typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef float f32x4u __attribute__((ext_vector_type(4), aligned(4)));       // dword-aligned: column slices, odd leading dimensions
typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));

constexpr int BM = 128, BN = 128, BK = 32;
constexpr int PITCH = 40;                        // bf16 per LDS line: 32 of data + 8 of padding (80 bytes)
constexpr int TILE = 128 * PITCH;                // bf16 per staged operand tile

struct Bf16Args {
    const float* A; const float* B; float* C; const float* bias;
    int64_t M, N, K, lda, ldb, ldc;
    int64_t k_chunk;                             // k values per workgroup along K (a multiple of BK); blockIdx.y picks the chunk
    int64_t chunk_stride;                        // elements between the partial results of two chunks (0: one chunk, straight into C)
    int tiles_m;
    int accumulate;
};

__device__ __forceinline__ uint32_t pk_bf16(float lo, float hi) {
    uint32_t r;
    asm("v_cvt_pk_bf16_f32 %0, %1, %2" : "=v"(r) : "v"(lo), "v"(hi));
    return r;
}

// the 4 x 4 block of thread (p, q) of the tile whose first line is line0 and whose first k is k0; k ends at kend (exclusive)
template <bool KC>
__device__ __forceinline__ void load_tile(f32x4 (&v)[4], const float* __restrict__ X, int64_t ld, int64_t lines, int64_t line0,
                                          int64_t k0, int64_t kend, int p, int q) {
    if constexpr (KC) {
        const int64_t k = k0 + 4 * q;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int64_t line = line0 + p + 32 * i;
            const bool ok = line < lines && k < kend;
            const f32x4u t = *reinterpret_cast<const f32x4u*>(ok ? X + line * ld + k : X);
#pragma unroll
            for (int e = 0; e < 4; ++e) v[i][e] = (ok && k + e < kend) ? t[e] : 0.f;
        }
    } else {
        const int64_t line = line0 + 4 * p;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int64_t k = k0 + 4 * q + j;
            const bool ok = line < lines && k < kend;
            const f32x4u t = *reinterpret_cast<const f32x4u*>(ok ? X + k * ld + line : X);
#pragma unroll
            for (int e = 0; e < 4; ++e) v[j][e] = ok ? t[e] : 0.f;          // lines beyond the operand: values of C nobody stores
        }
    }
}

template <bool KC>
__device__ __forceinline__ void store_tile(const f32x4 (&v)[4], uint16_t* S, int p, int q) {
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        uint2 w;
        if constexpr (KC) {
            w.x = pk_bf16(v[i][0], v[i][1]); w.y = pk_bf16(v[i][2], v[i][3]);
            *reinterpret_cast<uint2*>(S + (p + 32 * i) * PITCH + 4 * q) = w;
        } else {
            w.x = pk_bf16(v[0][i], v[1][i]); w.y = pk_bf16(v[2][i], v[3][i]);
            *reinterpret_cast<uint2*>(S + (4 * p + i) * PITCH + 4 * q) = w;
        }
    }
}

template <bool AKC, bool BKC>
__global__ __launch_bounds__(256) void gemm_bf16_kernel(const Bf16Args a) {
    __shared__ __attribute__((aligned(16))) uint16_t lds[4 * TILE];           // [buffer][A | B][line][PITCH]
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int r = lane & 31, h = lane >> 5, wm = wave >> 1, wn = wave & 1;
    const int p = tid >> 3, q = tid & 7;
    const int64_t m0 = int64_t(blockIdx.x % unsigned(a.tiles_m)) * BM, n0 = int64_t(blockIdx.x / unsigned(a.tiles_m)) * BN;
    const int64_t kbeg = int64_t(blockIdx.y) * a.k_chunk;
    const int64_t kend = kbeg + a.k_chunk < a.K ? kbeg + a.k_chunk : a.K;
    const int steps = int((kend - kbeg + BK - 1) / BK);

    f32x16 acc[2][2];
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j)
#pragma unroll
            for (int e = 0; e < 16; ++e) acc[i][j][e] = 0.f;

    f32x4 ra[4], rb[4];
    load_tile<AKC>(ra, a.A, a.lda, a.M, m0, kbeg, kend, p, q);
    load_tile<BKC>(rb, a.B, a.ldb, a.N, n0, kbeg, kend, p, q);
    store_tile<AKC>(ra, lds, p, q);
    store_tile<BKC>(rb, lds + TILE, p, q);

    for (int t = 0; t < steps; ++t) {
        // one barrier per step: the tile written during step t-1 is visible, and every wave has left step t-1, whose buffer
        // this step overwrites
        __syncthreads();
        const bool more = t + 1 < steps;
        if (more) {
            load_tile<AKC>(ra, a.A, a.lda, a.M, m0, kbeg + int64_t(t + 1) * BK, kend, p, q);
            load_tile<BKC>(rb, a.B, a.ldb, a.N, n0, kbeg + int64_t(t + 1) * BK, kend, p, q);
        }
        const uint16_t* As = lds + (t & 1) * 2 * TILE;
        const uint16_t* Bs = As + TILE;
#pragma unroll
        for (int ks = 0; ks < BK / 16; ++ks) {
            bf16x8 fa[2], fb[2];
#pragma unroll
            for (int i = 0; i < 2; ++i) {
                fa[i] = *reinterpret_cast<const bf16x8*>(As + (wm * 64 + i * 32 + r) * PITCH + ks * 16 + 8 * h);
                fb[i] = *reinterpret_cast<const bf16x8*>(Bs + (wn * 64 + i * 32 + r) * PITCH + ks * 16 + 8 * h);
            }
#pragma unroll
            for (int i = 0; i < 2; ++i)
#pragma unroll
                for (int j = 0; j < 2; ++j) acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(fa[i], fb[j], acc[i][j], 0, 0, 0);
        }
        if (more) {
            uint16_t* Wa = lds + ((t + 1) & 1) * 2 * TILE;
            store_tile<AKC>(ra, Wa, p, q);
            store_tile<BKC>(rb, Wa + TILE, p, q);
        }
    }

    // C/D map of the 32 x 32 MFMA: column = lane & 31, row = (e & 3) + 8 (e >> 2) + 4 (lane >> 5)
    float* C = a.C + int64_t(blockIdx.y) * a.chunk_stride;
#pragma unroll
    for (int j = 0; j < 2; ++j) {
        const int64_t col = n0 + wn * 64 + j * 32 + r;
        if (col >= a.N) continue;
        const float bias = a.bias != nullptr ? a.bias[col] : 0.f;
#pragma unroll
        for (int i = 0; i < 2; ++i)
#pragma unroll
            for (int e = 0; e < 16; ++e) {
                const int64_t row = m0 + wm * 64 + i * 32 + (e & 3) + 8 * (e >> 2) + 4 * h;
                if (row >= a.M) continue;
                float* dst = C + row * a.ldc + col;
                float v = acc[i][j][e];
                if (a.bias != nullptr) v += bias;
                if (a.accumulate) v = *dst + v;
                *dst = v;
            }
    }
}

// C (+)= chunk 0 + chunk 1 + ... (in that order) [+ bias], one element per thread (consecutive lanes on consecutive columns).
// chunks == 0 is the empty sum: C = 0 + bias, the K == 0 case with a bias.
__global__ __launch_bounds__(256) void gemm_bf16_fold(const float* __restrict__ part, int64_t chunk_stride, int chunks, float* C,
                                                      int64_t ldc, int64_t M, int64_t N, const float* __restrict__ bias, int accumulate) {
    const int64_t total = M * N;
    for (int64_t i = int64_t(blockIdx.x) * blockDim.x + threadIdx.x; i < total; i += int64_t(gridDim.x) * blockDim.x) {
        float s = chunks > 0 ? part[i] : 0.f;
        for (int c = 1; c < chunks; ++c) s += part[i + c * chunk_stride];
        const int64_t row = i / N, col = i - row * N;
        float* dst = C + row * ldc + col;
        if (bias != nullptr) s += bias[col];
        if (accumulate) s = *dst + s;
        *dst = s;
    }
}

// dst[i] = r(src[i]) kept as fp32: the conversion the staging pass applies, for references and tests
__global__ __launch_bounds__(256) void bf16_round_kernel(const float* src, float* dst, int64_t n) {        // (dst may be src)
    for (int64_t i = int64_t(blockIdx.x) * blockDim.x + threadIdx.x; i < n; i += int64_t(gridDim.x) * blockDim.x)
        dst[i] = __uint_as_float(pk_bf16(src[i], 0.f) << 16);
}

}  // namespace

}  // namespace lg

using namespace lg;

extern "C" int lg_gemm_bf16_f32(int transA, int transB, int64_t M, int64_t N, int64_t K, const float* A, int64_t lda, const float* B,
                                int64_t ldb, float* C, int64_t ldc, const float* bias, int accumulate) {
    LG_REQUIRE_INIT();
    LG_ARG(M >= 0 && N >= 0 && K >= 0, "lg_gemm_bf16_f32: negative extent (M=%lld N=%lld K=%lld)", (long long)M, (long long)N, (long long)K);
    LG_ARG(!(bias != nullptr && accumulate), "lg_gemm_bf16_f32: a bias together with accumulate is not supported");
    if (M == 0 || N == 0) return LG_OK;
    LG_ARG(C != nullptr && ldc >= N, "lg_gemm_bf16_f32: C is NULL or ldc=%lld is smaller than N=%lld", (long long)ldc, (long long)N);
    {
        const int rc = adam_epilogue_check_write(C, ((M - 1) * ldc + N) * int64_t(sizeof(float)));
        if (rc != LG_OK) return rc;
    }
    if (K == 0) {
        if (accumulate) return LG_OK;
        int64_t shape[2] = {M, N}, st[2] = {ldc, 1};
        if (bias == nullptr) return lg_fill_strided(4, 2, shape, C, st, 0);      // the empty sum
        // the empty sum plus the bias row: the fold over no chunks, no operand is touched
        hipLaunchKernelGGL(gemm_bf16_fold, dim3(stream_grid(M * N)), dim3(256), 0, rt().stream, static_cast<const float*>(nullptr),
                           int64_t(0), 0, C, ldc, M, N, bias, 0);
        LG_CHECK_LAUNCH();
        return LG_OK;
    }
    LG_ARG(A != nullptr && B != nullptr, "lg_gemm_bf16_f32: NULL operand");
    LG_ARG(lda >= (transA ? M : K) && ldb >= (transB ? K : N),
           "lg_gemm_bf16_f32: leading dimension too small (lda=%lld ldb=%lld for M=%lld N=%lld K=%lld tA=%d tB=%d)",
           (long long)lda, (long long)ldb, (long long)M, (long long)N, (long long)K, transA, transB);
    const int64_t tiles_m = (M + BM - 1) / BM, tiles_n = (N + BN - 1) / BN, tiles = tiles_m * tiles_n;
    LG_ARG(tiles < (int64_t(1) << 31) && tiles_m < (int64_t(1) << 30), "lg_gemm_bf16_f32: problem too large for one launch");

    // K in chunks when the tiles alone leave most of the chip idle and every chunk still gets at least 256 k values
    const int cus = rt().compute_units > 0 ? rt().compute_units : 256;
    int64_t chunks = 1;
    if (tiles * 2 <= cus && K >= 512) {
        chunks = cus / tiles;
        if (chunks > K / 256) chunks = K / 256;
        if (chunks > 64) chunks = 64;
    }
    const int64_t k_chunk = ((K + chunks - 1) / chunks + BK - 1) / BK * BK;
    chunks = (K + k_chunk - 1) / k_chunk;                              // no empty chunk

    Bf16Args a{};
    a.A = A; a.B = B;
    a.C = C; a.bias = bias;
    a.M = M; a.N = N; a.K = K; a.lda = lda; a.ldb = ldb; a.ldc = ldc;
    a.k_chunk = k_chunk; a.chunk_stride = 0; a.tiles_m = int(tiles_m); a.accumulate = accumulate ? 1 : 0;
    void* workspace = nullptr;
    if (chunks > 1) {
        const int rc = lg_malloc(&workspace, size_t(chunks) * size_t(M) * size_t(N) * sizeof(float));
        if (rc != LG_OK) return rc;
        a.C = static_cast<float*>(workspace); a.ldc = N; a.chunk_stride = M * N; a.bias = nullptr; a.accumulate = 0;
    }
    const dim3 grid{unsigned(tiles), unsigned(chunks), 1u};
    const bool akc = !transA, bkc = transB != 0;
    if (akc && bkc) hipLaunchKernelGGL((gemm_bf16_kernel<true, true>), grid, dim3(256), 0, rt().stream, a);
    else if (akc) hipLaunchKernelGGL((gemm_bf16_kernel<true, false>), grid, dim3(256), 0, rt().stream, a);
    else if (bkc) hipLaunchKernelGGL((gemm_bf16_kernel<false, true>), grid, dim3(256), 0, rt().stream, a);
    else hipLaunchKernelGGL((gemm_bf16_kernel<false, false>), grid, dim3(256), 0, rt().stream, a);
    hipError_t e = hipGetLastError();
    if (e == hipSuccess && chunks > 1) {
        hipLaunchKernelGGL(gemm_bf16_fold, dim3(stream_grid(M * N)), dim3(256), 0, rt().stream, static_cast<const float*>(workspace),
                           M * N, int(chunks), C, ldc, M, N, bias, accumulate ? 1 : 0);
        e = hipGetLastError();
    }
    if (workspace != nullptr) (void)lg_free(workspace);        // stream order: the next user of these bytes runs after the fold
    if (e != hipSuccess) {
        set_error("lg_gemm_bf16_f32: kernel launch failed: %s", hipGetErrorString(e));
        return LG_EHIP;
    }
    return LG_OK;
}

extern "C" int lg_bf16_round_f32(const float* src, float* dst, int64_t n) {
    LG_REQUIRE_INIT();
    LG_ARG(n >= 0, "lg_bf16_round_f32: negative count");
    if (n == 0) return LG_OK;
    LG_ARG(src != nullptr && dst != nullptr, "lg_bf16_round_f32: NULL pointer");
    const int rc = adam_epilogue_check_write(dst, n * int64_t(sizeof(float)));
    if (rc != LG_OK) return rc;
    hipLaunchKernelGGL(bf16_round_kernel, dim3(stream_grid(n)), dim3(256), 0, rt().stream, src, dst, n);
    LG_CHECK_LAUNCH();
    return LG_OK;
}
