// 2-D convolution (forward, input gradient, weight + bias gradient) and 2-D max / min pooling for gfx950, fp32
// (C ABI: include/lghip.h).  Dense NCHW tensors, OIHW weights, zero padding `pad` on both spatial axes, strides (sh, sw).
//
// THE CONVOLUTIONS are one implicit GEMM on v_mfma_f32_32x32x2f32: out[m][n] = sum_k A[m][k] * B[k][n], where the im2col
// matrix is never written - its elements are gathered from x (or g) while an operand tile is staged into LDS.
//
//             rows m     columns n (lanes)    reduction k            A[m][k]              B[k][n]
//   forward   o          (n, oh, ow)          (c, kh, kw)            w[o][c][kh][kw]      x[n][c][oh*sh+kh-p][ow*sw+kw-p]
//   dx        c          (n, h, w)            (o, kh, kw)            w[o][c][kh][kw]      g[n][o][(h+p-kh)/sh][(w+p-kw)/sw]
//   dw        o          (c, kh, kw) | ones   (n, oh, ow)            g[n][o][oh][ow]      x[n][c][oh*sh+kh-p][ow*sw+kw-p] | 1
//
// A tap in the padding (forward, dw) or a division that is inexact or out of range (dx) contributes 0 by SELECTION: the
// address is clamped to element 0 and the loaded value replaced, so nothing outside a tensor is read and no branch splits the
// loads.  LDS positions past the reduction length, past the last row and past the last column are written as zeros in BOTH
// operands: stale LDS times 0 is NaN when the stale value is NaN or inf.
//
// Forward / dx: a workgroup owns 32 rows x 128 columns (4 waves, 32 columns each) and walks k in chunks of 32.  The columns
// are output positions, so the gather and the stores are coalesced along (oh, ow) / (h, w) and the result goes straight into
// NCHW.  The k -> (c, kh, kw) decomposition is done once into a table in LDS; positions are decomposed once per thread.  The
// division by the stride in dx is a multiplication by ceil(2^32 / s) (exact for operands below 2^16, checked on the host).
// k ascends in one accumulator chain per output: lane half h of MFMA j takes k = 2j + h.  The next chunk's global loads are in
// flight while the current one is multiplied.
//
// dw: the output is tiny and the reduction long, so the reduction is split.  A workgroup owns a 32 x 32 output tile and one
// slice of the positions, walked in chunks of 128 of which every wave takes 32; the four accumulators are summed through LDS
// in wave order.  With more than one slice the workgroup publishes its partial tile, takes a ticket for the tile and the last
// arriver folds the partials in slice order (handoff.h).  The slice count depends on the shape only, so a result is the same
// bits on every run.  db is the column K of the tile: the gathered operand has a column of ones there, as in
// lg_gemm_rowsum_f32.
//
// POOLING: one thread per output element (forward) / per input element (backward); see lghip.h for the semantics.
#include "common.h"
#include "handoff.h"
#include "mfma_lds.h"

namespace lg {

enum { CONV_FWD = 0, CONV_DX = 1, CONV_DW = 2 };

constexpr int kConvTable = 2048;       // entries of the k -> (offset, kh, kw) table: the bound on C*KH*KW and O*KH*KW
constexpr int kConvMaxExtent = 16384;  // H, W, pad, sh, sw: keeps (h + p - kh) below 2^16 for the multiply-high division
constexpr int kConvMaxSlices = 256;    // dw: position slices at most; one ticket level suffices up to here
constexpr int kPA = 34, kPAW = 130;    // A rows (k contiguous): pitch = 2 mod 4 with an odd half -> 32 rows x 2 lane halves on 64 banks
constexpr int kPB = 160;               // B rows of 128 columns: 32 mod 64, the two lane halves (k, k + 1) on different bank halves

struct ConvP {
    int N, C, H, W, O, KH, KW, OH, OW, sh, sw, pad;
    int K;                 // forward: C*KH*KW; dx: O*KH*KW (reduction lengths); dw: C*KH*KW (+ 1 with db = columns)
    int M;                 // rows: O (forward, dw), C (dx)
    unsigned mh, mw;       // ceil(2^32 / sh), ceil(2^32 / sw); unused when the stride is 1
    int64_t P;             // forward, dw: N*OH*OW; dx: N*H*W
    int chunks_per_slice;  // dw
    int has_db;            // dw
};

__device__ __forceinline__ float relu_of(float t) { return (t != t) ? t : (t > 0.0f ? t : 0.0f); }   // elementwise.hip's OpRelu

// x[n][c][ih0 + kh][iw0 + kw] of the tap the table entry describes, 0 in the padding
template <bool RELU>
__device__ __forceinline__ float gather_x(const float* __restrict__ x, int64_t base, int ih0, int iw0, int off, int hw, bool live,
                                          const ConvP& p) {
    const int ih = ih0 + (hw >> 16), iw = iw0 + (hw & 0xffff);
    const bool ok = live && unsigned(ih) < unsigned(p.H) && unsigned(iw) < unsigned(p.W);
    float v = x[ok ? base + off : 0];
    if constexpr (RELU) v = relu_of(v);
    return ok ? v : 0.0f;
}

// t / s for 0 <= t < 2^16 and s <= 2^14: m = ceil(2^32 / s)
__device__ __forceinline__ int div_small(int t, int s, unsigned m) { return s == 1 ? t : int(__umulhi(unsigned(t), m)); }

template <int MODE, bool RELU>
__global__ void __launch_bounds__(256) conv2d_igemm(const float* __restrict__ A, const float* __restrict__ B,
                                                    const float* __restrict__ bias, float* out, float* out2, float* partial,
                                                    int* tickets, ConvP p) {
    constexpr bool DW = MODE == CONV_DW;
    constexpr int NA = DW ? 16 : 4;
    __shared__ float As[32 * kPAW];
    __shared__ float Bs[32 * kPB];
    __shared__ int tab_off[DW ? 32 : kConvTable];
    __shared__ int tab_hw[DW ? 32 : kConvTable];
    __shared__ int arrived_last;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, r = lane & 31, h = lane >> 5;
    const int khkw = p.KH * p.KW, hw_in = p.H * p.W, hw_out = p.OH * p.OW;
    const int row0 = blockIdx.y * 32;

    // ---- the table: one decomposition per k (forward, dx) / per column of this tile (dw)
    if constexpr (DW) {
        if (tid < 32) {
            const int col = blockIdx.x * 32 + tid, ncols = p.K - p.has_db;
            int off = 0, hw = -2;                                          // -2: past the last column, -1: the column of ones
            if (col < ncols) {
                const int c = col / khkw, t = col - c * khkw, kh = t / p.KW, kw = t - kh * p.KW;
                off = c * hw_in + kh * p.W + kw;
                hw = (kh << 16) | kw;
            } else if (col == ncols && p.has_db) {
                hw = -1;
            }
            tab_off[tid] = off;
            tab_hw[tid] = hw;
        }
    } else {
        for (int k = tid; k < p.K; k += 256) {
            const int c = k / khkw, t = k - c * khkw, kh = t / p.KW, kw = t - kh * p.KW;
            tab_off[k] = MODE == CONV_FWD ? c * hw_in + kh * p.W + kw : c;      // dx: the output channel o
            tab_hw[k] = (kh << 16) | kw;
        }
    }
    __syncthreads();

    float ra[NA], rb[16];
    af32x16 acc = zero16();

    if constexpr (!DW) {
        // ---- forward / dx: 32 rows x 128 positions, k in chunks of 32
        const int scol = tid & 127, sk = tid >> 7;                     // B staging: one position per thread, k = sk + 2 i
        const int64_t spos = int64_t(blockIdx.x) * 128 + scol;
        const bool slive = spos < p.P;
        const int plane = MODE == CONV_FWD ? hw_out : hw_in, pw = MODE == CONV_FWD ? p.OW : p.W;
        const int sq = slive ? int(spos) : 0, sn = sq / plane, srem = sq - sn * plane, sy = srem / pw, sx = srem - sy * pw;
        // forward: the window's corner in x; dx: (h + p, w + p)
        const int y0 = MODE == CONV_FWD ? sy * p.sh - p.pad : sy + p.pad, x0 = MODE == CONV_FWD ? sx * p.sw - p.pad : sx + p.pad;
        const int64_t bbase = MODE == CONV_FWD ? int64_t(sn) * p.C * hw_in + int64_t(y0) * p.W + x0 : int64_t(sn) * p.O * hw_out;
        const int ak = tid & 31, am = tid >> 5;                         // A staging: k = ak, rows am + 8 i
        const int chunks = (p.K + 31) >> 5;

        auto load = [&](int chunk) {
#pragma unroll
            for (int i = 0; i < 16; ++i) {
                const int k = chunk * 32 + sk + 2 * i;
                const bool live = slive && k < p.K;
                const int kk = k < p.K ? k : 0, off = tab_off[kk], hw = tab_hw[kk];
                if constexpr (MODE == CONV_FWD) {
                    rb[i] = gather_x<RELU>(B, bbase, y0, x0, off, hw, live, p);
                } else {
                    const int th = y0 - (hw >> 16), tw = x0 - (hw & 0xffff);
                    const int thc = th < 0 ? 0 : th, twc = tw < 0 ? 0 : tw;
                    const int qh = div_small(thc, p.sh, p.mh), qw = div_small(twc, p.sw, p.mw);
                    const bool ok = live && th >= 0 && tw >= 0 && qh * p.sh == thc && qw * p.sw == twc && qh < p.OH && qw < p.OW;
                    const float v = B[ok ? bbase + int64_t(off) * hw_out + qh * p.OW + qw : 0];
                    rb[i] = ok ? v : 0.0f;
                }
            }
            const int k = chunk * 32 + ak, kk = k < p.K ? k : 0;
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const int row = row0 + am + 8 * i;
                const bool ok = k < p.K && row < p.M;
                int64_t a;
                if constexpr (MODE == CONV_FWD) {
                    a = int64_t(row) * p.K + k;
                } else {
                    const int hw = tab_hw[kk];
                    a = (int64_t(tab_off[kk]) * p.C + row) * khkw + (hw >> 16) * p.KW + (hw & 0xffff);
                }
                const float v = A[ok ? a : 0];
                ra[i] = ok ? v : 0.0f;
            }
        };

        load(0);
        for (int chunk = 0; chunk < chunks; ++chunk) {
            if (chunk > 0) __syncthreads();                             // the previous chunk has been multiplied
#pragma unroll
            for (int i = 0; i < 16; ++i) Bs[(sk + 2 * i) * kPB + scol] = rb[i];
#pragma unroll
            for (int i = 0; i < 4; ++i) As[(am + 8 * i) * kPA + ak] = ra[i];
            __syncthreads();
            if (chunk + 1 < chunks) load(chunk + 1);                    // in flight during the MFMAs below
            const int left = p.K - chunk * 32, kend = left >= 32 ? 32 : (left + 7) & ~7;
            for (int k0 = 0; k0 < kend; k0 += 8) {
                float a[4], b[4];
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    a[j] = As[r * kPA + k0 + 2 * j + h];
                    b[j] = Bs[(k0 + 2 * j + h) * kPB + wave * 32 + r];
                }
#pragma unroll
                for (int j = 0; j < 4; ++j) acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a[j], b[j], acc, 0, 0, 0);
            }
        }

        // ---- straight into NCHW: lanes along the positions
        const int64_t opos = int64_t(blockIdx.x) * 128 + wave * 32 + r;
        if (opos < p.P) {
            const int on = int(opos) / plane, orem = int(opos) - on * plane;
#pragma unroll
            for (int e = 0; e < 16; ++e) {
                const int row = row0 + acc_row(e, h);
                if (row < p.M) {
                    float v = acc[e];
                    if constexpr (MODE == CONV_FWD) if (bias != nullptr) v = v + bias[row];          // a second rounding, like y + b
                    out[(int64_t(on) * p.M + row) * plane + orem] = v;
                }
            }
        }
    } else {
        // ---- dw: a 32 x 32 tile of (o, column) over one slice of the positions, 128 per chunk, 32 per wave
        const int sk = tid & 127, sj = tid >> 7;                        // staging: one position per thread, rows / columns sj + 2 i
        const int slice = blockIdx.z;
        const int64_t total_chunks = (p.P + 127) >> 7;
        const int64_t c_begin = int64_t(slice) * p.chunks_per_slice;
        int64_t c_end = c_begin + p.chunks_per_slice;
        if (c_end > total_chunks) c_end = total_chunks;

        auto load = [&](int64_t chunk) {
            const int64_t pos = chunk * 128 + sk;
            const bool live = pos < p.P;
            const int q = live ? int(pos) : 0, n = q / hw_out, rem = q - n * hw_out, oh = rem / p.OW, ow = rem - oh * p.OW;
            const int y0 = oh * p.sh - p.pad, x0 = ow * p.sw - p.pad;
            const int64_t xbase = int64_t(n) * p.C * hw_in + int64_t(y0) * p.W + x0;
            const int64_t gbase = int64_t(n) * p.O * hw_out + rem;
#pragma unroll
            for (int i = 0; i < 16; ++i) {
                const int row = row0 + sj + 2 * i;
                const bool ok = live && row < p.M;
                const float v = A[ok ? gbase + int64_t(row) * hw_out : 0];
                ra[i] = ok ? v : 0.0f;
            }
#pragma unroll
            for (int i = 0; i < 16; ++i) {
                const int hw = tab_hw[sj + 2 * i], off = tab_off[sj + 2 * i];
                const float v = gather_x<RELU>(B, xbase, y0, x0, off, hw < 0 ? 0 : hw, live && hw >= 0, p);
                rb[i] = hw == -1 ? (live ? 1.0f : 0.0f) : v;
            }
        };

        if (c_begin < c_end) load(c_begin);
        for (int64_t chunk = c_begin; chunk < c_end; ++chunk) {
            if (chunk > c_begin) __syncthreads();
#pragma unroll
            for (int i = 0; i < 16; ++i) {
                As[(sj + 2 * i) * kPAW + sk] = ra[i];
                Bs[(sj + 2 * i) * kPAW + sk] = rb[i];
            }
            __syncthreads();
            if (chunk + 1 < c_end) load(chunk + 1);
#pragma unroll
            for (int k0 = 0; k0 < 32; k0 += 8) {
                float a[4], b[4];
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    a[j] = As[r * kPAW + wave * 32 + k0 + 2 * j + h];
                    b[j] = Bs[r * kPAW + wave * 32 + k0 + 2 * j + h];
                }
#pragma unroll
                for (int j = 0; j < 4; ++j) acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a[j], b[j], acc, 0, 0, 0);
            }
        }

        // ---- the four waves' accumulators, summed in wave order by wave 0
        __syncthreads();
        float* red = Bs;                                                // 3 x 1024 floats
        if (wave > 0) {
#pragma unroll
            for (int e = 0; e < 16; ++e) red[(wave - 1) * 1024 + acc_row(e, h) * 32 + r] = acc[e];
        }
        __syncthreads();
        const int ncols = p.K - p.has_db, col0 = blockIdx.x * 32;
        const int live_rows = p.M - row0 < 32 ? p.M - row0 : 32, live_cols = p.K - col0 < 32 ? p.K - col0 : 32;
        const int slices = gridDim.z;
        auto store = [&](int rl, int cl, float v) {                     // element (rl, cl) of the tile, live
            const int col = col0 + cl;
            if (col < ncols) out[int64_t(row0 + rl) * ncols + col] = v;
            else out2[row0 + rl] = v;
        };
        if (wave == 0) {
#pragma unroll
            for (int e = 0; e < 16; ++e) {
                const int rl = acc_row(e, h);
                const float v = ((acc[e] + red[rl * 32 + r]) + red[1024 + rl * 32 + r]) + red[2048 + rl * 32 + r];
                if (rl < live_rows && r < live_cols) {
                    if (slices == 1) store(rl, r, v);
                    else {
                        const int64_t tile = int64_t(blockIdx.y) * gridDim.x + blockIdx.x, tiles = int64_t(gridDim.x) * gridDim.y;
                        handoff::publish<float>(partial + ((int64_t(slice) * tiles + tile) << 10) + rl * 32 + r, v);
                    }
                }
            }
        }
        if (slices == 1) return;
        // ---- the hand-off: one ticket per tile, the last arriver folds every slice.  (At most kConvMaxSlices slices: 1024 slices
        // folded through a second ticket level, groups of 32 first, were measured slower - profiles/conv2d.md.)
        const int64_t tile = int64_t(blockIdx.y) * gridDim.x + blockIdx.x, tiles = int64_t(gridDim.x) * gridDim.y;
        const int live = live_rows * live_cols;
        const int64_t pstride = tiles << 10;
        // fold `count` partial tiles from `src` on (pstride apart): thread (j, e) sums tiles j, j + J, ... of live element e in
        // ascending order, then the J sums are added in order of j.  J depends on the tile's live size and `count` only.
        auto fold_tiles = [&](const float* src, int count, auto&& sink) {
            int J = live > 128 ? 1 : 256 / live;
            if (J > count) J = count;
            if (J > 32) J = 32;
            auto fold = [&](int e, int j) {
                const int rl = e / live_cols, cl = e - rl * live_cols;
                const float* q = src + rl * 32 + cl;
                float f = 0.0f;
                int s = j;
                for (; s + 7 * J < count; s += 8 * J) {
                    float x[8];
#pragma unroll
                    for (int u = 0; u < 8; ++u) x[u] = __hip_atomic_load(q + int64_t(s + u * J) * pstride, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
#pragma unroll
                    for (int u = 0; u < 8; ++u) f = (s == j && u == 0) ? x[0] : f + x[u];
                }
                for (; s < count; s += J) {
                    const float x = __hip_atomic_load(q + int64_t(s) * pstride, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                    f = s == j ? x : f + x;
                }
                return f;
            };
            if (J == 1) {
                for (int e = tid; e < live; e += 256) sink(e / live_cols, e % live_cols, fold(e, 0));
            } else {
                float* sums = As;                                       // J * live <= 256 floats
                if (tid < J * live) sums[tid] = fold(tid % live, tid / live);
                __syncthreads();
                if (tid < live) {
                    float f = sums[tid];
                    for (int j = 1; j < J; ++j) f += sums[j * live + tid];
                    sink(tid / live_cols, tid % live_cols, f);
                }
            }
        };
        if (!handoff::arrive_workgroup(tickets + tile, slices, &arrived_last)) return;
        fold_tiles(partial + (tile << 10), slices, store);
    }
}

// ---- pooling ---------------------------------------------------------------------------------------------------------
template <int OP>
__device__ __forceinline__ float pool_pick(float v, float m) {           // np.max / np.min: the first NaN stays
    if constexpr (OP == 0) return (v > m || v != v) ? v : m;
    else return (v < m || v != v) ? v : m;
}

template <int OP>
__global__ void __launch_bounds__(256) pool2d_fwd(const float* __restrict__ x, float* __restrict__ y, unsigned n_out, int H, int W,
                                                  int OH, int OW, int kh, int kw) {
    const unsigned i = blockIdx.x * 256u + threadIdx.x;
    if (i >= n_out) return;
    const unsigned t = i / unsigned(OW), ow = i - t * unsigned(OW), l = t / unsigned(OH), oh = t - l * unsigned(OH);
    const float* px = x + int64_t(l) * H * W + int64_t(oh) * kh * W + ow * kw;
    float m = px[0];
    for (int a = 0; a < kh; ++a)
        for (int b = 0; b < kw; ++b) m = pool_pick<OP>(px[a * W + b], m);
    y[i] = m;
}

__global__ void __launch_bounds__(256) pool2d_bwd(const float* __restrict__ x, const float* __restrict__ y, const float* __restrict__ g,
                                                  float* __restrict__ dx, unsigned n_in, int H, int W, int OH, int OW, int kh, int kw) {
    const unsigned i = blockIdx.x * 256u + threadIdx.x;
    if (i >= n_in) return;
    const unsigned t = i / unsigned(W), w = i - t * unsigned(W), l = t / unsigned(H), hh = t - l * unsigned(H);
    const unsigned oh = hh / unsigned(kh), ow = w / unsigned(kw);
    const bool in = oh < unsigned(OH) && ow < unsigned(OW);             // else: the cropped margin
    const int64_t o = in ? (int64_t(l) * OH + oh) * OW + ow : 0;
    const float v = g[o] * (x[i] == y[o] ? 1.0f : 0.0f);                 // elementwise.hip's OpMaxBwd
    dx[i] = in ? v : 0.0f;
}

// ---- host --------------------------------------------------------------------------------------------------------------
static thread_local int32_t g_conv_plan[6] = {-1, 0, 0, 0, 0, 0};

static int conv_params(const char* who, int64_t N, int64_t C, int64_t H, int64_t W, int64_t O, int64_t KH, int64_t KW, int64_t sh,
                       int64_t sw, int64_t pad, ConvP& p) {
    LG_ARG(N >= 1 && C >= 1 && H >= 1 && W >= 1 && O >= 1 && KH >= 1 && KW >= 1, "%s: every extent must be at least 1", who);
    LG_ARG(sh >= 1 && sw >= 1 && pad >= 0, "%s: strides must be positive and the padding non-negative", who);
    LG_ARG(H <= kConvMaxExtent && W <= kConvMaxExtent && pad <= kConvMaxExtent && sh <= kConvMaxExtent && sw <= kConvMaxExtent,
           "%s: H, W, pad and the strides are limited to %d", who, kConvMaxExtent);
    LG_ARG(KH <= H + 2 * pad && KW <= W + 2 * pad, "%s: a %lldx%lld window does not fit the padded input", who, (long long)KH, (long long)KW);
    LG_ARG(C * KH * KW <= kConvTable && O * KH * KW <= kConvTable, "%s: C*KH*KW and O*KH*KW are limited to %d (the LDS offset table)", who,
           kConvTable);
    const int64_t OH = (H + 2 * pad - KH) / sh + 1, OW = (W + 2 * pad - KW) / sw + 1, lim = int64_t(1) << 31;
    LG_ARG(N * OH * OW < lim && N * H * W < lim && C * H * W < lim && O * OH * OW < lim,
           "%s: N*OH*OW, N*H*W, C*H*W and O*OH*OW must stay below 2^31", who);
    p.N = int(N); p.C = int(C); p.H = int(H); p.W = int(W); p.O = int(O); p.KH = int(KH); p.KW = int(KW);
    p.OH = int(OH); p.OW = int(OW); p.sh = int(sh); p.sw = int(sw); p.pad = int(pad);
    p.mh = sh > 1 ? unsigned(0xFFFFFFFFu / unsigned(sh)) + 1u : 0u;
    p.mw = sw > 1 ? unsigned(0xFFFFFFFFu / unsigned(sw)) + 1u : 0u;
    p.chunks_per_slice = 0; p.has_db = 0;
    return LG_OK;
}

static void note_conv_plan(int kernel, int cols, int kchunk, int relu) {
    g_conv_plan[0] = kernel; g_conv_plan[1] = 32; g_conv_plan[2] = cols; g_conv_plan[3] = kchunk; g_conv_plan[5] = relu;
}

}  // namespace lg

using namespace lg;

extern "C" int lg_conv2d_fwd_f32(const float* x, const float* w, const float* bias, float* y, int64_t N, int64_t C, int64_t H,
                                 int64_t W, int64_t O, int64_t KH, int64_t KW, int64_t sh, int64_t sw, int64_t pad, int relu_x) {
    LG_REQUIRE_INIT();
    LG_ARG(x != nullptr && w != nullptr && y != nullptr, "lg_conv2d_fwd_f32: NULL pointer");
    ConvP p;
    int rc = conv_params("lg_conv2d_fwd_f32", N, C, H, W, O, KH, KW, sh, sw, pad, p);
    if (rc != LG_OK) return rc;
    p.K = p.C * p.KH * p.KW; p.M = p.O; p.P = int64_t(p.N) * p.OH * p.OW;
    rc = adam_epilogue_check_write(y, p.P * p.O * int64_t(sizeof(float)));
    if (rc != LG_OK) return rc;
    const dim3 grid(unsigned((p.P + 127) / 128), unsigned((p.M + 31) / 32));
    if (relu_x) hipLaunchKernelGGL((conv2d_igemm<CONV_FWD, true>), grid, dim3(256), 0, rt().stream, w, x, bias, y, nullptr, nullptr, nullptr, p);
    else hipLaunchKernelGGL((conv2d_igemm<CONV_FWD, false>), grid, dim3(256), 0, rt().stream, w, x, bias, y, nullptr, nullptr, nullptr, p);
    LG_CHECK_LAUNCH();
    note_conv_plan(CONV_FWD, 128, 32, relu_x ? 1 : 0);
    return LG_OK;
}

extern "C" int lg_conv2d_dx_f32(const float* g, const float* w, float* dx, int64_t N, int64_t C, int64_t H, int64_t W, int64_t O,
                                int64_t KH, int64_t KW, int64_t sh, int64_t sw, int64_t pad) {
    LG_REQUIRE_INIT();
    LG_ARG(g != nullptr && w != nullptr && dx != nullptr, "lg_conv2d_dx_f32: NULL pointer");
    ConvP p;
    int rc = conv_params("lg_conv2d_dx_f32", N, C, H, W, O, KH, KW, sh, sw, pad, p);
    if (rc != LG_OK) return rc;
    p.K = p.O * p.KH * p.KW; p.M = p.C; p.P = int64_t(p.N) * p.H * p.W;
    rc = adam_epilogue_check_write(dx, p.P * p.C * int64_t(sizeof(float)));
    if (rc != LG_OK) return rc;
    const dim3 grid(unsigned((p.P + 127) / 128), unsigned((p.M + 31) / 32));
    hipLaunchKernelGGL((conv2d_igemm<CONV_DX, false>), grid, dim3(256), 0, rt().stream, w, g, nullptr, dx, nullptr, nullptr, nullptr, p);
    LG_CHECK_LAUNCH();
    note_conv_plan(CONV_DX, 128, 32, 0);
    return LG_OK;
}

extern "C" int lg_conv2d_dw_f32(const float* g, const float* x, float* dw, float* db, int64_t N, int64_t C, int64_t H, int64_t W,
                                int64_t O, int64_t KH, int64_t KW, int64_t sh, int64_t sw, int64_t pad, int relu_x) {
    LG_REQUIRE_INIT();
    LG_ARG(g != nullptr && x != nullptr && dw != nullptr, "lg_conv2d_dw_f32: NULL pointer");
    ConvP p;
    int rc = conv_params("lg_conv2d_dw_f32", N, C, H, W, O, KH, KW, sh, sw, pad, p);
    if (rc != LG_OK) return rc;
    p.has_db = db != nullptr ? 1 : 0;
    p.K = p.C * p.KH * p.KW + p.has_db; p.M = p.O; p.P = int64_t(p.N) * p.OH * p.OW;
    rc = adam_epilogue_check_write(dw, int64_t(p.O) * (p.K - p.has_db) * int64_t(sizeof(float)));
    if (rc == LG_OK && db != nullptr) rc = adam_epilogue_check_write(db, p.O * int64_t(sizeof(float)));
    if (rc != LG_OK) return rc;
    // slices: a function of the shape alone.  At least two chunks of 128 positions per workgroup, at most kConvMaxSlices slices.
    const int64_t chunks = (p.P + 127) / 128;
    const dim3 tiles(unsigned((p.K + 31) / 32), unsigned((p.M + 31) / 32));
    int64_t cps = (chunks + kConvMaxSlices - 1) / kConvMaxSlices;
    if (cps < 2) cps = 2;
    int64_t slices = (chunks + cps - 1) / cps;
    if (int64_t(tiles.x) * tiles.y > rt().n_tickets) { slices = 1; cps = chunks; }         // more tiles than tickets: no split
    LG_ARG(cps < (int64_t(1) << 31), "lg_conv2d_dw_f32: too many positions");
    p.chunks_per_slice = int(cps);
    float* partial = nullptr;
    if (slices > 1) {
        rc = lg_malloc(reinterpret_cast<void**>(&partial), size_t(slices) * tiles.x * tiles.y * 1024 * sizeof(float));
        if (rc != LG_OK) return rc;
    }
    const dim3 grid(tiles.x, tiles.y, unsigned(slices));
    if (relu_x) hipLaunchKernelGGL((conv2d_igemm<CONV_DW, true>), grid, dim3(256), 0, rt().stream, g, x, nullptr, dw, db, partial, rt().tickets, p);
    else hipLaunchKernelGGL((conv2d_igemm<CONV_DW, false>), grid, dim3(256), 0, rt().stream, g, x, nullptr, dw, db, partial, rt().tickets, p);
    const hipError_t launched = hipGetLastError();
    if (partial != nullptr) {
        rc = lg_free(partial);                                          // stream-ordered: only later launches reuse the block
        if (rc != LG_OK) return rc;
    }
    if (launched != hipSuccess) { set_error("lg_conv2d_dw_f32: kernel launch failed: %s", hipGetErrorString(launched)); return LG_EHIP; }
    note_conv_plan(CONV_DW, 32, 128, relu_x ? 1 : 0);
    g_conv_plan[4] = int32_t(slices);
    return LG_OK;
}

extern "C" int lg_conv2d_last_plan(int32_t out[6]) {
    LG_ARG(out != nullptr, "lg_conv2d_last_plan: NULL pointer");
    for (int i = 0; i < 6; ++i) out[i] = g_conv_plan[i];
    return LG_OK;
}

static int pool_args(const char* who, int64_t L, int64_t H, int64_t W, int64_t kh, int64_t kw) {
    LG_ARG(L >= 1 && H >= 1 && W >= 1 && kh >= 1 && kw >= 1, "%s: every extent must be at least 1", who);
    LG_ARG(kh <= H && kw <= W, "%s: the window is larger than the input (no output elements)", who);
    LG_ARG(L * H * W < (int64_t(1) << 31), "%s: at most 2^31 - 1 input elements", who);
    return LG_OK;
}

extern "C" int lg_pool2d_fwd_f32(int op, const float* x, float* y, int64_t L, int64_t H, int64_t W, int64_t kh, int64_t kw) {
    LG_REQUIRE_INIT();
    LG_ARG(x != nullptr && y != nullptr, "lg_pool2d_fwd_f32: NULL pointer");
    LG_ARG(op == 0 || op == 1, "lg_pool2d_fwd_f32: op must be 0 (max) or 1 (min)");
    int rc = pool_args("lg_pool2d_fwd_f32", L, H, W, kh, kw);
    if (rc != LG_OK) return rc;
    const int64_t OH = H / kh, OW = W / kw, n_out = L * OH * OW;
    rc = adam_epilogue_check_write(y, n_out * int64_t(sizeof(float)));
    if (rc != LG_OK) return rc;
    const dim3 grid(unsigned((n_out + 255) / 256));
    if (op == 0) hipLaunchKernelGGL((pool2d_fwd<0>), grid, dim3(256), 0, rt().stream, x, y, unsigned(n_out), int(H), int(W), int(OH), int(OW), int(kh), int(kw));
    else hipLaunchKernelGGL((pool2d_fwd<1>), grid, dim3(256), 0, rt().stream, x, y, unsigned(n_out), int(H), int(W), int(OH), int(OW), int(kh), int(kw));
    LG_CHECK_LAUNCH();
    return LG_OK;
}

extern "C" int lg_pool2d_bwd_f32(const float* x, const float* y, const float* g, float* dx, int64_t L, int64_t H, int64_t W, int64_t kh,
                                 int64_t kw) {
    LG_REQUIRE_INIT();
    LG_ARG(x != nullptr && y != nullptr && g != nullptr && dx != nullptr, "lg_pool2d_bwd_f32: NULL pointer");
    int rc = pool_args("lg_pool2d_bwd_f32", L, H, W, kh, kw);
    if (rc != LG_OK) return rc;
    const int64_t n_in = L * H * W;
    rc = adam_epilogue_check_write(dx, n_in * int64_t(sizeof(float)));
    if (rc != LG_OK) return rc;
    hipLaunchKernelGGL(pool2d_bwd, dim3(unsigned((n_in + 255) / 256)), dim3(256), 0, rt().stream, x, y, g, dx, unsigned(n_in), int(H), int(W),
                       int(H / kh), int(W / kw), int(kh), int(kw));
    LG_CHECK_LAUNCH();
    return LG_OK;
}
