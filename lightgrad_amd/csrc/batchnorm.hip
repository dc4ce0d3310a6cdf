// Batch normalisation over every axis but the channel axis (nn.BatchNorm1d / BatchNorm2d), gfx950.
//
// Geometry: dense fp32 (N, C, L), element (n, c, l) at (n*C + c)*L + l; count = N*L elements per channel.
//
//   training forward   stats launch + apply launch
//   backward           sums launch (db = sum g, dw = sum g*xhat) + dx launch (skipped without dx)
//   evaluation         one apply launch that forms scale and shift from the running statistics
//
// The stats and sums launches exist in two addressing forms:
//   form 0 (L > 1)   grid (C, slices): a workgroup reduces a range of its channel's N*L elements (in units of one float or one
//                    float4), lanes along L.  The unit -> (n, l) split is carried along the loop, no division per element.
//   form 1 (L == 1)  grid (ceil(C / 64), slices): 64 lanes across channels, the four waves walk down a range of rows, so every
//                    wave load is 256 contiguous bytes instead of a stride-C gather.
// Statistics are (count, mean, M2) triples: a thread sums (x - K) and (x - K)^2 around K = its own first element, turns the two
// sums into a triple, and triples are merged with Chan's formula - within the wave, across the waves, and across the slices - so
// nothing ever forms E[x^2] - E[x]^2 of the raw values.
// Across workgroups (handoff.h): every slice publishes its partial into a 16-byte slot and takes the channel's ticket; the last
// arriver merges the partials IN SLICE ORDER by a fixed tree, whoever it is - the same bits on every run.  The slice count depends
// on the shape alone.
// The last arriver also writes save_mean / save_rstd and updates the running statistics, all in the stats launch.
#include "common.h"
#include "handoff.h"

namespace lg {

constexpr int kBnMaxSlices = 256;      // one partial per thread of the folding workgroup
constexpr int kBnMaxSlicesCl = 64;     // form 1: each wave of the folding workgroup walks a quarter of the slices
constexpr int kBnTargetGroups = 1024;  // workgroups of a stats / sums launch: four per CU
constexpr int kBnMinUnits = 1024;      // form 0: at least 4 units per thread and slice (one batch of four loads)
constexpr int kBnMinRows = 16;         // form 1: at least 4 rows per wave and slice

struct Stat { float n, mean, m2; };
struct Pair { float a, b; };           // (sum g, sum g * xhat)

// Chan et al.: the triple of the concatenation `a` then `b`
__device__ __forceinline__ Stat merge(Stat a, Stat b) {
    if (b.n == 0.0f) return a;
    if (a.n == 0.0f) return b;
    const float n = a.n + b.n, delta = b.mean - a.mean, f = b.n / n;
    return Stat{n, a.mean + delta * f, a.m2 + b.m2 + delta * delta * (a.n * f)};
}
__device__ __forceinline__ Pair merge(Pair a, Pair b) { return Pair{a.a + b.a, a.b + b.b}; }

__device__ __forceinline__ Stat shuffle_down(Stat v, int off) {
    return Stat{__shfl_down(v.n, off, 64), __shfl_down(v.mean, off, 64), __shfl_down(v.m2, off, 64)};
}
__device__ __forceinline__ Pair shuffle_down(Pair v, int off) { return Pair{__shfl_down(v.a, off, 64), __shfl_down(v.b, off, 64)}; }

// the merge of the 256 values of a workgroup in thread order (neighbours first: an ordered tree); valid in thread 0
template <typename T>
__device__ __forceinline__ T block_merge(T v, T* lds4) {
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) v = merge(v, shuffle_down(v, off));
    __syncthreads();                                               // lds4 may still be read from an earlier call
    if ((threadIdx.x & 63) == 0) lds4[threadIdx.x >> 6] = v;
    __syncthreads();
    if (threadIdx.x == 0) v = merge(merge(lds4[0], lds4[1]), merge(lds4[2], lds4[3]));
    return v;
}

// two sums around K -> a triple
__device__ __forceinline__ Stat shifted_to_stat(float cnt, float k, float s1, float s2) {
    if (cnt == 0.0f) return Stat{0.0f, 0.0f, 0.0f};
    const float m2 = s2 - s1 * (s1 / cnt);
    return Stat{cnt, k + s1 / cnt, m2 < 0.0f ? 0.0f : m2};        // (a NaN stays)
}

__device__ __forceinline__ float relu_keep_nan(float v) { return v < 0.0f ? 0.0f : v; }

struct BnP {
    unsigned N, C, Lu;          // Lu: units per row (L / VEC)
    unsigned chunk;             // form 0: units per slice; form 1: rows per slice
    unsigned slices;
    unsigned tstride;           // ints between two tickets: on cache lines of their own while the pool allows
    float count, eps, momentum, unbias;      // unbias = count / (count - 1)
    int relu_x;
};

__device__ __forceinline__ void finish_channel(Stat t, unsigned c, const BnP& p, float* save_mean, float* save_rstd, float* running_mean,
                                               float* running_var) {
    const float var = t.m2 / p.count;
    save_mean[c] = t.mean;
    save_rstd[c] = 1.0f / sqrtf(var + p.eps);
    if (running_mean != nullptr) running_mean[c] = (1.0f - p.momentum) * running_mean[c] + p.momentum * t.mean;
    if (running_var != nullptr) running_var[c] = (1.0f - p.momentum) * running_var[c] + p.momentum * (var * p.unbias);
}

// ---- form 0: lanes along L -----------------------------------------------------------------------------------------------
// walks the units [begin, end) of channel c, 256 apart: use(load(index of the unit)) for each, in order, four loads in flight
template <typename Load, typename Use>
__device__ __forceinline__ void walk_channel(const BnP& p, unsigned c, unsigned begin, unsigned end, Load&& load, Use&& use) {
    unsigned u = begin + threadIdx.x;
    unsigned n = u / p.Lu, l = u - n * p.Lu;
    const unsigned dn = 256u / p.Lu, dl = 256u - dn * p.Lu;
    auto next = [&]() {
        const size_t unit = (size_t(n) * p.C + c) * p.Lu + l;
        l += dl; n += dn;
        if (l >= p.Lu) { l -= p.Lu; n += 1; }
        return unit;
    };
    for (; u + 768u < end; u += 1024u) {
        const size_t o0 = next(), o1 = next(), o2 = next(), o3 = next();
        const auto a0 = load(o0), a1 = load(o1), a2 = load(o2), a3 = load(o3);
        use(a0); use(a1); use(a2); use(a3);
    }
    for (; u < end; u += 256u) use(load(next()));
}

template <int VEC> struct Unit { float v[VEC]; };
template <int VEC>
__device__ __forceinline__ Unit<VEC> load_unit(const float* __restrict__ p, size_t unit) {
    Unit<VEC> r;
    if constexpr (VEC == 4) {
        const float4 q = reinterpret_cast<const float4*>(p)[unit];
        r.v[0] = q.x; r.v[1] = q.y; r.v[2] = q.z; r.v[3] = q.w;
    } else {
        r.v[0] = p[unit];
    }
    return r;
}
template <int VEC> struct UnitPair { Unit<VEC> x, g; };

template <int VEC>
__global__ void __launch_bounds__(256) bn_stats_l(const float* __restrict__ x, float4* partial, int* tickets, float* save_mean,
                                                  float* save_rstd, float* running_mean, float* running_var, BnP p) {
    __shared__ Stat lds4[4];
    __shared__ int last_flag;
    const unsigned c = blockIdx.x, s = blockIdx.y;
    const unsigned total = p.N * p.Lu, begin = s * p.chunk;
    const unsigned end = begin + p.chunk < total ? begin + p.chunk : total;
    const bool relu = p.relu_x != 0;
    float k = 0.0f, s1 = 0.0f, s2 = 0.0f, cnt = 0.0f;
    bool first = true;
    walk_channel(p, c, begin, end, [&](size_t unit) { return load_unit<VEC>(x, unit); }, [&](Unit<VEC> a) {
#pragma unroll
        for (int e = 0; e < VEC; ++e) {
            const float v = relu ? relu_keep_nan(a.v[e]) : a.v[e];
            if (first) { k = v; first = false; }
            const float d = v - k;
            s1 += d; s2 += d * d;
        }
        cnt += float(VEC);
    });
    Stat t = block_merge(shifted_to_stat(cnt, k, s1, s2), lds4);
    if (p.slices > 1) {
        if (threadIdx.x == 0) handoff::publish<float>(partial + size_t(c) * p.slices + s, t);
        if (!handoff::arrive_workgroup(tickets + size_t(c) * p.tstride, int(p.slices), &last_flag)) return;
        Stat mine{0.0f, 0.0f, 0.0f};
        if (threadIdx.x < p.slices) mine = handoff::fetch<Stat, float>(partial + size_t(c) * p.slices + threadIdx.x);
        t = block_merge(mine, lds4);
    }
    if (threadIdx.x == 0) finish_channel(t, c, p, save_mean, save_rstd, running_mean, running_var);
}

template <int VEC>
__global__ void __launch_bounds__(256) bn_sums_l(const float* __restrict__ g, const float* __restrict__ x, const float* __restrict__ save_mean,
                                                 const float* __restrict__ save_rstd, float4* partial, int* tickets, float* sums, float* dw,
                                                 float* db, BnP p) {
    __shared__ Pair lds4[4];
    __shared__ int last_flag;
    const unsigned c = blockIdx.x, s = blockIdx.y;
    const unsigned total = p.N * p.Lu, begin = s * p.chunk;
    const unsigned end = begin + p.chunk < total ? begin + p.chunk : total;
    const bool relu = p.relu_x != 0;
    const float mean = save_mean[c], rstd = save_rstd[c];
    float sg = 0.0f, sgx = 0.0f;
    walk_channel(p, c, begin, end, [&](size_t unit) { return UnitPair<VEC>{load_unit<VEC>(x, unit), load_unit<VEC>(g, unit)}; },
                 [&](UnitPair<VEC> a) {
#pragma unroll
        for (int e = 0; e < VEC; ++e) {
            const float v = relu ? relu_keep_nan(a.x.v[e]) : a.x.v[e];
            sg += a.g.v[e];
            sgx += a.g.v[e] * ((v - mean) * rstd);
        }
    });
    Pair t = block_merge(Pair{sg, sgx}, lds4);
    if (p.slices > 1) {
        if (threadIdx.x == 0) handoff::publish<float>(partial + size_t(c) * p.slices + s, t);
        if (!handoff::arrive_workgroup(tickets + size_t(c) * p.tstride, int(p.slices), &last_flag)) return;
        Pair mine{0.0f, 0.0f};
        if (threadIdx.x < p.slices) mine = handoff::fetch<Pair, float>(partial + size_t(c) * p.slices + threadIdx.x);
        t = block_merge(mine, lds4);
    }
    if (threadIdx.x == 0) {
        sums[2 * c] = t.a; sums[2 * c + 1] = t.b;
        if (db != nullptr) db[c] = t.a;
        if (dw != nullptr) dw[c] = t.b;
    }
}

// ---- form 1: L == 1, lanes across channels ---------------------------------------------------------------------------------
// the fold of form 1: wave w of the last arriver merges slices [w*q, (w+1)*q) of its lane's channel in order, then the four in order
template <typename T, typename Fetch>
__device__ __forceinline__ T fold_slices_cl(T zero, unsigned slices, T (*lds)[64], Fetch&& fetch) {
    const unsigned lane = threadIdx.x & 63, wave = threadIdx.x >> 6, q = (slices + 3) / 4;
    T acc = zero;
    const unsigned hi = (wave + 1) * q < slices ? (wave + 1) * q : slices;
    unsigned s = wave * q;
    for (; s + 3 < hi; s += 4) {                                   // four slices' partials in flight (their loads cross XCDs)
        const T a0 = fetch(s, lane), a1 = fetch(s + 1, lane), a2 = fetch(s + 2, lane), a3 = fetch(s + 3, lane);
        acc = merge(merge(merge(merge(acc, a0), a1), a2), a3);
    }
    for (; s < hi; ++s) acc = merge(acc, fetch(s, lane));
    __syncthreads();
    lds[wave][lane] = acc;
    __syncthreads();
    return merge(merge(lds[0][lane], lds[1][lane]), merge(lds[2][lane], lds[3][lane]));
}

__global__ void __launch_bounds__(256) bn_stats_c(const float* __restrict__ x, float4* partial, int* tickets, float* save_mean,
                                                  float* save_rstd, float* running_mean, float* running_var, BnP p) {
    __shared__ Stat lds[4][64];
    __shared__ int last_flag;
    const unsigned lane = threadIdx.x & 63, wave = threadIdx.x >> 6, s = blockIdx.y;
    const unsigned c_raw = blockIdx.x * 64 + lane;
    const bool live = c_raw < p.C;
    const unsigned c = live ? c_raw : p.C - 1;                    // idle lanes of the last block recompute a valid channel
    const unsigned begin = s * p.chunk, end = begin + p.chunk < p.N ? begin + p.chunk : p.N;
    const bool relu = p.relu_x != 0;
    float k = 0.0f, s1 = 0.0f, s2 = 0.0f, cnt = 0.0f;
    unsigned r = begin + wave;
    bool first = true;
    auto use = [&](float v) {
        if (relu) v = relu_keep_nan(v);
        if (first) { k = v; first = false; }
        const float d = v - k;
        s1 += d; s2 += d * d; cnt += 1.0f;
    };
    for (; r + 12 < end; r += 16) {                                // four rows in flight
        const float v0 = x[size_t(r) * p.C + c], v1 = x[size_t(r + 4) * p.C + c], v2 = x[size_t(r + 8) * p.C + c],
                    v3 = x[size_t(r + 12) * p.C + c];
        use(v0); use(v1); use(v2); use(v3);
    }
    for (; r < end; r += 4) use(x[size_t(r) * p.C + c]);
    lds[wave][lane] = shifted_to_stat(cnt, k, s1, s2);
    __syncthreads();
    Stat t = merge(merge(lds[0][lane], lds[1][lane]), merge(lds[2][lane], lds[3][lane]));
    if (p.slices > 1) {
        float4* mine = partial + size_t(blockIdx.x) * p.slices * 64;
        if (wave == 0) handoff::publish<float>(mine + s * 64 + lane, t);
        if (!handoff::arrive_workgroup(tickets + size_t(blockIdx.x) * p.tstride, int(p.slices), &last_flag)) return;
        t = fold_slices_cl(Stat{0.0f, 0.0f, 0.0f}, p.slices, lds, [&](unsigned sl, unsigned ln) { return handoff::fetch<Stat, float>(mine + sl * 64 + ln); });
    }
    if (wave == 0 && live) finish_channel(t, c, p, save_mean, save_rstd, running_mean, running_var);
}

__global__ void __launch_bounds__(256) bn_sums_c(const float* __restrict__ g, const float* __restrict__ x, const float* __restrict__ save_mean,
                                                 const float* __restrict__ save_rstd, float4* partial, int* tickets, float* sums, float* dw,
                                                 float* db, BnP p) {
    __shared__ Pair lds[4][64];
    __shared__ int last_flag;
    const unsigned lane = threadIdx.x & 63, wave = threadIdx.x >> 6, s = blockIdx.y;
    const unsigned c_raw = blockIdx.x * 64 + lane;
    const bool live = c_raw < p.C;
    const unsigned c = live ? c_raw : p.C - 1;
    const unsigned begin = s * p.chunk, end = begin + p.chunk < p.N ? begin + p.chunk : p.N;
    const bool relu = p.relu_x != 0;
    const float mean = save_mean[c], rstd = save_rstd[c];
    float sg = 0.0f, sgx = 0.0f;
    auto use = [&](float v, float d) {
        if (relu) v = relu_keep_nan(v);
        sg += d;
        sgx += d * ((v - mean) * rstd);
    };
    unsigned r = begin + wave;
    for (; r + 12 < end; r += 16) {                                // four rows of both tensors in flight
        const size_t o0 = size_t(r) * p.C + c, o1 = size_t(r + 4) * p.C + c, o2 = size_t(r + 8) * p.C + c, o3 = size_t(r + 12) * p.C + c;
        const float v0 = x[o0], v1 = x[o1], v2 = x[o2], v3 = x[o3], d0 = g[o0], d1 = g[o1], d2 = g[o2], d3 = g[o3];
        use(v0, d0); use(v1, d1); use(v2, d2); use(v3, d3);
    }
    for (; r < end; r += 4) use(x[size_t(r) * p.C + c], g[size_t(r) * p.C + c]);
    lds[wave][lane] = Pair{sg, sgx};
    __syncthreads();
    Pair t = merge(merge(lds[0][lane], lds[1][lane]), merge(lds[2][lane], lds[3][lane]));
    if (p.slices > 1) {
        float4* mine = partial + size_t(blockIdx.x) * p.slices * 64;
        if (wave == 0) handoff::publish<float>(mine + s * 64 + lane, t);
        if (!handoff::arrive_workgroup(tickets + size_t(blockIdx.x) * p.tstride, int(p.slices), &last_flag)) return;
        t = fold_slices_cl(Pair{0.0f, 0.0f}, p.slices, lds, [&](unsigned sl, unsigned ln) { return handoff::fetch<Pair, float>(mine + sl * 64 + ln); });
    }
    if (wave == 0 && live) {
        sums[2 * c] = t.a; sums[2 * c + 1] = t.b;
        if (db != nullptr) db[c] = t.a;
        if (dw != nullptr) dw[c] = t.b;
    }
}

// ---- the elementwise launches ------------------------------------------------------------------------------------------------
// One unit (VEC floats) per thread.  CVEC: L == 1 and the four floats of a unit are four neighbouring channels; otherwise a unit
// lies inside one row of L and has one channel.
enum { BN_APPLY = 0, BN_INFER = 1, BN_DX = 2 };

struct BnE {
    unsigned units, C, Lu;
    float eps, inv_count;
    int relu_x;
};

template <int KIND>
__device__ __forceinline__ float bn_element(float x, float g, float mean, float rstd, float w, float b, float sg, float sgx, float inv_count) {
    if constexpr (KIND == BN_DX) return (w * rstd) * ((g - sg * inv_count) - ((x - mean) * rstd) * (sgx * inv_count));
    else return (x - mean) * (rstd * w) + b;
}

// a: save_mean (BN_APPLY, BN_DX) or running_mean (BN_INFER); r: save_rstd or running_var
template <int KIND, int VEC, bool CVEC>
__global__ void __launch_bounds__(256) bn_elementwise(const float* __restrict__ x, const float* __restrict__ g, const float* __restrict__ w,
                                                      const float* __restrict__ b, const float* __restrict__ a, const float* __restrict__ r,
                                                      const float* __restrict__ sums, float* __restrict__ out, BnE p) {
    const bool relu = p.relu_x != 0;
    for (unsigned u = blockIdx.x * 256u + threadIdx.x; u < p.units; u += gridDim.x * 256u) {
        float xv[VEC], gv[VEC], ov[VEC];
        if constexpr (VEC == 4) {
            const float4 q = reinterpret_cast<const float4*>(x)[u];
            xv[0] = q.x; xv[1] = q.y; xv[2] = q.z; xv[3] = q.w;
            if constexpr (KIND == BN_DX) {
                const float4 t = reinterpret_cast<const float4*>(g)[u];
                gv[0] = t.x; gv[1] = t.y; gv[2] = t.z; gv[3] = t.w;
            }
        } else {
            xv[0] = x[u];
            if constexpr (KIND == BN_DX) gv[0] = g[u];
        }
        unsigned c0;
        if constexpr (CVEC) c0 = (u % (p.C / 4)) * 4;
        else c0 = (u / p.Lu) % p.C;
#pragma unroll
        for (int e = 0; e < VEC; ++e) {
            const unsigned c = CVEC ? c0 + e : c0;
            const float mean = a[c];
            const float rstd = KIND == BN_INFER ? 1.0f / sqrtf(r[c] + p.eps) : r[c];
            const float wc = w != nullptr ? w[c] : 1.0f, bc = (KIND != BN_DX && b != nullptr) ? b[c] : 0.0f;
            float sg = 0.0f, sgx = 0.0f;
            if constexpr (KIND == BN_DX) { sg = sums[2 * c]; sgx = sums[2 * c + 1]; }
            const float v = relu ? relu_keep_nan(xv[e]) : xv[e];
            ov[e] = bn_element<KIND>(v, KIND == BN_DX ? gv[e] : 0.0f, mean, rstd, wc, bc, sg, sgx, p.inv_count);
        }
        if constexpr (VEC == 4) reinterpret_cast<float4*>(out)[u] = make_float4(ov[0], ov[1], ov[2], ov[3]);
        else out[u] = ov[0];
    }
}

static thread_local int32_t g_bn_plan[4] = {-1, 0, 0, 0};

struct BnGeom {
    int64_t N, C, L, numel;
    int form;                   // 0 lanes along L, 1 lanes across channels (L == 1)
    int64_t slices, chunk, groups_x;
};

// the plan rule, a function of the shape (and of whether 16-byte units can be used) alone
static int bn_geometry(const char* who, int64_t N, int64_t C, int64_t L, bool training, int vec, BnGeom& o) {
    LG_ARG(N >= 1 && C >= 1 && L >= 1, "%s: every extent must be at least 1", who);
    LG_ARG(N < (int64_t(1) << 31) && C < (int64_t(1) << 31) && L < (int64_t(1) << 31) && N * C < (int64_t(1) << 31) &&
           N * C * L < (int64_t(1) << 31), "%s: at most 2^31 - 1 elements", who);
    LG_ARG(!training || N * L >= 2, "%s: batch statistics need at least 2 values per channel (N * L is %lld)", who, (long long)(N * L));
    o.N = N; o.C = C; o.L = L; o.numel = N * C * L;
    o.form = L == 1 ? 1 : 0;
    o.groups_x = o.form == 1 ? (C + 63) / 64 : C;
    LG_ARG(o.groups_x <= rt().n_tickets, "%s: %lld channels are more than the ticket pool holds", who, (long long)C);
    int64_t slices = (kBnTargetGroups + o.groups_x - 1) / o.groups_x;
    if (o.form == 0) {
        const int64_t units = N * (L / vec);
        if (slices > kBnMaxSlices) slices = kBnMaxSlices;
        if (slices * kBnMinUnits > units) slices = (units + kBnMinUnits - 1) / kBnMinUnits;
        if (slices < 1) slices = 1;
        o.chunk = (units + slices - 1) / slices;
        o.slices = (units + o.chunk - 1) / o.chunk;
    } else {
        if (slices > kBnMaxSlicesCl) slices = kBnMaxSlicesCl;
        if (slices * kBnMinRows > N) slices = N / kBnMinRows;
        if (slices < 1) slices = 1;
        o.chunk = (N + slices - 1) / slices;
        o.slices = (N + o.chunk - 1) / o.chunk;
    }
    return LG_OK;
}

static BnP bn_params(const BnGeom& g, int vec, float eps, float momentum, int relu_x) {
    BnP p;
    p.N = unsigned(g.N); p.C = unsigned(g.C); p.Lu = unsigned(g.L / vec);
    p.chunk = unsigned(g.chunk); p.slices = unsigned(g.slices);
    p.tstride = unsigned(ticket_stride(g.groups_x));
    const double count = double(g.N) * double(g.L);
    p.count = float(count); p.eps = eps; p.momentum = momentum;
    p.unbias = count > 1.0 ? float(count / (count - 1.0)) : 1.0f;
    p.relu_x = relu_x ? 1 : 0;
    return p;
}

static int bn_partials(const BnGeom& g, float4** partial) {
    *partial = nullptr;
    if (g.slices <= 1) return LG_OK;
    const size_t slots = size_t(g.groups_x) * size_t(g.slices) * (g.form == 1 ? 64 : 1);
    return lg_malloc(reinterpret_cast<void**>(partial), slots * sizeof(float4));
}

template <int KIND>
static void launch_elementwise(int vec, bool cvec, const float* x, const float* g, const float* w, const float* b, const float* a,
                               const float* r, const float* sums, float* out, const BnGeom& geo, float eps, int relu_x) {
    BnE e;
    e.units = unsigned(geo.numel / vec); e.C = unsigned(geo.C); e.Lu = unsigned(cvec ? 1 : geo.L / vec);
    e.eps = eps; e.inv_count = float(1.0 / (double(geo.N) * double(geo.L))); e.relu_x = relu_x ? 1 : 0;
    const dim3 grid(stream_grid(e.units));
    if (vec == 4 && cvec) hipLaunchKernelGGL((bn_elementwise<KIND, 4, true>), grid, dim3(256), 0, rt().stream, x, g, w, b, a, r, sums, out, e);
    else if (vec == 4) hipLaunchKernelGGL((bn_elementwise<KIND, 4, false>), grid, dim3(256), 0, rt().stream, x, g, w, b, a, r, sums, out, e);
    else hipLaunchKernelGGL((bn_elementwise<KIND, 1, false>), grid, dim3(256), 0, rt().stream, x, g, w, b, a, r, sums, out, e);
}

// 16-byte units: along L when L is a multiple of 4, across channels when L == 1 and C is one; every tensor pointer aligned
static int bn_vec(int64_t C, int64_t L, const void* p0, const void* p1, const void* p2) {
    const bool aligned = aligned16(p0) && (p1 == nullptr || aligned16(p1)) && (p2 == nullptr || aligned16(p2));
    if (!aligned) return 1;
    if (L > 1) return L % 4 == 0 ? 4 : 1;
    return C % 4 == 0 ? 4 : 1;
}

static void note_bn_plan(int kernel, int form, int64_t slices, int relu_x) {
    g_bn_plan[0] = kernel; g_bn_plan[1] = form; g_bn_plan[2] = int32_t(slices); g_bn_plan[3] = relu_x ? 1 : 0;
}

}  // namespace lg

using namespace lg;

extern "C" int lg_batchnorm_fwd_f32(const float* x, const float* w, const float* b, float* y, float* save_mean, float* save_rstd,
                                    float* running_mean, float* running_var, int64_t N, int64_t C, int64_t L, float eps, float momentum,
                                    int relu_x) {
    LG_REQUIRE_INIT();
    LG_ARG(x != nullptr && y != nullptr && save_mean != nullptr && save_rstd != nullptr, "lg_batchnorm_fwd_f32: NULL pointer");
    LG_ARG(eps >= 0.0f && momentum > 0.0f && momentum <= 1.0f, "lg_batchnorm_fwd_f32: eps must not be negative and momentum must lie in (0, 1]");
    // the stats launch reads x alone: its units follow x; the apply launch also writes y
    const int vec_stats = L > 1 ? bn_vec(C, L, x, nullptr, nullptr) : 1;
    BnGeom geo;
    int rc = bn_geometry("lg_batchnorm_fwd_f32", N, C, L, true, vec_stats, geo);
    if (rc != LG_OK) return rc;
    rc = adam_epilogue_check_write(y, geo.numel * int64_t(sizeof(float)));
    if (rc == LG_OK) rc = adam_epilogue_check_write(save_mean, C * int64_t(sizeof(float)));
    if (rc == LG_OK) rc = adam_epilogue_check_write(save_rstd, C * int64_t(sizeof(float)));
    if (rc == LG_OK) rc = adam_epilogue_check_write(running_mean, C * int64_t(sizeof(float)));
    if (rc == LG_OK) rc = adam_epilogue_check_write(running_var, C * int64_t(sizeof(float)));
    if (rc != LG_OK) return rc;
    float4* partial = nullptr;
    rc = bn_partials(geo, &partial);
    if (rc != LG_OK) return rc;
    const BnP p = bn_params(geo, vec_stats, eps, momentum, relu_x);
    const dim3 grid(unsigned(geo.groups_x), unsigned(geo.slices));
    if (geo.form == 1) hipLaunchKernelGGL(bn_stats_c, grid, dim3(256), 0, rt().stream, x, partial, rt().tickets, save_mean, save_rstd, running_mean, running_var, p);
    else if (vec_stats == 4) hipLaunchKernelGGL((bn_stats_l<4>), grid, dim3(256), 0, rt().stream, x, partial, rt().tickets, save_mean, save_rstd, running_mean, running_var, p);
    else hipLaunchKernelGGL((bn_stats_l<1>), grid, dim3(256), 0, rt().stream, x, partial, rt().tickets, save_mean, save_rstd, running_mean, running_var, p);
    hipError_t launched = hipGetLastError();
    if (partial != nullptr) {
        rc = lg_free(partial);                                          // stream-ordered: only later launches reuse the block
        if (rc != LG_OK) return rc;
    }
    if (launched == hipSuccess) {
        const int vec = bn_vec(C, L, x, y, nullptr);
        const bool cvec = L == 1 && vec == 4;
        launch_elementwise<BN_APPLY>((L == 1 && !cvec) ? 1 : vec, cvec, x, nullptr, w, b, save_mean, save_rstd, nullptr, y, geo, eps, relu_x);
        launched = hipGetLastError();
    }
    if (launched != hipSuccess) { set_error("lg_batchnorm_fwd_f32: kernel launch failed: %s", hipGetErrorString(launched)); return LG_EHIP; }
    note_bn_plan(0, geo.form, geo.slices, relu_x);
    return LG_OK;
}

extern "C" int lg_batchnorm_bwd_f32(const float* g, const float* x, const float* w, const float* save_mean, const float* save_rstd,
                                    float* dx, float* dw, float* db, int64_t N, int64_t C, int64_t L, int relu_x) {
    LG_REQUIRE_INIT();
    LG_ARG(g != nullptr && x != nullptr && save_mean != nullptr && save_rstd != nullptr, "lg_batchnorm_bwd_f32: NULL pointer");
    const int vec_sums = L > 1 ? bn_vec(C, L, x, g, nullptr) : 1;
    BnGeom geo;
    int rc = bn_geometry("lg_batchnorm_bwd_f32", N, C, L, false, vec_sums, geo);
    if (rc != LG_OK) return rc;
    rc = adam_epilogue_check_write(dx, geo.numel * int64_t(sizeof(float)));
    if (rc == LG_OK) rc = adam_epilogue_check_write(dw, C * int64_t(sizeof(float)));
    if (rc == LG_OK) rc = adam_epilogue_check_write(db, C * int64_t(sizeof(float)));
    if (rc != LG_OK) return rc;
    note_bn_plan(1, geo.form, geo.slices, relu_x);
    if (dx == nullptr && dw == nullptr && db == nullptr) return LG_OK;
    float* sums = nullptr;                                              // (sum g, sum g * xhat) per channel, for the dx launch
    rc = lg_malloc(reinterpret_cast<void**>(&sums), size_t(2 * C) * sizeof(float));
    if (rc != LG_OK) return rc;
    float4* partial = nullptr;
    rc = bn_partials(geo, &partial);
    if (rc != LG_OK) { (void)lg_free(sums); return rc; }
    const BnP p = bn_params(geo, vec_sums, 0.0f, 1.0f, relu_x);
    const dim3 grid(unsigned(geo.groups_x), unsigned(geo.slices));
    if (geo.form == 1) hipLaunchKernelGGL(bn_sums_c, grid, dim3(256), 0, rt().stream, g, x, save_mean, save_rstd, partial, rt().tickets, sums, dw, db, p);
    else if (vec_sums == 4) hipLaunchKernelGGL((bn_sums_l<4>), grid, dim3(256), 0, rt().stream, g, x, save_mean, save_rstd, partial, rt().tickets, sums, dw, db, p);
    else hipLaunchKernelGGL((bn_sums_l<1>), grid, dim3(256), 0, rt().stream, g, x, save_mean, save_rstd, partial, rt().tickets, sums, dw, db, p);
    hipError_t launched = hipGetLastError();
    if (launched == hipSuccess && dx != nullptr) {
        const int vec = bn_vec(C, L, x, g, dx);
        const bool cvec = L == 1 && vec == 4;
        launch_elementwise<BN_DX>((L == 1 && !cvec) ? 1 : vec, cvec, x, g, w, nullptr, save_mean, save_rstd, sums, dx, geo, 0.0f, relu_x);
        launched = hipGetLastError();
    }
    rc = lg_free(sums);
    if (partial != nullptr) {
        const int rc2 = lg_free(partial);
        if (rc == LG_OK) rc = rc2;
    }
    if (rc != LG_OK) return rc;
    if (launched != hipSuccess) { set_error("lg_batchnorm_bwd_f32: kernel launch failed: %s", hipGetErrorString(launched)); return LG_EHIP; }
    return LG_OK;
}

extern "C" int lg_batchnorm_infer_f32(const float* x, const float* w, const float* b, const float* running_mean, const float* running_var,
                                      float* y, int64_t N, int64_t C, int64_t L, float eps, int relu_x) {
    LG_REQUIRE_INIT();
    LG_ARG(x != nullptr && y != nullptr && running_mean != nullptr && running_var != nullptr, "lg_batchnorm_infer_f32: NULL pointer");
    LG_ARG(eps >= 0.0f, "lg_batchnorm_infer_f32: eps must not be negative");
    BnGeom geo;
    int rc = bn_geometry("lg_batchnorm_infer_f32", N, C, L, false, 1, geo);
    if (rc != LG_OK) return rc;
    rc = adam_epilogue_check_write(y, geo.numel * int64_t(sizeof(float)));
    if (rc != LG_OK) return rc;
    const int vec = bn_vec(C, L, x, y, nullptr);
    const bool cvec = L == 1 && vec == 4;
    launch_elementwise<BN_INFER>((L == 1 && !cvec) ? 1 : vec, cvec, x, nullptr, w, b, running_mean, running_var, nullptr, y, geo, eps, relu_x);
    LG_CHECK_LAUNCH();
    note_bn_plan(2, geo.form, 1, relu_x);
    return LG_OK;
}

extern "C" int lg_batchnorm_last_plan(int32_t out[4]) {
    LG_ARG(out != nullptr, "lg_batchnorm_last_plan: NULL pointer");
    for (int i = 0; i < 4; ++i) out[i] = g_bn_plan[i];
    return LG_OK;
}
