// What attention.hip (S <= 128: a (batch, head) pair lives in LDS) and attention_long.hip (129 .. 512: chunks stream through
// LDS) share: the kernels' argument structs and small device helpers, and the ONE host path behind the eight lg_attention_*
// launch entries and the causal forward entry - a call struct per direction, a descriptor per entry family, attn_forward /
// attn_backward (attention.hip).
#pragma once
#include "common.h"
#include "mfma_lds.h"
#include "rng_common.h"
#include <cmath>
#include <type_traits>

namespace lg {

#ifdef LG_GEMM_TIMELINE
// experiments build only (make timeline; tools/attn_timeline.py): 16 timestamps of the 100 MHz wall clock per workgroup
#define LG_ATL(slot) do { if (a.tl && threadIdx.x == 0) a.tl[size_t((blockIdx.z * gridDim.y + blockIdx.y) * gridDim.x + blockIdx.x) * 16 + (slot)] = wall_clock64(); } while (0)
#define LG_ATL_FIELD unsigned long long* tl;
#else
#define LG_ATL(slot) do { } while (0)
#define LG_ATL_FIELD
#endif

// ---- kernel arguments ------------------------------------------------------------------------------------------------------
// The forward arguments are AttnTailArgs for every kernel but the plain attn_fwd<D> (no mask, S % 32 == 0), which takes the
// base without the two mask fields: its kernarg segment stays the 128 bytes it was.  A launcher passes the most derived struct
// and the call slices it to what the instantiation takes.
struct AttnArgs {
    LG_ATL_FIELD
    const float *q, *k, *v;          // element (b, s, head, d) of X at X + b * sbX + s * ldX + head * D + d
    int64_t ldq, sbq, ldk, sbk, ldv, sbv;
    float* o;                        // context, same addressing
    int64_t ldo, sbo;
    float* p;                        // probabilities (batch, heads, S, S), dense
    int S, heads;
    float scale;
};

struct AttnTailArgs : AttnArgs {
    const float* mask;               // key-padding mask, element (b, j) at mask + b * sbm + j (sbm = 0: one row for the batch); NULL = none
    int64_t sbm;
};

struct AttnBwdArgs {
    LG_ATL_FIELD
    const float *q, *k, *v, *g;      // g = gradient of the context; addressing as in AttnArgs
    int64_t ldq, sbq, ldk, sbk, ldv, sbv, ldg, sbg;
    const float* p;                  // probabilities saved by the forward
    float *dq, *dk, *dv;
    int64_t lddq, sbdq, lddk, sbdk, lddv, sbdv;
    int S, heads, batch;
    float scale;
    double* shift;                   // [batch, heads, Sp]: the softmax shift of every query row, query role -> key role
    int*    flags;                   // [batch * heads][2]: rows published / key-role workgroups served; zero between launches
    int*    status;                  // device status flag (a wait that gives up raises it)
};

// DROP instantiations: the same arguments (mask NULL for none) and the call of the random stream (rng_common.h)
struct AttnDropArgs : AttnTailArgs {
    AttnDrop drop;
};
struct AttnBwdDropArgs : AttnBwdArgs {
    AttnDrop drop;
};

// ---- device helpers --------------------------------------------------------------------------------------------------------
__host__ __device__ constexpr int round32(int S) { return (S + 31) & ~31; }

// the two 64-bit words of a call in LDS (DROP instantiations only: 16 bytes of static LDS next to the dynamic tiles)
template <bool DROP>
__device__ __forceinline__ unsigned long long* rng_call_slot() {
    if constexpr (DROP) {
        __shared__ unsigned long long call[2];
        return call;
    } else {
        return nullptr;
    }
}

// linear index of this workgroup over the 3-D grid / workgroups of the launch: what the tickets of the random stream count
__device__ __forceinline__ int grid_linear_block() { return int((blockIdx.z * gridDim.y + blockIdx.y) * gridDim.x + blockIdx.x); }
__device__ __forceinline__ int grid_blocks() { return int(gridDim.x * gridDim.y * gridDim.z); }

// a float4 at flat element index i of the dense (batch, heads, S, S) tensor under the mask of the call: x * s where the stream
// keeps the element, +0.0 where it drops it (ALIGNED: S % 4 == 0, the float4 is one group of the stream; else the four words
// can come from two groups)
template <bool ALIGNED>
__device__ __forceinline__ af32x4 drop4(af32x4 t, int64_t i, unsigned long long seed, unsigned long long base, uint32_t threshold, float s) {
    uint32_t w[4];
    rng_words4<ALIGNED>(i, seed, base, w);
    return af32x4{rng_keep(t[0], w[0], threshold, s), rng_keep(t[1], w[1], threshold, s), rng_keep(t[2], w[2], threshold, s),
                  rng_keep(t[3], w[3], threshold, s)};
}

// store_rows that also clears rows [rows, padded): an MFMA operand row past the sequence must be zero, not stale LDS
template <int D, int N>
__device__ __forceinline__ void store_rows_padded(const af32x4 (&v)[N], float* dst, int pitch, int rows, int padded) {
    constexpr int Q = D / 4;
#pragma unroll
    for (int i = 0; i < N; ++i) {
        const int f = threadIdx.x + i * 256;
        if (f < padded * Q) {
            af32x4 t = v[i];
            if (f >= rows * Q) t = af32x4{0.f, 0.f, 0.f, 0.f};
            *reinterpret_cast<af32x4*>(dst + (f / Q) * pitch + (f % Q) * 4) = t;
        }
    }
}

// ---- host side -------------------------------------------------------------------------------------------------------------
template <class K>
static int allow_lds(K kernel, size_t bytes) {
    hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize, int(bytes));
    if (e != hipSuccess) { set_error("attention: %zu bytes of LDS refused: %s", bytes, hipGetErrorString(e)); return LG_EHIP; }
    return LG_OK;
}

// an operand of a call: element (b, s, head, d) at x + b * sb + s * ld + head * D + d
struct AttnIn  { const float* x; int64_t ld, sb; };
struct AttnOut { float* x; int64_t ld, sb; };

struct AttnFwdCall {
    AttnIn q, k, v;
    AttnOut o;
    float* p;
    int64_t batch, heads, S, D;
    float scale;
    const float* mask;               // NULL: none (always, for the family that takes none)
    int64_t sbm;
    double prob;                     // dropout family only
    uint64_t* base;                  // dropout family only: the call's number, written by the launch
};

struct AttnBwdCall {
    AttnIn q, k, v, g;
    const float* p;
    AttnOut dq, dk, dv;
    int64_t batch, heads, S, D;
    float scale;
    double prob;                     // dropout family only
    const uint64_t* base;            // dropout family only: what the forward wrote
};

// which kernels run a call
enum class AttnForm {
    Plain,                           // attn_fwd / attn_bwd, TAIL = false
    Tail,                            // attn_fwd / attn_bwd, TAIL = true: any S <= 128, a mask or none
    Long,                            // attn_long_fwd / attn_long_bwd
    ByLength                         // the dropout family: Long beyond 128, else Plain where the plain kernels can, else Tail
};

// what differs between the entry families (plain, masked, long, dropout; causal: a forward only)
struct AttnFamily {
    const char* fwd;                 // the entry points' names, for messages
    const char* bwd;
    int (*supported)(int64_t S, int64_t D);
    const char* range;               // the lengths `supported` takes, for the message of a refusal
    AttnForm form;                   // Plain takes no mask
    bool causal = false;             // the causal forward entry: the CAUSAL instantiations by length, DROP where the call has a base_out
    bool dropout() const { return form == AttnForm::ByLength && !causal; }      // the DROP instantiations, and the checks only they need
};

// the one path behind the launch entries (attention.hip): checks in their fixed order, arguments, launch
int attn_forward(const AttnFamily& f, const AttnFwdCall& c);
int attn_backward(const AttnFamily& f, const AttnBwdCall& c);

// attention_long.hip: the launches of its kernels (arguments checked, `shift` allocated; the caller checks the launch)
int attn_long_launch_fwd(const AttnDropArgs& a, dim3 grid, int64_t D, bool drop, bool causal = false);
int attn_long_launch_bwd(const AttnBwdDropArgs& a, dim3 grid, int64_t D, bool drop);

}  // namespace lg
