// BERT's token masking for the masked-LM objective, from the counter-based random stream of dropout.hip (C ABI and definition:
// include/lghip.h, lightgrad_amd/random.py `mlm_mask_words`).
//
// One call of the stream per launch, one element per thread, one Philox call each: for call number b, element i (flat index)
// takes the whole block  w = philox4x32_10((lo32(i), hi32(i), lo32(b), hi32(b)), key(seed)):
//   selected  iff ids[i] is none of the special ids and w[0] < T(p)             (T: the dropout threshold)
//   not selected:  masked = ids[i], label = ignore_index
//   selected:      label = ids[i];  w[1] < floor(0.8 * 2^32): masked = mask_token_id
//                                   w[1] < floor(0.9 * 2^32): masked = (uint64(w[2]) * vocab_size) >> 32     (a uniform token)
//                                   otherwise:                masked = ids[i]
// Seed and `draws` are read by the kernel with dropout_fwd's protocol (read, two-level tickets, the last arriver advances), so a
// captured training step masks a fresh batch at every replay.  Integer work: the numpy backend gives the same bits.
#include "common.h"
#include "rng_common.h"

namespace lg {

constexpr int kMlmMaxSpecial = 8;
constexpr uint32_t kMlmMaskBelow = 3435973836u;        // floor(0.8 * 2^32)
constexpr uint32_t kMlmRandomBelow = 3865470566u;      // floor(0.9 * 2^32)
constexpr int64_t kMlmMaxElements = int64_t(kRngMaxGroup) * kRngMaxGroup * 256;     // one element per thread

struct MlmSpecials {
    int64_t id[kMlmMaxSpecial];
    int n;
};

template <typename IdT>
__global__ void __launch_bounds__(256) mlm_mask_kernel(const IdT* __restrict__ ids, IdT* __restrict__ masked, IdT* __restrict__ labels,
                                                       int64_t n, uint32_t threshold, int64_t mask_token, uint64_t vocab, MlmSpecials special,
                                                       int64_t ignore, unsigned long long* state, unsigned long long* base_out, int group) {
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

    const int64_t i = int64_t(blockIdx.x) * 256 + threadIdx.x;
    if (i < n) {
        uint32_t w[4];
        philox4x32_10(uint32_t(i), uint32_t(uint64_t(i) >> 32), uint32_t(base), uint32_t(base >> 32), uint32_t(seed), uint32_t(seed >> 32), w);
        const IdT id = ids[i];
        bool selected = w[0] < threshold;
#pragma unroll
        for (int k = 0; k < kMlmMaxSpecial; ++k) selected = selected && !(k < special.n && int64_t(id) == special.id[k]);
        IdT out = id;
        if (selected && w[1] < kMlmRandomBelow)
            out = w[1] < kMlmMaskBelow ? IdT(mask_token) : IdT((uint64_t(w[2]) * vocab) >> 32);
        masked[i] = out;
        labels[i] = selected ? id : IdT(ignore);
    }

    if (threadIdx.x == 0) rng_last_arriver_advances(state, tickets, mine, order, grp, groups, group, int(gridDim.x), base);
}

static bool fits(int64_t v, int itemsize) { return itemsize == 8 || (v >= INT32_MIN && v <= INT32_MAX); }

}  // namespace lg

using namespace lg;

extern "C" int lg_mlm_mask(const void* ids, int itemsize, void* masked, void* labels, int64_t n, double p, int64_t mask_token_id,
                           int64_t vocab_size, const int64_t* special_ids, int n_special, int64_t ignore_index, uint64_t* base_out) {
    LG_REQUIRE_INIT();
    LG_ARG(itemsize == 4 || itemsize == 8, "lg_mlm_mask: ids must be int32/int64");
    LG_ARG(n >= 0 && n <= kMlmMaxElements, "lg_mlm_mask: n = %lld outside [0, 2^32]", (long long)n);
    LG_ARG(base_out != nullptr && (n == 0 || (ids != nullptr && masked != nullptr && labels != nullptr)), "lg_mlm_mask: NULL pointer");
    LG_ARG(p >= 0.0 && p < 1.0, "lg_mlm_mask: p = %g outside [0, 1)", p);
    LG_ARG(vocab_size >= 1 && vocab_size <= (int64_t(1) << 31), "lg_mlm_mask: vocab_size = %lld outside [1, 2^31]", (long long)vocab_size);
    LG_ARG(n_special >= 0 && n_special <= kMlmMaxSpecial && (n_special == 0 || special_ids != nullptr),
           "lg_mlm_mask: at most %d special ids (got %d)", kMlmMaxSpecial, n_special);
    LG_ARG(fits(mask_token_id, itemsize) && fits(ignore_index, itemsize), "lg_mlm_mask: mask_token_id / ignore_index do not fit the ids' type");
    LG_ARG(n == 0 || (masked != ids && labels != ids && masked != labels), "lg_mlm_mask: the outputs may alias neither the ids nor each other");
    { const int rc = adam_epilogue_check_write(masked, n * itemsize); if (rc != LG_OK) return rc; }
    { const int rc = adam_epilogue_check_write(labels, n * itemsize); if (rc != LG_OK) return rc; }
    uint32_t threshold;
    float unused;
    rng_threshold(p, threshold, unused);
    MlmSpecials special;
    for (int k = 0; k < kMlmMaxSpecial; ++k) special.id[k] = k < n_special ? special_ids[k] : 0;       // by value: host memory, read now
    special.n = n_special;
    const int64_t need = (n + 255) / 256;
    const dim3 grid(unsigned(need < 1 ? 1 : need)), block(256);      // an empty call still launches one workgroup, which advances `draws`
    unsigned long long* const state = rt().rng_state;
    unsigned long long* const out = reinterpret_cast<unsigned long long*>(base_out);
    const int group = rng_group(grid.x);
    if (itemsize == 4)
        hipLaunchKernelGGL(mlm_mask_kernel<int32_t>, grid, block, 0, rt().stream, static_cast<const int32_t*>(ids), static_cast<int32_t*>(masked),
                           static_cast<int32_t*>(labels), n, threshold, mask_token_id, uint64_t(vocab_size), special, ignore_index, state, out, group);
    else
        hipLaunchKernelGGL(mlm_mask_kernel<int64_t>, grid, block, 0, rt().stream, static_cast<const int64_t*>(ids), static_cast<int64_t*>(masked),
                           static_cast<int64_t*>(labels), n, threshold, mask_token_id, uint64_t(vocab_size), special, ignore_index, state, out, group);
    LG_CHECK_LAUNCH();
    return LG_OK;
}
