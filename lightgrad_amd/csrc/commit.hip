// The per-row bookkeeping of one decode step in ONE launch: lg_decode_commit_i32.
//
// A decode step of a batch whose sequences have their own positions ends with, per row r that is still live (done[r] == 0):
// the position moves on by one, the new token becomes the step's input token and column `position` of the row's ids, and a row
// whose new token is the end-of-sequence id is marked finished.  A finished row is not touched at all - its position, its
// token and its ids stay byte for byte - so the step keeps one shape whatever has finished (a captured step replays as it
// stands) while the row's recomputed attention rewrites the same cache row with the same bits.  As tensor expressions this is
// a compare, two selects, a masked add and a scatter - five launches; the launch boundaries are what a decode step is made of.
//
// One thread per row, any batch >= 1; nothing is shared between rows, so there is no fold and no order to fix.  A position
// outside the ids' columns writes nothing for that row and raises the status flag (LG_EINDEX at the next synchronisation).
#include "common.h"

namespace lg {

__global__ __launch_bounds__(256) void decode_commit(const int32_t* __restrict__ nxt, int64_t nxt_pitch, int32_t* __restrict__ token,
                                                     int32_t* __restrict__ out_ids, int64_t out_pitch, int columns,
                                                     int32_t* __restrict__ pos, int32_t* __restrict__ done, int batch, int32_t eos_id,
                                                     int* status) {
    const int r = blockIdx.x * 256 + threadIdx.x;
    if (r >= batch || done[r] != 0) return;
    const int64_t p = int64_t(pos[r]) + 1;
    if (p < 0 || p >= columns) {
        // a bounds check, never a fault: the row keeps its bytes, the next synchronising call reports LG_EINDEX
        __hip_atomic_fetch_or(status, LG_STATUS_BAD_INDEX, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
        return;
    }
    const int32_t id = nxt[int64_t(r) * nxt_pitch];
    pos[r] = int32_t(p);
    token[r] = id;
    out_ids[int64_t(r) * out_pitch + p] = id;
    if (eos_id >= 0 && id == eos_id) done[r] = 1;
}

}  // namespace lg

using namespace lg;

extern "C" int lg_decode_commit_i32(const int32_t* nxt, int64_t nxt_pitch, int32_t* token, int32_t* out_ids, int64_t out_pitch,
                                    int64_t columns, int32_t* pos, int32_t* done, int64_t batch, int32_t eos_id) {
    LG_REQUIRE_INIT();
    const char* name = "lg_decode_commit_i32";
    LG_ARG(batch >= 0 && batch < (int64_t(1) << 31) && columns >= 1 && columns < (int64_t(1) << 31), "%s: batch = %lld / columns = %lld outside [0, 2^31) / [1, 2^31)",
           name, (long long)batch, (long long)columns);
    if (batch == 0) return LG_OK;
    LG_ARG(nxt && token && out_ids && pos && done, "%s: NULL operand (a `done` word per row is required)", name);
    LG_ARG(((reinterpret_cast<uintptr_t>(nxt) | reinterpret_cast<uintptr_t>(token) | reinterpret_cast<uintptr_t>(out_ids) |
             reinterpret_cast<uintptr_t>(pos) | reinterpret_cast<uintptr_t>(done)) & 3u) == 0, "%s: operands must be 4-byte aligned", name);
    LG_ARG(nxt_pitch >= 1 && out_pitch >= columns, "%s: row pitches %lld (nxt, >= 1) / %lld (out_ids, >= columns = %lld)", name,
           (long long)nxt_pitch, (long long)out_pitch, (long long)columns);
    {
        // a thread writes its row of token, out_ids, pos and done: bytes shared by two operands would make a row's result depend on
        // which thread ran first
        const void* ptr[5] = {nxt, token, out_ids, pos, done};
        const int64_t bytes[5] = {((batch - 1) * nxt_pitch + 1) * 4, batch * 4, ((batch - 1) * out_pitch + columns) * 4, batch * 4, batch * 4};
        for (int i = 0; i < 5; ++i)
            for (int j = i + 1; j < 5; ++j)
                LG_ARG(!bytes_overlap(ptr[i], bytes[i], ptr[j], bytes[j]), "%s: operands %d and %d (of nxt, token, out_ids, pos, done) overlap", name, i, j);
        for (int i = 1; i < 5; ++i) { const int rc = adam_epilogue_check_write(ptr[i], bytes[i]); if (rc != LG_OK) return rc; }
    }
    hipLaunchKernelGGL(decode_commit, dim3(unsigned((batch + 255) / 256)), dim3(256), 0, rt().stream, nxt, nxt_pitch, token, out_ids, out_pitch,
                       int(columns), pos, done, int(batch), eos_id, rt().status_dev);
    LG_CHECK_LAUNCH();
    return LG_OK;
}
