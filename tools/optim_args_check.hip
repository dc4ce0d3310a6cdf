// Host-side argument handling of the multi-tensor optimizer launches (lightgrad_amd/csrc/adam_common.h: adam_segments_fill,
// adamw_recipe_fill - segment grouping, the copy of the decay flags, step-slot accounting) under AddressSanitizer / UBSan.
// A stand-alone program, CPU only: no device call is made and the library is never initialised.
//   hipcc -std=c++17 --offload-arch=gfx950 -Xarch_host -fsanitize=address,undefined -Xarch_host -fno-omit-frame-pointer \
//         tools/optim_args_check.hip -o optim_args_check -Llightgrad_amd -llghip -Wl,-rpath,$PWD/lightgrad_amd && ./optim_args_check
// The arrays handed in are heap blocks of EXACTLY the documented length, so a read past `offsets[nseg]` or `decay_flags[nseg - 1]`
// is a sanitizer report.
#include "../lightgrad_amd/csrc/adam_common.h"
#include <cstdio>
#include <cstdlib>
#include <vector>

using namespace lg;

static int failures = 0;
#define EXPECT(cond)                                                                   \
    do {                                                                               \
        if (!(cond)) { std::printf("FAILED line %d: %s\n", __LINE__, #cond); ++failures; } \
    } while (0)

// the loop of lg_adamw_multi_dev_f32 without the launches
static int walk(int nseg, const int64_t* offsets, const uint8_t* flags, double wd, int64_t step_slots, int kind, int64_t warmup, int64_t total,
                std::vector<AdamSegments>* segs, std::vector<AdamwRecipe>* recipes) {
    int slot_base = 0;
    bool mirrored = false;
    for (int first = 0; first < nseg; first += kMaxSegments) {
        const int count = nseg - first < kMaxSegments ? nseg - first : kMaxSegments;
        AdamwRecipe r;
        int rc = adamw_recipe_fill(r, count, first, 1e-3, wd, flags, nullptr, kind, warmup, total);
        if (rc != LG_OK) return rc;
        AdamSegments seg;
        int used = 0;
        rc = adam_segments_fill(seg, count, offsets + first, first, nseg, step_slots, slot_base, &mirrored, &used);
        if (rc != LG_OK) return rc;
        slot_base += used;
        segs->push_back(seg);          // (a group of empty parameters only: used == 0, nothing is launched)
        recipes->push_back(r);
    }
    return slot_base;
}

int main() {
    // the public entry points refuse an uninitialised library before they touch anything
    EXPECT(lg_adamw_multi_dev_f32(nullptr, nullptr, nullptr, nullptr, 1, nullptr, 1e-3, 0.9, 0.999, 1e-8, nullptr, 0, 1.0, 0, 0.0, nullptr, nullptr, 0, 0, 0) == LG_ENOTINIT);
    EXPECT(lg_grad_norm_clip_f32(nullptr, 1, 1.0, 1.0, nullptr, nullptr, nullptr) == LG_ENOTINIT);
    EXPECT(lg_adam_multi_dev_f32(nullptr, nullptr, nullptr, nullptr, 1, nullptr, 1e-3, 0.9, 0.999, 1e-8, nullptr, 0, 1.0, 0) == LG_ENOTINIT);

    for (int nseg : {1, 2, 63, 64, 65, 128, 129, 200}) {
        // ragged lengths with empty parameters in between, on the heap at their exact sizes
        int64_t* offsets = static_cast<int64_t*>(std::malloc(sizeof(int64_t) * (nseg + 1)));
        uint8_t* flags = static_cast<uint8_t*>(std::malloc(nseg));
        offsets[0] = 0;
        int64_t workgroups = 0;
        for (int j = 0; j < nseg; ++j) {
            const int64_t len = (j % 5 == 3) ? 0 : (j % 7 == 0 ? 4097 : 1 + (j * 37) % 1500);
            offsets[j + 1] = offsets[j] + len;
            workgroups += (len + 1023) / 1024;
            flags[j] = uint8_t(j % 2 == 0 ? (j % 4 == 0 ? 1 : 255) : 0);
        }
        std::vector<AdamSegments> segs;
        std::vector<AdamwRecipe> recipes;
        const int used = walk(nseg, offsets, flags, 0.1, workgroups, 1, 3, 8, &segs, &recipes);
        EXPECT(used == workgroups);
        int mirrors = 0, params = 0;
        int64_t slots = 0;
        for (size_t k = 0; k < segs.size(); ++k) {
            const AdamSegments& s = segs[k];
            EXPECT(s.first == int(k) * kMaxSegments);
            EXPECT(s.slot_base == slots && s.nseg_total == nseg && s.nseg >= 1 && s.nseg <= kMaxSegments);
            for (int j = 0; j < s.nseg; ++j) {
                EXPECT(s.offsets[j] == offsets[s.first + j] && s.offsets[j + 1] == offsets[s.first + j + 1]);
                EXPECT(s.wg_base[j + 1] - s.wg_base[j] == (s.offsets[j + 1] - s.offsets[j] + 1023) / 1024);
                EXPECT(recipes[k].decay[j] == ((s.first + j) % 2 == 0 ? 1 : 0));          // flags other than 0 count as 1
            }
            for (int j = s.nseg; j < kMaxSegments; ++j) EXPECT(recipes[k].decay[j] == 0);
            if (s.mirror_slot >= 0) { ++mirrors; EXPECT(s.mirror_slot >= s.slot_base && s.mirror_slot < s.slot_base + s.wg_base[s.nseg]); }
            slots += s.wg_base[s.nseg];
            params += s.nseg;
        }
        EXPECT(mirrors == 1 && params == nseg && slots == workgroups);
        // too few step slots for the grid, by one
        segs.clear(); recipes.clear();
        EXPECT(walk(nseg, offsets, flags, 0.1, workgroups - 1, 1, 3, 8, &segs, &recipes) == LG_EINVAL);
        // no weight decay: the flags are not read and may be NULL
        segs.clear(); recipes.clear();
        EXPECT(walk(nseg, offsets, nullptr, 0.0, workgroups, 0, 0, 0, &segs, &recipes) == workgroups);
        for (const AdamwRecipe& r : recipes)
            for (int j = 0; j < kMaxSegments; ++j) EXPECT(r.decay[j] == 0);
        // refused arguments
        segs.clear(); recipes.clear();
        EXPECT(walk(nseg, offsets, nullptr, 0.1, workgroups, 0, 0, 0, &segs, &recipes) == LG_EINVAL);          // decay without flags
        EXPECT(walk(nseg, offsets, flags, 0.1, workgroups, 2, 0, 0, &segs, &recipes) == LG_EINVAL);            // unknown schedule
        EXPECT(walk(nseg, offsets, flags, 0.1, workgroups, 1, 5, 4, &segs, &recipes) == LG_EINVAL);            // warmup > total
        EXPECT(walk(nseg, offsets, flags, 0.1, workgroups, 1, -1, 4, &segs, &recipes) == LG_EINVAL);
        if (nseg >= 2) {
            const int64_t keep = offsets[nseg - 1];
            offsets[nseg - 1] = offsets[nseg] + 1;                                                              // decreasing offsets
            segs.clear(); recipes.clear();
            EXPECT(walk(nseg, offsets, flags, 0.1, 1 << 20, 0, 0, 0, &segs, &recipes) == LG_EINVAL);
            offsets[nseg - 1] = keep;
        }
        std::free(offsets);
        std::free(flags);
    }
    // a bucket too large for one launch
    {
        int64_t offsets[2] = {0, (int64_t(1) << 22) * 1024};
        std::vector<AdamSegments> segs;
        std::vector<AdamwRecipe> recipes;
        EXPECT(walk(1, offsets, nullptr, 0.0, 0, 0, 0, 0, &segs, &recipes) == LG_EINVAL);
    }
    std::printf(failures ? "optim_args_check: %d FAILED\n" : "optim_args_check: ok\n", failures);
    return failures ? 1 : 0;
}
