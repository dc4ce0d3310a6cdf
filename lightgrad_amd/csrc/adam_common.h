// The per-element Adam / AdaBelief update shared by the optimizer kernels (optim.hip) and the optimizer launch that
// also exchanges the gradient bucket between the ranks of a node (p2p.hip).  Arithmetic: optim.hip's header.
#pragma once
#include "common.h"

namespace lg {

struct AdamScalars {
    float neg_lr, b1, one_minus_b1, b2, one_minus_b2, eps, inv_bias1, inv_bias2, gscale;
    int   belief, scale_grad;
};

__device__ __forceinline__ void adam_elem(float& p, float g, float& m, float& v, const AdamScalars& c) {
    if (c.scale_grad) g = g * c.gscale;
    m = c.b1 * m + c.one_minus_b1 * g;
    const float s = c.belief ? g - m : g;
    v = c.b2 * v + c.one_minus_b2 * (s * s);
    const float mh = m * c.inv_bias1, vh = v * c.inv_bias2;
    p = p + (c.neg_lr * mh) * (1.0f / (sqrtf(vh) + c.eps));
}

// adam_elem with the rest of a BERT recipe around it (lg_adamw_multi_dev_f32, optim.hip): the gradient is first multiplied by
// the clipping coefficient of the norm launch (clip != 0), and a decaying parameter (decay != 0) also moves by
// neg_decay * p = (-(lr_s * weight_decay)) * p - decoupled weight decay, added to the Adam update BEFORE that meets p, as
// the expression `p += delta + (-(lr_s * weight_decay)) * p` does.  c.neg_lr holds -lr_s, the scheduled learning rate.
// With clip == 0 and decay == 0 these are adam_elem's operations, so the same bits.
struct AdamwScalars {
    float coef, neg_decay;
    int   clip, decay;
};

__device__ __forceinline__ void adamw_elem(float& p, float g, float& m, float& v, const AdamScalars& c, const AdamwScalars& w) {
    if (c.scale_grad) g = g * c.gscale;
    if (w.clip) g = g * w.coef;
    m = c.b1 * m + c.one_minus_b1 * g;
    const float s = c.belief ? g - m : g;
    v = c.b2 * v + c.one_minus_b2 * (s * s);
    const float mh = m * c.inv_bias1, vh = v * c.inv_bias2;
    const float delta = (c.neg_lr * mh) * (1.0f / (sqrtf(vh) + c.eps));
    p = w.decay ? p + (delta + w.neg_decay * p) : p + delta;
}

// the host scalars of one update, rounded once to fp32 like numpy rounds a python float that meets an fp32 array
inline AdamScalars adam_scalars(double lr, double b1, double b2, double eps, double inv_bias1, double inv_bias2, double gscale, int belief) {
    AdamScalars c;
    c.neg_lr = float(-lr); c.b1 = float(b1); c.one_minus_b1 = float(1.0 - b1); c.b2 = float(b2); c.one_minus_b2 = float(1.0 - b2);
    c.eps = float(eps); c.inv_bias1 = float(inv_bias1); c.inv_bias2 = float(inv_bias2); c.gscale = float(gscale); c.belief = belief;
    c.scale_grad = gscale != 1.0;
    return c;
}

// ---- the argument block of the multi-tensor launches (lg_adam_multi_dev_f32 / lg_adamw_multi_dev_f32, optim.hip) ------------
constexpr int kMaxSegments = 64;
struct AdamSegments {
    int     nseg;          // parameters in THIS launch (<= kMaxSegments)
    int     nseg_total;    // parameters of the optimizer: the reference's `t` advances once per PARAMETER (optim.py:36/:48)
    int     first;         // index of this launch's first parameter
    int     slot_base;     // step slot of workgroup 0 of this launch
    int     mirror_slot;   // the workgroup with this slot also writes step[0] (-1: none in this launch)
    // COMPACT grid (round 4): parameter j owns workgroups wg_base[j] .. wg_base[j+1] - one per 1024 elements - instead of a row of
    // a 2-D grid as wide as the LONGEST parameter needs: for the MNIST MLP that grid had 1568 workgroups of which 399 had work,
    // and dispatching the 1169 that return at once is not free (the same lesson as the tail jobs of round 3)
    int     wg_base[kMaxSegments + 1];
    int64_t offsets[kMaxSegments + 1];
};

// what lg_adamw_multi_dev_f32 adds to the launch: by value like the segments, `decay` copied from the caller's HOST flags
struct AdamwRecipe {
    double       lr, weight_decay;
    const float* clip;             // device: {norm, coef} of lg_grad_norm_clip_f32, or NULL (no clipping)
    int          schedule_kind;    // 0: lr as given; 1: warmup / linear decay of the DEVICE step number
    int64_t      warmup_steps, total_steps;
    uint8_t      decay[kMaxSegments];      // per parameter of THIS launch: 1 = weight decay applies
};

// Host side of one group of <= kMaxSegments parameters: the compact grid, the group's step slots and which workgroup mirrors
// the step number.  *slots_used = workgroups of the group's grid (0: nothing to launch).  No device call in here.
inline int adam_segments_fill(AdamSegments& seg, int nseg, const int64_t* offsets, int first, int nseg_total, int64_t step_slots,
                              int slot_base, bool* mirrored, int* slots_used) {
    seg.nseg = nseg;
    seg.nseg_total = nseg_total;
    seg.first = first;
    seg.slot_base = slot_base;
    seg.mirror_slot = -1;
    int64_t total = 0;
    seg.wg_base[0] = 0;
    for (int j = 0; j <= nseg; ++j) {
        seg.offsets[j] = offsets[j];
        if (j > 0) {
            LG_ARG(offsets[j] >= offsets[j - 1], "lg_adam_multi_dev_f32: offsets must be non-decreasing");
            total += (offsets[j] - offsets[j - 1] + 1023) / 1024;          // one workgroup per 1024 elements (four per thread)
            LG_ARG(total < (int64_t(1) << 22), "lg_adam_multi_dev_f32: bucket too large for one launch");
            seg.wg_base[j] = int(total);
        }
    }
    *slots_used = int(total);
    if (total == 0) return LG_OK;
    if (step_slots > 0) {
        LG_ARG(slot_base + *slots_used <= step_slots, "lg_adam_multi_dev_f32: the grid spans %d step slots, the caller gave %lld (lghip.h)",
               slot_base + *slots_used, (long long)step_slots);
        if (!*mirrored)                                   // the first workgroup of the first non-empty parameter keeps step[0] current
            for (int j = 0; j < nseg; ++j)
                if (offsets[j + 1] > offsets[j]) { seg.mirror_slot = slot_base + seg.wg_base[j]; *mirrored = true; break; }
    }
    return LG_OK;
}

// Host side of the recipe for the group starting at parameter `first`: the scalars and this group's slice of the decay flags
// (decay_flags may be NULL when weight_decay == 0; flags other than 0 count as 1)
inline int adamw_recipe_fill(AdamwRecipe& r, int nseg, int first, double lr, double weight_decay, const uint8_t* decay_flags,
                             const float* clip, int schedule_kind, int64_t warmup_steps, int64_t total_steps) {
    LG_ARG(nseg >= 1 && nseg <= kMaxSegments && first >= 0, "lg_adamw_multi_dev_f32: a group of %d parameters", nseg);
    LG_ARG(schedule_kind == 0 || schedule_kind == 1, "lg_adamw_multi_dev_f32: schedule_kind %d (0 none, 1 warmup-linear)", schedule_kind);
    LG_ARG(schedule_kind == 0 || (0 <= warmup_steps && warmup_steps <= total_steps),
           "lg_adamw_multi_dev_f32: warmup-linear needs 0 <= warmup_steps <= total_steps, got %lld and %lld", (long long)warmup_steps,
           (long long)total_steps);
    LG_ARG(weight_decay == 0.0 || decay_flags != nullptr, "lg_adamw_multi_dev_f32: weight_decay without decay_flags");
    r.lr = lr;
    r.weight_decay = weight_decay;
    r.clip = clip;
    r.schedule_kind = schedule_kind;
    r.warmup_steps = warmup_steps;
    r.total_steps = total_steps;
    for (int j = 0; j < kMaxSegments; ++j) r.decay[j] = (j < nseg && weight_decay != 0.0 && decay_flags[first + j]) ? 1 : 0;
    return LG_OK;
}

// ---- the update applied where the gradient is made (lg_adam_plan_* / lg_adam_epilogue_*, optim.hip) --------------------
// One parameter's update as data in DEVICE memory: the kernel that produces the parameter's gradient (GEMM epilogue of
// gemm_tile_body.inc, the slab workgroups of head.hip) applies it to the values it is about to store, so the optimizer's own
// launch disappears from the step.  The new parameter values go to a SECOND buffer (p_out != p_in): other workgroups of the
// same launch still read the old ones (dx = g @ W next to dW = g^T @ x in sgemm_pair_wgrad_xgrad; the dx tiles next to the
// dW slabs in head_bwd).  The step number behind the bias corrections alternates between two words the same way: every
// workgroup reads step_in, which nobody writes during this step, and exactly one workgroup per step - the one that handles
// element 0 of the plan whose step_out is not NULL - writes step_out = step_in + 1.
struct AdamPlan {
    const float*   p_in;
    float*         p_out;
    float*         m;
    float*         v;
    const int64_t* step_in;     // optimizer steps done so far
    int64_t*       step_out;    // NULL except in the one plan of the optimizer that advances the step number
    int64_t        n;           // elements
    int64_t        t_mul, t_add;   // t = steps_done * t_mul + t_add (the reference advances t once per PARAMETER, optim.py:36/:48)
    double         b1, b2;
    AdamScalars    c;           // inv_bias1 / inv_bias2 are filled in on the device
    // The bias corrections 1/(1 - b^t) of every step this plan will ever see, made on the HOST when the plan is created
    // (libm pow in double, rounded once to fp32: the python expression `(1 - self.b1**self.t)` to the letter): entry s holds the
    // pair for steps_done == s; from entry table_steps - 1 on both are exactly 1.0f (b^t < 2^-25).  Two double-precision pow()
    // by one lane cost a wavefront ~2 us - in an epilogue that sits on the critical path of its launch they cost more than the
    // optimizer launch they replace (measured: the MLP step 59.7 -> 64.7 us with them, bench_v1 of round 4).  NULL: too many
    // steps to tabulate (b2 very close to 1): the powers are formed on the device as before.
    const float*   table;
    int64_t        table_steps;
};

// the scalars of this step for one wavefront: lane 0 reads the step number and forms the two double-precision powers
// (as the python expression does), every lane receives them - no LDS, no workgroup barrier, callable where only some waves
// of a workgroup are still alive
__device__ __forceinline__ AdamScalars adam_plan_scalars(const AdamPlan* pl, int64_t& steps_done) {
    AdamScalars c = pl->c;
    if (pl->table) {                          // uniform: kernel-argument pointer, scalar loads
        steps_done = pl->step_in[0];
        const int64_t s = steps_done < pl->table_steps ? steps_done : pl->table_steps - 1;
        c.inv_bias1 = pl->table[2 * s];
        c.inv_bias2 = pl->table[2 * s + 1];
        return c;
    }
    float i1 = 0.f, i2 = 0.f;
    long long done = 0;
    if ((threadIdx.x & 63) == 0) {
        done = __hip_atomic_load(pl->step_in, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        const double t = double(done * pl->t_mul + pl->t_add);
        i1 = float(1.0 / (1.0 - pow(pl->b1, t)));
        i2 = float(1.0 / (1.0 - pow(pl->b2, t)));
    }
    c.inv_bias1 = __shfl(i1, 0, 64);
    c.inv_bias2 = __shfl(i2, 0, 64);
    steps_done = (long long)(__shfl((unsigned long long)done, 0, 64));
    return c;
}

// host side (optim.hip): the plan armed for the gradient buffer `grad` of `n` floats, if the launch being prepared may apply
// it - i.e. it OVERWRITES the gradient (accumulate == 0: the first and only write of this step).  The plan then counts as
// applied.  NULL: nothing armed, or not applicable (the optimizer's lg_adam_epilogue_finish applies what is left).
// A launch that writes into the bytes of a gradient whose plan was already applied in this step is an error: *rc = LG_EINVAL
// (adam_epilogue_check_write, common.h: the same check for every other writer).
const AdamPlan* adam_epilogue_take(const void* grad, int64_t n, int accumulate, int* rc);

}  // namespace lg
