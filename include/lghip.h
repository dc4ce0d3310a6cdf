/* lghip.h - C ABI of liblghip.so, the MI355X (gfx950) device library behind
 * lightgrad's HipTensor backend.
 *
 * This is the drop-in boundary: plain C, opaque device
 * pointers, caller-owned int64 shape/stride arrays that only need to live for
 * the duration of a call.  Every entry point is what a lightgrad backend binds
 * instead of the pyopencl calls of the reference's OpenCL backend; the
 * reference interface each one replaces is cited as file:line (relative to the
 * lightgrad repository).
 *
 * Conventions
 *   - every function returns 0 on success, a negative LG_E* code otherwise;
 *     lg_last_error() returns a thread-local message for the last failure.
 *     Nothing throws across the boundary.
 *   - one process drives one GPU through one HIP stream owned by the library
 *     (the reference: one in-order queue per device, opencl/device.py:79-84).
 *     All device work is stream-ordered and asynchronous; only lg_memcpy_d2h,
 *     lg_sync and lg_event_elapsed_ms block the host.  (The reference blocks
 *     after every kernel: opencl/kernels.py:194, :334, :499.)
 *   - shapes and strides are in ELEMENTS (not bytes), row-major order, at
 *     most LG_MAX_DIMS dimensions; a stride of 0 broadcasts that dimension.
 *   - arithmetic entry points are fp32 only; layout entry points (copy, fill)
 *     take an item size in bytes and are bit-exact for any dtype.
 */
#ifndef LGHIP_H
#define LGHIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define LG_MAX_DIMS 8

/* error codes */
#define LG_OK            0
#define LG_EINVAL       -1   /* bad argument (shape/stride/op id/alignment) */
#define LG_EHIP         -2   /* a HIP runtime call failed (message has hipGetErrorString) */
#define LG_ENOMEM       -3   /* device allocation failed even after trimming the pool */
#define LG_ENOTINIT     -4   /* lg_init has not been called */
#define LG_ECOMM        -5   /* RCCL failure (liblghip_comm.so) or a peer-window exchange that gave up waiting (lghip_p2p.h) */
#define LG_EINDEX       -6   /* an EARLIER kernel met an index / label out of range (reported by the next synchronising call) */

const char* lg_last_error(void);

/* ---- runtime: device, stream, pool ---------------------------------------
 * replaces OpenCLDevice (opencl/device.py:68-115): context + in-order queue +
 * cl.tools.MemoryPool(ImmediateAllocator) (:83-84). */
int lg_device_count(int* count);
int lg_init(int device);                       /* idempotent for the same device */
int lg_device(int* device);                    /* device bound by lg_init */
typedef struct {
    char     name[128];
    char     arch[32];                          /* "gfx950" */
    int32_t  compute_units;
    int32_t  clock_mhz;                         /* max engine clock */
    int32_t  wavefront_size;
    int32_t  lds_bytes_per_cu;
    uint64_t hbm_bytes;
    int32_t  l2_bytes;
    int32_t  reserved;
} lg_device_info_t;
int lg_device_info(lg_device_info_t* out);
/* Preflight of a multi-GPU job (no counterpart in the reference: its device pool enumerates OpenCL devices and never
 * relates two of them, opencl/device.py:12-49).  Pure queries, usable before lg_init and without touching `peer`:
 * can_access = hipDeviceCanAccessPeer(device, peer); link_type = hipExtGetLinkTypeAndHopCount's type (HSA_AMD_LINK_INFO_TYPE:
 * 0 HyperTransport, 1 QPI, 2 PCIe, 3 InfiniBand, 4 xGMI), hops its hop count; both -1 when the runtime cannot say. */
int lg_peer_info(int device, int peer, int* can_access, int* link_type, int* hops);
void* lg_stream(void);                          /* hipStream_t of the library (for liblghip_comm / profilers) */
int lg_sync(void);                              /* block until the stream is idle */

/* caching, stream-ordered allocator (replaces device.mem_pool.allocate, opencl/tensor.py:64).
 * lg_free returns the block to the pool immediately: safe because all users are on one stream. */
int lg_malloc(void** ptr, size_t bytes);
int lg_free(void* ptr);
int lg_pool_trim(void);                         /* hipFree every cached free block */
int lg_pool_stats(uint64_t* reserved_bytes, uint64_t* in_use_bytes, uint64_t* hip_malloc_calls);

/* transfers (replace cl.enqueue_copy: H2D opencl/tensor.py:78, D2H :84, D2D :92) */
int lg_memcpy_h2d(void* dst, const void* src, size_t bytes);   /* returns after src may be reused */
int lg_memcpy_d2h(void* dst, const void* src, size_t bytes);   /* synchronises the stream */
int lg_memcpy_d2d(void* dst, const void* src, size_t bytes);   /* stream-ordered */
/* upload without waiting: src is staged into pinned memory (reusable on return), the DMA is stream-ordered.
 * Feeds a new batch into the static input tensor of a captured graph between two lg_graph_launch calls. */
int lg_memcpy_h2d_async(void* dst, const void* src, size_t bytes);
/* HIP events on the library's stream (timing in bench.py) */
int lg_event_create(void** ev);
int lg_event_record(void* ev);
int lg_event_elapsed_ms(void* start, void* stop, float* ms);   /* synchronises on `stop` */
int lg_event_destroy(void* ev);

/* hipGraph capture of the library's stream: a launch-bound step (the ~100
 * dispatches of one MLP training step) is recorded once and replayed with one
 * host call.  While capturing, pool blocks are pinned to the graph so replays
 * see the same addresses. */
int lg_graph_begin(void);
int lg_graph_end(void** graph_exec);
int lg_graph_launch(void* graph_exec);
int lg_graph_destroy(void* graph_exec);
int lg_graph_kernel_count(void* graph, int* kernels);          /* kernel launches one replay performs (reports, tests) */

/* ---- layout ops (bit-exact, any dtype) ----------------------------------- */

/* dst[idx] = src[idx] over `shape`; either side may be strided/broadcast.
 * replaces the `atom` kernel with op 'o = a' used by contiguous()/copy()/getitem/setitem
 * (opencl/tensor.py:103-116, opencl/ops.py:322-340). itemsize in {1,2,4,8}.
 * Elements are read and written in no particular order: `src` must not overlap `dst` unless it is the identical view (same
 * pointer, same strides).  A caller that moves data within one buffer (`t[:, 1:] = t[:, :-1]`) copies the source first. */
int lg_copy_strided(int itemsize, int ndim, const int64_t* shape,
                    void* dst, const int64_t* dst_strides,
                    const void* src, const int64_t* src_strides);

/* dst[idx] = value over a strided view; `value_bits` holds the item in its low bytes.
 * replaces clEnqueueFillBuffer (opencl/ops.py:172-177). */
int lg_fill_strided(int itemsize, int ndim, const int64_t* shape,
                    void* dst, const int64_t* dst_strides, uint64_t value_bits);

/* What the most recent lg_copy_strided / lg_fill_strided call of the calling thread did (calls the library makes itself, such
 * as the zero fill of an empty sum, count): host bookkeeping for tests, no device work.
 *   out = {path, index_bits, head_items, body_vectors}
 * path: 0 = device memcpy (both sides one contiguous run), 1 = handed to lg_ew (4-byte items; lg_ew_last_plan says the rest),
 * 2 = the copy gather kernel (1-, 2-, 8-byte items), 3 = the flat fill (a dense run), 4 = the fill gather kernel, -1 = nothing
 * launched (no elements, a refused call);
 * index_bits: 32 or 64, the width of the element counter of paths 2 and 4, else 0;
 * head_items, body_vectors: path 3 only - the items in front of the first 16-byte boundary (capped by the length) and the
 * 16-byte stores behind them (capped at INT32_MAX); the rest of the run is the tail.  Else 0. */
int lg_layout_last_plan(int32_t out[4]);

/* ---- elementwise fp32 ------------------------------------------------------
 * One generic entry point replacing the run-time generated `atom` kernels
 * (opencl/kernels.py:24-195) for every op string used in opencl/ops.py:40-400.
 * Operands a, b, c, d are fp32 inputs with their own strides (0 = broadcast);
 * a NULL operand pointer means "this operand is the scalar `scalar`"
 * (reference: scalar kernel arguments, kernels.py:139-150).
 * out0/out1 are written; an output may alias an input with identical strides
 * (in-place forms `a += b`, kernels.py `additional_read`).  That is the ONLY overlap allowed: an input that shares
 * memory with an output must be the identical view (same pointer, same strides), so that every element is read and
 * written by the one thread that owns it.  Any other overlap - `t += t^T`, a shifted slice of the output - is read in
 * no defined order relative to the writes and gives wrong values; the caller copies such an input first (numpy's
 * "right-hand side first", what autograd/hip/ops.py does).  The two outputs must not overlap each other.
 * The library picks a vectorised contiguous path, an inner-dimension
 * vectorised path or a generic strided path; results do not depend on it. */
typedef enum {
    /* unary: out0 = f(a) */
    LG_EW_COPY = 0, LG_EW_NEG, LG_EW_EXP, LG_EW_LOG, LG_EW_RELU, LG_EW_SIGMOID,
    LG_EW_TANH, LG_EW_SIN, LG_EW_COS, LG_EW_SQRT,
    LG_EW_GELU,          /* tanh-approximated gelu of examples/bert.py:12, same evaluation order */
    /* binary: out0 = f(a, b) */
    LG_EW_ADD = 32, LG_EW_SUB, LG_EW_MUL, LG_EW_DIV, LG_EW_POW,
    LG_EW_RELU_BWD,      /* a = saved input t, b = g :  g * (t >= 0)        (cpu/ops.py:229) */
    LG_EW_SIGMOID_BWD,   /* a = y, b = g            :  y * (1 - y) * g      (cpu/ops.py:208) */
    LG_EW_TANH_BWD,      /* a = y, b = g            :  (1 - y*y) * g        (cpu/ops.py:219) */
    LG_EW_LOG_BWD,       /* a = x, b = g            :  (1 / x) * g          (cpu/ops.py:197) */
    LG_EW_SIN_BWD,       /* a = t, b = g            :  cos(t) * g           (cpu/ops.py:166) */
    LG_EW_COS_BWD,       /* a = t, b = g            :  -sin(t) * g          (cpu/ops.py:176) */
    LG_EW_EQ,            /* (a == b) ? 1 : 0 */
    LG_EW_GE,            /* (a >= b) ? 1 : 0 */
    LG_EW_BIAS_RELU,     /* a = x, b = bias         :  max(x + b, 0)  (fused Linear bias + relu) */
    LG_EW_GELU_BWD,      /* a = x, b = g            :  g * gelu'(x) */
    /* ternary: out0 = f(a, b, c) */
    LG_EW_MAX_BWD = 64,  /* a = x, b = extremum, c = g : g * (x == b)      (cpu/ops.py:272) */
    LG_EW_FMA,           /* a * b + c (two roundings, like the tape's mul then add) */
    /* two outputs: (out0, out1) = f(a, b, c[, d]) */
    LG_EW_MUL_BWD = 96,  /* a, b, c = g : (g * b, a * g)                   (cpu/ops.py:84)  */
    LG_EW_DIV_BWD,       /* a, b, c = g : (g / b, -a / b^2 * g)            (cpu/ops.py:94)  */
    LG_EW_POW_BWD        /* a, b, c = g, d = y : (b * a^(b-1) * g, g * y * log a) (cpu/ops.py:105) */
} lg_ew_op_t;

int lg_ew(int op, int ndim, const int64_t* shape,
          void* out0, const int64_t* out0_strides,
          void* out1, const int64_t* out1_strides,
          const void* a, const int64_t* a_strides,
          const void* b, const int64_t* b_strides,
          const void* c, const int64_t* c_strides,
          const void* d, const int64_t* d_strides,
          float scalar);

/* Which kernel family the most recent lg_ew call of the calling thread launched (lg_copy_strided calls it for 4-byte items that
 * are not one dense run): host bookkeeping for tests, no device work.
 *   out = {path, form, ndim, mask}
 * path: 0 = flat, 1 = rows (float4 along the inner dimension), 2 = transposed tile (staged through LDS), 3 = flat-2D (dense 2-D
 * outputs, any 2-D inputs), 4 = gather (one element per thread), -1 = nothing launched (no elements, a refused call: the other
 * fields are then 0);
 * form: flat - bit 0 = the float4 kernel ran, bit 1 = the scalar tail kernel ran; transposed tile - 0 = the scalar tile, 1 = float4
 * with one staged input, 2 = float4 with two staged inputs, 3 = the 128 x 128 tile; otherwise 0;
 * ndim: dimensions left after dropping extents of 1 and merging jointly contiguous neighbours;
 * mask: bit i = input i, as the kernel got it - flat: the input steps through memory (clear: it is one value in memory);
 * transposed tile: the input is staged; flat-2D: the input is dense and moves as float4; otherwise 0. */
int lg_ew_last_plan(int32_t out[4]);

/* ---- reductions fp32 -------------------------------------------------------
 * replaces the multi-pass `reduce` kernel (opencl/kernels.py:344-501) as used by
 * sum/max/min (opencl/ops.py:344-400).  Dimensions whose bit is set in
 * `axis_mask` (bit i = dimension i) are reduced; `out` is CONTIGUOUS over the
 * kept dimensions in their original order.  max/min are exact; sum is a
 * tree reduction in fp32 (numpy uses pairwise blocks: agreement ~1e-6 rel). */
typedef enum { LG_RED_SUM = 0, LG_RED_MAX = 1, LG_RED_MIN = 2 } lg_red_op_t;
int lg_reduce(int op, int ndim, const int64_t* shape,
              const void* in, const int64_t* in_strides,
              uint32_t axis_mask, void* out);

/* ---- tensors that are not float32 (round 4) -----------------------------------
 * The reference's tensors keep whatever dtype their numpy array has (cpu/tensor.py:45-46: MNIST labels int16, data.py:43; BERT
 * ids int32, examples/bert.py:346) and its device backend generates every elementwise / reduction kernel per dtype
 * (opencl/kernels.py:9, :24-107, :344-431).  Here float32 - the north-star path - has its own tuned kernels (lg_ew, lg_reduce);
 * these entry points make int16 / int32 / int64 / float64 tensors computable on the device with numpy's semantics
 * (cpu/ops.py:52-84, :260-293): integers wrap around, integer sums are int64, max / min keep the dtype and propagate NaN.
 *   lg_ew_typed      out = a (op) b, all three of `dtype`, numpy broadcasting through strides; op = LG_EW_COPY / NEG (unary),
 *                    ADD / SUB / MUL, and for float64 DIV / POW; a NULL operand is the scalar (scalar_i for integers, scalar_f
 *                    for float64); out may alias an operand element for element (in-place forms) and in no other way: an operand that
 *                    overlaps `out` must be the identical view, as for lg_ew
 *   lg_reduce_typed  as lg_reduce; `out` holds int64 for integer sums, `dtype` otherwise
 *   lg_cast          out[i] = (dst type) in[i], any pair of the five dtypes (numpy's astype: float -> int truncates) */
typedef enum { LG_DT_I16 = 1, LG_DT_I32 = 2, LG_DT_I64 = 3, LG_DT_F64 = 4, LG_DT_F32 = 5 } lg_dtype_t;
int lg_ew_typed(int op, int dtype, int ndim, const int64_t* shape, void* out, const int64_t* out_strides,
                const void* a, const int64_t* a_strides, const void* b, const int64_t* b_strides,
                double scalar_f, int64_t scalar_i);
int lg_reduce_typed(int op, int dtype, int ndim, const int64_t* shape, const void* in, const int64_t* in_strides,
                    uint32_t axis_mask, void* out);
int lg_cast(int src_dtype, int dst_dtype, int ndim, const int64_t* shape, void* out, const int64_t* out_strides,
            const void* in, const int64_t* in_strides);

/* out (+)= reduction: with accumulate != 0 (sums only) the result is ADDED to `out`, so a bias gradient
 * can be accumulated straight into its gradient buffer (tensor.py:118 `grad += g` without the extra pass). */
int lg_reduce_acc(int op, int ndim, const int64_t* shape,
                  const void* in, const int64_t* in_strides,
                  uint32_t axis_mask, void* out, int accumulate);

/* Which kernel the most recent lg_reduce / lg_reduce_acc call of the calling thread launched (calls the library makes itself,
 * such as the mean of lg_cross_entropy_mean_f32, count): host bookkeeping for tests, no device work.
 *   out = {kernel, splits, groups, nk, nr, vector_path_possible}
 * kernel: 0 = one wave per row, 1 = rows split over workgroups, 2 = 64-column tiles, 3 = general / column kernel, -1 = nothing
 * launched (no output elements, the zero-length sum, a refused call: the other fields are then 0 except the last);
 * splits: workgroups that share one output (1 = no fold); groups: first-level fold groups of kernel 1, else 0;
 * nk, nr: kept and reduced dimensions left after merging contiguous neighbours; vector_path_possible: `in` is 16-byte aligned. */
int lg_reduce_last_plan(int32_t out[6]);

/* ---- argmax / argmin and top-1 counting (csrc/argreduce.hip) ------------------------------------------------
 * out[...] = the index along `axis` (axis = -1: into the row-major flattening of the whole view) of the maximum (LG_RED_MAX) or
 * minimum (LG_RED_MIN) of a strided fp32 view; `out` is int64, CONTIGUOUS over the kept dimensions in their original order.
 * numpy's answer bit for bit: a candidate (v, i) beats (w, j) when v is NaN and w is not; or neither is NaN and v > w (v < w
 * for the minimum); or neither of the two holds in either direction and i < j.  So the lowest index wins among equal extrema
 * (-0.0 == +0.0), a run of nothing but -inf answers 0, and a run that holds a NaN answers the index of its first NaN.  The
 * order is total: every fold order gives the same result.
 * The dimensions in front of the axis, the axis (every dimension for -1) and the dimensions behind it must each merge into at
 * most ONE (extent, stride): any other view is refused with LG_EINVAL (copy it dense first), as is a reduced extent of 0.
 * No output elements: LG_OK, nothing is launched. */
int lg_argreduce_f32(int op, int ndim, const int64_t* shape, const float* in, const int64_t* in_strides, int axis, int64_t* out);

/* What the most recent lg_argreduce_f32 call of the calling thread launched: host bookkeeping for tests, no device work.
 *   out = {kernel, splits, merged, vector}
 * kernel: 0 = one wave per row, 1 = rows split over workgroups (one workgroup per row segment), 2 = one thread per output with
 * the axis strided, -1 = nothing launched (no output elements, a refused call: the other fields are then 0);
 * splits: workgroups that share one output (1 = no fold); merged: the dimensions in front of and behind the axis form one
 * output dimension (always for kernels 0 and 1); vector: the first run read holds a 16-byte aligned float4 (kernels 0, 1). */
int lg_argreduce_last_plan(int32_t out[4]);

/* Top-1 counting of dense fp32 logits [rows, cols] against integer labels [rows] (int16/32/64) in ONE launch:
 *   counts[0] (+)= rows whose label equals the row's argmax (the rules above: a label on the second of two tied maxima is wrong,
 *                  a row with a NaN is right only for the label of its first NaN)
 *   counts[1] (+)= rows counted: all but those whose label, as stored, equals ignore_index (has_ignore != 0); those rows are not read
 * accumulate != 0 adds to `counts` (a running total over batches), else `counts` is overwritten.  A negative label that is not
 * ignored wraps by +cols; one out of range is not counted and raises the device status flag (LG_EINDEX at the next
 * synchronising call), as lg_cross_entropy_f32 does.  Nothing is a host scalar: a captured launch counts the batch that is in
 * the tensors at every replay. */
int lg_top1_count_f32(const float* logits, int64_t rows, int64_t cols, const void* labels, int label_itemsize, int has_ignore,
                      int64_t ignore_index, int accumulate, int64_t* counts);

/* ---- SGEMM on MFMA ---------------------------------------------------------
 * C[b] (M x N, row-major, leading dimension ldc) (+)= op(A[b]) @ op(B[b]), fp32
 * in/out, fp32 accumulate on v_mfma_f32_32x32x2_f32.
 *   transA = 0: A[m*lda + k]      transA = 1: A[k*lda + m]
 *   transB = 0: B[k*ldb + n]      transB = 1: B[n*ldb + k]
 * so stride-permuted views (W.T(1,0) in nn.Linear, nn.py:96; the transposed
 * operands of dot.backward, cpu/ops.py:116) are consumed WITHOUT the
 * contiguous() copies and zero-padding copies of the reference
 * (opencl/kernels.py:291-298, :319-320, :331).
 * batch > 1: operand b starts at base + b*stride{A,B,C} elements (stride 0
 * broadcasts an operand over the batch).  accumulate != 0 adds into C.
 * replaces kernels.dot (opencl/kernels.py:201-337) called from opencl/ops.py:116-132.  * Operands are fetched in 16-byte pieces along their contiguous index: when that extent is not a multiple of 4, up to
 * 12 bytes behind an operand's last row are READ (never used).  Memory from lg_malloc always has them; foreign
 * memory passed here must be readable that far.
 */
int lg_gemm_f32(int transA, int transB, int64_t M, int64_t N, int64_t K,
                const float* A, int64_t lda, int64_t strideA,
                const float* B, int64_t ldb, int64_t strideB,
                float* C, int64_t ldc, int64_t strideC,
                int64_t batch, int accumulate);

/* What the most recent fp32 product (any lg_gemm_*_f32 entry above or below, lg_gemm_bf16_f32 excepted) of the calling thread
 * resolved to: host bookkeeping for tests, recorded once the slice count is final; no device work, no effect on any launch.
 *   out = {BM, BN, BK, KG, k_slices, k_per_slice, flags, route}
 * BM x BN: the workgroup's tile of C; BK: k-values per K-group and K-step; KG: K-groups inside the workgroup (a K-step stages
 * BK * KG k-values).  BM = -1 before any product; BM = 0 (and everything else 0) when the call launched no GEMM kernel (M, N or
 * batch of 0; K = 0, which fills C).  k_slices: workgroups along K per tile as launched (1 = no cross-workgroup split), each over
 * k_per_slice k-values.  flags: bit 0 A K-contiguous (transA = 0), bit 1 B K-contiguous (transB = 1), bit 2 / 3 A / B staged as
 * float4, bit 4 the wave-private K loop ran.  route: 0 launched on its own, 1 deferred into a lg_gemm_pair_* bracket, 2 queued
 * in a lg_gemm_group_* bracket (either may still re-tune its slice count when it leaves), 3 the chained head launch of
 * lg_gemm_bias_head_fwd_f32. */
int lg_gemm_last_plan(int32_t out[8]);

/* The same product with both operands rounded to bfloat16 (nearest, ties to even; NaN, +-Inf and the sign of zero kept, a
 * finite value beyond the largest bfloat16 becomes +-Inf) on their way into the matrix cores: C (+)= r(op(A)) @ r(op(B)) [+ bias].
 * Products of two bfloat16 values are exact in fp32; the sums are formed in fp32 on v_mfma_f32_32x32x16_bf16.  Operands,
 * result and bias (N values, may be NULL) stay fp32 in memory; layouts and leading dimensions as for lg_gemm_f32, one matrix
 * product, all four transA x transB layouts consumed in place (the same 16-byte fetches, so the same 12 readable bytes behind
 * an operand).  bias is added after the fp32 sum; bias together with accumulate is LG_EINVAL.  M or N of 0: nothing happens;
 * K of 0: C = 0 (+ bias) unless accumulate.  Few output tiles over a long K are cut along K and folded in ascending order by a
 * second kernel: the same bits from run to run, no atomics.  Subnormal fp32 inputs are unspecified. */
int lg_gemm_bf16_f32(int transA, int transB, int64_t M, int64_t N, int64_t K,
                     const float* A, int64_t lda, const float* B, int64_t ldb,
                     float* C, int64_t ldc, const float* bias, int accumulate);

/* dst[i] = r(src[i]) for n dense fp32 values: rounded to bfloat16 exactly as lg_gemm_bf16_f32 rounds its operands, kept as fp32
 * (the low 16 bits zero).  dst may be src. */
int lg_bf16_round_f32(const float* src, float* dst, int64_t n);

/* Same product with a bias row added in the epilogue: C[b][m][n] = (op(A[b]) @ op(B[b]))[m][n] + bias[n]
 * (bias may be NULL).  The sum is rounded to fp32 before the bias is added, exactly like the separate
 * `x @ W.T + b` of nn.Linear (nn.py:96).  Fuses one elementwise pass per Linear layer. */
int lg_gemm_bias_f32(int transA, int transB, int64_t M, int64_t N, int64_t K,
                     const float* A, int64_t lda, int64_t strideA,
                     const float* B, int64_t ldb, int64_t strideB,
                     float* C, int64_t ldc, int64_t strideC,
                     int64_t batch, const float* bias);

/* One matrix product with every epilogue / prologue the tape can fold into it (any of them may be off):
 *   bias [N]            added to every row (nn.py:96)                                      - excludes accumulate, rowsum
 *   rowsum [M]          (+)= row sums of op(A), see lg_gemm_rowsum_f32
 *   relu_a / relu_b     op(A) / op(B) pass through np.maximum(., 0) (cpu/ops.py:226) on their way to LDS: the consumer of
 *                       a relu reads the PRE-activation, the relu kernel and its output tensor are never made
 * (The (t >= 0) factor of relu's backward is NOT folded into the input-gradient GEMM: the relu output's own `.grad` -
 * readable on every tensor of the tape, tensor.py:40-42 - would then hold the masked values.) */
int lg_gemm_fused_f32(int transA, int transB, int64_t M, int64_t N, int64_t K,
                      const float* A, int64_t lda, const float* B, int64_t ldb, float* C, int64_t ldc,
                      int accumulate, const float* bias, float* rowsum, int rowsum_accumulate,
                      int relu_a, int relu_b);

/* C = (op(A) @ op(B) [+ bias]) + addend, addend an [M, N] matrix with row pitch ldadd (>= N) that may be C itself only
 * through lg_gemm_f32's accumulate flag.  One matrix product.  The sums are formed in that order, each rounded to fp32 -
 * the values of the separate bias add and residual add (`dense(h) + h_in`, reference examples/bert.py:101; a gradient that
 * already holds a first contribution, autograd/tensor.py:111-118) without a pass over the result for either. */
int lg_gemm_addend_f32(int transA, int transB, int64_t M, int64_t N, int64_t K,
                       const float* A, int64_t lda, const float* B, int64_t ldb, float* C, int64_t ldc,
                       const float* bias, const float* addend, int64_t ldadd);

/* One matrix product with an activation applied where the result is made (small tiles):
 *   act = LG_ACT_GELU      C = op(A) @ op(B) + bias (the pre-activation, kept for the backward) and aux[m][n] = gelu(C[m][n])
 *                          - nn.Linear followed by the gelu of examples/bert.py:12 without the elementwise pass
 *   act = LG_ACT_GELU_BWD  C = (op(A) @ op(B)) * gelu'(aux[m][n]), aux the pre-activation saved by the forward: the input
 *                          gradient of the NEXT Linear (dot.backward, cpu/ops.py:116) multiplied by the gelu derivative
 *                          in the same launch (bias must be NULL)
 * aux is [M, N] with row pitch ldaux.  The same expressions as the elementwise gelu kernels, bit for bit. */
#define LG_ACT_GELU 1
#define LG_ACT_GELU_BWD 2
int lg_gemm_act_f32(int transA, int transB, int64_t M, int64_t N, int64_t K,
                    const float* A, int64_t lda, const float* B, int64_t ldb, float* C, int64_t ldc,
                    const float* bias, int act, float* aux, int64_t ldaux);

/* Three Linear layers on ONE input in one launch: C[i] = op(A) @ op(B[i]) + bias[i], i < 3, all of one shape - the query / key /
 * value projections of a transformer layer (reference examples/bert.py:78-80: three nn.Linear calls, each a kernels.dot and a
 * bias add).  The three weights stay where they are (separately allocated parameters; their addresses travel as offsets from
 * B[0]); the three results may be column blocks of one buffer (ldc = its row pitch).  bias may be NULL (no bias at all). */
int lg_gemm_multi3_f32(int transA, int transB, int64_t M, int64_t N, int64_t K, const float* A, int64_t lda,
                       const float* const* B, int64_t ldb, float* const* C, int64_t ldc, const float* const* bias);

/* One product whose K dimension runs through three separately allocated right-hand operands of seg_k k-values each:
 * C (+)= op(A)[M, 3 * seg_k] @ [op(B[0]); op(B[1]); op(B[2])] (+ addend) - the input gradient of the three projections above,
 * dx = [dq | dk | dv] @ [Wq; Wk; Wv], which the tape forms as three kernels.dot calls and two additions (dot.backward,
 * cpu/ops.py:116; add_grad, tensor.py:111-118).  seg_k a multiple of 64; the sum runs in K order like one long product. */
int lg_gemm_kseg3_f32(int transA, int transB, int64_t M, int64_t N, int64_t seg_k, const float* A, int64_t lda,
                      const float* const* B, int64_t ldb, float* C, int64_t ldc, int accumulate,
                      const float* addend, int64_t ldadd);

/* lg_gemm_f32 over a TWO-level batch: matrix (o, i) of operand X starts at X + o*strideX_outer + i*strideX_inner.
 * One launch for attention-shaped products whose (batch, head) dims do not collapse into one stride after the head
 * split `reshape(b, s, h, d).transpose(0, 2, 1, 3)` (examples/bert.py:70-95; the reference's kernel is launched per
 * batch by kernels.dot, opencl/kernels.py:318-334). */
int lg_gemm_batched2_f32(int transA, int transB, int64_t M, int64_t N, int64_t K,
                         const float* A, int64_t lda, int64_t strideA_outer, int64_t strideA_inner,
                         const float* B, int64_t ldb, int64_t strideB_outer, int64_t strideB_inner,
                         float* C, int64_t ldc, int64_t strideC_outer, int64_t strideC_inner,
                         int64_t batch_outer, int64_t batch_inner, int accumulate);

/* C (+)= op(A) @ op(B) and, from the same launch, rowsum (+)= row sums of op(A) (one matrix product, no batch).
 * With op(A) = g^T this is the weight gradient dW = g^T @ x together with the bias gradient db = column sums of g -
 * the dot.backward GEMM (cpu/ops.py:116) plus the un-broadcasting `sum(axis=0, keepdims=True)` of func.py:50-56 for
 * nn.Linear's `+ b` (nn.py:96).  The sums are column N of the product against a virtual column of ones appended to
 * op(B), i.e. they come off the same MFMA accumulators. */
int lg_gemm_rowsum_f32(int transA, int transB, int64_t M, int64_t N, int64_t K,
                       const float* A, int64_t lda, const float* B, int64_t ldb,
                       float* C, int64_t ldc, int accumulate, float* rowsum, int rowsum_accumulate);

/* ---- fused optimizer ---------------------------------
 * One Adam/AdaBelief update of a contiguous parameter, numerically the
 * expression sequence of optim.py:36-40 / :48-52 evaluated per element (one
 * rounding per operation; the tape's `/` is multiply-by-reciprocal):
 *   g' = g * gscale (skipped when gscale == 1)
 *   m  = b1*m + (1-b1)*g';   s = belief ? g' - m : g';   v = b2*v + (1-b2)*s*s
 *   p += ((-lr) * (m * inv_bias1)) * (1 / (sqrt(v * inv_bias2) + eps))
 * with inv_bias1 = 1/(1 - b1^t), inv_bias2 = 1/(1 - b2^t) computed by the caller
 * in double; every scalar is rounded once to fp32 inside (numpy's python-float rule).
 * gscale folds the data-parallel 1/world_size into the update. */
int lg_adam_step_f32(float* p, const float* g, float* m, float* v, int64_t n,
                     double lr, double b1, double b2, double eps,
                     double inv_bias1, double inv_bias2, double gscale, int belief);

/* Graph-safe form: the optimizer step number is read from device memory (t = *step * t_mul + t_add,
 * the reference's per-PARAMETER `t`, optim.py:36/:48), so a captured hipGraph stays correct when
 * replayed; lg_counter_add_i64 advances the counter inside the same graph. */
int lg_adam_step_dev_f32(float* p, const float* g, float* m, float* v, int64_t n,
                         double lr, double b1, double b2, double eps,
                         const int64_t* step, int64_t t_mul, int64_t t_add, double gscale, int belief);
int lg_counter_add_i64(int64_t* counter, int64_t delta);

/* All parameters of a model in one launch (groups of 64 parameters per launch beyond that): p, g, m, v are flat buckets holding `nseg` parameters
 * back to back, parameter j occupying [offsets[j], offsets[j+1]); its step number is
 * t = (steps done) * nseg + j + 1.  Same arithmetic as lg_adam_step_dev_f32.
 *   step_slots == 0: step[0] holds the steps done and is only read (advance it with lg_counter_add_i64).
 *   step_slots  > 0: the launch advances the step number itself, with no hand-off between workgroups: `step` points at
 *     2 + step_slots int64 that all hold the steps done (zeros for a new optimizer); step[2 + s] is the private copy of
 *     workgroup s of the launch grid, step[0] the copy readers see (step[1] is unused).  step_slots >= nseg *
 *     ceil(longest parameter / 1024) always suffices. */
int lg_adam_multi_dev_f32(float* p, const float* g, float* m, float* v, int nseg, const int64_t* offsets,
                          double lr, double b1, double b2, double eps,
                          int64_t* step, int64_t step_slots, double gscale, int belief);

/* The rest of a BERT training recipe around that launch: clipping by the global L2 norm, a warmup / linear-decay schedule of
 * the learning rate and decoupled weight decay (AdamW).  optim.py's expression form defines the arithmetic:
 *   lg_grad_norm_clip_f32   ONE launch over the flat gradient bucket:
 *                             out[0] = norm = sqrt(sum_i (g[i] * gscale)^2)      (the product rounded to fp32 first when gscale != 1,
 *                                                                                 squares in fp32, sums of workgroups folded in double)
 *                             out[1] = coef = min(1, max_norm / (norm + 1e-6))   (in double from the fp32 norm, rounded once)
 *                           `partial` is scratch of LG_GRAD_NORM_PARTIALS floats, `ticket` one int that is zero before the first
 *                           call and zero again after every call; both and `out` are device memory the caller keeps.  The
 *                           workgroup that finishes last folds the partial sums in an order that does not depend on timing:
 *                           the same input gives the same bits on every run.  No workgroup waits for another.
 *   lg_adamw_multi_dev_f32  lg_adam_multi_dev_f32 (same buckets, offsets, step slots) with, per element,
 *                             g' = g * gscale (skipped when gscale == 1);  g'' = g' * clip[1] (skipped when clip == NULL)
 *                             m, v and delta as above from g'' with lr_s = lr * factor(steps done) in place of lr
 *                             p += delta + (-(lr_s * weight_decay)) * p    where decay_flags[j] != 0 and weight_decay != 0
 *                             p += delta                                    elsewhere
 *                           lr_s and -(lr_s * weight_decay) are formed in double ON THE DEVICE from the step number the bias
 *                           corrections use, and rounded once: a replayed hipGraph follows the schedule.  schedule_kind 0:
 *                           factor = 1; 1 (warmup-linear): factor(s) = (s + 1) / warmup_steps for s < warmup_steps, else
 *                           max(0, (total_steps - s) / max(1, total_steps - warmup_steps)).  decay_flags: nseg bytes of HOST
 *                           memory (may be NULL when weight_decay == 0), copied into the launch arguments like `offsets`;
 *                           clip: the `out` of lg_grad_norm_clip_f32 (device) or NULL.  With weight_decay == 0, clip == NULL
 *                           and schedule_kind == 0 the result equals lg_adam_multi_dev_f32's bit for bit. */
#define LG_GRAD_NORM_PARTIALS 512
int lg_grad_norm_clip_f32(const float* g, int64_t n, double gscale, double max_norm, float* partial, int* ticket, float* out);
int lg_adamw_multi_dev_f32(float* p, const float* g, float* m, float* v, int nseg, const int64_t* offsets,
                           double lr, double b1, double b2, double eps,
                           int64_t* step, int64_t step_slots, double gscale, int belief,
                           double weight_decay, const uint8_t* decay_flags, const float* clip,
                           int schedule_kind, int64_t warmup_steps, int64_t total_steps);

/* The update applied by the kernel that MAKES the gradient (round 4): `p += compute_delta(p.grad, i)` of optim.py:10-13 / :47-52
 * without a launch of its own.  The reference's optimizer is ~14 tensor expressions per parameter after backward; the fused
 * kernels above made that one launch; these entry points let the backward kernels themselves apply it to the values they are
 * about to store - GEMM epilogues (lg_gemm_f32 / lg_gemm_rowsum_f32 / lg_gemm_fused_f32 on the small tiles: C and the row
 * sums) and lg_head_bwd_f32 (dW, db).  Same arithmetic per element as lg_adam_multi_dev_f32, so the same bits.
 *   lg_adam_plan_create     one parameter's update, p_in -> p_out (p_out != p_in: other workgroups of the producing launch
 *                           still read the old values, e.g. dx = g @ W next to dW = g^T @ x), moments m, v in place, the
 *                           step number read from step_in[0] (t = step_in[0] * t_mul + t_add) and, for ONE plan of an
 *                           optimizer, written as step_out[0] = step_in[0] + 1 (step_out NULL elsewhere; step_out !=
 *                           step_in: an optimizer keeps two plans per parameter, A -> B and B -> A, and alternates).
 *   lg_adam_epilogue_arm    before backward: the next kernel that OVERWRITES `grad` (n floats, dense; beta = 0) applies the
 *                           plan; the gradient itself is still written.  After that, ANY entry point of this library that
 *                           would write into those bytes in the same step - GEMMs, lg_ew, lg_reduce_acc, lg_copy_strided,
 *                           lg_fill_strided, lg_put_axis, lg_scatter_add_axis_f32, lg_scatter_add_rows_f32,
 *                           lg_layernorm_param_grads_f32, lg_gemm_group_colsum_f32, lg_head_bwd_f32; queued calls when they
 *                           are queued - is refused (LG_EINVAL) and writes nothing: for gradients made by ONE kernel per
 *                           step.  Writes before the overwrite, or into gradients no kernel took, are fine.  Host
 *                           bookkeeping only (range compares against the applied plans; none at all while nothing is applied).
 *   lg_adam_epilogue_finish after backward: applies the armed plans no kernel took, in one launch (none when all were
 *                           taken), and disarms everything.  Host bookkeeping only: a step recorded in a hipGraph replays
 *                           as recorded; the directions alternate, so a graph holds an EVEN number of steps. */
int lg_adam_plan_create(void** plan, const float* p_in, float* p_out, float* m, float* v, int64_t n,
                        const int64_t* step_in, int64_t* step_out, int64_t t_mul, int64_t t_add,
                        double lr, double b1, double b2, double eps, double gscale, int belief);
int lg_adam_plan_destroy(void* plan);
int lg_adam_epilogue_arm(const float* grad, int64_t n, const void* plan);
int lg_adam_epilogue_finish(int* applied_by_kernels, int* applied_here);
int lg_adam_epilogue_disarm(void);       /* forget everything armed without applying it (after a failed backward pass) */

/* ---- fused loss ----------------------------------------
 * loss.mse forward (loss.py:4-10) for dense fp32 tensors of n elements:
 *   err[i] = y[i] + (-y_hat[i]);   loss[0] = (sum_i err[i]^2 * (1/n)) * 0.5
 * `err` is what mse.backward multiplies by the upstream gradient (loss.py:11-12). */
int lg_mse_f32(const float* y, const float* y_hat, float* err, float* loss, int64_t n);

/* ---- integer-array indexing along one axis (csrc/index.hip) ------------------------
 * The dense tensor is seen as [outer][axis_len][inner]; `idx` holds n_idx int16/int32/int64 positions on the
 * axis (negative = from the end).  They do on the device what the reference's CPU backend does with numpy
 * (cpu/ops.py:234-255) for Dataset shuffling (data.py:15-21), embedding lookups (examples/bert.py:19-21) and
 * the label pick / update of loss.cross_entropy (loss.py:19, :22); the reference's OpenCL backend has none.
 *   lg_take_axis             dst[outer][n_idx][inner]: dst[o][j][i] = src[o][idx[j]][i]         any itemsize
 *   lg_put_axis              dst[o][idx[j]][i] = val[o][j][i]  (val == NULL: the scalar whose bits are given)
 *   lg_scatter_add_axis_f32  dst[o][idx[j]][i] += src[o][j][i]  (fp32 atomics: repeated indices accumulate;
 *                            their order of addition is not fixed, so sums of 3+ contributions may differ in
 *                            the last bit from run to run - the one non-reproducible kernel of the library)
 * pair_period = n > 0: the paired form `t[range(n), idx]` - idx has n entries, entry (o mod n) belongs to
 * outer position o, and the indexed array is [outer][inner] (no n_idx axis).
 * An index outside [-axis_len, axis_len): take writes all-ones bytes, put / scatter skip it, and the device
 * status flag is raised - the next lg_sync / lg_memcpy_d2h returns LG_EINDEX (numpy raises IndexError at
 * once; a kernel cannot). */
int lg_take_axis(int itemsize, const void* src, int64_t outer, int64_t axis_len, int64_t inner,
                 const void* idx, int idx_itemsize, int64_t n_idx, int64_t pair_period, void* dst);
int lg_put_axis(int itemsize, void* dst, int64_t outer, int64_t axis_len, int64_t inner,
                const void* idx, int idx_itemsize, int64_t n_idx, int64_t pair_period, const void* val, uint64_t scalar_bits);
int lg_scatter_add_axis_f32(float* dst, int64_t outer, int64_t axis_len, int64_t inner,
                            const void* idx, int idx_itemsize, int64_t n_idx, int64_t pair_period, const float* src);

/* Several index arrays / plain integers of one subscript folded into ONE flat index on the device (round 4): out[e] = the
 * row-major position of (idx_0[e], ..., idx_{k-1}[e]) in axes of lengths lens[0..k), e running over the arrays' common broadcast
 * `shape` (idx_strides[j][d] = stride of array j along broadcast dimension d in elements, 0 where it is broadcast; idx[j] NULL:
 * the plain integer constants[j]).  Negative indices count from the end; one out of range raises the device status flag like
 * the kernels above.  lg_mask_nonzero: the flat positions of the non-zero bytes of a boolean mask of n elements, ascending
 * (room for n), and their number - the one value a caller has to read back (it is the length of the result). */
int lg_index_fold(int k, const int64_t* lens, const void* const* idx, const int* idx_itemsize, const int64_t* constants,
                  int ndim, const int64_t* shape, const int64_t* const* idx_strides, int64_t* out);
int lg_mask_nonzero(const void* mask, int64_t n, int64_t* out_positions, int64_t* out_count);

/* ---- self-attention of a short sequence, one launch each way (csrc/attention.hip) ------------------------
 * Per (batch, head): P = softmax((Q K^T) * scale), O = P V (reference examples/bert.py:78-88: scores GEMM, `/ sqrt(d)`,
 * softmax, context GEMM - four kernels through kernels.dot / kernels.atom / the softmax composite), and its backward
 * dV = P^T dO, dS = P o (dO V^T - shift) * scale, dQ = dS K, dK = dS^T Q (dot.backward twice and the softmax composite's
 * backward).  Q, K, V, O, dO, dQ, dK, dV are addressed as (batch, position, head, d): element at X + b * sbX + pos * ldX +
 * head * D + d - the (b, s, heads * D) output of a Linear as it stands, no head-split copies; P is a dense
 * (batch, heads, S, S) tensor, written by the forward (the model returns it) and read by the backward.
 * Supported: D = 32 or 64, S = 32, 64, 96 or 128 (lg_attention_supported); operands 16-byte aligned, pitches multiples of 4.
 * The scaled scores are rounded to fp32 before the softmax and the backward's row shift is formed in double, like the separate
 * kernels (lg_softmax_scaled_f32 / _bwd_f32); sums run in a different order than the GEMM kernels', so values agree with the
 * composite form to rounding, not bit for bit. */
int lg_attention_supported(int64_t S, int64_t D);
int lg_attention_fwd_f32(const float* q, int64_t ldq, int64_t sbq, const float* k, int64_t ldk, int64_t sbk,
                         const float* v, int64_t ldv, int64_t sbv, float* o, int64_t ldo, int64_t sbo, float* p,
                         int64_t batch, int64_t heads, int64_t S, int64_t D, float scale);
int lg_attention_bwd_f32(const float* q, int64_t ldq, int64_t sbq, const float* k, int64_t ldk, int64_t sbk,
                         const float* v, int64_t ldv, int64_t sbv, const float* g, int64_t ldg, int64_t sbg,
                         const float* p, float* dq, int64_t lddq, int64_t sbdq, float* dk, int64_t lddk, int64_t sbdk,
                         float* dv, int64_t lddv, int64_t sbdv, int64_t batch, int64_t heads, int64_t S, int64_t D,
                         float scale);

/* The same two launches for what a tokenizer produces: any S in 1 .. 128 and a key-padding mask (reference
 * examples/bert.py:80-83: `scores + (1.0 - attention_mask) * -10000.0` between the scaling and the softmax; bert.py:341-350
 * feeds a sentence of arbitrary length).  mask: fp32, element (b, j) at mask + b * sbm + j, sbm = 0 for one row shared by
 * the batch (the reference's (1, 1, 1, s) mask), NULL for none; the score of key j is fl(fl(acc * scale) + fl(fl(1 - mask) *
 * -10000)) - the composite's own fp32 arithmetic, so a mask value between 0 and 1 means what it means there, and a mask
 * of ones gives the bits of lg_attention_fwd_f32.  The tiles cover S rounded up to 32; rows >= S are neither read nor
 * written, keys >= S take no part in any sum.  P is dense (batch, heads, S, S) with row pitch S.  The backward needs no
 * mask (it reads P).  Supported: D = 32 or 64, 1 <= S <= 128 (lg_attention_masked_supported); operands as above; a
 * non-NULL mask needs sbm == 0 or sbm >= S. */
int lg_attention_masked_supported(int64_t S, int64_t D);
int lg_attention_masked_fwd_f32(const float* q, int64_t ldq, int64_t sbq, const float* k, int64_t ldk, int64_t sbk,
                                const float* v, int64_t ldv, int64_t sbv, float* o, int64_t ldo, int64_t sbo, float* p,
                                int64_t batch, int64_t heads, int64_t S, int64_t D, float scale,
                                const float* mask, int64_t sbm);
int lg_attention_masked_bwd_f32(const float* q, int64_t ldq, int64_t sbq, const float* k, int64_t ldk, int64_t sbk,
                                const float* v, int64_t ldv, int64_t sbv, const float* g, int64_t ldg, int64_t sbg,
                                const float* p, float* dq, int64_t lddq, int64_t sbdq, float* dk, int64_t lddk, int64_t sbdk,
                                float* dv, int64_t lddv, int64_t sbdv, int64_t batch, int64_t heads, int64_t S, int64_t D,
                                float scale);

/* The same two launches for the lengths beyond what one CU's LDS holds of a (batch, head) pair: any S in 129 .. 512
 * (csrc/attention_long.hip).  Only the 32 x S tile of one block of queries stays in LDS; K, V, Q and dO stream through it in
 * chunks of 128 rows, accumulators stay in registers across the chunks and fold in a fixed order (no float atomics: the same
 * bits every run).  Arguments, mask semantics, addressing, the dense P with row pitch S, what is read and written, and the
 * rounding of scores and row shifts are those of the masked forms above.  Supported: D = 32 or 64, 129 <= S <= 512
 * (lg_attention_long_supported, pure host code). */
int lg_attention_long_supported(int64_t S, int64_t D);
int lg_attention_long_fwd_f32(const float* q, int64_t ldq, int64_t sbq, const float* k, int64_t ldk, int64_t sbk,
                              const float* v, int64_t ldv, int64_t sbv, float* o, int64_t ldo, int64_t sbo, float* p,
                              int64_t batch, int64_t heads, int64_t S, int64_t D, float scale,
                              const float* mask, int64_t sbm);
int lg_attention_long_bwd_f32(const float* q, int64_t ldq, int64_t sbq, const float* k, int64_t ldk, int64_t sbk,
                              const float* v, int64_t ldv, int64_t sbv, const float* g, int64_t ldg, int64_t sbg,
                              const float* p, float* dq, int64_t lddq, int64_t sbdq, float* dk, int64_t lddk, int64_t sbdk,
                              float* dv, int64_t lddv, int64_t sbdv, int64_t batch, int64_t heads, int64_t S, int64_t D,
                              float scale);

/* Attention with dropout of the probabilities inside the two launches, for every length the forms above take: 1 <= S <= 512,
 * D = 32 or 64 (lg_attention_dropout_supported, pure host code).  With keep / s / T of the random stream below (lg_dropout_*):
 *   P  = softmax(scores)                  written to `p` UNDROPPED, as above
 *   Pd = keep ? fl(P * s) : +0.0          the operand of the context, never leaves the CU:   O = Pd V,   dV = Pd^T dO
 *   dP = keep ? fl((dO V^T) * s) : +0.0   then dS = P o (dP - shift) * scale as above (shift in double from the masked dP)
 * One forward is ONE call of the stream (`draws` advances by 1; the launch reads `draws` from device memory, so a captured graph
 * draws a fresh mask at every replay) and element i of the call is the flat index into the dense (batch, heads, S, S)
 * probabilities, i = ((b * heads + head) * S + row) * S + col: the mask `P.dropout(p)` of the composite form draws.  The forward
 * writes the call's number to base_out (one word of device memory); the backward reads the seed from the generator's state and the
 * number from `base`, and draws nothing.  The host picks the kernels: no mask, S % 32 == 0 and S <= 128 the plain ones, otherwise
 * up to 128 the masked ones, beyond the long ones.  Arguments before `p` as for the masked forms and under their rules;
 * 0 <= p < 1 (p == 0 keeps everything and still draws once); base_out / base non-NULL; batch >= 1 in the forward. */
int lg_attention_dropout_supported(int64_t S, int64_t D);
int lg_attention_dropout_fwd_f32(const float* q, int64_t ldq, int64_t sbq, const float* k, int64_t ldk, int64_t sbk,
                                 const float* v, int64_t ldv, int64_t sbv, float* o, int64_t ldo, int64_t sbo, float* p,
                                 int64_t batch, int64_t heads, int64_t S, int64_t D, float scale,
                                 const float* mask, int64_t sbm, double prob, uint64_t* base_out);
int lg_attention_dropout_bwd_f32(const float* q, int64_t ldq, int64_t sbq, const float* k, int64_t ldk, int64_t sbk,
                                 const float* v, int64_t ldv, int64_t sbv, const float* g, int64_t ldg, int64_t sbg,
                                 const float* p, float* dq, int64_t lddq, int64_t sbdq, float* dk, int64_t lddk, int64_t sbdk,
                                 float* dv, int64_t lddv, int64_t sbdv, int64_t batch, int64_t heads, int64_t S, int64_t D,
                                 float scale, double prob, const uint64_t* base);

/* The forward with a causal mask, for every length: 1 <= S <= 512, D = 32 or 64 (lg_attention_causal_supported, pure host code).
 * Query i sees keys j <= i only: a key j > i takes no part in the max or the sum of row i, and P[i][j] = +0.0 is STORED for it
 * (the dense (batch, heads, S, S) tensor is what the model returns and what the backward reads).  The values are those of the
 * composite `scores + (1 - tril) * -10000` added after the key-padding bias whenever |scaled score| << 10000.  `mask` composes:
 * a padded key j <= i keeps its bias; key 0 is visible to every row, so no row is empty.  Up to 128 positions the masked forms'
 * kernels run (also at multiples of 32 and with mask == NULL), beyond them the long forms'; key blocks wholly above the diagonal
 * of a block of queries cost no MFMAs, and a row depends on S, its block and positions <= i only.
 *   base_out == NULL, prob == 0   no dropout, nothing drawn; an empty batch returns LG_OK
 *   base_out != NULL              dropout of P as in lg_attention_dropout_fwd_f32, under that entry's rules (one call of the
 *                                 stream over the whole dense tensor, element i at flat index i; a zero stays zero; batch >= 1)
 *   base_out == NULL, prob != 0   LG_EINVAL
 * Arguments as for lg_attention_dropout_fwd_f32, checked in its order.  There is no causal backward: P is zero above the
 * diagonal, so dS = P o (dP - shift) * scale is zero there, and the backward of a causal forward is the backward entry of the
 * same length and dropout: lg_attention_bwd_f32 / _masked_ / _long_ / _dropout_bwd_f32. */
int lg_attention_causal_supported(int64_t S, int64_t D);
int lg_attention_causal_fwd_f32(const float* q, int64_t ldq, int64_t sbq, const float* k, int64_t ldk, int64_t sbk,
                                const float* v, int64_t ldv, int64_t sbv, float* o, int64_t ldo, int64_t sbo, float* p,
                                int64_t batch, int64_t heads, int64_t S, int64_t D, float scale,
                                const float* mask, int64_t sbm, double prob, uint64_t* base_out);

/* ---- attention of ONE new token against a key / value cache (csrc/decode.hip) -----------------------------
 * Incremental decoding of the causal model: with t = *pos, the position of the new token, read BY THE KERNEL from one word in
 * device memory (a captured step replays with what the word holds then),
 *   - k_new is written to row t of k_cache and v_new to row t of v_cache, bit for bit;
 *   - o = softmax(scale * q K[0..t]^T + (1 - mask[0..t]) * -10000) V[0..t] per (batch, head); keys j > t take no part in the max
 *     or the sum, exactly as in lg_attention_causal_fwd_f32;
 *   - p, if given, holds the t + 1 probabilities followed by exact +0.0 up to `capacity`.
 * Rows j > t of the caches are neither read nor written; row t is taken from k_new / v_new, not read back.  One workgroup per
 * (batch, head) pair, K / V rows straight into registers, no matrix cores; every fold in a fixed order (same bits every run).
 * t < 0 or t >= capacity: the launch writes nothing and raises the device status flag - LG_EINDEX at the next lg_sync /
 * lg_memcpy_d2h, as for the index kernels.  Supported: D = 32 or 64, 1 <= capacity <= 512 (lg_attention_decode_supported, pure
 * host code).  Checked in this order, each LG_EINVAL, before anything is launched: D / capacity; a pitch that is no multiple of
 * 4 or a base that is not 16-byte aligned; ldc < heads * D; a mask with 0 < sbm < capacity. */
int lg_attention_decode_supported(int64_t capacity, int64_t D);
int lg_attention_decode_f32(const float* q, int64_t sbq,             /* the new token's rows: element (b, head, d) at x + b*sb + head*D + d */
                            const float* k_new, int64_t sbk, const float* v_new, int64_t sbv,
                            float* k_cache, float* v_cache, int64_t ldc, int64_t sbc,   /* (batch, capacity, heads*D), addressing as above */
                            const int32_t* pos,                      /* ONE word in device memory: the position of the new token */
                            float* o, int64_t sbo,                   /* context (batch, heads*D) */
                            float* p,                                /* NULL, or probabilities (batch, heads, capacity), dense */
                            int64_t batch, int64_t heads, int64_t capacity, int64_t D, float scale,
                            const float* mask, int64_t sbm);         /* key-padding mask over the capacity; NULL = none */

/* ---- attention of m NEW tokens against a filled key / value cache (csrc/extend.hip) --------------------------
 * Appending to a cache that already holds t = *pos tokens (a second prompt, a prompt prefilled in pieces, a continuation to
 * score, drafted tokens to verify): t is read BY THE KERNEL from one word in device memory, m is a host argument, and
 *   - rows i = 0 .. m - 1 of k_new / v_new are written to rows t + i of k_cache / v_cache, bit for bit;
 *   - for query row i: o_i = softmax(scale * q_i K[0..t+i]^T + (1 - mask[0..t+i]) * -10000) V[0..t+i] per (batch, head), where
 *     K[j] / V[j] is the cache's row for j < t and row j - t of k_new / v_new for j >= t - taken from the new-token buffers,
 *     never read back from the cache; keys j > t + i take no part in row i's max or sum, as in lg_attention_causal_fwd_f32;
 *   - p, if given, is dense (batch, heads, m, capacity): row i holds its t + i + 1 probabilities, then exact +0.0 up to `capacity`.
 * Cache rows >= t + m are neither read nor written, rows t .. t + m - 1 are written and never read: what they hold before the
 * launch (NaN included) reaches nothing.  One workgroup per (block of 32 query rows, head, batch) on the fp32 matrix cores, K
 * then V streamed through LDS in chunks of 128 rows up to the block's last visible key; every fold in a fixed order (same bits
 * every run).  t < 0 or t + m > capacity: the launch writes nothing and raises the device status flag - LG_EINDEX at the next
 * lg_sync / lg_memcpy_d2h, as for the decode and index kernels.  Supported: D = 32 or 64, 1 <= m <= capacity <= 512
 * (lg_attention_extend_supported, pure host code).  Checked in this order, each LG_EINVAL, before anything is launched: D / m /
 * capacity; (batch == 0 returns LG_OK here;) a pitch that is negative or no multiple of 4, or a base (p included) that is not
 * 16-byte aligned; ldc < heads * D; a mask with 0 < sbm < capacity; k_new or v_new overlapping a cache. */
int lg_attention_extend_supported(int64_t m, int64_t capacity, int64_t D);
int lg_attention_extend_f32(const float* q, int64_t ldq, int64_t sbq,   /* the new tokens' rows: element (b, i, head, d) at x + b*sb + i*ld + head*D + d */
                            const float* k_new, int64_t ldk, int64_t sbk, const float* v_new, int64_t ldv, int64_t sbv,
                            float* k_cache, float* v_cache, int64_t ldc, int64_t sbc,   /* (batch, capacity, heads*D) */
                            const int32_t* pos,                      /* ONE word in device memory: the position of new token 0 */
                            float* o, int64_t ldo, int64_t sbo,      /* context (batch, m, heads*D), addressed like q */
                            float* p,                                /* NULL, or probabilities (batch, heads, m, capacity), dense */
                            int64_t batch, int64_t heads, int64_t m, int64_t capacity, int64_t D, float scale,
                            const float* mask, int64_t sbm);         /* key-padding mask over the capacity; NULL = none */

/* ---- a position per sequence: ragged batches in the key / value cache (csrc/decode.hip, extend.hip, commit.hip) -------------
 * lg_attention_decode_rows_f32 / lg_attention_extend_rows_f32 take the arguments of lg_attention_decode_f32 / _extend_f32 with ONE
 * difference: `pos` points to `batch` contiguous int32 words in device memory and batch element b uses t = pos[b].  Everything
 * said above holds per batch element with its own t - the rows read and written, row t .. from the new-token buffers and never
 * read back, cache rows beyond reaching nothing (NaN included), +0.0 beyond the diagonal of p, every fold in a fixed order: a
 * batch element's bits are those of the one-word entry called on it alone at batch 1.  They are the same kernels (the position
 * is addressed with a pitch of 1 word in place of 0).  A batch element whose t is out of range (t < 0, t >= capacity for decode,
 * t + m > capacity for extend) writes nothing and raises the status flag; the OTHER elements of the launch are computed as
 * usual.  Host refusals as for the one-word entries; all four also refuse (LG_EINVAL) position words that overlap a cache. */
int lg_attention_decode_rows_f32(const float* q, int64_t sbq, const float* k_new, int64_t sbk, const float* v_new, int64_t sbv,
                                 float* k_cache, float* v_cache, int64_t ldc, int64_t sbc,
                                 const int32_t* pos,                 /* `batch` words in device memory: the position of each new token */
                                 float* o, int64_t sbo, float* p, int64_t batch, int64_t heads, int64_t capacity, int64_t D, float scale,
                                 const float* mask, int64_t sbm);
int lg_attention_extend_rows_f32(const float* q, int64_t ldq, int64_t sbq, const float* k_new, int64_t ldk, int64_t sbk,
                                 const float* v_new, int64_t ldv, int64_t sbv, float* k_cache, float* v_cache, int64_t ldc, int64_t sbc,
                                 const int32_t* pos,                 /* `batch` words in device memory: the position of each row's new token 0 */
                                 float* o, int64_t ldo, int64_t sbo, float* p, int64_t batch, int64_t heads, int64_t m, int64_t capacity,
                                 int64_t D, float scale, const float* mask, int64_t sbm);
/* lg_attention_extend_counts_f32: the `_rows` entry with `count`, `batch` contiguous int32 words in device memory.  Batch element b
 * has n = count[b] real new tokens among the m rows it is given; with t = pos[b]:
 *   - n < 0, n > m, t < 0 or t + n > capacity raises the status flag, nothing is written for that element, the others are
 *     computed; n = 0 is legal for any 0 <= t <= capacity, and t + m > capacity is no error when t + n fits;
 *   - query rows 0 .. n - 1 (context, p, cache rows t .. t + n - 1) are bit for bit what lg_attention_extend_rows_f32 gives for
 *     that element alone with m = n; no other cache row is written (NaN there stays NaN);
 *   - rows i >= n of o and of p (if given) are +0.0: what the launch returns is fully determined.  A workgroup whose 32 query rows
 *     start at or beyond n clears them and returns: no load, no MFMA.
 * Host refusals as for the `_rows` entry, then: count NULL or not 4-byte aligned, count overlapping a cache, count overlapping pos. */
int lg_attention_extend_counts_f32(const float* q, int64_t ldq, int64_t sbq, const float* k_new, int64_t ldk, int64_t sbk,
                                   const float* v_new, int64_t ldv, int64_t sbv, float* k_cache, float* v_cache, int64_t ldc, int64_t sbc,
                                   const int32_t* pos,               /* `batch` words: the position of each row's new token 0 */
                                   const int32_t* count,             /* `batch` words: the real new tokens of each row, 0 .. m */
                                   float* o, int64_t ldo, int64_t sbo, float* p, int64_t batch, int64_t heads, int64_t m, int64_t capacity,
                                   int64_t D, float scale, const float* mask, int64_t sbm);
/* The per-row bookkeeping of one decode step in one launch, one thread per row, any batch >= 1.  For each row r with
 * done[r] == 0: p = pos[r] + 1; if p < 0 or p >= columns the status flag is raised (LG_EINDEX at the next lg_sync /
 * lg_memcpy_d2h) and the row is left untouched; otherwise pos[r] = p, token[r] = nxt[r * nxt_pitch], out_ids[r * out_pitch + p] =
 * that id, and done[r] = 1 if eos_id >= 0 and the id equals it.  A row with done[r] != 0: nothing is written at all.  Refused
 * (LG_EINVAL): a NULL operand (`done` included), a misaligned one, nxt_pitch < 1, out_pitch < columns, any two operands that
 * overlap. */
int lg_decode_commit_i32(const int32_t* nxt, int64_t nxt_pitch,      /* the step's new ids, row r at nxt + r * nxt_pitch */
                         int32_t* token,                             /* (batch) the step's input ids */
                         int32_t* out_ids, int64_t out_pitch, int64_t columns,   /* (batch, columns), row pitch in elements */
                         int32_t* pos, int32_t* done,                /* (batch) each */
                         int64_t batch, int32_t eos_id);             /* eos_id < 0: none */
/* The slot bookkeeping of one step of continuous batching in one launch (csrc/serve.hip): one workgroup, one thread per cache
 * slot, 1 <= slots <= 1024.  The definition is the sequential loop of `CpuTensor.serve_commit` (autograd/cpu/ops.py), for slot
 * s = 0 .. slots - 1 in this order: (1) r = req[s]; if r >= 0, t = pos[s] + count[s]; with t < prompt_len[r] the slot takes the next
 * n = min(m, prompt_len[r] - t) tokens of its prompt, otherwise nxt[s] becomes out[r, out_len[r]++] and - eos_id, or the budget
 * used up - finishes the request (queue[1] += 1, the slot is free) or is the slot's one token (n = 1).  (2) A free slot takes
 * request queue[0]++ while that is < N: t = 0, the first n = min(m, prompt_len[r]) tokens of its prompt.  (3) Otherwise n = 0,
 * t = 0.  (4) req[s] = r, pos[s] = t, count[s] = n, ids[s] = the n tokens then 0, position_ids[s] = t .. t + n - 1 then 0,
 * last[s] = s * m + max(n - 1, 0).  The kernel decides the slots in parallel and takes the admission order from an exclusive
 * scan over the free slots: the result equals the loop's, a slot freed in a launch is admitted to in the same launch.
 * A slot that would leave its bounds (t + n > capacity, a token beyond column G of out, r >= N, t < 0, prompt tokens beyond column
 * P) raises the status flag - LG_EINDEX at the next lg_sync / lg_memcpy_d2h -, gets count[s] = 0 and nothing else of the slot is
 * written.  Refused (LG_EINVAL): sizes outside their ranges, a NULL or misaligned operand, prompt_pitch < P, out_pitch < G,
 * nxt_pitch < 1, any two operands that overlap.  ids and position_ids are dense (slots, m). */
int lg_serve_commit_i32(const int32_t* nxt, int64_t nxt_pitch,       /* the tokens just drawn, slot s at nxt + s * nxt_pitch */
                        const int32_t* prompts, int64_t prompt_pitch, int64_t P,   /* (N, P) right-padded ids, row pitch in elements */
                        const int32_t* prompt_len, const int32_t* budget,          /* (N) each */
                        int32_t* out, int64_t out_pitch, int64_t G,  /* (N, G) generated tokens, row pitch in elements */
                        int32_t* out_len,                            /* (N) */
                        int32_t* queue, int64_t N,                   /* {next request to admit, requests finished} */
                        int32_t* req, int32_t* pos, int32_t* count,  /* (slots) each */
                        int32_t* ids, int32_t* position_ids,         /* (slots, m) dense each */
                        int32_t* last,                               /* (slots) */
                        int64_t slots, int64_t m, int64_t capacity, int32_t eos_id);   /* eos_id < 0: none */
/* ---- token-packed serving steps: one flat token budget for all slots (csrc/extend.hip, serve_packed.hip) -------------------------
 * lg_attention_extend_packed_f32: the step's tokens of ALL cache slots lie in flat operands of T rows (q, k_new, v_new, o: row i
 * at x + i * ld, no batch pitch; p NULL or (heads, T, capacity) dense), and `cu`, slots + 1 int32 words in device memory, says
 * whose they are: slot z owns rows cu[z] .. cu[z + 1] - 1, n = cu[z + 1] - cu[z] of them, at most m_max; rows cu[slots] .. T - 1
 * belong to nobody.  The caches (slots, capacity, heads * D), pos (slots words) and the mask are addressed by the slot as the
 * `_rows` entry addresses them by the batch element.  It is the `_rows` kernel with the slot's first row in place of a batch
 * pitch, grid (ceil(m_max / 32), heads, slots + 1):
 *   - slot z with t = pos[z]: its context rows, its rows of p (exact +0.0 beyond column t + i of row cu[z] + i) and cache rows
 *     t .. t + n - 1 are bit for bit what lg_attention_extend_rows_f32 gives for it alone at batch 1 with m = n on those rows; no
 *     other cache row is written; a workgroup whose 32 query rows start at or beyond n returns before any load;
 *   - the last slice of the grid sets rows cu[slots] .. T - 1 of o and of p (if given) to +0.0;
 *   - a slot with cu[z] < 0, n < 0, n > m_max, cu[z + 1] > T, t < 0 or t + n > capacity raises the status flag (LG_EINDEX at the
 *     next lg_sync / lg_memcpy_d2h) and writes nothing, the others are computed; cu[slots] outside 0 .. T: the flag, and the
 *     clearing slice writes nothing.
 * Supported: D = 32 or 64, 1 <= m_max <= capacity <= 512, 1 <= T < 2^30 (T may exceed the capacity), slots <= 65534.  Host
 * refusals (LG_EINVAL) as for the `_counts` entry, with cu in place of count: cu NULL, misaligned, overlapping a cache, pos, q,
 * k_new, v_new, o or p. */
int lg_attention_extend_packed_f32(const float* q, int64_t ldq, const float* k_new, int64_t ldk, const float* v_new, int64_t ldv,   /* (T, heads*D) rows */
                                   float* k_cache, float* v_cache, int64_t ldc, int64_t sbc,   /* (slots, capacity, heads*D) */
                                   const int32_t* pos,               /* `slots` words: the position of each slot's new token 0 */
                                   const int32_t* cu,                /* `slots + 1` words: the first row of each slot, then the rows in use */
                                   float* o, int64_t ldo,            /* context (T, heads*D) */
                                   float* p,                         /* NULL, or probabilities (heads, T, capacity), dense */
                                   int64_t slots, int64_t heads, int64_t T, int64_t m_max, int64_t capacity, int64_t D, float scale,
                                   const float* mask, int64_t sbm);  /* key-padding mask (slots, capacity); sbm = 0: one row for all */
/* lg_serve_commit_packed_i32: lg_serve_commit_i32 for a token-packed step of T rows, T >= slots (csrc/serve_packed.hip).  The
 * definition is the loop of `CpuTensor.serve_commit_packed` (autograd/cpu/ops.py).  Steps (1) and (2) are those of
 * lg_serve_commit_i32 with m = chunk and give every slot its request r, its position t and the tokens it WANTS: min(chunk,
 * prompt_len[r] - t) of its prompt (a prefilling slot, a slot just admitted included), the one token just drawn (a decoding
 * slot), or none.  (3) The budget: a decoding slot gets its token; with R = T - (decoding slots), the prefilling slots take
 * n = min(want, what is left of R) in slot order.  A prefilling slot granted 0 keeps its request and its position, gets
 * count = 0 and asks again in the next step.  (4) cu = the exclusive sum of the n in slot order, cu[slots] = their total;
 * req[s] = r, pos[s] = t, count[s] = n, ids[cu[s] + i] = token i of the slot, position_ids[cu[s] + i] = t + i, both 0 in rows
 * >= cu[slots]; last[s] = min(cu[s] + max(n - 1, 0), T - 1).  A slot that would leave its bounds (those of lg_serve_commit_i32,
 * with t + want > capacity) raises the status flag, gets count[s] = 0, takes no rows - it counts neither as decoding nor as
 * prefilling - and nothing else of it is written.  One workgroup, one thread per slot; three exclusive sums in slot order (free
 * slots, prefill wants, grants).  Refused (LG_EINVAL): as lg_serve_commit_i32, T < slots, chunk < 1, cu among the operands that
 * must not overlap.  ids and position_ids are dense (T), cu dense (slots + 1). */
int lg_serve_commit_packed_i32(const int32_t* nxt, int64_t nxt_pitch, const int32_t* prompts, int64_t prompt_pitch, int64_t P,
                               const int32_t* prompt_len, const int32_t* budget, int32_t* out, int64_t out_pitch, int64_t G,
                               int32_t* out_len, int32_t* queue, int64_t N,
                               int32_t* req, int32_t* pos, int32_t* count,   /* (slots) each */
                               int32_t* cu,                          /* (slots + 1) */
                               int32_t* ids, int32_t* position_ids,  /* (T) dense each */
                               int32_t* last,                        /* (slots) */
                               int64_t slots, int64_t T, int64_t chunk, int64_t capacity, int32_t eos_id);   /* eos_id < 0: none */
/* ---- a paged key / value cache: block tables, a device allocator, a shared prefix (csrc/paged.hip, serve_paged.hip) -------------
 * lg_attention_extend_paged_f32: lg_attention_extend_counts_f32 with the caches POOLS of num_blocks blocks of B = 1 << log2_block
 * rows (pool row r at x + r * ldc, no batch pitch; 4 <= B <= 128) and `block_table`, (batch, max_blocks) dense int32 words in
 * device memory: position j of batch element b is pool row block_table[b, j >> log2_block] * B + (j & (B - 1)), for the keys
 * j < t that are streamed and for the count[b] new rows written at t ..; capacity = max_blocks * B <= 512.  Element b is bit for
 * bit (o, p, the new rows' bytes) what the counts entry gives on a contiguous (capacity, width) cache that holds the same rows.
 * Each workgroup reads its element's table once and checks words 0 .. ceil((t + count) / B) - 1 before it forms an address: a
 * word outside 0 .. num_blocks - 1 makes the element bad like a bad position (nothing written, status flag raised, the other
 * elements computed); the words behind may hold anything and are not used.  No row below t is written, so two elements may name
 * the same block where it lies wholly below both positions; a block no table names is not touched.  Refused (LG_EINVAL): as
 * the counts entry, B / max_blocks / num_blocks outside their ranges, and any overlap of what is written (pools, o, p) with
 * another operand (pools, new rows, pos, count, block_table, o, p), or of pos with count. */
int lg_attention_extend_paged_f32(const float* q, int64_t ldq, int64_t sbq, const float* k_new, int64_t ldk, int64_t sbk,
                                  const float* v_new, int64_t ldv, int64_t sbv,
                                  float* k_pool, float* v_pool, int64_t ldc,      /* (num_blocks * B, heads*D) rows each */
                                  const int32_t* pos, const int32_t* count,       /* (batch) each */
                                  const int32_t* block_table,                     /* (batch, max_blocks) dense */
                                  float* o, int64_t ldo, int64_t sbo, float* p, int64_t batch, int64_t heads, int64_t m,
                                  int64_t max_blocks, int64_t num_blocks, int64_t log2_block, int64_t D, float scale,
                                  const float* mask, int64_t sbm);
/* lg_attention_extend_paged_bf16_f32 (csrc/paged_bf16.hip): lg_attention_extend_paged_f32 over pools of BFLOAT16 words, 2 bytes
 * an element (ldc counts elements).  With r(x) = x rounded to bfloat16 (nearest, ties to even, kept as fp32), bits(x) = the
 * upper 16 bits of r(x) ((u >> 16) | 0x0040 for a NaN) and widen(w) = w << 16 as fp32: o and p are bit for bit what
 * lg_attention_extend_paged_f32 returns on (q, r(k_new), r(v_new), widen(pools), ...), and the launch writes bits(k_new[b, i]) /
 * bits(v_new[b, i]) to the pool rows of positions t .. t + count[b] - 1 and no other byte of the pools.  Every key and value
 * is attended to as r of what it was given as, whether an earlier launch stored it or this one brings it; q is not rounded.
 * Bounds as lg_attention_extend_paged_f32.  Refused (LG_EINVAL, nothing launched): as lg_attention_extend_paged_f32, with the
 * pools 8-byte aligned, ldc a multiple of 4 elements and >= heads * D, and the overlaps taken at 2 bytes a pool element. */
int lg_attention_extend_paged_bf16_f32(const float* q, int64_t ldq, int64_t sbq, const float* k_new, int64_t ldk, int64_t sbk,
                                       const float* v_new, int64_t ldv, int64_t sbv,
                                       uint16_t* k_pool, uint16_t* v_pool, int64_t ldc,  /* (num_blocks * B, heads*D) rows each */
                                       const int32_t* pos, const int32_t* count,       /* (batch) each */
                                       const int32_t* block_table,                     /* (batch, max_blocks) dense */
                                       float* o, int64_t ldo, int64_t sbo, float* p, int64_t batch, int64_t heads, int64_t m,
                                       int64_t max_blocks, int64_t num_blocks, int64_t log2_block, int64_t D, float scale,
                                       const float* mask, int64_t sbm);
/* lg_serve_commit_paged_i32: lg_serve_commit_i32 over a paged cache (csrc/serve_paged.hip); capacity = max_blocks << log2_block.
 * The definition is the loop of `CpuTensor.serve_commit_paged` (autograd/cpu/ops.py).  `free_stack` (num_blocks + 1): word 0 the
 * number n of free blocks, words 1 .. n their indices, the top at word n; held (slots): the blocks a slot's table names;
 * F = prefix_blocks: blocks 0 .. F - 1 are shared by every request and never on the stack.  A slot whose request has just
 * finished pushes block_table[s, F .. held[s] - 1] (slot order, table order), its row becomes -1 and held[s] = 0.  Free slots
 * are then offered the waiting requests in slot and queue order: request r needs ceil((prompt_len[r] + budget[r] - 1) / B) - F
 * blocks; the first that needs more than the stack holds ends the admission of this commit (no overtaking); otherwise the slot
 * pops them into table words F .., takes 0 .. F - 1 in front, held[s] = F + need, and starts at position F * B with the prompt's
 * tokens F * B ...  Raises the status flag (count[s] = 0, nothing else of the slot written): the bounds of lg_serve_commit_i32,
 * held outside 0 .. max_blocks, a released word outside 0 .. num_blocks - 1, free_stack[0] leaving 0 .. num_blocks, a request
 * with need < 0, F + need > max_blocks or no prompt token behind the prefix.  One workgroup, one thread per slot. */
int lg_serve_commit_paged_i32(const int32_t* nxt, int64_t nxt_pitch, const int32_t* prompts, int64_t prompt_pitch, int64_t P,
                              const int32_t* prompt_len, const int32_t* budget, int32_t* out, int64_t out_pitch, int64_t G,
                              int32_t* out_len, int32_t* queue, int64_t N,
                              int32_t* req, int32_t* pos, int32_t* count,   /* (slots) each */
                              int32_t* ids, int32_t* position_ids,  /* (slots, m) dense each */
                              int32_t* last,                        /* (slots) */
                              int32_t* block_table,                 /* (slots, max_blocks) dense */
                              int32_t* held, int32_t* free_stack,   /* (slots), (num_blocks + 1) */
                              int64_t slots, int64_t m, int64_t max_blocks, int64_t num_blocks, int64_t log2_block,
                              int64_t prefix_blocks, int32_t eos_id);   /* eos_id < 0: none */
/* The bookkeeping of one step of speculative decoding by prompt lookup in one launch (csrc/speculate.hip): one workgroup of 256
 * threads per row, 1 <= batch < 2^24.  The definition is the loop of `CpuTensor.speculate_commit` (autograd/cpu/ops.py), for each
 * row r on its own: (1) done[r] != 0: count[r] = 0, nothing else.  (2) c = count[r], p = pos[r]; unless 1 <= c <= m, p >= 0 and
 * p + c <= end[r] <= columns - 1 the status flag is raised - LG_EINDEX at the next lg_sync / lg_memcpy_d2h -, count[r] = 0 and
 * nothing else of the row is written.  (3) a = the leading j in 0 .. c - 2 with ids[r, j + 1] == tgt[r, j]; the row emits
 * e = a + 1 tokens tgt[r, 0 .. e), cut behind the first one that equals eos_id >= 0 (the row then stops).  (4) out_ids[r, p + 1 ..
 * p + e] = those tokens, pos[r] = p += e, stats[1] += c - 1, stats[2] += a.  (5) Stopped or p == end[r]: done[r] = 1, stats[0] += 1,
 * count[r] = 0.  (6) Otherwise, with L = p + 1, seq = out_ids[r, 0 .. L) and cap = min(draft, end[r] - p - 1): for n = max_ngram
 * down to min_ngram with L >= n + 1 the largest q <= L - n - 1 with seq[q .. q + n) == seq[L - n .. L), the first n that has one
 * wins, the drafts are seq[q + n .. min(q + n + cap, L)); ids[r] = seq[p], the drafts, then 0; count[r] = 1 + their number;
 * position_ids[r, i] = p + i for i < count[r], else 0.  The candidate starts are split over the threads and the largest match is
 * a fold of fixed shape over integers; stats takes integer atomic adds.  The sequence is staged in LDS for columns <= 4096; wider
 * rows are served as well, read from memory.  Refused (LG_EINVAL): sizes outside their ranges, draft outside 0 .. m - 1, n-gram
 * bounds that are not 1 <= min <= max, a NULL or misaligned operand, out_pitch < columns, any two operands that overlap.  Every
 * operand but out_ids is dense. */
int lg_speculate_commit_i32(const int32_t* tgt,                      /* (batch, m) the tokens drawn from the step's logits */
                            int32_t* ids, int32_t* count, int32_t* position_ids,   /* (batch, m), (batch), (batch, m): the step's inputs, then the next step's */
                            int32_t* out_ids, int64_t out_pitch, int64_t columns,  /* (batch, columns), row pitch in elements */
                            int32_t* pos, const int32_t* end, int32_t* done,       /* (batch) each */
                            int32_t* stats,                          /* {rows finished, tokens drafted, drafts accepted} */
                            int64_t batch, int64_t m, int64_t draft, int64_t max_ngram, int64_t min_ngram,
                            int32_t eos_id);                         /* eos_id < 0: none */
/* One step of beam search in one launch (csrc/beam.hip): beams are rows, group g is rows g * w .. g * w + w - 1 best first,
 * w = num_beams in 1 .. 8, rows a multiple of w, w <= vocab < 2^22.  The definition is the loop of `CpuTensor.beam_step`
 * (autograd/cpu/ops.py), for each group on its own: (1) a row with pos < 0 or a live row (done == 0) with pos + 1 >= columns: the
 * group keeps every byte, parent is the identity and the status flag is raised - LG_EINDEX at the next lg_sync / lg_memcpy_d2h.
 * (2) A group that is all done keeps every byte, parent is the identity.  (3) A live beam i offers scores[i] + log_softmax(x)[j]
 * for every j, a done beam offers itself once, at flat index i * vocab.  (4) The w largest, ties to the smaller flat index
 * i * vocab + j, best first.  (5) Slot n taking (s, i, j): parent[n] = g * w + i; from a done beam a copy of row i (score, token,
 * pos, done = 1, out_ids columns 0 .. pos[i]); otherwise out_ids columns 0 .. pos[i] of row i, column pos[i] + 1 = j, pos =
 * pos[i] + 1, token = j, scores = s, done = (j == eos_id >= 0).  (6) stats[0] += 1 when the group goes from some beam live to all
 * done, stats[1] += the slots whose parent is not themselves.  Grid (w, rows / w): a workgroup per row reads it once in 16-byte
 * loads, keeps its top w as integer keys, sums the exponentials as 64-bit integers (exact in any order) and publishes w keys and
 * the beam's one constant c_i = scores[i] - max - log(sum), a double; a candidate is fp32(x[j] + c_i).  The last workgroup of a group to
 * arrive (handoff.h) ranks the w * w survivors and commits, a thread per column of out_ids across the group's rows.  Refused
 * (LG_EINVAL): sizes outside their ranges, a NULL or misaligned operand, a pitch below the row length, any two operands that
 * overlap.  logits and out_ids may have any row pitch; every other operand is dense. */
int lg_beam_step_f32(const float* logits, int64_t logits_pitch,      /* (rows, vocab), row pitch in elements */
                     float* scores, int32_t* parent, int32_t* token, /* (rows) each */
                     int32_t* out_ids, int64_t out_pitch, int64_t columns,  /* (rows, columns), row pitch in elements */
                     int32_t* pos, int32_t* done,                    /* (rows) each */
                     int32_t* stats,                                 /* {groups finished, slots that changed their beam} */
                     int64_t rows, int64_t vocab, int64_t num_beams,
                     int32_t eos_id);                                /* eos_id < 0: none */
/* The rows of up to 64 cache tensors follow their beams in one launch (csrc/beam.hip; nn.KVCache.reorder, `CpuTensor.kv_reorder`):
 * element (r, j, c) of tensor t at tensors[t] + r * sbc + j * ldc + c, `tensors` a HOST array of device pointers that travel by
 * value in the kernel's arguments.  For each group of w = num_beams rows, with L = max pos over the group (at most capacity): row n
 * becomes the old row parent[n] at positions j < L, in place; positions >= L and a group whose parents are the identity are not
 * touched (no cache load).  A parent outside its group writes nothing for that group and raises the status flag.  Refused
 * (LG_EINVAL): more than 64 tensors, num_beams outside 1 .. 8, rows no multiple of it, width no multiple of 4, pitches below the
 * row / the sequence or no multiple of 4, a NULL or misaligned operand (tensors: 16 bytes), tensors that overlap each other or
 * parent / pos. */
int lg_beam_reorder_f32(float* const* tensors, int64_t n_tensors, int64_t ldc, int64_t sbc, int64_t capacity, int64_t width,
                        const int32_t* parent, const int32_t* pos, int64_t rows, int64_t num_beams);

/* ---- two independent products in one launch ----------------------------------------------------------
 * lg_gemm_pair_begin(); <product 1>; <product 2>; lg_gemm_pair_end();   with products issued through
 * lg_gemm_f32 / lg_gemm_rowsum_f32 / lg_gemm_fused_f32.  If the first resolves to the 64x64 tile with an
 * M-contiguous A and N-contiguous B (dW = g^T @ x of nn.Linear's backward) and the second to the 64x64 tile
 * with a K-contiguous A and N-contiguous B (dx = g @ W), neither is launched until _end, which launches both
 * as ONE grid: their workgroups share the CUs and hide each other's waits, and one launch floor disappears
 * (dot.backward of the reference is two kernels.dot calls: opencl/ops.py:127-132).  Any other product inside
 * the bracket runs as usual, after whatever was pending - results never depend on the bracket.  The two
 * products must not read each other's outputs. */
int lg_gemm_pair_begin(void);
int lg_gemm_pair_end(void);
/* THREE products in one launch: two of the first kind followed by one of the second - the backward pass of
 * `Linear -> relu -> skinny Linear -> mse` once the hidden layer's gradient exists: dW2 (+ db2) = err^T @ relu(pre) of the skinny
 * output layer (a skinny first-kind product takes the 64x64 tile inside a collecting bracket), then the hidden layer's dW1 (+ db1)
 * and dx.  The bracket may stay open between the calls (the tape runs relu.backward in between); whatever makes results visible
 * to the host or to a graph (lg_sync, device-to-host copies, graph launch, the end of a capture) launches what has been
 * collected so far, as single launches / a pair, and the bracket goes on collecting.
 * lg_gemm_pair_mse_loss: the scalar loss of lg_head_fwd_f32 ((sum(row_loss) * (1/n)) * 0.5, the value of lg_mse_finalize_f32,
 * bit for bit) rides as one spare workgroup of that three-product launch; if the bracket ends without one, it is finished by
 * a launch of its own at lg_gemm_pair_end.  row_loss and loss must stay valid until then. */
int lg_gemm_pair_mse_loss(const float* row_loss, int64_t rows, int64_t n, float* loss);
/* lg_gemm_pair_hold: the bracket stops collecting without launching what it has - products issued now run as if there were no
 * bracket (their results exist when the call returns, as always) - until lg_gemm_pair_resume makes it collect again.  The
 * caller vouches that nothing issued in between reads or writes what the held products write. */
int lg_gemm_pair_hold(void);
int lg_gemm_pair_resume(void);

/* Many weight-gradient products in ONE launch.  Between lg_gemm_group_begin and lg_gemm_group_end, lg_gemm_f32 /
 * lg_gemm_rowsum_f32 calls of the form dW (+ db) = g^T @ x (transA = 1, transB = 0, one matrix, at most 1024 output tiles of
 * 64 x 64) are prepared and QUEUED instead of launched (up to 14), and so are lg_layernorm_param_grads_f32 calls (up to 8) and
 * lg_scatter_add_rows_f32 calls of at most 4096 ids (up to 4; one more launch for these two kinds together);
 * anything else inside the bracket runs as usual.  The queue outlives the bracket: lg_gemm_group_flush launches it - ONE
 * kernel: the products, and behind them in the same grid the LayerNorm / scatter jobs (a launch of their own only when one of
 * them writes where a product writes: call order is kept then).  It is also launched when full, when a call writes where a queued one writes, and
 * before lg_sync, lg_memcpy_d2h, lg_graph_launch and the end of a capture.  Values are those of the immediate launches up to
 * rounding (a queued product always takes the 64 x 64 tile; launched at once it might split K differently); what changes is
 * WHEN they are computed: the caller must keep the queued calls' operands alive and unchanged and must not read
 * their outputs until the flush.  Made for the backward pass of a deep network: each Linear's weight gradient is a small
 * product with a long K (12 us alone, most of it launch, prologue and split-K hand-off on a handful of workgroups) that
 * nothing but the optimizer waits for; together they cost what the largest costs.  New design, no reference analog. */
int lg_gemm_group_begin(void);
/* out[c] (+)= sum over rows of in[r * ld + c]: the bias gradient of a Linear.  Inside a group bracket (one such job per
 * flush) it is queued and computed by extra workgroups of the group's launch - memory-bound work next to MFMA-bound work;
 * otherwise, or when the slot is taken, it is lg_reduce_acc at once.  Same caller obligations as for queued products. */
int lg_gemm_group_colsum_f32(const float* in, int64_t ld, int64_t rows, int64_t cols, float* out, int accumulate);
int lg_gemm_group_flush(void);
int lg_gemm_group_end(void);

/* ---- the skinny output layer and its loss (csrc/head.hip) ------------------------
 * An nn.Linear with at most 16 output features (a classifier head; reference nn.py:90-96) followed by
 * loss.mse (loss.py:4-12), forward and backward, in two launches.  `relu` != 0: `x` is the PRE-activation of
 * a relu whose output was never materialised (np.maximum(x, 0) is applied on the fly, cpu/ops.py:226).
 *   lg_head_fwd_f32   y = act(x) @ w^T + bias;  err = y + (-target);  row_loss[r] = sum_j err[r][j]^2
 *                     x: [rows, hidden] with row pitch ldx (hidden, ldx multiples of 4; x, w 16-byte aligned;
 *                     outs*hidden*4 <= 64 KiB), w: [outs, hidden] dense, bias: [outs] or NULL, target/y/err:
 *                     [rows, outs] dense, row_loss: [rows].
 *   lg_mse_finalize_f32   loss[0] = (sum_r row_loss[r] * (1/n)) * 0.5 with n = rows*outs (loss.py:9-10): one small
 *                     launch, needed only when the loss is read before lg_head_bwd_f32 has run (which finishes it
 *                     with one extra workgroup, in the same summation order - same bits either way).
 *   lg_head_bwd_f32   dx = g @ w  ([rows, hidden] dense, or NULL);  gpre = dx * (x >= 0)  (relu.backward's result,
 *                     cpu/ops.py:229; or NULL; needs relu != 0);  dw (+)= g^T @ act(x)  ([outs, hidden] dense, or
 *                     NULL);  db (+)= column sums of g  ([outs], or NULL)  - what dot.backward, transpose.backward
 *                     and the bias un-broadcast of func.py:50-56 compute for `act(x) @ w.T(1,0) + b`;
 *                     row_loss / loss: both NULL, or the row sums of lg_head_fwd_f32 and where to put the scalar.
 * They replace pyopencl launches of the reference's OpenCL backend: kernels.dot (opencl/ops.py:119-132),
 * kernels.atom (:285-288) and kernels.reduce (:344-368). */
int lg_head_fwd_f32(const float* x, int64_t ldx, int relu, const float* w, const float* bias, const float* target,
                    float* y, float* err, float* row_loss, int64_t rows, int64_t hidden, int64_t outs);
/* lg_head_fwd_f32 that also writes dx[rows, hidden] = err @ w and gpre[rows, hidden] = dx * (x >= 0) (relu != 0): what
 * lg_head_bwd_f32 writes for g = err, bit for bit - the gradients of the loss with respect to the layer's input and to the
 * pre-activation when backward() starts at this loss (its seed is 1: loss.py:12 hands `err` on as the output layer's gradient).
 * Computed while the row of x is in the cache and w in LDS; the caller uses them in the backward pass only if that is how the
 * pass goes and x, w, err are unchanged by then.  dx and gpre: both NULL (= lg_head_fwd_f32) or both given. */
int lg_head_fwd_grad_f32(const float* x, int64_t ldx, int relu, const float* w, const float* bias, const float* target,
                         float* y, float* err, float* row_loss, float* dx, float* gpre, int64_t rows, int64_t hidden, int64_t outs);
/* The hidden layer in front of such a head and the head itself: pre = x @ w1^T + b1 ([rows, hidden] dense; x: [rows, d_in] with row
 * pitch ldx, w1: [hidden, d_in] with row pitch ldw1 - nn.Linear's layout), then lg_head_fwd_grad_f32 on pre: two launches.
 * chain != 0: ONE launch when the product resolves to the 64x32 two-K-group tile (the MNIST MLP's 1024 x 512 x 784 does),
 * hidden <= 1024 and rows <= 4096 - the head's rows are computed by workgroups at the end of the product's grid, each waiting
 * for the tiles of its rows (written through, announced by a flag).  Same bits either way.  An experiment: measured SLOWER than
 * the two launches on MI355X (22.0 against 20.6 us, profiles/r4/chain_bench.txt) - the tape calls the two launches.
 * *launches (may be NULL) receives 1 or 2. */
int lg_gemm_bias_head_fwd_f32(const float* x, int64_t ldx, const float* w1, int64_t ldw1, const float* b1, float* pre,
                              int64_t rows, int64_t hidden, int64_t d_in, int relu,
                              const float* w2, const float* b2, const float* target, float* y, float* err, float* row_loss,
                              float* dx, float* gpre, int64_t outs, int chain, int* launches);
int lg_mse_finalize_f32(const float* row_loss, int64_t rows, int64_t n, float* loss);
int lg_head_bwd_f32(const float* x, int64_t ldx, int relu, const float* g, const float* w,
                    float* dx, float* gpre, float* dw, int dw_accumulate, float* db, int db_accumulate,
                    int64_t rows, int64_t hidden, int64_t outs, const float* row_loss, float* loss);

/* ---- row-wise fused ops for the tiny-BERT path -------
 * Dense fp32 [rows, cols] operands; one wavefront owns a row.
 * softmax over the last axis = the composite of autograd/ops.py:62-66; backward dx = y * (g - sum(g*y)).
 * layernorm = the composite of nn.py:109-124 for a 1-D normalised shape; saves xhat and rstd for the backward,
 * which returns dx only (dw = sum_rows(g * xhat), db = sum_rows(g) are lg_ew + lg_reduce calls). */
int lg_softmax_f32(const float* x, float* y, int64_t rows, int64_t cols);
int lg_softmax_bwd_f32(const float* y, const float* g, float* dx, int64_t rows, int64_t cols);
/* softmax(x * scale) and its backward (dx of the UNSCALED x) - attention's `(q @ k / sqrt(d)).softmax(-1)` (reference
 * examples/bert.py:81-86) without the separate scaling passes; x * scale is rounded to fp32 before anything else, and the
 * backward multiplies the finished fp32 gradient, so both give the bits of the two-kernel form. */
int lg_softmax_scaled_f32(const float* x, float* y, int64_t rows, int64_t cols, float scale);
int lg_softmax_scaled_bwd_f32(const float* y, const float* g, float* dx, int64_t rows, int64_t cols, float scale);
int lg_layernorm_f32(const float* x, const float* w, const float* b, float* y, float* xhat, float* rstd,
                     int64_t rows, int64_t cols, double eps);
int lg_layernorm_bwd_f32(const float* g, const float* w, const float* xhat, const float* rstd, float* dx,
                         int64_t rows, int64_t cols);
/* parameter gradients of the same LayerNorm from one launch: dw[c] (+)= sum_r g[r][c] * xhat[r][c], db[c] (+)= sum_r g[r][c]
 * (the tape's mul + two un-broadcasting column sums of func.py:50-56 + two `grad +=`) */
int lg_layernorm_param_grads_f32(const float* g, const float* xhat, float* dw, float* db, int64_t rows, int64_t cols,
                                 int dw_accumulate, int db_accumulate);
/* embedding lookup out[i, :] = table[ids[i], :] (ids int32 or int64, negative ids wrap like numpy) and its
 * gradient grad_table[ids[i], :] += grad_out[i, :] (float atomics: repeated ids ACCUMULATE; the reference's
 * numpy `grad[idx] = g`, cpu/ops.py:245, keeps only the last one, and its BERT example drops the gradient). */
int lg_gather_rows_f32(const float* table, const void* ids, int id_itemsize, float* out,
                       int64_t n_ids, int64_t row_len, int64_t table_rows);
/* out[i, :] = (t0[ids0[i % n0], :] + t1[ids1[i % n1], :]) + t2[ids2[i % n2], :] - three lookups and their sum in one pass
 * (BERT's word + position + token-type embeddings, examples/bert.py:36-40: three lookups and two kernels.atom adds).  n_k ids
 * for table k (n_k divides n_out: an id tensor broadcast over leading axes), rows_k rows in table k; ids all int32 or all
 * int64.  Sums in the order written, each rounded to fp32.  Out-of-range ids as in lg_gather_rows_f32. */
int lg_gather_sum3_rows_f32(const float* t0, const void* ids0, int64_t n0, int64_t rows0,
                            const float* t1, const void* ids1, int64_t n1, int64_t rows1,
                            const float* t2, const void* ids2, int64_t n2, int64_t rows2,
                            int id_itemsize, float* out, int64_t n_out, int64_t row_len);
int lg_scatter_add_rows_f32(const float* grad_out, const void* ids, int id_itemsize, float* grad_table,
                            int64_t n_ids, int64_t row_len, int64_t table_rows);
/* What the most recent call of the calling thread to lg_softmax_scaled_f32 / lg_softmax_scaled_bwd_f32 (and the unscaled forms,
 * which call them), lg_layernorm_f32, lg_layernorm_bwd_f32, lg_layernorm_param_grads_f32, lg_scatter_add_rows_f32 or
 * lg_gather_rows_f32 decided: host bookkeeping for tests, no device work.
 *   out = {kernel, a, b, queued}
 * kernel: 0 = softmax forward, 1 = softmax backward, 2 = LayerNorm forward, 3 = LayerNorm backward, 4 = LayerNorm parameter
 * gradients, 5 = scatter-add, 6 = gather, 7 / 8 = lg_dropout_layernorm_fwd_f32 / _bwd_f32 (a = mode), -1 = nothing launched or queued (an empty or refused call: the other fields are 0);
 * a: softmax forward - floats per lane held in registers (2, 8, 32; 0 = the loop that re-reads the row); parameter gradients -
 * the row splits, with b = the rows per split; scatter-add - 0 = queued, 1 = the chunked launch, 2 = the atomic kernel;
 * queued: 1 when the call only queued its work inside an open lg_gemm_group_begin bracket. */
int lg_rowwise_last_plan(int32_t out[4]);

/* loss.cross_entropy (loss.py:14-24) for dense fp32 logits [rows, cols] and integer labels [rows] (int16/32/64):
 *   nll[r] = -log(softmax(logits[r])[label[r]]);  dlogits[r][c] = (softmax(logits[r])[c] - [c == label[r]]) / rows
 * the loss is mean(nll) (lg_reduce + one scalar multiply), its gradient dlogits * upstream. */
int lg_cross_entropy_f32(const float* logits, const void* labels, int label_itemsize, float* dlogits, float* nll,
                         int64_t rows, int64_t cols);
/* The same plus the loss itself: mean[0] = (sum of nll) * (1 / rows), as `loss.cross_entropy` returns it (loss.py:21).  For
 * vocabulary-sized rows the mean is formed inside the row kernel (the workgroup that finishes last sums the row losses in a
 * fixed order); otherwise by the generic reduction + scaling behind it. */
int lg_cross_entropy_mean_f32(const float* logits, const void* labels, int label_itemsize, float* dlogits, float* nll,
                              float* mean, int64_t rows, int64_t cols);

/* The masked-LM form: rows whose label - as stored, before any negative-index wrap - equals ignore_index do not count.
 *   valid[r] = label[r] != ignore_index;  n = number of valid rows (written to n_valid[0], device memory, by a count launch in front)
 *   nll[r] = valid ? -log(softmax(logits[r])[label[r]]) : 0;   mean[0] = (sum of nll) * float(1.0 / double(n))
 *   dlogits[r][c] = valid ? (softmax(logits[r])[c] - [c == label[r]]) * float(1.0 / double(n)) : +0.0
 * An ignored row's logits are not read (they may hold NaN or infinities).  A valid label outside [-cols, cols) behaves as above
 * (NaN + LG_STATUS_BAD_INDEX).  n == 0: mean = NaN, dlogits all +0.0, no status flag.  The factor is formed on the device from
 * n_valid, so the call is legal under graph capture with labels that change between replays.  Launches: the count + what
 * lg_cross_entropy_mean_f32 takes for the shape (vocabulary-sized rows: 2 in all; otherwise count, rows, sum, scale).
 * Same argument checks as lg_cross_entropy_mean_f32; n_valid must not be NULL. */
int lg_cross_entropy_ignore_f32(const float* logits, const void* labels, int label_itemsize, float* dlogits, float* nll,
                                float* mean, int64_t* n_valid, int64_t rows, int64_t cols, int64_t ignore_index);

/* ---- dropout from a counter-based random stream (csrc/dropout.hip) -----------------------------------
 * The generator is Philox4x32-10 and its state - a 64-bit seed and the 64-bit number of dropout calls so far, `draws` - lives
 * in device memory owned by the library (allocated by lg_init: seed 0, draws 0).  For the call with draws == b, element i of
 * the dense tensor takes word i % 4 of
 *   philox4x32_10(counter = (lo32(i / 4), hi32(i / 4), lo32(b), hi32(b)), key = (lo32(seed), hi32(seed)))
 * and is KEPT iff that word >= T, T = min(floor(p * 2^32), 2^32 - 1):
 *   y[i] = kept ? x[i] * s : +0.0 (then + residual[i] when residual is not NULL, two roundings),  s = float(1.0 / (1.0 - p))
 *   dx[i] = kept ? g[i] * s : +0.0
 * No mask is stored: the forward kernel reads `draws` from the state, writes the value it read to base_out[0] and advances
 * `draws` by exactly one, whatever n is (n == 0 included); the backward kernel regenerates the mask from base[0] and the
 * state's seed (do not reseed between the two).  Because seed and draws are read from memory, a captured graph draws a fresh
 * mask on every replay and obeys an lg_rng_seed issued after the capture.  y may alias x, dx may alias g.
 * 0 <= p < 1; n >= 0; base_out / base are device pointers to one uint64. */
int lg_rng_seed(uint64_t seed);                          /* stream-ordered write of {seed, draws = 0}; refused while capturing */
int lg_rng_state(uint64_t* seed, uint64_t* draws);       /* synchronises the stream; refused while capturing */
int lg_dropout_fwd_f32(const float* x, const float* residual /* may be NULL */, float* y, int64_t n,
                       double p, uint64_t* base_out);
int lg_dropout_bwd_f32(const float* g, float* dx, int64_t n, double p, const uint64_t* base);

/* ---- BERT's token masking from the same stream (csrc/mlm.hip) ------------------------------------------
 * ONE call of the stream: `draws` advances by exactly one, whatever n is (n == 0 included: one workgroup is launched), and the
 * value read is written to base_out[0].  For the call with draws == b, element i (flat index) takes the WHOLE block
 *   w = philox4x32_10(counter = (lo32(i), hi32(i), lo32(b), hi32(b)), key = (lo32(seed), hi32(seed)))
 * and is SELECTED iff ids[i] is none of special_ids[0 .. n_special) and w[0] < T(p) (T as above):
 *   not selected:  masked[i] = ids[i], labels[i] = ignore_index
 *   selected:      labels[i] = ids[i];  masked[i] = mask_token_id                       if w[1] < 3435973836  (floor(0.8 * 2^32))
 *                                                   (uint64(w[2]) * vocab_size) >> 32   else if w[1] < 3865470566  (floor(0.9 * 2^32))
 *                                                   ids[i]                              otherwise
 * ids / masked / labels: dense int32 (itemsize 4) or int64 (8) device arrays of n elements, no two the same; special_ids is
 * HOST memory, read during the call (at most 8, passed to the kernel by value).  Seed and draws are read by the kernel: a
 * captured graph masks a fresh batch on every replay.  0 <= p < 1; 0 <= n <= 2^32; 1 <= vocab_size <= 2^31; mask_token_id and
 * ignore_index must fit the ids' type. */
int lg_mlm_mask(const void* ids, int itemsize, void* masked, void* labels, int64_t n, double p, int64_t mask_token_id,
                int64_t vocab_size, const int64_t* special_ids, int n_special, int64_t ignore_index, uint64_t* base_out);

/* ---- sampled decoding from the same stream (csrc/sample.hip) --------------------------------------------
 * One token per row of fp32 logits [rows, cols] (row r at logits + r * row_pitch, the vocabulary contiguous) with temperature,
 * top-k and top-p, in ONE launch.  ONE call of the stream: `draws` advances by exactly one, whatever the shape (rows == 0
 * included: one workgroup is launched), and the value read is written to base_out[0].  For the call with draws == b, row r takes
 * word 0 of philox4x32_10(counter = (lo32(r), hi32(r), lo32(b), hi32(b)), key = (lo32(seed), hi32(seed))) and
 * u = ((word >> 8) + 0.5) * 2^-24, strictly inside (0, 1).  For a row x of V = cols logits:
 *   1. m = max(x).  A DEGENERATE row - one that holds a NaN, or has m == +inf or m == -inf - answers its argmax under the rules
 *      of lg_argreduce_f32 (the first NaN, the lowest index).  No status flag is raised; the output is always a valid index.
 *   2. top-k, when 1 <= top_k < V (0 and >= V: off): v_k = the k-th largest value counted with multiplicity,
 *      K = {j : x_j >= v_k} - ties at the boundary are all kept; comparisons on x only, -0.0 == +0.0.  Off: K is everything.
 *   3. w_j = exp((x_j - m) * inv_T) for j in K, else 0;  inv_T = float(1.0 / temperature);  W = sum of w.
 *   4. top-p, when 0 < top_p < 1 (1.0: off, tested explicitly): t = the largest value v occurring in K with
 *      sum{w_j : x_j >= v} >= top_p * W;  N = {j in K : x_j >= t}.  Off: N = K.
 *   5. the token is the lowest i in N with sum{w_j : j in N, j <= i} >= u * W', W' = the sum over N.  A -inf logit has weight 0
 *      and is never returned.
 * lightgrad_amd/random.py `sample_tokens` evaluates this in float64 and is the numpy backend.  The kernel holds every weight as
 * the integer floor(2^40 * w_j) (2^(62 - bits(cols)) for rows of 2^22 elements and more): all its sums are exact and
 * order-free, so the same logits, seed and call number give the same token on every run, and its token agrees with the
 * float64 definition wherever u is further than the weights' rounding (about 1e-6 of cumulative probability) from a boundary.
 * out: rows tokens of out_itemsize 4 (int32) or 8 (int64).  Seed and draws are read by the kernel and no host scalar depends on
 * the data: the launch is legal under capture and draws fresh numbers on every replay.
 * temperature > 0, finite, 1 / temperature finite in float; top_k >= 0; 0 < top_p <= 1; 0 <= rows <= 2^24; 1 <= cols < 2^31;
 * row_pitch >= cols. */
int lg_sample_f32(const float* logits, int64_t rows, int64_t cols, int64_t row_pitch, double temperature, int64_t top_k,
                  double top_p, void* out, int out_itemsize, uint64_t* base_out);
/* What the most recent lg_sample_f32 or lg_sample_rows_f32 call of the calling thread launched: host bookkeeping for tests, no
 * device work.
 *   out[0] kernel: 0 = the row is held in LDS, 1 = the row is re-read from memory, -1 = nothing (a refused call, or no rows)
 *   out[1] threads per workgroup   out[2] passes over the row   out[3] 1 when the row is staged with 16-byte loads
 * lg_sample_rows_f32 reports the passes of a sampled row with every filter on (10): its table may turn them on per row. */
int lg_sample_last_plan(int32_t out[4]);

/* ---- per-request sampling: parameters, seed and counter per row (csrc/sample_rows.hip) --------------------
 * One token per row of fp32 logits [rows, cols] (row r at logits + r * row_pitch) in ONE launch, every row under the parameters
 * and the random stream of a table row of its own.  table: n rows of 8 int32 words (16-byte aligned) -
 *   word 0     the bits of inv_T = float(1.0 / temperature); +0.0 means GREEDY
 *   word 1     top_k             words 2, 3   the low and high half of the bits of top_p (a double)
 *   words 4, 5 the low and high half of a 64-bit seed          words 6, 7   0
 * index: rows int32 words, row r uses table row i = index[r]; counter: n int32 words, g = counter[i].  Per row, in this order:
 *   1. i < 0: the token is 0; the row's logits are not read.
 *   2. the row is BAD when i >= n, g < 0, top_k < 0, top_p is outside (0, 1], or inv_T has its sign set, is NaN or infinite: the
 *      token is 0 and LG_STATUS_BAD_INDEX is raised (LG_EINDEX at the next synchronisation); the other rows are computed.
 *   3. inv_T == +0.0: the row's argmax under the rules of lg_argreduce_f32, degenerate rows included.
 *   4. otherwise steps 1 to 5 of lg_sample_f32 with u = ((word >> 8) + 0.5) * 2^-24, word = word 0 of
 *      philox4x32_10(counter = (lo32(g), hi32(g), 0, 0), key = (lo32(seed), hi32(seed))): the number that call 0 of a stream seeded
 *      `seed` gives its row g.
 * The row body is lg_sample_f32's own: for equal (inv_T, top_k, top_p, u) the token is that launch's bit for bit.  The
 * generator's (seed, draws) state is neither read nor advanced.  lightgrad_amd/random.py `sample_tokens_rows` is the definition
 * in float64.  rows == 0 launches nothing.  0 <= rows <= 2^24; 1 <= cols < 2^31; row_pitch >= cols; n >= 1; out_itemsize 4 or
 * 8; no NULL or misaligned operand; `out` overlaps none of the others. */
int lg_sample_rows_f32(const float* logits, int64_t rows, int64_t cols, int64_t row_pitch, const int32_t* table, int64_t n,
                       const int32_t* index, const int32_t* counter, void* out, int out_itemsize);

/* ---- per-request penalties on the logits, in place (csrc/penalize.hip) -------------------------------------
 * Repetition, presence and frequency penalties and a minimum of new tokens, per row of fp32 logits [rows, cols] (row r at
 * logits + r * row_pitch), IN PLACE and in ONE launch, every row under the parameters and the history of a request of its own.
 * table: n rows of 4 int32 words (16-byte aligned) - the bits of rho (repetition), alpha (presence), beta (frequency) as floats,
 * and min_new.  index: rows int32 words, row r uses request i = index[r].  prompts [n, P] (row pitch prompt_pitch), prompt_len
 * [n], out [n, G] (row pitch out_pitch), out_len [n]: int32, the history of request i is prompts[i, :len] and out[i, :g] with
 * len = prompt_len[i], g = out_len[i]; words behind len and g are never read.  eos: -1 (none) or an id below cols.  Per row:
 *   1. i < 0: nothing of the row is read or written.
 *   2. the row is BAD when i >= n, len is outside [0, P], g is outside [0, G], rho is not finite, <= 0 or has its sign set, alpha
 *      or beta is not finite, min_new < 0, or an id of the history lies outside [0, cols): NOTHING of the row is written and
 *      LG_STATUS_BAD_INDEX is raised (LG_EINDEX at the next synchronisation); the other rows are computed.
 *   3. every id v of the history, once however often it occurs: x = x < 0 ? x * rho : x / rho (correctly rounded).
 *   4. every v with c > 0 occurrences in out[i, :g]: x = (x - beta * float(c)) - alpha, three roundings, nothing fused.
 *   5. eos >= 0 and g < min_new: logits[r, eos] = -inf, whatever 3 and 4 left there.
 * Only the logits at ids of the history (and eos) are touched: the cost does not grow with cols.  lightgrad_amd/random.py
 * `penalize_logits` is the definition; the results are its float32 results bit for bit.  rows == 0 returns LG_OK at once.
 * 1 <= rows <= 65535; 1 <= cols < 2^31; row_pitch >= cols; n >= 1; P, G >= 1 and P + G <= 4096 (the history is kept in LDS);
 * no NULL or misaligned operand; the logits share no byte with any other operand. */
int lg_penalize_rows_f32(float* logits, int64_t rows, int64_t cols, int64_t row_pitch, const int32_t* table, int64_t n,
                         const int32_t* index, const int32_t* prompts, int64_t prompt_pitch, int64_t P, const int32_t* prompt_len,
                         const int32_t* out, int64_t out_pitch, int64_t G, const int32_t* out_len, int32_t eos);

/* ---- per-token log-probabilities and top-n alternatives (csrc/logprob.hip) ------------------------------------
 * The log-probability of the token just drawn, and the n most likely ids with theirs, per row of fp32 logits [rows, cols] (row r
 * at logits + r * row_pitch) in ONE launch, every row into the cell of a request of its own.  token: rows int32, the id drawn
 * from row r.  want [n] int32 per request: -1 nothing, 0 the token's only, k in 1 .. n_max also the k most likely ids.  index:
 * rows int32, row r belongs to request i = index[r].  counter [n] int32: the column g = counter[i].  logprob fp32 [n, G], top_ids
 * int32 and top_logprob fp32 [n, G, n_max], dense.  Per row:
 *   1. i < 0, or i < n and want[i] == -1: nothing of the row is read, nothing is written.
 *   2. the row is BAD when i >= n, g is outside [0, G), want[i] is outside [-1, n_max] or the token is outside [0, cols): NOTHING
 *      is written and LG_STATUS_BAD_INDEX is raised (LG_EINDEX at the next synchronisation); the other rows are computed.
 *   3. with m = max x and S = sum_j exp(x_j - m): logprob[i, g] = (x_token - m) - log S; top_ids[i, g, :k'] the k' = min(want[i],
 *      cols) largest values' ids, descending, equal values (-0.0 == +0.0) to the lower index; top_logprob[i, g, :k'] their
 *      (x_j - m) - log S.  The entries behind k' keep their bytes.  A -inf logit has -inf.
 *   4. a row with a NaN, with +inf, or of nothing but -inf: NaN to logprob[i, g] and top_logprob[i, g, :want[i]], -1 to
 *      top_ids[i, g, :want[i]].
 * S is a sum of 64-bit integers floor(2^40 * __expf(x_j - m)): the same bits from run to run; the differences and log S are fp32.
 * lightgrad_amd/random.py `token_logprobs_rows` is the definition, in float64.  Two rows of one request write one cell: the
 * caller's rows name distinct requests.  rows == 0 returns LG_OK at once.  1 <= rows <= 65535; 1 <= cols < 2^31; row_pitch >=
 * cols; n, G >= 1; 1 <= n_max <= 8; no NULL operand, every operand 4-byte aligned; an output shares no byte with any other
 * operand.  A row of at most lg_logprob_lds_cols() floats is staged in LDS, a wider one is read again from memory. */
int lg_logprob_rows_f32(const float* logits, int64_t rows, int64_t cols, int64_t row_pitch, const int32_t* token, const int32_t* want,
                        int64_t n, const int32_t* index, const int32_t* counter, float* logprob, int64_t G, int32_t* top_ids,
                        float* top_logprob, int64_t n_max);
int lg_logprob_lds_cols(void);

/* ---- guided decoding: per-request token automata on the logits, in place (csrc/guide.hip) ------------------
 * Per row of fp32 logits [rows, cols] (row r at logits + r * row_pitch), IN PLACE and in ONE launch: the ids that the state of the
 * row's request does not allow go to -inf.  allow: S rows of W = ceil(cols / 32) int32 words, bit v % 32 of word v / 32 says id v
 * is allowed in the state (the bits at and behind cols are 0).  states: S rows of 4 int32 words (16-byte aligned): the default next
 * state or -1, the offset of the state's first exception in `edges`, the number of its exceptions, the forced id or -1.  edges: E
 * rows of (id, next state), sorted by id within a state.  index: rows int32 words, row r names request i = index[r].  out [N, G]
 * (row pitch out_pitch) and out_len [N]: the tokens request i has stored are out[i, :out_len[i]].  state [N, 2] (8-byte aligned):
 * (q, k), the state of request i's automaton behind its first k stored tokens; q == -1: the request is unguided.  Per row:
 *   1. i < 0, or q == -1: nothing of the row is read or written.
 *   2. the row is BAD when i >= N, g = out_len[i] is outside [0, G], q is outside [0, S), k is outside [0, g]; when a token
 *      out[i, j], j = k .. g - 1, lies outside [0, cols) or has its bit clear in the state that absorbs it; when a state's run of
 *      exceptions leaves [0, E] or the next state - the exception's target, found by binary search, else the default - lies outside
 *      [0, S); when the final state's forced id f is outside [-1, cols) or has its bit clear.  NOTHING of a bad row is written,
 *      neither logits nor state, and LG_STATUS_BAD_INDEX is raised (LG_EINDEX at the next synchronisation); the others are computed.
 *   3. state[i] = (q', g) as one 8-byte word; logits[r, v] = -inf wherever the bit of v is clear in q'; +0.0 at f if f >= 0.  No
 *      logit is read: every allowed value keeps its bytes.
 * lightgrad_amd/guide.py `guide_logits` is the definition; the results are its results bit for bit, whatever the grid.  The grid
 * is (slices, rows) workgroups; lg_guide_rows_slices(s) sets the slices of a row for the calls that follow (0: chosen from cols,
 * the default; at most 64) and returns the previous setting - the result does not depend on it.  rows == 0 returns LG_OK at once.
 * 1 <= rows <= 65535; 1 <= cols < 2^31; row_pitch >= cols; S, E, N, G >= 1; out_pitch >= G; no NULL or misaligned operand; the
 * logits share no byte with any other operand, and neither does `state`. */
int lg_guide_rows_f32(float* logits, int64_t rows, int64_t cols, int64_t row_pitch, const int32_t* allow, const int32_t* states, int64_t S,
                      const int32_t* edges, int64_t E, const int32_t* index, const int32_t* out, int64_t out_pitch, int64_t G,
                      const int32_t* out_len, int32_t* state, int64_t N);
int lg_guide_rows_slices(int slices);

/* ---- hidden dropout inside the LayerNorm launches (csrc/rowwise.hip) ----------------------------------
 * A dropout that sits directly in front of or behind a LayerNorm over dense fp32 [rows, cols], drawn where the LayerNorm
 * kernel loads or stores its row.  ONE call of the stream above per forward; element i = row * cols + col of the dense operand
 * takes the word lg_dropout_fwd_f32 would give element i, so the results are the bits of the two-launch forms:
 *   mode 0  y = layernorm(dropout(x, p) + residual)   = lg_dropout_fwd_f32(x, residual, t) then lg_layernorm_f32(t, ...)
 *           (residual may be NULL: no addition); t is never written to memory.  Backward, with d = lg_layernorm_bwd_f32's dx:
 *           dres[i] = d[i] (dres may be NULL), dx[i] = kept ? d[i] * s : +0.0
 *   mode 1  y = dropout(layernorm(x), p)               = lg_layernorm_f32 then lg_dropout_fwd_f32 (the embedding site; residual
 *           must be NULL).  Backward: gdrop[i] = kept ? g[i] * s : +0.0, dx = lg_layernorm_bwd_f32 of gdrop; gdrop is written
 *           to memory because the LayerNorm's parameter gradients are lg_layernorm_param_grads_f32(gdrop, xhat, ...).
 * xhat and rstd are those of the LayerNorm in both modes.  The forward reads `draws`, writes it to base_out[0] and advances it
 * by one, whatever the shape (rows == 0 included), like lg_dropout_fwd_f32, and a captured graph draws a fresh mask per replay;
 * the backward draws nothing (rows == 0: no launch).  No output may alias an input or another output.
 * 0 <= p < 1; rows >= 0 (at most 2^26), cols >= 1, rows * cols <= 2^34; lg_rowwise_last_plan: kernel 7 (forward) / 8
 * (backward), a = mode. */
int lg_dropout_layernorm_fwd_f32(const float* x, const float* residual /* NULL unless mode 0 */, const float* w, const float* b,
                                 float* y, float* xhat, float* rstd, int64_t rows, int64_t cols, float eps, double p, int mode,
                                 uint64_t* base_out);
int lg_dropout_layernorm_bwd_f32(const float* g, const float* w, const float* xhat, const float* rstd, float* dx,
                                 float* dres /* mode 0, may be NULL */, float* gdrop /* mode 1 */, int64_t rows, int64_t cols,
                                 double p, int mode, const uint64_t* base);

/* ---- 2-D convolution and pooling (csrc/conv.hip) -------------------------------------------------------
 * Dense fp32 tensors: x [N, C, H, W], w [O, C, KH, KW], y and g [N, O, OH, OW] with OH = (H + 2 pad - KH) / sh + 1 and
 * OW = (W + 2 pad - KW) / sw + 1: the cross-correlation of the reference's `conv` (cpu/ops.py:298-356) over an input that is
 * zero-padded by `pad` on both sides of both spatial axes.  Each entry point is ONE launch of an implicit GEMM on fp32 MFMA: the
 * window matrix is gathered while tiles are staged and never exists in memory; nothing outside a tensor is read.
 *   fwd  y[n,o,oh,ow] = fl(sum over (c, kh, kw) ascending of x[n,c,oh*sh+kh-pad,ow*sw+kw-pad] * w[o,c,kh,kw]), then + bias[o]
 *        as a second rounding when bias (O floats) is not NULL.
 *   dx   dx[n,c,h,w] = sum over (o, kh, kw) of g[n,o,(h+pad-kh)/sh,(w+pad-kw)/sw] * w[o,c,kh,kw] over the taps whose divisions
 *        are exact and in range.  Every element of dx is written exactly once.
 *   dw   dw[o,c,kh,kw] = sum over (n, oh, ow) of g[n,o,oh,ow] * x[n,c,oh*sh+kh-pad,ow*sw+kw-pad] and, when db is not NULL,
 *        db[o] = sum g[n,o,:,:] from the same launch.  The positions are split over workgroups whose partial tiles the last
 *        arriver folds in slice order: the slice count depends on the shape only, so the result is the same bits on every run.
 *        Both are OVERWRITTEN.
 * relu_x != 0: x is a pre-activation and max(x, 0) (NaN kept) is applied while it is staged (fwd, dw).
 * Refused with LG_EINVAL: an extent below 1, a stride below 1, a negative pad, a window larger than the padded input; H, W, pad
 * or a stride above 16384; C*KH*KW or O*KH*KW above 2048 (the offset table in LDS); N*OH*OW, N*H*W, C*H*W or O*OH*OW of 2^31 or
 * more.  The three entry points refuse the same shapes.  No output may alias an input. */
int lg_conv2d_fwd_f32(const float* x, const float* w, const float* bias /* may be NULL */, float* y, int64_t N, int64_t C, int64_t H,
                      int64_t W, int64_t O, int64_t KH, int64_t KW, int64_t sh, int64_t sw, int64_t pad, int relu_x);
int lg_conv2d_dx_f32(const float* g, const float* w, float* dx, int64_t N, int64_t C, int64_t H, int64_t W, int64_t O,
                     int64_t KH, int64_t KW, int64_t sh, int64_t sw, int64_t pad);
int lg_conv2d_dw_f32(const float* g, const float* x, float* dw, float* db /* may be NULL */, int64_t N, int64_t C, int64_t H, int64_t W,
                     int64_t O, int64_t KH, int64_t KW, int64_t sh, int64_t sw, int64_t pad, int relu_x);
/* What the most recent lg_conv2d_* call of the calling thread launched: host bookkeeping for tests, no device work.
 *   out = {kernel, tile_rows, tile_cols, k_chunk, dw_slices, relu_x}
 * kernel: 0 fwd, 1 dx, 2 dw, -1 nothing yet; the tile is that of a workgroup; dw_slices is the number of position slices of the
 * most recent dw call (1 = one workgroup per output tile, no fold; at most 256) and is left alone by fwd and dx. */
int lg_conv2d_last_plan(int32_t out[6]);

/* Max (op 0) / min (op 1) pooling over non-overlapping kh x kw windows of the last two axes of a dense fp32 [L, H, W] (all
 * leading axes flattened into L); the input is cropped to a multiple of the window: y is [L, H / kh, W / kw].  NaN as in np.max /
 * np.min: a window with a NaN gives NaN.
 *   bwd  dx[l,h,w] = g[l,h/kh,w/kw] * (x[l,h,w] == y[l,h/kh,w/kw] ? 1 : 0): every tied extremum receives the gradient (LG_EW_MAX_BWD),
 *        a window whose result is NaN none; the cropped margin gets +0.0.  Every element of dx is written once; y is fwd's output.
 * Refused with LG_EINVAL: an extent below 1, a window larger than the input, L*H*W of 2^31 or more. */
int lg_pool2d_fwd_f32(int op, const float* x, float* y, int64_t L, int64_t H, int64_t W, int64_t kh, int64_t kw);
int lg_pool2d_bwd_f32(const float* x, const float* y, const float* g, float* dx, int64_t L, int64_t H, int64_t W, int64_t kh,
                      int64_t kw);

/* ---- batch normalisation (csrc/batchnorm.hip) ------------------------------------------------------------
 * Dense fp32 x, y, g, dx of geometry (N, C, L): element (n, c, l) at (n*C + c)*L + l - (N, C, H, W) with L = H*W, (N, C) with
 * L = 1.  Per channel c over the count = N*L elements with that c: mean_c, the biased variance var_c = mean((x - mean_c)^2) and
 * rstd_c = 1 / sqrt(var_c + eps).  w, b, running_*, save_*, dw and db hold C floats.
 *   fwd    y = (x - mean_c) * (rstd_c * w_c) + b_c (w NULL: 1, b NULL: 0); save_mean = mean, save_rstd = rstd; when the running
 *          pointers are not NULL, on the device and in the same launch as the statistics:
 *            running_mean = (1 - momentum) * running_mean + momentum * mean
 *            running_var  = (1 - momentum) * running_var  + momentum * var * count / (count - 1)
 *          Two launches: statistics, then apply.  A workgroup reduces a slice of a channel to (count, mean, M2) around a shift
 *          (never E[x^2] - E[x]^2); the slices of a channel are merged with Chan's formula in slice order by the workgroup that
 *          arrives last at the channel's ticket.  The slice count depends on the shape and on 16-byte alignment only: the same
 *          bits on every run.
 *   bwd    db_c = sum g, dw_c = sum g * xhat with xhat = (x - save_mean_c) * save_rstd_c recomputed from x (folded the same
 *          way, OVERWRITTEN), then dx = w_c * rstd_c * (g - db_c / count - xhat * dw_c / count).  dx, dw and db may each be
 *          NULL; without dx the second launch is skipped.
 *   infer  y = (x - running_mean_c) * (w_c / sqrt(running_var_c + eps)) + b_c: one elementwise launch.
 * relu_x != 0: x is a pre-activation and max(x, 0) (NaN kept) is applied as it is loaded (all three).
 * Refused with LG_EINVAL: an extent below 1; N*L below 2 (fwd); N*C*L of 2^31 or more; more channels (L > 1) or blocks of 64
 * channels (L == 1) than the ticket pool holds (65536); a negative eps; a momentum outside (0, 1].  No output may alias an input. */
int lg_batchnorm_fwd_f32(const float* x, const float* w /* may be NULL */, const float* b /* may be NULL */, float* y, float* save_mean,
                         float* save_rstd, float* running_mean /* may be NULL */, float* running_var /* may be NULL */, int64_t N,
                         int64_t C, int64_t L, float eps, float momentum, int relu_x);
int lg_batchnorm_bwd_f32(const float* g, const float* x, const float* w /* may be NULL */, const float* save_mean, const float* save_rstd,
                         float* dx /* may be NULL */, float* dw /* may be NULL */, float* db /* may be NULL */, int64_t N, int64_t C,
                         int64_t L, int relu_x);
int lg_batchnorm_infer_f32(const float* x, const float* w /* may be NULL */, const float* b /* may be NULL */, const float* running_mean,
                           const float* running_var, float* y, int64_t N, int64_t C, int64_t L, float eps, int relu_x);
/* What the most recent lg_batchnorm_* call of the calling thread launched: host bookkeeping for tests, no device work.
 *   out = {kernel, form, slices, relu_x}
 * kernel: 0 fwd, 1 bwd, 2 infer, -1 nothing yet; form: 0 lanes along L, 1 lanes across channels (L == 1); slices: workgroups per
 * channel (form 0) or per block of 64 channels (form 1) of the statistics / sums launch, 1 for infer. */
int lg_batchnorm_last_plan(int32_t out[4]);

/* library build info: "liblghip <version> gfx950 <build date>" */
const char* lg_version(void);

#ifdef __cplusplus
}
#endif
#endif /* LGHIP_H */
