"""The case table of the elementwise dispatch sweep (tests/test_hip_elementwise.py) and its references.  No GPU code here:
tests/test_elementwise_cases_cpu.py checks on the host what the GPU test relies on.

csrc/elementwise.hip carries 31 ops over five kernel families chosen on the host from the collapsed strides: flat (float4 body
and scalar tail), rows (float4 along the inner dimension), the LDS-transposing tile (scalar, float4 with one or two staged inputs,
128 x 128), flat-2D (dense 2-D outputs, any 2-D inputs) and gather.  Every case names the plan it is MEANT to reach -
`lg_ew_last_plan`'s {path, form, collapsed ndim, mask} - and the GPU test asserts it, so a retuned condition that moves a case to
another kernel fails the test instead of silently emptying it.  The conditions themselves are not restated: the plans are literals.

A case is written in numpy's own view language: every operand is a view (slices, transposes, broadcasts) of a flat base array,
and its element offset and strides are read off numpy.  The base array is the operand's payload; on the device it lies between
GUARD elements on either side (`padded`).  Inputs: NaN in the guards and in every payload element the view does not hold (a
kernel that reads outside spoils its result).  Outputs: SENTINEL in the guards and in every payload element the view does not hold
(the gaps of a pitched view), NaN where the view will be written - or the input's values for an in-place case, whose output IS
one of its inputs.  The expected buffer is that prefill with the reference written through the same offsets, and the WHOLE buffer
is compared.

(a) the path sweep: neg (1 input, 1 output), sub / div (2, 1), fma / max_bwd (3, 1), mul_bwd / div_bwd (3, 2), pow_bwd (4, 2).  All
    but pow_bwd are compositions of correctly rounded operations and must equal numpy float32 bit for bit; pow_bwd is judged by
    the rule of (b).  Every family holds every arity class, the scalar operand (NULL) in every slot, and an in-place case.
(b) the value sweep: one flat case of 4096 elements per op id - special values first, seeded random values behind.  `exact` ops
    must equal numpy float32 (assert_array_equal, denormals included); `close` ops are judged per element against the same
    expression in float64 on the float32 inputs: non-finite references matched exactly, finite ones within
    max(FLOOR * |ref|, 2 * |np32 - ref|); an element leaves the comparison when its float64 reference is non-zero below 2**-126 or
    above float32's range, at most 2 % per output.

Not reached by any case, and no case is contorted to reach them: the uint64_t index instantiations and the second trip of the
grid-stride loops (2**31 elements and more), and the 128 x 128 tile, which starts at 2**25 elements and stays with
test_hip_ops.py::test_transposed_operand_large_tiles.
"""
from collections import namedtuple
from functools import lru_cache
import numpy as np
from lightgrad_amd.autograd.hip import lib as hiplib
from rowwise_cases import GUARD, SENTINEL, FLOOR, padded, guards_of, rng_for          # noqa: F401  (re-exported to the tests)

# lg_ew_last_plan: {path, form, ndim, mask}
NONE, FLAT, ROWS, TILE, FLAT2D, GATHER = -1, 0, 1, 2, 3, 4
FAMILIES = {FLAT: "flat", ROWS: "rows", TILE: "tile", FLAT2D: "flat2d", GATHER: "gather"}
VEC, TAIL = 1, 2                                  # flat: bits of `form`
TILE_SCALAR, TILE_V4_ONE, TILE_V4_TWO, TILE_BIG = 0, 1, 2, 3

MAX_ELEMENTS = 1 << 20           # no buffer holds more
MAX_CASES = 400
SCALAR = 2.0                     # the value of the NULL operand of the sweep (max_bwd: a value its integer operands take)
VALUE_N = 4096                   # elements of a value-sweep case
LEAVE_CAP = 0.02                 # of any output's elements may leave the comparison
TINY = float(np.finfo(np.float32).tiny)           # 2**-126
HUGE = float(np.finfo(np.float32).max)

# name -> (op id, inputs, outputs, class)
OPS = {
    "copy": (hiplib.EW_COPY, 1, 1, "exact"), "neg": (hiplib.EW_NEG, 1, 1, "exact"), "exp": (hiplib.EW_EXP, 1, 1, "close"),
    "log": (hiplib.EW_LOG, 1, 1, "close"), "relu": (hiplib.EW_RELU, 1, 1, "exact"), "sigmoid": (hiplib.EW_SIGMOID, 1, 1, "close"),
    "tanh": (hiplib.EW_TANH, 1, 1, "close"), "sin": (hiplib.EW_SIN, 1, 1, "close"), "cos": (hiplib.EW_COS, 1, 1, "close"),
    "sqrt": (hiplib.EW_SQRT, 1, 1, "exact"), "gelu": (hiplib.EW_GELU, 1, 1, "close"),
    "add": (hiplib.EW_ADD, 2, 1, "exact"), "sub": (hiplib.EW_SUB, 2, 1, "exact"), "mul": (hiplib.EW_MUL, 2, 1, "exact"),
    "div": (hiplib.EW_DIV, 2, 1, "exact"), "pow": (hiplib.EW_POW, 2, 1, "close"), "relu_bwd": (hiplib.EW_RELU_BWD, 2, 1, "exact"),
    "sigmoid_bwd": (hiplib.EW_SIGMOID_BWD, 2, 1, "close"), "tanh_bwd": (hiplib.EW_TANH_BWD, 2, 1, "close"),
    "log_bwd": (hiplib.EW_LOG_BWD, 2, 1, "close"), "sin_bwd": (hiplib.EW_SIN_BWD, 2, 1, "close"),
    "cos_bwd": (hiplib.EW_COS_BWD, 2, 1, "close"), "eq": (hiplib.EW_EQ, 2, 1, "exact"), "ge": (hiplib.EW_GE, 2, 1, "exact"),
    "bias_relu": (hiplib.EW_BIAS_RELU, 2, 1, "exact"), "gelu_bwd": (hiplib.EW_GELU_BWD, 2, 1, "close"),
    "max_bwd": (hiplib.EW_MAX_BWD, 3, 1, "exact"), "fma": (hiplib.EW_FMA, 3, 1, "exact"),
    "mul_bwd": (hiplib.EW_MUL_BWD, 3, 2, "exact"), "div_bwd": (hiplib.EW_DIV_BWD, 3, 2, "close"),
    "pow_bwd": (hiplib.EW_POW_BWD, 4, 2, "close"),
}
SWEEP_OPS = ("neg", "sub", "div", "fma", "max_bwd", "mul_bwd", "div_bwd", "pow_bwd")
ARITY_CLASSES = {(1, 1), (2, 1), (3, 1), (3, 2), (4, 2)}


# ---- the expressions: cpu/ops.py's (gelu_common.h's for gelu), in the type of their inputs ---------------------------------------

def _gelu_inner(T, x):
    return (x * T(np.float32(0.7978845608))) * (T(1) + (T(np.float32(0.044715)) * x) * x)


def _gelu(T, x):
    return ((T(0.5) * x) * (T(1) + np.tanh(_gelu_inner(T, x))),)


def _gelu_bwd(T, x, g):
    th = np.tanh(_gelu_inner(T, x))
    du = T(np.float32(0.7978845608)) * (T(1) + T(np.float32(0.134145)) * x * x)
    return (g * (T(0.5) * (T(1) + th) + (T(0.5) * x) * (T(1) - th * th) * du),)


EXPR = {
    "copy": lambda T, a: (a.copy(),),
    "neg": lambda T, a: (-a,),
    "exp": lambda T, a: (np.exp(a),),
    "log": lambda T, a: (np.log(a),),
    "relu": lambda T, a: (np.maximum(a, T(0)),),
    "sigmoid": lambda T, a: (T(1) / (T(1) + np.exp(-a)),),
    "tanh": lambda T, a: (np.tanh(a),),
    "sin": lambda T, a: (np.sin(a),),
    "cos": lambda T, a: (np.cos(a),),
    "sqrt": lambda T, a: (np.sqrt(a),),
    "gelu": _gelu,
    "add": lambda T, a, b: (a + b,),
    "sub": lambda T, a, b: (a - b,),
    "mul": lambda T, a, b: (a * b,),
    "div": lambda T, a, b: (a / b,),
    "pow": lambda T, a, b: (np.power(a, b),),
    "relu_bwd": lambda T, t, g: (g * (t >= 0).astype(T),),
    "sigmoid_bwd": lambda T, y, g: (y * (T(1) - y) * g,),
    "tanh_bwd": lambda T, y, g: ((T(1) - y * y) * g,),
    "log_bwd": lambda T, x, g: ((T(1) / x) * g,),
    "sin_bwd": lambda T, t, g: (np.cos(t) * g,),
    "cos_bwd": lambda T, t, g: (-np.sin(t) * g,),
    "eq": lambda T, a, b: ((a == b).astype(T),),
    "ge": lambda T, a, b: ((a >= b).astype(T),),
    "bias_relu": lambda T, x, b: (np.maximum(x + b, T(0)),),
    "gelu_bwd": _gelu_bwd,
    "max_bwd": lambda T, x, m, g: (g * (x == m).astype(T),),
    "fma": lambda T, a, b, c: (a * b + c,),
    "mul_bwd": lambda T, a, b, g: (g * b, a * g),
    "div_bwd": lambda T, a, b, g: (g / b, -a / (b * b) * g),
    "pow_bwd": lambda T, a, b, g, y: (b * np.power(a, b - T(1)) * g, g * y * np.log(a)),
}


def evaluate(op, inputs, dtype):
    """the outputs of `op` on the float32 `inputs`, computed in `dtype` (float32: numpy's own bits; float64: the yardstick)"""
    T = np.dtype(dtype).type
    with np.errstate(all="ignore"):
        outs = EXPR[op](T, *[np.asarray(a, np.float32).astype(dtype) for a in inputs])
    assert len(outs) == OPS[op][2] and all(o.dtype == dtype for o in outs), op
    return outs


def close_violations(got, ref, np32):
    """the rule of the `close` class: (violations, kept, distance, bound), boolean / float64 arrays of the shape of `got`"""
    got, ref, np32 = (np.asarray(a, np.float64) for a in (got, ref, np32))
    with np.errstate(all="ignore"):
        finite = np.isfinite(ref)
        kept = ~finite | ((np.abs(ref) <= HUGE) & ((ref == 0) | (np.abs(ref) >= TINY)))
        same_kind = np.where(np.isnan(ref), np.isnan(got), got == ref)               # NaN with NaN, infinities by sign
        dist = np.abs(got - ref)
        bound = np.maximum(FLOOR * np.abs(ref), 2 * np.abs(np32 - ref))
        ok = np.where(finite, dist <= bound, same_kind)
    return kept & ~ok, kept, np.where(finite, dist, np.where(same_kind, 0.0, np.inf)), np.where(finite, bound, 0.0)


# ---- views ----------------------------------------------------------------------------------------------------------------------------

View = namedtuple("View", "size offset strides")          # payload elements, element offset of [0, ..., 0], strides in elements
Case = namedtuple("Case", "name family op shape ins outs plan feature")     # ins: Views or None (the scalar); outs: Views or the index of the input they ARE


def A(*shape):
    """a fresh dense base array: the payload of one operand"""
    return np.zeros(shape, np.float32)


def _view(arr, shape):
    root = arr
    while root.base is not None:
        root = root.base
    b = np.broadcast_to(arr, shape)
    off = b.__array_interface__["data"][0] - root.__array_interface__["data"][0]
    assert off % 4 == 0 and all(s % 4 == 0 for s in b.strides)
    return View(int(root.size), off // 4, tuple(s // 4 for s in b.strides))


def element_index(view, shape):
    """the payload index of every element of a view, as an int64 array of `shape`"""
    idx = np.full(shape, view.offset, np.int64)
    for k, (n, st) in enumerate(zip(shape, view.strides)):
        idx += (np.arange(n, dtype=np.int64) * st).reshape((n,) + (1,) * (len(shape) - 1 - k))
    return idx


_cases = []


def case(family, name, op, shape, ins, outs, plan, feature=""):
    """ins: numpy views (of fresh bases) or None; outs: numpy views or the index of the input an output is (in place)"""
    shape = tuple(shape)
    nin, nout = OPS[op][1:3]
    assert len(ins) == nin and len(outs) == nout, name
    ins = tuple(None if a is None else _view(a, shape) for a in ins)
    outs = tuple(o if isinstance(o, int) else _view(o, shape) for o in outs)
    _cases.append(Case("%s_%s" % (FAMILIES[family], name), family, op, shape, ins, outs, (family,) + tuple(plan), feature))


def dense_ins(op, shape):
    return [A(*shape) for _ in range(OPS[op][1])]


def dense_outs(op, shape):
    return [A(*shape) for _ in range(OPS[op][2])]


def with_scalar(ins, slot):
    return [None if i == slot else a for i, a in enumerate(ins)]


def full_mask(op, but=None):
    m = (1 << OPS[op][1]) - 1
    return m if but is None else m & ~(1 << but)


def Tr(r, c, pitch=None, off=0):
    """an (r, c) view that is column-contiguous: the transpose of a dense (c, r) matrix (row pitch `pitch`, base off by `off`)"""
    pitch = pitch or r
    return A(c * pitch + off)[off:].reshape(c, pitch)[:, :r].T


def P(r, c, pitch, off=0):
    """an (r, c) view of rows `pitch` apart, base off by `off` elements"""
    return A(r * pitch + off)[off:].reshape(r, pitch)[:, :c]


# ---- flat -------------------------------------------------------------------------------------------------------------------------------
FLAT_FORM = {1: TAIL, 3: TAIL, 4: VEC, 5: VEC | TAIL, 1023: VEC | TAIL, 1024: VEC, 1027: VEC | TAIL}


def _flat_table():
    for n, form in FLAT_FORM.items():
        for op in SWEEP_OPS:
            # one element: every stride collapses to 0 and the mask is empty
            case(FLAT, "%s_n%d" % (op, n), op, (n,), dense_ins(op, (n,)), dense_outs(op, (n,)), (form, 1, full_mask(op) if n > 1 else 0))
    n = 1027
    for op in SWEEP_OPS:
        for slot in range(OPS[op][1]):
            if OPS[op][1] > 1:
                case(FLAT, "%s_scalar%d" % (op, slot), op, (n,), with_scalar(dense_ins(op, (n,)), slot), dense_outs(op, (n,)),
                     (VEC | TAIL, 1, full_mask(op, slot)))
    # a base off by one element: no float4 kernel, the tail kernel does everything
    case(FLAT, "sub_input_off_by_one", "sub", (n,), [A(n + 1)[1:], A(n)], [A(n)], (TAIL, 1, 0b11))
    case(FLAT, "neg_output_off_by_one", "neg", (n,), [A(n)], [A(n + 1)[1:]], (TAIL, 1, 0b1))
    case(FLAT, "mul_bwd_second_output_off_by_one", "mul_bwd", (n,), dense_ins("mul_bwd", (n,)), [A(n), A(n + 3)[3:]], (TAIL, 1, 0b111))
    case(FLAT, "pow_bwd_input_off_by_two", "pow_bwd", (n,), [A(n), A(n), A(n + 2)[2:], A(n)], dense_outs("pow_bwd", (n,)), (TAIL, 1, 0b1111))
    # an input of stride 0: one value in memory
    case(FLAT, "sub_b_stride0", "sub", (n,), [A(n), A(1)], [A(n)], (VEC | TAIL, 1, 0b01))
    case(FLAT, "fma_a_stride0", "fma", (n,), [A(1), A(n), A(n)], [A(n)], (VEC | TAIL, 1, 0b110))
    case(FLAT, "div_a_stride0_unaligned", "div", (n,), [A(2)[1:], A(n)], [A(n)], (VEC | TAIL, 1, 0b10), "a stride-0 input needs no alignment")
    case(FLAT, "div_bwd_two_stride0", "div_bwd", (n,), [A(1), A(n), A(1)], dense_outs("div_bwd", (n,)), (VEC | TAIL, 1, 0b010))
    # one element behind arbitrary strides
    case(FLAT, "sub_one_element_any_strides", "sub", (1, 1, 1), [A(7, 5, 3)[2:3, 1:2, 2:3], A(4, 4, 4)[3:, 3:, 1:2]], [A(3, 3, 3)[1:2, 2:, 0:1]], (TAIL, 1, 0))
    case(FLAT, "mul_bwd_one_element_any_strides", "mul_bwd", (1, 1), [A(3, 3)[1:2, 1:2], None, A(1, 1)], [A(2, 5)[1:, 3:4], A(5)[4:].reshape(1, 1)], (TAIL, 1, 0))
    # dense operands of several dimensions collapse to one run
    case(FLAT, "neg_3d_dense", "neg", (3, 5, 7), [A(3, 5, 7)], [A(3, 5, 7)], (VEC | TAIL, 1, 0b1))
    case(FLAT, "max_bwd_4d_dense_and_one_value", "max_bwd", (2, 3, 4, 5), [A(2, 3, 4, 5), A(1, 1, 1, 1), A(2, 3, 4, 5)], [A(2, 3, 4, 5)], (VEC, 1, 0b101))
    # in place
    case(FLAT, "sub_in_place_a", "sub", (n,), [A(n), A(n)], [0], (VEC | TAIL, 1, 0b11))
    case(FLAT, "div_in_place_b", "div", (n,), [A(n), A(n)], [1], (VEC | TAIL, 1, 0b11))
    case(FLAT, "fma_in_place_c", "fma", (n,), [A(n), None, A(n)], [2], (VEC | TAIL, 1, 0b101))
    case(FLAT, "mul_bwd_in_place_a", "mul_bwd", (n,), dense_ins("mul_bwd", (n,)), [0, A(n)], (VEC | TAIL, 1, 0b111))
    case(FLAT, "pow_bwd_in_place_g_off_by_one", "pow_bwd", (n,), [A(n), A(n), A(n + 1)[1:], A(n)], [A(n), 2], (TAIL, 1, 0b1111))


# ---- rows -------------------------------------------------------------------------------------------------------------------------------

def _rows_table():
    for r in (3, 5):
        for c in (4, 8, 260):
            s = (r, c)
            tag = "%dx%d" % s
            case(ROWS, "sub_row_vector_%s" % tag, "sub", s, [A(r, c), A(c)], [A(r, c)], (0, 2, 0))
            case(ROWS, "div_column_%s" % tag, "div", s, [A(r, c), A(r, 1)], [A(r, c)], (0, 2, 0))
            case(ROWS, "fma_both_broadcasts_%s" % tag, "fma", s, [A(c), A(r, 1), A(r, c)], [A(r, c)], (0, 2, 0))
            case(ROWS, "neg_input_pitch_%s" % tag, "neg", s, [P(r, c, c + 4)], [A(r, c)], (0, 2, 0))
            case(ROWS, "sub_output_pitch_%s" % tag, "sub", s, [A(r, c), A(r, c)], [P(r, c, c + 4)], (0, 2, 0), "the gap stays SENTINEL")
            # the same shapes, a pitch or a base that breaks the 16-byte alignment: ANOTHER path, and still right
            case(FLAT2D, "sub_input_pitch_plus_one_%s" % tag, "sub", s, [P(r, c, c + 1), A(c)], [A(r, c)], (0, 2, 0))
            case(FLAT2D, "div_input_off_by_one_%s" % tag, "div", s, [P(r, c, c, 1), A(r, 1)], [A(r, c)], (0, 2, 0))
            case(GATHER, "sub_output_pitch_plus_one_%s" % tag, "sub", s, [A(r, c), A(c)], [P(r, c, c + 1)], (0, 2, 0))
            case(GATHER, "fma_output_off_by_one_%s" % tag, "fma", s, [A(c), A(r, 1), A(r, c)], [P(r, c, c, 1)], (0, 2, 0))
    for c in (4, 8, 260):              # one row is one run: the flat path
        case(FLAT, "sub_row_vector_1x%d" % c, "sub", (1, c), [A(1, c), A(c)], [A(1, c)], (VEC, 1, 0b11))
        case(FLAT, "div_column_1x%d" % c, "div", (1, c), [A(1, c), A(1, 1)], [A(1, c)], (VEC, 1, 0b01))
    r, c = 5, 8
    s = (r, c)
    case(ROWS, "max_bwd_column_extremum", "max_bwd", s, [A(r, c), A(r, 1), A(r, c)], [A(r, c)], (0, 2, 0))
    case(ROWS, "mul_bwd_row_vector", "mul_bwd", s, [A(r, c), A(c), A(r, c)], [A(r, c), A(r, c)], (0, 2, 0))
    case(ROWS, "div_bwd_column_two_pitched_outputs", "div_bwd", s, [A(r, c), A(r, 1), A(r, c)], [P(r, c, c + 4), P(r, c, c + 8)], (0, 2, 0))
    case(ROWS, "pow_bwd_row_vector_and_column", "pow_bwd", s, [A(r, c), A(c), A(r, 1), P(r, c, c + 4)], [A(r, c), A(r, c)], (0, 2, 0))
    for op in SWEEP_OPS:
        for slot in range(OPS[op][1]):
            if OPS[op][1] > 1:
                ins = dense_ins(op, s)
                ins[(slot + 1) % len(ins)] = P(r, c, c + 4)          # what keeps the case off the flat path
                case(ROWS, "%s_scalar%d" % (op, slot), op, s, with_scalar(ins, slot), dense_outs(op, s), (0, 2, 0))
    case(ROWS, "sub_3d_middle_broadcast", "sub", (3, 5, 8), [A(3, 5, 8), A(3, 1, 8)], [A(3, 5, 8)], (0, 3, 0))
    case(ROWS, "div_3d_outer_and_inner_broadcast", "div", (3, 5, 8), [A(3, 5, 8), A(1, 5, 1)], [A(3, 5, 8)], (0, 3, 0))
    case(ROWS, "fma_3d_all_three", "fma", (3, 5, 8), [A(3, 1, 8), A(1, 5, 1), A(3, 5, 8)], [A(3, 5, 8)], (0, 3, 0))
    case(ROWS, "sub_4d_keepdims", "sub", (2, 3, 5, 8), [A(2, 3, 5, 8), A(2, 3, 5, 1)], [A(2, 3, 5, 8)], (0, 2, 0), "the leading dimensions merge")
    case(ROWS, "mul_bwd_4d_keepdims_two_axes", "mul_bwd", (2, 3, 5, 8), [A(2, 3, 5, 8), A(2, 1, 5, 1), A(2, 3, 5, 8)], [A(2, 3, 5, 8), A(2, 3, 5, 8)], (0, 4, 0))
    case(ROWS, "neg_3d_middle_axis_reversed", "neg", (3, 5, 8), [A(3, 5, 8)[:, ::-1, :]], [A(3, 5, 8)], (0, 3, 0), "a negative outer stride")
    case(ROWS, "sub_in_place_row_vector", "sub", s, [A(r, c), A(c)], [0], (0, 2, 0))
    case(ROWS, "fma_in_place_pitched_c", "fma", s, [A(r, 1), A(c), P(r, c, c + 4)], [2], (0, 2, 0))
    case(ROWS, "div_bwd_in_place_g", "div_bwd", s, [A(r, c), A(c), A(r, c)], [2, A(r, c)], (0, 2, 0))


# ---- the transposed tile ------------------------------------------------------------------------------------------------------------

def _tile_table():
    def one(op, r, c, form, name, feature=""):
        """`op` with input 1 transposed (input 0 for the one-input op), the rest dense"""
        ins = dense_ins(op, (r, c))
        t = 0 if len(ins) == 1 else 1
        ins[t] = Tr(r, c)
        case(TILE, "%s_%s_%dx%d" % (op, name, r, c), op, (r, c), ins, dense_outs(op, (r, c)), (form, 2, 1 << t), feature)
    for (r, c), form in (((16, 16), TILE_V4_ONE), ((17, 16), TILE_SCALAR), ((16, 18), TILE_SCALAR), ((64, 64), TILE_V4_ONE)):
        for op in ("neg", "sub", "mul_bwd"):
            one(op, r, c, form, "one_transposed")
    for op in SWEEP_OPS:                                               # several ragged tiles, every arity class
        one(op, 68, 132, TILE_V4_ONE, "ragged")
        one(op, 130, 67, TILE_SCALAR, "ragged")
    for (r, c) in ((64, 200), (200, 64)):                              # the diagonal walk with tiles_r != tiles_c
        one("sub", r, c, TILE_V4_ONE, "diagonal")
        case(TILE, "div_two_transposed_%dx%d" % (r, c), "div", (r, c), [Tr(r, c), Tr(r, c)], [A(r, c)], (TILE_V4_TWO, 2, 0b11))
        case(TILE, "pow_bwd_two_transposed_%dx%d" % (r, c), "pow_bwd", (r, c), [A(r, c), Tr(r, c), A(r, c), Tr(r, c)], [A(r, c), A(r, c)], (TILE_V4_TWO, 2, 0b1010))
    case(TILE, "sub_two_transposed_64x64", "sub", (64, 64), [Tr(64, 64), Tr(64, 64)], [A(64, 64)], (TILE_V4_TWO, 2, 0b11))
    case(TILE, "fma_two_transposed_130x67", "fma", (130, 67), [Tr(130, 67), A(130, 67), Tr(130, 67)], [A(130, 67)], (TILE_SCALAR, 2, 0b101))
    case(TILE, "div_bwd_two_transposed_17x16", "div_bwd", (17, 16), [Tr(17, 16), Tr(17, 16), A(17, 16)], [A(17, 16), A(17, 16)], (TILE_SCALAR, 2, 0b011))
    # a row-contiguous, a row-broadcast and a column-broadcast input next to a transposed one
    for (r, c), form in (((68, 132), TILE_V4_ONE), ((130, 67), TILE_SCALAR)):
        tag = "%dx%d" % (r, c)
        case(TILE, "fma_row_vector_and_column_%s" % tag, "fma", (r, c), [Tr(r, c), A(c), A(r, 1)], [A(r, c)], (form, 2, 0b001))
        case(TILE, "max_bwd_column_extremum_%s" % tag, "max_bwd", (r, c), [Tr(r, c), A(r, 1), A(r, c)], [A(r, c)], (form, 2, 0b001))
        case(TILE, "pow_bwd_all_kinds_%s" % tag, "pow_bwd", (r, c), [A(r, c), A(c), A(r, 1), Tr(r, c)], [A(r, c), A(r, c)], (form, 2, 0b1000))
        case(TILE, "mul_bwd_pitched_outputs_%s" % tag, "mul_bwd", (r, c), [A(r, c), Tr(r, c), A(c)], [P(r, c, c + 4), A(r, c)], (form, 2, 0b010))
    # pitches: C + 4 on the output; R + 4 on the transposed side keeps float4, R + 1 takes the scalar tile
    case(TILE, "sub_output_pitch_64x64", "sub", (64, 64), [A(64, 64), Tr(64, 64)], [P(64, 64, 68)], (TILE_V4_ONE, 2, 0b10))
    case(TILE, "sub_transposed_pitch_plus_four_64x64", "sub", (64, 64), [A(64, 64), Tr(64, 64, 68)], [A(64, 64)], (TILE_V4_ONE, 2, 0b10))
    case(TILE, "sub_transposed_pitch_plus_one_64x64", "sub", (64, 64), [A(64, 64), Tr(64, 64, 65)], [A(64, 64)], (TILE_SCALAR, 2, 0b10))
    case(TILE, "div_input_pitch_plus_one_68x132", "div", (68, 132), [P(68, 132, 133), Tr(68, 132)], [A(68, 132)], (TILE_SCALAR, 2, 0b10))
    # offset views that break the 16-byte alignment
    case(TILE, "sub_transposed_off_by_one_16x16", "sub", (16, 16), [A(16, 16), Tr(16, 16, None, 1)], [A(16, 16)], (TILE_SCALAR, 2, 0b10))
    case(TILE, "neg_output_off_by_one_64x64", "neg", (64, 64), [Tr(64, 64)], [P(64, 64, 64, 1)], (TILE_SCALAR, 2, 0b1))
    case(TILE, "fma_dense_input_off_by_two_68x132", "fma", (68, 132), [Tr(68, 132), P(68, 132, 132, 2), A(132)], [A(68, 132)], (TILE_SCALAR, 2, 0b001))
    # not this path: an extent below 16, three transposed inputs
    case(FLAT2D, "sub_transposed_15x16", "sub", (15, 16), [A(15, 16), Tr(15, 16)], [A(15, 16)], (0, 2, 0b01))
    case(FLAT2D, "fma_three_transposed_16x16", "fma", (16, 16), [Tr(16, 16), Tr(16, 16), Tr(16, 16)], [A(16, 16)], (0, 2, 0))
    # the scalar operand in every slot, float4 and scalar tiles alternating
    k = 0
    for op in SWEEP_OPS:
        for slot in range(OPS[op][1]):
            if OPS[op][1] > 1:
                (r, c), form = (((16, 16), TILE_V4_ONE), ((17, 16), TILE_SCALAR))[k % 2]
                k += 1
                ins = dense_ins(op, (r, c))
                t = (slot + 1) % len(ins)
                ins[t] = Tr(r, c)
                case(TILE, "%s_scalar%d_%dx%d" % (op, slot, r, c), op, (r, c), with_scalar(ins, slot), dense_outs(op, (r, c)), (form, 2, 1 << t))
    # in place: `grad += g.T`
    case(TILE, "sub_in_place_64x200", "sub", (64, 200), [A(64, 200), Tr(64, 200)], [0], (TILE_V4_ONE, 2, 0b10))
    case(TILE, "fma_in_place_pitched_130x67", "fma", (130, 67), [Tr(130, 67), None, P(130, 67, 71)], [2], (TILE_SCALAR, 2, 0b001))
    case(TILE, "mul_bwd_in_place_two_transposed_68x132", "mul_bwd", (68, 132), [Tr(68, 132), Tr(68, 132), A(68, 132)], [2, A(68, 132)], (TILE_V4_TWO, 2, 0b011))


# ---- flat-2D -----------------------------------------------------------------------------------------------------------------------------

def _flat2d_table():
    for r, c in ((4, 3), (6, 2), (4, 7), (36, 10), (128, 513)):
        s, tag = (r, c), "%dx%d" % (r, c)
        case(FLAT2D, "sub_row_vector_%s" % tag, "sub", s, [A(r, c), A(c)], [A(r, c)], (0, 2, 0b01), "one float4 spans rows")
        case(FLAT2D, "div_column_%s" % tag, "div", s, [A(r, 1), A(r, c)], [A(r, c)], (0, 2, 0b10))
        case(FLAT2D, "sub_both_broadcast_%s" % tag, "sub", s, [A(c), A(r, 1)], [A(r, c)], (0, 2, 0))
        case(FLAT2D, "mul_bwd_row_vector_%s" % tag, "mul_bwd", s, [A(r, c), A(c), A(r, c)], [A(r, c), A(r, c)], (0, 2, 0b101))
    r, c = 36, 10
    s = (r, c)
    case(FLAT2D, "neg_pitched_input", "neg", s, [P(r, c, c + 3)], [A(r, c)], (0, 2, 0))
    case(FLAT2D, "neg_last_axis_reversed", "neg", (4, 8), [A(4, 8)[:, ::-1]], [A(4, 8)], (0, 2, 0), "a negative inner stride")
    case(FLAT2D, "fma_row_vector_and_column", "fma", s, [A(c), A(r, 1), A(r, c)], [A(r, c)], (0, 2, 0b100))
    case(FLAT2D, "max_bwd_column_extremum", "max_bwd", s, [A(r, c), A(r, 1), A(r, c)], [A(r, c)], (0, 2, 0b101))
    case(FLAT2D, "div_bwd_column", "div_bwd", s, [A(r, c), A(r, 1), A(r, c)], [A(r, c), A(r, c)], (0, 2, 0b101))
    case(FLAT2D, "pow_bwd_row_vector_and_column", "pow_bwd", s, [A(r, c), A(c), A(r, 1), A(r, c)], [A(r, c), A(r, c)], (0, 2, 0b1001))
    case(GATHER, "sub_row_vector_3x5", "sub", (3, 5), [A(3, 5), A(5)], [A(3, 5)], (0, 2, 0), "15 elements: no float4 over the flat index")
    for op in SWEEP_OPS:
        for slot in range(OPS[op][1]):
            if OPS[op][1] > 1:
                ins = dense_ins(op, s)
                t = (slot + 1) % len(ins)
                ins[t] = A(c)
                case(FLAT2D, "%s_scalar%d" % (op, slot), op, s, with_scalar(ins, slot), dense_outs(op, s), (0, 2, full_mask(op) & ~(1 << t) & ~(1 << slot)))
    case(FLAT2D, "sub_in_place_row_vector", "sub", s, [A(r, c), A(c)], [0], (0, 2, 0b01))
    case(FLAT2D, "mul_bwd_in_place_g", "mul_bwd", s, [A(r, 1), A(r, c), A(r, c)], [A(r, c), 2], (0, 2, 0b110))


# ---- gather ------------------------------------------------------------------------------------------------------------------------------

def _gather_table():
    case(GATHER, "neg_3d_permuted_201", "neg", (7, 3, 5), [A(3, 5, 7).transpose(2, 0, 1)], [A(7, 3, 5)], (0, 2, 0), "two dimensions merge")
    case(GATHER, "neg_3d_permuted_102", "neg", (5, 3, 7), [A(3, 5, 7).transpose(1, 0, 2)], [A(5, 3, 7)], (0, 3, 0))
    case(GATHER, "sub_3d_permuted_210", "sub", (7, 5, 3), [A(3, 5, 7).transpose(2, 1, 0), A(7, 5, 3)], [A(7, 5, 3)], (0, 3, 0))
    case(GATHER, "fma_3d_three_permutations", "fma", (3, 5, 7), [A(5, 3, 7).transpose(1, 0, 2), A(7, 5, 3).transpose(2, 1, 0), A(3, 7, 5).transpose(0, 2, 1)],
         [A(3, 5, 7)], (0, 3, 0))
    case(GATHER, "neg_1d_reversed", "neg", (8,), [A(8)[::-1]], [A(8)], (0, 1, 0), "a negative stride")
    case(GATHER, "sub_last_axis_reversed", "sub", (5, 7), [A(5, 7)[:, ::-1], A(5, 7)], [A(5, 7)], (0, 2, 0))
    case(GATHER, "div_middle_axis_reversed", "div", (3, 5, 7), [A(3, 5, 7), A(3, 5, 7)[:, ::-1, :]], [A(3, 5, 7)], (0, 3, 0))
    case(GATHER, "max_bwd_every_axis_reversed", "max_bwd", (3, 5, 7), [A(3, 5, 7)[::-1, ::-1, ::-1], A(3, 1, 1), A(3, 5, 7)], [A(3, 5, 7)], (0, 2, 0))
    case(GATHER, "sub_transposed_15x17", "sub", (15, 17), [A(15, 17), Tr(15, 17)], [A(15, 17)], (0, 2, 0), "an extent below 16")
    case(GATHER, "mul_bwd_transposed_7x9", "mul_bwd", (7, 9), [Tr(7, 9), A(7, 9), Tr(7, 9)], [A(7, 9), A(7, 9)], (0, 2, 0))
    e = (2,) * 8
    case(GATHER, "neg_8d_reversed_axes", "neg", e, [A(*e).transpose(7, 6, 5, 4, 3, 2, 1, 0)], [A(*e)], (0, 8, 0), "nothing collapses")
    case(GATHER, "fma_8d_three_permutations", "fma", e, [A(*e).transpose(1, 0, 3, 2, 5, 4, 7, 6), A(*e).transpose(7, 6, 5, 4, 3, 2, 1, 0), A(*e)],
         [A(*e)], (0, 8, 0))
    case(GATHER, "pow_bwd_8d", "pow_bwd", e, [A(*e), A(*e).transpose(1, 0, 3, 2, 5, 4, 7, 6), A(*e), A(*e)], [A(*e), A(*e).transpose(7, 6, 5, 4, 3, 2, 1, 0)], (0, 8, 0))
    # the output itself a permuted view
    case(GATHER, "sub_permuted_output_5x7", "sub", (5, 7), [A(5, 7), A(5, 7)], [Tr(5, 7)], (0, 2, 0))
    case(GATHER, "div_permuted_output_17x20", "div", (17, 20), [A(17, 20), A(20)], [Tr(17, 20)], (0, 2, 0))
    case(GATHER, "div_bwd_permuted_outputs_3d", "div_bwd", (3, 5, 7), [A(3, 5, 7), A(5, 1), A(3, 5, 7)], [A(7, 5, 3).transpose(2, 1, 0), A(5, 3, 7).transpose(1, 0, 2)], (0, 3, 0))
    case(GATHER, "sub_strided_output", "sub", (9,), [A(9), A(9)], [A(18)[::2]], (0, 1, 0), "every second element: the others stay SENTINEL")
    s = (5, 7)
    for op in SWEEP_OPS:
        for slot in range(OPS[op][1]):
            if OPS[op][1] > 1:
                ins = dense_ins(op, s)
                ins[(slot + 1) % len(ins)] = Tr(*s)
                case(GATHER, "%s_scalar%d" % (op, slot), op, s, with_scalar(ins, slot), dense_outs(op, s), (0, 2, 0))
    case(GATHER, "sub_in_place_permuted_view", "sub", s, [Tr(*s), A(*s)], [0], (0, 2, 0))
    case(GATHER, "fma_in_place_reversed_c", "fma", (3, 5, 7), [A(3, 5, 7), A(7), A(3, 5, 7)[:, ::-1, :]], [2], (0, 3, 0))
    case(GATHER, "pow_bwd_in_place_transposed_a", "pow_bwd", s, [Tr(*s), A(*s), A(7), A(*s)], [0, A(*s)], (0, 2, 0))


_flat_table()
_rows_table()
_tile_table()
_flat2d_table()
_gather_table()
SWEEP_CASES = tuple(_cases)
SWEEP_BY_NAME = {c.name: c for c in SWEEP_CASES}


def out_view(c, o):
    v = c.outs[o]
    return c.ins[v] if isinstance(v, int) else v


def in_place_slots(c):
    return {v: o for o, v in enumerate(c.outs) if isinstance(v, int)}


def _sweep_values(c, slot):
    """the values of input `slot`, one per DISTINCT element of its view (broadcast extents are 1)"""
    v = c.ins[slot]
    own = tuple(1 if st == 0 else n for n, st in zip(c.shape, v.strides))
    rng = rng_for(c.name, "in%d" % slot)
    if c.op == "max_bwd" and slot < 2:
        return rng.randint(0, 3, own).astype(np.float32)                # ties between x and the extremum happen
    x = rng.uniform(0.5, 2.0, own).astype(np.float32)                   # away from zero: divisors, and the base of pow_bwd
    if not (c.op == "pow_bwd" and slot == 0):
        x *= rng.choice(np.float32([-1, 1]), own)
    return x


@lru_cache(maxsize=None)
def sweep_arrays(name):
    """(inputs broadcast to the case's shape [None: the scalar], float32 references, float64 references)"""
    c = SWEEP_BY_NAME[name]
    ins = [None if v is None else np.broadcast_to(_sweep_values(c, i), c.shape) for i, v in enumerate(c.ins)]
    full = [np.full(c.shape, SCALAR, np.float32) if a is None else a for a in ins]
    ref32, ref64 = evaluate(c.op, full, np.float32), evaluate(c.op, full, np.float64)
    for a in ref32 + ref64:
        a.setflags(write=False)
    return ins, ref32, ref64


def input_buffer(c, slot):
    """the guarded flat array of input `slot`: NaN wherever the view does not reach"""
    v = c.ins[slot]
    pay = np.full(v.size, np.nan, np.float32)
    pay[element_index(v, c.shape)] = sweep_arrays(c.name)[0][slot]
    return padded(pay, np.nan)


def output_buffers(c, o):
    """(prefill, expected) guarded flat arrays of output `o`: SENTINEL wherever the view does not reach"""
    v = out_view(c, o)
    idx = element_index(v, c.shape)
    pay = np.full(v.size, SENTINEL, np.float32)
    pay[idx] = sweep_arrays(c.name)[0][c.outs[o]] if isinstance(c.outs[o], int) else np.nan
    want = pay.copy()
    want[idx] = sweep_arrays(c.name)[1][o]
    return padded(pay, SENTINEL), padded(want, SENTINEL)


# ---- the value sweep ------------------------------------------------------------------------------------------------------------------

DENORMAL = 1e-41
COMMON = [0.0, -0.0, 1.0, -1.0, np.inf, -np.inf, np.nan, TINY, -TINY, DENORMAL, -DENORMAL, HUGE, -HUGE,
          88.7, -88.7, 87.3, -87.3, -104.0,                       # exp at overflow and underflow
          1 - 2.0 ** -24, 1 + 2.0 ** -23, 0.5, 2.0,               # straddling 1 for log
          1e4, -1e4, 1e6,                                         # large sin / cos arguments
          20.0, -20.0,                                            # tanh, sigmoid, gelu saturated
          -2.5, 3.0, 1e20]
GRADS = [1.0, -2.5, 0.0, np.inf, np.nan, HUGE]
SMALL = [0.0, -0.0, 1.0, -1.0, np.inf, -np.inf, np.nan, TINY, DENORMAL, HUGE, 2.5, -88.7]
POW_BASES = [0.0, -0.0, 1.0, -1.0, np.inf, -np.inf, np.nan, 2.0, -2.0, 0.5, -0.5, -2.5, 10.0, TINY, HUGE]
POW_EXPONENTS = [0.0, -0.0, 1.0, -1.0, 2.0, 3.0, -2.0, 0.5, -0.5, 2.5, np.inf, -np.inf, np.nan, 40.0, -40.0]
DIV_BWD_A, DIV_BWD_B, DIV_BWD_G = [0.0, -0.0, 1.0, -1.0, np.inf, np.nan, 2.5, -88.7, HUGE], [0.0, -0.0, 1.0, -2.5, np.inf, np.nan, 1e10, 1e-10], [1.0, -2.5, np.inf]
# special values of operand 0 at which float32 ITSELF leaves its range in an intermediate of the expression - y * (1 - y) and y * y
# overflow, 1 / x of a denormal is inf, gelu's inner product overflows before the tanh - so that numpy float32 gives NaN where the
# exact result is finite and is no reference: not paired with the gradients (the forward ops keep every one of them)
NOT_PAIRED = {"sigmoid_bwd": (HUGE, -HUGE, 1e20), "tanh_bwd": (HUGE, -HUGE, 1e20), "gelu_bwd": (HUGE, -HUGE, 1e20), "log_bwd": (DENORMAL, -DENORMAL)}
# where the random values of operand 0 lie: wide enough for every regime of the function, narrow enough that float32 itself
# evaluates the expression well (gelu: 1 + tanh(u) cancels below -2.4; the saturated ends are among the special values)
RANDOM_RANGE = {"exp": (-30, 30), "log": (0.01, 100), "sqrt": (0, 100), "sin": (-10, 10), "cos": (-10, 10), "sin_bwd": (-10, 10),
                "cos_bwd": (-10, 10), "gelu": (-2, 2), "gelu_bwd": (-2, 2), "sigmoid": (-30, 30), "tanh": (-6, 6),
                "sigmoid_bwd": (0, 1), "tanh_bwd": (-1, 1), "log_bwd": (0.01, 100), "pow": (0.1, 5), "pow_bwd": (0.1, 5)}


# gelu'(x) has a zero at x = -0.7518: the two terms of gelu_grad, of size 0.1 to 1, cancel there, and the four float32 roundings on the
# way (tanh, 1 + th, the products, the sum: 4 * 2**-24 of the larger term) are then 2.4e-7 / |gelu'(x)| of the result - above FLOOR for
# |gelu'(x)| < 0.024 whatever evaluates the expression, numpy included.  The random values keep |gelu'(x)| >= 2**-5.
GELU_SLOPE_MIN = 2.0 ** -5


def gelu_slope(x):
    return np.abs(evaluate("gelu_bwd", [x, np.ones_like(x, dtype=np.float32)], np.float64)[0])


def _cross(*lists):
    grids = np.meshgrid(*[np.float32(l) for l in lists], indexing="ij")
    return [g.reshape(-1) for g in grids]


@lru_cache(maxsize=None)
def value_inputs(op):
    """the NIN float32 arrays of VALUE_N elements: the special values (every combination for several operands), then random ones"""
    nin, klass = OPS[op][1], OPS[op][3]
    if op == "pow":
        special = _cross(POW_BASES, POW_EXPONENTS)
    elif op == "pow_bwd":
        a, b = _cross(POW_BASES, POW_EXPONENTS)
        g = np.float32([1.0, -0.5])[np.arange(a.size) % 2]
        with np.errstate(all="ignore"):
            special = [a, b, g, np.power(a, b)]
    elif op == "div_bwd":
        special = _cross(DIV_BWD_A, DIV_BWD_B, DIV_BWD_G)
    elif nin == 1:
        special = [np.float32(COMMON)]
    elif nin == 2:
        special = _cross([v for v in COMMON if v not in NOT_PAIRED.get(op, ())], COMMON if klass == "exact" else GRADS)
    else:
        special = _cross(*([SMALL] * nin))
    n_special = special[0].size
    assert n_special <= VALUE_N // 2, (op, n_special)
    rng = rng_for("value_" + op)
    out = []
    for i in range(nin):
        lo, hi = RANDOM_RANGE.get(op, (-4, 4)) if i == 0 else (-4, 4)
        r = rng.uniform(lo, hi, VALUE_N - n_special).astype(np.float32)
        if op in ("max_bwd", "eq", "ge") and i < 2:
            r = np.rint(r)                                              # ties happen
        if op == "gelu_bwd" and i == 0:
            r = np.where(gelu_slope(r) < GELU_SLOPE_MIN, r + np.float32(0.25), r).astype(np.float32)
        out.append(np.concatenate([special[i], r]).astype(np.float32))
    if op == "pow_bwd":
        with np.errstate(all="ignore"):
            out[3] = np.power(out[0], out[1])                           # y is what the forward saved
    for a in out:
        a.setflags(write=False)
    return tuple(out)


@lru_cache(maxsize=None)
def value_references(op):
    """(float32 numpy outputs, float64 outputs) on value_inputs(op)"""
    ins = value_inputs(op)
    return evaluate(op, ins, np.float32), evaluate(op, ins, np.float64)
