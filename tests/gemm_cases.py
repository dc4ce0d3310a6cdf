"""The case table of the SGEMM tile sweep (csrc/gemm.hip, gemm_tile_body.inc) and its float64 reference, shared by
tests/test_gemm_cases_cpu.py (no GPU: the table and the rules themselves) and tests/gemm_tile_worker.py (the GPU child of
tests/test_hip_gemm_tiles.py).

Every tile gemm_impl can choose - the two skinny tiles, 64x64 with and without the cross-workgroup K split, 32x32 with four
K-groups, 64x32 / 32x64 with two K-groups, 128x128 with and without the split, 256x256 - in all four operand layouts, at the
K, M, N, leading-dimension and slice-count edges of that tile.  The library reads LG_GEMM_TILE / LG_GEMM_SLICES once per
process, so each configuration is a CHILD (CHILDREN) with its own list of cases.

Operands live in buffers that are NaN wherever a kernel may read without being allowed to use what it reads: 64 floats in
front of and behind every operand, and the padding columns of its leading dimension.  A K-contiguous float4 that runs past K,
or an M- / N-contiguous one that straddles the edge of the matrix, then carries NaN; if the kernel drops only one factor of such a
pair, 0 * NaN shows where 0 * finite would not.  Outputs sit in buffers pre-filled with PATTERN, a quiet NaN with a payload:
whatever lies outside the result must still be those bits after the call."""
import functools
import numpy as np

GUARD = 64                                   # floats of NaN in front of and behind every matrix
PATTERN = np.uint32(0x7FC5A5A5)              # quiet NaN with a payload: the state of every output byte before the call
PADS = (0, 1, 3, 5)                          # leading-dimension paddings: rows are not all 16-byte aligned
U = 2.0 ** -24                               # unit roundoff of float32

K32 = (1, 2, 3, 4, 5, 31, 32, 33, 63, 64, 65, 67, 101, 197)                    # tiles that stage 32 k per K-step
K64 = (1, 2, 3, 4, 5, 15, 16, 17, 63, 64, 65, 127, 128, 129, 131, 197)         # ... 64 (tiles 5, 7, 8)
K_SPLIT = (33, 65, 97, 129, 197, 225)                                         # LG_GEMM_SLICES=7: 2, 3, 4, 5, 7, 4 slices launched
K_FEW = (3, 33, 65, 197)                                                      # the epilogue variants
K_FEW_SPLIT = (33, 129, 197, 225)                                             # ... under the forced split: 2, 5, 7, 4 slices
FORCED_SLICES = 7

LAYOUTS = ((0, 0), (0, 1), (1, 0), (1, 1))                                    # (transA, transB)
FULL_K_VARIANTS = ("plain", "rowsum")
FEW_K_VARIANTS = ("accumulate", "bias", "addend", "relu_a", "relu_b", "rowsum_acc", "gelu", "gelu_bwd")
BATCHED_VARIANTS = ("batched", "batched_accumulate", "batched_bias", "batched2")
EXTRAS = ("rowsum", "rowsum_acc", "relu_a", "relu_b", "gelu", "gelu_bwd", "multi3", "kseg3")      # never on the 256x256 tile
SKINNY_64x32, SKINNY_32x64 = (64, 32, 32, 1), (32, 64, 32, 1)

# child -> environment, the tile it forces (BM, BN, BK, KG; None: the skinny tiles by shape), k-values staged per K-step, (M, N)
CHILDREN = {
    "a": dict(env={}, tile=None, stage=32, ks=K32, few=K_FEW,
              shapes=((1, 1), (70, 1), (1, 10), (70, 10), (1, 32), (70, 32), (1, 70), (10, 70), (32, 70))),
    "b": dict(env={"LG_GEMM_TILE": "9"}, tile=(64, 64, 32, 1), stage=32, ks=K32, few=K_FEW, shapes=((64, 64), (70, 50), (130, 77))),
    "c": dict(env={"LG_GEMM_TILE": "9", "LG_GEMM_SLICES": "7"}, tile=(64, 64, 32, 1), stage=32, ks=K_SPLIT, few=K_FEW_SPLIT,
              shapes=((64, 64), (70, 50), (130, 77), (70, 10), (10, 70))),
    "d": dict(env={"LG_GEMM_TILE": "5"}, tile=(32, 32, 16, 4), stage=64, ks=K64, few=K_FEW, shapes=((70, 50), (130, 77))),
    "e": dict(env={"LG_GEMM_TILE": "7"}, tile=(64, 32, 32, 2), stage=64, ks=K64, few=K_FEW, shapes=((70, 50), (130, 77))),
    "f": dict(env={"LG_GEMM_TILE": "8"}, tile=(32, 64, 32, 2), stage=64, ks=K64, few=K_FEW, shapes=((70, 50), (130, 77))),
    "g": dict(env={"LG_GEMM_TILE": "0"}, tile=(128, 128, 32, 1), stage=32, ks=K32, few=K_FEW, shapes=((130, 77), (127, 257))),
    "h": dict(env={"LG_GEMM_TILE": "0", "LG_GEMM_SLICES": "7"}, tile=(128, 128, 32, 1), stage=32, ks=K_SPLIT, few=K_FEW_SPLIT,
              shapes=((130, 77),)),
    "i": dict(env={"LG_GEMM_TILE": "2"}, tile=(256, 256, 32, 1), stage=32, ks=K32, few=K_FEW, shapes=((257, 130), (300, 513))),
}
BATCHED_CHILDREN = ("b", "c", "g", "h", "i")                                  # tiles 9, 0 and 2


def is_skinny(m, n):
    return m <= 32 or n <= 32


def rowsum_shapes(child):
    """the child's (M, N) list for the row-sum variants: both stagings of the virtual ones-column must run - float4 needs
    N % 4 == 0 (gemm_impl: vb), the scalar form N % 4 != 0 - so a list without one of the two gets a pair that has it"""
    shapes = list(CHILDREN[child]["shapes"])
    wide = [s for s in shapes if not is_skinny(*s)] or shapes
    if not any(n % 4 == 0 for _, n in wide):
        m, n = wide[0]
        shapes.append((m, n + 4 - n % 4 if (n + 4 - n % 4) % 32 else n + 8 - n % 4))
    if not any(n % 4 != 0 for _, n in wide):
        shapes.append((wide[0][0], wide[0][1] + 1))
    return tuple(shapes)


def cases(child):
    """the cases of one child, in an order that keeps the cases on one product (same M, N, K, layout) together"""
    spec = CHILDREN[child]
    out = []

    def add(variant, m, n, k, ta, tb):
        out.append(dict(child=child, variant=variant, m=m, n=n, k=k, ta=ta, tb=tb))

    for (m, n) in rowsum_shapes(child):
        listed = (m, n) in spec["shapes"]
        for (ta, tb) in LAYOUTS:
            for k in sorted(set(spec["ks"]) | set(spec["few"])):
                if k in spec["ks"]:
                    if listed:
                        add("plain", m, n, k, ta, tb)
                    add("rowsum", m, n, k, ta, tb)
                if k in spec["few"]:
                    for variant in FEW_K_VARIANTS:
                        if listed or variant == "rowsum_acc":
                            add(variant, m, n, k, ta, tb)
                    if listed and (ta, tb) == (0, 1):
                        add("multi3", m, n, k, ta, tb)                    # x @ W_i^T only
            if listed and (ta, tb) == (0, 0):
                add("kseg3", m, n, 192, ta, tb)                           # g @ [W0; W1; W2] only, seg_k = 64
        if listed and not is_skinny(m, n) and (m, n) == [s for s in spec["shapes"] if not is_skinny(*s)][-1]:
            for (ta, tb) in LAYOUTS:
                add("offset", m, n, 65, ta, tb)                           # operand pointers moved by one float
                if child in BATCHED_CHILDREN:
                    for variant in BATCHED_VARIANTS:
                        add(variant, m, n, 197, ta, tb)
    if child == "a":                                                      # the skinny tiles' own offset cases
        for (m, n) in ((70, 10), (10, 70)):
            for (ta, tb) in LAYOUTS:
                add("offset", m, n, 65, ta, tb)
    return out


def expected_tile(case):
    """(BM, BN, BK, KG) the case must report: the skinny tiles by shape whatever is forced, the forced tile otherwise - but a
    call with extras never runs on the 256x256 tile: gemm_impl moves it to 64x64"""
    if case["n"] <= 32:
        return SKINNY_64x32
    if case["m"] <= 32:
        return SKINNY_32x64
    tile = CHILDREN[case["child"]]["tile"]
    if tile[0] == 256 and case["variant"] in EXTRAS:
        return (64, 64, 32, 1)
    return tile


def expected_slices(case):
    """(k_slices, k_per_slice) under LG_GEMM_SLICES=7 by the documented rule, None where the cost model decides: k_per_slice =
    ceil(ceil(K / 7) / BK) * BK, slices = ceil(K / k_per_slice).  Tiles with K-groups and the 256x256 tile never split, and
    neither does a product whose K runs through three operands."""
    bm, bn, bk, kg = expected_tile(case)
    k = case["k"]
    if kg > 1 or bm == 256 or case["variant"] == "kseg3":
        return 1, -(-k // bk) * bk
    if "LG_GEMM_SLICES" not in CHILDREN[case["child"]]["env"]:
        return None
    per = -(-(-(-k // FORCED_SLICES)) // bk) * bk
    return -(-k // per), per


def expected_flags(case):
    """bits 0-4 of the plan's flags: A / B K-contiguous, float4 staging of A / B, wave-private K loop"""
    akc, bkc = case["ta"] == 0, case["tb"] == 1
    vb = not case["variant"].startswith("rowsum") or bkc or case["n"] % 4 == 0
    tile = expected_tile(case)
    wave_private = tile == (32, 32, 16, 4) and akc and bkc
    return (1 if akc else 0) | (2 if bkc else 0) | 4 | (8 if vb else 0) | (16 if wave_private else 0)


# ---- operands ---------------------------------------------------------------------------------------------------------
class Matrix:
    """`count` matrices of rows x cols float32 values inside a flat buffer `fill` everywhere else: GUARD floats, `shift` more,
    then matrix i at i * stride with leading dimension ld = cols + pad, then GUARD floats"""

    def __init__(self, values, pad, shift=0, gap=0, fill=np.nan):
        values = np.asarray(values, np.float32)
        self.count, self.rows, self.cols = values.shape
        self.ld = self.cols + pad
        self.stride = self.rows * self.ld + gap
        self.start = GUARD + shift
        size = self.start + (self.count - 1) * self.stride + (self.rows - 1) * self.ld + self.cols + GUARD
        self.buf = np.full(size, fill, np.float32) if not isinstance(fill, np.uint32) else np.full(size, fill, np.uint32).view(np.float32)
        self.inside = np.zeros(size, bool)
        for i in range(self.count):
            for r in range(self.rows):
                at = self.start + i * self.stride + r * self.ld
                self.inside[at:at + self.cols] = True
        self.put(values)

    def put(self, values):
        for i in range(self.count):
            view = self.buf[self.start + i * self.stride:][:(self.rows - 1) * self.ld + self.cols]
            for r in range(self.rows):
                view[r * self.ld:r * self.ld + self.cols] = values[i][r]

    def blank(self):
        """the matrices themselves filled like their surroundings (an output that the call overwrites)"""
        self.buf.view(np.uint32)[self.inside] = self.buf.view(np.uint32)[0]
        return self

    def get(self, buf=None):
        buf = self.buf if buf is None else buf
        return buf[self.inside].reshape(self.count, self.rows, self.cols)

    def outside_untouched(self, buf):
        """every float outside the matrices still has the bits it was filled with"""
        return bool(np.array_equal(buf.view(np.uint32)[~self.inside], self.buf.view(np.uint32)[~self.inside]))


def kind_of(variant):
    return {"batched": "batch3", "batched_accumulate": "batch3", "batched_bias": "batch3", "batched2": "batch4",
            "multi3": "multi3", "kseg3": "kseg3", "offset": "offset"}.get(variant, "single")


def well_conditioned(a, b, c0, bias, addend, rs0, pre):
    """A result of a few numbers can cancel: sum a*b of K uniform(-1, 1) products is typically sqrt(K) / 3 where sum |a*b| is K / 4,
    and a 1 x 1 result is now and then a hundred times smaller - its RELATIVE distance from float64 then says how unlucky the draw
    was, for any correct kernel and for numpy alike.  Over hundreds of elements the Frobenius norm averages that out; for results
    (and row sums) of fewer than 1000 numbers the values are drawn again until no output of any variant cancels worse than a
    product typically does: the magnitudes that went into it (|A| @ |B| + |bias| + ..., times |gelu'| for gelu) at most
    max(4, sqrt(K)) times the output in the Frobenius norm.  A condition on the inputs alone, in float64."""
    limit = max(4.0, a.shape[2] ** 0.5)
    norm = np.linalg.norm
    a64, b64 = a.astype(np.float64), b.astype(np.float64)
    if a.shape[0] * a.shape[1] < 1000:
        s, mag = a64.sum(axis=2), np.abs(a64).sum(axis=2)
        if norm(mag) > limit * norm(s) or norm(mag + np.abs(rs0[0])) > limit * norm(s + rs0[0]):
            return False
    if b.shape[0] * a.shape[1] * b.shape[2] < 1000:
        for x, y in ((np.maximum(a64, 0), b64), (a64, np.maximum(b64, 0))):       # relu on an operand
            if norm(np.abs(x) @ np.abs(y)) > limit * norm(x @ y):
                return False
        prod, mag = a64 @ b64, np.abs(a64) @ np.abs(b64)
        biased, mag_biased = prod + bias[:, None, :], mag + np.abs(bias)[:, None, :]
        outputs = [(prod, mag), (biased, mag_biased), (c0 + prod, mag + np.abs(c0))]
        if b.shape[0] == 1:
            outputs += [(biased + addend, mag_biased + np.abs(addend)), (gelu(biased), np.abs(gelu_grad(biased)) * mag_biased),
                        (prod * gelu_grad(pre.astype(np.float64)), mag * np.abs(gelu_grad(pre.astype(np.float64))))]
        if any(norm(m_) > limit * norm(r_) for r_, m_ in outputs):
            return False
    return True


@functools.lru_cache(maxsize=4)
def inputs(m, n, k, ta, tb, kind):
    """everything the cases on one product read, the same on every call: op(A) [nb, m, k] and op(B) [nb or 3, k, n] as stored
    (transposed where the layout says so) in NaN-guarded buffers, old C, bias, addend, old row sums, the gelu-backward's
    pre-activation"""
    rng = np.random.RandomState((1000003 * k + 1009 * m + 31 * n + 4 * ta + 2 * tb
                                 + 7 * ("single", "batch3", "batch4", "multi3", "kseg3", "offset").index(kind)) % (2 ** 31))
    pads = [PADS[i] for i in rng.randint(0, len(PADS), 6)]
    nb = {"batch3": 3, "batch4": 4}.get(kind, 1)
    nbm = 3 if kind == "multi3" else nb
    shift = 1 if kind == "offset" else 0
    gap = 37 if nb > 1 else 0                                             # batch strides larger than the matrices
    for _ in range(20000):
        a = rng.uniform(-1, 1, (nb, m, k)).astype(np.float32)
        b = rng.uniform(-1, 1, (nbm, k, n)).astype(np.float32)
        c0 = rng.uniform(-1, 1, (nbm, m, n)).astype(np.float32)
        bias = rng.uniform(-1, 1, (3 if kind == "multi3" else 1, n)).astype(np.float32)
        addend = rng.uniform(-1, 1, (1, m, n)).astype(np.float32)
        rs0 = rng.uniform(-1, 1, (1, 1, m)).astype(np.float32)
        pre = rng.uniform(-2, 2, (1, m, n)).astype(np.float32)
        if well_conditioned(a, b, c0, bias, addend, rs0, pre):
            break
    else:
        raise AssertionError("no well-conditioned values for %s" % ((m, n, k, ta, tb, kind),))
    inp = dict(a=a, b=b, nb=nb, pads=pads, A=Matrix(a.transpose(0, 2, 1) if ta else a, pads[0], shift, gap), c0=c0, bias=bias,
               addend=Matrix(addend, pads[3]), rs0=rs0, pre=Matrix(pre, pads[4]))
    stored_b = b.transpose(0, 2, 1) if tb else b
    if kind == "multi3":                                                  # three weights allocated apart
        inp["B"] = [Matrix(stored_b[i:i + 1], pads[1]) for i in range(3)]
    elif kind == "kseg3":                                                 # K through three operands allocated apart
        seg = k // 3
        inp["B"] = [Matrix(stored_b[:, i * seg:(i + 1) * seg], pads[1]) for i in range(3)]
    else:
        inp["B"] = Matrix(stored_b, pads[1], shift, gap)
    return inp


def c_buffer(case, inp):
    """the output buffer as it is before the call: PATTERN, with the old C inside for the accumulating variants (three column
    blocks of one buffer for the three products on one input)"""
    m, n, variant = case["m"], case["n"], case["variant"]
    if variant == "multi3":
        c = Matrix(np.zeros((1, m, 3 * n), np.float32), inp["pads"][2], fill=PATTERN)
    else:
        c = Matrix(np.zeros((inp["nb"], m, n), np.float32), inp["pads"][2], gap=53 if inp["nb"] > 1 else 0, fill=PATTERN)
    if "acc" in variant:
        c.put(inp["c0"])
    else:
        c.blank()
    return c


def gelu(t):
    return 0.5 * t * (1.0 + np.tanh(t * 0.7978845608 * (1.0 + 0.044715 * t * t)))


def gelu_grad(t):
    th = np.tanh(t * 0.7978845608 * (1.0 + 0.044715 * t * t))
    return 0.5 * (1.0 + th) + 0.5 * t * (1.0 - th * th) * 0.7978845608 * (1.0 + 0.134145 * t * t)


@functools.lru_cache(maxsize=24)
def _product(m, n, k, ta, tb, kind, relu_a, relu_b, dtype, mode):
    """op(A) @ op(B) of inputs(...) in `dtype`: mode "matmul" numpy's own product, "sequential" one k after the other (the
    least favourable float32 order), "abs" |op(A)| @ |op(B)|"""
    inp = inputs(m, n, k, ta, tb, kind)
    a, b = inp["a"].astype(dtype), inp["b"].astype(dtype)
    if relu_a:
        a = np.maximum(a, 0)
    if relu_b:
        b = np.maximum(b, 0)
    if mode == "abs":
        a, b = np.abs(a), np.abs(b)
    if mode == "sequential":
        prod = np.zeros((b.shape[0], m, n), dtype)
        for j in range(k):
            prod += a[:, :, j, None] * b[:, j, None, :]
        return prod
    return np.matmul(a, b)


def reference(case, dtype, mode="matmul"):
    """what the case must leave in its outputs, computed in `dtype`: {"c": [nb or 3, m, n], "rowsum": [1, 1, m], "aux": [1, m, n]}"""
    m, n, k, ta, tb, variant = (case[x] for x in ("m", "n", "k", "ta", "tb", "variant"))
    kind = kind_of(variant)
    inp = inputs(m, n, k, ta, tb, kind)
    prod = _product(m, n, k, ta, tb, kind, variant == "relu_a", variant == "relu_b", dtype, mode)
    out = {}
    if "acc" in variant:
        out["c"] = inp["c0"].astype(dtype) + prod
    elif variant in ("bias", "batched_bias", "gelu", "multi3"):
        out["c"] = prod + inp["bias"].astype(dtype)[:, None, :]
    elif variant == "addend":
        out["c"] = (prod + inp["bias"].astype(dtype)[:, None, :]) + inp["addend"].get().astype(dtype)
    elif variant == "gelu_bwd":
        out["c"] = prod * gelu_grad(inp["pre"].get().astype(dtype))
    else:
        out["c"] = prod
    if variant == "gelu":
        out["aux"] = gelu(out["c"])
    if variant.startswith("rowsum"):
        a = inp["a"].astype(dtype)
        if mode == "sequential":
            s = np.zeros((1, m), dtype)
            for j in range(k):
                s += a[:, :, j]
        else:
            s = a.sum(axis=2)
        out["rowsum"] = (inp["rs0"].astype(dtype)[0] + s if variant == "rowsum_acc" else s)[None]
    return out


def element_bounds(case):
    """per element, what ANY order of summing the K float32 products may be away from the exact result:
    (K + 8) * 2^-24 * (|A| @ |B| + |bias| + |old C or addend|) for C, (K + 2) * 2^-24 * (sum |a| + |old sum|) for the row sums.
    (K roundings of a sum of K rounded products bound the error by gamma_K * |A| @ |B|, the epilogue's one or two additions by
    2^-24 of what they add up; K + 8 leaves room for 1 / (1 - K * 2^-24).)  None for the outputs of the gelu variants: those are
    judged by the Frobenius rule and by gelu of the stored pre-activation."""
    m, n, k, ta, tb, variant = (case[x] for x in ("m", "n", "k", "ta", "tb", "variant"))
    kind = kind_of(variant)
    inp = inputs(m, n, k, ta, tb, kind)
    out = {}
    if variant != "gelu_bwd":
        mag = _product(m, n, k, ta, tb, kind, variant == "relu_a", variant == "relu_b", np.float64, "abs").copy()
        if "acc" in variant:
            mag += np.abs(inp["c0"])
        if variant in ("bias", "batched_bias", "gelu", "multi3", "addend"):
            mag += np.abs(inp["bias"])[:, None, :]
        if variant == "addend":
            mag += np.abs(inp["addend"].get())
        out["c"] = (k + 8) * U * mag
    if variant.startswith("rowsum"):
        mag = np.abs(inp["a"]).astype(np.float64).sum(axis=2)
        if variant == "rowsum_acc":
            mag += np.abs(inp["rs0"][0])
        out["rowsum"] = ((k + 2) * U * mag)[None]
    return out


def rel_frobenius(got, ref64):
    d = np.linalg.norm(got.astype(np.float64) - ref64)
    s = np.linalg.norm(ref64)
    return float(d / s) if s > 0 else float(d)


def judge(case, got, ref64=None):
    """distances of `got` ({"c", "rowsum", "aux"} like reference()) from the float64 result: {"err": relative Frobenius per
    output, "ratio": largest |got - ref| / element bound per output that has one, "nan": any NaN in a result}"""
    ref64 = reference(case, np.float64) if ref64 is None else ref64
    bounds = element_bounds(case)
    rec = {"err": {}, "ratio": {}, "nan": False}
    for key, ref in ref64.items():
        g = got[key]
        rec["nan"] = rec["nan"] or bool(np.isnan(g).any())
        rec["err"][key] = rel_frobenius(g, ref)
        if key in bounds:
            with np.errstate(divide="ignore", invalid="ignore"):
                r = np.abs(g.astype(np.float64) - ref) / bounds[key]
            r = np.where((bounds[key] == 0) & (g == ref), 0.0, r)                # 0 / 0: an exact zero where the bound is zero
            rec["ratio"][key] = float(np.nan_to_num(r, nan=np.inf).max())
    return rec


def name(case):
    return "%(child)s %(variant)s M=%(m)d N=%(n)d K=%(k)d tA=%(ta)d tB=%(tb)d" % case
