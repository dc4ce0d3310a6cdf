"""Differential fuzzing of the tape: the same randomly drawn training program on CpuTensor (numpy, pinned to the reference) and on
another backend, every observable compared.

Why: the HIP backend answers many op sequences with something other than one kernel per op - a relu that never runs (folded into
the next Linear), a skinny Linear computed together with its loss, weight and input gradients sharing a launch, gradients added by
GEMM epilogues, a lazily zeroed gradient bucket, an optimizer update inside a hipGraph or inside the backward kernels.  Each of
these peepholes is tested on the sequence it was made for; what nobody writes by hand are the sequences in between (VERDICT r3,
Weak 10).  A program here is a random walk over exactly those ingredients: Linear layers of random sizes (some skinny enough for the
head kernels, some with no bias), relu / tanh / sigmoid, residual adds, scalar multiplies, reshapes and transposed views, reads of
intermediates in the middle of a forward pass (which make lazy tensors real), in-place writes into inputs that lazy tensors still
want to read, several losses, repeated backward passes with and without zero_grad, and one of the optimizers in one of its forms.
Some programs also use a parameter twice (SHARED_KEYS: a square layer applied again, a penalty on a weight or a bias before or
after the data loss) - the case where two kernels write one parameter gradient.

    run_program(T, seed, ...) -> {label: ndarray}          # everything a user could look at, in program order
    compare(cpu, other)                                     # raises AssertionError naming the first label that differs
    cpu_runs(prog) -> CpuRuns                               # the float64 run and the float32 runs of VARIANTS, each rounding elsewhere
    judge(ref64, variants32, got, what)                     # `got` against float64, the float32 runs as the yardstick

Used by tests/test_hip_tape_fuzz.py (GPU) and tests/test_tape_fuzz_cpu.py (the generator and the judge themselves, on the CPU
backend alone)."""
import contextlib
import numpy as np
import lightgrad_amd as light


class Net(light.nn.Module):
    def __init__(self, dims, biases, norms=None):
        light.nn.Module.__init__(self)
        self.layers = light.nn.ModuleList(*[light.nn.Linear(a, b, bias=bias) for a, b, bias in zip(dims[:-1], dims[1:], biases)])
        norms = norms or [False] * (len(dims) - 1)
        self.norms = light.nn.ModuleList(*[light.nn.LayerNorm(b) if on else light.nn.Module() for b, on in zip(dims[1:], norms)])


def draw_program(seed, shared=False):
    """the random choices of one program, independent of the backend; shared=True: with the shared-parameter ingredient
    (draw_shared), otherwise its keys say "none" - the program each seed drew before that ingredient existed"""
    rng = np.random.RandomState(seed)
    deep = seed % 4 == 3                             # every fourth program is deep enough for the queued weight gradients (GradGroup)
    depth = int(rng.randint(5, 8)) if deep else int(rng.randint(1, 4))
    batch = int(rng.choice([1, 3, 8, 32, 33, 64, 200]))
    dims = [int(rng.choice([4, 8, 12, 20, 48, 64, 100]))]
    for k in range(depth):
        last = k == depth - 1
        dims.append(int(rng.choice([1, 2, 5, 10, 16]) if (last and rng.rand() < 0.6) else rng.choice([4, 8, 24, 32, 48, 96])))
    prog = {
        "batch": batch, "dims": dims, "biases": [bool(rng.rand() < 0.8) for _ in range(depth)],
        "acts": [str(rng.choice(["relu", "relu", "tanh", "sigmoid", "none"])) for _ in range(depth)],
        "residual": [bool(rng.rand() < 0.3) for _ in range(depth)],
        "scale": [float(rng.choice([1.0, 0.5, -2.0])) if rng.rand() < 0.3 else None for _ in range(depth)],
        "peek": [bool(rng.rand() < 0.25) for _ in range(depth)],           # read an intermediate mid-forward
        "poke_input": [bool(rng.rand() < 0.15) for _ in range(depth)],     # write into the input in place mid-forward
        "view_in": str(rng.choice(["plain", "plain", "reshape", "transposed"])),
        "norm": [bool(deep and rng.rand() < 0.5 and dims[k + 1] >= 4) for k in range(depth)],      # nn.LayerNorm behind the layer
        "loss": str(rng.choice(["mse", "mse", "sum", "weighted", "ce"])) if dims[-1] >= 2 else "mse",
        "optimizer": str(rng.choice(["sgd", "adam", "adabelief", "adabelief"])),
        "fused": bool(rng.rand() < 0.6), "device_step": bool(rng.rand() < 0.5),
        "steps": int(rng.randint(1, 4)),
        "zero_grad": str(rng.choice(["before_backward", "before_backward", "after_step", "never"])),
        "second_backward": bool(rng.rand() < 0.25),                        # two backward passes over two forward passes, gradients add up
        "x_requires_grad": bool(rng.rand() < 0.7),
        "seed": int(seed),
    }
    if prog["norm"][-1] and prog["loss"] == "sum":
        # the sum over a freshly normalised row is 0 in exact arithmetic: the loss and every gradient behind it would be rounding
        # noise (which AdaBelief then normalises into steps of size lr) - nothing two correct backends have to agree on
        prog["loss"] = "weighted"
    prog.update(draw_shared(seed, prog) if shared else {"reuse": None, "penalty": None})
    return prog


SHARED_KEYS = ("reuse", "penalty")


def draw_shared(seed, prog):
    """the shared-parameter ingredient, drawn from a stream of its own: the keys above are what every seed drew before it existed.
      reuse    index k of a square layer applied a second time right behind itself (with its activation, tanh if it has
               none: two products in a row stay bounded), or None
      penalty  None or (target, layer, coefficient, place): coefficient * sum(p * p) of layer k's "weight" or "bias", added
               "before" or "after" the data loss in the expression"""
    rng = np.random.RandomState(7919 * seed + 104729)
    dims, depth = prog["dims"], len(prog["dims"]) - 1
    square = [k for k in range(depth) if dims[k] == dims[k + 1]]
    reuse = int(rng.choice(square)) if square and rng.rand() < 0.6 else None
    penalty = None
    if rng.rand() < 0.5:
        k = int(rng.randint(depth))
        target = "bias" if prog["biases"][k] and rng.rand() < 0.4 else "weight"
        penalty = (target, k, float(rng.choice([0.01, 0.05])), str(rng.choice(["before", "after"])))
    return {"reuse": reuse, "penalty": penalty}


def run_program(T, prog, dtype=np.float32, prepare=None):
    """run `prog` on tensor class T; returns the ordered list of (label, array) of everything observable.
    prepare(model, optimizer_factory) -> optimizer lets a backend test choose an optimizer form (flat buckets, ...)"""
    rng = np.random.RandomState(1000 + prog["seed"])
    batch, dims = prog["batch"], prog["dims"]
    np.random.seed(prog["seed"])                     # nn.Linear draws its weights from numpy's global stream
    model = Net(dims, prog["biases"], prog["norm"])
    w0 = [(n, p.numpy().astype(dtype)) for n, p in model.named_parameters()]
    model.load_parameters(w0)
    if T is not light.CpuTensor:
        model.map_parameters(lambda p: getattr(p, T.__module__.split(".")[-2])())        # p.hip()
    x_np = rng.uniform(-1, 1, (batch, dims[0])).astype(dtype)
    target_np = rng.uniform(-1, 1, (batch, dims[-1])).astype(dtype)
    w_np = rng.uniform(-1, 1, (batch, dims[-1])).astype(dtype)
    poke_np = rng.uniform(-1, 1, (batch, dims[0])).astype(dtype)
    labels_np = rng.randint(0, dims[-1], batch).astype(np.int64)

    def make_opt(params):
        kind = prog["optimizer"]
        if kind == "sgd":
            return light.optim.SGD(params, lr=1e-2, momentum=0.9)
        cls = light.optim.Adam if kind == "adam" else light.optim.AdaBelief
        kw = {}
        if T is not light.CpuTensor:
            kw = {"fused": prog["fused"], "device_step": prog["fused"] and prog["device_step"]}
        return cls(params, lr=1e-2, eps=1e-3, **kw)
    opt = prepare(model, make_opt) if prepare is not None else make_opt(model.parameters())
    out = []

    def see(label, t):
        out.append((label, np.array(t.numpy(), dtype=np.float64)))

    def forward(tag):
        if prog["view_in"] == "transposed":
            x = T.from_numpy(np.ascontiguousarray(x_np.T), requires_grad=prog["x_requires_grad"])
            h = x.transpose(1, 0)
        else:
            x = T.from_numpy(x_np.copy(), requires_grad=prog["x_requires_grad"])
            h = x.reshape(-1, dims[0]) if prog["view_in"] == "reshape" else x
        h_in = h
        for k, layer in enumerate(model.layers):
            prev = h
            h = layer(h)
            act = prog["acts"][k]
            if act != "none":
                h = getattr(h, act)()
            if prog["reuse"] == k:                       # the same weights once more: two writers of one gradient
                h = getattr(layer(h), act if act != "none" else "tanh")()
            if prog["norm"][k]:
                h = model.norms[k](h)
            if prog["residual"][k] and prev.shape == h.shape:
                h = h + prev
            if prog["scale"][k] is not None:
                h = h * prog["scale"][k]
            if prog["peek"][k]:
                see("%s/h%d" % (tag, k), h)
            if prog["poke_input"][k] and prog["view_in"] == "plain":
                with light.no_grad():                # a later write into the input must not show in anything computed before it
                    x[...] = T.from_numpy(poke_np, requires_grad=False)
        return x, h_in, h

    def data_loss(h):
        if prog["loss"] == "mse":
            return light.loss.mse(h, T.from_numpy(target_np, requires_grad=False))
        if prog["loss"] == "sum":
            return h.sum()
        if prog["loss"] == "ce":
            return light.loss.cross_entropy(h, T.from_numpy(labels_np, requires_grad=False))
        return (h * T.from_numpy(w_np, requires_grad=False)).sum()

    def loss_of(h):
        if prog["penalty"] is None:
            return data_loss(h)
        target, k, coef, place = prog["penalty"]
        p = getattr(model.layers[k], target)
        if place == "before":
            pen = (p * p).sum() * coef
            return pen + data_loss(h)
        loss = data_loss(h)
        return loss + (p * p).sum() * coef

    for step in range(prog["steps"]):
        tag = "s%d" % step
        x, h_in, h = forward(tag)
        loss = loss_of(h)
        if prog["zero_grad"] == "before_backward":
            opt.zero_grad()
        loss.backward()
        if prog["second_backward"]:
            x2, _, h2 = forward(tag + "b")
            loss_of(h2).backward()                   # parameter gradients accumulate over the two passes
        see(tag + "/loss", loss)
        see(tag + "/out", h)
        for n, p in model.named_parameters():
            if p.grad is not None:
                see("%s/grad/%s" % (tag, n), p.grad)
        if prog["x_requires_grad"] and x.grad is not None:
            see(tag + "/grad/x", x.grad)
        opt.step()
        if prog["zero_grad"] == "after_step":
            opt.zero_grad()
        for n, p in model.named_parameters():
            see("%s/param/%s" % (tag, n), p)
    return out


def compare(ref, got, rtol=2e-4, atol=2e-5, what=""):
    assert [l for l, _ in ref] == [l for l, _ in got], "%s: the two runs looked at different things:\n%s\n%s" % (what, [l for l, _ in ref], [l for l, _ in got])
    for (label, a), (_, b) in zip(ref, got):
        assert a.shape == b.shape, "%s %s: shape %s vs %s" % (what, label, a.shape, b.shape)
        scale = max(1.0, float(np.abs(a).max()) if a.size else 1.0)
        if not np.allclose(a, b, rtol=rtol, atol=atol * scale, equal_nan=True):
            bad = np.abs(a - b) > atol * scale + rtol * np.abs(a)
            raise AssertionError("%s %s: %d of %d values differ, max |diff| %.3g at scale %.3g" % (what, label, int(bad.sum()), a.size, float(np.abs(a - b).max()), scale))


# ---- the float64 yardstick ---------------------------------------------------------------------------------------------------
# A program is judged by its distance to a float64 run of the same tape code.  How far a correct float32 evaluation may be from
# that is the program's own property (a cancelling gradient behind a LayerNorm amplifies one rounding a thousandfold), so it is
# measured, and with more than one sample: the CPU backend run once per entry of VARIANTS - the matrix products summed in five
# orders (here), then the other ops evaluated the way the HIP backend evaluates them (further down).  Each is a correct float32
# evaluation of the program; the furthest of them is the yardstick.
FLOOR, FACTOR, LEFT_OUT_CAP = 1e-5, 2, 0.10        # the rule of common.assert_as_close_to_float64_as_the_cpu_backend; the cap on programs left out
CLASSES = ("loss", "out", "peek", "grad", "param")


def _blas(a, b):
    return a @ b


def _wide(a, b):
    return (a.astype(np.float64) @ b.astype(np.float64)).astype(np.float32)


def _chunk7(a, b):
    acc = np.zeros((a.shape[0], b.shape[1]), np.float32)
    for k in range(0, a.shape[1], 7):
        acc = acc + a[:, k:k + 7] @ b[k:k + 7]
    return acc


def _chunk16r(a, b):
    acc = None
    for k in reversed(range(0, a.shape[1], 16)):
        part = a[:, k:k + 16] @ b[k:k + 16]
        acc = part if acc is None else acc + part
    return a @ b if acc is None else acc


def _lanes4(a, b):
    """the order of the skinny-head kernels (csrc/head.hip): lane l of 64 owns k = 4 l .. 4 l + 3 (+ 256 c) and forms its part as
    one chain of fused multiply-adds, then the lanes fold in halves.  A fused multiply-add of float32 operands is exact in float64
    up to the one rounding."""
    (m, k), n = a.shape, b.shape[1]
    lanes = 1
    while lanes < 64 and 4 * lanes < k:              # the lanes above these hold zeros, and adding them changes nothing
        lanes *= 2
    pad = (-k) % (4 * lanes)
    a64 = np.concatenate([a, np.zeros((m, pad), np.float32)], axis=1).astype(np.float64).reshape(m, -1, lanes, 4)
    b64 = np.concatenate([b, np.zeros((pad, n), np.float32)], axis=0).astype(np.float64).reshape(-1, lanes, 4, n)
    acc = np.zeros((m, lanes, n), np.float32)
    for c in range(a64.shape[1]):
        for j in range(4):
            acc = (a64[:, c, :, j, None] * b64[None, c, :, j, :] + acc).astype(np.float32)
    width = lanes // 2
    while width:
        acc = acc[:, :width] + acc[:, width:2 * width]
        width //= 2
    return acc[:, 0]


PRODUCTS = {"blas": _blas, "wide": _wide, "chunk7": _chunk7, "chunk16r": _chunk16r, "lanes4": _lanes4}


def scaled_product(factor):
    """a subtly wrong product: `blas` times `factor` (tests/test_tape_fuzz_cpu.py shows that the judge notices it)"""
    factor = np.float32(factor)
    return lambda a, b: (a @ b) * factor


@contextlib.contextmanager
def product_order(name):
    """for its duration, CpuTensor's `dot` forms the products of 2-D float32 operands, forward and backward, by
    PRODUCTS[name] (or by `name` itself, a function of two matrices); everything else, float64 included, stays `a @ b`"""
    from lightgrad_amd.autograd.cpu import ops as cpu_ops
    product = PRODUCTS[name] if isinstance(name, str) else name
    inner = cpu_ops.dot.__mro__[1]                   # the class written on ndarrays; the registered op unwraps tensors around it

    def mul(a, b):
        if a.ndim == 2 and b.ndim == 2 and a.dtype == np.float32 and b.dtype == np.float32:
            return product(a, b)
        return a @ b

    def forward(ctx, a, b):
        ctx.save_for_backward(a, b)
        return mul(a, b)

    def backward(ctx, out_grad):
        a, b = ctx.get_saved_tensors()
        return mul(out_grad, np.swapaxes(b, -1, -2)), mul(np.swapaxes(a, -1, -2), out_grad)
    saved = inner.forward, inner.backward
    inner.forward, inner.backward = forward, backward
    try:
        yield
    finally:
        inner.forward, inner.backward = saved


def observable_class(label):
    tail = label.split("/", 1)[1]
    return "grad" if tail.startswith("grad/") else "param" if tail.startswith("param/") else tail if tail in ("loss", "out") else "peek"


def _norm(a):
    return float(np.linalg.norm(np.asarray(a, np.float64)))


def _distance(r, a):
    """of one observable `a` to its float64 value r: common.rel_frobenius, or the norm of `a` where r is exactly zero (no
    relative distance to that); nan if either holds a value that is not finite"""
    from common import rel_frobenius
    if not (np.isfinite(r).all() and np.isfinite(a).all()):
        return float("nan")
    return _norm(a) if _norm(r) == 0.0 else rel_frobenius(a, r)


def _accepts(r, e_got, yards):
    """the rule of judge() for one observable, from the distances: (accepted, yard)"""
    if not yards or not np.isfinite([e_got] + list(yards)).all():
        return False, float("nan")
    yard = max(yards)
    if _norm(r) == 0.0:
        return (e_got == 0.0 if yard == 0.0 else e_got <= FACTOR * yard), yard
    return e_got <= max(FLOOR, FACTOR * yard), yard


def distances(ref64, run):
    return [_distance(r, a) for (_, r), (_, a) in zip(ref64, run)]


def _same_observables(runs, what):
    names = [l for l, _ in runs[0]]
    for run in runs[1:]:
        assert names == [l for l, _ in run], "%s: the runs looked at different things:\n%s\n%s" % (what, names, [l for l, _ in run])
    for row in zip(*runs):
        assert len({a.shape for _, a in row}) == 1, "%s %s: shapes %s" % (what, row[0][0], [a.shape for _, a in row])
    return names


def judge(ref64, variants32, got, what, tally=None, known=None):
    """`got` against the float64 run `ref64`, with the float32 CPU runs `variants32` ({name: run}) as the yardstick.  For every
    observable: same labels and shapes in all runs, every value finite, and, with e = common.rel_frobenius to ref64 and
    yard = the largest e of the variants, e_got <= max(1e-5, 2 * yard); where ref64 is exactly zero, got exactly zero if every
    variant is, otherwise ||got|| <= 2 * the largest variant norm.  Raises AssertionError naming `what` (the seed and the
    program), the label and every distance; returns {class: worst (e_got, yard)} over the observables with a nonzero reference.
    tally: a dict that counts "observables" and "at_floor" (those judged at 1e-5, the yardstick being below it)
    known: {name: distances(ref64, variants32[name])} where the caller has them already (CpuRuns.apart)"""
    names = list(variants32)
    labels = _same_observables([ref64] + [variants32[n] for n in names] + [got], what)
    known = known or {}
    apart = {n: known[n] if n in known else distances(ref64, variants32[n]) for n in names}
    worst = {}
    for i, (label, e_got) in enumerate(zip(labels, distances(ref64, got))):
        r, g = ref64[i][1], got[i][1]
        ok, yard = _accepts(r, e_got, [apart[n][i] for n in names])
        zero = _norm(r) == 0.0
        if not ok:
            each = ", ".join("%s %.3g" % (n, apart[n][i]) for n in names)
            off = float(np.abs(g - variants32["blas"][i][1]).max()) if "blas" in variants32 and g.size else float("nan")
            raise AssertionError("%s\n%s: got %.3g %s, the float32 CPU runs: %s; max |got - blas| %.3g" % (
                what, label, e_got, "in norm where the float64 run is exactly 0" if zero else "from the float64 run (relative Frobenius)", each, off))
        if tally is not None:
            tally["observables"] = tally.get("observables", 0) + 1
            tally["at_floor"] = tally.get("at_floor", 0) + (not zero and FACTOR * yard <= FLOOR)
        if not zero:
            merge_worst(worst, {observable_class(label): (e_got, yard)})
    return worst


def merge_worst(total, worst):
    for kind, (e_got, yard) in worst.items():
        have = total.get(kind, (0.0, 0.0))
        total[kind] = (max(have[0], e_got), max(have[1], yard))
    return total


def worst_lines(name, worst, drawn=None, left_out=()):
    """what a test prints: one line per class with the worst (e_got, yard)"""
    head = [] if drawn is None else ["%s: %d programs drawn, left out %s" % (name, drawn, list(left_out))]
    return "\n".join(head + ["%s: %-5s worst e_got %.3g  worst yard %.3g" % ((name, k) + worst[k]) for k in CLASSES if k in worst])


# ---- float32 variants of the ops that are no product -----------------------------------------------------------------------------
# The HIP backend differs from the CPU backend in more than the order of its products, each difference a correct float32
# evaluation of the same op: its exp and tanh come from another libm, its sums are tree sums over the 64 lanes of a wave, and a
# LayerNorm is one kernel with a closed-form backward where the CPU backend differentiates the composite.  Where a program
# amplifies one of these (a LayerNorm over the five nearly equal outputs of a sigmoid turns a last-place difference into 1e-5)
# the product orders say nothing: with K <= 7 they are one sample.  So each difference is a variant of its own, made on the CPU
# backend the same way - patched for the duration of a run, the products left as `blas` - and one variant has them all at once.
# profiles/tape_fuzz_yardstick.md: the program that showed each, and what the variant moves there.
@contextlib.contextmanager
def _patched(cls, **attrs):
    saved = {k: getattr(cls, k) for k in attrs}
    for k, v in attrs.items():
        setattr(cls, k, v)
    try:
        yield
    finally:
        for k, v in saved.items():
            setattr(cls, k, v)


@contextlib.contextmanager
def activations_rounded_once():
    """sigmoid, tanh and exp of float32 operands evaluated in float64 and rounded once: another libm's last place"""
    from lightgrad_amd.autograd.cpu import ops as cpu_ops
    with contextlib.ExitStack() as stack:
        for name, f in (("sigmoid", lambda t: 1 / (1 + np.exp(-t))), ("tanh", np.tanh), ("exp", np.exp)):
            def forward(ctx, t, f=f):
                y = f(t.astype(np.float64)).astype(np.float32) if t.dtype == np.float32 else f(t)
                ctx.save_for_backward(y)             # all three keep their output for the backward
                return y
            stack.enter_context(_patched(getattr(cpu_ops, name).__mro__[1], forward=forward))
        yield


def _sum_over_lanes(t, axis, keepdims):
    """a float32 sum in the order of a wave: 64 lanes take the reduced elements in turn and add theirs up one after the other,
    then the lanes fold in halves"""
    nd = t.ndim
    axes = tuple(range(nd)) if axis is None else tuple(a % nd for a in (axis if isinstance(axis, tuple) else (axis,)))
    kept = [a for a in range(nd) if a not in axes]
    m = np.transpose(t, kept + list(axes)).reshape([t.shape[a] for a in kept] + [-1])
    m = np.concatenate([m, np.zeros(m.shape[:-1] + ((-m.shape[-1]) % 64,), np.float32)], axis=-1).reshape(m.shape[:-1] + (-1, 64))
    acc = np.zeros(m.shape[:-2] + (64,), np.float32)
    for k in range(m.shape[-2]):
        acc = acc + m[..., k, :]
    width = 32
    while width:
        acc = acc[..., :width] + acc[..., width:2 * width]
        width //= 2
    out = acc[..., 0]
    return np.asarray(out.reshape([1 if a in axes else t.shape[a] for a in range(nd)]) if keepdims else out)


def _sum_left_to_right(t, axis, keepdims):
    nd = t.ndim
    axes = tuple(range(nd)) if axis is None else tuple(a % nd for a in (axis if isinstance(axis, tuple) else (axis,)))
    kept = [a for a in range(nd) if a not in axes]
    m = np.transpose(t, kept + list(axes)).reshape([t.shape[a] for a in kept] + [-1])
    out = np.cumsum(m, axis=-1, dtype=np.float32)[..., -1]
    return np.asarray(out.reshape([1 if a in axes else t.shape[a] for a in range(nd)]) if keepdims else out)


@contextlib.contextmanager
def _sums_by(order):
    from lightgrad_amd.autograd.cpu import ops as cpu_ops
    inner = cpu_ops.sum.__mro__[1]

    def forward(ctx, t, axis=None, keepdims=False):
        ctx.save_for_backward(t.shape, axis, keepdims)
        if t.dtype != np.float32 or t.size == 0:
            return np.asarray(t.sum(axis=axis, keepdims=keepdims))
        return order(t, axis, keepdims)
    with _patched(inner, forward=forward):
        yield


def sums_over_lanes():
    return _sums_by(_sum_over_lanes)


def sums_left_to_right():
    """numpy adds pairwise, a wave over its lanes; the plain loop is the third order a float32 sum is met in"""
    return _sums_by(_sum_left_to_right)


class _layer_norm_rows(light.autograd.func.Function):
    """LayerNorm over the last axis as one op on ndarrays, the way csrc/rowwise.hip evaluates it: xhat = (x - mean) * rstd kept
    for the backward, dx = rstd * (gw - mean(gw) - xhat * mean(gw * xhat)) with gw = g * w, parameter gradients summed over rows"""

    def forward(ctx, x, w, b, eps=1e-5):
        one_nth = x.dtype.type(1.0) / x.dtype.type(x.shape[-1])
        d = x - _row_sums(x) * one_nth
        rstd = x.dtype.type(1.0) / np.sqrt(_row_sums(d * d) * one_nth + x.dtype.type(eps))
        xhat = d * rstd
        ctx.save_for_backward(xhat, rstd, w)
        return xhat * w + b

    def backward(ctx, g):
        xhat, rstd, w = ctx.get_saved_tensors()
        one_nth = g.dtype.type(1.0) / g.dtype.type(g.shape[-1])
        gw = g * w
        dx = rstd * (gw - _row_sums(gw) * one_nth - xhat * (_row_sums(gw * xhat) * one_nth))
        return dx, (g * xhat).reshape(-1, g.shape[-1]).sum(0), g.reshape(-1, g.shape[-1]).sum(0)


def _row_sums(t):
    """the sums of a row-wise kernel: one wave per row"""
    return _sum_over_lanes(t, -1, True) if t.dtype == np.float32 else t.sum(-1, keepdims=True)


@contextlib.contextmanager
def layer_norm_as_one_op():
    from lightgrad_amd.autograd.cpu import ops as cpu_ops
    op = cpu_ops._numpy_op(_layer_norm_rows)
    composite = light.nn.LayerNorm.forward

    def forward(self, x):
        if isinstance(x, light.CpuTensor) and len(self.shape) == 1 and x.dtype == np.float32:
            return op(x, self.weight, self.bias, eps=self.eps)
        return composite(self, x)
    with _patched(light.nn.LayerNorm, forward=forward):
        yield


# name: (product order, what else is patched)
VARIANT_TABLE = {"blas": ("blas", ()), "wide": ("wide", ()), "chunk7": ("chunk7", ()), "chunk16r": ("chunk16r", ()), "lanes4": ("lanes4", ()),
                 "libm": ("blas", (activations_rounded_once,)), "lanes": ("blas", (sums_over_lanes,)),
                 "sequence": ("blas", (sums_left_to_right,)), "rowwise": ("blas", (layer_norm_as_one_op,)),
                 # every difference at once, as the HIP backend has them
                 "together": ("lanes4", (activations_rounded_once, sums_over_lanes, layer_norm_as_one_op))}
VARIANTS = tuple(VARIANT_TABLE)


@contextlib.contextmanager
def variant(name):
    product, others = VARIANT_TABLE[name]
    with contextlib.ExitStack() as stack:
        stack.enter_context(product_order(product))
        for other in others:
            stack.enter_context(other())
        yield


class CpuRuns(object):
    """the CPU side of one program: ref64, variants ({name: float32 run}), apart ({name: distances to ref64}) and refused - the (variant, label) pairs that the
    rule of judge() refuses with the other variants as the yardstick.  kept = nothing refused: where correct float32
    evaluations cannot vouch for each other, the program says nothing about a fifth one."""

    def __init__(self, prog):
        from common import float64_tape
        with float64_tape():
            self.ref64 = run_program(light.CpuTensor, prog, dtype=np.float64)
        self.variants = {}
        for name in VARIANTS:
            with variant(name):                      # kept as float32, which they are: the cache holds some hundred programs
                self.variants[name] = [(l, a.astype(np.float32)) for l, a in run_program(light.CpuTensor, prog)]
        labels = _same_observables([self.ref64] + list(self.variants.values()), "seed %d" % prog["seed"])
        self.apart = {name: distances(self.ref64, run) for name, run in self.variants.items()}
        self.refused = []
        for i, label in enumerate(labels):
            for name in VARIANTS:
                if not _accepts(self.ref64[i][1], self.apart[name][i], [self.apart[n][i] for n in VARIANTS if n != name])[0]:
                    self.refused.append((name, label))
        self.kept = not self.refused
        self.dead = all(_norm(a) == 0.0 for l, a in self.ref64 if observable_class(l) == "out")


_CPU_RUNS = {}


def cpu_runs(prog):
    """CpuRuns(prog), once per program: the seed ranges of the tests overlap.  The CPU backend has one form of each optimizer, so
    the keys that choose a HIP form are not part of the key."""
    key = repr(sorted((k, v) for k, v in prog.items() if k not in ("fused", "device_step")))
    if key not in _CPU_RUNS:
        _CPU_RUNS[key] = CpuRuns(prog)
    return _CPU_RUNS[key]


def within_the_cap(left_out, drawn):
    return len(left_out) <= LEFT_OUT_CAP * drawn


# ---- the programs of the GPU tests (tests/test_hip_tape_fuzz.py), here so that tests/test_tape_fuzz_cpu.py checks the same ones ----
def shared_programs(first, count):
    for seed in range(first, first + count):
        prog = draw_program(seed, shared=True)
        if prog["reuse"] is not None or prog["penalty"] is not None:
            yield seed, prog


def flat_programs(programs, in_backward=False):
    """the programs an optimizer over flat buckets takes (no SGD), in their fused form; in_backward: those that the update inside
    the backward kernels accepts by contract (one backward pass per step, zero_grad before it)"""
    for seed, prog in programs:
        if prog["optimizer"] == "sgd":
            continue
        if in_backward and (prog["second_backward"] or prog["zero_grad"] != "before_backward"):
            continue
        yield seed, dict(prog, fused=True, device_step=True)


def plain_programs(first, count):
    return [(seed, draw_program(seed)) for seed in range(first, first + count)]


def gpu_test_programs():
    sets = {"plain/block%d" % b: plain_programs(b * 25, 25) for b in range(8)}
    sets["peepholes_off"] = plain_programs(0, 100)
    sets["flat_buckets"] = list(flat_programs(plain_programs(300, 80)))
    sets["update_in_backward"] = list(flat_programs(plain_programs(300, 80), in_backward=True))
    sets["shared"] = list(shared_programs(700, 60))
    sets["shared/flat_buckets"] = list(flat_programs(shared_programs(850, 100)))
    sets["shared/update_in_backward"] = list(flat_programs(shared_programs(900, 200), in_backward=True))
    return sets
