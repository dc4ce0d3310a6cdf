"""The batch-norm sweep shared by tests/test_batchnorm_cpu.py and tests/test_hip_batchnorm.py: shapes, one tape, and a direct numpy
reference in any float dtype that shares no code with either backend.

A case is (shape, affine).  The shapes are the smallest that reach every path of csrc/batchnorm.hip: two values per channel; an odd
L without 16-byte alignment; L == 1 (lanes across channels) with C no multiple of 64, as 4-D and as 2-D; a 3-D input; per form one
shape with several slices per channel and a ragged last one (the plan rule of lg_batchnorm_*: form 0 takes ceil(units / 1024)
slices while that is below 1024 / C, form 1 floor(N / 16) slices per block of 64 channels); the example's layout at a small batch
(float4 units: 676 = 4 * 169); and one shape without weight and bias."""
import numpy as np

CASES = [
    ((2, 1, 1, 1), True),
    ((4, 3, 5, 7), True),
    ((3, 5, 1, 1), True),
    ((33, 70), True),
    ((5, 4, 9), True),
    ((6, 3, 37, 41), True),          # form 0, scalar units: 9102 per channel -> 9 slices of 1012, the last one 1006
    ((7, 2, 25, 52), True),          # form 0, float4 units: 7 * 325 = 2275 per channel -> 3 slices of 759, the last one 757
    ((100, 70), True),               # form 1: 6 slices of 17 rows, the last one 15
    ((64, 8, 26, 26), True),
    ((4, 3, 5, 7), False),
    ((36, 8), False),                # form 1 with float4 apply / dx (C a multiple of 4), 2 slices of 18 rows
]
IDS = ["x".join(map(str, s)) + ("" if affine else "-plain") for s, affine in CASES]
MULTI_SLICE = [5, 6, 7]              # indices of the cases above whose statistics launch folds several slices


def expected_slices(shape, vec):
    """the plan rule of lg_batchnorm_fwd_f32 / bwd: a function of the shape and of whether 16-byte units are used (vec 4 or 1)"""
    n, c = shape[:2]
    length = int(np.prod(shape[2:], dtype=np.int64))
    if length == 1:
        slices = max(1, min(64, -(-1024 // -(-c // 64)), n // 16))
        chunk = -(-n // slices)
        return -(-n // chunk)
    units = n * (length // vec)
    slices = max(1, min(256, -(-1024 // c), -(-units // 1024)))
    chunk = -(-units // slices)
    return -(-units // chunk)


def draw(case, seed, offset=0.0):
    """x, weight, bias (or None, None) and the upstream gradient G as float32: standard normal values (+ offset for x), weights
    around 1"""
    shape, affine = case
    rng = np.random.RandomState(seed)
    c = shape[1]
    x = (rng.standard_normal(shape) + offset).astype(np.float32)
    w = (1 + 0.5 * rng.uniform(-1, 1, c)).astype(np.float32) if affine else None
    b = rng.uniform(-1, 1, c).astype(np.float32) if affine else None
    return x, w, b, rng.uniform(-1, 1, shape).astype(np.float32)


def run_tape(T, arrays, dtype=np.float32, calls=2, momentum=0.1, eps=1e-5, x_of=None):
    """`calls` training-mode calls on tensor class T with the running tensors starting at zeros / ones, (y * G).sum().backward() on
    the last: {"y", "dx", "dw", "db", "running_mean", "running_var", "save_mean", "save_rstd"} as numpy arrays.  `x_of(tensor)`
    turns the dense input leaf into what the op receives (a view, a lazy relu)."""
    xa, wa, ba, ga = arrays
    leaf = T.from_numpy(xa.astype(dtype))
    w, b = (None if a is None else T.from_numpy(a.astype(dtype)) for a in (wa, ba))
    g = T.from_numpy(ga.astype(dtype), requires_grad=False)
    c = xa.shape[1]
    rm, rv = T.from_numpy(np.zeros(c, dtype), requires_grad=False), T.from_numpy(np.ones(c, dtype), requires_grad=False)
    for _ in range(calls):
        x = leaf if x_of is None else x_of(leaf)
        y = x.batch_norm(w, b, rm, rv, momentum=momentum, eps=eps)
    (y * g).sum().backward()
    out = {"y": y.numpy(), "dx": leaf.grad.numpy(), "running_mean": rm.numpy(), "running_var": rv.numpy()}
    if w is not None:
        out["dw"], out["db"] = w.grad.numpy(), b.grad.numpy()
    saved = y.ctx.get_saved_tensors()
    if len(saved) >= 4:                                             # the kernel node: (x, weight, save_mean, save_rstd, geometry)
        out["save_mean"], out["save_rstd"] = saved[2].numpy(), saved[3].numpy()
    return out


def direct(arrays, dtype=np.float64, calls=2, momentum=0.1, eps=1e-5, relu=False):
    """the definition in numpy arithmetic of `dtype`, two passes: everything run_tape returns, and save_mean / save_rstd.  `relu`:
    the op's input is max(x, 0) and dx is the gradient with respect to x"""
    xa, wa, ba, ga = arrays
    leaf, g = xa.astype(dtype), ga.astype(dtype)
    x = np.maximum(leaf, 0) if relu else leaf
    c = x.shape[1]
    axes = (0,) + tuple(range(2, x.ndim))
    pshape = (1, c) + (1,) * (x.ndim - 2)
    w = np.ones(c, dtype) if wa is None else wa.astype(dtype)
    b = np.zeros(c, dtype) if ba is None else ba.astype(dtype)
    count = x.size // c
    mean = x.mean(axis=axes, keepdims=True, dtype=dtype)
    var = np.mean((x - mean) ** 2, axis=axes, keepdims=True, dtype=dtype)
    rstd = 1 / np.sqrt(var + dtype(eps))
    xhat = (x - mean) * rstd
    rm, rv = np.zeros(c, dtype), np.ones(c, dtype)
    for _ in range(calls):
        rm = dtype(1 - momentum) * rm + dtype(momentum) * mean.reshape(-1)
        rv = dtype(1 - momentum) * rv + dtype(momentum) * var.reshape(-1) * dtype(count / (count - 1))
    dw, db = (g * xhat).sum(axis=axes, dtype=dtype), g.sum(axis=axes, dtype=dtype)
    dx = w.reshape(pshape) * rstd * (g - db.reshape(pshape) / count - xhat * dw.reshape(pshape) / count)
    if relu:
        dx = dx * (leaf >= 0)
    out = {"y": xhat * w.reshape(pshape) + b.reshape(pshape), "dx": dx, "running_mean": rm, "running_var": rv,
           "save_mean": mean.reshape(-1), "save_rstd": rstd.reshape(-1)}
    if wa is not None:
        out["dw"], out["db"] = dw, db
    return {k: v.astype(dtype) for k, v in out.items()}


def direct_infer(arrays, running_mean, running_var, dtype=np.float64, eps=1e-5):
    """the evaluation form and its three gradients in numpy arithmetic of `dtype`"""
    xa, wa, ba, ga = arrays
    x, g = xa.astype(dtype), ga.astype(dtype)
    c = x.shape[1]
    axes = (0,) + tuple(range(2, x.ndim))
    pshape = (1, c) + (1,) * (x.ndim - 2)
    w = np.ones(c, dtype) if wa is None else wa.astype(dtype)
    b = np.zeros(c, dtype) if ba is None else ba.astype(dtype)
    rstd = 1 / np.sqrt(running_var.astype(dtype) + dtype(eps))
    xhat = (x - running_mean.astype(dtype).reshape(pshape)) * rstd.reshape(pshape)
    out = {"y": xhat * w.reshape(pshape) + b.reshape(pshape), "dx": g * (w * rstd).reshape(pshape)}
    if wa is not None:
        out["dw"], out["db"] = (g * xhat).sum(axis=axes, dtype=dtype), g.sum(axis=axes, dtype=dtype)
    return out


def run_infer_tape(T, arrays, running_mean, running_var, dtype=np.float32, eps=1e-5):
    xa, wa, ba, ga = arrays
    x = T.from_numpy(xa.astype(dtype))
    w, b = (None if a is None else T.from_numpy(a.astype(dtype)) for a in (wa, ba))
    rm, rv = (T.from_numpy(a.astype(dtype), requires_grad=False) for a in (running_mean, running_var))
    y = x.batch_norm_infer(w, b, rm, rv, eps=eps)
    (y * T.from_numpy(ga.astype(dtype), requires_grad=False)).sum().backward()
    out = {"y": y.numpy(), "dx": x.grad.numpy()}
    if w is not None:
        out["dw"], out["db"] = w.grad.numpy(), b.grad.numpy()
    assert rm.grad is None and rv.grad is None
    np.testing.assert_array_equal(rm.numpy(), running_mean.astype(dtype))
    np.testing.assert_array_equal(rv.numpy(), running_var.astype(dtype))
    return out
