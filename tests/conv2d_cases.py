"""The conv2d sweep shared by tests/test_conv2d_cpu.py and tests/test_hip_conv2d.py: shapes, one tape, and a direct float64
reference that shares no code with either backend.

(N, C, H, W, O, KH, KW, stride, pad, bias).  K = C*KH*KW takes values that are no multiple of 8 (9, 18, 25, 297, 98), the channel
counts sit on both sides of a 32-row tile (33, 40), the position counts are no multiples of 128, inputs and windows are not all
square, strides leave inexact divisions in dx, the padding exceeds 1, one kernel is 1x1 and one stride is a pair."""
import numpy as np

CASES = [
    (1, 1, 3, 3, 1, 3, 3, 1, 0, False),
    (2, 1, 28, 28, 8, 3, 3, 1, 0, False),
    (3, 8, 13, 13, 16, 3, 3, 1, 0, True),
    (2, 3, 9, 7, 5, 3, 2, 2, 1, True),
    (2, 33, 6, 5, 33, 3, 3, 1, 1, True),
    (1, 2, 10, 11, 3, 5, 5, 3, 2, False),
    (5, 4, 8, 8, 40, 1, 1, 1, 0, True),
    (2, 2, 7, 7, 2, 7, 7, 1, 3, True),
    (4, 1, 28, 28, 8, 3, 3, 1, 1, True),
    (2, 3, 9, 7, 5, 3, 2, (2, 1), 1, True),
]
IDS = ["%dx%dx%dx%d-o%d-k%dx%d-s%s-p%d-%s" % (c[:7] + ("x".join(map(str, c[7])) if isinstance(c[7], tuple) else c[7], c[8],
                                                        "b" if c[9] else "nob")) for c in CASES]


def strides_of(stride):
    return (stride, stride) if isinstance(stride, int) else tuple(stride)


def out_shape(case):
    n, c, h, w, o, kh, kw, stride, p, _ = case
    sh, sw = strides_of(stride)
    return n, o, (h + 2 * p - kh) // sh + 1, (w + 2 * p - kw) // sw + 1


def draw(case, seed):
    """x, w, bias (or None) and the upstream gradient G, float32, uniform(-1, 1)"""
    n, c, h, w, o, kh, kw, _, _, bias = case
    rng = np.random.RandomState(seed)
    u = lambda *s: rng.uniform(-1, 1, s).astype(np.float32)      # noqa: E731
    return u(n, c, h, w), u(o, c, kh, kw), (u(1, o, 1, 1) if bias else None), u(*out_shape(case))


def run_tape(T, case, arrays, dtype=np.float32):
    """(y * G).sum().backward() on tensor class T: {"y", "dx", "dw", "db"} as numpy arrays"""
    x, w, b, g = (None if a is None else T.from_numpy(a.astype(dtype)) for a in arrays)
    g._requires_grad = False
    y = x.conv2d(w, b, stride=case[7], pad=case[8])
    (y * g).sum().backward()
    out = {"y": y.numpy(), "dx": x.grad.numpy(), "dw": w.grad.numpy()}
    if b is not None:
        out["db"] = b.grad.numpy()
    return out


def direct_float64(case, arrays):
    """the definition, tap by tap, in float64: y = sum x_padded[.., oh*sh+kh, ow*sw+kw] * w[.., kh, kw] + b and its three gradients"""
    x, w, b, g = (None if a is None else a.astype(np.float64) for a in arrays)
    n, c, h, wd, o, kh, kw, stride, p, _ = case
    sh, sw = strides_of(stride)
    _, _, oh, ow = out_shape(case)
    xp = np.zeros((n, c, h + 2 * p, wd + 2 * p))
    xp[:, :, p:p + h, p:p + wd] = x
    y, dxp, dw = np.zeros((n, o, oh, ow)), np.zeros_like(xp), np.zeros_like(w)
    for i in range(kh):
        for j in range(kw):
            win = xp[:, :, i:i + sh * oh:sh, j:j + sw * ow:sw]                     # (n, c, oh, ow)
            y += np.einsum("nchw,oc->nohw", win, w[:, :, i, j])
            dw[:, :, i, j] = np.einsum("nohw,nchw->oc", g, win)
            dxp[:, :, i:i + sh * oh:sh, j:j + sw * ow:sw] += np.einsum("nohw,oc->nchw", g, w[:, :, i, j])
    out = {"y": y, "dx": dxp[:, :, p:p + h, p:p + wd], "dw": dw}
    if b is not None:
        out["y"] = y + b
        out["db"] = g.sum(axis=(0, 2, 3)).reshape(b.shape)
    return out
