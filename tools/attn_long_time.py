"""Time attention forward + backward beyond 128 positions: the node `self_attention` with the long launches
(csrc/attention_long.hip) against the composite tape that these lengths took before, at (8, 256, 2 heads, d = 64) and
(8, 512, 2, 64), with and without a key-padding mask:

    python tools/attn_long_time.py [--rounds 3] [--iters 300] [--out profiles/attention_long.txt]
    python tools/attn_long_time.py --dropout 0.1 --out profiles/attention_dropout.txt

With --dropout p both routes drop the probabilities with probability p - the fused node inside its two attention launches
(dropout=p), the composite with `probs.dropout(p)` between the softmax and the context product, the path such a model took before the
kernels drew masks - at tiny-BERT's shape (8, 128, 2 heads, d = 64: 16 (batch, head) pairs) and at (8, 512, 2, 64), without a mask.

Both routes start from the same (b, s, hidden) input and the same three projection weights, like BertSelfAttention.forward: the
fused route is the one node, the composite route three nn.Linear products, the head split by strides, the scores GEMM, divide,
mask, softmax, the context GEMM and their backward.  Every figure is device time per forward + backward by HIP events around
`--iters` steps after 20 warm-up steps, both issued eagerly from the tape (host time included where the host is slower than the
device) and replayed from a captured graph (device time alone).  Without a GPU this fails; nothing here falls back."""
import argparse
import ctypes
import math
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def measure(route, b, s, heads, d, masked, iters, dropout=0.0):
    """{"eager_us", "graph_us"} of one forward + backward of `route` ("fused" or "composite")"""
    import numpy as np
    from lightgrad_amd import HipTensor
    from lightgrad_amd.autograd.hip import HipGraph, HipDevice
    from lightgrad_amd.autograd.hip import lib as L
    lib = L.lib()
    rng = np.random.RandomState(0)
    width = hidden = heads * d
    x = HipTensor.from_numpy(rng.uniform(-1, 1, (b, s, hidden)).astype(np.float32))
    params = []
    for _ in range(3):
        params += [HipTensor.from_numpy(rng.uniform(-0.1, 0.1, (width, hidden)).astype(np.float32)),
                   HipTensor.from_numpy(rng.uniform(-0.1, 0.1, (width,)).astype(np.float32))]
    w = HipTensor.from_numpy(rng.uniform(-1, 1, (b, s, width)).astype(np.float32), requires_grad=False)
    mask = None
    if masked:
        m = np.ones((b, s), np.float32)
        for i in range(b):
            m[i, s - 1 - 23 * i:] = 0                                  # padded to different lengths
        mask = HipTensor.from_numpy(m, requires_grad=False)
    scale = math.sqrt(d) ** -1

    def step():
        for t in [x] + params:
            t.zero_grad()
        if route == "fused":
            out = x.self_attention(*params, heads=heads, scale=scale, **({"mask": mask} if masked else {}),
                                   **({"dropout": dropout} if dropout > 0 else {}))
        else:                                                          # examples/bert.py, the composite lines
            q, k, v = (x.linear(params[2 * i], params[2 * i + 1]) if hasattr(x, "linear") else x @ params[2 * i].transpose(1, 0) + params[2 * i + 1]
                       for i in range(3))
            q4 = q.reshape(b, s, heads, d).transpose(0, 2, 1, 3)
            k4 = k.reshape(b, s, heads, d).transpose(0, 2, 3, 1)
            v4 = v.reshape(b, s, heads, d).transpose(0, 2, 1, 3)
            scores = q4 @ k4
            if mask is None:
                probs = scores.scaled_softmax(scale)
            else:
                scores = scores / math.sqrt(d) + ((1.0 - mask.reshape(b, 1, 1, s)) * -10000.0).detach()
                probs = scores.softmax(axis=-1)
            if dropout > 0:
                probs = probs.dropout(dropout)
            out = (probs @ v4).transpose(0, 2, 1, 3).reshape(b, s, width)
        (out * w).backward(allow_fill=True)

    def timed(fn):
        for _ in range(20):
            fn()
        HipDevice.synchronize()
        e0, e1 = ctypes.c_void_p(), ctypes.c_void_p()
        L.check(lib.lg_event_create(ctypes.byref(e0)))
        L.check(lib.lg_event_create(ctypes.byref(e1)))
        L.check(lib.lg_event_record(e0))
        for _ in range(iters):
            fn()
        L.check(lib.lg_event_record(e1))
        HipDevice.synchronize()
        ms = ctypes.c_float()
        L.check(lib.lg_event_elapsed_ms(e0, e1, ctypes.byref(ms)))
        return 1e3 * ms.value / iters

    eager = timed(step)
    graph = HipGraph()
    with graph.capture():
        step()
    replayed = timed(graph.replay)
    graph.destroy()
    assert np.isfinite(x.grad.numpy()).all()
    return {"eager_us": round(eager, 2), "graph_us": round(replayed, 2)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--iters", type=int, default=300)
    ap.add_argument("--dropout", type=float, default=0.0)
    ap.add_argument("--out")
    args = ap.parse_args()
    lines = []

    def say(text):
        print(text, flush=True)
        lines.append(text)

    say("self-attention forward + backward beyond 128 positions (projections included), fused node (long launches) against the composite tape "
        "of this build, us per step, %d rounds of %d steps:" % (args.rounds, args.iters))
    if args.dropout > 0:
        say("dropout of the probabilities with p = %g on both routes" % args.dropout)
    for shape in ((8, 128, 2, 64), (8, 512, 2, 64)) if args.dropout > 0 else ((8, 256, 2, 64), (8, 512, 2, 64)):
        for masked in (False,) if args.dropout > 0 else (True, False):
            res = {route: [measure(route, *shape, masked, args.iters, args.dropout) for _ in range(args.rounds)] for route in ("fused", "composite")}
            for key in ("graph_us", "eager_us"):
                f, c = [r[key] for r in res["fused"]], [r[key] for r in res["composite"]]
                say("  %-22s %-12s %-9s fused %s   composite %s   composite / fused %.2f"
                    % (shape, "padding mask" if masked else "no mask", key, " ".join("%.2f" % x for x in f), " ".join("%.2f" % x for x in c),
                       min(c) / min(f)))
    if args.out:
        with open(args.out, "w") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
