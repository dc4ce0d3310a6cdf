"""Time causal self-attention, forward + backward: the node `self_attention(causal=True)` (the CAUSAL forward launches of
csrc/attention.hip / csrc/attention_long.hip, the backward launches as they are) against the composite causal tape of the same
build - what a causal model took before the kernels had the flag - and against the same node without the flag, at
(8, 128, 2 heads, d = 64) and (8, 512, 2, 64):

    python tools/attn_causal_time.py [--rounds 7] [--iters 200] [--out profiles/attention_causal.txt]

All routes start from the same (b, s, hidden) input and the same three projection weights, like BertSelfAttention.forward: the
fused routes are the one node, the composite route three nn.Linear products, the head split by strides, the scores GEMM, divide,
the `(1 - tril) * -10000` constant, softmax, the context GEMM and their backward.  Every figure is device time per step by HIP
events around `--iters` steps after 20 warm-up steps, issued eagerly from the tape (host time included where the host is slower
than the device) and replayed from a captured graph (device time alone); `fwd` rows are the forward alone (no tape), replayed.
Each round is a fresh set of tensors and a fresh capture; median and p10 .. p90 are over the rounds.  Without a GPU this fails;
nothing here falls back."""
import argparse
import ctypes
import math
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def measure(route, b, s, heads, d, iters):
    """{"eager_us", "graph_us", "fwd_graph_us"} of `route`: "causal" / "plain" (the fused node with / without the flag) or "composite" """
    import numpy as np
    import lightgrad_amd as light
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
    tril = HipTensor.from_numpy(np.tril(np.ones((1, 1, s, s), np.float32)), requires_grad=False)
    scale = math.sqrt(d) ** -1

    def forward():
        if route != "composite":
            return x.self_attention(*params, heads=heads, scale=scale, **({"causal": True} if route == "causal" else {}))
        q, k, v = (x.linear(params[2 * i], params[2 * i + 1]) for i in range(3))          # examples/bert.py, the composite lines
        q4 = q.reshape(b, s, heads, d).transpose(0, 2, 1, 3)
        k4 = k.reshape(b, s, heads, d).transpose(0, 2, 3, 1)
        v4 = v.reshape(b, s, heads, d).transpose(0, 2, 1, 3)
        scores = (q4 @ k4) / math.sqrt(d) + ((1.0 - tril) * -10000.0).detach()
        return (scores.softmax(axis=-1) @ v4).transpose(0, 2, 1, 3).reshape(b, s, width)

    def step():
        for t in [x] + params:
            t.zero_grad()
        (forward() * w).backward(allow_fill=True)

    def forward_only():
        with light.no_grad():
            forward()

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

    out = {"eager_us": timed(step)}
    for key, fn in (("graph_us", step), ("fwd_graph_us", forward_only)):
        fn()
        graph = HipGraph()
        with graph.capture():
            fn()
        out[key] = timed(graph.replay)
        graph.destroy()
    assert np.isfinite(x.grad.numpy()).all()
    return out


def main():
    import numpy as np
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--batch", type=int, default=8, help="more (batch, head, block) workgroups than CUs: several rounds of the grid")
    ap.add_argument("--routes", default="causal,plain,composite", help="e.g. `plain` alone, to time a build that has no causal flag")
    ap.add_argument("--out")
    args = ap.parse_args()
    routes = args.routes.split(",")
    lines = []

    def say(text):
        print(text, flush=True)
        lines.append(text)

    say("causal self-attention (projections included): fused node with causal=True, the same node without the flag, and the composite "
        "causal tape of this build; us per step, median (p10 .. p90) over %d rounds of %d steps:" % (args.rounds, args.iters))
    for shape in ((args.batch, 128, 2, 64), (args.batch, 512, 2, 64)):
        res = {route: [measure(route, *shape, args.iters) for _ in range(args.rounds)] for route in routes}
        for key, what in (("graph_us", "fwd+bwd graph"), ("eager_us", "fwd+bwd eager"), ("fwd_graph_us", "fwd graph")):
            cells, med = [], {}
            for route in routes:
                xs = [r[key] for r in res[route]]
                med[route] = float(np.median(xs))
                cells.append("%s %.2f (%.2f .. %.2f)" % (route, med[route], np.percentile(xs, 10), np.percentile(xs, 90)))
            ratios = ""
            if "causal" in med and "plain" in med:
                ratios += "   causal / plain %.3f" % (med["causal"] / med["plain"])
            if "causal" in med and "composite" in med:
                ratios += "   composite / causal %.2f" % (med["composite"] / med["causal"])
            say("  %-18s %-14s %s%s" % (shape, what, "   ".join(cells), ratios))
    if args.out:
        with open(args.out, "w") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
