"""Time forward + backward of `stream_attention` (csrc/attention_stream.hip) and count the bytes its tape keeps alive:

    python tools/attention_stream_time.py [--rounds 5] [--out profiles/attention_stream.txt]
    python tools/attention_stream_time.py --dropout 0.1 --lengths 1024 2048 4096      # attention dropout inside the streaming launches

  * at s = 256 and 512 against `long_attention` (csrc/attention_long.hip, the stored-P kernels these lengths have);
  * at s = 1024, 2048 and 4096 against the composite tape (examples/bert.py's lines: scores GEMM, divide, softmax, context GEMM),
    the only other route there;
batch 8, 2 heads, d = 64, no mask and causal.  All routes start from the same q, k, v (no projections: they are the same launches
for every route).  Times are device time per forward + backward by HIP events around a window of steps replayed from a captured
graph (no host time), after a warm-up of the same graph; the window is sized to about a quarter of a second; the routes of a shape
alternate within each round and every round's figure is printed, so the spread is visible.  Live bytes: what the allocator has in
use after the forward minus before it (lg_pool_stats) - the result and what the tape holds for the backward.
--dropout P: three routes per shape - `stream_attention` without dropout, `stream_attention(dropout=P)` and the composite tape with
`probs.dropout(P)` - each timed twice: forward + backward, and the forward alone under no_grad (the backward is the difference).
Without a GPU this fails; nothing here falls back."""
import argparse
import ctypes
import math
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def in_use(lib):
    reserved, used, calls = ctypes.c_uint64(), ctypes.c_uint64(), ctypes.c_uint64()
    lib.lg_pool_stats(ctypes.byref(reserved), ctypes.byref(used), ctypes.byref(calls))
    return used.value


class Route(object):
    """one route at one shape: its operands, its captured step, and the bytes its forward leaves alive"""

    def __init__(self, route, b, s, heads, d, causal, dropout=0.0, forward_only=False):
        import numpy as np
        import lightgrad_amd as light
        from lightgrad_amd import HipTensor
        from lightgrad_amd.autograd.hip import HipGraph, HipDevice
        from lightgrad_amd.autograd.hip import lib as L
        self.lib, self.sync = L.lib(), HipDevice.synchronize
        rng = np.random.RandomState(0)
        width, scale = heads * d, math.sqrt(d) ** -1
        q, k, v = (HipTensor.from_numpy(rng.uniform(-1.5, 1.5, (b, s, width)).astype(np.float32)) for _ in range(3))
        w = HipTensor.from_numpy(rng.uniform(-1, 1, (b, s, width)).astype(np.float32), requires_grad=False)
        tril = None
        if route == "composite" and causal:
            tril = HipTensor.from_numpy(((1.0 - np.tril(np.ones((1, 1, s, s), np.float32))) * -10000.0).astype(np.float32), requires_grad=False)

        def forward():
            if route == "stream":
                return q.stream_attention(k, v, heads=heads, scale=scale, causal=causal, **({"dropout": dropout} if dropout > 0 else {}))
            if route == "long":
                return q.long_attention(k, v, heads=heads, scale=scale, causal=causal)
            q4 = q.reshape(b, s, heads, d).transpose(0, 2, 1, 3)
            k4 = k.reshape(b, s, heads, d).transpose(0, 2, 3, 1)
            v4 = v.reshape(b, s, heads, d).transpose(0, 2, 1, 3)
            probs = (q4 @ k4).scaled_softmax(scale) if tril is None else ((q4 @ k4) / math.sqrt(d) + tril).softmax(axis=-1)
            return ((probs.dropout(dropout) if dropout > 0 else probs) @ v4).transpose(0, 2, 1, 3).reshape(b, s, width)

        def step():
            if forward_only:
                with light.no_grad():
                    return forward()
            for t in (q, k, v):
                t.zero_grad()
            (forward() * w).backward(allow_fill=True)

        step()
        self.sync()
        before = in_use(self.lib)
        out = forward()
        self.sync()
        self.live_bytes = in_use(self.lib) - before
        del out
        self.graph = HipGraph()
        with self.graph.capture():
            step()
        for _ in range(10):
            self.graph.replay()
        self.sync()
        self.iters = 10
        self.iters = max(10, int(0.25e6 / self.time()))               # a window of about a quarter of a second

    def time(self):
        """us per forward + backward over one window"""
        from lightgrad_amd.autograd.hip import lib as L
        e0, e1, ms = ctypes.c_void_p(), ctypes.c_void_p(), ctypes.c_float()
        L.check(self.lib.lg_event_create(ctypes.byref(e0)))
        L.check(self.lib.lg_event_create(ctypes.byref(e1)))
        L.check(self.lib.lg_event_record(e0))
        for _ in range(self.iters):
            self.graph.replay()
        L.check(self.lib.lg_event_record(e1))
        self.sync()
        L.check(self.lib.lg_event_elapsed_ms(e0, e1, ctypes.byref(ms)))
        return 1e3 * ms.value / self.iters


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--lengths", type=int, nargs="*", default=[256, 512, 1024, 2048, 4096])
    ap.add_argument("--dropout", type=float, default=0.0)
    ap.add_argument("--out")
    args = ap.parse_args()
    lines = []

    def say(text):
        print(text, flush=True)
        lines.append(text)

    b, heads, d = 8, 2, 64
    say("attention forward + backward from q, k, v at batch %d, %d heads, d = %d: stream_attention against long_attention (s <= 512) or the "
        "composite tape (beyond), us per step from a replayed graph, %d alternating rounds; live bytes after the forward" % (b, heads, d, args.rounds))
    if args.dropout > 0:
        say("dropout %g: stream (no dropout) | stream_dropout | composite with probs.dropout; fwd+bwd us and forward-only us per round" % args.dropout)
        for s in args.lengths:
            for causal in (False, True):
                specs = {"stream": ("stream", 0.0), "stream_dropout": ("stream", args.dropout), "composite_dropout": ("composite", args.dropout)}
                routes = {(name, only): Route(route, b, s, heads, d, causal, p, only) for name, (route, p) in specs.items() for only in (False, True)}
                times = {key: [] for key in routes}
                for _ in range(args.rounds):
                    for key, route in routes.items():
                        times[key].append(route.time())
                for name in specs:
                    say("  s = %-5d %-7s %-18s fwd+bwd %s us   fwd %s us   %d bytes alive after the forward" % (
                        s, "causal" if causal else "full", name, " ".join("%.1f" % t for t in times[(name, False)]),
                        " ".join("%.1f" % t for t in times[(name, True)]), routes[(name, False)].live_bytes))
                for route in routes.values():
                    route.graph.destroy()
        args.lengths = []
    for s in args.lengths:
        other = "long" if s <= 512 else "composite"
        for causal in (False, True):
            routes = {name: Route(name, b, s, heads, d, causal) for name in ("stream", other)}
            times = {name: [] for name in routes}
            for _ in range(args.rounds):
                for name, route in routes.items():
                    times[name].append(route.time())
            say("  s = %-5d %-7s stream %s us, %d bytes   %s %s us, %d bytes   %s / stream: time %.2f, bytes %.1f" % (
                s, "causal" if causal else "full", " ".join("%.1f" % t for t in times["stream"]), routes["stream"].live_bytes,
                other, " ".join("%.1f" % t for t in times[other]), routes[other].live_bytes, other,
                sorted(times[other])[len(times[other]) // 2] / sorted(times["stream"])[len(times["stream"]) // 2],
                routes[other].live_bytes / max(routes["stream"].live_bytes, 1)))
            for route in routes.values():
                route.graph.destroy()
    if args.out:
        with open(args.out, "w") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
