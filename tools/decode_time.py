"""Time incremental decoding of the causal tiny-BERT (TINY config, batch 8) on the GPU.

    python tools/decode_time.py [--rounds 5] [--iters 200] [--out profiles/decode.txt]
    python tools/decode_time.py --routes full --tree <a checkout of another commit, built>      # that commit's only route

Per-token latency at prefix lengths 128 and 511 (the new token is position 128 / 511, the last the model has):
  decode   one `decode_step` of examples/bert.py against an nn.KVCache that holds the prefix: the model's decode forward on one
           token per sequence (two launches of attention per layer, csrc/decode.hip), the head, argmax, the writes of the ids,
           `advance()`; after every timed step the position is set back, so each step decodes at the same length
  full     the only route a build without the cache has: the full causal forward over prefix + 1 positions, the head on the last
           row (`masked_positions`), argmax (`--tree`: import the package and the model from that tree instead of this one)
each issued eagerly (host time included) and replayed from a captured graph; the kernel count of the captured step is printed
(for `decode` it includes this tool's one fill kernel that sets the position back).

The decode launch alone, lg_attention_decode_f32 at (b, heads, d) = (8, 2, 64), t = 127 and t = 511, replayed from a graph of
32 launches: against the time to read 2 b heads (t + 1) d 4 bytes at 6.29 TB/s (the HBM rate MI355X_MICROARCH.md measured; the
caches of a step were written by the steps before, so most of them sit in the 256 MiB Infinity Cache) and against the 1.45 us
between two trivial dependent kernels of that guide - whichever is larger binds.

Every figure is device time by HIP events around `--iters` steps after 20 warm-up steps; each round is a fresh model, cache and
capture; median and p10 .. p90 are over the rounds.  Without a GPU this fails; nothing here falls back."""
import argparse
import ctypes
import importlib.util
import math
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BATCH, HBM_BYTES_PER_US, BOUNDARY_US = 8, 6.29e6, 1.45


def load(tree):
    sys.path.insert(0, tree)
    spec = importlib.util.spec_from_file_location("bert_example_timing", os.path.join(tree, "examples", "bert.py"))
    bert = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(bert)
    return bert


def timed(fn, iters):
    from lightgrad_amd.autograd.hip import HipDevice
    from lightgrad_amd.autograd.hip import lib as L
    lib = L.lib()
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


def measure_step(bert, route, prefix, iters):
    """{"eager_us", "graph_us", "kernels"} of one token at position `prefix`"""
    import numpy as np
    import lightgrad_amd as light
    from lightgrad_amd.autograd.hip import HipGraph
    np.random.seed(0)
    model = bert.BertForMaskedLM(**dict(bert.TINY, causal=True)).eval().map_parameters(lambda p: p.hip())
    ids = np.random.randint(0, bert.TINY["vocab_size"], (BATCH, prefix + 1)).astype(np.int32)
    to_device = lambda a: light.from_numpy(a, requires_grad=False).hip(requires_grad=False)          # noqa: E731
    if route == "decode":
        import lightgrad_amd.nn as nn
        cache = nn.KVCache(bert.TINY["num_hidden_layers"], BATCH, prefix + 1, bert.TINY["hidden_size"], like=model.cls.predictions.bias)
        model(to_device(ids[:, :prefix]), cache=cache)                     # the prefix: rows 0 .. prefix - 1 of the cache
        token, out_ids = to_device(ids[:, prefix:]), to_device(np.zeros((BATCH, prefix + 2), np.int32))

        def step():
            bert.decode_step(model, cache, token, out_ids)
            cache.set_length(prefix)                                       # (one fill kernel: every step decodes at the same length)
    else:
        full = to_device(ids)
        last = to_device(np.arange(BATCH, dtype=np.int32) * (prefix + 1) + prefix)        # the last row of every sequence

        def step():
            with light.no_grad():
                model(full, masked_positions=last).argmax(-1).astype(np.int32)
    out = {"eager_us": timed(step, iters)}
    graph = HipGraph()
    with graph.capture():
        step()
    out["graph_us"], out["kernels"] = timed(graph.replay, iters), graph.kernel_count()
    graph.destroy()
    return out


def measure_launch(t, iters, heads=2, d=64, per_graph=32):
    """us per lg_attention_decode_f32 launch at position t, replayed from a graph of `per_graph` launches"""
    import numpy as np
    from lightgrad_amd import HipTensor
    from lightgrad_amd.autograd.hip import HipGraph
    rng = np.random.RandomState(0)
    width, capacity = heads * d, t + 1
    k, v = (HipTensor.from_numpy(rng.uniform(-1.5, 1.5, (BATCH, capacity, width)).astype(np.float32), requires_grad=False) for _ in range(2))
    q, kn, vn = (HipTensor.from_numpy(rng.uniform(-1.5, 1.5, (BATCH, 1, width)).astype(np.float32), requires_grad=False) for _ in range(3))
    pos = HipTensor.from_numpy(np.array([t], np.int32), requires_grad=False)

    def launches():
        for _ in range(per_graph):
            q.decode_attention(kn, vn, k, v, pos, heads=heads, scale=math.sqrt(d) ** -1)
    launches()
    graph = HipGraph()
    with graph.capture():
        launches()
    us = timed(graph.replay, max(1, iters // 4)) / per_graph
    graph.destroy()
    return us


def main():
    import numpy as np
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--routes", default="decode,full,launch")
    ap.add_argument("--tree", default=ROOT, help="import lightgrad_amd and examples/bert.py from this tree")
    ap.add_argument("--out")
    args = ap.parse_args()
    routes = args.routes.split(",")
    bert = load(os.path.abspath(args.tree))
    lines = []

    def say(text):
        print(text, flush=True)
        lines.append(text)

    def spread(xs):
        return "%.1f (%.1f .. %.1f)" % (np.median(xs), np.percentile(xs, 10), np.percentile(xs, 90))

    say("tree %s; TINY causal model, batch %d; us per token, median (p10 .. p90) over %d rounds of %d steps" % (
        os.path.relpath(os.path.abspath(args.tree), ROOT), BATCH, args.rounds, args.iters))
    for prefix in (128, 511):
        med = {}
        for route in [r for r in routes if r in ("decode", "full")]:
            res = [measure_step(bert, route, prefix, args.iters) for _ in range(args.rounds)]
            med[route] = float(np.median([r["graph_us"] for r in res]))
            say("  prefix %3d  %-6s  eager %s   replayed %s   kernels of the captured step %d" % (
                prefix, route, spread([r["eager_us"] for r in res]), spread([r["graph_us"] for r in res]), res[0]["kernels"]))
        if len(med) == 2:
            say("  prefix %3d  full / decode, replayed: %.2f" % (prefix, med["full"] / med["decode"]))
    if "launch" in routes:
        for t in (127, 511):
            xs = [measure_launch(t, args.iters) for _ in range(args.rounds)]
            read_us = 2 * BATCH * 2 * (t + 1) * 64 * 4 / HBM_BYTES_PER_US
            say("  lg_attention_decode_f32 (8, 2, 64) t = %3d: %s us per launch, replayed; reading its %d KiB of K and V at 6.29 TB/s "
                "takes %.2f us, a kernel boundary %.2f us: the %s floor binds" % (
                    t, spread(xs), 2 * BATCH * 2 * (t + 1) * 64 * 4 // 1024, read_us, BOUNDARY_US, "read" if read_us > BOUNDARY_US else "launch"))
    if args.out:
        with open(args.out, "w") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
