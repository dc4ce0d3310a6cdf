"""Time the split-key decode attention (csrc/decode_split.hip) on the GPU: batch 8, 2 heads, d = 64.

    python tools/decode_split_time.py [--rounds 5] [--iters 200] [--out profiles/decode_split.txt]

The launch alone, replayed from a graph of 32 launches (tools/decode_time.py's `measure_launch`), capacity t + 1:
  below 512 keys   lg_attention_decode_split_f32 against lg_attention_decode_f32 at t = 127 and 511, alternating in one process -
                   what decides whether short caches may go to the split kernel
  beyond 512 keys  lg_attention_decode_split_f32 at t = 1023, 4095 and 16383; the read of its K and V at 6.29 TB/s next to it

One decode step of the causal TINY model (`attention_probs=False`, t + 1 position embeddings) at those three positions, the prompt
prefilled through the streaming attention node:
  split      `decode_step` of examples/bert.py as it stands: two split launches of attention per layer
  composite  the only route a build without the kernel has beyond 512 rows: the same step with the backend's decode node hidden,
             so `_decode` slices the cache with the host mirror of the position and goes through the tensor API
each issued eagerly (host time included) and replayed from a captured graph (a captured composite replays at its own t only: it
is timed as a lower bound of that route, not as something `generate` could use).

Every figure is device time by HIP events around `--iters` steps after 20 warm-up steps; each round is a fresh set of tensors,
model, cache and capture; median and p10 .. p90 are over the rounds.  Without a GPU this fails; nothing here falls back."""
import argparse
import math
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from decode_time import BATCH, HBM_BYTES_PER_US, load, timed  # noqa: E402

SHORT, LONG = (127, 511), (1023, 4095, 16383)


def measure_launch(t, split, iters, heads=2, d=64, per_graph=32):
    """us per decode attention launch at position t (split: the split-key entry), replayed from a graph of `per_graph` launches"""
    import numpy as np
    from lightgrad_amd import HipTensor
    from lightgrad_amd.autograd.hip import HipGraph
    rng = np.random.RandomState(0)
    width, capacity = heads * d, t + 1
    k, v = (HipTensor.from_numpy(rng.uniform(-1.5, 1.5, (BATCH, capacity, width)).astype(np.float32), requires_grad=False) for _ in range(2))
    q, kn, vn = (HipTensor.from_numpy(rng.uniform(-1.5, 1.5, (BATCH, 1, width)).astype(np.float32), requires_grad=False) for _ in range(3))
    pos = HipTensor.from_numpy(np.array([t], np.int32), requires_grad=False)
    extra = {"split": True} if split else {}

    def launches():
        for _ in range(per_graph):
            q.decode_attention(kn, vn, k, v, pos, heads=heads, scale=math.sqrt(d) ** -1, **extra)
    launches()
    graph = HipGraph()
    with graph.capture():
        launches()
    us = timed(graph.replay, max(1, iters // 4)) / per_graph
    graph.destroy()
    return us


def measure_step(bert, route, t, iters):
    """{"eager_us", "graph_us", "kernels"} of one token at position t of a cache of t + 1 rows"""
    import numpy as np
    import lightgrad_amd as light
    import lightgrad_amd.nn as nn
    from lightgrad_amd import HipTensor
    from lightgrad_amd.autograd.hip import HipGraph
    np.random.seed(0)
    cfg = dict(bert.TINY, causal=True, attention_probs=False, max_position_embeddings=t + 1)
    model = bert.BertForMaskedLM(**cfg).eval().map_parameters(lambda p: p.hip())
    ids = np.random.randint(0, cfg["vocab_size"], (BATCH, t + 1)).astype(np.int32)
    to_device = lambda a: light.from_numpy(a, requires_grad=False).hip(requires_grad=False)          # noqa: E731
    cache = nn.KVCache(cfg["num_hidden_layers"], BATCH, t + 1, cfg["hidden_size"], like=model.cls.predictions.bias)
    model(to_device(ids[:, :t]), cache=cache)                              # the prompt: rows 0 .. t - 1, through the streaming node
    token, out_ids = to_device(ids[:, t:]), to_device(np.zeros((BATCH, t + 2), np.int32))
    hidden = HipTensor.self_attention_decode_supported
    if route == "composite":
        HipTensor.self_attention_decode_supported = lambda *a, **k: False
    try:
        def step():
            bert.decode_step(model, cache, token, out_ids)
            cache.set_length(t)                                            # (one fill kernel: every step decodes at the same length)
        out = {"eager_us": timed(step, iters)}
        graph = HipGraph()
        with graph.capture():
            step()
        out["graph_us"], out["kernels"] = timed(graph.replay, iters), graph.kernel_count()
        graph.destroy()
    finally:
        HipTensor.self_attention_decode_supported = hidden
    return out


def main():
    import numpy as np
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--routes", default="launch,split,composite")
    ap.add_argument("--positions", default=",".join(str(t) for t in LONG), help="the positions beyond 512 keys")
    ap.add_argument("--out")
    args = ap.parse_args()
    routes, long_ts = args.routes.split(","), [int(t) for t in args.positions.split(",")]
    bert = load(ROOT)
    from lightgrad_amd.autograd.hip import lib as L
    lines = []

    def say(text):
        print(text, flush=True)
        lines.append(text)

    def spread(xs):
        return "%.1f (%.1f .. %.1f)" % (np.median(xs), np.percentile(xs, 10), np.percentile(xs, 90))

    say("slice length L = %d keys; batch %d, 2 heads, d = 64; us, median (p10 .. p90) over %d rounds" % (
        L.lib().lg_attention_decode_split_slice(), BATCH, args.rounds))
    if "launch" in routes:
        for t in SHORT:
            one, many = [], []
            for _ in range(args.rounds):                                   # alternating: both see the same neighbours on the machine
                one.append(measure_launch(t, False, args.iters))
                many.append(measure_launch(t, True, args.iters))
            say("  t = %5d  lg_attention_decode_f32 %s   lg_attention_decode_split_f32 %s   split / single %.2f" % (
                t, spread(one), spread(many), np.median(many) / np.median(one)))
        for t in long_ts:
            xs = [measure_launch(t, True, args.iters) for _ in range(args.rounds)]
            say("  t = %5d  lg_attention_decode_split_f32 %s us per launch; reading its %d KiB of K and V at 6.29 TB/s takes %.2f us" % (
                t, spread(xs), 2 * BATCH * 2 * (t + 1) * 64 * 4 // 1024, 2 * BATCH * 2 * (t + 1) * 64 * 4 / HBM_BYTES_PER_US))
    for t in long_ts:
        med = {}
        for route in [r for r in routes if r in ("split", "composite")]:
            res = [measure_step(bert, route, t, args.iters) for _ in range(args.rounds)]
            med[route] = (float(np.median([r["eager_us"] for r in res])), float(np.median([r["graph_us"] for r in res])))
            say("  decode step at t = %5d  %-9s  eager %s   replayed %s   kernels of the captured step %d" % (
                t, route, spread([r["eager_us"] for r in res]), spread([r["graph_us"] for r in res]), res[0]["kernels"]))
        if len(med) == 2:
            say("  decode step at t = %5d  composite / split: eager %.2f, replayed %.2f" % (
                t, med["composite"][0] / med["split"][0], med["composite"][1] / med["split"][1]))
    if args.out:
        with open(args.out, "w") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
