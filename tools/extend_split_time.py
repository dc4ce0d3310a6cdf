"""Time the split-key extend attention (csrc/extend_split.hip) on the GPU: batch 8, 2 heads, d = 64.

    python tools/extend_split_time.py [--rounds 5] [--iters 200] [--out profiles/extend_split.txt]

The launch alone, replayed from a graph of 32 launches (tools/decode_time.py's method); the m new rows end at key t, in a cache
of t + 1 rows:
  slice length   lg_attention_extend_split_f32 at t = 1023, 4095, 16383 and m = 4, 32, 128 for L = 256, 512 and 1024
                 (lg_attention_extend_split_set_slice), the candidates alternating inside every round of one process; the read of
                 its K and V at 6.29 TB/s and m launches of lg_attention_decode_split_f32 next to it
  short caches   the launch (at the built-in L) against lg_attention_extend_f32, m = 32 behind prefixes of 128 and 384 in a cache
                 of 512 rows - for the record: short caches are not routed to it

One append step of the causal TINY model (`attention_probs=False`, 2048 positions) behind a prompt of 2000 tokens, m = 4 and 32:
  split      the forward with `append=True` as it stands: one split launch of attention per layer
  composite  the only route a build without the kernel has beyond 512 rows: the same step with the split form hidden, so
             `_extend` slices the cache with the host mirror of the position and goes through the tensor API
each replayed from a captured graph (a captured composite replays at its own t only: a lower bound of that route).

Every figure is device time by HIP events around `--iters` replays after 20 warm-up ones; median and p10 .. p90 over the rounds.
Without a GPU this fails; nothing here falls back."""
import argparse
import math
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from decode_time import BATCH, HBM_BYTES_PER_US, load, timed  # noqa: E402
from decode_split_time import measure_launch as measure_decode_launch  # noqa: E402

SLICES, LONG, ROWS, SHORT = (256, 512, 1024), (1023, 4095, 16383), (4, 32, 128), (128, 384)


def measure_launch(t, m, split, iters, capacity=None, heads=2, d=64, per_graph=32):
    """us per extend attention launch whose m new rows end at key t (split: the split-key entry), replayed from a graph"""
    import numpy as np
    from lightgrad_amd import HipTensor
    from lightgrad_amd.autograd.hip import HipGraph
    rng = np.random.RandomState(0)
    width, capacity = heads * d, capacity or t + 1
    k, v = (HipTensor.from_numpy(rng.uniform(-1.5, 1.5, (BATCH, capacity, width)).astype(np.float32), requires_grad=False) for _ in range(2))
    q, kn, vn = (HipTensor.from_numpy(rng.uniform(-1.5, 1.5, (BATCH, m, width)).astype(np.float32), requires_grad=False) for _ in range(3))
    pos = HipTensor.from_numpy(np.array([t + 1 - m], np.int32), requires_grad=False)
    extra = {"split": True} if split else {}

    def launches():
        for _ in range(per_graph):
            q.extend_attention(kn, vn, k, v, pos, heads=heads, scale=math.sqrt(d) ** -1, **extra)
    launches()
    graph = HipGraph()
    with graph.capture():
        launches()
    us = timed(graph.replay, max(1, iters // 4)) / per_graph
    graph.destroy()
    return us


def measure_step(bert, route, prompt, m, iters, positions=2048):
    """us of one captured append step of m tokens behind `prompt` cached ones, and the kernels of the captured step"""
    import numpy as np
    import lightgrad_amd as light
    import lightgrad_amd.nn as nn
    from lightgrad_amd import HipTensor
    from lightgrad_amd.autograd.hip import HipGraph
    np.random.seed(0)
    cfg = dict(bert.TINY, causal=True, attention_probs=False, max_position_embeddings=positions)
    model = bert.BertForMaskedLM(**cfg).eval().map_parameters(lambda p: p.hip())
    ids = np.random.randint(0, cfg["vocab_size"], (BATCH, prompt + m)).astype(np.int32)
    to_device = lambda a: light.from_numpy(a, requires_grad=False).hip(requires_grad=False)          # noqa: E731
    cache = nn.KVCache(cfg["num_hidden_layers"], BATCH, positions, cfg["hidden_size"], like=model.cls.predictions.bias)
    model(to_device(ids[:, :prompt]), cache=cache)                         # the prompt, through the streaming node
    tokens = to_device(ids[:, prompt:])
    hidden = HipTensor.self_attention_extend_supported
    if route == "composite":
        HipTensor.self_attention_extend_supported = lambda *a, split=False, **k: not split and hidden(*a, **k)
    try:
        step = lambda: model(tokens, cache=cache, append=True)             # noqa: E731  (the position stays: every step appends at `prompt`)
        step()
        graph = HipGraph()
        with graph.capture():
            step()
        out = timed(graph.replay, iters), graph.kernel_count()
        graph.destroy()
    finally:
        HipTensor.self_attention_extend_supported = hidden
    return out


def main():
    import numpy as np
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--routes", default="launch,short,split,composite")
    ap.add_argument("--out")
    args = ap.parse_args()
    routes = args.routes.split(",")
    bert = load(ROOT)
    from lightgrad_amd.autograd.hip import lib as L
    lines, built_in = [], L.lib().lg_attention_extend_split_slice()

    def say(text):
        print(text, flush=True)
        lines.append(text)

    def spread(xs):
        return "%.1f (%.1f .. %.1f)" % (np.median(xs), np.percentile(xs, 10), np.percentile(xs, 90))

    say("built-in slice length L = %d keys; batch %d, 2 heads, d = 64; us, median (p10 .. p90) over %d rounds" % (built_in, BATCH, args.rounds))
    if "launch" in routes:
        for t in LONG:
            decode = [measure_decode_launch(t, True, args.iters) for _ in range(args.rounds)]
            say("  t = %5d  reading %d KiB of K and V at 6.29 TB/s takes %.2f us; one lg_attention_decode_split_f32 launch %s" % (
                t, 2 * BATCH * 2 * (t + 1) * 64 * 4 // 1024, 2 * BATCH * 2 * (t + 1) * 64 * 4 / HBM_BYTES_PER_US, spread(decode)))
            for m in ROWS:
                us = {s: [] for s in SLICES}
                for _ in range(args.rounds):                               # alternating: the candidates see the same neighbours on the machine
                    for s in SLICES:
                        L.check(L.lib().lg_attention_extend_split_set_slice(s))
                        us[s].append(measure_launch(t, m, True, args.iters))
                say("  t = %5d  m = %3d  %s   m decode launches %.1f" % (
                    t, m, "   ".join("L = %4d: %s" % (s, spread(us[s])) for s in SLICES), m * np.median(decode)))
        L.check(L.lib().lg_attention_extend_split_set_slice(built_in))
    if "short" in routes:
        for prefix in SHORT:
            one, many = [], []
            for _ in range(args.rounds):
                one.append(measure_launch(prefix + 31, 32, False, args.iters, capacity=512))
                many.append(measure_launch(prefix + 31, 32, True, args.iters, capacity=512))
            say("  prefix %3d  m = 32  lg_attention_extend_f32 %s   lg_attention_extend_split_f32 %s   split / single %.2f" % (
                prefix, spread(one), spread(many), np.median(many) / np.median(one)))
    for m in (4, 32):
        med = {}
        for route in [r for r in routes if r in ("split", "composite")]:
            res = [measure_step(bert, route, 2000, m, args.iters) for _ in range(args.rounds)]
            med[route] = float(np.median([r[0] for r in res]))
            say("  append step m = %2d behind 2000 of 2048  %-9s  replayed %s   kernels of the captured step %d" % (
                m, route, spread([r[0] for r in res]), res[0][1]))
        if len(med) == 2:
            say("  append step m = %2d  composite / split: %.2f" % (m, med["composite"] / med["split"]))
    if args.out:
        with open(args.out, "w") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
