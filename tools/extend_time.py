"""Time appending m tokens to a filled key / value cache of the causal tiny-BERT (TINY config, batch 8) on the GPU.

    python tools/extend_time.py [--rounds 5] [--iters 100] [--out profiles/extend.txt]
    python tools/extend_time.py --routes decode --tree <a checkout of another commit, built>      # that commit's only route

At prefixes 128 and 384 (tokens the nn.KVCache already holds) and m in {4, 32, 128} new tokens per sequence, the time to take the
m tokens in and have the argmax of every one of their logit rows (what scoring a continuation or verifying m drafted tokens asks
for):
  extend   ONE append step of examples/bert.py, `model(tokens, cache=cache, append=True)` on (8, m) ids - one projection launch
           and one lg_attention_extend_f32 launch per layer (csrc/extend.hip), the head on the m rows, argmax, `advance(m)` -
           captured once and replayed
  decode   the only route a build without the entry has for a filled cache: m replays of the captured `decode_step` (one token
           per sequence each, csrc/decode.hip) (`--tree`: import the package and the model from that tree instead of this one)
after every timed group the position is set back (one fill kernel), so each group starts at the same prefix.

The attention launch alone at (b, heads, d) = (8, 2, 64), capacity prefix + m: one lg_attention_extend_f32 launch against m
lg_attention_decode_f32 launches at positions prefix .. prefix + m - 1, each replayed from a captured graph.

Every figure is device time by HIP events around `--iters` groups after 20 warm-up groups; each round is a fresh model, cache
and capture; median and p10 .. p90 are over the rounds.  Without a GPU this fails; nothing here falls back."""
import argparse
import math
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from decode_time import BATCH, load, timed  # noqa: E402

PREFIXES, MS = (128, 384), (4, 32, 128)


def measure_group(bert, route, prefix, m, iters):
    """{"us", "kernels"}: device time of taking m tokens in behind `prefix` cached ones, and the kernels of the captured step"""
    import numpy as np
    import lightgrad_amd as light
    import lightgrad_amd.nn as nn
    from lightgrad_amd.autograd.hip import HipGraph
    np.random.seed(0)
    model = bert.BertForMaskedLM(**dict(bert.TINY, causal=True)).eval().map_parameters(lambda p: p.hip())
    ids = np.random.randint(0, bert.TINY["vocab_size"], (BATCH, prefix + m)).astype(np.int32)
    to_device = lambda a: light.from_numpy(a, requires_grad=False).hip(requires_grad=False)          # noqa: E731
    cache = nn.KVCache(bert.TINY["num_hidden_layers"], BATCH, prefix + m, bert.TINY["hidden_size"], like=model.cls.predictions.bias)
    model(to_device(ids[:, :prefix]), cache=cache)                         # the prefix: rows 0 .. prefix - 1 of the cache
    graph = HipGraph()
    if route == "extend":
        tokens = to_device(np.ascontiguousarray(ids[:, prefix:]))

        def step():
            model(tokens, cache=cache, append=True).argmax(-1).astype(np.int32)
            cache.advance(m)
        step()
        cache.set_length(prefix)
        with graph.capture():
            step()
        cache.set_length(prefix)

        def group():
            graph.replay()
            cache.set_length(prefix)
    else:
        token, out_ids = to_device(np.ascontiguousarray(ids[:, prefix:prefix + 1])), to_device(np.zeros((BATCH, prefix + m + 1), np.int32))
        bert.decode_step(model, cache, token, out_ids)
        cache.set_length(prefix)
        with graph.capture():
            bert.decode_step(model, cache, token, out_ids)
        cache.set_length(prefix)

        def group():
            for _ in range(m):
                graph.replay()
            cache.set_length(prefix)
    out = {"us": timed(group, iters), "kernels": graph.kernel_count()}
    graph.destroy()
    return out


def measure_launch(route, prefix, m, iters, heads=2, d=64):
    """us per group of attention launches that take m tokens in at position `prefix`: one extend launch, or m decode launches"""
    import numpy as np
    from lightgrad_amd import HipTensor
    from lightgrad_amd.autograd.hip import HipGraph
    rng = np.random.RandomState(0)
    width, capacity = heads * d, prefix + m
    tensor = lambda shape: HipTensor.from_numpy(rng.uniform(-1.5, 1.5, shape).astype(np.float32), requires_grad=False)      # noqa: E731
    k, v = tensor((BATCH, capacity, width)), tensor((BATCH, capacity, width))
    rows = m if route == "extend" else 1
    q, kn, vn = tensor((BATCH, rows, width)), tensor((BATCH, rows, width)), tensor((BATCH, rows, width))
    scale = math.sqrt(d) ** -1
    if route == "extend":
        pos = [HipTensor.from_numpy(np.array([prefix], np.int32), requires_grad=False)]
        launches = lambda: q.extend_attention(kn, vn, k, v, pos[0], heads=heads, scale=scale)                              # noqa: E731
    else:
        pos = [HipTensor.from_numpy(np.array([prefix + i], np.int32), requires_grad=False) for i in range(m)]

        def launches():
            for p in pos:
                q.decode_attention(kn, vn, k, v, p, heads=heads, scale=scale)
    launches()
    graph = HipGraph()
    with graph.capture():
        launches()
    us = timed(graph.replay, max(1, iters // 2))
    graph.destroy()
    return us


def main():
    import numpy as np
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--iters", type=int, default=100)
    ap.add_argument("--routes", default="extend,decode,launch")
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

    say("tree %s; TINY causal model, batch %d; us per group of m tokens, median (p10 .. p90) over %d rounds of %d groups" % (
        os.path.relpath(os.path.abspath(args.tree), ROOT), BATCH, args.rounds, args.iters))
    for prefix in PREFIXES:
        for m in MS:
            med = {}
            for route in [r for r in routes if r in ("extend", "decode")]:
                res = [measure_group(bert, route, prefix, m, args.iters) for _ in range(args.rounds)]
                med[route] = float(np.median([r["us"] for r in res]))
                say("  prefix %3d  m %3d  %-6s  %s   kernels of the captured step %d" % (prefix, m, route, spread([r["us"] for r in res]), res[0]["kernels"]))
            if len(med) == 2:
                say("  prefix %3d  m %3d  decode / extend: %.2f" % (prefix, m, med["decode"] / med["extend"]))
    if "launch" in routes:
        for prefix in PREFIXES:
            for m in MS:
                one = [measure_launch("extend", prefix, m, args.iters) for _ in range(args.rounds)]
                many = [measure_launch("decode", prefix, m, args.iters) for _ in range(args.rounds)]
                say("  launch alone (8, 2, 64)  prefix %3d  m %3d: lg_attention_extend_f32 %s us; %d x lg_attention_decode_f32 %s us; ratio %.2f" % (
                    prefix, m, spread(one), m, spread(many), np.median(many) / np.median(one)))
    if args.out:
        with open(args.out, "w") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
