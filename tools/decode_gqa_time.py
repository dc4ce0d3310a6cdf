"""Time the grouped-query decode attention (csrc/decode_gqa.hip) on the GPU: batch 8, 8 query heads, d = 64.

    python tools/decode_gqa_time.py [--rounds 5] [--iters 200] [--out profiles/decode_gqa.txt]

The launch alone, replayed from a graph of 32 launches, at t = 1023, 4095 and 16383 (capacity t + 1), alternating in one process:
  split   lg_attention_decode_split_f32 with 8 heads on caches of 8 heads - the only route of a build without the kernel, and
          what a grouped model costs there after its K/V heads were repeated
  gqa     lg_attention_decode_gqa_f32 with kv_heads = 8 (the same work as split), 2 and 1; next to each the K and V bytes it
          reads and the time their read takes at 6.29 TB/s
One decode step of the causal TINY model with 4 heads (`attention_probs=False`) behind 2000 positions, replayed from a captured
graph: num_key_value_heads = 4 (the split launch) against 1 (the grouped-query launch).

Every figure is device time by HIP events around `--iters` steps after 20 warm-up steps (tools/decode_time.py's `timed`); each
round is a fresh set of tensors, model, cache and capture; median and p10 .. p90 are over the rounds.  Without a GPU this fails."""
import argparse
import math
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from decode_time import BATCH, HBM_BYTES_PER_US, load, timed  # noqa: E402

HEADS, D, LONG = 8, 64, (1023, 4095, 16383)


def measure_launch(t, kv_heads, iters, per_graph=32):
    """us per launch at position t; kv_heads None: the split entry on caches of HEADS heads"""
    import numpy as np
    from lightgrad_amd import HipTensor
    from lightgrad_amd.autograd.hip import HipGraph
    rng = np.random.RandomState(0)
    kvw, capacity = (HEADS if kv_heads is None else kv_heads) * D, t + 1
    draw = lambda *shape: HipTensor.from_numpy(rng.uniform(-1.5, 1.5, shape).astype(np.float32), requires_grad=False)      # noqa: E731
    k, v, q, kn, vn = draw(BATCH, capacity, kvw), draw(BATCH, capacity, kvw), draw(BATCH, 1, HEADS * D), draw(BATCH, 1, kvw), draw(BATCH, 1, kvw)
    pos = HipTensor.from_numpy(np.array([t], np.int32), requires_grad=False)
    extra = {} if kv_heads is None else {"kv_heads": kv_heads}
    if kv_heads == HEADS:                # decode_attention sends kv_heads == heads to the split launch: the R = 1 kernel through the C ABI
        from lightgrad_amd.autograd.hip import lib as L
        o = HipTensor.empty((BATCH, 1, HEADS * D), requires_grad=False)

        def launches():
            for _ in range(per_graph):
                L.check(L.lib().lg_attention_decode_gqa_f32(q.ptr, kvw, kn.ptr, kvw, vn.ptr, kvw, k.ptr, v.ptr, kvw, capacity * kvw, pos.ptr, o.ptr, kvw,
                                                            None, BATCH, HEADS, HEADS, capacity, D, math.sqrt(D) ** -1, None, 0))
    else:
        def launches():
            for _ in range(per_graph):
                q.decode_attention(kn, vn, k, v, pos, heads=HEADS, scale=math.sqrt(D) ** -1, split=True, **extra)
    launches()
    graph = HipGraph()
    with graph.capture():
        launches()
    us = timed(graph.replay, max(1, iters // 4)) / per_graph
    graph.destroy()
    return us


def measure_step(bert, kv_heads, t, iters):
    """(us of one replayed decode step at position t of a cache of t + 1 rows, kernels of the captured step)"""
    import numpy as np
    import lightgrad_amd as light
    import lightgrad_amd.nn as nn
    from lightgrad_amd.autograd.hip import HipGraph
    np.random.seed(0)
    cfg = dict(bert.TINY, causal=True, attention_probs=False, max_position_embeddings=t + 1, num_attention_heads=4, num_key_value_heads=kv_heads)
    model = bert.BertForMaskedLM(**cfg).eval().map_parameters(lambda p: p.hip())
    ids = np.random.randint(0, cfg["vocab_size"], (BATCH, t + 1)).astype(np.int32)
    to_device = lambda a: light.from_numpy(a, requires_grad=False).hip(requires_grad=False)          # noqa: E731
    cache = nn.KVCache(cfg["num_hidden_layers"], BATCH, t + 1, model.bert.encoder.layer[0].attention.self.kv_width, like=model.cls.predictions.bias)
    for r in range(BATCH):               # the prompt, a sequence at a time: the grouped prefill is a composite with (R s, s) scores
        one = nn.KVCache(cfg["num_hidden_layers"], 1, t + 1, cache.width, like=model.cls.predictions.bias)
        model(to_device(ids[r:r + 1, :t]), cache=one)
        for layer in range(cache.layers):
            cache.k[layer][r:r + 1] = one.k[layer]
            cache.v[layer][r:r + 1] = one.v[layer]
    token, out_ids = to_device(ids[:, t:]), to_device(np.zeros((BATCH, t + 2), np.int32))

    def step():
        bert.decode_step(model, cache, token, out_ids)
        cache.set_length(t)                                                # (one fill kernel: every step decodes at the same length)
    cache.set_length(t)
    step()
    graph = HipGraph()
    with graph.capture():
        step()
    out = timed(graph.replay, iters), graph.kernel_count()
    graph.destroy()
    return out


def main():
    import numpy as np
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--step-position", type=int, default=2000)
    ap.add_argument("--out")
    args = ap.parse_args()
    bert = load(ROOT)
    lines = []

    def say(text):
        print(text, flush=True)
        lines.append(text)

    def spread(xs):
        return "%.1f (%.1f .. %.1f)" % (np.median(xs), np.percentile(xs, 10), np.percentile(xs, 90))

    say("batch %d, %d query heads, d = %d; us per launch, median (p10 .. p90) over %d rounds" % (BATCH, HEADS, D, args.rounds))
    routes = [("split, 8 heads", None), ("gqa, kv_heads 8", 8), ("gqa, kv_heads 2", 2), ("gqa, kv_heads 1", 1)]
    for t in LONG:
        us = {name: [] for name, _ in routes}
        for _ in range(args.rounds):                                       # alternating: all see the same neighbours on the machine
            for name, kv_heads in routes:
                us[name].append(measure_launch(t, kv_heads, args.iters))
        for name, kv_heads in routes:
            nbytes = 2 * BATCH * (kv_heads or HEADS) * (t + 1) * D * 4
            say("  t = %5d  %-16s %s   K and V: %6d KiB, %.2f us at 6.29 TB/s   split / this %.2f" % (
                t, name, spread(us[name]), nbytes // 1024, nbytes / HBM_BYTES_PER_US, np.median(us["split, 8 heads"]) / np.median(us[name])))
    t, steps = args.step_position, {}
    for kv_heads in (4, 1):
        res = [measure_step(bert, kv_heads, t, args.iters) for _ in range(args.rounds)]
        steps[kv_heads] = float(np.median([r[0] for r in res]))
        say("  decode step at t = %d, TINY with 4 heads over %d K/V heads: replayed %s us, %d kernels in the captured step" % (
            t, kv_heads, spread([r[0] for r in res]), res[0][1]))
    say("  decode step at t = %d: 4 K/V heads / 1 K/V head %.2f" % (t, steps[4] / steps[1]))
    if args.out:
        with open(args.out, "w") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
