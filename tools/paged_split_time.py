"""Time the paged split-key extend attention (csrc/paged_split.hip) on the GPU: batch 8, 2 heads, d = 64.

    python tools/paged_split_time.py [--rounds 5] [--iters 200] [--out profiles/paged_split.txt]

The launch alone, replayed from a graph of 32 launches (tools/decode_time.py's method); the m new rows end at key t = keys - 1:
  launch       `extend_attention(count=, block_table=, block_size=, split=True)` at keys = 1024, 4096, 16384 and m = 1, 4, 32, in
               blocks of 16 and 128, through identity and shuffled tables, over float32 and bfloat16 pools, next to the contiguous
               lg_attention_extend_split_counts_f32 at the same shape - all of them alternating inside every round of one process
  validation   keys = 16384 in blocks of 4 (every workgroup scans 4096 table words) next to blocks of 128 (128 words)
One counted append step of the causal TINY model (`attention_probs=False`, 2048 positions) behind 2000 cached tokens, m = 4 and 32,
captured and replayed: against an nn.PagedKVCache(split=True) in blocks of 16, and against the contiguous per-row nn.KVCache.

Every figure is device time by HIP events around `--iters` replays after 20 warm-up ones; median and p10 .. p90 over the rounds.
Without a GPU this fails; nothing here falls back."""
import argparse
import math
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from decode_time import BATCH, load, timed  # noqa: E402

KEYS, ROWS, BLOCKS = (1024, 4096, 16384), (1, 4, 32), (16, 128)


def measure_launch(keys, m, B, shuffled, bf16, iters, heads=2, d=64, per_graph=32):
    """us per launch whose m new rows end at key keys - 1, replayed from a graph; B = None: the contiguous counts entry"""
    import numpy as np
    import lightgrad_amd as light
    from lightgrad_amd import HipTensor
    from lightgrad_amd.autograd.hip import HipGraph
    rng = np.random.RandomState(0)
    width = heads * d
    up = lambda a: HipTensor.from_numpy(np.ascontiguousarray(a), requires_grad=False)                # noqa: E731
    q, kn, vn = (up(rng.uniform(-1.5, 1.5, (BATCH, m, width)).astype(np.float32)) for _ in range(3))
    pos, count = up(np.full(BATCH, keys - m, np.int32)), up(np.full(BATCH, m, np.int32))
    extra = {"count": count, "split": True}
    if B is None:
        k, v = (up(rng.uniform(-1.5, 1.5, (BATCH, keys, width)).astype(np.float32)) for _ in range(2))
    else:
        blocks = keys // B
        rows = [rng.uniform(-1.5, 1.5, (BATCH * blocks, B, width)).astype(np.float32) for _ in range(2)]
        k, v = (up(light.bf16_bits(a) if bf16 else a) for a in rows)
        order = rng.permutation(BATCH * blocks) if shuffled else np.arange(BATCH * blocks)
        extra.update(block_table=up(order.reshape(BATCH, blocks).astype(np.int32)), block_size=B, **({"kv_dtype": "bf16"} if bf16 else {}))

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


def measure_step(bert, paged, prompt, m, iters, positions=2048, block=16):
    """us of one captured counted append step of m tokens behind `prompt` cached ones, and the kernels of the captured step"""
    import numpy as np
    import lightgrad_amd as light
    import lightgrad_amd.nn as nn
    from lightgrad_amd.autograd.hip import HipGraph
    np.random.seed(0)
    cfg = dict(bert.TINY, causal=True, attention_probs=False, max_position_embeddings=positions)
    model = bert.BertForMaskedLM(**cfg).eval().map_parameters(lambda p: p.hip())
    to_device = lambda a: light.from_numpy(np.ascontiguousarray(a), requires_grad=False).hip(requires_grad=False)          # noqa: E731
    like, layers, width = model.cls.predictions.bias, cfg["num_hidden_layers"], cfg["hidden_size"]
    if paged:
        per = positions // block
        cache = nn.PagedKVCache(layers, BATCH, BATCH * per, block, width, per, like=like, split=True)
        cache.block_table[:] = to_device(np.random.permutation(BATCH * per).reshape(BATCH, per).astype(np.int32))
    else:
        cache = nn.KVCache(layers, BATCH, positions, width, like=like, per_row=True)
    # (what the cached rows hold does not change the time: the step runs on the rows as they are)
    cache.pos[:] = to_device(np.full(BATCH, prompt, np.int32))
    tokens = to_device(np.random.randint(0, cfg["vocab_size"], (BATCH, m)).astype(np.int32))
    at = to_device(np.tile(prompt + np.arange(m), (BATCH, 1)).astype(np.int32))
    count = to_device(np.full(BATCH, m, np.int32))
    step = lambda: model(tokens, cache=cache, append=True, count=count, token_positions=at)          # noqa: E731  (the position stays)
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
    ap.add_argument("--routes", default="launch,validation,step")
    ap.add_argument("--out")
    args = ap.parse_args()
    routes = args.routes.split(",")
    bert = load(ROOT)
    lines = []

    def say(text):
        print(text, flush=True)
        lines.append(text)

    def spread(xs):
        return "%.1f (%.1f .. %.1f)" % (np.median(xs), np.percentile(xs, 10), np.percentile(xs, 90))

    def compare(keys, m, forms):
        """forms: (label, B, shuffled, bf16), the contiguous entry in front; alternating inside every round"""
        us = {f[0]: [] for f in forms}
        for _ in range(args.rounds):
            for label, B, shuffled, bf16 in forms:
                us[label].append(measure_launch(keys, m, B, shuffled, bf16, args.iters))
        base = np.median(us[forms[0][0]])
        say("  keys = %5d  m = %2d  %s" % (keys, m, "   ".join("%s: %s x%.2f" % (f[0], spread(us[f[0]]), np.median(us[f[0]]) / base) for f in forms)))

    say("batch %d, 2 heads, d = 64; us, median (p10 .. p90) over %d rounds, and the ratio to the contiguous launch" % (BATCH, args.rounds))
    if "launch" in routes:
        for keys in KEYS:
            for m in ROWS:
                compare(keys, m, [("contiguous", None, False, False)] + [
                    ("B%d %s %s" % (B, "shuffled" if sh else "identity", "bf16" if bf else "fp32"), B, sh, bf)
                    for B in BLOCKS for sh in (False, True) for bf in (False, True)])
    if "validation" in routes:
        for m in ROWS:
            compare(16384, m, [("contiguous", None, False, False), ("B128 identity fp32", 128, False, False), ("B4 identity fp32", 4, False, False)])
    if "step" in routes:
        for m in (4, 32):
            res = {paged: [measure_step(bert, paged, 2000, m, args.iters) for _ in range(args.rounds)] for paged in (False, True)}
            say("  counted append step m = %2d behind 2000 of 2048  contiguous %s (%d kernels)   paged in blocks of 16 %s (%d kernels)   paged / contiguous %.2f" % (
                m, spread([r[0] for r in res[False]]), res[False][0][1], spread([r[0] for r in res[True]]), res[True][0][1],
                np.median([r[0] for r in res[True]]) / np.median([r[0] for r in res[False]])))
    if args.out:
        with open(args.out, "w") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
