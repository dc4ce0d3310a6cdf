"""Time the paged key / value cache on the GPU: the paged attention launch against the counts launch, a replayed paged serving
step against the counted one, and `serve` over prompts with a common prefix - paged with the prefix shared, paged without, unpaged.

    python tools/paged_time.py launch --form paged [--block 16] [--table identity|shuffled] | --form counts [--tree <a built checkout
                                      of another commit>] [--m 32] [--prefix 128] [--rounds 5] [--iters 200]
    python tools/paged_time.py step --route paged [--block 16] | --route serve [--tree ...] [--chunk 8] [--rounds 5] [--iters 200]
    python tools/paged_time.py prefix --route shared | --route paged | --route serve [--tree ...] [--block 16] [--blocks N] [--chunk 32] [--rounds 3]
    python tools/paged_time.py bytes [--block 16]
    ... [--out FILE]   appends the printed lines to FILE

launch   us per launch, replayed from a graph of 32 launches (tools/decode_time.py's method): `extend_attention(count=)` at
         (slots, heads, d) = (8, 2, 64), m new tokens behind a prefix of `--prefix`, capacity 512, every count = m.
           counts  on a contiguous (8, 512, 128) cache (lg_attention_extend_counts_f32; --tree: that commit's launch)
           paged   on pools of 8 * 512 / B blocks through tables of 512 / B words (lg_attention_extend_paged_f32): `identity` gives
                   slot s blocks s * 512 / B .., the rows lie where the contiguous cache has them; `shuffled` draws every word
                   from one permutation of the pool
step     us per replayed step of the TINY causal model with 8 slots that all decode, from position 8 on (tools/serve_time.py's
         step): `serve_step` with `chunk` token rows per slot, over an nn.PagedKVCache (paged) or an nn.KVCache (serve)
prefix   the TINY causal model, 32 prompts = one common prefix of 64 tokens + 8 .. 64 tokens of their own, budgets of 8 .. 64 new
         tokens (one seed), greedy, 8 slots, steps captured:
           shared  serve(num_blocks=, shared_prefix=64)      paged  serve(num_blocks=)      serve  serve() on a contiguous cache
         Wall time from the call to the synchronised end after one untimed run; tokens/s counts the sum of the budgets; the steps
         and a checksum of the tokens are printed.  The pool holds 8 slots' worth of the longest request's blocks, or --blocks.
bytes    arithmetic, no GPU: the pool bytes of the `prefix` runs against slots * capacity * width * 4 * 2 * layers

Median and p10 .. p90 over the rounds.  Without a GPU everything but `bytes` fails; nothing here falls back."""
import argparse
import math
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
SLOTS, REQUESTS, PREFIX = 8, 32, 64


def measure_launch(form, table, B, m, t, iters, heads=2, d=64, capacity=512, per_graph=32):
    import numpy as np
    from decode_time import timed
    from lightgrad_amd import HipTensor
    from lightgrad_amd.autograd.hip import HipGraph
    rng = np.random.RandomState(0)
    width = heads * d
    up = lambda a: HipTensor.from_numpy(np.ascontiguousarray(a), requires_grad=False)          # noqa: E731
    rows = rng.uniform(-1.5, 1.5, (2, SLOTS, capacity, width)).astype(np.float32)
    q, kn, vn = (up(rng.uniform(-1.5, 1.5, (SLOTS, m, width)).astype(np.float32)) for _ in range(3))
    pos, extra = up(np.full(SLOTS, t, np.int32)), {"count": up(np.full(SLOTS, m, np.int32))}
    if form == "paged":
        per_slot = capacity // B
        words = np.arange(SLOTS * per_slot) if table == "identity" else np.random.RandomState(1).permutation(SLOTS * per_slot)
        words = words.reshape(SLOTS, per_slot).astype(np.int32)
        pools = np.zeros((2, SLOTS * per_slot, B, width), np.float32)
        for s in range(SLOTS):
            pools[:, words[s]] = rows[:, s].reshape(2, per_slot, B, width)
        k, v = up(pools[0]), up(pools[1])
        extra.update(block_table=up(words), block_size=B)
    else:
        k, v = up(rows[0]), up(rows[1])

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


def measure_step(bert, route, model, chunk, B, iters, capacity=512, start=8):
    """(us per replayed step, kernels of the step): 8 sequences of `start` tokens, all decoding"""
    import numpy as np
    import lightgrad_amd as light
    import lightgrad_amd.nn as nn
    from decode_time import timed
    from lightgrad_amd.autograd.hip import HipGraph
    rng = np.random.RandomState(1)
    prompts = rng.randint(1, bert.TINY["vocab_size"], (SLOTS, start)).astype(np.int32)
    layer0 = model.bert.encoder.layer[0].attention.self
    layers, width, like = len(model.bert.encoder.layer), layer0.h * layer0.d, model.cls.predictions.bias
    if route == "paged":
        cache = nn.PagedKVCache(layers, SLOTS, SLOTS * capacity // B, B, width, capacity // B, like=like)
    else:
        cache = nn.KVCache(layers, SLOTS, capacity, width, like=like, per_row=True)
    graph = HipGraph()
    with light.no_grad():
        pool = nn.RequestPool(cache, prompts, [start] * SLOTS, [capacity - start] * SLOTS, chunk)
        pool.admit()
        for _ in range(-(-start // chunk) + 1):                           # the prompts, then one decoding step: kernels loaded
            bert.serve_step(model, pool)
        assert pool.count.numpy().tolist() == [1] * SLOTS
        with graph.capture():
            bert.serve_step(model, pool)
    assert 20 + iters + start + 4 < capacity
    us = timed(graph.replay, iters)
    kernels = graph.kernel_count()
    graph.destroy()
    return us, kernels


def requests(bert):
    import numpy as np
    rng = np.random.RandomState(0)
    common = rng.randint(1, bert.TINY["vocab_size"], PREFIX).astype(np.int32)
    lengths, budgets = rng.randint(8, 65, REQUESTS), rng.randint(8, 65, REQUESTS)
    return [np.concatenate([common, rng.randint(1, bert.TINY["vocab_size"], n).astype(np.int32)]) for n in lengths], [int(x) for x in budgets]


def pool_blocks(prompts, budgets, B, shared):
    """blocks of the pool: 8 slots' worth of the longest request's need behind the shared blocks, and the shared blocks"""
    F = min(PREFIX // B, (min(map(len, prompts)) - 1) // B) if shared else 0
    need = max(-(-(len(p) + n - 1) // B) for p, n in zip(prompts, budgets)) - F
    return F + SLOTS * need, F


def measure_prefix(bert, route, model, prompts, budgets, chunk, B, blocks=None):
    """(ms of the run, kernels of a captured step, steps, the requests' tokens)"""
    from lightgrad_amd.autograd.hip import HipDevice, HipGraph
    options = {}
    if route != "serve":
        options = dict(num_blocks=blocks or pool_blocks(prompts, budgets, B, route == "shared")[0], block_size=B, shared_prefix=PREFIX if route == "shared" else 0)
    HipDevice.synchronize()
    t0 = time.perf_counter()
    graph = HipGraph()
    (out, out_len), stats = bert.serve(model, prompts, budgets, slots=SLOTS, chunk=chunk, graph=graph, **options)
    HipDevice.synchronize()
    ms = 1e3 * (time.perf_counter() - t0)
    kernels, steps = graph.kernel_count(), stats["steps"]
    graph.destroy()
    out = out.numpy()
    return ms, kernels, steps, [out[r, :budgets[r]] for r in range(len(prompts))]


def main():
    import numpy as np
    from serve_time import load
    ap = argparse.ArgumentParser()
    ap.add_argument("what", choices=["launch", "step", "prefix", "bytes"])
    ap.add_argument("--form", choices=["paged", "counts"], default="paged")
    ap.add_argument("--table", choices=["identity", "shuffled"], default="shuffled")
    ap.add_argument("--route", choices=["paged", "shared", "serve"], default="paged")
    ap.add_argument("--block", type=int, default=16)
    ap.add_argument("--blocks", type=int, default=None, help="prefix: blocks of the pool (default: 8 slots' worth of the longest request)")
    ap.add_argument("--m", type=int, default=32)
    ap.add_argument("--prefix", type=int, default=128)
    ap.add_argument("--chunk", type=int, default=None)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--tree", default=ROOT, help="import lightgrad_amd and examples/bert.py from this tree")
    ap.add_argument("--out")
    args = ap.parse_args()
    tree = os.path.abspath(args.tree)
    bert = load(tree)
    lines = []

    def say(text):
        print(text, flush=True)
        lines.append(text)

    def spread(xs):
        return "%.2f (%.2f .. %.2f)" % (np.median(xs), np.percentile(xs, 10), np.percentile(xs, 90))

    name = os.path.relpath(tree, ROOT)
    if args.what == "bytes":
        prompts, budgets = requests(bert)
        layers, width = bert.TINY["num_hidden_layers"], bert.TINY["hidden_size"]
        capacity = max(len(p) + n - 1 for p, n in zip(prompts, budgets))
        flat = SLOTS * capacity * width * 4 * 2 * layers
        say("contiguous cache: %d slots x %d positions x %d floats x 4 bytes x 2 (k, v) x %d layers = %d bytes" % (SLOTS, capacity, width, layers, flat))
        for shared in (False, True):
            blocks, F = pool_blocks(prompts, budgets, args.block, shared)
            pool = blocks * args.block * width * 4 * 2 * layers
            say("paged, blocks of %d%s: %d blocks (%d shared) = %d bytes, %.2f of the contiguous cache" % (
                args.block, ", shared_prefix = %d" % PREFIX if shared else "", blocks, F, pool, pool / flat))
    elif args.what == "launch":
        xs = [measure_launch(args.form, args.table, args.block, args.m, args.prefix, args.iters) for _ in range(args.rounds)]
        form = "paged, blocks of %d, %s table" % (args.block, args.table) if args.form == "paged" else "contiguous cache (_counts entry)"
        say("tree %s  extend_attention(count=) (8, 2, 64) m %d behind %d, capacity 512, %s: %s us per launch, replayed; median (p10 .. p90) over %d rounds" % (
            name, args.m, args.prefix, form, spread(xs), args.rounds))
    else:
        np.random.seed(0)
        model = bert.BertForMaskedLM(**dict(bert.TINY, causal=True)).eval().map_parameters(lambda p: p.hip())
        if args.what == "step":
            chunk = args.chunk or 8
            res = [measure_step(bert, args.route, model, chunk, args.block, args.iters) for _ in range(args.rounds)]
            say("tree %s  step %-5s 8 slots decoding from position 8, %d token rows per slot%s: %s us per replayed step; kernels of the step %d; median (p10 .. p90) over %d rounds" % (
                name, args.route, chunk, ", blocks of %d" % args.block if args.route == "paged" else "", spread([r[0] for r in res]), res[0][1], args.rounds))
        else:
            chunk = args.chunk or 32
            prompts, budgets = requests(bert)
            measure_prefix(bert, args.route, model, prompts, budgets, chunk, args.block, args.blocks)             # untimed: kernels loaded, pool filled
            res = [measure_prefix(bert, args.route, model, prompts, budgets, chunk, args.block, args.blocks) for _ in range(args.rounds)]
            ms = [r[0] for r in res]
            say("tree %s  prefix %-6s %d prompts of %d .. %d tokens (the first %d common), budgets %d .. %d (%d tokens), 8 slots, pieces of %d%s: %s ms; %.0f tokens/s at the median; %d steps; kernels of a captured step %d; median (p10 .. p90) over %d rounds" % (
                name, args.route, len(prompts), min(map(len, prompts)), max(map(len, prompts)), PREFIX, min(budgets), max(budgets), sum(budgets), chunk,
                ", %d blocks of %d" % (args.blocks or pool_blocks(prompts, budgets, args.block, args.route == "shared")[0], args.block) if args.route != "serve" else "", spread(ms), 1e3 * sum(budgets) / np.median(ms), res[0][2], res[0][1], args.rounds))
            say("  tokens of the requests (a checksum to hold the routes against each other): %s" % " ".join(str(int(np.sum(t))) for t in res[0][3]))
    if args.out:
        with open(args.out, "a") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
