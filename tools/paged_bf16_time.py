"""Time the bfloat16 key / value pools of the paged cache on the GPU against the float32 pools: the attention launch, a replayed
all-decode serving step, and `serve` over prompts with a common prefix at an equal number of blocks and at equal bytes.

    python tools/paged_bf16_time.py launch --kv bf16 | --kv f32 [--tree <a built checkout of another commit>] [--m 32] [--prefix 128]
                                           [--block 16] [--rounds 5] [--iters 200]
    python tools/paged_bf16_time.py step   --kv bf16 | --kv f32 [--tree ...] [--chunk 8] [--block 16] [--rounds 5] [--iters 200]
    python tools/paged_bf16_time.py prefix --kv bf16 | --kv f32 [--tree ...] [--blocks N] [--block 16] [--chunk 32] [--rounds 3]
    ... [--out FILE]   appends the printed lines to FILE

launch   us per launch, replayed from a graph of 32 launches (tools/paged_time.py's method): `extend_attention(count=, block_table=)`
         at (slots, heads, d) = (8, 2, 64), m new tokens behind a prefix of `--prefix`, capacity 512, every count = m, pools of
         8 * 512 / B blocks through shuffled tables.  f32: float32 pools, lg_attention_extend_paged_f32 (--tree: that commit's);
         bf16: int16 pools of bfloat16 words, lg_attention_extend_paged_bf16_f32
step     us per replayed step of the TINY causal model with 8 slots that all decode, from position 8 on (tools/paged_time.py's
         step), over an nn.PagedKVCache with float32 pools or with kv_dtype="bf16"
prefix   tools/paged_time.py's workload - 32 prompts = one common prefix of 64 tokens + 8 .. 64 tokens of their own, budgets of
         8 .. 64 new tokens, greedy, 8 slots, steps captured, shared_prefix=64 - with --blocks blocks in the pool (default: 8 slots'
         worth of the longest request): time, tokens/s, steps and `pool_bytes`.  The bf16 pools at the f32 run's blocks hold half
         its bytes; at twice the blocks, its bytes

--kv f32 passes no keyword, so --tree may name a checkout from before the bfloat16 pools.  Each measurement is to be made in two
processes; median and p10 .. p90 over the rounds.  Without a GPU everything fails; nothing here falls back."""
import argparse
import math
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
SLOTS = 8


def measure_launch(kv, B, m, t, iters, heads=2, d=64, capacity=512, per_graph=32):
    import numpy as np
    from decode_time import timed
    import lightgrad_amd as light
    from lightgrad_amd import HipTensor
    from lightgrad_amd.autograd.hip import HipGraph
    rng = np.random.RandomState(0)
    width = heads * d
    up = lambda a: HipTensor.from_numpy(np.ascontiguousarray(a), requires_grad=False)          # noqa: E731
    rows = rng.uniform(-1.5, 1.5, (2, SLOTS, capacity, width)).astype(np.float32)
    q, kn, vn = (up(rng.uniform(-1.5, 1.5, (SLOTS, m, width)).astype(np.float32)) for _ in range(3))
    pos, count = up(np.full(SLOTS, t, np.int32)), up(np.full(SLOTS, m, np.int32))
    per_slot = capacity // B
    words = np.random.RandomState(1).permutation(SLOTS * per_slot).reshape(SLOTS, per_slot).astype(np.int32)
    pools = np.zeros((2, SLOTS * per_slot, B, width), np.float32)
    for s in range(SLOTS):
        pools[:, words[s]] = rows[:, s].reshape(2, per_slot, B, width)
    extra = dict(count=count, block_table=up(words), block_size=B)
    if kv == "bf16":
        k, v = up(light.bf16_bits(pools[0])), up(light.bf16_bits(pools[1]))
        extra["kv_dtype"] = "bf16"
    else:
        k, v = up(pools[0]), up(pools[1])

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


def measure_step(bert, kv, model, chunk, B, iters, capacity=512, start=8):
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
    cache = nn.PagedKVCache(layers, SLOTS, SLOTS * capacity // B, B, width, capacity // B, like=like, **({"kv_dtype": "bf16"} if kv == "bf16" else {}))
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
    return us, kernels, cache.pool_bytes()


def measure_prefix(bert, kv, model, prompts, budgets, chunk, B, blocks):
    """(ms of the run, kernels of a captured step, steps, pool bytes, the requests' tokens)"""
    from paged_time import PREFIX
    from lightgrad_amd.autograd.hip import HipDevice, HipGraph
    options = dict(num_blocks=blocks, block_size=B, shared_prefix=PREFIX, **({"kv_dtype": "bf16"} if kv == "bf16" else {}))
    HipDevice.synchronize()
    t0 = time.perf_counter()
    graph = HipGraph()
    (out, out_len), stats = bert.serve(model, prompts, budgets, slots=SLOTS, chunk=chunk, graph=graph, **options)
    HipDevice.synchronize()
    ms = 1e3 * (time.perf_counter() - t0)
    kernels, steps = graph.kernel_count(), stats["steps"]
    graph.destroy()
    out = out.numpy()
    layers, width = bert.TINY["num_hidden_layers"], bert.TINY["hidden_size"]
    pool_bytes = stats.get("pool_bytes", 2 * layers * blocks * B * width * 4)          # (a tree from before the bfloat16 pools: float32)
    return ms, kernels, steps, pool_bytes, [out[r, :budgets[r]] for r in range(len(prompts))]


def main():
    import numpy as np
    from serve_time import load
    from paged_time import requests, pool_blocks, PREFIX
    ap = argparse.ArgumentParser()
    ap.add_argument("what", choices=["launch", "step", "prefix"])
    ap.add_argument("--kv", choices=["bf16", "f32"], default="bf16")
    ap.add_argument("--block", type=int, default=16)
    ap.add_argument("--blocks", type=int, default=None, help="prefix: blocks of the pool (default: 8 slots' worth of the longest request behind the shared ones)")
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
    if args.what == "launch":
        xs = [measure_launch(args.kv, args.block, args.m, args.prefix, args.iters) for _ in range(args.rounds)]
        say("tree %s  extend_attention(count=, block_table=) (8, 2, 64) m %d behind %d, capacity 512, blocks of %d, shuffled table, %s pools: %s us per launch, replayed; median (p10 .. p90) over %d rounds" % (
            name, args.m, args.prefix, args.block, args.kv, spread(xs), args.rounds))
    else:
        np.random.seed(0)
        model = bert.BertForMaskedLM(**dict(bert.TINY, causal=True)).eval().map_parameters(lambda p: p.hip())
        if args.what == "step":
            chunk = args.chunk or 8
            res = [measure_step(bert, args.kv, model, chunk, args.block, args.iters) for _ in range(args.rounds)]
            say("tree %s  step, %s pools (%d bytes), 8 slots decoding from position 8, %d token rows per slot, blocks of %d: %s us per replayed step; kernels of the step %d; median (p10 .. p90) over %d rounds" % (
                name, args.kv, res[0][2], chunk, args.block, spread([r[0] for r in res]), res[0][1], args.rounds))
        else:
            chunk = args.chunk or 32
            prompts, budgets = requests(bert)
            blocks = args.blocks or pool_blocks(prompts, budgets, args.block, True)[0]
            measure_prefix(bert, args.kv, model, prompts, budgets, chunk, args.block, blocks)             # untimed: kernels loaded, pool filled
            res = [measure_prefix(bert, args.kv, model, prompts, budgets, chunk, args.block, blocks) for _ in range(args.rounds)]
            ms = [r[0] for r in res]
            say("tree %s  prefix, %s pools, %d blocks of %d = %d bytes; %d prompts of %d .. %d tokens (the first %d common and shared), budgets %d .. %d (%d tokens), 8 slots, pieces of %d: %s ms; %.0f tokens/s at the median; %d steps; kernels of a captured step %d; median (p10 .. p90) over %d rounds" % (
                name, args.kv, blocks, args.block, res[0][3], len(prompts), min(map(len, prompts)), max(map(len, prompts)), PREFIX, min(budgets), max(budgets),
                sum(budgets), chunk, spread(ms), 1e3 * sum(budgets) / np.median(ms), res[0][2], res[0][1], args.rounds))
            say("  tokens of the requests (a checksum; the bf16 pools are NOT promised the float32 run's tokens): %s" % " ".join(str(int(np.sum(t))) for t in res[0][4]))
    if args.out:
        with open(args.out, "a") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
