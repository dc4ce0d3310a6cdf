"""Time continuous batching on the GPU: the counts launch against the `_rows` launch, a replayed serving step against the captured
per-row decode step, and `serve` against `generate(lengths=)` in waves.

    python tools/serve_time.py launch [--counts] [--tree <a built checkout of another commit>] [--rounds 5] [--iters 200]
    python tools/serve_time.py step --route serve [--chunk 8] | --route rows [--tree ...] [--rounds 5] [--iters 200]
    python tools/serve_time.py throughput --route serve [--chunk 32] | --route waves [--tree ...] [--rounds 3]
    ... [--out FILE]   appends the printed lines to FILE

launch      us per launch, replayed from a graph of 32 launches (tools/decode_time.py's method): `extend_attention` at (b, heads, d) =
            (8, 2, 64), m = 32 new tokens behind a prefix of 128, capacity 512, 8 position words that hold the same t
            (lg_attention_extend_rows_f32 - with --tree: that commit's launch); with --counts also 8 count words that all hold m
            (lg_attention_extend_counts_f32): the same work, so any difference is what the count costs.  Run the `_rows` form in
            two processes: their difference is the noise the comparison has to be read against.
step        us per replayed step of the TINY causal model with 8 sequences that all decode, from position 8 on:
              serve  `serve_step` with `chunk` token rows per slot of which one is real (count = 1 everywhere)
              rows   `decode_step_rows`, the captured per-row decode step (--tree: that commit's)
            Both walk the same positions (20 warm-up replays, then --iters timed ones).  The kernel count of the step is printed.
throughput  the TINY causal model, 32 prompts of 16 .. 128 tokens with budgets of 8 .. 128 new tokens (one seed), greedy, no
            end-of-sequence id, steps captured:
              serve  ONE `serve` with 8 slots
              waves  four `generate(lengths=)` calls over 8 prompts each in the order given, each run to its wave's largest budget -
                     the only route of a tree without a request queue (--tree)
            Wall time from the call to the synchronised end after one untimed run of the same calls; tokens/s counts the tokens
            the requests asked for (the sum of the budgets).

Median and p10 .. p90 over the rounds.  Without a GPU this fails; nothing here falls back."""
import argparse
import importlib.util
import math
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
SLOTS, REQUESTS = 8, 32


def load(tree):
    sys.path.insert(0, tree)
    spec = importlib.util.spec_from_file_location("bert_example_timing", os.path.join(tree, "examples", "bert.py"))
    bert = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(bert)
    return bert


def measure_launch(counts, iters, heads=2, d=64, capacity=512, m=32, t=128, per_graph=32):
    import numpy as np
    from decode_time import timed
    from lightgrad_amd import HipTensor
    from lightgrad_amd.autograd.hip import HipGraph
    rng = np.random.RandomState(0)
    width = heads * d
    k, v = (HipTensor.from_numpy(rng.uniform(-1.5, 1.5, (SLOTS, capacity, width)).astype(np.float32), requires_grad=False) for _ in range(2))
    q, kn, vn = (HipTensor.from_numpy(rng.uniform(-1.5, 1.5, (SLOTS, m, width)).astype(np.float32), requires_grad=False) for _ in range(3))
    pos = HipTensor.from_numpy(np.full(SLOTS, t, np.int32), requires_grad=False)
    extra = {"count": HipTensor.from_numpy(np.full(SLOTS, m, np.int32), requires_grad=False)} if counts else {}

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


def measure_step(bert, route, model, chunk, iters, capacity=512, start=8):
    """(us per replayed step, kernels of the step): 8 sequences of `start` tokens, all decoding"""
    import numpy as np
    import lightgrad_amd as light
    import lightgrad_amd.nn as nn
    from decode_time import timed
    from lightgrad_amd import HipTensor
    from lightgrad_amd.autograd.hip import HipGraph
    rng = np.random.RandomState(1)
    prompts = rng.randint(1, bert.TINY["vocab_size"], (SLOTS, start)).astype(np.int32)
    layer0 = model.bert.encoder.layer[0].attention.self
    cache = nn.KVCache(len(model.bert.encoder.layer), SLOTS, capacity, layer0.h * layer0.d, like=model.cls.predictions.bias, per_row=True)
    graph = HipGraph()
    with light.no_grad():
        if route == "serve":
            pool = nn.RequestPool(cache, prompts, [start] * SLOTS, [capacity - start] * SLOTS, chunk)
            pool.admit()
            for _ in range(-(-start // chunk) + 1):                       # the prompts, then one decoding step: kernels loaded
                bert.serve_step(model, pool)
            assert pool.count.numpy().tolist() == [1] * SLOTS
            with graph.capture():
                bert.serve_step(model, pool)
        else:
            model(HipTensor.from_numpy(prompts, requires_grad=False), cache=cache)
            cache.set_lengths([start] * SLOTS)
            token = HipTensor.from_numpy(prompts[:, -1:].copy(), requires_grad=False)
            out_ids = HipTensor.from_numpy(np.zeros((SLOTS, capacity), np.int32), requires_grad=False)
            done = HipTensor.from_numpy(np.zeros(SLOTS, np.int32), requires_grad=False)
            bert.decode_step_rows(model, cache, token, out_ids, done)
            with graph.capture():
                bert.decode_step_rows(model, cache, token, out_ids, done)
    assert 20 + iters + start + 4 < capacity
    us = timed(graph.replay, iters)
    kernels = graph.kernel_count()
    graph.destroy()
    return us, kernels


def requests(bert):
    import numpy as np
    rng = np.random.RandomState(0)
    lengths = rng.randint(16, 129, REQUESTS)
    budgets = rng.randint(8, 129, REQUESTS)
    return [rng.randint(1, bert.TINY["vocab_size"], n).astype(np.int32) for n in lengths], [int(x) for x in budgets]


def measure_throughput(bert, route, model, prompts, budgets, chunk):
    """(ms of the whole route, kernels of a captured step, steps or None, the requests' tokens)"""
    import numpy as np
    import lightgrad_amd as light
    from lightgrad_amd.autograd.hip import HipDevice, HipGraph
    to_device = lambda a: light.from_numpy(a, requires_grad=False).hip(requires_grad=False)          # noqa: E731
    HipDevice.synchronize()
    t0 = time.perf_counter()
    if route == "serve":
        graph = HipGraph()
        (out, out_len), stats = bert.serve(model, prompts, budgets, slots=SLOTS, chunk=chunk, graph=graph)
        HipDevice.synchronize()
        ms = 1e3 * (time.perf_counter() - t0)
        kernels, steps = graph.kernel_count(), stats["steps"]
        graph.destroy()
        out = out.numpy()
        return ms, kernels, steps, [out[r, :budgets[r]] for r in range(len(prompts))]
    graphs, outs = [], []
    for lo in range(0, len(prompts), SLOTS):
        wave, new = prompts[lo:lo + SLOTS], max(budgets[lo:lo + SLOTS])
        padded = np.zeros((len(wave), max(len(p) for p in wave)), np.int32)
        for r, p in enumerate(wave):
            padded[r, :len(p)] = p
        graphs.append(HipGraph())
        outs.append(bert.generate(model, to_device(padded), new, lengths=[len(p) for p in wave], graph=graphs[-1]))
    HipDevice.synchronize()
    ms = 1e3 * (time.perf_counter() - t0)
    kernels = graphs[0].kernel_count()
    tokens = []
    for w, o in enumerate(outs):
        o = o.numpy()
        for r in range(o.shape[0]):
            i = w * SLOTS + r
            tokens.append(o[r, len(prompts[i]):len(prompts[i]) + budgets[i]])
    for g in graphs:
        g.destroy()
    return ms, kernels, None, tokens


def main():
    import numpy as np
    ap = argparse.ArgumentParser()
    ap.add_argument("what", choices=["launch", "step", "throughput"])
    ap.add_argument("--counts", action="store_true")
    ap.add_argument("--route", choices=["serve", "rows", "waves"], default="serve")
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
        xs = [measure_launch(args.counts, args.iters) for _ in range(args.rounds)]
        say("tree %s  extend_attention (8, 2, 64) m 32 behind 128, capacity 512, %s: %s us per launch, replayed; median (p10 .. p90) over %d rounds" % (
            name, "8 position and 8 count words (_counts entry, count = m)" if args.counts else "8 position words (_rows entry)", spread(xs), args.rounds))
    else:
        np.random.seed(0)
        model = bert.BertForMaskedLM(**dict(bert.TINY, causal=True)).eval().map_parameters(lambda p: p.hip())
        if args.what == "step":
            chunk = args.chunk or 8
            res = [measure_step(bert, args.route, model, chunk, args.iters) for _ in range(args.rounds)]
            say("tree %s  step %-5s 8 sequences decoding from position 8%s: %s us per replayed step; kernels of the step %d; median (p10 .. p90) over %d rounds" % (
                name, args.route, ", %d token rows per slot" % chunk if args.route == "serve" else "", spread([r[0] for r in res]), res[0][1], args.rounds))
        else:
            chunk = args.chunk or 32
            prompts, budgets = requests(bert)
            route = "serve" if args.route == "serve" else "waves"
            measure_throughput(bert, route, model, prompts, budgets, chunk)             # untimed: kernels loaded, pool filled
            res = [measure_throughput(bert, route, model, prompts, budgets, chunk) for _ in range(args.rounds)]
            ms = [r[0] for r in res]
            say("tree %s  throughput %-5s %d prompts of %d .. %d tokens, budgets %d .. %d (%d tokens)%s: %s ms; %.0f tokens/s at the median; kernels of a captured step %d%s; median (p10 .. p90) over %d rounds" % (
                name, route, len(prompts), min(map(len, prompts)), max(map(len, prompts)), min(budgets), max(budgets), sum(budgets),
                ", 8 slots, pieces of %d" % chunk if route == "serve" else ", 4 waves of 8", spread(ms), 1e3 * sum(budgets) / np.median(ms), res[0][1],
                "; %d steps" % res[0][2] if res[0][2] else "", args.rounds))
            say("  tokens of the requests (a checksum to hold the two routes against each other): %s" % " ".join(str(int(np.sum(t))) for t in res[0][3]))
    if args.out:
        with open(args.out, "a") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
