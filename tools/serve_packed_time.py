"""Time token-packed serving steps on the GPU: the packed attention launch against the `_counts` launch, a replayed packed step with
every slot decoding against the (slots, chunk) step and the captured per-row decode step, `serve(token_budget=)` against `serve`,
and the packed commit launch against the commit launch.

    python tools/serve_packed_time.py launch --route packed | --route counts [--tree <a built checkout of another commit>]
    python tools/serve_packed_time.py step --route packed --chunk 8 | --route serve --chunk 8 | --route rows [--tree ...]
    python tools/serve_packed_time.py throughput --route packed --chunk 32 | --route serve --chunk 32 [--tree ...]
    python tools/serve_packed_time.py commit --route packed | --route serve [--chunk 32] [--tree ...]
    ... [--rounds 5] [--iters 200] [--out FILE]   appends the printed lines to FILE

launch      us per launch, replayed from a graph of 32 launches (tools/decode_time.py's method), at the shape of
            tools/serve_time.py: 8 slots, (heads, d) = (2, 64), 32 new tokens per slot behind a prefix of 128, capacity 512
              packed  `extend_attention(cu=)` on (1, 256, 128) rows, cu = 0, 32, .., 256, m_max = 32 (lg_attention_extend_packed_f32)
              counts  `extend_attention(count=)` on (8, 32, 128) rows, every count = 32 (lg_attention_extend_counts_f32; --tree: that
                      commit's launch)
            The same work: any difference is what the flat layout and the clearing slice of the grid cost.
step        us per replayed step of the TINY causal model with 8 sequences that all decode, from position 8 on:
              packed  `serve_step` on a pool with token_budget = 8 + chunk: 8 + chunk token rows, 8 of them real
              serve   `serve_step` with `chunk` token rows per slot of which one is real (tools/serve_time.py's; --tree)
              rows    `decode_step_rows`, the captured per-row decode step (--tree)
throughput  tools/serve_time.py's workload - 32 prompts of 16 .. 128 tokens with budgets of 8 .. 128, greedy, steps captured -
            through 8 slots:
              packed  ONE `serve(token_budget = 8 + chunk)`
              serve   ONE `serve` (--tree)
commit      us per launch, replayed from a graph of 32 launches, of the commit alone on 8 slots that all decode:
              packed  lg_serve_commit_packed_i32 with T = 8 + chunk
              serve   lg_serve_commit_i32 with m = chunk (--tree)

Median and p10 .. p90 over the rounds.  Without a GPU this fails; nothing here falls back."""
import argparse
import math
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import serve_time as st                                                   # noqa: E402

SLOTS = st.SLOTS


def measure_launch_packed(iters, heads=2, d=64, capacity=512, m=32, t=128, per_graph=32):
    import numpy as np
    from decode_time import timed
    from lightgrad_amd import HipTensor
    from lightgrad_amd.autograd.hip import HipGraph
    rng = np.random.RandomState(0)
    width = heads * d
    k, v = (HipTensor.from_numpy(rng.uniform(-1.5, 1.5, (SLOTS, capacity, width)).astype(np.float32), requires_grad=False) for _ in range(2))
    q, kn, vn = (HipTensor.from_numpy(rng.uniform(-1.5, 1.5, (1, SLOTS * m, width)).astype(np.float32), requires_grad=False) for _ in range(3))
    pos = HipTensor.from_numpy(np.full(SLOTS, t, np.int32), requires_grad=False)
    cu = HipTensor.from_numpy((m * np.arange(SLOTS + 1)).astype(np.int32), requires_grad=False)

    def launches():
        for _ in range(per_graph):
            q.extend_attention(kn, vn, k, v, pos, heads=heads, scale=math.sqrt(d) ** -1, cu=cu, m_max=m)
    launches()
    graph = HipGraph()
    with graph.capture():
        launches()
    us = timed(graph.replay, max(1, iters // 4)) / per_graph
    graph.destroy()
    return us


def measure_step_packed(bert, model, chunk, iters, capacity=512, start=8):
    """(us per replayed step, kernels of the step): 8 sequences of `start` tokens, all decoding, 8 + chunk token rows"""
    import numpy as np
    import lightgrad_amd as light
    import lightgrad_amd.nn as nn
    from decode_time import timed
    from lightgrad_amd.autograd.hip import HipGraph
    rng = np.random.RandomState(1)
    prompts = rng.randint(1, bert.TINY["vocab_size"], (SLOTS, start)).astype(np.int32)
    layer0 = model.bert.encoder.layer[0].attention.self
    cache = nn.KVCache(len(model.bert.encoder.layer), SLOTS, capacity, layer0.h * layer0.d, like=model.cls.predictions.bias, per_row=True)
    graph = HipGraph()
    with light.no_grad():
        pool = nn.RequestPool(cache, prompts, [start] * SLOTS, [capacity - start] * SLOTS, chunk, token_budget=SLOTS + chunk)
        pool.admit()
        for _ in range(SLOTS * start):                                    # the prompts under the budget, then decoding steps: kernels loaded
            bert.serve_step(model, pool)
            if pool.count.numpy().tolist() == [1] * SLOTS and (pool.pos.numpy() >= start).all():
                break
        assert pool.count.numpy().tolist() == [1] * SLOTS and pool.cu.numpy().tolist() == list(range(SLOTS + 1))
        with graph.capture():
            bert.serve_step(model, pool)
    assert 20 + iters + 2 * start + SLOTS + 4 < capacity
    us = timed(graph.replay, iters)
    kernels = graph.kernel_count()
    graph.destroy()
    return us, kernels


def measure_throughput_packed(bert, model, prompts, budgets, chunk):
    """(ms of the whole route, kernels of a captured step, steps, the requests' tokens)"""
    from lightgrad_amd.autograd.hip import HipDevice, HipGraph
    HipDevice.synchronize()
    t0 = time.perf_counter()
    graph = HipGraph()
    (out, out_len), stats = bert.serve(model, prompts, budgets, slots=SLOTS, chunk=chunk, graph=graph, token_budget=SLOTS + chunk)
    HipDevice.synchronize()
    ms = 1e3 * (time.perf_counter() - t0)
    kernels, steps = graph.kernel_count(), stats["steps"]
    graph.destroy()
    out = out.numpy()
    return ms, kernels, steps, [out[r, :budgets[r]] for r in range(len(prompts))]


def measure_commit(route, chunk, iters, capacity=512, start=8, per_graph=32):
    """us per commit launch on 8 slots that all decode; the launches of a graph walk 32 positions, every replay the same ones"""
    import numpy as np
    from decode_time import timed
    from lightgrad_amd import HipTensor
    from lightgrad_amd.autograd.hip import HipGraph
    i32 = lambda a: HipTensor.from_numpy(np.ascontiguousarray(a, np.int32), requires_grad=False)          # noqa: E731
    G = capacity
    prompts, prompt_len, budget = i32(np.ones((SLOTS, start))), i32(np.full(SLOTS, start)), i32(np.full(SLOTS, G + 1))
    out, out_len, queue, req = i32(np.zeros((SLOTS, G))), i32(np.zeros(SLOTS)), i32([SLOTS, 0]), i32(np.arange(SLOTS))
    pos, count, last, nxt = i32(np.full(SLOTS, start - 1)), i32(np.ones(SLOTS)), i32(np.zeros(SLOTS)), i32(np.full(SLOTS, 5))
    T = SLOTS + chunk
    if route == "packed":
        ids, position_ids, cu = i32(np.zeros((1, T))), i32(np.zeros((1, T))), i32(np.zeros(SLOTS + 1))
    else:
        ids, position_ids = i32(np.zeros((SLOTS, chunk))), i32(np.zeros((SLOTS, chunk)))
    zeros, first = i32(np.zeros(SLOTS)), i32(np.full(SLOTS, start - 1))

    def launches():
        # back to the first position: the replays of the graph never leave out or the cache
        out_len[:] = zeros
        pos[:] = first
        for _ in range(per_graph):
            if route == "packed":
                nxt.serve_commit_packed(prompts, prompt_len, budget, out, out_len, queue, req, pos, count, cu, ids, position_ids, last, capacity, chunk)
            else:
                nxt.serve_commit(prompts, prompt_len, budget, out, out_len, queue, req, pos, count, ids, position_ids, last, capacity)
    launches()
    assert count.numpy().tolist() == [1] * SLOTS and pos.numpy().tolist() == [start - 1 + per_graph] * SLOTS
    graph = HipGraph()
    with graph.capture():
        launches()
    kernels = graph.kernel_count()
    us = timed(graph.replay, max(1, iters // 4)) / per_graph
    graph.destroy()
    return us, kernels - per_graph


def main():
    import numpy as np
    ap = argparse.ArgumentParser()
    ap.add_argument("what", choices=["launch", "step", "throughput", "commit"])
    ap.add_argument("--route", choices=["packed", "counts", "serve", "rows"], default="packed")
    ap.add_argument("--chunk", type=int, default=None)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--tree", default=ROOT, help="import lightgrad_amd and examples/bert.py from this tree")
    ap.add_argument("--out")
    args = ap.parse_args()
    tree = os.path.abspath(args.tree)
    bert = st.load(tree)
    lines = []

    def say(text):
        print(text, flush=True)
        lines.append(text)

    def spread(xs):
        return "%.2f (%.2f .. %.2f)" % (np.median(xs), np.percentile(xs, 10), np.percentile(xs, 90))

    name = os.path.relpath(tree, ROOT)
    if args.what == "launch":
        assert args.route in ("packed", "counts")
        xs = [measure_launch_packed(args.iters) if args.route == "packed" else st.measure_launch(True, args.iters) for _ in range(args.rounds)]
        say("tree %s  extend_attention 8 slots (2, 64) 32 tokens each behind 128, capacity 512, %s: %s us per launch, replayed; median (p10 .. p90) over %d rounds" % (
            name, "(1, 256, 128) rows and 9 words of cu (_packed entry)" if args.route == "packed" else "(8, 32, 128) rows and 8 count words (_counts entry, count = m)",
            spread(xs), args.rounds))
    elif args.what == "commit":
        assert args.route in ("packed", "serve")
        chunk = args.chunk or 32
        res = [measure_commit(args.route, chunk, args.iters) for _ in range(args.rounds)]
        say("tree %s  commit %-6s 8 slots decoding, %s: %s us per launch, replayed; %d other kernels in the graph of 32; median (p10 .. p90) over %d rounds" % (
            name, args.route, "T = %d token rows" % (SLOTS + chunk) if args.route == "packed" else "%d token rows per slot" % chunk,
            spread([r[0] for r in res]), res[0][1], args.rounds))
    else:
        np.random.seed(0)
        model = bert.BertForMaskedLM(**dict(bert.TINY, causal=True)).eval().map_parameters(lambda p: p.hip())
        if args.what == "step":
            chunk = args.chunk or 8
            if args.route == "packed":
                res = [measure_step_packed(bert, model, chunk, args.iters) for _ in range(args.rounds)]
                shape = ", %d token rows for all slots" % (SLOTS + chunk)
            else:
                res = [st.measure_step(bert, args.route, model, chunk, args.iters) for _ in range(args.rounds)]
                shape = ", %d token rows per slot" % chunk if args.route == "serve" else ""
            say("tree %s  step %-6s 8 sequences decoding from position 8%s: %s us per replayed step; kernels of the step %d; median (p10 .. p90) over %d rounds" % (
                name, args.route, shape, spread([r[0] for r in res]), res[0][1], args.rounds))
        else:
            assert args.route in ("packed", "serve")
            chunk = args.chunk or 32
            prompts, budgets = st.requests(bert)
            run = (lambda: measure_throughput_packed(bert, model, prompts, budgets, chunk)) if args.route == "packed" else \
                (lambda: st.measure_throughput(bert, "serve", model, prompts, budgets, chunk))
            run()                                                         # untimed: kernels loaded, pool filled
            res = [run() for _ in range(args.rounds)]
            ms = [r[0] for r in res]
            say("tree %s  throughput %-6s %d prompts of %d .. %d tokens, budgets %d .. %d (%d tokens), 8 slots, pieces of %d%s: %s ms; %.0f tokens/s at the median; kernels of a captured step %d; %d steps; median (p10 .. p90) over %d rounds" % (
                name, args.route, len(prompts), min(map(len, prompts)), max(map(len, prompts)), min(budgets), max(budgets), sum(budgets), chunk,
                " under %d token rows a step" % (SLOTS + chunk) if args.route == "packed" else "", spread(ms), 1e3 * sum(budgets) / np.median(ms), res[0][1],
                res[0][2], args.rounds))
            say("  tokens of the requests (a checksum to hold the two routes against each other): %s" % " ".join(str(int(np.sum(t))) for t in res[0][3]))
    if args.out:
        with open(args.out, "a") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
