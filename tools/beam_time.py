"""Time beam search on the GPU against the captured per-row decode step of `generate(lengths=)`.

    python tools/beam_time.py step --route beam --w 4 | --route rows [--tree <a built checkout of another commit>]
    python tools/beam_time.py select --w 8 --vocab 30522
    python tools/beam_time.py reorder --w 4 --prefix 500 --parent cycle|identity
    python tools/beam_time.py call --route beam --w 4 | --route rows [--tree ...]
    ... [--rounds 5] [--iters 200] [--out FILE]   appends the printed lines to FILE

step     us per replayed step of the TINY causal model, 8 rows behind a prefix of 128 tokens, capacity 512:
           beam  `beam_search_step` with 8 / w prompts of w beams each (the decode forward at batch 8, one beam_step, one reorder)
           rows  `decode_step_rows`, the captured per-row decode step at batch 8 (--tree: that commit's)
         Both walk the same positions (20 warm-up replays, then --iters timed ones).  The kernel count of the step is printed.
select   us per `beam_step` launch alone on 8 rows of random logits (8 / w groups), beside `sample` (temperature 1, no filter) on the
         same rows: both read every logit once.  A graph of one restoring copy per written operand and 8 launches, over 8.
reorder  us per `KVCache.reorder` launch alone, TINY's cache (2 layers, width 128), 8 rows at position `prefix`, a cycle or the
         identity as parents, with the bytes moved (2 * layers * rows * prefix * width * 4 read, the same written) per second.
call     `generate(num_beams=w)` for 8 prompts of 64 tokens and 64 new ones, the step captured, against `generate(lengths=)` of
         8 * w rows (--route rows; --tree: that commit's): wall time from the call to the synchronised end after one untimed run.

Median and p10 .. p90 over the rounds.  Run every command under its own `timeout -k 10 <seconds>` and chain them with `&&`.
Without a GPU this fails; nothing here falls back."""
import argparse
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
from serve_time import load  # noqa: E402

ROWS, PREFIX, CAPACITY, NEW, PROMPT = 8, 128, 512, 64, 64


def measure_step(bert, route, model, w, iters):
    """(us per replayed step, kernels of the step): 8 rows of PREFIX tokens"""
    import numpy as np
    import lightgrad_amd as light
    import lightgrad_amd.nn as nn
    from decode_time import timed
    from lightgrad_amd import HipTensor
    from lightgrad_amd.autograd.hip import HipGraph
    rng = np.random.RandomState(1)
    prompts = rng.randint(1, bert.TINY["vocab_size"], (ROWS, PREFIX)).astype(np.int32)
    layer0 = model.bert.encoder.layer[0].attention.self
    cache = nn.KVCache(len(model.bert.encoder.layer), ROWS, CAPACITY, layer0.h * layer0.d, like=model.cls.predictions.bias, per_row=True)
    i32 = lambda a: HipTensor.from_numpy(np.ascontiguousarray(a, np.int32), requires_grad=False)       # noqa: E731
    graph = HipGraph()
    assert PREFIX + 20 + iters + 4 < CAPACITY
    with light.no_grad():
        model(i32(prompts), cache=cache)
        cache.set_lengths([PREFIX] * ROWS)
        out_ids = i32(np.zeros((ROWS, CAPACITY)))
        out_ids[:, :PREFIX] = i32(prompts)
        token = i32(prompts[:, -1:].copy())
        done = i32(np.zeros(ROWS))
        if route == "beam":
            cache.num_beams = w
            state = dict(token=token, out_ids=out_ids, done=done, parent=i32(np.arange(ROWS)), stats=i32(np.zeros(2)),
                         scores=HipTensor.from_numpy(-rng.uniform(0, 1, ROWS).astype(np.float32), requires_grad=False))
            bert.beam_search_step(model, cache, state, w)
            with graph.capture():
                bert.beam_search_step(model, cache, state, w)
        else:
            bert.decode_step_rows(model, cache, token, out_ids, done)
            with graph.capture():
                bert.decode_step_rows(model, cache, token, out_ids, done)
    us = timed(graph.replay, iters)
    kernels = graph.kernel_count()
    graph.destroy()
    return us, kernels


def measure_select(w, vocab, iters, per_graph=8):
    """(us per beam_step launch, us per sample launch) on the same 8 rows of logits"""
    import numpy as np
    from decode_time import timed
    from lightgrad_amd import HipTensor
    from lightgrad_amd.autograd.hip import HipGraph
    rng = np.random.RandomState(2)
    tensor = lambda a: HipTensor.from_numpy(np.ascontiguousarray(a), requires_grad=False)          # noqa: E731
    logits = tensor((rng.standard_normal((ROWS, vocab)) * 4).astype(np.float32))
    fresh = dict(scores=-rng.uniform(0, 8, ROWS).astype(np.float32), parent=np.arange(ROWS, dtype=np.int32), token=np.zeros((ROWS, 1), np.int32),
                 out_ids=np.zeros((ROWS, 64), np.int32), pos=np.full(ROWS, 8, np.int32), done=np.zeros(ROWS, np.int32), stats=np.zeros(2, np.int32))
    state, saved = {k: tensor(v) for k, v in fresh.items()}, tensor(fresh["pos"])

    def launches():
        state["pos"][:] = saved                                             # the positions go back: no row reaches its last column
        for _ in range(per_graph):
            logits.beam_step(state["scores"], state["parent"], state["token"], state["out_ids"], state["pos"], state["done"], state["stats"], w)
    launches()
    graph = HipGraph()
    with graph.capture():
        launches()
    beam_us = timed(graph.replay, max(1, iters // 4)) / per_graph
    graph.destroy()

    def draws():
        for _ in range(per_graph):
            logits.sample(temperature=1.0, dtype=np.int32)
    draws()
    graph = HipGraph()
    with graph.capture():
        draws()
    sample_us = timed(graph.replay, max(1, iters // 4)) / per_graph
    graph.destroy()
    return beam_us, sample_us


def measure_reorder(bert, w, prefix, kind, iters, per_graph=8):
    """us per reorder launch: TINY's cache, 8 rows at position `prefix`"""
    import numpy as np
    import lightgrad_amd.nn as nn
    from decode_time import timed
    from lightgrad_amd import HipTensor
    from lightgrad_amd.autograd.hip import HipGraph
    layers, width = bert.TINY["num_hidden_layers"], bert.TINY["hidden_size"]
    cache = nn.KVCache(layers, ROWS, CAPACITY, width, like=HipTensor.from_numpy(np.zeros(1, np.float32), requires_grad=False), per_row=True)
    cache.set_lengths([prefix] * ROWS)
    local = (np.arange(w) + 1) % w if kind == "cycle" else np.arange(w)
    parent = HipTensor.from_numpy(np.concatenate([g * w + local for g in range(ROWS // w)]).astype(np.int32), requires_grad=False)

    def launches():
        for _ in range(per_graph):
            cache.reorder(parent, w)
    launches()
    graph = HipGraph()
    with graph.capture():
        launches()
    us = timed(graph.replay, max(1, iters // 4)) / per_graph
    graph.destroy()
    return us, 2 * layers * ROWS * prefix * width * 4


def measure_call(bert, route, model, w):
    """(ms of the call, kernels of the captured step, a checksum of the new tokens)"""
    import numpy as np
    import lightgrad_amd as light
    from lightgrad_amd.autograd.hip import HipDevice, HipGraph
    rng = np.random.RandomState(0)
    n = ROWS if route == "beam" else ROWS * w
    prompts = np.tile(rng.randint(1, bert.TINY["vocab_size"], (ROWS, PROMPT)), (n // ROWS, 1)).astype(np.int32)
    ids = light.from_numpy(prompts, requires_grad=False).hip(requires_grad=False)
    extra = dict(num_beams=w, poll=4) if route == "beam" else {}
    graph = HipGraph()
    HipDevice.synchronize()
    t0 = time.perf_counter()
    out = bert.generate(model, ids, NEW, lengths=[PROMPT] * n, graph=graph, **extra)
    HipDevice.synchronize()
    ms = 1e3 * (time.perf_counter() - t0)
    kernels = graph.kernel_count()
    graph.destroy()
    return ms, kernels, int(out.numpy()[:, PROMPT:].sum())


def main():
    import numpy as np
    ap = argparse.ArgumentParser()
    ap.add_argument("what", choices=["step", "select", "reorder", "call"])
    ap.add_argument("--route", choices=["beam", "rows"], default="beam")
    ap.add_argument("--w", type=int, default=4)
    ap.add_argument("--vocab", type=int, default=30522)
    ap.add_argument("--prefix", type=int, default=128)
    ap.add_argument("--parent", choices=["cycle", "identity"], default="cycle")
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
    if args.what == "select":
        res = [measure_select(args.w, args.vocab, args.iters) for _ in range(args.rounds)]
        say("tree %s  select 8 rows, %d beams, vocab %d: beam_step %s us per launch, sample %s us per launch (graphs of 8 launches, over 8); median (p10 .. p90) over %d rounds" % (
            name, args.w, args.vocab, spread([r[0] for r in res]), spread([r[1] for r in res]), args.rounds))
    elif args.what == "reorder":
        res = [measure_reorder(bert, args.w, args.prefix, args.parent, args.iters) for _ in range(args.rounds)]
        us, moved = np.median([r[0] for r in res]), res[0][1]
        say("tree %s  reorder 8 rows, %d beams, prefix %d, %s parents: %s us per launch (a graph of 8 launches, over 8)%s; median (p10 .. p90) over %d rounds" % (
            name, args.w, args.prefix, args.parent, spread([r[0] for r in res]),
            "; %d bytes read and as many written: %.1f GB/s" % (moved, 2 * moved / us / 1e3) if args.parent == "cycle" else "", args.rounds))
    else:
        np.random.seed(0)
        model = bert.BertForMaskedLM(**dict(bert.TINY, causal=True)).eval().map_parameters(lambda p: p.hip())
        if args.what == "step":
            res = [measure_step(bert, args.route, model, args.w, args.iters) for _ in range(args.rounds)]
            say("tree %s  step %-4s 8 rows behind a prefix of 128%s: %s us per replayed step; kernels of the step %d; median (p10 .. p90) over %d rounds" % (
                name, args.route, ", %d beams per prompt" % args.w if args.route == "beam" else "", spread([r[0] for r in res]), res[0][1], args.rounds))
        else:
            measure_call(bert, args.route, model, args.w)                       # untimed: kernels loaded, pool filled
            res = [measure_call(bert, args.route, model, args.w) for _ in range(args.rounds)]
            say("tree %s  call %-4s %s, 64 new tokens each: %s ms; kernels of the captured step %d; checksum %d; median (p10 .. p90) over %d rounds" % (
                name, args.route, "8 prompts of 64 ids, %d beams" % args.w if args.route == "beam" else "%d rows of 64 ids" % (ROWS * args.w),
                spread([r[0] for r in res]), res[0][1], res[0][2], args.rounds))
    if args.out:
        with open(args.out, "a") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
