"""Time speculative decoding by prompt lookup on the GPU against the captured per-row decode step of `generate(lengths=)`.

    python tools/speculate_time.py step --route spec --k 3 | --route rows [--tree <a built checkout of another commit>]
    python tools/speculate_time.py tokens --route spec --k 3 [--prompts random] | --route rows [--tree ...] [--prompts random]
    python tools/speculate_time.py commit --columns 512 [--k 3]
    ... [--rounds 5] [--iters 200] [--out FILE]   appends the printed lines to FILE

step    us per replayed step of the TINY causal model, 8 sequences behind a prefix of 128 tokens, capacity 512:
          spec  `speculate_step` with m = k + 1 token rows per sequence and drafting made impossible (n-grams of 1024 tokens: longer
                than any sequence), so every count is 1 - the price of the step's shape when nothing is accepted
          rows  `decode_step_rows`, the captured per-row decode step (--tree: that commit's)
        Both walk the same positions (20 warm-up replays, then --iters timed ones).  The kernel count of the step is printed.
tokens  `generate` of 128 new tokens for 8 prompts of 64 tokens, greedy, the step captured, wall time from the call to the
        synchronised end after one untimed run of the same call:
          spec  generate(lengths=, speculate=k, poll=4): steps, tokens per step per sequence, drafts accepted, ms, us per token
          rows  generate(lengths=) (--tree: that commit's), 127 replayed steps
        --prompts repeat (default): every prompt is a motif of 8 random ids repeated 8 times (np.random.RandomState(0)) - ids on
        which lookup works from the first step; --prompts random: 64 random ids.  A randomly initialised model decoded greedily
        falls into loops either way, which flatters the acceptance rate: read `step` beside it.
commit  us per `speculate_commit` launch alone, 8 rows of random ids with m = k + 1, at `columns` columns: a graph of one copy launch
        (the positions go back to columns - 2 - 8 m - k: no row reaches its end) and 8 commits, replayed; the time is the graph's
        over 8.  The tokens "drawn" are the same in every launch, so the lookup soon drafts them and they are accepted: the rows
        search sequences of nearly `columns` ids at n = 3, 2 and 1.

Median and p10 .. p90 over the rounds.  Run every command under its own `timeout -k 10 <seconds>` and chain them with `&&`.
Without a GPU this fails; nothing here falls back."""
import argparse
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
from serve_time import load  # noqa: E402

ROWS, PREFIX, CAPACITY, NEW, PROMPT = 8, 128, 512, 128, 64


def measure_step(bert, route, model, k, iters):
    """(us per replayed step, kernels of the step): 8 sequences of PREFIX tokens, one real token per sequence and step"""
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
    assert PREFIX + 20 + iters + 4 + k < CAPACITY
    with light.no_grad():
        model(i32(prompts), cache=cache)
        cache.set_lengths([PREFIX] * ROWS)
        out_ids = i32(np.zeros((ROWS, CAPACITY)))
        out_ids[:, :PREFIX] = i32(prompts)
        if route == "spec":
            m = k + 1
            drafter = bert.NgramDrafter(k, max_ngram=1024, min_ngram=1024)
            state = dict(ids=i32(np.zeros((ROWS, m))), count=i32(np.ones(ROWS)), position_ids=i32(np.zeros((ROWS, m))), out_ids=out_ids,
                         end=i32(np.full(ROWS, CAPACITY - 1)), done=i32(np.zeros(ROWS)), stats=i32(np.zeros(3)))
            cache.advance(-1)
            cache.lengths, cache.length = None, CAPACITY - 1
            tgt = i32(np.zeros((ROWS, m)))
            tgt[:, 0:1] = i32(prompts[:, -1:])
            drafter.commit(tgt, state, cache)
            bert.speculate_step(model, cache, state, drafter)
            with graph.capture():
                bert.speculate_step(model, cache, state, drafter)
        else:
            token = i32(prompts[:, -1:].copy())
            done = i32(np.zeros(ROWS))
            bert.decode_step_rows(model, cache, token, out_ids, done)
            with graph.capture():
                bert.decode_step_rows(model, cache, token, out_ids, done)
    us = timed(graph.replay, iters)
    kernels = graph.kernel_count()
    if route == "spec":
        assert state["count"].numpy().tolist() == [1] * ROWS and state["stats"].numpy().tolist() == [0, 0, 0]
    graph.destroy()
    return us, kernels


def prompts_of(bert, kind):
    import numpy as np
    rng = np.random.RandomState(0)
    if kind == "random":
        return rng.randint(1, bert.TINY["vocab_size"], (ROWS, PROMPT)).astype(np.int32)
    return np.tile(rng.randint(1, bert.TINY["vocab_size"], (ROWS, 8)), (1, PROMPT // 8)).astype(np.int32)


def measure_tokens(bert, route, model, prompts, k):
    """(ms of the call, kernels of the captured step, statistics or None, a checksum of the new tokens)"""
    import lightgrad_amd as light
    from lightgrad_amd.autograd.hip import HipDevice, HipGraph
    ids = light.from_numpy(prompts, requires_grad=False).hip(requires_grad=False)
    stats = {}
    extra = dict(speculate=k, poll=4, stats=stats) if route == "spec" else {}
    graph = HipGraph()
    HipDevice.synchronize()
    t0 = time.perf_counter()
    out = bert.generate(model, ids, NEW, lengths=[PROMPT] * ROWS, graph=graph, **extra)
    HipDevice.synchronize()
    ms = 1e3 * (time.perf_counter() - t0)
    kernels = graph.kernel_count()
    graph.destroy()
    return ms, kernels, stats or None, int(out.numpy()[:, PROMPT:].sum())


def measure_commit(columns, k, iters, per_graph=8):
    import numpy as np
    from decode_time import timed
    from lightgrad_amd import HipTensor
    from lightgrad_amd.autograd.hip import HipGraph
    rng = np.random.RandomState(2)
    m = k + 1
    start = columns - 2 - per_graph * m - k
    assert start >= 4
    i32 = lambda a: HipTensor.from_numpy(np.ascontiguousarray(a, np.int32), requires_grad=False)       # noqa: E731
    out_ids = i32(rng.randint(1, 50, (ROWS, columns)))
    state = [i32(rng.randint(1, 50, (ROWS, m))), i32(np.ones(ROWS)), i32(np.zeros((ROWS, m))), out_ids, i32(np.full(ROWS, start)),
             i32(np.full(ROWS, columns - 1)), i32(np.zeros(ROWS)), i32(np.zeros(3))]
    saved = i32(np.full(ROWS, start))
    tgt = i32(np.tile(60 + np.arange(m), (ROWS, 1)))                        # ids no row holds yet

    def launches():
        state[4][:] = saved
        for _ in range(per_graph):
            tgt.speculate_commit(*state, k)
    launches()
    graph = HipGraph()
    with graph.capture():
        launches()
    us = timed(graph.replay, max(1, iters // 4)) / per_graph
    assert state[6].numpy().tolist() == [0] * ROWS and (state[4].numpy() > start).all()
    graph.destroy()
    return us


def main():
    import numpy as np
    ap = argparse.ArgumentParser()
    ap.add_argument("what", choices=["step", "tokens", "commit"])
    ap.add_argument("--route", choices=["spec", "rows"], default="spec")
    ap.add_argument("--k", type=int, default=3)
    ap.add_argument("--prompts", choices=["repeat", "random"], default="repeat")
    ap.add_argument("--columns", type=int, default=512)
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
    if args.what == "commit":
        xs = [measure_commit(args.columns, args.k, args.iters) for _ in range(args.rounds)]
        say("tree %s  speculate_commit 8 rows, m = %d, %d columns: %s us per launch (a graph of 1 copy + 8 commits, over 8); median (p10 .. p90) over %d rounds" % (
            name, args.k + 1, args.columns, spread(xs), args.rounds))
    else:
        np.random.seed(0)
        model = bert.BertForMaskedLM(**dict(bert.TINY, causal=True)).eval().map_parameters(lambda p: p.hip())
        if args.what == "step":
            res = [measure_step(bert, args.route, model, args.k, args.iters) for _ in range(args.rounds)]
            say("tree %s  step %-4s 8 sequences behind a prefix of 128%s: %s us per replayed step; kernels of the step %d; median (p10 .. p90) over %d rounds" % (
                name, args.route, ", %d token rows per sequence, no drafts (count = 1)" % (args.k + 1) if args.route == "spec" else "",
                spread([r[0] for r in res]), res[0][1], args.rounds))
        else:
            prompts = prompts_of(bert, args.prompts)
            measure_tokens(bert, args.route, model, prompts, args.k)               # untimed: kernels loaded, pool filled
            res = [measure_tokens(bert, args.route, model, prompts, args.k) for _ in range(args.rounds)]
            ms, stats = [r[0] for r in res], res[0][2]
            say("tree %s  tokens %-4s 8 prompts of 64 ids (%s), 128 new tokens each%s: %s ms; %.1f us per token and sequence at the median; kernels of the captured step %d%s; checksum %d; median (p10 .. p90) over %d rounds" % (
                name, args.route, args.prompts, ", up to %d drafts" % args.k if args.route == "spec" else "", spread(ms), 1e3 * np.median(ms) / NEW,
                res[0][1], "; %d steps (%.2f tokens per step and sequence), %d of %d drafts accepted" % (
                    stats["steps"], (NEW - 1) / stats["steps"], stats["accepted"], stats["drafted"]) if stats else "; %d steps" % (NEW - 1),
                res[0][3], args.rounds))
    if args.out:
        with open(args.out, "a") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
