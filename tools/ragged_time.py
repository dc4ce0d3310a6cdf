"""Time the per-row positions of the KV cache on the GPU: the `_rows` attention launches against the one-word launches, and one
ragged `generate` against one `generate` per sequence.

    python tools/ragged_time.py launch [--rows] [--tree <a built checkout of another commit>] [--rounds 5] [--iters 200]
    python tools/ragged_time.py generate --route ragged|alone [--tree ...] [--rounds 5]
    ... [--out FILE]   appends the printed lines to FILE

launch    us per launch, replayed from a graph of 32 launches (tools/decode_time.py's method): `decode_attention` at (b, heads, d)
          = (8, 2, 64), capacity 512, t = 255, and `extend_attention` with m = 32 new tokens at t = 224.  Without --rows the
          position is one word (lg_attention_decode_f32 / lg_attention_extend_f32 - with --tree: that commit's launch); with
          --rows it is 8 words that all hold the same t (lg_attention_decode_rows_f32 / lg_attention_extend_rows_f32): the same
          work, so any difference is what the per-row addressing costs.  Run the one-word form twice, in two processes: their
          difference is the run-to-run noise the comparison has to be read against.
generate  the TINY causal model, 8 prompts of 16, 32, .. 128 tokens, 32 new tokens each, greedy, the decode step captured:
            ragged  ONE `generate(lengths=)` over the right-padded batch (this tree only)
            alone   eight `generate` calls at batch 1, one per prompt - the only correct route of a tree without per-row
                    positions (--tree: import the package and the model from that tree)
          Wall time from the call to the synchronised end, after one untimed run of the same calls (kernels loaded, pool filled);
          every run captures its step anew, as a caller would.  The kernel count of the captured step is printed.

Median and p10 .. p90 over the rounds.  Without a GPU this fails; nothing here falls back."""
import argparse
import importlib.util
import math
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
BATCH, NEW = 8, 32
LENGTHS = tuple(range(16, 129, 16))


def load(tree):
    sys.path.insert(0, tree)
    spec = importlib.util.spec_from_file_location("bert_example_timing", os.path.join(tree, "examples", "bert.py"))
    bert = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(bert)
    return bert


def measure_launch(op, rows, iters, heads=2, d=64, capacity=512, per_graph=32):
    import numpy as np
    from decode_time import timed
    from lightgrad_amd import HipTensor
    from lightgrad_amd.autograd.hip import HipGraph
    rng = np.random.RandomState(0)
    width = heads * d
    m, t = (1, 255) if op == "decode_attention" else (32, 224)
    k, v = (HipTensor.from_numpy(rng.uniform(-1.5, 1.5, (BATCH, capacity, width)).astype(np.float32), requires_grad=False) for _ in range(2))
    q, kn, vn = (HipTensor.from_numpy(rng.uniform(-1.5, 1.5, (BATCH, m, width)).astype(np.float32), requires_grad=False) for _ in range(3))
    pos = HipTensor.from_numpy(np.full(BATCH if rows else 1, t, np.int32), requires_grad=False)

    def launches():
        for _ in range(per_graph):
            getattr(q, op)(kn, vn, k, v, pos, heads=heads, scale=math.sqrt(d) ** -1)
    launches()
    graph = HipGraph()
    with graph.capture():
        launches()
    us = timed(graph.replay, max(1, iters // 4)) / per_graph
    graph.destroy()
    return us


def measure_generate(bert, route, model, prompts):
    """(ms of the whole route, kernels of a captured step)"""
    import numpy as np
    import lightgrad_amd as light
    from lightgrad_amd.autograd.hip import HipDevice, HipGraph
    to_device = lambda a: light.from_numpy(a, requires_grad=False).hip(requires_grad=False)          # noqa: E731
    if route == "ragged":
        padded = np.zeros((BATCH, max(LENGTHS)), np.int32)
        for r, p in enumerate(prompts):
            padded[r, :len(p)] = p
        inputs = [to_device(padded)]
    else:
        inputs = [to_device(p[None, :]) for p in prompts]
    HipDevice.synchronize()
    t0 = time.perf_counter()
    graphs, outs = [], []
    for ids in inputs:
        graphs.append(HipGraph())
        extra = {"lengths": LENGTHS} if route == "ragged" else {}
        outs.append(bert.generate(model, ids, NEW, graph=graphs[-1], **extra))
    HipDevice.synchronize()
    ms = 1e3 * (time.perf_counter() - t0)
    kernels = graphs[0].kernel_count()
    tokens = [o.numpy() for o in outs]
    for g in graphs:
        g.destroy()
    return ms, kernels, tokens


def main():
    import numpy as np
    ap = argparse.ArgumentParser()
    ap.add_argument("what", choices=["launch", "generate"])
    ap.add_argument("--rows", action="store_true")
    ap.add_argument("--route", choices=["ragged", "alone"], default="ragged")
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
        for op in ("decode_attention", "extend_attention"):
            xs = [measure_launch(op, args.rows, args.iters) for _ in range(args.rounds)]
            say("tree %s  %-16s (8, 2, 64) capacity 512, %s: %s us per launch, replayed; median (p10 .. p90) over %d rounds" % (
                name, op, "8 position words, all equal (_rows entry)" if args.rows else "one position word", spread(xs), args.rounds))
    else:
        np.random.seed(0)
        model = bert.BertForMaskedLM(**dict(bert.TINY, causal=True)).eval().map_parameters(lambda p: p.hip())
        prompts = [np.random.randint(1, bert.TINY["vocab_size"], n).astype(np.int32) for n in LENGTHS]
        measure_generate(bert, args.route, model, prompts)                  # untimed: kernels loaded, pool filled
        res = [measure_generate(bert, args.route, model, prompts) for _ in range(args.rounds)]
        first = res[0][2]
        if args.route == "ragged":
            new = [first[0][r, LENGTHS[r]:LENGTHS[r] + NEW] for r in range(BATCH)]
        else:
            new = [t[0, LENGTHS[r]:] for r, t in enumerate(first)]
        say("tree %s  generate %-6s 8 prompts of %s tokens, %d new: %s ms for the route; kernels of a captured step %d; median (p10 .. p90) over %d rounds" % (
            name, args.route, "/".join(str(n) for n in LENGTHS), NEW, spread([r[0] for r in res]), res[0][1], args.rounds))
        say("  new tokens of the rows (a checksum to hold the two routes against each other): %s" % " ".join(str(int(np.sum(t))) for t in new))
    if args.out:
        with open(args.out, "a") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
