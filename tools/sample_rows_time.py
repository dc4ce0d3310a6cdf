"""Time per-request sampling on the GPU against the parent commit's own tree and library.

    python tools/sample_rows_time.py --parent-tree DIR [--processes 2] [--out FILE.json]

DIR is a checkout of the parent commit with its library built in place.  Every figure comes from a process of its own that
imports ONE tree (`--worker TREE`, started here one after the other, each under a time limit), `--processes` of them per tree; the
table gives each process's median, so the spread between two processes stands next to the difference between two trees.

(a), (b) The launch on float32 logits of (8, 30522), standard_normal * 4 - the C ABI called directly, HIP events around 20
   back-to-back launches, 10 warm-up launches, the median of 30 windows, the cases alternating inside every repetition:
     sample_plain / sample_nucleus   lg_sample_f32 with (1, 0, 1) and (0.8, 50, 0.95): both trees - (b) the move of the row body
     rows_plain / rows_nucleus       lg_sample_rows_f32 with the same set in every table row, 8 seeds: this tree only - (a)
     rows_mixed                      every second row greedy, the others (0.8, 50, 0.95)
(c) The all-decode step of examples/bert.py's `serve` (TINY, causal, 8 slots, prompts of 16 tokens, no end-of-sequence id)
   replayed from a captured graph, 200 replays after 20 warm-up replays, 3 rounds (each a fresh model, pool and capture):
     step_sampled       temperature=0.8, top_k=50, top_p=0.95: one set, the global stream - both trees
     step_per_request   the same set with seeds=0: this tree only
     step_mixed         every second request greedy: this tree only
Without a GPU this fails; nothing here falls back."""
import argparse
import ctypes
import importlib.util
import json
import os
import subprocess
import sys
import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ROWS, COLS, WARMUP, REPS, WINDOW = 8, 30522, 10, 30, 20
NUCLEUS = (0.8, 50, 0.95)
SLOTS, PROMPT, BUDGET, ROUNDS, REPLAYS = 8, 16, 480, 3, 200
WORKER_LIMIT = 300        # seconds for one worker process


def windows(lib, cases, sync):
    """cases: [(name, run())] -> {name: median us per launch}"""
    def event():
        e = ctypes.c_void_p()
        assert lib.lg_event_create(ctypes.byref(e)) == 0
        return e
    samples = {name: [] for name, _ in cases}
    for _, run in cases:
        for _ in range(WARMUP):
            run()
    sync()
    for _ in range(REPS):
        for name, run in cases:
            e0, e1 = event(), event()
            assert lib.lg_event_record(e0) == 0
            for _ in range(WINDOW):
                run()
            assert lib.lg_event_record(e1) == 0
            ms = ctypes.c_float()
            assert lib.lg_event_elapsed_ms(e0, e1, ctypes.byref(ms)) == 0          # waits for the window
            samples[name].append(1e3 * ms.value / WINDOW)
            lib.lg_event_destroy(e0), lib.lg_event_destroy(e1)
    return {name: float(np.median(v)) for name, v in samples.items()}


def worker(tree):
    """this process imports the tree at `tree` alone: one JSON line of medians in us"""
    sys.path.insert(0, tree)
    import lightgrad_amd as light
    import lightgrad_amd.nn as nn
    from lightgrad_amd import HipTensor
    from lightgrad_amd.autograd.hip import HipGraph, HipDevice
    from lightgrad_amd.autograd.hip import lib as L
    assert os.path.abspath(light.__file__).startswith(os.path.abspath(tree) + os.sep), light.__file__
    lib = L.lib()
    has_rows = hasattr(HipTensor, "sample_rows")
    up = lambda a, dtype=None: HipTensor.from_numpy(np.ascontiguousarray(a, dtype), requires_grad=False)        # noqa: E731

    # ---- the launch
    host = (np.random.RandomState(ROWS).standard_normal((ROWS, COLS)) * 4.0).astype(np.float32)
    x, out = up(host), HipTensor.empty((ROWS,), dtype=np.int32, requires_grad=False)
    base = HipTensor.empty((1,), dtype=np.uint64, requires_grad=False)

    def global_launch(t, k, p):
        return lambda: L.check(lib.lg_sample_f32(x.ptr, ROWS, COLS, COLS, t, k, p, out.ptr, 4, base.ptr))
    cases = [("sample_plain", global_launch(1.0, 0, 1.0)), ("sample_nucleus", global_launch(*NUCLEUS))]
    if has_rows:
        index, counter = up(np.arange(ROWS), np.int32), up(np.arange(ROWS) * 3, np.int32)

        def rows_launch(t, k, p):
            table = up(light.random.sampling_table(t, k, p, list(range(ROWS))))
            return lambda table=table: L.check(lib.lg_sample_rows_f32(x.ptr, ROWS, COLS, COLS, table.ptr, ROWS, index.ptr, counter.ptr, out.ptr, 4))
        mixed = [0.0 if r % 2 else NUCLEUS[0] for r in range(ROWS)]
        cases += [("rows_plain", rows_launch(1.0, 0, 1.0)), ("rows_nucleus", rows_launch(*NUCLEUS)), ("rows_mixed", rows_launch(mixed, NUCLEUS[1], NUCLEUS[2]))]
        # results must be right before anything is timed: greedy rows are the argmax, the others valid ids
        cases[-1][1]()
        got = out.numpy()
        np.testing.assert_array_equal(got[1::2], host.argmax(axis=1)[1::2])
        assert (got >= 0).all() and (got < COLS).all()
    result = windows(lib, cases, HipDevice.synchronize)

    # ---- the replayed all-decode step of serve
    spec = importlib.util.spec_from_file_location("bert_example_timing", os.path.join(tree, "examples", "bert.py"))
    bert = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(bert)
    routes = [("step_sampled", None)]
    if has_rows:
        routes += [("step_per_request", [NUCLEUS[0]] * SLOTS), ("step_mixed", mixed)]
    per_round = {name: [] for name, _ in routes}
    for _ in range(ROUNDS):
        for name, temperatures in routes:
            np.random.seed(0)
            model = bert.BertForMaskedLM(**dict(bert.TINY, causal=True)).eval().map_parameters(lambda p: p.hip())
            prompts = np.random.randint(0, bert.TINY["vocab_size"], (SLOTS, PROMPT)).astype(np.int32)
            cache = nn.KVCache(bert.TINY["num_hidden_layers"], SLOTS, PROMPT + BUDGET - 1, bert.TINY["hidden_size"], like=model.cls.predictions.bias, per_row=True)
            table = None if temperatures is None else light.random.sampling_table(temperatures, NUCLEUS[1], NUCLEUS[2], list(range(SLOTS)))
            extra = {} if table is None else {"sampling": table}
            pool = nn.RequestPool(cache, prompts, [PROMPT] * SLOTS, [BUDGET] * SLOTS, PROMPT, **extra)
            sampler = NUCLEUS if table is None else None
            light.manual_seed(0)
            with light.no_grad():
                pool.admit(None)
                for _ in range(3):                                   # the prompts, then every slot decodes
                    bert.serve_step(model, pool, sampler, None)
                assert pool.count.numpy().tolist() == [1] * SLOTS
                graph = HipGraph()
                with graph.capture():
                    bert.serve_step(model, pool, sampler, None)
            for _ in range(20):
                graph.replay()
            HipDevice.synchronize()
            e0, e1 = ctypes.c_void_p(), ctypes.c_void_p()
            L.check(lib.lg_event_create(ctypes.byref(e0))), L.check(lib.lg_event_create(ctypes.byref(e1)))
            L.check(lib.lg_event_record(e0))
            for _ in range(REPLAYS):
                graph.replay()
            L.check(lib.lg_event_record(e1))
            HipDevice.synchronize()
            ms = ctypes.c_float()
            L.check(lib.lg_event_elapsed_ms(e0, e1, ctypes.byref(ms)))
            per_round[name].append(1e3 * ms.value / REPLAYS)
            result[name + "_kernels"] = graph.kernel_count()
            assert pool.out_len.numpy().tolist() == [3 + 20 + REPLAYS] * SLOTS and pool.finished() == 0          # every replay was a decode step
            graph.destroy()
    result.update({name: float(np.median(v)) for name, v in per_round.items()})
    print(json.dumps(result), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-tree", default=None)
    ap.add_argument("--processes", type=int, default=2)
    ap.add_argument("--worker", default=None, help=argparse.SUPPRESS)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if args.worker:
        return worker(os.path.abspath(args.worker))
    trees = ([("parent", os.path.abspath(args.parent_tree))] if args.parent_tree else []) + [("this", ROOT)]
    runs = {name: [] for name, _ in trees}
    for k in range(args.processes):                                  # the trees alternate; one process holds the GPU at a time
        for name, tree in trees:
            child = subprocess.run([sys.executable, os.path.abspath(__file__), "--worker", tree], stdout=subprocess.PIPE, text=True, timeout=WORKER_LIMIT)
            if child.returncode != 0:
                sys.exit("the worker of the %s tree ended with status %d - nothing more is started" % (name, child.returncode))
            runs[name].append(json.loads(child.stdout.strip().splitlines()[-1]))
    keys = sorted({k for rs in runs.values() for r in rs for k in r})
    print("%-26s %s" % ("us (median per process)", "  ".join("%-22s" % name for name, _ in trees)))
    for key in keys:
        print("%-26s %s" % (key, "  ".join("%-22s" % " ".join("%.1f" % r[key] if key in r else "-" for r in runs[name]) for name, _ in trees)), flush=True)
    if args.out:
        with open(args.out, "w") as f:
            json.dump(runs, f, indent=1, sort_keys=True)


if __name__ == "__main__":
    main()
