"""Time the log-probability launch and the serving step with it, on the GPU, against the parent commit's own tree and library.

    python tools/logprob_time.py --parent-tree DIR [--processes 2] [--out FILE.json]

DIR is a checkout of the parent commit with its library built in place.  Every figure comes from a process of its own that
imports ONE tree (`--worker TREE`, started here one after the other, each under a time limit), `--processes` of them per tree; the
table gives each process's median, so the spread between two processes stands next to the difference between two trees.

(a) The launch on float32 logits of (8, 30522), standard_normal * 4 - the C ABI called directly, HIP events around 20
   back-to-back launches, 10 warm-up launches, the median of 30 windows, the cases alternating inside every repetition:
     logprob_0 / _3 / _8    lg_logprob_rows_f32 with want = 0, 3, 8 for every request (n_max = 8), the token the row's argmax:
                            this tree only
     logprob_3_memory       the same with want = 3 on rows of 40000 floats, which the launch re-reads from memory: this tree only
     rows_nucleus           lg_sample_rows_f32 with (0.8, 50, 0.95) on the same rows, the launch it follows: the yardstick
(b) The all-decode step of examples/bert.py's `serve` (TINY, causal, 8 slots, prompts of 128 tokens, greedy, no end-of-sequence
   id) replayed from a captured graph, 200 replays after 20 warm-up replays, 3 rounds (each a fresh model, pool and capture):
     step_greedy      no log-probabilities: both trees
     step_none        this tree, built the way `serve` builds it for logprobs=None: this tree only
     step_logprobs    logprobs = 3 for every request: this tree only
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
ROWS, COLS, WIDE, WARMUP, REPS, WINDOW = 8, 30522, 40000, 10, 30, 20
NUCLEUS, G, N_MAX = (0.8, 50, 0.95), 4, 8
SLOTS, PROMPT, BUDGET, ROUNDS, REPLAYS = 8, 128, 300, 3, 200
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
    has_logprobs = hasattr(HipTensor, "logprob_rows")
    up = lambda a, dtype=None: HipTensor.from_numpy(np.ascontiguousarray(a, dtype), requires_grad=False)        # noqa: E731

    # ---- the launch
    rng = np.random.RandomState(ROWS)
    host = (rng.standard_normal((ROWS, WIDE)) * 4.0).astype(np.float32)
    wide, x, out = up(host), up(host[:, :COLS]), HipTensor.empty((ROWS,), dtype=np.int32, requires_grad=False)
    index, counter = up(np.arange(ROWS), np.int32), up(np.arange(ROWS) % G, np.int32)
    sampling = up(light.random.sampling_table(*NUCLEUS, list(range(ROWS))))
    cases = [("rows_nucleus", lambda: L.check(lib.lg_sample_rows_f32(x.ptr, ROWS, COLS, COLS, sampling.ptr, ROWS, index.ptr, counter.ptr, out.ptr, 4)))]
    if has_logprobs:
        for name, k, src, cols in (("logprob_0", 0, x, COLS), ("logprob_3", 3, x, COLS), ("logprob_8", 8, x, COLS), ("logprob_3_memory", 3, wide, WIDE)):
            logits = host[:, :cols]
            token, want = logits.argmax(-1).astype(np.int32), np.full(ROWS, k, np.int32)
            operands = [up(token), up(want)]
            outs = [up(np.zeros((ROWS, G), np.float32)), up(np.full((ROWS, G, N_MAX), -1, np.int32)), up(np.zeros((ROWS, G, N_MAX), np.float32))]

            def launch(src=src, cols=cols, operands=operands, outs=outs):
                L.check(lib.lg_logprob_rows_f32(src.ptr, ROWS, cols, cols, operands[0].ptr, operands[1].ptr, ROWS, index.ptr, counter.ptr, outs[0].ptr, G,
                                                outs[1].ptr, outs[2].ptr, N_MAX))
            # results must be right before anything is timed: one launch against the definition
            launch()
            ref = [np.zeros((ROWS, G)), np.full((ROWS, G, N_MAX), -1, np.int32), np.zeros((ROWS, G, N_MAX))]
            assert not light.random.token_logprobs_rows(logits, token, want, np.arange(ROWS), np.arange(ROWS) % G, *ref).any()
            got = [t.numpy() for t in outs]
            assert (got[1] == ref[1]).all() and np.abs(got[0] - ref[0]).max() <= 1e-5 * max(1.0, np.abs(ref[0]).max()) and \
                np.abs(got[2] - ref[2]).max() <= 1e-5 * max(1.0, np.abs(ref[2]).max())
            cases.append((name, launch))
    result = windows(lib, cases, HipDevice.synchronize)

    # ---- the replayed all-decode step of serve
    spec = importlib.util.spec_from_file_location("bert_example_timing", os.path.join(tree, "examples", "bert.py"))
    bert = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(bert)
    routes = [("step_greedy", {})]
    if has_logprobs:
        routes += [("step_none", {"logprobs": None}), ("step_logprobs", {"logprobs": [3] * SLOTS})]
    per_round = {name: [] for name, _ in routes}
    for _ in range(ROUNDS):
        for name, extra in routes:
            np.random.seed(0)
            model = bert.BertForMaskedLM(**dict(bert.TINY, causal=True)).eval().map_parameters(lambda p: p.hip())
            prompts = np.random.randint(0, bert.TINY["vocab_size"], (SLOTS, PROMPT)).astype(np.int32)
            cache = nn.KVCache(bert.TINY["num_hidden_layers"], SLOTS, PROMPT + BUDGET - 1, bert.TINY["hidden_size"], like=model.cls.predictions.bias, per_row=True)
            pool = nn.RequestPool(cache, prompts, [PROMPT] * SLOTS, [BUDGET] * SLOTS, PROMPT, **extra)
            with light.no_grad():
                pool.admit(None)
                for _ in range(3):                                   # the prompts, then every slot decodes
                    bert.serve_step(model, pool, None, None)
                assert pool.count.numpy().tolist() == [1] * SLOTS
                graph = HipGraph()
                with graph.capture():
                    bert.serve_step(model, pool, None, None)
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
            steps = 3 + 20 + REPLAYS
            assert pool.out_len.numpy().tolist() == [steps] * SLOTS and pool.finished() == 0          # every replay was a decode step
            if name == "step_logprobs":
                # greedy: every token is its step's most likely id, and a probability
                tokens, scores, best = pool.out.numpy()[:, :steps], pool.logprob.numpy()[:, :steps], pool.top_ids.numpy()[:, :steps]
                assert (best[:, :, 0] == tokens).all() and (scores < 0).all() and (pool.logprob.numpy()[:, steps:] == 0).all()
                result["mean_token_logprob"] = float(scores.mean())
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
