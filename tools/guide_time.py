"""Time the guided-decoding launch and the serving step with it, on the GPU, against the parent commit's own tree and library.

    python tools/guide_time.py --parent-tree DIR [--processes 2] [--out FILE.json]

DIR is a checkout of the parent commit with its library built in place.  Every figure comes from a process of its own that
imports ONE tree (`--worker TREE`, started here one after the other, each under a time limit), `--processes` of them per tree; the
table gives each process's median, so the spread between two processes stands next to the difference between two trees.

(a) The launch on float32 logits of (8, 30522), standard_normal * 4 - the C ABI called directly, HIP events around 20
   back-to-back launches, 10 warm-up launches, the median of 30 windows, the cases alternating inside every repetition; the
   launches work in place, so the logits are written back from a copy and the state pairs set back in front of every window
   (outside the events).  Every request has stored one token that its state has not absorbed yet: each launch catches up:
     guide_ban3 / _allow50 / _forced   lg_guide_rows_f32 under `ban_sequences` of 3 ids (few stores), `allow_only` of 50 ids
                                       (nearly every id stored) and a state that forces one id, with the automatic grid (8 slices
                                       a row at this width); the same with `_1` behind the name: one workgroup per row: this tree only
     penalize_17                       lg_penalize_rows_f32 with (1.3, 0.5, 0.25, 0) and a history of 17 ids: both trees
     logprob_token                     lg_logprob_rows_f32, the token alone (want = 0): both trees
(b) The all-decode step of examples/bert.py's `serve` (TINY, causal, 8 slots, prompts of 128 tokens, greedy, no end-of-sequence
   id) replayed from a captured graph, 200 replays after 20 warm-up replays, 3 rounds (each a fresh model, pool and capture):
     step_greedy      no guides: both trees
     step_none        this tree, built the way `serve` builds it for guide=None (no tables): this tree only
     step_guides      `ban_sequences` of 3 ids for every request: this tree only
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
PENALTIES, HISTORY = (1.3, 0.5, 0.25, 0), (9, 8)
BANNED = (7, 1000, 30000)
SLOTS, PROMPT, BUDGET, ROUNDS, REPLAYS = 8, 128, 300, 3, 200
WORKER_LIMIT = 300        # seconds for one worker process


def windows(lib, cases, sync):
    """cases: [(name, run(), reset() or None)] -> {name: median us per launch}"""
    def event():
        e = ctypes.c_void_p()
        assert lib.lg_event_create(ctypes.byref(e)) == 0
        return e
    samples = {name: [] for name, _, _ in cases}
    for _, run, _ in cases:
        for _ in range(WARMUP):
            run()
    sync()
    for _ in range(REPS):
        for name, run, reset in cases:
            if reset is not None:
                reset()
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
    has_guides = hasattr(HipTensor, "guide_rows")
    up = lambda a, dtype=None: HipTensor.from_numpy(np.ascontiguousarray(a, dtype), requires_grad=False)        # noqa: E731

    # ---- the launches
    rng = np.random.RandomState(ROWS)
    host = (rng.standard_normal((ROWS, COLS)) * 4.0).astype(np.float32)
    x, fresh = up(host), up(host)
    index = up(np.arange(ROWS), np.int32)

    def reset():
        x[:, :] = fresh
    P, G = HISTORY
    table = up(np.repeat(light.random.penalty_table(*PENALTIES), ROWS, axis=0))
    history = [up(rng.randint(0, COLS, (ROWS, P)), np.int32), up(np.full(ROWS, P), np.int32), up(rng.randint(0, COLS, (ROWS, G)), np.int32), up(np.full(ROWS, G), np.int32)]
    token, want, counter = up(rng.randint(0, COLS, ROWS), np.int32), up(np.zeros(ROWS), np.int32), up(np.zeros(ROWS), np.int32)
    score, top_ids, top = (HipTensor.from_numpy(np.zeros(s, d), requires_grad=False) for s, d in (((ROWS, 1), np.float32), ((ROWS, 1, 1), np.int32), ((ROWS, 1, 1), np.float32)))
    cases = [("penalize_17", lambda: L.check(lib.lg_penalize_rows_f32(x.ptr, ROWS, COLS, COLS, table.ptr, ROWS, index.ptr, history[0].ptr, P, P, history[1].ptr,
                                                                     history[2].ptr, G, G, history[3].ptr, -1)), reset),
             ("logprob_token", lambda: L.check(lib.lg_logprob_rows_f32(x.ptr, ROWS, COLS, COLS, token.ptr, want.ptr, ROWS, index.ptr, counter.ptr, score.ptr, 1,
                                                                       top_ids.ptr, top.ptr, 1)), reset)]
    if has_guides:
        guide = light.guide
        forced = guide.one_of(COLS, [[11, 12]])
        masks = (("ban3", guide.ban_sequences(COLS, [[v] for v in BANNED]), 5), ("allow50", guide.allow_only(COLS, range(100, 30100, 600)), 100),
                 ("forced", forced, 11))
        for name, automaton, stored in masks:
            tables = guide.compile_guides(automaton, ROWS, 0)
            allow, states, edges = (up(a) for a in (tables.allow, tables.states, tables.edges))
            out, out_len = up(np.full((ROWS, 4), stored), np.int32), up(np.ones(ROWS), np.int32)
            start = np.stack([tables.start, np.zeros(ROWS, np.int32)], axis=1)
            state, state0 = up(start), up(start)
            S, E = tables.states.shape[0], tables.edges.shape[0]

            def launch(allow=allow, states=states, edges=edges, out=out, out_len=out_len, state=state, S=S, E=E):
                L.check(lib.lg_guide_rows_f32(x.ptr, ROWS, COLS, COLS, allow.ptr, states.ptr, S, edges.ptr, E, index.ptr, out.ptr, 4, 4, out_len.ptr, state.ptr, ROWS))

            def reset_both(state=state, state0=state0):
                x[:, :] = fresh
                state[:, :] = state0
            for slices in (0, 1):
                # results must be right before anything is timed: one launch against the definition, bit for bit
                lib.lg_guide_rows_slices(slices)
                reset_both()
                launch()
                y, new_state, bad = guide.guide_logits(host, tables.allow, tables.states, tables.edges, np.arange(ROWS), out.numpy(), np.ones(ROWS), start)
                assert not bad.any() and (x.numpy().view(np.uint32) == y.view(np.uint32)).all() and state.numpy().tolist() == new_state.tolist()

                def run(launch=launch, slices=slices):
                    lib.lg_guide_rows_slices(slices)
                    launch()
                cases.append(("guide_%s%s" % (name, "_1" if slices else ""), run, reset_both))
    result = windows(lib, cases, HipDevice.synchronize)
    if has_guides:
        lib.lg_guide_rows_slices(0)

    # ---- the replayed all-decode step of serve
    spec = importlib.util.spec_from_file_location("bert_example_timing", os.path.join(tree, "examples", "bert.py"))
    bert = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(bert)
    routes = [("step_greedy", {})]
    if has_guides:
        vocab = bert.TINY["vocab_size"]
        tables = light.guide.compile_guides(light.guide.ban_sequences(vocab, [[v] for v in BANNED]), SLOTS, None)
        routes += [("step_none", {"guide": None}), ("step_guides", {"guide": tuple(tables)})]
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
            assert pool.out_len.numpy().tolist() == [3 + 20 + REPLAYS] * SLOTS and pool.finished() == 0          # every replay was a decode step
            if name == "step_guides":
                assert not np.isin(pool.out.numpy()[:, :3 + 20 + REPLAYS], BANNED).any() and pool.guide_state.numpy()[:, 1].tolist() == [2 + 20 + REPLAYS] * SLOTS
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
