"""Time sampled decoding on the GPU: the sampling launch against the two-launch greedy tail it replaces, and the captured decode
step with and without sampling.

    python tools/sample_time.py [--parent-lib PATH] [--steps-only | --launch-only] [--out FILE.json]

1. The launch, on float32 logits of (8, 30522) - a decode step of batch 8 - and (1024, 30522) (the C ABI called directly, HIP
   events around 20 back-to-back launches so that the device and not the host sets the pace, 10 warm-up launches, the median of
   30 such windows; the cases of this library alternate inside every repetition):
     sample_plain    lg_sample_f32, temperature 1, top-k and top-p off             (stage, max, two scan passes)
     sample_nucleus  lg_sample_f32, temperature 0.8, top_k 50, top_p 0.95          (and both four-pass selects)
     greedy          lg_argreduce_f32 + lg_cast to int32: `argmax(-1).astype(np.int32)`, two launches, THIS library
     parent_greedy   the same two launches of another build of the library, --parent-lib PATH: the yardstick is the parent
                     commit's greedy tail on the same tensors.  It runs first, in a child process of its own that loads nothing
                     but that library, with the same windows; without the option the line says "not measured"
   Each case is timed `hot` (one tensor again and again) and `cold` (rotating over three tensors; at 1024 rows that is 375 MB
   against the 256 MiB Infinity Cache, at 8 rows everything stays cached and the two agree).  The logits are standard_normal * 4.
   Before anything is timed, `sample(top_k=1)` must equal `argmax` on every row without a tied maximum.
2. The decode step of examples/bert.py (TINY, causal, batch 8) replayed from a captured graph at the prefixes of
   profiles/decode.md, 128 and 511: greedy against sampled (0.8, 50, 0.95), 200 replays after 20 warm-up replays, 5 rounds (each
   a fresh model, cache and capture), median and p10 .. p90.  As in tools/decode_time.py the step includes one fill kernel that
   sets the position back.
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
COLS, SHAPES, WARMUP, REPS, WINDOW = 30522, (8, 1024), 10, 30, 20
NUCLEUS = (0.8, 50, 0.95)
CHILD_LIMIT = 240         # seconds for the parent library's process


def host_logits(rows):
    rng = np.random.RandomState(rows)
    return [(rng.standard_normal((rows, COLS)) * 4.0).astype(np.float32) for _ in range(3)]


def time_windows(cases, tensors, sync):
    """cases: [(name, library handle, run(tensor))] -> {"name_hot" / "name_cold": {median, p10, p90}} in us per call"""
    def event(which):
        e = ctypes.c_void_p()
        assert which.lg_event_create(ctypes.byref(e)) == 0
        return e

    us = {}
    for mode in ("hot", "cold"):
        pick = (lambda k: tensors[k % 3]) if mode == "cold" else (lambda k: tensors[0])
        samples = {name: [] for name, _, _ in cases}
        for name, which, run in cases:
            for k in range(WARMUP):
                run(pick(k))
        sync()
        for k in range(REPS):                                 # the cases alternate inside every repetition
            for name, which, run in cases:
                e0, e1 = event(which), event(which)
                assert which.lg_event_record(e0) == 0
                for j in range(WINDOW):
                    run(pick(k * WINDOW + j))
                assert which.lg_event_record(e1) == 0
                ms = ctypes.c_float()
                assert which.lg_event_elapsed_ms(e0, e1, ctypes.byref(ms)) == 0      # waits for the window: the next case starts on an idle device
                samples[name].append(1e3 * ms.value / WINDOW)
                which.lg_event_destroy(e0), which.lg_event_destroy(e1)
        for name, v in samples.items():
            v = np.sort(v)
            us["%s_%s" % (name, mode)] = {"median": float(np.median(v)), "p10": float(v[len(v) // 10]), "p90": float(v[(9 * len(v)) // 10])}
    return us


def greedy_tail(L, which, rows, idx64, idx32):
    """run(x): argmax over the last axis into idx64, then the cast to int32 into idx32 - what `argmax(-1).astype(np.int32)` launches"""
    shape, strides, oshape, ostrides = L.i64((rows, COLS)), L.i64((COLS, 1)), L.i64((rows,)), L.i64((1,))

    def run(x):
        assert which.lg_argreduce_f32(L.RED_MAX, 2, shape, x, strides, 1, idx64) == 0, which.lg_last_error()
        assert which.lg_cast(L.DT_I64, L.DT_I32, 1, oshape, idx32, ostrides, idx64, ostrides) == 0, which.lg_last_error()
    return run


def parent_child(path):
    """this process loads only the library at `path`: its greedy tail over the same logits, one JSON line"""
    sys.path.insert(0, ROOT)
    from lightgrad_amd.autograd.hip import lib as L
    names = ("lg_init", "lg_last_error", "lg_argreduce_f32", "lg_cast", "lg_event_create", "lg_event_record", "lg_event_elapsed_ms",
             "lg_event_destroy", "lg_sync", "lg_malloc", "lg_memcpy_h2d", "lg_memcpy_d2h")
    P = L.load_library(os.path.abspath(path), {n: L.PROTOTYPES[n] for n in names}, mode=ctypes.RTLD_GLOBAL)
    assert P.lg_init(0) == 0, P.lg_last_error()

    def device(nbytes, host=None):
        p = ctypes.c_void_p()
        assert P.lg_malloc(ctypes.byref(p), nbytes) == 0, P.lg_last_error()
        if host is not None:
            assert P.lg_memcpy_h2d(p, host.ctypes.data, nbytes) == 0, P.lg_last_error()
        return p
    result = {}
    for rows in SHAPES:
        host = host_logits(rows)
        tensors = [device(h.nbytes, h) for h in host]
        idx64, idx32 = device(rows * 8), device(rows * 4)
        run = greedy_tail(L, P, rows, idx64, idx32)
        run(tensors[0])
        got = np.empty(rows, np.int32)
        assert P.lg_memcpy_d2h(got.ctypes.data, idx32, got.nbytes) == 0
        np.testing.assert_array_equal(got, host[0].argmax(axis=1))
        result[str(rows)] = time_windows([("parent_greedy", P, run)], tensors, lambda: P.lg_sync())
    print(json.dumps(result), flush=True)


def measure_launches(parent_us):
    import lightgrad_amd as light
    from lightgrad_amd import HipTensor
    from lightgrad_amd.autograd.hip import lib as L
    lib = L.lib()
    result = {}
    for rows in SHAPES:
        host = host_logits(rows)
        xs = [HipTensor.from_numpy(h, requires_grad=False) for h in host]
        idx64 = HipTensor.empty((rows,), dtype=np.int64, requires_grad=False)
        idx32 = HipTensor.empty((rows,), dtype=np.int32, requires_grad=False)
        base = HipTensor.empty((1,), dtype=np.uint64, requires_grad=False)
        tail = greedy_tail(L, lib, rows, idx64.ptr, idx32.ptr)

        def sampler(temperature, top_k, top_p):
            return lambda x: L.check(lib.lg_sample_f32(x.ptr, rows, COLS, COLS, temperature, top_k, top_p, idx32.ptr, 4, base.ptr))
        cases = [("sample_plain", lib, sampler(1.0, 0, 1.0)), ("sample_nucleus", lib, sampler(*NUCLEUS)), ("greedy", lib, lambda x: tail(x.ptr))]

        # results must be right before anything is timed
        untied = (host[0] == host[0].max(axis=1, keepdims=True)).sum(axis=1) == 1
        light.manual_seed(0)
        np.testing.assert_array_equal(xs[0].sample(top_k=1).numpy()[untied], host[0].argmax(axis=1)[untied])
        tail(xs[0].ptr)
        np.testing.assert_array_equal(idx32.numpy(), host[0].argmax(axis=1))

        us = time_windows(cases, xs, lambda: L.check(lib.lg_sync()))
        if parent_us is not None:
            us.update(parent_us[str(rows)])
        print("logits (%d, %d):" % (rows, COLS))
        for key, r in sorted(us.items()):
            print("  %-20s median %8.2f us  (p10 %8.2f, p90 %8.2f)" % (key, r["median"], r["p10"], r["p90"]), flush=True)
        ratios = {}
        for mode in ("hot", "cold"):
            yardstick = "parent_greedy" if parent_us is not None else "greedy"
            for name in ("sample_plain", "sample_nucleus"):
                ratios["%s_%s" % (name, mode)] = us["%s_%s" % (name, mode)]["median"] / us["%s_%s" % (yardstick, mode)]["median"]
                print("  %s / %s (%s): %.2f%s" % (name, yardstick, mode, ratios["%s_%s" % (name, mode)],
                                                  "" if parent_us is not None else "   (the parent library's: not measured, no --parent-lib)"))
        result[str(rows)] = {"us": us, "ratio_to_greedy_tail": ratios}
    return result


def measure_steps(rounds=5, iters=200, batch=8):
    import lightgrad_amd as light
    import lightgrad_amd.nn as nn
    from lightgrad_amd.autograd.hip import HipGraph
    spec = importlib.util.spec_from_file_location("decode_time_tool", os.path.join(ROOT, "tools", "decode_time.py"))
    decode_time = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(decode_time)
    bert = decode_time.load(ROOT)
    result = {}
    for prefix in (128, 511):
        per_round = {"greedy": [], "sampled": []}
        kernels = {}
        for _ in range(rounds):
            np.random.seed(0)
            model = bert.BertForMaskedLM(**dict(bert.TINY, causal=True)).eval().map_parameters(lambda p: p.hip())
            ids = np.random.randint(0, bert.TINY["vocab_size"], (batch, prefix + 1)).astype(np.int32)
            to_device = lambda a: light.from_numpy(a, requires_grad=False).hip(requires_grad=False)          # noqa: E731
            cache = nn.KVCache(bert.TINY["num_hidden_layers"], batch, prefix + 1, bert.TINY["hidden_size"], like=model.cls.predictions.bias)
            model(to_device(ids[:, :prefix]), cache=cache)
            token, out_ids = to_device(ids[:, prefix:]), to_device(np.zeros((batch, prefix + 2), np.int32))
            graphs = {}
            for name, sampler in (("greedy", None), ("sampled", NUCLEUS)):
                def step(sampler=sampler):
                    bert.decode_step(model, cache, token, out_ids, None, sampler)
                    cache.set_length(prefix)
                step()
                graphs[name] = HipGraph()
                with graphs[name].capture():
                    step()
                kernels[name] = graphs[name].kernel_count()
            for name in ("greedy", "sampled"):                               # the two alternate from round to round
                per_round[name].append(decode_time.timed(graphs[name].replay, iters))
            for g in graphs.values():
                g.destroy()
        result[str(prefix)] = {name: {"median": float(np.median(v)), "p10": float(np.percentile(v, 10)), "p90": float(np.percentile(v, 90)),
                                      "kernels": kernels[name]} for name, v in per_round.items()}
        g, s = result[str(prefix)]["greedy"], result[str(prefix)]["sampled"]
        print("prefix %3d, replayed, us per token: greedy %.1f (%.1f .. %.1f), %d kernels; sampled %.1f (%.1f .. %.1f), %d kernels; "
              "sampled - greedy %+.1f us, sampled / greedy %.3f" % (prefix, g["median"], g["p10"], g["p90"], g["kernels"], s["median"], s["p10"],
                                                                     s["p90"], s["kernels"], s["median"] - g["median"], s["median"] / g["median"]),
              flush=True)
    return result


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-lib", default=None)
    ap.add_argument("--parent-child", default=None, help=argparse.SUPPRESS)
    ap.add_argument("--steps-only", action="store_true")
    ap.add_argument("--launch-only", action="store_true")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if args.parent_child:
        return parent_child(args.parent_child)
    parent_us = None
    if args.parent_lib and not args.steps_only:               # before this process opens the GPU: a fresh child, under a time limit
        child = subprocess.run([sys.executable, os.path.abspath(__file__), "--parent-child", args.parent_lib], stdout=subprocess.PIPE,
                               text=True, timeout=CHILD_LIMIT)
        if child.returncode != 0:
            sys.exit("the parent library's process ended with status %d - nothing more is started" % child.returncode)
        parent_us = json.loads(child.stdout.strip().splitlines()[-1])
    sys.path.insert(0, ROOT)
    result = {"cols": COLS, "windows": REPS, "launches_per_window": WINDOW}
    if not args.steps_only:
        result["launch"] = measure_launches(parent_us)
    if not args.launch_only:
        result["decode_step"] = measure_steps()
    if args.out:
        with open(args.out, "w") as f:
            json.dump(result, f, indent=1, sort_keys=True)


if __name__ == "__main__":
    main()
