"""Time lg_gemm_bf16_f32 (csrc/gemm_bf16.hip) against lg_gemm_f32, and the captured masked-LM step of examples/bert.py with and
without --bf16-decoder.

  (a) per shape - the three products of tiny-BERT's decoder at batch 8 (forward 1024 x 30522 x 128 NT, dx 1024 x 128 x 30522 NN,
      dW 30522 x 128 x 1024 TN) and 4096^3 NN: us per call of the bf16 kernel and of the fp32 kernel of THIS build, alternating
      inside every repetition, and bf16 time over fp32 time.  With --parent-tree DIR (the parent commit checked out and built in
      a directory of its own) the fp32 kernel of THAT library is timed as well: first, in a child process that imports the
      package from that directory and so loads only that library - the figure the ratio `bf16 / parent fp32` is formed with.
  (b) `examples/bert.py --mlm --graph` at batch 8: kernels per replay and us per replayed step for decoder_precision None / "bf16"
      (and None on the parent's build).

Method: random uniform(-1, 1) operands; every call of a case uses the next of SETS copies of its operands and result, SETS
chosen so that the copies together exceed 600 MB - more than twice the 256 MiB Infinity Cache, so no call finds its operands
cached by the previous one (cache state: cold beyond L2 for every call).  Calls are enqueued back to back between two device
events (WINDOW calls per window after WARMUP windows, the median and the 10th / 90th percentile of REPS windows).

    python tools/bf16_gemm_time.py [--parent-tree DIR] [--out FILE.json] [--no-step]
"""
import argparse
import ctypes
import importlib.util
import json
import os
import subprocess
import sys
import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WARMUP, REPS, WINDOW = 2, 15, 200       # a window of the shortest case (65 us per call) lasts 13 ms
STEP_WINDOW = 50                          # replays of the captured step per window (30 ms)
CHILD_LIMIT = 400         # seconds for the parent library's process
FOOTPRINT = 600e6

# (name, M, N, K, transA, transB)
SHAPES = [("decoder forward  1024x30522x128 NT", 1024, 30522, 128, 0, 1),
          ("decoder dx       1024x128x30522 NN", 1024, 128, 30522, 0, 0),
          ("decoder dW       30522x128x1024 TN", 30522, 128, 1024, 1, 0),
          ("square           4096x4096x4096 NN", 4096, 4096, 4096, 0, 0)]


def windows(lib, cases):
    """cases: [(name, callable enqueueing ONE call)] -> {name: {median, p10, p90}} in us per call"""
    def event():
        e = ctypes.c_void_p()
        assert lib.lg_event_create(ctypes.byref(e)) == 0
        return e
    samples = {name: [] for name, _ in cases}
    for rep in range(WARMUP + REPS):
        for name, call in cases:
            e0, e1 = event(), event()
            assert lib.lg_event_record(e0) == 0
            for _ in range(WINDOW):
                call()
            assert lib.lg_event_record(e1) == 0
            ms = ctypes.c_float()
            assert lib.lg_event_elapsed_ms(e0, e1, ctypes.byref(ms)) == 0        # waits: the next case starts on an idle device
            if rep >= WARMUP:
                samples[name].append(1e3 * ms.value / WINDOW)
            lib.lg_event_destroy(e0), lib.lg_event_destroy(e1)
    out = {}
    for name, v in samples.items():
        v = np.sort(v)
        out[name] = {"median": float(np.median(v)), "p10": float(v[len(v) // 10]), "p90": float(v[(9 * len(v)) // 10])}
    return out


def gemm_numbers(kernels, root=ROOT):
    """(a) for the kernels named in `kernels` ("fp32", "bf16") on the package (and its library) under `root`"""
    sys.path.insert(0, root)
    from lightgrad_amd import HipTensor
    from lightgrad_amd.autograd.hip import lib as L
    lib = L.lib()
    out = {}
    for name, M, N, K, tA, tB in SHAPES:
        a_shape, b_shape = ((K, M) if tA else (M, K)), ((N, K) if tB else (K, N))
        sets = int(min(8, max(2, np.ceil(FOOTPRINT / (4.0 * (M * K + K * N + M * N))))))
        rng = np.random.RandomState(M + N + K)
        bufs = [(HipTensor.from_numpy(rng.uniform(-1, 1, a_shape).astype(np.float32)),
                 HipTensor.from_numpy(rng.uniform(-1, 1, b_shape).astype(np.float32)), HipTensor.empty((M, N))) for _ in range(sets)]
        turn = {"fp32": 0, "bf16": 0}

        def fp32():
            a, b, c = bufs[turn["fp32"] % sets]
            turn["fp32"] += 1
            L.check(lib.lg_gemm_f32(tA, tB, M, N, K, a.ptr, a_shape[1], 0, b.ptr, b_shape[1], 0, c.ptr, N, 0, 1, 0))

        def bf16():
            a, b, c = bufs[turn["bf16"] % sets]
            turn["bf16"] += 1
            L.check(lib.lg_gemm_bf16_f32(tA, tB, M, N, K, a.ptr, a_shape[1], b.ptr, b_shape[1], c.ptr, N, None, 0))
        cases = [(k, {"fp32": fp32, "bf16": bf16}[k]) for k in kernels]
        r = windows(lib, cases)
        r["sets"], r["flop"] = sets, 2.0 * M * N * K
        out[name] = r
        del bufs
    return out


def step_numbers(precisions, root=ROOT, batch=8):
    """(b): the captured masked-LM step of examples/bert.py under `root` for each decoder_precision in `precisions`"""
    sys.path.insert(0, root)
    import lightgrad_amd as light
    from lightgrad_amd.autograd.hip import HipGraph, lib as L
    lib = L.lib()
    spec = importlib.util.spec_from_file_location("bert_example_timed", os.path.join(root, "examples", "bert.py"))
    bert = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(bert)
    out, cases, keep = {}, [], []
    for precision in precisions:
        light.manual_seed(0)
        np.random.seed(0)
        config = dict(bert.TINY) if precision is None else dict(bert.TINY, decoder_precision=precision)
        model = bert.BertForMaskedLM(**config).map_parameters(lambda p: p.hip())
        ids = light.from_numpy(np.random.randint(0, bert.TINY["vocab_size"], (batch, 128)).astype(np.int32), requires_grad=False).hip()
        for _ in range(2):
            bert.mlm_forward_backward(model, ids).item()
        graph = HipGraph()
        with graph.capture():
            loss = bert.mlm_forward_backward(model, ids)
        name = "decoder_precision=%s" % precision
        out[name] = {"kernels_per_step": graph.kernel_count()}
        cases.append((name, graph.replay))
        keep.append((model, ids, loss, graph))
    global WINDOW
    saved, WINDOW = WINDOW, STEP_WINDOW
    try:
        for name, us in windows(lib, cases).items():
            out[name]["step_us"] = us
    finally:
        WINDOW = saved
    for _, _, loss, _ in keep:
        assert np.isfinite(loss.item())
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-tree", default=None)
    ap.add_argument("--parent-child", default=None, help=argparse.SUPPRESS)
    ap.add_argument("--no-step", action="store_true")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if args.parent_child:                                        # this process imports the parent's package and nothing of this tree
        r = {"gemm": gemm_numbers(["fp32"], root=args.parent_child)}
        if not args.no_step:
            r["step"] = step_numbers([None], root=args.parent_child)
        print(json.dumps(r), flush=True)
        return
    result = {"windows": REPS, "calls_per_window": WINDOW}
    if args.parent_tree:                                         # before this process opens the GPU: a fresh child, under a time limit
        cmd = [sys.executable, os.path.abspath(__file__), "--parent-child", os.path.abspath(args.parent_tree)] + (["--no-step"] if args.no_step else [])
        child = subprocess.run(cmd, stdout=subprocess.PIPE, text=True, timeout=CHILD_LIMIT)
        if child.returncode != 0:
            sys.exit("the parent library's process ended with status %d - nothing more is started" % child.returncode)
        result["parent_build"] = json.loads(child.stdout.strip().splitlines()[-1])
    result["gemm"] = gemm_numbers(["fp32", "bf16"])
    if not args.no_step:
        result["step"] = step_numbers([None, "bf16"])
    parent = result.get("parent_build")
    print("%-38s %12s %12s %12s %10s %10s" % ("shape", "bf16 us", "fp32 us", "parent fp32", "bf16/fp32", "bf16 TF/s"))
    for name, r in result["gemm"].items():
        p = parent["gemm"][name]["fp32"]["median"] if parent else None
        base = p if p is not None else r["fp32"]["median"]
        print("%-38s %12.1f %12.1f %12s %10.3f %10.1f   (p10-p90 bf16 %.1f-%.1f, fp32 %.1f-%.1f; %d operand sets)" % (
            name, r["bf16"]["median"], r["fp32"]["median"], ("%.1f" % p) if p is not None else "not measured",
            r["bf16"]["median"] / base, r["flop"] / r["bf16"]["median"] * 1e-6, r["bf16"]["p10"], r["bf16"]["p90"],
            r["fp32"]["p10"], r["fp32"]["p90"], r["sets"]))
    if not args.no_step:
        rows = sorted(result["step"].items()) + ([("parent build, decoder_precision=None", parent["step"]["decoder_precision=None"])] if parent else [])
        for name, r in rows:
            print("step %-40s %3d kernels  %9.1f us (p10 %9.1f, p90 %9.1f)" % (
                name, r["kernels_per_step"], r["step_us"]["median"], r["step_us"]["p10"], r["step_us"]["p90"]))
    if args.out:
        with open(args.out, "w") as f:
            json.dump(result, f, indent=1, sort_keys=True)


if __name__ == "__main__":
    main()
