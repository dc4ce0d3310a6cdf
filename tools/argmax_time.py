"""Time argmax and top-1 counting on the masked-LM head's logits, (1024, 30522) float32 = 125 MB (the C ABI called directly, HIP
events around 20 back-to-back launches so that the device and not the host sets the pace, 10 warm-up launches, the median of 30
such windows):
  argmax      x.argmax(-1)                                          (lg_argreduce_f32, a wave per row)
  acc0        metrics.accuracy, no row ignored                      (lg_top1_count_f32)
  acc85       metrics.accuracy, 85 % of the rows ignored            (expected: clearly below acc0 - ignored rows are not read)
  max         x.max(-1) of THIS library                             (csrc/reduce.hip)
  parent_max  x.max(-1) of another build of the library, --parent-lib PATH: the yardstick is the parent commit's `max`, which is
              bound by the same single read of the logits.  It runs first, in a child process of its own that loads nothing but
              that library (two builds in one process resolve each other's symbols), on the same seeded data and with the same
              windows; without the option the line says "not measured"
  host        the route being replaced: numpy() + np.argmax, host clock, 5 runs
The cases of this library alternate inside every repetition.  Each device case is timed twice: `hot` on one tensor again and
again (125 MB stay in the 256 MiB Infinity Cache) and `cold` rotating over three tensors (375 MB: every launch reads from HBM).

    python tools/argmax_time.py [--parent-lib PATH] [--out FILE.json]
"""
import argparse
import ctypes
import json
import os
import subprocess
import sys
import time
import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ROWS, COLS, WARMUP, REPS, WINDOW = 1024, 30522, 10, 30, 20
CHILD_LIMIT = 240         # seconds for the parent library's process


def host_logits():
    rng = np.random.RandomState(0)
    return rng, [rng.uniform(-8, 8, (ROWS, COLS)).astype(np.float32) for _ in range(3)]


def time_windows(cases, tensors, sync):
    """cases: [(name, library handle, run(tensor))] -> {"name_hot" / "name_cold": {median, p10, p90}} in us per launch"""
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


def parent_child(path):
    """this process loads only the library at `path`: lg_reduce(max) over the last axis of the same logits, one JSON line"""
    sys.path.insert(0, ROOT)
    from lightgrad_amd.autograd.hip import lib as L
    names = ("lg_init", "lg_last_error", "lg_reduce", "lg_event_create", "lg_event_record", "lg_event_elapsed_ms", "lg_event_destroy",
             "lg_sync", "lg_malloc", "lg_memcpy_h2d", "lg_memcpy_d2h")
    P = L.load_library(os.path.abspath(path), {n: L.PROTOTYPES[n] for n in names}, mode=ctypes.RTLD_GLOBAL)
    assert P.lg_init(0) == 0, P.lg_last_error()
    _, host = host_logits()
    tensors = []
    for h in host:
        p = ctypes.c_void_p()
        assert P.lg_malloc(ctypes.byref(p), h.nbytes) == 0 and P.lg_memcpy_h2d(p, h.ctypes.data, h.nbytes) == 0, P.lg_last_error()
        tensors.append(p)
    out = ctypes.c_void_p()
    assert P.lg_malloc(ctypes.byref(out), ROWS * 4) == 0
    shape, strides = L.i64((ROWS, COLS)), L.i64((COLS, 1))

    def run(x):
        assert P.lg_reduce(L.RED_MAX, 2, shape, x, strides, 2, out) == 0, P.lg_last_error()
    run(tensors[0])
    got = np.empty(ROWS, np.float32)
    assert P.lg_memcpy_d2h(got.ctypes.data, out, got.nbytes) == 0
    np.testing.assert_array_equal(got, host[0].max(axis=1))
    print(json.dumps(time_windows([("parent_max", P, run)], tensors, lambda: P.lg_sync())), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-lib", default=None)
    ap.add_argument("--parent-child", default=None, help=argparse.SUPPRESS)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if args.parent_child:
        return parent_child(args.parent_child)
    parent_us = None
    if args.parent_lib:                                       # before this process opens the GPU: a fresh child, under a time limit
        child = subprocess.run([sys.executable, os.path.abspath(__file__), "--parent-child", args.parent_lib], stdout=subprocess.PIPE,
                               text=True, timeout=CHILD_LIMIT)
        if child.returncode != 0:
            sys.exit("the parent library's process ended with status %d - nothing more is started" % child.returncode)
        parent_us = json.loads(child.stdout.strip().splitlines()[-1])

    sys.path.insert(0, ROOT)
    import lightgrad_amd as light
    from lightgrad_amd import HipTensor
    from lightgrad_amd.autograd.hip import lib as L
    lib = L.lib()
    rng, host = host_logits()
    xs = [HipTensor.from_numpy(h, requires_grad=False) for h in host]
    labels = rng.randint(0, COLS, ROWS).astype(np.int64)
    labels[:ROWS // 2] = np.argmax(host[0], axis=1)[:ROWS // 2]
    ignoring = labels.copy()
    ignoring[rng.permutation(ROWS)[:int(round(0.85 * ROWS))]] = -100
    lab0, lab85 = HipTensor.from_numpy(labels, requires_grad=False), HipTensor.from_numpy(ignoring, requires_grad=False)
    total = HipTensor.from_numpy(np.zeros(2, np.int64), requires_grad=False)
    shape, strides = L.i64((ROWS, COLS)), L.i64((COLS, 1))
    idx = HipTensor.empty((ROWS,), dtype=np.int64, requires_grad=False)
    val = HipTensor.empty((ROWS,), requires_grad=False)
    cases = [("argmax", lib, lambda x: L.check(lib.lg_argreduce_f32(L.RED_MAX, 2, shape, x.ptr, strides, 1, idx.ptr))),
             ("acc0", lib, lambda x: L.check(lib.lg_top1_count_f32(x.ptr, ROWS, COLS, lab0.ptr, 8, 0, 0, 1, total.ptr))),
             ("acc85", lib, lambda x: L.check(lib.lg_top1_count_f32(x.ptr, ROWS, COLS, lab85.ptr, 8, 1, -100, 1, total.ptr))),
             ("max", lib, lambda x: L.check(lib.lg_reduce(L.RED_MAX, 2, shape, x.ptr, strides, 2, val.ptr)))]

    # results must not change: the same answers as numpy before anything is timed
    np.testing.assert_array_equal(xs[0].argmax(-1).numpy(), np.argmax(host[0], axis=1))
    np.testing.assert_array_equal(light.metrics.accuracy(xs[0], lab0).numpy(), [(np.argmax(host[0], axis=1) == labels).sum(), ROWS])

    result = {"shape": [ROWS, COLS], "bytes": ROWS * COLS * 4, "windows": REPS, "launches_per_window": WINDOW,
              "us": time_windows(cases, xs, lambda: L.check(lib.lg_sync()))}
    if parent_us is not None:
        result["us"].update(parent_us)
    t = []
    for _ in range(5):
        t0 = time.perf_counter()
        np.argmax(xs[0].numpy(), axis=1)
        t.append(1e6 * (time.perf_counter() - t0))
    result["us"]["host_numpy_argmax"] = {"median": float(np.median(t)), "p10": float(min(t)), "p90": float(max(t))}
    for key, r in sorted(result["us"].items()):
        print("%-20s median %9.2f us  (p10 %9.2f, p90 %9.2f)  %6.2f TB/s of the logits" % (
            key, r["median"], r["p10"], r["p90"], result["bytes"] / r["median"] / 1e6), flush=True)
    for mode in ("hot", "cold"):
        if parent_us is None:
            print("ratio to the parent library's max (%s): not measured (no --parent-lib)" % mode)
            continue
        for name in ("argmax", "acc0", "acc85", "max"):
            ratio = result["us"]["%s_%s" % (name, mode)]["median"] / result["us"]["parent_max_%s" % mode]["median"]
            result.setdefault("ratio_to_parent_max", {})["%s_%s" % (name, mode)] = ratio
            print("%s / parent_max (%s): %.3f" % (name, mode, ratio))
    if args.out:
        with open(args.out, "w") as f:
            json.dump(result, f, indent=1, sort_keys=True)


if __name__ == "__main__":
    main()
