"""Time dropout against the elementwise yardstick at 2^24 and 2^28 float32 elements:

    python tools/dropout_time.py [--reps 30] [--out profiles/dropout.txt]

Four launches, interleaved in one process, each timed alone by a pair of HIP events around it, medians over `--reps`
repetitions after 5 warm-up rounds:
    x.dropout(0.1) forward            reads n, writes n floats
    its backward                      reads n, writes n
    x.dropout(0.1, residual=r)        reads 2n, writes n
    a * b (csrc/elementwise.hip)      reads 2n, writes n - the yardstick, with its own run-to-run spread
The kernels are called with the tape switched off, on buffers allocated once, so a figure is the device time of one launch.
Without a GPU this fails; nothing here estimates."""
import argparse
import ctypes
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def measure(n, reps, p=0.1):
    import numpy as np
    import lightgrad_amd as light
    from lightgrad_amd import HipTensor
    from lightgrad_amd.autograd.hip import HipDevice
    from lightgrad_amd.autograd.hip import lib as L
    from lightgrad_amd.autograd.hip import ops
    lib = L.lib()
    light.manual_seed(1)
    x, r, y = (HipTensor.empty((n,), requires_grad=False) for _ in range(3))
    x.fill(1.5)
    r.fill(0.25)
    base = HipTensor.empty((1,), dtype=np.uint64, requires_grad=False)
    e0, e1 = ctypes.c_void_p(), ctypes.c_void_p()
    L.check(lib.lg_event_create(ctypes.byref(e0)))
    L.check(lib.lg_event_create(ctypes.byref(e1)))
    launches = {
        "dropout forward": (lambda: L.check(lib.lg_dropout_fwd_f32(x.ptr, None, y.ptr, n, p, base.ptr)), 2),
        "dropout backward": (lambda: L.check(lib.lg_dropout_bwd_f32(x.ptr, y.ptr, n, p, base.ptr)), 2),
        "dropout + residual": (lambda: L.check(lib.lg_dropout_fwd_f32(x.ptr, r.ptr, y.ptr, n, p, base.ptr)), 3),
        "a * b": (lambda: ops._ew(L.EW_MUL, (n,), [x, r], out=y), 3),
    }
    times = {name: [] for name in launches}
    ms = ctypes.c_float()
    for rep in range(5 + reps):
        for name, (launch, _) in launches.items():
            L.check(lib.lg_event_record(e0))
            launch()
            L.check(lib.lg_event_record(e1))
            L.check(lib.lg_event_elapsed_ms(e0, e1, ctypes.byref(ms)))
            if rep >= 5:
                times[name].append(ms.value * 1e3)
    HipDevice.synchronize()
    lib.lg_event_destroy(e0)
    lib.lg_event_destroy(e1)
    rows = []
    for name, (_, words) in launches.items():
        t = np.sort(np.asarray(times[name]))
        rows.append((name, float(np.median(t)), float(t[0]), float(t[-1]), 4.0 * words * n / (np.median(t) * 1e-6) / 1e12))
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    assert args.reps >= 20, "medians of at least 20 repetitions"
    from lightgrad_amd.autograd.hip import HipDevice
    lines = ["dropout (csrc/dropout.hip, p = 0.1) against a * b, %s, medians of %d single launches (HIP events), us"
             % (HipDevice.info()["name"], args.reps),
             "%-12s %-20s %10s %10s %10s %8s %12s" % ("n", "launch", "median", "min", "max", "TB/s", "vs a * b")]
    for n in (1 << 24, 1 << 28):
        rows = measure(n, args.reps)
        yard = next(r for r in rows if r[0] == "a * b")
        for name, med, lo, hi, tbs in rows:
            lines.append("%-12d %-20s %10.1f %10.1f %10.1f %8.2f %12.3f" % (n, name, med, lo, hi, tbs, med / yard[1]))
        lines.append("%-12d spread of a * b: %.1f us (%.1f %% of its median)" % (n, yard[3] - yard[2], 100 * (yard[3] - yard[2]) / yard[1]))
    text = "\n".join(lines) + "\n"
    sys.stdout.write(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
