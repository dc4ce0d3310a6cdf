"""Host cost of a call of the KV-cache attention entries, one library against another (csrc/cache_entry.h holds their checks).

    python tools/cache_entry_host_time.py --old <liblghip.so of the parent commit> [--repeats 5] [--calls 2000] [--out FILE]

Two entries, through the C ABI with fixed operands: lg_attention_decode_split_f32 at batch 8, 2 heads, d = 64, t = 1023 of a
cache of 1024 rows (profiles/decode_split.md: four slices, so the workspace is taken and returned around the launch), and
lg_attention_extend_paged_f32 at 8 slots, 2 heads, d = 64, m = 1 behind 128 positions, blocks of 16 rows, identity tables,
capacity 512 (profiles/paged.md).  A child process per (library, repeat), the two libraries alternating; the child issues
`--calls` eager calls after 200 warm-up calls and one synchronise, and reports the host clock around calls + synchronise,
divided by the calls - and, next to it, around the loop that issues the calls alone: the first is bound by the device once the
kernels take longer than the host needs per call, the second is the host's share while the queue does not fill.  Without a GPU
this fails; nothing here falls back."""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def child(calls):
    import numpy as np
    from lightgrad_amd import HipTensor
    from lightgrad_amd.autograd.hip import HipDevice
    from lightgrad_amd.autograd.hip import lib as hiplib
    lib, rng = hiplib.lib(), np.random.RandomState(0)
    b, heads, d = 8, 2, 64
    width = heads * d
    f32 = lambda *shape: HipTensor.from_numpy(rng.uniform(-1.5, 1.5, shape).astype(np.float32), requires_grad=False)      # noqa: E731
    i32 = lambda a: HipTensor.from_numpy(np.ascontiguousarray(a, np.int32), requires_grad=False)      # noqa: E731
    q, kn, vn, o = (f32(b, width) for _ in range(4))

    capacity = 1024
    k, v, pos = f32(b, capacity, width), f32(b, capacity, width), i32([capacity - 1])
    split = lambda: lib.lg_attention_decode_split_f32(q.ptr, width, kn.ptr, width, vn.ptr, width, k.ptr, v.ptr, width, capacity * width, pos.ptr,      # noqa: E731
                                                      o.ptr, width, None, b, heads, capacity, d, 0.125, None, 0)

    B, max_blocks = 16, 32
    kp, vp = f32(b * max_blocks, B, width), f32(b * max_blocks, B, width)
    ppos, count, table = i32([128] * b), i32([1] * b), i32(np.arange(b * max_blocks).reshape(b, max_blocks))
    paged = lambda: lib.lg_attention_extend_paged_f32(q.ptr, width, width, kn.ptr, width, width, vn.ptr, width, width, kp.ptr, vp.ptr, width, ppos.ptr,      # noqa: E731
                                                      count.ptr, table.ptr, o.ptr, width, width, None, b, heads, 1, max_blocks, b * max_blocks, 4, d,
                                                      0.125, None, 0)
    result = {}
    for name, call in (("lg_attention_decode_split_f32", split), ("lg_attention_extend_paged_f32", paged)):
        for _ in range(200):
            assert call() == 0, lib.lg_last_error()
        HipDevice.synchronize()
        start = time.perf_counter()
        for _ in range(calls):
            call()
        issued = time.perf_counter()
        HipDevice.synchronize()
        result[name] = (time.perf_counter() - start) / calls * 1e6
        result[name + ", issue loop alone"] = (issued - start) / calls * 1e6
    print(json.dumps(result))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--old")
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--calls", type=int, default=2000)
    ap.add_argument("--out")
    ap.add_argument("--child", action="store_true")
    args = ap.parse_args()
    if args.child:
        return child(args.calls)
    libs = {"parent": os.path.abspath(args.old), "this tree": os.path.join(ROOT, "lightgrad_amd", "liblghip.so")}
    runs = {name: [] for name in libs}
    for repeat in range(args.repeats):
        for name, path in list(libs.items())[::1 if repeat % 2 == 0 else -1]:      # who goes first alternates too
            done = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", "--calls", str(args.calls)],
                                  env=dict(os.environ, LIGHTGRAD_HIP_LIB=path), stdout=subprocess.PIPE, text=True, timeout=120, check=True)
            runs[name].append(json.loads(done.stdout.strip().splitlines()[-1]))
    lines = ["us per call (host clock around %d eager calls and one synchronise), %d fresh processes per library, alternating" % (args.calls, args.repeats)]
    for entry in runs["parent"][0]:
        for name in libs:
            us = sorted(r[entry] for r in runs[name])
            lines.append("%-50s %-10s median %.3f  min %.3f  max %.3f  all %s" % (entry, name, statistics.median(us), us[0], us[-1],
                                                                                  " ".join("%.3f" % x for x in us)))
    text = "\n".join(lines)
    print(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
